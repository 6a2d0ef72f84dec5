"""CPU (hipcc cross-compiles gfx950 without a GPU): the register budget of kdb_spectrum's and kdb_rank_transform's kernels, read from the
compiler's own assembly like tests/test_isa_budget_gram.py does for kdb_gram.  Both are launched with __launch_bounds__(256, 4): four
workgroups of four waves per CU, four waves per SIMD, so 128 VGPRs per lane at most and no scratch; their LDS (32 KiB and 16 KiB) leaves room
for the four workgroups in a CU's 160 KiB."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    import isa_stats
    d = tmp_path_factory.mktemp("isa_spectrum")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    # the header alone: it includes nothing of the engine's but include/kdbhip.h, and its kernels compile as they do inside kdb_engine.hip
    src = d / "spectrum_only.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "kmerdb_amd", "csrc", "kdb_spectrum.hip.h"))
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-save-temps",
           "-o", str(d / "lib.so"), str(src)]
    subprocess.check_call(cmd, cwd=str(d), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    s = [f for f in os.listdir(d) if f.endswith("gfx950.s")]
    assert len(s) == 1
    return isa_stats.kernel_stats(str(d / s[0]))


@pytest.mark.parametrize("kernel,lds", [("kdbspectrum::spectrum_kernel", 32768), ("kdbspectrum::rank_map_kernel", 16384)])
def test_both_kernels_keep_four_waves_per_simd_and_do_not_spill(isa, kernel, lds):
    v = [s for n, s in isa.items() if kernel + "(" in n]
    assert len(v) == 1, sorted(isa)
    v = v[0]
    assert v["scratch"] == 0 and v["vgprs"] <= 128, v
    assert v["occupancy"] >= 4 and v["lds"] == lds and 4 * v["lds"] <= 160 * 1024, v
    assert v["vmem"] >= 3                                                     # (two 16-byte loads a step, and what it writes)
    assert v["ds_rtn_atomics"] == 0, v                                        # (no LDS add waits for its old value)
