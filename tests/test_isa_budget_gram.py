"""CPU (hipcc cross-compiles gfx950 without a GPU): the register budget of kdb_gram's sweep, read from the compiler's own assembly like
tests/test_isa_budget.py does for the counting kernels.  Every gram_kernel instantiation keeps its accumulators in registers -- no scratch --
within 128 VGPRs per lane: four waves per SIMD, the budget the other streaming kernels keep."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    import isa_stats
    d = tmp_path_factory.mktemp("isa_gram")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-save-temps",
           "-o", str(d / "lib.so"), os.path.join(ROOT, "kmerdb_amd", "csrc", "kdb_engine.hip"), "-lz", "-lpthread"]
    subprocess.check_call(cmd, cwd=str(d), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    s = [f for f in os.listdir(d) if f.endswith("gfx950.s")]
    assert len(s) == 1
    return isa_stats.kernel_stats(str(d / s[0]))


def test_every_gram_kernel_keeps_four_waves_per_simd_and_does_not_spill(isa):
    hits = {n: v for n, v in isa.items() if "kdbgram::gram_kernel<" in n}
    # the diagonal blocks of 1..4 vectors, and a full block against a last block of 1..4
    want = ["gram_kernel<%d, %d, true>" % (a, a) for a in (1, 2, 3, 4)] + ["gram_kernel<4, %d, false>" % b for b in (1, 2, 3, 4)]
    for w in want:
        assert sum(1 for n in hits if w in n) == 1, (w, sorted(hits))
    assert len(hits) == len(want), sorted(hits)
    for n, v in hits.items():
        assert v["scratch"] == 0 and v["vgprs"] <= 128, (n, v)
        assert v["vmem"] >= 2                                                     # (its loads and its one store are there)
    for name in ("kdbgram::gram_tail_kernel", "kdbgram::gram_combine_kernel"):
        v = [s for n, s in isa.items() if name in n]
        assert len(v) == 1 and v[0]["scratch"] == 0, (name, v)
