"""CPU: what kdb_size_factors / kdb_scale_counts and kmerdb_amd.matrix can be held to without a device -- the radix select's host code under
AddressSanitizer + UBSan in a stand-alone program, the kernels' register budget from the compiler's own assembly, the exported symbols and
constants, the argument ladder of the host layer, and the text the matrix driver prints."""
import ctypes
import io
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_radix_select_host_code_is_right_and_clean_under_asan_ubsan(tmp_path):
    """kdb_select_host.cpp.h -- the key transform the device runs and the narrowing step the host runs -- as a complete host radix select
    against a sort: m = 1, 2, 3 and a few hundred, ties, both signs and both zeros, values that differ in the last digit only, middle ranks
    that part at the first, a middle and the last digit."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "select_host_check")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-o", exe, os.path.join(ROOT, "tests/c/select_host_check.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "select host check ok" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr


def test_the_three_kernels_keep_their_registers_and_do_not_spill(tmp_path):
    """hipcc cross-compiles gfx950 without a GPU.  The kernels' header alone, with the library's flags: each kernel once, no scratch memory,
    at most 128 VGPRs (four waves per SIMD, the budget the other streaming kernels keep)."""
    import isa_stats
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = tmp_path / "sizefactors_only.hip"
    src.write_text('#include "%s"\n' % os.path.join(ROOT, "kmerdb_amd", "csrc", "kdb_sizefactors.hip.h"))
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-save-temps",
           "-o", str(tmp_path / "lib.so"), str(src)]
    subprocess.check_call(cmd, cwd=str(tmp_path), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    s = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert len(s) == 1
    isa = isa_stats.kernel_stats(str(tmp_path / s[0]))
    hits = {n: v for n, v in isa.items() if "kdbsf::" in n}
    for name in ("kdbsf::geomean_kernel", "kdbsf::select_kernel", "kdbsf::scale_kernel"):
        v = [st for n, st in hits.items() if name in n]
        assert len(v) == 1, (name, sorted(hits))
        assert v[0]["scratch"] == 0 and v[0]["vgprs"] <= 128, (name, v[0])
        assert v[0]["vmem"] >= 2                                                    # (its loads and its stores or atomics are there)
    assert len(hits) == 3, sorted(hits)
    sel = [st for n, st in hits.items() if "select_kernel" in n][0]
    assert sel["lds"] == 2 * 2048 * 4 and sel["ds_rtn_atomics"] == 0                # two histograms of 2^11 counters; the adds return nothing


def test_symbols_and_constants_are_exported():
    import kmerdb_amd
    from kmerdb_amd import _abi
    _abi.build()
    L = ctypes.CDLL(_abi.LIB_PATH)
    assert hasattr(L, "kdb_size_factors") and hasattr(L, "kdb_scale_counts")
    header = open(os.path.join(ROOT, "include", "kdbhip.h")).read()
    assert int(re.search(r"#define\s+KDB_SIZEFACTORS_WG_BINS\s+(\d+)", header).group(1)) == _abi.KDB_SIZEFACTORS_WG_BINS
    assert hasattr(kmerdb_amd, "matrix")
    # refusals that come before any device is asked for
    lib = _abi.lib()
    for s in (0.0, -2.0, float("inf"), float("nan")):
        assert lib.kdb_scale_counts(0, ctypes.c_void_p(64), 4, ctypes.c_double(s), ctypes.c_void_p(64), 0, None) == _abi.KDB_ERR_ARG
    assert lib.kdb_scale_counts(0, ctypes.c_void_p(64), 4, ctypes.c_double(1.0), ctypes.c_void_p(72), 0, None) == _abi.KDB_ERR_ARG
    assert lib.kdb_scale_counts(0, None, 4, ctypes.c_double(1.0), ctypes.c_void_p(64), 0, None) == _abi.KDB_ERR_ARG
    assert lib.kdb_scale_counts(0, ctypes.c_void_p(64), 2 ** 36 + 1, ctypes.c_double(1.0), ctypes.c_void_p(64), 0, None) == _abi.KDB_ERR_ARG
    arr = (ctypes.c_void_p * 1)(ctypes.c_void_p(64))
    out, m = (ctypes.c_double * 1)(), ctypes.c_uint64(0)
    assert lib.kdb_size_factors(0, arr, 0, 4, out, ctypes.byref(m), None) == _abi.KDB_ERR_ARG
    assert lib.kdb_size_factors(0, arr, 1, 0, out, ctypes.byref(m), None) == _abi.KDB_ERR_ARG
    assert lib.kdb_size_factors(0, arr, 1, 4, None, ctypes.byref(m), None) == _abi.KDB_ERR_ARG
    assert lib.kdb_size_factors(0, arr, 1, 4, out, None, None) == _abi.KDB_ERR_ARG


def _write(path, k, counts):
    from kmerdb_amd import fileutil
    md = {"version": fileutil.VERSION, "metadata_blocks": 1, "k": k, "total_kmers": int(counts.sum()), "unique_kmers": int(np.count_nonzero(counts)),
          "unique_nullomers": 0, "sorted": False, "tags": [], "files": []}
    fileutil.write_kdb(str(path), md, counts)
    return str(path)


def test_matrix_argument_errors_and_the_pass_through(tmp_path):
    from kmerdb_amd import matrix
    rng = np.random.default_rng(2)
    a = _write(tmp_path / "a.2.kdb", 2, rng.integers(0, 9, 16).astype(np.uint64))
    b = _write(tmp_path / "b.2.kdb", 2, rng.integers(0, 9, 16).astype(np.uint64))
    c = _write(tmp_path / "c.3.kdb", 3, rng.integers(0, 9, 64).astype(np.uint64))
    out = io.StringIO()
    with pytest.raises(IOError):
        matrix.matrix([a, str(tmp_path / "b.tsv")], "from", out=out)
    with pytest.raises(TypeError):
        matrix.matrix([a, c], "from", out=out)
    with pytest.raises(ValueError):
        matrix.matrix([a], "from", out=out)
    names = tmp_path / "names.txt"
    names.write_text("x\ny\nz\n")
    with pytest.raises(RuntimeError):
        matrix.matrix([a, b], "from", column_names=str(names), out=out)
    with pytest.raises(ValueError, match="unsupported method"):
        matrix.matrix([a, b], "Normalize", out=out)
    for method in ("PCA", "tSNE"):
        with pytest.raises(ValueError, match=method + "' is not offered"):
            matrix.matrix([a, b], method, out=out)
    assert out.getvalue() == ""
    names.write_text("x\ny\n")
    from kmerdb_amd import fileutil
    va, vb = fileutil.read_kdb(a).counts, fileutil.read_kdb(b).counts
    for method in ("from", "Frequency"):                                            # pass-through: no device is needed
        out = io.StringIO()
        cols = matrix.matrix([a, b], method, column_names=str(names), out=out, with_index=True, output_delimiter=",")
        assert out.getvalue() == ",x,y\n" + "".join("%d,%d,%d\n" % (i, int(p), int(q)) for i, (p, q) in enumerate(zip(va, vb)))
        assert cols[0].tobytes() == va.tobytes() and cols[1].tobytes() == vb.tobytes()


def test_an_unknown_normalisation_is_rejected_by_every_distance_entry_point(tmp_path):
    from kmerdb_amd import distance
    v = np.arange(16, dtype=np.uint64)
    with pytest.raises(ValueError, match="unsupported normalisation 'nonsense'"):
        distance.distance_matrix([v, v], "euclidean", normalize="nonsense")
    with pytest.raises(ValueError, match="unsupported normalisation 'nonsense'"):
        distance.distances(["a.kdb", "b.kdb"], "euclidean", normalize="nonsense")
    with pytest.raises(ValueError, match="unsupported normalisation 'nonsense'"):
        distance.profile_distances(["a.fa", "b.fa"], 4, metric="euclidean", normalize="nonsense")
    from kmerdb_amd import profile
    for argv in (["distance", "euclidean", "--normalize", "nonsense", "a.kdb", "b.kdb"], ["matrix", "PCA", "a.kdb", "b.kdb"], ["matrix", "DESeq2"]):
        with pytest.raises(SystemExit):                                             # (the command line's parser refuses them)
            profile.main(argv)


def test_size_factors_need_a_device():
    """no CPU fallback: without a device every entry point that would compute raises"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from kmerdb_amd import _abi, distance, matrix
    v = np.arange(1, 17, dtype=np.uint64)
    with pytest.raises(_abi.KdbHipError):
        matrix.size_factors([v, v])
    with pytest.raises(_abi.KdbHipError):
        matrix.normalize([v, v])
    with pytest.raises(_abi.KdbHipError):
        distance.distance_matrix([v, v], "euclidean", normalize="DESeq2")


def test_the_text_of_a_small_matrix():
    from kmerdb_amd import matrix
    ints = [np.array([0, 12, 3], dtype=np.int64), np.array([7, 0, 2 ** 64 - 1], dtype=np.uint64)]
    assert matrix.format_columns(ints, ["a", "b"]) == "a\tb\n0\t7\n12\t0\n3\t18446744073709551615\n"
    assert matrix.format_columns(ints, ["a", "b"], ",", with_index=True) == ",a,b\n0,0,7\n1,12,0\n2,3,18446744073709551615\n"
    floats = [np.array([0.0, 1.5, 1.0 / 3.0]), np.array([2.0, 1e-05, 123456789.125])]
    assert matrix.format_columns(floats, ["s1", "s2"]) == "s1\ts2\n0.0\t2.0\n1.5\t1e-05\n0.3333333333333333\t123456789.125\n"
    assert matrix.format_columns(floats, ["s1", "s2"], " ", with_index=True) == " s1 s2\n0 0.0 2.0\n1 1.5 1e-05\n2 0.3333333333333333 123456789.125\n"
    # a later chunk of a long matrix: no header, the index goes on
    assert matrix.format_columns(ints, ["a", "b"], "\t", with_index=True, first_row=65536, header=False) == "65536\t0\t7\n65537\t12\t0\n65538\t3\t18446744073709551615\n"
    assert matrix.format_columns([c[:0] for c in ints], ["a", "b"]) == "a\tb\n"
    with pytest.raises(ValueError):
        matrix.format_columns(ints, ["a"])
