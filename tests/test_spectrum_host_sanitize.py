"""The host part of kdb_rank_transform (kdb_spectrum_host.cpp.h: prefix sums over the dense table, the sort of the list of large values, the
two rank tables) under AddressSanitizer + UBSan on the CPU, driven by a stand-alone program: an empty list, duplicates in it, 2^64 - 1,
a dense entry above 2^32, every rank against a count over all bins."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_tables_are_right_and_clean_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "spectrum_host_check")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                            "-o", exe, os.path.join(ROOT, "tests/c/spectrum_host_check.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "spectrum host check ok" in run.stdout and "ERROR" not in run.stderr and "runtime error" not in run.stderr
