"""The 5x5 tap table of the l1_cv kernels (csrc/dtfill_taps.hpp: offsets, weights, parent codes, step encoding, tap_decode) is
the one the parallel model states -- and tests/test_parallel_model.py pins that model to the sequential oracle.  A host compiler
reads the header as it stands (tests/tap_table_main.cpp prints it), so a wrong table fails here, without a GPU."""
import os
import shutil
import subprocess

import pytest

import parallel_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distancetransform-depthcompletion_amd", "csrc")


def test_header_table_is_the_models(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path / "tap_table")
    subprocess.run([cxx, "-std=c++14", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "tap_table_main.cpp")],
                   check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 16 + 1 + 8
    taps = pm.FWD + pm.BWD  # code t: forward tap t; code 8 | t: backward tap t
    for code, line in enumerate(out[:16]):
        di, dj, w = taps[code]
        assert w == abs(di) + abs(dj)
        want = [code, di, dj, w, (di + 2) << 3 | (dj + 2), int(code < 8), di, dj]
        assert [int(v) for v in line.split()] == want, (line, want)
    for t in range(8):  # backward tap t is the negated forward tap t
        assert pm.BWD[t] == (-pm.FWD[t][0], -pm.FWD[t][1], pm.FWD[t][2])
        assert out[17 + t].split() == ["tap", str(t), str(pm.FWD[t][0]), str(pm.FWD[t][1])]
    nib = out[16].split()
    assert nib[0] == "nibbles"
    for axis in (0, 1):
        assert int(nib[1 + axis], 16) == sum((pm.FWD[t][axis] + 2) << (4 * t) for t in range(8))
