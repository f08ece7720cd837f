"""The plane codes of the window kernel (csrc/dtfill_taps.hpp: plane_code, CODE_SOURCE, CODE_NONE, CODE_STEP, code_step): the four
code planes of k_fused hold a winner's parent code itself, and the two parent codes that never win there -- backward taps 5 and 6,
codes 13 and 14 -- mean "source" and "undecided".  A host compiler reads the header as it stands (tests/fused_codes_main.cpp
prints it): the step table is the tap table's, the reserved codes step (0, 0), and no two meanings share a code.  Without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import parallel_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distancetransform-depthcompletion_amd", "csrc")


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("fused_codes") / "fused_codes")
    subprocess.run([cxx, "-std=c++14", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "fused_codes_main.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == 16 + 1 + 1 + 8
    rows = [[int(v) for v in line.split()] for line in out[:16]]
    reserved = [int(v) for v in out[16].split()[1:]]
    plane = [int(v) for v in out[17].split()[1:]]
    taps = [[int(v) for v in line.split()[1:]] for line in out[18:]]
    return rows, reserved, plane, taps


def test_step_table_is_the_tap_tables(printed):
    rows, (source, none), _, taps = printed
    assert taps == [[t, pm.FWD[t][0], pm.FWD[t][1]] for t in range(8)]  # TAP_OFFSET as the model states it
    for code, (c, di, dj, rdi, rdj, wins) in enumerate(rows):
        assert c == code
        t = code & 7
        off = (taps[t][1], taps[t][2]) if code < 8 else (-taps[t][1], -taps[t][2])  # TAP_OFFSET, negated for a backward code
        want = (0, 0) if code in (source, none) else off
        assert (di, dj) == want, (code, di, dj, want)
        assert (rdi, rdj) == want, "code_step(%d) at run time: %s, table %s" % (code, (rdi, rdj), want)
        assert wins == int(code not in (source, none))


def test_reserved_codes_step_nowhere_and_never_win(printed):
    rows, (source, none), _, _ = printed
    assert {source, none} == {13, 14}  # backward taps 5 and 6
    for c in (source, none):
        assert rows[c][1:5] == [0, 0, 0, 0] and rows[c][5] == 0


def test_codes_are_distinct(printed):
    rows, (source, none), plane, _ = printed
    winners = [c for c in range(16) if rows[c][5]]
    assert len(winners) == 14
    codes = [plane[c] for c in winners] + [source, none]
    assert sorted(codes) == list(range(16)), codes  # 14 winners, source, undecided: sixteen different codes in four planes
    # ... and no two winners share a step: the step bytes lose nothing
    assert len({(rows[c][1], rows[c][2]) for c in winners}) == 14


def test_model_never_lets_the_reserved_codes_win():
    """What the header proves, on the parallel model (pinned to the oracle by tests/test_parallel_model.py): in random frames
    from thin to dense, backward taps 5 and 6 are never the first match, and every other code is."""
    rng = np.random.default_rng(3)
    seen = set()
    for p in (0.002, 0.01, 0.05, 0.3):
        src = rng.random((96, 160)) < p
        gu, g = pm.colscan(src)
        d, live = pm.rowscan(g, gu, pm.skew(gu))
        seen |= set(np.unique(pm.parent(d, live)).tolist())
    assert seen == set(range(13)) | {15, 255}, sorted(seen)
