"""k_fused keeps its place on a CU: no scratch, at most 128 VGPRs, at most 40 960 B of LDS and four waves per SIMD for each
of its three instances (scripts/check_fused_resources.py compiles for gfx950 and reads the compiler's resource remarks).
Needs hipcc, not a GPU."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _checker():
    spec = importlib.util.spec_from_file_location("check_fused_resources", os.path.join(ROOT, "scripts", "check_fused_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parse_reads_the_remarks():
    chk = _checker()
    rem = "./dtfill_fused.hpp:1:1: remark: %s [-Rpass-analysis=kernel-resource-usage]\n"
    text = "".join(rem % s for s in (
        "Function Name: _Z7k_otherv", "    VGPRs: 200",
        "Function Name: _ZN1a7k_fusedILb1ELb0EEEvv", "    TotalSGPRs: 106", "    VGPRs: 109", "    ScratchSize [bytes/lane]: 0",
        "    Occupancy [waves/SIMD]: 4", "    SGPRs Spill: 2", "    VGPRs Spill: 0", "    LDS Size [bytes/block]: 37936"))
    assert chk.parse(text) == {"_ZN1a7k_fusedILb1ELb0EEEvv": {"vgprs": 109, "scratch": 0, "occupancy": 4, "sgpr_spills": 2, "vgpr_spills": 0, "lds": 37936}}


def test_k_fused_resources_within_limits():
    chk = _checker()
    if chk.hipcc() is None:
        pytest.skip("hipcc not found")
    res, bad = chk.report()
    print(res)
    assert len(res) == 3, sorted(res)
    assert not bad, bad
