"""Guards k_fused's place on a CU: runs the compile of `make resources` (hipcc cross-compiles for gfx950 without a GPU),
reads the kernel-resource-usage remarks of the three k_fused instances and fails unless each has no scratch, at most 128
VGPRs, at most 40 960 B of LDS (four blocks in a CU's 160 KB) and an occupancy of 4 waves per SIMD.  The headline runs its
1 024 windows on 1 024 block slots in one round; a build that drops to three blocks per CU makes that two rounds.
Usage: python scripts/check_fused_resources.py   (exit status 0 = all three instances within the limits)"""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distancetransform-depthcompletion_amd", "csrc")
LIMITS = {"scratch": 0, "vgprs": 128, "lds": 40960}
OCCUPANCY = 4
INSTANCES = 3
FIELDS = {
    "VGPRs": "vgprs",
    "ScratchSize [bytes/lane]": "scratch",
    "Occupancy [waves/SIMD]": "occupancy",
    "SGPRs Spill": "sgpr_spills",
    "VGPRs Spill": "vgpr_spills",
    "LDS Size [bytes/block]": "lds",
}


def hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def parse(text):
    """{function name: {field: int}} of the remarks of every k_fused instance in the compiler's output"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name:\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {}) if "k_fused" in m.group(1) else None
            continue
        m = re.search(r"remark:\s+(.+?):\s+(\d+)\s+\[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def report():
    """Runs the compile and returns (resources per instance, list of violations)"""
    cc = hipcc()
    if cc is None:
        raise RuntimeError("hipcc not found")
    p = subprocess.run(["make", "-s", "-C", CSRC, "resources", "HIPCC=" + cc], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("`make resources` failed:\n" + p.stdout[-2000:])
    res = parse(p.stdout)
    bad = []
    if len(res) != INSTANCES:
        bad.append("expected %d k_fused instances in the remarks, found %d" % (INSTANCES, len(res)))
    for name, r in sorted(res.items()):
        missing = [k for k in ("scratch", "vgprs", "lds", "occupancy") if k not in r]
        if missing:
            bad.append("%s: no remark for %s" % (name, ", ".join(missing)))
            continue
        for k, lim in LIMITS.items():
            if r[k] > lim:
                bad.append("%s: %s %d > %d" % (name, k, r[k], lim))
        if r["occupancy"] != OCCUPANCY:
            bad.append("%s: occupancy %d, want %d" % (name, r["occupancy"], OCCUPANCY))
    return res, bad


def main():
    res, bad = report()
    for name, r in sorted(res.items()):
        print(name)
        print("   " + ", ".join("%s %s" % (k, r.get(k, "?")) for k in ("vgprs", "scratch", "lds", "occupancy", "sgpr_spills", "vgpr_spills")))
    for b in bad:
        print("FAIL:", b)
    print("k_fused resources:", "FAIL" if bad else "ok")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
