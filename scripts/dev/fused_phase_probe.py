"""Development probe: where a k_fused window's cycles go (needs a libdtfill.so built with -DFUSED_PROF:
   make -C distancetransform-depthcompletion_amd/csrc -B HIPFLAGS='-O3 -std=c++17 --offload-arch=gfx950 -fPIC -DFUSED_PROF').
Prints, per phase, the cycles summed over all working waves and their share, and the trip counts of the level loop and the walk.
Then the timeline of one pass: per 1 us bin from the first wave's start, the working waves alive and the share of them in each
phase (absolute phase-entry times per wave, s_memrealtime at 100 MHz).  Usage: fused_phase_probe.py [workload] [bin_us]"""
import ctypes, importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
L = pkg._lib.load()
L.dtfill_fused_prof.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
L.dtfill_fused_timeline.argtypes = [ctypes.c_void_p, ctypes.c_int]
synth = importlib.import_module("distancetransform-depthcompletion_amd.synth")
wl = sys.argv[1] if len(sys.argv) > 1 else "kitti_b32"
bin_us = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
x = torch.from_numpy(synth.make(wl)).cuda()
op = pkg.device.DtFill(device="cuda:0")
for _ in range(20): op.run(x)
torch.cuda.synchronize()
buf = (ctypes.c_ulonglong * 16)()
L.dtfill_fused_prof(buf, 1)
n = 50
for _ in range(n): op.run(x)
torch.cuda.synchronize()
L.dtfill_fused_prof(buf, 1)
names = ["P0 load", "P1 levels", "P1b bwd taps", "P2 un-slice", "P3 hops", "P3 epilogue", "tail"]
tot = sum(buf[:7])
w = max(buf[8], 1)
print("workload", wl)
for k, nm in enumerate(names):
    print("%-14s %12d cycles/pass  %7.0f cycles/wave  %5.1f %%" % (nm, buf[k] // n, buf[k] / w, 100.0 * buf[k] / max(tot, 1)))
bt = max(buf[10], 1)
print("waves/pass %d  levels/wave %.2f  batches/wave %.2f  walkers/batch %.1f  hop trips (two hops each)/batch %.2f"
      % (buf[8] // n, buf[9] / w, buf[10] / w, buf[11] / bt, buf[13] / bt))

# ---- timeline of one pass
NW, NE = 1 << 16, 32
tl = np.zeros((NW, NE), dtype=np.uint64)
assert L.dtfill_fused_timeline(None, 1) == 0
op.run(x)
torch.cuda.synchronize()
assert L.dtfill_fused_timeline(tl.ctypes.data, 1) == 0
ev = tl[(tl[:, 0] != 0)]
t = (ev >> np.uint64(4)).astype(np.int64)
k = (ev & np.uint64(15)).astype(np.int64)
valid = ev != 0
t0 = t[:, 0].min()
tend = np.where(valid, t, 0).max()
nb = int(np.ceil((tend - t0) / (100.0 * bin_us))) + 1
# groups: front (P0..P2: 0-3), walk hops (4), epilogue + stores (5), tail (6)
groups = {"front": (0, 1, 2, 3), "hops": (4,), "epi+st": (5,), "tail": (6,)}
acc = {g: np.zeros(nb) for g in groups}
for i in range(ev.shape[0]):
    m = int(valid[i].sum())
    for j in range(1, m):
        a, b_, ph = (t[i, j - 1] - t0) / (100.0 * bin_us), (t[i, j] - t0) / (100.0 * bin_us), k[i, j]
        for g, ks in groups.items():
            if ph in ks:
                lo, hi = int(a), int(b_)
                for q in range(lo, hi + 1):
                    acc[g][q] += max(0.0, min(b_, q + 1) - max(a, q))
starts = (t[:, 0] - t0) / 100.0
last = np.where(valid, t, 0).max(axis=1)
lens = (last - t[:, 0]) / 100.0
print("timeline: %d working waves, span %.1f us, wave start min/med/max %.2f/%.2f/%.2f us, wave life med %.1f us (min %.1f, max %.1f)"
      % (ev.shape[0], (tend - t0) / 100.0, starts.min(), np.median(starts), starts.max(), np.median(lens), lens.min(), lens.max()))
print("%6s %7s %6s %6s %6s %6s" % ("us", "waves", "front", "hops", "epi+st", "tail"))
for q in range(nb):
    alive = sum(acc[g][q] for g in groups)
    if alive <= 0:
        continue
    print("%6.1f %7.0f %5.0f%% %5.0f%% %5.0f%% %5.0f%%" % (q * bin_us, alive, *(100.0 * acc[g][q] / alive for g in groups)))
