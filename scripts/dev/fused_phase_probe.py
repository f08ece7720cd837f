"""Development probe: where a k_fused window's cycles go (needs a libdtfill.so built with -DFUSED_PROF:
   make -C distancetransform-depthcompletion_amd/csrc -B HIPFLAGS='-O3 -std=c++17 --offload-arch=gfx950 -fPIC -DFUSED_PROF').
Prints, per phase, the cycles summed over all working waves and their share, and the trip counts of the level loop and the walk."""
import ctypes, importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
pkg = importlib.import_module("distancetransform-depthcompletion_amd")
L = pkg._lib.load()
L.dtfill_fused_prof.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
synth = importlib.import_module("distancetransform-depthcompletion_amd.synth")
x = torch.from_numpy(synth.make(sys.argv[1] if len(sys.argv) > 1 else "kitti_b32")).cuda()
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
for k, nm in enumerate(names):
    print("%-14s %12d cycles/pass  %7.0f cycles/wave  %5.1f %%" % (nm, buf[k] // n, buf[k] / w, 100.0 * buf[k] / max(tot, 1)))
bt = max(buf[10], 1)
print("waves/pass %d  levels/wave %.2f  batches/wave %.2f  walkers/batch %.1f  hop trips (two hops each)/batch %.2f"
      % (buf[8] // n, buf[9] / w, buf[10] / w, buf[11] / bt, buf[13] / bt))
