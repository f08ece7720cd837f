"""How far a TRUNCATING bf16 weight gradient lies from the statement, in units of the contract's bound: the figure behind
DESIGN.md section 29's "a bound cannot see the rounding".  CPU only; the operands are tests/test_gpu_conv2d_bf16_backward.py's own
N(0,1) data at (2,33,65), Cin 48, Cout 80, with x and g truncated to bf16 instead of rounded to nearest even.

    python scripts/bf16_dw_truncation.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import conv_ref as R  # noqa: E402
import convb_bf16_ref as RHB  # noqa: E402
import test_gpu_conv2d_bf16_backward as T  # noqa: E402  (numpy only at import)

F = np.float32


def truncated(a):
    return (np.ascontiguousarray(a, F).view(np.uint32) & 0xFFFF0000).view(F)


for (ksize, stride, transposed), name in zip(T.LAYERS, T.IDS):
    x, w, dy, y = T.random_layer(ksize, stride, transposed)
    dw, db, bw, bb = RHB.dw_ref(x, dy, y, ksize, stride, R.LEAKY, 0.2, transposed)
    tdw, tdb = RHB.dw_sum(truncated(x), truncated(RHB.g_ref(dy, y, R.LEAKY, 0.2)), ksize, stride, transposed)
    print("%-10s truncated operands: worst |dw - statement| / bound %.2f, db %.2f" % (name, (np.abs(tdw - dw) / bw).max(), (np.abs(tdb - db) / bb).max()))
