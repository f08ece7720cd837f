"""numpy statement of the depth_read contract (include/dtfill.h, dtfill_depth_read): the reference loader's
data_read.py:81-99 on decoded 16-bit PNG values.  Test infrastructure only: the product never imports it.

Pillow's NEAREST resize samples source index (int)xo with xo a running double sum (xo = 0.5 * a, then xo += a per output
pixel, a = in / out), not floor((j + 0.5) * in / out); the two differ for some size pairs (tests/golden/read_maps.npz)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

NOT_16BIT = 1  # DTFILL_READ_NOT_16BIT
BAD_DIMS = 2  # DTFILL_READ_BAD_DIMS


def running_map(n_in, n_out):
    """The source index of each of n_out output positions: a = n_in / n_out in double, y = 0.5 * a, idx = (int)y, y += a."""
    a = float(n_in) / float(n_out)
    y = 0.5 * a
    idx = np.empty(n_out, np.int64)
    for i in range(n_out):
        idx[i] = int(y)  # truncation toward zero; y > 0
        y += a
    return np.minimum(idx, n_in - 1)


def closed_form_map(n_in, n_out):
    """The textbook nearest-neighbour index floor((i + 0.5) * n_in / n_out): NOT what Pillow computes."""
    i = np.arange(n_out, dtype=np.float64)
    return np.minimum(np.floor((i + 0.5) * n_in / n_out).astype(np.int64), n_in - 1)


def depth_read_frame(raw, H, W):
    """One frame: raw (h, w) integer array with values in [0, 65535] -> (float32 [H, W], status bits)."""
    raw = np.asarray(raw)
    h, w = raw.shape
    ry, rx = running_map(h, H), running_map(w, W)
    out = raw[ry][:, rx].astype(np.float32) * np.float32(1.0 / 256.0)
    return out, (0 if raw.max() > 255 else NOT_16BIT)


def depth_read_batch(frames, H, W):
    """A list of 2-D frames of any sizes -> (float32 [B, H, W], int32 [B])."""
    outs, st = zip(*(depth_read_frame(f, H, W) for f in frames))
    return np.stack(outs), np.array(st, np.int32)


def reference_depth_read(depth_png, size=(1216, 352)):
    """What data_read.py:81-99 does to a decoded PNG array after the max check, restated with Pillow (np.float64 for the
    np.float the reference names, which newer numpy has removed): float64 / 256, a mode-F image, NEAREST resize to
    size = (width, height), float32 back, a channel axis."""
    from PIL import Image

    depth = np.asarray(depth_png, dtype=np.int64).astype(np.float64) / 256.0
    img = Image.fromarray(depth)
    nearest = Image.Resampling.NEAREST if hasattr(Image, "Resampling") else Image.NEAREST
    return np.expand_dims(np.array(img.resize(tuple(size), nearest)), -1)


def golden_pairs():
    """tests/golden/read_maps.npz (make_golden_read.py): name -> ((h, w, H, W), Pillow's ry, Pillow's rx)."""
    z = np.load(os.path.join(GOLDEN, "read_maps.npz"), allow_pickle=False)
    meta = json.load(open(os.path.join(GOLDEN, "read_maps.json")))
    return {name: (tuple(hwHW), z[name + "/ry"], z[name + "/rx"]) for name, hwHW in meta["pairs"].items()}
