import functools
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_cases():
    z = np.load(os.path.join(GOLDEN, "cases.npz"), allow_pickle=False)
    meta = json.load(open(os.path.join(GOLDEN, "digests.json")))
    cases = {}
    for name in meta["cases"]:
        cases[name] = {k: z[name + "/" + k] for k in ("x", "thr", "dt", "lbl", "depth", "status")}
    return cases, meta["digests"]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def load_l2_cases():
    """The scipy-pinned fixtures of the l2 mode (tests/golden/make_golden_l2.py): x, squared distances, canonical nearest
    source (raster index, -1 without sources)."""
    z = np.load(os.path.join(GOLDEN, "l2_cases.npz"), allow_pickle=False)
    meta = json.load(open(os.path.join(GOLDEN, "l2_digests.json")))
    return {name: {k: z[name + "/" + k] for k in ("x", "d2", "near")} for name in meta["cases"]}, meta["digests"]


def labels_from_nearest(x, near, src_thr=0.1):
    """1-based raster rank of the source at raster index `near` (0 where near < 0): the label the l2 mode reports."""
    src = ~((np.float32(1.0) - x) > np.float32(src_thr))
    rank = (np.cumsum(src.ravel()) * src.ravel()).astype(np.int32)
    return np.where(near.ravel() >= 0, rank[np.maximum(near.ravel(), 0)], 0).reshape(x.shape).astype(np.int32)


def dt_bits(dt):
    """A distance map as uint32 bit patterns: an l2 dt is sqrtf (correctly rounded) of the exact integer d2 on the device, in the
    oracle and in numpy alike, so two of them are compared for equality of every bit (+inf included), not within a tolerance."""
    return np.ascontiguousarray(dt, np.float32).view(np.uint32)


TAP_CODES = tuple(range(13)) + (15,)  # the parent codes that can win (13 and 14 never do: code 12 matches wherever they match)


@functools.lru_cache(maxsize=None)
def tap_cover_batches():
    """Two small batches whose tie pixels make EVERY parent code that can win win somewhere, so that a wrong offset, weight or
    code at any call site of the 5x5 rule (the any-distance kernels' and k_pts's tie pixels, the window kernel's every pixel)
    shows as a wrong label: (a) 8 frames of 64 x 96 with 24 sources each, (b) 4 frames of 64 x 96 with 5 % sources (no distance
    beyond the window kernel's smaller halo).  The coverage is checked here, on the CPU, with the parallel model (once: the result is
    cached and shared, callers do not write to it)."""
    import parallel_model as pm

    H, W = 64, 96
    rng = np.random.default_rng(0)
    a = np.zeros((8, H, W), np.float32)
    for f in a:
        pos = rng.choice(H * W, 24, replace=False)
        f.flat[pos] = rng.uniform(0.95, 10, 24)
    rng = np.random.default_rng(0)
    b = np.stack([np.where(rng.random((H, W)) < 0.05, rng.uniform(0.95, 80, (H, W)), 0) for _ in range(4)]).astype(np.float32)

    def codes(x):
        tie, every, dmax = np.zeros(256, int), np.zeros(256, int), 0
        for f in x:
            src = ~((np.float32(1.0) - f) > np.float32(0.1))
            d, uniq, _, _, live = pm.rowscan_argmin(*pm.colscan_flags(src))
            code = pm.parent(d, live)
            finite = d < pm.BIG // 2
            tie += np.bincount(code[~(uniq | src) & finite], minlength=256)
            every += np.bincount(code[~src & finite], minlength=256)
            dmax = max(dmax, int(d[finite].max()))
        return tie, every, dmax

    tie_a, _, _ = codes(a)
    tie_b, every_b, dmax_b = codes(b)
    for c in TAP_CODES:
        assert tie_a[c] > 0 and tie_b[c] > 0 and every_b[c] > 0, (c, tie_a[c], tie_b[c], every_b[c])
    assert dmax_b <= 16
    return a, b
