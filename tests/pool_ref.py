"""The contracts of dtfill_max_pool_pyramid and dtfill_max_pool_pyramid_backward (include/dtfill.h) in numpy, literally, for the
tests only: every window is scanned in raster order, element by element, vectorised over the batch and the channels and over
nothing else, and the backward is the three-term sum in its grouping.  The product does not import this file.
"""
import numpy as np

F = np.float32
LEVELS = (2, 4, 8)


def scan(x, k):
    """x float32 [B,H,W,C], H and W multiples of k -> (the winners' values [B,H/k,W/k,C], bit for bit, and their positions
    i * k + j in their windows, int64 of the same shape)."""
    x = np.ascontiguousarray(x, F)
    B, H, W, C = x.shape
    assert H % k == 0 and W % k == 0 and H >= k and W >= k, (x.shape, k)
    best = np.empty((B, H // k, W // k, C), F)
    at = np.zeros((B, H // k, W // k, C), np.int64)
    for h in range(H // k):
        for v in range(W // k):
            b = x[:, k * h, k * v, :].copy()  # best = the first element
            p = np.zeros((B, C), np.int64)
            for i in range(k):
                for j in range(k):
                    if i == 0 and j == 0:
                        continue
                    e = x[:, k * h + i, k * v + j, :]
                    with np.errstate(invalid="ignore"):
                        take = ~np.isnan(b) & ((e > b) | np.isnan(e))  # if best is not NaN and (e > best or e is NaN): best = e
                    b = np.where(take, e, b)
                    p = np.where(take, i * k + j, p)
            best[:, h, v, :] = b
            at[:, h, v, :] = p
    return best, at


def max_pool(x, k):
    """The forward of one level."""
    return scan(x, k)[0]


def pyramid(x, levels=LEVELS):
    """The forward: a tuple of pooled tensors along `levels`."""
    return tuple(max_pool(x, k) for k in levels)


def term(x, dy, k):
    """t_k [B,H,W,C]: dy_k at p's level-k window if p is that window's winner, +0 otherwise; all +0 for a dy of None."""
    x = np.ascontiguousarray(x, F)
    t = np.zeros(x.shape, F)
    if dy is None:
        return t
    dy = np.asarray(dy, F)
    _, at = scan(x, k)
    assert dy.shape == at.shape, (dy.shape, at.shape)
    for i in range(k):
        for j in range(k):
            t[:, i::k, j::k, :] = np.where(at == i * k + j, dy, F(0))
    return t


def backward(x, dys):
    """dys: (dy2, dy4, dy8), each an array or None.  dx[p] = (t_2 + t_4) + t_8 in float32."""
    t2, t4, t8 = (term(x, dy, k) for dy, k in zip(dys, LEVELS))
    with np.errstate(over="ignore", invalid="ignore"):
        return ((t2 + t4).astype(F) + t8).astype(F)


def hand_cases():
    """One 8 x 8 window of four channels each, [1,8,8,4]: (name, x, {level: (i, j) of the winner of the window that holds pixel
    (0, 0)}), the winners worked out by hand from the contract."""
    nan_a, nan_b = (np.array([bits], np.uint32).view(F)[0] for bits in (0x7FC00123, 0x7FC00456))

    def window(base, **at):
        x = np.full((1, 8, 8, 4), base, F)
        for key, value in at.items():
            x[0, int(key[1]), int(key[2]), :] = value
        return x

    return [
        # maxima in the 2x2 blocks 0 and 1 of a 4x4 window: (0,2) comes first in raster order, (1,0) first in block order
        ("tie across 2x2 blocks", window(0, p10=1, p02=1), {2: (1, 0), 4: (0, 2), 8: (0, 2)}),
        # the same one level up: the 4x4 blocks 0 and 1 of the 8x8 window
        ("tie across 4x4 blocks", window(0, p10=1, p04=1), {2: (1, 0), 4: (1, 0), 8: (0, 4)}),
        ("tie across 4x4 blocks, lower half first in block order", window(0, p30=1, p27=1), {2: (0, 0), 4: (3, 0), 8: (2, 7)}),
        ("+0 before -0", window(-1, p00=F(0.0), p01=F(-0.0)), {2: (0, 0), 4: (0, 0), 8: (0, 0)}),
        ("-0 before +0", window(-1, p00=F(-0.0), p01=F(0.0)), {2: (0, 0), 4: (0, 0), 8: (0, 0)}),
        ("a NaN after a larger value", window(0, p00=5, p23=np.nan), {2: (0, 0), 4: (2, 3), 8: (2, 3)}),
        ("two NaNs", window(0, p11=nan_a, p33=nan_b, p05=nan_b), {2: (1, 1), 4: (1, 1), 8: (0, 5)}),
    ]
