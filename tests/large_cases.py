"""Tiled batches near the shape rule's limits and an on-device comparer (helpers only: no tests, no fixtures).

A large batch is T distinct frames repeated: frame b is tile[b % T].  Only the tile crosses the host link (upload_tiled
repeats it on the device), the references run on the T frames only, and mismatching_frames compares bit patterns on the
device in chunks, so that the only numbers that come back to the host are the first few frame indices that differ.

What makes a wrapped offset visible:
  the alias condition   T*H*W has an odd prime factor, so an offset that is wrong by a multiple of a power of two (2^29 ..
                        2^33 elements or bytes) never lands on identical content: the batch's period is T*H*W elements;
  the poison            every output is poisoned before a call: a store that went to another frame's copy of the same tile
                        frame (b - k*T) writes the right content there and still leaves frame b's poison behind;
  the inputs            are compared with the tile again after a call, so a stray store into them shows.

Tiers (frames of KITTI geometry, 352 x 1216 = 428 032 = 2^10 * 418 pixels):
  a  B = 1255  537 180 160 px    2^29 + 309 248 elements: a float32 array crosses 2 GiB
  b  B = 2509  1 073 932 288 px  2^30 + 190 464 elements: 4 GiB
  c  B = 5017  2 147 436 544 px  2^31 - 47 104: the shape rule's limit itself
and two more geometries at the limit: 96 x 352 with B = 63550 (2 048 px below 2^31, B near 65535) and 40 x 8150 with
B = 6587 (H + W - 2 = 8188, near 8192).
"""
import numpy as np

F = np.float32
KITTI = (352, 1216)
TIERS = {"a": 1255, "b": 2509, "c": 5017}  # KITTI frames per tier
LIMIT_GEOMETRIES = {"96x352": (63550, 96, 352), "40x8150": (6587, 40, 8150)}
FAMILIES = ("5%", "0.3%", "sky", "handful", "misaligned", "none")  # one frame of a fill tile each
CHUNK_BYTES = 512 << 20  # of `out` per comparison step: the gathered expectation and the mask stay under 2 GB with it


def has_odd_factor(n):
    """Does n have an odd prime factor (is it no power of two)?"""
    n = int(n)
    assert n >= 1
    while n % 2 == 0:
        n //= 2
    return n > 1


def assert_alias_free(T, frame_elems):
    """The alias condition: the period of a tiled batch, T * frame_elems elements, is no power of two."""
    assert T >= 1 and frame_elems >= 1
    assert has_odd_factor(T * frame_elems), "T * H * W = %d * %d is a power of two: a wrapped offset would read identical content" % (T, frame_elems)


def tier_shape(name):
    """(B, H, W) of a tier or of a limit geometry, with the arithmetic its name promises checked."""
    if name in TIERS:
        B, (H, W) = TIERS[name], KITTI
        lo = {"a": 2 ** 29, "b": 2 ** 30, "c": 2 ** 31 - H * W}[name]  # the first batch size past the threshold / the last one legal
        assert lo <= B * H * W < lo + H * W and B * H * W < 2 ** 31, (name, B * H * W)
    else:
        B, H, W = LIMIT_GEOMETRIES[name]
        assert 2 ** 31 - H * W <= B * H * W < 2 ** 31 and B <= 65535 and H + W - 2 < 8192
    return B, H, W


def fill_tile(H, W, seed=0):
    """The T = 6 frames of a fill tile [6, H, W], one per kernel family (FAMILIES): 5 % sources (the window kernel), 0.3 %
    (the any-distance kernels), 5 % sources under an empty sky of 30 rows (k_sky), a handful of sources (k_pts / k_l2pts),
    values in (val_thr, 0.9) that are no sources (the value list), and no source at all (label 0, the index-error status).
    The frames are those of tests/test_gpu_frame_ride.py."""
    from test_gpu_frame_ride import frame

    rng = np.random.default_rng(seed)
    frames = [frame("sky30" if kind == "sky" else kind, rng, H, W) for kind in FAMILIES]
    x = np.ascontiguousarray(np.stack(frames), F)
    assert_alias_free(len(FAMILIES), H * W)
    # the family mix, as far as the input decides it
    src = ~((F(1) - x) > F(0.1))
    n = src.reshape(len(FAMILIES), -1).sum(1)
    assert n[0] > 0.04 * H * W and 0 < n[3] <= 512 and n[5] == 0 and not src[2, :9].any() and n[2] > 0, n
    assert ((x[4] > F(0.1)) & (x[4] < F(0.9))).any()
    return x


def with_outliers(x, seed=0):
    """A copy of tile x with planted outliers (depths far above their neighbourhood's mean) in every frame that has sources
    and one negative value in the first frame: the outlier filter removes pixels, and its exhaustive second launch runs."""
    x = x.copy()
    rng = np.random.default_rng(seed)
    for f in x:
        pos = np.flatnonzero(f.reshape(-1) > 1.0)
        if pos.size:
            f.reshape(-1)[rng.choice(pos, min(40, pos.size), replace=False)] += F(60.0)
    x[0, x.shape[1] // 2, x.shape[2] // 2] = F(-2.5)
    return x


def payload_planes(P, H, W, seed=0):
    """P distinct payload planes [P, H, W] of arbitrary float32 bit patterns (NaN payloads, -0.0, subnormals among them): a
    gather copies bits."""
    rng = np.random.default_rng(seed)
    assert_alias_free(P, H * W)
    return rng.integers(0, 2 ** 32, (P, H, W), dtype=np.uint64).astype(np.uint32).view(F)


# ------------------------------------------------------------------------------------------------ device side
def _rows(t, n):
    """t as [n, elements per row] integer bit patterns (int32, or int16 for two-byte types)."""
    import torch

    t = t.reshape(n, -1)
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.int8}[t.element_size()])


def fill_tiled(out, tile):
    """out[j] = tile[j % T] for every row j of out ([n, ...] with the tile's frame shape), on out's device."""
    n, T = out.shape[0], tile.shape[0]
    assert tuple(out.shape[1:]) == tuple(tile.shape[1:]) and out.dtype == tile.dtype
    full = n // T
    if full:
        out[:full * T].view((full, T) + tuple(tile.shape[1:])).copy_(tile.unsqueeze(0).expand((full,) + tuple(tile.shape)))
    if n - full * T:
        out[full * T:].copy_(tile[:n - full * T])
    return out


def upload_tiled(tile, B, device):
    """numpy tile [T, ...] -> a new device tensor [B, ...] with frame b = tile[b % T]; only the tile crosses the host link."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(tile)).to(device)
    return fill_tiled(torch.empty((B,) + tuple(t.shape[1:]), dtype=t.dtype, device=device), t)


def mismatching_frames(out, expected, B, pick=None, frames=None, ignore=None, limit=8, chunk_bytes=CHUNK_BYTES, visited=None):
    """The first `limit` rows j of out ([B, ...], any 2- or 4-byte dtype) whose bit patterns differ from expected[pick(j)]
    (default j % T; expected: [T, ...] on out's device, same dtype).  frames: optional bool [T] on the host, rows whose
    expectation is not selected are not compared.  ignore: optional bool tensor of expected's shape on out's device, elements
    that are not compared (a rule that leaves single pixels open).  Works in chunks of at most chunk_bytes of out; only the mismatching row
    numbers come back to the host.  visited: optional list that receives the (first, last + 1) row ranges compared."""
    import torch

    T = expected.shape[0]
    assert out.shape[0] == B and out.dtype == expected.dtype and out.device == expected.device
    o, e = _rows(out, B), _rows(expected, T)
    assert o.shape[1] == e.shape[1], (tuple(out.shape), tuple(expected.shape))
    keep = None if frames is None else torch.as_tensor(np.asarray(frames, bool), device=out.device)
    ign = None if ignore is None else ignore.reshape(T, -1)
    step = max(1, int(chunk_bytes) // max(1, o.shape[1] * o.element_size()))
    bad = []
    for j0 in range(0, B, step):
        j1 = min(B, j0 + step)
        j = torch.arange(j0, j1, device=out.device)
        k = j % T if pick is None else pick(j)
        diff = o[j0:j1] != e[k]
        diff = (diff if ign is None else diff & ~ign[k]).any(1)
        if keep is not None:
            diff &= keep[k]
        if visited is not None:
            visited.append((j0, j1))
        hit = torch.nonzero(diff).reshape(-1)
        if hit.numel():
            bad += (hit[:limit] + j0).tolist()
            if len(bad) >= limit:
                break
    return bad[:limit]


def plane_pick(C, T, P):
    """pick() for a [B, C, H, W] payload seen as B*C planes: plane j = b*C + c expects expected[b % T][j % P], with expected
    flattened to [T*P, H, W].  P is coprime to C, so every channel meets every payload plane."""
    assert np.gcd(C, P) == 1 or C == 1
    return lambda j: ((j // C) % T) * P + j % P


def mismatching_planes(out, expected, B, C, limit=8, chunk_bytes=CHUNK_BYTES):
    """out [B, C, H, W] against expected [T, P, H, W] (tile frame x payload plane): the first (b, c) whose plane differs."""
    T, P = expected.shape[:2]
    bad = mismatching_frames(out.view((B * C,) + tuple(out.shape[2:])), expected.reshape((T * P,) + tuple(expected.shape[2:])), B * C,
                             pick=plane_pick(C, T, P), limit=limit, chunk_bytes=chunk_bytes)
    return [(j // C, j % C) for j in bad]


def poison_bits(t, byte=0xFF):
    """Fill any tensor with one byte value (0xFF: a NaN for float32, -1 for int32, 65535 for uint16)."""
    import torch

    t.view(torch.uint8).fill_(byte) if t.dtype != torch.uint8 else t.fill_(byte)
    return t


# ------------------------------------------------------------------------------------------------ exact host-side sums
def exact_sum(terms):
    """The exact sum of finite float32 terms as a Fraction, in integers: every term is an integer multiple of 2^s for the
    smallest unit in the last place s among them; the multiples are added as two 24-bit-apart limbs in int64."""
    from fractions import Fraction

    t = np.asarray(terms, F).reshape(-1).astype(np.float64)
    t = t[t != 0]
    if not t.size:
        return Fraction(0)
    assert np.isfinite(t).all()
    _, e = np.frexp(t)
    s = int(e.min()) - 24  # every term is a multiple of 2^s
    assert int(e.max()) - s <= 62 and t.size < 2 ** 24, "terms too far apart for the two-limb sum"
    k = np.ldexp(t, -s)
    assert np.array_equal(k, np.rint(k))
    k = k.astype(np.int64)
    total = (int((k >> 24).sum()) << 24) + int((k & ((1 << 24) - 1)).sum())
    return Fraction(total) * Fraction(2) ** s


def cell_sums(ids, terms, ncells):
    """The cell sum S(C) of include/dtfill.h (dtfill_fill_backward) for many cells at once: term i belongs to cell ids[i]
    (ids < 0: to none).  The same definition as fill_grad_ref.cell_sum, with the integer sums in int64 (|t| < 2^38, fewer
    than 2^24 terms) and only the last two roundings per cell in Python integers.  Returns float32 [ncells]."""
    import fill_grad_ref as R

    ids = np.asarray(ids, np.int64).reshape(-1)
    g = np.asarray(terms, F).reshape(-1)
    assert ids.shape == g.shape and g.size < 2 ** 24
    inside = ids >= 0
    ids, g = ids[inside], g[inside].astype(np.float64)
    flag = lambda sel: np.bincount(ids[sel], minlength=ncells) > 0  # noqa: E731
    nan, pinf, ninf = flag(np.isnan(g)), flag(np.isposinf(g)), flag(np.isneginf(g))
    fin = np.isfinite(g) & (g != 0)
    ids, g = ids[fin], g[fin]
    _, e = np.frexp(g)
    E = np.full(ncells, -10000, np.int64)
    np.maximum.at(E, ids, e.astype(np.int64) - 1)  # the true exponent floor(log2 |g|), subnormals included
    q = E - 37
    t = np.rint(np.ldexp(g, (-q[ids]).astype(np.int32)))  # exact scaling in float64, then round half to even
    Tsum = np.zeros(ncells, np.int64)
    np.add.at(Tsum, ids, t.astype(np.int64))
    out = np.zeros(ncells, F)
    for c in np.flatnonzero(Tsum):
        m, sh = R.f32_of_int(int(Tsum[c]))
        out[c] = R.ldexp_f32(m, sh + int(q[c]))
    out[pinf] = np.inf
    out[ninf] = -np.inf
    bits = out.view(np.uint32)
    bits[nan | (pinf & ninf)] = R.QNAN
    return out


def fill_backward_tile(x, index, grad, val_thr=0.1):
    """fill_grad_ref.backward with cell_sums: (grad_x float32 [T,H,W], status int32 [T])."""
    import fill_grad_ref as R

    x, grad = np.asarray(x, F), np.asarray(grad, F)
    gx, status = np.zeros(x.shape, F), np.zeros(x.shape[0], np.int32)
    for b in range(x.shape[0]):
        valued, idx, ok = R.frame_cells(x[b], np.asarray(index[b], np.int32), val_thr)
        if not ok:
            status[b] = R.INDEX_ERROR
            continue
        gx[b].reshape(-1)[valued] = cell_sums(idx, grad[b], valued.size)
    return gx, status


def gather_backward_tile(x, index, grad_planes, src_thr=0.1):
    """near_ref.backward for every (tile frame, gradient plane) pair with cell_sums: grad_planes [P,H,W] ->
    (grad_values float32 [T,P,H,W], status int32 [T])."""
    import near_ref as N

    x = np.asarray(x, F)
    P = grad_planes.shape[0]
    gv, status = np.zeros((x.shape[0], P) + x.shape[1:], F), np.zeros(x.shape[0], np.int32)
    for b in range(x.shape[0]):
        pix, k, status[b] = N.frame_ranks(x[b], index[b], src_thr)
        for p in range(P):
            gv[b, p].reshape(-1)[pix] = cell_sums(k, grad_planes[p], pix.size)
    return gv, status
