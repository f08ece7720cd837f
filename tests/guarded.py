"""Guarded and poisoned buffers for the buffer-contract tests (helpers only: no fixtures, no hooks).

GuardedBuffer lays one uint8 allocation out as [guard | offset | payload | guard]: a kernel that stores one byte outside its
payload changes a guard byte, and .check() says where.  poison() fills a buffer with contents a kernel must not depend on;
poison_op() does it to everything a DtFill owns (outputs, cropped depth, workspace) before a pass, so that a comparison can
only pass on values the pass itself stored.

The output poisons are values no correct pass can produce for these inputs:
  dt      a NaN bit pattern (a correct l1_cv dt is integer-valued or 8192; an l2 dt is sqrtf of an integer or +inf)
  index   INT32_MIN (labels are >= 0)
  depth   a NaN payload no input holds (depths are copies of input values; an epilogue's NaN is the canonical one)
  status  0x5A5A5A5A (defined bits: DTFILL_FRAME_*, 0..3)
"""
import numpy as np

GUARD_BYTE = 0xA5
GUARD_MIN = 64 << 10
KINDS = ("zero", "ones", "random", "previous")  # poison kinds, in the order the tests cycle through them

POISON_BITS = {"dt": 0x7FB5B5B5, "index": -0x80000000, "depth": 0x7FA5A5A5, "status": 0x5A5A5A5A}
_POISON_DTYPE = {"dt": np.float32, "index": np.int32, "depth": np.float32, "status": np.int32}


def _bits(name):
    """Output `name`'s poison as an int32 bit pattern."""
    return int(np.array([POISON_BITS[name]], np.int64).astype(np.uint32).view(np.int32)[0])


def poison_value(name):
    """The poison of output `name` as a numpy scalar of that output's dtype."""
    return np.array([_bits(name)], np.int32).view(_POISON_DTYPE[name])[0]


def is_poison(a, name):
    """Elementwise: does `a` (numpy, the output's dtype) still hold output `name`'s poison bit pattern?"""
    return np.ascontiguousarray(a).view(np.int32) == np.int32(_bits(name))


def _align256(n):
    return (n + 255) & ~255


class GuardedBuffer:
    """nbytes of payload starting `offset` bytes after a 256-byte boundary, with guards of at least frame_bytes + 64 KiB
    (a multiple of 256) on both sides.  The guards and the offset gap hold GUARD_BYTE."""

    def __init__(self, nbytes, offset=0, device="cuda:0", frame_bytes=0):
        import torch

        self.nbytes, self.offset = int(nbytes), int(offset)
        self.guard = _align256(int(frame_bytes) + GUARD_MIN)
        total = self.guard + _align256(self.offset + self.nbytes) + self.guard + 256
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        self.start = (-self.buf.data_ptr()) % 256  # first byte of the head guard, 256-byte aligned
        self.p0 = self.start + self.guard + self.offset  # payload, in bytes from the allocation's start
        self.p1 = self.p0 + self.nbytes
        self.buf.fill_(GUARD_BYTE)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.p0

    def payload(self):
        return self.buf[self.p0:self.p1]

    def view(self, dtype, shape):
        return self.payload().view(dtype).view(shape)

    def check(self, what="buffer"):
        """Raise AssertionError at the first guard byte that changed (the offset gap counts as head guard)."""
        import torch

        head = self.buf[self.start:self.p0]
        tail = self.buf[self.p1:self.p1 + self.guard]
        for part, name in ((head, "head"), (tail, "tail")):
            bad = torch.nonzero(part != GUARD_BYTE)
            if bad.numel():
                if name == "head":
                    k = int(bad[-1])  # the corrupted byte nearest to the payload
                    dist = "%d bytes before the payload" % (head.numel() - k)
                else:
                    k = int(bad[0])
                    dist = "%d bytes after the payload" % (k + 1)
                raise AssertionError("%s: %s guard corrupted (%d bytes), nearest at %s: 0x%02x" %
                                     (what, name, bad.numel(), dist, int(part[k])))


def poison(t, kind, seed=0):
    """Fill tensor t (any dtype, contiguous) with poison `kind`: "zero" (0x00), "ones" (0xFF) or "random" (seeded bytes
    generated on t's device).  "previous" needs a pass to run and is poison_op's."""
    import torch

    raw = t.view(torch.uint8) if t.dtype != torch.uint8 else t
    raw = raw.view(-1)
    if kind == "zero":
        raw.fill_(0)
    elif kind == "ones":
        raw.fill_(0xFF)
    elif kind == "random":
        g = torch.Generator(device=raw.device).manual_seed(int(seed))
        raw.copy_(torch.randint(0, 256, raw.shape, dtype=torch.uint8, device=raw.device, generator=g))
    else:
        raise ValueError("poison kind %r" % (kind,))
    return t


def poison_output(t, name):
    """Fill output tensor t (depth / dt / index / status) with that output's impossible value."""
    import torch

    t.view(torch.int32).fill_(_bits(name))
    return t


def other_input(shape, seed, device):
    """A different input of the same shape for the "previous pass" poison: 5 % sources, a few of them below the source
    threshold so that the value list is misaligned, generated on the device."""
    import torch

    g = torch.Generator(device=device).manual_seed(int(seed))
    u = torch.rand(shape, generator=g, device=device)
    v = torch.rand(shape, generator=g, device=device) * 79.0 + 1.0
    x = torch.where(u < 0.05, v, torch.zeros((), device=device))
    return torch.where(u < 0.002, torch.full((), 0.5, device=device), x).contiguous()


def poison_op(op, seed, shape=None, kind=None, path="auto", outlier_removal=False, depth_rows_from=None):
    """Poison a DtFill's outputs (_out, _crop) and its workspace in place before the next pass.  `shape` makes sure the
    buffers of that shape exist first; `depth_rows_from` (a pass with a depth epilogue next) that the cropped depth buffer of
    that pass exists, so that it is poisoned too.  kind (default: KINDS[seed % 4]):
      zero / ones / random  the workspace gets those bytes, every output its impossible value;
      previous              outputs and workspace hold what a pass over a different input of the same shape, on the other path
                            than `path`, left there -- values that look valid.
    Returns the kind used."""
    import torch

    if shape is not None:
        op._ensure(*shape)
    kind = KINDS[seed % len(KINDS)] if kind is None else kind
    B, H, W = op._shape
    if depth_rows_from is not None:
        crop = getattr(op, "_crop", None)
        if crop is None or tuple(crop.shape) != (B, H - depth_rows_from, W):
            op._crop = torch.empty((B, H - depth_rows_from, W), dtype=torch.float32, device=op.device)
    crop = getattr(op, "_crop", None)
    if kind == "previous":
        other = "general" if path != "general" else "auto"
        prev = op.run(other_input((B, H, W), seed, op.device), path=other, outlier_removal=outlier_removal and H >= 4 and W >= 4)
        if crop is not None and crop.shape[0] == B and crop.shape[2] == W:
            crop.copy_(prev["depth"][:, H - crop.shape[1]:])
        return kind
    for name, t in op._out.items():
        poison_output(t, name)
    if crop is not None:
        poison_output(crop, "depth")
    poison(op._ws, kind, seed)
    return kind
