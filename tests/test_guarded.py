"""Negative controls of the guarded / poisoned buffers (tests/guarded.py), on CPU tensors: a checker that cannot fail proves
nothing.  A store one element past the payload or one before it must trip .check(); every output poison must be a value no
correct pass can produce; every poison kind must fill what it says."""
import numpy as np
import pytest

from guarded import KINDS, GuardedBuffer, is_poison, poison, poison_output, poison_value

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("dtype,shape,offset", [(d, s, o) for d, s in ((torch.float32, (2, 3, 5)), (torch.int32, (7,)), (torch.uint16, (3, 9)),
                                                                          (torch.float64, (2, 9)))
                                                 for o in (0, 2, 4, 12, 64, 132) if o % torch.empty((), dtype=d).element_size() == 0])
def test_guard_catches_a_store_one_element_outside(dtype, shape, offset):
    esz = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape))
    g = GuardedBuffer(n * esz, offset, device="cpu", frame_bytes=n * esz)
    assert g.ptr % 256 == offset and g.guard % 256 == 0 and g.guard >= n * esz + (64 << 10)
    v = g.view(dtype, shape)
    assert v.data_ptr() == g.ptr and tuple(v.shape) == shape
    v.fill_(3)  # the whole payload, first and last byte included: legal
    g.check()
    for k, where in ((-1, "before"), (n, "after")):
        h = GuardedBuffer(n * esz, offset, device="cpu", frame_bytes=n * esz)
        # one element outside the payload, through the same typed view a kernel would use
        flat = h.buf[h.p0 + k * esz:h.p0 + (k + 1) * esz].view(dtype)
        flat.fill_(0)
        with pytest.raises(AssertionError, match="guard corrupted .%d bytes., nearest at 1 bytes %s the payload" % (esz, where)):
            h.check()
    # a single flipped byte deep in the tail guard, and in the offset gap between head guard and payload
    h = GuardedBuffer(n * esz, offset, device="cpu")
    h.buf[h.p1 + h.guard - 1] = 0
    with pytest.raises(AssertionError, match="tail guard"):
        h.check()
    if offset:
        h = GuardedBuffer(n * esz, offset, device="cpu")
        h.buf[h.p0 - offset] = 0x5A
        with pytest.raises(AssertionError, match="head guard"):
            h.check()


def test_output_poisons_are_impossible_answers():
    dt, depth = poison_value("dt"), poison_value("depth")
    # dt: NaN (legal: integer-valued >= 0, 8192, +inf); depth: a NaN whose payload is neither numpy's NaN nor the GPU's canonical
    # one (an epilogue's arithmetic on a NaN), so it cannot be a copy of an input or a computed value
    assert np.isnan(dt) and np.isnan(depth)
    canonical = {int(np.array([np.nan], np.float32).view(np.int32)[0]), 0x7FC00000, -0x400000}
    for v in (dt, depth):
        bits = int(np.array([v], np.float32).view(np.int32)[0])
        assert bits not in canonical
    assert int(np.array([dt], np.float32).view(np.int32)[0]) != int(np.array([depth], np.float32).view(np.int32)[0])
    assert poison_value("index") == np.iinfo(np.int32).min  # labels are >= 0
    st = int(poison_value("status"))
    assert st & ~3  # defined status bits: DTFILL_FRAME_INDEX_ERROR | DTFILL_FRAME_GENERAL_PATH
    # is_poison separates the poison from every legal value of the same dtype
    legal_dt = np.array([0, 1, 2, 8189, 8192, np.inf, np.sqrt(2.0)], np.float32)
    assert not is_poison(legal_dt, "dt").any() and not is_poison(np.array([np.nan], np.float32), "dt").any()
    assert not is_poison(np.array([0, 1, 2**31 - 1], np.int32), "index").any()
    assert not is_poison(np.arange(4, dtype=np.int32), "status").any()
    for name in ("dt", "index", "depth", "status"):
        t = poison_output(torch.zeros(5, dtype=torch.int32 if name in ("index", "status") else torch.float32), name)
        assert is_poison(t.numpy(), name).all()


def test_poison_kinds_fill_what_they_say():
    t = torch.zeros(4096, dtype=torch.float32)
    assert (poison(t, "ones").view(torch.uint8) == 0xFF).all()
    assert (poison(t, "zero").view(torch.uint8) == 0).all()
    a = poison(torch.zeros(4096, dtype=torch.uint8), "random", seed=1).clone()
    b = poison(torch.zeros(4096, dtype=torch.uint8), "random", seed=1)
    c = poison(torch.zeros(4096, dtype=torch.uint8), "random", seed=2)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.unique().numel() > 200  # random bytes, not a constant
    assert KINDS == ("zero", "ones", "random", "previous")
    with pytest.raises(ValueError):
        poison(t, "previous")  # needs a pass: poison_op's
