"""The optimizer of the reference's training loop on the device: tf.keras.optimizers.Adam(lr, beta_1=0.9) (train.py:169,
:253-254) as one fused pass over every variable, every bit fixed (include/dtfill.h, dtfill_adam_step; csrc/dtfill_adam.hpp).
adam_step_device is the call itself on torch tensors, KerasAdam the torch.optim.Optimizer a training loop holds, adam_step the
numpy form.  Reached as <package>.optim.

No captured-graph form: lr and the lists of pointers are launch arguments, read afresh on every call (a schedule changes lr,
zero_grad(set_to_none=True) makes every .grad a new tensor), and a replayed graph would freeze both.
"""
import ctypes
import math
import struct

import numpy as np
import torch

from . import _lib
from .device import _check_tensor, _require_gpu, _stream

RECORD_WORDS = 3  # the step record as int64 words: t, and the bits of the float64 b1p and b2p (dtfill_adam_record_bytes() / 8)


def segment_offsets(counts):
    """(per variable the offset of its moments in m and in v, the floats each of m and v holds): the prefix sum of the counts,
    each rounded up to a multiple of 4 (include/dtfill.h).  dtfill_adam_state_floats is the library's word on the total."""
    offsets, at = [], 0
    for n in counts:
        offsets.append(at)
        at += (int(n) + 3) // 4 * 4
    return offsets, at


def _check_scalars(lr, beta1, beta2, eps):
    """What dtfill_adam_step refuses with DTFILL_ERR_SHAPE, said by name."""
    for name, x in (("lr", lr), ("eps", eps)):
        if not (math.isfinite(x) and x >= 0):
            raise ValueError("%s must be finite and >= 0, got %r" % (name, x))
    for name, x in (("beta1", beta1), ("beta2", beta2)):
        if not 0 <= x < 1:
            raise ValueError("%s must lie in [0, 1), got %r" % (name, x))


def new_record(device):
    """A step record on `device` that has not stepped: t = 0, b1p = b2p = 1.0, written on the current stream."""
    record = torch.empty(RECORD_WORDS, dtype=torch.int64, device=device)
    init_record(record)
    return record


def init_record(record):
    _check_tensor(record, "record", dtype=torch.int64, layout="[3]")
    with torch.cuda.device(record.device):
        _lib.check(_lib.load().dtfill_adam_init(record.data_ptr(), _stream(record.device)))


def read_record(record):
    """(t, b1p, b2p) of a record as Python values; waits for the device."""
    return struct.unpack("<qdd", record.cpu().numpy().tobytes())


def write_record(record, t, b1p, b2p):
    record.copy_(torch.from_numpy(np.frombuffer(struct.pack("<qdd", int(t), float(b1p), float(b2p)), np.int64).copy()))


def adam_step_device(params, grads, m, v, record, lr, beta1=0.9, beta2=0.999, eps=1e-7):
    """One step of Keras' Adam on every variable that has a gradient, in place (include/dtfill.h, dtfill_adam_step).  params:
    contiguous float32 CUDA tensors on one device; grads: as many, each of its parameter's shape, or None for a variable that
    has no gradient in this step (its values and moments stay as they are).  m, v: flat float32 tensors of
    segment_offsets(counts)[1] floats, zero at the start; variable i's moments lie at segment_offsets(counts)[0][i] whoever
    else has a gradient.  record: new_record()'s.  lr, beta1, beta2, eps are rounded to float32.  Asynchronous on the current
    stream: no host synchronisation, no allocation on the device."""
    _require_gpu()
    params, grads = list(params), list(grads)
    if not params or len(grads) != len(params):
        raise ValueError("params and grads must be two lists of one length >= 1, got %d and %d" % (len(params), len(grads)))
    dev = params[0].device
    for i, (p, g) in enumerate(zip(params, grads)):
        _check_tensor(p, "params[%d]" % i, layout="[...]")
        if g is not None:
            _check_tensor(g, "grads[%d]" % i, layout="[...]", like=p, like_name="params[%d]" % i)
        if p.device != dev:
            raise ValueError("params[%d] is on %s, params[0] on %s" % (i, p.device, dev))
    counts = [p.numel() for p in params]
    floats = segment_offsets(counts)[1]
    for t, name in ((m, "m"), (v, "v")):
        _check_tensor(t, name, layout="[floats]")
        if t.numel() != floats or t.device != dev:
            raise ValueError("%s must hold %d floats on %s, got %d on %s" % (name, floats, dev, t.numel(), t.device))
    _check_tensor(record, "record", dtype=torch.int64, layout="[3]")
    if record.numel() != RECORD_WORDS or record.device != dev:
        raise ValueError("record must be new_record(%s)'s" % dev)
    _check_scalars(lr, beta1, beta2, eps)
    if all(g is None for g in grads):
        raise ValueError("no variable has a gradient")
    _launch(params, grads, (ctypes.c_longlong * len(counts))(*counts), m, v, record, lr, beta1, beta2, eps)


def _launch(params, grads, counts, m, v, record, lr, beta1, beta2, eps):
    """The call itself on checked tensors; counts: the ctypes array of the parameters' sizes.  The pointers are read here, on
    every call: a gradient is a new tensor each step."""
    n, dev = len(params), record.device
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dtfill_adam_step(
            (ctypes.c_void_p * n)(*[p.data_ptr() for p in params]),
            (ctypes.c_void_p * n)(*[None if g is None else g.data_ptr() for g in grads]),
            counts, n, m.data_ptr(), v.data_ptr(), record.data_ptr(), lr, beta1, beta2, eps, _stream(dev)))


class KerasAdam(torch.optim.Optimizer):
    """tf.keras.optimizers.Adam(lr, beta_1, beta_2, epsilon) for a torch training loop: train.py:169's optimizer, with every bit
    of the step fixed (include/dtfill.h, dtfill_adam_step).

        opt = KerasAdam(model.parameters(), lr=1e-3)
        loss.backward(); opt.step(); opt.zero_grad()

    It owns the moments m and v (two flat tensors, a segment per parameter, fixed here) and the step record.  step() passes
    the parameters whose .grad is not None, in parameter order; one without a gradient keeps its value and its moments.  The
    .grad tensors may be new ones every step.  After the first step nothing is allocated on the device and the host never
    waits.  lr is a plain attribute: the schedule is the driver's (train.py:166-167 halves it).  train.py builds a NEW
    optimizer every epoch, so its moments and step count restart there: reset() is that.  state_dict() / load_state_dict()
    carry m, v, t and the running powers, so a run resumed inside an epoch continues with the same bits."""

    def __init__(self, params, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        lr, beta_1, beta_2, epsilon = float(lr), float(beta_1), float(beta_2), float(epsilon)
        _check_scalars(lr, beta_1, beta_2, epsilon)
        super().__init__(params, {})
        if len(self.param_groups) != 1:
            raise ValueError("KerasAdam takes one group of parameters: Keras' optimizer has one lr for every variable")
        self.lr, self.beta_1, self.beta_2, self.epsilon = lr, beta_1, beta_2, epsilon
        self._params = list(self.param_groups[0]["params"])
        for i, p in enumerate(self._params):
            _check_tensor(p, "parameter %d" % i, layout="[...]")
            if p.device != self._params[0].device:
                raise ValueError("parameter %d is on %s, parameter 0 on %s" % (i, p.device, self._params[0].device))
        _require_gpu()
        dev = self._params[0].device
        self._counts = [p.numel() for p in self._params]
        self.offsets, floats = segment_offsets(self._counts)
        n = len(self._counts)
        self._counts_arr = (ctypes.c_longlong * n)(*self._counts)
        if _lib.load().dtfill_adam_state_floats(self._counts_arr, n) != floats:
            _lib.check(-2)
        self.m = torch.zeros(floats, dtype=torch.float32, device=dev)
        self.v = torch.zeros(floats, dtype=torch.float32, device=dev)
        self.record = new_record(dev)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grads = [p.grad for p in self._params]
        some = False
        for i, g in enumerate(grads):  # (the parameters, m, v and the record were checked when this object was built)
            if g is not None:
                _check_tensor(g, "a gradient", layout="[...]", like=self._params[i], like_name="its parameter")
                some = True
        if some:  # (no gradient anywhere: nothing moves and t stays, as torch's optimizers do)
            _check_scalars(self.lr, self.beta_1, self.beta_2, self.epsilon)
            _launch(self._params, grads, self._counts_arr, self.m, self.v, self.record, self.lr, self.beta_1, self.beta_2, self.epsilon)
        return loss

    def reset(self):
        """A new optimizer in place: zero moments, t = 0, on the current stream."""
        self.m.zero_()
        self.v.zero_()
        init_record(self.record)

    def moments(self, i):
        """(m, v) of parameter i, as views of its shape."""
        at, n, shape = self.offsets[i], self._counts[i], self._params[i].shape
        return self.m[at:at + n].view(shape), self.v[at:at + n].view(shape)

    def state_dict(self):
        t, b1p, b2p = read_record(self.record)
        return dict(m=self.m.clone(), v=self.v.clone(), t=t, b1p=b1p, b2p=b2p, counts=list(self._counts), lr=self.lr,
                    beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon)

    def load_state_dict(self, state):
        if list(state["counts"]) != self._counts:
            raise ValueError("the state is of parameters of %s elements, these have %s" % (list(state["counts"]), self._counts))
        lr, beta_1, beta_2, epsilon = (float(state[k]) for k in ("lr", "beta_1", "beta_2", "epsilon"))
        _check_scalars(lr, beta_1, beta_2, epsilon)
        self.lr, self.beta_1, self.beta_2, self.epsilon = lr, beta_1, beta_2, epsilon
        self.m.copy_(state["m"])
        self.v.copy_(state["v"])
        write_record(self.record, state["t"], state["b1p"], state["b2p"])


def adam_step(params, grads, m, v, state, lr, beta1=0.9, beta2=0.999, eps=1e-7):
    """The numpy form: one step on host arrays through the device.  params: float32 arrays; grads: as many, or None per entry;
    m, v: flat float32 arrays laid out by segment_offsets; state: (t, b1p, b2p), (0, 1.0, 1.0) at the start.  Returns (the new
    params, m, v, state); nothing is changed in place."""
    _require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    tp = [up(p) for p in params]
    tg = [None if g is None else up(g) for g in grads]
    tm, tv = up(m), up(v)
    record = torch.empty(RECORD_WORDS, dtype=torch.int64, device=dev)
    write_record(record, *state)
    adam_step_device(tp, tg, tm, tv, record, lr, beta1, beta2, eps)
    return [t.cpu().numpy() for t in tp], tm.cpu().numpy(), tv.cpu().numpy(), read_record(record)
