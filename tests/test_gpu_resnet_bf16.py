"""The three inference ResNets under precision = "bf16": the same sequence of layer calls on the same buffers as the float32
instance, only the wide and transposed calls going to the bf16 functions; every recorded bf16 call within the layer contract's
bound on its own recorded input (tests/conv_bf16_ref.py); and the properties the classes keep: no allocation on a second call,
finite outputs, and precision = "float32" the bits of an instance built without the argument."""
import importlib

import numpy as np
import pytest

import conv_bf16_ref as H
import conv_ref as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
SHAPE = (2, 8, 8)  # level 4 is 1 x 1
CLASSES = ("ResNet18", "ResNet18Image", "ResNet18LightImage")
GLOROT = {"ResNet18": "glorot_weights_resnet18", "ResNet18Image": "glorot_weights_resnet18_image",
          "ResNet18LightImage": "glorot_weights_resnet18_light_image"}
RECORDED = ("conv2d_device", "conv2d_image_device", "conv2d_strided_device", "conv2d_transpose_device", "conv2d_strided_bf16_device",
            "conv2d_transpose_bf16_device")


@pytest.fixture(scope="module")
def net(pkg):
    import torch

    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    pkg._lib.load()
    return importlib.import_module(pkg.__name__ + ".net")


def _labels(model, key):
    """data_ptr -> the name of the instance's own buffer there."""
    t = model._buffers[key]
    named = {"level[%d][%d]" % (k, i): b for k, three in enumerate(t.level) for i, b in enumerate(three)}
    named.update({"cat[%d]" % n: b for n, b in t.cat.items()})
    named.update({"pooled[%d]" % f: b for f, b in t.pooled.items()})
    named.update({"fills[%d]" % k: b for k, b in enumerate(t.fills)})
    for name in ("mask", "scaled", "correct", "a16", "b16", "one", "stems", "total1", "output", "correct_out"):
        named.setdefault(name, getattr(t, name))
    labels = {}
    for name, b in named.items():
        labels.setdefault(b.data_ptr(), name)  # (total1 may BE stems: the first name stands)
    return labels


def _recorded_run(net, monkeypatch, model, inputs):
    """One forward with every layer function of net.py wrapped; -> ([record], outputs).  A record: the function, the kernel
    tensor's data_ptr, the tensors and the other arguments as the call got them, clones of x and the residual from before the
    call and of the written slice of out from after it."""
    records = []

    def wrap(fname):
        inner = getattr(net, fname)

        def f(*args, **kw):
            assert not kw, "net.py passes the layer arguments by position"
            x, w, bias = args[:3]
            if "strided" in fname:
                stride, residual, act, alpha, out, out_offset = args[3:]
            elif "transpose" in fname:
                (act, alpha, out), stride, residual, out_offset = args[3:], 2, None, 0
            else:
                (act, alpha, out), stride, residual = args[3:6], 1, None
                out_offset = args[6] if len(args) > 6 else 0
            rec = dict(fn=fname, w=w.data_ptr(), x=x.data_ptr(), res=None if residual is None else residual.data_ptr(), out=out.data_ptr(),
                       bias=bias.detach().cpu().numpy(), stride=stride, act=act, alpha=alpha, out_offset=out_offset,
                       x_in=x.detach().clone(), res_in=None if residual is None else residual.detach().clone())
            got = inner(*args)
            rec["cout"] = bias.shape[0]
            rec["y"] = out[..., out_offset:out_offset + rec["cout"]].detach().clone()
            records.append(rec)
            return got

        return f

    with monkeypatch.context() as m:
        for fname in RECORDED:
            m.setattr(net, fname, wrap(fname))
        outputs = model(*inputs)
    return records, outputs


_runs = {}


def runs(net, monkeypatch, cls):
    """(float32 model, its records, bf16 model, its records, the inputs) of a class, run once per module and shared."""
    import torch

    if cls not in _runs:
        B, Hh, W = SHAPE
        synth = importlib.import_module(net.__name__.rsplit(".", 1)[0] + ".synth")
        weights = getattr(net, GLOROT[cls])(500 + len(cls), bias=0.1)
        x = torch.from_numpy(synth.kitti_iid(B, p=0.3, seed=5, hw=(Hh, W))).to(DEV)
        rgb = torch.from_numpy((np.random.default_rng(6).integers(0, 256, SHAPE + (3,)) / 255.0).astype(F)).to(DEV)
        inputs = (x, rgb) if cls != "ResNet18" else (x,)
        out = []
        for precision in ("float32", "bf16"):
            model = getattr(net, cls)(weights, precision=precision)
            records, outputs = _recorded_run(net, monkeypatch, model, inputs)
            out += [model, records, tuple(o.clone() for o in outputs)]
        _runs[cls] = tuple(out) + (inputs, weights)
    return _runs[cls]


def _layer_names(model, records):
    """The layer of each record, by the kernel tensor the call got."""
    by_ptr = {k.data_ptr(): name for name, (k, _) in model._on[next(iter(model._on))][0].items()}
    for packed in model._packed.values():
        by_ptr.update({p.data_ptr(): name for name, p in packed.items()})
    return [by_ptr[r["w"]] for r in records]


@pytest.mark.parametrize("cls", CLASSES)
def test_same_call_sequence_as_float32(net, monkeypatch, cls):
    import torch

    m32, r32, _, m16, r16, _, inputs, _ = runs(net, monkeypatch, cls)
    key = (inputs[0].device,) + SHAPE
    l32, l16 = _labels(m32, key), _labels(m16, key)
    n32, n16 = _layer_names(m32, r32), _layer_names(m16, r16)
    assert n32 == n16 and len(r32) == len(r16) > 30
    in32 = {t.data_ptr(): "input %d" % k for k, t in enumerate(inputs)}
    seen_wide = False
    for name, a, b in zip(n32, r32, r16):
        wide = name in m16.wide_layers
        assert wide == (a["fn"] in ("conv2d_strided_device", "conv2d_transpose_device")), name
        assert b["fn"] == (a["fn"].replace("_device", "_bf16_device") if wide else a["fn"]), name
        for what in ("x", "res", "out"):
            la = None if a[what] is None else l32.get(a[what], in32.get(a[what]))
            lb = None if b[what] is None else l16.get(b[what], in32.get(b[what]))
            assert la == lb and (la is not None or a[what] is None), (name, what, la, lb)
        for what in ("stride", "act", "alpha", "out_offset", "cout"):
            assert a[what] == b[what], (name, what)
        assert (a["bias"] == b["bias"]).all(), name
        if not seen_wide and not wide:  # the head, the stems and img_conv in front of the first wide layer: float32 in both
            assert torch.equal(a["y"].view(torch.int32), b["y"].view(torch.int32)), name
        seen_wide = seen_wide or wide
    assert sorted(set(n for n in n16 if n in m16.wide_layers)) == sorted(m16.wide_layers)


@pytest.mark.parametrize("cls", CLASSES)
def test_every_bf16_layer_within_its_contract(net, monkeypatch, cls):
    _, _, _, m16, r16, _, _, _ = runs(net, monkeypatch, cls)
    worst = 0.0
    for name, rec in zip(_layer_names(m16, r16), r16):
        if name not in m16.wide_layers:
            continue
        w = m16._host[name][0]  # [ksize,ksize,Cin,Cout]; the transposed layers' already exchanged
        x, res = rec["x_in"].cpu().numpy(), None if rec["res_in"] is None else rec["res_in"].cpu().numpy()
        act = C.LEAKY if rec["act"] == "leaky" else C.LINEAR
        if "transpose" in rec["fn"]:
            want, S = H.conv2d_transpose_bf16_ref(x, w, rec["bias"], act, rec["alpha"])
        else:
            want, S = H.conv2d_strided_bf16_ref(x, w, rec["bias"], rec["stride"], res, act, rec["alpha"])
        err, lim = np.abs(rec["y"].cpu().numpy().astype(np.float64) - want), H.bound(w.shape[0], w.shape[2], S, rec["bias"], res)
        assert want.shape == err.shape and (err <= lim).all(), "%s: worst |out - ref| / bound = %g" % (name, (err / lim).max())
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
    print("%s: worst |out - ref| / bound over the layers = %.4g" % (cls, worst))


@pytest.mark.parametrize("cls", CLASSES)
def test_bf16_keeps_the_instance_properties(net, monkeypatch, cls):
    import torch

    _, _, o32, m16, _, o16, inputs, _ = runs(net, monkeypatch, cls)
    for b in o16:
        assert torch.isfinite(b).all() and tuple(b.shape) == SHAPE
    assert torch.equal(o32[1].view(torch.int32), o16[1].view(torch.int32))  # lidar_correct: the correction branch is float32
    first = m16(*inputs)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    second = m16(*inputs)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(DEV) == before
    assert torch.cuda.max_memory_allocated(DEV) == before, "a bf16 call at a known shape allocated a temporary"
    assert second[0] is first[0] and second[1] is first[1]
    assert torch.equal(second[0].view(torch.int32), o16[0].view(torch.int32)), "two calls, two results"


@pytest.mark.parametrize("cls", CLASSES)
def test_float32_precision_is_the_default_bit_for_bit(net, monkeypatch, cls):
    import torch

    _, _, o32, _, _, _, inputs, weights = runs(net, monkeypatch, cls)
    plain = getattr(net, cls)(weights)
    assert plain.precision == "float32" and not plain._packed
    for a, b in zip(plain(*inputs), o32):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
