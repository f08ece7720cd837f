"""Every argument check of the device layer, one bad call per row: the exception type and the argument it names.

Each row starts from a call that is right, spoils one thing, and expects the call to raise before anything is launched, so the
file costs tensor allocations only.  The tensors are tiny: [2,4,6] frames, [2,3,4,6] payloads, [2,5,7] uint16 / [2,5,7,3] uint8
raws with size=(6,4)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F, P = (2, 4, 6), (2, 3, 4, 6)


def _t(shape, dtype=torch.float32, device=DEV):
    return torch.empty(shape, dtype=dtype, device=device)


def _frames(*names):
    return lambda: {n: _t(F) for n in names}


def _gmcb():
    return dict(mask=_t(F), out2=_t(F), out3=_t(F), grads=[None, _t(F), _t(F), _t(F)], scale_num=4)


def _near():
    return dict(x=_t(F), index=_t(F, torch.int32), values=_t(P))


# call -> the arguments of a call that is right
GOOD = {
    "run": _frames("x"),
    "outlier_removal_device": _frames("x"),
    "generate_multi_channel_device": _frames("data", "mask"),
    "generate_multi_channel_backward_device": _gmcb,
    "demo_multi_channel_device": lambda: dict(lidar=_t(F), rgb=_t(F + (3,))),
    "crop_floor_device": _frames("x"),
    "png16_device": _frames("x"),
    "metrics_device": _frames("output", "target"),
    "train_loss_device": _frames("pred", "gt", "lidar", "correction"),
    "train_loss_backward_device": lambda: dict(_frames("pred", "gt", "lidar", "correction")(), stats=_t((6,), torch.float64),
                                               g_main=_t((), torch.float32), g_aux=_t((), torch.float32)),
    "fill_backward_device": lambda: dict(x=_t(F), index=_t(F, torch.int32), grad_depth=_t(F)),
    "nearest_gather_device": _near,
    "nearest_gather_backward_device": lambda: dict(x=_t(F), index=_t(F, torch.int32), grad_out=_t(P)),
    "line_subsample_device": lambda: dict(x=_t(F), K=torch.eye(3), E=torch.eye(4)),
    "depth_read_device": lambda: dict(raw=_t((2, 5, 7), torch.uint16), dims=[[5, 7], [4, 6]], size=(6, 4)),
    "rgb_read_device": lambda: dict(raw=_t((2, 5, 7, 3), torch.uint8), dims=[[5, 7], [4, 6]], size=(6, 4)),
}

# call -> its tensor arguments that get the four generic spoilings; the message names `arg must` unless a word is given
TENSOR_ARGS = {
    "run": ["x"],
    "outlier_removal_device": ["x"],
    "generate_multi_channel_device": [("data", "data"), ("mask", "mask")],
    "generate_multi_channel_backward_device": ["mask", "out2", "out3", "grads.1", "grads.3"],
    "demo_multi_channel_device": ["lidar", "rgb"],
    "crop_floor_device": ["x"],
    "png16_device": ["x"],
    "metrics_device": [("output", "output"), ("target", "target")],
    "train_loss_device": ["pred", "gt", "lidar", "correction"],
    "train_loss_backward_device": ["pred", "gt", "lidar", "correction"],
    "fill_backward_device": ["x", "index", "grad_depth"],
    "nearest_gather_device": ["x", "index", "values"],
    "nearest_gather_backward_device": ["x", "index", "grad_out"],
    "line_subsample_device": ["x"],
    "depth_read_device": ["raw"],
    "rgb_read_device": ["raw"],
}

OTHER_DTYPE = {torch.float32: torch.float64, torch.int32: torch.int64, torch.uint16: torch.int32, torch.uint8: torch.int32}


def _spoil(t, how):
    shape = tuple(t.shape)
    if how == "dtype":
        return _t(shape, OTHER_DTYPE[t.dtype])
    if how == "rank":
        return t[0]
    if how == "strided":
        v = _t(shape[:-1] + (2 * shape[-1],), t.dtype)[..., ::2]
        assert tuple(v.shape) == shape and not v.is_contiguous()
        return v
    assert how == "host"
    return _t(shape, t.dtype, "cpu")


def _set(kw, arg, f):
    """kw[arg] = f(kw[arg]); `grads.1` is element 1 of kw["grads"]."""
    if "." in arg:
        name, k = arg.split(".")
        kw[name][int(k)] = f(kw[name][int(k)])
    else:
        kw[arg] = f(kw[arg])


def _named(arg):
    return "%s[%s]" % tuple(arg.split(".")) if "." in arg else arg


ROWS = []  # (id, call, spoil(kw), exception, substring of the message)
for _call, _args in TENSOR_ARGS.items():
    for _a in _args:
        _arg, _word = _a if isinstance(_a, tuple) else (_a, _named(_a) + " must")
        for _how in ("dtype", "rank", "strided", "host"):
            ROWS.append(("%s-%s-%s" % (_call, _arg, _how), _call,
                         (lambda kw, arg=_arg, how=_how: _set(kw, arg, lambda t: _spoil(t, how))), ValueError, _word))


def row(call, what, exc, word, **changes):
    """A right call with these arguments replaced (a callable gets the right value and returns the wrong one)."""
    def spoil(kw):
        for k, v in changes.items():
            if callable(v):
                _set(kw, k.replace("__", "."), v)
            else:
                kw[k] = v
    ROWS.append(("%s-%s" % (call, what), call, spoil, exc, word))


wider = lambda t: _t((2, 4, 7), t.dtype)  # paired arguments whose shapes differ
row("generate_multi_channel_device", "shapes", ValueError, "mask", mask=wider)
row("generate_multi_channel_backward_device", "shapes", ValueError, "out2 must have mask's shape", out2=wider)
row("generate_multi_channel_backward_device", "grad-shapes", ValueError, "grads[2] must have mask's shape", grads__2=wider)
row("generate_multi_channel_backward_device", "out2-missing", ValueError, "out2 is needed", out2=None, scale_num=3)
row("generate_multi_channel_backward_device", "out3-missing", ValueError, "out3 is needed", out3=None, scale_num=4)
row("generate_multi_channel_backward_device", "three-grads", ValueError, "grads must hold four", grads=[None, None, None])
row("generate_multi_channel_backward_device", "scale_num", ValueError, "scale_num", scale_num=5)
row("demo_multi_channel_device", "shapes", ValueError, "rgb must", rgb=lambda t: _t((2, 4, 7, 3)))
row("demo_multi_channel_device", "scale_num", ValueError, "scale_num", scale_num=0)
row("crop_floor_device", "empty-crop", ValueError, "crop", rows=(3, 3))
row("crop_floor_device", "crop-outside", ValueError, "crop", cols=(0, 7))
row("metrics_device", "shapes", ValueError, "target", target=wider)
row("metrics_device", "rank", ValueError, "output", output=lambda t: _t((24,)), target=lambda t: _t((24,)))
row("metrics_device", "kind", ValueError, "kind", kind="eth3d")
for _loss in ("train_loss_device", "train_loss_backward_device"):
    row(_loss, "shapes", ValueError, "gt must have pred's shape", gt=wider)
    row(_loss, "dataset", ValueError, "dataset", dataset="ETH3D")
    row(_loss, "lidar-alone", ValueError, "lidar and correction", correction=None)
    row(_loss, "window", ValueError, "window", rows=(2, 9))
row("train_loss_backward_device", "stats-dtype", ValueError, "stats must", stats=lambda t: _t((6,), torch.float32))
row("train_loss_backward_device", "stats-size", ValueError, "stats must", stats=lambda t: _t((5,), torch.float64))
row("train_loss_backward_device", "g_main", ValueError, "g_main must", g_main=lambda t: _t((2,)))
row("train_loss_backward_device", "g_aux", ValueError, "g_aux must", g_aux=lambda t: _t((), torch.float64))
row("train_loss_backward_device", "no-gradient", ValueError, "no gradient", want_pred=False, want_correction=False)
row("train_loss_backward_device", "no-correction", ValueError, "needs correction", lidar=None, correction=None, want_correction=True)
row("fill_backward_device", "index-shape", ValueError, "index must have x's shape", index=wider)
row("fill_backward_device", "grad-shape", ValueError, "grad_depth must have x's shape", grad_depth=wider)
row("nearest_gather_device", "index-shape", ValueError, "index must have x's shape", index=wider)
row("nearest_gather_device", "values-frames", ValueError, "values must have x's frames", values=lambda t: _t((2, 3, 4, 7)))
row("nearest_gather_device", "values-batch", ValueError, "values must have x's frames", values=lambda t: _t((3, 3, 4, 6)))
row("nearest_gather_device", "no-channel", ValueError, "values must have 1 to 64 channels", values=lambda t: _t((2, 0, 4, 6)))
row("nearest_gather_device", "65-channels", ValueError, "values must have 1 to 64 channels", values=lambda t: _t((2, 65, 4, 6)))
row("nearest_gather_device", "nothing", ValueError, "nothing to compute", values=None, want_pixel=False)
row("nearest_gather_backward_device", "index-shape", ValueError, "index must have x's shape", index=wider)
row("nearest_gather_backward_device", "grad-frames", ValueError, "grad_out must have x's frames", grad_out=lambda t: _t((2, 3, 5, 6)))
row("nearest_gather_backward_device", "65-channels", ValueError, "grad_out must have 1 to 64 channels",
    grad_out=lambda t: _t((2, 65, 4, 6)))
row("nearest_gather_backward_device", "no-grad", ValueError, "grad_out must", grad_out=None)
row("line_subsample_device", "K-shape", ValueError, "K must be", K=torch.eye(4))
row("line_subsample_device", "E-batch", ValueError, "E must be", E=torch.zeros(3, 4, 4))
row("line_subsample_device", "keep_ratio", ValueError, "keep_ratio", keep_ratio=0.3)
row("line_subsample_device", "n_bins", ValueError, "n_bins", n_bins=0)
for _read in ("depth_read_device", "rgb_read_device"):
    row(_read, "dims-rows", ValueError, "dims must be [B, 2]", dims=[[5, 7], [4, 6], [3, 3]])
    row(_read, "dims-columns", ValueError, "dims must be [B, 2]", dims=torch.ones((2, 3), dtype=torch.int32))
    row(_read, "dims-flat", ValueError, "dims must be [B, 2]", dims=[5, 7, 4, 6])
    row(_read, "size-order", ValueError, "size must", size=(6.5, 4))
    row(_read, "size-zero", ValueError, "size must", size=(6, 0))
    row(_read, "size-one-number", ValueError, "size must", size=6)
row("rgb_read_device", "first_row-high", ValueError, "first_row must", first_row=4)
row("rgb_read_device", "first_row-negative", ValueError, "first_row must", first_row=-1)
row("rgb_read_device", "first_row-fraction", ValueError, "first_row must", first_row=1.5)
row("rgb_read_device", "want", ValueError, "want must", want="half")
row("rgb_read_device", "layout", ValueError, "layout must", layout="hwcn")
row("run", "out-name", ValueError, "no output named 'depht'", out=dict(depht=lambda: _t(F)))
row("run", "out-shape", ValueError, "out['depth'] must", out=dict(depth=lambda: _t((2, 4, 7))))
row("run", "out-dtype", ValueError, "out['index'] must", out=dict(index=lambda: _t(F, torch.int64)))
row("run", "out-status-shape", ValueError, "out['status'] must", out=dict(status=lambda: _t((3,), torch.int32)))
row("run", "out-host", ValueError, "out['dt'] must", out=dict(dt=lambda: _t(F, device="cpu")))
row("run", "out-strided", ValueError, "out['dt'] must", out=dict(dt=lambda: _spoil(_t(F), "strided")))
row("run", "out-cropped-depth", ValueError, "out['depth'] must", out=dict(depth=lambda: _t(F)), depth_rows_from=1)
row("run", "rows-from", ValueError, "depth_rows_from", depth_rows_from=4)
row("run", "timed-epilogue", ValueError, "depth_rows_from", depth_floor=0.9, timed=True)
row("run", "path", KeyError, "diagonal", path="diagonal")


@pytest.fixture(scope="module")
def op(pkg):
    """An operator of this file's own: the rows that reach the buffer check leave it with [2,4,6] buffers."""
    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    return pkg.device.DtFill(device=DEV)


@pytest.mark.parametrize("call,spoil,exc,word", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_bad_call_raises_and_names_the_argument(op, pkg, call, spoil, exc, word):
    kw = GOOD[call]()
    spoil(kw)
    if "out" in kw:  # (tensors are made inside the test, not while the table is read)
        kw["out"] = {k: v() if callable(v) else v for k, v in kw["out"].items()}
    f = op.run if call == "run" else getattr(pkg.device, call)
    with pytest.raises(exc) as e:
        f(**kw)
    assert word in str(e.value), "%s does not name %r" % (e.value, word)


def test_every_device_function_is_in_the_table(pkg):
    public = {n for n in vars(pkg.device) if n.endswith("_device") and not n.startswith("_")}
    assert public == set(GOOD) - {"run"}


def test_operator_metric(pkg):
    with pytest.raises(ValueError, match="metric"):
        pkg.device.DtFill(device=DEV, metric="l3")
