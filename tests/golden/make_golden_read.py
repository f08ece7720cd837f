"""Writes tests/golden/read_maps.npz: the source row / column index Pillow's NEAREST resize picks for each output row and
column, for the size pairs below.  Run on a machine where Pillow imports; the GPU tests read the maps instead of Pillow.

For each pair (h, w) -> (H, W): a mode-F image whose pixel (r, c) holds r * w + c (exact in float32 for these sizes) is
resized with Image.NEAREST; the result must be separable -- every output row samples one source row, every output column
one source column -- and the two index vectors are what is stored.

    python tests/golden/make_golden_read.py"""
import json
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
KITTI = (352, 1216)

# name -> ((h, w), (H, W))
PAIRS = {
    "kitti_375x1242": ((375, 1242), KITTI),
    "kitti_370x1224": ((370, 1224), KITTI),
    "kitti_374x1238": ((374, 1238), KITTI),
    "kitti_376x1241": ((376, 1241), KITTI),
    "identity_352x1216": (KITTI, KITTI),
    "vga_480x640": ((480, 640), KITTI),  # the closed form is wrong on the columns (640 -> 1216)
    "nyu_352x320_to_240x320": ((352, 320), (240, 320)),  # ... and on the rows (352 -> 240)
    "up_240x320": ((240, 320), KITTI),
    "one_1x1": ((1, 1), KITTI),
    "thin_1000x7": ((1000, 7), KITTI),
    "wide_100x3000": ((100, 3000), KITTI),
}


def pil_maps(h, w, H, W):
    code = (np.arange(h, dtype=np.float64)[:, None] * w + np.arange(w)[None, :]).astype(np.float32)
    assert code.max() < 2 ** 24
    img = Image.fromarray(code)
    assert img.mode == "F"
    out = np.array(img.resize((W, H), Image.NEAREST)).astype(np.int64)
    ry, rx = out // w, out % w
    assert (ry == ry[:, :1]).all() and (rx == rx[:1, :]).all(), "not separable"
    return ry[:, 0].astype(np.int32), rx[0].astype(np.int32)


def main():
    import PIL

    arrays, meta = {}, {"pillow": PIL.__version__, "pairs": {}}
    for name, ((h, w), (H, W)) in PAIRS.items():
        ry, rx = pil_maps(h, w, H, W)
        arrays[name + "/ry"], arrays[name + "/rx"] = ry, rx
        meta["pairs"][name] = [h, w, H, W]
    np.savez_compressed(os.path.join(HERE, "read_maps.npz"), **arrays)
    with open(os.path.join(HERE, "read_maps.json"), "w") as f:
        f.write('{"pillow": %s, "pairs": {\n' % json.dumps(meta["pillow"]))
        f.write(",\n".join(' %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in meta["pairs"].items()))
        f.write("\n}}\n")


if __name__ == "__main__":
    main()
