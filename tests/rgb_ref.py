"""numpy statement of the rgb_read contract (include/dtfill.h, dtfill_rgb_read): the reference loader's data_read.py:66-73
on decoded uint8 images and the drivers' rgb = img_batch[:, first_row:] / 255.0 as float32 (train.py:213-214).  Test
infrastructure only: the product never imports it.

Pillow's NEAREST resize of a uint8 image of any band count samples the same source indices as its mode-F resize, the running
double sum of read_ref.running_map (tests/test_rgb_read.py holds the two against each other)."""
import numpy as np

from read_ref import running_map

BAD_DIMS = 2  # DTFILL_READ_BAD_DIMS
UNIT = (np.arange(256) / 255.0).astype(np.float32)  # float32(float64(v) / 255.0): the reference's bits


def resize(raw, H, W):
    """One frame: uint8 [h, w] or [h, w, C] -> the same rank at H x W, as Image.fromarray(raw).resize((W, H), NEAREST)."""
    raw = np.asarray(raw)
    return raw[running_map(raw.shape[0], H)][:, running_map(raw.shape[1], W)]


def rgb_read_frame(raw, H, W, first_row=0, normalize=True, layout="nhwc"):
    """One frame: uint8 [h, w, C] -> (uint8 [H - first_row, W, C], float32 in `layout`)."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint8 and raw.ndim == 3
    u8 = resize(raw, H, W)[first_row:]
    f32 = (u8 / 255.0).astype(np.float32) if normalize else u8.astype(np.float32)
    if layout == "nchw":
        f32 = f32.transpose(2, 0, 1)
    return np.ascontiguousarray(u8), np.ascontiguousarray(f32)


def rgb_read_batch(frames, H, W, first_row=0, normalize=True, layout="nhwc", dims=None, hmax=None, wmax=None):
    """A list of [h, w, C] frames of any sizes -> (uint8 [B, H - first_row, W, C], float32 in `layout`, int32 [B]).  dims
    (optional, [B, 2]) stands for what a caller passes as the frames' sizes: a frame whose entry lies outside
    [1, hmax] x [1, wmax] comes back all zero with BAD_DIMS."""
    us, fs, st = [], [], []
    for b, f in enumerate(frames):
        u8, f32 = rgb_read_frame(f, H, W, first_row, normalize, layout)
        bad = dims is not None and not (1 <= dims[b][0] <= hmax and 1 <= dims[b][1] <= wmax)
        us.append(np.zeros_like(u8) if bad else u8)
        fs.append(np.zeros_like(f32) if bad else f32)
        st.append(BAD_DIMS if bad else 0)
    return np.stack(us), np.stack(fs), np.array(st, np.int32)


def hashed_frame(h, w, C, seed=0):
    """uint8 [h, w, C] whose values are a hash of (row, column, channel, seed): a shifted row or column or a swapped channel
    changes almost every value."""
    i, j, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(C, dtype=np.uint64),
                          indexing="ij")
    x = i * np.uint64(0x9E3779B1) + j * np.uint64(0x85EBCA77) + c * np.uint64(0xC2B2AE3D) + np.uint64(seed * 0x27D4EB2F)
    x ^= x >> np.uint64(15)
    x *= np.uint64(0x2C1B3C6D)
    x ^= x >> np.uint64(12)
    return (x & np.uint64(0xFF)).astype(np.uint8)


def padded(frames, fill=0xFF):
    """uint8 [B, hmax, wmax, C] with the padding holding `fill`, and the dims [B, 2]."""
    hmax = max(f.shape[0] for f in frames)
    wmax = max(f.shape[1] for f in frames)
    raw = np.full((len(frames), hmax, wmax, frames[0].shape[2]), fill, np.uint8)
    for b, f in enumerate(frames):
        raw[b, :f.shape[0], :f.shape[1]] = f
    return raw, np.array([f.shape[:2] for f in frames], np.int32)
