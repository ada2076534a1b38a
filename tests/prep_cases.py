"""The data-preparation rules restated in numpy, and the case tables of the data-preparation tests (test_cpu_data_prep*.py,
test_gpu_data_prep.py).  Independent of inconsistencymasks_amd.prep: nothing here imports the package.

The linear rule is OpenCV's default cv2.resize for 8-bit data as its published resize.cpp has it (fixed point, 11-bit weights);
the grey rule is cvtColor(BGR2GRAY)'s 15-bit fixed point of OpenCV 4.  Neither can be compared with OpenCV here."""
import math

import numpy as np

LINEAR, NEAREST = 0, 1
LABEL_PLUS1 = 1
GRAY, GRAY_THRESH, CLASS8 = 0, 1, 2


def scale_of(d, s):
    """1 / inv_scale as cv::resize forms it from dsize"""
    return 1.0 / (float(d) / float(s))


def _coord(n_dst, scale):
    """f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s: product and sum rounded separately in double"""
    f = (((np.arange(n_dst, dtype=np.float64) + 0.5) * np.float64(scale)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(np.float32)).astype(np.float32)


def _coef(v):
    return np.clip(np.rint(v.astype(np.float32) * np.float32(2048.0)), -32768, 32767).astype(np.int32)      # np.rint: half to even


def resize_linear(img, dh, dw):
    a = np.asarray(img, np.uint8)
    a3 = a if a.ndim == 3 else a[..., None]
    ch, cw = a3.shape[:2]
    s32 = a3.astype(np.int32)
    if cw == 2 * dw and ch == 2 * dh:
        out = (s32[0::2, 0::2] + s32[0::2, 1::2] + s32[1::2, 0::2] + s32[1::2, 1::2] + 2) >> 2
    else:
        sx, fx = _coord(dw, scale_of(dw, cw))
        lo, hi = sx < 0, sx >= cw - 1
        sx = np.where(lo, 0, np.where(hi, cw - 1, sx))
        fx = np.where(lo | hi, np.float32(0), fx).astype(np.float32)
        sx1 = np.minimum(sx + 1, cw - 1)
        a0, a1 = _coef(np.float32(1) - fx), _coef(fx)
        sy, fy = _coord(dh, scale_of(dh, ch))
        sy0, sy1 = np.clip(sy, 0, ch - 1), np.clip(sy + 1, 0, ch - 1)
        b0, b1 = _coef(np.float32(1) - fy), _coef(fy)
        hor = s32[:, sx] * a0[None, :, None] + s32[:, sx1] * a1[None, :, None]                            # [ch, dw, c] int32
        out = (((b0[:, None, None] * (hor[sy0] >> 4)) >> 16) + ((b1[:, None, None] * (hor[sy1] >> 4)) >> 16) + 2) >> 2
    out = out.astype(np.uint8)
    return out if a.ndim == 3 else out[..., 0]


def resize_nearest(img, dh, dw):
    a = np.asarray(img, np.uint8)
    ch, cw = a.shape[:2]
    sx = np.minimum(np.floor(np.arange(dw, dtype=np.float64) * scale_of(dw, cw)).astype(np.int64), cw - 1)
    sy = np.minimum(np.floor(np.arange(dh, dtype=np.float64) * scale_of(dh, ch)).astype(np.int64), ch - 1)
    return a[sy][:, sx]


def resize_float(img, dh, dw):
    """the second opinion: float64 half-pixel bilinear with edge clamp, unrounded"""
    a = np.asarray(img, np.float64)
    a3 = a if a.ndim == 3 else a[..., None]
    ch, cw = a3.shape[:2]
    x = np.clip((np.arange(dw) + 0.5) * (cw / dw) - 0.5, 0, cw - 1)
    y = np.clip((np.arange(dh) + 0.5) * (ch / dh) - 0.5, 0, ch - 1)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    x1, y1 = np.minimum(x0 + 1, cw - 1), np.minimum(y0 + 1, ch - 1)
    wx, wy = (x - x0)[None, :, None], (y - y0)[:, None, None]
    top = a3[y0][:, x0] * (1 - wx) + a3[y0][:, x1] * wx
    bot = a3[y1][:, x0] * (1 - wx) + a3[y1][:, x1] * wx
    out = top * (1 - wy) + bot * wy
    return out if a.ndim == 3 else out[..., 0]


def label_plus1(m):
    m = np.asarray(m, np.uint8)
    return np.where(m > 0, m + np.uint8(1), m).astype(np.uint8)      # uint8 wrap: 255 -> 0


def resize(img, dh, dw, interp, post=0, rect=None):
    a = np.asarray(img, np.uint8)
    if rect is not None:
        x0, y0, cw, ch = rect
        a = a[y0:y0 + ch, x0:x0 + cw]
    out = resize_linear(a, dh, dw) if interp == LINEAR else resize_nearest(a, dh, dw)
    return label_plus1(out) if post == LABEL_PLUS1 else out


def gray(img, b_first=False):
    """[h, w, 3] -> (R 9798 + G 19235 + B 3735 + 16384) >> 15; [h, w] / [h, w, 1]: a copy"""
    a = np.asarray(img, np.uint8)
    if a.ndim == 2 or a.shape[2] == 1:
        return a.reshape(a.shape[:2]).copy()
    a = a.astype(np.int64)
    r, b = (a[..., 2], a[..., 0]) if b_first else (a[..., 0], a[..., 2])
    return ((r * 9798 + a[..., 1] * 19235 + b * 3735 + 16384) >> 15).astype(np.uint8)


def gray_thresh(img, b_first=False):
    return np.where(gray(img, b_first) > 10, 255, 0).astype(np.uint8)


def class_table(color_to_class_mapping):
    """8 entries by (R >= 128) << 2 | (G >= 128) << 1 | (B >= 128) of a mapping {(r, g, b) in {0, 255}^3: class}; absent: 0"""
    t = np.zeros(8, np.uint8)
    for (r, g, b), k in color_to_class_mapping.items():
        t[((r >= 128) << 2) | ((g >= 128) << 1) | (b >= 128)] = k
    return t


def class8(img, table, b_first=False):
    a = np.asarray(img, np.uint8)
    r, b = (a[..., 2], a[..., 0]) if b_first else (a[..., 0], a[..., 2])
    code = ((r >= 128).astype(np.int64) << 2) | ((a[..., 1] >= 128).astype(np.int64) << 1) | (b >= 128)
    return np.asarray(table, np.uint8)[code]


def crops(plane, positions, ch, cw):
    return np.stack([plane[y:y + ch, x:x + cw] for x, y in positions], 0)


def get_positions(img_height, img_width, crop_size, overlap):
    x_count = round(img_width / (crop_size * (1 - overlap)))
    y_count = round(img_height / (crop_size * (1 - overlap)))
    x_move, y_move = img_width / x_count, img_height / y_count
    return [(min(int(i * x_move), img_width - crop_size), min(int(j * y_move), img_height - crop_size))
            for i in range(x_count) for j in range(y_count)]


def split(items, test_size, seed):
    """scikit-learn's train_test_split(items, test_size=float, random_state=seed) -> (train, test)"""
    n = len(items)
    n_test = int(math.ceil(test_size * n))
    if n_test <= 0 or n - n_test <= 0:
        raise ValueError("empty part")
    perm = np.random.RandomState(seed).permutation(n)
    return [items[i] for i in perm[n_test:]], [items[i] for i in perm[:n_test]]


def cityscapes_size(h, w, factor, base=16):
    """(dh, dw)"""
    return base * int(np.ceil(int(h * factor) / base)), base * int(np.ceil(int(w * factor) / base))


def noise(seed, *shape):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


# (source h, w) -> (dh, dw) of the linear items of the ragged batch; the last is a (x0, y0, cw, ch) rectangle of a 40 x 56 source
LINEAR_SIZES = [((17, 19), (16, 16)), ((37, 53), (16, 24)), ((5, 7), (16, 16)), ((32, 48), (16, 24)), ((16, 24), (16, 24))]
RECT_SOURCE, RECT, RECT_DST = (40, 56), (5, 3, 28, 20), (16, 24)
# second opinion on the linear rule: every size pair stays strictly below one grey level from the float bilinear
SECOND_OPINION_SIZES = [((37, 53), (16, 24)), ((48, 64), (256, 256)), ((96, 160), (32, 48)), ((64, 96), (32, 48)),
                        ((100, 75), (16, 16)), ((17, 19), (16, 16)), ((301, 257), (16, 32)), ((256, 256), (256, 256))]
