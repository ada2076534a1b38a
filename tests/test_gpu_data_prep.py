"""Data preparation on the GPU: imk_prep_resize and imk_prep_crops against the numpy restatement in tests/prep_cases.py (bit-exact), their
buffer and stream contract (tests/arena.py, tests/stream_skew.py), and the nine scripts end to end on toy raw trees."""
import ctypes
import os
import random
import shutil
import socket
import subprocess
import sys
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_cases as pc  # noqa: E402


@pytest.fixture(scope="module")
def prep():
    from inconsistencymasks_amd import prep as p
    return p


def _pack(arrays, pad=0):
    offs, total = [], pad
    for a in arrays:
        offs.append(total)
        total += a.size
    buf = np.full(total, 0xA5, np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.size] = a.reshape(-1)
    return buf, offs


def _resize(prep, arrays, dh, dw, interp, post=0, rects=None, pad=0):
    """one launch over the ragged batch -> numpy [n, dh, dw, c]"""
    buf, offs = _pack(arrays, pad)
    items = [prep.make_item(o, a.shape[0], a.shape[1], dh, dw, rects[i] if rects else None) for i, (a, o) in enumerate(zip(arrays, offs))]
    return prep.prep_resize(torch.from_numpy(buf).cuda(), items, arrays[0].shape[2], dh, dw, interp, post).cpu().numpy()


def _rect_source(c, seed):
    """40 x 56 noise in 0..127 inside the rectangle, 255 everywhere around it: a tap outside the rectangle moves the result"""
    x0, y0, cw, ch = pc.RECT
    a = np.full(pc.RECT_SOURCE + (c,), 255, np.uint8)
    a[y0:y0 + ch, x0:x0 + cw] = pc.noise(seed, ch, cw, c) >> 1
    return a


def _linear_sources(c):
    srcs = [pc.noise(10 + i, h, w, c) for i, ((h, w), _) in enumerate(pc.LINEAR_SIZES)] + [_rect_source(c, 77)]
    return srcs, [None] * len(pc.LINEAR_SIZES) + [pc.RECT]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("dst", [(16, 24), (16, 16), (16, 18), (24, 36)])
@pytest.mark.parametrize("pad", [0, 1])
def test_resize_linear_ragged_batch(prep, c, dst, pad):
    """every source of the table (both borders, upscale with s < 0, exact 2x, identity, a poisoned sub-rectangle) in ONE launch per
    destination size: 16 x 24 and 16 x 16 are the table's own pairs, 16 x 18 has 54-byte rows at c = 3, 24 x 36 upscales the
    rectangle so that both of its borders clamp.  pad = 1 makes every src_off odd or unaligned."""
    srcs, rects = _linear_sources(c)
    got = _resize(prep, srcs, dst[0], dst[1], pc.LINEAR, 0, rects, pad)
    for i, (a, r) in enumerate(zip(srcs, rects)):
        want = pc.resize(a, dst[0], dst[1], pc.LINEAR, 0, r)
        assert np.array_equal(got[i], want), (i, a.shape, r, int(np.abs(got[i].astype(int) - want).max()))
    if dst == (16, 24):
        assert np.array_equal(got[4], srcs[4])                                                  # equal sizes: the identity
        s = srcs[3].astype(np.int32)
        assert np.array_equal(got[3], ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    assert got[5].max() <= 127                                                                  # nothing of the 255 border came in


@pytest.mark.parametrize("c", [1, 3])
def test_resize_single_item_batch(prep, c):
    a = pc.noise(5, 37, 53, c)
    assert np.array_equal(_resize(prep, [a], 16, 24, pc.LINEAR)[0], pc.resize_linear(a, 16, 24))


@pytest.mark.parametrize("dst", [(16, 24), (16, 16), (24, 36)])
def test_resize_nearest_label_plus1(prep, dst):
    """the same sizes with c = 1 and label values: 255 wraps to 0, 0 stays 0"""
    vals = np.array([0, 1, 33, 254, 255], np.uint8)
    srcs, rects = _linear_sources(1)
    srcs = [vals[a % 5] for a in srcs]
    got = _resize(prep, srcs, dst[0], dst[1], pc.NEAREST, pc.LABEL_PLUS1, rects, 1)
    for i, (a, r) in enumerate(zip(srcs, rects)):
        assert np.array_equal(got[i], pc.resize(a, dst[0], dst[1], pc.NEAREST, pc.LABEL_PLUS1, r)), i
    assert set(np.unique(got)) == {0, 2, 34, 255}
    plain = _resize(prep, srcs, dst[0], dst[1], pc.NEAREST, 0, rects)
    assert np.array_equal(pc.label_plus1(plain), got)


@pytest.mark.parametrize("src,dst,c,interp,post", [((300, 400), (256, 256), 3, pc.LINEAR, 0), ((1024, 2048), (208, 416), 3, pc.LINEAR, 0),
                                                   ((1024, 2048), (208, 416), 3, pc.NEAREST, pc.LABEL_PLUS1),
                                                   ((1024, 2048), (208, 416), 1, pc.LINEAR, 0),
                                                   ((1024, 2048), (208, 416), 1, pc.NEAREST, pc.LABEL_PLUS1)])
def test_resize_product_shapes(prep, src, dst, c, interp, post):
    a = pc.noise(3, src[0], src[1], c)
    assert np.array_equal(_resize(prep, [a], dst[0], dst[1], interp, post)[0], pc.resize(a, dst[0], dst[1], interp, post))


def test_resize_refusals(prep):
    from inconsistencymasks_amd._lib import lib
    a = pc.noise(1, 8, 8, 3)
    src = torch.from_numpy(a.reshape(-1).copy()).cuda()
    items = prep.items_to_device([prep.make_item(0, 8, 8, 4, 4)])
    out = torch.full((4 * 4 * 4,), 7, dtype=torch.uint8, device="cuda")
    call = lambda **k: lib.imk_prep_resize(k.get("src", src.data_ptr()), src.numel(), items.data_ptr(), k.get("n", 1), k.get("c", 3), 4,
                                           k.get("dw", 4), k.get("interp", 0), k.get("post", 0), out.data_ptr(), None)
    assert call(c=2) == -2 and call(c=4) == -2
    assert call(n=0) == -1 and call(dw=0) == -1 and call(interp=2) == -1 and call(post=2) == -1 and call(src=None) == -1 and call(n=65536) == -1
    torch.cuda.synchronize()
    assert int((out != 7).sum()) == 0                      # a refused call writes nothing
    # an item whose rectangle or source leaves what it was given is written as zeros, nothing is read for it
    bad = [prep.make_item(0, 8, 8, 4, 4), prep.make_item(0, 8, 8, 4, 4), prep.make_item(0, 8, 8, 4, 4)]
    bad[0].cw, bad[1].src_off, bad[2].src_h = 9, 1, 9
    got = prep.prep_resize(src, bad + [prep.make_item(0, 8, 8, 4, 4)], 3, 4, 4).cpu().numpy()
    assert not got[:3].any() and np.array_equal(got[3], pc.resize_linear(a, 4, 4))


# ---- imk_prep_crops -------------------------------------------------------------------------------
POSITIONS = [(0, 0), (40, 24), (13, 7), (20, 10), (21, 11)]      # the corners of a 40 x 56 source, an odd one, two that overlap it
TABLE = np.array([9, 3, 0, 250, 1, 77, 255, 5], np.uint8)


def _crops(prep, a, positions, ch, cw, rule, table=None, b_first=False):
    return prep.prep_crops(torch.from_numpy(np.ascontiguousarray(a)).cuda(), positions, ch, cw, rule, table, b_first).cpu().numpy()


def _want(a, rule, b_first):
    if rule == pc.CLASS8:
        return pc.class8(a, TABLE, b_first)
    return pc.gray(a, b_first) if rule == pc.GRAY else pc.gray_thresh(a, b_first)


@pytest.mark.parametrize("c,rule", [(1, pc.GRAY), (3, pc.GRAY), (1, pc.GRAY_THRESH), (3, pc.GRAY_THRESH), (3, pc.CLASS8)])
@pytest.mark.parametrize("b_first", [False, True])
def test_crops_rules(prep, c, rule, b_first):
    a = pc.noise(21 + c, 40, 56, c)
    if rule == pc.CLASS8:
        a = np.array([0, 127, 128, 255], np.uint8)[a % 4]      # all 8 codes, both sides of the threshold
    if rule == pc.GRAY_THRESH:
        a[:4] = np.array([9, 10, 11, 255], np.uint8)[:, None, None]
    plane = _want(a, rule, b_first)
    got = _crops(prep, a, POSITIONS, 16, 16, rule, TABLE if rule == pc.CLASS8 else None, b_first)
    assert np.array_equal(got, pc.crops(plane, POSITIONS, 16, 16))
    whole = _crops(prep, a, [(0, 0)], 40, 56, rule, TABLE if rule == pc.CLASS8 else None, b_first)      # the whole-image form
    assert np.array_equal(whole[0], plane)
    odd = _crops(prep, a, POSITIONS[2:4], 15, 13, rule, TABLE if rule == pc.CLASS8 else None, b_first)  # rows that are no words
    assert np.array_equal(odd, pc.crops(plane, POSITIONS[2:4], 15, 13))
    if rule == pc.CLASS8:
        assert set(np.unique(whole)) == set(TABLE.tolist())


def test_crops_grey_pins(prep):
    """the pinned property: R == G == B comes out as it is (every channel image HeLa reads from a grey file); the threshold is > 10"""
    g = pc.noise(4, 40, 56, 1)
    g[0, :4, 0] = [9, 10, 11, 255]
    rep = np.repeat(g, 3, 2)
    for b_first in (False, True):
        assert np.array_equal(_crops(prep, rep, [(0, 0)], 40, 56, pc.GRAY, None, b_first)[0], g[..., 0])
        t = _crops(prep, rep, [(0, 0)], 40, 56, pc.GRAY_THRESH, None, b_first)[0]
        assert t[0, :4].tolist() == [0, 0, 255, 255] and np.array_equal(t, np.where(g[..., 0] > 10, 255, 0))
    assert np.array_equal(_crops(prep, g, [(0, 0)], 40, 56, pc.GRAY)[0], g[..., 0])


def test_crops_refusals(prep):
    from inconsistencymasks_amd._lib import lib
    a = torch.from_numpy(pc.noise(1, 8, 8, 3)).cuda()
    pos = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    out = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    call = lambda c=3, rule=0, n=1, table=None, cw=8: lib.imk_prep_crops(a.data_ptr(), 8, 8, c, pos.data_ptr(), n, 8, cw, rule, table, 0,
                                                                        out.data_ptr(), None)
    assert call(c=2) == -2 and call(rule=3) == -1 and call(n=0) == -1 and call(cw=0) == -1
    assert call(rule=2) == -1                                        # CLASS8 without its table
    assert call(c=1, rule=2, table=TABLE.ctypes.data) == -2          # CLASS8 on one channel
    torch.cuda.synchronize()
    assert int((out != 7).sum()) == 0
    # a crop that leaves the source: the pixels outside are 0
    got = _crops(prep, a.cpu().numpy(), [(4, 5)], 8, 8, pc.GRAY)[0]
    want = np.zeros((8, 8), np.uint8)
    want[:3, :4] = pc.gray(a.cpu().numpy())[5:, 4:]
    assert np.array_equal(got, want)


# ---- the public functions themselves ---------------------------------------------------------------
def test_random_crop_under_the_recorded_seeds(prep):
    """random_crop itself, on the global generators: the reference's recorded (y, x, size) draws decide what it returns"""
    with np.load(os.path.join(ROOT, "tests", "golden", "data_prep.npz")) as d:
        cases = [(int(d[f"crop{i}_seed"]), d[f"crop{i}_shape"].tolist(), d[f"crop{i}_draw"].tolist()) for i in range(6)]
    for seed, (h, w), (y, x, size) in cases:
        img, mask = pc.noise(seed, h, w, 3), pc.noise(seed + 1, h, w)
        random.seed(seed)
        np.random.seed(seed)
        got_i, got_m = prep.random_crop(img, mask)
        rect = None if size < 0 else (x, y, size, size)
        assert got_i.shape == (256, 256, 3) and got_m.shape == (256, 256)
        assert np.array_equal(got_i, pc.resize(img, 256, 256, pc.LINEAR, 0, rect)), seed
        assert np.array_equal(got_m, pc.resize(mask, 256, 256, pc.NEAREST, 0, rect)), seed


def test_single_file_functions(prep, tmp_path):
    """resize_image, convert_color_bmp_to_class_mask_png, ImagePreprocessor.process_crops / mod_pos_size, create_random_crops: each
    called once as the reference's callers would, against prep_cases on the Pillow-decoded source"""
    from PIL import Image
    from inconsistencymasks_amd import functions as F
    save = lambda a, p: (os.makedirs(os.path.dirname(p), exist_ok=True), Image.fromarray(a).save(p))
    # Cityscapes: one image, one label map
    img, lab = pc.noise(1, 64, 96, 3), np.array([0, 1, 33, 254, 255], np.uint8)[pc.noise(2, 64, 96) % 5]
    save(img, str(tmp_path / "c" / "a_leftImg8bit.png"))
    save(lab, str(tmp_path / "c" / "a_gtFine_labelIds.png"))
    assert np.array_equal(prep.resize_image(str(tmp_path / "c" / "a_leftImg8bit.png"), 0.2), pc.resize_linear(img, 16, 32))
    got = prep.resize_image(str(tmp_path / "c" / "a_gtFine_labelIds.png"), 0.2, 16, True)
    assert np.array_equal(got, np.repeat(pc.resize_nearest(lab, 16, 32)[..., None], 3, 2))           # no + 1 here: that is process_images'
    # SUIM: one colour mask
    mapping = {(255 * (k >> 2 & 1), 255 * (k >> 1 & 1), 255 * (k & 1)): k + 1 for k in range(8)}
    bmp = np.array([0, 120, 130, 255], np.uint8)[pc.noise(3, 30, 44, 3) % 4]
    save(bmp, str(tmp_path / "s" / "m.bmp"))
    prep.convert_color_bmp_to_class_mask_png(str(tmp_path / "s" / "m.bmp"), str(tmp_path / "s" / "m.png"), mapping)
    assert np.array_equal(_png(str(tmp_path / "s" / "m.png"), 1), pc.class8(bmp, pc.class_table(mapping)))
    # HeLa: one crop of every channel, then the position redraw of a directory
    org = tmp_path / "h" / "org"
    bf, alive = pc.noise(4, 64, 96), np.array([0, 9, 10, 11, 255], np.uint8)[pc.noise(5, 64, 96) % 5]
    pos = np.zeros((64, 96), np.uint8)
    for cy, cx in ((12, 14), (30, 60), (50, 20)):
        pos[cy - 2:cy + 3, cx - 2:cx + 3] = 255
    save(bf, str(org / "brightfield" / "x.png"))
    save(alive, str(org / "alive" / "x.png"))
    save(pos, str(org / "position" / "x.png"))
    pre = prep.ImagePreprocessor(str(org), str(tmp_path / "h" / "out"), 48, 0.6, use_mod_pos_size=False)
    pre.process_crops((13, 7), "x.png", 5)
    assert np.array_equal(_png(str(tmp_path / "h" / "out" / "brightfield" / "x_5.png"), 1), bf[7:55, 13:61])
    assert np.array_equal(_png(str(tmp_path / "h" / "out" / "alive" / "x_5.png"), 1), pc.gray_thresh(alive)[7:55, 13:61])
    assert np.array_equal(_png(str(tmp_path / "h" / "out" / "position" / "x_5.png"), 1), pos[7:55, 13:61])
    assert not (tmp_path / "h" / "out" / "dead").exists()
    pre.mod_pos_size(str(org / "position"), str(org / "mod_position"))
    want = F.mod_pos_size(pos)
    assert want.any() and np.array_equal(_png(str(org / "mod_position" / "x.png")), np.repeat(want[..., None], 3, 2))
    # SUIM crops with the reference's own sizes (256 .. 511 -> 256): one image that is cropped, one too small for its draw
    files = {"big.jpg": (300, 400), "small.jpg": (200, 260)}
    for n, (h, w) in files.items():
        save(pc.noise(6, h // 8 + 1, w // 8 + 1, 3).repeat(8, 0).repeat(8, 1)[:h, :w].copy(), str(tmp_path / "u" / "images" / n))
        save(pc.noise(7, h, w) % 9, str(tmp_path / "u" / "masks" / (n[:-4] + ".png")))
    prep.create_random_crops(str(tmp_path / "u" / "images"), str(tmp_path / "u" / "masks"), str(tmp_path / "u" / "val"), 2)
    listing = [f for f in os.listdir(tmp_path / "u" / "images") if f.endswith(".jpg")]
    kinds = set()
    for i, f in enumerate(listing):
        image, mask = _decode(str(tmp_path / "u" / "images" / f)), _decode(str(tmp_path / "u" / "masks" / (f[:-4] + ".png")), 1)
        key = f"42|val|{f}"
        rng, np_rng = random.Random(key), np.random.RandomState(zlib.crc32(key.encode()))
        h, w = image.shape[:2]
        for j in range(2):
            size = int(np_rng.randint(256, min(512, max(h, w))))
            rect = None
            if h >= size and w >= size:
                x = rng.randint(0, w - size)
                rect = (x, rng.randint(0, h - size), size, size)
            kinds.add(rect is None)
            name = f"{f[:-4]}_{i}_{j}.png"
            assert np.array_equal(_png(str(tmp_path / "u" / "val" / "images" / name)), pc.resize(image, 256, 256, pc.LINEAR, 0, rect)), name
            assert np.array_equal(_png(str(tmp_path / "u" / "val" / "masks" / name), 1), pc.resize(mask, 256, 256, pc.NEAREST, 0, rect)), name
    assert kinds == {True, False}


# ---- buffer and stream contract -------------------------------------------------------------------
def _resize_case(prep, c, dw):
    srcs, rects = _linear_sources(c)
    buf, offs = _pack(srcs, 1)
    items = prep.items_to_device([prep.make_item(o, a.shape[0], a.shape[1], 16, dw, r) for a, o, r in zip(srcs, offs, rects)], "cpu")
    want = np.stack([pc.resize(a, 16, dw, pc.LINEAR, 0, r) for a, r in zip(srcs, rects)])
    return torch.from_numpy(buf), items, len(srcs), want


@pytest.mark.parametrize("c,dw", [(1, 24), (3, 18)])
def test_resize_buffer_contract(prep, c, dw):
    """guard bands intact, inputs unchanged, every output byte written whatever it held (tests/arena.py)"""
    from arena import Arena
    from inconsistencymasks_amd._lib import lib
    src, items, n, want = _resize_case(prep, c, dw)
    ar = Arena([("src", src, "in"), ("items", items, "in"), ("out", n * 16 * dw * c, "out")], "cuda")
    stream = torch.cuda.current_stream().cuda_stream
    first = ar.check(lambda p: lib.imk_prep_resize(p["src"], src.numel(), p["items"], n, c, 16, dw, 0, 0, p["out"], stream))
    assert np.array_equal(first["out"].cpu().numpy().reshape(want.shape), want)


@pytest.mark.parametrize("c,cw", [(1, 16), (3, 13)])
def test_crops_buffer_contract(prep, c, cw):
    from arena import Arena
    from inconsistencymasks_amd._lib import lib
    a = pc.noise(8, 40, 56, c)
    pos = torch.tensor(POSITIONS, dtype=torch.int32)
    ar = Arena([("src", torch.from_numpy(a), "in"), ("pos", pos, "in"), ("out", len(POSITIONS) * 15 * cw, "out")], "cuda")
    stream = torch.cuda.current_stream().cuda_stream
    first = ar.check(lambda p: lib.imk_prep_crops(p["src"], 40, 56, c, p["pos"], len(POSITIONS), 15, cw, 1, None, 0, p["out"], stream))
    assert np.array_equal(first["out"].cpu().numpy().reshape(-1, 15, cw), pc.crops(pc.gray_thresh(a), POSITIONS, 15, cw))


@pytest.mark.parametrize("fill", [0xFF, 0x3C])
def test_stream_contract(prep, fill):
    """both entry points on a non-default stream whose predecessor is held back: the inputs arrive behind the hold, the outputs hold
    poison until then (tests/stream_skew.py)"""
    import stream_skew as sk
    src, items, n, want = _resize_case(prep, 3, 18)
    a = pc.noise(8, 40, 56, 3)
    dev = lambda t: (torch.empty_like(t, device="cuda"), t.cuda())
    inputs = {"src": dev(src), "items": dev(items), "img": dev(torch.from_numpy(a)), "pos": dev(torch.tensor(POSITIONS, dtype=torch.int32))}
    out_r = torch.empty((n, 16, 18, 3), dtype=torch.uint8, device="cuda")
    out_c = torch.empty((len(POSITIONS), 16, 16), dtype=torch.uint8, device="cuda")
    calls = [lambda: prep.prep_resize(inputs["src"][0], inputs["items"][0], 3, 16, 18, pc.LINEAR, 0, out_r),
             lambda: prep.prep_crops(inputs["img"][0], inputs["pos"][0], 16, 16, pc.GRAY, None, False, out_c)]
    s = torch.cuda.Stream()
    for buf, pristine in inputs.values():      # one undisturbed run first: the kernels' code is loaded before a hold is timed
        buf.copy_(pristine)
    for f in calls:
        f()
    torch.cuda.synchronize()
    snaps = sk.run_skewed(calls, inputs, {"resize": out_r, "crops": out_c}, [], ("main",), s, fill)
    assert np.array_equal(snaps["resize"].cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(snaps["crops"].cpu().numpy().reshape(out_c.shape), pc.crops(pc.gray(a), POSITIONS, 16, 16))


# ---- the nine scripts end to end ------------------------------------------------------------------
CONFIG = """[DEFAULT]
SEED = 42
NUM_EPOCHS = 2
BATCH_SIZE = 8
LR = 0.003
WD = 1e-4
THRESHOLD = 0.5
TOP_Ks = 2

[ISIC_2018]
IMAGE_HEIGHT = 64
IMAGE_WIDTH = 64
IMAGE_CHANNELS = 3
NUM_CLASSES = 1
BASE_DIR = {base}/ISIC_2018/
ALPHA = 0.5
ACTIFU = relu
ACTIFU_OUTPUT = sigmoid
ERODE_KERNEL = 0
DILATE_KERNEL = 0
BLOCK_INPUT = True
BLOCK_OUTPUT = True

[CITYSCAPES]
BASE_DIR = {base}/Cityscapes/
RESIZE_FACTOR = 0.2

[HELA]
BASE_DIR = {base}/HeLa/
USE_MOD_POS_SIZE = True

[SUIM]
BASE_DIR = {base}/SUIM/
"""
RUNNER = "import runpy, sys\nfor s in sys.argv[1:]:\n    runpy.run_path(s, run_name='__main__')\n"
SCRIPTS = ["ISIC_2018/00_ISIC_2018_preprocess_images.py", "ISIC_2018/01_ISIC_2018_split_original_train.py",
           "Cityscapes/00_Cityscapes_resize_images_and_masks.py", "Cityscapes/01_Cityscapes_split_original_train_val.py",
           "HeLa/00_HeLa_create_crops.py", "HeLa/01_HeLa_split_train_in_labeled_and_unlabeled.py",
           "SUIM/00_SUIM_convert_bmp_to_png_masks.py", "SUIM/01_SUIM_split_original_train_val.py", "SUIM/02_SUIM_create_crops.py"]
ENV = {"IM_PREP_HELA_CROP": "48", "IM_PREP_SUIM_CROP": "32,24,48", "IM_RUNIDS": "1", "IM_CANDIDATES": "0"}
ISIC_SPLITS = (("Training", "train_full", 40), ("Validation", "val", 4), ("Test", "test", 4))
SIZES = [(64, 96), (40, 56), (30, 30), (20, 26), (61, 47)]


def _blob(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - rng.integers(h // 3, 2 * h // 3)) ** 2 + (xx - rng.integers(w // 3, 2 * w // 3)) ** 2) < (min(h, w) // 4) ** 2


def _make_trees(base):
    from PIL import Image
    rng = np.random.default_rng(0)
    save = lambda a, path, **kw: (os.makedirs(os.path.dirname(path), exist_ok=True), Image.fromarray(a).save(path, **kw))
    # ISIC: ragged JPEGs (one with an EXIF orientation), `_segmentation.png` masks, a text file in every folder
    org = os.path.join(base, "ISIC_2018", "original_data")
    k = 0
    for folder, _, n in ISIC_SPLITS:
        for i in range(n):
            h, w = SIZES[k % len(SIZES)]
            ell = _blob(rng, h, w)
            img = (170 + rng.integers(-10, 10, (h, w, 3)) - ell[..., None] * 90).clip(0, 255).astype(np.uint8)
            kw = {}
            if k == 1:
                exif = Image.Exif()
                exif[0x0112] = 6
                kw = {"exif": exif}
            save(img, os.path.join(org, f"ISIC2018_Task1-2_{folder}_Input", f"ISIC_{k:07d}.jpg"), quality=95, **kw)
            save((ell * 255).astype(np.uint8), os.path.join(org, f"ISIC2018_Task1_{folder}_GroundTruth", f"ISIC_{k:07d}_segmentation.png"))
            k += 1
        for d, name in ((f"ISIC2018_Task1-2_{folder}_Input", "ATTRIBUTION.txt"), (f"ISIC2018_Task1_{folder}_GroundTruth", "LICENSE.txt")):
            with open(os.path.join(org, d, name), "w") as f:
                f.write("not an image\n")
    # Cityscapes: two cities per split, one image without its label file, two sizes
    org = os.path.join(base, "Cityscapes", "original_data")
    for split, cities in (("train", (("aachen", 6), ("bochum", 4))), ("val", (("lindau", 2), ("munster", 2)))):
        for city, n in cities:
            for i in range(n):
                h, w = (64, 96) if i % 2 == 0 else (48, 80)
                common = f"{city}_{i:06d}_000019"
                save(pc.noise(100 + i, h, w, 3), os.path.join(org, "leftImg8bit", split, city, common + "_leftImg8bit.png"))
                lab = np.array([0, 1, 7, 33, 254, 255], np.uint8)[rng.integers(0, 6, (h // 8, w // 8))].repeat(8, 0).repeat(8, 1)
                save(lab, os.path.join(org, "gtFine", split, city, common + "_gtFine_labelIds.png"))
                save(lab, os.path.join(org, "gtFine", split, city, common + "_gtFine_color.png"))
    save(pc.noise(1, 64, 96, 3), os.path.join(org, "leftImg8bit", "train", "aachen", "aachen_000099_000019_leftImg8bit.png"))
    # HeLa: grey PNG channels, one colour brightfield, one image without its `dead` file
    org = os.path.join(base, "HeLa", "original_data")
    for data_set, n in (("train_full", 3), ("val", 1), ("test", 1)):
        for i in range(n):
            name = f"{data_set}_{i:03d}.png"
            bf = pc.noise(200 + i, 64, 96, 3) if (data_set, i) == ("train_full", 1) else pc.noise(200 + i, 64, 96)
            save(bf, os.path.join(org, data_set, "brightfield", name))
            for ch_i, channel in enumerate(("alive", "dead", "mod_position")):
                if channel == "dead" and (data_set, i) == ("train_full", 2):
                    continue
                m = np.array([0, 9, 10, 11, 255], np.uint8)[rng.integers(0, 5, (16, 24))].repeat(4, 0).repeat(4, 1)
                save(m, os.path.join(org, data_set, channel, name))
    # SUIM: JPEG images of several sizes with colour BMP masks (pure colours and values on both sides of 128)
    org = os.path.join(base, "SUIM", "original_data")
    for folder, n in (("train_val", 12), ("TEST", 3)):
        for i in range(n):
            h, w = SIZES[i % len(SIZES)]
            stem = f"{'d' if folder == 'TEST' else 'f'}_r_{i:03d}_"
            save(pc.noise(300 + i, h // 4 + 1, w // 4 + 1, 3).repeat(4, 0).repeat(4, 1)[:h, :w].copy(), os.path.join(org, folder, "images", stem + ".jpg"),
                 quality=90)
            m = np.array([0, 120, 130, 255], np.uint8)[rng.integers(0, 4, (h // 4 + 1, w // 4 + 1, 3))].repeat(4, 0).repeat(4, 1)[:h, :w].copy()
            save(m, os.path.join(org, folder, "masks", stem + ".bmp"))


def _run(work, cmd, extra=None):
    env = {**os.environ, "IM_CONFIG": os.path.join(work, "config.ini"), **ENV, **(extra or {})}
    r = subprocess.run(cmd, env=env, cwd=work, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    """the toy raw trees of the four datasets, prepared by the nine scripts in one child process"""
    work = str(tmp_path_factory.mktemp("prep"))
    base = os.path.join(work, "data")
    with open(os.path.join(work, "config.ini"), "w") as f:
        f.write(CONFIG.format(base=base))
    with open(os.path.join(work, "runner.py"), "w") as f:
        f.write(RUNNER)
    _make_trees(base)
    raw = os.path.join(work, "raw_isic")
    shutil.copytree(os.path.join(base, "ISIC_2018", "original_data"), os.path.join(raw, "ISIC_2018", "original_data"))
    out = _run(work, [sys.executable, "runner.py"] + [os.path.join(ROOT, s) for s in SCRIPTS])
    return work, base, out


def _decode(path, channels=3):
    """the source as Pillow decodes it (EXIF orientation applied), RGB or grey"""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        a = np.asarray(ImageOps.exif_transpose(im).convert("RGB" if channels == 3 else "L"), np.uint8)
    return a


def _png(path, channels=3):
    from PIL import Image
    with Image.open(path) as im:
        want_mode = "RGB" if channels == 3 else "L"
        assert im.mode == want_mode, (path, im.mode)
        return np.asarray(im, np.uint8)


def test_scripts_isic(prepared):
    work, base, out = prepared
    org, dst = os.path.join(base, "ISIC_2018", "original_data"), os.path.join(base, "ISIC_2018")
    for folder, split, n in ISIC_SPLITS:
        src_i, src_m = os.path.join(org, f"ISIC2018_Task1-2_{folder}_Input"), os.path.join(org, f"ISIC2018_Task1_{folder}_GroundTruth")
        stems = sorted(f[:-4] for f in os.listdir(src_i) if f.endswith(".jpg"))
        assert len(stems) == n
        assert sorted(os.listdir(os.path.join(dst, split, "images"))) == [s + ".png" for s in stems]      # the text files are skipped
        assert sorted(os.listdir(os.path.join(dst, split, "masks"))) == [s + ".png" for s in stems]       # `_segmentation` dropped
        for s in stems:
            a = _decode(os.path.join(src_i, s + ".jpg"))
            assert np.array_equal(_png(os.path.join(dst, split, "images", s + ".png")), pc.resize_linear(a, 64, 64)), s
            m = _decode(os.path.join(src_m, s + "_segmentation.png"))
            assert np.array_equal(_png(os.path.join(dst, split, "masks", s + ".png")), pc.resize_linear(m, 64, 64)), s      # linear, 3 channels
    assert _decode(os.path.join(org, "ISIC2018_Task1-2_Training_Input", "ISIC_0000001.jpg")).shape == (56, 40, 3)          # EXIF 6: turned
    assert "ATTRIBUTION.txt" in out and "LICENSE.txt" in out                                                                # reported
    # 01: the split of the listing as it is, 3-channel rewrites of the same pixels
    listing = os.listdir(os.path.join(dst, "train_full", "images"))
    lab, unl = pc.split(listing, 0.9, 42)
    for split, names in (("train_labeled", lab), ("train_unlabeled", unl)):
        for sub in ("images", "masks"):
            assert sorted(os.listdir(os.path.join(dst, split, sub))) == sorted(names)
            for nm in names:
                assert np.array_equal(_png(os.path.join(dst, split, sub, nm)), _png(os.path.join(dst, "train_full", sub, nm)))
    assert len(lab) == 4 and len(unl) == 36


def test_scripts_cityscapes(prepared):
    work, base, out = prepared
    org, dst = os.path.join(base, "Cityscapes", "original_data"), os.path.join(base, "Cityscapes")
    for split, out_i, out_m, n in (("train", os.path.join(dst, "train_full", "images"), os.path.join(dst, "train_full", "masks"), 10),
                                   ("val", os.path.join(org, "val_test", "images"), os.path.join(org, "val_test", "masks"), 4)):
        want = {}
        for city in os.listdir(os.path.join(org, "leftImg8bit", split)):
            for f in os.listdir(os.path.join(org, "leftImg8bit", split, city)):
                common = "_".join(f.split("_")[:-1])
                mask = os.path.join(org, "gtFine", split, city, common + "_gtFine_labelIds.png")
                if os.path.exists(mask):
                    want[common + ".png"] = (os.path.join(org, "leftImg8bit", split, city, f), mask)
        assert len(want) == n and "aachen_000099_000019.png" not in want                      # the image without labels is skipped
        assert sorted(os.listdir(out_i)) == sorted(want) == sorted(os.listdir(out_m))
        for name, (ip, mp) in want.items():
            a, m = _decode(ip), _decode(mp)
            dh, dw = pc.cityscapes_size(a.shape[0], a.shape[1], 0.2)
            assert (dh, dw) == ((16, 32) if a.shape[0] == 64 else (16, 16))
            assert np.array_equal(_png(os.path.join(out_i, name)), pc.resize(a, dh, dw, pc.LINEAR)), name
            assert np.array_equal(_png(os.path.join(out_m, name)), pc.resize(m, dh, dw, pc.NEAREST, pc.LABEL_PLUS1)), name
    for src_i, src_m, parts, ratio in ((os.path.join(dst, "train_full", "images"), os.path.join(dst, "train_full", "masks"),
                                        ("train_labeled", "train_unlabeled"), 0.9),
                                       (os.path.join(org, "val_test", "images"), os.path.join(org, "val_test", "masks"), ("val", "test"), 0.5)):
        a, b = pc.split(os.listdir(src_i), ratio, 42)
        for split, names in zip(parts, (a, b)):
            assert sorted(os.listdir(os.path.join(dst, split, "images"))) == sorted(names) == sorted(os.listdir(os.path.join(dst, split, "masks")))
            for nm in names:
                assert np.array_equal(_png(os.path.join(dst, split, "images", nm)), _png(os.path.join(src_i, nm)))
                assert np.array_equal(_png(os.path.join(dst, split, "masks", nm)), _png(os.path.join(src_m, nm)))


def test_scripts_hela(prepared):
    work, base, out = prepared
    org, dst = os.path.join(base, "HeLa", "original_data"), os.path.join(base, "HeLa")
    positions = pc.get_positions(64, 96, 48, 0.6)
    assert len(positions) == 15
    for data_set in ("train_full", "val", "test"):
        for name in os.listdir(os.path.join(org, data_set, "brightfield")):
            for channel in ("brightfield", "alive", "dead", "mod_position"):
                src = os.path.join(org, data_set, channel, name)
                outs = [os.path.join(dst, data_set, channel, f"{name[:-4]}_{k}.png") for k in range(len(positions))]
                if not os.path.exists(src):
                    assert channel == "dead" and not any(os.path.exists(o) for o in outs)      # a missing channel is skipped
                    continue
                a = _decode(src)
                plane = pc.gray(a) if channel == "brightfield" else pc.gray_thresh(a)
                for o, (x, y) in zip(outs, positions):
                    assert np.array_equal(_png(o, 1), plane[y:y + 48, x:x + 48]), o
        assert len(os.listdir(os.path.join(dst, data_set, "brightfield"))) == 15 * len(os.listdir(os.path.join(org, data_set, "brightfield")))
    names = os.listdir(os.path.join(dst, "train_full", "brightfield"))
    random.Random(42).shuffle(names)
    lab, unl = names[:int(len(names) * 0.10)], names[int(len(names) * 0.10):]
    assert len(lab) == 4
    for split, part in (("train_labeled", lab), ("train_unlabeled", unl)):
        for channel in ("brightfield", "alive", "dead", "mod_position"):
            have = [n for n in part if os.path.exists(os.path.join(dst, "train_full", channel, n))]
            assert sorted(os.listdir(os.path.join(dst, split, channel))) == sorted(have)
            for n in have:
                assert open(os.path.join(dst, split, channel, n), "rb").read() == open(os.path.join(dst, "train_full", channel, n), "rb").read()


def test_scripts_suim(prepared):
    work, base, out = prepared
    org = os.path.join(base, "SUIM", "original_data")
    table = pc.class_table({(255 * (k >> 2 & 1), 255 * (k >> 1 & 1), 255 * (k & 1)): k + 1 for k in range(8)})
    for folder in ("train_val", "TEST"):
        bmps = [f for f in os.listdir(os.path.join(org, folder, "masks")) if f.endswith(".bmp")]
        assert sorted(os.listdir(os.path.join(org, folder, "masks_png"))) == sorted(f[:-4] + ".png" for f in bmps)
        for f in bmps:
            assert np.array_equal(_png(os.path.join(org, folder, "masks_png", f[:-4] + ".png"), 1),
                                  pc.class8(_decode(os.path.join(org, folder, "masks", f)), table)), f
    # 01: two splits of the listing's stems; the JPEG bytes are copied, the masks rewritten with 3 channels
    for src, parts in (("train_val", ("train_full", "val")), ("train_full", ("train_unlabeled", "train_labeled"))):
        src_m = os.path.join(org, src, "masks_png" if src == "train_val" else "masks")
        stems = [os.path.splitext(f)[0] for f in os.listdir(os.path.join(org, src, "images"))]
        a, b = pc.split(stems, 0.1, 42)
        for split, part in zip(parts, (a, b)):
            assert sorted(os.listdir(os.path.join(org, split, "images"))) == sorted(s + ".jpg" for s in part)
            assert sorted(os.listdir(os.path.join(org, split, "masks"))) == sorted(s + ".png" for s in part)
            for s in part:
                assert open(os.path.join(org, split, "images", s + ".jpg"), "rb").read() == open(os.path.join(org, src, "images", s + ".jpg"), "rb").read()
                assert np.array_equal(_png(os.path.join(org, split, "masks", s + ".png")), _decode(os.path.join(src_m, s + ".png")))
    # 02: two crops per image, drawn per file from (SEED, output directory, file name)
    took_crop = took_whole = 0
    for split, mask_sub in (("train_full", "masks"), ("train_labeled", "masks"), ("train_unlabeled", "masks"), ("val", "masks"), ("TEST", "masks_png")):
        out_dir = os.path.join(base, "SUIM", split.lower())
        files = [f for f in os.listdir(os.path.join(org, split, "images")) if f.endswith(".jpg")]
        want = [f"{f[:-4]}_{i}_{j}.png" for i, f in enumerate(files) for j in range(2)]
        assert sorted(os.listdir(os.path.join(out_dir, "images"))) == sorted(want) == sorted(os.listdir(os.path.join(out_dir, "masks")))
        for i, f in enumerate(files):
            img, mask = _decode(os.path.join(org, split, "images", f)), _decode(os.path.join(org, split, mask_sub, f[:-4] + ".png"), 1)
            key = f"42|{split.lower()}|{f}"
            rng, np_rng = random.Random(key), np.random.RandomState(zlib.crc32(key.encode()))
            h, w = img.shape[:2]
            for j in range(2):
                size = int(np_rng.randint(24, min(48, max(h, w))))
                rect = None
                if h >= size and w >= size:
                    x = rng.randint(0, w - size)
                    rect = (x, rng.randint(0, h - size), size, size)
                took_crop, took_whole = took_crop + (rect is not None), took_whole + (rect is None)
                name = f"{f[:-4]}_{i}_{j}.png"
                assert np.array_equal(_png(os.path.join(out_dir, "images", name)), pc.resize(img, 32, 32, pc.LINEAR, 0, rect)), name
                assert np.array_equal(_png(os.path.join(out_dir, "masks", name), 1), pc.resize(mask, 32, 32, pc.NEAREST, 0, rect)), name
    assert took_crop and took_whole


def test_prepared_isic_tree_trains_a_subset_candidate(prepared):
    """the prepared ISIC tree is what the drivers read: one candidate of ISIC_2018/03_ISIC_2018_subset.py on it"""
    work, base, out = prepared
    _run(work, [sys.executable, os.path.join(ROOT, "ISIC_2018", "03_ISIC_2018_subset.py")])
    assert "ISIC_2018_subset_1_topK_1.h5" in os.listdir(os.path.join(base, "ISIC_2018", "models"))
    rows = open(os.path.join(base, "ISIC_2018", "csv", "results_ISIC_2018_subset_1.csv")).read().strip().splitlines()
    assert len(rows) == 2 and all(0.0 <= float(v) <= 1.0 for v in rows[1].split(";")[1:])


def test_isic_00_two_ranks_write_the_same_files(prepared):
    work, base, out = prepared
    two = os.path.join(work, "two")
    os.makedirs(two)
    shutil.copytree(os.path.join(work, "raw_isic"), os.path.join(two, "data"))
    with open(os.path.join(two, "config.ini"), "w") as f:
        f.write(CONFIG.format(base=os.path.join(two, "data")))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    _run(two, [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, SCRIPTS[0])], {"IMK_DIST_BACKEND": "gloo", "IMK_ONE_GPU": "1"})
    for _, split, n in ISIC_SPLITS:
        for sub in ("images", "masks"):
            a, b = os.path.join(base, "ISIC_2018", split, sub), os.path.join(two, "data", "ISIC_2018", split, sub)
            assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(b)) == n
            for nm in os.listdir(a):
                assert np.array_equal(_png(os.path.join(a, nm)), _png(os.path.join(b, nm))), (split, sub, nm)
