"""The model-ensemble baseline on the GPU: imk_vote_* against the reference's outputs (tests/golden/model_ensemble.npz), the functions
of record with `.predict` fakes, imk_unet_forward_vote bit-identical to imk_unet_forward x N + imk_vote_*, the hard votes against
imk_unet_forward_im's label maps, the writers, and toy runs of the four model-ensemble scripts (functions.py:1864-1990, 2409-2566;
ISIC_2018/06_ISIC_2018_model_ensemble.py, HeLa/06_HeLa_model_ensemble.py, SUIM/07_SUIM_model_ensemble.py,
Cityscapes/06_Cityscapes_model_ensemble.py)."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

from inconsistencymasks_amd import functions as F  # noqa: E402
from inconsistencymasks_amd import vote as V  # noqa: E402
from inconsistencymasks_amd._lib import check, lib  # noqa: E402
from inconsistencymasks_amd.unet import UNet  # noqa: E402

F32 = np.float32


def gold():
    with np.load(os.path.join(GOLD, "model_ensemble.npz")) as d:
        return {k: d[k] for k in d.files}


def cases(d, kind):
    return sorted({k.split("_")[0] for k in d if k.startswith(kind) and k[len(kind)].isdigit()})


class Fixed:
    def __init__(self, arr):
        self.arr = arr

    def predict(self, x):
        return self.arr


# ---- 1. the vote kernels against the reference ---------------------------------------------------------------------------------
def test_vote_kernels_match_the_reference_bit_exactly():
    d = gold()
    for c in cases(d, "bin"):
        got = V.vote_binary(torch.from_numpy(d[c + "_preds"]).cuda(), float(d[c + "_thr"]), soft=False)[0, 0].cpu().numpy()
        assert np.array_equal(got.astype(np.float64), d[c + "_out"]), c
    for c in cases(d, "hela"):
        got = V.vote_binary(torch.from_numpy(d[c + "_preds"]).cuda(), float(d[c + "_thr"]), soft=True)[0].cpu().numpy()
        for j, key in enumerate(("alive", "dead", "pos")):
            assert np.array_equal(got[j], d[f"{c}_{key}"]), (c, key)
    for c in cases(d, "mc"):
        p = torch.from_numpy(d[c + "_probs"]).cuda()
        assert np.array_equal(V.vote_multiclass(p, soft=True)[0].cpu().numpy(), d[c + "_soft"]), c
        assert np.array_equal(V.vote_multiclass(p, soft=False)[0].cpu().numpy(), d[c + "_hard"]), c


# ---- 2. the functions of record with .predict fakes -----------------------------------------------------------------------------
def test_functions_of_record_with_predict_fakes():
    d = gold()
    for c in cases(d, "bin"):
        preds = d[c + "_preds"]
        n, _, h, w, _ = preds.shape
        out = F.get_model_ensemble_prediction_ISIC_2018([Fixed(preds[j]) for j in range(n)], np.zeros((1, h, w, 3), np.uint8), h, w,
                                                        float(d[c + "_thr"]))
        assert out.dtype == np.float64 and out.shape == (h, w) and np.array_equal(out, d[c + "_out"]), c
    for c in cases(d, "hela"):
        preds = d[c + "_preds"]
        n, _, h, w, _ = preds.shape
        r = F.get_model_ensemble_prediction_hela_soft([Fixed(preds[j]) for j in range(n)], np.zeros((1, h, w, 1), np.uint8),
                                                      float(d[c + "_thr"]))
        assert isinstance(r, tuple) and len(r) == 3
        alive, dead, pos = r
        assert alive.dtype == dead.dtype == pos.dtype == np.uint8 and alive.shape == dead.shape == (h, w) and pos.shape == (h, w, 3)
        assert np.array_equal(alive, d[c + "_alive"]) and np.array_equal(dead, d[c + "_dead"]), c
        want = np.repeat(F._redraw_positions(d[c + "_pos"], 8, 3, 99, 0)[..., None], 3, 2)
        assert np.array_equal(pos, want), c
    for c in cases(d, "mc"):
        probs = d[c + "_probs"]
        n, _, h, w, _ = probs.shape
        models = [Fixed(probs[j]) for j in range(n)]
        x = np.zeros((1, h, w, 3), np.uint8)
        for fn, key in ((F.get_model_ensemble_prediction_multiclass_soft, "_soft"), (F.get_model_ensemble_prediction_multiclass_hard, "_hard")):
            out = fn(models, x)
            assert out.dtype == np.uint8 and out.shape == (h, w) and np.array_equal(out, d[c + key]), (c, key)


# ---- 3. the fused forward + vote against forward x N + vote -----------------------------------------------------------------------
def _models(cfg, n, seed=0):
    h, w, c, k, alpha, act = cfg
    ms = [UNet(h, w, c, k, alpha, act, seed=seed + 11 * j) for j in range(n)]
    g = torch.Generator().manual_seed(seed)
    for m in ms:      # non-trivial BatchNorm statistics: the moving mean / variance of every BN layer perturbed
        sd = m.state_dict()
        for name, t in sd.items():
            if name.endswith(".mean"):
                sd[name] = t + 0.1 * torch.randn(t.shape, generator=g)
            elif name.endswith(".var"):
                sd[name] = t * (0.5 + torch.rand(t.shape, generator=g))
        m.load_state_dict(sd)
    return ms


def _forward_vote(models, x, thr, soft, n_streams, out=None):
    p = models[0].plan
    n, b = len(models), x.shape[0]
    for m in models:
        m.ready_for_inference()
    nbytes = lib.imk_unet_forward_im_workspace_bytes(p.ptr, n, b, n_streams)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
    params = (ctypes.c_void_p * n)(*[m.params.data_ptr() for m in models])
    packed = (ctypes.c_void_p * n)(*[m.packed.data_ptr() for m in models])
    shape = (b, p.n_out, p.h, p.w) if p.act_out == "sigmoid" else (b, p.h, p.w)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device="cuda")
    check(lib.imk_unet_forward_vote(p.ptr, n, params, packed, x.data_ptr(), b, float(thr), int(soft), out.data_ptr(), ws.data_ptr(),
                                    ws.numel(), torch.cuda.current_stream().cuda_stream), "imk_unet_forward_vote")
    return out


def _unfused(models, x, thr, soft):
    probs = torch.stack([m.predict_device(x) for m in models], 0).contiguous()
    if models[0].plan.act_out == "sigmoid":
        return V.vote_binary(probs, thr, soft)
    return V.vote_multiclass(probs, soft)


ISIC, HELA, SUIM = (256, 256, 3, 1, 0.5, "sigmoid"), (256, 256, 1, 3, 1.0, "sigmoid"), (256, 256, 3, 9, 1.0, "softmax")
CITY1, CITY2 = (208, 416, 3, 35, 1.0, "softmax"), (208, 416, 3, 35, 2.0, "softmax")
# 48 x 80: H*W = 3840 is not a multiple of the sigmoid kernel's 1024-pixel chunk nor of the softmax kernels' chunks (the short last chunk)
ISIC_T, HELA_T, SUIM_T = (48, 80, 3, 1, 0.5, "sigmoid"), (48, 80, 1, 3, 1.0, "sigmoid"), (48, 80, 3, 9, 1.0, "softmax")
FUSED_CASES = [(ISIC_T, 2, 2, 3), (HELA_T, 3, 3, 2), (SUIM_T, 3, 2, 3), (ISIC, 2, 1, 5), (ISIC, 3, 3, 7), (ISIC, 8, 2, 3), (HELA, 2, 2, 5), (HELA, 3, 1, 3), (HELA, 8, 3, 2),
               (SUIM, 2, 2, 5), (SUIM, 3, 3, 3), (SUIM, 8, 1, 2), (CITY1, 2, 2, 5), (CITY1, 3, 1, 3), (CITY2, 2, 3, 3), (CITY2, 8, 2, 2)]


@pytest.mark.parametrize("cfg,n,k,b", FUSED_CASES, ids=[f"{c[3]}-a{c[4]}-n{n}-s{k}-b{b}" for c, n, k, b in FUSED_CASES])
def test_forward_vote_is_bit_identical_to_forward_plus_vote(cfg, n, k, b):
    models = _models(cfg, n, seed=100 * n + k)
    rng = np.random.default_rng(n * 7 + b)
    x = torch.from_numpy(rng.integers(0, 256, (b, cfg[0], cfg[1], cfg[2])).astype(np.uint8)).cuda()
    for soft in (False, True):
        want = _unfused(models, x, 0.5, soft)
        got = _forward_vote(models, x, 0.5, soft, k)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (soft, int((got != want).sum()))


def test_forward_vote_fallback_route_and_ensemble_class():
    """the materialize debug switch forces the unfused route (probability stack + imk_vote_*): the same labels as imk_unet_forward x N
    + imk_vote_* under the same switch; EnsembleVote / StackVote give the same labels as each other"""
    for cfg in (HELA, SUIM):
        models = _models(cfg, 3, seed=5)
        x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (3, cfg[0], cfg[1], cfg[2])).astype(np.uint8)).cuda()
        binary = cfg[5] == "sigmoid"
        for s in (False, True):
            assert torch.equal(V.EnsembleVote(models).run(x, 0.5, s), V.StackVote(models, binary).run(x, 0.5, s))
        for m in models:
            m.debug(materialize=True)
        try:
            for s in (False, True):
                assert torch.equal(_forward_vote(models, x, 0.5, s, 3), _unfused(models, x, 0.5, s))
        finally:
            for m in models:
                m.debug(materialize=False)


# ---- 4. hard votes = imk_unet_forward_im's label map with blocking off ------------------------------------------------------------
@pytest.mark.parametrize("cfg", [ISIC, HELA, SUIM, CITY1], ids=["isic", "hela", "suim", "city"])
def test_hard_vote_equals_the_im_label_map(cfg):
    models = _models(cfg, 2, seed=9)
    x = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (3, cfg[0], cfg[1], cfg[2])).astype(np.uint8)).cuda()
    r = F.EnsembleIM(models).run(x, 0.5, False, False, False)
    got = _forward_vote(models, x, 0.5, False, 2)
    want = r["masks"] if cfg[5] == "sigmoid" else r["masks"][:, 0]
    assert torch.equal(got, want)


# ---- 5. writers ---------------------------------------------------------------------------------------------------------------------
def _toy_images(d, n, h, w, c, seed):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    for i in range(n):
        F.write_png(os.path.join(d, f"img_{i:03d}.png"), rng.integers(0, 256, (h, w, c) if c == 3 else (h, w)).astype(np.uint8))


class Lookup:
    """fake model: the prediction looked up by the content of the [1,H,W,C] batch it is given"""

    def __init__(self, table):
        self.table = table

    def predict(self, x):
        return self.table[hashlib.sha1(np.ascontiguousarray(x[0]).tobytes()).hexdigest()]


def _seq_mean(p):
    s = p[0].copy()
    for q in p[1:]:
        s = (s + q).astype(F32)
    return (s / F32(len(p))).astype(F32)


@pytest.mark.parametrize("native", [True, False], ids=["unet", "lookup"])
@pytest.mark.parametrize("rgb", [True, False], ids=["rgb", "file-order"])
def test_isic_and_multiclass_writers(tmp_path, native, rgb):
    h = w = 64
    src = str(tmp_path / "src")
    _toy_images(src, 7, h, w, 3, 3)
    names = sorted(os.listdir(src))
    files = {n: F.read_png(os.path.join(src, n), 3) for n in names}
    for cfg, binary in (((h, w, 3, 1, 0.5, "sigmoid"), True), ((h, w, 3, 4, 0.5, "softmax"), False)):
        units = _models(cfg, 3, seed=21)
        preds = {}
        for nme, img in files.items():       # what every model predicts for the image the nets see
            xin = img if rgb else img[..., ::-1]
            xt = torch.from_numpy(np.ascontiguousarray(xin)[None]).cuda()
            preds[nme] = [m.predict_device(xt).cpu().numpy() for m in units]
        if native:
            models = units
        else:
            tabs = [{} for _ in units]
            for nme, img in files.items():
                xin = np.ascontiguousarray((img if rgb else img[..., ::-1])[None])
                for j in range(len(units)):
                    tabs[j][hashlib.sha1(xin[0].tobytes()).hexdigest()] = preds[nme][j]
            models = [Lookup(t) for t in tabs]
        out = tmp_path / ("isic" if binary else "multi") / ("n" if native else "l")
        if binary:
            F.create_pseudo_labels_model_ensemble_ISIC_2018(models, src, str(out), h, w, 3, rgb)
        else:
            F.create_pseudo_labels_model_ensemble_multiclass(models, src, str(out), h, w, 3, rgb)
        assert sorted(os.listdir(out)) == ["images", "masks"]
        for nme in names:
            assert sorted(os.listdir(out / "images")) == names and sorted(os.listdir(out / "masks")) == names
            assert np.array_equal(F.read_png(str(out / "images" / nme), 3), files[nme])
            p = np.stack(preds[nme])[:, 0]
            want = np.where(np.all(p[..., 0] > F32(0.5), 0), 255, 0) if binary else np.argmax(_seq_mean(p), -1)
            assert np.array_equal(F.read_png(str(out / "masks" / nme), 1)[..., 0], want.astype(np.uint8)), nme


@pytest.mark.parametrize("native", [True, False], ids=["unet", "lookup"])
def test_hela_writer(tmp_path, native):
    from PIL import Image
    h = w = 64
    src = str(tmp_path / "bf")
    _toy_images(src, 5, h, w, 1, 4)
    names = sorted(os.listdir(src))
    units = _models((h, w, 1, 3, 0.5, "sigmoid"), 2, seed=31)
    files = {n: F.read_png(os.path.join(src, n), 1) for n in names}
    preds = {n: [m.predict_device(torch.from_numpy(img[None]).cuda()).cpu().numpy() for m in units] for n, img in files.items()}
    models = units if native else [Lookup({hashlib.sha1(files[n].tobytes()).hexdigest(): preds[n][j] for n in names}) for j in range(2)]
    out = tmp_path / "out"
    F.create_pseudo_labels_model_ensemble_hela(models, src, str(out), h, w, 1)
    assert sorted(os.listdir(out)) == ["alive", "brightfield", "dead", "mod_position"]
    for nme in names:
        p = np.stack(preds[nme])[:, 0].astype(np.float64)
        on = np.where((p[0] + p[1]) / 2.0 > 0.5, 255, 0).astype(np.uint8)
        assert np.array_equal(F.read_png(str(out / "brightfield" / nme), 1), files[nme])
        assert np.array_equal(F.read_png(str(out / "alive" / nme), 1)[..., 0], on[..., 0])
        assert np.array_equal(F.read_png(str(out / "dead" / nme), 1)[..., 0], on[..., 1])
        with Image.open(out / "mod_position" / nme) as im:
            assert im.mode == "RGB"
            pos = np.asarray(im)
        assert pos.shape == (h, w, 3)
        assert np.array_equal(pos, np.repeat(F._redraw_positions(on[..., 2], 8, 3, 99, 0)[..., None], 3, 2))


# ---- 6 / 7. the four scripts on toy data ----------------------------------------------------------------------------------------
# ---- toy data sets and generation-0 ensembles of the four datasets (the set-up pattern of tests/test_gpu_driver.py) -------------
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
BASE_DIR = {base}/
ALPHA = 0.5
ACTIFU = relu
ACTIFU_OUTPUT = sigmoid
ERODE_KERNEL = 0
DILATE_KERNEL = 0
BLOCK_INPUT = True
BLOCK_OUTPUT = True
"""


SETUP = """
import os, sys
import numpy as np
sys.path.insert(0, {root!r})
from inconsistencymasks_amd import functions as F, paths
from inconsistencymasks_amd.unet import get_unet
rng = np.random.default_rng(0)
def sample(n, d_img, d_mask):
    os.makedirs(d_img, exist_ok=True); os.makedirs(d_mask, exist_ok=True)
    yy, xx = np.mgrid[0:64, 0:64]
    for i in range(n):
        cy, cx, r = rng.integers(20, 44), rng.integers(20, 44), rng.integers(8, 18)
        ell = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        img = (170 + rng.integers(-10, 10, (64, 64, 3)) - ell[..., None] * 90).clip(0, 255).astype(np.uint8)
        F.write_png(os.path.join(d_img, f"ISIC_{{i:05d}}.png"), img)
        F.write_png(os.path.join(d_mask, f"ISIC_{{i:05d}}.png"), (ell * 255).astype(np.uint8))
sample(16, paths.ISIC_2018_TRAIN_LABELED_IMAGES_DIR, paths.ISIC_2018_TRAIN_LABELED_MASKS_DIR)
sample(24, paths.ISIC_2018_TRAIN_UNLABELED_IMAGES_DIR, paths.ISIC_2018_TRAIN_UNLABELED_MASKS_DIR)
sample(8, paths.ISIC_2018_VAL_IMAGES_DIR, paths.ISIC_2018_VAL_MASKS_DIR)
sample(8, paths.ISIC_2018_TEST_IMAGES_DIR, paths.ISIC_2018_TEST_MASKS_DIR)
os.makedirs(paths.ISIC_2018_MODEL_DIR, exist_ok=True)
import torch
x = torch.from_numpy(np.stack([F.read_png(os.path.join(paths.ISIC_2018_TRAIN_LABELED_IMAGES_DIR, n), 3) for n in sorted(os.listdir(paths.ISIC_2018_TRAIN_LABELED_IMAGES_DIR))])).cuda()
y = torch.from_numpy(np.stack([F.read_png(os.path.join(paths.ISIC_2018_TRAIN_LABELED_MASKS_DIR, n), 1) // 255 for n in sorted(os.listdir(paths.ISIC_2018_TRAIN_LABELED_MASKS_DIR))])).cuda()
for j in (1, 2):      # the gen-0 ensemble (03_ISIC_2018_subset.py's product), trained long enough for the BN statistics
    m = get_unet(64, 64, 3, 1, 0.5, "relu", "sigmoid", seed=j)
    for it in range(700):
        m.train_step(x, y, 0, 3e-3 if it < 200 else 0.0, 1e-4 if it < 200 else 0.0)
    m.repack()
    F.save_model(m, os.path.join(paths.ISIC_2018_MODEL_DIR, f"ISIC_2018_subset_1_topK_{{j}}.h5"))
"""


MULTI_CONFIG = """[DEFAULT]
SEED = 42
NUM_EPOCHS = 2
BATCH_SIZE = 8
LR = 0.003
WD = 1e-4
THRESHOLD = 0.5
TOP_Ks = 2

[SUIM]
IMAGE_HEIGHT = 64
IMAGE_WIDTH = 64
IMAGE_CHANNELS = 3
NUM_CLASSES = 3
BASE_DIR = {base}/
ALPHA = 0.5
ACTIFU = relu
ACTIFU_OUTPUT = softmax
ERODE_KERNEL = 0
DILATE_KERNEL = 0
BLOCK_INPUT = True
BLOCK_OUTPUT = True
FILTER_INCONSISTENT_CLASS_PRED = False
FREE_ROTATION = False
NUM_IMAGES_IM_PLUS = 1
"""


MULTI_SETUP = """
import os, sys
import numpy as np
sys.path.insert(0, {root!r})
from inconsistencymasks_amd import functions as F, paths
from inconsistencymasks_amd.unet import get_unet
rng = np.random.default_rng(0)
def sample(n, d_img, d_mask):
    os.makedirs(d_img, exist_ok=True); os.makedirs(d_mask, exist_ok=True)
    yy, xx = np.mgrid[0:64, 0:64]
    for i in range(n):
        cy, cx, r = rng.integers(20, 44), rng.integers(20, 44), rng.integers(8, 16)
        cls = np.zeros((64, 64), np.uint8)
        cls[yy > 40] = 1                                        # "sea floor"
        cls[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 2        # "object"
        img = np.stack([60 + 70 * (cls == 1) + 150 * (cls == 2), 90 + 60 * (cls == 2), 200 - 80 * (cls == 1)], -1)
        img = (img + rng.integers(-10, 10, (64, 64, 3))).clip(0, 255).astype(np.uint8)
        F.write_png(os.path.join(d_img, f"s_{{i:04d}}.png"), img)
        F.write_png(os.path.join(d_mask, f"s_{{i:04d}}.png"), cls)
sample(16, paths.SUIM_TRAIN_LABELED_IMAGES_DIR, paths.SUIM_TRAIN_LABELED_MASKS_DIR)
sample(24, paths.SUIM_TRAIN_UNLABELED_IMAGES_DIR, paths.SUIM_TRAIN_UNLABELED_MASKS_DIR)
sample(8, paths.SUIM_VAL_IMAGES_DIR, paths.SUIM_VAL_MASKS_DIR)
sample(8, paths.SUIM_TEST_IMAGES_DIR, paths.SUIM_TEST_MASKS_DIR)
os.makedirs(paths.SUIM_MODEL_DIR, exist_ok=True)
import torch
names = sorted(os.listdir(paths.SUIM_TRAIN_LABELED_IMAGES_DIR))
x = torch.from_numpy(np.stack([F.read_png(os.path.join(paths.SUIM_TRAIN_LABELED_IMAGES_DIR, n), 3) for n in names])).cuda()
y = torch.from_numpy(np.stack([F.read_png(os.path.join(paths.SUIM_TRAIN_LABELED_MASKS_DIR, n), 1)[..., 0] for n in names])).cuda()
for j in (1, 2):
    m = get_unet(64, 64, 3, 3, 0.5, "relu", "softmax", seed=j)
    for it in range(700):
        m.train_step(x, y, 1, 3e-3 if it < 200 else 0.0, 1e-4 if it < 200 else 0.0)
    m.repack()
    F.save_model(m, os.path.join(paths.SUIM_MODEL_DIR, f"SUIM_subset_1_topK_{{j}}.h5"))
"""


HELA_CONFIG = """[DEFAULT]
SEED = 42
NUM_EPOCHS = 2
BATCH_SIZE = 8
LR = 0.003
WD = 1e-4
THRESHOLD = 0.5
TOP_Ks = 2

[HELA]
IMAGE_HEIGHT = 64
IMAGE_WIDTH = 64
IMAGE_CHANNELS = 1
NUM_CLASSES = 3
BASE_DIR = {base}/
ALPHA = 0.5
ACTIFU = relu
ACTIFU_OUTPUT = sigmoid
ERODE_KERNEL = 0
DILATE_KERNEL = 0
BLOCK_INPUT = True
BLOCK_OUTPUT = True
FREE_ROTATION = True
NUM_IMAGES_IM_PLUS = 1
"""


HELA_SETUP = """
import os, sys
import numpy as np
sys.path.insert(0, {root!r})
from inconsistencymasks_amd import functions as F, paths
from inconsistencymasks_amd.unet import get_unet
rng = np.random.default_rng(0)
yy, xx = np.mgrid[0:64, 0:64]
def sample(n, d, tag):
    for k in ("brightfield", "alive", "dead", "mod_position"):
        os.makedirs(os.path.join(d, k), exist_ok=True)
    for i in range(n):
        bf = np.full((64, 64), 120, np.int64) + rng.integers(-8, 8, (64, 64))
        alive = np.zeros((64, 64), np.uint8); dead = np.zeros((64, 64), np.uint8); pos = np.zeros((64, 64), np.uint8)
        for cy, cx, is_dead in ((16, 16, 0), (16, 46, 1), (46, 30, int(rng.integers(0, 2)))):
            cy += int(rng.integers(-4, 5)); cx += int(rng.integers(-4, 5))
            cell = (yy - cy) ** 2 + (xx - cx) ** 2 < 64
            bf[cell] += 70 if is_dead else -60
            (dead if is_dead else alive)[cell] = 255
            pos[(yy - cy) ** 2 + (xx - cx) ** 2 < 9] = 255
        name = f"{{tag}}_{{i:04d}}.png"
        F.write_png(os.path.join(d, "brightfield", name), bf.clip(0, 255).astype(np.uint8))
        F.write_png(os.path.join(d, "alive", name), alive); F.write_png(os.path.join(d, "dead", name), dead)
        F.write_png(os.path.join(d, "mod_position", name), pos)
sample(16, paths.HELA_TRAIN_LABELED_DIR, "lab"); sample(24, paths.HELA_TRAIN_UNLABELED_DIR, "unl")
sample(8, paths.HELA_VAL_DIR, "val"); sample(8, paths.HELA_TEST_DIR, "tst")
os.makedirs(paths.HELA_MODEL_DIR, exist_ok=True)
import torch
bfd = os.path.join(paths.HELA_TRAIN_LABELED_DIR, "brightfield")
items = [F.parse_image_hela(os.path.join(bfd, n), 1) for n in sorted(os.listdir(bfd))]
x = torch.from_numpy(np.stack([it[0] for it in items])).cuda()
y = torch.from_numpy(np.stack([it[1] for it in items])).cuda()
for j in (1, 2):
    m = get_unet(64, 64, 1, 3, 0.5, "relu", "sigmoid", seed=j)
    for it in range(700):
        m.train_step(x, y, 0, 3e-3 if it < 200 else 0.0, 1e-4 if it < 200 else 0.0)
    m.repack()
    F.save_model(m, os.path.join(paths.HELA_MODEL_DIR, f"HELA_subset_1_topK_{{j}}.h5"))
"""


CITY_CONFIG = MULTI_CONFIG.replace("[SUIM]", "[CITYSCAPES]").replace("IMAGE_HEIGHT = 64", "IMAGE_HEIGHT = 48") \
    .replace("IMAGE_WIDTH = 64", "IMAGE_WIDTH = 96").replace("NUM_CLASSES = 3", "NUM_CLASSES = 5").replace("ALPHA = 0.5", "ALPHA = 1")


CITY_SETUP = """
import os, sys
import numpy as np
sys.path.insert(0, {root!r})
from inconsistencymasks_amd import functions as F, paths
from inconsistencymasks_amd.unet import get_unet
rng = np.random.default_rng(0)
H, W = 48, 96
def sample(n, d_img, d_mask):
    os.makedirs(d_img, exist_ok=True); os.makedirs(d_mask, exist_ok=True)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        horizon, cx = rng.integers(16, 30), rng.integers(20, 76)
        cls = np.full((H, W), 1, np.uint8)                       # "sky"
        cls[yy > horizon] = 2                                     # "road"
        cls[(yy > horizon - 8) & (abs(xx - cx) < 9) & (yy < horizon + 6)] = 3      # "car"
        cls[(xx < 6) & (yy > 8)] = 4                              # "pole"
        img = np.stack([40 * cls + 20, 250 - 45 * cls, 30 + 50 * (cls == 3) + 20 * cls], -1)
        img = (img + rng.integers(-10, 10, (H, W, 3))).clip(0, 255).astype(np.uint8)
        F.write_png(os.path.join(d_img, f"c_{{i:04d}}.png"), img)
        F.write_png(os.path.join(d_mask, f"c_{{i:04d}}.png"), cls)
sample(16, paths.CITYSCAPES_TRAIN_LABELED_IMAGES_DIR, paths.CITYSCAPES_TRAIN_LABELED_MASKS_DIR)
sample(24, paths.CITYSCAPES_TRAIN_UNLABELED_IMAGES_DIR, paths.CITYSCAPES_TRAIN_UNLABELED_MASKS_DIR)
sample(8, paths.CITYSCAPES_VAL_IMAGES_DIR, paths.CITYSCAPES_VAL_MASKS_DIR)
sample(8, paths.CITYSCAPES_TEST_IMAGES_DIR, paths.CITYSCAPES_TEST_MASKS_DIR)
"""


def _run_one_and_two_ranks(tmp_path, config, setup, script, extra_env=None, worlds=(1, 2)):
    """the same toy driver run with one rank and with two (or `worlds[1]`) ranks time-slicing one GPU over gloo; returns the data dirs"""
    import socket
    outs = {}
    for world in worlds:
        work = tmp_path / f"w{world}"
        base = work / "data"
        work.mkdir()
        cfg = work / "config.ini"
        cfg.write_text(config.format(base=base))
        env = {**os.environ, "IM_CONFIG": str(cfg), "IM_RUNIDS": "1", "IM_NS": "2", "IM_GENS": "0", "IM_CANDIDATES": "0,1",
               **(extra_env or {})}
        subprocess.run([sys.executable, "-c", setup.format(root=ROOT)], env=env, check=True, cwd=work)
        if world == 1:
            cmd = [sys.executable, script]
        else:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            env.update(IMK_DIST_BACKEND="gloo", IMK_ONE_GPU="1")
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                   "--master-port", str(port), script]
        r = subprocess.run(cmd, env=env, cwd=work, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[world] = base
    return outs


def _same_png_tree(a, b, subs, channels):
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import functions as F
    for sub in subs:
        assert sorted(os.listdir(a / sub)) == sorted(os.listdir(b / sub)), sub
        for n in sorted(os.listdir(a / sub)):
            ch = channels.get(sub, 1)
            assert np.array_equal(F.read_png(str(a / sub / n), ch), F.read_png(str(b / sub / n), ch)), (sub, n)


def _toy_run(tmp_path, config, setup, script, gens="0,1", seed_script=None):
    base = tmp_path / "data"
    cfg = tmp_path / "config.ini"
    cfg.write_text(config.format(base=base))
    env = {**os.environ, "IM_CONFIG": str(cfg), "IM_RUNIDS": "1", "IM_NS": "2", "IM_GENS": gens, "IM_CANDIDATES": "0,1"}
    subprocess.run([sys.executable, "-c", setup.format(root=ROOT)], env=env, check=True, cwd=tmp_path)
    if seed_script:      # the labelled-subset baseline that provides the generation-0 models
        r = subprocess.run([sys.executable, seed_script], env=env, cwd=tmp_path, capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    r = subprocess.run([sys.executable, script], env=env, cwd=tmp_path, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return base, r.stdout


@pytest.mark.parametrize("ds", ["ISIC_2018", "SUIM", "Cityscapes", "HeLa"])
def test_model_ensemble_script_toy_run(tmp_path, ds):
    config, setup, script, tag, subs = {
        "ISIC_2018": (CONFIG, SETUP, "ISIC_2018/06_ISIC_2018_model_ensemble.py", "ISIC_2018", ("images", "masks")),
        "SUIM": (MULTI_CONFIG, MULTI_SETUP, "SUIM/07_SUIM_model_ensemble.py", "SUIM", ("images", "masks")),
        "Cityscapes": (CITY_CONFIG, CITY_SETUP, "Cityscapes/06_Cityscapes_model_ensemble.py", "CITYSCAPES", ("images", "masks")),
        "HeLa": (HELA_CONFIG, HELA_SETUP, "HeLa/06_HeLa_model_ensemble.py", "HELA", ("brightfield", "alive", "dead", "mod_position")),
    }[ds]
    seed = os.path.join(ROOT, "Cityscapes", "03_Cityscapes_subset.py") if ds == "Cityscapes" else None
    base, out = _toy_run(tmp_path, config, setup, os.path.join(ROOT, script), seed_script=seed)
    csvs = sorted(os.listdir(base / "csv"))
    assert not [f for f in csvs if f.startswith("mean_im_size_")], csvs
    for g in (0, 1):
        stem = f"{tag}_model_ensemble_1_n2_gen{g}"
        assert f"results_{stem}.csv" in csvs
        models = sorted(os.listdir(base / "models"))
        assert f"{stem}_topK_1.h5" in models and f"{stem}_topK_2.h5" in models
        for split in ("val", "test", "train_unlabeled"):
            d = base / f"{split}_predictions" / "model_ensemble" / stem
            assert sorted(os.listdir(d)) == sorted(subs), (split, os.listdir(d))
        rows = [r.split(";") for r in (base / "csv" / f"results_{stem}.csv").read_text().strip().splitlines()]
        assert len(rows) == 3 and {r[0] for r in rows[1:]} == {f"{stem}_0", f"{stem}_1"}
        if ds == "HeLa":      # ranked by mean_cell_count_error_test (row index 6), ascending; the driver prints the ranking
            order = sorted(rows[1:], key=lambda r: float(r[6]))
            line = next(ln for ln in out.splitlines() if ln.startswith("[(") and f"{stem}_" in ln)
            assert line.index(f"'{order[0][0]}'") < line.index(f"'{order[1][0]}'") or float(order[0][6]) == float(order[1][6])
    unl = base / "train_unlabeled_predictions" / "model_ensemble" / f"{tag}_model_ensemble_1_n2_gen0" / subs[0]
    assert len(os.listdir(unl)) >= 24      # the pseudo-labelled set (24 toy images) plus the labelled pairs copied in


def test_isic_model_ensemble_two_ranks_on_one_gpu(tmp_path):
    outs = _run_one_and_two_ranks(tmp_path, CONFIG, SETUP, os.path.join(ROOT, "ISIC_2018", "06_ISIC_2018_model_ensemble.py"))
    stem = "ISIC_2018_model_ensemble_1_n2_gen0"
    for split in ("val", "test", "train_unlabeled"):
        a, b = (outs[w] / f"{split}_predictions" / "model_ensemble" / stem for w in (1, 2))
        _same_png_tree(a, b, ("images", "masks"), {"images": 3})
