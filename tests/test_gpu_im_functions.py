"""The IM functions of record (rows a4-a7: get_im_prediction_binary / _hela / _multiclass, pred_masks_to_im_binary /
_multiclass) against the outputs the real reference recorded for the same calls (tests/golden/im_*.npz, written by
tests/golden/make_golden.py:134-253), called the way the reference's scripts call them: through the repo-root `functions`
module, with Keras-like `.predict` models.  What is pinned here is the wrapper, not the kernel underneath (tests/test_gpu_im.py
has that): tuple order, [H,W] shapes, uint8 masks, np.int64 sizes, the first image of the batch, HeLa's `>=` and summed size,
the lists_equal rule, the one-hot detour of pred_masks_to_im_multiclass with its K <= 64 limit, both branches of
_stack_predictions and both ranks of `prepared_image`.  Every comparison is exact."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import im_oracle as O  # noqa: E402

FIVE = ("get_im_prediction_binary", "get_im_prediction_hela", "get_im_prediction_multiclass", "pred_masks_to_im_binary",
        "pred_masks_to_im_multiclass")


class FixedModel:
    """Fake Keras model (tests/golden/make_golden.py:99-106): .predict([x]) returns a fixed [1,H,W,K] float32 array.  It has
    no predict_device, so _stack_predictions takes its duck-typed branch."""

    def __init__(self, arr):
        self.arr = arr

    def predict(self, x):
        assert isinstance(x, list) and len(x) == 1 and x[0].dtype == np.uint8 and x[0].ndim == 4     # Keras' model.predict([batch])
        return self.arr


@pytest.fixture(scope="module")
def F():
    """the import the reference's scripts use (`from functions import ...`); it must hand out the package's own objects"""
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    import functions as root
    from inconsistencymasks_amd import functions as pkg
    for name in FIVE:
        assert getattr(root, name) is getattr(pkg, name), name
    return root


def _load(golden_dir, name):
    with np.load(os.path.join(golden_dir, name)) as d:
        return {k: d[k] for k in d.files}


def _mask(got, want):
    assert got.dtype == np.uint8 and want.dtype == np.uint8
    assert np.array_equal(got, want)                  # shape included


def _size(got, want):
    assert isinstance(got, np.int64)
    assert int(got) == int(want)


# ---- binary (a4 / a5) ----------------------------------------------------------------------------------------------------------
def test_binary_functions_reproduce_the_reference(F, golden_dir):
    g = _load(golden_dir, "im_binary.npz")
    lo, hi = np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))
    seen = set()
    assert len(g["cases"]) == 37
    for k in g["cases"]:
        preds = g[k + "_preds"]                                                     # [N,1,H,W,1]
        n, _, h, w, _ = preds.shape
        for v, tag in ((np.nan, "nan"), (np.inf, "+inf"), (-np.inf, "-inf"), (0.5, "thr"), (lo, "below"), (hi, "above")):
            if (np.isnan(preds).any() if tag == "nan" else (preds == np.float32(v)).any()):
                seen.add(tag)
        models = [FixedModel(preds[i]) for i in range(n)]
        for x in (np.zeros((1, h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8)):
            out = F.get_im_prediction_binary(models, x, 0.5)
            assert isinstance(out, tuple) and len(out) == 4, k
            _mask(out[0], g[k + "_final"])
            _mask(out[1], g[k + "_im"])
            _size(out[2], g[k + "_sizes"][0])                                       # (im_size, pred_size), in that order
            _size(out[3], g[k + "_sizes"][1])
        with np.errstate(invalid="ignore"):
            votes = [(preds[i][0] > 0.5).astype(int) for i in range(n)]             # [H,W,1] int64, as functions.py:3157 passes them
        assert votes[0].shape == (h, w, 1) and votes[0].dtype == np.int64
        for maps in (votes, [v[..., 0] for v in votes]):
            out = F.pred_masks_to_im_binary(maps)
            assert isinstance(out, tuple) and len(out) == 4, k
            _mask(out[0], g[k + "_final"])
            _mask(out[1], g[k + "_im"])
            _size(out[2], g[k + "_sizes"][0])
            _size(out[3], g[k + "_sizes"][1])
    assert seen == {"nan", "+inf", "-inf", "thr", "below", "above"}, seen          # the adversarial cases are all here
    assert any(int(g[k + "_sizes"][0]) != int(g[k + "_sizes"][1]) for k in g["cases"])     # a swapped pair would show


# ---- HeLa (a4', `>=`) ----------------------------------------------------------------------------------------------------------
def _check_hela(out, want_masks, want_im, want_size):
    assert isinstance(out, tuple) and len(out) == 5
    for got, want in zip(out[:3], want_masks):                                       # alive, dead, pos
        _mask(got, want)
    _mask(out[3], want_im)
    _size(out[4], want_size)


def test_hela_function_reproduces_the_reference(F, golden_dir):
    g = _load(golden_dir, "im_hela.npz")
    assert len(g["cases"]) == 12
    for k in g["cases"]:
        preds = g[k + "_preds"]                                                     # [N,1,H,W,3]
        n, _, h, w, _ = preds.shape
        models = [FixedModel(preds[i]) for i in range(n)]
        for x in (np.zeros((1, h, w, 1), np.uint8), np.zeros((h, w, 1), np.uint8)):
            _check_hela(F.get_im_prediction_hela(models, x), [g[f"{k}_{nm}"] for nm in ("alive", "dead", "pos")], g[k + "_im"],
                        g[k + "_sizes"][0])
        e = O.im_binary(preds[:, 0], 0.5, True)
        assert int(g[k + "_sizes"][0]) == int(e["im_size_ch"].sum())                 # the recorded size is the sum over the maps


def test_hela_threshold_is_inclusive(F, golden_dir):
    """a pixel where EVERY model sits exactly on the threshold is foreground under `>=` and background under `>`"""
    g = _load(golden_dir, "im_hela.npz")
    hits = 0
    for k in g["cases"]:
        preds = g[k + "_preds"]
        on_thr = np.all(preds[:, 0] == np.float32(0.5), axis=0)                      # [H,W,3]
        if not on_thr.any():
            continue
        hits += int(on_thr.sum())
        n, _, h, w, _ = preds.shape
        ge, gt = O.im_binary(preds[:, 0], 0.5, True), O.im_binary(preds[:, 0], 0.5, False)
        out = F.get_im_prediction_hela([FixedModel(preds[i]) for i in range(n)], np.zeros((1, h, w, 1), np.uint8))
        for c in range(3):
            assert np.all(out[c][on_thr[..., c]] == 255)
            assert np.all(ge["final"][c][on_thr[..., c]] == 255) and np.all(gt["final"][c][on_thr[..., c]] == 0)
        _check_hela(out, ge["final"], ge["im"], ge["im_size"])
    assert hits > 0, "the fixture has no pixel where every model equals the threshold"
    # and one built for it: every model on the threshold at every pixel of map 0, one model below it on map 1
    stack = np.full((3, 1, 8, 8, 3), 0.5, np.float32)
    stack[1, ..., 1] = np.nextafter(np.float32(0.5), np.float32(0))
    stack[:, ..., 2] = np.nextafter(np.float32(0.5), np.float32(0))
    e = O.im_binary(stack[:, 0], 0.5, True)
    assert e["final"][0].all() and e["im_ch"][1].all() and not e["final"][2].any() and int(e["im_size"]) == 64
    _check_hela(F.get_im_prediction_hela([FixedModel(stack[i]) for i in range(3)], np.zeros((8, 8, 1), np.uint8), 0.5),
                e["final"], e["im"], e["im_size"])


def test_hela_other_threshold(F):
    """threshold=0.3 (float32(0.3) is what the kernel compares with): values on it, next to it and far from it"""
    rng = np.random.default_rng(30)
    t = np.float32(0.3)
    stack = rng.random((3, 1, 16, 24, 3), dtype=np.float32)
    pool = np.array([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1)), 0.5, np.nan, np.inf, -np.inf], np.float32)
    flat = stack.reshape(-1)
    idx = rng.choice(flat.size, flat.size // 4, replace=False)
    flat[idx] = pool[rng.integers(0, len(pool), idx.size)]
    stack[:, 0, 0, 0, :] = t                                                         # all models on the threshold
    e = O.im_binary(stack[:, 0], 0.3, True)
    assert int(e["im_size"]) > 0 and not np.array_equal(e["final"], O.im_binary(stack[:, 0], 0.5, True)["final"])
    out = F.get_im_prediction_hela([FixedModel(stack[i]) for i in range(3)], np.zeros((1, 16, 24, 1), np.uint8), threshold=0.3)
    _check_hela(out, e["final"], e["im"], e["im_size"])
    assert np.all(out[0][0, 0] == 255)


# ---- multiclass (a6 / a7) ------------------------------------------------------------------------------------------------------
def test_multiclass_functions_reproduce_the_reference(F, golden_dir):
    g = _load(golden_dir, "im_multiclass.npz")
    unequal = [k for k in g["cases"] if int(g[k + "_lists_equal"][0]) == 0]
    equal = [k for k in g["cases"] if int(g[k + "_lists_equal"][0]) == 1]
    assert unequal and equal, "the fixture must hold both outcomes of the unique-set filter"
    for k in g["cases"]:
        preds = g[k + "_preds"]                                                     # [N,1,H,W,K]
        n, _, h, w, _ = preds.shape
        models = [FixedModel(preds[i]) for i in range(n)]
        for filt in (False, True):
            for x in (np.zeros((1, h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8)):
                out = F.get_im_prediction_multiclass(models, x, filt)
                assert isinstance(out, tuple) and len(out) == 4, k
                _mask(out[0], g[k + "_final"])
                _mask(out[1], g[k + "_im"])
                _size(out[2], g[k + "_sizes"][0])
                assert type(out[3]) is bool, k
                assert out[3] == (bool(g[k + "_lists_equal"][0]) if filt else True), (k, filt)
        labels = [np.argmax(preds[i], -1) for i in range(n)]                        # [1,H,W] int64, as functions.py:3225-3236 passes them
        assert labels[0].shape == (1, h, w) and labels[0].dtype == np.int64
        for maps in (labels, [m[0] for m in labels]):
            out = F.pred_masks_to_im_multiclass(maps)
            assert isinstance(out, tuple) and len(out) == 3, k
            _mask(out[0], g[k + "_final"])
            _mask(out[1], g[k + "_im"])
            _size(out[2], g[k + "_sizes"][0])


def _label_case(F, labels):
    final, im, size = F.pred_masks_to_im_multiclass(list(labels))
    wf, wi, ws = O.im_multiclass_from_labels(np.stack([np.asarray(m).reshape(np.asarray(m).shape[-2:]) for m in labels]))
    _mask(final, wf)
    _mask(im, wi)
    _size(size, ws)
    return final, im, size


def test_label_map_detour_edges(F):
    """pred_masks_to_im_multiclass builds one-hot rows of k = labels.max() + 1 classes for the kernel: k = 1, k = 64 (the
    kernel's ceiling) and one class too many"""
    from inconsistencymasks_amd._lib import ImkError
    rng = np.random.default_rng(64)
    zeros = [np.zeros((8, 8), np.int64) for _ in range(3)]
    final, im, size = _label_case(F, zeros)                                          # K = 1
    assert not final.any() and not im.any() and int(size) == 0
    a = rng.integers(0, 64, (8, 8))
    a[0, 0] = a[7, 7] = 63
    b = a.copy()
    b[3, :] = (a[3, :] + 1) % 64                                                     # one row of disagreement
    final, im, size = _label_case(F, [a, b])                                         # largest label 63: K = 64
    assert final[0, 0] == 63 and final[7, 7] == 63 and int(size) == 8 and np.all(im[3] == 255)
    _label_case(F, [a[None], b[None], a[None]])                                      # [1,H,W] maps
    c = a.copy()
    c[4, 4] = 64
    with pytest.raises(ImkError, match="unsupported shape"):
        F.pred_masks_to_im_multiclass([a, c])
    c[4, 4] = 200
    with pytest.raises(ImkError, match="unsupported shape"):
        F.pred_masks_to_im_multiclass([c, c])


# ---- native models: the predict_device branch of _stack_predictions ------------------------------------------------------------
def test_native_models_binary(F):
    from inconsistencymasks_amd.unet import UNet
    models = [UNet(32, 32, 3, 1, 0.5, "sigmoid", seed=11 + j) for j in range(2)]
    x = np.random.default_rng(5).integers(0, 256, (32, 32, 3)).astype(np.uint8)
    xd = torch.from_numpy(x[None]).cuda()
    stack = np.stack([m.predict_device(xd).cpu().numpy()[0] for m in models])       # [2,32,32,1]
    e = O.im_binary(stack, 0.5, False)
    assert 0 < int(e["im_size"]) < 32 * 32                                           # the two models do disagree somewhere
    for xin in (x, x[None]):
        out = F.get_im_prediction_binary(models, xin, 0.5)
        _mask(out[0], e["final"][0])
        _mask(out[1], e["im"])
        _size(out[2], e["im_size"])
        _size(out[3], e["pred_size"])
    # one native model and one `.predict` fake in the same call: both branches of _stack_predictions
    other = np.random.default_rng(6).random((1, 32, 32, 1), dtype=np.float32)
    e = O.im_binary(np.stack([stack[0], other[0]]), 0.5, False)
    out = F.get_im_prediction_binary([models[0], FixedModel(other)], x, 0.5)
    _mask(out[0], e["final"][0])
    _mask(out[1], e["im"])
    _size(out[2], e["im_size"])
    _size(out[3], e["pred_size"])
    assert int(e["im_size"]) != int(e["pred_size"])                                  # a swapped pair would show


def test_native_models_multiclass(F):
    from inconsistencymasks_amd.unet import UNet
    models = [UNet(32, 48, 3, 9, 0.5, "softmax", seed=21 + j) for j in range(2)]
    x = np.random.default_rng(7).integers(0, 256, (32, 48, 3)).astype(np.uint8)
    xd = torch.from_numpy(x[None]).cuda()
    stack = np.stack([m.predict_device(xd).cpu().numpy()[0] for m in models])       # [2,32,48,9]
    for filt in (False, True):
        e = O.im_multiclass(stack, filt)
        out = F.get_im_prediction_multiclass(models, x, filt)
        _mask(out[0], e["final"])
        _mask(out[1], e["im"])
        _size(out[2], e["im_size"])
        assert type(out[3]) is bool and out[3] == e["lists_equal"]
    assert 0 < int(e["im_size"]) < 32 * 48
    fake = np.zeros((1, 32, 48, 9), np.float32)
    fake[..., 4] = 1.0                                                               # a model that says class 4 everywhere
    mixed = np.stack([stack[0], fake[0]])
    for filt in (False, True):
        e = O.im_multiclass(mixed, filt)
        out = F.get_im_prediction_multiclass([models[0], FixedModel(fake)], x[None], filt)
        _mask(out[0], e["final"])
        _mask(out[1], e["im"])
        _size(out[2], e["im_size"])
        assert type(out[3]) is bool and out[3] == e["lists_equal"]
