"""imk_label_counts (csrc/imk_label.hip) against its numpy restatement (tests/label_cases.py: explicit loops), bit for bit: counts, the
blocked prediction and the blocked image.  Sizes: 13 x 7 (91 pixels: a ragged tail, the second image at an odd base), 16 x 16,
48 x 40 (two workgroups per image), 33 x 31 with three images (image bases 0, 1023, 2046 bytes: head bytes, 16-byte pieces and tail
bytes meet inside one batch).  Then the equalities that hold whatever the values are, and the buffer contract through the C ABI inside
the guarded arena (tests/arena.py)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import arena as A  # noqa: E402
import label_cases as LC  # noqa: E402

SIZES = [(2, 13, 7), (2, 16, 16), (2, 48, 40), (3, 33, 31)]
IMK_EINVAL = -1
_REF = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def maps(b, h, w, im_value, full_range=False):
    """the maps of a case and their restated results, computed once: pred, gt, im, image per c, counts, blocked, blocked image per c"""
    key = (b, h, w, im_value, full_range)
    if key not in _REF:
        pred, gt, im = LC.case_maps(h, w, b, 7 * h + w + (im_value or 0), im_value=im_value, full_range=full_range)
        rng = np.random.default_rng(h * w)
        image = {c: rng.integers(1, 256, (b, h, w, c), dtype=np.uint8) for c in (1, 3)}
        counts = np.stack([LC.counts(pred[i], gt[i], None if im is None else im[i]) for i in range(b)])
        blocked = np.stack([LC.block(pred[i], None if im is None else im[i])[0] for i in range(b)])
        bimage = {c: np.stack([LC.block(pred[i], None if im is None else im[i], image[c][i])[1] for i in range(b)]) for c in (1, 3)}
        _REF[key] = (pred, gt, im, image, counts, blocked, bimage)
    return _REF[key]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("im_value", [None, 1, 255])
@pytest.mark.parametrize("b,h,w", SIZES)
def test_against_the_restatement(b, h, w, im_value, c):
    from inconsistencymasks_amd import evaluate
    pred, gt, im, image, counts, blocked, bimage = maps(b, h, w, im_value, full_range=(h == 16))      # 16 x 16: ids over 0..255
    p, g, m, img = dev(pred), dev(gt), None if im is None else dev(im), dev(image[c])
    out, got = evaluate.label_counts(p, g, m, img, True)
    assert got.dtype == np.int64 and np.array_equal(got, counts)
    assert np.array_equal(out.cpu().numpy(), blocked) and np.array_equal(img.cpu().numpy(), bimage[c])
    assert np.array_equal(p.cpu().numpy(), pred)                                  # the prediction itself is an input
    if im is None:
        assert np.array_equal(got[:, 3], got[:, 0])
    # pred_blocked aliasing pred, no image; a second run is bit-equal
    alias, got2 = evaluate.label_counts(p, g, m, None, p)
    assert alias is p and np.array_equal(p.cpu().numpy(), blocked) and np.array_equal(got2, counts)
    # counts alone
    assert np.array_equal(evaluate.label_counts(dev(pred), g, m)[1], counts)
    # per-image independence: an image alone (its base is aligned then, inside the batch it need not be)
    for i in range(b):
        one = evaluate.label_counts(dev(pred[i:i + 1]), dev(gt[i:i + 1]), None if im is None else dev(im[i:i + 1]))[1]
        assert np.array_equal(one[0], counts[i]), i
    for i in range(b):
        want = LC.label(counts[i])
        assert evaluate.iou_multi_unique_from_counts(got[i], "pred") == want


def test_one_class_and_fully_blocked():
    from inconsistencymasks_amd import evaluate
    b, h, w = 3, 33, 31
    pred, gt = np.full((b, h, w), 5, np.uint8), np.full((b, h, w), 5, np.uint8)
    gt[1] = 7
    im = np.zeros((b, h, w), np.uint8)
    im[2] = 255                                                                   # the third image is blocked completely
    img = dev(np.full((b, h, w, 3), 9, np.uint8))
    out, got = evaluate.label_counts(dev(pred), dev(gt), dev(im), img, True)
    want = np.zeros((b, 4, 256), np.int64)
    want[0, :, 5] = h * w
    want[1, 0, 7] = want[1, 3, 7] = want[1, 1, 5] = h * w
    want[2, 0, 5] = want[2, 1, 0] = h * w                                         # nothing of the ground truth is left unblocked
    assert np.array_equal(got, want)
    assert (out[:2] == 5).all() and (out[2] == 0).all() and (img[:2] == 9).all() and (img[2] == 0).all()
    assert evaluate.iou_multi_unique_from_counts(got[0], "pred") == (h * w) / (h * w + 1e-7)
    assert evaluate.iou_multi_unique_from_counts(got[1], "pred") == 0.0 and evaluate.iou_multi_unique_from_counts(got[2], "pred") == 0.0


def test_equals_block_apply_and_the_evaluation_counts():
    """where they apply: imk_block_apply's bytes, and rows 0..2 of imk_eval_multiclass on the probabilities whose arg-max the prediction is"""
    from inconsistencymasks_amd import evaluate
    from inconsistencymasks_amd import im as IM
    b, h, w, k = 3, 33, 31, 9
    rng = np.random.default_rng(5)
    probs = dev(rng.random((b, h, w, k), dtype=np.float32))
    gt = dev(rng.integers(0, k + 1, (b, h, w)).astype(np.uint8))
    pred, ev = evaluate.eval_multiclass(probs, gt)
    got = evaluate.label_counts(pred, gt)[1]
    assert np.array_equal(got[:, :3], ev[:, :3]) and np.array_equal(got[:, 3], ev[:, 0])
    for i in range(b):
        assert evaluate.iou_multi_unique_from_counts(got[i], "gt") == evaluate.pa_iou_from_counts(ev[i], h * w)[1]
    im = dev((rng.random((b, h, w)) < 0.3).astype(np.uint8) * 255)
    img = dev(rng.integers(1, 256, (b, h, w, 3), dtype=np.uint8))
    wi, wm = img.clone(), pred.clone()[:, None].contiguous()
    IM.block_apply(im, wi, wm)
    out, _ = evaluate.label_counts(pred, gt, im, img, True)
    assert torch.equal(img, wi) and torch.equal(out, wm[:, 0])


def _lib():
    from inconsistencymasks_amd._lib import lib
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("b,h,w,c,alias", [(3, 33, 31, 3, False), (2, 48, 40, 1, True), (2, 13, 7, 3, False)])
def test_buffer_contract(b, h, w, c, alias):
    """counts holds the fill on entry and is zeroed by the call; every output byte is written, nothing outside the buffers is, the
    inputs stay as they were, and the results do not depend on the fill"""
    pred, gt, im, image, counts, blocked, bimage = maps(b, h, w, 255)
    n = b * h * w
    specs = [("pred", dev(pred), "inout" if alias else "in"), ("gt", dev(gt), "in"), ("im", dev(im), "in"),
             ("image", dev(image[c]), "inout"), ("counts", b * 4 * 256 * 8, "out")]
    if not alias:
        specs.append(("blocked", n, "out"))
    ar = A.Arena(specs, "cuda")
    out = ar.check(lambda p: _lib().imk_label_counts(p["pred"], p["gt"], p["im"], p["image"], c, b, h, w, p["pred" if alias else "blocked"],
                                                     p["counts"], _stream()))
    assert np.array_equal(out["counts"].view(torch.int64).cpu().numpy().reshape(b, 4, 256), counts)
    assert np.array_equal(out["pred" if alias else "blocked"].cpu().numpy().reshape(b, h, w), blocked)
    assert np.array_equal(out["image"].cpu().numpy().reshape(b, h, w, c), bimage[c])
    # optional arguments left out: the outputs that remain are the same, the others stay unwritten
    ar = A.Arena([("pred", dev(pred), "in"), ("gt", dev(gt), "in"), ("counts", b * 4 * 256 * 8, "out")], "cuda")
    out = ar.check(lambda p: _lib().imk_label_counts(p["pred"], p["gt"], None, None, 0, b, h, w, None, p["counts"], _stream()))
    no_im = np.stack([LC.counts(pred[i], gt[i]) for i in range(b)])
    assert np.array_equal(out["counts"].view(torch.int64).cpu().numpy().reshape(b, 4, 256), no_im)


def test_argument_errors_write_nothing():
    b, h, w = 2, 16, 16
    pred, gt, im, image, *_ = maps(b, h, w, 255, True)
    ar = A.Arena([("pred", dev(pred), "in"), ("gt", dev(gt), "in"), ("im", dev(im), "in"), ("image", dev(image[3]), "inout"),
                  ("counts", b * 4 * 256 * 8, "out"), ("blocked", b * h * w, "out")], "cuda")
    bad = [lambda p: _lib().imk_label_counts(p["pred"], p["gt"], p["im"], p["image"], 2, b, h, w, p["blocked"], p["counts"], _stream()),
           lambda p: _lib().imk_label_counts(p["pred"], p["gt"], p["im"], p["image"], 4, b, h, w, p["blocked"], p["counts"], _stream()),
           lambda p: _lib().imk_label_counts(p["pred"], p["gt"], p["im"], p["image"], 3, 0, h, w, p["blocked"], p["counts"], _stream()),
           lambda p: _lib().imk_label_counts(p["pred"], p["gt"], p["im"], p["image"], 3, b, -1, w, p["blocked"], p["counts"], _stream()),
           lambda p: _lib().imk_label_counts(p["pred"], p["gt"], p["im"], p["image"], 3, b, h, 0, p["blocked"], p["counts"], _stream()),
           lambda p: _lib().imk_label_counts(None, p["gt"], p["im"], p["image"], 3, b, h, w, p["blocked"], p["counts"], _stream()),
           lambda p: _lib().imk_label_counts(p["pred"], None, p["im"], p["image"], 3, b, h, w, p["blocked"], p["counts"], _stream()),
           lambda p: _lib().imk_label_counts(p["pred"], p["gt"], p["im"], p["image"], 3, b, h, w, p["blocked"], None, _stream())]
    for call in bad:
        for fill in A.FILLS:
            ar.run(fill, call, want_rc=IMK_EINVAL, untouched=True)
