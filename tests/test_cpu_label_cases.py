"""The rules of the scalar-IoU multiclass EvalNet family against the recorded reference run (tests/golden/evalnet_scalar.npz, made by
tests/golden/make_golden_evalnet_scalar.py with the reference's own functions): the numpy restatement of the label
(tests/label_cases.py: counts by explicit loops, the label from the counts), the host half of the package's label
(evaluate.iou_multi_unique_from_counts), the writers' names, draws, selection rule and copy numbers.  No GPU."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import label_cases as LC  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "evalnet_scalar.npz")) as d:
        return {k: d[k] for k in d.files}


def _case(gold, i):
    return gold[f"iou{i}_pred"], gold[f"iou{i}_gt"], gold.get(f"iou{i}_im"), gold[f"iou{i}_value"]


def test_label_from_counts_equals_the_reference(gold):
    from inconsistencymasks_amd import evaluate
    n = int(gold["iou_count"])
    assert n >= 9
    for i in range(n):
        pred, gt, im, (value, rounded) = _case(gold, i)
        c = LC.counts(pred, gt, im)
        assert c[0].sum() == c[1].sum() == gt.size and (c[2] <= np.minimum(c[0], c[1])).all()
        assert LC.label(c) == value and LC.rounded(c) == rounded, i                       # bit for bit: float64 ==
        assert evaluate.iou_multi_unique_from_counts(c, "pred") == value, i
        assert round(evaluate.iou_multi_unique_from_counts(c, "pred"), 4) == rounded, i
        blocked, _ = LC.block(pred, im)
        swapped = LC.counts(gt, blocked)      # the maps in each other's seat: "gt" of the swapped counts is "pred" of these
        assert evaluate.iou_multi_unique_from_counts(swapped, "gt") == value, i
        if im is None:
            assert np.array_equal(c[3], c[0])
    with pytest.raises(ValueError):
        evaluate.iou_multi_unique_from_counts(c, "both")


def test_the_cases_tell_the_rule_from_its_neighbours(gold):
    """the properties the issue lists are in the fixture: the other map's classes, the 1e-7, the divisor, the decimal half"""
    differs = {"gt": 0, "no_eps": 0}
    for i in range(int(gold["iou_count"])):
        pred, gt, im, (value, rounded) = _case(gold, i)
        c = LC.counts(pred, gt, im)
        differs["gt"] += LC.label(c, "gt") != value
        lst = [c[2, v] / float(c[0, v] + c[1, v] - c[2, v]) for v in range(256) if c[1, v] > 0]
        differs["no_eps"] += round(sum(lst) / len(lst), 4) != rounded
    assert differs["gt"] and differs["no_eps"]
    pred, gt, im, (value, rounded) = _case(gold, 1)      # class 0 through blocking alone
    assert not (pred == 0).any() and not (gt == 0).any() and LC.counts(pred, gt, im)[1, 0] == (im > 0).sum() > 0
    assert (_case(gold, 2)[1] == 255).any()
    assert _case(gold, 3)[3][0] == 256 / (256 + 1e-7)
    assert tuple(_case(gold, 4)[3]) == (3 / (800 + 1e-7), 0.0037) and round(np.float64(3 / 800), 4) == 0.0038


def test_single_writer_names_masks_and_labels(gold):
    names, gt, probs = [str(n) for n in gold["sw_names"]], gold["sw_gt"], gold["sw_probs"]
    files, lines, k = [], [], 0
    for step_i, step in enumerate((0, 11)):
        for j, n in enumerate(names):
            pred = np.argmax(probs[j], -1).astype(np.uint8)
            assert np.array_equal(pred, gold["sw_masks"][step_i, j])
            files.append("/tout/masks/" + LC.pred_name(n, step))
            lines.append(f"{LC.pred_name(n, step)};{LC.rounded(LC.counts(pred, gt[j]))}")
        if step == 0:
            for n in names:
                files += ["/tout/images/" + n, "/tout/masks/" + n]
                lines.append(f"{n};1.0")
    assert files == [str(f) for f in gold["sw_files"]]
    assert lines == [str(s) for s in gold["sw_labels"]]
    assert LC.pred_name("l_001_aug_03.png", 11) == "l_001____11_03.png" and LC.pred_name("l_001_aug_03.png", 0) == "l_001_aug_03___0.png"
    from inconsistencymasks_amd.evalnet_functions import _pred_name
    assert all(_pred_name(n, i) == LC.pred_name(n, i) for n in names for i in (0, 9, 10, 11))


def test_im_writer_draw_order_names_and_labels(gold):
    from inconsistencymasks_amd.evalnet_functions import _draw_plan
    assert [str(k) for k in gold["imw_kinds"]] == ["randint", "sample", "choice", "choice", "random"]
    names, draws = [str(n) for n in gold["imw_names"]], gold["imw_draws"]
    loops, n = gold["imw_pred"].shape[:2]
    rng = random.Random(int(gold["imw_seed"]))
    lines = []
    for nl in range(loops):
        plan = _draw_plan(rng, n, gold["imw_probs"].shape[0], 2, 4)      # the draws of one loop, in the reference's order
        for j, (subset, ke, kd, aug) in enumerate(plan):
            cnt, word, rke, rkd, coin = draws[nl * n + j, :5]
            assert (len(subset), sum(1 << m for m in subset), ke, kd, aug) == (cnt, word, rke, rkd, coin < 0.5), (nl, j)
            pred, im = gold["imw_pred"][nl, j], gold["imw_im"][nl, j]
            blocked, image = LC.block(pred, im, gold["imw_images"][j])
            assert np.array_equal(blocked, gold["imw_out_masks"][nl, j]) and np.array_equal(image, gold["imw_out_images"][nl, j])
            lines.append(f"{names[j][:-4]}_aug_{nl}.png;{LC.rounded(LC.counts(pred, gold['imw_gt'][j], im))}")
    assert lines == [str(s) for s in gold["imw_labels"]]
    assert (draws[:, 2] > 0).any() and (draws[:, 3] > 0).any() and not np.array_equal(gold["imw_im"], gold["imw_im_raw"])


def test_selection_rule(gold):
    seen = set()
    for i in range(int(gold["sel_count"])):
        scores, (thr, last, best, keep, n) = gold[f"sel{i}_scores"], gold[f"sel{i}_meta"]
        assert scores.shape[0] == n
        got_best, got_score, got_keep = LC.select(scores, thr)
        given = gold[f"sel{i}_argmax_in"].reshape(-1)
        mean = scores[0] if n == 1 else np.mean(scores, axis=0)
        assert np.array_equal(mean, given, equal_nan=True) and mean.dtype == np.float32, i
        assert (got_best, got_keep) == (int(best), bool(keep)), i
        files = [str(f) for f in gold[f"sel{i}_files"]]
        if keep:
            assert files == [f"/out/images/u_{i:03d}.png", f"/out/masks/u_{i:03d}.png"]
            assert np.array_equal(gold[f"sel{i}_mask"], gold[f"sel{i}_cands"][int(best)])
        else:
            assert files == [""]
        seen.add((int(n), scores.shape[1]))
    assert {s[0] for s in seen} >= {1, 2, 3} and {s[1] for s in seen} == {5, 6, 10, 11}


def test_num_augs(gold):
    from inconsistencymasks_amd.evalnet_functions import num_augs_from_iou_f32
    for (lo, hi), scores, nums in zip(gold["aug_thresholds"], gold["aug_scores"], gold["aug_num"]):
        for v, want in zip(scores, nums):
            assert LC.num_augs(v, float(lo), float(hi)) == want, (lo, hi, v)
            assert num_augs_from_iou_f32(v, float(lo), float(hi)) == want, (lo, hi, v)
        assert set(nums.tolist()) == {1.0, 2.0, 3.0, 4.0, 5.0}


def test_confluence_helpers():
    from inconsistencymasks_amd import functions as F
    gt = np.zeros((10, 10), np.uint8)
    gt[:3] = 1
    gt[3, :3] = 2
    assert F.compute_classwise_confluence(gt, 4) == [0.67, 0.3, 0.03, 0.0]
    assert F.compute_classwise_confluence(np.full((3, 3), 2), 3) == [0.0, 0.0, 1.0]
    third = np.zeros((3, 1), np.uint8)
    third[0] = 1
    assert F.compute_classwise_confluence(third, 2) == [0.6667, 0.3333]
    assert F.get_confluence_binary(gt > 0) == 0.33 and F.get_confluence_binary(third) == 0.3333
    assert F.get_confluence_binary(gt) == 0.36       # the sum of the values, not the foreground count
