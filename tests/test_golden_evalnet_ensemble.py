"""The pin of the EvalNet-ensemble selection: tests/golden/make_golden_evalnet_ensemble.py drives the REAL reference's
create_training_data_for_segnet_with_ensemble_binary / ..._with_miou_ensemble_hela / ..._with_miou_ensemble_multiclass
(functions.py:5070-5577) with fixed-score fake EvalNets and numpy stand-ins for cv2 / os / shutil, and records a sha256 of every array in
tests/golden/evalnet_ensemble_digests.json.  The committed fixture must be exactly what that regeneration recorded; with a reference
checkout on disk (IMK_REFERENCE) it is regenerated into a temporary directory and compared.  The two rules imk_evalnet_select
implements (include/imk.h), restated in numpy below, must reproduce every recorded choice, every keep decision and every written mask.
tests/test_gpu_evalnet_select.py holds the kernel to the same recorded values.

The generator drives the reference's three EvalNet training-data writers as well (create_training_data_evalnet_ISIC_2018 / _miou_hela /
_miou_multiclass, functions.py:3419-3492, 4011-4135, 4248-4323) with a fixed-probability fake U-Net, for i = 0 and i = 11, and records
the written names, masks and labels.csv ("td*" keys).  training_data_rule below restates those writers in numpy and must reproduce
the record; tests/test_gpu_evalnet_ensemble_scripts.py holds the GPU writers to the record and to the same restatement."""
import csv
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_golden_model_ensemble import array_digest, np_argmax_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
KINDS = ("bin", "hela", "mc")


def load():
    with np.load(os.path.join(GOLD, "evalnet_ensemble.npz")) as d:
        return {k: d[k] for k in d.files}


def cases(d, kind):
    return sorted({k.split("_")[0] for k in d if k.startswith(kind) and k[len(kind)].isdigit()}, key=lambda c: int(c[len(kind):]))


def meta(d, c):
    thr, last, best, keep = d[c + "_meta"].tolist()
    return float(thr), int(last), int(best), int(keep)


def mean_models(s):
    """np.mean(axis=0) of the float32 stack written out: the sum in model order, each add rounded, one float32 divide"""
    acc = s[0].astype(F32)
    for n in range(1, s.shape[0]):
        acc = (acc + s[n]).astype(F32)
    return (acc / F32(s.shape[0])).astype(F32)


def select_rule(scores, thr, miou, count=None):
    """scores float32 [N,M,U] of one image -> (best index, best score float32, keep); only the first `count` candidates exist"""
    mean = mean_models(scores)
    m = mean.shape[0] if count is None else count
    if not miou:
        sc = mean[:m, 0].copy()
    else:
        k = mean.shape[1] // 2
        sc = np.zeros(m, F32)
        for c in range(m):
            s, cnt = None, 0
            for q in range(k):
                if mean[c, k + q] >= F32(0.5):                       # NaN compares false
                    s = mean[c, q] if s is None else F32(s + mean[c, q])
                    cnt += 1
            sc[c] = F32(s / F32(cnt)) if cnt else F32(0)
    best = int(np_argmax_rule(sc[None])[0])
    return best, sc[best], bool(sc[best] >= F32(thr))             # NaN compares false


def test_fixture_digests():
    with open(os.path.join(GOLD, "evalnet_ensemble_digests.json")) as f:
        want = json.load(f)["evalnet_ensemble"]
    d = load()
    assert sorted(d) == sorted(want)
    for k, v in d.items():
        assert array_digest(v) == want[k], k
    assert os.path.getsize(os.path.join(GOLD, "evalnet_ensemble.npz")) < 100 * 1024


@pytest.mark.skipif(not os.environ.get("IMK_REFERENCE"), reason="needs a reference checkout (IMK_REFERENCE)")
def test_fixture_regenerates(tmp_path):
    env = dict(os.environ, IMK_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(GOLD, "make_golden_evalnet_ensemble.py")], env=env)
    for name in ("evalnet_ensemble_digests.json", "reference_surface_evalnet_ensemble.json"):
        with open(tmp_path / name) as f, open(os.path.join(GOLD, name)) as g:
            assert json.load(f) == json.load(g), name


def test_cases_present():
    d = load()
    assert int(str(d["numpy"]).split(".")[0]) >= 2      # the float32 compare against a Python float is NumPy 2's
    ns, ms, thrs = set(), set(), set()
    for kind in KINDS:
        cs = cases(d, kind)
        assert len(cs) == 12
        for c in cs:
            thr, last, best, keep = meta(d, c)
            n, m, u = d[c + "_scores"].shape
            assert d[c + "_cands"].shape[0] == m and 0 <= best < m
            ns.add(n), ms.add(m), thrs.add(thr)
            assert u == (1 if kind == "bin" else 6 if kind == "hela" else u) and (kind != "mc" or u in (18, 70))
        assert any(np.isnan(d[c + "_scores"]).any() for c in cs), kind
        assert {meta(d, c)[1] for c in cs} == {0, 1} and {meta(d, c)[3] for c in cs} == {0, 1}, kind
    assert ns == {2, 3, 4} and ms == {5, 6, 10, 11} and thrs == {0.75, 0.62, 0.51, 0.453}
    assert sorted(t for t in thrs if float(F32(t)) != t) == [0.453, 0.51, 0.62]      # 0.75 is exact in float32, the others are not
    # a best score at the float32 threshold and one ulp to either side; ties; detection means at 0.5 and one ulp below; no class counting
    at = {"at": 0, "above": 0, "below": 0, "tie": 0, "half": 0, "lower": 0, "none": 0}
    for kind in KINDS:
        for c in cases(d, kind):
            thr, _, best, keep = meta(d, c)
            s = d[c + "_scores"]
            _, bs, _ = select_rule(s, thr, kind != "bin")
            t = F32(thr)
            at["at"] += bs == t
            at["above"] += bs == np.nextafter(t, F32(2))
            at["below"] += bs == np.nextafter(t, F32(0))
            if kind == "bin":
                sc = mean_models(s)[:, 0]
                at["tie"] += int((sc == bs).sum() > 1)
            else:
                k = s.shape[2] // 2
                det = mean_models(s)[:, k:]
                at["half"] += int((det == F32(0.5)).any())
                at["lower"] += int((det == np.nextafter(F32(0.5), F32(0))).any())
                at["none"] += int((~(det >= F32(0.5))).all())
    assert all(v > 0 for v in at.values()), at


def test_rules_restated_reproduce_the_reference():
    d = load()
    for kind in KINDS:
        for c in cases(d, kind):
            thr, last, best, keep = meta(d, c)
            got_best, _, got_keep = select_rule(d[c + "_scores"], thr, kind != "bin")
            assert (got_best, int(got_keep)) == (best, keep), c
            cand = d[c + "_cands"][best]
            if not keep:
                assert not any(k.startswith(c + "_") and k.split("_", 1)[1] in ("mask", "alive", "dead", "pos") for k in d), c
            elif kind == "hela":      # fed as 0/1 (mask / 255.0), written as plane * 255
                assert np.array_equal(d[c + "_alive"], cand[..., 0]) and np.array_equal(d[c + "_dead"], cand[..., 1]), c
                assert np.array_equal(d[c + "_pos"], cand[..., 2]), c
            else:
                assert np.array_equal(d[c + "_mask"], cand) and d[c + "_mask"].dtype == np.uint8, c


def test_a_missing_last_candidate_changes_nothing_before_it():
    """`counts`: the rule over the first M - 1 candidates is the rule of the stack without the last one"""
    d = load()
    for kind in KINDS:
        for c in cases(d, kind):
            s, thr = d[c + "_scores"], meta(d, c)[0]
            assert select_rule(s, thr, kind != "bin", s.shape[1] - 1)[::2] == select_rule(s[:, :-1], thr, kind != "bin")[::2], c


# ---- the EvalNet training-data writers ---------------------------------------------------------------------------------------------
TD_PLANES = ("alive", "dead", "mod_position")
TD_SHARE = (0.01, 0.01, 0.001)      # a plane counts from 1 % of the pixels on, the positions from 0.1 %


def pred_name(name, i):
    return f"{name[:-10]}___{i}_{name[-6:-4]}.png" if (i >= 10 and "aug" in name) else f"{name[:-4]}___{i}.png"


def _iou_binary(a, b):
    return np.logical_and(a, b).sum() / (np.logical_or(a, b).sum() + 1e-7)


def _classwise_iou(first, second, k):
    """class 0 starts at 1 where `first` has a class-0 pixel; a class present in `second` gets its IoU rounded to 4"""
    out = [0] * k
    if (first == 0).sum() > 0:
        out[0] = 1
    for cls in range(k):
        if (second == cls).any():
            union = np.logical_or(first == cls, second == cls).sum()
            if union > 0:
                out[cls] = round(np.logical_and(first == cls, second == cls).sum() / union, 4)
    return out


def _classwise_detection(mask, k):
    return [int((mask == cls).sum() > mask.size * 0.01) for cls in range(k)]


def training_data_rule(kind, names, gt, probs, steps, thr=0.5):
    """names in the order walked, gt uint8 [n,h,w] (hela: [n,h,w,3]), probs float32 [n,h,w,K] of the model, steps: the `i` of
    successive calls into one output directory -> (files "<sub>/<name>" in the order written and copied, per step the uint8 masks
    [n,h,w] (hela: [n,h,w,3]), the lines of labels.csv)"""
    k = probs.shape[-1]
    subs = TD_PLANES if kind == "hela" else ("masks",)
    img_sub = "brightfield" if kind == "hela" else "images"
    files, masks, text = [], [], io.StringIO()
    rows = csv.writer(text, delimiter=";")
    for i in steps:
        if kind == "mc":
            pred = np.argmax(probs, -1).astype(np.uint8)
        else:
            pred = ((probs > (thr if kind == "hela" else 0.5)) * 255).astype(np.uint8)
            pred = pred if kind == "hela" else pred[..., 0]
        masks.append(pred)
        for j, n in enumerate(names):
            pn = pred_name(n, i)
            files += [f"{sub}/{pn}" for sub in subs]
            if kind == "bin":
                rows.writerow((pn, round(_iou_binary(gt[j], pred[j]), 4)))
            elif kind == "hela":
                det = [int(np.count_nonzero(gt[j, ..., q]) >= gt[j, ..., q].size * TD_SHARE[q]) for q in range(3)]
                rows.writerow((pn, *[_iou_binary(gt[j, ..., q], pred[j, ..., q]) if det[q] else 0 for q in range(3)], *det))
            else:
                rows.writerow((pn, *_classwise_iou(gt[j], pred[j], k), *_classwise_detection(gt[j], k)))
        if i == 0:      # the labelled samples themselves; HeLa and multi-class: every row from the LAST image's masks, left over from above
            for n in names:
                files += [f"{sub}/{n}" for sub in (img_sub,) + subs]
                if kind == "bin":
                    rows.writerow((n, 1.0))
                elif kind == "hela":
                    det = [int(np.count_nonzero(gt[-1, ..., q]) >= gt[-1, ..., q].size * TD_SHARE[q]) for q in range(3)]
                    rows.writerow((n, *det, *det))
                else:
                    rows.writerow((n, *_classwise_iou(gt[-1], gt[-1], k), *_classwise_detection(gt[-1], k)))
    return files, masks, text.getvalue().split("\r\n")[:-1]


def test_training_data_rules_restated_reproduce_the_reference():
    d = load()
    names = d["td_names"].tolist()
    assert any("aug" in n for n in names) and any("aug" not in n for n in names)
    for kind in KINDS:
        key = "td" + kind
        files, masks, lines = training_data_rule(kind, names, d[key + "_gt"], d[key + "_probs"], (0, 11))
        assert ["/tout/" + f for f in files] == d[key + "_files"].tolist(), kind
        assert d[key + "_masks"].dtype == np.uint8 and np.array_equal(np.stack(masks), d[key + "_masks"]), kind
        assert lines == d[key + "_labels"].tolist(), kind
    assert "/tout/masks/l_001____11_03.png" in d["tdbin_files"].tolist() and "/tout/masks/l_001_aug_03___0.png" in d["tdbin_files"].tolist()
    for key, rgb in zip(("tdbin", "tdmc"), d["td_rgb"].tolist()):      # rgb: the model is given the channels reversed
        assert np.array_equal(d[key + "_io"][1], d[key + "_io"][0][..., ::-1] if rgb else d[key + "_io"][0]), key
    assert sorted(d["td_rgb"].tolist()) == [0, 1]


def test_training_data_cases_tell_the_rules_apart():
    """the record distinguishes what it pins: p == 0.5 is no foreground, the 1 % and 0.1 % shares, the leftover masks of the i == 0 loop,
    the class-0 prefill"""
    d = load()
    assert (d["tdbin_probs"] == F32(0.5)).any() and not d["tdbin_masks"][0][d["tdbin_probs"][..., 0] == F32(0.5)].any()
    gt = d["tdhela_gt"]
    n_pix = gt[0, ..., 0].size
    one = [(j, q) for j in range(len(gt)) for q in range(3) if np.count_nonzero(gt[j, ..., q]) == 1]
    assert {q for _, q in one} == {1, 2} and 0.001 * n_pix <= 1 < 0.01 * n_pix      # one pixel: a position, but no dead cell
    rows = [r.split(";") for r in d["tdhela_labels"].tolist()]
    assert rows[0][2] == "0" and rows[0][5] == "0" and rows[0][6] == "1"
    own = [[int(np.count_nonzero(gt[j, ..., q]) >= n_pix * TD_SHARE[q]) for q in range(3)] for j in range(len(gt))]
    assert own[1] != own[2] and all(r[4:] == [str(v) for v in own[2]] for r in rows[3:6])      # every i == 0 row: the last image's
    rows = [r.split(";") for r in d["tdmc_labels"].tolist()]
    assert rows[1][1] == "1" and not (d["tdmc_masks"][0][1] == 0).any() and (d["tdmc_gt"][1] == 0).sum() == 1      # the prefill stays
    assert rows[3][1:] == rows[4][1:] == rows[5][1:] and rows[3][1:] != rows[0][1:]


def circle_rule(positions, max_r=8, min_r=3):
    """the radius of every position's circle: the distance to the nearest other position // 4, 99 // 4 for a lone one, clamped"""
    out = []
    for x, y in positions:
        others = [np.hypot(x - u, y - v) for u, v in positions if (u, v) != (x, y)]
        dist = min(others) if len(positions) > 1 else 99
        out.append([x, y, max(min(int(dist // 4), max_r), min_r), 255, 255, 255, -1])
    return out


def test_hela_circle_rule_restated_reproduces_the_reference():
    d = load()
    several, lone = d["hela0_circles"], d["hela1_circles"]
    assert len(several) > 2 and len(lone) == 1 and lone[0, 2] == 8      # 99 // 4, clamped to the largest circle
    assert {3, 5, 6} <= set(several[:, 2].tolist())      # the lower clamp (10 // 4 = 2 -> 3) and two radii between the clamps
    for rec in (several, lone):
        assert circle_rule([tuple(p) for p in rec[:, :2].tolist()]) == rec.tolist()
