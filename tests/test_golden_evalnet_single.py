"""The pin of the single-EvalNet selection: tests/golden/make_golden_evalnet_single.py drives the REAL reference's
create_training_data_for_segnet_ISIC_2018 (functions.py:4991-5063) and create_training_data_by_evalnet_miou_for_segnet_multiclass
(:5583-5677) with a fixed-score fake EvalNet and numpy stand-ins for cv2 / os / shutil, and records a sha256 of every array in
tests/golden/evalnet_single_digests.json.  The committed fixture must be exactly what that regeneration recorded; with a reference checkout on
disk (IMK_REFERENCE) it is regenerated into a temporary directory and compared.

select_rule_gated below restates IMK_SELECT_CONF_GATED (include/imk.h) in numpy and must reproduce, for every recorded case, the index
np.argmax returned, the bits of every candidate's score as the reference handed them to np.argmax, the keep decision, the written files
and the written mask.  The binary cases pin the N = 1 case of IMK_SELECT_IOU (test_golden_evalnet_ensemble.select_rule) to the ISIC
writer.  One case cannot be recorded because the rule cannot produce it: a NaN detection value in a COUNTING class (and with it a
NaN score).  The value is part of the mean over the candidates that decides whether its class counts, so the class is gated out for
every candidate; the "nangate" cases pin exactly that.  tests/test_gpu_evalnet_select_gated.py holds the kernel to the same recorded
values and to the same restatement."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_golden_evalnet_ensemble import cases, mean_models, meta, select_rule
from test_golden_model_ensemble import array_digest, np_argmax_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
GATE = F32(0.03)
KINDS = ("bin", "gat")


def load():
    with np.load(os.path.join(GOLD, "evalnet_single.npz")) as d:
        return {k: d[k] for k in d.files}


def gated_scores(scores, count=None):
    """scores float32 [N,M,2K] of one image -> (the float32 score of each of the first `count` candidates, which classes count)"""
    mean = mean_models(scores)
    m = mean.shape[0] if count is None else count
    k = mean.shape[1] // 2
    det = mean[:m, k:]
    gate = det[0].copy()      # np.mean(axis=0) of the float32 [M,K]: the sum in candidate order, each add rounded, one float32 divide
    for c in range(1, m):
        gate = (gate + det[c]).astype(F32)
    gate = (gate / F32(m)).astype(F32)
    counting = [q for q in range(k) if gate[q] >= GATE]      # NaN compares false
    sc = np.zeros(m, F32)
    for c in range(m):
        s = None
        for q in counting:
            s = det[c, q] if s is None else F32(s + det[c, q])
        sc[c] = F32(s / F32(len(counting))) if counting else F32(0)
    return sc, counting


def select_rule_gated(scores, thr, count=None):
    """scores float32 [N,M,2K] of one image -> (best index, best score float32, keep); only the first `count` candidates exist"""
    sc, _ = gated_scores(scores, count)
    best = int(np_argmax_rule(sc[None])[0])
    return best, sc[best], bool(sc[best] >= F32(thr))             # NaN compares false


def rule(kind, scores, thr, count=None):
    return select_rule(scores, thr, False, count) if kind == "bin" else select_rule_gated(scores, thr, count)


def test_fixture_digests():
    with open(os.path.join(GOLD, "evalnet_single_digests.json")) as f:
        want = json.load(f)["evalnet_single"]
    d = load()
    assert sorted(d) == sorted(want)
    for k, v in d.items():
        assert array_digest(v) == want[k], k
    assert os.path.getsize(os.path.join(GOLD, "evalnet_single.npz")) < 100 * 1024


@pytest.mark.skipif(not os.environ.get("IMK_REFERENCE"), reason="needs a reference checkout (IMK_REFERENCE)")
def test_fixture_regenerates(tmp_path):
    env = dict(os.environ, IMK_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(GOLD, "make_golden_evalnet_single.py")], env=env)
    for name in ("evalnet_single_digests.json", "reference_surface_evalnet_single.json"):
        with open(tmp_path / name) as f, open(os.path.join(GOLD, name)) as g:
            assert json.load(f) == json.load(g), name
    with np.load(tmp_path / "evalnet_single.npz") as new:
        d = load()
        assert sorted(new.files) == sorted(d)
        for k in d:
            assert new[k].dtype == d[k].dtype and new[k].tobytes() == d[k].tobytes(), k


def test_cases_present():
    d = load()
    assert int(str(d["numpy"]).split(".")[0]) >= 2      # the float32 compare against a Python float is NumPy 2's
    assert len(cases(d, "bin")) == len(d["bin_variants"]) == 12 and len(cases(d, "gat")) == len(d["gat_variants"]) == 20
    for kind in KINDS:
        cs = cases(d, kind)
        assert {d[c + "_scores"].shape[1] for c in cs} == {5, 6, 10, 11}, kind
        assert {meta(d, c)[1] for c in cs} == {0, 1} and {meta(d, c)[3] for c in cs} == {0, 1}, kind
        for c in cs:
            n, m, u = d[c + "_scores"].shape
            assert n == 1 and d[c + "_cands"].shape[0] == m == len(d[c + "_given"]) and u == (1 if kind == "bin" else u), c
            assert m == (5 if m < 8 else 10) + meta(d, c)[1], c      # the last generation's mask is one more candidate
    assert {d[c + "_scores"].shape[2] for c in cases(d, "gat")} == {16, 70}      # K = 8 and 35
    # a best score at the float32 threshold and one ulp to either side, for an exact and an inexact threshold, in both kinds
    for kind, exact, inexact in (("bin", 0.75, 0.62), ("gat", 0.5, 0.453)):
        assert float(F32(exact)) == exact and float(F32(inexact)) != inexact
        seen = set()
        for c, v in zip(cases(d, kind), d[kind + "_variants"].tolist()):
            thr = meta(d, c)[0]
            bs = rule(kind, d[c + "_scores"], thr)[1]
            t = F32(thr)
            for name, val in (("at", t), ("above", np.nextafter(t, F32(2))), ("below", np.nextafter(t, F32(0)))):
                if v == name:
                    assert bs == val and thr in (exact, inexact), c
                    seen.add((name, thr))
        assert seen == {(n, t) for n in ("at", "above", "below") for t in (exact, inexact)}, kind
    # ties, NaN (binary: the first NaN wins and nothing is kept)
    for c, v in zip(cases(d, "bin"), d["bin_variants"].tolist()):
        s = d[c + "_scores"][0, :, 0]
        if v == "tie":
            assert (s == s[meta(d, c)[2]]).sum() > 1 and meta(d, c)[2] == int(np.argmax(s == s.max())), c
        if v == "nan":
            assert np.isnan(s).sum() >= 1 and meta(d, c)[2] == int(np.argmax(np.isnan(s))) and meta(d, c)[3] == 0, c
    seen = set()
    for c, v in zip(cases(d, "gat"), d["gat_variants"].tolist()):
        s, (thr, _, best, keep) = d[c + "_scores"], meta(d, c)
        k = s.shape[2] // 2
        det = s[0, :, k:]
        sc, counting = gated_scores(s)
        gate = np.mean(det, axis=0)
        seen.add(v)
        if v == "gate_at":      # the class at exactly 0.03f counts, alone: without it candidate 0 would win with 0.0
            assert gate[1] == GATE and counting == [1] and best == int(np.argmax(det[:, 1])) != 0, c
        if v == "gate_below":      # one ulp below: it does not count, and counting it would choose differently
            assert gate[2] == np.nextafter(GATE, F32(0)) and counting == [1], c
            assert int(np.argmax(det[:, 1] + det[:, 2])) != best == int(np.argmax(det[:, 1])), c
        if v in ("none", "none0"):
            assert counting == [] and best == 0 and keep == int(v == "none0") and thr == (0.0 if v == "none0" else 0.5), c
        if v == "nangate":      # the NaN makes its class's mean NaN: gated out for every candidate; no score is NaN
            assert np.isnan(det[:, 1]).sum() == 1 and np.isnan(gate[1]) and counting == [2] and not np.isnan(sc).any() and keep == 1, c
            assert np.nanargmax(det[:, 1] + det[:, 2]) != best, c
        if v == "tie":
            assert (sc == sc[best]).sum() == 2 and best == int(np.argmax(sc == sc.max())), c
        if v == "contra":      # IMK_SELECT_MIOU, which reads the iou half, chooses another candidate
            assert len(counting) == k and select_rule(s, thr, True)[0] != best, c
    assert seen == {"rand", "gate_at", "gate_below", "none", "none0", "nangate", "tie", "at", "above", "below", "contra"}


def test_rules_restated_reproduce_the_reference():
    d = load()
    for kind in KINDS:
        for c in cases(d, kind):
            thr, last, best, keep = meta(d, c)
            s = d[c + "_scores"]
            got_best, got_score, got_keep = rule(kind, s, thr)
            assert (got_best, int(got_keep)) == (best, keep), c
            # every candidate's score, bit for bit, as the reference handed it to np.argmax (float32 values; Python's 0.0 where no class counts)
            given = d[c + "_given"]
            want = s[0, :, 0] if kind == "bin" else gated_scores(s)[0]
            assert np.array_equal(given.astype(F32).astype(np.float64), given, equal_nan=True), c
            assert given.astype(F32).tobytes() == want.tobytes() and F32(got_score).tobytes() == given.astype(F32)[best].tobytes(), c
            name = ("ISIC_%07d.png" if kind == "bin" else "d_%d.png") % int(c[3:])
            if keep:
                assert d[c + "_files"].tolist() == [f"/out/images/{name}", f"/out/masks/{name}"], c
                assert np.array_equal(d[c + "_mask"], d[c + "_cands"][best]) and d[c + "_mask"].dtype == np.uint8, c
            else:
                assert d[c + "_files"].tolist() == [""] and c + "_mask" not in d, c


def test_single_evalnet_iou_is_the_n1_case_of_the_ensemble_rule():
    """ISIC: np.argmax of the one net's [M,1] output and `pred[best] >= threshold` = IMK_SELECT_IOU with N = 1 (the mean of one value
    is the value: x / 1.0f is exact)"""
    d = load()
    for c in cases(d, "bin"):
        s = d[c + "_scores"]
        assert mean_models(s).tobytes() == s[0].tobytes(), c
        assert select_rule(s, meta(d, c)[0], False)[::2] == (meta(d, c)[2], bool(meta(d, c)[3])), c


def test_a_missing_last_candidate_changes_neither_gate_nor_choice():
    """`counts`: the rule over the first M - 1 candidates is the rule of the stack without the last one -- the gate included"""
    d = load()
    changed = 0
    for c in cases(d, "gat"):
        s, thr = d[c + "_scores"], meta(d, c)[0]
        m = s.shape[1]
        a, b = select_rule_gated(s, thr, m - 1), select_rule_gated(s[:, :-1], thr)
        assert a[0] == b[0] and F32(a[1]).tobytes() == F32(b[1]).tobytes() and a[2] == b[2], c
        garbage = np.concatenate([s[:, :-1], np.full_like(s[:, -1:], np.nan)], 1)
        g = select_rule_gated(garbage, thr, m - 1)
        assert g[0] == a[0] and F32(g[1]).tobytes() == F32(a[1]).tobytes(), c
        changed += gated_scores(s)[1] != gated_scores(s, m - 1)[1]
    assert changed > 0, "in some case the last candidate must decide whether a class counts"
