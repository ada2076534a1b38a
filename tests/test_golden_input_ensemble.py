"""The pin of the input-ensemble vote: tests/golden/make_golden_input_ensemble.py drives the REAL reference's
get_input_ensemble_prediction_* (functions.py:2127-2407) with fixed-prediction fake models and a numpy cv2 stub, and records a
sha256 of every array in tests/golden/input_ensemble_digests.json.  The committed fixture must be exactly what that regeneration
recorded; with a reference checkout on disk (IMK_REFERENCE) it is regenerated into a temporary directory and compared.  The host
draws of input_ensemble.py must reproduce the recorded ops, blur sizes and coins under the recorded seeds, and the rules the
kernels implement, restated in numpy, must reproduce every recorded output."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from test_golden_model_ensemble import array_digest, np_argmax_rule, vote_binary_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


def load():
    with np.load(os.path.join(GOLD, "input_ensemble.npz")) as d:
        return {k: d[k] for k in d.files}


def cases(d, kind):
    return sorted({k.split("_")[0] for k in d if k.startswith(kind) and k[len(kind)].isdigit()})


def ie():
    from inconsistencymasks_amd import input_ensemble
    return input_ensemble


def test_fixture_digests():
    with open(os.path.join(GOLD, "input_ensemble_digests.json")) as f:
        want = json.load(f)["input_ensemble"]
    d = load()
    assert sorted(d) == sorted(want)
    for k, v in d.items():
        assert array_digest(v) == want[k], k


@pytest.mark.skipif(not os.environ.get("IMK_REFERENCE"), reason="needs a reference checkout (IMK_REFERENCE)")
def test_fixture_regenerates(tmp_path):
    env = dict(os.environ, IMK_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(GOLD, "make_golden_input_ensemble.py")], env=env)
    with open(tmp_path / "input_ensemble_digests.json") as f, open(os.path.join(GOLD, "input_ensemble_digests.json")) as g:
        assert json.load(f) == json.load(g)


def test_cases_present():
    d = load()
    assert len(cases(d, "isic")) == 4 and len(cases(d, "hela")) == 4 and len(cases(d, "mc")) == 4
    assert sorted(len(d[c + "_ops"]) for c in cases(d, "isic")) == [3, 5, 7, 13]
    assert any(np.isnan(d[c + "_preds"]).any() for c in cases(d, "isic"))
    assert sorted({int(d[c + "_probs"].shape[-1]) for c in cases(d, "mc")}) == [3, 9, 35]


@pytest.mark.parametrize("op", range(13))
def test_op_then_inverse_is_identity(op):
    a = np.arange(7 * 7 * 2).reshape(7, 7, 2)
    m = ie()
    assert np.array_equal(m.restore_op(m.apply_op(a, op), op), a)
    if not m.is_quarter_turn(op):
        b = np.arange(5 * 9).reshape(5, 9)
        assert np.array_equal(m.restore_op(m.apply_op(b, op), op), b)


def test_op_order_is_the_reference_enumeration():
    m = ie()
    seen = [m.op_of(fh, fv, rot) for fh in range(2) for fv in range(2) for rot in range(1, 4)]
    assert seen == list(range(1, 13))
    a = np.arange(16).reshape(4, 4)
    assert np.array_equal(m.apply_op(a, m.op_of(1, 0, 2)), np.rot90(a[::-1], 2))
    assert np.array_equal(m.apply_op(a, m.op_of(0, 1, 1)), np.rot90(a[:, ::-1], -1))


def test_host_draws_match_the_reference():
    m, d = ie(), load()
    for c in cases(d, "isic"):
        ops = d[c + "_ops"]
        if len(ops) == 13:
            assert [q.op for q in m.all_views()] == list(range(13))
            continue
        random.seed(int(d[c + "_seed"]))
        views = m.draw_random_views(len(ops), 3, 25, (0.5, 1.5), (-25, 25), np_rng=np.random.RandomState(0))
        assert [q.op for q in views] == ops.tolist(), c
        assert [q.blur_k for q in views] == d[c + "_blur"].tolist(), c
        assert [q.bright_on for q in views] == d[c + "_coin"].tolist(), c
    for kind in ("hela", "mc"):
        for c in cases(d, kind):
            n = len(d[c + "_blur"]) - 1
            random.seed(int(d[c + "_seed"]))
            views = m.draw_chain_views(n, 1, 15, (0.7, 1.3), (-15, 15), np_rng=np.random.RandomState(0))
            assert [q.op for q in views] == [0] * (n + 1)
            assert [q.blur_k for q in views] == d[c + "_blur"].tolist(), c
            assert [q.bright_on for q in views] == d[c + "_coin"].tolist(), c


def test_rules_restated_reproduce_the_reference():
    m, d = ie(), load()
    for c in cases(d, "isic"):
        preds, ops, thr = d[c + "_preds"], d[c + "_ops"], d[c + "_thr"]
        votes = [m.restore_op(preds[v, ..., 0] >= F32(thr), int(op)) for v, op in enumerate(ops)]
        assert np.array_equal(np.where(np.all(votes, 0), 255, 0).astype(np.uint8), d[c + "_out"]), c
    for c in cases(d, "hela"):
        p = d[c + "_preds"]
        o = vote_binary_rule(p, d[c + "_thr"], bool(d[c + "_soft"]))
        assert np.array_equal(o[..., 0], d[c + "_alive"]) and np.array_equal(o[..., 1], d[c + "_dead"]), c
        assert np.array_equal(o[..., 2], d[c + "_pos"]), c
    for c in cases(d, "mc"):
        probs = d[c + "_probs"]
        soft = np_argmax_rule(probs.mean(0, dtype=F32)).astype(np.uint8)
        assert np.array_equal(soft, d[c + "_soft"]), c
        lab = np_argmax_rule(probs)
        major = np.apply_along_axis(lambda x: np.argmax(np.bincount(x)), 0, lab).astype(np.uint8)
        assert np.array_equal(major, d[c + "_major"]), c
