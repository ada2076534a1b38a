"""The rule of loss kind 4 (tests/dice_cases.py, a float64 numpy restatement of the reference's dice_loss, functions.py:162-184) checked
three ways without a GPU:
  * against the reference: tests/golden/make_golden_dice_loss.py ran the reference's own dice_loss on recorded arrays (tf.cast /
    reduce_sum / reduce_mean stubbed by numpy) and recorded a sha256 of every array; the committed fixture is exactly that, and the
    restatement reproduces every recorded loss -- 1e-12 relative against the float64 run, 1e-5 against the float32 run (float32 sums
    of at most 600 values in [0, 3]) -- while each of the three planted defects misses at least one case by more than 1e-3;
  * against torch autograd in float64: d loss / d p and d loss / d logit within 1e-12;
  * the Python surface: train_ISIC_2018 and train_hela take dice_loss (the function or its name) into fit() with loss kind 4 before
    touching any path, 'mse' stays kind 0, anything else is refused; train_multiclass, depth._loss_kind and the consistency trainers
    keep refusing dice_loss, the softmax trainer saying that the reference's form is the binary one."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dice_cases as DC  # noqa: E402
from test_golden_model_ensemble import array_digest  # noqa: E402

GOLD = os.path.join(HERE, "golden")


def load():
    with np.load(os.path.join(GOLD, "dice_loss.npz")) as d:
        return {k: d[k] for k in d.files}


def case_names(d):
    return sorted(k[:-len("_true")] for k in d if k.endswith("_true"))


def test_fixture_equals_what_the_reference_regeneration_recorded():
    with open(os.path.join(GOLD, "dice_loss_digests.json")) as f:
        rec = json.load(f)
    assert sorted(rec) == ["dice_loss"]
    d = load()
    assert sorted(d) == sorted(rec["dice_loss"])
    for k, a in d.items():
        assert array_digest(a) == rec["dice_loss"][k], k


def test_fixture_covers_the_issue_cases():
    d = load()
    names = case_names(d)
    assert {d[n + "_true"].shape[0] for n in names} >= {1, 3, 5}
    assert {d[n + "_true"].shape[3] for n in names} == {1, 3}
    assert any(not d[n + "_true"][i].any() for n in names for i in range(d[n + "_true"].shape[0])), "an all-zero target image"
    assert any((d[n + "_pred"] == 1.0).all() for n in names), "an all-one prediction"
    assert any(d[n + "_true"].max() == 3 for n in names), "targets containing 3"
    for n in names:
        assert d[n + "_true"].dtype == np.uint8 and d[n + "_pred"].dtype == np.float32 and d[n + "_true"].shape == d[n + "_pred"].shape
        assert d[n + "_loss32"].dtype == np.float32 and d[n + "_loss64"].dtype == np.float64


def test_restatement_reproduces_the_reference():
    d = load()
    for n in case_names(d):
        t, p = d[n + "_true"], d[n + "_pred"]
        got = DC.loss(t, p)
        l64, l32 = float(d[n + "_loss64"]), float(d[n + "_loss32"])
        print(f"{n}: restatement {got!r} reference float64 {l64!r} float32 {l32!r}")
        assert abs(got - l64) <= 1e-12 * max(abs(l64), 1e-3), n
        assert abs(got - l32) <= 1e-5 * max(abs(l32), 1e-2), n
        # the package's own host function is the float32 form
        from inconsistencymasks_amd import functions as F
        assert abs(float(F.dice_loss(t, p)) - l32) <= 1e-5 * max(abs(l32), 1e-2), n


@pytest.mark.parametrize("defect", sorted(DC.DEFECTS))
def test_fixture_tells_the_planted_defects_from_the_rule(defect):
    d = load()
    miss = [n for n in case_names(d) if not abs(DC.DEFECTS[defect](d[n + "_true"], d[n + "_pred"]) - float(d[n + "_loss64"])) <= 1e-3]
    assert miss, f"{defect} passes every case of the fixture"


def test_gradient_against_float64_autograd():
    torch = pytest.importorskip("torch")
    d = load()
    rng = np.random.default_rng(4)
    for n in case_names(d):
        t = d[n + "_true"].astype(np.float64)
        logit = torch.from_numpy(rng.normal(0, 2, t.shape)).requires_grad_(True)
        p = torch.sigmoid(logit)
        p.retain_grad()
        lv = DC.torch_loss(torch.from_numpy(t), p)
        lv.backward()
        pn = p.detach().numpy()
        assert abs(float(lv.detach()) - DC.loss(t, pn)) <= 1e-12
        assert np.abs(DC.dloss_dp(t, pn) - p.grad.numpy()).max() <= 1e-12, n
        assert np.abs(DC.dloss_dlogit(t, pn) - logit.grad.numpy()).max() <= 1e-12, n
        s = DC.sums(t, pn)
        assert s.shape == (t.shape[0], 3) and np.allclose(DC.dice_from_sums(s).mean(), 1.0 - float(lv.detach()), rtol=0, atol=1e-12)


# ---- surface --------------------------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def _dry(monkeypatch, F):
    """fit() records its loss kind and stops the trainer: nothing before it may touch a path"""
    seen = {}

    def fit(model, loader, steps_per_epoch, epochs, loss_kind, on_epoch_end=None, **kw):
        seen["kind"] = loss_kind
        raise _Stop()
    monkeypatch.setattr(F, "fit", fit)
    monkeypatch.setattr(F, "_train_shard", lambda files: files)
    monkeypatch.setattr(F, "_EpochLoader", lambda *a, **k: None)
    return seen


def _isic(F, loss):
    return F.train_ISIC_2018("no/such/dir", "no/v", "no/vm", "no/t", "no/tm", "no/u", "no/um", "m", "no/m.h5", None, loss, 1, 32, 32, 3,
                             "no/vp", "no/tp", "no/up")


def _hela(F, loss):
    return F.train_hela("no/such/dir", "no/v", "no/vg", "no/tg", "no/ug", "m", "no/m.h5", None, loss, 1, 32, 32, 1, "no/vp", "no/tp", "no/up")


@pytest.mark.parametrize("trainer", ["isic", "hela"])
def test_the_sigmoid_trainers_take_dice_loss(monkeypatch, trainer):
    from inconsistencymasks_amd import functions as F
    seen = _dry(monkeypatch, F)
    run = _isic if trainer == "isic" else _hela
    for loss, kind in ((F.dice_loss, 4), ("dice_loss", 4), ("mse", 0)):
        seen.clear()
        with pytest.raises(_Stop):
            run(F, loss)
        assert seen == {"kind": kind}, (loss, seen)
    for bad in ("mae", F.ignore_im_dice_loss_multiclass(), F.ignore_im_categorical_crossentropy, None):
        seen.clear()
        with pytest.raises(NotImplementedError):
            run(F, bad)
        assert not seen


def test_the_other_trainers_keep_refusing_dice_loss():
    from inconsistencymasks_amd import consistency as C
    from inconsistencymasks_amd import depth as D
    from inconsistencymasks_amd import functions as F
    for loss in (F.dice_loss, "dice_loss"):
        with pytest.raises(NotImplementedError, match="binary form"):
            F.train_multiclass(*([None] * 10), loss, *([None] * 9))
        with pytest.raises(NotImplementedError):
            D._loss_kind(loss, "train_depth_map")
        for want in (0, 1):
            with pytest.raises(NotImplementedError):
                C._loss_kind(loss, "train_ISIC_2018_consistency_loss", want)
    # the host function stays what it was
    t = np.zeros((2, 4, 4, 1), np.uint8)
    t[0, :2] = 1
    p = np.full((2, 4, 4, 1), 0.25, np.float32)
    want = 1 - np.mean([(2 * 2.0 + 1) / (8 + 4 + 1), 1 / (4 + 1)])
    assert abs(float(F.dice_loss(t, p)) - want) < 1e-6
