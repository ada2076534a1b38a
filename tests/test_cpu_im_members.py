"""The IM over per-image sub-ensembles on the CPU: tests/im_members_cases.py (the rule of imk_im_binary_members /
imk_im_multiclass_members in numpy) against tests/golden/im_members.npz, which tests/golden/make_golden_im_members.py recorded from the
reference's own get_im_prediction_binary / _hela / _multiclass on the sub-list of models of every image.  The three planted defects
(non-members counted, the pool size instead of the member count, model 0 as the anchor where it is no member) each have to miss a
record: a fixture that could not tell them from the rule would pin nothing."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import im_members_cases as MC  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "im_members.npz")


@pytest.fixture(scope="module")
def cases():
    return MC.load(GOLDEN)


def test_fixture_holds_arrays_only_and_covers_the_cases(cases):
    assert os.path.getsize(GOLDEN) < 200 * 1024
    with np.load(GOLDEN, allow_pickle=False) as d:
        for key in d.files:
            assert d[key].dtype.kind in "fuiUb", (key, d[key].dtype)
    assert {c["kind"] for c in cases} == {"binary", "hela", "multi"}
    assert {c["preds"].shape[0] for c in cases} == {2, 5, 10, 16}
    assert {c["preds"].shape[-1] for c in cases if c["kind"] == "multi"} == {3, 9, 35}
    half = np.float32(0.5)
    flat = np.concatenate([c["preds"].reshape(-1) for c in cases if c["kind"] != "multi"])
    for v in (half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0))):
        assert (flat == v).any(), v
    assert np.isnan(flat).any() and any(np.isnan(c["preds"]).any() for c in cases if c["kind"] == "multi")
    seen = set()
    for c in cases:
        n = c["preds"].shape[0]
        pool = (1 << n) - 1
        for word in c["words"]:
            word = int(word)
            cnt = bin(word & pool).count("1")
            seen |= {"one"} if cnt == 1 else set()
            seen |= {"all"} if word & pool == pool else set()
            seen |= {"highest"} if word & pool == 1 << (n - 1) else set()
            seen |= {"more than 8"} if cnt > 8 else set()
            seen |= {"zero"} if word == 0 else set()
            seen |= {"above the pool"} if word & ~pool else set()
        w = [int(v) & pool for v in c["words"]]
        if any(a and b and not (a & b) for a, b in zip(w, w[1:])):
            seen.add("disjoint neighbours")
    assert seen == {"one", "all", "highest", "more than 8", "zero", "above the pool", "disjoint neighbours"}


def test_restatement_reproduces_every_record(cases):
    for c in cases:
        assert MC.check_case(c) == [], c["name"]


@pytest.mark.parametrize("defect", MC.DEFECTS)
def test_planted_defect_misses_a_record(cases, defect):
    assert any(MC.check_case(c, defect) for c in cases), defect


def test_all_members_is_the_whole_ensemble_rule(cases):
    """with every bit set the rule is pred_masks_to_im_binary / _multiclass over the whole stack, blocking included"""
    for c in cases:
        n = c["preds"].shape[0]
        words = np.full(c["preds"].shape[1], (1 << n) - 1, np.uint32)
        if c["kind"] == "multi":
            final, im, size, pres = MC.multiclass(c["preds"], words, True)
            lab = np.argmax(c["preds"], -1)
            agree = (lab == lab[0:1]).all(0)
            assert np.array_equal(final, np.where(agree, lab[0], 0)) and np.array_equal(im, np.where(agree, 0, 255))
            assert np.array_equal(size, (~agree).sum((1, 2))) and pres.any(2).all()
        else:
            ge = c["kind"] == "hela"
            masks, im, im_size, pred_size = MC.binary(c["preds"], words, 0.5, ge, True)
            with np.errstate(invalid="ignore"):
                s = ((c["preds"] >= np.float32(0.5)) if ge else (c["preds"] > np.float32(0.5))).sum(0).transpose(0, 3, 1, 2)
            mx = (s != 0) & (s != n)
            assert np.array_equal(im > 0, mx.any(1)) and np.array_equal(masks > 0, (s == n) & ~mx.any(1)[:, None])
            assert np.array_equal(im_size, mx.sum((2, 3))) and np.array_equal(pred_size, (s == n).sum((2, 3)))
