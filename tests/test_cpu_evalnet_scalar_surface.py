"""The import surface of the scalar-IoU multiclass EvalNet family: the eight names resolve from the repo-root `functions` module the
reference's scripts import from, with the reference's parameter names, order and defaults (read out of the reference into
tests/golden/reference_surface_evalnet_scalar.json by tests/golden/make_golden_evalnet_scalar.py: names and values only); and
get_evalnet builds the one-hot plan such a net needs.  No GPU."""
import inspect
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SURFACE = os.path.join(ROOT, "tests", "golden", "reference_surface_evalnet_scalar.json")
NAMES = ["compute_classwise_confluence", "create_augment_images_and_masks_with_evalnet_multiclass",
         "create_training_data_evalnet_im_multiclass", "create_training_data_evalnet_multiclass",
         "create_training_data_for_segnet_multiclass", "create_training_data_for_segnet_with_ensemble_multiclass",
         "get_confluence_binary", "train_evalnet_multiclass"]


def test_the_eight_names_keep_the_reference_signatures():
    import functions as top      # the repo-root module the scripts import from
    from inconsistencymasks_amd import functions as F
    with open(SURFACE) as f:
        rec = json.load(f)
    assert sorted(rec["signatures"]) == NAMES
    for f, want in rec["signatures"].items():
        got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(getattr(F, f)).parameters.values()]
        assert got[:len(want)] == want, f
        assert got[len(want):] in ([], [["seed", "None"]]), f      # the writers and the loop that draw random numbers take a seed
        assert getattr(top, f) is getattr(F, f), f


@pytest.mark.parametrize("alpha", [0.5, 2])
def test_get_evalnet_plans_a_one_hot_input(alpha):
    from inconsistencymasks_amd import evalnet as EV
    from oracle import evalnet_oracle as E
    p = EV.EvalPlan(64, 64, 3, 9, 1, alpha, False, True, True, b_onehot=True)
    assert (p.n_total, p.n_trainable) == E.count_params(3, 9, 1, alpha, False)
    assert p.b_onehot and p.cfg.normalize_b == 1 and not p.two_heads
    assert [l["name"] for l in p.layers] == [t[0] for t in E.layer_table(3, 9, 1, alpha, False)]
    sig = inspect.signature(EV.get_evalnet).parameters
    assert list(sig)[-3:] == ["seed", "device", "onehot_B"] and sig["onehot_B"].default is None and sig["normalize_B"].default is True
    for refusing in (EV.get_evalnet_miou, EV.get_evalnet_miou_v2):      # the mIoU constructors keep refusing a normalised one-hot stack
        with pytest.raises(NotImplementedError):
            refusing(128, 128, 3, 9, normalize_B=True)
