"""The consistency-loss baseline's host logic against what tests/golden/make_golden_consistency_loss.py recorded from the reference's
own functions (tests/golden/consistency_loss.npz; data only):

  * the (flip 0, flip 1, turn) draws of apply_random_flip_and_rotation map to the imk_views operation whose pixel permutation equals
    the recorded one, for all 16 combinations (the operations' definition: input_ensemble.apply_op = csrc/imk_pixmap.h);
  * the draw planner, on the recorded seed, makes the reference's `random` draws in its order: all flips / turns of the batch, then
    view 1's blur sizes and brightness coins, then view 2's;
  * the epoch loop, on the scripted losses, makes the recorded sequence of train_on_batch / evaluate / save / model(..., training=True)
    x 2 / apply_gradients calls with the recorded batch sizes, for the three training functions.
"""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "consistency_loss.npz")) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def C():
    from inconsistencymasks_amd import consistency
    return consistency


def test_d4_mapping_of_all_16_combinations(gold, C):
    from inconsistencymasks_amd.input_ensemble import apply_op
    idx = np.arange(16, dtype=np.uint8).reshape(4, 4)
    combos = [tuple(int(v) for v in c) for c in gold["d4_combos"]]
    assert len(set(combos)) == 16
    ops = set()
    for combo, perm in zip(combos, gold["d4_perm"]):
        op = C.d4_op(*combo)
        assert 0 <= op <= 12
        assert np.array_equal(apply_op(idx, op), perm), (combo, op)
        ops.add(op)
    assert len(ops) == 8          # the 16 draws are the 8 elements of D4, each twice


def test_draw_planner_follows_the_reference_order(gold, C):
    from inconsistencymasks_amd.input_ensemble import apply_op
    seed = int(gold["draws_seed"])
    random.seed(seed)
    views = C.plan_batch_draws(5, True, 3, 25, (0.5, 1.5), (-25, 25), np_rng=np.random.RandomState(0))
    idx = np.arange(16, dtype=np.uint8).reshape(4, 4)
    for b in range(5):
        assert views[b][0].op == views[b][1].op == C.d4_op(*gold["draws_geometry"][b])
        assert np.array_equal(apply_op(idx, views[b][0].op), gold["draws_perm"][b]), b
        for v, key in ((0, "draws_view1"), (1, "draws_view2")):
            assert [views[b][v].blur_k, views[b][v].bright_on] == gold[key][b].tolist(), (b, key)
    # the ordered cv2 calls say the same: 5 images' flips / turns first, then ten augmentations
    calls = gold["draws_calls"].tolist()
    n_geo = sum(int(g[0]) + int(g[1]) + int(g[2] > 0) for g in gold["draws_geometry"])
    assert all(k in (0, 1) for k, _ in calls[:n_geo]) and all(k in (2, 3) for k, _ in calls[n_geo:])
    # the multi-class form draws no geometry: the same seed then starts with view 1's blur draw
    random.seed(seed)
    plain = C.plan_batch_draws(5, False, 3, 25, (0.5, 1.5), (-25, 25), np_rng=np.random.RandomState(0))
    assert all(q.op == 0 for pair in plain for q in pair)


@pytest.mark.parametrize("kind", ["isic", "hela", "multi"])
def test_epoch_loop_reproduces_the_recorded_trace(gold, C, kind):
    want = gold["trace_" + kind].tolist()
    assert want[0] == "compile" and want[-4:] == ["load_model", "benchmark", "benchmark", "benchmark"]
    log, losses = [], gold["trace_losses"].tolist()
    seen = C.run_epochs(5, 7, 2, 2, 1,
                        labeled_step=lambda idx: log.append(f"train_on_batch:{len(idx)}"),
                        consistency_step=lambda idx: log.extend([f"call:{len(idx)}", f"call:{len(idx)}", "apply_gradients"]),
                        evaluate=lambda: (log.append("evaluate"), losses.pop(0))[1],
                        save=lambda: log.append("save"), np_rng=np.random.RandomState(1), log=lambda *a: None)
    assert log == want[1:-4]
    assert seen == gold["trace_losses"].tolist()
    saves = [i for i, s in enumerate(log) if s == "save"]
    evals = [i for i, s in enumerate(log) if s == "evaluate"]
    assert [evals.index(i - 1) for i in saves] == [0, 2]          # the first (below 100) and the third (0.4 < 0.5) evaluate saved
    assert {"isic": 6, "hela": 9, "multi": 6}[kind] == int(gold["trace_arity_" + kind])


def test_permutations_come_from_numpys_global_generator_labelled_first(C):
    got = []
    np.random.seed(5)
    C.run_epochs(5, 7, 2, 1, 1, lambda i: got.append(("l", list(i))), lambda i: got.append(("u", list(i))), lambda: 1.0, lambda: None,
                 log=lambda *a: None)
    np.random.seed(5)
    lab, unl = np.random.permutation(5), np.random.permutation(7)
    assert [i for k, b in got if k == "l" for i in b] == lab.tolist()
    assert [i for k, b in got if k == "u" for i in b] == unl.tolist()
