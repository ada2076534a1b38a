"""GPU tests of the input-ensemble writers (create_pseudo_labels_input_ensemble_*) and of the four script shims: the ISIC erosion
keep-filter, files independent of the batch size and of the rank count, and toy runs of ISIC_2018/07, HeLa/07, SUIM/08 and
Cityscapes/07.  The toy datasets and configs are the model-ensemble tests'."""
import os
import sys

import numpy as np
import pytest

from test_gpu_model_ensemble import (CITY_CONFIG, CITY_SETUP, CONFIG, HELA_CONFIG, HELA_SETUP, MULTI_CONFIG, MULTI_SETUP, ROOT, SETUP,
                                     _run_one_and_two_ranks, _same_png_tree, _toy_images, _toy_run)

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)
from inconsistencymasks_amd import functions as F  # noqa: E402


class Square:
    """fake model: every view gets a centred square of the width written in the image's pixels (D4-symmetric, so the 13 restored
    votes agree)"""

    def predict(self, x):
        m, h, w = x.shape[:3]
        k = int(x[0, 0, 0, 0])
        p = np.zeros((m, h, w, 1), np.float32)
        p[:, h // 2 - k // 2:h // 2 + (k + 1) // 2, w // 2 - k // 2:w // 2 + (k + 1) // 2] = 0.9
        return p


def test_isic_writer_erosion_keep_filter(tmp_path):
    src = tmp_path / "src"
    src.mkdir()
    for k in (0, 1, 2, 3, 4, 12):
        F.write_png(str(src / f"w{k:02d}.png"), np.full((32, 32, 3), k, np.uint8))
    out = tmp_path / "out"
    F.create_pseudo_labels_input_ensemble_ISIC_2018(Square(), str(src), str(out), 32, 32, 3, 2, True, False)
    assert sorted(os.listdir(out / "masks")) == ["w12.png"] == sorted(os.listdir(out / "images"))
    m = F.read_png(str(out / "masks" / "w12.png"), 1)
    assert int((m == 255).sum()) == 144


def _native(h, w, c, k, act):
    from inconsistencymasks_amd.unet import UNet
    return UNet(h, w, c, k, 0.5, act, seed=3)


@pytest.mark.parametrize("kind", ["isic", "hela", "multi"])
def test_writers_match_per_image_votes_and_ignore_batch_size(tmp_path, monkeypatch, kind):
    from inconsistencymasks_amd import input_ensemble as ie
    from inconsistencymasks_amd import vote
    import torch
    h = w = 32
    c, k, act = {"isic": (3, 1, "sigmoid"), "hela": (1, 3, "sigmoid"), "multi": (3, 4, "softmax")}[kind]
    model = _native(h, w, c, k, act)
    src = str(tmp_path / "src")
    _toy_images(src, 7, h, w, c, 11)
    trees = []
    for batch in ("3", "64"):
        monkeypatch.setenv("IMK_INFER_BATCH", batch)
        out = tmp_path / f"b{batch}" / "pl"
        if kind == "isic":
            F.create_pseudo_labels_input_ensemble_ISIC_2018(model, src, str(out), h, w, c, 3)
            subs, ch = ("images", "masks"), {"images": 3}
        elif kind == "hela":
            F.create_pseudo_labels_input_ensemble_hela(model, src, str(out), h, w, c, 3)
            subs, ch = ("brightfield", "alive", "dead", "mod_position"), {"mod_position": 3}
        else:
            F.create_pseudo_labels_input_ensemble_multiclass(model, src, str(out), h, w, c, 3)
            subs, ch = ("images", "masks"), {"images": 3}
        trees.append(out)
    _same_png_tree(trees[0], trees[1], subs, ch)
    # restatement: each image alone, its draws from (SEED, output directory, file name)
    for name in sorted(os.listdir(src)):
        img = F.read_png(os.path.join(src, name), c)
        r, nr = F._view_rngs(str(trees[0]), name)
        views = ie.draw_random_views(3, rng=r, np_rng=nr) if kind == "isic" else ie.draw_chain_views(3, rng=r, np_rng=nr)
        plan = ie.ViewPlan([views], chain=kind != "isic", restore=kind == "isic")
        x = torch.from_numpy(np.ascontiguousarray(img.reshape(1, h, w, c))).cuda()
        mode = vote.VOTE_SOFT if kind == "multi" else vote.VOTE_HARD
        lab = ie.ViewVote(model, kind != "multi").run(x, plan, 0.5, mode, kind == "isic")[0].cpu().numpy()
        if kind == "isic":
            if (trees[0] / "masks" / name).exists():
                assert np.array_equal(F.read_png(str(trees[0] / "masks" / name), 1)[..., 0], lab[0]), name
        elif kind == "hela":
            assert np.array_equal(F.read_png(str(trees[0] / "alive" / name), 1)[..., 0], lab[0]), name
            assert np.array_equal(F.read_png(str(trees[0] / "dead" / name), 1)[..., 0], lab[1]), name
        else:
            assert np.array_equal(F.read_png(str(trees[0] / "masks" / name), 1)[..., 0], lab), name


@pytest.mark.parametrize("ds", ["ISIC_2018", "SUIM", "Cityscapes", "HeLa"])
def test_input_ensemble_script_toy_run(tmp_path, ds):
    config, setup, script, tag, subs = {
        "ISIC_2018": (CONFIG, SETUP, "ISIC_2018/07_ISIC_2018_input_ensemble.py", "ISIC_2018", ("images", "masks")),
        "SUIM": (MULTI_CONFIG, MULTI_SETUP, "SUIM/08_SUIM_input_ensemble.py", "SUIM", ("images", "masks")),
        "Cityscapes": (CITY_CONFIG, CITY_SETUP, "Cityscapes/07_Cityscapes_input_ensemble.py", "CITYSCAPES", ("images", "masks")),
        "HeLa": (HELA_CONFIG, HELA_SETUP, "HeLa/07_HeLa_input_ensemble.py", "HELA", ("brightfield", "alive", "dead", "mod_position")),
    }[ds]
    seed = os.path.join(ROOT, "Cityscapes", "03_Cityscapes_subset.py") if ds == "Cityscapes" else None
    base, out = _toy_run(tmp_path, config, setup, os.path.join(ROOT, script), seed_script=seed)
    csvs = sorted(os.listdir(base / "csv"))
    assert not [f for f in csvs if f.startswith("mean_im_size_")], csvs
    for g in (0, 1):
        stem = f"{tag}_input_ensemble_1_n2_gen{g}"      # the toy runs set IM_NS=2
        assert f"results_{stem}.csv" in csvs, csvs
        models = sorted(os.listdir(base / "models"))
        assert f"{stem}_topK_1.h5" in models
        for split in ("val", "test", "train_unlabeled"):
            d = base / f"{split}_predictions" / "input_ensemble" / stem
            assert sorted(os.listdir(d)) == sorted(subs), (split, os.listdir(d))
        rows = [r.split(";") for r in (base / "csv" / f"results_{stem}.csv").read_text().strip().splitlines()]
        assert len(rows) == 3 and {r[0] for r in rows[1:]} == {f"{stem}_0", f"{stem}_1"}
        if ds == "HeLa":      # ranked by mean_cell_count_error_test (row index 6), ascending (HeLa/07_HeLa_input_ensemble.py:115)
            order = sorted(rows[1:], key=lambda r: float(r[6]))
            line = next(ln for ln in out.splitlines() if ln.startswith("[(") and f"{stem}_" in ln)
            assert line.index(f"'{order[0][0]}'") < line.index(f"'{order[1][0]}'") or float(order[0][6]) == float(order[1][6])
    unl = base / "train_unlabeled_predictions" / "input_ensemble" / f"{tag}_input_ensemble_1_n2_gen0" / subs[0]
    assert len(os.listdir(unl)) >= 16      # at least the labelled pairs copied in beside the pseudo-labels


def test_isic_input_ensemble_two_ranks_on_one_gpu(tmp_path):
    outs = _run_one_and_two_ranks(tmp_path, CONFIG, SETUP, os.path.join(ROOT, "ISIC_2018", "07_ISIC_2018_input_ensemble.py"),
                                  extra_env={"IM_NS": "3"})
    stem = "ISIC_2018_input_ensemble_1_n3_gen0"
    for split in ("val", "test", "train_unlabeled"):
        a, b = (outs[w] / f"{split}_predictions" / "input_ensemble" / stem for w in (1, 2))
        _same_png_tree(a, b, ("images", "masks"), {"images": 3})
