"""GPU tests of the noisy-student writers (create_pseudo_labels_noisy_student_*) and of the four script shims: files independent of
the batch size and of the rank count, each file equal to its image run alone with the draws of (SEED, output directory, file name),
and toy runs of ISIC_2018/08, HeLa/08, SUIM/09 and Cityscapes/08.  The toy datasets and configs are the model-ensemble tests'."""
import os
import sys

import numpy as np
import pytest

from test_gpu_model_ensemble import (CITY_CONFIG, CITY_SETUP, CONFIG, HELA_CONFIG, HELA_SETUP, MULTI_CONFIG, MULTI_SETUP, ROOT, SETUP,
                                     _run_one_and_two_ranks, _same_png_tree, _toy_images, _toy_run)

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)
from inconsistencymasks_amd import functions as F  # noqa: E402

STRENGTH = dict(brightness_range_alpha=(0.7, 1.3), brightness_range_beta=(-15, 15), max_blur=3, max_noise=15, free_rotation=True)


def _native(h, w, c, k, act):
    from inconsistencymasks_amd.unet import UNet
    return UNet(h, w, c, k, 0.5, act, seed=3)


@pytest.mark.parametrize("kind", ["isic", "hela", "multi"])
def test_writers_match_per_image_passes_and_ignore_batch_size(tmp_path, monkeypatch, kind):
    from inconsistencymasks_amd import noisy_student as ns
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
            F.create_pseudo_labels_noisy_student_ISIC_2018(model, h, w, c, src, str(out), True, **STRENGTH)
            subs, ch = ("images", "masks"), {"images": 3}
        elif kind == "hela":
            F.create_pseudo_labels_noisy_student_hela(model, h, w, c, src, str(out), **STRENGTH)
            subs, ch = ("brightfield", "alive", "dead", "mod_position"), {"mod_position": 3}
        else:
            F.create_pseudo_labels_noisy_student_multiclass(model, h, w, c, src, str(out), True, **STRENGTH)
            subs, ch = ("images", "masks"), {"images": 3}
        trees.append(out)
    _same_png_tree(trees[0], trees[1], subs, ch)
    # restatement: each image alone, its draws from (SEED, output directory, file name)
    tl = ns.TeacherLabel(model, kind != "multi")
    turned = 0
    for name in sorted(os.listdir(src)):
        img = F.read_png(os.path.join(src, name), c)
        q = ns.draw_for(F._view_rngs(str(trees[0]), name), **STRENGTH)
        turned += q.rot in (1, 3)
        x = torch.from_numpy(np.ascontiguousarray(img.reshape(1, h, w, c))).cuda()
        bgr = x.flip(-1).contiguous() if c == 3 else x
        o, lab = tl.run(x, bgr, ns.pack_params([q]), 0.5, kind == "hela")
        o = (o.flip(-1) if c == 3 else o)[0].cpu().numpy()
        lab = lab[0].cpu().numpy()
        if kind == "hela":
            stem = ns.aug_name(name)
            assert stem.endswith("_aug.png") and not (trees[0] / "alive" / name).exists()
            assert np.array_equal(F.read_png(str(trees[0] / "brightfield" / stem), 1), o), name
            assert np.array_equal(F.read_png(str(trees[0] / "alive" / stem), 1)[..., 0], lab[0]), name
            assert np.array_equal(F.read_png(str(trees[0] / "dead" / stem), 1)[..., 0], lab[1]), name
            pos = F.read_png(str(trees[0] / "mod_position" / stem), 3)
            assert np.array_equal(pos, F._hela_vote_positions(lab[2], 8, 3)), name      # circles drawn in the moved frame
        else:
            assert np.array_equal(F.read_png(str(trees[0] / "images" / name), 3), o), name
            assert np.array_equal(F.read_png(str(trees[0] / "masks" / name), 1)[..., 0], lab[0] if kind == "isic" else lab), name
    assert turned > 0


@pytest.mark.parametrize("ds", ["ISIC_2018", "SUIM", "Cityscapes", "HeLa"])
def test_noisy_student_script_toy_run(tmp_path, ds):
    config, setup, script, tag, subs = {
        "ISIC_2018": (CONFIG, SETUP, "ISIC_2018/08_ISIC_2018_noisy_student.py", "ISIC_2018", ("images", "masks")),
        "SUIM": (MULTI_CONFIG, MULTI_SETUP, "SUIM/09_SUIM_noisy_student.py", "SUIM", ("images", "masks")),
        "Cityscapes": (CITY_CONFIG, CITY_SETUP, "Cityscapes/08_Cityscapes_noisy_student.py", "CITYSCAPES", ("images", "masks")),
        "HeLa": (HELA_CONFIG, HELA_SETUP, "HeLa/08_HeLa_noisy_student.py", "HELA", ("brightfield", "alive", "dead", "mod_position")),
    }[ds]
    seed = os.path.join(ROOT, "Cityscapes", "03_Cityscapes_subset.py") if ds == "Cityscapes" else None
    base, out = _toy_run(tmp_path, config, setup, os.path.join(ROOT, script), seed_script=seed)
    csvs = sorted(os.listdir(base / "csv"))
    assert not [f for f in csvs if f.startswith("mean_im_size_")], csvs
    assert not [f for f in csvs if "_n2_" in f and "noisy_student" in f], csvs      # IM_NS is set by the toy run and must not matter
    models = sorted(os.listdir(base / "models"))
    for g in (0, 1):
        stem = f"{tag}_noisy_student_1_gen{g}"
        assert f"results_{stem}.csv" in csvs, csvs
        assert f"{stem}_topK_1.h5" in models, models
        d = base / "train_unlabeled_predictions" / "noisy_student" / stem
        assert sorted(os.listdir(d)) == sorted(subs), os.listdir(d)
        for split in ("val", "test"):      # no pseudo-labels for val / test: only the candidates' own prediction directories
            assert not (base / f"{split}_predictions" / "noisy_student" / stem).exists(), split
        lines = (base / "csv" / f"results_{stem}.csv").read_text().strip().splitlines()
        rows = [r.split(";") for r in lines]
        assert len(rows) == 3 and {r[0] for r in rows[1:]} == {f"{stem}_0", f"{stem}_1"}
        if ds == "HeLa":      # this approach's header abbreviates; ranked by index 6 ascending (HeLa/08_HeLa_noisy_student.py:130, 143)
            assert rows[0] == ["modelname", "mIoU_val", "mIoU_ad_val", "mcce_val", "mIoU_test", "mIoU_ad_test", "mcce_test",
                               "mIoU_unlabeled", "mIoU_ad_unlabeled", "mcce_unlabeled"]
            order = sorted(rows[1:], key=lambda r: float(r[6]))
            line = next(ln for ln in out.splitlines() if ln.startswith("[(") and f"{stem}_" in ln)
            assert line.index(f"'{order[0][0]}'") < line.index(f"'{order[1][0]}'") or float(order[0][6]) == float(order[1][6])
        elif ds == "ISIC_2018":
            assert rows[0][:3] == ["modelname", "mIoU_val", "mIoU_test"]
        else:
            assert rows[0][:2] == ["modelname", "mPA_val"] and rows[0][4] == "mIoU_val"
    # gen 1's teacher is gen 0's topK_1: the generation-0 checkpoint exists before generation 1 is labelled, and generation 1 ran
    assert f"{tag}_noisy_student_1_gen0_topK_1.h5" in models and f"{tag}_noisy_student_1_gen1_topK_1.h5" in models
    unl = base / "train_unlabeled_predictions" / "noisy_student" / f"{tag}_noisy_student_1_gen0" / subs[0]
    names = os.listdir(unl)
    assert len(names) >= 16      # at least the labelled pairs copied in beside the pseudo-labels
    if ds == "HeLa":
        assert any(n.endswith("_aug.png") for n in names) and any(not n.endswith("_aug.png") for n in names)


def test_isic_noisy_student_two_ranks_on_one_gpu(tmp_path):
    outs = _run_one_and_two_ranks(tmp_path, CONFIG, SETUP, os.path.join(ROOT, "ISIC_2018", "08_ISIC_2018_noisy_student.py"))
    stem = "ISIC_2018_noisy_student_1_gen0"
    a, b = (outs[w] / "train_unlabeled_predictions" / "noisy_student" / stem for w in (1, 2))
    _same_png_tree(a, b, ("images", "masks"), {"images": 3})
