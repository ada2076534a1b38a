"""GPU tests of the single-EvalNet selection writers (create_training_data_for_segnet_ISIC_2018,
create_training_data_by_evalnet_miou_for_segnet_multiclass) and of the single-EvalNet and full-dataset scripts on toy data.

The writers run on toy directories of 64x64 and 64x128 images (7 images, 5 candidate directories, a last generation that kept the even
images, batches of 3); their file sets and bytes are compared with the pinned rules (tests/test_golden_evalnet_single.py:
select_rule_gated; tests/test_golden_evalnet_ensemble.py: select_rule with N = 1) restated in numpy on the SAME model's predict outputs,
image by image, as the reference walks them -- once with a native EvalNet (the fused call), once with a `.predict`-only model (the
unfused route) whose scores gate a class out."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from test_golden_evalnet_ensemble import select_rule
from test_golden_evalnet_single import gated_scores, select_rule_gated
from test_gpu_evalnet_ensemble_scripts import EVALNET_EXTRA, _candidate_stack, _evalnets, _make_set
from test_gpu_model_ensemble import CONFIG, MULTI_CONFIG, MULTI_SETUP, ROOT, SETUP

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)
from inconsistencymasks_amd import evalnet_functions as EF  # noqa: E402
from inconsistencymasks_amd import functions as F  # noqa: E402


class PredictOnly:
    """a Keras-like model with .predict alone: scores computed from the masks it is given, row by row.  Binary: [M,1].  Multi-class (it
    is handed the one-hot stack): [iou [M,K], detection [M,K]] with the last class's detection at 0.01 -- gated out -- and iou values that
    rank the candidates the other way round."""

    def __init__(self, k):
        self.k, self.calls = k, 0

    def predict(self, x):
        images, masks = np.asarray(x[0]), np.asarray(x[1])
        assert images.dtype == np.uint8 and len(images) == len(masks)
        self.calls += 1
        light = images.reshape(len(images), -1).mean(1) / 255.0
        if self.k == 1:
            assert masks.shape[-1] == 1
            share = (masks.reshape(len(masks), -1) > 0).mean(1)
            return (0.2 + 0.6 * np.abs(np.sin(37.0 * share + light)))[:, None].astype(np.float32)
        assert masks.shape[-1] == self.k and set(np.unique(masks).tolist()) <= {0, 1}
        share = masks.reshape(len(masks), -1, self.k).mean(1)
        det = (0.1 + 0.8 * np.abs(np.sin(23.0 * share + light[:, None]))).astype(np.float32)
        det[:, -1] = np.float32(0.01)
        return [(1.0 - det).astype(np.float32), det]


@pytest.mark.parametrize("native", [True, False], ids=["native", "predict_only"])
@pytest.mark.parametrize("kind,h,w,k,rgb", [("isic", 64, 64, 1, True), ("isic", 64, 128, 1, False), ("multi", 64, 64, 4, False),
                                            ("multi", 64, 128, 5, True)])
def test_single_evalnet_writers_match_the_restated_rule(tmp_path, monkeypatch, kind, h, w, k, rgb, native):
    monkeypatch.setattr(EF, "SELECT_BATCH", 3)      # several batches, with and without a last-generation candidate in one batch
    n_dirs = 5
    names, img_dir, dirs, last = _make_set(str(tmp_path), kind, h, w, k, 7, n_dirs, 3)
    net = _evalnets(kind, h, w, k, 1)[0] if native else PredictOnly(k)

    contradicted = []

    def expected(thr, with_last):      # the restated rule on the same model's predict outputs, image by image
        exp = {}
        for n in names:
            img = F.read_png(os.path.join(img_dir, n), 3)
            if not rgb:
                img = img[..., ::-1]
            stack = _candidate_stack(kind, h, w, k, n, dirs, last, with_last)      # `last` was copied into the output first
            m = len(stack)
            rep = np.repeat(img[None], m, 0)
            if kind == "isic":
                sc = np.asarray(net.predict([rep, stack[..., None]]), np.float32)[None]
                best, score, keep = select_rule(sc, thr, False)
            else:
                xb = stack if native else (stack[..., None] == np.arange(k)).astype(np.uint8)
                sc = np.concatenate(net.predict([rep, xb]), 1).astype(np.float32)[None]
                best, score, keep = select_rule_gated(sc, thr)
                if not native:
                    assert gated_scores(sc)[1] == list(range(k - 1)), n      # the last class is gated out
                    contradicted.append(select_rule(sc, thr, True)[0] != best)      # where the iou units would choose differently
            exp[n] = (m, best, float(score), keep, stack[best])
        return exp

    scores = sorted(v[2] for v in expected(0.0, False).values())
    thr = (scores[3] + scores[4]) / 2 if scores[3] != scores[4] else scores[3]      # about half of the images pass
    assert native or kind == "isic" or any(contradicted), "the predict-only model's iou half must contradict its detection half somewhere"
    for with_last in (False, True):
        out = str(tmp_path / f"out{int(with_last)}")
        args = (net, h, w, 3) + ((k,) if kind == "multi" else ()) + (img_dir, dirs, out, thr) + ((last,) if with_last else ())
        if kind == "isic":
            F.create_training_data_for_segnet_ISIC_2018(*args, rgb=rgb)
        else:
            F.create_training_data_by_evalnet_miou_for_segnet_multiclass(*args, rgb=rgb)
        exp = expected(thr, with_last)
        assert {v[0] for v in exp.values()} == ({n_dirs, n_dirs + 1} if with_last else {n_dirs})
        kept = {n for n, v in exp.items() if v[3]}
        assert 0 < len(kept) < len(names), "the threshold must split the toy set"
        before = set(os.listdir(os.path.join(last, "images"))) if with_last else set()
        assert set(os.listdir(os.path.join(out, "images"))) == kept | before
        assert set(os.listdir(os.path.join(out, "masks"))) == kept | before
        for n in kept | before:
            src = os.path.join(img_dir if n in kept else os.path.join(last, "images"), n)
            assert open(os.path.join(out, "images", n), "rb").read() == open(src, "rb").read(), n      # the image file, copied
            if n not in kept:      # the last generation's pair stays as it was copied
                assert open(os.path.join(out, "masks", n), "rb").read() == open(os.path.join(last, "masks", n), "rb").read(), n
            else:
                assert np.array_equal(F.read_png(os.path.join(out, "masks", n), 1)[..., 0], exp[n][4]), n


# ---- the scripts on toy data ---------------------------------------------------------------------------------------------------------
CANDIDATE_DIRS = """
import shutil
tag, runid = {tag!r}, 1
base = getattr(paths, tag + "_BASE_DIR")
unl = getattr(paths, tag + "_TRAIN_UNLABELED_MASKS_DIR")
for j in range(10):      # the `subset` models' predictions of the unlabeled set: the ground truth shifted by 2 j pixels
    d = os.path.join(base, "train_unlabeled_predictions", "subset", f"{{tag}}_subset_{{runid}}_{{j}}")
    os.makedirs(d, exist_ok=True)
    for n in os.listdir(unl):
        F.write_png(os.path.join(d, n), np.roll(F.read_png(os.path.join(unl, n), 1)[..., 0], 2 * j, 1))
for sub in ("images", "masks"):      # TRAIN_FULL: the labelled and the unlabeled set together
    os.makedirs(os.path.join(getattr(paths, tag + "_TRAIN_FULL_DIR"), sub))
    for split in ("TRAIN_LABELED", "TRAIN_UNLABELED"):
        src = os.path.join(getattr(paths, tag + "_" + split + "_DIR"), sub)
        for n in os.listdir(src):
            shutil.copy(os.path.join(src, n), os.path.join(getattr(paths, tag + "_TRAIN_FULL_DIR"), sub, split[6] + n))
"""


def _toy(tmp_path, ds, env):
    config, setup = (CONFIG, SETUP) if ds == "ISIC_2018" else (MULTI_CONFIG, MULTI_SETUP)
    config = config.replace("TOP_Ks = 2\n", "TOP_Ks = 2\n" + EVALNET_EXTRA) + "ALPHA_EVALNET = 0.5\nMIN_THRESHOLD = 0.3\nMAX_THRESHOLD = 0.35\n"
    base = tmp_path / "data"
    cfg = tmp_path / "config.ini"
    cfg.write_text(config.format(base=base))
    env = {**os.environ, "IM_CONFIG": str(cfg), "IM_RUNIDS": "1", "IM_CANDIDATES": "0,1", **env}
    subprocess.run([sys.executable, "-c", setup.format(root=ROOT) + CANDIDATE_DIRS.format(tag=ds)], env=env, check=True, cwd=tmp_path)
    return base, env


def _rows(path):
    with open(path, newline="") as f:
        return [r for r in csv.reader(f, delimiter=";")]


@pytest.mark.parametrize("ds", ["ISIC_2018", "SUIM"])
def test_single_evalnet_script_toy_run(tmp_path, ds):
    base, env = _toy(tmp_path, ds, {"IM_GENS": "0,1"})
    script = "ISIC_2018/10_ISIC_2018_evalnet.py" if ds == "ISIC_2018" else "SUIM/11_SUIM_evalnet_miou.py"
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)], env=env, cwd=tmp_path, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    isic = ds == "ISIC_2018"
    csvs, models = sorted(os.listdir(base / "csv")), sorted(os.listdir(base / "models"))
    ev_name = "ISIC_2018_evalnet_1" if isic else "SUIM_evalnet_miou_1"
    seg = "ISIC_2018_segnet_1" if isic else "SUIM_segnet_miou_1"
    # the EvalNet stage: BOTH `subset` models write train and val data (no first-three limit to see here, but both splits from both)
    for split, n_src in (("train", 16), ("val", 8)):
        rows = _rows(base / "evalnet" / "run_1" / split / "labels.csv")
        assert len(rows) == 3 * n_src and len(rows[0]) == (2 if isic else 7), split      # two models' predictions + the ground truth
        assert sum("___0.png" in r[0] for r in rows) == n_src and sum("___1.png" in r[0] for r in rows) == n_src
    assert f"{ev_name}.h5" in models and not [m for m in models if "evalnet" in m and m != f"{ev_name}.h5"]      # one EvalNet, no rename
    ev_rows = _rows(base / "csv" / f"results_{ev_name}.csv")
    assert ev_rows[0] == ["modelname", "mse", "mae"] and len(ev_rows) == 2
    if isic:
        assert ev_rows[1][0] == ev_name and len(ev_rows[1]) == 3 and all(float(v) >= 0 for v in ev_rows[1][1:])
    else:      # five values and no name under the three-name header, as the script writes it
        assert len(ev_rows[1]) == 5 and all(float(v) >= 0 for v in ev_rows[1])
    for g in (0, 1):
        stem = f"{seg}_gen{g}"
        assert f"results_{stem}.csv" in csvs, csvs
        assert f"{stem}_topK_1.h5" in models and f"{stem}_topK_2.h5" in models and f"{stem}_0.h5" not in models, models
        d = base / "train_unlabeled_predictions" / "segnet" / stem
        assert sorted(os.listdir(d)) == ["images", "masks"]
        names = set(os.listdir(d / "images"))
        labelled = set(os.listdir(base / "train_labeled" / "images"))
        assert labelled <= names and set(os.listdir(d / "masks")) == names      # labelled pairs joined; whole pairs only
        rows = _rows(base / "csv" / f"results_{stem}.csv")
        assert len(rows) == 3 and [r[0] for r in rows[1:]] == [f"{stem}_0", f"{stem}_1"]
        assert rows[0] == (["modelname", "mIoU_val", "mIoU_test", "mIoU_train_unlabeled", "dice_score_val", "dice_score_test",
                            "dice_score_train_unlabeled"] if isic else
                           ["modelname", "mPA_val", "mPA_test", "mPA_train_unlabeled", "mIoU_val", "mIoU_test", "mIoU_train_unlabeled"])
        for i in (0, 1):      # the candidates' predictions of the unlabeled set: the next generation's candidate masks
            assert (base / "train_unlabeled_predictions" / "segnet" / f"{stem}_{i}").is_dir()
    g0 = set(os.listdir(base / "train_unlabeled_predictions" / "segnet" / f"{seg}_gen0" / "images"))
    g1 = set(os.listdir(base / "train_unlabeled_predictions" / "segnet" / f"{seg}_gen1" / "images"))
    assert g0 <= g1      # a generation starts from the last one's selected set


def test_full_dataset_script_toy_run(tmp_path):
    base, env = _toy(tmp_path, "ISIC_2018", {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "ISIC_2018/02_ISIC_2018_full_dataset.py")], env=env, cwd=tmp_path,
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    models = sorted(os.listdir(base / "models"))
    stem = "ISIC_2018_full_dataset_1"
    assert f"{stem}_topK_1.h5" in models and f"{stem}_topK_2.h5" in models and f"{stem}_0.h5" not in models and f"{stem}_1.h5" not in models
    rows = _rows(base / "csv" / f"results_{stem}.csv")
    assert rows[0] == ["modelname", "mIoU_val", "mIoU_test", "mIoU_train_unlabeled", "dice_score_val", "dice_score_test",
                       "dice_score_train_unlabeled"]
    assert [r[0] for r in rows[1:]] == [f"{stem}_0", f"{stem}_1"] and all(0.0 <= float(v) <= 1.0 for r in rows[1:] for v in r[1:])
    for k in ("val", "test", "train_unlabeled"):
        for i in (0, 1):
            assert (base / f"{k}_predictions" / "full_dataset" / f"{stem}_{i}").is_dir()
