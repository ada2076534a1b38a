"""GPU tests of the EvalNet-ensemble selection writers (create_training_data_for_segnet_with_*ensemble*), of the EvalNet training-data
writers (create_training_data_evalnet_ISIC_2018 / _miou_hela / _miou_multiclass) and of two script shims on toy data.

The writers run on toy directories of 64x64 images and of Cityscapes-shaped 64x128 images; their file sets, bytes and labels.csv are
compared with the pinned rules (tests/test_golden_evalnet_ensemble.py: select_rule, training_data_rule) restated in numpy on the SAME
models' predict outputs -- image by image, candidate stack by candidate stack, as the reference walks them.  The training-data writers
are also run on the labelled set of the recorded reference run with a model that returns the recorded probabilities: names, masks and
labels.csv must be the reference's own (tests/golden/evalnet_ensemble.npz, "td*")."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from test_golden_evalnet_ensemble import load, pred_name, select_rule, training_data_rule
from test_gpu_model_ensemble import CONFIG, HELA_CONFIG, HELA_SETUP, ROOT, SETUP

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)
from inconsistencymasks_amd import evalnet_functions as EF  # noqa: E402
from inconsistencymasks_amd import functions as F  # noqa: E402

PLANES = ("alive", "dead", "mod_position")


def _blobs(rng, h, w, k):
    """a class-id map of k classes in blocks (class 0 the background)"""
    m = np.zeros((h, w), np.uint8)
    for c in range(1, k):
        y, x = int(rng.integers(0, h - 16)), int(rng.integers(0, w - 16))
        m[y:y + int(rng.integers(8, 24)), x:x + int(rng.integers(8, 24))] = c
    return m


def _make_set(root, kind, h, w, k, n_images, n_dirs, seed):
    """unlabeled images, n_dirs candidate directories and a last generation that selected the even images"""
    rng = np.random.default_rng(seed)
    names = [f"u_{i:03d}.png" for i in range(n_images)]
    img_dir = os.path.join(root, "in", "brightfield" if kind == "hela" else "images")
    os.makedirs(img_dir)
    subs = PLANES if kind == "hela" else ("masks",)

    def write_masks(main, name, in_subdirs):
        """one random mask per plane: <main>/<sub>/<name> (a selected set, HeLa's candidate directories) or <main>/<name>"""
        for sub in subs:
            d = os.path.join(main, sub) if (kind == "hela" or in_subdirs) else main
            os.makedirs(d, exist_ok=True)
            F.write_png(os.path.join(d, name), _blobs(rng, h, w, 2 if kind != "multi" else k) * (255 if kind != "multi" else 1))
    for i, n in enumerate(names):
        F.write_png(os.path.join(img_dir, n), rng.integers(0, 256, (h, w) if kind == "hela" else (h, w, 3)).astype(np.uint8) // (1 + i % 3))
        for j in range(n_dirs):
            write_masks(os.path.join(root, f"d{j}"), n, False)
    last = os.path.join(root, "last")
    os.makedirs(os.path.join(last, os.path.basename(img_dir)))
    for n in names[::2] + ["lab_000.png"]:      # the last generation's set: some unlabeled images and a labelled pair
        F.write_png(os.path.join(last, os.path.basename(img_dir), n), rng.integers(0, 256, (h, w) if kind == "hela" else (h, w, 3)).astype(np.uint8))
        write_masks(last, n, True)
    return names, img_dir, [os.path.join(root, f"d{j}") for j in range(n_dirs)], last


def _evalnets(kind, h, w, k, n):
    from inconsistencymasks_amd.evalnet import get_evalnet, get_evalnet_miou
    if kind == "isic":
        return [get_evalnet(h, w, 3, 1, 0.5, normalize_B=True, seed=50 + j) for j in range(n)]
    if kind == "hela":
        return [get_evalnet_miou(h, w, 1, 3, 0.5, seed=50 + j) for j in range(n)]
    return [get_evalnet_miou(h, w, 3, k, 0.5, seed=50 + j, onehot_B=True) for j in range(n)]


def _candidate_stack(kind, h, w, k, name, dirs, out, with_last):
    """the reference's stack of one image: the directories' masks, then the output directory's where it exists"""
    roots = list(dirs) + ([out] if with_last else [])
    if kind == "hela":
        roots = [r for r in roots if os.path.exists(os.path.join(r, "alive", name))]
        return np.stack([np.stack([F.read_png(os.path.join(r, p, name), 1)[..., 0] for p in PLANES], -1) for r in roots])
    paths = [os.path.join(r, name) for r in dirs] + ([os.path.join(out, "masks", name)] if with_last else [])
    return np.stack([F.read_png(p, 1)[..., 0] for p in paths if os.path.isfile(p)])


@pytest.mark.parametrize("kind,h,w,k,rgb", [("isic", 64, 64, 1, True), ("isic", 64, 128, 1, False), ("hela", 64, 64, 3, True),
                                            ("multi", 64, 64, 4, True), ("multi", 64, 128, 5, False)])
def test_selection_writers_match_the_restated_rule(tmp_path, monkeypatch, kind, h, w, k, rgb):
    monkeypatch.setattr(EF, "SELECT_BATCH", 3)      # several batches, with and without a last-generation candidate in one batch
    n_dirs = 5
    names, img_dir, dirs, last = _make_set(str(tmp_path), kind, h, w, k, 7, n_dirs, 3)
    nets = _evalnets(kind, h, w, k, 2)
    c = 1 if kind == "hela" else 3
    img_sub = os.path.basename(img_dir)

    # the restated rule on the same EvalNets' predict outputs, image by image
    def expected(thr, with_last):
        exp = {}
        for n in names:
            img = F.read_png(os.path.join(img_dir, n), c)
            if c == 3 and not rgb:
                img = img[..., ::-1]
            stack = _candidate_stack(kind, h, w, k, n, dirs, last, with_last)      # `last` was copied into the output first
            m = len(stack)
            rep = np.repeat(img[None], m, 0)
            xb = stack[..., None] if kind == "isic" else (stack // 255 if kind == "hela" else stack)
            outs = [e.predict([rep, xb]) for e in nets]
            sc = np.stack([o if kind == "isic" else np.concatenate(o, 1) for o in outs]).astype(np.float32)
            best, score, keep = select_rule(sc, thr, kind != "isic")
            exp[n] = (m, best, float(score), keep, stack[best])
        return exp

    scores = sorted(v[2] for v in expected(0.0, False).values())
    thr = (scores[3] + scores[4]) / 2 if scores[3] != scores[4] else scores[3]      # about half of the images pass
    for with_last in (False, True):
        out = str(tmp_path / f"out{int(with_last)}")
        args = (nets, h, w, c) + ((k,) if kind == "multi" else ()) + (img_dir, dirs, out, thr) + ((last,) if with_last else ())
        if kind == "isic":
            F.create_training_data_for_segnet_with_ensemble_binary(*args, rgb=rgb)
        elif kind == "hela":
            F.create_training_data_for_segnet_with_miou_ensemble_hela(*args)
        else:
            F.create_training_data_for_segnet_with_miou_ensemble_multiclass(*args, rgb=rgb)
        exp = expected(thr, with_last)
        assert {v[0] for v in exp.values()} == ({n_dirs, n_dirs + 1} if with_last else {n_dirs})
        kept = {n for n, v in exp.items() if v[3]}
        assert 0 < len(kept) < len(names), "the threshold must split the toy set"
        before = set(os.listdir(os.path.join(last, img_sub))) if with_last else set()
        assert set(os.listdir(os.path.join(out, img_sub))) == kept | before
        for sub in (PLANES if kind == "hela" else ("masks",)):
            assert set(os.listdir(os.path.join(out, sub))) == kept | before, sub
        for n in kept | before:
            src = os.path.join(img_dir if n in kept else os.path.join(last, img_sub), n)
            assert open(os.path.join(out, img_sub, n), "rb").read() == open(src, "rb").read(), n      # the image file, copied
            if n not in kept:      # the last generation's pair stays as it was copied
                for sub in (PLANES if kind == "hela" else ("masks",)):
                    assert open(os.path.join(out, sub, n), "rb").read() == open(os.path.join(last, sub, n), "rb").read(), (sub, n)
                continue
            chosen = exp[n][4]
            if kind == "hela":
                assert np.array_equal(F.read_png(os.path.join(out, "alive", n), 1)[..., 0], chosen[..., 0]), n
                assert np.array_equal(F.read_png(os.path.join(out, "dead", n), 1)[..., 0], chosen[..., 1]), n
                assert np.array_equal(F.read_png(os.path.join(out, "mod_position", n), 3), F._hela_vote_positions(chosen[..., 2], 8, 3)), n
            else:
                assert np.array_equal(F.read_png(os.path.join(out, "masks", n), 1)[..., 0], chosen), n


def _unet(kind, h, w, k):
    from inconsistencymasks_amd.unet import UNet
    return UNet(h, w, 1 if kind == "hela" else 3, k, 0.5, "softmax" if kind == "multi" else "sigmoid", seed=5)


def _labels(path):
    with open(os.path.join(path, "labels.csv"), newline="") as f:
        return [row for row in csv.reader(f, delimiter=";")]


@pytest.mark.parametrize("kind,h,w,k", [("isic", 64, 64, 1), ("hela", 64, 64, 3), ("multi", 64, 64, 4), ("multi", 64, 128, 5)])
def test_training_data_writers_match_the_restated_rules(tmp_path, kind, h, w, k):
    """the writers on a real U-Net against training_data_rule, the restatement that the recorded reference run pins"""
    import torch
    rng = np.random.default_rng(9)
    c = 1 if kind == "hela" else 3
    names = [f"l_{i:03d}.png" for i in range(5)] + ["l_005_aug_03.png"]
    src = str(tmp_path / "labelled")
    img_sub = "brightfield" if kind == "hela" else "images"
    subs = PLANES if kind == "hela" else ("masks",)
    for d in (img_sub,) + subs:
        os.makedirs(os.path.join(src, d))
    for i, n in enumerate(names):
        F.write_png(os.path.join(src, img_sub, n), rng.integers(0, 256, (h, w) if c == 1 else (h, w, 3)).astype(np.uint8))
        for sub in subs:
            F.write_png(os.path.join(src, sub, n), _blobs(rng, h, w, 2 if kind != "multi" else k) * (255 if kind != "multi" else 1))
    model = _unet(kind, h, w, k)
    out = str(tmp_path / "evalnet_data")
    listed = sorted(os.listdir(os.path.join(src, img_sub)))      # the writers walk the sorted list (shard_list)
    if kind == "hela":      # the image the first loop ends on has no dead cells: every i == 0 row must say so (the leftover masks)
        F.write_png(os.path.join(src, "dead", listed[-1]), np.zeros((h, w), np.uint8))
    for i in (0, 11):
        if kind == "isic":
            F.create_training_data_evalnet_ISIC_2018(model, h, w, c, os.path.join(src, "images"), os.path.join(src, "masks"), out, i)
        elif kind == "hela":
            F.create_training_data_evalnet_miou_hela(model, h, w, c, src, out, i)
        else:
            F.create_training_data_evalnet_miou_multiclass(model, h, w, c, k, os.path.join(src, "images"), os.path.join(src, "masks"), out, i)
    assert pred_name("l_005_aug_03.png", 11) == "l_005____11_03.png" and pred_name("l_005_aug_03.png", 0) == "l_005_aug_03___0.png"
    # the restatement that the recorded reference run pins (test_golden_evalnet_ensemble.training_data_rule), on this model's outputs
    x = torch.from_numpy(np.stack([F.read_png(os.path.join(src, img_sub, n), c) for n in listed])).cuda()
    probs = model.predict_device(x).cpu().numpy()
    gt = np.stack([np.stack([F.read_png(os.path.join(src, sub, n), 1)[..., 0] for sub in subs], -1) for n in listed])
    files, masks, lines = training_data_rule({"isic": "bin", "multi": "mc"}.get(kind, kind), listed, gt if kind == "hela" else gt[..., 0],
                                             probs, (0, 11))
    want_rows = [line.split(";") for line in lines]
    want_files = {f.split("/")[1] for f in files if f.split("/")[0] == subs[0]}
    assert len(want_files) == 3 * len(listed)
    for step, i in enumerate((0, 11)):
        for j, n in enumerate(listed):
            for q, sub in enumerate(subs):
                want = masks[step][j][..., q] if kind == "hela" else masks[step][j]
                assert np.array_equal(F.read_png(os.path.join(out, sub, pred_name(n, i)), 1)[..., 0], want), (sub, n, i)
    assert _labels(out) == want_rows
    for sub in subs:
        assert set(os.listdir(os.path.join(out, sub))) == want_files, sub
    assert set(os.listdir(os.path.join(out, img_sub))) == set(listed)
    for n in listed:      # i == 0: the labelled files, copied
        for sub in (img_sub,) + subs:
            assert open(os.path.join(out, sub, n), "rb").read() == open(os.path.join(src, sub, n), "rb").read(), (sub, n)
    if kind == "hela":      # the leftover rule is visible: not every ground-truth row is all ones
        gt_rows = [r for r in _labels(out) if "___" not in r[0]]
        assert len({tuple(r[1:]) for r in gt_rows}) == 1 and gt_rows[0][1:] == ["1", "0", "1", "1", "0", "1"]


class _FixedModel:
    """predict_device -> the recorded probabilities of the next images, whatever it is fed; what it was fed is kept"""

    def __init__(self, probs):
        import torch
        self.probs, self.fed, self.at = torch.from_numpy(probs).cuda(), [], 0

    def predict_device(self, x):
        self.fed.append(x.cpu().numpy())
        self.at += len(x)
        return self.probs[self.at - len(x):self.at].contiguous()


@pytest.mark.parametrize("kind", ["bin", "hela", "mc"])
def test_training_data_writers_reproduce_the_reference(tmp_path, kind):
    """the recorded run of the reference's own writers (tests/golden/evalnet_ensemble.npz, "td*"): the same labelled set on disk, a
    model that returns the recorded probabilities -> the recorded file names, masks and labels.csv, for i = 0 and then i = 11"""
    d = load()
    key = "td" + kind
    names, gt, probs = d["td_names"].tolist(), d[key + "_gt"], d[key + "_probs"]
    h, w, k = probs.shape[1:]
    src, out = str(tmp_path / "labelled"), str(tmp_path / "evalnet_data")
    img_sub = "brightfield" if kind == "hela" else "images"
    subs = PLANES if kind == "hela" else ("masks",)
    for sub in (img_sub,) + subs:
        os.makedirs(os.path.join(src, sub))
    rgb = None if kind == "hela" else bool(d["td_rgb"][("bin", "mc").index(kind)])
    rng = np.random.default_rng(4)
    for j, n in enumerate(names):      # the images as cv2 read them are BGR; on disk and from read_png they are RGB
        img = rng.integers(0, 256, (h, w), dtype=np.uint8) if kind == "hela" else d[key + "_io"][0][j][..., ::-1]
        F.write_png(os.path.join(src, img_sub, n), img)
        for q, sub in enumerate(subs):
            F.write_png(os.path.join(src, sub, n), gt[j][..., q] if kind == "hela" else gt[j])
    for i in (0, 11):
        model = _FixedModel(probs)
        if kind == "bin":
            F.create_training_data_evalnet_ISIC_2018(model, h, w, 3, os.path.join(src, "images"), os.path.join(src, "masks"), out, i, rgb=rgb)
        elif kind == "hela":
            F.create_training_data_evalnet_miou_hela(model, h, w, 1, src, out, i)
        else:
            F.create_training_data_evalnet_miou_multiclass(model, h, w, 3, k, os.path.join(src, "images"), os.path.join(src, "masks"), out, i,
                                                           rgb=rgb)
        if kind != "hela":
            assert np.array_equal(np.concatenate(model.fed), d[key + "_io"][1]), i      # the recorded input of the reference's model
    with open(os.path.join(out, "labels.csv"), newline="") as f:
        assert f.read().split("\r\n")[:-1] == d[key + "_labels"].tolist()
    recorded = [p.split("/")[2:] for p in d[key + "_files"].tolist()]      # /tout/<sub>/<name>
    for sub in (img_sub,) + subs:
        assert set(os.listdir(os.path.join(out, sub))) == {n for s_, n in recorded if s_ == sub}, sub
    for step, i in enumerate((0, 11)):
        for j, n in enumerate(names):
            for q, sub in enumerate(subs):
                want = d[key + "_masks"][step][j][..., q] if kind == "hela" else d[key + "_masks"][step][j]
                assert np.array_equal(F.read_png(os.path.join(out, sub, pred_name(n, i)), 1)[..., 0], want), (sub, n, i)
    for n in names:      # i == 0: the labelled files, copied
        for sub in (img_sub,) + subs:
            assert open(os.path.join(out, sub, n), "rb").read() == open(os.path.join(src, sub, n), "rb").read(), (sub, n)


# ---- the scripts on toy data ---------------------------------------------------------------------------------------------------------
EVALNET_EXTRA = "NUM_EPOCHS_EVALNET = 1\nBATCH_SIZE_EVALNET = 8\n"
CANDIDATE_DIRS = """
import shutil
tag, runid = {tag!r}, 1
base = paths.{tag}_BASE_DIR
if tag == "HELA":
    unl, subs = paths.HELA_TRAIN_UNLABELED_DIR, ("alive", "dead", "mod_position")
    shutil.copytree(os.path.join(paths.HELA_TRAIN_LABELED_DIR, "brightfield"), os.path.join(paths.HELA_TRAIN_FULL_DIR, "brightfield"))
else:
    unl, subs = os.path.dirname(paths.ISIC_2018_TRAIN_UNLABELED_MASKS_DIR), ("masks",)
for j in range(10):      # the `subset` models' predictions of the unlabeled set: the ground truth shifted by 2 j pixels
    d = os.path.join(base, "train_unlabeled_predictions", "subset", f"{{tag}}_subset_{{runid}}_{{j}}")
    for sub in subs:
        os.makedirs(os.path.join(d, sub) if tag == "HELA" else d, exist_ok=True)
        for n in os.listdir(os.path.join(unl, sub)):
            m = np.roll(F.read_png(os.path.join(unl, sub, n), 1)[..., 0], 2 * j, 1)
            F.write_png(os.path.join(d, sub, n) if tag == "HELA" else os.path.join(d, n), m)
"""


@pytest.mark.parametrize("ds", ["ISIC_2018", "HeLa"])
def test_evalnet_ensemble_script_toy_run(tmp_path, ds):
    config, setup, script, tag, subs = {
        "ISIC_2018": (CONFIG, SETUP, "ISIC_2018/10_ISIC_2018_evalnet_ensemble.py", "ISIC_2018", ("images", "masks")),
        "HeLa": (HELA_CONFIG, HELA_SETUP, "HeLa/10_HeLa_evalnet_miou_ensemble.py", "HELA", ("brightfield", "alive", "dead", "mod_position")),
    }[ds]
    config = config.replace("TOP_Ks = 2\n", "TOP_Ks = 2\n" + EVALNET_EXTRA) + "ALPHA_EVALNET = 0.5\nMIN_THRESHOLD = 0.3\nMAX_THRESHOLD = 0.35\n"
    base = tmp_path / "data"
    cfg = tmp_path / "config.ini"
    cfg.write_text(config.format(base=base))
    env = {**os.environ, "IM_CONFIG": str(cfg), "IM_RUNIDS": "1", "IM_NS": "2", "IM_GENS": "0,1", "IM_CANDIDATES": "0,1",
           "IM_EVALNET_CANDIDATES": "0,1"}
    subprocess.run([sys.executable, "-c", setup.format(root=ROOT) + CANDIDATE_DIRS.format(tag=tag)], env=env, check=True, cwd=tmp_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)], env=env, cwd=tmp_path, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    csvs, models = sorted(os.listdir(base / "csv")), sorted(os.listdir(base / "models"))
    ev_tag, ev_sub = ("ISIC_2018_evalnet", "evalnet_ensemble") if ds == "ISIC_2018" else ("HELA_evalnet_miou", "evalnet_miou_ensemble")
    seg = "ISIC_2018_segnet" if ds == "ISIC_2018" else "HELA_segnet_ensemble"
    # the EvalNet stage: training data of the two `subset` models (train: both; val: both, model_i < 3), candidates ranked and renamed
    for split, n_src in (("train", 16), ("val", 8)):
        rows = [r for r in csv.reader(open(base / ev_sub / "run_1" / split / "labels.csv", newline=""), delimiter=";")]
        assert len(rows) == 3 * n_src and len(rows[0]) == (2 if ds == "ISIC_2018" else 7), split      # two models' predictions + the ground truth
        assert sum("___0.png" in r[0] for r in rows) == n_src and sum("___1.png" in r[0] for r in rows) == n_src
    assert f"{ev_tag}_1_topK_1.h5" in models and f"{ev_tag}_1_topK_2.h5" in models and f"{ev_tag}_1_0.h5" not in models
    assert f"results_{ev_tag}_1_1.csv" in csvs
    ev_rows = [r.split(";") for r in (base / "csv" / f"results_{ev_tag}_1_1.csv").read_text().strip().splitlines()]
    assert ev_rows[0] == (["modelname", "mse", "mae"] if ds == "ISIC_2018" else
                          ["modelname", "total_loss", "iou_loss", "detection_loss", "iou_mae", "detection_mae"])
    assert [r[0] for r in ev_rows[1:]] == [f"{ev_tag}_1_0", f"{ev_tag}_1_1"]
    for g in (0, 1):
        stem = f"{seg}_1_n2_gen{g}"
        assert f"results_{stem}.csv" in csvs, csvs
        assert f"{stem}_topK_1.h5" in models and f"{stem}_topK_2.h5" in models, models
        d = base / "train_unlabeled_predictions" / "segnet" / stem
        assert sorted(os.listdir(d)) == sorted(subs)
        names = set(os.listdir(d / subs[0]))
        labelled = set(os.listdir(base / "train_labeled" / subs[0]))
        assert labelled <= names and all(set(os.listdir(d / s)) == names for s in subs)      # labelled pairs joined; whole samples only
        rows = [r.split(";") for r in (base / "csv" / f"results_{stem}.csv").read_text().strip().splitlines()]
        assert len(rows) == 3 and {r[0] for r in rows[1:]} == {f"{stem}_0", f"{stem}_1"}
        if ds == "HeLa":
            assert rows[0] == ["modelname", "mIoU_val", "mIoU_ad_val", "mcce_val", "mIoU_test", "mIoU_ad_test", "mcce_test",
                               "mIoU_unlabeled", "mIoU_ad_unlabeled", "mcce_unlabeled"]
        else:
            assert rows[0] == ["modelname", "mIoU_val", "mIoU_test", "mIoU_train_unlabeled", "dice_score_val", "dice_score_test",
                               "dice_score_train_unlabeled"]
        for i in (0, 1):      # the candidates' predictions of the unlabeled set: the next generation's candidate masks
            assert (base / "train_unlabeled_predictions" / "segnet" / f"{stem}_{i}").is_dir()
    g0 = set(os.listdir(base / "train_unlabeled_predictions" / "segnet" / f"{seg}_1_n2_gen0" / subs[0]))
    g1 = set(os.listdir(base / "train_unlabeled_predictions" / "segnet" / f"{seg}_1_n2_gen1" / subs[0]))
    assert g0 <= g1      # a generation starts from the last one's selected set
