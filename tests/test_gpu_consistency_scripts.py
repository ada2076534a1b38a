"""GPU runs of the consistency-loss training functions and of the driver on toy data: train_ISIC_2018_consistency_loss and
train_multiclass_consistency_loss on toy directories (8 labelled, 8 unlabelled, 4 validation images of 32 x 32, NUM_EPOCHS_CS 2, batch
4) from a toy model -- the checkpoint exists and reloads, the return tuple has the reference's arity, the four validation losses are
finite and the saved model is the one with the lowest of them -- and one toy consistency_driver.run("ISIC_2018") (one run id, one
strength) whose CSV, topK files and prediction directories carry the reference's names.  The driver's toy dataset and config are the
model-ensemble tests'."""
import os
import sys

import numpy as np
import pytest

from test_gpu_model_ensemble import CONFIG, ROOT, SETUP, _toy_run

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)
from inconsistencymasks_amd import functions as F  # noqa: E402

H = W = 32


def _toy_set(d_img, d_mask, n, k, seed):
    """images with a bright disc; masks: the disc as 0 / 255 (k == 1) or as class ids 0 .. k-1 by quadrant"""
    os.makedirs(d_img, exist_ok=True)
    os.makedirs(d_mask, exist_ok=True)
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        cy, cx, r = rng.integers(10, 22), rng.integers(10, 22), rng.integers(5, 9)
        disc = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        img = (90 + rng.integers(-10, 10, (H, W, 3)) + disc[..., None] * 100).clip(0, 255).astype(np.uint8)
        mask = (disc * 255).astype(np.uint8) if k == 1 else (disc * (1 + (yy > cy) + (xx > cx) % (k - 1))).clip(0, k - 1).astype(np.uint8)
        F.write_png(os.path.join(d_img, f"t_{i:03d}.png"), img)
        F.write_png(os.path.join(d_mask, f"t_{i:03d}.png"), mask)


def _toy_hela(main, n, seed):
    """brightfield images with two bright discs; alive / dead = one disc each, mod_position = small discs at their centres"""
    rng = np.random.default_rng(seed)
    for sub in ("brightfield", "alive", "dead", "mod_position"):
        os.makedirs(os.path.join(main, sub), exist_ok=True)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        cs = [(rng.integers(7, 12), rng.integers(7, 25)), (rng.integers(20, 25), rng.integers(7, 25))]
        discs = [(yy - cy) ** 2 + (xx - cx) ** 2 < 25 for cy, cx in cs]
        pos = sum(((yy - cy) ** 2 + (xx - cx) ** 2 < 5) for cy, cx in cs) > 0
        img = (90 + rng.integers(-10, 10, (H, W)) + discs[0] * 100 + discs[1] * 50).clip(0, 255).astype(np.uint8)
        for sub, a in (("brightfield", img), ("alive", discs[0] * 255), ("dead", discs[1] * 255), ("mod_position", pos * 255)):
            F.write_png(os.path.join(main, sub, f"t_{i:03d}.png"), np.asarray(a, np.uint8))


def test_hela_training_function_on_toy_directories(tmp_path, monkeypatch):
    import torch
    from inconsistencymasks_amd import consistency
    from inconsistencymasks_amd.unet import UNet
    monkeypatch.setattr(F, "NUM_EPOCHS_CS", 2)
    monkeypatch.setattr(F, "BATCH_SIZE", 4)
    d = {n: str(tmp_path / n) for n in ("lab", "unl", "val", "pv", "pt", "pu")}
    _toy_hela(d["lab"], 8, 1)
    _toy_hela(d["unl"], 8, 2)
    _toy_hela(d["val"], 4, 3)
    h5 = str(tmp_path / "cand.h5")
    model = UNet(H, W, 1, 3, 0.5, "sigmoid", seed=5)
    import random
    random.seed(3)
    np.random.seed(3)
    out = F.train_hela_consistency_loss(d["lab"], d["val"], d["val"], d["unl"], "toy", h5, model, "mse", H, W, 1, d["pv"], d["pt"], d["pu"],
                                        1, 10, (0.85, 1.15), (-10, 10))
    losses = consistency.train_hela_consistency_loss.last_validation_losses
    assert len(out) == 9 and len(losses) == 4 and all(np.isfinite(v) for v in losses), (out, losses)
    best = F.load_model(h5)
    names = sorted(os.listdir(os.path.join(d["val"], "brightfield")))
    x = torch.from_numpy(np.stack([F.read_png(os.path.join(d["val"], "brightfield", n), 1) for n in names])).cuda()
    y = np.stack([np.stack([F.read_png(os.path.join(d["val"], k, n), 1)[..., 0] > 127 for n in names]) for k in ("alive", "dead", "mod_position")], -1)
    got = float(((best.predict_device(x).double().cpu().numpy() - y) ** 2).mean())
    print(f"hela: validation losses {losses}; the reloaded checkpoint's {got}")
    assert abs(got - min(losses)) <= 1e-5 * min(losses), (got, losses)


def _val_loss(model, d_img, d_mask, kind):
    import torch
    names = sorted(os.listdir(d_img))
    x = torch.from_numpy(np.stack([F.read_png(os.path.join(d_img, n), 3) for n in names])).cuda()
    y = np.stack([F.read_png(os.path.join(d_mask, n), 1)[..., 0] for n in names])
    p = model.predict_device(x).double().cpu().numpy()
    if kind == "isic":
        return float(((p[..., 0] - (y > 127)) ** 2).mean())
    return float(-np.log(np.take_along_axis(p, y[..., None].astype(np.int64), -1)).mean())


@pytest.mark.parametrize("kind", ["isic", "multi"])
def test_training_function_on_toy_directories(tmp_path, monkeypatch, kind):
    from inconsistencymasks_amd import consistency
    from inconsistencymasks_amd.unet import UNet
    monkeypatch.setattr(F, "NUM_EPOCHS_CS", 2)
    monkeypatch.setattr(F, "BATCH_SIZE", 4)
    k = 1 if kind == "isic" else 4
    d = {n: str(tmp_path / n) for n in ("li", "lm", "ui", "um", "vi", "vm", "pv", "pt", "pu")}
    _toy_set(d["li"], d["lm"], 8, k, 1)
    _toy_set(d["ui"], d["um"], 8, k, 2)
    _toy_set(d["vi"], d["vm"], 4, k, 3)
    h5 = str(tmp_path / "cand.h5")
    model = UNet(H, W, 3, k, 0.5, "sigmoid" if kind == "isic" else "softmax", seed=5)      # the toy subset model
    import random
    random.seed(3)
    np.random.seed(3)
    aug = (1, 10, (0.85, 1.15), (-10, 10))
    if kind == "isic":
        out = F.train_ISIC_2018_consistency_loss(d["li"], d["lm"], d["vi"], d["vm"], d["vi"], d["vm"], d["ui"], d["um"], "toy", h5, model,
                                                 "mse", H, W, 3, d["pv"], d["pt"], d["pu"], *aug)
        losses = consistency.train_ISIC_2018_consistency_loss.last_validation_losses
    else:
        from inconsistencymasks_amd.im_driver import color_mapping
        out = F.train_multiclass_consistency_loss(d["li"], d["lm"], d["vi"], d["vm"], d["vi"], d["vm"], d["ui"], d["um"], "toy", h5, model,
                                                  "categorical_crossentropy", H, W, 3, k, color_mapping("SUIM", 9), d["pv"], d["pt"], d["pu"],
                                                  *aug)
        losses = consistency.train_multiclass_consistency_loss.last_validation_losses
    assert len(out) == 6 and all(np.isfinite(float(v)) for v in out)
    assert len(losses) == 4 and all(np.isfinite(v) for v in losses), losses
    assert os.path.exists(h5)
    best = F.load_model(h5)
    got = _val_loss(best, d["vi"], d["vm"], kind)
    print(f"{kind}: validation losses {losses}; the reloaded checkpoint's {got}")
    assert abs(got - min(losses)) <= 1e-5 * min(losses), (got, losses)
    assert len(os.listdir(d["pu"])) > 0
    # the step counter of the one optimizer state: 2 epochs x (2 labelled + 2 consistency steps), minus the steps the loss scale skipped
    import struct
    off = model.plan.state_bytes - 256
    step = struct.unpack("ffii", bytes(model.train_state[off:off + 16].cpu().tolist()))[3]
    assert 4 <= step <= 8, step


def test_refused_losses():
    from inconsistencymasks_amd.unet import UNet
    with pytest.raises(NotImplementedError):
        F.train_multiclass_consistency_loss(*["x"] * 10, None, F.ignore_im_categorical_crossentropy(), 32, 32, 3, 4, {}, "a", "b", "c", 1, 10,
                                            (0.9, 1.1), (-1, 1))
    with pytest.raises(NotImplementedError):
        F.train_ISIC_2018_consistency_loss(*["x"] * 10, None, "binary_crossentropy", 32, 32, 3, "a", "b", "c", 1, 10, (0.9, 1.1), (-1, 1))


def test_consistency_driver_toy_run(tmp_path, monkeypatch):
    monkeypatch.setenv("IM_CS_STRENGTHS", "0")
    config = CONFIG.replace("NUM_EPOCHS = 2\n", "NUM_EPOCHS = 2\nNUM_EPOCHS_CS = 2\n")
    assert "NUM_EPOCHS_CS" in config
    base, out = _toy_run(tmp_path, config, SETUP, os.path.join(ROOT, "ISIC_2018", "05_ISIC_2018_consistency_loss.py"))
    stem = "ISIC_2018_consistency_loss_1_aug_low"
    csvs, models = sorted(os.listdir(base / "csv")), sorted(os.listdir(base / "models"))
    assert f"results_{stem}.csv" in csvs and not [c for c in csvs if "aug_mid" in c or "aug_high" in c], csvs
    assert f"{stem}_topK_1.h5" in models and f"{stem}_topK_2.h5" in models, models
    rows = [r.split(";") for r in (base / "csv" / f"results_{stem}.csv").read_text().strip().splitlines()]
    assert rows[0] == ["modelname", "mIoU_val", "mIoU_test", "mIoU_train_unlabeled", "dice_score_val", "dice_score_test",
                       "dice_score_train_unlabeled"]
    assert len(rows) == 3 and {r[0] for r in rows[1:]} == {f"{stem}_0", f"{stem}_1"}
    for split in ("val", "test", "train_unlabeled"):
        for i in (0, 1):
            assert len(os.listdir(base / f"{split}_predictions" / "consistency_loss" / f"{stem}_{i}")) > 0, split
    order = sorted(rows[1:], key=lambda r: float(r[1]), reverse=True)
    line = next(ln for ln in out.splitlines() if ln.startswith("[(") and f"{stem}_" in ln)
    assert line.index(f"'{order[0][0]}'") < line.index(f"'{order[1][0]}'") or float(order[0][1]) == float(order[1][1])
