"""train_ISIC_2018 and train_hela with loss_func=dice_loss on toy directories (8 training and 4 validation files of 32 x 32, 2 epochs,
batch 4): the checkpoint is written and reloads, the six / nine return values come back, the prediction PNGs are on disk; for HeLa
the saved epoch is the one with the lowest val_loss = 1 - mean dice_b over the validation images, recomputed here from
imk_eval_dice_sums after every epoch.  The toy files are tests/test_gpu_consistency_scripts.py's."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_consistency_scripts import H, W, _toy_hela, _toy_set  # noqa: E402
from inconsistencymasks_amd import evaluate as E  # noqa: E402
from inconsistencymasks_amd import functions as F  # noqa: E402
from inconsistencymasks_amd.unet import UNet  # noqa: E402


def _toy_epochs(monkeypatch):
    monkeypatch.setattr(F, "NUM_EPOCHS", 2)
    monkeypatch.setattr(F, "BATCH_SIZE", 4)
    import random
    random.seed(3)
    np.random.seed(3)


def _watch_fit(monkeypatch, after_epoch):
    """fit() as it is, with `after_epoch(ep, model)` behind the trainer's own epoch-end hook; -> the loss kinds fit() was given"""
    real, kinds = F.fit, []

    def fit(model, loader, steps_per_epoch, epochs, loss_kind, on_epoch_end=None, **kw):
        kinds.append(loss_kind)

        def hook(ep, loss):
            on_epoch_end(ep, loss)
            after_epoch(ep, model)
        return real(model, loader, steps_per_epoch, epochs, loss_kind, hook, **kw)
    monkeypatch.setattr(F, "fit", fit)
    return kinds


@pytest.mark.parametrize("loss_func", [F.dice_loss, "dice_loss"], ids=["function", "name"])
def test_train_isic_with_dice_loss(tmp_path, monkeypatch, loss_func):
    _toy_epochs(monkeypatch)
    d = {n: str(tmp_path / n.split("_")[0] / ("images" if n.endswith("_i") else "masks" if n.endswith("_m") else n))
         for n in ("trn_i", "trn_m", "val_i", "val_m", "unl_i", "unl_m")}
    d.update({n: str(tmp_path / n) for n in ("pv", "pt", "pu")})
    _toy_set(d["trn_i"], d["trn_m"], 8, 1, 1)
    _toy_set(d["val_i"], d["val_m"], 4, 1, 3)
    _toy_set(d["unl_i"], d["unl_m"], 4, 1, 2)
    h5 = str(tmp_path / "cand.h5")
    model = UNet(H, W, 3, 1, 0.5, "sigmoid", seed=5)
    ious, saves = [], []
    kinds = _watch_fit(monkeypatch, lambda ep, m: ious.append(F._binary_iou_dataset(m, d["val_i"], d["val_m"], 3)))
    real_save = F.save_model
    monkeypatch.setattr(F, "save_model", lambda m, p: (saves.append(len(ious)), real_save(m, p))[1])
    out = F.train_ISIC_2018(d["trn_i"], d["val_i"], d["val_m"], d["val_i"], d["val_m"], d["unl_i"], d["unl_m"], "toy", h5, model,
                            loss_func, 2, H, W, 3, d["pv"], d["pt"], d["pu"])
    assert kinds == [4]
    assert len(out) == 6 and all(np.isfinite(float(v)) for v in out), out
    assert os.path.exists(h5) and F.load_model(h5) is not None
    for k in ("pv", "pt", "pu"):
        assert len([n for n in os.listdir(d[k]) if n.endswith(".png")]) >= 4, k
    # the val_binary_io_u rule is kept: the last save is the first epoch that reached the best IoU
    assert len(ious) == 2 and saves and saves[-1] == int(np.argmax(ious)), (ious, saves)


def test_train_hela_with_dice_loss(tmp_path, monkeypatch):
    _toy_epochs(monkeypatch)
    d = {n: str(tmp_path / n) for n in ("trn", "val", "unl", "pv", "pt", "pu")}
    _toy_hela(d["trn"], 8, 1)
    _toy_hela(d["val"], 4, 3)
    _toy_hela(d["unl"], 4, 2)
    names = sorted(os.listdir(os.path.join(d["val"], "brightfield")))
    items = [F.parse_image_hela(os.path.join(d["val"], "brightfield", n), 1) for n in names]
    xs = torch.from_numpy(np.stack([it[0] for it in items])).cuda()
    ys = torch.from_numpy(np.stack([it[1] for it in items])).cuda()
    assert int(ys.max()) == 3

    def val_loss(m):      # one image per call: imk_eval_dice_sums' rows do not depend on the batch
        dices = np.concatenate([E.dice_from_sums(E.dice_sums(m.predict_device(xs[i:i + 1]), ys[i:i + 1])) for i in range(len(names))])
        return 1.0 - float(np.mean(dices))
    losses, saves = [], []
    kinds = _watch_fit(monkeypatch, lambda ep, m: losses.append(val_loss(m)))
    real_save = F.save_model
    monkeypatch.setattr(F, "save_model", lambda m, p: (saves.append(len(losses)), real_save(m, p))[1])
    h5 = str(tmp_path / "cand.h5")
    model = UNet(H, W, 1, 3, 0.5, "sigmoid", seed=5)
    out = F.train_hela(os.path.join(d["trn"], "brightfield"), os.path.join(d["val"], "brightfield"), d["val"], d["val"], d["unl"], "toy", h5,
                       model, F.dice_loss, 2, H, W, 1, d["pv"], d["pt"], d["pu"])
    assert kinds == [4]
    assert len(out) == 9 and all(np.isfinite(float(v)) for v in out), out
    assert os.path.exists(h5)
    for k in ("pv", "pt", "pu"):
        for sub in ("alive", "dead", "mod_position"):
            assert len(os.listdir(os.path.join(d[k], sub))) >= 4, (k, sub)
    assert len(losses) == 2 and all(0.0 < v < 1.0 for v in losses), losses
    assert saves and saves[-1] == int(np.argmin(losses)), (losses, saves)
    got = val_loss(F.load_model(h5))
    print(f"hela: val_loss per epoch {losses}, saved after epoch {saves[-1]}; the reloaded checkpoint's {got}")
    assert abs(got - min(losses)) <= 1e-6 * min(losses), (got, losses)
