"""The depth-map family end to end on a toy tree (eight 32 x 32 training images, six for validation): train_depth_map with 'mse' and
with rmse for two epochs -- the checkpoint exists, six finite numbers come back and they are the sums imk_eval_depth gives for the
checkpointed model, the prediction PNGs are imk_eval_depth's pred_out -- then get_im_prediction_depth_map on the two trained models
against tests/depth_cases.py on their `predict` outputs."""
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

import depth_cases as DC  # noqa: E402
from inconsistencymasks_amd import depth as D  # noqa: E402
from inconsistencymasks_amd import functions as F  # noqa: E402
from inconsistencymasks_amd.unet import UNet  # noqa: E402

H = W = 32


def _tree(base, split, n, seed):
    """images: smooth colour ramps + noise; depth maps: a function of the image (something to learn), every value 0..255 possible"""
    rng = np.random.default_rng(seed)
    img_dir, dep_dir = os.path.join(base, split, "images"), os.path.join(base, split, "depth_maps")
    os.makedirs(img_dir), os.makedirs(dep_dir)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        ramp = 127 + 100 * np.sin((xx + 3 * i) / 6.0) * np.cos((yy - 2 * i) / 5.0)
        img = (ramp[..., None] + rng.integers(-20, 20, (H, W, 3))).clip(0, 255).astype(np.uint8)
        dep = (0.6 * img[..., 0] + 0.4 * img[..., 2].astype(np.float64)).clip(0, 255).astype(np.uint8)
        F.write_png(os.path.join(img_dir, f"t{i:02d}.png"), img)
        F.write_png(os.path.join(dep_dir, f"t{i:02d}.png"), dep)
    return img_dir


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    base = str(tmp_path_factory.mktemp("depth_toy"))
    train, val = _tree(base, "train", 8, 1), _tree(base, "val", 6, 2)
    saved = F.NUM_EPOCHS, F.BATCH_SIZE
    F.NUM_EPOCHS, F.BATCH_SIZE = 2, 4      # config.ini's values, read by the family at call time
    out = {}
    try:
        for name, loss in (("mse", "mse"), ("rmse", F.rmse)):
            model = UNet(H, W, 3, 1, 0.5, "sigmoid", seed=40 + len(out))
            h5 = os.path.join(base, f"toy_{name}.h5")
            preds = [os.path.join(base, f"pred_{name}_{s}") for s in ("val", "test", "unlabeled")]
            res = F.train_depth_map(train, val, val, val, f"toy_{name}", h5, model, loss, 2, *preds)
            out[name] = dict(res=res, h5=h5, preds=preds)
    finally:
        F.NUM_EPOCHS, F.BATCH_SIZE = saved
    return dict(out, val=val)


@pytest.mark.parametrize("name", ["mse", "rmse"])
def test_train_depth_map(trained, name):
    t = trained[name]
    assert os.path.exists(t["h5"]) and len(t["res"]) == 6 and all(np.isfinite(v) for v in t["res"]), t["res"]
    best = F.load_model(t["h5"])
    names = sorted(os.listdir(trained["val"]))
    assert len(names) == 6
    x = torch.from_numpy(np.stack([F.read_png(os.path.join(trained["val"], n), 3) for n in names])).cuda()
    g = torch.from_numpy(np.stack([F.read_png(os.path.join(trained["val"].replace("images", "depth_maps"), n), 1) for n in names])).cuda()
    pred, sums = D.eval_depth(best.predict_device(x), g)
    per = H * W
    mse = sums[:, 0].sum() / (6 * per)
    batch_mse = [sums[:4, 0].sum() / (4 * per), sums[4:, 0].sum() / (2 * per)]      # validation batches of 4 in sorted order: 4 + 2
    loss = mse if name == "mse" else (4 * np.sqrt(batch_mse[0]) + 2 * np.sqrt(batch_mse[1])) / 6
    rmse_val, rmse_test, rmse_unl, mse_val, mse_test, mse_unl = t["res"]
    assert rmse_val == rmse_test == rmse_unl and mse_val == mse_test == mse_unl      # the three benchmarks saw the same directory
    assert abs(mse_val - mse) <= 1e-12 * mse and abs(rmse_val - loss) <= 1e-12 * loss
    assert 0 < mse < 0.25
    pred = pred.cpu().numpy()
    for d in t["preds"]:
        assert sorted(os.listdir(d)) == names
        for j, n in enumerate(names):
            assert np.array_equal(F.read_png(os.path.join(d, n), 1)[..., 0], pred[j]), (d, n)
    assert len(np.unique(pred)) > 8      # a depth map, not a mask


def test_im_of_the_two_trained_models(trained):
    models = [F.load_model(trained[n]["h5"]) for n in ("mse", "rmse")]
    names = sorted(os.listdir(trained["val"]))
    for n in names[:3]:
        x = F.read_png(os.path.join(trained["val"], n), 3)[None]
        out = F.get_im_prediction_depth_map(models, x)
        preds = np.stack([m.predict(x)[0, ..., 0] for m in models])
        mask, thr, _ = DC.im_depth(preds, 2)
        assert out.shape == (1, H, W, 1) and np.array_equal(out[0, ..., 0], mask.astype(int)), n
        assert np.isfinite(thr)
    # the fused ensemble call gives the same mask and blocks the image with it
    x = torch.from_numpy(np.stack([F.read_png(os.path.join(trained["val"], n), 3) for n in names])).cuda()
    r = D.EnsembleDepthIM(models).run(x, 2, True, want_std=True)
    for j, n in enumerate(names):
        preds = np.stack([m.predict(x[j:j + 1].cpu().numpy())[0, ..., 0] for m in models])
        mask, thr, std = DC.im_depth(preds, 2)
        assert np.array_equal(r["im"][j].cpu().numpy() == 255, mask) and DC.same_bits(r["thr"][j].cpu().numpy(), thr), n
        assert DC.same_bits(r["std"][j].cpu().numpy(), std), n
        want = x[j].cpu().numpy().copy()
        want[mask] = 0
        assert np.array_equal(r["img_out"][j].cpu().numpy(), want), n
