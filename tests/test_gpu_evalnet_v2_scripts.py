"""The late-fusion EvalNet through the functions the scripts call: train_evalnet_miou_model_hela on a toy 128 x 128 tree, and the
checkpoint round trip through both formats (safetensors; IMK_MODEL_FORMAT=keras_h5, recognised by its 24 Conv2D / 13 BatchNormalization /
2 Dense layers).  A v1 file still loads as a v1 net."""
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

import evalnet_v2_cases as V  # noqa: E402
from tests.test_gpu_unet import randomize_bn  # noqa: E402


def _tree(root, n, seed):
    """brightfield / alive / dead / mod_position PNGs and labels.csv (name; three IoU values; three detection flags)"""
    from inconsistencymasks_amd import functions as F
    rng = np.random.default_rng(seed)
    for sub in ("brightfield", "alive", "dead", "mod_position"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    rows = []
    for i in range(n):
        name = f"img{i}.png"
        F.write_png(os.path.join(root, "brightfield", name), rng.integers(0, 256, (128, 128), dtype=np.uint8))
        for sub in ("alive", "dead", "mod_position"):
            F.write_png(os.path.join(root, sub, name), (rng.integers(0, 2, (16, 16), dtype=np.uint8) * 255).repeat(8, 0).repeat(8, 1))
        rows.append(";".join([name] + [f"{v:.4f}" for v in rng.random(3)] + [str(int(v)) for v in rng.integers(0, 2, 3)]))
    with open(os.path.join(root, "labels.csv"), "w", encoding="utf-8", newline="") as f:
        f.write("\r\n".join(rows) + "\r\n")


def test_train_evalnet_miou_model_hela_with_a_v2_net(tmp_path):
    from inconsistencymasks_amd import functions as F
    from inconsistencymasks_amd.evalnet import get_evalnet_miou_v2
    tr, va = str(tmp_path / "train"), str(tmp_path / "val")
    _tree(tr, 8, 1)
    _tree(va, 4, 2)
    net = get_evalnet_miou_v2(128, 128, 1, 3, alpha=0.5, seed=3)
    h5 = str(tmp_path / "evalnet_v2.h5")
    res = F.train_evalnet_miou_model_hela(net, tr, va, h5, 4, 2, seed=4)
    assert len(res) == 5 and np.isfinite(res).all(), res
    assert abs(res[0] - res[1] - res[2]) < 1e-6
    back = F.load_evalnet(h5)
    assert back.plan.arch == "v2" and back.plan.n_total == net.plan.n_total
    assert [l["name"] for l in back.plan.layers] == [t[0] for t in V.layer_table(1, 3, 3, 0.5)]


def _net(arch, seed):
    from inconsistencymasks_amd.evalnet import EvalNet
    cfg = V.CASES["hela"]
    m = EvalNet(cfg["h"], cfg["w"], cfg["ca"], cfg["cb"], cfg["cb"], cfg["alpha"], True, True, False, seed=seed, arch=arch)
    m.load_state_dict(randomize_bn(m.state_dict(), seed + 1))
    return m, cfg


@pytest.mark.parametrize("fmt", ["safetensors", "keras_h5"])
def test_checkpoint_round_trip(tmp_path, monkeypatch, fmt):
    from inconsistencymasks_amd import functions as F
    monkeypatch.setenv("IMK_MODEL_FORMAT", fmt)
    xa, xb, _ = V.make_inputs(V.CASES["hela"], 5)
    for arch in ("v2", "v1"):
        m, cfg = _net(arch, 70)
        want = m.predict([xa, xb])
        path = str(tmp_path / f"{arch}.h5")
        F.save_evalnet(m, path)
        back = F.load_evalnet(path)
        assert back.plan.arch == arch and (back.plan.h, back.plan.w) == (cfg["h"], cfg["w"])
        assert [l["name"] for l in back.plan.layers] == [l["name"] for l in m.plan.layers]
        assert torch.equal(back.params.cpu(), m.params.cpu())
        got = back.predict([xa, xb])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), arch


def test_keras_h5_names_follow_creation_order(tmp_path, monkeypatch):
    """conv2d .. conv2d_23 and batch_normalization .. batch_normalization_12 number the layers in creation order (tower A completely,
    tower B, trunk); `layer_names` lists them in the order of Keras' model.layers, the two towers interleaved by depth"""
    from inconsistencymasks_amd import functions as F, h5lite, keras_h5
    monkeypatch.setenv("IMK_MODEL_FORMAT", "keras_h5")
    m, cfg = _net("v2", 80)
    path = str(tmp_path / "v2.h5")
    F.save_evalnet(m, path)
    sd, meta = keras_h5.evalnet_state_dict_from_keras_h5(path)
    assert meta["arch"] == "v2" and (meta["ca"], meta["cb"], meta["n_out"], meta["alpha"]) == (1, 3, 3, 0.5)
    table = V.layer_table(1, 3, 3, 0.5)
    kn = keras_h5.evalnet_keras_layer_names(keras_h5.evalnet_layer_table(1, 3, 3, 0.5, True, "v2"))
    assert keras_h5.evalnet_layer_table(1, 3, 3, 0.5, True, "v2") == table
    assert kn["a.in.c"] == "conv2d" and kn["a4.c1"] == "conv2d_8" and kn["b.in.c"] == "conv2d_9" and kn["m1.c3"] == "conv2d_18"
    assert kn["m3.c1"] == "conv2d_23" and kn["b.in.bn"] == "batch_normalization_5" and kn["m3.bn"] == "batch_normalization_12"
    want = m.state_dict()
    for k, v in sd.items():
        assert np.array_equal(np.asarray(v), want[k].numpy()), k
    with h5lite.File(path) as f:
        order = [n.decode() if isinstance(n, bytes) else n for n in h5lite.load_attr_list(f, "layer_names")]
    assert order[:4] == ["conv2d", "conv2d_9", "batch_normalization", "batch_normalization_5"] and order[-2:] == ["iou", "detection"]
    assert sorted(order) == sorted(kn.values())
