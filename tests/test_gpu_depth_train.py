"""Loss kinds 2 and 3 of imk_unet_fwd_bwd: training on the continuous targets float32(y) / 255.0f of the depth-map family.

  * kind 2 with y in {0,255} is kind 0 with y in {0,1}, bit for bit (loss, every gradient, the parameters after imk_unet_adamw_step),
    on both head routes: imk_head_mse_fused_ok (csrc/imk_headf.hip) takes a last decoder width of 8 (padded) channels with one map --
    alpha 0.5 -- and rejects everything else -- alpha 1.25: 20 channels, padded to 24, head_loss_kernel + the head's dgrad;
  * kind 2 with random y against oracle/unet_oracle.train_step(target = y / 255, "mse") with the project's tolerances: loss 1e-4
    relative, every gradient tensor rel-L2 <= 2e-2 with the oracle's forward values pinned to the GPU's;
  * kind 3 (rmse): the gradients are kind 2's times fl32(0.5f / fl32(sqrt(mse))) bit for bit, stats[0] is the square root;
  * a batch with mse == 0 is skipped;  * both kinds are bit-reproducible."""
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

import test_gpu_unet as TU  # noqa: E402  (make_input, randomize_bn, first_finite_step, rel_l2: the procedure of test_train_step_parity)
from inconsistencymasks_amd.unet import UNet  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402

F32 = np.float32
# name -> (configuration, the head route it takes)
CFGS = {"fused_head": dict(h=32, w=32, c=3, k=1, alpha=0.5, act="sigmoid", loss="mse", b=2),
        "loss_then_dgrad": dict(h=64, w=64, c=3, k=1, alpha=1.25, act="sigmoid", loss="mse", b=2)}


def _model(cfg, seed=21):
    m = UNet(cfg["h"], cfg["w"], cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], seed=seed)
    sd = TU.randomize_bn(m.state_dict(), seed + 1)
    m.load_state_dict(sd)
    return m, sd


def _bits(t):
    return t.contiguous().view(torch.int32)


def _batch(cfg, seed):
    x, _, _ = TU.make_input(cfg, seed)
    y = np.random.default_rng(seed).integers(0, 256, (cfg["b"], cfg["h"], cfg["w"], cfg["k"]), dtype=np.uint8)
    return x, y


@pytest.mark.parametrize("name", list(CFGS))
def test_kind2_on_0_255_is_kind0_on_0_1(name):
    cfg = CFGS[name]
    x, y01, _ = TU.make_input(cfg, 5)
    assert set(np.unique(y01)) == {0, 1}
    xd, y0, y2 = torch.from_numpy(x).cuda(), torch.from_numpy(y01).cuda(), torch.from_numpy(y01 * np.uint8(255)).cuda()
    (m0, _), (m2, _) = _model(cfg), _model(cfg)
    applied = 0
    for step in range(6):      # the dynamic loss scale skips the first steps at 2^15: both models alike
        m0.fwd_bwd(xd, y0, 0)
        m2.fwd_bwd(xd, y2, 2)
        assert torch.equal(_bits(m0.stats), _bits(m2.stats)), (step, m0.stats, m2.stats)
        assert torch.equal(_bits(m0.grads), _bits(m2.grads)), step
        applied += int(m0.stats[1] == 0)
        m0.adamw_step(3e-3, 1e-4)
        m2.adamw_step(3e-3, 1e-4)
        assert torch.equal(_bits(m0.params), _bits(m2.params)), step
    assert applied >= 2


# The oracle comparison runs at tests/test_gpu_unet.py's own `isic` shape for the fused head (64 x 64, batch 4): at 32 x 32 x 2 the stem's
# bias gradient `in.c.b` -- a sum of ReLU-masked terms whose unmasked sum is exactly zero behind the BatchNorm, the one
# cancellation-dominated tensor (test_gpu_unet.train_step_parity says so) -- is 0.106 rel-L2 from the oracle's while every other tensor
# is within 2e-2; the bound is the project's, so the shape is the one the project holds it at.
ORACLE_CFGS = {"fused_head": TU.CFGS["isic"], "loss_then_dgrad": CFGS["loss_then_dgrad"]}


@pytest.mark.parametrize("name", list(ORACLE_CFGS))
def test_kind2_against_the_oracle(name):
    """test_gpu_unet.train_step_parity's procedure with loss kind 2 and the targets y / 255"""
    cfg = ORACLE_CFGS[name]
    c, k, alpha, act, b = cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], cfg["b"]
    m, sd = _model(cfg, 11)
    x, y = _batch(cfg, 13)
    tgt = y.astype(F32) / F32(255.0)
    scale = 32768.0
    while True:
        stats = TU.first_finite_step(m, sd, x, y, 2, scale)
        g1 = m.grads.clone()
        m.fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 2)
        assert torch.equal(_bits(g1), _bits(m.grads))      # bit-reproducible
        ov = {l["name"]: m.intermediate(l["name"], b, 1) for l in m.plan.layers if l["kind"] == 0 and l["name"] != "out"}
        sd_ref = {kk: v.clone() for kk, v in sd.items()}
        loss_ref, grads_ref = U.train_step(sd_ref, U.new_opt_state(sd_ref), x, tgt, c, k, alpha, act, "mse", emulate_fp16=True,
                                           loss_scale=float(stats[2]), return_grads=True, override=ov)
        if all(bool(torch.isfinite(v).all()) for v in grads_ref.values()):
            break
        scale = float(stats[2]) / 2      # the oracle's step overflows where the GPU's survived: both skip (as train_step_parity)
        assert scale >= 1.0
        m.load_state_dict(sd)
    print(f"{name}: loss {stats[0]!r} against {loss_ref!r}")
    assert abs(stats[0] - loss_ref) <= 1e-4 * abs(loss_ref)
    g, errs = g1.cpu(), {}
    for l in m.plan.layers:
        n = l["name"]
        if l["kind"] == 0:
            kk, ci, co = l["ksize"], l["cin"], l["cout"]
            errs[n + ".w"] = TU.rel_l2(g[l["off_w"]:l["off_w"] + kk * kk * ci * co].reshape(kk, kk, ci, co).numpy(), grads_ref[n + ".w"].numpy())
            errs[n + ".b"] = TU.rel_l2(g[l["off_b"]:l["off_b"] + co].numpy(), grads_ref[n + ".b"].numpy())
        else:
            cc = l["cout"]
            errs[n + ".gamma"] = TU.rel_l2(g[l["off_w"]:l["off_w"] + cc].numpy(), grads_ref[n + ".gamma"].numpy())
            errs[n + ".beta"] = TU.rel_l2(g[l["off_b"]:l["off_b"] + cc].numpy(), grads_ref[n + ".beta"].numpy())
    print(f"{name}: worst gradient tensor {max(errs, key=errs.get)} at {max(errs.values()):.4f} rel-L2")
    bad = {kk: round(v, 4) for kk, v in errs.items() if not v <= 2e-2}
    assert not bad, f"gradient tensors off by more than 2e-2 rel-L2: {bad}"


@pytest.mark.parametrize("name", list(CFGS))
def test_kind3_is_kind2_scaled(name):
    cfg = CFGS[name]
    x, y = _batch(cfg, 7)
    (m2, sd), (m3, _) = _model(cfg), _model(cfg)
    s2 = TU.first_finite_step(m2, sd, x, y, 2)
    s3 = TU.first_finite_step(m3, sd, x, y, 3)
    assert s2[2] == s3[2]                              # the same loss scale
    mse = F32(s2[0])
    root = np.sqrt(mse)
    assert F32(s3[0]).view(np.uint32) == root.view(np.uint32) and s3[1] == 0.0
    want = m2.grads.cpu().numpy() * (F32(0.5) / root)
    got = m3.grads.cpu().numpy()
    assert want.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.count_nonzero(got) > got.size // 2 and np.isfinite(got).all()
    g3 = m3.grads.clone()                              # bit-reproducible
    m3.fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 3)
    assert torch.equal(_bits(g3), _bits(m3.grads)) and float(m3.stats[0]) == float(root)
    before = m3.params.clone()
    m3.adamw_step(3e-3, 1e-4)
    assert not torch.equal(before, m3.params)


@pytest.mark.parametrize("name", list(CFGS))
def test_rmse_of_an_all_equal_batch_is_skipped(name):
    """out.w = 0 and out.b = 30: every probability is sigmoid(30) = 1.0f exactly, the targets 255 / 255.0f = 1.0f: mse == 0.  rmse's
    gradient is 0 / 0 there; the step sets the overflow flag and imk_unet_adamw_step leaves the parameters alone and halves the loss
    scale.  'mse' (kind 2) on the same batch is an ordinary step with zero gradients."""
    cfg = CFGS[name]
    x, _ = _batch(cfg, 9)
    y = np.full((cfg["b"], cfg["h"], cfg["w"], 1), 255, np.uint8)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for kind in (3, 2):
        m, sd = _model(cfg)
        sd["out.w"] = torch.zeros_like(sd["out.w"])
        sd["out.b"] = torch.full_like(sd["out.b"], 30.0)
        m.load_state_dict(sd)
        m.init_train_state()
        m.fwd_bwd(xd, yd, kind)
        stats = m.stats.cpu().numpy()
        assert stats[0] == 0.0 and stats[1] == (1.0 if kind == 3 else 0.0), (kind, stats)
        nt = m.plan.n_trainable
        before = m.params[:nt].clone()
        m.adamw_step(3e-3, 1e-4)
        m.fwd_bwd(xd, yd, kind)
        scale_after = float(m.stats[2])
        if kind == 3:
            assert torch.equal(before, m.params[:nt]) and scale_after == float(stats[2]) / 2
        else:
            assert not torch.equal(before, m.params[:nt]) and scale_after == float(stats[2])      # the weight decay moved them


def test_refusals():
    soft = UNet(32, 32, 3, 4, 0.5, "softmax", seed=1)
    x = torch.zeros((1, 32, 32, 3), dtype=torch.uint8, device="cuda")
    y = torch.zeros((1, 32, 32, 4), dtype=torch.uint8, device="cuda")
    from inconsistencymasks_amd._lib import ImkError
    for kind in (2, 3, 4, -1):
        with pytest.raises(ImkError):
            soft.fwd_bwd(x, y, kind)
    from inconsistencymasks_amd import depth as D
    from inconsistencymasks_amd import functions as F
    assert D._loss_kind("mse", "t") == 2 and D._loss_kind(F.rmse, "t") == 3
    for bad in (F.dice_loss, "mae", F.ignore_im_dice_loss_multiclass()):
        with pytest.raises(NotImplementedError):
            D._loss_kind(bad, "train_depth_map")
