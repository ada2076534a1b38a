"""Cases, inputs and the torch-CPU oracle of the consistency-loss step (a plain helper module, imported by
tests/test_cpu_consistency_yardstick.py, tests/test_gpu_consistency.py and tests/test_gpu_consistency_buffer_contract.py).

The step (functions.py:367-474 of the reference): p1 = model(v1, training=True), p2 = model(v2, training=True) as two separate
calls, L = mean((p1 - p2)^2) over B*H*W*K on the fp32 head outputs, the gradient w.r.t. the trainable variables through BOTH
forwards; every BatchNorm normalises with its own view's batch statistics and moves the moving statistics twice, view 1 first.
The oracle composes that from oracle/unet_oracle.py: two forward() calls on shared leaves, one backward.
"""
import numpy as np
import torch

from oracle import unet_oracle as U

# the cases of tests/test_gpu_unet.py that can still break the two-view head:
#   isic    64x64, batch 4, K 1 on 8 channels: the fused kernel, one lane per pixel
#   hela    32x48, one input channel, K 3 on 16 channels: the fused kernel, two lanes per pixel, not square
#   suim    48x64, softmax K 9: composed route
#   tiny16  16x16, batch 5: one tile per image, odd batch, softmax
#   alpha2  32x48, sigmoid on 32 channels: a width the fused kernel does not cover, so composed
CASES = {
    "isic": dict(h=64, w=64, c=3, k=1, alpha=0.5, act="sigmoid", b=4),
    "hela": dict(h=32, w=48, c=1, k=3, alpha=1.0, act="sigmoid", b=3),
    "suim": dict(h=48, w=64, c=3, k=9, alpha=1.0, act="softmax", b=2),
    "tiny16": dict(h=16, w=16, c=3, k=3, alpha=1.0, act="softmax", b=5),
    "alpha2": dict(h=32, w=48, c=3, k=1, alpha=2.0, act="sigmoid", b=2),
}
FUSED = ("isic", "hela")        # imk_consistency_fused_ok: sigmoid, K 1 / 3, 8 / 16 padded channels
MODEL_SEED, BN_SEED, INPUT_SEED = 51, 52, 53


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30)))


def randomize_bn(sd, seed):
    """tests/test_gpu_unet.py::randomize_bn"""
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if k.endswith(".gamma"):
            sd[k] = 0.8 + 0.4 * torch.rand(sd[k].shape, generator=g)
        elif k.endswith(".beta"):
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith(".mean"):
            sd[k] = 0.4 + 0.1 * torch.randn(sd[k].shape, generator=g)
        elif k.endswith(".var"):
            sd[k] = 0.5 + 0.5 * torch.rand(sd[k].shape, generator=g)
        elif k.endswith(".b"):
            sd[k] = 0.05 * torch.randn(sd[k].shape, generator=g)
    return sd


def weights(cfg):
    """the case's weights without a GPU: unet_oracle's initialisation with perturbed BatchNorm parameters and biases"""
    return randomize_bn(U.init_weights(cfg["c"], cfg["k"], cfg["alpha"], MODEL_SEED), BN_SEED)


def make_views(cfg, seed=INPUT_SEED):
    """one random image batch (the smooth pattern + noise of tests/test_gpu_unet.py::make_input) under two different noise draws"""
    rng = np.random.default_rng(seed)
    h, w, c, b = cfg["h"], cfg["w"], cfg["c"], cfg["b"]
    yy, xx = np.mgrid[0:h, 0:w]
    base = (127 + 80 * np.sin(xx / 7.0)[None, :, :, None] * np.cos(yy / 5.0)[None, :, :, None] + rng.integers(-30, 30, (b, h, w, c)))
    v1 = (base + rng.integers(-25, 26, (b, h, w, c))).clip(0, 255).astype(np.uint8)
    v2 = (base + rng.integers(-25, 26, (b, h, w, c))).clip(0, 255).astype(np.uint8)
    return v1, v2


def two_view_step(sd, v1, v2, cfg, emulate_fp16, loss_scale=1.0, ov1=None, ov2=None):
    """-> (loss, {name: gradient}, {name: moving statistic after the step}).  ov1 / ov2 pin the stored conv outputs of each view's
    forward (unet_oracle.forward's `override`)."""
    c, k, alpha, act = cfg["c"], cfg["k"], cfg["alpha"], cfg["act"]
    names = U.trainable_names(sd)
    leaves = {n: sd[n].clone().requires_grad_(True) for n in names}
    q = dict(sd)
    q.update(leaves)
    st1, st2 = {}, {}
    p1 = U.forward(q, v1, c, k, alpha, act, training=True, emulate_fp16=emulate_fp16, stats_out=st1, override=ov1)
    p2 = U.forward(q, v2, c, k, alpha, act, training=True, emulate_fp16=emulate_fp16, stats_out=st2, override=ov2)
    loss = ((p1 - p2) ** 2).mean()
    (loss * loss_scale).backward()
    grads = {n: (leaves[n].grad / loss_scale).detach() for n in names}
    moving = {}
    for name in st1:      # moving = moving * m + batch * (1 - m), view 1 first
        mean, var = sd[name + ".mean"].clone(), sd[name + ".var"].clone()
        for st in (st1, st2):
            mean = mean * U.BN_MOMENTUM + st[name][0] * (1 - U.BN_MOMENTUM)
            var = var * U.BN_MOMENTUM + st[name][1] * (1 - U.BN_MOMENTUM)
        moving[name + ".mean"], moving[name + ".var"] = mean, var
    return float(loss.detach()), grads, moving


def yardstick(sd, v1, v2, cfg, ov1, ov2, loss_scale=1.0):
    """The distance, per gradient tensor, between the oracle's fp16-emulating and fp32 forms of the same two-view gradient on the
    same pinned forward values: what fp16 storage alone costs a gradient that is a sum of two partly cancelling contributions.
    -> (fp16 form's loss, its gradients, its moving statistics, {name: rel-L2(fp16 form, fp32 form)}, fp32 form's gradients)"""
    loss16, g16, mov16 = two_view_step(sd, v1, v2, cfg, True, loss_scale, ov1, ov2)
    _, g32, _ = two_view_step(sd, v1, v2, cfg, False, 1.0, ov1, ov2)
    return loss16, g16, mov16, {n: rel_l2(g16[n].numpy(), g32[n].numpy()) for n in g16}, g32


def grad_bound(distance):
    """the labelled step's 2e-2, or 1.5 x the yardstick where that is larger (the margin check_against_fp32 gives)"""
    return max(2e-2, 1.5 * distance)
