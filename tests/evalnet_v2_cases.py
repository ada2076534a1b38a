"""CPU restatement of the late-fusion EvalNet, get_evalnet_miou_v2 (evalnet.py:76-106), and the cases its tests share.  TEST
INFRASTRUCTURE ONLY; the interface is oracle/evalnet_oracle.py's, the primitives are oracle/unet_oracle.py's.

  input_block = [Lambda x/255 if normalize] -> Conv1x1+ReLU -> BN                       (evalnet.py:4-11)
  conv_block  = Conv3x3+ReLU -> Conv1x1+ReLU -> BN -> MaxPooling2D(2,2)                 (evalnet.py:14-21)
  a = input_block(A, 16a) -> conv_block x4 at 16a, 32a, 64a, 128a;  b = the same on B   (evalnet.py:80-90)
  c = add([a, b])                                                                       (evalnet.py:96)
  c = conv_block x3 at 64a, 128a, 256a;  GlobalAvgPool2D;  Dense 'iou', 'detection'     (evalnet.py:98-104)

Parameter order = Keras' creation order: tower A completely, tower B, the trunk, the heads.  MaxPooling2D is 'valid': an odd last
row / column is dropped.  Under mixed_float16 the Add layer takes two fp16 tensors and yields fp16: the exact sum rounded once.
Parity status: PARITY UNPINNED, like oracle/evalnet_oracle.py -- the reference runs this network inside Keras."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_oracle as U
from oracle.evalnet_oracle import loss_fn, one_hot  # noqa: F401

TOWER = (16, 32, 64, 128)
TRUNK = (64, 128, 256)
HEADS = ("iou", "detection")

# the smallest shapes that still reach every path (seven poolings: 128 x 128 is the smallest input)
CASES = {
    "hela": dict(h=128, w=128, ca=1, cb=3, alpha=0.5, b=4),                   # narrow kernels; the last BatchNorm over 16 samples
    "alpha2": dict(h=128, w=128, ca=1, cb=3, alpha=2.0, b=2),                 # GEMM-class families; the trunk up to 512 channels
    "suim": dict(h=128, w=128, ca=3, cb=9, alpha=1.0, b=3, onehot=True),      # one-hot input B
    # towers 152 -> 76 -> 38 -> 19 -> 9 and 208 -> ... -> 13; trunk 9 x 13 -> 4 x 6 -> 2 x 3 -> 1 x 1: a drop inside a tower, at the add's
    # source and twice in the trunk
    "odd": dict(h=152, w=208, ca=3, cb=35, alpha=0.5, b=2, onehot=True),
}


def layer_table(ca, cb, n_out, alpha, two_heads=True):
    """Ordered (name, kind, k, cin, cout), Keras creation order of evalnet.py:76-104."""
    assert two_heads, "get_evalnet_miou_v2 has the two heads only"
    f = lambda v: int(v * alpha)
    t = []

    def block(name, ci, co):
        return [(f"{name}.c3", "conv", 3, ci, co), (f"{name}.c1", "conv", 1, co, co), (f"{name}.bn", "bn", 0, co, co)]

    prev = f(16)
    for tw, cin in (("a", ca), ("b", cb)):
        t += [(f"{tw}.in.c", "conv", 1, cin, f(16)), (f"{tw}.in.bn", "bn", 0, f(16), f(16))]
        prev = f(16)
        for j, v in enumerate(TOWER, start=1):
            t += block(f"{tw}{j}", prev, f(v))
            prev = f(v)
    for i, v in enumerate(TRUNK, start=1):
        t += block(f"m{i}", prev, f(v))
        prev = f(v)
    return t + [("iou", "conv", 1, prev, n_out), ("detection", "conv", 1, prev, n_out)]


def count_params(ca, cb, n_out, alpha, two_heads=True):
    total = trainable = 0
    for name, kind, k, ci, co in layer_table(ca, cb, n_out, alpha, two_heads):
        if kind == "conv":
            total += k * k * ci * co + co
            trainable += k * k * ci * co + co
        else:
            total += 4 * co
            trainable += 2 * co
    return total, trainable


def init_weights(ca, cb, n_out, alpha, two_heads=True, seed=0):
    gen = torch.Generator().manual_seed(seed)
    w = {}
    for name, kind, k, ci, co in layer_table(ca, cb, n_out, alpha, two_heads):
        if kind == "conv":
            if name in HEADS:      # Keras Dense default: glorot_uniform
                lim = math.sqrt(6.0 / (ci + co))
                w[name + ".w"] = (torch.rand((1, 1, ci, co), generator=gen) * 2 - 1) * lim
            else:
                w[name + ".w"] = U.he_normal_((k, k, ci, co), k * k * ci, gen)
            w[name + ".b"] = torch.zeros(co)
        else:
            w[name + ".gamma"] = torch.ones(co)
            w[name + ".beta"] = torch.zeros(co)
            w[name + ".mean"] = torch.zeros(co)
            w[name + ".var"] = torch.ones(co)
    return w


class _AddF16(torch.autograd.Function):
    """fp16(a + b) of two fp16-valued tensors with ONE rounding: the sum is exact in float64 (fp16 spans 2^-24 .. 2^16, 40 bits, plus 11
    of significand) and numpy's float64 -> float16 conversion is correctly rounded.  The gradient of the sum is the gradient of both
    addends, stored in fp16 like every activation gradient."""

    @staticmethod
    def forward(ctx, a, b):
        return torch.from_numpy((a.double() + b.double()).numpy().astype(np.float16).astype(np.float32))

    @staticmethod
    def backward(ctx, g):
        g = g.half().float()
        return g, g


def forward(p, xa_u8, xb_u8, two_heads=True, normalize_a=True, normalize_b=False, training=False, emulate_fp16=False,
            stats_out=None, taps=None, override=None, sums=None):
    """xa [B,H,W,Ca], xb [B,H,W,Cb] uint8 (one-hot nets: one_hot(class ids)) -> (outputs [B, 2K] float32, logits).  `sums`, if a
    dict, receives the two pooled tower outputs "a", "b" and their sum "sum", NHWC."""
    f16 = emulate_fp16

    def nhwc(t):
        return t.detach().permute(0, 2, 3, 1).contiguous()

    def c(name, t):
        if override is not None and name in override:
            ov = torch.as_tensor(override[name]).float().permute(0, 3, 1, 2)
            pre = U._conv(t, p[name + ".w"], p[name + ".b"], False, f16)
            mask = (ov > 0).float()
            y = pre * mask + (ov - pre * mask).detach()
        else:
            y = U._conv(t, p[name + ".w"], p[name + ".b"], True, f16)
        if taps is not None:
            taps[name] = nhwc(y)
        return y

    def bn(name, t):
        return U._bn(t, p, name, training, f16, stats_out)

    def block(name, t):
        return F.max_pool2d(bn(f"{name}.bn", c(f"{name}.c1", c(f"{name}.c3", t))), 2)      # floor: the odd last row / column is dropped

    def tower(tw, x_u8, normalize):
        x = torch.as_tensor(np.asarray(x_u8)).float().permute(0, 3, 1, 2)
        if normalize:
            x = x / 255.0
        y = bn(f"{tw}.in.bn", c(f"{tw}.in.c", U._r(x, f16)))
        for j in range(1, 5):
            y = block(f"{tw}{j}", y)
        return y

    a, b = tower("a", xa_u8, normalize_a), tower("b", xb_u8, normalize_b)
    y = _AddF16.apply(a, b) if f16 else a + b
    if sums is not None:
        sums.update(a=nhwc(a), b=nhwc(b), sum=nhwc(y))
    for i in range(1, 4):
        y = block(f"m{i}", y)
    feat = y.mean(dim=(2, 3))                       # GlobalAvgPool2D, fp32
    logits = torch.cat([feat @ p[h + ".w"][0, 0] + p[h + ".b"] for h in HEADS], dim=1)
    return torch.sigmoid(logits), logits


def grads(p, xa, xb, y, two_heads=True, normalize_a=True, normalize_b=False, emulate_fp16=False, loss_scale=1.0, override=None):
    """One training-mode forward + backward.  Returns (losses tuple of floats, outputs, grads dict, batch stats)."""
    names = U.trainable_names(p)
    leaves = {k: p[k].clone().requires_grad_(True) for k in names}
    q = dict(p)
    q.update(leaves)
    stats = {}
    out, logits = forward(q, xa, xb, True, normalize_a, normalize_b, training=True, emulate_fp16=emulate_fp16, stats_out=stats,
                          override=override)
    total, l0, l1 = loss_fn(out, logits, y, True)
    (total * loss_scale).backward()
    g = {k: leaves[k].grad / loss_scale for k in names}
    return (float(total.detach()), float(l0.detach()), float(l1.detach())), out.detach(), g, stats


def make_inputs(cfg, seed):
    """-> (xa u8 [B,H,W,ca], xb u8 (mask stack [B,H,W,cb], or class ids [B,H,W,1] for a one-hot net), y f32 [B, 2*cb])"""
    rng = np.random.default_rng(seed)
    b, h, w = cfg["b"], cfg["h"], cfg["w"]
    yy, xx = np.mgrid[0:h, 0:w]
    xa = (127 + 80 * np.sin(xx / 7.0)[None, :, :, None] * np.cos(yy / 5.0)[None, :, :, None]
          + rng.integers(-30, 30, (b, h, w, cfg["ca"]))).clip(0, 255).astype(np.uint8)
    if cfg.get("onehot"):
        xb = rng.integers(0, cfg["cb"], (b, h // 8, w // 8, 1)).astype(np.uint8).repeat(8, 1).repeat(8, 2)
    else:
        xb = ((rng.random((b, h // 8, w // 8, cfg["cb"])) > 0.6).astype(np.uint8) * 255).repeat(8, 1).repeat(8, 2)
    y = rng.random((b, 2 * cfg["cb"])).astype(np.float32)
    y[:, cfg["cb"]:] = (y[:, cfg["cb"]:] > 0.5)
    return xa, xb, y


def oracle_b(cfg, xb):
    """input B as the restatement takes it"""
    return one_hot(xb, cfg["cb"]) if cfg.get("onehot") else xb
