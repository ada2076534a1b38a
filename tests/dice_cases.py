"""The Dice loss of loss kind 4 (the reference's dice_loss, functions.py:162-184, smooth = 1) restated in float64 numpy: the loss, the
per-image sums and d loss / d logit, plus the torch form the GPU tests hand to the oracle.  tests/test_cpu_dice_rule.py checks this
restatement against the reference's recorded results and against float64 autograd; the GPU tests check the kernels against it.

    I_b = sum t p    U_b = sum t + sum p    dice_b = (2 I_b + 1) / (U_b + 1)      over the H W K elements of image b
    L = 1 - mean_b dice_b
    dL/dp = c0_b - c1_b t     c0_b = (2 I_b + 1) / (B (U_b + 1)^2)     c1_b = 2 / (B (U_b + 1))
    dL/dlogit = dL/dp * p (1 - p)                                                  (sigmoid head)
"""
import numpy as np

F64 = np.float64


def sums(t, p):
    """t, p [B,H,W,K] -> float64 [B,3] = (sum t p, sum t, sum p) per image"""
    t, p = np.asarray(t, F64), np.asarray(p, F64)
    ax = (1, 2, 3)
    return np.stack([(t * p).sum(ax), t.sum(ax), p.sum(ax)], 1)


def dice_from_sums(s, smooth=1.0):
    s = np.asarray(s, F64)
    return (2.0 * s[:, 0] + smooth) / (s[:, 1] + s[:, 2] + smooth)


def loss(t, p, smooth=1.0):
    return float(1.0 - dice_from_sums(sums(t, p), smooth).mean())


def coefficients(t, p, smooth=1.0):
    """-> (c0 [B], c1 [B]) in float64"""
    s = sums(t, p)
    b = s.shape[0]
    den = s[:, 1] + s[:, 2] + smooth
    return (2.0 * s[:, 0] + smooth) / (b * den * den), 2.0 / (b * den)


def dloss_dp(t, p, smooth=1.0):
    c0, c1 = coefficients(t, p, smooth)
    return c0[:, None, None, None] - c1[:, None, None, None] * np.asarray(t, F64)


def dloss_dlogit(t, p, smooth=1.0):
    p64 = np.asarray(p, F64)
    return dloss_dp(t, p, smooth) * p64 * (1.0 - p64)


# ---- the three defects a fixture must be able to tell from the rule (tests/golden/make_golden_dice_loss.py refuses one that cannot) ----
def defect_whole_batch(t, p, smooth=1.0):
    """one Dice over the whole batch instead of one per image"""
    t, p = np.asarray(t, F64), np.asarray(p, F64)
    return float(1.0 - (2.0 * (t * p).sum() + smooth) / (t.sum() + p.sum() + smooth))


def defect_no_smooth_below(t, p, smooth=1.0):
    """`smooth` missing from the denominator"""
    s = sums(t, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(1.0 - ((2.0 * s[:, 0] + smooth) / (s[:, 1] + s[:, 2])).mean())


def defect_dice_of_summed(t, p, smooth=1.0):
    """mean(1 - dice_b) replaced by 1 - dice of the images' summed I and U"""
    s = sums(t, p).sum(0)
    return float(1.0 - (2.0 * s[0] + smooth) / (s[1] + s[2] + smooth))


DEFECTS = {"whole_batch": defect_whole_batch, "no_smooth_below": defect_no_smooth_below, "dice_of_summed": defect_dice_of_summed}


# ---- torch ---------------------------------------------------------------------------------------------------------------------------
def torch_loss(t, p, smooth=1.0):
    """the same expression on torch tensors [B,H,W,K] (any float dtype): what autograd differentiates"""
    inter = (t * p).sum(dim=(1, 2, 3))
    union = t.sum(dim=(1, 2, 3)) + p.sum(dim=(1, 2, 3))
    return 1.0 - ((2.0 * inter + smooth) / (union + smooth)).mean()


def oracle_step(U, sd, x, tgt, cfg, emulate_fp16, loss_scale, override):
    """oracle/unet_oracle.train_step's gradient part with the Dice loss: U.forward in training mode with the conv outputs pinned to
    `override`, torch_loss on its probabilities, backward under the loss scale -> (loss, {name: gradient})"""
    import torch
    names = U.trainable_names(sd)
    leaves = {k: sd[k].clone().requires_grad_(True) for k in names}
    q = dict(sd)
    q.update(leaves)
    probs = U.forward(q, x, cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], training=True, emulate_fp16=emulate_fp16, override=override)
    lv = torch_loss(torch.as_tensor(np.asarray(tgt)).float(), probs)
    (lv * loss_scale).backward()
    return float(lv.detach()), {k: leaves[k].grad / loss_scale for k in names}
