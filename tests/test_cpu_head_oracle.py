"""oracle/head_oracle.py (the output layer alone, numpy float64) against torch float64 autograd and against the head of the whole-network
oracle; the yardsticks tests/test_gpu_heads.py holds the HIP heads to; and planted defects that must land outside those bounds.

The bounds (the GPU test computes them with the functions of this file, on its own data):
  * inference: max |p_gpu - p_64| <= INFER_FACTOR x max |p_32 - p_64|, p_32 = `head_f32`, a plain numpy float32 evaluation of the same
    head on the same x.  Factor 8 = 4 (the kernels' split weights hi + lo carry 22 of float32's 24 bits) x 2 (one ulp each for the
    hardware exponential and the reciprocal).  Rows of a softmax sum to 1 within K x that bound.
  * training, per quantity the head alone owns (gradients of out.w, out.b, the last BatchNorm's gamma and beta): rel-L2 to the NEARER of
    the two references (logit gradient rounded to fp16, or not) <= TRAIN_MARGIN x (d_round + d_stat); d_round = rel-L2 between those two
    references, d_stat = rel-L2 between the reference and itself with the BatchNorm scale and shift both moved up by 4 float32 ulps (a kernel
    reduces its batch statistics from fp32 partial rows, so it cannot have the float64 statistics' scale and shift; both moved the same
    way is the worst case for x = z sc + sh with z >= 0).  Margin 2: both yardsticks are extremes (every gradient rounded, a 4-ulp move
    of every channel); the factor covers fp32 summation order over the pixels.  Loss: 1e-6 relative + the loss's own d_stat.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import head_oracle as H  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402

INFER_FACTOR = 8.0
TRAIN_MARGIN = 2.0
LOSS_RTOL = 1e-6
STAT_ULPS = 4

# padded channel stride of the last decoder block -> (alpha, its real width int(16 alpha))
WIDTHS = {8: (0.5, 8), 16: (1.0, 16), 24: (1.25, 20), 32: (2.0, 32)}
SOFTMAX_K = (2, 15, 16, 17, 32, 33, 48, 49, 63, 64)      # tile edges of the 16-class tiles: full tiles, one class in the last, KT 1..4
SIGMOID_K = (1, 3, 4, 7)
INFER_CASES = [(cs, act, k) for cs in WIDTHS for act, ks in (("softmax", SOFTMAX_K), ("sigmoid", SIGMOID_K)) for k in ks]

# training cases: (cs, K, activation, loss, the kernel form the step takes by imk_launch_head_cce_fused's rule: CSV = 16 for cs <= 16 else
# 32, KT = ceil(K / 16); sigmoid heads: head_mse_fused_kernel<8,1> for (cs 8, K 1) only, else head_loss_kernel<cs> + the head's dgrad)
TRAIN_CASES = [
    (8, 17, "softmax", "cce", "head_cce_fused_kernel<16,2>"), (8, 33, "softmax", "cce", "head_cce_fused_kernel<16,3>"),
    (8, 64, "softmax", "cce", "head_cce_fused_kernel<16,4>"),
    (16, 16, "softmax", "cce", "head_cce_fused_kernel<16,1>"), (16, 35, "softmax", "cce", "head_cce_fused_kernel<16,3>"),
    (16, 49, "softmax", "cce", "head_cce_fused_kernel<16,4>"),
    (24, 32, "softmax", "cce", "head_cce_fused_kernel<32,2>"), (24, 64, "softmax", "cce", "head_cce_fused_kernel<32,4>"),
    (32, 2, "softmax", "cce", "head_cce_fused_kernel<32,1>"), (32, 48, "softmax", "cce", "head_cce_fused_kernel<32,3>"),
    (8, 3, "sigmoid", "mse", "head_loss_kernel<8>"), (8, 4, "sigmoid", "mse", "head_loss_kernel<8>"),
    (24, 1, "sigmoid", "mse", "head_loss_kernel<24>"), (32, 4, "sigmoid", "mse", "head_loss_kernel<32>"),
]


def case_id(case):
    return "-".join(str(v) for v in case[:3])


# ---- the batch of a training case ------------------------------------------------------------------------------------------------------------
# The whole-step comparison (test_train_step_parity's procedure) bounds EVERY gradient tensor by 2e-2 rel-L2.  On the 2048 pixels of these
# cases that bound presupposes a batch on which the reference itself is unambiguous: the stem's bias gradient is a sum of ReLU-masked terms
# whose unmasked sum is exactly zero behind the BatchNorm, and on some batches what is left of it is smaller than the fp16 rounding of its
# terms (first seen with K = 3 on alpha 0.5: the oracle with and without the fp16 rounding of that one gradient 0.27 apart, the GPU 0.21
# from the first -- a statement about the batch, not about a kernel).  So a case takes the first batch seed from 13 (the procedure's own) up
# on which the oracle ALONE is conditioned: its gradients with the fp16 rounding of the gradients in front of a BatchNorm (the pinned form
# the GPU is compared with) and without it (the unpinned form) within COND_LIMIT = a quarter of the bound, for every tensor, at the scale
# where its step is finite.  Nothing of the code under test enters the choice.
COND_LIMIT = 5e-3
_BATCHES = {}


def oracle_conditioning(cfg, x, tgt):
    """-> (the largest distance between the oracle's two roundings over the gradient tensors, its tensor's name)"""
    import test_gpu_unet as TU
    c, k, alpha, act = cfg["c"], cfg["k"], cfg["alpha"], cfg["act"]
    sd = TU.randomize_bn(U.init_weights(c, k, alpha, 11), 12)
    taps = {}
    U.forward(sd, x, c, k, alpha, act, training=True, emulate_fp16=True, taps=taps)

    def step(scale, ov):
        q = {n: v.clone() for n, v in sd.items()}
        return U.train_step(q, U.new_opt_state(q), x, tgt, c, k, alpha, act, cfg["loss"], emulate_fp16=True, loss_scale=scale,
                            return_grads=True, override=ov)[1]
    scale = 32768.0
    while True:
        pinned = step(scale, taps)
        if all(bool(torch.isfinite(v).all()) for v in pinned.values()):
            break
        scale /= 2
    plain = step(scale, None)
    d = {n: rel_l2(pinned[n].numpy(), plain[n].numpy()) for n in pinned}
    worst = max(d, key=d.get)
    return d[worst], worst


def training_batch(case):
    """-> (cfg, (x, y, tgt), seed): 32 x 32 images at batch 2, drawn as test_train_step_parity draws them; labels of a cce case contain
    class 0 and class K - 1"""
    import test_gpu_unet as TU
    if case not in _BATCHES:
        cs, k, act, loss, _ = case
        cfg = dict(h=32, w=32, c=3, k=k, alpha=WIDTHS[cs][0], act=act, loss=loss, b=2)
        for seed in range(13, 13 + 32):
            x, y, tgt = TU.make_input(cfg, seed)
            if loss == "cce":
                y[0, 0, 0], y[0, 0, 1] = 0, k - 1
                tgt = np.eye(k, dtype=np.float32)[y]
            if oracle_conditioning(cfg, x, tgt)[0] <= COND_LIMIT:
                break
        else:
            raise AssertionError(f"no conditioned batch for {case_id(case)} among 32 seeds")
        _BATCHES[case] = (cfg, (x, y, tgt), seed)
    return _BATCHES[case]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-300)))


# ---- the data both suites draw ------------------------------------------------------------------------------------------------------
def draw_head_params(cin, k, seed):
    """The last BatchNorm and the output layer of a case: gamma in [51, 77] / 64 and beta in [-8, 8] / 64 (multiples of 1/64, so that
    z * gamma + beta is exact in float64 AND in the kernels' single-rounding fma), He-normal W as `init_weights` draws it, a small random
    bias as `randomize_bn` draws it.  float32."""
    rng = np.random.default_rng(seed)
    gamma = (rng.integers(51, 78, cin) / 64.0).astype(np.float32)
    beta = (rng.integers(-8, 9, cin) / 64.0).astype(np.float32)
    w = U.he_normal_((cin, k), cin, torch.Generator().manual_seed(int(seed))).numpy()
    b = (0.05 * rng.standard_normal(k)).astype(np.float32)
    return gamma, beta, w, b


def synthetic_z(cin, seed, n_pix=2048):
    """a stand-in for the stored last activation: post-ReLU, fp16-valued, a third of it zero"""
    rng = np.random.default_rng(seed)
    return np.maximum(rng.standard_normal((n_pix, cin)) * 0.9 + 0.4, 0).astype(np.float16).astype(np.float32)


def synthetic_target(k, loss, seed, n_pix=2048):
    rng = np.random.default_rng(seed)
    if loss == "mse":
        return (rng.random((n_pix, k)) > 0.6).astype(np.float32)
    y = rng.integers(0, k, n_pix)
    y[0], y[1] = 0, k - 1
    return np.eye(k, dtype=np.float32)[y]


# ---- the yardsticks --------------------------------------------------------------------------------------------------------------------
def head_f32(z, sc, sh, w, b, act):
    """the same head in plain numpy float32 on the same x: what the reference's float32 layer is entitled to"""
    f = np.float32
    x = H.head_input(z, sc, sh).astype(f)
    logits = x @ np.asarray(w, f) + np.asarray(b, f)[None, :]
    assert logits.dtype == f
    if act == "sigmoid":
        p = f(1) / (f(1) + np.exp(-logits))
    else:
        e = np.exp(logits - logits.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
    assert p.dtype == f
    return p


def infer_yardstick(z, sc, sh, w, b, act):
    """-> (p_64 [P,K], max |p_32 - p_64|, the bound for max |p_gpu - p_64|)"""
    p64 = H.forward(z, sc, sh, w, b, act)["probs"]
    d32 = float(np.abs(head_f32(z, sc, sh, w, b, act).astype(np.float64) - p64).max())
    return p64, d32, INFER_FACTOR * d32


def infer_distance(p, p64):
    return float(np.abs(np.asarray(p, np.float64).reshape(p64.shape) - p64).max())


TRAIN_QUANTITIES = ("out.w", "out.b", "gamma", "beta")


def _up(v, ulps):
    v = np.asarray(v, np.float32)
    return (v + np.float32(ulps) * np.abs(np.spacing(v))).astype(np.float32)


def train_quantities(z, gamma, beta, w, b, act, loss, target, loss_scale, round_dlogit, move_ulps=0, logit_w=None):
    """The head's training quantities from the float64 batch statistics of z.  move_ulps: scale and shift (as float32) moved up by that
    many ulps.  logit_w: other weights in the LOGITS only (planted defects)."""
    mean, var = H.batch_stats(z)
    sc, sh = (v.astype(np.float32) for v in H.bn_affine(gamma, beta, mean, var))
    if move_ulps:
        sc, sh = _up(sc, move_ulps), _up(sh, move_ulps)
    r = H.train(z, sc, sh, w, b, act, loss, target, loss_scale, round_dlogit)
    if logit_w is not None:      # a head whose forward read other weights: its probabilities drive every gradient
        bad = H.forward(z, sc, sh, logit_w, b, act)
        lv, g = H.loss_and_dlogit(bad["logits"], bad["probs"], target, act, loss)
        g = g * loss_scale
        g = g.astype(np.float16).astype(np.float64) if round_dlogit else g
        dy = (g @ np.asarray(w, np.float32).astype(np.float16).astype(np.float64).T).astype(np.float16).astype(np.float64)
        zz = np.asarray(z, np.float64).reshape(dy.shape)
        r = dict(loss=lv, dW=r["x"].T @ g / loss_scale, db=g.sum(0) / loss_scale, sum_dy=dy.sum(0), sum_dyz=(dy * zz).sum(0))
    dgamma, dbeta = H.bn_param_grads(r["sum_dy"], r["sum_dyz"], mean, var, loss_scale)
    return {"loss": r["loss"], "out.w": r["dW"], "out.b": r["db"], "gamma": dgamma, "beta": dbeta}


def train_yardsticks(z, gamma, beta, w, b, act, loss, target, loss_scale):
    """-> dict(on, off: the two references; d_round, d_stat: per quantity; d_stat_loss; bound: per quantity; loss_bound (absolute))"""
    args = (z, gamma, beta, w, b, act, loss, target, loss_scale)
    on, off, moved = train_quantities(*args, True), train_quantities(*args, False), train_quantities(*args, True, STAT_ULPS)
    y = dict(on=on, off=off, d_round={}, d_stat={}, bound={})
    for q in TRAIN_QUANTITIES:
        y["d_round"][q], y["d_stat"][q] = rel_l2(off[q], on[q]), rel_l2(moved[q], on[q])
        y["bound"][q] = TRAIN_MARGIN * (y["d_round"][q] + y["d_stat"][q])
    y["d_stat_loss"] = abs(moved["loss"] - on["loss"]) / abs(on["loss"])
    y["loss_bound"] = (LOSS_RTOL + y["d_stat_loss"]) * abs(on["loss"])
    return y


def train_distances(got, y):
    """got: dict quantity -> array (+ 'loss').  -> (dict quantity -> rel-L2 to the nearer reference, |loss - reference loss|)"""
    d = {q: min(rel_l2(got[q], y["on"][q]), rel_l2(got[q], y["off"][q])) for q in TRAIN_QUANTITIES}
    return d, abs(float(got["loss"]) - y["on"]["loss"])


# ---- (a) the oracle against torch float64 autograd and the whole-network oracle -----------------------------------------------------------
def _synthetic(cs, k, seed):
    cin = WIDTHS[cs][1]
    gamma, beta, w, b = draw_head_params(cin, k, seed)
    return synthetic_z(cin, seed + 1), gamma, beta, w, b


@pytest.mark.parametrize("case", TRAIN_CASES, ids=case_id)
def test_head_oracle_equals_torch_float64_autograd(case):
    cs, k, act, loss, _ = case
    z, sc, sh, w, b = _synthetic(cs, k, 100 + cs + k)
    w = w.astype(np.float16).astype(np.float32)          # fp16-valued weights: fp16(W) == W, so dy can be compared with autograd's
    tgt = synthetic_target(k, loss, 7)
    s = 1024.0
    r = H.train(z, sc, sh, w, b, act, loss, tgt, s, round_dlogit=False)
    d = torch.float64
    x = torch.tensor(H.head_input(z, sc, sh), dtype=d, requires_grad=True)
    wt, bt = torch.tensor(w, dtype=d, requires_grad=True), torch.tensor(b, dtype=d, requires_grad=True)
    # the head of the whole-network oracle (unet_oracle.head, what unet_oracle.forward runs in float32) and its loss_fn, in float64
    probs, logits4 = U.head(x.t()[None, :, :, None], wt[None, None], bt, act)
    logits4.retain_grad()
    probs, logits = probs[0, :, :, 0].t(), logits4[0, :, :, 0].t()
    lv = U.loss_fn(probs, torch.tensor(tgt, dtype=d), loss, logits if act == "softmax" else None)
    (lv * s).backward()
    tol = dict(rtol=0, atol=1e-12)
    assert np.allclose(r["probs"], probs.detach().numpy(), **tol) and np.allclose(r["logits"], logits.detach().numpy(), **tol)
    assert abs(r["loss"] - float(lv.detach())) <= 1e-12
    assert np.allclose(r["dlogit"], logits4.grad[0, :, :, 0].t().numpy(), **tol)
    assert np.allclose(r["dW"], wt.grad.numpy() / s, **tol) and np.allclose(r["db"], bt.grad.numpy() / s, **tol)
    assert np.allclose(r["dy_exact"], x.grad.numpy(), **tol)
    assert np.array_equal(r["dy"], r["dy_exact"].astype(np.float16).astype(np.float64))
    zz = np.asarray(z, np.float64)
    assert np.allclose(r["sum_dy"], r["dy"].sum(0), **tol) and np.allclose(r["sum_dyz"], (r["dy"] * zz).sum(0), **tol)
    # the switch: the rounded logit gradient is the fp16 rounding of the unrounded one, and everything behind it is formed from it
    q = H.train(z, sc, sh, w, b, act, loss, tgt, s, round_dlogit=True)
    assert np.array_equal(q["dlogit"], r["dlogit"].astype(np.float16).astype(np.float64)) and q["loss"] == r["loss"]
    assert np.allclose(q["dW"], q["x"].T @ q["dlogit"] / s, **tol) and np.allclose(q["dy_exact"], q["dlogit"] @ w.astype(np.float64).T, **tol)
    # BatchNorm parameter gradients: autograd through x = gamma (z - mean) / sqrt(var + eps) + beta with the statistics held fixed
    mean, var = H.batch_stats(z)
    gt, bt2 = torch.ones(zz.shape[1], dtype=d, requires_grad=True), torch.zeros(zz.shape[1], dtype=d, requires_grad=True)
    xb = gt * torch.tensor((zz - mean) / np.sqrt(var + H.BN_EPS)) + bt2
    (xb * torch.tensor(r["dy"])).sum().backward()
    dgamma, dbeta = H.bn_param_grads(r["sum_dy"], r["sum_dyz"], mean, var, s)
    assert np.allclose(dgamma, gt.grad.numpy() / s, rtol=0, atol=1e-10) and np.allclose(dbeta, bt2.grad.numpy() / s, **tol)


def test_one_rounding_of_the_batchnorm_affine():
    """x = fp16(z sc + sh) is the correctly rounded exact sum, not fp16(fp32(fp32(z sc) + sh)): on ties of the fp32 result the two differ"""
    rng = np.random.default_rng(5)
    z = np.abs(rng.standard_normal((1 << 16, 8))).astype(np.float16).astype(np.float32)
    sc, sh = (0.8 + 0.4 * rng.random(8)).astype(np.float32), (0.1 * rng.standard_normal(8)).astype(np.float32)
    x = H.head_input(z, sc, sh)
    from fractions import Fraction
    for i in range(0, 64):            # exact rational arithmetic on a sample
        for c in range(8):
            exact = Fraction(float(z[i, c])) * Fraction(float(sc[c])) + Fraction(float(sh[c]))
            lo, hi = np.nextafter(np.float16(x[i, c]), np.float16(-np.inf)), np.nextafter(np.float16(x[i, c]), np.float16(np.inf))
            assert abs(Fraction(float(x[i, c])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    staged = ((z * sc[None, :]).astype(np.float32) + sh[None, :]).astype(np.float32).astype(np.float16).astype(np.float64)
    assert 0 < (staged != x).mean() < 1e-3
    # the exact fold of the isolated GPU cases: var = float32(0.999), mean 0 -> scale == gamma, shift == beta bit for bit
    assert np.float32(np.float32(0.999) + np.float32(1e-3)) == np.float32(1.0)


@pytest.mark.parametrize("act,k,alpha", [("softmax", 17, 0.5), ("sigmoid", 3, 1.0)])
def test_head_oracle_equals_the_head_of_the_network_oracle(act, k, alpha):
    """unet_oracle.forward / train_step (torch float32, fp16-emulating) on a 16 x 16 net: fed the d9.c1 tap and the last BatchNorm as scale
    and shift, head_oracle gives the same probabilities, loss and gradients of out.w / out.b / d9.bnb.gamma / d9.bnb.beta to float32
    accuracy.  (unet_oracle takes dy = dlogit . W^T with the fp32 W and the unrounded logit gradient: the BatchNorm gradients differ
    by the fp16 rounding of W, 2^-11 relative per weight, at most.)"""
    h = w_ = 16
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (2, h, w_, 3)).astype(np.uint8)
    sd = U.init_weights(3, k, alpha, 9)
    g = torch.Generator().manual_seed(4)
    for n in sd:
        if n.endswith(".gamma"):
            sd[n] = 0.8 + 0.4 * torch.rand(sd[n].shape, generator=g)
        elif n.endswith(".beta") or n.endswith(".b"):
            sd[n] = 0.05 * torch.randn(sd[n].shape, generator=g)
        elif n.endswith(".var"):
            sd[n] = 0.5 + 0.5 * torch.rand(sd[n].shape, generator=g)
    taps = {}
    probs = U.forward(sd, x, 3, k, alpha, act, emulate_fp16=True, taps=taps).numpy()
    z = taps["d9.c1"].numpy()
    sc = sd["d9.bnb.gamma"] * torch.rsqrt(sd["d9.bnb.var"] + U.BN_EPS)
    sh = sd["d9.bnb.beta"] - sd["d9.bnb.mean"] * sc
    wk, bk = sd["out.w"][0, 0].numpy(), sd["out.b"].numpy()
    r = H.forward(z, sc.numpy(), sh.numpy(), wk, bk, act)
    assert np.abs(r["probs"].reshape(probs.shape) - probs).max() <= 2e-6
    # training mode
    loss = "cce" if act == "softmax" else "mse"
    tgt = synthetic_target(k, loss, 11, 2 * h * w_).reshape(2, h, w_, k)
    taps = {}
    U.forward(sd, x, 3, k, alpha, act, training=True, emulate_fp16=True, taps=taps)
    z = taps["d9.c1"].numpy()
    s = 256.0
    sd2 = {n: v.clone() for n, v in sd.items()}
    lv, grads = U.train_step(sd2, U.new_opt_state(sd2), x, tgt, 3, k, alpha, act, loss, emulate_fp16=True, loss_scale=s, return_grads=True)
    q = train_quantities(z, sd["d9.bnb.gamma"].numpy(), sd["d9.bnb.beta"].numpy(), wk, bk, act, loss, tgt, s, round_dlogit=False)
    assert abs(q["loss"] - lv) <= 1e-5 * abs(lv)
    assert rel_l2(q["out.w"], grads["out.w"][0, 0].numpy()) <= 1e-5 and rel_l2(q["out.b"], grads["out.b"].numpy()) <= 1e-5
    assert rel_l2(q["gamma"], grads["d9.bnb.gamma"].numpy()) <= 1e-3 and rel_l2(q["beta"], grads["d9.bnb.beta"].numpy()) <= 1e-3


@pytest.mark.parametrize("case", TRAIN_CASES, ids=case_id)
def test_training_batches_are_conditioned(case):
    cfg, (x, y, tgt), seed = training_batch(case)
    assert x.shape == (2, 32, 32, 3) and x.dtype == np.uint8 and 13 <= seed < 45
    assert oracle_conditioning(cfg, x, tgt)[0] <= COND_LIMIT
    if case[3] == "cce":
        assert y.shape == (2, 32, 32) and {0, case[1] - 1} <= set(np.unique(y).tolist()) and tgt.shape == (2, 32, 32, case[1])
        assert np.array_equal(tgt.argmax(-1), y) and np.array_equal(tgt.sum(-1), np.ones((2, 32, 32), np.float32))
    else:
        assert y.shape == (2, 32, 32, case[1]) and np.array_equal(tgt, y.astype(np.float32))


# ---- (b) the float32 yardstick --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", INFER_CASES, ids=case_id)
def test_float32_yardstick(case):
    """float32 sits a few ulps of a probability from float64 -- and not AT it: a yardstick of 0 would make the bound unmeetable, one
    above 1e-5 would make it toothless"""
    cs, act, k = case
    z, sc, sh, w, b = _synthetic(cs, k, 300 + cs + k)
    p64, d32, bound = infer_yardstick(z, sc, sh, w, b, act)
    assert 2.0 ** -25 <= d32 <= 2e-6 and bound == INFER_FACTOR * d32
    assert infer_distance(p64.astype(np.float32), p64) <= 2.0 ** -24        # rounding the float64 result to float32: half an ulp of 1
    if act == "softmax":
        assert np.abs(p64.sum(-1) - 1).max() <= 1e-15
        assert np.abs(head_f32(z, sc, sh, w, b, act).astype(np.float64).sum(-1) - 1).max() <= k * bound


# ---- (c) planted defects -------------------------------------------------------------------------------------------------------------------
def planted_probs(z, sc, sh, w, b, act, kind):
    """the reference with one defect a head kernel could have; None where the defect does not apply to the shape"""
    k = w.shape[1]
    w, b = np.array(w, np.float32), np.array(b, np.float32)
    if kind == "fp16_weights":                      # the `lo` half of the split weights dropped
        w = w.astype(np.float16).astype(np.float32)
    elif kind == "bias_last_zero":
        b[k - 1] = 0
    f = H.forward(z, sc, sh, w, b, act)
    logits = f["logits"]
    if kind == "swap_in_last_tile":                 # two classes of the last 16-class tile change places
        lo = 16 * ((k - 1) // 16)
        if k - 1 == lo:
            return None
        logits = logits.copy()
        logits[:, [lo, k - 1]] = logits[:, [k - 1, lo]]
    elif kind == "drop_last_class":                 # the single class of the last tile treated as padding
        if act != "softmax" or k % 16 != 1:
            return None
        logits = logits.copy()
        logits[:, k - 1] = -np.inf
    return H.activation(logits, act)


DEFECTS = ("fp16_weights", "swap_in_last_tile", "drop_last_class", "bias_last_zero")


@pytest.mark.parametrize("case", INFER_CASES, ids=case_id)
def test_planted_defects_land_outside_the_inference_bound(case):
    cs, act, k = case
    z, sc, sh, w, b = _synthetic(cs, k, 500 + cs + k)
    p64, d32, bound = infer_yardstick(z, sc, sh, w, b, act)
    applied = 0
    for kind in DEFECTS:
        p = planted_probs(z, sc, sh, w, b, act, kind)
        if p is None:
            continue
        applied += 1
        d = infer_distance(p, p64)
        assert d > 10 * bound, f"{kind}: {d:.3g} from float64, the bound is {bound:.3g}"
    # every case has the weight and the bias defect, and one that is about its last tile: a swap where that tile holds two classes or
    # more, the dropped class where it holds one (a sigmoid head with one map has no third)
    assert applied == (2 if k == 1 else 3)


@pytest.mark.parametrize("case", TRAIN_CASES, ids=case_id)
def test_planted_fp16_weights_land_outside_the_training_bound(case):
    """a training head whose logits read fp16 weights: at least one of the quantities the GPU test compares is outside its bound; and the
    reference itself (either rounding) is inside every one"""
    cs, k, act, loss, _ = case
    z, gamma, beta, w, b = _synthetic(cs, k, 700 + cs + k)
    tgt = synthetic_target(k, loss, 13)
    s = 32768.0
    y = train_yardsticks(z, gamma, beta, w, b, act, loss, tgt, s)
    for q in TRAIN_QUANTITIES:
        assert 0 < y["d_stat"][q] < 1e-3 and 0 < y["d_round"][q] < 1e-2, (q, y["d_stat"][q], y["d_round"][q])
    for ref in (y["on"], y["off"]):
        d, dl = train_distances(ref, y)
        assert all(d[q] == 0 for q in TRAIN_QUANTITIES) and dl <= y["loss_bound"]
    w16 = w.astype(np.float16).astype(np.float32)
    outside = []
    for rd in (True, False):
        d, dl = train_distances(train_quantities(z, gamma, beta, w, b, act, loss, tgt, s, rd, logit_w=w16), y)
        outside.append([q for q in TRAIN_QUANTITIES if d[q] > y["bound"][q]] + (["loss"] if dl > y["loss_bound"] else []))
    assert all(outside), (outside, y["bound"])
