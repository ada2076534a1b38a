"""CPU oracle of the U-Net's output layer ALONE, in numpy float64.  TEST INFRASTRUCTURE ONLY.

The output layer is the one layer the reference keeps in float32 under its mixed_float16 policy (unet.py:63:
Conv2D(num_outputmasks, (1,1), activation=actifuout, dtype='float32')); every decision of the method -- thresholds, np.argmax, the
inconsistency mask -- is taken on its probabilities.  This file restates that layer and the two losses (`unet_oracle.loss_fn`: Keras
'mse', CategoricalCrossentropy going back to the logits) from their definitions, not from the kernels, at a precision far above the
float32 it stands for, so that a HIP head can be held to float32's own distance from it.

Inputs (shapes: P pixels, any leading dimensions are flattened):
  z         [P, cin]  the stored last activation (the conv output in front of the last BatchNorm), fp16-valued
  sc, sh    [cin]     that BatchNorm as scale and shift, float32
  W, b      [cin, K], [K]  the output layer, float32
  act       'sigmoid' | 'softmax'

What follows the project's design rather than the reference:
  x = fp16(z * sc + sh)       the BatchNorm output is a stored fp16 activation, formed exactly and rounded ONCE (section 6, deviation 1);
                              z (11 bits) times sc (24 bits) plus sh is exact in float64's 53 bits for the magnitudes of a network, and
                              numpy's float64 -> float16 conversion is correctly rounded
  round_dlogit                the gradient w.r.t. the logits, d(loss * S)/d(logits) with the loss scale S, is a stored fp16 tensor
                              (section 3); the switch turns that rounding on or off, because a fused kernel may sum either form
  dy = fp16(dlogit . fp16(W)^T)   the gradient w.r.t. x: fp16 operands like every dgrad of the step, stored as fp16
"""
import numpy as np

BN_EPS = 1e-3


def head_input(z, sc, sh):
    """x = fp16(z * sc + sh), one rounding; returned as float64 [P, cin]"""
    z = np.asarray(z, np.float64).reshape(-1, np.shape(z)[-1])
    x = z * np.asarray(sc, np.float64)[None, :] + np.asarray(sh, np.float64)[None, :]
    return x.astype(np.float16).astype(np.float64)


def activation(logits, act):
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-logits))
    if act != "softmax":
        raise ValueError(f"unsupported output activation {act!r} (sigmoid | softmax)")
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def forward(z, sc, sh, W, b, act):
    """-> dict(x [P,cin], logits [P,K], probs [P,K]), float64"""
    x = head_input(z, sc, sh)
    logits = x @ np.asarray(W, np.float64) + np.asarray(b, np.float64)[None, :]
    return dict(x=x, logits=logits, probs=activation(logits, act))


def loss_and_dlogit(logits, probs, target, act, loss):
    """loss and d(loss)/d(logits) (unscaled), float64.  target [P,K]: 0/1 maps (mse) or one-hot rows (cce)."""
    t = np.asarray(target, np.float64).reshape(probs.shape)
    n_pix, k = probs.shape
    if loss == "mse":                       # Keras 'mse': the mean over every element; through the sigmoid
        if act != "sigmoid":
            raise ValueError("mse goes with the sigmoid head")
        return float(((probs - t) ** 2).mean()), 2.0 * (probs - t) / (n_pix * k) * probs * (1.0 - probs)
    if loss != "cce" or act != "softmax":
        raise ValueError("cce goes with the softmax head")
    # CategoricalCrossentropy on a softmax activation's cached logits: mean over pixels of -sum_k t_k log softmax(logits)_k,
    # no probability clipping, d loss / d logits = (p - t) / pixels
    m = logits.max(-1, keepdims=True)
    logp = logits - m - np.log(np.exp(logits - m).sum(-1, keepdims=True))
    return float(-(t * logp).sum(-1).mean()), (probs - t) / n_pix


def train(z, sc, sh, W, b, act, loss, target, loss_scale=1.0, round_dlogit=True):
    """One training evaluation of the head at loss scale S.  Returns a dict of float64 arrays:
      loss                     the unscaled loss
      probs, logits, x         the forward
      dlogit [P,K]             d(loss * S)/d(logits), fp16-rounded if round_dlogit
      dW [cin,K], db [K]       x^T . dlogit / S and sum dlogit / S: the output layer's (unscaled) gradient
      dy [P,cin]               fp16(dlogit . fp16(W)^T): the (scaled) gradient w.r.t. the BatchNorm output, as stored
      dy_exact [P,cin]         the same product before its rounding to fp16
      sum_dy, sum_dyz [cin]    its per-channel sums over the pixels: sum dy and sum dy * z (what the BatchNorm backward needs)"""
    f = forward(z, sc, sh, W, b, act)
    z2 = np.asarray(z, np.float64).reshape(f["x"].shape)
    s = float(loss_scale)
    lv, g = loss_and_dlogit(f["logits"], f["probs"], target, act, loss)
    g = g * s
    if round_dlogit:
        g = g.astype(np.float16).astype(np.float64)
    w16 = np.asarray(W, np.float32).astype(np.float16).astype(np.float64)
    dy_exact = g @ w16.T
    dy = dy_exact.astype(np.float16).astype(np.float64)
    return dict(f, loss=lv, dlogit=g, dW=f["x"].T @ g / s, db=g.sum(0) / s, dy=dy, dy_exact=dy_exact,
                sum_dy=dy.sum(0), sum_dyz=(dy * z2).sum(0))


def batch_stats(z):
    """training-mode BatchNorm statistics of z [P, cin] in float64: mean and biased variance per channel"""
    z = np.asarray(z, np.float64).reshape(-1, np.shape(z)[-1])
    return z.mean(0), z.var(0)


def bn_affine(gamma, beta, mean, var):
    """scale = gamma / sqrt(var + eps), shift = beta - mean * scale, in float64 (the caller rounds them to the float32 a kernel holds)"""
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + BN_EPS)
    return scale, np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * scale


def bn_param_grads(sum_dy, sum_dyz, mean, var, loss_scale=1.0):
    """(unscaled) gradient of the last BatchNorm's gamma and beta from the head's sums: with x = gamma (z - mean) / sqrt(var + eps) + beta,
    d/dbeta = sum dy and d/dgamma = sum dy (z - mean) / sqrt(var + eps) = (sum dy z - mean sum dy) / sqrt(var + eps)"""
    inv = 1.0 / np.sqrt(np.asarray(var, np.float64) + BN_EPS)
    return (sum_dyz - np.asarray(mean, np.float64) * sum_dy) * inv / loss_scale, sum_dy / loss_scale
