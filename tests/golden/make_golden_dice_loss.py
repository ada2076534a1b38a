#!/usr/bin/env python3
"""Golden vectors of the reference's dice_loss (functions.py:162-184), computed by the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_dice_loss.py

It writes tests/golden/dice_loss.npz and tests/golden/dice_loss_digests.json (a sha256 per array), which
tests/test_cpu_dice_rule.py holds the committed fixture to.  IMK_GOLDEN_OUT=<dir> writes elsewhere.

The reference's module is loaded as tests/golden/make_golden_model_ensemble.py loads it (stub modules for its heavyweight imports);
the four TensorFlow calls dice_loss makes -- tf.cast, tf.reduce_sum (twice with an axis list), tf.reduce_mean -- are numpy here.  Each
case is run twice: with tf.float32 = numpy's float32, as the reference computes (key "<case>_loss32"), and with the cast widened to
float64 ("<case>_loss64"), which is the rule itself without float32's rounding.  Nothing of the reference is copied: the fixture
holds arrays only.

Cases ("<case>_true" u8 [B,H,W,K], "<case>_pred" f32 [B,H,W,K]): B in {1, 3, 5}, K in {1, 3}, images with very different foreground
shares, an all-zero target image, an all-one prediction, HeLa's targets containing 3.

The maker refuses a fixture on which one of the three planted defects of tests/dice_cases.py (one Dice over the whole batch; `smooth`
missing from the denominator; 1 - Dice of the summed I and U instead of the mean of the images' losses) comes within 1e-3 of the
reference's result on EVERY case.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_golden_model_ensemble as G  # noqa: E402  (load_reference, array_digest)
import dice_cases as DC  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
NAME = "dice_loss"
F32 = np.float32


def cases():
    rng = np.random.default_rng(20181)
    out = {}

    def pred(shape):
        return rng.random(shape).astype(F32)

    def shares(b, h, w, k, fr):
        return np.stack([(rng.random((h, w, k)) < f).astype(np.uint8) for f in fr[:b]], 0)

    fr = [0.02, 0.5, 0.98, 0.2, 0.7]
    for b in (1, 3, 5):
        for k in (1, 3):
            out[f"b{b}k{k}"] = (shares(b, 12, 10, k, fr), pred((b, 12, 10, k)))
    t = shares(3, 8, 8, 1, fr)
    t[1] = 0                                                   # an all-zero target image
    out["zero_target"] = (t, pred((3, 8, 8, 1)))
    out["ones_pred"] = (shares(3, 8, 8, 1, fr), np.ones((3, 8, 8, 1), F32))
    t = shares(3, 8, 12, 3, fr)
    t[..., 2] *= 3                                             # HeLa: the position plane is 0 / 3
    out["hela_three"] = (t, pred((3, 8, 12, 3)))
    return out


def run_reference(ref, y_true, y_pred, dtype):
    tf = ref.tf
    saved = {n: getattr(tf, n, None) for n in ("cast", "reduce_sum", "reduce_mean", "float32")}
    tf.float32 = dtype
    tf.cast = lambda a, dtype: np.asarray(a).astype(dtype)
    tf.reduce_sum = lambda a, axis=None: np.sum(a, axis=tuple(axis) if axis is not None else None)
    tf.reduce_mean = lambda a, axis=None: np.mean(a, axis=axis)
    try:
        return ref.dice_loss(y_true, y_pred)
    finally:
        for n, v in saved.items():
            setattr(tf, n, v)


def main():
    assert G.REF, "set IMK_REFERENCE to a checkout of the reference"
    ref = G.load_reference()
    rec, told = {}, {n: False for n in DC.DEFECTS}
    for name, (t, p) in cases().items():
        l32 = run_reference(ref, t, p, np.float32)
        l64 = run_reference(ref, t, p, np.float64)
        assert np.asarray(l32).dtype == np.float32 and np.asarray(l64).dtype == np.float64
        rec[name + "_true"], rec[name + "_pred"] = t, p
        rec[name + "_loss32"], rec[name + "_loss64"] = np.float32(l32), np.float64(l64)
        for n, f in DC.DEFECTS.items():
            d = f(t, p)
            told[n] = told[n] or not abs(d - float(l64)) <= 1e-3
    assert all(told.values()), f"the fixture cannot tell these defects from the rule: {[n for n, v in told.items() if not v]}"
    assert rec["hela_three_true"].max() == 3 and not rec["zero_target_true"][1].any() and rec["ones_pred_pred"].min() == 1.0
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME + ".npz"), **rec)
    with np.load(os.path.join(OUT, NAME + ".npz")) as d:
        dig = {NAME: {key: G.array_digest(d[key]) for key in sorted(d.files)}}
    with open(os.path.join(OUT, NAME + "_digests.json"), "w") as f:
        json.dump(dig, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(rec)} arrays to {os.path.join(OUT, NAME + '.npz')}")


if __name__ == "__main__":
    main()
