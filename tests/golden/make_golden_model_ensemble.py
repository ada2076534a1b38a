#!/usr/bin/env python3
"""Golden vectors of the model-ensemble vote, computed by the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_model_ensemble.py

It writes tests/golden/model_ensemble.npz and tests/golden/model_ensemble_digests.json (a sha256 per array), which
tests/test_golden_model_ensemble.py holds the committed fixture to.  IMK_GOLDEN_OUT=<dir> writes elsewhere.

The reference's functions.py imports cv2 / tensorflow / tensorflow_addons at the top; empty stub modules stand in so that
its body executes.  The four functions driven here (get_model_ensemble_prediction_ISIC_2018 / _multiclass_hard /
_multiclass_soft / _hela_soft, functions.py:2409-2566) are numpy on the predictions of fake models that return fixed
arrays.  cv2.split is np.moveaxis.  For HeLa, get_pos_contours is intercepted: it records the thresholded position mask
it is given and reports no positions, so the circle stage (pinned by the geometry tests) does not run.  Nothing from the
reference is copied: the outputs are data.

Cases (keys "<kind><i>_*" in model_ensemble.npz):
  bin   hard binary vote (ISIC): preds [N,1,H,W,1], thr, out float64 [H,W]
  hela  soft binary vote (HeLa): preds [N,1,H,W,3], thr, alive / dead / pos u8 [H,W] (pos = the mask given to get_pos_contours)
  mc    multi-class votes: probs [N,1,H,W,K], soft u8 [H,W], hard u8 [H,W]
with N in {2, 3, 4, 5, 8}, K in {3, 9, 35, 64}, values at thr +- 1 ulp, NaN everywhere, soft multi-class ties created by the
fp32 divide (argmax(sum) != argmax(mean)) and pixels whose argmax depends on the summation order, and HeLa pixels whose fp64
average differs from the fp32 one, and one HeLa case at thr = 0.3 (not exact in fp32; the threshold is stored as float64).
"""
import hashlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
REF = os.environ.get("IMK_REFERENCE")
NAME = "model_ensemble"


def array_digest(a):
    """sha256 over dtype, shape and bytes of one array"""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(f"{a.dtype.str}|{a.shape}|".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def _module(name):
    m = types.ModuleType(name)
    sys.modules[name] = m
    return m


def load_reference():
    """the reference's functions module with its heavyweight imports replaced by empty modules"""
    for name in ("cv2", "tensorflow", "tensorflow_addons", "tensorflow.keras", "tensorflow.keras.preprocessing",
                 "tensorflow.keras.preprocessing.image", "tensorflow.keras.utils"):
        _module(name)
    tf = sys.modules["tensorflow"]
    keras = sys.modules["tensorflow.keras"]
    tf.keras = keras
    sys.modules["tensorflow.keras.preprocessing.image"].load_img = None
    sys.modules["tensorflow.keras.preprocessing.image"].img_to_array = None
    sys.modules["tensorflow.keras.utils"].to_categorical = None

    class Empty:      # base classes of the reference's metric / loss classes
        pass

    keras.metrics = types.SimpleNamespace(Metric=Empty)
    keras.losses = types.SimpleNamespace(Loss=Empty)
    cv2 = sys.modules["cv2"]
    cv2.split = lambda a: list(np.moveaxis(a, -1, 0))
    cv2.COLOR_BGR2RGB = 4
    cwd = os.getcwd()
    os.chdir(REF)            # the reference reads config.ini from the working directory
    sys.path.insert(0, REF)
    try:
        import functions as ref  # noqa: E402
    finally:
        os.chdir(cwd)
    return ref


class Fixed:
    """.predict([x]) -> a fixed [1,H,W,K] float32 array"""

    def __init__(self, arr):
        self.arr = arr

    def predict(self, x):
        return self.arr


F32 = np.float32


def ulp_values(thr):
    t = F32(thr)
    return np.array([t, np.nextafter(t, F32(1)), np.nextafter(t, F32(0)), np.nextafter(np.nextafter(t, F32(1)), F32(1)),
                     F32(0), F32(1), F32(np.nan), F32(-0.0), F32(np.inf), F32(-np.inf)], F32)


def salted(rng, shape, specials, frac=0.3):
    p = rng.random(shape, dtype=F32)
    flat = p.reshape(-1)
    n = max(1, int(flat.size * frac))
    idx = rng.choice(flat.size, size=n, replace=False)
    flat[idx] = specials[rng.integers(0, len(specials), size=n)]
    return p


def softmaxish(rng, n, h, w, k):
    """float32 probability maps [n,1,h,w,k] (rows summing to about 1) with a few NaN"""
    x = rng.standard_normal((n, 1, h, w, k)).astype(F32) * F32(2)
    e = np.exp(x - x.max(-1, keepdims=True))
    p = (e / e.sum(-1, keepdims=True)).astype(F32)
    flat = p.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, flat.size // 200), replace=False)
    flat[idx] = F32(np.nan)
    return p


def seq_sum(col):
    s = col[0]
    for v in col[1:]:
        s = F32(s + v)
    return s


def tie_pixel(rng, n, k):
    """[n, k] probabilities of one pixel whose two leading classes have different fp32 sums but the same fp32 mean, the lower
    class carrying the smaller sum: argmax of the sum != argmax of the mean"""
    while True:
        s_lo = F32(rng.uniform(0.4, 0.9))
        s_hi = np.nextafter(s_lo, F32(2))
        if F32(s_lo / F32(n)) != F32(s_hi / F32(n)):
            continue
        px = np.zeros((n, k), F32)
        px[:, 2:] = (rng.random((n, k - 2), dtype=F32) * F32(0.01))
        ok = True
        for cls, target in ((0, s_lo), (1, s_hi)):
            head = rng.random(n - 1, dtype=F32) * F32(target / n)
            last = F32(target - seq_sum(head)) if n > 1 else target
            col = np.concatenate([head, [last]]).astype(F32)
            if seq_sum(col) != target:
                ok = False
                break
            px[:, cls] = col
        if ok and seq_sum(px[:, 0]) < seq_sum(px[:, 1]):
            return px


def order_pixel(rng, n, k):
    """[n, k] probabilities of one pixel whose argmax depends on the summation order: class 0's sequential sum has a smaller mean
    than its sum in the reverse association, and class 1 carries exactly that other sum (a tie that class 0 would win)"""
    while True:
        col = (rng.random(n, dtype=F32) * F32(10.0) ** rng.integers(-8, 1, n)).astype(F32)
        seq = seq_sum(col)
        alt = col[-1]
        for v in col[-2::-1]:
            alt = F32(v + alt)
        if not F32(seq / F32(n)) < F32(alt / F32(n)):
            continue
        px = np.zeros((n, k), F32)
        px[:, 0] = col
        px[0, 1] = alt
        return px


def hela_fp64_pixels():
    """[2, 3] values of N = 2 where the fp64 average differs from an fp32 one: the fp32 sum of 0.5 + 2^-24 and 0.5 - 2^-25 rounds
    to 1.0 (average 0.5: 0) while the fp64 average is 0.5 + 2^-26 (> 0.5: 255)"""
    a = F32(0.5) + F32(2.0 ** -24)
    b = F32(0.5) - F32(2.0 ** -25)
    assert F32(a + b) == F32(1.0) and (float(a) + float(b)) / 2 > 0.5
    return np.array([[a, b, a], [b, a, F32(0.5)]], F32)


def main():
    assert REF, "set IMK_REFERENCE to a checkout of the reference"
    ref = load_reference()
    rng = np.random.default_rng(20261015)
    rec = {}

    # ---- binary, hard (ISIC) ----------------------------------------------------------------------------------------------
    for i, (n, thr) in enumerate([(2, 0.5), (3, 0.5), (4, 0.3), (5, 0.5), (8, 0.7)]):
        h, w = 16, 24
        preds = salted(rng, (n, 1, h, w, 1), ulp_values(thr))
        if n == 2:
            preds[:, 0, 0, :4, 0] = np.array([[np.nan, 0.9, 0.9, np.nan], [0.9, np.nan, 0.9, np.nan]], F32)
        out = ref.get_model_ensemble_prediction_ISIC_2018([Fixed(preds[j]) for j in range(n)], np.zeros((1, h, w, 3), np.uint8),
                                                          h, w, thr)
        rec[f"bin{i}_preds"], rec[f"bin{i}_thr"], rec[f"bin{i}_out"] = preds, np.float32(thr), np.asarray(out)

    # ---- binary, soft (HeLa) ----------------------------------------------------------------------------------------------
    for i, (n, thr) in enumerate([(2, 0.5), (3, 0.5), (4, 0.5), (5, 0.375), (8, 0.5)]):
        h = w = 16
        preds = salted(rng, (n, 1, h, w, 3), ulp_values(thr))
        if n == 2:
            preds[:, 0, 1, 0, :] = hela_fp64_pixels()
            preds[:, 0, 1, 1, :] = hela_fp64_pixels()[::-1]
        seen = []
        real = ref.get_pos_contours
        ref.get_pos_contours = lambda img, *a, **k: (seen.append(np.array(img)), [])[1]
        try:
            alive, dead, _ = ref.get_model_ensemble_prediction_hela_soft([Fixed(preds[j]) for j in range(n)],
                                                                        np.zeros((1, h, w, 1), np.uint8), thr)
        finally:
            ref.get_pos_contours = real
        assert len(seen) == 1
        rec[f"hela{i}_preds"], rec[f"hela{i}_thr"] = preds, np.float32(thr)
        rec[f"hela{i}_alive"], rec[f"hela{i}_dead"], rec[f"hela{i}_pos"] = alive, dead, seen[0]

    # ---- multi-class, soft and hard ------------------------------------------------------------------------------------------
    for i, (n, k, h, w) in enumerate([(2, 3, 16, 16), (3, 9, 16, 16), (4, 35, 8, 16), (5, 64, 8, 8), (8, 9, 8, 16), (3, 35, 8, 8),
                                      (2, 64, 8, 8), (8, 3, 8, 8), (3, 3, 8, 8)]):
        probs = softmaxish(rng, n, h, w, k)
        for x in range(w):        # row 0: ties made by the fp32 divide (N not a power of two: otherwise the divide is exact);
            if n & (n - 1):       # row 1: summation-order pixels (N >= 3); row 2: exact ties
                probs[:, 0, 0, x, :] = tie_pixel(rng, n, k)
            if n >= 3:
                probs[:, 0, 1, x, :] = order_pixel(rng, n, k)
        probs[:, 0, 2, :, :] = F32(1.0 / k)
        models = [Fixed(probs[j]) for j in range(n)]
        x0 = np.zeros((1, h, w, 3), np.uint8)
        rec[f"mc{i}_probs"] = probs
        rec[f"mc{i}_soft"] = ref.get_model_ensemble_prediction_multiclass_soft(models, x0)
        rec[f"mc{i}_hard"] = ref.get_model_ensemble_prediction_multiclass_hard(models, x0)
        s = probs[:, 0].sum(0, dtype=F32)
        assert not (n & (n - 1)) or np.any(np.argmax(s[0], -1) != rec[f"mc{i}_soft"][0]), "no fp32-divide tie survived"

    # ---- HeLa at a threshold that is not exact in fp32: the reference compares its float64 average with the Python double --------
    n, thr, h, w = 3, 0.3, 16, 16
    preds = salted(rng, (n, 1, h, w, 3), ulp_values(thr))
    preds[:, 0, 0, :, :] = F32(thr)          # average fl32(0.3) = 0.30000001 > 0.3: 255 in fp64, 0 against fl32(0.3)
    seen = []
    real = ref.get_pos_contours
    ref.get_pos_contours = lambda img, *a, **k: (seen.append(np.array(img)), [])[1]
    try:
        alive, dead, _ = ref.get_model_ensemble_prediction_hela_soft([Fixed(preds[j]) for j in range(n)], np.zeros((1, h, w, 1), np.uint8),
                                                                    thr)
    finally:
        ref.get_pos_contours = real
    assert alive[0].max() == 255
    rec["hela5_preds"], rec["hela5_thr"] = preds, np.float64(thr)
    rec["hela5_alive"], rec["hela5_dead"], rec["hela5_pos"] = alive, dead, seen[0]

    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME + ".npz"), **rec)
    with np.load(os.path.join(OUT, NAME + ".npz")) as d:
        dig = {NAME: {key: array_digest(d[key]) for key in sorted(d.files)}}
    with open(os.path.join(OUT, NAME + "_digests.json"), "w") as f:
        json.dump(dig, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(rec)} arrays to {os.path.join(OUT, NAME + '.npz')}")


if __name__ == "__main__":
    main()
