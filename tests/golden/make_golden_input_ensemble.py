#!/usr/bin/env python3
"""Golden vectors of the input-ensemble vote, computed by the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_input_ensemble.py

It writes tests/golden/input_ensemble.npz and tests/golden/input_ensemble_digests.json (a sha256 per array), which
tests/test_golden_input_ensemble.py holds the committed fixture to.  IMK_GOLDEN_OUT=<dir> writes elsewhere.

The reference's functions.py is loaded with the stub modules of make_golden_model_ensemble.py.  The cv2 stub is numpy: flip and
rotate are exact permutations; GaussianBlur and convertScaleAbs return their input and record their arguments.  The fake models
return fixed arrays whatever they are fed, so the views' pixels do not matter, while the reference's own random / np.random draws
run unmodified.  Every case records the seed (random.seed and np.random.seed), the op of every view (the transformations handed
to restore_random_transformations), the blur size and the brightness coin of every view (0 = no blur), the fixed predictions and
the outputs.  For HeLa, get_pos_contours is intercepted as in the model-ensemble generator: it records the thresholded position
mask and reports no positions.  Nothing from the reference is copied: the outputs are data.

Cases (keys "<kind><i>_*" in input_ensemble.npz):
  isic  get_input_ensemble_prediction_ISIC_2018: n in {3, 5, 7} random views and the 13-view form; preds [M,H,W,1] with values at
        thr +- 1 ulp and NaN; out u8 [H,W]
  hela  get_input_ensemble_prediction_hela_hard / _soft (n + 1 chained views), thr 0.5 and 0.3; alive / dead / pos u8 [H,W]
  mc    get_input_ensemble_prediction_multiclass_soft and _multiclass (the majority) on the same draws, K in {3, 9, 35}, with
        count ties and NaN; soft / major u8 [H,W]
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_model_ensemble import F32, array_digest, load_reference, salted, softmaxish, ulp_values  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
NAME = "input_ensemble"
TRANSFORMS = [(fh, fv, rot) for fh in range(2) for fv in range(2) for rot in range(1, 4)]


class Fixed:
    """.predict(views) -> a fixed [M,H,W,K] float32 array (a copy: the ISIC function thresholds it in place)"""

    def __init__(self, arr):
        self.arr = arr

    def predict(self, x):
        return self.arr.copy()


class Recorder:
    """the cv2 stub and the per-view log of blur sizes and coins"""

    def __init__(self):
        self.views = []

    def install(self, ref):
        cv2 = sys.modules["cv2"]
        cv2.ROTATE_90_CLOCKWISE, cv2.ROTATE_180, cv2.ROTATE_90_COUNTERCLOCKWISE = 0, 1, 2
        cv2.flip = lambda a, code: np.ascontiguousarray(a[::-1] if code == 0 else a[:, ::-1])
        cv2.rotate = lambda a, code: np.ascontiguousarray(np.rot90(a, k={0: -1, 1: 2, 2: 1}[code]))

        def blur(a, ksize, sigma):
            self.views[-1]["blur"] = ksize[0]
            return a

        def csa(a, alpha=1.0, beta=0.0):
            self.views[-1]["coin"] = 1
            self.views[-1]["alpha"], self.views[-1]["beta"] = alpha, beta
            return a

        cv2.GaussianBlur, cv2.convertScaleAbs = blur, csa
        real_aug = ref.data_augmentation_image

        def aug(image, *a, **k):
            self.views.append({"blur": 0, "coin": 0})
            return real_aug(image, *a, **k)

        ref.data_augmentation_image = aug
        self.ops = None
        real_restore = ref.restore_random_transformations

        def restore(images, applied):
            self.ops = [1 + TRANSFORMS.index(tuple(t)) for t in applied]
            return real_restore(images, applied)

        ref.restore_random_transformations = restore

    def start(self, seed):
        random.seed(seed)
        np.random.seed(seed)
        self.views, self.ops = [], None

    def record(self, rec, key):
        rec[key + "_blur"] = np.array([v["blur"] for v in self.views], np.int32)
        rec[key + "_coin"] = np.array([v["coin"] for v in self.views], np.int32)


def main():
    ref = load_reference()
    r = Recorder()
    r.install(ref)
    rng = np.random.default_rng(20261016)
    rec = {}

    # ---- ISIC: n random views of the original (and the 13-view form), restored, >= thr ----------------------------------------
    h = w = 16
    for i, (n, rnd) in enumerate([(3, True), (5, True), (7, True), (13, False)]):
        seed, thr = 1000 + i, 0.5
        preds = salted(rng, (n, h, w, 1), ulp_values(thr), frac=0.1)
        preds = np.where(preds < 0.4, F32(0.9), preds)      # keeps the specials (NaN compares false)
        r.start(seed)
        out = ref.get_input_ensemble_prediction_ISIC_2018(Fixed(preds), np.zeros((h, w, 3), np.uint8), h, w, 3, thr, n,
                                                          use_n_rnd_transformations=rnd)
        key = f"isic{i}"
        rec[key + "_seed"], rec[key + "_thr"], rec[key + "_preds"], rec[key + "_out"] = np.int64(seed), np.float64(thr), preds, out
        rec[key + "_ops"] = np.array(r.ops if rnd else list(range(13)), np.int32)
        r.record(rec, key)
        assert len(rec[key + "_ops"]) == n and out.max() == 255

    # ---- HeLa: n + 1 chained views, hard (all p > thr) and soft (fp64 mean > thr) ------------------------------------------------
    for i, (n, soft, thr) in enumerate([(2, False, 0.5), (3, True, 0.5), (4, False, 0.3), (2, True, 0.3)]):
        seed = 2000 + i
        preds = salted(rng, (n + 1, h, w, 3), ulp_values(thr))
        preds[:, :4] = np.where(preds[:, :4] < 0.5, F32(0.95), preds[:, :4])
        if soft:
            preds[:, 4, :, :] = F32(thr)      # the fp64 mean of fl32(thr): > thr at 0.3, not at 0.5
        seen = []
        real = ref.get_pos_contours
        ref.get_pos_contours = lambda img, *a, **k: (seen.append(np.array(img)), [])[1]
        r.start(seed)
        try:
            fn = ref.get_input_ensemble_prediction_hela_soft if soft else ref.get_input_ensemble_prediction_hela_hard
            alive, dead, _ = fn(Fixed(preds), np.zeros((h, w), np.uint8), h, w, 1, n, threshold=thr)
        finally:
            ref.get_pos_contours = real
        key = f"hela{i}"
        rec[key + "_seed"], rec[key + "_thr"], rec[key + "_soft"], rec[key + "_preds"] = np.int64(seed), np.float64(thr), np.int32(soft), preds
        rec[key + "_alive"], rec[key + "_dead"], rec[key + "_pos"] = alive, dead, seen[0]
        r.record(rec, key)
        assert len(r.views) == n + 1 and alive.max() == 255

    # ---- multi-class: soft (argmax of the fp32 mean) and the majority of the per-view arg-maxes ----------------------------------
    for i, (n, k, hh, ww) in enumerate([(2, 3, 16, 16), (3, 9, 8, 16), (5, 35, 8, 8), (3, 3, 8, 8)]):
        seed = 3000 + i
        probs = softmaxish(rng, n + 1, hh, ww, k)[:, 0]
        # row 0: every view's arg-max from two labels, so the counts tie (n + 1 even) or nearly do
        for x in range(ww):
            labs = rng.permutation([x % k, (x + 1) % k] * ((n + 2) // 2))[: n + 1]
            for m, lab in enumerate(labs):
                probs[m, 0, x, :] = F32(0.5 / k)
                probs[m, 0, x, lab] = F32(0.6)
        key = f"mc{i}"
        r.start(seed)
        rec[key + "_soft"] = ref.get_input_ensemble_prediction_multiclass_soft(Fixed(probs), np.zeros((hh, ww, 3), np.uint8), hh, ww, 3, n)
        r.record(rec, key)
        r.start(seed)
        rec[key + "_major"] = ref.get_input_ensemble_prediction_multiclass(Fixed(probs), np.zeros((hh, ww, 3), np.uint8), hh, ww, 3, n)
        rec[key + "_seed"], rec[key + "_probs"] = np.int64(seed), probs

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
