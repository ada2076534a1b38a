#!/usr/bin/env python3
"""Golden vectors of the noisy-student pseudo-label writers, computed by the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_noisy_student.py

It writes tests/golden/noisy_student.npz, tests/golden/noisy_student_digests.json (a sha256 per array) and
tests/golden/reference_surface_noisy_student.json, which tests/test_golden_noisy_student.py and
tests/test_cpu_noisy_student_surface.py hold the repository to.  IMK_GOLDEN_OUT=<dir> writes elsewhere.

The reference's functions.py is loaded with the stub modules of make_golden_model_ensemble.py.  The cv2 stub is numpy: flip and
rotate are exact permutations; GaussianBlur and convertScaleAbs return their input and record their arguments; imread returns a
fixed image, imwrite records (file name, array).  The fake models return fixed arrays whatever they are fed, while the reference's own
create_pseudo_labels_noisy_student_* (functions.py:3243-3417) and augment_image_and_mask(s) run unmodified with their random /
np.random draws.  One image per case.  Every case records the seed (random.seed and np.random.seed), free_rotation, the draws
[flip_v, flip_h, rot, coin, blur size] (rot: 0 none, 1 = 90 CW, 2 = 180, 3 = 90 CCW; blur size 0 = none) read off the recorded
cv2 calls, the fixed prediction, every written label array as it reached imwrite, and the written file names in order.  For HeLa,
get_pos_contours is intercepted as in the model-ensemble generator: it records the thresholded, MOVED position mask and reports no
positions.  Nothing from the reference is copied: the outputs are data.

Cases (keys "<kind><i>_*" in noisy_student.npz):
  isic  create_pseudo_labels_noisy_student_ISIC_2018: preds [1,H,W,1] with values at 0.5 +- 1 ulp, NaN, +-0; mask u8 [H,W]
  hela  create_pseudo_labels_noisy_student_hela: preds [1,H,W,3]; alive / dead [H,W] (as written: integers 0 / 255), pos u8 [H,W]
  mc    create_pseudo_labels_noisy_student_multiclass: probs [1,H,W,K], K in {3, 9, 35}, with arg-max ties and NaN; mask [H,W] in the
        dtype np.argmax gave it (int64: what OpenCV makes of that cannot be recorded here)

reference_surface_noisy_student.json: the four noisy-student scripts, every name they import (tools/dump_reference_surface.py's
reading of their syntax trees), the signatures and defaults of the three writers, and per script the per-generation lists, the
ranking index / direction, the CSV header and the model-name pattern -- names and values only."""
import ast
import inspect
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_model_ensemble import F32, REF, array_digest, load_reference, salted, softmaxish, ulp_values  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
NAME = "noisy_student"
SCRIPTS = {"ISIC_2018/08_ISIC_2018_noisy_student.py": "ISIC_2018", "HeLa/08_HeLa_noisy_student.py": "HeLa",
           "SUIM/09_SUIM_noisy_student.py": "SUIM", "Cityscapes/08_Cityscapes_noisy_student.py": "Cityscapes"}
WRITERS = ("create_pseudo_labels_noisy_student_ISIC_2018", "create_pseudo_labels_noisy_student_hela",
           "create_pseudo_labels_noisy_student_multiclass")


class Fixed:
    def __init__(self, arr):
        self.arr = arr

    def predict(self, x):
        return self.arr.copy()


class Recorder:
    """the cv2 stub: exact geometry, recorded pixel operations, recorded file writes"""

    def install(self, ref):
        import types
        cv2 = sys.modules["cv2"]
        cv2.ROTATE_90_CLOCKWISE, cv2.ROTATE_180, cv2.ROTATE_90_COUNTERCLOCKWISE = 0, 1, 2

        def flip(a, code):
            self.draw["flip_v" if code == 0 else "flip_h"] = 1      # called for the image and for every mask: the same draw
            return np.ascontiguousarray(a[::-1] if code == 0 else a[:, ::-1])

        def rotate(a, code):
            self.draw["rot"] = code + 1
            return np.ascontiguousarray(np.rot90(a, k={0: -1, 1: 2, 2: 1}[code]))

        def blur(a, ksize, sigma):
            self.draw["blur"] = ksize[0]
            return a

        def csa(a, alpha=1.0, beta=0.0):
            self.draw["coin"] = 1
            return a

        cv2.flip, cv2.rotate, cv2.GaussianBlur, cv2.convertScaleAbs = flip, rotate, blur, csa
        cv2.imread = lambda path, flag=1: self.image.copy()
        cv2.cvtColor = lambda a, code: np.ascontiguousarray(a[..., ::-1])
        cv2.circle = lambda *a, **k: None
        cv2.imwrite = lambda path, arr: self.written.append((os.path.relpath(path, self.root).replace(os.sep, "/"), np.array(arr)))
        if not hasattr(np, "int"):
            np.int = int      # the HeLa writer spells astype(np.int) (functions.py:3346)
        ref.tqdm = lambda it, *a, **k: it
        ref.os = types.SimpleNamespace(path=os.path, makedirs=lambda *a, **k: None, listdir=lambda p: list(self.names))

    def start(self, seed, image, names):
        random.seed(seed)
        np.random.seed(seed)
        self.image, self.names, self.written, self.root = image, names, [], "/out"
        self.draw = {"flip_v": 0, "flip_h": 0, "rot": 0, "coin": 0, "blur": 0}

    def draws(self):
        d = self.draw
        return np.array([d["flip_v"], d["flip_h"], d["rot"], d["coin"], d["blur"]], np.int32)


def golden(ref):
    r = Recorder()
    r.install(ref)
    rng = np.random.default_rng(20261017)
    rec = {}

    def finish(key, seed, free):
        rec[key + "_seed"], rec[key + "_free"], rec[key + "_draws"] = np.int64(seed), np.int32(free), r.draws()
        rec[key + "_files"] = np.array([p for p, _ in r.written])

    # ---- ISIC: (p > 0.5) * 255, moved with the image ----------------------------------------------------------------------------
    h = w = 16
    for i in range(8):
        seed, free = 4000 + i, int(i != 6)
        preds = salted(rng, (1, h, w, 1), ulp_values(0.5), frac=0.3)
        r.start(seed, rng.integers(0, 256, (h, w, 3), dtype=np.uint8), [f"ISIC_{i:07d}.png"])
        ref.create_pseudo_labels_noisy_student_ISIC_2018(Fixed(preds), h, w, 3, "/in", "/out", True, (0.9, 1.1), (-5, 5), 3, 5, bool(free))
        key = f"isic{i}"
        finish(key, seed, free)
        rec[key + "_preds"], rec[key + "_mask"] = preds, r.written[1][1]
        assert [p for p, _ in r.written] == [f"images/ISIC_{i:07d}.png", f"masks/ISIC_{i:07d}.png"] and r.written[1][1].max() == 255

    # ---- HeLa: the float maps moved, then >= 0.5; the position mask reaches get_pos_contours in the moved frame -------------------
    for i in range(6):
        seed, free = 5000 + i, int(i != 4)
        preds = salted(rng, (1, h, w, 3), ulp_values(0.5), frac=0.3)
        seen = []
        real = ref.get_pos_contours
        ref.get_pos_contours = lambda img, *a, **k: (seen.append(np.array(img)), [])[1]
        r.start(seed, rng.integers(0, 256, (h, w), dtype=np.uint8), [f"cell_{i:03d}.png"])
        try:
            ref.create_pseudo_labels_noisy_student_hela(Fixed(preds), h, w, 1, "/in", "/out", (0.9, 1.1), (-3, 3), 2, 10, bool(free))
        finally:
            ref.get_pos_contours = real
        key = f"hela{i}"
        finish(key, seed, free)
        by = dict(r.written)
        rec[key + "_preds"], rec[key + "_pos"] = preds, seen[0]
        rec[key + "_alive"], rec[key + "_dead"] = by[f"alive/cell_{i:03d}_aug.png"], by[f"dead/cell_{i:03d}_aug.png"]
        assert len(r.written) == 4 and all(p.endswith("_aug.png") for p, _ in r.written)

    # ---- multi-class: np.argmax (first maximum, first NaN), moved with the image ------------------------------------------------
    for i, (k, hh, ww, free) in enumerate([(3, 16, 16, 1), (9, 16, 16, 1), (35, 8, 8, 1), (9, 8, 16, 0), (35, 8, 16, 0), (3, 8, 8, 1)]):
        seed = 6000 + i
        probs = softmaxish(rng, 1, hh, ww, k)[:, 0]
        for x in range(ww):      # row 0: two classes tie for the maximum
            probs[0, 0, x, :] = F32(0.5 / k)
            probs[0, 0, x, [x % k, (x + 1) % k]] = F32(0.6)
        r.start(seed, rng.integers(0, 256, (hh, ww, 3), dtype=np.uint8), [f"d_{i}.png"])
        ref.create_pseudo_labels_noisy_student_multiclass(Fixed(probs), hh, ww, 3, "/in", "/out", True, (0.9, 1.1), (-5, 5), 1, 5, bool(free))
        key = f"mc{i}"
        finish(key, seed, free)
        rec[key + "_probs"], rec[key + "_mask"] = probs, r.written[1][1]
    return rec


def _literal(node):
    return ast.literal_eval(node)


def script_facts(path):
    """the per-generation lists, the ranking key and the CSV header of one noisy-student script, read from its syntax tree"""
    tree = ast.parse(open(path, encoding="utf-8", errors="replace").read())
    facts = {}
    for n in ast.walk(tree):
        if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
            t = n.targets[0].id
            if t in ("alphas", "max_blurs", "max_noises", "brightness_range_alphas", "brightness_range_betas", "Header", "approach"):
                facts[t] = _literal(n.value)
            elif t == "modelname" and isinstance(n.value, ast.JoinedStr):
                facts["modelname"] = "".join(v.value if isinstance(v, ast.Constant) else "{" + ast.unparse(v.value) + "}"
                                             for v in n.value.values)
            elif t == "FREE_ROTATION":
                facts["free_rotation_parsed"] = ".lower()" in ast.unparse(n.value)
        if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "sorted":
            kw = {k.arg: k.value for k in n.keywords}
            facts["rank_index"] = _literal(kw["key"].body.slice)
            facts["rank_descending"] = _literal(kw["reverse"])
        if isinstance(n, ast.For) and isinstance(n.target, ast.Name) and n.target.id in ("runid", "gen", "n", "i"):
            facts.setdefault("loops", []).append([n.target.id] + [_literal(a) for a in n.iter.args])
    return facts


def surface(ref):
    import dump_reference_surface as D
    sig = {}
    for f in WRITERS:
        sig[f] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                  for p in inspect.signature(getattr(ref, f)).parameters.values()]
    return {"scripts": sorted(SCRIPTS), "wanted": D.wanted_names(REF, sorted(SCRIPTS)), "signatures": sig,
            "script_facts": {p: script_facts(os.path.join(REF, p)) for p in sorted(SCRIPTS)}}


def main():
    ref = load_reference()
    surf = surface(ref)      # before the stubs replace the module's os
    rec = golden(ref)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME + ".npz"), **rec)
    with np.load(os.path.join(OUT, NAME + ".npz")) as d:
        dig = {NAME: {key: array_digest(d[key]) for key in sorted(d.files)}}
    with open(os.path.join(OUT, NAME + "_digests.json"), "w") as f:
        json.dump(dig, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(OUT, "reference_surface_" + NAME + ".json"), "w") as f:
        json.dump(surf, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(rec)} arrays to {os.path.join(OUT, NAME + '.npz')}")


if __name__ == "__main__":
    main()
