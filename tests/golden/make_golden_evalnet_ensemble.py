#!/usr/bin/env python3
"""Golden vectors of the EvalNet-ensemble selection writers, computed by the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_evalnet_ensemble.py

It writes tests/golden/evalnet_ensemble.npz, tests/golden/evalnet_ensemble_digests.json (a sha256 per array) and
tests/golden/reference_surface_evalnet_ensemble.json, which tests/test_golden_evalnet_ensemble.py and
tests/test_cpu_evalnet_ensemble_surface.py hold the repository to.  IMK_GOLDEN_OUT=<dir> writes elsewhere.

The reference's functions.py is loaded with the stub modules of make_golden_model_ensemble.py.  The cv2 stub is numpy: imread
returns the fixed image or the candidate mask of the directory it is asked for, cvtColor reverses the channels (BGR2RGB) or takes
the first one (BGR2GRAY), imwrite records (file name, array).  os / shutil are stand-ins that list one image name, say whether the
last generation's mask "exists" and record the copies.  The fake EvalNets return fixed float32 arrays whatever they are fed, while
the reference's own create_training_data_for_segnet_with_ensemble_binary (functions.py:5070-5152),
..._with_miou_ensemble_hela (:5323-5465) and ..._with_miou_ensemble_multiclass (:5468-5577) run unmodified.  The module's `np` is a
pass-through that also records what np.argmax returned, so that the chosen index is pinned where nothing is written (a NaN score).
For HeLa, get_pos_contours records the plane it is given and reports the fixed positions of POSITIONS (several, one or none), and
cv2.circle records its arguments: the reference's own radius rule (min_dist // 4 clamped to [3, 8], 99 for a single position) is
pinned as "<case>_circles", while finding the positions in a plane and rasterising a circle stay with the host geometry's own
tests (tests/test_cpu_geom.py).  Nothing from the reference is copied: the outputs are data.

One image per case.  Keys "<kind><i>_*" in evalnet_ensemble.npz:
  scores  float32 [N,M,U]: what the N fake EvalNets returned for the M candidates (U = 1; or K iou units then K detection units)
  meta    float64 [thr, last, best, keep]: the threshold handed over (the configs' 0.75, 0.62, 0.51, 0.453 -- all but 0.75 inexact in float32);
          last = 1: the last generation's mask existed and was appended as candidate M-1; best: the index np.argmax returned;
          keep = 1: the pair was written
  cands   uint8 [M,H,W] (HeLa: [M,H,W,3] in {0,255}): the candidate masks as imread returned them
  files   the written / copied file names in order;   mask (bin, mc) or alive, dead, pos (hela): the arrays as they reached imwrite
  circles int64 [n,7] (hela, where positions were reported): x, y, radius, colour (3), thickness of every cv2.circle call
  numpy   the NumPy version the rules ran under (one key for the file)
Kinds: bin (binary, U = 1), hela (K = 3), mc (K in {9, 35}).  Variants: ties between candidates, a NaN score, a best score at the float32
threshold and one ulp to either side, a mean detection of exactly 0.5 and one ulp below, no class counting, N in {2, 3, 4} and
M in {5, 6, 10, 11}.

reference_surface_evalnet_ensemble.json: the four scripts, every name they import, the signatures and defaults of the six functions,
and per script the loops, ranking keys, CSV headers and name patterns read from its syntax tree -- names and values only."""
import ast
import contextlib
import inspect
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_model_ensemble import F32, REF, array_digest, load_reference  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
NAME = "evalnet_ensemble"
SCRIPTS = {"ISIC_2018/10_ISIC_2018_evalnet_ensemble.py": "ISIC_2018", "HeLa/10_HeLa_evalnet_miou_ensemble.py": "HeLa",
           "SUIM/11_SUIM_evalnet_miou_ensemble.py": "SUIM", "Cityscapes/10_Cityscapes_evalnet_miou_ensemble.py": "Cityscapes"}
FUNCTIONS = ("create_training_data_for_segnet_with_ensemble_binary", "create_training_data_for_segnet_with_miou_ensemble_hela",
             "create_training_data_for_segnet_with_miou_ensemble_multiclass", "create_training_data_evalnet_ISIC_2018",
             "create_training_data_evalnet_miou_hela", "create_training_data_evalnet_miou_multiclass")
THRESHOLDS = (0.75, 0.62, 0.51, 0.453)
H = W = 8
# what get_pos_contours is made to report for HeLa case i (i % 3): several positions 10 to 24 pixels apart, a single one, none
POSITIONS = ([(8, 8), (8, 28), (44, 44), (44, 54), (20, 56)], [(30, 21)], [])


def mean32(col):
    """np.mean(axis=0) of a float32 column: the sum in order, one float32 divide"""
    return np.mean(np.asarray(col, F32).reshape(-1, 1), axis=0)[0]


class Unreachable(Exception):
    """the float32 means of n values step by more than one ulp of the target: not every float32 is one (n = 3)"""


def with_mean(rng, n, target):
    """n float32 values whose np.mean is exactly `target`"""
    target = F32(target)
    col = np.full(n, target, F32)
    for _ in range(3000):
        if mean32(col) == target:
            return col
        col = np.full(n, target, F32)
        for j in range(n):
            for _ in range(int(rng.integers(0, 4))):
                col[j] = np.nextafter(col[j], F32(rng.choice([0.0, 2.0])))
    raise Unreachable(f"no column of {n} with mean {target}")


class FakeEvalNet:
    """.predict([images, masks]) -> the fixed scores of this model: [M,1], or [iou [M,K], detection [M,K]]"""

    def __init__(self, arr, two_heads):
        self.arr, self.two_heads = arr, two_heads

    def predict(self, x):
        assert len(x[0]) == len(x[1]) == len(self.arr)
        k = self.arr.shape[1] // 2
        return [self.arr[:, :k].copy(), self.arr[:, k:].copy()] if self.two_heads else self.arr.copy()


class NpRecorder:
    """the module's `np`: numpy itself, with np.argmax's scalar results recorded"""

    def __init__(self):
        self.best = []

    def __getattr__(self, name):
        return getattr(np, name)

    def argmax(self, a, *args, **kw):
        r = np.argmax(a, *args, **kw)
        if np.ndim(r) == 0:
            self.best.append(int(r))
        return r


class World:
    """cv2 / os / shutil stand-ins of one case"""

    def install(self, ref):
        cv2 = sys.modules["cv2"]
        cv2.COLOR_BGR2RGB, cv2.COLOR_BGR2GRAY = 4, 6
        cv2.imread = lambda path, flag=1: self.read(path, flag)
        cv2.cvtColor = lambda a, code: np.ascontiguousarray(a[..., ::-1] if code == 4 else a[..., 0])
        cv2.circle = lambda img, centre, radius, colour, thickness: self.circles.append([*centre, radius, *colour, thickness])
        cv2.split = lambda a: [a[..., q] for q in range(a.shape[-1])]
        cv2.imwrite = lambda path, arr: self.files.append(path) or self.written.__setitem__(path, np.array(arr))
        ref.tqdm = lambda it, *a, **k: it
        ref.np = self.np = NpRecorder()
        path = types.SimpleNamespace(join=lambda *a: "/".join(a), isfile=lambda p: self.last, exists=lambda p: self.last)
        ref.os = types.SimpleNamespace(path=path, makedirs=lambda *a, **k: None, listdir=lambda p: list(self.listing.get(p, [])))
        ref.shutil = types.SimpleNamespace(copy=lambda s, d: self.files.append(d))
        ref.open = self.open

    def start(self, name, image, cands, last, planes=None):
        self.name, self.image, self.cands, self.last, self.planes = name, image, cands, bool(last), planes
        self.files, self.written, self.np.best, self.circles = [], {}, [], []
        self.listing = {"/in": [name]}

    def start_labelled(self, listing, tree):
        """the labelled set of the training-data writers: /tin/<sub>/<name> -> tree[sub][name]; labels.csv is a string"""
        self.listing, self.tree, self.last = listing, tree, False
        self.files, self.written, self.np.best, self.csv = [], {}, [], io.StringIO()

    def open(self, path, mode, **kw):
        assert path == "/tout/labels.csv" and mode == "a" and kw == {"encoding": "utf-8", "newline": ""}, (path, mode, kw)
        return contextlib.nullcontext(self.csv)      # the real csv.writer formats the rows

    def read(self, path, flag):
        parts = path.split("/")
        if parts[1] == "tin":
            a = self.tree[parts[2]][parts[3]]
            return (np.repeat(a[..., None], 3, -1) if flag and a.ndim == 2 else a).copy()
        if parts[1] == "in":
            return self.image.copy() if flag else self.image[..., 0].copy()
        m = len(self.cands) - 1 if parts[1] == "out" else int(parts[1][1:])      # /out/...: the last generation's mask; /d<j>/...
        a = self.cands[m]
        if self.planes:                                                        # HeLa: /d<j>/alive/<name>
            return a[..., self.planes.index(parts[2])].copy()
        return (np.repeat(a[..., None], 3, -1) if flag else a).copy()


def case_scores(rng, variant, n, m, k, thr):
    """[n', m, U] scores, U = 1 (k = 0) or 2k; n' = n, or 4 where a mean the variant needs is not reachable with n values"""
    try:
        return _case_scores(rng, variant, n, m, k, thr)
    except Unreachable:
        return _case_scores(rng, variant, 4, m, k, thr)


def _case_scores(rng, variant, n, m, k, thr):
    t = F32(thr)
    u = 2 * k if k else 1
    s = (rng.random((n, m, u), dtype=F32) * F32(float(t) - 0.1)).astype(F32)      # every mean below the threshold
    if k:
        s[:, :, k:] = F32(0.6) + rng.random((n, m, k), dtype=F32) * F32(0.3)       # every class counts
    j = int(rng.integers(0, m))

    def put(c, value, unit=0):
        s[:, c, unit] = with_mean(rng, n, value)

    def single(c):      # mIoU = the mean iou of class 0 alone
        if k:
            s[:, c, k + 1:] = F32(0.1)

    if variant == "rand":
        s[:, :, :max(k, 1)] = rng.random((n, m, max(k, 1)), dtype=F32)
    elif variant == "tie":
        j2 = (j + 1 + int(rng.integers(0, m - 1))) % m
        for c in (j, j2):
            single(c)
            put(c, F32(0.9))
    elif variant == "nan":
        single(j)
        put(j, F32(0.95))
        c = (j + 1) % m
        s[int(rng.integers(0, n)), c, 0] = F32(np.nan)
        if m > 2:
            s[0, (j + 2) % m, int(rng.integers(0, max(k, 1)))] = F32(np.nan)       # a later NaN as well: the first one wins
    elif variant in ("at", "above", "below"):
        single(j)
        put(j, {"at": t, "above": np.nextafter(t, F32(2)), "below": np.nextafter(t, F32(0))}[variant])
    elif variant == "half":      # detection means of exactly 0.5 (counts) and one ulp below (does not)
        s[:, j, :k] = F32(0.2)
        put(j, F32(0.97), 1)
        put(j, F32(0.5), k + 1)
        put(j, F32(0.01), 2)
        put(j, np.nextafter(F32(0.5), F32(0)), k + 2)
        s[:, j, k + 3:] = F32(0.1)
        s[:, j, k] = F32(0.1)
        s[:, j, 0] = F32(0.99)                                                     # a high iou that must not count
    elif variant == "none":
        s[:, :, k:] = rng.random((n, m, k), dtype=F32) * F32(0.49)
    elif variant == "some":      # some candidates without a counting class (score 0.0), the rest below them or above
        for c in range(0, m, 2):
            s[:, c, k:] = F32(0.2)
    return s


def golden(ref):
    wd = World()
    wd.install(ref)
    rng = np.random.default_rng(20261018)
    rec = {"numpy": np.array(np.__version__)}
    shapes = [(2, 5, 0), (3, 5, 1), (4, 10, 0), (2, 10, 1), (3, 10, 0), (4, 5, 1), (3, 5, 0), (2, 5, 1)]      # (N, directories, last)

    def record(key, scores, thr, last, cands):
        assert len(wd.np.best) == 1
        rec[key + "_scores"], rec[key + "_cands"] = scores, cands
        rec[key + "_meta"] = np.array([thr, last, wd.np.best[0], bool(wd.written)], np.float64)
        rec[key + "_files"] = np.array(wd.files if wd.files else [""])

    # ---- binary (ISIC): the mean IoU of the ensemble, arg-max, >= threshold -----------------------------------------------------
    for i, variant in enumerate(["rand", "tie", "nan", "at", "above", "below", "at", "above", "below", "tie", "nan", "rand"]):
        n, dirs, last = shapes[i % len(shapes)]
        m, thr = dirs + last, THRESHOLDS[i % 4]
        scores = case_scores(rng, variant, n, m, 0, thr)
        n = len(scores)
        cands = rng.integers(0, 256, (m, H, W), dtype=np.uint8)
        wd.start(f"ISIC_{i:07d}.png", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), cands, last)
        ref.create_training_data_for_segnet_with_ensemble_binary([FakeEvalNet(scores[q], False) for q in range(n)], H, W, 3, "/in",
                                                                 [f"/d{j}" for j in range(dirs)], "/out", thr, "/lg" if last else "",
                                                                 rgb=bool(i % 2))
        key = f"bin{i}"
        record(key, scores, thr, last, cands)
        if wd.written:
            rec[key + "_mask"] = wd.written[f"/out/masks/ISIC_{i:07d}.png"]

    # ---- HeLa: mean mIoU over the classes whose mean detection reaches 0.5 ------------------------------------------------------
    planes = ["alive", "dead", "mod_position"]
    variants = ["rand", "tie", "nan", "at", "above", "below", "half", "none", "some", "at", "above", "below"]
    for i, variant in enumerate(variants):
        n, dirs, last = shapes[(i + 3) % len(shapes)]
        m, thr = dirs + last, THRESHOLDS[(i + 1) % 4]
        scores = case_scores(rng, variant, n, m, 3, thr)
        n = len(scores)
        cands = (rng.integers(0, 2, (m, H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)
        seen = []
        real = ref.get_pos_contours
        ref.get_pos_contours = lambda img, *a, i=i, **k: (seen.append(np.array(img)), list(POSITIONS[i % 3]))[1]
        wd.start(f"cell_{i:03d}.png", rng.integers(0, 256, (H, W, 1), dtype=np.uint8), cands, last, planes)
        try:
            ref.create_training_data_for_segnet_with_miou_ensemble_hela([FakeEvalNet(scores[q], True) for q in range(n)], H, W, 1, "/in",
                                                                        [f"/d{j}" for j in range(dirs)], "/out", thr,
                                                                        "/lg" if last else "")
        finally:
            ref.get_pos_contours = real
        key = f"hela{i}"
        record(key, scores, thr, last, cands)
        if wd.written:
            rec[key + "_alive"], rec[key + "_dead"] = wd.written[f"/out/alive/cell_{i:03d}.png"], wd.written[f"/out/dead/cell_{i:03d}.png"]
            rec[key + "_pos"] = seen[0]
            if wd.circles and i < 3:      # the first case of either kind; x, y, radius, the colour's three values, thickness of every cv2.circle call, in order
                rec[key + "_circles"] = np.array(wd.circles, np.int64)

    # ---- multi-class (SUIM: 9 classes, Cityscapes: 35) -----------------------------------------------------------------------------
    for i, variant in enumerate(variants):
        n, dirs, last = shapes[(i + 5) % len(shapes)]
        k = 35 if i % 4 == 1 else 9
        m, thr = dirs + last, THRESHOLDS[(i + 2) % 4]
        scores = case_scores(rng, variant, n, m, k, thr)
        n = len(scores)
        cands = rng.integers(0, k, (m, H, W), dtype=np.uint8)
        wd.start(f"d_{i}.png", rng.integers(0, 256, (H, W, 3), dtype=np.uint8), cands, last)
        ref.create_training_data_for_segnet_with_miou_ensemble_multiclass([FakeEvalNet(scores[q], True) for q in range(n)], H, W, 3, k,
                                                                          "/in", [f"/d{j}" for j in range(dirs)], "/out", thr,
                                                                          "/lg" if last else "", rgb=bool(i % 2))
        key = f"mc{i}"
        record(key, scores, thr, last, cands)
        if wd.written:
            rec[key + "_mask"] = wd.written[f"/out/masks/d_{i}.png"]
    golden_training_data(ref, wd, rec)
    return rec


TH = TW = 12      # 144 pixels: one pixel is below the 1 % share (1.44) and above the 0.1 % share (0.144), two pixels are above both
LABELLED = ["l_000.png", "l_001_aug_03.png", "l_002.png"]
STEPS = (0, 11)


class FakeUNet:
    """.predict(x) -> the fixed probabilities of the next image [1,h,w,K], whatever it is fed; what it was fed is kept"""

    def __init__(self, probs):
        self.probs, self.fed = probs, []

    def predict(self, x):
        x = x[0] if isinstance(x, list) else x
        self.fed.append(np.array(x[0]))
        return self.probs[len(self.fed) - 1:len(self.fed)].copy()


def _probs(rng, k):
    """float32 [3,h,w,k] from a few values, 0.5 and the float32 next above it among them (the writers test p > 0.5)"""
    values = np.array([0.0, 0.25, 0.5, np.nextafter(F32(0.5), F32(1)), 0.75, 1.0], F32)
    return values[rng.integers(0, len(values), (len(LABELLED), TH, TW, k))]


def _block(rng, value=255):
    m = np.zeros((TH, TW), np.uint8)
    y, x = int(rng.integers(0, 5)), int(rng.integers(0, 5))
    m[y:y + int(rng.integers(3, 7)), x:x + int(rng.integers(3, 7))] = value
    return m


def _one_pixel(rng, value=255):
    m = np.zeros((TH, TW), np.uint8)
    m[int(rng.integers(0, TH)), int(rng.integers(0, TW))] = value
    return m


def golden_training_data(ref, wd, rec):
    """the reference's own create_training_data_evalnet_ISIC_2018 (functions.py:3419-3492), ..._miou_hela (:4011-4135) and
    ..._miou_multiclass (:4248-4323) on a labelled set of three images, one of them an `aug` file, for i = 0 and then i = 11 into one
    labels.csv.  The last image's planes differ from the others', so that the i == 0 loop's leftover masks show.
    Keys "td<kind>_*": io [2,3,h,w,c] (bin, mc): the images as imread returned them and as the model was given them in the i = 0 pass;
    gt [3,h,w] or [3,h,w,3]; probs float32 [3,h,w,K]: what the fake U-Net returned; files: the written and copied paths of both passes
    in order; masks uint8 [2,3,h,w] or [2,3,h,w,3]: per pass the arrays that reached imwrite, in the order of td_names; labels: the lines
    of labels.csv after both passes.  td_names: the listed file names; td_rgb: the rgb argument of the bin and of the mc pass."""
    rng = np.random.default_rng(20261019)
    for kind, c, k, rgb in (("bin", 3, 1, True), ("hela", 1, 3, None), ("mc", 3, 4, False)):
        images = (rng.integers(0, 4, (len(LABELLED), TH, TW, c)) * 64).astype(np.uint8)
        probs = _probs(rng, k)
        if kind == "bin":
            gt = np.stack([_block(rng) for _ in LABELLED])
            tree = {"images": dict(zip(LABELLED, images)), "masks": dict(zip(LABELLED, gt))}
            listing = {"/tin/images": LABELLED}
        elif kind == "hela":      # alive, dead, mod_position: [block, one pixel, one pixel], [block, block, block], [block, nothing, one pixel]
            gt = np.stack([np.stack([_block(rng), _one_pixel(rng), _one_pixel(rng)], -1),
                           np.stack([_block(rng), _block(rng), _block(rng)], -1),
                           np.stack([_block(rng), np.zeros((TH, TW), np.uint8), _one_pixel(rng)], -1)])
            tree = {"brightfield": dict(zip(LABELLED, images[..., 0]))}
            for q, plane in enumerate(("alive", "dead", "mod_position")):
                tree[plane] = dict(zip(LABELLED, gt[..., q]))
            listing = {"/tin/brightfield": LABELLED}
        else:      # class ids: {0, 1, 2}; {1, 2, 3} and one pixel of 0, never predicted as 0; {1, 3} alone in the last image
            g0 = np.maximum(_block(rng, 1), _block(rng, 2))
            g1 = np.where(_block(rng, 1) > 0, 2, 1).astype(np.uint8)
            g1[:2] = 3
            g1[TH - 1, TW - 1] = 0
            probs[1, ..., 0] = 0
            probs[1, ..., 1] = np.maximum(probs[1, ..., 1], F32(0.25))      # class 0 loses everywhere in the second image
            probs[0, 0, 0] = (0, 0, 0, 0)      # a tie of all classes: np.argmax takes the first
            g2 = np.where(_block(rng, 1) > 0, 3, 1).astype(np.uint8)
            gt = np.stack([g0, g1, g2])
            tree = {"images": dict(zip(LABELLED, images)), "masks": dict(zip(LABELLED, gt))}
            listing = {"/tin/images": LABELLED}
        wd.start_labelled(listing, tree)
        key, files, masks = "td" + kind, [], []
        subs = ("alive", "dead", "mod_position") if kind == "hela" else ("masks",)
        for step in STEPS:
            model = FakeUNet(probs)
            wd.files, wd.written = [], {}
            if kind == "bin":
                ref.create_training_data_evalnet_ISIC_2018(model, TH, TW, c, "/tin/images", "/tin/masks", "/tout", step, rgb=rgb)
            elif kind == "hela":
                ref.create_training_data_evalnet_miou_hela(model, TH, TW, c, "/tin", "/tout", step)
            else:
                ref.create_training_data_evalnet_miou_multiclass(model, TH, TW, c, k, "/tin/images", "/tin/masks", "/tout", step, rgb=rgb)
            files += wd.files
            written = [p for p in wd.files if p in wd.written]
            assert len(written) == len(wd.written) == len(subs) * len(LABELLED)
            m = np.stack([np.stack([wd.written[written[len(subs) * j + q]] for q in range(len(subs))], -1) for j in range(len(LABELLED))])
            assert m.min() >= 0 and m.max() <= 255
            masks.append((m if kind == "hela" else m[..., 0]).astype(np.uint8))
            if kind != "hela" and step == 0:
                rec[key + "_io"] = np.stack([images, np.stack(model.fed).reshape(images.shape)])
        rec[key + "_files"], rec[key + "_masks"], rec[key + "_gt"], rec[key + "_probs"] = np.array(files), np.stack(masks), gt, probs
        rec[key + "_labels"] = np.array(wd.csv.getvalue().split("\r\n")[:-1])
    rec["td_names"], rec["td_rgb"] = np.array(LABELLED), np.array([1, 0], np.int64)      # rgb of the binary and of the multi-class writer


def script_facts(path):
    """loops, ranking keys, CSV headers, name patterns, model_i starts and limits of one script, read from its syntax tree"""
    tree = ast.parse(open(path, encoding="utf-8", errors="replace").read())
    facts = {"loops": [], "ranks": [], "headers": [], "names": {}, "model_i": [], "joined": []}
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            t = node.targets[0].id
            if t == "Header":
                facts["headers"].append(ast.literal_eval(node.value))
            elif t == "model_i" and isinstance(node.value, ast.Constant):
                facts["model_i"].append(node.value.value)
            elif isinstance(node.value, ast.JoinedStr):
                pat = "".join(v.value if isinstance(v, ast.Constant) else "{" + ast.unparse(v.value) + "}" for v in node.value.values)
                facts["names"].setdefault(t, [])
                if pat not in facts["names"][t]:
                    facts["names"][t].append(pat)
        if isinstance(node, ast.Call) and getattr(node.func, "id", None) == "sorted":
            kw = {k.arg: k.value for k in node.keywords}
            facts["ranks"].append([ast.literal_eval(kw["key"].body.slice), ast.literal_eval(kw["reverse"])])
        if isinstance(node, ast.For) and isinstance(node.target, ast.Name) and isinstance(node.iter, ast.Call) and \
                getattr(node.iter.func, "id", None) == "range":
            facts["loops"].append([node.target.id] + [a.value if isinstance(a, ast.Constant) else [a.left.id, a.right.value]
                                                      for a in node.iter.args])      # a bound is a number or [name, number added]
        if isinstance(node, ast.Compare) and isinstance(node.left, ast.Name) and node.left.id == "model_i":
            facts["model_i"].append(node.comparators[0].value)      # model_i < 3, model_i < 13
        if isinstance(node, ast.Call) and ast.unparse(node.func) == "os.path.join":
            s = [a.value for a in node.args if isinstance(a, ast.Constant) and isinstance(a.value, str)]
            for v in s:
                if v not in facts["joined"]:
                    facts["joined"].append(v)
        if isinstance(node, ast.Call) and getattr(node.func, "id", "").startswith("train_") and "loss" not in facts:
            for a in node.args:
                if isinstance(a, ast.Constant) and a.value in ("mse", "categorical_crossentropy", "binary_crossentropy"):
                    facts["loss"] = a.value
        if isinstance(node, ast.Assign) and ast.unparse(node.targets[0]) == "THRESHOLD":
            facts["threshold_key"] = [c.value for c in ast.walk(node.value) if isinstance(c, ast.Constant)]      # [section, key]
    return facts


def surface(ref):
    import dump_reference_surface as D
    sig = {}
    for f in FUNCTIONS:
        sig[f] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                  for p in inspect.signature(getattr(ref, f)).parameters.values()]
    return {"scripts": sorted(SCRIPTS), "wanted": D.wanted_names(REF, sorted(SCRIPTS)), "signatures": sig,
            "script_facts": {p: script_facts(os.path.join(REF, p)) for p in sorted(SCRIPTS)}}


def main():
    ref = load_reference()
    surf = surface(ref)      # before the stand-ins replace the module's os
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
