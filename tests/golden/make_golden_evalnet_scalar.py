#!/usr/bin/env python3
"""Golden vectors of the scalar-IoU multiclass EvalNet family, computed by the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_evalnet_scalar.py

It writes tests/golden/evalnet_scalar.npz and tests/golden/reference_surface_evalnet_scalar.json, which
tests/test_cpu_label_cases.py, tests/test_cpu_evalnet_scalar_surface.py and tests/test_gpu_evalnet_scalar_writers.py hold the
repository to.  IMK_GOLDEN_OUT=<dir> writes elsewhere.

The reference's functions.py is loaded with the stub modules of make_golden_model_ensemble.py and the cv2 / os / shutil stand-ins of
make_golden_evalnet_ensemble.py (numpy; imwrite records).  Its own get_IoU_multi_unique (functions.py:1791-1816),
create_training_data_evalnet_multiclass (:3496-3567), create_training_data_evalnet_im_multiclass (:3673-3769) with its own
get_im_prediction_multiclass, create_training_data_for_segnet_multiclass (:5158-5231), ..._with_ensemble_multiclass (:5236-5317) and
create_augment_images_and_masks_with_evalnet_multiclass (:5762-5831) run unmodified on fake models that return fixed arrays.
cv2.erode / cv2.dilate are a numpy minimum / maximum over the k x k window (clipped at the border) that records its window size;
augment_image_and_mask records its call and returns its inputs, drawing nothing; the module's `random` records every draw.
Nothing from the reference is copied: the outputs are data.

Keys of evalnet_scalar.npz:
  iou<i>_pred, _gt u8 [h,w], _im u8 [h,w] (where the case has an IM), _value float64 [2]: the label of case i -- the reference's
      get_IoU_multi_unique(gt, pred with its IM pixels set to 0), as both writers call it -- and round(label, 4).  Cases: a class of the
      prediction that the ground truth lacks and the reverse; class 0 present only through blocking; a ground-truth value of 255; an
      image of one class; 3 / (800 + 1e-7), whose quotient without the 1e-7 rounds to 0.0038 and with it to 0.0037; random maps.
  sw_*   the single-model writer for i = 0 and then 11 into one labels.csv: names, gt u8 [n,h,w], probs f32 [n,h,w,K],
         masks u8 [2,n,h,w] (as they reached imwrite), files (written and copied paths in order), labels (the csv's lines)
  imw_*  the IM writer, two loops of the same set with 5 fake models: probs f32 [5,n,h,w,K]; draws float64 [2*n, 8]: per loop and image
         the number of members, the member word (bit j = model j), erode kernel, dilate kernel, the coin, then 3 spare; kinds: the names
         of the draws of ONE image in order; pred u8 [2,n,h,w] the agreement mask before blocking, im_raw / im u8 [2,n,h,w] the IM before
         and after the recorded morphology; images u8 [n,h,w,3] as imread returned them; out_images / out_masks as they reached
         imwrite; files; labels; seed
  sel<i>_* the selection writers: scores f32 [N,M] as the fake EvalNets returned them, argmax_in f32 [M] or [M,1] what reached np.argmax,
         meta float64 [thr, last, best, keep, N], cands u8 [M,h,w], files, mask (where kept)
  aug_*  thresholds float64 [T,2]; scores f32 [T,S]; num f64 [T,S]: the number of `___{j}.png` pairs written for a predicted IoU
  numpy  the NumPy version the rules ran under"""
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_golden_evalnet_ensemble import FakeEvalNet, NpRecorder, World, case_scores  # noqa: E402
from make_golden_model_ensemble import F32, load_reference  # noqa: E402
import label_cases as LC  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
NAME = "evalnet_scalar"
FUNCTIONS = ("create_training_data_evalnet_multiclass", "create_training_data_evalnet_im_multiclass", "train_evalnet_multiclass",
             "create_training_data_for_segnet_multiclass", "create_training_data_for_segnet_with_ensemble_multiclass",
             "create_augment_images_and_masks_with_evalnet_multiclass", "compute_classwise_confluence", "get_confluence_binary")
H = W = 16
K = 4
LABELLED = ["l_000.png", "l_001_aug_03.png", "l_002.png"]
DRAW_KINDS = ("randint", "sample", "choice", "choice", "random")


class ArgmaxRecorder(NpRecorder):
    """np.argmax's scalar results AND what it was given"""

    def __init__(self):
        super().__init__()
        self.given = []

    def argmax(self, a, *args, **kw):
        r = np.argmax(a, *args, **kw)
        if np.ndim(r) == 0:
            self.best.append(int(r))
            self.given.append(np.array(a))
        return r


class RandomRecorder:
    """the module's `random`: Python's, seeded here, every draw recorded as (name, value)"""

    def __init__(self, seed):
        import random
        self.rng, self.draws = random.Random(seed), []

    def _rec(self, name, value):
        self.draws.append((name, value))
        return value

    def randint(self, a, b):
        return self._rec("randint", self.rng.randint(a, b))

    def sample(self, population, k):
        return self._rec("sample", self.rng.sample(population, k))

    def choice(self, seq):
        return self._rec("choice", self.rng.choice(seq))

    def random(self):
        return self._rec("random", self.rng.random())


class ScalarWorld(World):
    """+ /ain/<sub>/<name> of the augmentation writer, np.argmax's argument, recording morphology"""

    def install(self, ref):
        super().install(ref)
        ref.np = self.np = ArgmaxRecorder()
        cv2 = sys.modules["cv2"]
        self.morph = []
        cv2.erode = lambda a, kernel, iterations=1: self._morph(a, kernel, np.min, "erode")
        cv2.dilate = lambda a, kernel, iterations=1: self._morph(a, kernel, np.max, "dilate")

    def _morph(self, a, kernel, op, name):
        k = kernel.shape[0]
        assert kernel.shape == (k, k) and k % 2 == 1 and kernel.all()
        self.morph.append((name, k))
        r = k // 2
        out = np.empty_like(a)
        for y in range(a.shape[0]):
            for x in range(a.shape[1]):
                out[y, x] = op(a[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1])
        return out

    def read(self, path, flag):
        parts = path.split("/")
        if parts[1] == "ain":
            a = self.tree[parts[2]][parts[3]]
            return (np.repeat(a[..., None], 3, -1) if flag and a.ndim == 2 else a).copy()
        return super().read(path, flag)


class FakeSeg:
    """.predict([x]) -> this model's fixed probabilities of the image whose index sits in pixel (0, 0); the calls are kept"""

    def __init__(self, ident, probs, calls):
        self.ident, self.probs, self.calls = ident, probs, calls

    def predict(self, x):
        x = x[0] if isinstance(x, list) else x
        idx = int(x[0, 0, 0, 0])
        self.calls.append((self.ident, idx))
        return self.probs[idx:idx + 1].copy()


def _blocks(rng, h, w, k, cell=4):
    return rng.integers(0, k, ((h + cell - 1) // cell, (w + cell - 1) // cell)).astype(np.uint8).repeat(cell, 0).repeat(cell, 1)[:h, :w]


def _probs(rng, n, h, w, k):
    """float32 probabilities in blocks with exact ties (np.argmax takes the first) and a NaN (np.argmax takes it)"""
    values = np.array([0.0, 0.25, 0.5, 0.75, 1.0], F32)
    p = values[rng.integers(0, len(values), (n, (h + 1) // 2, (w + 1) // 2, k))].repeat(2, 1).repeat(2, 2)[:, :h, :w].copy()
    p[0, 1, 1] = 0.5
    p[n - 1, 2, 3, k - 1] = np.nan
    return p


def _images(rng, n, h, w):
    img = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    for j in range(n):
        img[j, 0, 0] = j      # what FakeSeg reads, whichever channel order it is handed
    return img


def golden_labels(ref, rec):
    rng = np.random.default_rng(20261021)
    cases = []
    g = np.zeros((H, W), np.uint8); g[:8] = 1; g[8:, :8] = 2
    p = g.copy(); p[:4] = 3; p[8:, :8] = 1
    cases.append((p, g, None))                                    # class 3 only in the prediction, class 2 only in the ground truth
    g = _blocks(rng, H, W, 3) + 1
    p = np.where(rng.random((H, W)) < 0.8, g, 1).astype(np.uint8)
    im = np.zeros((H, W), np.uint8); im[3:6, 2:9] = 255; im[12, 12] = 1
    cases.append((p, g, im))                                      # no class 0 in either map: it comes from the blocking alone
    g = _blocks(rng, H, W, 3); g[0:4, 0:4] = 255
    p = _blocks(rng, H, W, 3)
    cases.append((p, g, None))                                    # a ground-truth value >= num_classes
    cases.append((np.full((H, W), 3, np.uint8), np.full((H, W), 3, np.uint8), None))      # one class
    g = np.zeros((25, 32), np.uint8); g[0, :3] = 2
    cases.append((np.full((25, 32), 2, np.uint8), g, None))       # 3 / (800 + 1e-7): 0.0037, without the 1e-7 0.0038
    im = np.full((H, W), 255, np.uint8)
    cases.append((_blocks(rng, H, W, K), _blocks(rng, H, W, K), im))      # fully blocked
    for _ in range(4):
        h, w = int(rng.integers(16, 33)), int(rng.integers(16, 33))
        im = (rng.random((h, w)) < 0.2).astype(np.uint8) * 255 if rng.random() < 0.5 else None
        g = _blocks(rng, h, w, K)
        cases.append((np.where(rng.random((h, w)) < 0.7, g, _blocks(rng, h, w, K)).astype(np.uint8), g, im))
    for i, (p, g, im) in enumerate(cases):
        blocked = p.copy()
        if im is not None:
            blocked[im > 0] = 0                                    # functions.py:3744
        v = ref.get_IoU_multi_unique(g, blocked)                  # functions.py:3550, 3747: the ground truth first
        rec[f"iou{i}_pred"], rec[f"iou{i}_gt"] = p, g
        if im is not None:
            rec[f"iou{i}_im"] = im
        rec[f"iou{i}_value"] = np.array([v, round(v, 4)], np.float64)
    return len(cases)


def check_discriminates(rec, n_cases):
    """refuse a fixture that cannot tell the rule from: the other map's classes, a union without 1e-7, a mean over num_classes"""
    def variants(c):
        out = {}
        for name, present, eps, fixed_n in (("rule", c[1], 1e-7, None), ("other map", c[0], 1e-7, None), ("no 1e-7", c[1], 0.0, None),
                                             ("over num_classes", c[1], 1e-7, K)):
            lst = [c[2, v] / ((c[0, v] + c[1, v] - c[2, v]) + eps) for v in range(256) if present[v] > 0]
            out[name] = round(sum(lst) / (fixed_n or len(lst)), 4)
        return out
    told = {"other map": 0, "no 1e-7": 0, "over num_classes": 0}
    for i in range(n_cases):
        c = LC.counts(rec[f"iou{i}_pred"], rec[f"iou{i}_gt"], rec.get(f"iou{i}_im"))
        v = variants(c)
        if v["rule"] != rec[f"iou{i}_value"][1]:
            raise SystemExit(f"label case {i}: the restated rule gives {v['rule']!r}, the reference {rec[f'iou{i}_value'][1]!r}")
        for name in told:
            told[name] += v[name] != v["rule"]
    missing = [name for name, n in told.items() if not n]
    if missing:
        raise SystemExit(f"the label cases cannot tell the rule from: {missing}")


def golden_single_writer(ref, wd, rec):
    rng = np.random.default_rng(20261022)
    n = len(LABELLED)
    images, probs = _images(rng, n, H, W), _probs(rng, n, H, W, K)
    gt = np.stack([_blocks(rng, H, W, K) for _ in range(n)])
    gt[1][gt[1] == 0] = 1                                         # no class 0 in the second ground truth
    gt[2, :2, :2] = 255
    wd.start_labelled({"/tin/images": LABELLED}, {"images": dict(zip(LABELLED, images)), "masks": dict(zip(LABELLED, gt))})
    files, masks = [], []
    for step in (0, 11):
        calls = []
        wd.files, wd.written = [], {}
        ref.create_training_data_evalnet_multiclass(FakeSeg(0, probs, calls), H, W, 3, "/tin/images", "/tin/masks", "/tout", step,
                                                    rgb=step == 0)
        assert [c[1] for c in calls] == list(range(n))
        files += wd.files
        written = [p for p in wd.files if p in wd.written]
        assert len(written) == n
        masks.append(np.stack([wd.written[p] for p in written]).astype(np.uint8))
    rec["sw_names"], rec["sw_gt"], rec["sw_probs"], rec["sw_masks"] = np.array(LABELLED), gt, probs, np.stack(masks)
    rec["sw_files"], rec["sw_labels"] = np.array(files), np.array(wd.csv.getvalue().split("\r\n")[:-1])


def golden_im_writer(ref, wd, rec):
    rng = np.random.default_rng(20261023)
    n, n_models, loops, seed = len(LABELLED), 5, 2, 4242
    images = _images(rng, n, H, W)
    base = _probs(rng, n, H, W, K)
    probs = np.stack([np.where(rng.random((n, H // 4, W // 4, 1)).repeat(4, 1).repeat(4, 2) < 0.8, base, _probs(rng, n, H, W, K))
                      for _ in range(n_models)]).astype(F32)
    gt = np.stack([_blocks(rng, H, W, K) for _ in range(n)])
    wd.start_labelled({"/tin/images": LABELLED}, {"images": dict(zip(LABELLED, images)), "masks": dict(zip(LABELLED, gt))})
    calls, seen = [], []
    models = [FakeSeg(j, probs[j], calls) for j in range(n_models)]
    ref.random = rnd = RandomRecorder(seed)
    real_im, real_aug = ref.get_im_prediction_multiclass, ref.augment_image_and_mask

    def im_spy(selected, prepared):
        out = real_im(selected, prepared)
        seen.append((np.array(out[0]), np.array(out[1])))
        return out
    ref.get_im_prediction_multiclass = im_spy
    ref.augment_image_and_mask = lambda image, mask, *a, **k: (image, mask)
    ref.tf = type("tf", (), {"keras": type("keras", (), {"backend": type("backend", (), {"clear_session": staticmethod(lambda: None)})})})
    wd.morph = []
    try:
        ref.create_training_data_evalnet_im_multiclass(models, H, W, 3, "/tin/images", "/tin/masks", "/tout", loops)
    finally:
        ref.get_im_prediction_multiclass, ref.augment_image_and_mask = real_im, real_aug
    per = len(DRAW_KINDS)
    assert len(rnd.draws) == per * loops * n and [d[0] for d in rnd.draws[:per]] == list(DRAW_KINDS)
    draws = np.zeros((loops * n, 8), np.float64)
    morph = list(wd.morph)
    im_final = []
    for q in range(loops * n):
        cnt, members, ke, kd, coin = (d[1] for d in rnd.draws[per * q:per * q + per])
        word = sum(1 << m.ident for m in members)
        assert cnt == len(members)
        draws[q, :5] = (cnt, word, ke, kd, float(coin))
        im = seen[q][1]
        for name, k in (("erode", ke), ("dilate", kd)):
            if k:
                assert morph.pop(0) == (name, k)
                im = wd._morph(im, np.ones((k, k), np.uint8), np.min if name == "erode" else np.max, name)
        im_final.append(im)
    written = [p for p in wd.files if p in wd.written]
    assert len(written) == 2 * loops * n
    shape = (loops, n, H, W)
    rec["imw_probs"], rec["imw_gt"], rec["imw_images"], rec["imw_draws"] = probs, gt, images, draws
    rec["imw_kinds"], rec["imw_seed"], rec["imw_names"] = np.array(DRAW_KINDS), np.array(seed), np.array(LABELLED)
    rec["imw_pred"] = np.stack([s[0] for s in seen]).astype(np.uint8).reshape(shape)
    rec["imw_im_raw"] = np.stack([s[1] for s in seen]).astype(np.uint8).reshape(shape)
    rec["imw_im"] = np.stack(im_final).astype(np.uint8).reshape(shape)
    rec["imw_out_images"] = np.stack([wd.written[p] for p in written[0::2]]).astype(np.uint8).reshape(shape + (3,))
    rec["imw_out_masks"] = np.stack([wd.written[p] for p in written[1::2]]).astype(np.uint8).reshape(shape)
    rec["imw_files"], rec["imw_labels"] = np.array(wd.files), np.array(wd.csv.getvalue().split("\r\n")[:-1])


def golden_selection(ref, wd, rec):
    rng = np.random.default_rng(20261024)
    # (N, directories, last generation's mask): N = 1 is create_training_data_for_segnet_multiclass
    shapes = [(1, 5, 0), (2, 5, 1), (3, 10, 0), (1, 10, 1), (2, 10, 0), (3, 5, 1), (1, 5, 1), (3, 10, 1)]
    variants = ["rand", "tie", "nan", "at", "above", "below"]
    i = 0
    for thr in (0.75, 0.62):                                      # exact and inexact in float32
        for variant in variants:
            for rep in range(2):
                n, dirs, last = shapes[3 * i % len(shapes)]      # 3 and 8 are coprime: every shape, under changing variants
                m = dirs + last
                scores = case_scores(rng, variant, n, m, 0, thr)
                n = len(scores)                                    # (a mean that three float32 values cannot reach: four of them)
                cands = np.stack([_blocks(rng, H, W, K) for _ in range(m)])
                name = f"u_{i:03d}.png"
                wd.start(name, rng.integers(0, 256, (H, W, 3), dtype=np.uint8), cands, last)
                wd.np.given = []
                nets = [FakeEvalNet(scores[q], False) for q in range(n)]
                args = (H, W, 3, K, "/in", [f"/d{j}" for j in range(dirs)], "/out", thr, "/lg" if last else "")
                if n == 1:
                    ref.create_training_data_for_segnet_multiclass(nets[0], *args, rgb=bool(i % 2))
                else:
                    ref.create_training_data_for_segnet_with_ensemble_multiclass(nets, *args, rgb=bool(i % 2))
                assert len(wd.np.best) == 1
                key = f"sel{i}"
                rec[key + "_scores"], rec[key + "_cands"], rec[key + "_argmax_in"] = scores[:, :, 0], cands, wd.np.given[0].astype(F32)
                rec[key + "_meta"] = np.array([thr, last, wd.np.best[0], bool(wd.written), n], np.float64)
                rec[key + "_files"] = np.array(wd.files if wd.files else [""])
                if wd.written:
                    rec[key + "_mask"] = wd.written[f"/out/masks/{name}"]
                i += 1
    rec["sel_count"] = np.array(i)


def golden_num_augs(ref, wd, rec):
    rng = np.random.default_rng(20261025)
    thresholds = [(0.5, 0.9), (0.62, 0.87), (0.3, 0.8)]
    scores, nums = [], []
    image, mask = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), _blocks(rng, H, W, K)
    real_aug = ref.augment_image_and_mask
    ref.augment_image_and_mask = lambda img, msk, *a, **k: (img, msk)
    try:
        for lo, hi in thresholds:
            step = F32((hi - lo) / 5)
            row = [F32(0), F32(1), F32(np.nan)]
            for j in range(6):      # every step edge as float32 forms it, and the float32 neighbours either side
                e = F32(F32(lo) + F32(j) * step)
                row += [np.nextafter(e, F32(0)), e, np.nextafter(e, F32(2)), np.nextafter(np.nextafter(e, F32(2)), F32(2))]
            row += [F32(hi), np.nextafter(F32(hi), F32(0)), np.nextafter(F32(hi), F32(2))]
            got = []
            for v in row:
                wd.start_labelled({"/ain/images": ["p.png"]}, {"images": {"p.png": image}, "masks": {"p.png": mask}})
                ref.create_augment_images_and_masks_with_evalnet_multiclass(FakeEvalNet(np.array([[v]], F32), False), H, W, 3, K, lo, hi,
                                                                            "/ain", "/aout")
                assert len(wd.files) % 2 == 0 and wd.files[0::2] == [f"/aout/images/p___{j}.png" for j in range(len(wd.files) // 2)]
                got.append(len(wd.files) // 2)
            scores.append(np.array(row, F32))
            nums.append(np.array(got, np.float64))
    finally:
        ref.augment_image_and_mask = real_aug
    rec["aug_thresholds"], rec["aug_scores"], rec["aug_num"] = np.array(thresholds, np.float64), np.stack(scores), np.stack(nums)


def surface(ref):
    sig = {}
    for f in FUNCTIONS:
        sig[f] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                  for p in inspect.signature(getattr(ref, f)).parameters.values()]
    return {"signatures": sig}


def main():
    ref = load_reference()
    surf = surface(ref)      # before the stand-ins replace the module's os
    wd = ScalarWorld()
    wd.install(ref)
    rec = {"numpy": np.array(np.__version__)}
    n_cases = golden_labels(ref, rec)
    rec["iou_count"] = np.array(n_cases)
    check_discriminates(rec, n_cases)
    golden_single_writer(ref, wd, rec)
    golden_im_writer(ref, wd, rec)
    golden_selection(ref, wd, rec)
    golden_num_augs(ref, wd, rec)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME + ".npz"), **rec)
    with open(os.path.join(OUT, "reference_surface_" + NAME + ".json"), "w") as f:
        json.dump(surf, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(rec)} arrays to {os.path.join(OUT, NAME + '.npz')} ({os.path.getsize(os.path.join(OUT, NAME + '.npz'))} bytes)")


if __name__ == "__main__":
    main()
