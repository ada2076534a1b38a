#!/usr/bin/env python3
"""Golden vectors of the single-EvalNet selection writers, computed by the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_evalnet_single.py

It writes tests/golden/evalnet_single.npz, tests/golden/evalnet_single_digests.json (a sha256 per array) and
tests/golden/reference_surface_evalnet_single.json, which tests/test_golden_evalnet_single.py and
tests/test_cpu_evalnet_single_surface.py hold the repository to.  IMK_GOLDEN_OUT=<dir> writes elsewhere.

Built as make_golden_evalnet_ensemble.py is (its World of cv2 / os / shutil stand-ins, its fixed-score fake EvalNets and its `np`
pass-through that records what np.argmax returned are imported from there): the reference's own
create_training_data_for_segnet_ISIC_2018 (functions.py:4991-5063) and create_training_data_by_evalnet_miou_for_segnet_multiclass
(:5583-5677) run unmodified on one image per case.  Nothing from the reference is copied: the outputs are data.

Keys "<kind><i>_*" in evalnet_single.npz, as in evalnet_ensemble.npz with N = 1:
  scores  float32 [1,M,U]: what the fake EvalNet returned for the M candidates (U = 1; or K iou units then K detection units)
  meta    float64 [thr, last, best, keep];  cands uint8 [M,H,W];  files: the written / copied names in order;  mask: what reached imwrite
  given   float64 [M]: what the reference handed to np.argmax -- the candidates' scores as it computed them (float32 values, or Python's 0.0)
  numpy   the NumPy version the rules ran under (one key for the file)
Kinds: bin (create_training_data_for_segnet_ISIC_2018, U = 1) and gat (the multi-class writer, K in {8, 35}); M in {5, 6, 10, 11}.
Variants of gat (GATED_VARIANTS, in order; "<kind>_variants" lists them):
  rand            random detection values, most classes counting
  gate_at         a class whose mean detection over the candidates is exactly float32(0.03): it counts, and alone decides the choice
  gate_below      a class whose mean is one ulp below float32(0.03): it does not count, though its values would change the choice.
                  (Float32 means of M values step by more than an ulp: 0.03f is a mean for M = 6 and 11 only, the value below it for
                  M = 5 and 10 only, so these cases move to the next M that has such a column.)
  none            no class counts: every score is 0.0, candidate 0 is the arg-max; with the threshold 0.5 nothing is kept, with 0.0 the pair is
  nangate         a NaN detection value: its class's mean over the candidates is NaN and the class does not count, for any candidate,
                  although it carries the highest values.  A NaN value in a COUNTING class cannot occur under this rule, nor can a NaN
                  score: the value is part of the mean that decides whether its class counts (and a column holding +inf and -inf has
                  a NaN mean as well), so every counting class is NaN-free for every candidate.
  tie             two candidates with the same score: the first wins
  at/above/below  a best score at the float32 threshold and one ulp to either side, for 0.5 (exact in float32) and for 0.453 (inexact)
  contra          every class counts under either rule, and the iou units rank the candidates the other way round: IMK_SELECT_MIOU
                  (a rule that reads the iou half) chooses another candidate
bin: rand, tie, nan, at / above / below for 0.75 (exact) and 0.62 (inexact).

reference_surface_evalnet_single.json: the six scripts (the two single-EvalNet scripts and the four full-dataset scripts), every name they
import, the signatures and defaults of the two functions, and per script the loops, ranking keys, CSV headers, the names in the EvalNet
CSV's row, name patterns, the `paths` constants used and whether a max() floors the step count -- names and values only."""
import ast
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_model_ensemble import F32, REF, array_digest, load_reference  # noqa: E402
from make_golden_evalnet_ensemble import FakeEvalNet, NpRecorder, Unreachable, World, _case_scores, mean32, script_facts  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
NAME = "evalnet_single"
SCRIPTS = {"ISIC_2018/10_ISIC_2018_evalnet.py": "ISIC_2018", "SUIM/11_SUIM_evalnet_miou.py": "SUIM",
           "ISIC_2018/02_ISIC_2018_full_dataset.py": "ISIC_2018", "HeLa/02_HeLa_full_dataset.py": "HeLa",
           "Cityscapes/02_Cityscapes_full_dataset.py": "Cityscapes", "SUIM/03_SUIM_full_dataset.py": "SUIM"}
FUNCTIONS = ("create_training_data_for_segnet_ISIC_2018", "create_training_data_by_evalnet_miou_for_segnet_multiclass")
H = W = 8
GATE = F32(0.03)
SHAPES = [(5, 0), (5, 1), (10, 0), (10, 1)]      # (directories, last): M = 5, 6, 10, 11
BIN_VARIANTS = ["rand", "tie", "nan", "at", "above", "below", "at", "above", "below", "tie", "nan", "rand"]
BIN_THRESHOLDS = (0.75, 0.62)
GATED_VARIANTS = ["rand", "gate_at", "none", "none0", "nangate", "nangate", "tie", "at", "above", "below", "at", "above", "below", "contra",
                  "gate_below", "rand", "tie", "contra", "gate_at", "gate_below"]
GATED_THRESHOLDS = (0.5, 0.453)


class ScoreRecorder(NpRecorder):
    """... and what np.argmax was given: the candidates' scores as the reference computed them"""

    def argmax(self, a, *args, **kw):
        self.given = np.array(a, np.float64).reshape(-1)
        return super().argmax(a, *args, **kw)


def column_with_mean(rng, m, target, hi):
    """m float32 values spread over [0, hi) whose np.mean(axis=0) is exactly `target`: random draws, the last value walked ulp by ulp"""
    target = F32(target)
    for _ in range(200):
        col = (rng.random(m, dtype=F32) * F32(hi)).astype(F32)
        col[-1] = F32(max(float(target) * m - float(col[:-1].sum(dtype=np.float64)), 0.0))
        for _ in range(400):
            got = mean32(col)
            if got == target:
                return col
            col[-1] = np.nextafter(col[-1], F32(2.0) if got < target else F32(-1.0))
    raise Unreachable(f"no column of {m} with mean {target}")


def gated_scores(rng, variant, m, k, thr):
    """[1, m, 2k]: k iou units, then k detection units"""
    t = F32(thr)
    s = np.empty((1, m, 2 * k), F32)
    s[0, :, :k] = rng.random((m, k), dtype=F32)
    det = s[0, :, k:]
    det[:] = rng.random((m, k), dtype=F32) * F32(0.02)      # nothing counts: every mean is below 0.02
    j = int(rng.integers(0, m))
    others = [c for c in range(m) if c != j]
    if variant == "rand":
        det[:] = rng.random((m, k), dtype=F32)
        det[:, rng.integers(0, k, 2)] *= F32(0.02)            # one or two classes gated out
    elif variant == "gate_at":      # class 1's mean is exactly 0.03f: it counts and decides; without it every score would be 0.0
        while True:
            det[:, 1] = column_with_mean(rng, m, GATE, 0.06)
            if int(np.argmax(det[:, 1])) != 0 and np.sort(det[:, 1])[-1] > np.sort(det[:, 1])[-2]:
                break
    elif variant == "gate_below":      # class 2's mean is one ulp below 0.03f: it does not count, though it would change the choice
        while True:
            det[:, 1] = F32(0.03) + rng.random(m, dtype=F32) * F32(0.03)
            det[:, 2] = column_with_mean(rng, m, np.nextafter(GATE, F32(0)), 0.06)
            with_b = det[:, 1].astype(np.float64) + det[:, 2]
            if int(np.argmax(det[:, 1])) != int(np.argmax(with_b)) and np.sort(det[:, 1])[-1] > np.sort(det[:, 1])[-2]:
                break
    elif variant in ("none", "none0"):
        pass
    elif variant == "nangate":      # class 1 carries the highest values and a NaN: it must not count; class 2 decides
        det[:, 1] = F32(0.8) + rng.random(m, dtype=F32) * F32(0.15)
        det[others[0], 1] = F32(np.nan)
        det[:, 2] = F32(0.3) + rng.random(m, dtype=F32) * F32(0.1)
        det[j, 2] = F32(0.97)
        det[j, 1] = F32(0.0)      # with class 1 counted, every other candidate would beat this one (and the NaN would win)
    elif variant == "tie":
        j2 = others[int(rng.integers(0, m - 1))]
        det[:, 1:4] = rng.random((m, 3), dtype=F32) * F32(0.5) + F32(0.1)
        det[j, 1:4] = (F32(0.9), F32(0.8), F32(0.95))
        det[j2, 1:4] = det[j, 1:4]
    elif variant in ("at", "above", "below"):      # class 1 alone counts; the best candidate's value sits at the threshold
        det[:, 1] = F32(0.05) + rng.random(m, dtype=F32) * F32(float(t) - 0.15)
        det[j, 1] = {"at": t, "above": np.nextafter(t, F32(2)), "below": np.nextafter(t, F32(0))}[variant]
    elif variant == "contra":
        det[:] = F32(0.55) + rng.random((m, k), dtype=F32) * F32(0.1)
        det[j] += F32(0.3)
        s[0, :, :k] = F32(0.6) + rng.random((m, k), dtype=F32) * F32(0.1)
        s[0, j, :k] = F32(0.05)                                 # the iou units say the opposite
    else:
        raise KeyError(variant)
    return s


def golden(ref):
    wd = World()
    wd.install(ref)
    ref.np = wd.np = ScoreRecorder()
    rng = np.random.default_rng(20261019)
    rec = {"numpy": np.array(np.__version__), "bin_variants": np.array(BIN_VARIANTS), "gat_variants": np.array(GATED_VARIANTS)}

    def record(key, scores, thr, last, cands, name):
        assert len(wd.np.best) == 1
        rec[key + "_scores"], rec[key + "_cands"] = scores, cands
        rec[key + "_meta"] = np.array([thr, last, wd.np.best[0], bool(wd.written)], np.float64)
        rec[key + "_files"] = np.array(wd.files if wd.files else [""])
        rec[key + "_given"] = wd.np.given
        if wd.written:
            rec[key + "_mask"] = wd.written[f"/out/masks/{name}"]

    # ---- binary (ISIC): the one EvalNet's predicted IoU, arg-max, >= threshold ----------------------------------------------------------
    for i, variant in enumerate(BIN_VARIANTS):
        dirs, last = SHAPES[i % len(SHAPES)]
        m, thr = dirs + last, BIN_THRESHOLDS[(i // 3) % 2]
        scores = _case_scores(rng, variant, 1, m, 0, thr)
        cands = rng.integers(0, 256, (m, H, W), dtype=np.uint8)
        name = f"ISIC_{i:07d}.png"
        wd.start(name, rng.integers(0, 256, (H, W, 3), dtype=np.uint8), cands, last)
        ref.create_training_data_for_segnet_ISIC_2018(FakeEvalNet(scores[0], False), H, W, 3, "/in", [f"/d{j}" for j in range(dirs)], "/out",
                                                      thr, "/lg" if last else "", rgb=bool(i % 2))
        record(f"bin{i}", scores, thr, last, cands, name)

    # ---- multi-class (SUIM's rule; K = 8 and 35) ---------------------------------------------------------------------------------------
    for i, variant in enumerate(GATED_VARIANTS):
        k = 35 if i % 3 == 1 else 8
        thr = {"none0": 0.0, "gate_at": 0.035, "gate_below": 0.035, "rand": 0.4}.get(variant, GATED_THRESHOLDS[int(i >= 10)])
        for shift in range(len(SHAPES)):      # another M where a column with the exact mean does not exist for this one
            dirs, last = SHAPES[(i + shift) % len(SHAPES)]
            m = dirs + last
            try:
                scores = gated_scores(rng, variant, m, k, thr)
                break
            except Unreachable:
                continue
        else:
            raise Unreachable(variant)
        cands = rng.integers(0, k, (m, H, W), dtype=np.uint8)
        name = f"d_{i}.png"
        wd.start(name, rng.integers(0, 256, (H, W, 3), dtype=np.uint8), cands, last)
        ref.create_training_data_by_evalnet_miou_for_segnet_multiclass(FakeEvalNet(scores[0], True), H, W, 3, k, "/in",
                                                                       [f"/d{j}" for j in range(dirs)], "/out", thr,
                                                                       "/lg" if last else "", rgb=bool(i % 2))
        record(f"gat{i}", scores, thr, last, cands, name)
    return rec


def single_script_facts(path):
    """script_facts of the ensemble generator, plus: the names in the EvalNet CSV's row, the approach string, the `paths` constants the
    script uses and whether a max() floors the step count"""
    facts = script_facts(path)
    tree = ast.parse(open(path, encoding="utf-8", errors="replace").read())
    facts["results"], facts["approach"], facts["floor"] = [], [], False
    used = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            if node.targets[0].id == "results" and isinstance(node.value, ast.List):
                facts["results"].append([e.id for e in node.value.elts])
            if node.targets[0].id == "approach" and isinstance(node.value, ast.Constant):
                facts["approach"].append(node.value.value)
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "paths":
            used.add(node.attr)
        if isinstance(node, ast.Call) and getattr(node.func, "id", None) == "max":
            facts["floor"] = True
    facts["paths"] = sorted(used)
    return facts


def surface(ref):
    import dump_reference_surface as D
    sig = {}
    for f in FUNCTIONS:
        sig[f] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                  for p in inspect.signature(getattr(ref, f)).parameters.values()]
    return {"scripts": sorted(SCRIPTS), "wanted": D.wanted_names(REF, sorted(SCRIPTS)), "signatures": sig,
            "script_facts": {p: single_script_facts(os.path.join(REF, p)) for p in sorted(SCRIPTS)}}


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
