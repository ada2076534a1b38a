#!/usr/bin/env python3
"""Golden vectors of the depth-map family's standard-deviation IM, computed by the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_depth_map.py

It writes tests/golden/depth_map.npz, tests/golden/depth_map_digests.json (a sha256 per array) and
tests/golden/reference_surface_depth_map.json (names, positional arguments and defaults of the family's seven functions), which
tests/test_cpu_depth_rule.py holds the repository to.  IMK_GOLDEN_OUT=<dir> writes elsewhere.

The reference's own get_im_prediction_depth_map (functions.py:6155-6177) runs unmodified on fake models whose .predict returns a fixed
[1,H,W,1] float32 array; the module's `np` is a pass-through that records what np.mean returned, so the threshold the reference formed
(threshold_multiplier * that mean, the reference's own expression) is on record by its bits.  Nothing from the reference is copied: the
outputs are data.

Per case "<name>_*" (names in "names"):
  shape      [N, H, W]
  codes      uint8 [N*H*W] and lut float32 [256]: the predictions are lut[codes] (the large cases draw from 16 levels so that the file
             stays small; the small ones from 256)
  mults      float32 [M]: the multipliers the case was run with;  kinds [M]: "given", or "at" / "above" / "below" for a multiplier
             searched so that the threshold equals some pixel's standard deviation bit for bit / sits one ulp above / below it
  thr_bits   uint32 [M]: the thresholds' bits;  masks uint8 [M, ceil(H*W/8)]: np.packbits of the returned {0,1} array
  numpy      the NumPy version the rule ran under (one key for the file)

The maker refuses to write a fixture that cannot tell tests/depth_cases.py's three planted defects (no 8192 chunking, a sequential sum
over the models, FMA-contracted squares) from the rule: each has to change the threshold bits or the mask of at least one recorded
case.  It also asserts that the restatement itself reproduces every record and that the at / above / below multipliers were found."""
import inspect
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import depth_cases as DC  # noqa: E402
from make_golden_model_ensemble import F32, Fixed, array_digest, load_reference  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
NAME = "depth_map"
FUNCTIONS = ("rmse", "delta_metric", "train_depth_map", "load_labeled_data_depth_map", "parse_image_depth_map", "benchmark_depth_map",
             "get_im_prediction_depth_map")
# (N, H, W, multipliers given, levels, special): every N of {2,3,4,5,8,9}, every size, the multipliers 2, 1, 2.5
CASES = [(2, 16, 16, (2,), 256, None), (9, 16, 16, (1,), 256, None), (3, 16, 16, (2,), 256, "nan"), (4, 16, 16, (2,), 256, "inf"),
         (3, 48, 80, (2.5,), 256, None), (8, 48, 80, (2,), 256, "edges"), (4, 64, 64, (1,), 256, "edges"), (5, 64, 64, (2,), 256, None),
         (9, 96, 96, (2,), 256, "edges"), (2, 96, 96, (2.5,), 256, None), (2, 256, 256, (2,), 16, None), (3, 256, 256, (1,), 16, "edges"),
         (2, 208, 416, (2,), 16, None), (3, 208, 416, (2.5, 1), 16, None)]


class NpRecorder:
    """numpy, except that np.mean's results are kept"""

    def __init__(self):
        self.means = []

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, *a, **k):
        r = np.mean(*a, **k)
        self.means.append(r)
        return r


def edge_multipliers(std, mean, prefer):
    """multipliers m (float32) with float32(m * mean) == s, nextafter(s, up) and nextafter(s, down) for some pixel's std s, taken from the
    pixels `prefer` marks: those whose standard deviation a planted defect moves, so that the defect flips the pixel in one of the records"""
    flat = np.unique(std[prefer])
    flat = flat[np.isfinite(flat) & (flat > mean)]
    for s in flat[len(flat) // 2:]:
        found = {}
        for kind, target in (("at", s), ("above", np.nextafter(s, F32(np.inf))), ("below", np.nextafter(s, F32(0)))):
            m = F32(target / mean)
            for cand in [m] + [f(m) for f in (lambda v: np.nextafter(v, F32(np.inf)), lambda v: np.nextafter(v, F32(0)))]:
                if F32(cand * mean) == target:
                    found[kind] = cand
                    break
        if len(found) == 3:
            return found
    return None


def golden(ref):
    rec_np = NpRecorder()
    ref.np = rec_np
    rng = np.random.default_rng(20261020)
    rec = {"numpy": np.array(np.__version__)}
    names, edge_cases = [], 0
    for n, h, w, mults, levels, special in CASES:
        name = f"n{n}_{h}x{w}" + (f"_{special}" if special else "")
        lut = np.zeros(256, F32)
        lut[:levels] = rng.random(levels, dtype=F32)
        codes = rng.integers(0, levels, n * h * w).astype(np.uint8)
        if special in ("nan", "inf"):
            lut[255] = F32(np.nan) if special == "nan" else F32(np.inf)
            codes[(n - 1) * h * w + 5 * w + 7] = 255
        preds = lut[codes].reshape(n, h, w)
        models = [Fixed(np.ascontiguousarray(preds[i]).reshape(1, h, w, 1)) for i in range(n)]

        def run(mult):
            rec_np.means.clear()
            with np.errstate(all="ignore"):
                out = ref.get_im_prediction_depth_map(models, None, float(mult) if float(mult) != int(mult) else int(mult))
            assert len(rec_np.means) == 1 and out.shape == (1, h, w, 1) and set(np.unique(out)) <= {0, 1}
            with np.errstate(all="ignore"):
                thr = (float(mult) if float(mult) != int(mult) else int(mult)) * rec_np.means[0]      # the reference's own expression
            assert np.asarray(thr).dtype == F32, "this maker needs NumPy >= 2 (float32 products stay float32)"
            return np.packbits(out.reshape(-1).astype(np.uint8)), np.asarray(thr, F32).view(np.uint32)

        kinds = ["given"] * len(mults)
        mults = [F32(m) for m in mults]
        if special == "edges":
            with np.errstate(all="ignore"):
                std = np.std(np.stack([m.arr for m in models], axis=-1), axis=-1)
                moved = np.zeros(std.shape, bool)
                for defect in ("sequential_models",) if n == 8 else ("fma_squares",):      # the N = 8 case is the order's, the others the FMA's
                    moved |= DC.std_map(preds, defect).reshape(std.shape) != std
                found = edge_multipliers(std, np.mean(std), moved)
            assert found is not None, f"{name}: no multiplier puts the threshold on a pixel's standard deviation"
            for kind in ("at", "above", "below"):
                mults.append(found[kind])
                kinds.append(kind)
            edge_cases += 1
        runs = [run(m) for m in mults]
        if special == "edges":      # the three thresholds are neighbours, and the pixel flips between `at` and `below`
            at, above, below = (int(runs[kinds.index(k)][1]) for k in ("at", "above", "below"))
            assert above == at + 1 and below == at - 1, name
            pa, pb = (np.unpackbits(runs[kinds.index(k)][0])[:h * w] for k in ("at", "below"))
            assert int(pb.sum()) > int(pa.sum()), name
        rec[name + "_shape"] = np.array([n, h, w], np.int32)
        rec[name + "_codes"], rec[name + "_lut"] = codes, lut
        rec[name + "_mults"] = np.array(mults, F32)
        rec[name + "_kinds"] = np.array(kinds)
        rec[name + "_thr_bits"] = np.array([r[1] for r in runs], np.uint32)
        rec[name + "_masks"] = np.stack([r[0] for r in runs])
        names.append(name)
    assert edge_cases >= 3
    rec["names"] = np.array(names)
    return rec


def verify(path):
    """the restatement reproduces every record; each planted defect changes at least one"""
    cases = DC.load_cases(path)
    caught = {d: [] for d in DC.DEFECTS}
    for c in cases:
        for defect in (None,) + DC.DEFECTS:
            std = DC.std_map(c["preds"], defect)
            for i, mult in enumerate(c["mults"]):
                thr = DC.threshold(std, mult, defect)
                with np.errstate(all="ignore"):
                    mask = std > thr
                ok = DC.same_bits(thr, c["thr_bits"][i:i + 1].view(F32)[0]) and np.array_equal(mask, c["masks"][i])
                if defect is None:
                    assert ok, f"the restatement misses {c['name']} at multiplier {mult}"
                elif not ok:
                    caught[defect].append(f"{c['name']}@{mult}")
    for defect, where in caught.items():
        assert where, f"the fixture cannot tell the planted defect {defect!r} from the rule"
        print(f"{defect}: caught by {len(where)} record(s), e.g. {where[:3]}")


def surface(ref):
    sig = {}
    for f in FUNCTIONS:
        sig[f] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                  for p in inspect.signature(getattr(ref, f)).parameters.values()]
    return {"signatures": sig, "delta_metric_name": ref.delta_metric(1.25).__name__}


def main():
    ref = load_reference()
    surf = surface(ref)
    rec = golden(ref)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, NAME + ".npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 1024 * 1024, os.path.getsize(path)
    verify(path)
    with np.load(path) as d:
        dig = {NAME: {key: array_digest(d[key]) for key in sorted(d.files)}}
    with open(os.path.join(OUT, NAME + "_digests.json"), "w") as f:
        json.dump(dig, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(OUT, "reference_surface_" + NAME + ".json"), "w") as f:
        json.dump(surf, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(rec)} arrays to {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
