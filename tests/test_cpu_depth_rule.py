"""The depth-map family's standard-deviation IM on the CPU: tests/depth_cases.py (numpy's summation order written as explicit loops)
against tests/golden/depth_map.npz, which tests/golden/make_golden_depth_map.py recorded from the reference's own
get_im_prediction_depth_map -- thresholds by their bits, masks by every pixel.  The three planted defects (no 8192 chunking, a
sequential sum over the models, FMA-contracted squares) each have to miss a record: a fixture that could not tell them from the rule
would pin nothing.  And the seven functions keep the reference's names, positional arguments and defaults
(tests/golden/reference_surface_depth_map.json)."""
import ast
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_cases as DC  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_map.npz")
SURFACE = os.path.join(ROOT, "tests", "golden", "reference_surface_depth_map.json")
FUNCTIONS = ("rmse", "delta_metric", "train_depth_map", "load_labeled_data_depth_map", "parse_image_depth_map", "benchmark_depth_map",
             "get_im_prediction_depth_map")


@pytest.fixture(scope="module")
def cases():
    return DC.load_cases(GOLDEN)


def _misses(case, defect):
    """records of `case` that the restatement (with `defect` planted) does not reproduce"""
    std = DC.std_map(case["preds"], defect)
    out = []
    for i, mult in enumerate(case["mults"]):
        thr = DC.threshold(std, mult, defect)
        with np.errstate(all="ignore"):
            mask = std > thr
        if not (DC.same_bits(thr, case["thr_bits"][i:i + 1].view(np.float32)[0]) and np.array_equal(mask, case["masks"][i])):
            out.append(f"{case['name']}@{mult}")
    return out


def test_fixture_is_the_committed_one_and_covers_the_cases():
    with open(os.path.join(ROOT, "tests", "golden", "depth_map_digests.json")) as f:
        want = json.load(f)["depth_map"]
    with np.load(GOLDEN) as d:
        assert sorted(d.files) == sorted(want)
        for key in d.files:
            a = np.ascontiguousarray(d[key])
            h = hashlib.sha256(f"{a.dtype.str}|{a.shape}|".encode())
            h.update(a.tobytes())
            assert h.hexdigest() == want[key], key
        shapes = {tuple(int(v) for v in d[str(n) + "_shape"]) for n in d["names"]}
        mults = {float(m) for n in d["names"] for m, k in zip(d[str(n) + "_mults"], d[str(n) + "_kinds"]) if str(k) == "given"}
        kinds = [str(k) for n in d["names"] for k in d[str(n) + "_kinds"]]
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    assert {s[0] for s in shapes} == {2, 3, 4, 5, 8, 9}
    assert {s[1:] for s in shapes} == {(16, 16), (48, 80), (64, 64), (96, 96), (256, 256), (208, 416)}
    assert mults == {2.0, 1.0, 2.5}
    assert min(kinds.count(k) for k in ("at", "above", "below")) >= 3


def test_restatement_reproduces_every_threshold_and_mask(cases):
    for c in cases:
        assert _misses(c, None) == [], c["name"]


def test_nan_and_inf_make_the_threshold_nan_and_the_mask_empty(cases):
    seen = 0
    for c in cases:
        if c["name"].endswith(("_nan", "_inf")):
            seen += 1
            assert not np.isfinite(c["preds"]).all()
            assert np.isnan(c["thr_bits"].view(np.float32)).all() and not c["masks"].any()
    assert seen == 2


def test_thresholds_on_a_pixel_s_standard_deviation(cases):
    """at: some pixel's std equals the threshold bit for bit and is NOT masked; one ulp below it is; the thresholds are neighbours"""
    seen = 0
    for c in cases:
        if "at" not in c["kinds"]:
            continue
        seen += 1
        at, above, below = (c["kinds"].index(k) for k in ("at", "above", "below"))
        bits = c["thr_bits"].astype(np.int64)
        assert bits[above] == bits[at] + 1 and bits[below] == bits[at] - 1
        std = DC.std_map(c["preds"])
        on = std.view(np.uint32) == c["thr_bits"][at]
        assert on.any() and not c["masks"][at][on].any() and c["masks"][below][on].all()
    assert seen >= 3


@pytest.mark.parametrize("defect", DC.DEFECTS)
def test_each_planted_defect_misses_a_record(cases, defect):
    missed = [m for c in cases for m in _misses(c, defect)]
    assert missed, f"the fixture cannot tell {defect!r} from the rule"


def test_reference_names_signatures_and_defaults():
    with open(SURFACE) as f:
        rec = json.load(f)
    assert sorted(rec["signatures"]) == sorted(FUNCTIONS)
    assert rec["delta_metric_name"] == "delta_1.25"
    # read from the source: importing the package needs the built library, and this test runs without one as well
    tree = ast.parse(open(os.path.join(ROOT, "inconsistencymasks_amd", "depth.py")).read())
    defs = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    for name, want in rec["signatures"].items():
        a = defs[name].args
        assert not a.vararg and not a.kwarg and not a.kwonlyargs and not a.posonlyargs, name
        names = [x.arg for x in a.args]
        defaults = [None] * (len(names) - len(a.defaults)) + [repr(ast.literal_eval(d)) for d in a.defaults]
        assert [[n, d] for n, d in zip(names, defaults)] == want, name
    src = open(os.path.join(ROOT, "inconsistencymasks_amd", "functions.py")).read()
    for name in FUNCTIONS:      # exported from the package's functions module, which the repo-root `functions` re-exports with *
        assert name in src.split("from .depth import")[1].split(")")[0], name


def test_metric_name_and_values_without_the_library():
    """rmse and delta_metric are host restatements: load depth.py's two functions alone"""
    tree = ast.parse(open(os.path.join(ROOT, "inconsistencymasks_amd", "depth.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("rmse", "delta_metric")]
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "depth.py", "exec"), ns)
    m = ns["delta_metric"]()
    assert m.__name__ == "delta_1.25" and ns["delta_metric"](1.5).__name__ == "delta_1.5"
    y = np.array([0.0, 0.5, 0.5, 1.0, 0.2], np.float32)
    p = np.array([0.3, 0.5, 0.7, 0.81, np.nan], np.float32)
    assert m(y, p) == np.float32(2 / 5)            # y = 0 and NaN count as false; 0.7 / 0.5 = 1.4 misses, 1 / 0.81 = 1.23 hits
    assert ns["rmse"](y[:4], p[:4]) == np.sqrt(np.mean((p[:4] - y[:4]) ** 2, dtype=np.float32))
