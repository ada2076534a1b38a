"""The pin of the model-ensemble vote: tests/golden/make_golden_model_ensemble.py drives the REAL reference's
get_model_ensemble_prediction_* (functions.py:2409-2566) with fixed-prediction fake models and records a sha256 of every array in
tests/golden/model_ensemble_digests.json.  The committed fixture must be exactly what that regeneration recorded; with a reference
checkout on disk (IMK_REFERENCE) it is regenerated into a temporary directory and compared array for array.  The rules the kernels
implement (include/imk.h: imk_vote_binary / imk_vote_multiclass), restated in numpy, must reproduce every recorded output."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


def array_digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(f"{a.dtype.str}|{a.shape}|".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def load():
    with np.load(os.path.join(GOLD, "model_ensemble.npz")) as d:
        return {k: d[k] for k in d.files}


def cases(d, kind):
    return sorted({k.split("_")[0] for k in d if k.startswith(kind) and k[len(kind)].isdigit()})


# ---- the kernels' rules, restated --------------------------------------------------------------------------------------------
def np_argmax_rule(v):
    """np.argmax over the last axis written out as the kernels scan: the first NaN wins, else the first maximum"""
    out = np.zeros(v.shape[:-1], np.int64)
    for idx in np.ndindex(v.shape[:-1]):
        row = v[idx]
        bk, bv = 0, row[0]
        for k in range(1, row.shape[0]):
            if np.isnan(bv):
                break
            if np.isnan(row[k]) or row[k] > bv:
                bk, bv = k, row[k]
        out[idx] = bk
    return out


def vote_binary_rule(preds, thr, soft):
    """preds [N,...] float32 -> u8 {0,255}: hard = every p > thr (float32 compare); soft = fp64 sum in model order / N > thr"""
    if soft:
        s = np.zeros(preds.shape[1:], np.float64)
        for p in preds:
            s = s + p.astype(np.float64)
        on = s / float(len(preds)) > float(thr)
    else:
        on = np.all(preds > F32(thr), 0)
    return np.where(on, 255, 0).astype(np.uint8)


def vote_multi_rule(probs, soft):
    """probs [N,...,K] float32 -> u8 labels: soft = argmax of fl32(sequential fp32 sum / N); hard = common argmax else 0"""
    if soft:
        s = probs[0].copy()
        for p in probs[1:]:
            s = (s + p).astype(F32)
        return np_argmax_rule((s / F32(len(probs))).astype(F32)).astype(np.uint8)
    labs = np.stack([np_argmax_rule(p) for p in probs])
    return np.where(np.all(labs == labs[0], 0), labs[0], 0).astype(np.uint8)


# ---- tests ---------------------------------------------------------------------------------------------------------------------
def test_fixture_equals_what_the_reference_regeneration_recorded():
    with open(os.path.join(GOLD, "model_ensemble_digests.json")) as f:
        rec = json.load(f)
    assert sorted(rec) == ["model_ensemble"]
    d = load()
    assert sorted(d) == sorted(rec["model_ensemble"])
    for k, a in d.items():
        assert array_digest(a) == rec["model_ensemble"][k], k


def test_fixture_covers_the_issue_cases():
    d = load()
    ns = {d[c + "_preds"].shape[0] for c in cases(d, "bin")} | {d[c + "_preds"].shape[0] for c in cases(d, "hela")}
    ns |= {d[c + "_probs"].shape[0] for c in cases(d, "mc")}
    assert {2, 3, 4, 5, 8} <= ns
    assert {3, 9, 35, 64} <= {d[c + "_probs"].shape[-1] for c in cases(d, "mc")}
    assert all(np.isnan(d[c + "_preds"]).any() for c in cases(d, "bin") + cases(d, "hela"))
    assert all(np.isnan(d[c + "_probs"]).any() for c in cases(d, "mc"))
    # argmax(sum) != argmax(mean): ties the fp32 divide creates
    tie = 0
    for c in cases(d, "mc"):
        p = d[c + "_probs"][:, 0]
        s = p[0].copy()
        for q in p[1:]:
            s = (s + q).astype(F32)
        tie += int(np.sum(np_argmax_rule(s) != d[c + "_soft"]))
    assert tie > 0
    # HeLa: a pixel where the fp64 average says 255 and an fp32 one 0
    p = d["hela0_preds"][:, 0]
    f32 = ((p[0] + p[1]).astype(F32) / F32(2)) > F32(0.5)
    assert np.any((d["hela0_alive"] == 255) & ~f32[..., 0])


def test_numpy_restatement_of_the_kernel_rules_reproduces_the_reference():
    d = load()
    for c in cases(d, "bin"):
        preds, thr, out = d[c + "_preds"][:, 0, ..., 0], d[c + "_thr"], d[c + "_out"]
        assert out.dtype == np.float64 and out.shape == preds.shape[1:]
        assert np.array_equal(vote_binary_rule(preds, thr, False).astype(np.float64), out), c
    for c in cases(d, "hela"):
        preds, thr = d[c + "_preds"][:, 0], d[c + "_thr"]
        got = vote_binary_rule(preds, thr, True)
        for j, key in enumerate(("alive", "dead", "pos")):
            assert np.array_equal(got[..., j], d[f"{c}_{key}"]), (c, key)
    for c in cases(d, "mc"):
        probs = d[c + "_probs"][:, 0]
        assert np.array_equal(vote_multi_rule(probs, True), d[c + "_soft"]), c
        assert np.array_equal(vote_multi_rule(probs, False), d[c + "_hard"]), c


@pytest.mark.skipif(not os.environ.get("IMK_REFERENCE"), reason="needs a reference checkout (IMK_REFERENCE)")
def test_regeneration_from_the_reference_matches(tmp_path):
    env = dict(os.environ, IMK_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_model_ensemble.py")], check=True, env=env, cwd=str(tmp_path),
                   capture_output=True)
    with np.load(tmp_path / "model_ensemble.npz") as fresh:
        d = load()
        assert sorted(fresh.files) == sorted(d)
        for k in d:
            assert np.array_equal(fresh[k], d[k], equal_nan=d[k].dtype.kind == "f"), k
