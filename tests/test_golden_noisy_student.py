"""The pin of the noisy-student label pass: tests/golden/make_golden_noisy_student.py drives the REAL reference's
create_pseudo_labels_noisy_student_* (functions.py:3243-3417) with fixed-prediction fake models and a numpy cv2 stub, and records a
sha256 of every array in tests/golden/noisy_student_digests.json.  The committed fixture must be exactly what that regeneration
recorded; with a reference checkout on disk (IMK_REFERENCE) it is regenerated into a temporary directory and compared.
augment.draw_params must reproduce the recorded flips, turn, coin and blur size under the recorded seeds, and the label rules the
kernels implement, restated in numpy (threshold or arg-max, then the recorded geometry), must reproduce every recorded mask."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from test_golden_model_ensemble import array_digest, np_argmax_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
# the strengths the generator handed to the three writers: (brightness alpha range, beta range, max_blur, max_noise)
STRENGTH = {"isic": ((0.9, 1.1), (-5, 5), 3, 5), "hela": ((0.9, 1.1), (-3, 3), 2, 10), "mc": ((0.9, 1.1), (-5, 5), 1, 5)}


def load():
    with np.load(os.path.join(GOLD, "noisy_student.npz")) as d:
        return {k: d[k] for k in d.files}


def cases(d, kind):
    return sorted({k.split("_")[0] for k in d if k.startswith(kind) and k[len(kind)].isdigit()})


def moved(a, draws):
    from oracle.aug_oracle import geometric
    return geometric(a, int(draws[0]), int(draws[1]), int(draws[2]))


def test_fixture_digests():
    with open(os.path.join(GOLD, "noisy_student_digests.json")) as f:
        want = json.load(f)["noisy_student"]
    d = load()
    assert sorted(d) == sorted(want)
    for k, v in d.items():
        assert array_digest(v) == want[k], k


@pytest.mark.skipif(not os.environ.get("IMK_REFERENCE"), reason="needs a reference checkout (IMK_REFERENCE)")
def test_fixture_regenerates(tmp_path):
    env = dict(os.environ, IMK_GOLDEN_OUT=str(tmp_path))
    subprocess.check_call([sys.executable, os.path.join(GOLD, "make_golden_noisy_student.py")], env=env)
    with open(tmp_path / "noisy_student_digests.json") as f, open(os.path.join(GOLD, "noisy_student_digests.json")) as g:
        assert json.load(f) == json.load(g)
    with open(tmp_path / "reference_surface_noisy_student.json") as f, open(os.path.join(GOLD, "reference_surface_noisy_student.json")) as g:
        assert json.load(f) == json.load(g)


def test_cases_present():
    d = load()
    assert len(cases(d, "isic")) == 8 and len(cases(d, "hela")) == 6 and len(cases(d, "mc")) == 6
    assert sorted({int(d[c + "_probs"].shape[-1]) for c in cases(d, "mc")}) == [3, 9, 35]
    draws = np.stack([d[c + "_draws"] for k in ("isic", "hela", "mc") for c in cases(d, k)])
    assert set(draws[:, 2]) == {0, 1, 2, 3} and set(draws[:, 0]) == {0, 1} and set(draws[:, 1]) == {0, 1}      # every turn, both flips
    assert set(draws[:, 3]) == {0, 1} and {0, 3}.issubset(set(draws[:, 4]))
    half = F32(0.5)
    for c in cases(d, "isic") + cases(d, "hela"):
        p = d[c + "_preds"]
        assert np.isnan(p).any() and (p == half).any() and (p == np.nextafter(half, F32(1))).any() and (p == np.nextafter(half, F32(0))).any(), c
    assert any(np.isnan(d[c + "_probs"]).any() for c in cases(d, "mc"))
    assert any(int(d[c + "_free"]) == 0 for c in cases(d, "isic")) and any(int(d[c + "_free"]) == 0 for c in cases(d, "mc"))


def test_file_names():
    d = load()
    for c in cases(d, "isic") + cases(d, "mc"):
        img, msk = d[c + "_files"].tolist()
        assert img.startswith("images/") and msk == "masks/" + img[len("images/"):], c
    for c in cases(d, "hela"):
        files = d[c + "_files"].tolist()
        assert [f.split("/")[0] for f in files] == ["brightfield", "alive", "dead", "mod_position"], c
        assert all(f.endswith("_aug.png") for f in files) and len({f.split("/")[1] for f in files}) == 1, c


def test_host_draws_match_the_reference():
    from inconsistencymasks_amd import augment
    d = load()
    for kind in ("isic", "hela", "mc"):
        bra, brb, max_blur, max_noise = STRENGTH[kind]
        for c in cases(d, kind):
            rng = random.Random(int(d[c + "_seed"]))
            q = augment.draw_params(1, bra, brb, max_blur, max_noise, bool(d[c + "_free"]), rng=rng, np_rng=np.random.RandomState(0))[0]
            assert [q.flip_v, q.flip_h, q.rot, q.bright_on, q.blur_k] == d[c + "_draws"].tolist(), c
            assert q.noise_max == max_noise


def test_rules_restated_reproduce_the_reference():
    d = load()
    for c in cases(d, "isic"):
        lab = np.where(d[c + "_preds"][0, ..., 0] > F32(0.5), 255, 0).astype(np.uint8)      # NaN compares false
        got = moved(lab, d[c + "_draws"])
        assert got.dtype == d[c + "_mask"].dtype and np.array_equal(got, d[c + "_mask"]), c
    for c in cases(d, "hela"):
        lab = np.where(d[c + "_preds"][0] >= F32(0.5), 255, 0).astype(np.uint8)               # threshold, then move: they commute
        got = moved(lab, d[c + "_draws"])
        for j, what in enumerate(("alive", "dead", "pos")):
            assert np.array_equal(got[..., j], d[c + "_" + what]), (c, what)
        assert d[c + "_pos"].dtype == np.uint8
    for c in cases(d, "mc"):
        lab = np_argmax_rule(d[c + "_probs"][0])
        assert np.array_equal(lab, np.argmax(d[c + "_probs"][0], -1))
        want = d[c + "_mask"]
        assert want.dtype == np.int64      # what np.argmax hands to imwrite; the writer here stores uint8 class ids
        assert np.array_equal(moved(lab, d[c + "_draws"]), want) and want.max() < 256, c
