"""The EvalNet-ensemble shims (ISIC_2018/10_*, HeLa/10_*, SUIM/11_*, Cityscapes/10_*): they exist, parse and call the shared driver
once; every name their reference scripts import resolves against the repo-root shims + compat layer; the six functions keep the
reference's signatures; and the driver's loops, names, rankings, CSV headers and threshold keys are the scripts'.  All of that was read
out of the reference into tests/golden/reference_surface_evalnet_ensemble.json by tests/golden/make_golden_evalnet_ensemble.py (names and
values only), so the test needs nothing outside this repository.  The last test holds the host geometry that redraws HeLa's position plane to the
reference's recorded circle calls."""
import ast
import inspect
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE = os.path.join(ROOT, "tests", "golden", "reference_surface_evalnet_ensemble.json")
SHIMS = {"ISIC_2018/10_ISIC_2018_evalnet_ensemble.py": "ISIC_2018", "HeLa/10_HeLa_evalnet_miou_ensemble.py": "HeLa",
         "SUIM/11_SUIM_evalnet_miou_ensemble.py": "SUIM", "Cityscapes/10_Cityscapes_evalnet_miou_ensemble.py": "Cityscapes"}
DATASETS = ("ISIC_2018", "HeLa", "SUIM", "Cityscapes")


def _surface():
    with open(SURFACE) as f:
        return json.load(f)


def test_shims_exist_parse_and_run_the_segnet_driver():
    rec = _surface()
    assert sorted(SHIMS) == rec["scripts"]
    for path, ds in SHIMS.items():
        src = open(os.path.join(ROOT, path)).read()
        assert len(src.splitlines()) == 11, path
        tree = ast.parse(src)
        calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "run"]
        assert len(calls) == 1, path
        assert [a.value for a in calls[0].args] == [ds] and not calls[0].keywords, path
        imports = [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
        assert [(n.module, [a.name for a in n.names]) for n in imports] == [("inconsistencymasks_amd.segnet_driver", ["run"])], path


def test_every_name_the_evalnet_ensemble_scripts_import_resolves():
    rec = _surface()
    wanted = sorted(rec["wanted"])
    for f in rec["signatures"]:
        assert "from:functions:" + f in wanted, f
    probe = r"""
import importlib, json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
for ds in %r:
    sys.path.insert(0, %r + "/" + ds)
missing = []
for key in json.load(sys.stdin):
    kind, mod, name = key.split(":", 2)
    try:
        parts = mod.split(".")
        m = importlib.import_module(parts[0])
        for part in parts[1:]:
            m = getattr(m, part) if hasattr(m, part) else importlib.import_module(m.__name__ + "." + part)
        obj = m
        for part in name.split("."):
            try:
                obj = getattr(obj, part)
            except AttributeError:
                obj = importlib.import_module(obj.__name__ + "." + part)
    except Exception as e:
        missing.append(f"{key} ({type(e).__name__}: {e})")
print(json.dumps(missing))
""" % (ROOT, os.path.join(ROOT, "inconsistencymasks_amd", "compat"), list(DATASETS), ROOT)
    r = subprocess.run([sys.executable, "-c", probe], input=json.dumps(wanted), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    missing = json.loads(r.stdout.strip().splitlines()[-1])
    assert not missing, missing


def test_the_six_functions_keep_the_reference_signatures():
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import functions as F
    rec = _surface()
    assert len(rec["signatures"]) == 6
    for f, want in rec["signatures"].items():
        got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(getattr(F, f)).parameters.values()]
        assert got == want, f


def test_driver_facts_equal_the_scripts():
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import segnet_driver as D
    from inconsistencymasks_amd.im_driver import DATASETS as DS
    rec = _surface()
    for path, ds in SHIMS.items():
        facts = rec["script_facts"][path]
        kind = DS[ds]["kind"]
        tag, evalnet_tag, ev_sub, segnet_tag = D.names(ds)
        assert facts["names"]["modelname"] == [segnet_tag + "_{runid}_n{n}_gen{gen}"], path
        assert facts["names"]["modelname_last_gen"] == [segnet_tag + "_{runid}_n{n}_gen{gen - 1}"], path
        assert facts["names"]["modelname_evalnet"] == [evalnet_tag + "_{runid}_{i}"], path
        assert facts["names"]["modelname_i"] == ["{modelname}_{i}"], path
        assert facts["ranks"] == [[D.EVALNET_RANK[kind], False], [DS[ds]["rank"], True]], path
        assert facts["headers"] == [D.EVALNET_HEADER[kind], D.csv_header(ds)], path
        assert sorted(facts["threshold_key"]) == sorted([tag, D.THRESHOLD_KEY[kind]]), path
        assert {ev_sub, "segnet", "subset", "train", "val", "train_unlabeled_predictions"} <= set(facts["joined"]), path
        assert sorted(facts["model_i"]) == [0, 3, 10, 13], path      # model_i starts at 0 / 10, validation data while < 3 / < 13
        assert facts["loops"] == [["runid", 1, 4], ["n", 2, 5], ["i", 0, 5], ["gen", 0, 5], ["j", 1, ["n", 1]],
                                  ["i", 0, 5], ["j", 0, 10], ["j", 0, 5]], path
        if kind != "multi":      # the multi-class scripts pass a CategoricalCrossentropy object
            assert facts["loss"] == "mse", path
        # the same loops as the driver's constants have them
        loops = facts["loops"]
        assert [loops[0], loops[1], loops[3]] == [["runid", D.RUNIDS[0], D.RUNIDS[-1] + 1], ["n", D.NS[0], D.NS[-1] + 1],
                                                  ["gen", D.GENS[0], D.GENS[-1] + 1]], path
        assert loops[2] == ["i", D.EVALNET_CANDIDATES[0], D.EVALNET_CANDIDATES[-1] + 1], path
        assert loops[5] == ["i", D.CANDIDATES[0], D.CANDIDATES[-1] + 1] and loops[7] == ["j", D.CANDIDATES[0], D.CANDIDATES[-1] + 1], path
        assert loops[6] == ["j", 0, D.N_SUBSET_MODELS], path
        firsts = [f for f, _ in D.EVALNET_SOURCES]
        assert sorted(facts["model_i"]) == sorted(firsts + [f + D.N_VAL_MODELS for f in firsts]), path
    for v in (D.RUNIDS, D.NS, D.GENS, D.CANDIDATES, D.EVALNET_CANDIDATES):
        assert v == list(range(v[0], v[-1] + 1))
    assert [w for _, w in D.EVALNET_SOURCES] == ["subset", "subset_aug"]


def test_hela_redraw_draws_the_recorded_circles():
    """the HeLa selection writer redraws the chosen position plane with F._hela_vote_positions(plane, 8, 3).  The reference's own
    cv2.circle calls for reported positions are recorded in tests/golden/evalnet_ensemble.npz ("hela0_circles": several positions,
    "hela1_circles": a lone one): on a plane whose blobs sit at those positions the host geometry must draw those radii."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import functions as F
    from oracle import hela_geometry as G
    with np.load(os.path.join(ROOT, "tests", "golden", "evalnet_ensemble.npz")) as d:
        records = [d["hela0_circles"], d["hela1_circles"]]
    for rec in records:
        plane = np.zeros((64, 64), np.uint8)
        for x, y in rec[:, :2].tolist():      # a 5 x 5 blob whose eroded centre of mass, plus one, is (x, y)
            plane[y - 3:y + 2, x - 3:x + 2] = 255
        assert sorted(F.get_pos_contours(plane)) == sorted(map(tuple, rec[:, :2].tolist()))
        want = np.zeros((64, 64), np.uint8)
        for x, y, r in rec[:, :3].tolist():
            G._disc(want, x, y, r, 255)
        assert rec[:, 3:].tolist() == [[255, 255, 255, -1]] * len(rec)      # filled, white on all three channels
        assert np.array_equal(F._hela_vote_positions(plane, 8, 3), np.repeat(want[..., None], 3, 2))
