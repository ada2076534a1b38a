"""The consistency-loss shims (ISIC_2018/05_*, HeLa/05_*, SUIM/06_*, Cityscapes/05_*): they exist, parse and call the shared driver, every
name their reference scripts import resolves against the repo-root shims + compat layer, the three training functions carry the
reference's signatures and defaults, and the driver's facts (model and pretrained-file names, run ids, candidates, strengths, the four
schedule tables, ranking, headers) equal what tests/golden/make_golden_consistency_loss.py read out of the reference scripts' syntax
trees into tests/golden/reference_surface_consistency_loss.json (names and values only): nothing outside this repository is read."""
import ast
import inspect
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE = os.path.join(ROOT, "tests", "golden", "reference_surface_consistency_loss.json")
SHIMS = {"ISIC_2018/05_ISIC_2018_consistency_loss.py": "ISIC_2018", "HeLa/05_HeLa_consistency_loss.py": "HeLa",
         "SUIM/06_SUIM_consistency_loss.py": "SUIM", "Cityscapes/05_Cityscapes_consistency_loss.py": "Cityscapes"}
TRAINERS = ("train_ISIC_2018_consistency_loss", "train_hela_consistency_loss", "train_multiclass_consistency_loss")


def _surface():
    with open(SURFACE) as f:
        return json.load(f)


def _driver():
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import consistency_driver
    return consistency_driver


def test_shims_exist_parse_and_run_the_consistency_driver():
    rec = _surface()
    assert set(SHIMS) == set(rec["scripts"])
    for path, ds in SHIMS.items():
        src = open(os.path.join(ROOT, path)).read()
        assert len(src.splitlines()) == 11, path
        tree = ast.parse(src)
        imports = [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
        assert [(n.module, [a.name for a in n.names]) for n in imports] == [("inconsistencymasks_amd.consistency_driver", ["run"])], path
        calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "run"]
        assert len(calls) == 1 and [a.value for a in calls[0].args] == [ds] and not calls[0].keywords, path


def test_every_name_the_consistency_scripts_import_resolves():
    rec = _surface()
    wanted = sorted(rec["wanted"])
    assert any(k.endswith(":" + TRAINERS[0]) for k in wanted)
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
""" % (ROOT, os.path.join(ROOT, "inconsistencymasks_amd", "compat"), sorted(SHIMS.values()), ROOT)
    r = subprocess.run([sys.executable, "-c", probe], input=json.dumps(wanted), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    missing = json.loads(r.stdout.strip().splitlines()[-1])
    assert not missing, missing


def test_reference_signatures_of_the_training_functions():
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import functions as F
    import functions as root_functions
    rec = _surface()["signatures"]
    assert sorted(rec) == sorted(TRAINERS)
    for f in TRAINERS:
        got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(getattr(F, f)).parameters.values()]
        assert got == rec[f], f
        assert getattr(root_functions, f) is getattr(F, f), f
    assert rec["train_multiclass_consistency_loss"][-2:] == [["validation_frequency", "1"], ["print_results", "False"]]


def test_names_loops_and_schedules_equal_the_scripts():
    D, facts = _driver(), _surface()["script_facts"]
    pairs = lambda v: [tuple(p) for p in v]
    for path, ds in SHIMS.items():
        f, s = facts[path], D.SCHEDULES[ds]
        assert f["approach"] == D.APPROACH == "consistency_loss"
        assert f["loops"] == [["runid", 1, 4], ["i", 0, 5]], path
        assert f["aug_strenghts"] == D.AUG_STRENGTHS
        assert D.model_name(ds, 2, "mid") == f["modelname"].format(approach=D.APPROACH, runid=2, augs="mid"), path
        assert D.pretrained_name(ds, 3) == f["pretrained"].format(runid=3), path
        assert s["max_blurs"] == f["max_blurs"] and s["max_noises"] == f["max_noises"], path
        assert s["brightness_range_alphas"] == pairs(f["brightness_range_alphas"]), path
        assert s["brightness_range_betas"] == pairs(f["brightness_range_betas"]), path
    assert D.SCHEDULES["Cityscapes"]["max_blurs"] == [0, 0, 1]


def test_ranking_and_headers():
    D, facts = _driver(), _surface()["script_facts"]
    for path, ds in SHIMS.items():
        f = facts[path]
        assert D.RANK[ds] == (f["rank_index"], f["rank_descending"]), path
        assert D.HEADERS[ds] == f["Header"], path
    assert D.RANK["HeLa"] == (6, False) and len(D.HEADERS["HeLa"]) == 10      # nine values per candidate


def test_gradient_data_parallelism_is_refused(monkeypatch):
    """world size above 1 in gradient mode: a clear error, not a silently wrong run; whole candidates per rank run inside
    functions.local_rank_scope, where the world is 1"""
    import pytest
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import consistency, functions as F
    monkeypatch.setattr(F, "_rank_world", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="gradient data parallelism"):
        consistency._train("t", None, "x.h5", None, None, None, None, None, 0, True, 1, 10, (0.9, 1.1), (-1, 1), 1)
