"""The model-ensemble shims (ISIC_2018/06_*, HeLa/06_*, SUIM/07_*, Cityscapes/06_*): they exist, parse, call the shared driver with
approach="model_ensemble", and every name their reference scripts import resolves against the repo-root shims + compat layer.  The names
were read out of the reference scripts' syntax trees into tests/golden/reference_surface_model_ensemble.json
(tools/dump_reference_surface.py --out ...; names and table values only), so the test needs nothing outside this repository."""
import ast
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE = os.path.join(ROOT, "tests", "golden", "reference_surface_model_ensemble.json")
SHIMS = {"ISIC_2018/06_ISIC_2018_model_ensemble.py": "ISIC_2018", "HeLa/06_HeLa_model_ensemble.py": "HeLa",
         "SUIM/07_SUIM_model_ensemble.py": "SUIM", "Cityscapes/06_Cityscapes_model_ensemble.py": "Cityscapes"}
DATASETS = ("ISIC_2018", "HeLa", "SUIM", "Cityscapes")


def _surface():
    with open(SURFACE) as f:
        return json.load(f)


def test_shims_exist_parse_and_run_the_model_ensemble_driver():
    rec = _surface()
    assert set(SHIMS) <= set(rec["scripts"])
    for path, ds in SHIMS.items():
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "run"]
        assert len(calls) == 1, path
        c = calls[0]
        assert [a.value for a in c.args] == [ds], path
        assert {k.arg: k.value.value for k in c.keywords} == {"approach": "model_ensemble"}, path


def test_every_name_the_model_ensemble_scripts_import_resolves():
    rec = _surface()
    wanted = sorted(k for k, v in rec["wanted"].items() if set(v) & set(SHIMS))
    assert "from:functions:create_pseudo_labels_model_ensemble_ISIC_2018" in wanted
    assert "from:functions:create_pseudo_labels_model_ensemble_hela" in wanted
    assert "from:functions:create_pseudo_labels_model_ensemble_multiclass" in wanted
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
import functions
for f in ("get_model_ensemble_prediction_ISIC_2018", "get_model_ensemble_prediction_multiclass_hard",
          "get_model_ensemble_prediction_multiclass_soft", "get_model_ensemble_prediction_hela_soft"):
    if not callable(getattr(functions, f, None)):
        missing.append("functions." + f)
print(json.dumps(missing))
""" % (ROOT, os.path.join(ROOT, "inconsistencymasks_amd", "compat"), list(DATASETS), ROOT)
    r = subprocess.run([sys.executable, "-c", probe], input=json.dumps(wanted), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    missing = json.loads(r.stdout.strip().splitlines()[-1])
    assert not missing, missing


def test_reference_signatures_of_the_writers_and_predictions():
    import inspect
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import functions as F
    sig = lambda f: list(inspect.signature(getattr(F, f)).parameters)
    assert sig("create_pseudo_labels_model_ensemble_ISIC_2018") == ["models", "images_path", "main_output_path", "h", "w", "c", "rgb",
                                                                    "threshold"]
    assert sig("create_pseudo_labels_model_ensemble_multiclass") == ["models", "images_path", "main_output_path", "h", "w", "c", "rgb"]
    assert sig("create_pseudo_labels_model_ensemble_hela") == ["models", "bf_images_path", "main_output_path", "h", "w", "c"]
    assert sig("get_model_ensemble_prediction_ISIC_2018") == ["models", "prepared_image", "image_width", "image_height", "threshold"]
    assert sig("get_model_ensemble_prediction_hela_soft") == ["models", "prepared_image", "threshold", "max_pos_circle_size",
                                                              "min_pos_circle_size"]
    assert sig("get_model_ensemble_prediction_multiclass_soft") == sig("get_model_ensemble_prediction_multiclass_hard") == \
        ["models", "prepared_image"]
