"""The input-ensemble shims (ISIC_2018/07_*, HeLa/07_*, SUIM/08_*, Cityscapes/07_*): they exist, parse, call the shared driver with
approach="input_ensemble", and every name their reference scripts import resolves against the repo-root shims + compat layer.  The names
were read out of the reference scripts' syntax trees into tests/golden/reference_surface_input_ensemble.json
(tools/dump_reference_surface.py --out ...; names and table values only), so the test needs nothing outside this repository."""
import ast
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE = os.path.join(ROOT, "tests", "golden", "reference_surface_input_ensemble.json")
SHIMS = {"ISIC_2018/07_ISIC_2018_input_ensemble.py": "ISIC_2018", "HeLa/07_HeLa_input_ensemble.py": "HeLa",
         "SUIM/08_SUIM_input_ensemble.py": "SUIM", "Cityscapes/07_Cityscapes_input_ensemble.py": "Cityscapes"}
DATASETS = ("ISIC_2018", "HeLa", "SUIM", "Cityscapes")


def _surface():
    with open(SURFACE) as f:
        return json.load(f)


def test_shims_exist_parse_and_run_the_input_ensemble_driver():
    rec = _surface()
    assert set(SHIMS) <= set(rec["scripts"])
    for path, ds in SHIMS.items():
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "run"]
        assert len(calls) == 1, path
        c = calls[0]
        assert [a.value for a in c.args] == [ds], path
        assert {k.arg: k.value.value for k in c.keywords} == {"approach": "input_ensemble"}, path


def test_every_name_the_input_ensemble_scripts_import_resolves():
    rec = _surface()
    wanted = sorted(k for k, v in rec["wanted"].items() if set(v) & set(SHIMS))
    assert "from:functions:create_pseudo_labels_input_ensemble_ISIC_2018" in wanted
    assert "from:functions:create_pseudo_labels_input_ensemble_hela" in wanted
    assert "from:functions:create_pseudo_labels_input_ensemble_multiclass" in wanted
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
for f in ("get_input_ensemble_prediction_ISIC_2018", "get_input_ensemble_prediction_hela_hard",
          "get_input_ensemble_prediction_hela_soft", "get_input_ensemble_prediction_multiclass",
          "get_input_ensemble_prediction_multiclass_soft", "input_ensemble_prediction", "data_augmentation_image"):
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
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(getattr(F, f)).parameters.values()]
    E = inspect.Parameter.empty
    head = [("model", E), ("image", E), ("h", E), ("w", E), ("c", E)]
    aug = lambda b, m, a, be: [("max_blur", b), ("max_noise", m), ("brightness_range_alpha", a), ("brightness_range_beta", be)]
    assert sig("create_pseudo_labels_input_ensemble_ISIC_2018") == [("model", E), ("images_path", E), ("main_output_path", E), ("h", E),
        ("w", E), ("c", E), ("n", 2), ("rgb", True), ("use_n_rnd_transformations", True), ("threshold", 0.5)]
    assert sig("create_pseudo_labels_input_ensemble_hela") == [("model", E), ("bf_images_path", E), ("main_output_path", E), ("h", E),
        ("w", E), ("c", E), ("n", 2), ("use_soft_voting", False)]
    assert sig("create_pseudo_labels_input_ensemble_multiclass") == [("model", E), ("images_path", E), ("main_output_path", E),
        ("h", E), ("w", E), ("c", E), ("n", 2), ("rgb", True)]
    assert sig("get_input_ensemble_prediction_ISIC_2018") == head + [("threshold", E), ("n", 2)] + \
        aug(3, 25, (0.5, 1.5), (-25, 25)) + [("use_n_rnd_transformations", True)]
    assert sig("input_ensemble_prediction") == head + [("threshold", E)] + aug(3, 25, (0.5, 1.5), (-25, 25)) + \
        [("n", 2), ("use_n_rnd_transformations", False)]
    for f in ("get_input_ensemble_prediction_hela_hard", "get_input_ensemble_prediction_hela_soft"):
        assert sig(f) == head + [("n", 2)] + aug(1, 15, (0.7, 1.3), (-15, 15)) + [("threshold", 0.5), ("max_pos_circle_size", 8),
                                                                                ("min_pos_circle_size", 3)]
    for f in ("get_input_ensemble_prediction_multiclass", "get_input_ensemble_prediction_multiclass_soft"):
        assert sig(f) == head + [("n", 2)] + aug(1, 15, (0.7, 1.3), (-15, 15))
    assert [p for p, _ in sig("data_augmentation_image")] == ["image", "max_blur", "max_noise", "brightness_range_alpha",
                                                             "brightness_range_beta"]


def test_driver_defaults_for_the_input_ensemble():
    src = open(os.path.join(ROOT, "inconsistencymasks_amd", "im_driver.py")).read()
    assert '_ints("IM_NS", [3, 5, 7] if inp else [2, 3, 4])' in src
    assert 'inp = approach == "input_ensemble"' in src
