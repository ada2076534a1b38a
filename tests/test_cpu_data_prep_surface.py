"""The data-preparation shims (ISIC_2018/00, 01; Cityscapes/00, 01; HeLa/00, 01; SUIM/00, 01, 02): they exist, parse and call
prep_driver.run with their dataset and step; every name their reference scripts take from `paths`, `functions` and the class-mapping
module resolves against the repo-root shims; every `*_ORG_*` constant has the reference's value below its BASE_DIR; the functions and
methods the reference scripts define exist in inconsistencymasks_amd.prep with the same parameters and defaults; and config.ini has
the two keys the scripts read, with the reference's values.  All of it against tests/golden/reference_surface_data_prep.json
(tests/golden/make_golden_data_prep.py: names and values only), so the test needs nothing outside this repository."""
import ast
import configparser
import inspect
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE = os.path.join(ROOT, "tests", "golden", "reference_surface_data_prep.json")
SHIMS = {"ISIC_2018/00_ISIC_2018_preprocess_images.py": ("ISIC_2018", 0), "ISIC_2018/01_ISIC_2018_split_original_train.py": ("ISIC_2018", 1),
         "Cityscapes/00_Cityscapes_resize_images_and_masks.py": ("Cityscapes", 0),
         "Cityscapes/01_Cityscapes_split_original_train_val.py": ("Cityscapes", 1),
         "HeLa/00_HeLa_create_crops.py": ("HeLa", 0), "HeLa/01_HeLa_split_train_in_labeled_and_unlabeled.py": ("HeLa", 1),
         "SUIM/00_SUIM_convert_bmp_to_png_masks.py": ("SUIM", 0), "SUIM/01_SUIM_split_original_train_val.py": ("SUIM", 1),
         "SUIM/02_SUIM_create_crops.py": ("SUIM", 2)}


def _surface():
    with open(SURFACE) as f:
        return json.load(f)


def test_shims_exist_parse_and_run_the_prep_driver():
    rec = _surface()
    assert set(SHIMS) == set(rec["scripts"])
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import prep_driver
    assert {v[0] for v in prep_driver.SCRIPTS.values()} == set(SHIMS)
    for path, (ds, step) in SHIMS.items():
        tree = ast.parse(open(os.path.join(ROOT, path)).read())
        calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "run"]
        assert len(calls) == 1 and [a.value for a in calls[0].args] == [ds, step], path
        assert prep_driver.SCRIPTS[(ds, step)][0] == path
        # the names the reference script defines are importable from the shim under the same names
        imported = {a.asname or a.name for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.module == "inconsistencymasks_amd.prep"
                    for a in n.names}
        assert imported == {k.split(".")[0] for k in rec["signatures"].get(path, {})}, path


def test_every_name_the_scripts_import_resolves():
    wanted = sorted(_surface()["wanted"])
    assert "chain:paths:SUIM_ORG_TEST_MASKS_PNG_PATH" in wanted and "from:functions:get_pos_contours" in wanted
    probe = r"""
import importlib, json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/SUIM")
missing = []
for key in json.load(sys.stdin):
    kind, mod, name = key.split(":", 2)
    try:
        obj = importlib.import_module(mod)
        for part in name.split("."):
            obj = getattr(obj, part)
    except Exception as e:
        missing.append(f"{key} ({type(e).__name__}: {e})")
print(json.dumps(missing))
""" % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", probe], input=json.dumps(wanted), capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    missing = json.loads(r.stdout.strip().splitlines()[-1])
    assert not missing, missing


def test_org_constants_have_the_reference_values(tmp_path):
    rec = _surface()["org_paths"]
    assert len(rec) == 47
    cfg = tmp_path / "config.ini"
    cfg.write_text("".join(f"[{s}]\nBASE_DIR = /data/{s}/\n" for s in ("ISIC_2018", "HELA", "SUIM", "CITYSCAPES")))
    probe = ("import json, sys; sys.path.insert(0, %r)\nfrom inconsistencymasks_amd import paths\n"
             "print(json.dumps({k: v for k, v in vars(paths).items() if '_ORG_' in k}))" % ROOT)
    r = subprocess.run([sys.executable, "-c", probe], env={**os.environ, "IM_CONFIG": str(cfg)}, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(got) == sorted(rec)
    for k, rel in rec.items():
        section = next(s for s in ("ISIC_2018", "HELA", "SUIM", "CITYSCAPES") if k.startswith(s + "_"))
        assert os.path.normpath(got[k]) == os.path.normpath(os.path.join(f"/data/{section}", rel)), k


def test_reference_signatures():
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import prep, prep_driver
    rec = _surface()["signatures"]
    n = 0
    for (ds, step), (path, names) in prep_driver.SCRIPTS.items():
        assert sorted(names) == sorted({k.split(".")[0] for k in rec.get(path, {})}), path
        for key, want in rec.get(path, {}).items():
            obj = getattr(prep, names[key.split(".")[0]])
            if "." in key:
                obj = getattr(obj, key.split(".")[1])
            got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in inspect.signature(obj).parameters.values()]
            assert got == want, (path, key, got)
            n += 1
    assert n == 15


def test_config_has_the_keys_the_scripts_read():
    rec = _surface()
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(ROOT, "config.ini"))
    for path, keys in rec["config_keys"].items():
        for k in keys:
            section, key = k.split(".")
            assert key in cfg[section], k
    for k, v in rec["config_values"].items():
        section, key = k.split(".")
        assert cfg[section][key] == v, k
    assert sorted(rec["config_values"]) == ["CITYSCAPES.RESIZE_FACTOR", "HELA.USE_MOD_POS_SIZE"]
