"""The single-EvalNet shims (ISIC_2018/10_ISIC_2018_evalnet.py, SUIM/11_SUIM_evalnet_miou.py) and the full-dataset shims
(ISIC_2018/02_*, HeLa/02_*, Cityscapes/02_*, SUIM/03_*): they exist, parse and call their driver once; every name their reference scripts
import resolves against the repo-root shims + compat layer; the two selection writers keep the reference's signatures; and the drivers'
loops, names, rankings, CSV headers, threshold keys and directories are the scripts'.  All of that was read out of the reference into
tests/golden/reference_surface_evalnet_single.json by tests/golden/make_golden_evalnet_single.py (names and values only), so the test needs
nothing outside this repository.  The drivers are also run dry -- the `functions` entry points replaced by recorders, no GPU -- and the
trace of their calls is held to the same record."""
import ast
import inspect
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACE = os.path.join(ROOT, "tests", "golden", "reference_surface_evalnet_single.json")
SINGLE = {"ISIC_2018/10_ISIC_2018_evalnet.py": "ISIC_2018", "SUIM/11_SUIM_evalnet_miou.py": "SUIM"}
FULL = {"ISIC_2018/02_ISIC_2018_full_dataset.py": "ISIC_2018", "HeLa/02_HeLa_full_dataset.py": "HeLa",
        "Cityscapes/02_Cityscapes_full_dataset.py": "Cityscapes", "SUIM/03_SUIM_full_dataset.py": "SUIM"}
DATASETS = ("ISIC_2018", "HeLa", "SUIM", "Cityscapes")


def _surface():
    with open(SURFACE) as f:
        return json.load(f)


def test_shims_exist_parse_and_run_their_driver():
    rec = _surface()
    assert sorted({**SINGLE, **FULL}) == rec["scripts"]
    for shims, module, keyword, value in ((SINGLE, "segnet_driver", "ensemble", False), (FULL, "subset_driver", "full", True)):
        for path, ds in shims.items():
            src = open(os.path.join(ROOT, path)).read()
            assert len(src.splitlines()) == 11, path
            tree = ast.parse(src)
            calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "run"]
            assert len(calls) == 1, path
            assert [a.value for a in calls[0].args] == [ds] and [(k.arg, k.value.value) for k in calls[0].keywords] == [(keyword, value)], path
            imports = [n for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
            assert [(n.module, [a.name for a in n.names]) for n in imports] == [("inconsistencymasks_amd." + module, ["run"])], path


def test_every_name_the_six_scripts_import_resolves():
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


def test_the_two_writers_keep_the_reference_signatures():
    sys.path.insert(0, ROOT)
    import functions as top      # the repo-root module the scripts import from
    from inconsistencymasks_amd import functions as F
    rec = _surface()
    assert sorted(rec["signatures"]) == ["create_training_data_by_evalnet_miou_for_segnet_multiclass",
                                         "create_training_data_for_segnet_ISIC_2018"]
    for f, want in rec["signatures"].items():
        got = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(getattr(F, f)).parameters.values()]
        assert got == want, f
        assert getattr(top, f) is getattr(F, f), f


def test_single_evalnet_driver_facts_equal_the_scripts():
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import segnet_driver as D
    from inconsistencymasks_amd.im_driver import DATASETS as DS
    rec = _surface()
    assert sorted(D.SINGLE_DATASETS) == sorted(SINGLE.values())
    for ds in ("HeLa", "Cityscapes"):      # no such script in the reference: refused by name
        with pytest.raises(ValueError, match=ds):
            D.single_names(ds)
        with pytest.raises(ValueError, match=ds):
            D.run(ds, ensemble=False)
    for path, ds in SINGLE.items():
        facts = rec["script_facts"][path]
        tag, evalnet_tag, ev_sub, segnet_tag = D.single_names(ds)
        assert facts["names"]["modelname"] == [segnet_tag + "_{runid}_gen{gen}"], path      # no n
        assert facts["names"]["modelname_last_gen"] == [segnet_tag + "_{runid}_gen{gen - 1}"], path
        assert facts["names"]["modelname_evalnet"] == [evalnet_tag + "_{runid}"], path      # one EvalNet per run id
        assert facts["names"]["modelname_i"] == ["{modelname}_{i}"], path
        assert facts["ranks"] == [[DS[ds]["rank"], True]], path      # the U-Nets alone are ranked
        assert facts["headers"] == [D.SINGLE_HEADER, DS[ds]["header"]], path
        assert sorted(facts["threshold_key"]) == sorted(D.SINGLE_THRESHOLD_KEY[ds]), path
        assert {ev_sub, "segnet", "subset", "train", "val", "train_unlabeled_predictions"} <= set(facts["joined"]), path
        assert "evalnet_ensemble" not in facts["joined"] and "evalnet_miou_ensemble" not in facts["joined"], path
        assert facts["model_i"] == [f for f, _ in D.EVALNET_SOURCES] == [0, 10], path      # no `model_i < 3`: every model writes val data
        assert facts["loops"] == [["runid", D.RUNIDS[0], D.RUNIDS[-1] + 1], ["gen", D.GENS[0], D.GENS[-1] + 1],
                                  ["i", D.CANDIDATES[0], D.CANDIDATES[-1] + 1], ["j", 0, D.N_SUBSET_MODELS],
                                  ["j", D.CANDIDATES[0], D.CANDIDATES[-1] + 1]], path
        assert facts["floor"] is False, path      # STEPS_PER_EPOCH = images // BATCH_SIZE, no max() with a share of the full set
        assert {f"{tag}_TRAIN_LABELED_AUG_IMAGES_DIR", f"{tag}_TRAIN_LABELED_AUG_MASKS_DIR"} <= set(facts["paths"]), path
    isic, suim = (rec["script_facts"][p] for p in SINGLE)
    assert isic["results"] == [["modelname_evalnet", "mse", "mae"]] and isic["loss"] == "mse"
    assert suim["results"] == [["total_loss", "iou_loss", "conf_loss", "iou_mae", "conf_mae"]]      # five values, no name, three headers
    assert len(suim["results"][0]) == 5 and len(D.SINGLE_HEADER) == 3


def test_full_dataset_driver_facts_equal_the_scripts():
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd import subset_driver as D
    from inconsistencymasks_amd.im_driver import DATASETS as DS
    rec = _surface()
    for path, ds in FULL.items():
        facts = rec["script_facts"][path]
        kind = DS[ds]["kind"]
        tag = {"HeLa": "HELA", "Cityscapes": "CITYSCAPES"}.get(ds, ds)
        assert facts["approach"] == ["full_dataset"], path
        assert facts["names"] == {"modelname": [tag + "_{approach}_{runid}"], "modelname_i": ["{modelname}_{i}"]}, path
        assert facts["loops"] == [["runid", 1, 4], ["i", 0, 10]], path
        assert facts["ranks"] == [list(D._RANK[kind])], path
        assert facts["headers"] == [D.csv_header(ds, full=True)], path
        train = f"{tag}_TRAIN_FULL_BRIGHTFIELD_DIR" if kind == "hela" else f"{tag}_TRAIN_FULL_IMAGES_DIR"
        assert train in facts["paths"] and not any("TRAIN_LABELED" in p for p in facts["paths"]), path
    assert D.csv_header("HeLa") == DS["HeLa"]["header"]      # the subset baseline's own header is as it was


DRY_RUN = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
from inconsistencymasks_amd import functions as F, paths, segnet_driver, subset_driver
trace = []
touch = lambda p: (os.makedirs(os.path.dirname(p), exist_ok=True), open(p, "w").close())
rel = lambda p: os.path.relpath(p, %(base)r) if isinstance(p, str) and p.startswith(%(base)r) else p
def recorder(name, result=None, makes=None):
    def call(*a, **k):
        trace.append([name] + [rel(v) if isinstance(v, str) else [rel(x) for x in v] if isinstance(v, list) else
                               v if isinstance(v, (int, float)) else type(v).__name__ for v in a] + [[q, k[q]] for q in sorted(k)])
        if makes:
            makes(*a)
        return result
    return call
class Net:
    def debug(self, **k): pass
def selected(*a):
    out = [v for v in a if isinstance(v, str) and "segnet" in v][0]
    for sub in ("images", "masks"):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
for f in ("create_training_data_evalnet_ISIC_2018", "create_training_data_evalnet_miou_multiclass"):
    setattr(F, f, recorder(f))
for f in ("create_training_data_for_segnet_ISIC_2018", "create_training_data_by_evalnet_miou_for_segnet_multiclass",
          "create_training_data_for_segnet_with_ensemble_binary", "create_training_data_for_segnet_with_miou_ensemble_multiclass"):
    setattr(F, f, recorder(f, makes=selected))
F.load_model = recorder("load_model", Net())
F.load_evalnet = recorder("load_evalnet", Net())
F.train_evalnet_ISIC_2018 = recorder("train_evalnet_ISIC_2018", (0.25, 0.125), lambda *a: touch(a[3]))
F.train_evalnet_miou_model_multiclass = recorder("train_evalnet_miou_model_multiclass", (5.0, 4.0, 3.0, 2.0, 1.0), lambda *a: touch(a[5]))
score = lambda h5: float(int(h5[-4]))      # candidate i scores i: the last one ranks first
F.train_ISIC_2018 = lambda *a: (touch(a[8]), trace.append(["train_ISIC_2018", rel(a[0]), a[7], a[10], a[11]]), (score(a[8]),) * 6)[2]
F.train_multiclass = lambda *a: (touch(a[8]), trace.append(["train_multiclass", rel(a[0]), a[7], a[10], a[11]]), (score(a[8]),) * 6)[2]
F.train_hela = lambda *a: (touch(a[6]), trace.append(["train_hela", rel(a[0]), a[5], a[8], a[9]]), (score(a[6]),) * 9)[2]
for mod in (segnet_driver, subset_driver):
    mod.get_unet = lambda *a, **k: Net()
segnet_driver.get_evalnet = recorder("get_evalnet", Net())
segnet_driver.get_evalnet_miou = recorder("get_evalnet_miou", Net())
what, ds = sys.argv[1], sys.argv[2]
tag = {"HeLa": "HELA", "Cityscapes": "CITYSCAPES"}.get(ds, ds)
P = lambda n: getattr(paths, tag + "_" + n)
if what == "single":
    for n in ("subset_1_topK_1", "subset_1_topK_2", "subset_1_7", "subset_aug_1_topK_1", "subset_2_topK_1", "model_ensemble_1_n3_gen0_topK_1"):
        touch(os.path.join(P("MODEL_DIR"), tag + "_" + n + ".h5"))
    for i in range(20):
        touch(os.path.join(P("TRAIN_LABELED_IMAGES_DIR"), "l%%d.png" %% i)); touch(os.path.join(P("TRAIN_LABELED_MASKS_DIR"), "l%%d.png" %% i))
    segnet_driver.run(ds, ensemble=False)
else:
    sub = "BRIGHTFIELD" if tag == "HELA" else "IMAGES"
    for i in range(40):
        touch(os.path.join(P("TRAIN_FULL_" + sub + "_DIR"), "f%%d.png" %% i))
    for i in range(8):
        touch(os.path.join(P("TRAIN_LABELED_" + sub + "_DIR"), "l%%d.png" %% i))
    subset_driver.run(ds, full=True)
files = sorted(os.path.relpath(os.path.join(d, f), %(base)r) for d, _, fs in os.walk(%(base)r) for f in fs if f.endswith((".h5", ".csv")))
csvs = {f: open(os.path.join(%(base)r, f), newline="").read().split("\r\n")[:-1] for f in files if f.endswith(".csv")}
print(json.dumps({"trace": trace, "files": files, "csvs": csvs}))
"""
DRY_CONFIG = """[DEFAULT]
SEED = 42
NUM_EPOCHS = 1
BATCH_SIZE = 8
BATCH_SIZE_EVALNET = 4
NUM_EPOCHS_EVALNET = 1
LR = 0.003
WD = 1e-4
THRESHOLD = 0.4375
TOP_Ks = 2
"""
DRY_SECTION = """
[{section}]
IMAGE_HEIGHT = 64
IMAGE_WIDTH = 64
IMAGE_CHANNELS = {c}
NUM_CLASSES = {k}
BASE_DIR = {base}/
ALPHA = 0.5
ALPHA_EVALNET = 0.5
ACTIFU = relu
ACTIFU_OUTPUT = sigmoid
MIN_THRESHOLD = 0.25
MAX_THRESHOLD = 0.8125
"""


def _dry_run(tmp_path, what, ds, env=()):
    base = str(tmp_path / "data")
    section = {"HeLa": "HELA", "Cityscapes": "CITYSCAPES"}.get(ds, ds)
    cfg = tmp_path / "config.ini"
    cfg.write_text(DRY_CONFIG + DRY_SECTION.format(section=section, base=base, c=1 if ds == "HeLa" else 3,
                                                   k={"ISIC_2018": 1, "HeLa": 3, "SUIM": 8, "Cityscapes": 35}[ds]))
    e = {**os.environ, "IM_CONFIG": str(cfg), "IM_PARALLEL_CANDIDATES": "1", "WORLD_SIZE": "1", **dict(env)}
    r = subprocess.run([sys.executable, "-c", DRY_RUN % {"root": ROOT, "base": base}, what, ds], env=e, capture_output=True, text=True,
                       cwd=tmp_path, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("ds", ["ISIC_2018", "SUIM"])
def test_single_evalnet_driver_dry_run(tmp_path, ds):
    out = _dry_run(tmp_path, "single", ds, {"IM_RUNIDS": "1", "IM_GENS": "0,1", "IM_CANDIDATES": "0,1,2"}.items())
    trace, files, csvs = out["trace"], out["files"], out["csvs"]
    isic = ds == "ISIC_2018"
    evalnet = f"{ds}_evalnet_1" if isic else "SUIM_evalnet_miou_1"
    seg = f"{ds}_segnet_1" if isic else "SUIM_segnet_miou_1"
    data = [t for t in trace if t[0].startswith("create_training_data_evalnet")]
    # three `subset` models of run 1 (model_i 0..2) and one `subset_aug` model (10): each writes train AND val; the aug model from TRAIN_LABELED_AUG
    shape = (lambda t: (t[5 if isic else 6], t[7 if isic else 8], t[8 if isic else 9]))
    assert [shape(t) for t in data] == [(src, f"evalnet/run_1/{split}", i) for i, lab in ((0, "train_labeled"), (1, "train_labeled"),
                                        (2, "train_labeled"), (10, "train_labeled_aug")) for src, split in ((lab + "/images", "train"), ("val/images", "val"))]
    assert len([t for t in trace if t[0] == "load_model"]) == 4
    fit = [t for t in trace if t[0].startswith("train_evalnet")]
    assert len(fit) == 1 and f"models/{evalnet}.h5" in fit[0] and "evalnet/run_1/train" in fit[0] and "evalnet/run_1/val" in fit[0]
    assert csvs[f"csv/results_{evalnet}.csv"] == (["modelname;mse;mae", f"{evalnet};0.25;0.125"] if isic else
                                                  ["modelname;mse;mae", "5.0;4.0;3.0;2.0;1.0"])
    assert f"models/{evalnet}.h5" in files and not any("topK" in f for f in files if "evalnet" in f)      # no candidates, no rename
    sel = [t for t in trace if t[0].startswith("create_training_data_for_segnet") or t[0].startswith("create_training_data_by")]
    assert [t[0] for t in sel] == ["create_training_data_for_segnet_ISIC_2018" if isic else
                                   "create_training_data_by_evalnet_miou_for_segnet_multiclass"] * 2
    dirs = lambda t: [v for v in t if isinstance(v, list) and v and isinstance(v[0], str)][0]
    assert dirs(sel[0]) == [f"train_unlabeled_predictions/subset/{ds}_subset_1_{j}" for j in range(10)]
    assert dirs(sel[1]) == [f"train_unlabeled_predictions/segnet/{seg}_gen0_{j}" for j in (0, 1, 2)]
    thr = 0.8125 if isic else 0.4375      # [ISIC_2018] MAX_THRESHOLD; [DEFAULT] THRESHOLD
    assert sel[0][-2:] == [f"train_unlabeled_predictions/segnet/{seg}_gen0", thr], sel[0]
    assert sel[1][-3:] == [f"train_unlabeled_predictions/segnet/{seg}_gen1", thr, f"train_unlabeled_predictions/segnet/{seg}_gen0"], sel[1]
    assert [t[1:] for t in trace if t[0] == "load_evalnet"] == [[f"models/{evalnet}.h5"]] * 2
    fits = [t for t in trace if t[0] in ("train_ISIC_2018", "train_multiclass")]
    assert [t[2] for t in fits] == [f"{seg}_gen{g}_{i}" for g in (0, 1) for i in (0, 1, 2)]
    assert all(t[1] == f"train_unlabeled_predictions/segnet/{seg}_gen{t[2][-3]}/images" for t in fits)
    assert all(t[3] == ("mse" if isic else "categorical_crossentropy") and t[4] == 20 // 8 for t in fits)      # the 20 labelled pairs joined
    for g in (0, 1):      # TOP_Ks = 2 of the three, ranked descending: candidates 2 and 1
        assert {f"models/{seg}_gen{g}_topK_1.h5", f"models/{seg}_gen{g}_topK_2.h5", f"models/{seg}_gen{g}_0.h5"} <= set(files)
        rows = csvs[f"csv/results_{seg}_gen{g}.csv"]
        assert rows[0].split(";")[0] == "modelname" and len(rows[0].split(";")) == 7
        assert [r.split(";")[0] for r in rows[1:]] == [f"{seg}_gen{g}_{i}" for i in (0, 1, 2)]


@pytest.mark.parametrize("ds", DATASETS)
def test_full_dataset_driver_dry_run(tmp_path, ds):
    out = _dry_run(tmp_path, "full", ds, {"IM_RUNIDS": "1,2"}.items())
    trace, files, csvs = out["trace"], out["files"], out["csvs"]
    tag = {"HeLa": "HELA", "Cityscapes": "CITYSCAPES"}.get(ds, ds)
    hela = ds == "HeLa"
    assert [t[2] for t in trace] == [f"{tag}_full_dataset_{r}_{i}" for r in (1, 2) for i in range(10)]
    assert all(t[1] == ("train_full/brightfield" if hela else "train_full/images") and t[4] == 40 // 8 for t in trace)
    for r in (1, 2):
        rows = csvs[f"csv/results_{tag}_full_dataset_{r}.csv"]
        assert len(rows) == 11 and rows[0].split(";")[:2] == ["modelname", "mIoU_val" if ds in ("ISIC_2018", "HeLa") else "mPA_val"]
        assert ("mcce_val" in rows[0]) == hela
        best = (0, 1) if hela else (9, 8)      # HeLa ranks ascending
        gone = {f"models/{tag}_full_dataset_{r}_{i}.h5" for i in best}
        assert {f"models/{tag}_full_dataset_{r}_topK_1.h5", f"models/{tag}_full_dataset_{r}_topK_2.h5"} <= set(files) and not gone & set(files)
