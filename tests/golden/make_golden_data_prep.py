#!/usr/bin/env python3
"""Golden records of the data-preparation scripts, produced by the REAL reference.

Run where a checkout of the reference is on disk (scikit-learn and tqdm installed: they run for real):

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_data_prep.py

It writes tests/golden/data_prep.npz, tests/golden/data_prep_digests.json (a sha256 per array) and
tests/golden/reference_surface_data_prep.json, which tests/test_cpu_data_prep.py and tests/test_cpu_data_prep_surface.py hold the
repository to.  IMK_GOLDEN_OUT=<dir> writes elsewhere.

The reference's nine scripts (ISIC_2018/00, 01; Cityscapes/00, 01; HeLa/00, 01; SUIM/00, 01, 02) run unmodified, each as
`__main__`, on toy trees in a temporary directory: `paths` is the reference's own module with every directory moved below that
directory, `functions` is loaded with the stub modules of make_golden_model_ensemble.py, and cv2 is a recording stub:
  imread    serves arrays by path (None for a path it was never given: the text files), 2-D under IMREAD_GRAYSCALE
  resize    records (source shape, dsize, interpolation, the source's first pixel) and returns a nearest sample
  cvtColor  BGR2RGB reverses the channels, BGR2GRAY takes channel 0 (the toy channel images are replicated grey)
  threshold numpy
  imwrite   records (path relative to the data root, array), puts an empty file there and serves the array to later imreads
os.listdir and os.walk hand out a seeded shuffle of the sorted names, and that order is recorded per directory: the order a real
file system gives is not reproducible, the order that was FED is.  The toy images of the crop cases hold their own coordinates
(pixel (y, x) = [y, x, 7]), so the first pixel of what reaches cv2.resize is the crop's (y, x) draw.

Recorded (data only, nothing of the reference's text):
  <script key>_listing_<i> / _listed_<i>   directories listed (relative) and the names handed out, in call order
  <script key>_written                      relative paths in imwrite order;   _copied: shutil.copy destinations (HeLa 01)
  <script key>_resize                       int64 [calls, 8]: source h, w, channels, dsize w, h, interpolation, first pixel y, x
  city00_mask_<name>_in / _out              the label map's nearest sample [dh, dw] and the mask as written [dh, dw, 3]: np.where(m > 0, m + 1, m)
  suim00_<name>_<folder>_in / _out          the colour mask as cv2.imread served it and the class mask as written
  positions_<h>_<w>_<crop>_<overlap%>       ImagePreprocessor.get_positions tables, int64 [n, 2]
  split_<n>_<test_size%>_<seed>_test        train_test_split(list(range(n)), ...)'s test part, int64;  _train the other part
  split_errors                              int64 [k, 3]: (n, test_size %, seed) where scikit-learn raised ValueError
  crop<i>_seed / _shape / _draw             random_crop under random.seed(s); np.random.seed(s): image shape and the recorded
                                            (y, x, crop size) of the image's (and the mask's) resize, or (-1, -1, -1) where the whole image was resized
reference_surface_data_prep.json: the nine scripts, the names they take from `functions`, `paths` and the class-mapping module
(tools/dump_reference_surface.py's reading of their syntax trees), the signatures and defaults of the functions and methods they
define, the config keys they read, and the value of every `*_ORG_*` constant relative to its BASE_DIR."""
import inspect
import json
import os
import random
import runpy
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_model_ensemble import REF, array_digest, load_reference  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
NAME = "data_prep"
SCRIPTS = [("isic00", "ISIC_2018/00_ISIC_2018_preprocess_images.py"), ("isic01", "ISIC_2018/01_ISIC_2018_split_original_train.py"),
           ("city00", "Cityscapes/00_Cityscapes_resize_images_and_masks.py"), ("city01", "Cityscapes/01_Cityscapes_split_original_train_val.py"),
           ("hela00", "HeLa/00_HeLa_create_crops.py"), ("hela01", "HeLa/01_HeLa_split_train_in_labeled_and_unlabeled.py"),
           ("suim00", "SUIM/00_SUIM_convert_bmp_to_png_masks.py"), ("suim01", "SUIM/01_SUIM_split_original_train_val.py"),
           ("suim02", "SUIM/02_SUIM_create_crops.py")]
DEFINED = {"isic00": ["preprocess_data"], "isic01": ["split_and_resize_dataset"], "city00": ["resize_image", "process_images"],
           "city01": ["split_and_resize_dataset"], "hela00": ["ImagePreprocessor"], "hela01": [],
           "suim00": ["convert_color_bmp_to_class_mask_png", "convert_all_masks_in_folder"], "suim01": ["split_and_resize_dataset"],
           "suim02": ["random_crop", "create_random_crops"]}
POSITION_CASES = [(300, 400, 256, 0.6), (512, 512, 256, 0.6), (1024, 1360, 256, 0.6), (256, 256, 256, 0.6), (600, 700, 256, 0.6),
                  (64, 96, 48, 0.6), (300, 400, 128, 0.5), (257, 1000, 256, 0.0)]
SPLIT_NS = (10, 11, 37, 100, 2594)
SPLIT_ARGS = ((0.9, 42), (0.1, 42), (0.5, 7), (0.9, 0))
INTER_NEAREST, INTER_LINEAR = 0, 1


def _norm(p):
    return os.path.normpath(os.path.abspath(p))


def coord_image(h, w):
    """pixel (y, x) = [y, x, 7]: a crop names its own origin"""
    a = np.zeros((h, w, 3), np.int32)
    a[..., 0], a[..., 1], a[..., 2] = np.arange(h)[:, None], np.arange(w)[None, :], 7
    return a


class Recorder:
    def __init__(self, root):
        self.root = _norm(root)
        self.images = {}
        self.reset()

    def reset(self):
        self.written, self.resized, self.listings, self.copied = [], [], [], []

    def rel(self, p):
        return os.path.relpath(_norm(p), self.root).replace(os.sep, "/")

    def put(self, path, arr):
        """a file the scripts can read: an empty placeholder on disk, the array behind cv2.imread"""
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "wb").close()
        if arr is not None:
            self.images[_norm(path)] = np.array(arr)

    def order(self, path, names):
        names = sorted(names)
        rng = random.Random("listing|" + self.rel(path))
        rng.shuffle(names)
        return names

    def install(self):
        cv2 = sys.modules["cv2"]
        cv2.INTER_NEAREST, cv2.INTER_LINEAR = INTER_NEAREST, INTER_LINEAR
        cv2.COLOR_BGR2GRAY, cv2.COLOR_BGR2RGB, cv2.THRESH_BINARY, cv2.IMREAD_GRAYSCALE = 6, 4, 0, 0

        def imread(path, flag=1):
            a = self.images.get(_norm(path))
            if a is None:
                return None
            a = a.copy()
            return (a[..., 0] if a.ndim == 3 else a) if flag == cv2.IMREAD_GRAYSCALE else (a if a.ndim == 3 else np.repeat(a[..., None], 3, 2))

        def resize(a, dsize, interpolation=INTER_LINEAR):
            dw, dh = int(dsize[0]), int(dsize[1])
            first = a[0, 0] if a.ndim == 2 else a[0, 0, :2]
            y, x = (int(first[0]), int(first[1])) if a.ndim == 3 else (int(first), -1)
            self.resized.append([a.shape[0], a.shape[1], 1 if a.ndim == 2 else a.shape[2], dw, dh, int(interpolation), y, x])
            return np.ascontiguousarray(a[np.arange(dh) * a.shape[0] // dh][:, np.arange(dw) * a.shape[1] // dw])

        def cvt(a, code):
            return np.ascontiguousarray(a[..., 0] if code == cv2.COLOR_BGR2GRAY else a[..., ::-1])

        def imwrite(path, arr):
            self.written.append((self.rel(path), np.array(arr)))
            self.put(path, arr)
            return True

        cv2.imread, cv2.resize, cv2.cvtColor, cv2.imwrite = imread, resize, cvt, imwrite
        cv2.threshold = lambda a, thr, maxval, kind: (thr, np.where(a > thr, maxval, 0).astype(np.uint8))
        real_listdir, real_walk, real_copy = os.listdir, os.walk, shutil.copy

        def listdir(path="."):
            names = real_listdir(path)
            if not _norm(path).startswith(self.root):
                return names
            names = self.order(path, names)
            self.listings.append((self.rel(path), list(names)))      # a copy: HeLa/01 shuffles what it was handed
            return names

        def walk(top, *a, **k):
            for root, dirs, files in real_walk(top, *a, **k):
                dirs.sort()
                files = self.order(root, files)
                self.listings.append((self.rel(root), list(files)))
                yield root, dirs, files

        def copy(src, dst, *a, **k):
            self.copied.append(self.rel(dst))
            return real_copy(src, dst, *a, **k)

        os.listdir, os.walk, shutil.copy = listdir, walk, copy
        return lambda: (setattr(os, "listdir", real_listdir), setattr(os, "walk", real_walk), setattr(shutil, "copy", real_copy))


def make_paths(root):
    """the reference's paths module, every directory moved from its BASE_DIR to `root`/<dataset>; also the *_ORG_* table"""
    import importlib.util
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        spec = importlib.util.spec_from_file_location("paths", os.path.join(REF, "paths.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        os.chdir(cwd)
    org = {}
    for ds in ("ISIC_2018", "HELA", "SUIM", "CITYSCAPES"):
        base = getattr(m, f"{ds}_BASE_DIR")
        for k, v in list(vars(m).items()):
            if k.startswith(ds + "_") and isinstance(v, str) and k.isupper():
                rel = os.path.relpath(v, base).replace(os.sep, "/")
                if "_ORG_" in k:
                    org[k] = rel
                setattr(m, k, os.path.normpath(os.path.join(root, ds, rel)))
    sys.modules["paths"] = m
    return m, org


def make_trees(r, P, rng):
    u8 = lambda *s: rng.integers(0, 256, s, dtype=np.uint8)
    for d_i, d_m, n, k0 in ((P.ISIC_2018_ORG_TRAIN_IMAGES_DIR, P.ISIC_2018_ORG_TRAIN_MASKS_DIR, 12, 0),
                            (P.ISIC_2018_ORG_VAL_IMAGES_DIR, P.ISIC_2018_ORG_VAL_MASKS_DIR, 3, 12),
                            (P.ISIC_2018_ORG_TEST_IMAGES_DIR, P.ISIC_2018_ORG_TEST_MASKS_DIR, 3, 15)):
        for i in range(k0, k0 + n):
            h, w = 9 + i % 4, 12 + i % 5
            r.put(os.path.join(d_i, f"ISIC_{i:07d}.jpg"), u8(h, w, 3))
            r.put(os.path.join(d_m, f"ISIC_{i:07d}_segmentation.png"), u8(h, w))
        r.put(os.path.join(d_i, "ATTRIBUTION.txt"), None)
        r.put(os.path.join(d_m, "LICENSE.txt"), None)
    for d_i, d_m, cities in ((P.CITYSCAPES_ORG_TRAIN_IMAGES_DIR, P.CITYSCAPES_ORG_TRAIN_MASKS_DIR, (("aachen", 6), ("bochum", 5))),
                             (P.CITYSCAPES_ORG_VAL_IMAGES_DIR, P.CITYSCAPES_ORG_VAL_MASKS_DIR, (("lindau", 2), ("munster", 2)))):
        for city, n in cities:
            for i in range(n):
                common = f"{city}_{i:06d}_000019"
                r.put(os.path.join(d_i, city, common + "_leftImg8bit.png"), u8(1024 // 8, 2048 // 8, 3))
                lab = np.array([0, 1, 7, 33, 254, 255], np.uint8)[rng.integers(0, 6, (128, 256))]
                r.put(os.path.join(d_m, city, common + "_gtFine_labelIds.png"), lab)
                r.put(os.path.join(d_m, city, common + "_gtFine_color.png"), u8(128, 256, 3))
            r.put(os.path.join(d_i, city, "README.txt"), None)
        r.put(os.path.join(d_i, cities[0][0], f"{cities[0][0]}_000099_000019_leftImg8bit.png"), u8(128, 256, 3))      # no label file
    for data_set, n in (("train_full", 4), ("val", 1), ("test", 1)):
        for i in range(n):
            name = f"{data_set}_{i:03d}.png"
            r.put(os.path.join(P.HELA_ORG_DIR, data_set, "brightfield", name), u8(300, 400))
            for channel in ("alive", "dead", "mod_position", "position"):
                if (channel, data_set, i) != ("dead", "train_full", 2):
                    r.put(os.path.join(P.HELA_ORG_DIR, data_set, channel, name), np.array([0, 9, 10, 11, 255], np.uint8)[rng.integers(0, 5, (300, 400))])
    colours = np.array([0, 120, 130, 255], np.uint8)
    for d_i, d_m, n, tag in ((P.SUIM_ORG_TRAIN_VAL_IMAGES_DIR, P.SUIM_ORG_TRAIN_VAL_MASKS_BMP_DIR, 12, "f"),
                             (P.SUIM_ORG_TEST_IMAGES_DIR, P.SUIM_ORG_TEST_MASKS_BMP_PATH, 3, "d")):
        for i in range(n):
            h, w = [(300, 400), (270, 300), (200, 260), (480, 640)][i % 4]
            r.put(os.path.join(d_i, f"{tag}_r_{i:03d}_.jpg"), coord_image(h, w))
            blocks = colours[rng.integers(0, 4, (6, 8, 3))]      # blocks of one colour: full size on disk, small in the fixture
            r.put(os.path.join(d_m, f"{tag}_r_{i:03d}_.bmp"), blocks.repeat(-(-h // 6), 0).repeat(-(-w // 8), 1)[:h, :w])
        r.put(os.path.join(d_m, "notes.txt"), None)


def run_scripts(r, rec):
    """the nine scripts in workflow order; returns {key: the globals the script left}"""
    left = {}
    for key, rel in SCRIPTS:
        r.reset()
        random.seed(1234)
        np.random.seed(1234)
        argv, path = sys.argv, list(sys.path)
        sys.argv = [os.path.join(REF, rel)]
        sys.path.insert(0, os.path.dirname(os.path.join(REF, rel)))       # a script's own directory (SUIM_class_mapping)
        try:
            left[key] = runpy.run_path(os.path.join(REF, rel), run_name="__main__")
        finally:
            sys.argv, sys.path[:] = argv, path
        for i, (d, names) in enumerate(r.listings):
            rec[f"{key}_listing_{i}"], rec[f"{key}_listed_{i}"] = np.array(d), np.array(names if names else [""])
        rec[key + "_written"] = np.array([p for p, _ in r.written] or [""])
        rec[key + "_resize"] = np.array(r.resized, np.int64).reshape(-1, 8)
        if r.copied:
            rec[key + "_copied"] = np.array(r.copied)
        if key == "city00":
            for p, arr in r.written:
                if "/masks/" in "/" + p:
                    common = os.path.basename(p)[:-4]
                    src = [a for q, a in r.images.items() if q.endswith(common + "_gtFine_labelIds.png")][0]
                    dh, dw = arr.shape[:2]
                    rec[f"city00_mask_{common}_in"] = src[np.arange(dh) * src.shape[0] // dh][:, np.arange(dw) * src.shape[1] // dw]
                    rec[f"city00_mask_{common}_out"] = arr
        if key == "suim00":
            for p, arr in r.written:
                src = os.path.join(r.root, os.path.dirname(os.path.dirname(p)), "masks", os.path.basename(p)[:-4] + ".bmp")
                rec[f"suim00_{os.path.basename(p)[:-4]}_{p.split('/')[-3]}_in"] = r.images[_norm(src)]
                rec[f"suim00_{os.path.basename(p)[:-4]}_{p.split('/')[-3]}_out"] = arr
    return left


def function_cases(r, left, rec):
    pre = left["hela00"]["ImagePreprocessor"]
    for h, w, crop, overlap in POSITION_CASES:
        rec[f"positions_{h}_{w}_{crop}_{int(round(overlap * 100))}"] = np.array(pre("/in", "/out", crop, overlap).get_positions(h, w), np.int64).reshape(-1, 2)
    from sklearn.model_selection import train_test_split
    errors = []
    for n in list(range(1, 13)) + list(SPLIT_NS):
        for ts, seed in SPLIT_ARGS:
            try:
                a, b = train_test_split(list(range(n)), test_size=ts, random_state=seed)
            except ValueError:
                errors.append([n, int(round(ts * 100)), seed])
                continue
            rec[f"split_{n}_{int(round(ts * 100))}_{seed}_train"], rec[f"split_{n}_{int(round(ts * 100))}_{seed}_test"] = np.array(a, np.int64), np.array(b, np.int64)
    rec["split_errors"] = np.array(errors, np.int64).reshape(-1, 3)
    random_crop = left["suim02"]["random_crop"]
    for i, (h, w) in enumerate([(300, 400), (480, 640), (270, 300), (257, 257), (600, 258), (1000, 1000)]):
        seed = 9000 + i
        r.reset()
        random.seed(seed)
        np.random.seed(seed)
        random_crop(coord_image(h, w), coord_image(h, w)[..., 0])
        (ih, iw, _, _, _, ii, iy, ix), (mh, mw, _, _, _, mi, my, _) = r.resized
        assert (ii, mi) == (INTER_LINEAR, INTER_NEAREST) and (ih, iw) == (mh, mw) and iy == my
        whole = (ih, iw) == (h, w)
        rec[f"crop{i}_seed"], rec[f"crop{i}_shape"] = np.int64(seed), np.array([h, w], np.int64)
        rec[f"crop{i}_draw"] = np.array([-1, -1, -1] if whole else [iy, ix, ih], np.int64)


def surface(left, org):
    import ast
    import dump_reference_surface as D
    rels = [rel for _, rel in SCRIPTS]
    sig = {}
    for key, rel in SCRIPTS:
        for name in DEFINED[key]:
            obj = left[key][name]
            fns = {name: obj} if not inspect.isclass(obj) else {f"{name}.{m}": f for m, f in vars(obj).items() if inspect.isfunction(f)}
            for n, f in fns.items():
                sig.setdefault(rel, {})[n] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                                              for p in inspect.signature(f).parameters.values()]
    keys = {}
    for rel in rels:
        tree = ast.parse(open(os.path.join(REF, rel), encoding="utf-8", errors="replace").read())
        found = set()
        for n in ast.walk(tree):      # config['SECTION']['KEY']
            if isinstance(n, ast.Subscript) and isinstance(n.value, ast.Subscript) and getattr(n.value.value, "id", None) == "config":
                found.add(f"{ast.literal_eval(n.value.slice)}.{ast.literal_eval(n.slice)}")
        keys[rel] = sorted(found)
    import configparser
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(REF, "config.ini"))
    values = {k: cfg[k.split(".")[0]][k.split(".")[1]] for ks in keys.values() for k in ks if k.split(".")[1] in ("RESIZE_FACTOR", "USE_MOD_POS_SIZE")}
    return {"scripts": rels, "wanted": D.wanted_names(REF, rels), "signatures": sig, "config_keys": keys, "config_values": values,
            "org_paths": dict(sorted(org.items()))}


def main():
    ref = load_reference()      # `from functions import get_pos_contours, get_min_dist` (HeLa/00) finds it in sys.modules
    assert "functions" in sys.modules and ref is sys.modules["functions"]
    root = tempfile.mkdtemp(prefix="imk_prep_golden_")
    rec = {}
    try:
        P, org = make_paths(root)
        r = Recorder(root)
        undo = r.install()
        try:
            make_trees(r, P, np.random.default_rng(20261019))
            left = run_scripts(r, rec)
            function_cases(r, left, rec)
        finally:
            undo()
        surf = surface(left, org)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME + ".npz"), **rec)
    with np.load(os.path.join(OUT, NAME + ".npz")) as d:
        dig = {NAME: {key: array_digest(d[key]) for key in sorted(d.files)}}
    with open(os.path.join(OUT, NAME + "_digests.json"), "w") as f:
        json.dump(dig, f, indent=1, sort_keys=True)
        f.write("\n")
    with open(os.path.join(OUT, "reference_surface_" + NAME + ".json"), "w") as f:
        json.dump(surf, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(rec)} arrays to {os.path.join(OUT, NAME + '.npz')}")


if __name__ == "__main__":
    main()
