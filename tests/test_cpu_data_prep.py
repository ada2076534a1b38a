"""The pins of the data-preparation rules: tests/golden/make_golden_data_prep.py runs the REAL reference's nine scripts and their
functions on toy trees with a recording cv2 and real scikit-learn, and records a sha256 of every array in
tests/golden/data_prep_digests.json.  The committed fixture must be exactly what that regeneration recorded; with a reference checkout on
disk (IMK_REFERENCE) it is regenerated into a temporary directory and compared.  Against the records: get_positions tables, split
memberships and ValueError cases, output names and skip rules in the order the listings were fed, the requested sizes and flags,
random_crop's draws under the recorded seeds, the + 1 label rule and the SUIM class masks -- for inconsistencymasks_amd.prep's host
rules and for the numpy restatement (tests/prep_cases.py) the GPU tests compare the kernels with.  Last, the second opinion on the
linear rule: the fixed-point restatement stays strictly below one grey level from a float64 bilinear."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import prep_cases as pc  # noqa: E402
from test_golden_regenerate import array_digest  # noqa: E402

SUIM_MAPPING = {(211, 211, 211): 0, **{(255 * (k >> 2 & 1), 255 * (k >> 1 & 1), 255 * (k & 1)): k + 1 for k in range(8)}}


@pytest.fixture(scope="module")
def rec():
    with np.load(os.path.join(GOLD, "data_prep.npz")) as d:
        return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def prep():
    from inconsistencymasks_amd import prep as p
    return p


def _listings(rec, key):
    out, i = [], 0
    while f"{key}_listing_{i}" in rec:
        names = [str(n) for n in rec[f"{key}_listed_{i}"]]
        out.append((str(rec[f"{key}_listing_{i}"]), [n for n in names if n]))
        i += 1
    return out


def _written(rec, key):
    return [str(p) for p in rec[key + "_written"] if str(p)]


def test_fixture_equals_what_the_regeneration_recorded(rec):
    with open(os.path.join(GOLD, "data_prep_digests.json")) as f:
        want = json.load(f)["data_prep"]
    assert sorted(rec) == sorted(want)
    for k, v in rec.items():
        assert array_digest(v) == want[k], k


@pytest.mark.skipif(not os.environ.get("IMK_REFERENCE"), reason="needs a reference checkout (IMK_REFERENCE)")
def test_fixture_regenerates(tmp_path):
    env = dict(os.environ, IMK_GOLDEN_OUT=str(tmp_path))
    subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_data_prep.py")], env=env, check=True, capture_output=True)
    for name in ("data_prep_digests.json", "reference_surface_data_prep.json"):
        with open(tmp_path / name) as f, open(os.path.join(GOLD, name)) as g:
            assert json.load(f) == json.load(g), name


def test_get_positions_tables(rec, prep):
    keys = [k for k in rec if k.startswith("positions_")]
    assert len(keys) == 8
    bites = 0
    for k in keys:
        h, w, crop, ov = (int(v) for v in k.split("_")[1:])
        want = [tuple(p) for p in rec[k].tolist()]
        assert prep.ImagePreprocessor("/in", "/out", crop, ov / 100).get_positions(h, w) == want, k
        assert pc.get_positions(h, w, crop, ov / 100) == want, k
        bites += any(x == w - crop and x != int(i * (w / round(w / (crop * (1 - ov / 100)))))
                     for i, x in enumerate(sorted({p[0] for p in want})))
    assert bites                                                    # a table where min(x, W - crop) decides


def test_split_restatement_equals_the_recorded_memberships(rec, prep):
    n_cases = 0
    for k in [k for k in rec if k.startswith("split_") and k.endswith("_test")]:
        n, ts, seed = (int(v) for v in k.split("_")[1:4])
        for split in (prep.train_test_split, pc.split):
            train, test = split(list(range(n)), ts / 100, seed)
            assert train == rec[k[:-5] + "_train"].tolist() and test == rec[k].tolist(), (k, split.__module__)
        n_cases += 1
    errors = [tuple(e) for e in rec["split_errors"].tolist()]
    assert n_cases + len(errors) == 15 * 4 and {(n, 90, 42) for n in range(1, 10)} <= set(errors) and (10, 90, 42) not in errors
    for n, ts, seed in errors:
        for split in (prep.train_test_split, pc.split):
            with pytest.raises(ValueError):
                split(list(range(n)), ts / 100, seed)


def test_size_rules(rec, prep):
    assert prep.cityscapes_size(1024, 2048, 0.2) == (208, 416) == pc.cityscapes_size(1024, 2048, 0.2)      # 2048 x 1024 -> 416 x 208
    rows = rec["city00_resize"]
    assert len(rows) == 30
    for i, (h, w, c, dw, dh, interp, _, _) in enumerate(rows.tolist()):
        assert (dh, dw) == prep.cityscapes_size(h, w, 0.2) and interp == (1 if i % 2 == 0 else 0) and c == 3      # image linear, mask nearest
    for h, w, c, dw, dh, interp, _, _ in rec["isic00_resize"].tolist():
        assert (dw, dh, interp, c) == (256, 256, 1, 3)                                                         # masks too: no flag


def test_isic_names_in_the_order_the_listings_were_fed(rec, prep):
    want = _written(rec, "isic00")
    got = []
    for d, names in _listings(rec, "isic00"):
        is_mask = "GroundTruth" in d
        out = {"Training": "train_full", "Validation": "val", "Test": "test"}[d.split("_")[-2]]
        got += [f"ISIC_2018/{out}/{'masks' if is_mask else 'images'}/{prep.isic_out_name(n, is_mask)}" for n in names if not n.endswith(".txt")]
    assert got == want and len(want) == 36
    assert prep.isic_out_name("ISIC_0000008_segmentation.png", True) == "ISIC_0000008.png" == prep.isic_out_name("ISIC_0000008.jpg")


def test_cityscapes_names_and_skip_rule(rec, prep, tmp_path):
    listings = _listings(rec, "city00")
    for d, names in listings:
        for n in names:
            os.makedirs(tmp_path / d, exist_ok=True)
            (tmp_path / d / n).touch()
            if n.endswith("_leftImg8bit.png") and "000099" not in n:      # the generator's one image without a label file
                m = tmp_path / d.replace("leftImg8bit", "gtFine")
                os.makedirs(m, exist_ok=True)
                (m / n.replace("_leftImg8bit.png", "_gtFine_labelIds.png")).touch()
    org = tmp_path / "CITYSCAPES" / "original_data"
    for split, out in (("train", "CITYSCAPES/train_full"), ("val", "CITYSCAPES/original_data/val_test")):
        pairs = prep.cityscapes_pairs(str(org / "leftImg8bit" / split), str(org / "gtFine" / split))
        want = [p for p in _written(rec, "city00") if p.startswith(out + "/images/")]
        assert sorted(f"{out}/images/{c}.png" for _, _, c in pairs) == sorted(want)
        assert all(os.path.basename(os.path.dirname(i)) == os.path.basename(os.path.dirname(m)) for i, m, _ in pairs)      # the city
        assert not any("000099" in c for _, _, c in pairs)
    w = _written(rec, "city00")
    assert all(w[i].replace("/images/", "/masks/") == w[i + 1] for i in range(0, len(w), 2))


def test_hela_crop_names_in_listing_order(rec, prep):
    """HeLa/00: per brightfield file in the order listed, per position, per channel whose file exists: `{stem}_{count}.png`; the
    generator's train_full_002 has no `dead` file and gets no `dead` crops"""
    pre = prep.ImagePreprocessor("/in", "/out", 256, 0.6, use_mod_pos_size=True)
    assert pre.channels == ["brightfield", "alive", "dead", "mod_position"]
    n_pos = len(pre.get_positions(300, 400))
    got = []
    for d, names in _listings(rec, "hela00"):
        data_set = d.split("/")[-2]
        for name in names:
            for count in range(n_pos):
                got += [f"HELA/{data_set}/{ch}/{prep.hela_crop_name(name, count)}" for ch in pre.channels
                        if not (ch == "dead" and name == "train_full_002.png")]
    want = _written(rec, "hela00")
    assert got == want and len(want) == n_pos * (6 * 4 - 1)
    assert not any("/position/" in p for p in want)                      # USE_MOD_POS_SIZE = True: `mod_position`, never `position`


def test_suim_mask_names_in_listing_order(rec, prep):
    """SUIM/00: every `.bmp` of the listing, in its order, as `masks_png/{stem}.png`; other files are passed over"""
    got, seen_other = [], 0
    for d, names in _listings(rec, "suim00"):
        out = d[:-len("masks")] + "masks_png"
        got += [f"{out}/{prep.suim_mask_png_name(n)}" for n in names if n.endswith(".bmp")]
        seen_other += sum(not n.endswith(".bmp") for n in names)
    assert got == _written(rec, "suim00") and len(got) == 15 and seen_other == 2      # a notes.txt in each of the two folders


def test_script_splits_follow_the_listing(rec, prep):
    for key, cases in (("isic01", [("ISIC_2018", ("train_labeled", "train_unlabeled"), 0.9, ".png", ".png")]),
                       ("city01", [("CITYSCAPES", ("train_labeled", "train_unlabeled"), 0.9, ".png", ".png"),
                                   ("CITYSCAPES", ("val", "test"), 0.5, ".png", ".png")]),
                       ("suim01", [("SUIM/original_data", ("train_full", "val"), 0.1, ".jpg", ".png"),
                                   ("SUIM/original_data", ("train_unlabeled", "train_labeled"), 0.1, ".jpg", ".png")])):
        listings = _listings(rec, key)
        want, got = _written(rec, key), []
        for i, (base, subsets, ratio, iext, mext) in enumerate(cases):
            names = listings[2 * i][1]                                   # images_dir is listed first, masks_dir second
            items = [os.path.splitext(n)[0] for n in names] if key == "suim01" else names
            parts = prep.train_test_split(items, ratio, 42)
            for subset, part in zip(subsets, parts):
                for f in part:
                    stem = f if key == "suim01" else f[:-4]
                    got += [f"{base}/{subset}/images/{stem}{iext}", f"{base}/{subset}/masks/{stem}{mext}"]
        assert got == want, key


def test_hela_split_follows_the_listing(rec, prep, tmp_path, monkeypatch):
    (d, names), = _listings(rec, "hela01")
    copied = [str(p) for p in rec["hela01_copied"]]
    root = tmp_path / "train_full"
    for p in copied:
        folder, name = p.split("/")[-2:]
        os.makedirs(root / folder, exist_ok=True)
        (root / folder / name).touch()
    real = os.listdir
    monkeypatch.setattr(prep.os, "listdir", lambda p: list(names) if str(p).endswith("brightfield") else real(p))
    lab, unl = prep.hela_split(str(root), str(tmp_path / "train_labeled"), str(tmp_path / "train_unlabeled"), True, 42)
    monkeypatch.undo()
    assert len(lab) == int(len(names) * 0.10)
    bf = [p for p in copied if "/brightfield/" in p]
    assert [os.path.basename(p) for p in bf if "/train_labeled/" in p] == lab
    assert [os.path.basename(p) for p in bf if "/train_unlabeled/" in p] == unl
    for split in ("train_labeled", "train_unlabeled"):
        for folder in ("brightfield", "alive", "dead", "mod_position"):
            assert sorted(os.listdir(tmp_path / split / folder)) == sorted(os.path.basename(p) for p in copied if f"/{split}/{folder}/" in p)


def _draw(prep, h, w):
    r = prep._draw_crop(h, w, 256, 512, random, np.random)
    return [-1, -1, -1] if r is None else [r[1], r[0], r[2]]


def test_random_crop_draws_under_the_recorded_seeds(rec, prep):
    """np.random.randint for the size, then random.randint for x, then for y, on the global generators"""
    whole = 0
    for i in range(6):
        seed, (h, w) = int(rec[f"crop{i}_seed"]), rec[f"crop{i}_shape"].tolist()
        random.seed(seed)
        np.random.seed(seed)
        assert _draw(prep, h, w) == rec[f"crop{i}_draw"].tolist(), i
        whole += rec[f"crop{i}_draw"][0] < 0
    assert 0 < whole < 6
    # the whole script: one stream of draws over five directories, two crops per `.jpg` in listing order (seeded once, 1234)
    sizes = [(300, 400), (270, 300), (200, 260), (480, 640)]
    rows = rec["suim02_resize"].tolist()
    random.seed(1234)
    np.random.seed(1234)
    k = 0
    for d, names in _listings(rec, "suim02"):
        for n in names:
            if not n.endswith(".jpg"):
                continue
            h, w = sizes[int(n.split("_")[2]) % 4]
            for j in range(2):
                y, x, size = _draw(prep, h, w)
                img, mask = rows[k], rows[k + 1]
                assert img[:6] == [h if size < 0 else size, w if size < 0 else size, 3, 256, 256, 1] and img[6:] == [max(y, 0), max(x, 0)], (n, j)
                assert mask[:6] == img[:2] + [1, 256, 256, 0]
                k += 2
    assert k == len(rows) == 100
    w = _written(rec, "suim02")
    assert all(a.replace("/images/", "/masks/") == b for a, b in zip(w[0::2], w[1::2]))
    (d0, names0) = _listings(rec, "suim02")[0]
    jpgs = [n for n in names0 if n.endswith(".jpg")]
    assert w[:4:2] == [f"SUIM/train_full/images/{jpgs[0][:-4]}_0_{j}.png" for j in range(2)]      # {stem}_{i}_{j}: i indexes the listing


def test_label_plus1_masks(rec):
    keys = [k for k in rec if k.startswith("city00_mask_") and k.endswith("_in")]
    assert len(keys) == 15
    seen = set()
    for k in keys:
        m, out = rec[k], rec[k[:-3] + "_out"]
        assert out.dtype == np.uint8 and out.shape == m.shape + (3,)
        assert np.array_equal(out, np.repeat(pc.label_plus1(m)[..., None], 3, 2)), k
        seen |= set(np.unique(m).tolist())
    assert {0, 1, 33, 254, 255} <= seen
    assert pc.label_plus1(np.array([0, 1, 33, 254, 255], np.uint8)).tolist() == [0, 2, 34, 255, 0]


def test_suim_class_masks(rec, prep):
    table = pc.class_table({k: v for k, v in SUIM_MAPPING.items() if k != (211, 211, 211)})
    assert np.array_equal(prep.class_table(SUIM_MAPPING), table) and table.tolist() == list(range(1, 9))
    from inconsistencymasks_amd.im_driver import color_mapping
    assert color_mapping("SUIM", 9) == SUIM_MAPPING
    keys = [k for k in rec if k.startswith("suim00_") and k.endswith("_in")]
    assert len(keys) == 15
    for k in keys:
        bgr, out = rec[k], rec[k[:-3] + "_out"]
        assert np.array_equal(out, pc.class8(bgr, table, b_first=True)), k
        assert {120, 130} <= set(np.unique(bgr).tolist())                 # values on both sides of 128 that are no palette colour
    assert np.array_equal(pc.class8(np.array([[[0, 127, 128]]], np.uint8), prep.class_table({(0, 0, 255): 7})), [[7]])      # absent -> 0 elsewhere
    assert pc.class8(np.array([[[255, 255, 255]]], np.uint8), prep.class_table({(0, 0, 255): 7})).tolist() == [[0]]


@pytest.mark.parametrize("c", [1, 3])
def test_linear_rule_second_opinion(c):
    """every pixel of every size pair within one grey level of the float64 half-pixel bilinear; equal sizes come out as they went in"""
    for i, (src, dst) in enumerate(pc.SECOND_OPINION_SIZES):
        a = pc.noise(40 + i, src[0], src[1], c)
        fixed = pc.resize_linear(a, dst[0], dst[1])
        worst = float(np.abs(fixed.astype(np.float64) - pc.resize_float(a, dst[0], dst[1])).max())
        assert worst < 1.0, (src, dst, worst)
        if src == dst:
            assert np.array_equal(fixed, a)
