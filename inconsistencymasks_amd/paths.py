"""Directory constants with the reference's names (paths.py:10-201), generated from BASE_DIR in config.ini by the rule
the reference's table follows: `{DATASET}_{SPLIT}[_MAIN]_DIR = BASE_DIR/{split}` and below it `images` / `masks`
(HeLa: `brightfield` / `alive` / `dead` / `pos` / `mod_position`), plus `models` and `csv`.  Every processed-dataset
constant of the reference exists here with the same value, and so does every `*_ORG_*` constant of the dataset-preparation
scripts (paths.py:12-17, 44-64, 116-132, 167-173): the downloads live under `BASE_DIR/original_data`."""
import configparser
import os

config = configparser.ConfigParser()
config.read(os.environ.get("IM_CONFIG", "config.ini"))

_SPLITS = ("TRAIN_FULL", "TRAIN_LABELED", "TRAIN_LABELED_AUG", "TRAIN_UNLABELED", "VAL", "TEST")
_HELA_SUBS = (("BRIGHTFIELD", "brightfield"), ("ALIVE", "alive"), ("DEAD", "dead"), ("POS", "pos"),
              ("MOD_POS", "mod_position"))


def _dataset(prefix, section):
    if section not in config:
        return
    base = config[section]["BASE_DIR"]
    g = globals()
    g[f"{prefix}_BASE_DIR"] = base
    for split in _SPLITS:
        d = os.path.join(base, split.lower())
        g[f"{prefix}_{split}_DIR"] = d
        g[f"{prefix}_{split}_MAIN_DIR"] = d
        if prefix == "HELA":
            for name, sub in _HELA_SUBS:
                g[f"{prefix}_{split}_{name}_DIR"] = os.path.join(d, sub)
        else:
            g[f"{prefix}_{split}_IMAGES_DIR"] = os.path.join(d, "images")
            g[f"{prefix}_{split}_MASKS_DIR"] = os.path.join(d, "masks")
    g[f"{prefix}_MODEL_DIR"] = os.path.join(base, "models")
    g[f"{prefix}_CSV_DIR"] = os.path.join(base, "csv")
    _original(prefix, base, g)


def _original(prefix, base, g):
    """the raw trees the 00_* / 01_* / SUIM 02_* scripts read, with the reference's (irregular) names"""
    org = os.path.join(base, "original_data")
    if prefix == "ISIC_2018":
        for split, folder in (("TRAIN", "Training"), ("VAL", "Validation"), ("TEST", "Test")):
            g[f"{prefix}_ORG_{split}_IMAGES_DIR"] = os.path.join(org, f"ISIC2018_Task1-2_{folder}_Input")
            g[f"{prefix}_ORG_{split}_MASKS_DIR"] = os.path.join(org, f"ISIC2018_Task1_{folder}_GroundTruth")
    elif prefix == "HELA":
        g["HELA_ORG_DIR"] = org
        for split in ("TRAIN", "VAL", "TEST"):
            d = g[f"HELA_ORG_{split}_DIR"] = os.path.join(org, split.lower())
            for name, sub in _HELA_SUBS:
                g[f"HELA_ORG_{split}_{name}_DIR"] = os.path.join(d, sub)
    elif prefix == "SUIM":
        g["SUIM_ORG_DATA_DIR"] = org
        for split in ("TRAIN_FULL", "TRAIN_LABELED", "TRAIN_UNLABELED", "VAL"):
            g[f"SUIM_ORG_{split}_IMAGES_DIR"] = os.path.join(org, split.lower(), "images")
            g[f"SUIM_ORG_{split}_MASKS_DIR"] = os.path.join(org, split.lower(), "masks")
        g["SUIM_ORG_TRAIN_VAL_IMAGES_DIR"] = os.path.join(org, "train_val", "images")
        g["SUIM_ORG_TRAIN_VAL_MASKS_BMP_DIR"] = os.path.join(org, "train_val", "masks")
        g["SUIM_ORG_TRAIN_VAL_MASKS_PNG_DIR"] = os.path.join(org, "train_val", "masks_png")
        g["SUIM_ORG_TEST_IMAGES_DIR"] = os.path.join(org, "TEST", "images")
        g["SUIM_ORG_TEST_MASKS_BMP_PATH"] = os.path.join(org, "TEST", "masks")
        g["SUIM_ORG_TEST_MASKS_PNG_PATH"] = os.path.join(org, "TEST", "masks_png")
    elif prefix == "CITYSCAPES":
        g["CITYSCAPES_ORG_DATA_DIR"] = org
        for split in ("TRAIN", "VAL"):
            g[f"CITYSCAPES_ORG_{split}_IMAGES_DIR"] = os.path.join(org, "leftImg8bit", split.lower())
            g[f"CITYSCAPES_ORG_{split}_MASKS_DIR"] = os.path.join(org, "gtFine", split.lower())
        g["CITYSCAPES_ORG_VAL_TEST_IMAGES_DIR"] = os.path.join(org, "val_test", "images")
        g["CITYSCAPES_ORG_VAL_TEST_MASKS_DIR"] = os.path.join(org, "val_test", "masks")


_dataset("ISIC_2018", "ISIC_2018")
_dataset("SUIM", "SUIM")
_dataset("CITYSCAPES", "CITYSCAPES")
_dataset("HELA", "HELA")
