"""The data-preparation scripts: counterparts of the reference's ISIC_2018/00_*, 01_*; Cityscapes/00_*, 01_*; HeLa/00_*, 01_*;
SUIM/00_*, 01_*, 02_* -- step one of its workflow, from the four datasets' downloads under `BASE_DIR/original_data` to the
directory trees every other driver of this package reads.  run(dataset, step) makes the calls the script of that number makes at
import time, with its arguments; the functions live in prep.py.

Ranks: the 00 / 02 stages shard their file lists and end in a barrier; the 01 splits run on rank 0 only, the others wait.
Environment overrides for short runs (toy trees smaller than the reference's fixed crop sizes): IM_PREP_HELA_CROP (crop size, 256),
IM_PREP_SUIM_CROP (`target,min,max`, 256,256,512), IM_PREP_SUIM_CROPS_PER_IMAGE (2)."""
import os

from . import functions as F
from . import paths
from . import prep

# script -> the public names it defines in the reference (the names prep.py keeps; SUIM's split has its own signature)
SCRIPTS = {
    ("ISIC_2018", 0): ("ISIC_2018/00_ISIC_2018_preprocess_images.py", {"preprocess_data": "preprocess_data"}),
    ("ISIC_2018", 1): ("ISIC_2018/01_ISIC_2018_split_original_train.py", {"split_and_resize_dataset": "split_and_resize_dataset"}),
    ("Cityscapes", 0): ("Cityscapes/00_Cityscapes_resize_images_and_masks.py", {"resize_image": "resize_image",
                                                                                "process_images": "process_images"}),
    ("Cityscapes", 1): ("Cityscapes/01_Cityscapes_split_original_train_val.py", {"split_and_resize_dataset": "split_and_resize_dataset"}),
    ("HeLa", 0): ("HeLa/00_HeLa_create_crops.py", {"ImagePreprocessor": "ImagePreprocessor"}),
    ("HeLa", 1): ("HeLa/01_HeLa_split_train_in_labeled_and_unlabeled.py", {}),
    ("SUIM", 0): ("SUIM/00_SUIM_convert_bmp_to_png_masks.py", {"convert_color_bmp_to_class_mask_png": "convert_color_bmp_to_class_mask_png",
                                                              "convert_all_masks_in_folder": "convert_all_masks_in_folder"}),
    ("SUIM", 1): ("SUIM/01_SUIM_split_original_train_val.py", {"split_and_resize_dataset": "split_and_resize_dataset_suim"}),
    ("SUIM", 2): ("SUIM/02_SUIM_create_crops.py", {"random_crop": "random_crop", "create_random_crops": "create_random_crops"}),
}


def _ints_env(name, default):
    v = os.environ.get(name)
    return [int(x) for x in v.split(",")] if v else list(default)


def _rank0_only(fn):
    """the 01 splits: rank 0 works, every rank leaves together"""
    rank, _ = F._rank_world()
    if rank == 0:
        with F.local_rank_scope():
            fn()
    d = F._dist()
    if d:
        d.barrier()


def _isic(step):
    P = lambda n: getattr(paths, f"ISIC_2018_{n}")
    if step == 0:      # 00_ISIC_2018_preprocess_images.py:21-31, 58-59
        prep.preprocess_data([(P("ORG_TRAIN_IMAGES_DIR"), P("TRAIN_FULL_IMAGES_DIR")), (P("ORG_VAL_IMAGES_DIR"), P("VAL_IMAGES_DIR")),
                              (P("ORG_TEST_IMAGES_DIR"), P("TEST_IMAGES_DIR"))])
        prep.preprocess_data([(P("ORG_TRAIN_MASKS_DIR"), P("TRAIN_FULL_MASKS_DIR")), (P("ORG_VAL_MASKS_DIR"), P("VAL_MASKS_DIR")),
                              (P("ORG_TEST_MASKS_DIR"), P("TEST_MASKS_DIR"))], is_mask=True)
    else:              # 01_ISIC_2018_split_original_train.py:47-55
        _rank0_only(lambda: prep.split_and_resize_dataset(P("TRAIN_FULL_IMAGES_DIR"), P("TRAIN_FULL_MASKS_DIR"), P("BASE_DIR"),
                                                          ["train_labeled", "train_unlabeled"], 0.9, prep.SEED))


def _cityscapes(step):
    P = lambda n: getattr(paths, f"CITYSCAPES_{n}")
    if step == 0:      # 00_Cityscapes_resize_images_and_masks.py:69-79
        factor = float(F.config["CITYSCAPES"]["RESIZE_FACTOR"])
        prep.process_images(P("ORG_TRAIN_IMAGES_DIR"), P("ORG_TRAIN_MASKS_DIR"), P("TRAIN_FULL_IMAGES_DIR"), P("TRAIN_FULL_MASKS_DIR"),
                            factor)
        prep.process_images(P("ORG_VAL_IMAGES_DIR"), P("ORG_VAL_MASKS_DIR"), P("ORG_VAL_TEST_IMAGES_DIR"), P("ORG_VAL_TEST_MASKS_DIR"),
                            factor)
    else:              # 01_Cityscapes_split_original_train_val.py:47-63
        def both():
            prep.split_and_resize_dataset(P("TRAIN_FULL_IMAGES_DIR"), P("TRAIN_FULL_MASKS_DIR"), P("BASE_DIR"),
                                          ["train_labeled", "train_unlabeled"], 0.9, prep.SEED)
            prep.split_and_resize_dataset(P("ORG_VAL_TEST_IMAGES_DIR"), P("ORG_VAL_TEST_MASKS_DIR"), P("BASE_DIR"), ["val", "test"], 0.5,
                                          prep.SEED)
        _rank0_only(both)


def _hela(step):
    use_mod = F.config["HELA"]["USE_MOD_POS_SIZE"].lower() == "true"
    if step == 0:      # 00_HeLa_create_crops.py:198-218
        prep.hela_create_crops(paths.HELA_ORG_DIR, paths.HELA_BASE_DIR, use_mod, crop_size=_ints_env("IM_PREP_HELA_CROP", [256])[0])
    else:              # 01_HeLa_split_train_in_labeled_and_unlabeled.py:22-59
        _rank0_only(lambda: prep.hela_split(paths.HELA_TRAIN_FULL_DIR, paths.HELA_TRAIN_LABELED_DIR, paths.HELA_TRAIN_UNLABELED_DIR,
                                            use_mod, prep.SEED))


def _suim(step):
    P = lambda n: getattr(paths, f"SUIM_{n}")
    if step == 0:      # 00_SUIM_convert_bmp_to_png_masks.py:54-55
        from .im_driver import color_mapping
        mapping = color_mapping("SUIM", 9)
        prep.convert_all_masks_in_folder(P("ORG_TRAIN_VAL_MASKS_BMP_DIR"), P("ORG_TRAIN_VAL_MASKS_PNG_DIR"), mapping)
        prep.convert_all_masks_in_folder(P("ORG_TEST_MASKS_BMP_PATH"), P("ORG_TEST_MASKS_PNG_PATH"), mapping)
    elif step == 1:    # 01_SUIM_split_original_train_val.py:53-64
        def both():
            prep.split_and_resize_dataset_suim(P("ORG_TRAIN_VAL_IMAGES_DIR"), P("ORG_TRAIN_VAL_MASKS_PNG_DIR"), P("ORG_DATA_DIR"),
                                               ["train_full", "val"], 0.1)
            prep.split_and_resize_dataset_suim(P("ORG_TRAIN_FULL_IMAGES_DIR"), P("ORG_TRAIN_FULL_MASKS_DIR"), P("ORG_DATA_DIR"),
                                               ["train_unlabeled", "train_labeled"], 0.1)
        _rank0_only(both)
    else:              # 02_SUIM_create_crops.py:67-90
        sizes = _ints_env("IM_PREP_SUIM_CROP", [256, 256, 512])
        n = _ints_env("IM_PREP_SUIM_CROPS_PER_IMAGE", [2])[0]
        for images, masks, out in (("ORG_TRAIN_FULL_IMAGES_DIR", "ORG_TRAIN_FULL_MASKS_DIR", "TRAIN_FULL_MAIN_DIR"),
                                   ("ORG_TRAIN_LABELED_IMAGES_DIR", "ORG_TRAIN_LABELED_MASKS_DIR", "TRAIN_LABELED_MAIN_DIR"),
                                   ("ORG_TRAIN_UNLABELED_IMAGES_DIR", "ORG_TRAIN_UNLABELED_MASKS_DIR", "TRAIN_UNLABELED_MAIN_DIR"),
                                   ("ORG_VAL_IMAGES_DIR", "ORG_VAL_MASKS_DIR", "VAL_MAIN_DIR"),
                                   ("ORG_TEST_IMAGES_DIR", "ORG_TEST_MASKS_PNG_PATH", "TEST_MAIN_DIR")):
            prep._create_random_crops(P(images), P(masks), P(out), n, *sizes)


_RUN = {"ISIC_2018": _isic, "Cityscapes": _cityscapes, "HeLa": _hela, "SUIM": _suim}


def run(dataset, step):
    if (dataset, step) not in SCRIPTS:
        raise ValueError(f"no data-preparation step {step} for {dataset}")
    F.init_distributed()
    _RUN[dataset](step)
    F.flush_writes(all_threads=True)
