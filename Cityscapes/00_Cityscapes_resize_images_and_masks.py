"""Cityscapes data preparation on MI355X: counterpart of the reference script Cityscapes/00_Cityscapes_resize_images_and_masks.py --
leftImg8bit / gtFine pairs resized by RESIZE_FACTOR up to a multiple of 16 (images linear, label ids nearest then + 1) into train_full and
original_data/val_test. The calls live in inconsistencymasks_amd/prep_driver.py, the functions and their HIP kernels in
inconsistencymasks_amd/prep.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.prep import resize_image, process_images  # noqa: E402,F401
from inconsistencymasks_amd.prep_driver import run  # noqa: E402

if __name__ == "__main__":
    run("Cityscapes", 0)
