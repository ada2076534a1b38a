"""SUIM data preparation on MI355X: counterpart of the reference script SUIM/00_SUIM_convert_bmp_to_png_masks.py -- the colour `.bmp` masks of
train_val and TEST converted to class-id PNGs. The calls live in inconsistencymasks_amd/prep_driver.py, the functions and their HIP kernels
in inconsistencymasks_amd/prep.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.prep import convert_color_bmp_to_class_mask_png, convert_all_masks_in_folder  # noqa: E402,F401
from inconsistencymasks_amd.prep_driver import run  # noqa: E402

if __name__ == "__main__":
    run("SUIM", 0)
