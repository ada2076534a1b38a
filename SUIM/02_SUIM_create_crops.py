"""SUIM data preparation on MI355X: counterpart of the reference script SUIM/02_SUIM_create_crops.py -- two random 256..511-pixel square crops
per image, resized to 256 x 256 (image linear, mask nearest), for all five sets. The calls live in inconsistencymasks_amd/prep_driver.py,
the functions and their HIP kernels in inconsistencymasks_amd/prep.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.prep import random_crop, create_random_crops  # noqa: E402,F401
from inconsistencymasks_amd.prep_driver import run  # noqa: E402

if __name__ == "__main__":
    run("SUIM", 2)
