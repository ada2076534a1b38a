"""ISIC_2018 data preparation on MI355X: counterpart of the reference script ISIC_2018/00_ISIC_2018_preprocess_images.py -- every file of the
three download folders (images and `_segmentation` masks) resized to IMAGE_WIDTH x IMAGE_HEIGHT into train_full / val / test. The calls live
in inconsistencymasks_amd/prep_driver.py, the functions and their HIP kernels in inconsistencymasks_amd/prep.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.prep import preprocess_data  # noqa: E402,F401
from inconsistencymasks_amd.prep_driver import run  # noqa: E402

if __name__ == "__main__":
    run("ISIC_2018", 0)
