"""SUIM data preparation on MI355X: counterpart of the reference script SUIM/01_SUIM_split_original_train_val.py -- train_val split into
train_full / val, train_full into train_unlabeled / train_labeled (10 % each time, seed 42); the JPEGs are copied byte for byte. The calls
live in inconsistencymasks_amd/prep_driver.py, the functions and their HIP kernels in inconsistencymasks_amd/prep.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.prep import split_and_resize_dataset_suim as split_and_resize_dataset  # noqa: E402,F401
from inconsistencymasks_amd.prep_driver import run  # noqa: E402

if __name__ == "__main__":
    run("SUIM", 1)
