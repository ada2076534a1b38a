"""Cityscapes data preparation on MI355X: counterpart of the reference script Cityscapes/01_Cityscapes_split_original_train_val.py --
train_full split into train_labeled / train_unlabeled (10 % / 90 %), val_test into val / test (halves). The calls live in
inconsistencymasks_amd/prep_driver.py, the functions and their HIP kernels in inconsistencymasks_amd/prep.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.prep import split_and_resize_dataset  # noqa: E402,F401
from inconsistencymasks_amd.prep_driver import run  # noqa: E402

if __name__ == "__main__":
    run("Cityscapes", 1)
