"""ISIC_2018 data preparation on MI355X: counterpart of the reference script ISIC_2018/01_ISIC_2018_split_original_train.py -- train_full split
10 % / 90 % into train_labeled / train_unlabeled (train_test_split restated, SEED). The calls live in inconsistencymasks_amd/prep_driver.py,
the functions and their HIP kernels in inconsistencymasks_amd/prep.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.prep import split_and_resize_dataset  # noqa: E402,F401
from inconsistencymasks_amd.prep_driver import run  # noqa: E402

if __name__ == "__main__":
    run("ISIC_2018", 1)
