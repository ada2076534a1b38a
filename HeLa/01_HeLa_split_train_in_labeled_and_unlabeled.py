"""HeLa data preparation on MI355X: counterpart of the reference script HeLa/01_HeLa_split_train_in_labeled_and_unlabeled.py -- train_full
crops shuffled with SEED, the first 10 % copied to train_labeled, the rest to train_unlabeled. The calls live in
inconsistencymasks_amd/prep_driver.py, the functions and their HIP kernels in inconsistencymasks_amd/prep.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.prep_driver import run  # noqa: E402

if __name__ == "__main__":
    run("HeLa", 1)
