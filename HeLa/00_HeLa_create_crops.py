"""HeLa data preparation on MI355X: counterpart of the reference script HeLa/00_HeLa_create_crops.py -- 256 x 256 crops with 60 % overlap of
every brightfield image and its alive / dead / position channels. The calls live in inconsistencymasks_amd/prep_driver.py, the functions and
their HIP kernels in inconsistencymasks_amd/prep.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.prep import ImagePreprocessor  # noqa: E402,F401
from inconsistencymasks_amd.prep_driver import run  # noqa: E402

if __name__ == "__main__":
    run("HeLa", 0)
