"""HeLa full-dataset baseline (the upper bound) on MI355X: counterpart of the reference driver HeLa/02_HeLa_full_dataset.py
(same loops, file / model / CSV names); the loop body lives in inconsistencymasks_amd/subset_driver.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.subset_driver import run  # noqa: E402

if __name__ == "__main__":
    run("HeLa", full=True)
