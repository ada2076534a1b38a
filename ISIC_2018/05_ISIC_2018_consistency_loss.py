"""ISIC_2018 consistency-loss baseline on MI355X: counterpart of the reference driver ISIC_2018/05_ISIC_2018_consistency_loss.py
(same loops, file / model / CSV names); the loop body lives in inconsistencymasks_amd/consistency_driver.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.consistency_driver import run  # noqa: E402

if __name__ == "__main__":
    run("ISIC_2018")
