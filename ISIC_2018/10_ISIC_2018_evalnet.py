"""ISIC_2018 single-EvalNet selection baseline on MI355X: counterpart of the reference driver ISIC_2018/10_ISIC_2018_evalnet.py
(same loops, file / model / CSV names); the loop body lives in inconsistencymasks_amd/segnet_driver.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.segnet_driver import run  # noqa: E402

if __name__ == "__main__":
    run("ISIC_2018", ensemble=False)
