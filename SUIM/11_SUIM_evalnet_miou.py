"""SUIM single-EvalNet selection baseline on MI355X: counterpart of the reference driver SUIM/11_SUIM_evalnet_miou.py
(same loops, file / model / CSV names); the loop body lives in inconsistencymasks_amd/segnet_driver.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.segnet_driver import run  # noqa: E402

if __name__ == "__main__":
    run("SUIM", ensemble=False)
