"""Cityscapes noisy-student baseline on MI355X: counterpart of the reference driver Cityscapes/08_Cityscapes_noisy_student.py
(same loops, file / model / CSV names); the loop body lives in inconsistencymasks_amd/im_driver.py."""
import os
import sys

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from inconsistencymasks_amd.im_driver import run  # noqa: E402

if __name__ == "__main__":
    run("Cityscapes", approach="noisy_student")
