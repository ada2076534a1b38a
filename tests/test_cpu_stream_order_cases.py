"""The case lists of tests/stream_order_runner.py without a GPU: every name exists where the runner looks it up, the student cases
fork (last decoder width above 8) and the skew sets are the ones tests/test_gpu_stream_order.py expects."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import stream_order_runner as R  # noqa: E402


def test_case_names_exist():
    import consistency_cases as C
    from tests.test_gpu_evalnet import CFGS as EVALNET
    from tests.test_gpu_noisy_student import SMALL
    from tests.test_gpu_unet import CFGS as UNET
    assert set(R.UNET_CASES) | set(R.ENSEMBLE_CASES) <= set(UNET)
    assert set(R.EVALNET_CASES) <= set(EVALNET)
    assert set(R.CONSISTENCY_CASES) <= set(C.CASES)
    assert ("isic" in C.FUSED) and ("suim" not in C.FUSED)          # one fused, one composed
    small = {s[0]: s for s in SMALL}
    assert set(R.STUDENT_CASES) <= set(small)
    assert {small[n][6] for n in R.STUDENT_CASES} == {"sigmoid", "softmax"}
    assert all(int(16 * small[n][5]) > 8 for n in R.STUDENT_CASES)  # the image path forks above 8 channels


def test_skew_sets():
    names = lambda skews: [R.skew_name(s) for s in skews]  # noqa: E731
    assert names(R.training_skews(0)) == ["none", "main", "side0+side1"]
    assert names(R.training_skews(1)) == ["none", "main", "side0"]
    assert names(R.training_skews(2)) == ["none", "main", "side0", "side1", "side0+side1"]
    assert names(R.steps_skews(0)) == names(R.steps_skews(1)) == ["none", "main>side0"]
    assert names(R.steps_skews(2)) == ["none", "main>side0", "main>side1"]
    assert names(R.inference_skews(1)) == names(R.inference_skews(2)) == ["none", "main", "side0"]
    assert names(R.inference_skews(3)) == names(R.training_skews(2))
    assert len(set(R.training_case_ids() + R.inference_case_ids())) == 20 + 12 + 2
