"""The single-head EvalNet with a one-hot input B (get_evalnet(..., onehot_B=True): the scalar-IoU multiclass family's network)
against the torch-CPU oracle (oracle/evalnet_oracle.py, fed the explicit one-hot stack and two_heads=False), with exactly the checks
and bounds of tests/test_gpu_evalnet.py (its training-pass test body runs here on these configurations, its inference test is restated
for one head): outputs, per-layer rel-L2, losses, gradient tensors with pinned forward values, determinism bit for bit.  normalize_B
divides the one-hot stack by 255 like any input (get_evalnet's default); the hot channel then holds fp16(1 / 255), which is what the
oracle's x / 255 rounds to.

For K = 3 the one-hot plan is also held to the plan that existed before: get_evalnet(64, 64, 3, 3) without one-hot, fed the explicit
0 / 1 uint8 stack, same weights.  And get_evalnet_miou's one-hot forward, which goes through the same kernel with the hot value 1, is
held to the bits it gave before that value became a parameter."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import evalnet_oracle as E  # noqa: E402
from tests import test_gpu_evalnet as T  # noqa: E402

CFGS = {f"k{k}_{'norm' if nb else 'raw'}": dict(h=64, w=64, ca=3, cb=k, k=1, alpha=0.5, two=False, na=True, nb=nb, b=3, onehot=True)
        for k in (9, 3) for nb in (False, True)}


@pytest.mark.parametrize("name", list(CFGS))
def test_inference_parity(name):
    """tests/test_gpu_evalnet.py::test_inference_parity for one head (its one-hot branch concatenates the two heads' arrays)"""
    cfg = CFGS[name]
    m, sd, xa, xb, _ = T.make(cfg, 21)
    m.debug(materialize=True)
    try:
        got = m.predict([xa, xb])
    finally:
        m.debug(materialize=False)
    taps = {}
    ref, _ = E.forward(sd, xa, T.ob(cfg, xb), False, cfg["na"], cfg["nb"], emulate_fp16=True, taps=taps)
    for n, t in taps.items():
        assert T.rel_l2(m.intermediate(n, cfg["b"], 0).numpy(), t.numpy()) <= 1e-2, n
    assert got.shape == (cfg["b"], 1) and np.abs(got - ref.numpy()).max() <= 2e-2
    assert np.array_equal(m.predict([xa, E.one_hot(xb, cfg["cb"])]), got)      # the one-hot stack itself, as the call sites pass it
    assert np.array_equal(m.predict([xa, xb]), got)                           # determinism
    assert np.abs(m.predict([xa[:1], xb[:1]]) - got[:1]).max() <= 1e-6        # batch invariance of inference


@pytest.mark.parametrize("name", list(CFGS))
def test_train_pass_parity(monkeypatch, name):
    monkeypatch.setitem(T.CFGS, name, CFGS[name])
    T.test_train_pass_parity(name)


def test_get_evalnet_builds_this_plan_and_the_files_keep_it(tmp_path, monkeypatch):
    from inconsistencymasks_amd import evalnet_functions as EF
    from inconsistencymasks_amd.evalnet import CandidateScorer, get_evalnet
    m = get_evalnet(64, 64, 3, 9, 0.5, seed=3)                                    # more than 4 channels: one-hot, normalised
    assert m.plan.b_onehot and m.plan.cfg.normalize_b == 1 and m.n_heads == 1
    assert (m.plan.n_total, m.plan.n_trainable) == E.count_params(3, 9, 1, 0.5, False)
    assert not get_evalnet(64, 64, 3, 3, 0.5, seed=3).plan.b_onehot and get_evalnet(64, 64, 3, 3, 0.5, seed=3, onehot_B=True).plan.b_onehot
    rng = np.random.default_rng(1)
    xa = rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    ids = rng.integers(0, 9, (2, 8, 8, 1)).astype(np.uint8).repeat(8, 1).repeat(8, 2)
    want = m.predict([xa, ids])
    assert want.shape == (2, 1) and np.array_equal(m.predict([xa, E.one_hot(ids, 9)]), want)      # the stack the call sites pass
    for fmt in ("safetensors", "keras_h5"):
        monkeypatch.setenv("IMK_MODEL_FORMAT", fmt)
        path = str(tmp_path / f"net_{fmt}.h5")
        EF.save_evalnet(m, path)
        back = EF.load_evalnet(path)
        assert back.plan.b_onehot and back.plan.cfg.normalize_b == 1 and np.array_equal(back.predict([xa, ids]), want), fmt
    # CandidateScorer takes it unchanged: class-id candidates, one score each
    xad, cand = torch.from_numpy(xa).cuda(), torch.from_numpy(np.stack([ids[..., 0], ids[::-1, ..., 0]], 1)).cuda().contiguous()
    sc = CandidateScorer([m, back]).scores(xad, cand)
    assert sc.shape == (2, 2, 2, 1) and np.array_equal(sc[0, :, 0].cpu().numpy(), want) and torch.equal(sc[0], sc[1])


@pytest.mark.parametrize("nb", [False, True])
def test_k3_one_hot_plan_against_the_mask_stack_plan(nb):
    """one non-zero term per pixel in the input block's 1x1 convolution on either route: the outputs are held to the output bound of
    tests/test_gpu_evalnet.py (2e-2).  Observed on an MI355X, with and without normalize_B: bit-equal (max |d| = 0); the line printed
    here (run with -s) says what a later run sees."""
    from inconsistencymasks_amd.evalnet import get_evalnet
    cfg = CFGS[f"k3_{'norm' if nb else 'raw'}"]
    m, sd, xa, xb, _ = T.make(cfg, 21)
    plain = get_evalnet(64, 64, 3, 3, 0.5, normalize_B=nb, seed=21, onehot_B=False)
    plain.load_state_dict(sd)
    got, want = m.predict([xa, xb]), plain.predict([xa, E.one_hot(xb, 3)])
    print(f"\none-hot plan vs mask-stack plan, normalize_B={nb}: max |d| = {np.abs(got - want).max():.3e}, bit-equal = {np.array_equal(got, want)}")
    assert np.abs(got - want).max() <= 2e-2


def test_get_evalnet_miou_one_hot_forward_keeps_its_bits():
    """tests/golden/evalnet_miou_onehot_forward.npz: the outputs of these two forwards as the library gave them on an MI355X before
    onehot_kernel took its hot value as a parameter (the SUIM and the Cityscapes-like shape of tests/test_gpu_evalnet.py, seed 21);
    with the value 1 the kernel writes the bytes it wrote, so the outputs are the same bits"""
    from inconsistencymasks_amd.evalnet import get_evalnet_miou
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with np.load(os.path.join(root, "tests", "golden", "evalnet_miou_onehot_forward.npz")) as d:
        want = {k: d[k] for k in d.files}
    for name, (h, w, k, alpha, b) in {"suim": (64, 64, 9, 1.0, 3), "city": (104, 208, 35, 0.5, 2)}.items():
        m = get_evalnet_miou(h, w, 3, k, alpha, seed=21, onehot_B=True)
        rng = np.random.default_rng(23)
        xa = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
        xb = rng.integers(0, k, (b, h // 8, w // 8, 1)).astype(np.uint8).repeat(8, 1).repeat(8, 2)
        got = np.concatenate(m.predict([xa, xb]), 1)
        assert got.tobytes() == want[name].tobytes(), (name, float(np.abs(got - want[name]).max()))
