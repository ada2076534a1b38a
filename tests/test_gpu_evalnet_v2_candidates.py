"""Scoring B images x M candidate masks with the late-fusion EvalNet: imk_evalnet_forward_candidates runs ALL of the image tower (input
block + four conv blocks) once per image and must give the bits imk_evalnet_forward gives on the image repeated M times;
imk_evalnet_forward_select must give the bits of forward_candidates + imk_evalnet_select; IMK_SELECT_SHARED=0 (read once per process,
so run in a fresh child) scores the repeated images and gives the same bits again; and a v1 plan that goes through the same calls in a
process that also runs v2 plans gives the bits it gives in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import evalnet_v2_cases as V  # noqa: E402
from tests.test_gpu_unet import randomize_bn  # noqa: E402

B = 2
_MODELS = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def models(name, n, arch="v2"):
    """n EvalNets of one plan with perturbed BatchNorm statistics (cached; nothing here changes a model's weights)"""
    from inconsistencymasks_amd.evalnet import EvalNet
    cfg = V.CASES[name]
    out = []
    for j in range(n):
        key = (name, arch, j)
        if key not in _MODELS:
            h, w = (cfg["h"], cfg["w"]) if arch == "v2" else (64, 64)
            m = EvalNet(h, w, cfg["ca"], cfg["cb"], cfg["cb"], cfg["alpha"], True, True, False, seed=50 + 7 * j,
                        b_onehot=cfg.get("onehot", False), arch=arch)
            m.load_state_dict(randomize_bn(m.state_dict(), 51 + 7 * j))
            # One training-mode pass with momentum 0 puts the batch statistics of realistic inputs into the moving statistics: the
            # layers then stay normalised at inference and the sigmoid outputs are not saturated -- a saturated 0.0 / 1.0 would be
            # "bit-identical" whatever the towers computed.  The weights do not move (no optimizer step).
            xa, xb, _, _ = inputs(name, 2, arch, seed=90 + j)
            flat = xb.reshape((B * 2,) + tuple(xb.shape[2:]))
            flat = (flat if flat.dim() == 4 else flat[..., None]).contiguous()
            y = torch.rand((B * 2, 2 * cfg["cb"]), device="cuda", generator=torch.Generator(device="cuda").manual_seed(j))
            m.set_bn_momentum(0.0)
            m.fwd_bwd(xa.repeat_interleave(2, 0).contiguous(), flat, y)
            m.set_bn_momentum(0.99)
            sd = m.state_dict()      # ... and the last BatchNorm saw 16 samples: a tenth of the Dense kernels keeps the logits small
            sd["iou.w"], sd["detection.w"] = sd["iou.w"] * 0.1, sd["detection.w"] * 0.1
            m.load_state_dict(sd)
            m.ready_for_inference()
            _MODELS[key] = m
        out.append(_MODELS[key])
    return out


def inputs(name, m_cand, arch="v2", seed=0):
    """xa [B,H,W,ca]; xb [B,M,H,W,cb], or class ids [B,M,H,W] for a one-hot net; cand [B,M,H*W] bytes; counts [B]"""
    cfg = V.CASES[name]
    h, w = (cfg["h"], cfg["w"]) if arch == "v2" else (64, 64)
    rng = np.random.default_rng(seed + h + m_cand)
    xa = rng.integers(0, 256, (B, h, w, cfg["ca"]), dtype=np.uint8)
    if cfg.get("onehot"):
        xb = rng.integers(0, cfg["cb"], (B, m_cand, h // 4, w // 4), dtype=np.uint8).repeat(4, 2).repeat(4, 3)
    else:
        xb = (rng.integers(0, 2, (B, m_cand, h // 4, w // 4, cfg["cb"]), dtype=np.uint8) * 255).astype(np.uint8).repeat(4, 2).repeat(4, 3)
    cand = rng.integers(0, 256, (B, m_cand, h * w), dtype=np.uint8)
    counts = np.asarray([m_cand, max(1, m_cand - 2)][:B], dtype=np.int32)
    return dev(xa), dev(xb), dev(cand), dev(counts)


def repeated(ms, xa, xb):
    """imk_evalnet_forward on the image repeated M times -> [N,B,M,U]"""
    b, m_cand = xb.shape[:2]
    rep = xa.repeat_interleave(m_cand, 0).contiguous()
    flat = xb.reshape((b * m_cand,) + tuple(xb.shape[2:]))
    flat = (flat if flat.dim() == 4 else flat[..., None]).contiguous()
    return torch.stack([m.predict_device(rep, flat).reshape(b, m_cand, -1) for m in ms], 0)


@pytest.mark.parametrize("name", ["hela", "odd"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("m_cand", [1, 5, 11])
def test_forward_candidates_equals_forward_on_repeated_images(name, n, m_cand):
    from inconsistencymasks_amd.evalnet import CandidateScorer
    ms = models(name, n)
    xa, xb, _, _ = inputs(name, m_cand)
    scorer = CandidateScorer(ms)
    assert scorer.shared
    got = scorer.scores(xa, xb)
    want = repeated(ms, xa, xb)
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.isfinite(got).all()
    assert float(((got > 1e-3) & (got < 1 - 1e-3)).float().mean()) > 0.5, "saturated outputs cannot tell one tower pass from another"
    if m_cand > 1:      # the candidates of an image do get different scores: tower B is not shared
        assert not torch.equal(got[:, :, 0], got[:, :, 1])


def select_all(name, n, m_cand, arch="v2"):
    """forward_select in both modes, with and without counts -> {key: tensors}; also checked against candidates + select here"""
    from inconsistencymasks_amd import evalnet as EV
    ms = models(name, n, arch)
    xa, xb, cand, counts = inputs(name, m_cand, arch)
    scorer = EV.CandidateScorer(ms)
    scores = scorer.scores(xa, xb)
    thr = float(scores.mean(0)[..., :ms[0].plan.n_out].mean())
    out = {"scores": scores.cpu()}
    for mode in (EV.SELECT_MIOU, EV.SELECT_CONF_GATED):
        for cnt in (None, counts):
            got = scorer.run(xa, xb, cand, thr, cnt, mode)
            assert torch.equal(scorer.last_scores, scores)
            want = EV.select_candidates(scores, cand, thr, mode, cnt)
            for g, w_, what in zip(got, want, ("best_idx", "best_score", "keep", "chosen")):
                assert torch.equal(g, w_), (mode, cnt is not None, what)
                out[f"{mode}.{int(cnt is not None)}.{what}"] = g.cpu()
    return out


@pytest.mark.parametrize("name", ["hela", "odd"])
def test_forward_select_equals_candidates_then_select(name):
    out = select_all(name, 3, 5)
    assert set(out["1.1.best_idx"].tolist()) <= set(range(5))


CHILD = ("import sys, torch\n"
         "sys.path[:0] = [%r, %r]\n"
         "import test_gpu_evalnet_v2_candidates as T\n"
         "torch.save(T.select_all(sys.argv[2], 3, 5, sys.argv[3]), sys.argv[1])\n") % (ROOT, HERE)


def _child(tmp_path, name, arch, env):
    path = str(tmp_path / f"{name}_{arch}.pt")
    r = subprocess.run([sys.executable, "-c", CHILD, path, name, arch], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return torch.load(path)


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_select_shared_off_gives_the_same_bits(tmp_path):
    assert os.environ.get("IMK_SELECT_SHARED", "1") != "0", "this process must run the shared tower"
    _same(select_all("odd", 3, 5), _child(tmp_path, "odd", "v2", {"IMK_SELECT_SHARED": "0"}))


def test_a_v1_plan_beside_v2_plans_gives_the_bits_it_gives_alone(tmp_path):
    select_all("hela", 3, 5)                          # v2 plans have run in this process ...
    here = select_all("hela", 3, 5, "v1")             # ... then a v1 plan through the same calls
    select_all("hela", 3, 5)
    _same(here, select_all("hela", 3, 5, "v1"))
    _same(here, _child(tmp_path, "hela", "v1", {}))   # and in a process that never made a v2 plan
