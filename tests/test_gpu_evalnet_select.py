"""imk_evalnet_select / imk_evalnet_forward_candidates / imk_evalnet_forward_select (include/imk.h) on the GPU.

Rules: the select kernel on the scores the real reference was driven with (tests/golden/evalnet_ensemble.npz) must give the recorded
choice and keep decision, bit for bit, and gather the chosen candidate's bytes -- with `counts` (cases of different M padded to 16
candidates with NaN / inf garbage behind their own) and without, for 16-byte and 64*64-byte candidates.
Shared tower: imk_evalnet_forward_candidates == imk_evalnet_forward on the image repeated M times, bit for bit.
Fused: imk_evalnet_forward_select == the two calls == itself under IMK_SELECT_SHARED=0 (a child process), bit for bit.
Argument errors come back as error codes before anything is launched."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from test_golden_evalnet_ensemble import KINDS, cases, load, meta, select_rule

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inconsistencymasks_amd import evalnet
    return evalnet


# ---- rules ---------------------------------------------------------------------------------------------------------------------
def fixture_groups():
    """the fixture's cases grouped by (kind, N, U): one batch per group"""
    d = load()
    groups = {}
    for kind in KINDS:
        for c in cases(d, kind):
            n, m, u = d[c + "_scores"].shape
            groups.setdefault((kind, n, u), []).append(c)
    return d, groups


@pytest.mark.parametrize("cand_bytes", [16, 64 * 64])
def test_rules_match_the_recorded_reference(ev, cand_bytes):
    import torch
    d, groups = fixture_groups()
    rng = np.random.default_rng(5)
    assert len(groups) >= 8
    for (kind, n, u), cs in sorted(groups.items()):
        mode = ev.SELECT_IOU if kind == "bin" else ev.SELECT_MIOU
        # (a) counts given: every case padded to 16 candidates; what lies behind a case's own candidates must not matter
        garbage = np.array([np.nan, np.inf, 1.0, 0.999], F32)
        sc = garbage[rng.integers(0, 4, (n, len(cs), ev.SELECT_MAX_CAND, u))]
        counts = np.zeros(len(cs), np.int32)
        for b, c in enumerate(cs):
            s = d[c + "_scores"]
            sc[:, b, :s.shape[1]] = s
            counts[b] = s.shape[1]
        thrs = sorted({meta(d, c)[0] for c in cs})
        cand = torch.from_numpy(rng.integers(0, 256, (len(cs), ev.SELECT_MAX_CAND, cand_bytes), dtype=np.uint8)).cuda()
        for thr in thrs:      # one launch per threshold of the group
            bi, bs, keep, out = ev.select_candidates(torch.from_numpy(sc).cuda(), cand, thr, mode, torch.from_numpy(counts).cuda())
            bi, bs, keep, out = bi.cpu().numpy(), bs.cpu().numpy(), keep.cpu().numpy(), out.cpu().numpy()
            for b, c in enumerate(cs):
                want_best, want_score, want_keep = select_rule(d[c + "_scores"], thr, kind != "bin")
                assert int(bi[b]) == want_best and bs[b].tobytes() == F32(want_score).tobytes() and int(keep[b]) == int(want_keep), (c, thr)
                assert np.array_equal(out[b], cand[b, want_best].cpu().numpy()), c
                if thr == meta(d, c)[0]:      # the reference's own run of this case
                    assert (int(bi[b]), int(keep[b])) == meta(d, c)[2:], c
        # (b) counts NULL: the cases of one M together
        for m in sorted(set(counts.tolist())):
            sub = [c for c in cs if d[c + "_scores"].shape[1] == m]
            s = np.stack([d[c + "_scores"] for c in sub], 1)
            cand_m = torch.from_numpy(rng.integers(0, 256, (len(sub), m, cand_bytes), dtype=np.uint8)).cuda()
            for thr in sorted({meta(d, c)[0] for c in sub}):
                bi, bs, keep, out = ev.select_candidates(torch.from_numpy(s).cuda(), cand_m, thr, mode)
                for b, c in enumerate(sub):
                    if thr == meta(d, c)[0]:
                        assert (int(bi[b]), int(keep[b])) == meta(d, c)[2:], c
                        assert torch.equal(out[b], cand_m[b, int(bi[b])]), c


# ---- shared tower ----------------------------------------------------------------------------------------------------------------
CONFIGS = {       # name: (cb, n_out, two_heads, normalize_b, b_onehot)
    "one_head": (1, 1, False, True, False),
    "two_head_raw": (3, 3, True, False, False),
    "onehot9": (9, 9, True, False, True),
    "onehot35": (35, 35, True, False, True),
}


def make_models(ev, h, w, width, config, n, ca=3):
    cb, n_out, two, norm_b, onehot = CONFIGS[config]
    return [ev.EvalNet(h, w, ca, cb, n_out, width / 16.0, two, True, norm_b, seed=900 + 7 * j, b_onehot=onehot) for j in range(n)]


def make_inputs(h, w, config, b, m, seed, ca=3):
    """images of clearly different brightness (so that a wrong row / M mapping shows) and m candidate masks each"""
    import torch
    cb, _, _, norm_b, onehot = CONFIGS[config]
    rng = np.random.default_rng(seed)
    xa = np.stack([np.clip(rng.integers(0, 60, (h, w, ca)) + 90 * i, 0, 255) for i in range(b)]).astype(np.uint8)
    if onehot:
        xb = rng.integers(0, cb, (b, m, h, w), dtype=np.uint8)
    else:
        xb = (rng.integers(0, 2, (b, m, h, w, cb), dtype=np.uint8) * (255 if norm_b else 1)).astype(np.uint8)
    yy = np.arange(h)[:, None]
    for i in range(b):
        for j in range(m):      # candidates that differ in a large region, not only in noise
            xb[i, j][yy[:, 0] < (h * (j + 1)) // (m + 1)] = 0
    return torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()


def repeated_reference(models, xa, xb):
    """imk_evalnet_forward per model on the repeated image -> [N,B,M,U]"""
    import torch
    b, m = xb.shape[:2]
    rep = xa.repeat_interleave(m, 0).contiguous()
    flat = xb.reshape((b * m,) + tuple(xb.shape[2:]))
    if flat.dim() == 3:
        flat = flat[..., None]
    return torch.stack([mod.predict_device(rep, flat.contiguous()).reshape(b, m, -1) for mod in models], 0)


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("width", [8, 16, 32])
@pytest.mark.parametrize("hw", [(64, 64), (80, 96)])
def test_shared_tower_equals_repeated_image(ev, hw, width, config):
    import torch
    h, w = hw
    models = make_models(ev, h, w, width, config, 3)
    for m in (1, 2, 5, 11):
        xa, xb = make_inputs(h, w, config, 3, m, seed=m)
        want = repeated_reference(models, xa, xb)
        got3 = ev.CandidateScorer(models).scores(xa, xb)
        got1 = ev.CandidateScorer(models[:1]).scores(xa, xb)
        torch.cuda.synchronize()
        assert got3.shape == want.shape and torch.equal(got3.view(torch.int32), want.view(torch.int32)), (m, "N=3")
        assert torch.equal(got1.view(torch.int32), want[:1].view(torch.int32)), (m, "N=1")
        flat = want[0].reshape(3 * m, -1)
        assert len(torch.unique(flat, dim=0)) == 3 * m, "every (image, candidate) pair must score differently for this test to see a wrong row"


# ---- fused -------------------------------------------------------------------------------------------------------------------------
FUSED_CASES = [((64, 64), 16, "one_head", 2, 5), ((80, 96), 32, "two_head_raw", 3, 11), ((64, 64), 8, "onehot9", 3, 6),
               ((80, 96), 16, "onehot35", 2, 2), ((64, 64), 32, "one_head", 1, 1)]


def run_fused_case(ev, hw, width, config, n, m, dump):
    import torch
    h, w = hw
    b = 3
    models = make_models(ev, h, w, width, config, n)
    xa, xb = make_inputs(h, w, config, b, m, seed=100 + m)
    rng = np.random.default_rng(m)
    cand = torch.from_numpy(rng.integers(0, 256, (b, m, h * w), dtype=np.uint8)).cuda()
    counts = torch.from_numpy(np.array([m, max(1, m - 1), max(1, m // 2)], np.int32)).cuda()
    scorer = ev.CandidateScorer(models)
    composed_scores = scorer.scores(xa, xb)
    mode = ev.SELECT_MIOU if CONFIGS[config][2] else ev.SELECT_IOU
    sc0 = composed_scores[..., 0].mean(0) if mode == ev.SELECT_IOU else None
    thr = float(sc0.max(1).values.median()) if sc0 is not None else 0.25      # IoU mode: some images kept, some not
    key = f"{hw[0]}x{hw[1]}_{width}_{config}_{n}_{m}"
    for tag, cnt in (("counts", counts), ("all", None)):
        fused = scorer.run(xa, xb, cand, thr, cnt)
        fused_scores = scorer.last_scores
        composed = ev.select_candidates(composed_scores, cand, thr, mode, cnt)
        torch.cuda.synchronize()
        assert torch.equal(fused_scores.view(torch.int32), composed_scores.view(torch.int32)), (key, tag)
        for f, c, what in zip(fused, composed, ("best_idx", "best_score", "keep", "out")):
            assert torch.equal(f.view(torch.int32) if f.dtype == torch.float32 else f, c.view(torch.int32) if c.dtype == torch.float32 else c), (key, tag, what)
            dump[f"{key}_{tag}_{what}"] = f.cpu().numpy()
        dump[f"{key}_{tag}_scores"] = fused_scores.cpu().numpy()
        # ... and the restated rule on those scores
        s = composed_scores.cpu().numpy()
        for i in range(b):
            want = select_rule(s[:, i], thr, mode == ev.SELECT_MIOU, None if cnt is None else int(cnt[i]))
            assert (int(fused[0][i]), int(fused[2][i])) == (want[0], int(want[2])), (key, tag, i)
            assert torch.equal(fused[3][i], cand[i, want[0]])


def test_fused_equals_composed_and_repeated_route(ev, tmp_path):
    """fused == scores + select in this process; the same call in a child process with IMK_SELECT_SHARED=0 (the switch table is read
    once per process), which scores through imk_evalnet_forward on a device-side repeat of the images, gives the same bytes"""
    child = ("import sys, numpy as np\n"
             "sys.path[:0] = [%r, %r]\n"
             "import test_gpu_evalnet_select as T\n"
             "from inconsistencymasks_amd import evalnet\n"
             "dump = {}\n"
             "for case in T.FUSED_CASES:\n"
             "    T.run_fused_case(evalnet, *case, dump=dump)\n"
             "np.savez(sys.argv[1], **dump)\n") % (ROOT, os.path.join(ROOT, "tests"))
    path = str(tmp_path / "repeated.npz")
    r = subprocess.run([sys.executable, "-c", child, path], env=dict(os.environ, IMK_SELECT_SHARED="0"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.environ.get("IMK_SELECT_SHARED", "1") != "0", "this process must run the shared-tower route"
    fused = {}
    for case in FUSED_CASES:
        run_fused_case(ev, *case, dump=fused)
    with np.load(path) as rep:
        assert sorted(rep.files) == sorted(fused)
        for k in fused:
            assert rep[k].tobytes() == fused[k].tobytes(), k
    keeps = np.concatenate([v for k, v in fused.items() if k.endswith("_keep")])
    assert set(keeps.tolist()) == {0, 1}, "both keep values must occur"


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors(ev):
    import torch
    from inconsistencymasks_amd._lib import lib
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    stream = torch.cuda.current_stream().cuda_stream
    b = 2

    def select(n, m, counts=None):
        sc = torch.rand((n, b, m, 1), device="cuda")
        cand = torch.zeros((b, m, 16), dtype=torch.uint8, device="cuda")
        outs = (torch.zeros(b, dtype=torch.int32, device="cuda"), torch.zeros(b, device="cuda"),
                torch.zeros(b, dtype=torch.uint8, device="cuda"), torch.zeros((b, 16), dtype=torch.uint8, device="cuda"))
        rc = lib.imk_evalnet_select(sc.data_ptr(), n, b, m, 1, 1, counts.data_ptr() if counts is not None else None, cand.data_ptr(), 16,
                                    0.5, 0, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), stream)
        torch.cuda.synchronize()
        return rc

    assert select(2, 16) == 0 and select(8, 5) == 0
    assert select(2, 17) == EUNSUPPORTED
    assert select(9, 5) == EUNSUPPORTED
    assert select(2, 5, torch.tensor([5, 0], dtype=torch.int32, device="cuda")) == EINVAL
    assert select(2, 5, torch.tensor([6, 1], dtype=torch.int32, device="cuda")) == EINVAL
    assert select(2, 5, torch.tensor([5, 1], dtype=torch.int32, device="cuda")) == 0

    models = make_models(ev, 64, 64, 16, "one_head", 2)
    scorer = ev.CandidateScorer(models)
    plan = models[0].plan.ptr
    assert lib.imk_evalnet_forward_candidates_workspace_bytes(plan, b, 17) == EUNSUPPORTED
    need = lib.imk_evalnet_forward_candidates_workspace_bytes(plan, b, 5)
    assert need > 0
    xa, xb = make_inputs(64, 64, "one_head", b, 5, seed=1)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    sc = torch.full((2, b, 5, 1), -1.0, device="cuda")

    def forward(n, m, ws_bytes):
        rc = lib.imk_evalnet_forward_candidates(plan, n, scorer._params, scorer._packed, xa.data_ptr(), xb.data_ptr(), b, m, sc.data_ptr(),
                                                ws.data_ptr(), ws_bytes, stream)
        torch.cuda.synchronize()
        return rc

    assert forward(2, 5, need - 1) == EWORKSPACE
    assert forward(2, 17, need) == EUNSUPPORTED
    params9 = (ctypes.c_void_p * 9)(*([scorer._params[0]] * 9))
    rc = lib.imk_evalnet_forward_candidates(plan, 9, params9, params9, xa.data_ptr(), xb.data_ptr(), b, 5, sc.data_ptr(), ws.data_ptr(), need,
                                            stream)
    assert rc == EUNSUPPORTED
    assert float(sc.max()) == -1.0, "a refused call must not have launched anything"
    assert forward(2, 5, need) == 0 and float(sc.min()) >= 0.0

    cand = torch.zeros((b, 5, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception):
        scorer.run(xa, xb, cand, 0.5, torch.tensor([0, 5], dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
