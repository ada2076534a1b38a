"""IMK_SELECT_CONF_GATED (include/imk.h) on the GPU: the rule of the reference's single-EvalNet multi-class writer in imk_evalnet_select and
imk_evalnet_forward_select.

Rules: the kernel on the scores the real reference was driven with (tests/golden/evalnet_single.npz) must give, bit for bit, what the
restated rule (tests/test_golden_evalnet_single.py: select_rule_gated) gives -- best index, score, keep decision, gathered bytes -- and at
every case's own threshold what the reference recorded; with `counts` (cases padded to 16 candidates with NaN / inf garbage behind their
own, which must change neither gate nor choice) and without, for 16-byte and 64*64-byte candidates.  A few hundred random stacks (several
models, exact 0.03f, NaN, +-0 among the values) against the restatement.  The binary cases of the fixture under IMK_SELECT_IOU with N = 1.
Fused: imk_evalnet_forward_select == imk_evalnet_forward_candidates + imk_evalnet_select == itself under IMK_SELECT_SHARED=0 (a child
process), on networks one of whose classes is really gated out.  Argument errors come back before any launch.  Both entry points keep the
buffer contract (tests/arena.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_golden_evalnet_ensemble import cases, meta, select_rule
from test_golden_evalnet_single import gated_scores, load, select_rule_gated
from test_gpu_evalnet_select import make_inputs, make_models

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATED = 2


@pytest.fixture(scope="module")
def ev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from inconsistencymasks_amd import evalnet
    assert evalnet.SELECT_CONF_GATED == GATED
    return evalnet


def _check(got, want, cand_row, what):
    bi, bs, keep, out = got
    assert int(bi) == want[0] and F32(bs).tobytes() == F32(want[1]).tobytes() and int(keep) == int(want[2]), (what, int(bi), float(bs), want)
    assert np.array_equal(out, cand_row[want[0]]), what


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cand_bytes", [16, 64 * 64])
def test_gated_rule_matches_the_recorded_reference(ev, cand_bytes):
    import torch
    d = load()
    rng = np.random.default_rng(11)
    groups = {}
    for c in cases(d, "gat"):
        groups.setdefault(d[c + "_scores"].shape[2], []).append(c)
    assert sorted(groups) == [16, 70]
    for u, cs in sorted(groups.items()):
        # (a) counts given: every case padded to 16 candidates; what lies behind a case's own candidates changes neither gate nor choice
        garbage = np.array([np.nan, np.inf, -np.inf, 1.0, 0.999], F32)
        sc = garbage[rng.integers(0, len(garbage), (1, len(cs), ev.SELECT_MAX_CAND, u))]
        counts = np.zeros(len(cs), np.int32)
        for b, c in enumerate(cs):
            s = d[c + "_scores"]
            sc[:, b, :s.shape[1]] = s
            counts[b] = s.shape[1]
        cand = rng.integers(0, 256, (len(cs), ev.SELECT_MAX_CAND, cand_bytes), dtype=np.uint8)
        for thr in sorted({meta(d, c)[0] for c in cs}):      # one launch per threshold of the group
            got = ev.select_candidates(torch.from_numpy(sc).cuda(), torch.from_numpy(cand).cuda(), thr, GATED, torch.from_numpy(counts).cuda())
            got = [t.cpu().numpy() for t in got]
            for b, c in enumerate(cs):
                want = select_rule_gated(d[c + "_scores"], thr)
                _check([g[b] for g in got], want, cand[b], (c, thr))
                if thr == meta(d, c)[0]:      # the reference's own run of this case
                    assert (int(got[0][b]), int(got[2][b])) == meta(d, c)[2:], c
                    assert got[1][b].tobytes() == d[c + "_given"].astype(F32)[meta(d, c)[2]].tobytes(), c
        # (b) counts NULL: the cases of one M together
        for m in sorted(set(counts.tolist())):
            sub = [c for c in cs if d[c + "_scores"].shape[1] == m]
            s = np.stack([d[c + "_scores"] for c in sub], 1)
            cand_m = rng.integers(0, 256, (len(sub), m, cand_bytes), dtype=np.uint8)
            for thr in sorted({meta(d, c)[0] for c in sub}):
                got = [t.cpu().numpy() for t in ev.select_candidates(torch.from_numpy(s).cuda(), torch.from_numpy(cand_m).cuda(), thr, GATED)]
                for b, c in enumerate(sub):
                    _check([g[b] for g in got], select_rule_gated(d[c + "_scores"], thr), cand_m[b], (c, thr, "all"))
                    if thr == meta(d, c)[0]:
                        assert (int(got[0][b]), int(got[2][b])) == meta(d, c)[2:], c


def test_single_evalnet_iou_rule_matches_the_recorded_reference(ev):
    """the ISIC writer's cases: IMK_SELECT_IOU with N = 1"""
    import torch
    d = load()
    rng = np.random.default_rng(12)
    cs = cases(d, "bin")
    for m in sorted({d[c + "_scores"].shape[1] for c in cs}):
        sub = [c for c in cs if d[c + "_scores"].shape[1] == m]
        s = np.stack([d[c + "_scores"] for c in sub], 1)
        cand = rng.integers(0, 256, (len(sub), m, 16), dtype=np.uint8)
        for thr in sorted({meta(d, c)[0] for c in sub}):
            got = [t.cpu().numpy() for t in ev.select_candidates(torch.from_numpy(s).cuda(), torch.from_numpy(cand).cuda(), thr, ev.SELECT_IOU)]
            for b, c in enumerate(sub):
                _check([g[b] for g in got], select_rule(d[c + "_scores"], thr, False), cand[b], (c, thr))
                if thr == meta(d, c)[0]:
                    assert (int(got[0][b]), int(got[2][b])) == meta(d, c)[2:], c
                    assert got[1][b].tobytes() == d[c + "_given"].astype(F32)[meta(d, c)[2]].tobytes(), c


# ---- random stacks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 8, 35, 64])
def test_random_stacks_match_the_restated_rule(ev, k):
    import torch
    rng = np.random.default_rng(100 + k)
    special = np.array([0.03, np.nextafter(F32(0.03), F32(0)), np.nextafter(F32(0.03), F32(1)), np.nan, 0.0, -0.0, 0.5, 1.0], F32)
    stacks = gated_out = nan_gate = 0
    for n in (1, 3):
        for b, m in ((8, 16), (8, 5), (7, 11), (5, 1), (8, 2), (3, 10)):
            det_scale = rng.choice(np.array([0.02, 0.05, 0.1, 1.0], F32), (1, b, 1, k))      # per class: far below, around and above the gate
            s = rng.random((n, b, m, 2 * k), dtype=F32)
            s[..., k:] *= det_scale
            pick = rng.random(s.shape) < 0.04
            s[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
            same = rng.random((b, m)) < 0.15      # equal rows: ties
            s[:, same] = s[:, np.nonzero(same)[0], 0]
            counts = rng.integers(1, m + 1, b).astype(np.int32)
            cand = rng.integers(0, 256, (b, m, 32), dtype=np.uint8)
            thr = float(rng.choice([0.03, 0.05, 0.3]))
            for cnt in (counts, None):
                got = ev.select_candidates(torch.from_numpy(s).cuda(), torch.from_numpy(cand).cuda(), thr, GATED,
                                           None if cnt is None else torch.from_numpy(cnt).cuda())
                got = [t.cpu().numpy() for t in got]
                for i in range(b):
                    c = None if cnt is None else int(cnt[i])
                    _check([g[i] for g in got], select_rule_gated(s[:, i], thr, c), cand[i], (k, n, b, m, i, c))
                    counting = gated_scores(s[:, i], c)[1]
                    gated_out += len(counting) < k
                    nan_gate += bool(np.isnan(s[:, i, :c, k:]).any())
                    stacks += 1
    assert stacks >= 80 and gated_out > stacks // 4 and nan_gate > 0


# ---- fused ---------------------------------------------------------------------------------------------------------------------------
def gated_models(ev, n, gated_class=2):
    """onehot9-style EvalNets of width 16 whose detection bias of one class is pushed down through state_dict / load_state_dict"""
    models = make_models(ev, 64, 64, 16, "onehot9", n)
    for mod in models:
        sd = mod.state_dict()
        keys = [k for k, v in sd.items() if "detection" in k and v.dim() == 1]
        assert len(keys) == 1 and sd[keys[0]].numel() == 9, keys
        sd[keys[0]] = sd[keys[0]].clone()
        sd[keys[0]][gated_class] = -9.0      # sigmoid(-9 + a small activation) is far below 0.03
        mod.load_state_dict(sd)
        mod.repack()
    return models


def run_fused_gated(ev, dump):
    import torch
    b, m, k = 3, 5, 9
    models = gated_models(ev, 2)
    xa, xb = make_inputs(64, 64, "onehot9", b, m, seed=77)
    cand = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (b, m, 64 * 64), dtype=np.uint8)).cuda()
    counts = torch.from_numpy(np.array([m, m - 1, 2], np.int32)).cuda()
    scorer = ev.CandidateScorer(models)
    composed_scores = scorer.scores(xa, xb)
    s = composed_scores.cpu().numpy()
    best = sorted(float(select_rule_gated(s[:, i], 0.0)[1]) for i in range(b))
    thr = (best[0] + best[1]) / 2 if best[0] != best[1] else best[1]      # some images kept, some not
    for tag, cnt in (("counts", counts), ("all", None)):
        fused = scorer.run(xa, xb, cand, thr, cnt, GATED)
        fused_scores = scorer.last_scores
        composed = ev.select_candidates(composed_scores, cand, thr, GATED, cnt)
        torch.cuda.synchronize()
        assert torch.equal(fused_scores.view(torch.int32), composed_scores.view(torch.int32)), tag
        for f, c, what in zip(fused, composed, ("best_idx", "best_score", "keep", "out")):
            assert torch.equal(f.view(torch.int32) if f.dtype == torch.float32 else f, c.view(torch.int32) if c.dtype == torch.float32 else c), (tag, what)
            dump[f"{tag}_{what}"] = f.cpu().numpy()
        dump[f"{tag}_scores"] = fused_scores.cpu().numpy()
        for i in range(b):      # ... and the restated rule on those scores; the pushed-down class really is gated out, most others count
            c = None if cnt is None else int(cnt[i])
            want = select_rule_gated(s[:, i], thr, c)
            _check([f[i].cpu().numpy() for f in fused], want, cand[i].cpu().numpy(), (tag, i))
            counting = gated_scores(s[:, i], c)[1]
            assert 2 not in counting and len(counting) >= k // 2, (tag, i, counting)


def test_fused_equals_composed_and_repeated_route(ev, tmp_path):
    child = ("import sys, numpy as np\n"
             "sys.path[:0] = [%r, %r]\n"
             "import test_gpu_evalnet_select_gated as T\n"
             "from inconsistencymasks_amd import evalnet\n"
             "dump = {}\n"
             "T.run_fused_gated(evalnet, dump)\n"
             "np.savez(sys.argv[1], **dump)\n") % (ROOT, os.path.join(ROOT, "tests"))
    path = str(tmp_path / "repeated.npz")
    r = subprocess.run([sys.executable, "-c", child, path], env=dict(os.environ, IMK_SELECT_SHARED="0"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.environ.get("IMK_SELECT_SHARED", "1") != "0", "this process must run the shared-tower route"
    fused = {}
    run_fused_gated(ev, fused)
    with np.load(path) as rep:
        assert sorted(rep.files) == sorted(fused)
        for key in fused:
            assert rep[key].tobytes() == fused[key].tobytes(), key
    assert set(np.concatenate([fused["counts_keep"], fused["all_keep"]]).tolist()) == {0, 1}, "both keep values must occur"


# ---- argument errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ev):
    import torch
    from inconsistencymasks_amd._lib import lib
    EINVAL, EUNSUPPORTED = -1, -2
    stream = torch.cuda.current_stream().cuda_stream
    b = 2

    def select(n, m, n_heads, k, mode):
        sc = torch.rand((n, b, m, n_heads * k), device="cuda")
        cand = torch.zeros((b, m, 16), dtype=torch.uint8, device="cuda")
        outs = (torch.full((b,), -7, dtype=torch.int32, device="cuda"), torch.full((b,), -7.0, device="cuda"),
                torch.full((b,), 7, dtype=torch.uint8, device="cuda"), torch.full((b, 16), 7, dtype=torch.uint8, device="cuda"))
        rc = lib.imk_evalnet_select(sc.data_ptr(), n, b, m, n_heads, k, None, cand.data_ptr(), 16, 0.5, mode, outs[0].data_ptr(),
                                    outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), stream)
        torch.cuda.synchronize()
        if rc:      # a refused call has launched nothing
            assert outs[0].tolist() == [-7] * b and outs[1].tolist() == [-7.0] * b and outs[2].tolist() == [7] * b and int(outs[3].min()) == 7
        return rc

    assert select(1, 5, 2, 8, GATED) == 0 and select(8, 16, 2, 64, GATED) == 0
    assert select(1, 5, 1, 8, GATED) == EINVAL and select(1, 5, 1, 1, GATED) == EINVAL      # the rule needs the detection head
    assert select(1, 5, 2, 8, 3) == EINVAL and select(1, 5, 2, 8, -1) == EINVAL
    assert select(1, 17, 2, 8, GATED) == EUNSUPPORTED
    assert select(9, 5, 2, 8, GATED) == EUNSUPPORTED
    assert select(1, 5, 2, 65, GATED) == EUNSUPPORTED

    models = make_models(ev, 64, 64, 16, "one_head", 1)      # a one-head plan: the fused call refuses the mode as well
    scorer = ev.CandidateScorer(models)
    xa, xb = make_inputs(64, 64, "one_head", b, 5, seed=1)
    cand = torch.zeros((b, 5, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(Exception):
        scorer.run(xa, xb, cand, 0.5, None, GATED)
    two = make_models(ev, 64, 64, 16, "onehot9", 1)
    xa, xb = make_inputs(64, 64, "onehot9", b, 5, seed=1)
    with pytest.raises(Exception):
        ev.CandidateScorer(two).run(xa, xb, cand, 0.5, None, 3)
    torch.cuda.synchronize()


# ---- the buffer contract ---------------------------------------------------------------------------------------------------------------
def test_buffer_contract(ev):
    import torch
    from test_gpu_buffer_contract import Arena, L, S, dev, model_specs, ptr_arrays, same
    b, m, k, n = 2, 5, 8, 2
    rng = np.random.default_rng(21)
    cand_bytes = 64 * 64
    cand = dev(rng.integers(0, 256, (b, m, cand_bytes), dtype=np.uint8))
    cnt = dev(np.array([5, 3], np.int32))
    scores = rng.random((n, b, m, 2 * k), dtype=F32)
    scores[..., k:k + 2] *= F32(0.03)      # two classes around and below the gate
    scores[0, 1, 4, k + 3] = np.nan       # behind image 1's count
    scores = dev(scores)
    outs = [("best_idx", b * 4, "out"), ("best_score", b * 4, "out"), ("keep", b, "out"), ("chosen", b * cand_bytes, "out")]
    for counts in (None, cnt):
        specs = [("scores", scores, "in"), ("cand", cand, "in")] + ([("counts", counts, "in")] if counts is not None else [])
        out = Arena(specs + outs, "cuda").check(lambda p: L().imk_evalnet_select(
            p["scores"], n, b, m, 2, k, p["counts"] if counts is not None else None, p["cand"], cand_bytes, 0.3, GATED, p["best_idx"],
            p["best_score"], p["keep"], p["chosen"], S()))
        for key, want in zip(("best_idx", "best_score", "keep", "chosen"), ev.select_candidates(scores, cand, 0.3, GATED, counts)):
            same(out[key], want, key)
        s = scores.cpu().numpy()
        for i in range(b):
            want = select_rule_gated(s[:, i], 0.3, None if counts is None else int(counts[i]))
            assert int(out["best_idx"].view(torch.int32)[i]) == want[0] and int(out["keep"][i]) == int(want[2])

    models = [ev.EvalNet(64, 64, 3, k, k, 1.0, True, True, False, seed=40 + j, b_onehot=True) for j in range(n)]
    plan = models[0].plan
    scorer = ev.CandidateScorer(models)
    xa = dev(rng.integers(0, 256, (b, 64, 64, 3), dtype=np.uint8))
    xb = dev(rng.integers(0, k, (b, m, 64, 64), dtype=np.uint8))
    nws = L().imk_evalnet_forward_candidates_workspace_bytes(plan.ptr, b, m)
    specs = model_specs(models) + [("xa", xa, "in"), ("xb", xb, "in"), ("cand", cand, "in"), ("scores", n * b * m * 2 * k * 4, "out")] + outs

    def call(p):
        pa, pk = ptr_arrays(p, n)
        return L().imk_evalnet_forward_select(plan.ptr, n, pa, pk, p["xa"], p["xb"], b, m, None, p["cand"], cand_bytes, 0.5, GATED,
                                              p["scores"], p["best_idx"], p["best_score"], p["keep"], p["chosen"], p["ws"], nws, S())
    out = Arena(specs + [("ws", nws, "scratch")], "cuda").check(call)
    bi, bs, keep, chosen = scorer.run(xa, xb, cand, 0.5, None, GATED)
    torch.cuda.synchronize()
    for key, want in (("scores", scorer.last_scores), ("best_idx", bi), ("best_score", bs), ("keep", keep), ("chosen", chosen)):
        same(out[key], want, key)
