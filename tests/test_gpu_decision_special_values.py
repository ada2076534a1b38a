"""One table of rows through every arg-max (and threshold) entry point of the library, numpy as the reference, no tolerance.

The reference takes np.argmax wherever it turns class probabilities into a label (functions.py:3225 the IM chain, :1309 the
evaluation, :2438-2566 the model ensemble, :2182-2218 the input ensemble): the first maximum wins and a NaN counts as the maximum,
so the first NaN wins.  rows() holds the rows on which a scan that is not np.argmax gives another class -- NaN at either end and
in the middle, NaN beside +inf, all NaN, all -inf, ties of +inf, of -0.0 with 0.0 and of every entry, a denormal against 0 -- and
every multi-class kernel gets them at every K of the matrix-core tile edge (16 / 17), of both parities of the `K | 1` LDS pitch,
of both sides of the float4 path's `total & 3 == 0` condition and of the K <= 64 ceiling, at 1, 255, 256 and 257 pixels (one
workgroup chunk is 256), some in the last partial chunk, some with the same NaN pattern in every model (numpy then lets the
models agree: IM = 0).  The binary siblings get NaN, +-inf, the threshold and its float32 neighbours at the same pixel counts."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import im_oracle as O  # noqa: E402
from test_golden_model_ensemble import vote_binary_rule, vote_multi_rule  # noqa: E402

F32 = np.float32
KS = (2, 3, 4, 9, 16, 17, 35, 64)
SHAPES = ((1, 1), (3, 85), (16, 16), (257, 1))
NB = ((2, 1), (3, 1), (2, 2), (3, 2))                      # (models, batch)
BLOCKING = ((True, True), (False, True), (True, False), (False, False))
MULTI = [pytest.param(k, hw, i, id=f"K{k}-{hw[0]}x{hw[1]}") for i, (k, hw) in enumerate((k, hw) for k in KS for hw in SHAPES)]


def _blind(row):
    """the scan np.argmax is NOT: start at row[0], strict >.  A NaN at index >= 1 never wins, one at index 0 always does."""
    best, arg = row[0], 0
    for k in range(1, len(row)):
        if row[k] > best:
            best, arg = row[k], k
    return arg


@functools.lru_cache(maxsize=None)
def rows(K):
    """name -> float32 row [K]; the finite filler is quarters in [0, 1] so that ordinary ties stay common"""
    rng = np.random.default_rng(1000 + K)
    nan, inf = F32(np.nan), F32(np.inf)
    mid, last = (K - 1) // 2, K - 1                        # K = 2 has no middle: mid = 0, the NaN is at index 0 there

    def fill():
        return (rng.integers(0, 5, K) / 4).astype(F32)

    t = {}
    t["nan_first"] = fill(); t["nan_first"][0] = nan
    t["nan_last"] = fill(); t["nan_last"][last] = nan
    t["nan_mid_then_larger"] = fill(); t["nan_mid_then_larger"][mid] = nan; t["nan_mid_then_larger"][last] = 9.0
    t["two_nans"] = fill(); t["two_nans"][[mid, last]] = nan
    t["nan_and_inf"] = fill(); t["nan_and_inf"][0] = inf; t["nan_and_inf"][last] = nan
    t["all_nan"] = np.full(K, nan, F32)
    t["all_neg_inf"] = np.full(K, -inf, F32)
    t["inf_twice"] = fill(); t["inf_twice"][[mid, last]] = inf
    t["neg_zero_then_zero"] = np.full(K, -1, F32); t["neg_zero_then_zero"][K // 2 - 1 if K > 2 else 0] = -0.0; t["neg_zero_then_zero"][last] = 0.0
    t["zero_then_neg_zero"] = np.full(K, -1, F32); t["zero_then_neg_zero"][K // 2 - 1 if K > 2 else 0] = 0.0; t["zero_then_neg_zero"][last] = -0.0
    t["denormal_after_zero"] = np.zeros(K, F32); t["denormal_after_zero"][last] = 1e-38
    t["zero_after_denormal"] = np.full(K, -1, F32); t["zero_after_denormal"][0] = 1e-38; t["zero_after_denormal"][last] = 0.0
    t["all_equal"] = np.full(K, 0.25, F32)
    # what the table is for: numpy's answer on each row, and the rows a NaN-blind scan gets wrong
    am = {n: int(np.argmax(r)) for n, r in t.items()}
    assert am["nan_first"] == 0 and am["nan_last"] == last and am["nan_mid_then_larger"] == mid and am["nan_and_inf"] == last
    assert am["all_nan"] == 0 and am["all_neg_inf"] == 0 and am["all_equal"] == 0 and am["inf_twice"] == mid
    assert am["two_nans"] == mid
    assert am["neg_zero_then_zero"] == am["zero_then_neg_zero"] == (K // 2 - 1 if K > 2 else 0)
    assert am["denormal_after_zero"] == last and am["zero_after_denormal"] == 0 and 0 < t["denormal_after_zero"][last] < np.finfo(F32).tiny
    wrong = {n for n, r in t.items() if _blind(r) != am[n]}
    assert {"nan_last", "nan_and_inf"} <= wrong and (K == 2 or {"nan_mid_then_larger", "two_nans"} <= wrong), wrong
    return t


@functools.lru_cache(maxsize=None)
def stack(K, H, W, N, B):
    """probs [N,B,H,W,K] float32 (read-only), same [B,H*W] bool: pixels where every model holds the same table row"""
    rng = np.random.default_rng(K * 100003 + H * 1009 + W * 31 + N * 7 + B)
    table = list(rows(K).values())
    S, hw = len(table), H * W
    base = rng.integers(0, 5, (1, B, hw, K))
    own = rng.integers(0, 5, (N, B, hw, K))
    p = (np.where(rng.random((N, B, hw, K)) < 0.15, own, base) / 4).astype(F32)
    pixels = range(hw) if hw <= 3 * S else list(range(S)) + list(range(hw - 2 * S, hw))      # the head and the last (partial) chunk
    same = np.zeros((B, hw), bool)
    used = set()
    rot = 7 * (N - 2)
    for b in range(B):
        for px in pixels:
            same[b, px] = (px + b) % 2 == 0
            for n in range(N):
                i = (px + 3 * b + rot + (0 if same[b, px] else 4 * n)) % S
                p[n, b, px] = table[i]
                used.add(i)
    assert hw < S or used == set(range(S))
    p = p.reshape(N, B, H, W, K)
    p.setflags(write=False)
    same.setflags(write=False)
    return p, same


@functools.lru_cache(maxsize=None)
def labels(K, H, W, N, B):
    lab = np.argmax(stack(K, H, W, N, B)[0], -1)           # [N,B,H,W]: the reference's labels
    lab.setflags(write=False)
    return lab


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()            # a copy: the cached inputs are read-only


def _np(t):
    return t.cpu().numpy()


# ---- multi-class: the IM chain -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,hw,idx", MULTI)
def test_im_multiclass(K, hw, idx):
    from inconsistencymasks_amd import im
    H, W = hw
    seen_blocking = set()
    for j, (N, B) in enumerate(NB):
        probs, same = stack(K, H, W, N, B)
        bi, bo = BLOCKING[(idx + j) % 4]
        seen_blocking.add((bi, bo))
        c = (1, 3)[(idx + j) % 2]
        img = np.random.default_rng(idx * 4 + j).integers(1, 256, (B, H, W, c)).astype(np.uint8)
        r = im.im_multiclass(_dev(probs), _dev(img), bi, bo)
        for b in range(B):
            e = O.im_multiclass(probs[:, b])
            assert not e["im"].ravel()[same[b]].any()                                  # the same row in every model: they agree
            eimg, (efinal,) = O.block(img[b], [e["final"]], e["im"], bi, bo)
            where = (K, hw, N, B, b)
            assert np.array_equal(_np(r["final"])[b], efinal), where
            assert np.array_equal(_np(r["im"])[b], e["im"]), where
            assert int(r["im_size"][b]) == int(e["im_size"]), where
            assert np.array_equal(_np(r["presence"])[:, b], e["presence"]), where
            assert np.array_equal(_np(r["img_out"])[b], eimg), where
    assert len(seen_blocking) == 4


# ---- multi-class: the evaluation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,hw,idx", MULTI)
def test_eval_multiclass(K, hw, idx):
    from inconsistencymasks_amd import evaluate as E, functions as F
    H, W = hw
    for N, B in NB:
        probs, _ = stack(K, H, W, N, B)
        lab = labels(K, H, W, N, B)
        rng = np.random.default_rng(idx * 8 + N * 2 + B)
        for n in (0, N - 1):
            want = lab[n].astype(np.uint8)
            gt = np.where(rng.random((B, H, W)) < 0.6, want, rng.integers(0, K + 1, (B, H, W))).astype(np.uint8)   # K: an id never predicted
            pred, counts = E.eval_multiclass(_dev(probs[n]), _dev(gt))
            where = (K, hw, N, B, n)
            assert np.array_equal(_np(pred), want), where
            for b in range(B):
                hit = want[b] == gt[b]
                assert np.array_equal(counts[b, 0], np.bincount(gt[b].ravel(), minlength=256)), where
                assert np.array_equal(counts[b, 1], np.bincount(want[b].ravel(), minlength=256)), where
                assert np.array_equal(counts[b, 2], np.bincount(gt[b][hit].ravel(), minlength=256)), where
                assert int(counts[b, 3, 0]) == int(hit.sum()), where
                pa, iou = E.pa_iou_from_counts(counts[b], gt[b].size)
                assert pa == F.pixel_accuracy(want[b], gt[b]) and iou == F.get_IoU_multi_unique(want[b], gt[b]), where


# ---- multi-class: the model-ensemble and input-ensemble votes --------------------------------------------------------------------
@pytest.mark.parametrize("K,hw,idx", MULTI)
def test_vote_multiclass(K, hw, idx):
    from inconsistencymasks_amd import vote
    H, W = hw
    for N, B in NB:
        probs, _ = stack(K, H, W, N, B)
        d = _dev(probs)
        lab = labels(K, H, W, N, B)
        for soft in (False, True):
            with np.errstate(invalid="ignore"):                                         # inf - inf, NaN sums: the values under test
                want = vote_multi_rule(probs, soft)
            if not soft:
                assert np.array_equal(want, np.where(np.all(lab == lab[0], 0), lab[0], 0))       # the written-out rule IS np.argmax
            assert np.array_equal(_np(vote.vote_multiclass(d, soft)), want), (K, hw, N, B, soft)


@pytest.mark.parametrize("K,hw,idx", MULTI)
def test_vote_views_majority(K, hw, idx):
    from inconsistencymasks_amd import input_ensemble as ie
    H, W = hw
    for N, B in NB:
        probs, _ = stack(K, H, W, N, B)
        lab = labels(K, H, W, N, B)                                                      # the per-view np.argmax
        votes = (lab[..., None] == np.arange(K)).sum(0)                                 # np.bincount per pixel
        want = np.argmax(votes, -1).astype(np.uint8)                                    # ties go to the smallest label
        assert np.array_equal(_np(ie.vote_views_majority(_dev(probs))), want), (K, hw, N, B)


# ---- the binary siblings ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def binary_stack(H, W, N, B, kb, thr):
    rng = np.random.default_rng(H * 1009 + W * 31 + N * 7 + B + kb * 3 + int(thr * 100))
    t = F32(thr)
    base = rng.random((1, B, H, W, kb), dtype=np.float32)
    p = np.clip(base + (rng.random((N, B, H, W, kb), dtype=np.float32) - 0.5) * 0.3, 0, 1).astype(F32)
    pool = np.array([np.nan, np.inf, -np.inf, t, np.nextafter(t, F32(0)), np.nextafter(t, F32(1))], F32)
    flat = p.reshape(-1)
    flat[np.arange(flat.size) % 3 == 0] = pool[rng.integers(0, len(pool), (flat.size + 2) // 3)]
    p[:, 0, H - 1, W - 1, :] = t                           # every model on the threshold at the last pixel (the partial chunk) of image 0
    if H * W >= 255:
        for v in pool[1:]:
            assert (p == v).any()
        assert np.isnan(p).any()
    p.setflags(write=False)
    return p


def _bc(gt, pr):
    gn, p, gh = gt != 0, pr != 0, gt >= 128
    return [int((gn & p).sum()), int((gn | p).sum()), int(gh.sum()), int(p.sum()), int((gh & p).sum())]


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_eval_binary(hw, thr):
    from inconsistencymasks_amd import evaluate as E, functions as F
    H, W = hw
    for N, B in NB:
        probs = binary_stack(H, W, N, B, 1, thr)[N - 1, ..., 0]                          # [B,H,W]
        gt = np.random.default_rng(B).choice(np.array([0, 1, 127, 128, 255], np.uint8), (B, H, W))
        for ge in (False, True):
            with np.errstate(invalid="ignore"):
                want = ((probs >= F32(thr)) if ge else (probs > F32(thr))).astype(np.uint8) * 255
            pred, counts = E.eval_binary(_dev(probs), _dev(gt), thr, ge)
            assert np.array_equal(_np(pred), want), (hw, thr, N, B, ge)
            for b in range(B):
                assert counts[b].tolist() == _bc(gt[b], want[b]), (hw, thr, N, B, ge)
                iou, dice = E.iou_dice_from_counts(counts[b])
                assert iou == F.get_IoU_binary(gt[b], want[b]) and float(dice) == float(F.dice_score_numpy_binary(gt[b], want[b]))


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_vote_binary(hw, thr):
    from inconsistencymasks_amd import vote
    H, W = hw
    for N, B in NB:
        for kb in (1, 3):
            preds = binary_stack(H, W, N, B, kb, thr)
            d = _dev(preds)
            for soft in (False, True):
                with np.errstate(invalid="ignore"):
                    want = vote_binary_rule(preds, thr, soft)                             # [B,H,W,kb]
                got = _np(vote.vote_binary(d, thr, soft))                                 # [B,kb,H,W]
                assert np.array_equal(got, want.transpose(0, 3, 1, 2)), (hw, thr, N, B, kb, soft)


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("thr", [0.5, 0.3])
def test_vote_views_binary(hw, thr):
    from inconsistencymasks_amd import input_ensemble as ie
    H, W = hw
    for N, B in NB:
        for kb in (1, 3):
            preds = binary_stack(H, W, N, B, kb, thr)
            d = _dev(preds)
            for ge in (True, False):
                with np.errstate(invalid="ignore"):
                    on = np.all((preds >= F32(thr)) if ge else (preds > F32(thr)), 0)     # the comparison is made in float32
                want = np.where(on, 255, 0).astype(np.uint8).transpose(0, 3, 1, 2)
                assert np.array_equal(_np(ie.vote_views_binary(d, None, thr, ge)), want), (hw, thr, N, B, kb, ge)


# ---- the all-NaN row through the fused head + IM kernel ----------------------------------------------------------------------
@pytest.mark.parametrize("K,alpha", [(9, 0.5), (35, 1.0)], ids=["K9-one-class-tile", "K35-three-class-tiles"])
def test_all_nan_rows_fused_and_unfused(K, alpha):
    """One NaN in a model's output-layer bias makes every softmax row of that model NaN; numpy's label is then 0 everywhere.  The
    fused head + IM kernel (its own arg-max on the matrix-core layout), the unfused route (predict_device -> im_multiclass) and the
    oracle on the predict_device outputs must agree bit for bit, whichever position the NaN model has in the ensemble."""
    from inconsistencymasks_amd import functions as F, im
    from inconsistencymasks_amd.unet import UNet
    H = W = 32
    models = [UNet(H, W, 3, K, alpha, "softmax", seed=40 + j) for j in range(2)]
    head = [l for l in models[1].plan.layers if l["kind"] == 0][-1]
    assert head["ksize"] == 1 and head["cout"] == K
    sd = models[1].state_dict()
    sd[head["name"] + ".b"][K // 2] = float("nan")
    models[1].load_state_dict(sd)
    x = np.random.default_rng(K).integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    xd = _dev(x)
    for order in ((0, 1), (1, 0)):
        ms = [models[i] for i in order]
        probs = torch.stack([m.predict_device(xd) for m in ms], 0).contiguous()          # [2,B,H,W,K]
        pn = _np(probs)
        nan_at = order.index(1)
        assert np.isnan(pn[nan_at]).all() and np.isfinite(pn[1 - nan_at]).all()
        fused = F.EnsembleIM(ms).run(xd, 0.5, False, True, True, want_presence=True)
        unfused = im.im_multiclass(probs, xd, True, True)
        for b in range(x.shape[0]):
            e = O.im_multiclass(pn[:, b])
            other = np.argmax(pn[1 - nan_at, b], -1)
            assert np.array_equal(e["im"], np.where(other == 0, 0, 255)) and e["im"].any()       # the NaN model says class 0 everywhere
            eimg, (efinal,) = O.block(x[b], [e["final"]], e["im"], True, True)
            for name, r, final, size in (("fused", fused, fused["masks"][b, 0], fused["im_size"][b, 0]),
                                         ("unfused", unfused, unfused["final"][b], unfused["im_size"][b])):
                assert np.array_equal(_np(final), efinal), (name, order, b)
                assert np.array_equal(_np(r["im"])[b], e["im"]), (name, order, b)
                assert int(size) == int(e["im_size"]), (name, order, b)
                assert np.array_equal(_np(r["presence"])[:, b], e["presence"]), (name, order, b)
                assert np.array_equal(_np(r["img_out"])[b], eimg), (name, order, b)
