"""imk_eval_depth against numpy float32: benchmark_depth_map's PNG rule (clip(p * 255, 0, 255) truncated, NaN -> 0) and delta_metric's
count exactly, the squared-error sums within 1e-12 relative of the same float32 differences summed in float64 (the kernel squares and
adds in double in a fixed order: only the order of double additions differs)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from inconsistencymasks_amd import depth as D  # noqa: E402

F32 = np.float32


def reference(p, g):
    """p float32 [B,H,W], g uint8 [B,H,W] -> (pred u8, squared-error sums float64 [B], delta counts int [B])"""
    with np.errstate(all="ignore"):
        y = g.astype(F32) / F32(255.0)
        e = (p - y).astype(F32)
        sq = (e.astype(np.float64) ** 2).reshape(len(p), -1).sum(1)
        ratio = np.maximum(p / y, y / p)                       # NaN if either is (tf.maximum)
        hits = (ratio < F32(1.25)).reshape(len(p), -1).sum(1)
        s = np.clip(p * F32(255.0), 0, 255)
        pred = np.where(np.isnan(s), F32(0), s).astype(np.uint8)      # truncation toward zero
    return pred, sq, hits


def special_values():
    """0, 1, NaN, p * 255 at exact integers and one ulp either side, y = 0, ratios at 1.25 and one ulp either side, out of range"""
    p, g = [], []
    for k in (0, 1, 2, 127, 128, 254, 255):
        v = F32(k) / F32(255.0)
        for q in (v, np.nextafter(v, F32(2)), np.nextafter(v, F32(-1))):
            p.append(q); g.append(k)
    for k in (1, 51, 100, 204, 255):
        y = F32(k) / F32(255.0)
        for f in (F32(1.25), np.nextafter(F32(1.25), F32(2)), np.nextafter(F32(1.25), F32(0)), F32(0.8), np.nextafter(F32(0.8), F32(1))):
            p.append(F32(y * f)); g.append(k)
            p.append(F32(y / f)); g.append(k)
    for v, k in ((0.0, 0), (1.0, 255), (0.0, 255), (1.0, 0), (np.nan, 0), (np.nan, 200), (0.5, 0), (-0.25, 10), (1.5, 250), (np.inf, 3),
                 (-np.inf, 3), (-0.0, 0), (1e-30, 1), (0.999999, 255), (1.0000001, 255), (255.5 / 255, 255), (0.9999 / 255, 0)):
        p.append(F32(v)); g.append(k)
    return np.array(p, F32), np.array(g, np.uint8)


@pytest.mark.parametrize("shape", [(1, 16, 16), (3, 37, 51), (2, 96, 96)])
def test_eval_depth_against_numpy(shape):
    b, h, w = shape
    rng = np.random.default_rng(h)
    p = (rng.random(shape, dtype=F32) * F32(1.1) - F32(0.05)).astype(F32)
    g = rng.integers(0, 256, shape, dtype=np.uint8)
    near = rng.random(shape) < 0.3                              # a share of predictions close to their targets: ratios around 1.25
    p[near] = (g[near].astype(F32) / F32(255.0) * (F32(0.75) + F32(0.55) * rng.random(int(near.sum()), dtype=F32))).astype(F32)
    sp, sg = special_values()
    assert sp.size <= h * w
    p.reshape(b, -1)[0, :sp.size] = sp
    g.reshape(b, -1)[0, :sg.size] = sg
    pred_want, sq_want, hits_want = reference(p, g)
    assert 0 < hits_want.sum() < p.size
    for probs, gt in ((torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()),
                      (torch.from_numpy(p[..., None]).cuda(), torch.from_numpy(g[..., None]).cuda())):
        pred, sums = D.eval_depth(probs, gt)
        assert np.array_equal(pred.cpu().numpy(), pred_want)
        assert np.array_equal(sums[:, 1], hits_want.astype(np.float64))
        finite = np.isfinite(sq_want)
        assert np.array_equal(np.isnan(sums[:, 0]), np.isnan(sq_want)) and np.array_equal(np.isinf(sums[:, 0]), np.isinf(sq_want))
        assert np.all(np.abs(sums[finite, 0] - sq_want[finite]) <= 1e-12 * sq_want[finite]), (sums[:, 0], sq_want)
    none, sums2 = D.eval_depth(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), want_pred=False)
    assert none is None and np.array_equal(sums2[:, 1], sums[:, 1]) and np.array_equal(sums2[finite, 0], sums[finite, 0])


def test_finite_sums_and_reproducibility():
    """without the special values every sum is finite and two calls give the same bits (a fixed summation order)"""
    rng = np.random.default_rng(1)
    p, g = rng.random((4, 64, 80), dtype=F32), rng.integers(0, 256, (4, 64, 80), dtype=np.uint8)
    _, sq_want, hits_want = reference(p, g)
    a = D.eval_depth(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda())[1]
    b = D.eval_depth(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda())[1]
    assert np.array_equal(a, b) and np.array_equal(a[:, 1], hits_want)
    assert np.all(np.abs(a[:, 0] - sq_want) <= 1e-12 * sq_want)
