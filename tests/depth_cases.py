"""The standard-deviation IM of the depth-map family restated with explicit loops (a plain helper module: the fixture maker and the
CPU and GPU tests import it).

get_im_prediction_depth_map is np.std over the models -> threshold_multiplier * np.mean over the image -> `>`.  The restatement spells
out the ORDER in which numpy's float32 add.reduce adds -- no call of np.sum, np.mean, np.std or add.reduce here; `+` between float32
arrays is one IEEE addition per element, so a loop over positions with elementwise adds states an order exactly:

  S(a[0..n)):  n < 8: sequential from the left;  8 <= n <= 128: eight accumulators r[j] = a[j], r[j] += a[i + j] for i = 8, 16, ..
               below n - n % 8, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remaining n % 8 elements sequentially;
               n > 128: S(a[0..n2)) + S(a[n2..n)) with n2 = n / 2, n2 -= n2 % 8
  a whole-array reduction is cut into chunks of 8192 elements: S(chunk 0), then + S(chunk 1), + S(chunk 2) ... sequentially
  per pixel: m = S(p) / N, d_n = p_n - m, std = sqrt(S(d_n * d_n) / N);  per image: thr = float32(mult) * (S_chunked(std) / (H*W))

Three planted defects (the `defect` argument) are what a plausible wrong kernel would compute; the fixture has to tell each apart:
  "no_chunking"        the image sum as one pairwise recursion over all H*W elements
  "sequential_models"  the sums over the models from the left for every N (differs from N = 8 on)
  "fma_squares"        a + d * d contracted into a fused multiply-add (formed here in float64 and rounded once: d * d is exact in
                       float64, and the one extra rounding of the float64 sum does not make it less of a defect)
"""
import numpy as np

F32 = np.float32
CHUNK = 8192
LEAF = 128
DEFECTS = ("no_chunking", "sequential_models", "fma_squares")


def load_cases(path):
    """tests/golden/depth_map.npz -> a list of dicts: name, preds float32 [N,H,W], mults float32 [M], thr_bits uint32 [M],
    masks bool [M,H,W], kinds [M] str (what the multiplier was chosen for)"""
    out = []
    with np.load(path) as d:
        for name in [str(s) for s in d["names"]]:
            n, h, w = (int(v) for v in d[name + "_shape"])
            preds = d[name + "_lut"][d[name + "_codes"]].reshape(n, h, w)
            mults = d[name + "_mults"]
            masks = np.unpackbits(d[name + "_masks"], axis=1)[:, :h * w].astype(bool).reshape(len(mults), h, w)
            out.append({"name": name, "preds": preds, "mults": mults, "thr_bits": d[name + "_thr_bits"], "masks": masks,
                        "kinds": [str(s) for s in d[name + "_kinds"]]})
    return out


def _leaf(a):
    """a [n, ...] float32 with n <= 128, reduced over axis 0"""
    n = a.shape[0]
    if n < 8:
        r = a[0]
        for i in range(1, n):
            r = r + a[i]
        return r
    r = [a[j] for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(n - n % 8, n):
        res = res + a[i]
    return res


def pairwise(a):
    """S over axis 0"""
    n = a.shape[0]
    if n <= LEAF:
        return _leaf(a)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[:n2]) + pairwise(a[n2:])


def chunked(a):
    """a whole-array reduction of a 1-D float32 array"""
    r = pairwise(a[:CHUNK])
    for c in range(CHUNK, a.shape[0], CHUNK):
        r = r + pairwise(a[c:c + CHUNK])
    return r


def _sequential(a):
    r = a[0]
    for i in range(1, a.shape[0]):
        r = r + a[i]
    return r


def _fma_sum_of_squares(d, sequential):
    """S(d * d) with every `acc + d * d` fused; an accumulator's first square is a plain product"""
    n = d.shape[0]
    sq = lambda i: d[i] * d[i]                                                              # noqa: E731
    fma = lambda acc, i: (acc.astype(np.float64) + d[i].astype(np.float64) * d[i].astype(np.float64)).astype(F32)   # noqa: E731
    if n < 8 or sequential:
        r = sq(0)
        for i in range(1, n):
            r = fma(r, i)
        return r
    r = [sq(j) for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = fma(r[j], i + j)
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(n - n % 8, n):
        res = fma(res, i)
    return res


def std_map(preds, defect=None):
    """preds float32 [N, ...] -> the per-pixel standard deviation over axis 0, float32"""
    assert preds.dtype == F32 and defect in (None,) + DEFECTS
    n = preds.shape[0]
    seq = defect == "sequential_models"
    over_models = _sequential if seq else pairwise
    with np.errstate(all="ignore"):
        m = over_models(preds) / F32(n)
        d = preds - m
        ss = _fma_sum_of_squares(d, seq) if defect == "fma_squares" else over_models(d * d)
        return np.sqrt(ss / F32(n))


def threshold(std, mult, defect=None):
    """std float32 [...] (one image) -> float32(mult) * mean, float32"""
    flat = np.ascontiguousarray(std, F32).reshape(-1)
    with np.errstate(all="ignore"):
        total = pairwise(flat) if defect == "no_chunking" else chunked(flat)
        return F32(F32(mult) * F32(total / F32(flat.shape[0])))


def im_depth(preds, mult, defect=None):
    """preds float32 [N,H,W] -> (mask bool [H,W], thr float32, std float32 [H,W])"""
    std = std_map(preds, defect)
    thr = threshold(std, mult, defect)
    with np.errstate(all="ignore"):
        return std > thr, thr, std


def same_bits(a, b):
    """float32 equality by bits, every NaN equal to every NaN (numpy and the GPU hand on different NaN payloads)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
