"""The label of the scalar-IoU multiclass EvalNet family, restated in numpy with explicit loops (a plain helper module): what
imk_label_counts has to leave and what the writers make of it.  Imported by tests/test_cpu_label_cases.py (against the recorded
reference run, tests/golden/evalnet_scalar.npz), tests/test_gpu_label_counts.py (against the kernel) and the fixture's maker.

    counts[0][v] = #(gt == v)    counts[1][v] = #(p' == v)    counts[2][v] = #(gt == v and p' == v)    counts[3][v] = #(gt == v and im == 0)

with p' the prediction whose blocked pixels (im > 0) are class 0.  The label is the reference's get_IoU_multi_unique(gt, p')
(functions.py:1791-1816 as its writers call it, functions.py:3550, 3747): the ground truth sits in the `pred` seat, so the classes that
count are those of p'."""
import numpy as np


def block(pred, im=None, image=None):
    """-> (p', the blocked image or None): the writers' `image[im > 0] = 0; pred[im > 0] = 0` (functions.py:3739-3744)"""
    pred = np.array(pred, np.uint8)
    image = None if image is None else np.array(image, np.uint8)
    if im is not None:
        for y in range(pred.shape[0]):
            for x in range(pred.shape[1]):
                if im[y, x] > 0:
                    pred[y, x] = 0
                    if image is not None:
                        image[y, x] = 0
    return pred, image


def counts(pred, gt, im=None):
    """int64 [4,256] of one image, pixel by pixel"""
    c = np.zeros((4, 256), np.int64)
    blocked, _ = block(pred, im)
    for y in range(gt.shape[0]):
        for x in range(gt.shape[1]):
            g, p = int(gt[y, x]), int(blocked[y, x])
            c[0, g] += 1
            c[1, p] += 1
            if g == p:
                c[2, g] += 1
            if im is None or im[y, x] == 0:
                c[3, g] += 1
    return c


def label(c, unique_of="pred"):
    """get_IoU_multi_unique from the counts of one image, with the reference's own float expressions: numpy int64 intersection over
    (numpy int64 union + 1e-7), Python's sum of the list in ascending class order, over the number of classes"""
    c = np.asarray(c, np.int64)
    present = c[1] if unique_of == "pred" else c[0]
    iou_list = []
    for v in range(256):
        if present[v] > 0:
            inter = c[2, v]
            union = c[0, v] + c[1, v] - c[2, v]
            iou_list.append(inter / (union + 1e-7))
    return sum(iou_list) / len(iou_list)


def rounded(c, unique_of="pred"):
    """the labels.csv value: round(np.float64, 4) -- numpy's rounding, which is not Python's on a decimal half"""
    return round(label(c, unique_of), 4)


def num_augs(pred_iou, min_threshold, max_threshold):
    """functions.py:5816-5825 on predict()'s float32 value: the comparisons, the difference and the quotient are float32"""
    f = np.float32
    v = f(pred_iou)
    step = f((max_threshold - min_threshold) / 5)
    if v > f(max_threshold):
        n = 5
    elif v > f(min_threshold):
        n = 1 + int((v - f(min_threshold)) / step)
    else:
        n = 1
    return min(n, 5)


def select(scores, threshold):
    """the two selection writers (functions.py:5223-5226, 5304-5312) on scores float32 [N,M]: np.mean over the EvalNets (N = 1: the one
    net's own values), np.argmax, best >= threshold in float32 -> (index, best, keep)"""
    s = np.asarray(scores, np.float32)
    mean = s[0] if s.shape[0] == 1 else np.mean(s, axis=0)
    best = int(np.argmax(mean))
    return best, mean[best], bool(mean[best] >= np.float32(threshold))


def pred_name(imagename, i):
    """functions.py:3541-3547"""
    if i >= 10 and "aug" in imagename:
        return f"{imagename[:-10]}___{i}_{imagename[-6:-4]}.png"
    return f"{imagename[:-4]}___{i}.png"


def case_maps(h, w, batch, seed, ids=9, im_value=None, full_range=False):
    """class-id maps in blocks with a few stray pixels, and (im_value given) an IM of that value: pred, gt, im or None, u8 [B,H,W]"""
    rng = np.random.default_rng(seed)
    hi = 256 if full_range else ids
    coarse = lambda: rng.integers(0, hi, (batch, (h + 3) // 4, (w + 3) // 4)).astype(np.uint8).repeat(4, 1).repeat(4, 2)[:, :h, :w]
    gt = np.ascontiguousarray(coarse())
    pred = np.where(rng.random((batch, h, w)) < 0.7, gt, coarse()).astype(np.uint8)
    stray = rng.random((batch, h, w)) < 0.05
    pred[stray] = rng.integers(0, hi, int(stray.sum())).astype(np.uint8)
    im = None
    if im_value is not None:
        im = ((rng.random((batch, h, w)) < 0.2) * im_value).astype(np.uint8)
    return np.ascontiguousarray(pred), gt, im
