"""Host side of the evaluation kernels (csrc/imk_eval.hip): integer pixel counts on the GPU, the reference's float
expressions on the host (functions.py:1767-1861), so every metric value is bit-identical to the numpy loop."""
import numpy as np
import torch

from ._lib import check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def eval_binary(probs, gt, thr=0.5, cmp_ge=False, want_pred=True):
    """probs [B,H,W] or [B,H,W,1] f32 cuda, gt [B,H,W] u8 cuda -> (pred u8 {0,255} cuda | None, counts [B,5] int64 numpy)."""
    if probs.dim() == 4:
        assert probs.shape[3] == 1
        probs = probs[..., 0]
    probs, gt = probs.contiguous(), gt.contiguous()
    assert probs.is_cuda and probs.dtype == torch.float32 and gt.dtype == torch.uint8 and gt.shape == probs.shape
    B, H, W = probs.shape
    pred = torch.empty((B, H, W), dtype=torch.uint8, device=probs.device) if want_pred else None
    counts = torch.empty((B, 5), dtype=torch.int64, device=probs.device)
    check(lib.imk_eval_binary(probs.data_ptr(), float(thr), int(bool(cmp_ge)), gt.data_ptr(), B, H, W,
                              pred.data_ptr() if want_pred else None, counts.data_ptr(), _stream()), "imk_eval_binary")
    return pred, counts.cpu().numpy()


def iou_dice_from_counts(c, smooth=1):
    """get_IoU_binary (functions.py:1767-1788) and dice_score_numpy_binary (:1837-1861) from one image's counts."""
    inter, union, g, p, gp = (int(v) for v in c)
    iou = np.int64(inter) / (np.int64(union) + 1e-7)
    f = np.float32
    dice = (2.0 * f(gp) + smooth) / ((f(g) + f(p)) + smooth)     # float32 sums of 0/1 arrays are exact integers
    return iou, dice


def eval_multiclass(probs, gt, want_pred=True):
    """probs [B,H,W,K] f32 cuda, gt [B,H,W] u8 cuda -> (pred u8 class ids cuda | None, counts [B,4,256] int64 numpy)."""
    probs, gt = probs.contiguous(), gt.contiguous()
    assert probs.is_cuda and probs.dtype == torch.float32 and gt.dtype == torch.uint8 and gt.shape == probs.shape[:3]
    B, H, W, K = probs.shape
    pred = torch.empty((B, H, W), dtype=torch.uint8, device=probs.device) if want_pred else None
    counts = torch.empty((B, 4, 256), dtype=torch.int64, device=probs.device)
    check(lib.imk_eval_multiclass(probs.data_ptr(), gt.data_ptr(), B, H, W, K, pred.data_ptr() if want_pred else None,
                                  counts.data_ptr(), _stream()), "imk_eval_multiclass")
    return pred, counts.cpu().numpy()


def pa_iou_from_counts(c, n_pix):
    """pixel_accuracy (functions.py:1820-1834) and get_IoU_multi_unique (:1791-1816) from one image's counts."""
    n_gt, n_pr, n_both = c[0], c[1], c[2]
    pa = np.int64(c[3, 0]) / np.int64(n_pix)
    classes = np.nonzero(n_gt)[0]            # np.unique(gt), ascending
    total = 0.0
    for i in classes:
        total += np.int64(n_both[i]) / ((np.int64(n_gt[i]) + np.int64(n_pr[i]) - np.int64(n_both[i])) + 1e-7)
    return pa, total / len(classes)


def label_counts(pred, gt, im=None, image=None, pred_blocked=None):
    """imk_label_counts: pred, gt [B,H,W] u8 cuda class ids; im [B,H,W] u8 cuda or None -- where im > 0 the prediction counts as
    class 0, `image` [B,H,W,c] u8 cuda (c = 1 or 3), if given, is zeroed there IN PLACE, and `pred_blocked` receives the blocked
    prediction: a uint8 tensor [B,H,W] (it may be `pred` itself), or True for a new one.
    -> (blocked prediction cuda | None, counts [B,4,256] int64 numpy: #(gt == v), #(p' == v), #(gt == v & p' == v), #(gt == v & im == 0))."""
    assert pred.is_cuda and pred.dtype == torch.uint8 and pred.dim() == 3 and pred.is_contiguous()
    assert gt.is_cuda and gt.dtype == torch.uint8 and gt.shape == pred.shape and gt.is_contiguous()
    B, H, W = pred.shape
    c = 0
    if im is not None:
        assert im.is_cuda and im.dtype == torch.uint8 and im.shape == pred.shape and im.is_contiguous()
    if image is not None:
        assert image.is_cuda and image.dtype == torch.uint8 and image.dim() == 4 and image.shape[:3] == pred.shape and image.is_contiguous()
        c = image.shape[3]
    if pred_blocked is True:
        pred_blocked = torch.empty_like(pred)
    if pred_blocked is not None:
        assert pred_blocked.is_cuda and pred_blocked.dtype == torch.uint8 and pred_blocked.shape == pred.shape and pred_blocked.is_contiguous()
    counts = torch.empty((B, 4, 256), dtype=torch.int64, device=pred.device)
    check(lib.imk_label_counts(pred.data_ptr(), gt.data_ptr(), im.data_ptr() if im is not None else None,
                               image.data_ptr() if image is not None else None, c, B, H, W,
                               pred_blocked.data_ptr() if pred_blocked is not None else None, counts.data_ptr(), _stream()),
          "imk_label_counts")
    return pred_blocked, counts.cpu().numpy()


def iou_multi_unique_from_counts(counts, unique_of):
    """get_IoU_multi_unique (functions.py:1791-1816) from one image's label counts [4,256]: the mean, over the classes present in one of
    the two maps, of inter / (union + 1e-7).  unique_of names the map whose classes count: "gt", or "pred" -- the blocked prediction,
    class 0 included as soon as one pixel is blocked.  The training-data writers call get_IoU_multi_unique(mask_gray, mask_pred), the
    ground truth in the `pred` seat (functions.py:3550, 3747): their labels are unique_of="pred"."""
    if unique_of not in ("pred", "gt"):
        raise ValueError(f"unique_of must be 'pred' or 'gt', got {unique_of!r}")
    c = np.asarray(counts, dtype=np.int64)
    n_gt, n_pr, n_both = c[0], c[1], c[2]
    iou_list = []
    for v in np.nonzero(n_pr if unique_of == "pred" else n_gt)[0]:      # np.unique: ascending
        union = n_gt[v] + n_pr[v] - n_both[v]
        iou_list.append(n_both[v] / (union + 1e-7))
    return sum(iou_list) / len(iou_list)


def soft_sums(probs, gt, mode):
    """Validation-monitor reductions on the device (imk_eval_soft_sums), deterministic.
    mode 0: probs [..., K] f32, gt [...] u8 class ids -> float64 numpy [3, K] = (sum [gt == k] p_k, sum [gt == k], sum p_k)
    mode 1: probs [..., K] f32, gt [..., K] u8 targets -> float64 sum of squared errors"""
    probs, gt = probs.contiguous(), gt.contiguous()
    K = probs.shape[-1]
    n_pix = probs.numel() // K
    assert probs.is_cuda and probs.dtype == torch.float32 and gt.dtype == torch.uint8
    assert gt.numel() == (n_pix if mode == 0 else n_pix * K)
    out = torch.empty(lib.imk_eval_soft_out_doubles(K), dtype=torch.float64, device=probs.device)
    check(lib.imk_eval_soft_sums(probs.data_ptr(), gt.data_ptr(), n_pix, K, int(mode), out.data_ptr(), _stream()),
          "imk_eval_soft_sums")
    res = out[:3 * K].cpu().numpy()
    return res.reshape(3, K) if mode == 0 else float(res[0])


def dice_sums(probs, gt):
    """The per-image sums of the reference's dice_loss (functions.py:162-184) on the device (imk_eval_dice_sums), deterministic:
    probs [B,H,W,K] f32 cuda, gt [B,H,W,K] u8 cuda targets -> float64 numpy [B,3] = (sum t p, sum t, sum p).  An image's row does not
    depend on the batch it is in."""
    probs, gt = probs.contiguous(), gt.contiguous()
    assert probs.is_cuda and probs.dtype == torch.float32 and gt.dtype == torch.uint8 and probs.dim() == 4 and gt.shape == probs.shape
    B, H, W, K = probs.shape
    out = torch.empty((B, 3), dtype=torch.float64, device=probs.device)
    check(lib.imk_eval_dice_sums(probs.data_ptr(), gt.data_ptr(), B, H, W, K, out.data_ptr(), _stream()), "imk_eval_dice_sums")
    return out.cpu().numpy()


def dice_from_sums(sums, smooth=1):
    """dice_b = (2 I_b + smooth) / (U_b + smooth) per row of dice_sums' result, in float64"""
    sums = np.asarray(sums, dtype=np.float64)
    return (2.0 * sums[:, 0] + smooth) / (sums[:, 1] + sums[:, 2] + smooth)
