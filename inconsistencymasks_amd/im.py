"""Host wrappers of the fused IM kernels (imk_im_binary / imk_im_multiclass / imk_morph / imk_block_apply and their per-image
forms imk_im_binary_members / imk_im_multiclass_members / imk_morph_var).  torch is used for device memory and streams only."""
import numpy as np
import torch

from ._lib import check, lib


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_u8(x, device):
    if x is None:
        return None
    t = torch.as_tensor(x)
    if t.dtype != torch.uint8:
        raise TypeError("images must be uint8")
    return t.to(device).contiguous()


def _words(members, batch, n_models, device):
    """the member words on the device (int32 view of member_words), or None for the whole ensemble"""
    return None if members is None else torch.from_numpy(member_words(members, batch, n_models).view(np.int32)).to(device)


def _im_binary(preds, members, thr, cmp_ge, img, block_in, block_out):
    if preds.dtype != torch.float32 or preds.dim() != 5 or not preds.is_cuda:
        raise TypeError("preds must be a float32 CUDA tensor [N,B,H,W,Kb]")
    preds = preds.contiguous()
    n, b, h, w, kb = preds.shape
    dev = preds.device
    words = _words(members, b, n, dev)
    img = _dev_u8(img, dev)
    c = 0 if img is None else img.shape[-1]
    masks = torch.empty((b, kb, h, w), dtype=torch.uint8, device=dev)
    im = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    im_size = torch.empty((b, kb), dtype=torch.int64, device=dev)
    pred_size = torch.empty((b, kb), dtype=torch.int64, device=dev)
    img_out = None if img is None else torch.empty_like(img)
    tail = (n, b, h, w, kb, float(thr), int(bool(cmp_ge)), _ptr(img), c, int(bool(block_in)), int(bool(block_out)),
            _ptr(img_out), masks.data_ptr(), im.data_ptr(), im_size.data_ptr(), pred_size.data_ptr(), _stream())
    if words is None:
        check(lib.imk_im_binary(preds.data_ptr(), *tail), "imk_im_binary")
    else:
        check(lib.imk_im_binary_members(preds.data_ptr(), words.data_ptr(), *tail), "imk_im_binary_members")
    return {"masks": masks, "im": im, "im_size": im_size, "pred_size": pred_size, "img_out": img_out}


def _im_multiclass(probs, members, img, block_in, block_out, want_presence):
    if probs.dtype != torch.float32 or probs.dim() != 5 or not probs.is_cuda:
        raise TypeError("probs must be a float32 CUDA tensor [N,B,H,W,K]")
    probs = probs.contiguous()
    n, b, h, w, k = probs.shape
    dev = probs.device
    words = _words(members, b, n, dev)
    img = _dev_u8(img, dev)
    c = 0 if img is None else img.shape[-1]
    final = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    im = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    im_size = torch.empty((b,), dtype=torch.int64, device=dev)
    presence = torch.empty((n, b, k), dtype=torch.uint8, device=dev) if want_presence else None
    img_out = None if img is None else torch.empty_like(img)
    tail = (n, b, h, w, k, _ptr(img), c, int(bool(block_in)), int(bool(block_out)), _ptr(img_out),
            final.data_ptr(), im.data_ptr(), im_size.data_ptr(), _ptr(presence), _stream())
    if words is None:
        check(lib.imk_im_multiclass(probs.data_ptr(), *tail), "imk_im_multiclass")
    else:
        check(lib.imk_im_multiclass_members(probs.data_ptr(), words.data_ptr(), *tail), "imk_im_multiclass_members")
    return {"final": final, "im": im, "im_size": im_size, "presence": presence, "img_out": img_out}


def im_binary(preds, thr=0.5, cmp_ge=False, img=None, block_in=True, block_out=True):
    """preds float32 [N,B,H,W,Kb] (device) -> dict of device tensors:
    masks [B,Kb,H,W] u8, im [B,H,W] u8, im_size [B,Kb] i64, pred_size [B,Kb] i64, img_out [B,H,W,C] u8|None.
    Semantics: functions.py:3104-3120, 3140-3202, 2867-2874 (see include/imk.h)."""
    return _im_binary(preds, None, thr, cmp_ge, img, block_in, block_out)


def im_multiclass(probs, img=None, block_in=True, block_out=True, want_presence=True):
    """probs float32 [N,B,H,W,K] (device) -> final [B,H,W] u8, im [B,H,W] u8, im_size [B] i64,
    presence [N,B,K] u8, img_out.  Semantics: functions.py:3123-3137, 3206-3238."""
    return _im_multiclass(probs, None, img, block_in, block_out, want_presence)


def member_words(members, batch, n_models):
    """per-image member words as a uint32 numpy array [B]: bit n set = model n of the pool votes for the image.  Accepts the words
    themselves or, per image, an iterable of model indices."""
    if n_models < 1 or n_models > 16:
        raise ValueError("a model pool has 1 to 16 models")
    words = np.zeros(batch, dtype=np.uint32)
    if len(members) != batch:
        raise ValueError(f"{len(members)} member sets for {batch} images")
    for i, m in enumerate(members):
        if isinstance(m, (int, np.integer)):
            words[i] = int(m) & 0xFFFFFFFF
        else:
            for j in m:
                if not 0 <= int(j) < n_models:
                    raise ValueError(f"member {j} outside a pool of {n_models}")
                words[i] |= np.uint32(1 << int(j))
    return words


def im_binary_members(preds, members, thr=0.5, cmp_ge=False, img=None, block_in=True, block_out=True):
    """im_binary over per-image sub-ensembles: preds [N,B,H,W,Kb] holds the whole pool (N <= 16), members (member_words) says which
    models vote for which image.  Semantics: include/imk.h, imk_im_binary_members."""
    if members is None:
        raise TypeError("members: one member word or set of model indices per image")
    return _im_binary(preds, members, thr, cmp_ge, img, block_in, block_out)


def im_multiclass_members(probs, members, img=None, block_in=True, block_out=True, want_presence=True):
    """im_multiclass over per-image sub-ensembles (see im_binary_members); presence [N,B,K] is 0 in the rows of non-members."""
    if members is None:
        raise TypeError("members: one member word or set of model indices per image")
    return _im_multiclass(probs, members, img, block_in, block_out, want_presence)


def morph_var(mask, ksizes, op):
    """morph with one window per image: ksizes [B] ints, odd and at most 31, 0 = the image is copied (imk_morph_var)."""
    mask = mask.contiguous()
    b, h, w = mask.shape
    ks = [int(k) for k in ksizes]
    if len(ks) != b:
        raise ValueError(f"{len(ks)} window sizes for {b} images")
    for k in ks:
        if k < 0 or k > 31 or (k and k % 2 == 0):
            raise ValueError(f"window size {k}: 0 (copy) or odd and at most 31")
    kd = torch.tensor(ks, dtype=torch.int32).to(mask.device)
    out = torch.empty_like(mask)
    check(lib.imk_morph_var(mask.data_ptr(), out.data_ptr(), b, h, w, kd.data_ptr(), 0 if op == "erode" else 1,
                            _stream()), "imk_morph_var")
    return out


def morph(mask, ksize, op):
    """mask u8 [B,H,W] device; op 'erode' | 'dilate' with a ksize x ksize ones kernel (functions.py:2858-2864)."""
    mask = mask.contiguous()
    b, h, w = mask.shape
    out = torch.empty_like(mask)
    check(lib.imk_morph(mask.data_ptr(), out.data_ptr(), b, h, w, int(ksize), 0 if op == "erode" else 1,
                        _stream()), "imk_morph")
    return out


def block_apply(im, img=None, masks=None):
    """In place: img[im>0]=0 (img [B,H,W,C]) and masks[:, m][im>0]=0 (masks [B,M,H,W])."""
    b, h, w = im.shape
    c = 0 if img is None else img.shape[-1]
    m = 0 if masks is None else masks.shape[1]
    check(lib.imk_block_apply(im.data_ptr(), _ptr(img), c, _ptr(masks), m, b, h, w, _stream()), "imk_block_apply")
