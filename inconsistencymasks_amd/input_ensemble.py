"""Host side of the input-ensemble baseline (imk_views / imk_vote_views_* / imk_unet_forward_views_vote, include/imk.h): one model
voting with itself over augmented views of each image, the pseudo-label rules of the reference's get_input_ensemble_prediction_*
(functions.py:1409-1459, 1570-1764, 2127-2407).

The random draws happen here, in the reference's order: per view, random.choice over the 12 geometric combinations (ISIC only),
then random.randint(0, max_blur), then the coin random.randint(0, 1) -- exactly the Python draws of generate_random_transformations
and data_augmentation_image, so a caller that seeds `random` gets the reference's ops, blur sizes and coins.  The numpy draws cannot
line up: the reference adds numpy-drawn noise, the kernel a counter-hash field whose seed comes from the numpy stream, and alpha /
beta come after that seed.  torch is used for device memory and streams only."""
import random

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .unet import UNet
from .vote import VOTE_HARD, VOTE_SOFT, vote_binary, vote_multiclass

VOTE_MAJORITY = 2
MAX_VIEWS = 16      # IMK_VIEWS_MAX

# generate_random_transformations' list of 12 (flip_horizontal, flip_vertical, rotation), in its order; op = index + 1, op 0 = identity
TRANSFORMS = [(fh, fv, rot) for fh in range(2) for fv in range(2) for rot in range(1, 4)]


def op_of(flip_horizontal, flip_vertical, rotation):
    return 1 + 6 * flip_horizontal + 3 * flip_vertical + (rotation - 1)


def is_quarter_turn(op):
    return op > 0 and TRANSFORMS[op - 1][2] in (1, 3)


def apply_op(a, op):
    """the view of op: cv2.flip(., 0) (rows), cv2.flip(., 1) (columns), then cv2.rotate, on the first two axes (numpy)"""
    if op == 0:
        return a
    fh, fv, rot = TRANSFORMS[op - 1]
    if fh:
        a = a[::-1]
    if fv:
        a = a[:, ::-1]
    return np.ascontiguousarray(np.rot90(a, k={1: -1, 2: 2, 3: 1}[rot]))


def restore_op(a, op):
    """restore_random_transformations (functions.py:1729-1764): the inverse rotation, then flip 1, then flip 0"""
    if op == 0:
        return a
    fh, fv, rot = TRANSFORMS[op - 1]
    a = np.rot90(a, k={1: 1, 2: 2, 3: -1}[rot])
    if fv:
        a = a[:, ::-1]
    if fh:
        a = a[::-1]
    return np.ascontiguousarray(a)


def _blur_k(rndint):
    return {1: 3, 2: 5, 3: 7}.get(rndint, 0)      # add_noise_and_blur (functions.py:1494-1501)


def _augment_draws(q, max_blur, max_noise, brightness_range_alpha, brightness_range_beta, rng, np_rng):
    """data_augmentation_image's draws (functions.py:1570-1594) into one ViewParams: blur, noise, the coin, alpha / beta"""
    q.blur_k = _blur_k(rng.randint(0, max_blur))
    q.noise_max = int(max_noise) if max_noise > 0 else 0
    q.seed = int(np_rng.randint(0, 2 ** 32, dtype=np.int64)) if max_noise > 0 else 0
    q.bright_on = int(rng.randint(0, 1) == 1)
    if q.bright_on:
        q.alpha = float(np_rng.uniform(brightness_range_alpha[0], brightness_range_alpha[1]))
        q.beta = float(np_rng.uniform(brightness_range_beta[0], brightness_range_beta[1]))


def draw_random_views(n, max_blur=3, max_noise=25, brightness_range_alpha=(0.5, 1.5), brightness_range_beta=(-25, 25),
                      rng=None, np_rng=None):
    """generate_random_transformations (functions.py:1675-1726) for one image: n independent views of the original, each a
    random.choice of the 12 combinations, then data_augmentation_image.  -> list of n ViewParams"""
    rng, np_rng = rng or random, np_rng or np.random
    out = []
    for _ in range(n):
        q = _lib.ViewParams()
        q.op = op_of(*rng.choice(TRANSFORMS))
        _augment_draws(q, max_blur, max_noise, brightness_range_alpha, brightness_range_beta, rng, np_rng)
        out.append(q)
    return out


def draw_chain_views(n, max_blur=1, max_noise=15, brightness_range_alpha=(0.7, 1.3), brightness_range_beta=(-15, 15),
                     rng=None, np_rng=None):
    """the HeLa / multi-class loops (functions.py:2221-2407): n + 1 chained views, view i = data_augmentation_image(view i-1)"""
    rng, np_rng = rng or random, np_rng or np.random
    out = []
    for _ in range(n + 1):
        q = _lib.ViewParams()
        _augment_draws(q, max_blur, max_noise, brightness_range_alpha, brightness_range_beta, rng, np_rng)
        out.append(q)
    return out


def all_views():
    """generate_all_transformations (functions.py:1597-1633): the image itself, then the 12 combinations, no pixel augmentation"""
    out = []
    for op in range(13):
        q = _lib.ViewParams()
        q.op = op
        out.append(q)
    return out


class ViewPlan:
    """The views of a batch: per_image[b] is image b's list of M ViewParams (all of one length).  chain: view m is made from view
    m-1 (HeLa / multi-class); restore: the vote reads each view at its op's pixel map (ISIC)."""

    def __init__(self, per_image, chain=False, restore=False):
        self.n_views = len(per_image[0])
        self.batch = len(per_image)
        if any(len(v) != self.n_views for v in per_image):
            raise ValueError("every image needs the same number of views")
        self.chain, self.restore = chain, restore
        self.params = (_lib.ViewParams * (self.n_views * self.batch))()       # [M][B], member-major
        for b, views in enumerate(per_image):
            for m, q in enumerate(views):
                self.params[m * self.batch + b] = q
        self.ops = np.array([q.op for q in self.params], np.int32)
        self.quarter = int(any(is_quarter_turn(int(o)) for o in self.ops))


def make_views(x_u8, plan):
    """x_u8 [B,H,W,C] uint8 device -> views [M,B,H,W,C] uint8 device (imk_views)"""
    if x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or not x_u8.is_cuda:
        raise TypeError("x_u8 must be a uint8 CUDA tensor [B,H,W,C]")
    x_u8 = x_u8.contiguous()
    b, h, w, c = x_u8.shape
    if b != plan.batch:
        raise ValueError(f"the plan has {plan.batch} images, the batch {b}")
    prm = torch.frombuffer(bytearray(bytes(plan.params)), dtype=torch.uint8).to(x_u8.device)
    views = torch.empty((plan.n_views, b, h, w, c), dtype=torch.uint8, device=x_u8.device)
    check(lib.imk_views(x_u8.data_ptr(), b, h, w, c, plan.n_views, prm.data_ptr(), int(plan.chain), plan.quarter, views.data_ptr(),
                        torch.cuda.current_stream().cuda_stream), "imk_views")
    return views


def vote_views_binary(preds, ops=None, thr=0.5, cmp_ge=True):
    """preds float32 [M,B,H,W,K] device, ops int [M,B] (None: identity) -> masks [B,K,H,W] u8: 255 where every view, read at the
    pixel its op moved the output pixel to, has p >= thr (cmp_ge) or p > thr"""
    if preds.dtype != torch.float32 or preds.dim() != 5 or not preds.is_cuda:
        raise TypeError("preds must be a float32 CUDA tensor [M,B,H,W,K]")
    preds = preds.contiguous()
    m, b, h, w, k = preds.shape
    masks = torch.empty((b, k, h, w), dtype=torch.uint8, device=preds.device)
    ops_d, quarter = None, 0
    if ops is not None:
        ops = np.asarray(ops, np.int32).reshape(m, b)
        quarter = int(any(is_quarter_turn(int(o)) for o in ops.ravel()))
        ops_d = torch.from_numpy(np.ascontiguousarray(ops)).to(preds.device)
    check(lib.imk_vote_views_binary(preds.data_ptr(), m, b, h, w, k, ops_d.data_ptr() if ops_d is not None else None, quarter,
                                    float(thr), int(bool(cmp_ge)), masks.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "imk_vote_views_binary")
    return masks


def vote_views_majority(probs):
    """probs float32 [M,B,H,W,K] device -> labels [B,H,W] u8: np.argmax(np.bincount(per-view np.argmax))"""
    if probs.dtype != torch.float32 or probs.dim() != 5 or not probs.is_cuda:
        raise TypeError("probs must be a float32 CUDA tensor [M,B,H,W,K]")
    probs = probs.contiguous()
    m, b, h, w, k = probs.shape
    out = torch.empty((b, h, w), dtype=torch.uint8, device=probs.device)
    check(lib.imk_vote_views_majority(probs.data_ptr(), m, b, h, w, k, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "imk_vote_views_majority")
    return out


class ViewVote:
    """One model + its input-ensemble vote.  run(x_u8, plan, thr, mode, cmp_ge) -> masks [B,K,H,W] u8 (sigmoid heads) or labels
    [B,H,W] u8 (softmax heads).  A native UNet goes through imk_unet_forward_views_vote (one forward over the B*M views, the vote
    fused with the head where the kernels cover the shape); anything with `.predict(x)` is called once per image with its M views,
    as the reference does, and the stack goes through the unfused votes."""

    def __init__(self, model, binary):
        self.model, self.binary = model, binary
        self.native = isinstance(model, UNet)
        if self.native:
            model.ready_for_inference()
        self._ws = None

    def stack(self, views):
        """views [M,B,H,W,C] u8 device -> predictions [M,B,H,W,K] float32 device"""
        m, b = views.shape[:2]
        if self.native:
            p = self.model.predict_device(views.reshape(m * b, *views.shape[2:]))
            return p.reshape(m, b, *p.shape[1:])
        v = views.cpu().numpy()
        per = [np.asarray(self.model.predict(np.ascontiguousarray(v[:, i])), dtype=np.float32) for i in range(b)]
        return torch.from_numpy(np.stack(per, 1)).cuda().contiguous()

    def run(self, x_u8, plan, thr=0.5, mode=VOTE_HARD, cmp_ge=False):
        views = make_views(x_u8, plan)
        if not self.native:
            preds = self.stack(views)
            if plan.restore:
                return vote_views_binary(preds, plan.ops.reshape(plan.n_views, plan.batch), thr, cmp_ge)
            if mode == VOTE_MAJORITY:
                return vote_views_majority(preds)
            if self.binary:
                return vote_views_binary(preds, None, thr, True) if (cmp_ge and mode == VOTE_HARD) else vote_binary(preds, thr, mode == VOTE_SOFT)
            return vote_multiclass(preds, mode == VOTE_SOFT)
        p = self.model.plan
        m, b = plan.n_views, plan.batch
        nbytes = lib.imk_unet_forward_views_vote_workspace_bytes(p.ptr, m, b)
        if nbytes < 0:
            check(int(nbytes), "imk_unet_forward_views_vote_workspace_bytes")
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=x_u8.device)
        ops_d = torch.from_numpy(plan.ops).to(x_u8.device) if plan.restore else None
        shape = (b, p.n_out, p.h, p.w) if p.act_out == "sigmoid" else (b, p.h, p.w)
        out = torch.empty(shape, dtype=torch.uint8, device=x_u8.device)
        check(lib.imk_unet_forward_views_vote(p.ptr, self.model.params.data_ptr(), self.model.packed.data_ptr(), views.data_ptr(), m, b,
                                              ops_d.data_ptr() if ops_d is not None else None, plan.quarter, float(thr), int(mode),
                                              int(bool(cmp_ge)), out.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                              torch.cuda.current_stream().cuda_stream), "imk_unet_forward_views_vote")
        return out
