"""Host side of the noisy-student baseline (imk_unet_forward_student, include/imk.h): the teacher's pass of the reference's
create_pseudo_labels_noisy_student_* (functions.py:3243-3417).  Per image: predict on the un-augmented image, label it, then move
image and label with ONE draw of flips / quarter turn (augment_image_and_mask(s), :2725-2826); the image alone gets brightness,
blur and noise.

The draws are augment.draw_params': `random` calls in the reference's order (flip_v if free, flip_h, rot if free, the coin, the blur
size), so a seeded stream gives the reference's geometry, coin and blur size.  Its numpy stream (alpha, beta, the noise) cannot be
followed -- the noise here is a counter-hash field -- so the writers draw each image's values from (SEED, output directory, file
name): files do not depend on the rank count or the batch size.  torch is used for device memory and streams only."""
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .augment import augment_batch, draw_params
from .input_ensemble import vote_views_binary
from .unet import UNet
from .vote import vote_multiclass


def pack_params(per_image):
    """a list of one-element (or longer) AugParams arrays / AugParams records -> one AugParams array"""
    flat = [q for p in per_image for q in (p if hasattr(p, "__len__") else [p])]
    arr = (_lib.AugParams * len(flat))()
    for i, q in enumerate(flat):
        arr[i] = q
    return arr


class TeacherLabel:
    """One teacher + its label pass.  run(x_u8, img_u8, params, thr, cmp_ge) -> (img_out [B,H,W,C] u8, labels): masks [B,K,H,W]
    u8 {0,255} (sigmoid heads: p > thr, or p >= thr with cmp_ge) or class ids [B,H,W] u8 (softmax heads: np.argmax), both in the
    moved frame.  A native UNet goes through imk_unet_forward_student; anything with `.predict(x)` is called on the batch, labelled
    by the single-member vote kernels and moved by imk_augment with the label as its mask."""

    def __init__(self, model, binary):
        self.model, self.binary = model, binary
        self.native = isinstance(model, UNet)
        if self.native:
            model.ready_for_inference()
        self._ws = None

    def run(self, x_u8, img_u8, params, thr=0.5, cmp_ge=False):
        for t in (x_u8, img_u8):
            if t.dtype != torch.uint8 or t.dim() != 4 or not t.is_cuda:
                raise TypeError("x_u8 and img_u8 must be uint8 CUDA tensors [B,H,W,C]")
        x_u8, img_u8 = x_u8.contiguous(), img_u8.contiguous()
        b, h, w, _ = img_u8.shape
        if len(params) != b or x_u8.shape != img_u8.shape:
            raise ValueError("one AugParams per image, and x_u8 shaped like img_u8")
        if not self.native:
            preds = torch.from_numpy(np.ascontiguousarray(np.asarray(self.model.predict(x_u8.cpu().numpy()), np.float32))).cuda()
            if self.binary:
                lab = vote_views_binary(preds[None], None, thr, cmp_ge).permute(0, 2, 3, 1).contiguous()      # [B,H,W,K]
            else:
                lab = vote_multiclass(preds[None], soft=False)[..., None].contiguous()                        # [B,H,W,1]
            out, moved = augment_batch(img_u8, lab, params)
            return out, (moved.permute(0, 3, 1, 2).contiguous() if self.binary else moved[..., 0].contiguous())
        p = self.model.plan
        self.model.ready_for_inference()
        nbytes = lib.imk_unet_forward_student_workspace_bytes(p.ptr, b)
        if nbytes < 0:
            check(int(nbytes), "imk_unet_forward_student_workspace_bytes")
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=x_u8.device)
        quarter = int(any(q.rot in (1, 3) for q in params))
        prm = torch.frombuffer(bytearray(bytes(params)), dtype=torch.uint8).to(x_u8.device)
        out = torch.empty_like(img_u8)
        labels = torch.empty((b, p.n_out, h, w) if p.act_out == "sigmoid" else (b, h, w), dtype=torch.uint8, device=x_u8.device)
        check(lib.imk_unet_forward_student(p.ptr, self.model.params.data_ptr(), self.model.packed.data_ptr(), x_u8.data_ptr(),
                                           img_u8.data_ptr(), b, float(thr), int(bool(cmp_ge)), prm.data_ptr(), quarter,
                                           out.data_ptr(), labels.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                           torch.cuda.current_stream().cuda_stream), "imk_unet_forward_student")
        # prm stays referenced until the caller's stream has passed the launches (the allocator is stream-ordered on this stream)
        return out, labels


def draw_for(rngs, brightness_range_alpha, brightness_range_beta, max_blur, max_noise, free_rotation):
    """one image's AugParams from its (random.Random, numpy RandomState) pair"""
    return draw_params(1, brightness_range_alpha, brightness_range_beta, max_blur, max_noise, free_rotation, rng=rngs[0],
                       np_rng=rngs[1])[0]


def aug_name(imagename):
    """the HeLa writer's file name: f'{imagename[:-4]}_aug.png' (functions.py:3345)"""
    return f"{imagename[:-4]}_aug.png"


def out_dirs(main_output_path, subs):
    out = {k: os.path.join(main_output_path, k) for k in subs}
    for d in out.values():
        os.makedirs(d, exist_ok=True)
    return out
