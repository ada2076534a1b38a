"""Host wrappers of the model-ensemble vote (imk_vote_binary / imk_vote_multiclass / imk_unet_forward_vote, include/imk.h):
the pseudo-label rules of the reference's model-ensemble baseline (get_model_ensemble_prediction_*, functions.py:2409-2566).
torch is used for device memory and streams only."""
import ctypes

import numpy as np
import torch

from ._lib import check, lib
from .unet import UNet

VOTE_HARD, VOTE_SOFT = 0, 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_stack(t, what):
    if t.dtype != torch.float32 or t.dim() != 5 or not t.is_cuda:
        raise TypeError(f"{what} must be a float32 CUDA tensor [N,B,H,W,K]")
    return t.contiguous()


def vote_binary(preds, thr=0.5, soft=False):
    """preds float32 [N,B,H,W,Kb] (device) -> masks [B,Kb,H,W] u8 {0,255}.  hard: every model has p > thr;
    soft: the fp64 mean of the N probabilities (summed in model order) > thr."""
    preds = _check_stack(preds, "preds")
    n, b, h, w, kb = preds.shape
    masks = torch.empty((b, kb, h, w), dtype=torch.uint8, device=preds.device)
    check(lib.imk_vote_binary(preds.data_ptr(), n, b, h, w, kb, float(thr), VOTE_SOFT if soft else VOTE_HARD,
                              masks.data_ptr(), _stream()), "imk_vote_binary")
    return masks


def vote_multiclass(probs, soft=False):
    """probs float32 [N,B,H,W,K] (device) -> final [B,H,W] u8 class ids.  hard: the label where all arg-maxes agree, else 0;
    soft: argmax of the fp32 mean over the models (np.mean(axis=0) of the stack).  np.argmax's NaN rule in both."""
    probs = _check_stack(probs, "probs")
    n, b, h, w, k = probs.shape
    final = torch.empty((b, h, w), dtype=torch.uint8, device=probs.device)
    check(lib.imk_vote_multiclass(probs.data_ptr(), n, b, h, w, k, VOTE_SOFT if soft else VOTE_HARD, final.data_ptr(),
                                  _stream()), "imk_vote_multiclass")
    return final


class EnsembleVote:
    """N native UNet models of one architecture + the workspace of imk_unet_forward_vote (the size of imk_unet_forward_im's: up to
    3 models run side by side on streams).  run() -> masks [B,Kb,H,W] u8 (sigmoid heads) or labels [B,H,W] u8 (softmax heads)."""

    def __init__(self, models):
        if not all(isinstance(m, UNet) for m in models):
            raise TypeError("EnsembleVote needs inconsistencymasks_amd.unet.UNet models")
        self.models = list(models)
        self.plan = models[0].plan
        for m in models:
            m.ready_for_inference()
        n = len(models)
        self._params = (ctypes.c_void_p * n)(*[m.params.data_ptr() for m in models])
        self._packed = (ctypes.c_void_p * n)(*[m.packed.data_ptr() for m in models])
        self._ws = None
        self._ws_batch = 0

    def run(self, x_u8, thr=0.5, soft=False):
        p = self.plan
        b, n, dev = x_u8.shape[0], len(self.models), x_u8.device
        x_u8 = x_u8.contiguous()
        if self._ws is None or self._ws_batch < b:
            nbytes = lib.imk_unet_forward_im_workspace_bytes(p.ptr, n, b, min(n, 3))
            if nbytes < 0:
                check(int(nbytes), "imk_unet_forward_im_workspace_bytes")
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self._ws_batch = b
        shape = (b, p.n_out, p.h, p.w) if p.act_out == "sigmoid" else (b, p.h, p.w)
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
        check(lib.imk_unet_forward_vote(p.ptr, n, self._params, self._packed, x_u8.data_ptr(), b, float(thr),
                                        VOTE_SOFT if soft else VOTE_HARD, out.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                        _stream()), "imk_unet_forward_vote")
        return out


class StackVote:
    """The same run() as EnsembleVote for duck-typed models (anything with `.predict(x)` like a Keras model, called once per image
    with a [1,H,W,C] batch as the reference does): the probability stack goes through imk_vote_binary / imk_vote_multiclass."""

    def __init__(self, models, binary):
        self.models, self.binary = list(models), binary

    def stack(self, x_u8):
        outs = []
        for m in self.models:
            if hasattr(m, "predict_device"):
                outs.append(m.predict_device(x_u8))
            else:
                xs = x_u8.cpu().numpy()
                p = np.concatenate([np.asarray(m.predict(xs[i:i + 1]), dtype=np.float32) for i in range(len(xs))], 0)
                outs.append(torch.from_numpy(p).cuda())
        return torch.stack(outs, 0).contiguous()

    def run(self, x_u8, thr=0.5, soft=False):
        preds = self.stack(x_u8)
        return vote_binary(preds, thr, soft) if self.binary else vote_multiclass(preds, soft)


def ensemble_vote(models, binary):
    return EnsembleVote(models) if all(isinstance(m, UNet) for m in models) else StackVote(models, binary)
