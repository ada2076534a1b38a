"""Host-side mirror of the reference's evalnet.py on top of libimk.so.

`get_evalnet(i_height, i_width, inputA_channels, inputB_channels, alpha=2, ...)` (evalnet.py:24),
`get_evalnet_miou(...)` (evalnet.py:49) and `get_evalnet_miou_v2(...)` (evalnet.py:76) keep the reference signatures and
return an `EvalNet` whose `.predict([A, B])` takes uint8 NHWC batches like `tf.keras.Model.predict` and returns what the
Keras models return: one float32 [B,1] array, or the list [iou [B,Cb], detection [B,Cb]].  `get_evalnet_miou_v2` is the
late-fusion network (four conv blocks per tower, add at 1/16 resolution, three trunk blocks; inputs from 128 x 128 up): no
reference script calls it, but every EvalNet function here takes it, and `CandidateScorer` then runs the whole image tower
once per image.  torch is used for device memory only.
"""
import ctypes

import numpy as np
import torch

from ._lib import EvalnetCfg, check, lib
from .unet import Plan, UNet, _stream


class EvalPlan(Plan):
    """imk_evalnet_plan_create: the same C plan object as the U-Net's (parameter layout, packing, optimizer state)."""

    _ws_fn = "imk_evalnet_workspace_bytes"

    def __init__(self, h, w, ca, cb, n_out, alpha, two_heads, normalize_a, normalize_b, b_onehot=False, arch="v1"):
        if arch not in ("v1", "v2"):
            raise ValueError(f"arch must be 'v1' or 'v2', got {arch!r}")
        self.arch = arch                                               # "v2": get_evalnet_miou_v2 (evalnet.py:76-106)
        ch = [int(v * alpha) for v in (16, 32, 64, 128, 256)]          # evalnet.py:28-41, 80-100
        self.cfg = EvalnetCfg(h, w, ca, cb, n_out, int(two_heads), int(normalize_a), int(normalize_b), (ctypes.c_int * 5)(*ch),
                              int(b_onehot))
        self.h, self.w, self.ca, self.cb, self.n_out, self.alpha = h, w, ca, cb, n_out, alpha
        self.two_heads, self.b_onehot = bool(two_heads), bool(b_onehot)
        self._p = ctypes.c_void_p()
        create = "imk_evalnet_v2_plan_create" if arch == "v2" else "imk_evalnet_plan_create"
        check(getattr(lib, create)(ctypes.byref(self.cfg), ctypes.byref(self._p)), create)
        self._describe()


class EvalNet(UNet):
    N_STATS = 8     # loss, overflow flag, loss scale, step, loss of head 0 (mse), loss of head 1 (bce), 2 spare

    def __init__(self, h, w, ca, cb, n_out, alpha, two_heads, normalize_a=True, normalize_b=True, seed=None, device="cuda",
                 b_onehot=False, arch="v1"):
        self._init_from_plan(EvalPlan(h, w, ca, cb, n_out, alpha, two_heads, normalize_a, normalize_b, b_onehot, arch), seed, device,
                             dense=("dense", "iou", "detection"))
        self.n_heads = 2 if two_heads else 1

    # ---- inference ----------------------------------------------------------------------------------
    def _as_u8(self, x, c):
        t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
        if t.dim() == 3:
            t = t[None]
        if t.dtype != torch.uint8:
            t = t.round().clamp(0, 255).to(torch.uint8)
        if t.shape[1:] != (self.plan.h, self.plan.w, c):
            raise ValueError(f"expected [B,{self.plan.h},{self.plan.w},{c}], got {tuple(t.shape)}")
        return t.to(self.device).contiguous()

    def _as_input_b(self, x):
        """input B as the kernels take it: the uint8 mask stack [B,H,W,Cb], or with b_onehot the class-id map [B,H,W,1]
        (a one-hot stack [B,H,W,K], which is what the reference's call sites pass, is folded back to class ids)"""
        if not self.plan.b_onehot:
            return self._as_u8(x, self.plan.cb)
        t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
        if t.dim() == 4 and t.shape[-1] == self.plan.cb and self.plan.cb > 1:
            t = t.argmax(-1)
        if t.dim() == 2:
            t = t[None]
        if t.dim() == 3:
            t = t[..., None]
        return self._as_u8(t, 1)

    def predict_device(self, xa_u8, xb_u8):
        """uint8 device tensors [B,H,W,Ca], [B,H,W,Cb] (b_onehot: class ids [B,H,W,1]) -> float32 [B, n_heads*n_out]."""
        self.ready_for_inference()
        b = xa_u8.shape[0]
        ws = self.workspace(b, 0)
        out = torch.empty((b, self.n_heads * self.plan.n_out), dtype=torch.float32, device=self.device)
        check(lib.imk_evalnet_forward(self.plan.ptr, self.params.data_ptr(), self.packed.data_ptr(), xa_u8.data_ptr(),
                                      xb_u8.data_ptr(), b, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
              "imk_evalnet_forward")
        return out

    def predict(self, x, batch_size=32, verbose=0):
        """Keras-like: [A, B] numpy batches in; [B,1] (get_evalnet) or [iou, detection] (get_evalnet_miou) out."""
        xa, xb = self._as_u8(x[0], self.plan.ca), self._as_input_b(x[1])
        outs = [self.predict_device(xa[i:i + batch_size], xb[i:i + batch_size]) for i in range(0, xa.shape[0], batch_size)]
        o = torch.cat(outs, 0).cpu().numpy()
        k = self.plan.n_out
        return [o[:, :k], o[:, k:]] if self.n_heads == 2 else o

    def intermediate(self, layer_name, batch, mode=0, which=0):
        idx = [l["name"] for l in self.plan.layers].index(layer_name)
        off, h, w, c, cs = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(lib.imk_evalnet_tensor_info(self.plan.ptr, batch, mode, idx, which, ctypes.byref(off), ctypes.byref(h),
                                          ctypes.byref(w), ctypes.byref(c), ctypes.byref(cs)), "imk_evalnet_tensor_info")
        ws = [v for k, v in self._ws.items() if k[0] == batch and k[1] == mode][0]
        n = batch * h.value * w.value * cs.value
        t = ws[off.value:off.value + 2 * n].view(torch.float16).reshape(batch, h.value, w.value, cs.value)
        return t[..., :c.value].float().cpu()

    # ---- training ---------------------------------------------------------------------------------------
    def fwd_bwd(self, xa_u8, xb_u8, y):
        """One forward/backward on device batches (y float32 [B, n_heads*n_out]); fills self.grads / self.stats and
        returns the training-mode outputs [B, n_heads*n_out]."""
        if self.train_state is None:
            self.init_train_state()
        if not self._packed_ok:
            self.repack()
        self._fold_ok = False
        b = xa_u8.shape[0]
        ws = self.workspace(b, 1)
        out = torch.empty((b, self.n_heads * self.plan.n_out), dtype=torch.float32, device=self.device)
        check(lib.imk_evalnet_fwd_bwd(self.plan.ptr, self.params.data_ptr(), self.packed.data_ptr(),
                                      self.train_state.data_ptr(), xa_u8.data_ptr(), xb_u8.data_ptr(), y.data_ptr(), b,
                                      out.data_ptr(), self.grads.data_ptr(), self.stats.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _stream()), "imk_evalnet_fwd_bwd")
        return out

    def train_step(self, xa_u8, xb_u8, y, lr, wd):
        out = self.fwd_bwd(xa_u8, xb_u8, y)
        self.adamw_step(lr, wd)
        return out


# ---- EvalNet-ensemble selection (imk_evalnet_select / imk_evalnet_forward_select, include/imk.h) -----------------------------
SELECT_IOU, SELECT_MIOU, SELECT_CONF_GATED = 0, 1, 2
SELECT_MAX_CAND, SELECT_MAX_MODELS = 16, 8


def _select_outputs(b, cand):
    dev = cand.device
    return (torch.empty(b, dtype=torch.int32, device=dev), torch.empty(b, dtype=torch.float32, device=dev),
            torch.empty(b, dtype=torch.uint8, device=dev), torch.empty((b,) + tuple(cand.shape[2:]), dtype=torch.uint8, device=dev))


def _cand_bytes(cand, b, m):
    if cand.dtype != torch.uint8 or not cand.is_cuda or cand.dim() < 3 or tuple(cand.shape[:2]) != (b, m):
        raise TypeError(f"cand must be a uint8 CUDA tensor [{b},{m},...]")
    return cand[0, 0].numel()


def select_candidates(scores, cand, thr, mode, counts=None):
    """scores float32 [N,B,M,U] (device; U = 1, or the iou units then the detection units), cand uint8 [B,M,...] (device; a multiple
    of 16 bytes per candidate), counts int32 [B] (device) or None -> (best_idx [B] i32, best_score [B] f32, keep [B] u8, out [B,...] u8):
    the arg-max candidate by the ensemble's mean IoU (SELECT_IOU) or mean mIoU over the detected classes (SELECT_MIOU), kept where the
    score reaches thr -- the rule of the reference's create_training_data_for_segnet_with_*ensemble* writers.  SELECT_CONF_GATED is the
    single-EvalNet multi-class writer's rule: the mean detection value over the classes whose mean detection over the image's
    candidates reaches 0.03 (create_training_data_by_evalnet_miou_for_segnet_multiclass); the iou units are not read."""
    if scores.dtype != torch.float32 or scores.dim() != 4 or not scores.is_cuda:
        raise TypeError("scores must be a float32 CUDA tensor [N,B,M,U]")
    scores, cand = scores.contiguous(), cand.contiguous()
    n, b, m, u = scores.shape
    nbytes = _cand_bytes(cand, b, m)
    n_heads = 1 if mode == SELECT_IOU else 2
    if counts is not None:
        counts = counts.to(device=scores.device, dtype=torch.int32).contiguous()
    best_idx, best_score, keep, out = _select_outputs(b, cand)
    check(lib.imk_evalnet_select(scores.data_ptr(), n, b, m, n_heads, u // n_heads, counts.data_ptr() if counts is not None else None,
                                 cand.data_ptr(), nbytes, float(thr), mode, best_idx.data_ptr(), best_score.data_ptr(),
                                 keep.data_ptr(), out.data_ptr(), _stream()), "imk_evalnet_select")
    return best_idx, best_score, keep, out


class CandidateScorer:
    """The EvalNets of one ensemble + the workspace of imk_evalnet_forward_select.  EvalNets of one architecture take the fused call
    (the image tower once per image); other ensembles (different plans, duck-typed models with .predict) are scored model by model
    on the repeated images and go through imk_evalnet_select."""

    def __init__(self, evalnets):
        self.models = list(evalnets)
        native = all(isinstance(m, EvalNet) for m in self.models)
        self.shared = native and all(bytes(m.plan.cfg) == bytes(self.models[0].plan.cfg) and m.plan.arch == self.models[0].plan.arch
                                     for m in self.models)
        self.n_heads = self.models[0].n_heads if native else None
        self._ws = {}
        if self.shared:
            for m in self.models:
                m.ready_for_inference()
            n = len(self.models)
            self._params = (ctypes.c_void_p * n)(*[m.params.data_ptr() for m in self.models])
            self._packed = (ctypes.c_void_p * n)(*[m.packed.data_ptr() for m in self.models])

    def _workspace(self, b, m, dev):
        if (b, m) not in self._ws:
            nbytes = lib.imk_evalnet_forward_candidates_workspace_bytes(self.models[0].plan.ptr, b, m)
            if nbytes < 0:
                check(int(nbytes), "imk_evalnet_forward_candidates_workspace_bytes")
            self._ws = {(b, m): torch.empty(nbytes, dtype=torch.uint8, device=dev)}
        return self._ws[(b, m)]

    def scores(self, xa, xb):
        """xa u8 [B,H,W,Ca], xb u8 [B,M,H,W,Cb] (b_onehot: class ids [B,M,H,W]) on the device -> scores float32 [N,B,M,U]"""
        xa, xb = xa.contiguous(), xb.contiguous()
        b, m = xb.shape[:2]
        if self.shared:
            p = self.models[0].plan
            out = torch.empty((len(self.models), b, m, self.n_heads * p.n_out), dtype=torch.float32, device=xa.device)
            ws = self._workspace(b, m, xa.device)
            check(lib.imk_evalnet_forward_candidates(p.ptr, len(self.models), self._params, self._packed, xa.data_ptr(), xb.data_ptr(),
                                                     b, m, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                  "imk_evalnet_forward_candidates")
            return out
        rep = xa.repeat_interleave(m, 0)
        flat = xb.reshape((b * m,) + tuple(xb.shape[2:]))
        outs = []
        for mod in self.models:
            if hasattr(mod, "predict_device"):
                fb = flat if flat.dim() == 4 else flat[..., None]
                o = mod.predict_device(rep, fb.contiguous())
            else:
                o = mod.predict([rep.cpu().numpy(), flat.cpu().numpy()])
                o = np.concatenate([np.asarray(v, np.float32) for v in o], 1) if isinstance(o, (list, tuple)) else np.asarray(o, np.float32)
                o = torch.from_numpy(np.ascontiguousarray(o)).to(xa.device)
            outs.append(o.reshape(b, m, -1))
        return torch.stack(outs, 0).contiguous()

    def run(self, xa, xb, cand, thr, counts=None, mode=None):
        """-> (best_idx [B], best_score [B], keep [B], out [B,...] = the best candidate's bytes of `cand` [B,M,...])"""
        if not self.shared:
            sc = self.scores(xa, xb)
            if mode is None:
                mode = SELECT_IOU if sc.shape[-1] == 1 else SELECT_MIOU
            return select_candidates(sc, cand, thr, mode, counts)
        if mode is None:
            mode = SELECT_MIOU if self.n_heads == 2 else SELECT_IOU
        xa, xb, cand = xa.contiguous(), xb.contiguous(), cand.contiguous()
        b, m = xb.shape[:2]
        p = self.models[0].plan
        nbytes = _cand_bytes(cand, b, m)
        if counts is not None:
            counts = counts.to(device=xa.device, dtype=torch.int32).contiguous()
        scores = torch.empty((len(self.models), b, m, self.n_heads * p.n_out), dtype=torch.float32, device=xa.device)
        best_idx, best_score, keep, out = _select_outputs(b, cand)
        ws = self._workspace(b, m, xa.device)
        check(lib.imk_evalnet_forward_select(p.ptr, len(self.models), self._params, self._packed, xa.data_ptr(), xb.data_ptr(), b, m,
                                             counts.data_ptr() if counts is not None else None, cand.data_ptr(), nbytes, float(thr),
                                             mode, scores.data_ptr(), best_idx.data_ptr(), best_score.data_ptr(), keep.data_ptr(),
                                             out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "imk_evalnet_forward_select")
        self.last_scores = scores
        return best_idx, best_score, keep, out


def score_candidates(evalnets, xa, xb, cand, thr, counts=None, mode=None):
    """One call of CandidateScorer(evalnets).run(...)."""
    return CandidateScorer(evalnets).run(xa, xb, cand, thr, counts, mode)


def _check_defaults(actifu, ksi, kernel_ini):
    if actifu != "relu" or ksi != 3 or kernel_ini != "he_normal":
        raise NotImplementedError("only the defaults every reference script uses: relu, 3x3, he_normal")


def get_evalnet(i_height, i_width, inputA_channels, inputB_channels, alpha=2, actifu="relu", ksi=3, kernel_ini="he_normal",
                normalize_A=True, normalize_B=True, seed=None, device="cuda", onehot_B=None):
    """evalnet.py:24 -- one sigmoid unit.  onehot_B as get_evalnet_miou: input B is the one-hot stack of a class-id map (the scalar-IoU
    multiclass scripts, functions.py:5217), passed as class ids and expanded on the device; default True when inputB_channels > 4.
    With normalize_B (this constructor's default) the stack goes through the x / 255 Lambda like any input: the hot channel then
    holds the fp16 value the normalised uint8 stem forms for the byte 1."""
    _check_defaults(actifu, ksi, kernel_ini)
    onehot = inputB_channels > 4 if onehot_B is None else bool(onehot_B)
    return EvalNet(i_height, i_width, inputA_channels, inputB_channels, 1, alpha, False, normalize_A, normalize_B, seed, device,
                   b_onehot=onehot)


def get_evalnet_miou(i_height, i_width, inputA_channels, inputB_channels, alpha=2, actifu="relu", ksi=3,
                     kernel_ini="he_normal", normalize_A=True, normalize_B=False, seed=None, device="cuda", onehot_B=None):
    """evalnet.py:49 -- heads 'iou' and 'detection', inputB_channels sigmoid units each.  onehot_B: input B is the
    one-hot stack of a class-id map (the multiclass scripts, functions.py:4978); it is then passed as class ids and
    expanded on the device.  Default: True when inputB_channels > 4 (SUIM: 9 classes), False for mask stacks (HeLa: 3)."""
    _check_defaults(actifu, ksi, kernel_ini)
    onehot = inputB_channels > 4 if onehot_B is None else bool(onehot_B)
    if onehot and normalize_B:
        raise NotImplementedError("a one-hot input is not divided by 255 in any reference script")
    return EvalNet(i_height, i_width, inputA_channels, inputB_channels, inputB_channels, alpha, True, normalize_A,
                   normalize_B, seed, device, b_onehot=onehot)


def get_evalnet_miou_v2(i_height, i_width, inputA_channels, inputB_channels, alpha=2, actifu="relu", ksi=3,
                        kernel_ini="he_normal", normalize_A=True, normalize_B=False, seed=None, device="cuda", onehot_B=None):
    """evalnet.py:76 -- the late-fusion network: input block + four conv blocks per tower, add() of the towers at 1/16
    resolution, three conv blocks, heads 'iou' and 'detection'.  Seven poolings: inputs from 128 x 128 up.  onehot_B as
    get_evalnet_miou."""
    _check_defaults(actifu, ksi, kernel_ini)
    onehot = inputB_channels > 4 if onehot_B is None else bool(onehot_B)
    if onehot and normalize_B:
        raise NotImplementedError("a one-hot input is not divided by 255 in any reference script")
    return EvalNet(i_height, i_width, inputA_channels, inputB_channels, inputB_channels, alpha, True, normalize_A,
                   normalize_B, seed, device, b_onehot=onehot, arch="v2")
