"""The depth-map (image-to-image regression) family of the reference's functions.py, on top of libimk.so (csrc/imk_depth.hip):

  rmse, delta_metric (functions.py:36-48)            host restatements of the loss / metric VALUES on arrays
  parse_image_depth_map (:1051-1073)                  image + depth map of one file pair
  load_labeled_data_depth_map (:903-927)              two directories -> arrays
  train_depth_map (:320-364)                          model.fit with 'mse' or rmse on continuous targets + three benchmarks
  benchmark_depth_map (:1345-1384)                    model.evaluate + the prediction PNGs
  get_im_prediction_depth_map (:6155-6177)            the standard-deviation inconsistency mask

Names, positional arguments and defaults are the reference's.  No reference script calls these functions (SURVEY section 2 lists the
family); they are here because the family is the one place where the inconsistency-mask idea leaves classification, and a user who
takes this package as a drop-in wants it for regression targets too.  Out of scope: train_depth_map_consistency_loss (its tail cannot
run in the reference: it calls benchmark_depth_map with three arguments), a pseudo-label writer (the reference defines no rule), K > 1.
There is no CPU fallback: the rule, the evaluation sums and the training step are HIP kernels."""
import ctypes
import glob
import os
import re

import numpy as np
import torch

from ._lib import check, lib

DEPTH_MIN_MODELS, DEPTH_MAX_MODELS = 2, 16      # imk_im_depth's limits (include/imk.h)
IMK_EUNSUPPORTED = -2


def _F():
    from . import functions
    return functions


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _check_n(n, who):
    if not DEPTH_MIN_MODELS <= n <= DEPTH_MAX_MODELS:
        raise ValueError(f"{who}: the standard-deviation IM takes {DEPTH_MIN_MODELS} to {DEPTH_MAX_MODELS} models, got {n}")


# ---------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------
def im_depth(preds, mult=2, img=None, block_in=True, want_std=False):
    """preds float32 [N,B,H,W] (device), one threshold PER IMAGE of the batch -> dict of device tensors: im [B,H,W] u8 {0,255},
    im_size [B] i64, thr [B] f32, std [B,H,W] f32 | None, img_out [B,H,W,C] u8 | None.  Semantics: include/imk.h, imk_im_depth."""
    if preds.dtype != torch.float32 or preds.dim() != 4 or not preds.is_cuda:
        raise TypeError("preds must be a float32 CUDA tensor [N,B,H,W]")
    preds = preds.contiguous()
    n, b, h, w = preds.shape
    _check_n(n, "im_depth")
    dev = preds.device
    if img is not None:
        img = torch.as_tensor(img)
        if img.dtype != torch.uint8:
            raise TypeError("images must be uint8")
        img = img.to(dev).contiguous()
    c = 0 if img is None else img.shape[-1]
    im = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    im_size = torch.empty((b,), dtype=torch.int64, device=dev)
    thr = torch.empty((b,), dtype=torch.float32, device=dev)
    img_out = None if img is None else torch.empty_like(img)
    nbytes = lib.imk_im_depth_workspace_bytes(b, h, w)
    if nbytes == IMK_EUNSUPPORTED:
        raise ValueError(f"im_depth: an image of {h} x {w} pixels (limit 2^24) or a batch of {b} (limit 65535) is out of range")
    if nbytes < 0:
        check(int(nbytes), "imk_im_depth_workspace_bytes")
    std = torch.empty((b, h, w), dtype=torch.float32, device=dev) if want_std else None
    ws = None if want_std else torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.imk_im_depth(preds.data_ptr(), n, b, h, w, float(np.float32(mult)), _ptr(img), c, int(bool(block_in)), _ptr(img_out),
                          im.data_ptr(), im_size.data_ptr(), thr.data_ptr(), _ptr(std), _ptr(ws), 0 if ws is None else ws.numel(),
                          _stream())
    check(rc, "imk_im_depth")
    return {"im": im, "im_size": im_size, "thr": thr, "std": std, "img_out": img_out}


def eval_depth(probs, gt, want_pred=True):
    """probs [B,H,W] or [B,H,W,1] f32 cuda, gt [B,H,W] or [B,H,W,1] u8 cuda -> (pred u8 cuda | None, sums [B,2] float64 numpy:
    per image the squared error against gt / 255 and the number of pixels with max(p / y, y / p) < 1.25)."""
    if probs.dim() == 4:
        assert probs.shape[3] == 1
        probs = probs[..., 0]
    if gt.dim() == 4:
        assert gt.shape[3] == 1
        gt = gt[..., 0]
    probs, gt = probs.contiguous(), gt.contiguous()
    assert probs.is_cuda and probs.dtype == torch.float32 and gt.dtype == torch.uint8 and gt.shape == probs.shape
    b, h, w = probs.shape
    pred = torch.empty((b, h, w), dtype=torch.uint8, device=probs.device) if want_pred else None
    sums = torch.empty((b, 2), dtype=torch.float64, device=probs.device)
    check(lib.imk_eval_depth(probs.data_ptr(), gt.data_ptr(), b, h, w, _ptr(pred), sums.data_ptr(), _stream()), "imk_eval_depth")
    return pred, sums.cpu().numpy()


class EnsembleDepthIM:
    """N U-Nets of one architecture + the workspace of imk_unet_forward_im_depth: forwards and the rule in one call, the probability
    stack never written (where the fused head covers the shape; bit-identical to predict_device x N + im_depth either way)."""

    def __init__(self, models, n_streams=None):
        F = _F()
        if not F._is_native(models):
            raise TypeError("EnsembleDepthIM needs inconsistencymasks_amd.unet.UNet models")
        _check_n(len(models), "EnsembleDepthIM")
        self.models, self.plan = list(models), models[0].plan
        if self.plan.act_out != "sigmoid" or self.plan.n_out != 1:
            raise ValueError("EnsembleDepthIM: the depth-map family has one sigmoid output map")
        n = len(models)
        self.n_streams = min(n, 3) if n_streams is None else int(n_streams)
        self._params = (ctypes.c_void_p * n)(*[m.params.data_ptr() for m in models])
        self._packed = (ctypes.c_void_p * n)(*[m.packed.data_ptr() for m in models])
        self._ws, self._ws_batch = None, 0

    def run(self, x_u8, mult=2, block_in=True, want_std=False):
        p, n, b, dev = self.plan, len(self.models), x_u8.shape[0], x_u8.device
        for m in self.models:
            m.ready_for_inference()
        if self._ws is None or self._ws_batch < b:
            nbytes = lib.imk_unet_forward_im_depth_workspace_bytes(p.ptr, n, b, self.n_streams)
            if nbytes < 0:
                check(int(nbytes), "imk_unet_forward_im_depth_workspace_bytes")
            self._ws, self._ws_batch = torch.empty(nbytes, dtype=torch.uint8, device=dev), b
        im = torch.empty((b, p.h, p.w), dtype=torch.uint8, device=dev)
        im_size = torch.empty((b,), dtype=torch.int64, device=dev)
        thr = torch.empty((b,), dtype=torch.float32, device=dev)
        std = torch.empty((b, p.h, p.w), dtype=torch.float32, device=dev) if want_std else None
        img_out = torch.empty_like(x_u8)
        # the workspace is sized for self._ws_batch images; the call takes as many streams as what it is given has room for
        nbytes = lib.imk_unet_forward_im_depth_workspace_bytes(p.ptr, n, b, self.n_streams)
        check(lib.imk_unet_forward_im_depth(p.ptr, n, self._params, self._packed, x_u8.data_ptr(), b, float(np.float32(mult)),
                                            x_u8.data_ptr(), int(bool(block_in)), img_out.data_ptr(), im.data_ptr(), im_size.data_ptr(),
                                            thr.data_ptr(), _ptr(std), self._ws.data_ptr(), min(int(nbytes), self._ws.numel()),
                                            _stream()), "imk_unet_forward_im_depth")
        return {"im": im, "im_size": im_size, "thr": thr, "std": std, "img_out": img_out}


# ---------------------------------------------------------------------------------------------------
# the reference's names
# ---------------------------------------------------------------------------------------------------
def rmse(y_true, y_pred):
    """functions.py:36-37 on arrays: sqrt(mean((y_pred - y_true)^2)) in float32.  Passed to train_depth_map as `loss_func` it selects
    the fused rmse training step (loss kind 3 of imk_unet_fwd_bwd); called, it is this host restatement of the value."""
    d = np.asarray(y_pred, np.float32) - np.asarray(y_true, np.float32)
    return np.sqrt(np.mean(d * d, dtype=np.float32))


def delta_metric(threshold=1.25):
    """functions.py:39-48: the share of elements with max(y_pred / y_true, y_true / y_pred) < threshold (tf.maximum hands a NaN on,
    `<` is false on it: y_true = 0 counts as false)."""
    def metric(y_true, y_pred):
        y_true, y_pred = np.asarray(y_true, np.float32), np.asarray(y_pred, np.float32)
        with np.errstate(all="ignore"):
            max_ratio = np.maximum(y_pred / y_true, y_true / y_pred)
            return np.mean((max_ratio < np.float32(threshold)).astype(np.float32))

    metric.__name__ = f"delta_{threshold}"
    return metric


def _depth_path(image_path):
    return re.sub("images", "depth_maps", image_path)      # tf.strings.regex_replace(image_dir, 'images', 'depth_maps')


def parse_image_depth_map(image_dir, IMG_CHANNELS=3):
    """functions.py:1051-1073: (image u8 [H,W,C], depth map u8 [H,W,1]).  The reference hands the depth map on as float32(d / 255); here
    it stays the file's uint8 and the training and evaluation kernels form float32(d) / 255.0f themselves (a correctly rounded divide:
    the same float32 values)."""
    F = _F()
    return F.read_png(image_dir, IMG_CHANNELS), F.read_png(_depth_path(image_dir), 1)


def load_labeled_data_depth_map(labeled_images_dir, labeled_depth_maps_dir):
    """functions.py:903-927: (images u8 [N,H,W,3] in cv2.imread's BGR order, depth maps float32 [N,H,W] = d / 255.0)."""
    F = _F()
    image_filenames = sorted(os.listdir(labeled_images_dir))
    mask_filenames = sorted(os.listdir(labeled_depth_maps_dir))
    images = np.array([F.read_png(os.path.join(labeled_images_dir, f), 3)[..., ::-1] for f in image_filenames])
    depth_maps = np.array([F.read_png(os.path.join(labeled_depth_maps_dir, f), 1)[..., 0] for f in mask_filenames])
    return images, depth_maps.astype(np.float32) / 255.0


def _loss_kind(loss_func, who):
    """'mse' -> 2, rmse (the function above, or its name) -> 3; everything else is refused"""
    F = _F()
    if isinstance(loss_func, str) and loss_func == "mse":
        return 2
    if loss_func is rmse or (isinstance(loss_func, str) and loss_func == "rmse"):
        return 3
    F._reject_untrainable(loss_func, who)
    raise NotImplementedError(f"{who}: the depth-map family trains with 'mse' or rmse, got {loss_func!r}")


class DepthDataset:
    """What stands in for the reference's tf.data pipeline list_files(dir/*.png).map(parse_image_depth_map).batch(BATCH_SIZE): the
    directory's files in SORTED order (list_files(seed=SEED)'s shuffled order cannot be reproduced without TensorFlow's generator; the
    batch-size-weighted means formed over the batches differ from the reference's in the last digits where the loss is rmse, whose
    per-batch square roots depend on which files share a batch), decoded once, on the device."""

    def __init__(self, images_dir, channels=3, batch=None):
        F = _F()
        self.images_dir, self.batch = images_dir, F.BATCH_SIZE if batch is None else int(batch)
        self.names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(images_dir, "*.png")))
        self.channels = channels
        self._xy = None

    def tensors(self):
        if self._xy is None:
            F = _F()
            with F._pool() as pool:
                self._xy = tuple(F._decoded_set(pool, [(self.images_dir, self.channels), (_depth_path(self.images_dir), 1)], self.names))
        return self._xy

    def batches(self):
        if not self.names:
            return
        x, y = self.tensors()
        for lo in range(0, len(self.names), self.batch):
            yield self.names[lo:lo + self.batch], x[lo:lo + self.batch], y[lo:lo + self.batch]


def _evaluate(model, dataset, loss_kind, on_batch=None):
    """model.evaluate(dataset) -> [loss, mse, delta_1.25]: Keras' batch-size-weighted means of the per-batch values; the sums come from
    imk_eval_depth.  loss = mse for 'mse', the mean of the per-batch square roots for rmse."""
    n_img, loss_acc, sq_acc, hit_acc, n_el = 0, 0.0, 0.0, 0.0, 0
    for names, x, y in dataset.batches():
        probs = model.predict_device(x)
        pred, sums = eval_depth(probs, y, want_pred=on_batch is not None)
        per = y[0].numel()
        sq, hits, nb = float(sums[:, 0].sum()), float(sums[:, 1].sum()), len(names)
        mse_b = sq / (nb * per)
        loss_acc += nb * (np.sqrt(mse_b) if loss_kind == 3 else mse_b)
        sq_acc, hit_acc, n_el, n_img = sq_acc + sq, hit_acc + hits, n_el + nb * per, n_img + nb
        if on_batch is not None:
            on_batch(names, pred)
    if n_img == 0:
        return [float("nan")] * 3
    return [loss_acc / n_img, sq_acc / n_el, hit_acc / n_el]


def benchmark_depth_map(model, dataset, input_dir, output_dir):
    """functions.py:1345-1384: (results[0], results[1]) of model.evaluate(dataset) -- the compiled loss (rmse or mse; the reference
    names it rmse whatever the model was compiled with) and the 'mse' metric -- and the predictions of input_dir's images as PNGs in
    output_dir: clip(p * 255, 0, 255) truncated to uint8 (imk_eval_depth's pred_out), written through the write pool.
    dataset: a DepthDataset, or a directory of images (its depth maps beside it under 'depth_maps')."""
    F = _F()
    os.makedirs(output_dir, exist_ok=True)
    if not isinstance(dataset, DepthDataset):
        dataset = DepthDataset(dataset, model.plan.c_in)
    kind = getattr(model, "depth_loss_kind", 2)
    same = os.path.abspath(dataset.images_dir) == os.path.abspath(input_dir)

    def write(names, pred):
        pred = pred.cpu().numpy()
        F.write_pngs_async([(os.path.join(output_dir, n), pred[j]) for j, n in enumerate(names)])

    results = _evaluate(model, dataset, kind, write if same else None)
    if not same:      # the reference predicts input_dir on its own; the evaluated set is usually the same directory
        names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(input_dir, "*.png")))
        with F._pool() as pool:
            for lo in range(0, len(names), F.BATCH_SIZE):
                chunk = names[lo:lo + F.BATCH_SIZE]
                x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(input_dir, n) for n in chunk], model.plan.c_in)).cuda()
                probs = model.predict_device(x)
                pred, _ = eval_depth(probs, torch.zeros(probs.shape[:3], dtype=torch.uint8, device=probs.device))
                write(chunk, pred)
    return results[0], results[1]


def train_depth_map(train_images_dir, val_images_dir, test_images_dir, unlabeled_images_dir, modelname, filepath_h5, model, loss_func,
                    steps_per_epoch, val_pred_dir, test_pred_dir, unlabeled_pred_dir):
    """functions.py:320-364.  loss_func: 'mse' or rmse.  ModelCheckpoint(save_best_only, monitor='val_loss', mode='min') with val_loss
    formed over validation batches of BATCH_SIZE in sorted file order (DepthDataset says why).  Returns the reference's six numbers:
    (loss_val, loss_test, loss_unlabeled, mse_val, mse_test, mse_unlabeled)."""
    F = _F()
    kind = _loss_kind(loss_func, "train_depth_map")
    if kind == 3 and F._rank_world()[1] > 1:
        raise RuntimeError(f"train_depth_map: rmse has no gradient data parallelism (world size {F._rank_world()[1]}): a rank's rmse is "
                           "not the batch's; run one rank, or whole candidates per rank with IM_DP_MODE=candidates")
    c = model.plan.c_in
    files = F._train_shard(glob.glob(os.path.join(train_images_dir, "*.png")))
    loader = F._EpochLoader(files, lambda p: parse_image_depth_map(p, c), F.BATCH_SIZE, F.SEED, ("depth_map", c))
    val = DepthDataset(val_images_dir, c)
    best = {"loss": float("inf")}
    model.depth_loss_kind = kind

    def on_epoch_end(ep, loss):
        val_loss = _evaluate(model, val, kind)[0]
        if val_loss < best["loss"] or not os.path.exists(filepath_h5):
            best["loss"] = min(val_loss, best["loss"])
            if F._rank_world()[0] == 0:
                F.save_model(model, filepath_h5)

    F.fit(model, loader, steps_per_epoch, F.NUM_EPOCHS, kind, on_epoch_end)
    d = F._dist()
    if d:
        d.barrier()
    best_model = F.load_model(filepath_h5, custom_objects={"rmse": rmse, "delta_1.25": delta_metric(1.25)})
    best_model.depth_loss_kind = kind
    rmse_val, mse_val = benchmark_depth_map(best_model, val, val_images_dir, val_pred_dir)
    rmse_test, mse_test = benchmark_depth_map(best_model, DepthDataset(test_images_dir, c), test_images_dir, test_pred_dir)
    rmse_unlabeled, mse_unlabeled = benchmark_depth_map(best_model, DepthDataset(unlabeled_images_dir, c), unlabeled_images_dir,
                                                        unlabeled_pred_dir)
    print(f"{modelname} rmse_val: {rmse_val}")
    F.flush_writes()
    return rmse_val, rmse_test, rmse_unlabeled, mse_val, mse_test, mse_unlabeled


def get_im_prediction_depth_map(models, prepared_image, threshold_multiplier=2):
    """functions.py:6155-6177: the int array of {0,1}, shape (1,H,W,1) for one prepared image, 1 where the models' per-pixel standard
    deviation exceeds threshold_multiplier times its mean.  Handed a batch of B > 1 images the reference forms ONE threshold over the
    whole array; so does this (the kernel is called with batch 1 and height B*H: the element order is the same), and the result is
    (B,H,W,1).  Bit-exact given the models' predictions."""
    F = _F()
    models = list(models)
    _check_n(len(models), "get_im_prediction_depth_map")
    preds = F._stack_predictions(models, F._prep(prepared_image))            # [N,B,H,W,1]
    if preds.shape[-1] != 1:
        raise ValueError("get_im_prediction_depth_map: the models have more than one output map (K > 1 is out of scope)")
    n, b, h, w, _ = preds.shape
    r = im_depth(preds.reshape(n, 1, b * h, w), threshold_multiplier)
    return (r["im"].reshape(b, h, w, 1) != 0).cpu().numpy().astype(int)
