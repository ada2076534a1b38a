"""Host-side mirror of the reference's EvalNet call sites for the HeLa IM++ / AIM++ drivers (HeLa/12_HeLa_IM++.py,
HeLa/14_HeLa_aug_IM++.py): same function names, positional arguments, directory layout, file names and CSV format.
Ensemble inference + IM, EvalNet inference / training, morphology and augmentation run on the GPU through libimk.so;
PNG I/O and the CSV bookkeeping stay on the host.  Re-exported by functions.py."""
import csv
import os
import random
import shutil

import numpy as np
import torch

from . import im as _im
from .augment import augment_batch, draw_params
from .evalnet import EvalNet


def _F():
    from . import functions
    return functions


def _draw_plan(rng, n_images, n_models, n_min_models, n_max_models):
    """per image, in the reference's order of draws (functions.py:3623-3640, 3931-3953): size and members of the
    sub-ensemble, erode and dilate kernel from {0, 3, 5}, the augment-or-not coin"""
    n_max = min(n_max_models, n_models)
    n_min = min(n_min_models, n_max)
    plan = []
    for _ in range(n_images):
        n_sel = rng.randint(n_min, n_max)
        subset = tuple(sorted(rng.sample(range(n_models), n_sel)))
        plan.append((subset, rng.choice([0, 3, 5]), rng.choice([0, 3, 5]), rng.random() < 0.5))
    return plan


def _random_morph(im, plan, idx):
    """erode, then dilate each image's IM with its own kernel (functions.py:3630-3638)"""
    for op, col in (("erode", 1), ("dilate", 2)):
        ks = torch.tensor([plan[i][col] for i in idx], device="cuda")
        for k in (3, 5):
            sel = torch.nonzero(ks == k).flatten()
            if sel.numel():
                im[sel] = _im.morph(im[sel].contiguous(), k, op)
    return im


def _groups(plan):
    g = {}
    for i, p in enumerate(plan):
        g.setdefault(p[0], []).append(i)
    return g


# IMK_TRAINDATA_POOLED, read once: 1 (default) = a loop's images go through ONE model pool in file order (PoolIM: per-image member
# sets, one ensemble call per INFER_BATCH chunk, one imk_morph_var per operation); 0 = the images are grouped by sub-ensemble and
# every group runs its own EnsembleIM (also the route of a pool of more than 16 models, which a member word does not hold).  Both
# routes write the same bytes (tests/test_gpu_traindata_members.py); DESIGN.md has the measurement that chose the default.
POOLED = os.environ.get("IMK_TRAINDATA_POOLED", "1") != "0"


def _var_morph(im, plan, idx):
    """_random_morph in two launches: every image's own window, 0 = untouched"""
    for op, col in (("erode", 1), ("dilate", 2)):
        ks = [plan[i][col] for i in idx]
        if any(ks):
            im = _im.morph_var(im, ks, op)
    return im


def _chunks(plan, batch, pooled):
    """the (subset or None, image indices) chunks of one loop: grouped by sub-ensemble, or the file list in order"""
    if pooled:
        n = len(plan)
        return [(None, list(range(s, min(s + batch, n)))) for s in range(0, n, batch)]
    return [(subset, idx_all[s:s + batch]) for subset, idx_all in _groups(plan).items() for s in range(0, len(idx_all), batch)]


def _draw_aug(plan, batch, draw_kw):
    """the augmentation draws of one loop, per image, made in the grouped route's order (group by group, chunk by chunk, the
    augmented images of a chunk in order) whichever route runs: the random streams do not depend on the route"""
    prm = {}
    for _, idx in _chunks(plan, batch, False):
        sel = [i for i in idx if plan[i][3]]
        if sel:
            for i, q in zip(sel, draw_params(len(sel), **draw_kw)):
                prm[i] = q
    return prm


def _aug_params(prm, sel_images):
    from ._lib import AugParams
    return (AugParams * len(sel_images))(*[prm[i] for i in sel_images])


class _LoopIM:
    """the ensemble stage of a writer: `run(subset, idx, x, ...)` on the pool (per-image members) or on the group's own ensemble"""

    def __init__(self, models, pooled):
        F = _F()
        self.models, self.pooled, self.ensembles = models, pooled and len(models) <= 16, {}
        self.pool = F.PoolIM(models) if self.pooled else None

    def run(self, plan, subset, idx, x, thr, cmp_ge):
        """-> (result dict, IM after the per-image random erosion / dilation)"""
        F = _F()
        if self.pooled:
            r = self.pool.run(x, [plan[i][0] for i in idx], thr, cmp_ge, False, False)
            return r, _var_morph(r["im"], plan, idx)
        if subset not in self.ensembles:
            self.ensembles[subset] = F.EnsembleIM([self.models[j] for j in subset])
        r = self.ensembles[subset].run(x, thr, cmp_ge, False, False)
        return r, _random_morph(r["im"], plan, idx)


# ---------------------------------------------------------------------------------------------------
# training data of the binary EvalNet from ensemble IM predictions (functions.py:3572-3670)
# ---------------------------------------------------------------------------------------------------
def create_training_data_evalnet_im_binary(models, h, w, c, images_path, masks_path, main_output_path, num_loops,
                                           n_min_models=2, n_max_models=4, rgb=True, brightness_range_alpha=(0.6, 1.4),
                                           brightness_range_beta=(-20, 20), max_blur=3, max_noise=20, free_rotation=False,
                                           seed=None):
    """Per loop and labelled image: a random sub-ensemble -> binary IM (>), randomly eroded / dilated -> blocked image +
    mask, IoU of the blocked mask against the ground truth (rounded to 4 decimals) as the label; half of the samples are
    written augmented (geometry on image and mask, photometry on the image).  `{stem}_aug_{loop}.png`, labels.csv."""
    F = _F()
    flip = (not rgb) and c == 3      # rgb=False (functions.py:3611 ff.): the nets see the file's channels in OpenCV's order (BGR)
    rng = random.Random(F.SEED if seed is None else seed)
    np_rng = np.random.default_rng(rng.getrandbits(32))
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    names = sorted(os.listdir(images_path))
    draw_kw = dict(brightness_range_alpha=brightness_range_alpha, brightness_range_beta=brightness_range_beta,
                   max_blur=max_blur, max_noise=max_noise, free_rotation=free_rotation, rng=rng, np_rng=np_rng)
    rows, stage = [], _LoopIM(models, POOLED)
    with F._pool() as pool:
        for nl in range(num_loops):
            plan = _draw_plan(rng, len(names), len(models), n_min_models, n_max_models)
            prm = _draw_aug(plan, F.INFER_BATCH, draw_kw)
            loop_rows = {}
            for subset, idx in _chunks(plan, F.INFER_BATCH, stage.pooled):
                x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(images_path, names[i]) for i in idx], c)).cuda()
                gt = torch.from_numpy(F.read_png_stack(pool, [os.path.join(masks_path, names[i]) for i in idx], 1)).cuda()
                r, im = stage.run(plan, subset, idx, x.flip(-1).contiguous() if flip else x, F.THRESHOLD, False)
                masks, img = r["masks"], x.clone()
                _im.block_apply(im, img, masks)
                pred, g = masks[:, 0] > 0, gt[..., 0] > 0
                inter = (pred & g).sum(dim=(1, 2)).cpu().numpy()
                union = (pred | g).sum(dim=(1, 2)).cpu().numpy()
                ious = inter / (union + 1e-7)
                mk = masks.permute(0, 2, 3, 1).contiguous()
                aug = torch.tensor([plan[i][3] for i in idx], device="cuda")
                sel = torch.nonzero(aug).flatten()
                if sel.numel():      # functions.py:3657-3658
                    o, om = augment_batch(img[sel].contiguous(), mk[sel].contiguous(), _aug_params(prm, [i for i in idx if plan[i][3]]))
                    img[sel], mk[sel] = o, om
                img_np, mk_np = img.cpu().numpy(), mk.cpu().numpy()
                jobs = []
                for row, i in enumerate(idx):
                    out_name = f"{names[i][:-4]}_aug_{nl}.png"
                    loop_rows[i] = (out_name, round(float(ious[row]), 4))
                    jobs.append((os.path.join(iout, out_name), img_np[row]))
                    jobs.append((os.path.join(mout, out_name), mk_np[row, :, :, 0]))
                F.write_pngs_async(jobs)      # on the writer pool: the next batch's decode, network pass and augmentation run meanwhile
            rows += [loop_rows[i] for i in range(len(names))]
    F.flush_writes()
    with open(os.path.join(main_output_path, "labels.csv"), "a", encoding="utf-8", newline="") as f:
        wr = csv.writer(f, delimiter=";")
        for row in rows:
            wr.writerow(row)


# ---------------------------------------------------------------------------------------------------
# multiclass: label helpers (functions.py:4328-4358, 4400-4459) and training data (functions.py:3773-3877)
# ---------------------------------------------------------------------------------------------------
def compute_classwise_IoU(pred, gt, num_classes):
    """functions.py:4328-4358: IoU per class present in gt, rounded to 4 decimals; class 0 scores 1 as soon as the
    prediction has a class-0 pixel and gt has none of them (the prefill), else its IoU like the others."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    iou_list = [0] * num_classes
    if (pred == 0).sum() > 0:
        iou_list[0] = 1
    for cls in range(num_classes):
        if cls in gt:
            inter = np.logical_and(gt == cls, pred == cls).sum()
            union = np.logical_or(gt == cls, pred == cls).sum()
            if union > 0:
                iou_list[cls] = round(inter / union, 4)
    return iou_list


def compute_classwise_detection(mask, num_classes):
    """functions.py:4400-4421: class present on more than 1 % of the pixels"""
    mask = np.asarray(mask)
    return [1 if (mask == cls).sum() > mask.size * 0.01 else 0 for cls in range(num_classes)]


def compute_classwise_detection_im(pred_mask, num_classes, gt_class_counts, threshold):
    """functions.py:4424-4459: class detected if its pixel count in the IM-blocked mask is at least `threshold` of its
    ground-truth count, or at least 10 % of the image; class 0 as soon as one pixel of it is left."""
    pred_mask = np.asarray(pred_mask)
    total = pred_mask.size
    out = [0] * num_classes
    for cls in range(num_classes):
        n = (pred_mask == cls).sum()
        ratio = 0 if gt_class_counts[cls] == 0 else n / gt_class_counts[cls]
        if cls == 0 and n > 0:
            out[cls] = 1
        elif ratio >= threshold:
            out[cls] = 1
        elif n / total >= 0.1:
            out[cls] = 1
    return out


def create_training_data_evalnet_miou_im_multiclass(models, h, w, c, num_classes, images_path, masks_path, main_output_path,
                                                    num_loops, n_min_models=2, n_max_models=4, rgb=True,
                                                    brightness_range_alpha=(0.8, 1.2), brightness_range_beta=(-10, 10),
                                                    max_blur=1, max_noise=10, free_rotation=False, seed=None):
    """Per loop and labelled image: a random sub-ensemble -> argmax agreement IM, randomly eroded / dilated -> blocked
    image + label map; labels = class-wise IoU of the blocked prediction against the ground truth and class-wise
    detection of the IM-blocked ground truth (threshold 0.3); half of the samples are written augmented."""
    F = _F()
    flip = (not rgb) and c == 3      # rgb=False (functions.py:3611 ff.): the nets see the file's channels in OpenCV's order (BGR)
    rng = random.Random(F.SEED if seed is None else seed)
    np_rng = np.random.default_rng(rng.getrandbits(32))
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    names = sorted(os.listdir(images_path))
    draw_kw = dict(brightness_range_alpha=brightness_range_alpha, brightness_range_beta=brightness_range_beta,
                   max_blur=max_blur, max_noise=max_noise, free_rotation=free_rotation, rng=rng, np_rng=np_rng)
    rows, stage = [], _LoopIM(models, POOLED)
    with F._pool() as pool:
        for nl in range(num_loops):
            plan = _draw_plan(rng, len(names), len(models), n_min_models, n_max_models)
            prm = _draw_aug(plan, F.INFER_BATCH, draw_kw)
            loop_rows = {}
            for subset, idx in _chunks(plan, F.INFER_BATCH, stage.pooled):
                x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(images_path, names[i]) for i in idx], c)).cuda()
                gts = list(pool.map(lambda i: F.read_png(os.path.join(masks_path, names[i]), 1)[..., 0], idx))
                r, im = stage.run(plan, subset, idx, x.flip(-1).contiguous() if flip else x, F.THRESHOLD, False)
                masks, img = r["masks"], x.clone()
                _im.block_apply(im, img, masks)
                pred_np, im_np = masks[:, 0].cpu().numpy(), im.cpu().numpy()
                mk = masks.permute(0, 2, 3, 1).contiguous()
                sel = torch.nonzero(torch.tensor([plan[i][3] for i in idx], device="cuda")).flatten()
                if sel.numel():      # functions.py:3859-3860
                    o, om = augment_batch(img[sel].contiguous(), mk[sel].contiguous(), _aug_params(prm, [i for i in idx if plan[i][3]]))
                    img[sel], mk[sel] = o, om
                img_np, mk_np = img.cpu().numpy(), mk.cpu().numpy()
                jobs = []
                for row, i in enumerate(idx):
                    gt = gts[row]
                    ious = compute_classwise_IoU(pred_np[row], gt, num_classes)
                    counts = np.zeros(num_classes)
                    bins = np.bincount(gt.ravel(), minlength=num_classes)
                    counts[:len(bins)] += bins[:num_classes] if len(bins) > num_classes else bins
                    gt_blocked = gt.copy()
                    gt_blocked[im_np[row] > 0] = 0
                    det = compute_classwise_detection_im(gt_blocked, num_classes, counts, 0.3)
                    out_name = f"{names[i][:-4]}_aug_{nl}.png"
                    loop_rows[i] = (out_name, *ious, *det)
                    jobs.append((os.path.join(iout, out_name), img_np[row]))
                    jobs.append((os.path.join(mout, out_name), mk_np[row, :, :, 0]))
                F.write_pngs_async(jobs)      # on the writer pool: the next batch's decode, network pass and augmentation run meanwhile
            rows += [loop_rows[i] for i in range(len(names))]
    F.flush_writes()
    with open(os.path.join(main_output_path, "labels.csv"), "a", encoding="utf-8", newline="") as f:
        wr = csv.writer(f, delimiter=";")
        for row in rows:
            wr.writerow(row)


# ---------------------------------------------------------------------------------------------------
# training data of the mIoU EvalNet from ensemble IM predictions (functions.py:3881-4006)
# ---------------------------------------------------------------------------------------------------
def create_training_data_evalnet_miou_im_hela(models, h, w, c, main_input_path, main_output_path, num_loops, n_min_models=2,
                                              n_max_models=4, brightness_range_alpha=(0.8, 1.2),
                                              brightness_range_beta=(-10, 10), max_blur=1, max_noise=10,
                                              free_rotation=False, seed=None):
    """Per loop and labelled image: a random sub-ensemble (n_min..n_max models) -> three binary IMs (>=) -> combined IM,
    randomly eroded / dilated with a kernel from {0, 3, 5} -> blocked brightfield + masks written as
    `{stem}_aug_{loop}.png`, labels.csv row (name; IoU alive, dead, pos against the ground truth; detection flags).

    Two behaviours of the reference that are kept because they shape EvalNet's inputs:
      * `final_mask * 255` on the uint8 {0,255} masks wraps to {0,1} (functions.py:3939-3942): the masks are written, and
        later read by the EvalNet generator, with values 0 / 1;
      * the randomly augmented copy (functions.py:3983-3990) is overwritten by the plain one under the same name
        (:3993-3996), so only the plain files exist afterwards -- the augmentation is not computed here.
    The sub-ensembles of a loop are batched by model subset."""
    F = _F()
    rng = random.Random(F.SEED if seed is None else seed)
    sub = ("brightfield", "alive", "dead", "mod_position")
    din = {k: os.path.join(main_input_path, k) for k in sub}
    dout = {k: os.path.join(main_output_path, k) for k in sub}
    for d in dout.values():
        os.makedirs(d, exist_ok=True)
    names = sorted(os.listdir(din["brightfield"]))
    rows = []
    stage = _LoopIM(models, POOLED)
    with F._pool() as pool:
        for nl in range(num_loops):
            plan = _draw_plan(rng, len(names), len(models), n_min_models, n_max_models)
            loop_rows = {}
            for subset, idx in _chunks(plan, F.INFER_BATCH, stage.pooled):
                rd = lambda k: torch.from_numpy(np.stack(list(pool.map(
                    lambda i: F.read_png(os.path.join(din[k], names[i]), 1), idx)), 0)).cuda()
                bf, gt = rd("brightfield"), torch.cat([rd("alive"), rd("dead"), rd("mod_position")], 3)
                r, im = stage.run(plan, subset, idx, bf, 0.5, True)     # erode first, then dilate (functions.py:3945-3953)
                masks = r["masks"]
                bf = bf.clone()
                _im.block_apply(im, bf, masks)
                pred = masks > 0
                g = gt.permute(0, 3, 1, 2) > 0
                inter = (pred & g).sum(dim=(2, 3)).cpu().numpy()
                union = (pred | g).sum(dim=(2, 3)).cpu().numpy()
                gt_nz = g.sum(dim=(2, 3)).cpu().numpy()
                ious = inter / (union + 1e-7)                       # get_IoU_binary, functions.py:1767-1788
                det = np.stack([gt_nz[:, 0] >= h * w * 0.01, gt_nz[:, 1] >= h * w * 0.01, gt_nz[:, 2] >= h * w * 0.001], 1)
                bf_np = bf.cpu().numpy()
                m_np = (masks > 0).to(torch.uint8).cpu().numpy()    # {0,1}: the uint8 wrap of `mask * 255`
                jobs = []
                for row, i in enumerate(idx):
                    out_name = f"{names[i][:-4]}_aug_{nl}.png"
                    loop_rows[i] = (out_name, ious[row, 0], ious[row, 1], ious[row, 2], int(det[row, 0]), int(det[row, 1]),
                                    int(det[row, 2]))
                    jobs.append((os.path.join(dout["brightfield"], out_name), bf_np[row, :, :, 0]))
                    for k, key in enumerate(("alive", "dead", "mod_position")):
                        jobs.append((os.path.join(dout[key], out_name), m_np[row, k]))
                F.write_pngs_async(jobs)      # on the writer pool: the next batch's decode, network pass and augmentation run meanwhile
            rows += [loop_rows[i] for i in range(len(names))]
    F.flush_writes()
    with open(os.path.join(main_output_path, "labels.csv"), "a", encoding="utf-8", newline="") as f:
        wr = csv.writer(f, delimiter=";")
        for row in rows:
            wr.writerow(row)


# ---------------------------------------------------------------------------------------------------
# EvalNet training (functions.py:4673-4722 with the generator of :4823-4882)
# ---------------------------------------------------------------------------------------------------
def _read_labels(main_path, num_classes=3):
    rows = []
    with open(os.path.join(main_path, "labels.csv"), encoding="utf-8", newline="") as f:
        for r in csv.reader(f, delimiter=";"):
            if r:
                rows.append((r[0], np.asarray(r[1:1 + 2 * num_classes], dtype=np.float32)))
    return rows


def _cached_evalnet_set(kind, main_path, load):
    """the EvalNet candidates of a run train on the same two directories: decode them once (device decode cache, keyed by the
    directory, its labels.csv and what `kind` of set it is read as)"""
    F = _F()
    st = os.stat(os.path.join(main_path, "labels.csv"))
    key = ("evalnet", kind, os.path.abspath(main_path), st.st_size, st.st_mtime_ns)
    with F._CACHE_LOCK:
        hit = F._DECODE_CACHE.get(key)
        if hit is not None:
            return tuple(F._used_here(hit))
        out = list(load())
        F._uploaded()
        F._decode_cache_put(key, out)
        return tuple(out)


def _load_evalnet_set(main_path, rows, pool):
    """brightfield (grey) [N,H,W,1], masks alive|dead|mod_position [N,H,W,3] (raw uint8 values), labels [N,6] on the device"""
    F = _F()

    def one(r):
        mask_name = r[0]
        image_name = mask_name.split("___")[0] + ".png" if "___" in mask_name else mask_name   # functions.py:4863-4866
        bf = F.read_png(os.path.join(main_path, "brightfield", image_name), 1)
        gt = np.concatenate([F.read_png(os.path.join(main_path, k, mask_name), 1) for k in ("alive", "dead", "mod_position")], 2)
        return bf, gt

    items = list(pool.map(one, rows))
    xa = torch.from_numpy(np.stack([i[0] for i in items], 0)).cuda()
    xb = torch.from_numpy(np.stack([i[1] for i in items], 0)).cuda()
    y = torch.from_numpy(np.stack([r[1] for r in rows], 0)).cuda()
    return xa, xb, y


def _evaluate_evalnet(model, xa, xb, y, batch_size, steps, k):
    """model.evaluate(generator, steps): inference-mode forward over `steps` batches -> (total, mse, bce, mae, acc)"""
    rows = []
    for s in range(steps):
        sl = slice(s * batch_size, (s + 1) * batch_size)
        out = model.predict_device(xa[sl].contiguous(), xb[sl].contiguous()).double()
        t = y[sl].double()
        p_iou, p_det, t_iou, t_det = out[:, :k], out[:, k:], t[:, :k], t[:, k:]
        pc = p_det.clamp(1e-7, 1 - 1e-7)
        rows.append(torch.stack([((p_iou - t_iou) ** 2).mean(), -(t_det * pc.log() + (1 - t_det) * (1 - pc).log()).mean(),
                                 (p_iou - t_iou).abs().mean(), ((p_det > 0.5).double() == t_det).double().mean()]))
    tot = np.zeros(4)
    for r in (torch.stack(rows).cpu().numpy() if rows else []):      # one transfer; the batches' float64 values summed in order
        tot += r
    mse, bce, mae, acc = tot / max(steps, 1)
    return mse + bce, mse, bce, mae, acc


def save_evalnet(model, path):
    """ModelCheckpoint's model.save(path) for the EvalNet; IMK_MODEL_FORMAT=keras_h5: a Keras save_weights HDF5 file (keras_h5.py)"""
    if os.environ.get("IMK_MODEL_FORMAT", "safetensors") == "keras_h5":
        from .keras_h5 import save_keras_evalnet_weights
        return save_keras_evalnet_weights(model, path)
    from safetensors.torch import save_file
    p = model.plan
    meta = {"net": "evalnet", "h": str(p.h), "w": str(p.w), "ca": str(p.ca), "cb": str(p.cb), "n_out": str(p.n_out),
            "alpha": repr(p.alpha), "two_heads": str(int(p.two_heads)), "normalize_a": str(p.cfg.normalize_a),
            "normalize_b": str(p.cfg.normalize_b), "b_onehot": str(int(p.b_onehot))}
    if p.arch != "v1":          # get_evalnet_miou_v2; a v1 file stays byte for byte what it was
        meta["arch"] = p.arch
    save_file({k: v.contiguous() for k, v in model.state_dict().items()}, path, metadata=meta)


def load_evalnet(path, device="cuda"):
    """load_model for an EvalNet file: this package's safetensors, or a Keras HDF5 checkpoint of evalnet.get_evalnet / get_evalnet_miou /
    get_evalnet_miou_v2"""
    from . import h5lite
    if h5lite.is_hdf5(path):
        from .keras_h5 import load_keras_evalnet
        return load_keras_evalnet(path, device=device)
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        meta = f.metadata()
        sd = {k: f.get_tensor(k) for k in f.keys()}
    m = EvalNet(int(meta["h"]), int(meta["w"]), int(meta["ca"]), int(meta["cb"]), int(meta["n_out"]), float(meta["alpha"]),
                bool(int(meta["two_heads"])), bool(int(meta["normalize_a"])), bool(int(meta["normalize_b"])), seed=0, device=device,
                b_onehot=bool(int(meta.get("b_onehot", "0"))), arch=meta.get("arch", "v1"))
    m.load_state_dict(sd)
    return m


def _fit_evalnet(model, train_set, val_set, filepath_h5, batch_size, epochs, evaluate, monitor, seed):
    """model.fit(train_generator, validation_data=val_generator, steps_per_epoch=len//batch, validation_steps=len//batch,
    callbacks=[ModelCheckpoint(save_best_only, monitor, mode='min')]) then load_model + evaluate.  `evaluate(model, set,
    steps)` returns the metric tuple, `monitor` indexes it.  Every rank of a multi-GPU launch trains the same model from
    the same seed (the sets are small)."""
    F = _F()
    rng = np.random.default_rng(F.SEED if seed is None else seed)
    xa, xb, y = train_set
    n_train, n_val = xa.shape[0], val_set[0].shape[0]
    steps, val_steps = n_train // batch_size, n_val // batch_size
    vperm = torch.as_tensor(rng.permutation(n_val), device="cuda")          # the validation generator shuffles too
    val_set = tuple(t[vperm] for t in val_set)
    model.init_train_state()
    best = float("inf")
    order = []
    for ep in range(epochs):
        for _ in range(steps):
            if not order:      # dataframe.sample(frac=1): a new shuffled pass, one short batch at its end (functions.py:4794-4799)
                perm = torch.as_tensor(rng.permutation(n_train), device="cuda")
                pa, pb, py = xa[perm], xb[perm], y[perm]
                order = [(i, min(i + batch_size, n_train)) for i in range(0, n_train, batch_size)]
            lo, hi = order.pop(0)
            model.fwd_bwd(pa[lo:hi], pb[lo:hi], py[lo:hi])
            model.adamw_step(F.LR, F.WD)
        val = evaluate(model, val_set, val_steps)[monitor]
        if val < best:
            best = val
            if F._rank_world()[0] == 0:
                save_evalnet(model, filepath_h5)
    d = F._dist()
    if d:
        d.barrier()
    return tuple(float(v) for v in evaluate(load_evalnet(filepath_h5), val_set, val_steps))


def train_evalnet_miou_model_hela(model, train_main_path, val_main_path, filepath_h5, batch_size, epochs, seed=None):
    """functions.py:4673-4722: AdamW(LR, WD), loss ['mse', 'binary_crossentropy'], best epoch by val_loss (min), then
    the best model evaluated on the validation generator.  Returns (total_loss, iou_loss, detection_loss, iou_mae,
    detection_acc)."""
    F = _F()
    k = model.plan.n_out
    with F._pool() as pool:
        tr = _cached_evalnet_set(("hela", k), train_main_path, lambda: _load_evalnet_set(train_main_path, _read_labels(train_main_path, k), pool))
        va = _cached_evalnet_set(("hela", k), val_main_path, lambda: _load_evalnet_set(val_main_path, _read_labels(val_main_path, k), pool))
    ev = lambda m, st, steps: _evaluate_evalnet(m, st[0], st[1], st[2], batch_size, steps, k)
    return _fit_evalnet(model, tr, va, filepath_h5, batch_size, epochs, ev, 0, seed)


def _load_binary_evalnet_set(main_path, pool):
    """images (RGB) [N,H,W,3], masks (grey) [N,H,W,1], labels [N,1] (functions.py:4778-4820)"""
    F = _F()
    rows = []
    with open(os.path.join(main_path, "labels.csv"), encoding="utf-8", newline="") as f:
        for r in csv.reader(f, delimiter=";"):
            if r:
                rows.append((r[0], float(r[1])))

    def one(r):
        mask_name = r[0]
        image_name = mask_name.split("___")[0] + ".png" if "___" in mask_name else mask_name
        return (F.read_png(os.path.join(main_path, "images", image_name), 3), F.read_png(os.path.join(main_path, "masks", mask_name), 1))

    items = list(pool.map(one, rows))
    return (torch.from_numpy(np.stack([i[0] for i in items], 0)).cuda(), torch.from_numpy(np.stack([i[1] for i in items], 0)).cuda(),
            torch.tensor([[r[1]] for r in rows], dtype=torch.float32, device="cuda"))


def _mse_mae_evaluator(batch_size):
    """model.evaluate of a one-unit EvalNet compiled with loss 'mean_squared_error', metrics ['mean_absolute_error'] -> (mse, mae)"""
    def ev(m, st, steps):
        rows = []
        for s in range(steps):
            sl = slice(s * batch_size, (s + 1) * batch_size)
            d = m.predict_device(st[0][sl].contiguous(), st[1][sl].contiguous()).double() - st[2][sl].double()
            rows.append(torch.stack([(d ** 2).mean(), d.abs().mean()]))
        tot = np.zeros(2)
        for r in (torch.stack(rows).cpu().numpy() if rows else []):      # one transfer; summed on the host in batch order
            tot += r
        return tuple(tot / max(steps, 1))
    return ev


def train_evalnet_ISIC_2018(model, train_main_path, val_main_path, filepath_h5, batch_size, epochs, seed=None):
    """functions.py:4464-4506: loss 'mean_squared_error', metric 'mean_absolute_error', best epoch by
    val_mean_absolute_error (min).  Returns (mse, mae) of the best model on the validation generator."""
    F = _F()
    with F._pool() as pool:
        tr = _cached_evalnet_set("binary", train_main_path, lambda: _load_binary_evalnet_set(train_main_path, pool))
        va = _cached_evalnet_set("binary", val_main_path, lambda: _load_binary_evalnet_set(val_main_path, pool))
    return _fit_evalnet(model, tr, va, filepath_h5, batch_size, epochs, _mse_mae_evaluator(batch_size), 1, seed)


def _load_multiclass_evalnet_set(main_path, num_classes, pool):
    """images (RGB) [N,H,W,3], class-id masks [N,H,W,1] (one-hot on the device), labels [N,2K] (functions.py:4940-4984)"""
    F = _F()
    rows = _read_labels(main_path, num_classes)

    def one(r):
        mask_name = r[0]
        image_name = mask_name.split("___")[0] + ".png" if "___" in mask_name else mask_name
        return (F.read_png(os.path.join(main_path, "images", image_name), 3), F.read_png(os.path.join(main_path, "masks", mask_name), 1))

    items = list(pool.map(one, rows))
    return (torch.from_numpy(np.stack([i[0] for i in items], 0)).cuda(), torch.from_numpy(np.stack([i[1] for i in items], 0)).cuda(),
            torch.from_numpy(np.stack([r[1] for r in rows], 0)).cuda())


def train_evalnet_miou_model_multiclass(model, h, w, train_main_path, val_main_path, filepath_h5, batch_size, num_classes, epochs,
                                        seed=None):
    """functions.py:4726-4775: like the HeLa variant, masks are label maps fed as one-hot stacks.  Returns (total_loss,
    iou_loss, detection_loss, iou_mae, detection_acc)."""
    F = _F()
    if not model.plan.b_onehot or model.plan.n_out != num_classes:
        raise ValueError("needs a get_evalnet_miou(..., inputB_channels=num_classes) model with a one-hot input B")
    with F._pool() as pool:
        tr = _cached_evalnet_set(("multi", num_classes), train_main_path, lambda: _load_multiclass_evalnet_set(train_main_path, num_classes, pool))
        va = _cached_evalnet_set(("multi", num_classes), val_main_path, lambda: _load_multiclass_evalnet_set(val_main_path, num_classes, pool))
    ev = lambda m, st, steps: _evaluate_evalnet(m, st[0], st[1], st[2], batch_size, steps, num_classes)
    return _fit_evalnet(model, tr, va, filepath_h5, batch_size, epochs, ev, 0, seed)


# ---------------------------------------------------------------------------------------------------
# EvalNet-weighted augmentation of the pseudo-labelled set (functions.py:5837-5941)
# ---------------------------------------------------------------------------------------------------
def num_augs_from_miou(miou, min_threshold, max_threshold):
    """functions.py:5921-5930"""
    step = (max_threshold - min_threshold) / 5
    if miou > max_threshold:
        n = 5
    elif miou > min_threshold:
        n = 1 + int((miou - min_threshold) / step)
    else:
        n = 1
    return min(n, 5)


def create_augment_images_and_masks_with_evalnet_ensemble_hela(evalnets, h, w, c, min_threshold, max_threshold,
                                                               main_input_path, main_output_path,
                                                               brightness_range_alpha=(0.6, 1.4),
                                                               brightness_range_beta=(-20, 20), max_blur=3, max_noise=20,
                                                               free_rotation=True):
    """Every pseudo-labelled sample gets 1..5 augmented copies `{stem}___{j}.png`, the number growing with the mean
    IoU the EvalNet ensemble predicts for it (classes whose mean detection score is below 0.5 do not count).
    EvalNet sees the masks as 0 / 1 here (mask / 255, functions.py:5881-5883)."""
    F = _F()
    sub = ("brightfield", "alive", "dead", "mod_position")
    din = {k: os.path.join(main_input_path, k) for k in sub}
    dout = {k: os.path.join(main_output_path, k) for k in sub}
    for d in dout.values():
        os.makedirs(d, exist_ok=True)
    mine = F.shard_list(os.listdir(din["brightfield"]))
    draw_kw = dict(brightness_range_alpha=brightness_range_alpha, brightness_range_beta=brightness_range_beta,
                   max_blur=max_blur, max_noise=max_noise, free_rotation=free_rotation)
    with F._pool() as pool:
        for s in range(0, len(mine), F.INFER_BATCH):
            chunk = mine[s:s + F.INFER_BATCH]
            rd = lambda k: torch.from_numpy(F.read_png_stack(pool, [os.path.join(din[k], n) for n in chunk], 1)).cuda()
            bf = rd("brightfield")
            m255 = torch.cat([rd("alive"), rd("dead"), rd("mod_position")], 3)
            m01 = (m255.float() / 255.0).round().clamp(0, 255).to(torch.uint8)      # what predict() receives: mask / 255
            outs = torch.stack([e.predict_device(bf, m01) for e in evalnets], 0).double().mean(0).cpu().numpy()
            k = outs.shape[1] // 2
            n_augs = []
            for row in outs:
                valid = [row[ci] for ci in range(k) if row[k + ci] >= 0.5]
                n_augs.append(num_augs_from_miou(sum(valid) / len(valid) if valid else 0, min_threshold, max_threshold))
            n_augs = torch.tensor(n_augs, device="cuda")
            jobs = []
            for j in range(5):
                sel = torch.nonzero(n_augs > j).flatten()
                if not sel.numel():
                    break
                o, om = augment_batch(bf[sel].contiguous(), m255[sel].contiguous(), draw_params(int(sel.numel()), **draw_kw))
                o, om = o.cpu().numpy(), ((om >= 128).to(torch.uint8) * 255).cpu().numpy()   # (mask/255 >= 0.5) * 255
                for row, i in enumerate(sel.tolist()):
                    name = f"{chunk[i][:-4]}___{j}.png"
                    jobs.append((os.path.join(dout["brightfield"], name), o[row, :, :, 0]))
                    for ci, key in enumerate(("alive", "dead", "mod_position")):
                        jobs.append((os.path.join(dout[key], name), om[row, :, :, ci]))
            F.write_pngs_async(jobs)      # on the writer pool: the next batch's decode, network pass and augmentation run meanwhile
    F.flush_writes()
    if F._dist():
        F._dist().barrier()


def create_augment_images_and_masks_with_evalnet_ensemble_binary(evalnets, h, w, c, min_threshold, max_threshold,
                                                                 main_input_path, main_output_path,
                                                                 brightness_range_alpha=(0.6, 1.4),
                                                                 brightness_range_beta=(-20, 20), max_blur=3, max_noise=20,
                                                                 free_rotation=True, rgb=True):
    """functions.py:5684-5757: 1..5 augmented copies `{stem}___{j}.png` of every pseudo-labelled pair, the number growing
    with the IoU the EvalNet ensemble predicts for (image, mask)."""
    F = _F()
    flip = (not rgb) and c == 3      # rgb=False (functions.py:3611 ff.): the nets see the file's channels in OpenCV's order (BGR)
    iin, min_ = os.path.join(main_input_path, "images"), os.path.join(main_input_path, "masks")
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    mine = F.shard_list(os.listdir(iin))
    draw_kw = dict(brightness_range_alpha=brightness_range_alpha, brightness_range_beta=brightness_range_beta,
                   max_blur=max_blur, max_noise=max_noise, free_rotation=free_rotation)
    with F._pool() as pool:
        for s in range(0, len(mine), F.INFER_BATCH):
            chunk = mine[s:s + F.INFER_BATCH]
            x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(iin, n) for n in chunk], c)).cuda()
            m = torch.from_numpy(F.read_png_stack(pool, [os.path.join(min_, n) for n in chunk], 1)).cuda()
            xin = x.flip(-1).contiguous() if flip else x
            mean_iou = torch.stack([e.predict_device(xin, m) for e in evalnets], 0).double().mean(0)[:, 0].cpu().numpy()
            n_augs = [num_augs_from_miou(v, min_threshold, max_threshold) for v in mean_iou]
            # on the writer pool: the next batch's decode, network pass and augmentation run meanwhile
            F.write_pngs_async(_write_augmented(chunk, x, m, n_augs, draw_kw, iout, mout))
    F.flush_writes()
    if F._dist():
        F._dist().barrier()


def create_augment_images_and_masks_with_gt(main_gt_input_path, min_threshold, max_threshold, main_input_path, main_output_path,
                                            brightness_range_alpha=(0.6, 1.4), brightness_range_beta=(-20, 20), max_blur=3,
                                            max_noise=20, free_rotation=False, rgb=True):
    """functions.py:6057-6121 (SUIM/16_SUIM_GT_IM++.py: a "perfect EvalNet"): the number of augmented copies `{stem}___{j}.png`
    of a pseudo-labelled pair follows the IoU (get_IoU_multi_unique) of its pseudo-label against the ground-truth mask with the
    IM pixels blanked.  `rgb` only chooses the channel order the reference hands to nobody here (the augmented image is made
    from the file's own order): accepted, no effect."""
    F = _F()
    iin, min_, imin = (os.path.join(main_input_path, k) for k in ("images", "masks", "im"))
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    mine = F.shard_list(os.listdir(iin))
    draw_kw = dict(brightness_range_alpha=brightness_range_alpha, brightness_range_beta=brightness_range_beta,
                   max_blur=max_blur, max_noise=max_noise, free_rotation=free_rotation)
    with F._pool() as pool:
        for s in range(0, len(mine), F.INFER_BATCH):
            chunk = mine[s:s + F.INFER_BATCH]
            rd = lambda d, ch: F.read_png_stack(pool, [os.path.join(d, n) for n in chunk], ch)
            x_np, m_np, im_np, gt_np = rd(iin, 3), rd(min_, 1), rd(imin, 1), rd(main_gt_input_path, 1)
            n_augs = []
            for i in range(len(chunk)):
                gt = gt_np[i, :, :, 0].copy()
                gt[im_np[i, :, :, 0] > 0] = 0                                  # :6102
                n_augs.append(num_augs_from_miou(F.get_IoU_multi_unique(m_np[i, :, :, 0], gt), min_threshold, max_threshold))
            x, m = torch.from_numpy(x_np).cuda(), torch.from_numpy(m_np).cuda()
            # on the writer pool: the next batch's decode, network pass and augmentation run meanwhile
            F.write_pngs_async(_write_augmented(chunk, x, m, n_augs, draw_kw, iout, mout))
    F.flush_writes()
    if F._dist():
        F._dist().barrier()


def create_augment_images_and_masks_with_evalnet_ensemble_multiclass(evalnets, h, w, c, num_classes, min_threshold,
                                                                     max_threshold, main_input_path, main_output_path,
                                                                     brightness_range_alpha=(0.6, 1.4),
                                                                     brightness_range_beta=(-20, 20), max_blur=3,
                                                                     max_noise=20, free_rotation=False, rgb=True):
    """functions.py:5946-6035: the number of augmented copies follows the mean predicted IoU over the classes > 0 whose
    mean detection score is at least 0.5."""
    F = _F()
    flip = (not rgb) and c == 3      # rgb=False (functions.py:3611 ff.): the nets see the file's channels in OpenCV's order (BGR)
    iin, min_ = os.path.join(main_input_path, "images"), os.path.join(main_input_path, "masks")
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    mine = F.shard_list(os.listdir(iin))
    draw_kw = dict(brightness_range_alpha=brightness_range_alpha, brightness_range_beta=brightness_range_beta,
                   max_blur=max_blur, max_noise=max_noise, free_rotation=free_rotation)
    with F._pool() as pool:
        for s in range(0, len(mine), F.INFER_BATCH):
            chunk = mine[s:s + F.INFER_BATCH]
            x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(iin, n) for n in chunk], c)).cuda()
            m = torch.from_numpy(F.read_png_stack(pool, [os.path.join(min_, n) for n in chunk], 1)).cuda()
            xin = x.flip(-1).contiguous() if flip else x
            outs = torch.stack([e.predict_device(xin, m) for e in evalnets], 0).double().mean(0).cpu().numpy()
            n_augs = []
            for row in outs:
                valid = [row[ci] for ci in range(1, num_classes) if row[num_classes + ci] >= 0.5]
                n_augs.append(num_augs_from_miou(sum(valid) / len(valid) if valid else 0.0, min_threshold, max_threshold))
            # on the writer pool: the next batch's decode, network pass and augmentation run meanwhile
            F.write_pngs_async(_write_augmented(chunk, x, m, n_augs, draw_kw, iout, mout))
    F.flush_writes()
    if F._dist():
        F._dist().barrier()


# ---------------------------------------------------------------------------------------------------
# EvalNet-ensemble selection baseline (functions.py:5070-5155, 5323-5577; */1x_*_evalnet*_ensemble.py): for every unlabeled
# image the candidate masks of several models (and, where one was selected, the last generation's) are scored by the EvalNet
# ensemble; the candidate with the best mean score is kept if that score reaches the threshold.  Scoring, arg-max, threshold and
# the gather of the chosen mask are one call per batch (evalnet.CandidateScorer: imk_evalnet_forward_select).
# ---------------------------------------------------------------------------------------------------
SELECT_BATCH = int(os.environ.get("IMK_SELECT_BATCH", 8))      # images per call; every image brings up to 11 candidates


def _copy_last_generation(last_gen_main_path, main_output_path, subs):
    """the last generation's selected set goes in first (functions.py:5099-5102); rank 0 copies, the others wait"""
    F = _F()
    if last_gen_main_path != '' and F._rank_world()[0] == 0:
        for name in os.listdir(os.path.join(last_gen_main_path, subs[0])):
            for k in subs:
                shutil.copy(os.path.join(last_gen_main_path, k, name), os.path.join(main_output_path, k, name))
    if F._dist():
        F._dist().barrier()


def _run_selection(evalnets, images_path, c, flip, threshold, load, emit, mode=None):
    """Shared body of the selection writers: this rank's shard of the file list in batches of SELECT_BATCH images;
    load(pool, chunk) -> (input B of the nets u8 [B,M,...], what is written for a candidate u8 [B,M,...], candidates per image);
    emit(name, chosen bytes) -> PNG jobs of a kept image.  mode: the rule (evalnet.SELECT_*); None = the ensemble rule of the nets' heads."""
    from .evalnet import SELECT_MAX_CAND, CandidateScorer
    F = _F()
    scorer = CandidateScorer(evalnets)
    mine = F.shard_list(os.listdir(images_path))
    with F._pool() as pool:
        for s in range(0, len(mine), SELECT_BATCH):
            chunk = mine[s:s + SELECT_BATCH]
            x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(images_path, n) for n in chunk], c)).cuda()
            if flip:
                x = x.flip(-1).contiguous()
            xb, cand, counts = load(pool, chunk)
            b, m = xb.shape[:2]
            if m > SELECT_MAX_CAND:
                raise ValueError(f"{m} candidates per image: imk_evalnet_forward_select takes at most {SELECT_MAX_CAND}")
            cand = cand.reshape(b, m, -1)
            nbytes = cand.shape[2]
            if nbytes % 16:      # the gather moves 16 bytes at a time
                cand = torch.nn.functional.pad(cand, (0, 16 - nbytes % 16))
            cnt = None if all(v == m for v in counts) else torch.tensor(counts, dtype=torch.int32, device="cuda")
            _, _, keep, out = scorer.run(x, xb, cand.contiguous(), threshold, cnt, mode)
            keep, out = keep.cpu().numpy(), out.cpu().numpy()[:, :nbytes]
            jobs = []
            for i, name in enumerate(chunk):
                if keep[i]:
                    jobs += emit(name, out[i])
            F.write_pngs_async(jobs)      # encoded while the next batch is decoded and scored
    F.flush_writes()
    if F._dist():
        F._dist().barrier()


def _mask_candidates(mask_paths, masks_path_out, h, w, class_ids):
    """load() of the binary and multi-class writers: one gray PNG per candidate; the file of the same name in the output's masks/
    (the last generation's choice, copied in before) is one more candidate where it exists (functions.py:5120-5124)"""
    F = _F()

    def load(pool, chunk):
        has_last = [os.path.isfile(os.path.join(masks_path_out, n)) for n in chunk]
        m = len(mask_paths) + int(any(has_last))
        paths = []
        for n, hl in zip(chunk, has_last):
            paths += [os.path.join(d, n) for d in mask_paths]
            if m > len(mask_paths):      # without a last-generation mask the slot repeats candidate 0 and is excluded by its count
                paths.append(os.path.join(masks_path_out if hl else mask_paths[0], n))
        t = torch.from_numpy(F.read_png_stack(pool, paths, 1)).cuda().reshape(len(chunk), m, h, w, 1)
        return (t[..., 0].contiguous() if class_ids else t), t, [len(mask_paths) + int(hl) for hl in has_last]
    return load


def _takes_class_ids(evalnets):
    return all(isinstance(e, EvalNet) and e.plan.b_onehot for e in evalnets)


def create_training_data_for_segnet_with_ensemble_binary(evalnets, h, w, c, images_path, mask_paths, main_output_path, threshold,
                                                         last_gen_main_path='', rgb=True):
    """functions.py:5070-5152: images/ (the file, copied) and masks/ (the candidate with the best mean predicted IoU) of every
    unlabeled image whose best mean reaches `threshold`."""
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    _copy_last_generation(last_gen_main_path, main_output_path, ("images", "masks"))

    def emit(name, chosen):
        shutil.copy(os.path.join(images_path, name), os.path.join(iout, name))
        return [(os.path.join(mout, name), chosen.reshape(h, w))]
    _run_selection(evalnets, images_path, c, (not rgb) and c == 3, threshold, _mask_candidates(mask_paths, mout, h, w, False), emit)


def create_training_data_for_segnet_with_miou_ensemble_multiclass(evalnets, h, w, c, num_classes, images_path, mask_paths,
                                                                  main_output_path, threshold, last_gen_main_path='', rgb=True):
    """functions.py:5468-5577: as the binary writer with class-id masks; the score of a candidate is the mean of the ensemble's mean
    predicted IoUs over the classes whose mean detection score is at least 0.5 (0 if there is none)."""
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    _copy_last_generation(last_gen_main_path, main_output_path, ("images", "masks"))
    class_ids = _takes_class_ids(evalnets)

    def emit(name, chosen):
        shutil.copy(os.path.join(images_path, name), os.path.join(iout, name))
        return [(os.path.join(mout, name), chosen.reshape(h, w))]
    load = _mask_candidates(mask_paths, mout, h, w, class_ids)
    if not class_ids:      # models that take the one-hot stack (functions.py:5528)
        ids = load

        def load(pool, chunk):
            xb, cand, counts = ids(pool, chunk)
            return (xb == torch.arange(num_classes, device=xb.device, dtype=xb.dtype)).to(torch.uint8), cand, counts
    _run_selection(evalnets, images_path, c, (not rgb) and c == 3, threshold, load, emit)


def create_training_data_for_segnet_with_miou_ensemble_hela(evalnets, h, w, c, bf_images_path_in, mask_paths_in, main_output_path,
                                                            threshold, last_gen_main_path='', max_pos_circle_size=8,
                                                            min_pos_circle_size=3):
    """functions.py:5323-5465: the nets see alive / dead / mod_position as 0 / 1 (mask / 255), the chosen alive and dead planes are
    written as 0 / 255 and the position mask is redrawn from the chosen position plane: a filled circle per blob, radius
    min_dist // 4 within [min, max], a lone cell drawn with distance 99."""
    F = _F()
    planes = ("alive", "dead", "mod_position")
    out = {k: os.path.join(main_output_path, k) for k in ("brightfield",) + planes}
    for d in out.values():
        os.makedirs(d, exist_ok=True)
    _copy_last_generation(last_gen_main_path, main_output_path, ("brightfield",) + planes)

    def load(pool, chunk):
        has_last = [last_gen_main_path != '' and os.path.exists(os.path.join(out["alive"], n)) for n in chunk]
        m = len(mask_paths_in) + int(any(has_last))
        paths = []
        for n, hl in zip(chunk, has_last):
            roots = list(mask_paths_in)
            if m > len(mask_paths_in):
                roots.append(main_output_path if hl else mask_paths_in[0])
            paths += [os.path.join(r, k, n) for r in roots for k in planes]
        t = torch.from_numpy(F.read_png_stack(pool, paths, 1)).cuda().reshape(len(chunk), m, 3, h, w)
        m01 = (t.float() / 255.0).round().clamp(0, 255).to(torch.uint8)      # what predict() receives: mask / 255
        return m01.permute(0, 1, 3, 4, 2).contiguous(), m01 * 255, [len(mask_paths_in) + int(hl) for hl in has_last]

    def emit(name, chosen):
        alive, dead, pos = chosen.reshape(3, h, w)
        shutil.copy(os.path.join(bf_images_path_in, name), os.path.join(out["brightfield"], name))
        return [(os.path.join(out["alive"], name), alive), (os.path.join(out["dead"], name), dead),
                (os.path.join(out["mod_position"], name), F._hela_vote_positions(pos, max_pos_circle_size, min_pos_circle_size))]
    _run_selection(evalnets, bf_images_path_in, c, False, threshold, load, emit)


# ---------------------------------------------------------------------------------------------------
# single-EvalNet selection baseline (functions.py:4991-5063, 5583-5677; ISIC_2018/10_ISIC_2018_evalnet.py, SUIM/11_SUIM_evalnet_miou.py):
# the writers above with one EvalNet.  ISIC: the arg-max of the one net's predicted IoU = SELECT_IOU with N = 1.  Multi-class: a rule of
# its own (SELECT_CONF_GATED): a class counts if its detection value, averaged over the image's candidates, reaches 0.03, and a
# candidate's score is the mean of its detection values over the counting classes -- the predicted ious are not used.
# ---------------------------------------------------------------------------------------------------
def create_training_data_for_segnet_ISIC_2018(evalnet_model, h, w, c, images_path, mask_paths, main_output_path, threshold,
                                              last_gen_main_path='', rgb=True):
    """functions.py:4991-5063: images/ (the file, copied) and masks/ (the candidate with the best predicted IoU) of every unlabeled
    image whose best predicted IoU reaches `threshold`."""
    from .evalnet import SELECT_IOU
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    _copy_last_generation(last_gen_main_path, main_output_path, ("images", "masks"))

    def emit(name, chosen):
        shutil.copy(os.path.join(images_path, name), os.path.join(iout, name))
        return [(os.path.join(mout, name), chosen.reshape(h, w))]
    _run_selection([evalnet_model], images_path, c, (not rgb) and c == 3, threshold, _mask_candidates(mask_paths, mout, h, w, False), emit,
                   SELECT_IOU)


def create_training_data_by_evalnet_miou_for_segnet_multiclass(evalnet_model, h, w, c, num_classes, images_path, mask_paths,
                                                               main_output_path, miou_threshold, last_gen_main_path='', rgb=True):
    """functions.py:5583-5677: as the writer above with class-id masks; a class counts for an image if the mean of its detection
    value over the image's candidates is at least 0.03, the score of a candidate is the mean of its detection values over the counting
    classes (0 if there is none), and the best candidate is kept if its score reaches `miou_threshold`."""
    from .evalnet import SELECT_CONF_GATED
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    _copy_last_generation(last_gen_main_path, main_output_path, ("images", "masks"))
    class_ids = _takes_class_ids([evalnet_model])

    def emit(name, chosen):
        shutil.copy(os.path.join(images_path, name), os.path.join(iout, name))
        return [(os.path.join(mout, name), chosen.reshape(h, w))]
    load = _mask_candidates(mask_paths, mout, h, w, class_ids)
    if not class_ids:      # models that take the one-hot stack (functions.py:5642)
        ids = load

        def load(pool, chunk):
            xb, cand, counts = ids(pool, chunk)
            return (xb == torch.arange(num_classes, device=xb.device, dtype=xb.dtype)).to(torch.uint8), cand, counts
    _run_selection([evalnet_model], images_path, c, (not rgb) and c == 3, miou_threshold, load, emit, SELECT_CONF_GATED)


# ---------------------------------------------------------------------------------------------------
# training data of the EvalNets from single models' predictions on the labelled set (functions.py:3419-3492)
# ---------------------------------------------------------------------------------------------------
def _pred_name(imagename, i):
    """functions.py:3466-3472: predictions of the augmented-subset models (i >= 10) on augmented files fold the copy number in"""
    if i >= 10 and 'aug' in imagename:
        return f'{imagename[:-10]}___{i}_{imagename[-6:-4]}.png'
    return f'{imagename[:-4]}___{i}.png'


def _append_labels(main_output_path, rows):
    F = _F()
    rows = F._gather_lists(rows)[0] if F._dist() else rows
    if F._rank_world()[0] == 0:
        with open(os.path.join(main_output_path, 'labels.csv'), 'a', encoding='utf-8', newline='') as f:
            csv.writer(f, delimiter=';').writerows(rows)
    if F._dist():
        F._dist().barrier()


def create_training_data_evalnet_ISIC_2018(model, h, w, c, images_path, masks_path, main_output_path, i, rgb=True):
    """functions.py:3419-3492: masks/<stem>___{i}.png = (p > 0.5) * 255 of every labelled image with its IoU against the ground truth
    (rounded to 4) appended to labels.csv; for i == 0 also the labelled pairs themselves with IoU 1.0."""
    from . import evaluate as _ev
    F = _F()
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    names = os.listdir(images_path)
    mine = F.shard_list(names)
    rows = []
    with F._pool() as pool:
        for s in range(0, len(mine), 64):
            chunk = mine[s:s + 64]
            x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(images_path, n) for n in chunk], c)).cuda()
            g = torch.from_numpy(F.read_png_stack(pool, [os.path.join(masks_path, n) for n in chunk], 1)).cuda()
            if (not rgb) and c == 3:
                x = x.flip(-1).contiguous()
            pred, counts = _ev.eval_binary(model.predict_device(x), g[..., 0].contiguous(), 0.5, False, want_pred=True)
            pred = pred.cpu().numpy()
            jobs = []
            for j, n in enumerate(chunk):
                jobs.append((os.path.join(mout, _pred_name(n, i)), pred[j]))
                rows.append((_pred_name(n, i), round(float(_ev.iou_dice_from_counts(counts[j])[0]), 4)))
            F.write_pngs_async(jobs)
    F.flush_writes()
    if i == 0:
        for n in mine:
            rows.append((n, 1.0))
            shutil.copy(os.path.join(images_path, n), os.path.join(iout, n))
            shutil.copy(os.path.join(masks_path, n), os.path.join(mout, n))
    _append_labels(main_output_path, rows)


def create_training_data_evalnet_miou_hela(model, h, w, c, main_input_path, main_output_path, i, threshold=0.5):
    """functions.py:4011-4135: alive / dead / mod_position/<stem>___{i}.png = (p > threshold) * 255 of every labelled image, with per
    plane the IoU against the ground truth (0 where the plane covers less than 1 % of the image, 0.1 % for the positions) and that
    detection flag appended to labels.csv; for i == 0 also the labelled samples themselves.  The reference's i == 0 loop tests the
    masks its first loop left behind -- the LAST image's -- for every image; so does this one."""
    from . import evaluate as _ev
    F = _F()
    planes = ("alive", "dead", "mod_position")
    din = {k: os.path.join(main_input_path, k) for k in ("brightfield",) + planes}
    dout = {k: os.path.join(main_output_path, k) for k in ("brightfield",) + planes}
    for d in dout.values():
        os.makedirs(d, exist_ok=True)
    names = sorted(os.listdir(din["brightfield"]))      # the writers walk the sorted list; its last image is the one left behind
    mine = F.shard_list(names)
    share = (0.01, 0.01, 0.001)
    rows = []
    with F._pool() as pool:
        for s in range(0, len(mine), 64):
            chunk = mine[s:s + 64]
            x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(din["brightfield"], n) for n in chunk], c)).cuda()
            probs = model.predict_device(x)
            preds, ious, dets = [], [], []
            for q, k in enumerate(planes):
                g = torch.from_numpy(F.read_png_stack(pool, [os.path.join(din[k], n) for n in chunk], 1)).cuda()[..., 0].contiguous()
                pred, counts = _ev.eval_binary(probs[..., q].contiguous(), g, threshold, False, want_pred=True)
                det = ((g != 0).sum((1, 2)).cpu().numpy() >= h * w * share[q])
                preds.append(pred.cpu().numpy())
                dets.append(det)
                ious.append([float(_ev.iou_dice_from_counts(counts[j])[0]) if det[j] else 0 for j in range(len(chunk))])
            jobs = []
            for j, n in enumerate(chunk):
                pn = _pred_name(n, i)
                jobs += [(os.path.join(dout[k], pn), preds[q][j]) for q, k in enumerate(planes)]
                rows.append((pn, ious[0][j], ious[1][j], ious[2][j], int(dets[0][j]), int(dets[1][j]), int(dets[2][j])))
            F.write_pngs_async(jobs)
    F.flush_writes()
    if i == 0 and names:
        left = [F.read_png(os.path.join(din[k], names[-1]), 1) for k in planes]      # what the first loop's last image left behind
        det = [int(np.count_nonzero(m) >= h * w * share[q]) for q, m in enumerate(left)]
        for n in mine:
            rows.append((n, det[0], det[1], det[2], det[0], det[1], det[2]))
            for k in ("brightfield",) + planes:
                shutil.copy(os.path.join(din[k], n), os.path.join(dout[k], n))
    _append_labels(main_output_path, rows)


def create_training_data_evalnet_miou_multiclass(model, h, w, c, num_classes, images_path, masks_path, main_output_path, i, rgb=True):
    """functions.py:4248-4323: masks/<stem>___{i}.png = the arg-max class ids of every labelled image, with compute_classwise_IoU
    (called with the ground truth first and the prediction second, as the reference does) and the ground truth's
    compute_classwise_detection appended to labels.csv; for i == 0 also the labelled pairs, every one with the rows of the LAST
    image's ground truth against itself (the masks the reference's first loop left behind)."""
    from . import evaluate as _ev
    F = _F()
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    names = sorted(os.listdir(images_path))      # the writers walk the sorted list; its last image is the one left behind
    mine = F.shard_list(names)
    rows = []
    with F._pool() as pool:
        for s in range(0, len(mine), 64):
            chunk = mine[s:s + 64]
            x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(images_path, n) for n in chunk], c)).cuda()
            g_np = F.read_png_stack(pool, [os.path.join(masks_path, n) for n in chunk], 1)[..., 0]
            if (not rgb) and c == 3:
                x = x.flip(-1).contiguous()
            pred = _ev.eval_multiclass(model.predict_device(x), torch.from_numpy(g_np).cuda(), want_pred=True)[0].cpu().numpy()
            stats = list(pool.map(lambda j: (compute_classwise_IoU(g_np[j], pred[j], num_classes),
                                             compute_classwise_detection(g_np[j], num_classes)), range(len(chunk))))
            jobs = []
            for j, n in enumerate(chunk):
                jobs.append((os.path.join(mout, _pred_name(n, i)), pred[j]))
                rows.append((_pred_name(n, i), *stats[j][0], *stats[j][1]))
            F.write_pngs_async(jobs)
    F.flush_writes()
    if i == 0 and names:
        left = F.read_png(os.path.join(masks_path, names[-1]), 1)
        left = left[..., 0] if left.ndim == 3 else left
        gt_row = (*compute_classwise_IoU(left, left, num_classes), *compute_classwise_detection(left, num_classes))
        for n in mine:
            rows.append((n, *gt_row))
            shutil.copy(os.path.join(images_path, n), os.path.join(iout, n))
            shutil.copy(os.path.join(masks_path, n), os.path.join(mout, n))
    _append_labels(main_output_path, rows)


# ---------------------------------------------------------------------------------------------------
# the scalar-IoU multiclass EvalNet family (functions.py:3496-3567, 3673-3769, 4509-4552, 5158-5317, 5762-5831; the SUIM / Cityscapes
# twin of the ISIC chain): get_evalnet with the one-hot class stack as input B and one sigmoid unit, trained on the mean IoU over the
# classes of a prediction.  Every label is get_IoU_multi_unique(ground truth, prediction) -- the ground truth in the `pred` seat, so the
# classes that count are the PREDICTION's, class 0 included as soon as an IM pixel is blocked -- formed on the host from the integer
# counts of imk_label_counts (evaluate.label_counts / iou_multi_unique_from_counts).
# ---------------------------------------------------------------------------------------------------
def compute_classwise_confluence(gt, num_classes):
    """functions.py:4360-4379: the share of the pixels each class covers, rounded to 4 decimals"""
    gt = np.asarray(gt)
    total_pixels = gt.size
    confluence_list = [0] * num_classes
    for cls in range(num_classes):
        confluence_list[cls] = round((gt == cls).sum() / total_pixels, 4)
    return confluence_list


def get_confluence_binary(gt):
    """functions.py:4381-4395: sum of the mask over its size, rounded to 4 decimals (a 0 / 1 mask: the foreground share)"""
    gt = np.asarray(gt)
    return round(gt.sum() / gt.size, 4)


def _class_probs(model, x):
    """a segmentation model's probabilities [B,H,W,K] f32 on the device: a native U-Net, or anything with Keras' .predict"""
    if hasattr(model, "predict_device"):
        return model.predict_device(x)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(model.predict(x.cpu().numpy()), dtype=np.float32))).cuda()


def _one_hot_u8(ids, num_classes):
    """class ids u8 [...,1] or [...] -> the 0 / 1 stack u8 [...,K] (functions.py:5217: a value >= num_classes has no hot channel)"""
    ids = ids[..., 0] if ids.shape[-1] == 1 and ids.dim() > 3 else ids
    return (ids[..., None] == torch.arange(num_classes, device=ids.device, dtype=ids.dtype)).to(torch.uint8)


def create_training_data_evalnet_multiclass(model, h, w, c, images_path, masks_path, main_output_path, i, rgb=True):
    """functions.py:3496-3567: masks/<stem>___{i}.png = the arg-max class ids of every labelled image, with the mean IoU over the
    prediction's classes against the ground truth (rounded to 4 decimals as numpy rounds a float64) appended to labels.csv; for
    i == 0 also the labelled pairs themselves with the label 1.0."""
    from . import evaluate as _ev
    F = _F()
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    mine = F.shard_list(os.listdir(images_path))
    rows = []
    with F._pool() as pool:
        for s in range(0, len(mine), 64):
            chunk = mine[s:s + 64]
            x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(images_path, n) for n in chunk], c)).cuda()
            g = torch.from_numpy(F.read_png_stack(pool, [os.path.join(masks_path, n) for n in chunk], 1)).cuda()[..., 0].contiguous()
            if (not rgb) and c == 3:
                x = x.flip(-1).contiguous()
            pred = _ev.eval_multiclass(_class_probs(model, x), g, want_pred=True)[0]      # np.argmax's rule
            counts = _ev.label_counts(pred, g)[1]
            pred = pred.cpu().numpy()
            jobs = []
            for j, n in enumerate(chunk):
                jobs.append((os.path.join(mout, _pred_name(n, i)), pred[j]))
                rows.append((_pred_name(n, i), round(_ev.iou_multi_unique_from_counts(counts[j], "pred"), 4)))
            F.write_pngs_async(jobs)
    F.flush_writes()
    if i == 0:
        for n in mine:
            rows.append((n, 1.0))
            shutil.copy(os.path.join(images_path, n), os.path.join(iout, n))
            shutil.copy(os.path.join(masks_path, n), os.path.join(mout, n))
    _append_labels(main_output_path, rows)


def create_training_data_evalnet_im_multiclass(models, h, w, c, images_path, masks_path, main_output_path, num_loops, n_min_models=2,
                                               n_max_models=4, rgb=True, brightness_range_alpha=(0.6, 1.4),
                                               brightness_range_beta=(-20, 20), max_blur=3, max_noise=20, free_rotation=False,
                                               seed=None):
    """functions.py:3673-3769.  Per loop and labelled image: a random sub-ensemble -> argmax agreement IM, randomly eroded / dilated
    -> blocked image + label map, label = the mean IoU over the blocked prediction's classes against the ground truth (rounded to 4
    decimals); half of the samples are written augmented.  Blocking (image and label map) and the label counts of a chunk are ONE
    imk_label_counts call.  `{stem}_aug_{loop}.png`, labels.csv."""
    from . import evaluate as _ev
    F = _F()
    flip = (not rgb) and c == 3      # rgb=False (functions.py:3611 ff.): the nets see the file's channels in OpenCV's order (BGR)
    rng = random.Random(F.SEED if seed is None else seed)
    np_rng = np.random.default_rng(rng.getrandbits(32))
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    names = sorted(os.listdir(images_path))
    draw_kw = dict(brightness_range_alpha=brightness_range_alpha, brightness_range_beta=brightness_range_beta,
                   max_blur=max_blur, max_noise=max_noise, free_rotation=free_rotation, rng=rng, np_rng=np_rng)
    rows, stage = [], _LoopIM(models, POOLED)
    with F._pool() as pool:
        for nl in range(num_loops):
            plan = _draw_plan(rng, len(names), len(models), n_min_models, n_max_models)
            prm = _draw_aug(plan, F.INFER_BATCH, draw_kw)
            loop_rows = {}
            for subset, idx in _chunks(plan, F.INFER_BATCH, stage.pooled):
                x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(images_path, names[i]) for i in idx], c)).cuda()
                gt = torch.from_numpy(F.read_png_stack(pool, [os.path.join(masks_path, names[i]) for i in idx], 1)).cuda()[..., 0].contiguous()
                r, im = stage.run(plan, subset, idx, x.flip(-1).contiguous() if flip else x, F.THRESHOLD, False)
                img, pred = x.clone(), r["masks"][:, 0].contiguous()
                _, counts = _ev.label_counts(pred, gt, im.contiguous(), img, pred)      # functions.py:3739-3747 in one pass
                mk = pred[..., None]
                sel = torch.nonzero(torch.tensor([plan[i][3] for i in idx], device="cuda")).flatten()
                if sel.numel():      # functions.py:3756-3757
                    o, om = augment_batch(img[sel].contiguous(), mk[sel].contiguous(), _aug_params(prm, [i for i in idx if plan[i][3]]))
                    img[sel], mk[sel] = o, om
                img_np, mk_np = img.cpu().numpy(), mk.cpu().numpy()
                jobs = []
                for row, i in enumerate(idx):
                    out_name = f"{names[i][:-4]}_aug_{nl}.png"
                    loop_rows[i] = (out_name, round(_ev.iou_multi_unique_from_counts(counts[row], "pred"), 4))
                    jobs.append((os.path.join(iout, out_name), img_np[row]))
                    jobs.append((os.path.join(mout, out_name), mk_np[row, :, :, 0]))
                F.write_pngs_async(jobs)      # on the writer pool: the next batch's decode, network pass and augmentation run meanwhile
            rows += [loop_rows[i] for i in range(len(names))]
    F.flush_writes()
    with open(os.path.join(main_output_path, "labels.csv"), "a", encoding="utf-8", newline="") as f:
        wr = csv.writer(f, delimiter=";")
        for row in rows:
            wr.writerow(row)


def _scalar_evalnet_input_b(model, ids, num_classes):
    """input B of a get_evalnet model for class-id masks u8 [N,H,W,1]: the ids themselves where the net expands them on the device,
    else the explicit 0 / 1 stack"""
    if model.plan.cb != num_classes or model.n_heads != 1 or model.plan.n_out != 1:
        raise ValueError("needs a get_evalnet(..., inputB_channels=num_classes) model")
    return ids if model.plan.b_onehot else _one_hot_u8(ids, num_classes).contiguous()


def train_evalnet_multiclass(model, train_main_path, val_main_path, filepath_h5, batch_size, num_classes, epochs, seed=None):
    """functions.py:4509-4552: train_evalnet_ISIC_2018's loop (loss 'mean_squared_error', best epoch by val_mean_absolute_error,
    len // batch_size steps) with the masks read as class ids and fed as one-hot stacks (generate_images_batch_multiclass); images of
    any size.  Returns (mse, mae) of the best model on the validation generator."""
    F = _F()

    def load(main_path):
        xa, ids, y = _load_binary_evalnet_set(main_path, pool)
        return xa, _scalar_evalnet_input_b(model, ids, num_classes), y

    kind = ("scalar_multi", num_classes, bool(model.plan.b_onehot))
    with F._pool() as pool:
        tr = _cached_evalnet_set(kind, train_main_path, lambda: load(train_main_path))
        va = _cached_evalnet_set(kind, val_main_path, lambda: load(val_main_path))
    return _fit_evalnet(model, tr, va, filepath_h5, batch_size, epochs, _mse_mae_evaluator(batch_size), 1, seed)


def _scalar_selection(evalnets, h, w, c, num_classes, images_path, mask_paths, main_output_path, threshold, last_gen_main_path, rgb):
    """the body of the two writers below: the candidate with the best (mean) predicted IoU, kept if it reaches the threshold"""
    from .evalnet import SELECT_IOU
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    _copy_last_generation(last_gen_main_path, main_output_path, ("images", "masks"))
    class_ids = _takes_class_ids(evalnets)

    def emit(name, chosen):
        shutil.copy(os.path.join(images_path, name), os.path.join(iout, name))
        return [(os.path.join(mout, name), chosen.reshape(h, w))]
    load = _mask_candidates(mask_paths, mout, h, w, class_ids)
    if not class_ids:      # models that take the one-hot stack (functions.py:5217)
        ids = load

        def load(pool, chunk):
            xb, cand, counts = ids(pool, chunk)
            return _one_hot_u8(xb, num_classes), cand, counts
    _run_selection(evalnets, images_path, c, (not rgb) and c == 3, threshold, load, emit, SELECT_IOU)


def create_training_data_for_segnet_multiclass(evalnet_model, h, w, c, num_classes, images_path, mask_paths, main_output_path, threshold,
                                               last_gen_main_path='', rgb=True):
    """functions.py:5158-5231: images/ (the file, copied) and masks/ (the class-id candidate with the best predicted IoU) of every
    unlabeled image whose best predicted IoU reaches `threshold`."""
    _scalar_selection([evalnet_model], h, w, c, num_classes, images_path, mask_paths, main_output_path, threshold, last_gen_main_path, rgb)


def create_training_data_for_segnet_with_ensemble_multiclass(evalnets, h, w, c, num_classes, images_path, mask_paths, main_output_path,
                                                             threshold, last_gen_main_path='', rgb=True):
    """functions.py:5236-5317: as the writer above with the mean of the EvalNets' predicted IoUs."""
    _scalar_selection(list(evalnets), h, w, c, num_classes, images_path, mask_paths, main_output_path, threshold, last_gen_main_path, rgb)


def num_augs_from_iou_f32(pred_iou, min_threshold, max_threshold):
    """functions.py:5816-5825 as numpy evaluates it: pred_iou is predict()'s float32 [1,1] array, so the Python thresholds and the
    step are rounded to float32, and difference and quotient are float32 operations"""
    f = np.float32
    v, step = f(pred_iou), f((max_threshold - min_threshold) / 5)
    if v > f(max_threshold):
        n = 5
    elif v > f(min_threshold):
        n = 1 + int((v - f(min_threshold)) / step)
    else:
        n = 1
    return min(n, 5)


def _write_augmented(chunk, x, m, n_augs, draw_kw, iout, mout):
    """copies j = 0 .. n_augs[i] - 1 of every pair of a chunk, `{stem}___{j}.png`: copy j of all the images that get one is one
    augment_batch call -> the PNG jobs"""
    n_augs = torch.tensor(n_augs, device="cuda")
    jobs = []
    for j in range(5):
        sel = torch.nonzero(n_augs > j).flatten()
        if not sel.numel():
            break
        o, om = augment_batch(x[sel].contiguous(), m[sel].contiguous(), draw_params(int(sel.numel()), **draw_kw))
        o, om = o.cpu().numpy(), om.cpu().numpy()
        for row, i in enumerate(sel.tolist()):
            name = f"{chunk[i][:-4]}___{j}.png"
            jobs.append((os.path.join(iout, name), o[row]))
            jobs.append((os.path.join(mout, name), om[row, :, :, 0]))
    return jobs


def create_augment_images_and_masks_with_evalnet_multiclass(evalnet_model, h, w, c, num_classes, min_threshold, max_threshold,
                                                            main_input_path, main_output_path, brightness_range_alpha=(0.6, 1.4),
                                                            brightness_range_beta=(-20, 20), max_blur=3, max_noise=20,
                                                            free_rotation=False, rgb=True):
    """functions.py:5762-5831: 1..5 augmented copies `{stem}___{j}.png` of every pseudo-labelled pair, the number growing with the
    IoU the one EvalNet predicts for (image, class-id mask)."""
    F = _F()
    flip = (not rgb) and c == 3      # rgb=False (functions.py:3611 ff.): the nets see the file's channels in OpenCV's order (BGR)
    iin, min_ = os.path.join(main_input_path, "images"), os.path.join(main_input_path, "masks")
    iout, mout = os.path.join(main_output_path, "images"), os.path.join(main_output_path, "masks")
    os.makedirs(iout, exist_ok=True)
    os.makedirs(mout, exist_ok=True)
    mine = F.shard_list(os.listdir(iin))
    native = isinstance(evalnet_model, EvalNet)
    draw_kw = dict(brightness_range_alpha=brightness_range_alpha, brightness_range_beta=brightness_range_beta,
                   max_blur=max_blur, max_noise=max_noise, free_rotation=free_rotation)
    with F._pool() as pool:
        for s in range(0, len(mine), F.INFER_BATCH):
            chunk = mine[s:s + F.INFER_BATCH]
            x = torch.from_numpy(F.read_png_stack(pool, [os.path.join(iin, n) for n in chunk], c)).cuda()
            m = torch.from_numpy(F.read_png_stack(pool, [os.path.join(min_, n) for n in chunk], 1)).cuda()
            xin = x.flip(-1).contiguous() if flip else x
            if native:
                ious = evalnet_model.predict_device(xin, _scalar_evalnet_input_b(evalnet_model, m, num_classes))[:, 0].cpu().numpy()
            else:      # anything with Keras' .predict: the repeated call of the reference, the one-hot stack as it builds it
                ious = np.asarray(evalnet_model.predict([xin.cpu().numpy(), _one_hot_u8(m, num_classes).cpu().numpy().astype(np.int32)]),
                                  dtype=np.float32).reshape(-1)
            n_augs = [num_augs_from_iou_f32(v, min_threshold, max_threshold) for v in ious]
            F.write_pngs_async(_write_augmented(chunk, x, m, n_augs, draw_kw, iout, mout))
    F.flush_writes()
    if F._dist():
        F._dist().barrier()
