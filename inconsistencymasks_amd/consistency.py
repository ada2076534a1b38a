"""The consistency-loss baseline's training functions (functions.py:367-707 of the reference): per epoch one pass of labelled
`train_on_batch` steps, an evaluate-and-save, one pass of consistency steps on two augmented views of every unlabelled batch, another
evaluate-and-save; after the last epoch the saved file is loaded and benchmarked.

The draws follow the reference's order.  numpy's global generator: per epoch the labelled permutation, then the unlabelled one.
`random`: per unlabelled batch all flips / turns of the batch (coin, coin, randint(0, 3) per image; ISIC and HeLa only), then view 1's
(randint(0, max_blur), then the brightness coin, per image), then view 2's.  Noise and alpha / beta follow imk_views' convention
(input_ensemble._augment_draws): the noise field's seed, then alpha / beta, from numpy's stream -- they cannot follow the reference's.
The step itself is imk_unet_consistency_fwd_bwd + imk_unet_adamw_step (unet.UNet.consistency_step) on the state the labelled steps use.
"""
import math
import os
import random

import numpy as np
import torch

from . import _lib
from .input_ensemble import TRANSFORMS, ViewPlan, _augment_draws, apply_op, make_views

BEST_START = 100      # `current_validation_loss = 100` (functions.py:395)


def _d4_table():
    """(flip 0, flip 1, turn) of apply_random_flip_and_rotation (functions.py:1509-1537: cv2.flip(., 0), cv2.flip(., 1), then 0 none /
    1 = 90 CW / 2 = 180 / 3 = 90 CCW) -> the imk_views operation with the same pixel permutation.  The operations' own definition is
    csrc/imk_pixmap.h through input_ensemble.apply_op (op 0 identity, 1..12 = flip rows, flip columns, then a turn 1..3); the flips
    without a turn are not among the 12 as such, but D4 has them: flip 0 = flip 1 + 180, flip 1 = flip 0 + 180, both = 180."""
    idx = np.arange(12).reshape(3, 4)
    want = {}
    for f0 in (0, 1):
        for f1 in (0, 1):
            for rot in range(4):
                a = idx
                if f0:
                    a = a[::-1]
                if f1:
                    a = a[:, ::-1]
                if rot:
                    a = np.rot90(a, k={1: -1, 2: 2, 3: 1}[rot])
                want[(f0, f1, rot)] = np.ascontiguousarray(a)
    table = {}
    for key, a in want.items():
        ops = [op for op in range(13) if apply_op(idx, op).shape == a.shape and np.array_equal(apply_op(idx, op), a)]
        table[key] = ops[0]
    return table


D4_OP = _d4_table()


def d4_op(flip0, flip1, rot):
    return D4_OP[(int(bool(flip0)), int(bool(flip1)), int(rot))]


def plan_batch_draws(n, geometry, max_blur, max_noise, brightness_range_alpha, brightness_range_beta, rng=None, np_rng=None):
    """The draws of one unlabelled batch of n images -> per image [view 1's ViewParams, view 2's]: both views of an image share its
    flips / turn and differ in blur, noise and brightness."""
    rng, np_rng = rng or random, np_rng or np.random
    ops = [0] * n
    if geometry:
        for b in range(n):
            f0 = rng.randint(0, 1) == 1
            f1 = rng.randint(0, 1) == 1
            ops[b] = d4_op(f0, f1, rng.randint(0, 3))
    views = [[None, None] for _ in range(n)]
    for v in (0, 1):
        for b in range(n):
            q = _lib.ViewParams()
            q.op = ops[b]
            _augment_draws(q, max_blur, max_noise, brightness_range_alpha, brightness_range_beta, rng, np_rng)
            views[b][v] = q
    return views


def run_epochs(n_labeled, n_unlabeled, batch_size, epochs, validation_frequency, labeled_step, consistency_step, evaluate, save,
               np_rng=None, log=print):
    """The epoch loop of functions.py:398-463 over index batches; the callbacks do the work.  -> the evaluate results, in order."""
    np_rng = np_rng or np.random
    best = BEST_START
    seen = []

    def evaluate_and_save(epoch, after):
        nonlocal best
        loss = evaluate()
        seen.append(loss)
        log(f"Epoch: {epoch}, Validation Loss: {round(loss, 4)}  after {after} training")
        if loss < best:
            best = loss
            log(f" -------------------------- Model saved with val_loss {round(loss, 4)}")
            save()

    for epoch in range(epochs):
        labeled_indices = np_rng.permutation(n_labeled)
        unlabeled_indices = np_rng.permutation(n_unlabeled)
        for i in range(int(math.ceil(n_labeled / batch_size))):
            labeled_step(labeled_indices[i * batch_size:(i + 1) * batch_size])
        if epoch % validation_frequency == 0:
            evaluate_and_save(epoch, "labeled")
        for i in range(int(math.ceil(n_unlabeled / batch_size))):
            consistency_step(unlabeled_indices[i * batch_size:(i + 1) * batch_size])
        if epoch % validation_frequency == 0:
            evaluate_and_save(epoch, "unlabeled")
    return seen


# ---- the three training functions -----------------------------------------------------------------------------------------------------
def _F():
    from . import functions
    return functions


def _stack(paths_, channels, bgr=False):
    F = _F()
    with F._pool() as pool:
        a = F.read_png_stack(pool, paths_, channels)
    if bgr and channels == 3:       # cv2.imread without the BGR -> RGB conversion (load_unlabeled_images, functions.py:930-951)
        a = np.ascontiguousarray(a[..., ::-1])
    return a


def _sorted_files(d):
    return [os.path.join(d, n) for n in sorted(os.listdir(d))]


def _listed_files(d):
    return [os.path.join(d, n) for n in os.listdir(d)]


def _binary(masks):
    """np.where(mask / 255 > 0.5, 1, 0) (functions.py:862-865)"""
    return (masks > 127).astype(np.uint8)


def _loss_kind(loss_func, who, want):
    F = _F()
    F._reject_untrainable(loss_func, who)
    if isinstance(loss_func, (F.ignore_im_categorical_crossentropy, F.ignore_im_dice_loss_multiclass)):
        raise NotImplementedError(f"{who}: the ignore_im_* losses are not trained by the consistency scripts")
    if want == 0 and loss_func != "mse":
        raise NotImplementedError(f"{who}: the consistency scripts train this model with 'mse'")
    return want


def _train(who, model, filepath_h5, lab_x, lab_y, unl_x, val_x, val_y, loss_kind, geometry, max_blur, max_noise,
           brightness_range_alpha, brightness_range_beta, validation_frequency):
    """lab_* / unl_x / val_*: uint8 numpy sets.  Trains `model` in place, saves the best epoch half to filepath_h5."""
    F = _F()
    from . import evaluate as ev
    if F._rank_world()[1] > 1:
        raise RuntimeError(f"{who}: the consistency step has no gradient data parallelism (world size {F._rank_world()[1]}); "
                           "run one rank, or whole candidates per rank with IM_DP_MODE=candidates")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lab_x, lab_y, unl_x, val_x, val_y = dev(lab_x), dev(lab_y), dev(unl_x), dev(val_x), dev(val_y)
    if model.train_state is None:
        model.init_train_state()
    model.set_bn_momentum(0.99)

    def labeled_step(idx):
        i = torch.as_tensor(np.asarray(idx), device="cuda")
        x, _ = F.gather_pairs(i, img=lab_x)
        y, _ = F.gather_pairs(i, img=lab_y)
        model.train_step(x, y, loss_kind, F.LR, F.WD)

    def consistency_step(idx):
        i = torch.as_tensor(np.asarray(idx), device="cuda")
        x, _ = F.gather_pairs(i, img=unl_x)
        per_image = plan_batch_draws(len(idx), geometry, max_blur, max_noise, brightness_range_alpha, brightness_range_beta)
        views = make_views(x, ViewPlan(per_image))
        model.consistency_step(views[0], views[1], F.LR, F.WD)

    def evaluate():
        """model.evaluate: the compiled loss over the validation set, Keras' sample-weighted mean over its batches"""
        total, n = 0.0, 0
        for lo in range(0, val_x.shape[0], F.BATCH_SIZE):
            p, y = model.predict_device(val_x[lo:lo + F.BATCH_SIZE]), val_y[lo:lo + F.BATCH_SIZE]
            if loss_kind == 0:      # 'mse': mean over every element
                total += float(ev.soft_sums(p, y, 1))
                n += y.numel()
            else:                   # CategoricalCrossentropy on the softmax output: -log p[class], mean over the pixels
                pt = p.gather(-1, y.long().unsqueeze(-1)).clamp_min(1.17549435e-38)
                total += float(-pt.log().double().sum())
                n += y.numel()
        return total / max(n, 1)

    return run_epochs(lab_x.shape[0], unl_x.shape[0], F.BATCH_SIZE, F.NUM_EPOCHS_CS, validation_frequency, labeled_step,
                      consistency_step, evaluate, lambda: F.save_model(model, filepath_h5))


def train_ISIC_2018_consistency_loss(train_images_dir, train_masks_dir, val_images_dir, val_masks_dir, test_images_dir,
                                     test_masks_dir, unlabeled_images_dir, unlabeled_masks_dir, modelname, filepath_h5, model,
                                     loss_func, h, w, c, val_pred_dir, test_pred_dir, unlabeled_pred_dir, max_blur, max_noise,
                                     brightness_range_alpha, brightness_range_beta, validation_frequency=1):
    """functions.py:367-474."""
    F = _F()
    kind = _loss_kind(loss_func, "train_ISIC_2018_consistency_loss", 0)
    lab_x, lab_y = _stack(_sorted_files(train_images_dir), c), _binary(_stack(_sorted_files(train_masks_dir), 1))
    val_x, val_y = _stack(_sorted_files(val_images_dir), c), _binary(_stack(_sorted_files(val_masks_dir), 1))
    unl_x = _stack(_listed_files(unlabeled_images_dir), c, bgr=True)
    train_ISIC_2018_consistency_loss.last_validation_losses = _train(
        "train_ISIC_2018_consistency_loss", model, filepath_h5, lab_x, lab_y, unl_x, val_x, val_y, kind, True, max_blur, max_noise,
        brightness_range_alpha, brightness_range_beta, validation_frequency)
    best_model = F.load_model(filepath_h5)
    mIoU_val, dice_val = F.benchmark_ISIC2018(best_model, val_images_dir, val_masks_dir, val_pred_dir, h, w, c)
    mIoU_test, dice_test = F.benchmark_ISIC2018(best_model, test_images_dir, test_masks_dir, test_pred_dir, h, w, c)
    mIoU_unl, dice_unl = F.benchmark_ISIC2018(best_model, unlabeled_images_dir, unlabeled_masks_dir, unlabeled_pred_dir, h, w, c)
    print(f"{modelname} mIoU_val: {mIoU_val}")
    F.flush_writes()
    return mIoU_val, mIoU_test, mIoU_unl, dice_val, dice_test, dice_unl


def train_hela_consistency_loss(train_main_dir, val_main_dir, test_main_dir, unlabeled_main_dir, modelname, filepath_h5, model,
                                loss_func, h, w, c, val_pred_dir, test_pred_dir, unlabeled_pred_dir, max_blur, max_noise,
                                brightness_range_alpha, brightness_range_beta, validation_frequency=1):
    """functions.py:479-595: targets (alive, dead, mod_position), each np.where(mask / 255 > 0.5, 1, 0) -- no position weight here."""
    F = _F()
    kind = _loss_kind(loss_func, "train_hela_consistency_loss", 0)

    def load(main):
        x = _stack(_sorted_files(os.path.join(main, "brightfield")), c)
        y = np.stack([_binary(_stack(_sorted_files(os.path.join(main, k)), 1))[..., 0] for k in ("alive", "dead", "mod_position")], -1)
        return x, y
    lab_x, lab_y = load(train_main_dir)
    val_x, val_y = load(val_main_dir)
    unl_x = _stack(_sorted_files(os.path.join(unlabeled_main_dir, "brightfield")), c, bgr=True)
    train_hela_consistency_loss.last_validation_losses = _train(
        "train_hela_consistency_loss", model, filepath_h5, lab_x, lab_y, unl_x, val_x, val_y, kind, True, max_blur, max_noise,
        brightness_range_alpha, brightness_range_beta, validation_frequency)
    best_model = F.load_model(filepath_h5)
    res = []
    for gt, pd in ((val_main_dir, val_pred_dir), (test_main_dir, test_pred_dir), (unlabeled_main_dir, unlabeled_pred_dir)):
        res += list(F.benchmark_hela(best_model, gt, pd, h, w, c))
    print(f"{modelname} mIoU_val: {res[0]}   mean_cell_count_error_val: {res[2]}")
    F.flush_writes()
    return tuple(res)


def train_multiclass_consistency_loss(train_images_dir, train_masks_dir, val_images_dir, val_masks_dir, test_images_dir,
                                      test_masks_dir, unlabeled_images_dir, unlabeled_masks_dir, modelname, filepath_h5, model,
                                      loss_func, h, w, c, n_classes, class_to_color_mapping, val_pred_dir, test_pred_dir,
                                      unlabeled_pred_dir, max_blur, max_noise, brightness_range_alpha, brightness_range_beta,
                                      validation_frequency=1, print_results=False):
    """functions.py:601-707: no flips / turns; the masks stay class-id maps (the one-hot is formed inside the loss kernel)."""
    F = _F()
    kind = _loss_kind(loss_func, "train_multiclass_consistency_loss", 1)
    lab_x, lab_y = _stack(_sorted_files(train_images_dir), c), _stack(_sorted_files(train_masks_dir), 1)[..., 0]
    val_x, val_y = _stack(_sorted_files(val_images_dir), c), _stack(_sorted_files(val_masks_dir), 1)[..., 0]
    unl_x = _stack(_listed_files(unlabeled_images_dir), c, bgr=True)
    train_multiclass_consistency_loss.last_validation_losses = _train(
        "train_multiclass_consistency_loss", model, filepath_h5, lab_x, lab_y, unl_x, val_x, val_y, kind, False, max_blur, max_noise,
        brightness_range_alpha, brightness_range_beta, validation_frequency)
    best_model = F.load_model(filepath_h5, custom_objects={"MeanIoU": F.MeanIoU})
    out = []
    for img, gt, pd in ((val_images_dir, val_masks_dir, val_pred_dir), (test_images_dir, test_masks_dir, test_pred_dir),
                        (unlabeled_images_dir, unlabeled_masks_dir, unlabeled_pred_dir)):
        out.append(F.benchmark_multiclass(best_model, img, gt, pd, h, w, c, class_to_color_mapping, print_results=print_results))
    print(f"{modelname} mIoU_val: {out[0][1]}")
    F.flush_writes()
    return out[0][0], out[1][0], out[2][0], out[0][1], out[1][1], out[2][1]
