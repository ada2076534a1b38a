"""The consistency-loss baseline: counterpart of the reference's ISIC_2018/05_ISIC_2018_consistency_loss.py, HeLa/05_HeLa_consistency_loss.py,
SUIM/06_SUIM_consistency_loss.py and Cityscapes/05_Cityscapes_consistency_loss.py (copies of one template).  Per run id 1..3 and
augmentation strength low / mid / high, five candidates start from `{TAG}_subset_{runid}_topK_1.h5`, train with
`functions.train_*_consistency_loss`, are ranked (ISIC: mIoU_val; SUIM / Cityscapes: mIoU_val at index 4; HeLa: index 6 ascending, as in the
reference), the best TOP_Ks renamed `..._topK_{j}.h5`, and every row written to `results_{modelname}.csv`.
Environment overrides for short runs: IM_RUNIDS, IM_CANDIDATES, IM_CS_STRENGTHS (comma-separated indices into low, mid, high)."""
import csv
import os

import torch

from . import functions as F
from . import paths
from .im_driver import DATASETS, _ints, color_mapping, train_candidates

APPROACH = "consistency_loss"
AUG_STRENGTHS = ["low", "mid", "high"]
# max_blurs, max_noises, brightness_range_alphas, brightness_range_betas per strength (the scripts' four tables)
_STRONG = dict(max_blurs=[1, 2, 3], max_noises=[10, 17, 25], brightness_range_alphas=[(0.85, 1.15), (0.7, 1.3), (0.5, 1.5)],
               brightness_range_betas=[(-10, 10), (-17, 17), (-25, 25)])
SCHEDULES = {
    "ISIC_2018": _STRONG, "HeLa": _STRONG, "SUIM": _STRONG,
    "Cityscapes": dict(max_blurs=[0, 0, 1], max_noises=[3, 9, 15], brightness_range_alphas=[(0.95, 1.05), (0.8, 1.2), (0.6, 1.4)],
                       brightness_range_betas=[(-3, 3), (-9, 9), (-15, 15)]),
}
# (index of the ranking value in the row, descending?)
RANK = {"ISIC_2018": (1, True), "HeLa": (6, False), "SUIM": (4, True), "Cityscapes": (4, True)}
HEADERS = {
    "ISIC_2018": ["modelname", "mIoU_val", "mIoU_test", "mIoU_train_unlabeled", "dice_score_val", "dice_score_test", "dice_score_train_unlabeled"],
    "HeLa": ["modelname", "mIoU_val", "mIoU_ad_val", "mcce_val", "mIoU_test", "mIoU_ad_test", "mcce_test", "mIoU_unlabeled",
             "mIoU_ad_unlabeled", "mcce_unlabeled"],
    "SUIM": ["modelname", "mPA_val", "mPA_test", "mPA_train_unlabeled", "mIoU_val", "mIoU_test", "mIoU_train_unlabeled"],
    "Cityscapes": ["modelname", "mPA_val", "mPA_test", "mPA_train_unlabeled", "mIoU_val", "mIoU_test", "mIoU_train_unlabeled"],
}
TAGS = {"ISIC_2018": "ISIC_2018", "HeLa": "HELA", "SUIM": "SUIM", "Cityscapes": "CITYSCAPES"}


def model_name(dataset, runid, strength):
    return f"{TAGS[dataset]}_{APPROACH}_{runid}_aug_{strength}"


def pretrained_name(dataset, runid):
    return f"{TAGS[dataset]}_subset_{runid}_topK_1.h5"


def train_candidate(ds, dataset, name_i, h5, model, H, W, C, K, preds, aug):
    P = lambda name: getattr(paths, f"{TAGS[dataset]}_{name}")
    if ds["kind"] == "isic":
        return F.train_ISIC_2018_consistency_loss(P("TRAIN_LABELED_IMAGES_DIR"), P("TRAIN_LABELED_MASKS_DIR"), P("VAL_IMAGES_DIR"),
                                                  P("VAL_MASKS_DIR"), P("TEST_IMAGES_DIR"), P("TEST_MASKS_DIR"),
                                                  P("TRAIN_UNLABELED_IMAGES_DIR"), P("TRAIN_UNLABELED_MASKS_DIR"), name_i, h5, model,
                                                  "mse", H, W, C, *preds, *aug)
    if ds["kind"] == "multi":
        return F.train_multiclass_consistency_loss(P("TRAIN_LABELED_IMAGES_DIR"), P("TRAIN_LABELED_MASKS_DIR"), P("VAL_IMAGES_DIR"),
                                                   P("VAL_MASKS_DIR"), P("TEST_IMAGES_DIR"), P("TEST_MASKS_DIR"),
                                                   P("TRAIN_UNLABELED_IMAGES_DIR"), P("TRAIN_UNLABELED_MASKS_DIR"), name_i, h5, model,
                                                   "categorical_crossentropy", H, W, C, K, color_mapping(dataset, K), *preds, *aug)
    return F.train_hela_consistency_loss(P("TRAIN_LABELED_DIR"), P("VAL_DIR"), P("TEST_DIR"), P("TRAIN_UNLABELED_DIR"), name_i, h5,
                                         model, "mse", H, W, C, *preds, *aug)


def run(dataset):
    ds = DATASETS[dataset]
    S = F.config[ds["section"]]
    H, W, C, K = int(S["IMAGE_HEIGHT"]), int(S["IMAGE_WIDTH"]), int(S["IMAGE_CHANNELS"]), int(S["NUM_CLASSES"])
    top_k = int(F.config["DEFAULT"]["TOP_Ks"])
    P = lambda name: getattr(paths, f"{TAGS[dataset]}_{name}")
    base, model_dir, csv_dir = P("BASE_DIR"), P("MODEL_DIR"), P("CSV_DIR")
    F.init_distributed()
    rank, world = F._rank_world()
    sched = SCHEDULES[dataset]
    idx, desc = RANK[dataset]
    for runid in _ints("IM_RUNIDS", [1, 2, 3]):
        for index in _ints("IM_CS_STRENGTHS", [0, 1, 2]):
            modelname = model_name(dataset, runid, AUG_STRENGTHS[index])
            aug = (sched["max_blurs"][index], sched["max_noises"][index], sched["brightness_range_alphas"][index],
                   sched["brightness_range_betas"][index])

            def one(i, side_by_side=False):
                name_i = f"{modelname}_{i}"
                h5 = os.path.join(model_dir, name_i + ".h5")
                preds = [os.path.join(base, f"{k}_predictions", APPROACH, name_i) for k in ("val", "test", "train_unlabeled")]
                model = F.load_model(os.path.join(model_dir, pretrained_name(dataset, runid)))
                if side_by_side:
                    model.debug(single_stream=True)
                row = (name_i,) + tuple(train_candidate(ds, dataset, name_i, h5, model, H, W, C, K, preds, aug))
                del model
                return row
            # the draws come from the process-wide `random` / numpy generators in the reference's order: one candidate at a time
            rows = train_candidates(_ints("IM_CANDIDATES", list(range(5))), one, world, parallel=1)
            if rank == 0:
                top = sorted(rows, key=lambda r: r[idx], reverse=desc)[:top_k]
                print(top)
                for j, row in enumerate(top, start=1):
                    os.rename(os.path.join(model_dir, f"{row[0]}.h5"), os.path.join(model_dir, f"{row[0][:-2]}_topK_{j}.h5"))
                os.makedirs(csv_dir, exist_ok=True)
                with open(os.path.join(csv_dir, f"results_{modelname}.csv"), "w", encoding="utf-8", newline="") as f:
                    wr = csv.writer(f, delimiter=";")
                    wr.writerow(HEADERS[dataset])
                    wr.writerows(rows)
            if torch.distributed.is_initialized():
                torch.distributed.barrier()
