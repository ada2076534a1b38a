"""Generation loop of the EvalNet-ensemble selection baseline of the reference: ISIC_2018/10_ISIC_2018_evalnet_ensemble.py,
HeLa/10_HeLa_evalnet_miou_ensemble.py, SUIM/11_SUIM_evalnet_miou_ensemble.py, Cityscapes/10_Cityscapes_evalnet_miou_ensemble.py
(copies of one template).  Per run an ensemble of EvalNets is trained on single models' predictions of the labelled set -- the
`subset` models with model_i from 0, the `subset_aug` models with model_i from 10, validation data from the first three of each --
5 candidates ranked ascending by mae (ISIC) or iou_mae (the others) and renamed `..._topK_{i}`.  Then for n = 2..4 EvalNets and
generations 0..4: every unlabeled image's candidate masks (generation 0: the predictions of the 10 `subset` models; later: of the
previous generation's 5 candidates, plus the pair selected last generation) are scored by the n best EvalNets, the best candidate is
kept where its score reaches the threshold (create_training_data_for_segnet_with_*ensemble*: one fused call per batch), the labelled
pairs join the selected set, and 5 U-Net candidates are trained on it and ranked.  Same loops, model / directory / CSV names.
Environment overrides for short runs: IM_RUNIDS, IM_NS, IM_GENS, IM_CANDIDATES, IM_EVALNET_CANDIDATES (comma-separated).

run(dataset, ensemble=False) is the single-EvalNet baseline the ensemble row is measured against: ISIC_2018/10_ISIC_2018_evalnet.py and
SUIM/11_SUIM_evalnet_miou.py (copies of one template; HeLa and Cityscapes have no such script).  EvalNet training data under
`evalnet/run_{runid}`: EVERY `subset` and `subset_aug` model writes train and val, the `subset_aug` models from TRAIN_LABELED_AUG.  One
EvalNet per run id (`{TAG}_evalnet_{runid}.h5` / `SUIM_evalnet_miou_{runid}.h5`), no candidates, no ranking; its results CSV has the
header modelname;mse;mae in both scripts -- SUIM's over a row of its five values without a name.  Generations 0..4 without the n loop,
the threshold from [ISIC_2018] MAX_THRESHOLD / [DEFAULT] THRESHOLD, the candidates chosen by
create_training_data_for_segnet_ISIC_2018 / create_training_data_by_evalnet_miou_for_segnet_multiclass, STEPS_PER_EPOCH = images //
BATCH_SIZE without the third-of-the-full-set floor.  Overrides: IM_RUNIDS, IM_GENS, IM_CANDIDATES."""
import csv
import os
import shutil

import torch

from . import functions as F
from . import paths
from .evalnet import get_evalnet, get_evalnet_miou, get_evalnet_miou_v2
from .im_driver import DATASETS, NOISY_STUDENT_HELA_HEADER, _ints, color_mapping, epoch_steps, train_candidates
from .unet import get_unet

RUNIDS, NS, GENS = [1, 2, 3], [2, 3, 4], [0, 1, 2, 3, 4]      # the scripts' loops: range(1, 4), range(2, 5), range(0, 5)
CANDIDATES = EVALNET_CANDIDATES = [0, 1, 2, 3, 4]      # U-Nets per generation, EvalNets per run id
N_SUBSET_MODELS = 10      # generation 0: `*_subset_{runid}_{j}`, j = 0..9 (:173-174)
EVALNET_SOURCES = ((0, "subset"), (10, "subset_aug"))      # (first model_i, the models named `{tag}_{which}_{runid}`) (:56-93)
N_VAL_MODELS = 3      # validation data from the first three models of either source: model_i < 3, model_i < 13
EVALNET_HEADER = {"isic": ["modelname", "mse", "mae"],
                  "hela": ["modelname", "total_loss", "iou_loss", "detection_loss", "iou_mae", "detection_mae"],
                  "multi": ["modelname", "total_loss", "iou_loss", "detection_loss", "iou_mae", "detection_mae"]}
EVALNET_RANK = {"isic": 2, "hela": 4, "multi": 4}      # ascending (:115)
THRESHOLD_KEY = {"isic": "MAX_THRESHOLD", "hela": "MIN_THRESHOLD", "multi": "MAX_THRESHOLD"}      # line 34 / 35 of each script


def names(dataset):
    """(tag, EvalNet name stem, EvalNet data directory, U-Net name stem) of a dataset's script"""
    kind = DATASETS[dataset]["kind"]
    tag = {"HeLa": "HELA", "Cityscapes": "CITYSCAPES"}.get(dataset, dataset)
    if kind == "isic":
        return tag, f"{tag}_evalnet", "evalnet_ensemble", f"{tag}_segnet"
    return tag, f"{tag}_evalnet_miou", "evalnet_miou_ensemble", f"{tag}_segnet_ensemble" if kind == "hela" else f"{tag}_segnet"


def csv_header(dataset):
    return NOISY_STUDENT_HELA_HEADER if DATASETS[dataset]["kind"] == "hela" else DATASETS[dataset]["header"]


SINGLE_DATASETS = ("ISIC_2018", "SUIM")      # the datasets that have a single-EvalNet script
SINGLE_HEADER = ["modelname", "mse", "mae"]      # both scripts; SUIM's row below it has five values and no name (:98-99)
SINGLE_THRESHOLD_KEY = {"ISIC_2018": ("ISIC_2018", "MAX_THRESHOLD"), "SUIM": ("DEFAULT", "THRESHOLD")}      # line 34 / 40


def single_names(dataset):
    """(tag, EvalNet name stem, EvalNet data directory, U-Net name stem) of a dataset's single-EvalNet script"""
    if dataset not in SINGLE_DATASETS:
        raise ValueError(f"the reference has no single-EvalNet script for {dataset}: only {', '.join(SINGLE_DATASETS)}")
    if DATASETS[dataset]["kind"] == "isic":
        return dataset, f"{dataset}_evalnet", "evalnet", f"{dataset}_segnet"
    return dataset, f"{dataset}_evalnet_miou", "evalnet", f"{dataset}_segnet_miou"


def _miou_constructor(evalnet_arch, dataset):
    """evalnet_arch "v1": get_evalnet_miou, what every reference script builds; "v2": get_evalnet_miou_v2 (evalnet.py:76), the late-fusion
    network, in its place.  ISIC_2018's EvalNet is get_evalnet, of which the reference has no v2: refused by name."""
    if evalnet_arch not in ("v1", "v2"):
        raise ValueError(f"evalnet_arch must be 'v1' or 'v2', got {evalnet_arch!r}")
    if evalnet_arch == "v2" and DATASETS[dataset]["kind"] == "isic":
        raise ValueError(f"evalnet_arch='v2': {dataset} scores with get_evalnet, which has no v2 (get_evalnet_miou_v2 is the two-head network)")
    return get_evalnet_miou_v2 if evalnet_arch == "v2" else get_evalnet_miou


def run(dataset, train_new_evalnet=True, ensemble=True, evalnet_arch="v1"):
    miou_net = _miou_constructor(evalnet_arch, dataset)
    if not ensemble:
        return _run_single(dataset, train_new_evalnet, miou_net)
    kind = DATASETS[dataset]["kind"]            # isic | hela | multi
    hela, multi = kind == "hela", kind == "multi"
    tag, evalnet_tag, ev_sub, segnet_tag = names(dataset)
    S, D = F.config[tag], F.config["DEFAULT"]
    H, W, C, K = int(S["IMAGE_HEIGHT"]), int(S["IMAGE_WIDTH"]), int(S["IMAGE_CHANNELS"]), int(S["NUM_CLASSES"])
    alpha, alpha_evalnet = float(S["ALPHA"]), float(S["ALPHA_EVALNET"])
    actifu, actifu_out = S["ACTIFU"], S["ACTIFU_OUTPUT"]
    threshold = float(S[THRESHOLD_KEY[kind]])
    batch, top_k = int(D["BATCH_SIZE"]), int(D["TOP_Ks"])
    bs_evalnet, ep_evalnet = int(D["BATCH_SIZE_EVALNET"]), int(D["NUM_EPOCHS_EVALNET"])
    P = lambda name: getattr(paths, f"{tag}_{name}")
    base, model_dir, csv_dir = P("BASE_DIR"), P("MODEL_DIR"), P("CSV_DIR")
    subs = ("brightfield", "alive", "dead", "mod_position") if hela else ("images", "masks")
    F.init_distributed()
    rank, world = F._rank_world()
    barrier = lambda: torch.distributed.barrier() if torch.distributed.is_initialized() else None
    os.makedirs(csv_dir, exist_ok=True)

    def evalnet_data(model, split, out_dir, model_i):
        if hela:
            F.create_training_data_evalnet_miou_hela(model, H, W, C, P(f"{split}_DIR"), out_dir, model_i)
        elif multi:
            F.create_training_data_evalnet_miou_multiclass(model, H, W, C, K, P(f"{split}_IMAGES_DIR"), P(f"{split}_MASKS_DIR"), out_dir,
                                                           model_i)
        else:
            F.create_training_data_evalnet_ISIC_2018(model, H, W, C, P(f"{split}_IMAGES_DIR"), P(f"{split}_MASKS_DIR"), out_dir, model_i)

    for runid in _ints("IM_RUNIDS", RUNIDS):
        if train_new_evalnet:
            ev_dir = os.path.join(base, ev_sub, f"run_{runid}")
            for first, which in EVALNET_SOURCES:
                model_i = first
                for fname in sorted(os.listdir(model_dir)):
                    if f"{tag}_{which}_{runid}" in fname:
                        model = F.load_model(os.path.join(model_dir, fname))
                        evalnet_data(model, "TRAIN_LABELED", os.path.join(ev_dir, "train"), model_i)
                        if model_i < first + N_VAL_MODELS:
                            evalnet_data(model, "VAL", os.path.join(ev_dir, "val"), model_i)
                        model_i += 1
                        del model

            def train_evalnet_candidate(i, side_by_side=False):
                name = f"{evalnet_tag}_{runid}_{i}"
                h5 = os.path.join(model_dir, name + ".h5")
                if hela:
                    evalnet = miou_net(H, W, C, K, alpha_evalnet, seed=9000 * runid + i)
                elif multi:
                    evalnet = miou_net(H, W, C, K, alpha_evalnet, seed=9000 * runid + i, onehot_B=True)
                else:
                    evalnet = get_evalnet(H, W, C, K, alpha_evalnet, normalize_B=True, seed=9000 * runid + i)
                if side_by_side:      # no side stream of its own: the other candidates fill the gaps (results identical)
                    evalnet.debug(single_stream=True)
                tr, va = os.path.join(ev_dir, "train"), os.path.join(ev_dir, "val")
                if hela:
                    res = F.train_evalnet_miou_model_hela(evalnet, tr, va, h5, bs_evalnet, ep_evalnet)
                elif multi:
                    res = F.train_evalnet_miou_model_multiclass(evalnet, H, W, tr, va, h5, bs_evalnet, K, ep_evalnet)
                else:
                    res = F.train_evalnet_ISIC_2018(evalnet, tr, va, h5, bs_evalnet, ep_evalnet)
                del evalnet
                return (name,) + tuple(res)
            rows = train_candidates(_ints("IM_EVALNET_CANDIDATES", EVALNET_CANDIDATES), train_evalnet_candidate, world)
            if rank == 0:
                top = sorted(rows, key=lambda r: r[EVALNET_RANK[kind]])[:top_k]
                print(top)
                for i, row in enumerate(top, start=1):
                    os.rename(os.path.join(model_dir, f"{row[0]}.h5"), os.path.join(model_dir, f"{row[0][:-2]}_topK_{i}.h5"))
                with open(os.path.join(csv_dir, f"results_{rows[-1][0]}.csv"), "w", encoding="utf-8", newline="") as f:
                    wr = csv.writer(f, delimiter=";")
                    wr.writerow(EVALNET_HEADER[kind])
                    wr.writerows(rows)
            barrier()

        for n in _ints("IM_NS", NS):
            for gen in _ints("IM_GENS", GENS):
                name_of = lambda g: f"{segnet_tag}_{runid}_n{n}_gen{g}"
                modelname = name_of(gen)
                pred_dir = lambda k, name: os.path.join(base, f"{k}_predictions", "segnet", name)
                unl = pred_dir("train_unlabeled", modelname)
                best_evalnets = [F.load_evalnet(os.path.join(model_dir, f"{evalnet_tag}_{runid}_topK_{j}.h5")) for j in range(1, n + 1)]
                if gen == 0:
                    mask_dirs = [os.path.join(base, "train_unlabeled_predictions", "subset", f"{tag}_subset_{runid}_{j}")
                                 for j in range(N_SUBSET_MODELS)]
                    last = ()
                else:      # the previous generation's candidates (0..4 in the scripts) and its selected set
                    mask_dirs = [pred_dir("train_unlabeled", f"{name_of(gen - 1)}_{j}") for j in _ints("IM_CANDIDATES", CANDIDATES)]
                    last = (pred_dir("train_unlabeled", name_of(gen - 1)),)
                if hela:
                    F.create_training_data_for_segnet_with_miou_ensemble_hela(best_evalnets, H, W, C, P("TRAIN_UNLABELED_BRIGHTFIELD_DIR"),
                                                                              mask_dirs, unl, threshold, *last)
                elif multi:
                    F.create_training_data_for_segnet_with_miou_ensemble_multiclass(best_evalnets, H, W, C, K, P("TRAIN_UNLABELED_IMAGES_DIR"),
                                                                                    mask_dirs, unl, threshold, *last)
                else:
                    F.create_training_data_for_segnet_with_ensemble_binary(best_evalnets, H, W, C, P("TRAIN_UNLABELED_IMAGES_DIR"), mask_dirs,
                                                                           unl, threshold, *last)
                del best_evalnets
                if rank == 0:      # the labelled pairs join the selected set (:199-201)
                    lab = P("TRAIN_LABELED_DIR")
                    for name in os.listdir(os.path.join(lab, subs[0])):
                        for sub in subs:
                            shutil.copy(os.path.join(lab, sub, name), os.path.join(unl, sub, name))
                barrier()
                train_dir = os.path.join(unl, subs[0])
                steps = epoch_steps(len(os.listdir(train_dir)), batch, world)
                if kind != "isic":      # HeLa/10_...:207-213, SUIM/11_...:205-211: at least a third of an epoch over the full training set
                    steps = max(steps, epoch_steps(len(os.listdir(os.path.join(P("TRAIN_FULL_DIR"), subs[0]))), batch, world) // 3)

                def train_candidate(i, side_by_side=False):
                    name_i = f"{modelname}_{i}"
                    h5 = os.path.join(model_dir, name_i + ".h5")
                    preds = [pred_dir(k, name_i) for k in ("val", "test", "train_unlabeled")]
                    model = get_unet(H, W, C, K, alpha, actifu, actifu_out, seed=1000 * runid + 100 * gen + 10 * n + i)
                    if side_by_side:      # the other candidates' streams fill this one's gaps: no side stream of its own (results identical)
                        model.debug(single_stream=True)
                    if hela:
                        res = F.train_hela(train_dir, os.path.join(P("VAL_DIR"), "brightfield"), P("VAL_DIR"), P("TEST_DIR"),
                                           P("TRAIN_UNLABELED_DIR"), name_i, h5, model, "mse", steps, H, W, C, *preds)
                    elif multi:
                        res = F.train_multiclass(train_dir, P("VAL_IMAGES_DIR"), P("VAL_MASKS_DIR"), P("TEST_IMAGES_DIR"),
                                                 P("TEST_MASKS_DIR"), P("TRAIN_UNLABELED_IMAGES_DIR"), P("TRAIN_UNLABELED_MASKS_DIR"),
                                                 name_i, h5, model, "categorical_crossentropy", steps, H, W, C, K,
                                                 color_mapping(dataset, K), *preds)
                    else:
                        res = F.train_ISIC_2018(train_dir, P("VAL_IMAGES_DIR"), P("VAL_MASKS_DIR"), P("TEST_IMAGES_DIR"),
                                                P("TEST_MASKS_DIR"), P("TRAIN_UNLABELED_IMAGES_DIR"), P("TRAIN_UNLABELED_MASKS_DIR"),
                                                name_i, h5, model, "mse", steps, H, W, C, *preds)
                    del model
                    return (name_i,) + tuple(res)
                rows = train_candidates(_ints("IM_CANDIDATES", CANDIDATES), train_candidate, world)
                if rank == 0:
                    top = sorted(rows, key=lambda r: r[DATASETS[dataset]["rank"]], reverse=True)[:top_k]
                    print(top)
                    for i, row in enumerate(top, start=1):
                        os.rename(os.path.join(model_dir, f"{row[0]}.h5"), os.path.join(model_dir, f"{row[0][:-2]}_topK_{i}.h5"))
                    with open(os.path.join(csv_dir, f"results_{modelname}.csv"), "w", encoding="utf-8", newline="") as f:
                        wr = csv.writer(f, delimiter=";")
                        wr.writerow(csv_header(dataset))
                        wr.writerows(rows)
                barrier()


def _run_single(dataset, train_new_evalnet=True, miou_net=None):
    """the single-EvalNet loop (module docstring)"""
    tag, evalnet_tag, ev_sub, segnet_tag = single_names(dataset)
    multi = DATASETS[dataset]["kind"] == "multi"
    S, D = F.config[tag], F.config["DEFAULT"]
    H, W, C, K = int(S["IMAGE_HEIGHT"]), int(S["IMAGE_WIDTH"]), int(S["IMAGE_CHANNELS"]), int(S["NUM_CLASSES"])
    alpha, alpha_evalnet = float(S["ALPHA"]), float(S["ALPHA_EVALNET"])
    actifu, actifu_out = S["ACTIFU"], S["ACTIFU_OUTPUT"]
    section, key = SINGLE_THRESHOLD_KEY[dataset]
    threshold = float(F.config[section][key])
    batch, top_k = int(D["BATCH_SIZE"]), int(D["TOP_Ks"])
    bs_evalnet, ep_evalnet = int(D["BATCH_SIZE_EVALNET"]), int(D["NUM_EPOCHS_EVALNET"])
    P = lambda name: getattr(paths, f"{tag}_{name}")
    base, model_dir, csv_dir = P("BASE_DIR"), P("MODEL_DIR"), P("CSV_DIR")
    F.init_distributed()
    rank, world = F._rank_world()
    barrier = lambda: torch.distributed.barrier() if torch.distributed.is_initialized() else None
    os.makedirs(csv_dir, exist_ok=True)

    def evalnet_data(model, split, out_dir, model_i):
        if multi:
            F.create_training_data_evalnet_miou_multiclass(model, H, W, C, K, P(f"{split}_IMAGES_DIR"), P(f"{split}_MASKS_DIR"), out_dir,
                                                           model_i)
        else:
            F.create_training_data_evalnet_ISIC_2018(model, H, W, C, P(f"{split}_IMAGES_DIR"), P(f"{split}_MASKS_DIR"), out_dir, model_i)

    for runid in _ints("IM_RUNIDS", RUNIDS):
        evalnet_name = f"{evalnet_tag}_{runid}"
        evalnet_h5 = os.path.join(model_dir, evalnet_name + ".h5")
        if train_new_evalnet:
            ev_dir = os.path.join(base, ev_sub, f"run_{runid}")
            tr, va = os.path.join(ev_dir, "train"), os.path.join(ev_dir, "val")
            for (first, which), split in zip(EVALNET_SOURCES, ("TRAIN_LABELED", "TRAIN_LABELED_AUG")):      # :55-85
                model_i = first
                for fname in sorted(os.listdir(model_dir)):
                    if f"{tag}_{which}_{runid}" in fname:
                        model = F.load_model(os.path.join(model_dir, fname))
                        evalnet_data(model, split, tr, model_i)
                        evalnet_data(model, "VAL", va, model_i)      # every model: no first-three limit here
                        model_i += 1
                        del model
            if multi:
                evalnet = (miou_net or get_evalnet_miou)(H, W, C, K, alpha_evalnet, seed=9000 * runid, onehot_B=True)
                res = F.train_evalnet_miou_model_multiclass(evalnet, H, W, tr, va, evalnet_h5, bs_evalnet, K, ep_evalnet)
                row = list(res)      # total_loss, iou_loss, conf_loss, iou_mae, conf_mae under the three-name header, as the script writes it
            else:
                evalnet = get_evalnet(H, W, C, K, alpha_evalnet, normalize_B=True, seed=9000 * runid)
                res = F.train_evalnet_ISIC_2018(evalnet, tr, va, evalnet_h5, bs_evalnet, ep_evalnet)
                row = [evalnet_name, *res]
            del evalnet
            if rank == 0:
                with open(os.path.join(csv_dir, f"results_{evalnet_name}.csv"), "w", encoding="utf-8", newline="") as f:
                    wr = csv.writer(f, delimiter=";")
                    wr.writerow(SINGLE_HEADER)
                    wr.writerow(row)
            barrier()

        for gen in _ints("IM_GENS", GENS):
            name_of = lambda g: f"{segnet_tag}_{runid}_gen{g}"
            modelname = name_of(gen)
            pred_dir = lambda k, name: os.path.join(base, f"{k}_predictions", "segnet", name)
            unl = pred_dir("train_unlabeled", modelname)
            evalnet = F.load_evalnet(evalnet_h5)
            if gen == 0:
                mask_dirs = [os.path.join(base, "train_unlabeled_predictions", "subset", f"{tag}_subset_{runid}_{j}")
                             for j in range(N_SUBSET_MODELS)]
                last = ()
            else:      # the previous generation's candidates (0..4 in the scripts) and its selected set
                mask_dirs = [pred_dir("train_unlabeled", f"{name_of(gen - 1)}_{j}") for j in _ints("IM_CANDIDATES", CANDIDATES)]
                last = (pred_dir("train_unlabeled", name_of(gen - 1)),)
            if multi:
                F.create_training_data_by_evalnet_miou_for_segnet_multiclass(evalnet, H, W, C, K, P("TRAIN_UNLABELED_IMAGES_DIR"), mask_dirs,
                                                                             unl, threshold, *last)
            else:
                F.create_training_data_for_segnet_ISIC_2018(evalnet, H, W, C, P("TRAIN_UNLABELED_IMAGES_DIR"), mask_dirs, unl, threshold, *last)
            del evalnet
            if rank == 0:      # the labelled pairs join the selected set
                lab = P("TRAIN_LABELED_DIR")
                for name in os.listdir(os.path.join(lab, "images")):
                    for sub in ("images", "masks"):
                        shutil.copy(os.path.join(lab, sub, name), os.path.join(unl, sub, name))
            barrier()
            train_dir = os.path.join(unl, "images")
            steps = epoch_steps(len(os.listdir(train_dir)), batch, world)      # no floor from the full set in these two scripts

            def train_candidate(i, side_by_side=False):
                name_i = f"{modelname}_{i}"
                h5 = os.path.join(model_dir, name_i + ".h5")
                preds = [pred_dir(k, name_i) for k in ("val", "test", "train_unlabeled")]
                model = get_unet(H, W, C, K, alpha, actifu, actifu_out, seed=1000 * runid + 100 * gen + i)
                if side_by_side:      # the other candidates' streams fill this one's gaps: no side stream of its own (results identical)
                    model.debug(single_stream=True)
                if multi:
                    res = F.train_multiclass(train_dir, P("VAL_IMAGES_DIR"), P("VAL_MASKS_DIR"), P("TEST_IMAGES_DIR"),
                                             P("TEST_MASKS_DIR"), P("TRAIN_UNLABELED_IMAGES_DIR"), P("TRAIN_UNLABELED_MASKS_DIR"),
                                             name_i, h5, model, "categorical_crossentropy", steps, H, W, C, K,
                                             color_mapping(dataset, K), *preds)
                else:
                    res = F.train_ISIC_2018(train_dir, P("VAL_IMAGES_DIR"), P("VAL_MASKS_DIR"), P("TEST_IMAGES_DIR"),
                                            P("TEST_MASKS_DIR"), P("TRAIN_UNLABELED_IMAGES_DIR"), P("TRAIN_UNLABELED_MASKS_DIR"),
                                            name_i, h5, model, "mse", steps, H, W, C, *preds)
                del model
                return (name_i,) + tuple(res)
            rows = train_candidates(_ints("IM_CANDIDATES", CANDIDATES), train_candidate, world)
            if rank == 0:
                top = sorted(rows, key=lambda r: r[DATASETS[dataset]["rank"]], reverse=True)[:top_k]
                print(top)
                for i, row in enumerate(top, start=1):
                    os.rename(os.path.join(model_dir, f"{row[0]}.h5"), os.path.join(model_dir, f"{row[0][:-2]}_topK_{i}.h5"))
                with open(os.path.join(csv_dir, f"results_{modelname}.csv"), "w", encoding="utf-8", newline="") as f:
                    wr = csv.writer(f, delimiter=";")
                    wr.writerow(DATASETS[dataset]["header"])
                    wr.writerows(rows)
            barrier()
