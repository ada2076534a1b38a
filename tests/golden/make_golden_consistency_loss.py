#!/usr/bin/env python3
"""Golden data of the consistency-loss baseline, recorded from the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_consistency_loss.py

It writes tests/golden/consistency_loss.npz and tests/golden/reference_surface_consistency_loss.json, which
tests/test_golden_consistency_loss.py and tests/test_cpu_consistency_loss_surface.py hold the repository to.  IMK_GOLDEN_OUT=<dir>
writes elsewhere.  Nothing from the reference is copied: the outputs are data.

The reference's functions.py is loaded with the stub modules of make_golden_model_ensemble.py.  The cv2 stub is numpy: flip and rotate
are exact permutations and record their codes; GaussianBlur and convertScaleAbs return their input and record that they ran (blur: its
kernel size); tf.convert_to_tensor / tf.expand_dims are numpy.

consistency_loss.npz:
  draws_seed                      random.seed / np.random.seed of the batch below
  draws_calls [n, 2]              every cv2 call that apply_random_flip_and_rotation on a batch of 5 images and then two rounds of
                                  data_augmentation_image2tensor(max_blur 3, max_noise 25) on the same 5 make, in order: (kind, value) with
                                  kind 0 = flip (value = code), 1 = rotate (value: 1 = 90 CW, 2 = 180, 3 = 90 CCW), 2 = GaussianBlur (kernel size),
                                  3 = convertScaleAbs (1)
  draws_geometry [5, 3]           per image (flip 0, flip 1, turn) read off those calls
  draws_view1, draws_view2 [5, 2] per image (blur kernel size or 0, convertScaleAbs ran)
  draws_perm [5, 4, 4]            the 4 x 4 index image of every image after apply_random_flip_and_rotation
  d4_combos [16, 3], d4_perm [16, 4, 4]   every (flip 0, flip 1, turn) combination, drawn by the reference's own function under
                                  successive seeds, with the index image it produced
  trace_<isic|hela|multi>         the calls of train_ISIC_2018_consistency_loss / train_hela_consistency_loss /
                                  train_multiclass_consistency_loss on 5 labelled / 7 unlabelled / 3 validation images with BATCH_SIZE 2
                                  and NUM_EPOCHS_CS 2, driven with a recording model and optimizer: "train_on_batch:<n>", "evaluate",
                                  "save", "call:<n>" (model(x, training=True)), "apply_gradients", "load_model", "benchmark"
  trace_losses                    the scripted evaluate results (four per run)
  trace_arity_<kind>              length of the returned tuple

reference_surface_consistency_loss.json: the four scripts, every name they import, the three functions' signatures and defaults, and per
script the schedules, the ranking index / direction, the header, the model-name and pretrained-file patterns -- names and values only."""
import ast
import contextlib
import inspect
import json
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_model_ensemble import REF, load_reference  # noqa: E402
from make_golden_noisy_student import script_facts  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
NAME = "consistency_loss"
SCRIPTS = {"ISIC_2018/05_ISIC_2018_consistency_loss.py": "ISIC_2018", "HeLa/05_HeLa_consistency_loss.py": "HeLa",
           "SUIM/06_SUIM_consistency_loss.py": "SUIM", "Cityscapes/05_Cityscapes_consistency_loss.py": "Cityscapes"}
TRAINERS = ("train_ISIC_2018_consistency_loss", "train_hela_consistency_loss", "train_multiclass_consistency_loss")
LOSSES = [0.5, 0.6, 0.4, 0.45]
N_LAB, N_UNL, N_VAL, BATCH, EPOCHS = 5, 7, 3, 2, 2


class Cv2:
    def __init__(self):
        self.calls = []

    def install(self):
        cv2 = sys.modules["cv2"]
        cv2.ROTATE_90_CLOCKWISE, cv2.ROTATE_180, cv2.ROTATE_90_COUNTERCLOCKWISE = 0, 1, 2
        cv2.IMREAD_GRAYSCALE = 0

        def flip(a, code):
            self.calls.append((0, code))
            return np.ascontiguousarray(a[::-1] if code == 0 else a[:, ::-1])

        def rotate(a, code):
            self.calls.append((1, code + 1))
            return np.ascontiguousarray(np.rot90(a, k={0: -1, 1: 2, 2: 1}[code]))

        def blur(a, ksize, sigma):
            self.calls.append((2, ksize[0]))
            return a

        def csa(a, alpha=1.0, beta=0.0):
            self.calls.append((3, 1))
            return a

        cv2.flip, cv2.rotate, cv2.GaussianBlur, cv2.convertScaleAbs = flip, rotate, blur, csa
        cv2.imread = lambda path, flag=1: np.zeros((4, 4) if flag == 0 else (4, 4, 3), np.uint8)
        cv2.cvtColor = lambda a, code: np.ascontiguousarray(a[..., ::-1])
        tf = sys.modules["tensorflow"]
        tf.convert_to_tensor = lambda a: np.asarray(a)
        tf.expand_dims = lambda a, axis=-1: np.expand_dims(a, axis)


def split_calls(calls, n):
    """the ordered calls of n images' flips / turns, then two rounds of n augmentations -> geometry [n,3], view1 [n,2], view2 [n,2]"""
    return calls


def draws(ref, c):
    rec = {}
    idx = np.arange(16, dtype=np.uint8).reshape(4, 4)
    seed = 20261019
    random.seed(seed)
    np.random.seed(seed)
    c.calls = []
    geometry, perms, marks = [], [], []
    for _ in range(5):
        a = len(c.calls)
        perms.append(ref.apply_random_flip_and_rotation(idx.copy()))
        mine = c.calls[a:]
        geometry.append([int((0, 0) in mine), int((0, 1) in mine), max([v for k, v in mine if k == 1] or [0])])
    views = []
    for _ in (0, 1):
        per = []
        for b in range(5):
            a = len(c.calls)
            ref.data_augmentation_image2tensor(perms[b].copy(), 3, 25, (0.5, 1.5), (-25, 25))
            mine = c.calls[a:]
            per.append([max([v for k, v in mine if k == 2] or [0]), int((3, 1) in mine)])
        views.append(per)
    rec["draws_seed"] = np.int64(seed)
    rec["draws_calls"] = np.array(c.calls, np.int32)
    rec["draws_geometry"] = np.array(geometry, np.int32)
    rec["draws_view1"], rec["draws_view2"] = np.array(views[0], np.int32), np.array(views[1], np.int32)
    rec["draws_perm"] = np.stack(perms)
    found = {}
    s = 0
    while len(found) < 16:
        random.seed(s)
        s += 1
        a = len(c.calls)
        out = ref.apply_random_flip_and_rotation(idx.copy())
        mine = c.calls[a:]
        found.setdefault((int((0, 0) in mine), int((0, 1) in mine), max([v for k, v in mine if k == 1] or [0])), out)
    keys = sorted(found)
    rec["d4_combos"], rec["d4_perm"] = np.array(keys, np.int32), np.stack([found[k] for k in keys])
    return rec


class Model:
    def __init__(self, log):
        self.log, self.losses = log, list(LOSSES)
        self.trainable_variables = ["w"]

    def compile(self, optimizer=None, loss=None):
        self.log.append("compile")

    def train_on_batch(self, x, y):
        self.log.append(f"train_on_batch:{len(x)}")

    def evaluate(self, x, y):
        self.log.append("evaluate")
        return self.losses.pop(0)

    def save(self, path):
        self.log.append("save")

    def __call__(self, x, training=False):
        assert training is True
        self.log.append(f"call:{len(x)}")
        return np.zeros(1)


def traces(ref):
    rec = {"trace_losses": np.array(LOSSES)}
    log = []
    tf, tfa = sys.modules["tensorflow"], sys.modules["tensorflow_addons"]

    class Opt:
        def apply_gradients(self, pairs):
            list(pairs)
            log.append("apply_gradients")

    class Tape:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def gradient(self, loss, weights):
            return ["g"]

    tfa.optimizers = types.SimpleNamespace(AdamW=lambda learning_rate=None, weight_decay=None: Opt())
    tf.GradientTape = Tape
    tf.reduce_mean = lambda a: 0.0
    tf.keras.losses.mean_squared_error = lambda a, b: 0.0

    def load_model(path, custom_objects=None):
        log.append("load_model")
        return "best"
    tf.keras.models = types.SimpleNamespace(load_model=load_model)
    ref.to_categorical = lambda m, n: np.eye(n, dtype=np.float32)[m]

    def bench(n):
        def f(*a, **k):
            log.append("benchmark")
            return tuple(range(n))
        return f
    ref.benchmark_ISIC2018, ref.benchmark_multiclass, ref.benchmark_hela = bench(2), bench(2), bench(3)
    ref.BATCH_SIZE, ref.NUM_EPOCHS_CS = BATCH, EPOCHS
    with tempfile.TemporaryDirectory() as tmp:
        def mk(name, n, subs=("",)):
            d = os.path.join(tmp, name)
            for s in subs:
                os.makedirs(os.path.join(d, s), exist_ok=True)
                for i in range(n):
                    open(os.path.join(d, s, f"{i}.png"), "w").close()
            return d
        hs = ("brightfield", "alive", "dead", "mod_position")
        li, lm, vi, vm, ui = mk("li", N_LAB), mk("lm", N_LAB), mk("vi", N_VAL), mk("vm", N_VAL), mk("ui", N_UNL)
        hl, hv, hu = mk("hl", N_LAB, hs), mk("hv", N_VAL, hs), mk("hu", N_UNL, hs)
        aug = (1, 10, (0.85, 1.15), (-10, 10))
        runs = {
            "isic": lambda m: ref.train_ISIC_2018_consistency_loss(li, lm, vi, vm, vi, vm, ui, ui, "m", "f.h5", m, "mse", 4, 4, 3, "a", "b", "c", *aug),
            "hela": lambda m: ref.train_hela_consistency_loss(hl, hv, hv, hu, "m", "f.h5", m, "mse", 4, 4, 1, "a", "b", "c", *aug),
            "multi": lambda m: ref.train_multiclass_consistency_loss(li, lm, vi, vm, vi, vm, ui, ui, "m", "f.h5", m, "cce", 4, 4, 3, 3, {}, "a", "b", "c", *aug),
        }
        for kind, fn in runs.items():
            random.seed(1)
            np.random.seed(1)
            del log[:]
            with contextlib.redirect_stdout(open(os.devnull, "w")):
                out = fn(Model(log))
            rec["trace_" + kind] = np.array(log)
            rec["trace_arity_" + kind] = np.int32(len(out))
    return rec


def surface(ref):
    import dump_reference_surface as D
    sig = {}
    for f in TRAINERS:
        sig[f] = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                  for p in inspect.signature(getattr(ref, f)).parameters.values()]
    facts = {}
    for p in sorted(SCRIPTS):
        facts[p] = script_facts(os.path.join(REF, p))
        tree = ast.parse(open(os.path.join(REF, p), encoding="utf-8", errors="replace").read())
        for n in ast.walk(tree):
            if isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name):
                if n.targets[0].id == "aug_strenghts":
                    facts[p]["aug_strenghts"] = ast.literal_eval(n.value)
                if n.targets[0].id == "best_pretrained_filepath_h5":
                    js = n.value.args[-1]
                    facts[p]["pretrained"] = "".join(v.value if isinstance(v, ast.Constant) else "{" + ast.unparse(v.value) + "}" for v in js.values)
    return {"scripts": sorted(SCRIPTS), "wanted": D.wanted_names(REF, sorted(SCRIPTS)), "signatures": sig, "script_facts": facts}


def main():
    ref = load_reference()
    surf = surface(ref)
    c = Cv2()
    c.install()
    rec = draws(ref, c)
    rec.update(traces(ref))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, NAME + ".npz"), **rec)
    with open(os.path.join(OUT, "reference_surface_" + NAME + ".json"), "w") as f:
        json.dump(surf, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(rec)} arrays to {os.path.join(OUT, NAME + '.npz')}")


if __name__ == "__main__":
    main()
