#!/usr/bin/env python3
"""Golden vectors of the IM over per-image sub-ensembles, computed by the REAL reference.

Run where a checkout of the reference is on disk:

    IMK_REFERENCE=/path/to/InconsistencyMasks python tests/golden/make_golden_im_members.py

It writes tests/golden/im_members.npz (IMK_GOLDEN_OUT=<dir> writes elsewhere): arrays only.  The EvalNet training-data writers of the
reference hand `random.sample(models, n)` to get_im_prediction_binary / _hela / _multiclass per image (functions.py:3621-3640, 3826,
3931-3953).  Here a pool of fake models (.predict returns a fixed [1,H,W,K] float32 array) stands for the run's models, every image
carries a member word, and the reference's own three functions run unmodified on the sub-list of models of each image, under the stub
modules of tests/golden/make_golden.py.  Nothing from the reference is copied: the outputs are data.

Per case "<name>/..." (names in "names"; the name starts with binary_ / hela_ / multi_):
  preds        float32 [N,B,H,W,K]: the pool's predictions, on a coarse grid so that the file stays small, salted with exactly 0.5,
               0.5 +- 1 ulp, NaN and ties; image 0 is an all-agree plane, image 1 an all-differ plane (multi-class)
  words        uint32 [B]: the member words -- one member, all members, only the highest bit, disjoint sets in neighbouring images,
               more than 8 members, zero, bits above the pool
  binary:      masks [B,1,H,W], im [B,H,W], im_size [B], pred_size [B]
  hela:        masks [B,3,H,W] (alive, dead, position), im [B,H,W] (combined), im_size [B] (summed)
  multi:       final [B,H,W], im [B,H,W], im_size [B], lists_equal [B] (the unique-set filter's verdict)
An image nobody votes for has no reference call (the reference cannot stack an empty list): its records are the zeros that
include/imk.h defines.

The maker refuses a fixture that cannot tell tests/im_members_cases.py's three planted defects (non-members counted, the pool size
instead of the member count, model 0 as the anchor where it is no member) from the rule: each has to miss an image of some case.  It
also asserts that the restatement itself reproduces every record."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import im_members_cases as MC  # noqa: E402
import make_golden as MG  # noqa: E402

OUT = os.environ.get("IMK_GOLDEN_OUT", HERE)
F32 = np.float32
EDGE = np.array([0.5, np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(0.5), F32(0)), np.nan, 0.0, 1.0], F32)

# (name, N, B, H, W, K): 8 x 12 has the 16-byte paths (96 % 16 == 0), 7 x 5 none of them
CASES = [("binary_n5", 5, 7, 8, 12, 1), ("binary_n16", 16, 7, 7, 5, 1), ("binary_n2", 2, 5, 4, 4, 1), ("hela_n10", 10, 7, 8, 8, 3),
         ("multi_k3_n5", 5, 7, 8, 12, 3), ("multi_k9_n10", 10, 7, 7, 5, 9), ("multi_k35_n16", 16, 7, 4, 4, 35), ("multi_k3_n2", 2, 5, 4, 4, 3)]


def words_for(rng, n_models, batch):
    full = (1 << n_models) - 1
    half = sum(1 << n for n in range(0, n_models, 2))
    w = [1 << int(rng.integers(n_models)),                  # one member
         full,                                              # all members
         1 << (n_models - 1),                               # only the highest bit
         half, full & ~half,                                # disjoint sets in neighbouring images
         0,                                                 # nobody
         (0b110 & full) | (0xABC << n_models)]              # bits above the pool (a pool of 16: bits 16..27)
    if n_models > 8:
        w[1] = full & ~1                                    # more than 8 members, model 0 not among them
    w = [v & 0xFFFFFFFF for v in w]
    if not (w[6] & full):
        w[6] |= 1
    if batch == 5:      # a pool of 2 has no room for the rest: one member, all, the highest bit, nobody, the bits above
        w = [w[i] for i in (0, 1, 2, 5, 6)]
    assert len(w) == batch
    return np.array(w, np.uint32)


def make_preds(rng, kind, n_models, batch, h, w, k):
    if kind == "multi":
        p = (rng.integers(0, 9, (n_models, batch, h, w, k)) / 8).astype(F32)          # a grid of 9 levels: ties are common
        p[:, 0] = p[0:1, 0]                                                            # image 0: all agree
        p[:, 1] = 0
        for n in range(n_models):
            p[n, 1, ..., (n + 1) % k] = 1                                              # image 1: neighbours in the pool differ
        flat = p[:, 2:].reshape(-1)
        idx = rng.choice(flat.size, flat.size // 12, replace=False)
        flat[idx] = np.nan                                                             # the first NaN wins
        p[:, 2:] = flat.reshape(p[:, 2:].shape)
        return p
    base = rng.integers(0, 17, (1, batch, h, w, k))
    p = (np.clip(base + rng.integers(-3, 4, (n_models, batch, h, w, k)), 0, 16) / 16).astype(F32)   # the models mostly agree
    flat = p.reshape(-1)
    idx = rng.choice(flat.size, flat.size // 6, replace=False)
    flat[idx] = EDGE[rng.integers(0, len(EDGE), idx.size)]
    return flat.reshape(p.shape)


def record(F, kind, preds, words):
    n_models, batch, h, w, k = preds.shape
    x = np.zeros((1, h, w, 1), np.uint8)
    out = {"preds": preds, "words": words}
    if kind == "multi":
        out.update(final=np.zeros((batch, h, w), np.uint8), im=np.zeros((batch, h, w), np.uint8), im_size=np.zeros(batch, np.int64),
                   lists_equal=np.ones(batch, np.uint8))
    else:
        out.update(masks=np.zeros((batch, k, h, w), np.uint8), im=np.zeros((batch, h, w), np.uint8), im_size=np.zeros(batch, np.int64))
        if kind == "binary":
            out["pred_size"] = np.zeros(batch, np.int64)
    for b in range(batch):
        models = [MG.FixedModel(preds[n, b:b + 1]) for n in MC.member_list(words[b], n_models)]
        if not models:
            continue
        if kind == "binary":
            final, im, im_size, pred_size = F.get_im_prediction_binary(models, x, 0.5)
            out["masks"][b, 0], out["im"][b], out["im_size"][b], out["pred_size"][b] = final, im, im_size, pred_size
        elif kind == "hela":
            alive, dead, pos, im, im_size = F.get_im_prediction_hela(models, x)
            out["masks"][b, 0], out["masks"][b, 1], out["masks"][b, 2], out["im"][b], out["im_size"][b] = alive, dead, pos, im, im_size
        else:
            final, im, im_size, equal = F.get_im_prediction_multiclass(models, x, True)
            out["final"][b], out["im"][b], out["im_size"][b], out["lists_equal"][b] = final, im, im_size, int(bool(equal))
    return out


def main():
    if not MG.REF or not os.path.exists(os.path.join(MG.REF, "functions.py")):
        sys.exit("set IMK_REFERENCE to a checkout of the reference (the directory that holds functions.py)")
    F, _ = MG.import_reference()
    rng = np.random.default_rng(20261021)
    arrays, cases = {"names": np.array([c[0] for c in CASES])}, []
    with np.errstate(all="ignore"):
        for name, n_models, batch, h, w, k in CASES:
            kind = name.split("_")[0]
            rec = record(F, kind, make_preds(rng, kind, n_models, batch, h, w, k), words_for(rng, n_models, batch))
            cases.append(dict(rec, name=name, kind=kind))
            for key, a in rec.items():
                arrays[f"{name}/{key}"] = a
    for c in cases:
        missed = MC.check_case(c)
        assert not missed, f"the restatement misses images {missed} of {c['name']}"
    for defect in MC.DEFECTS:
        caught = [c["name"] for c in cases if MC.check_case(c, defect)]
        if not caught:
            sys.exit(f"refused: no case of this fixture tells the planted defect {defect!r} from the rule")
        print(f"defect {defect!r}: caught by {caught}")
    specials = np.concatenate([c["preds"].reshape(-1) for c in cases if c["kind"] != "multi"])
    for v in EDGE[:3]:
        assert (specials == v).any(), v
    assert np.isnan(specials).any()
    path = os.path.join(OUT, "im_members.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print(f"{path}: {len(cases)} cases, {size} bytes")


if __name__ == "__main__":
    main()
