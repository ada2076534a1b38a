"""What the ensemble stage of the EvalNet training-data writers (IM++ / AIM++ family) costs on its two routes, on one GPU.

The GPU path of create_training_data_evalnet_miou_im_hela as the writer runs it -- per loop: the draws (_draw_plan), then per chunk
the ensemble + IM, the per-image random erosion / dilation, the blocking, the IoU sums and the copies of the results to the host --
with the files pre-decoded (the set lives on the device; no PNG is read or written):

  grouped   the images grouped by sub-ensemble, one EnsembleIM per group (IMK_TRAINDATA_POOLED=0)
  pooled    the file list in INFER_BATCH chunks through one PoolIM, one imk_morph_var per operation (IMK_TRAINDATA_POOLED=1)

HeLa shape: 256 x 256 x 1, alpha 1, K 3, a pool of 10 models, 2..4 members per image, 3 loops per pass, a fixed seed.  The reference
does not say how many labelled HeLa crops a run has: 256 images are used here.  A pass is timed with the host clock between two device
synchronisations, after one untimed warm-up pass of each route (which also fills the grouped route's cache of ensembles, as a
writer's first loop does); the two routes alternate inside every round.  Medians over the rounds with min .. max, in ms per pass.
--also runs the ISIC-like (256 x 256 x 3, alpha 0.5, K 1, `>`) and SUIM-like (K 9, softmax) stages once each (one timed pass per
route after the warm-up: a single figure, no spread).

--writer times the whole HeLa writer, files and all, on a small set in a temporary directory (the route of the process's
IMK_TRAINDATA_POOLED): the figure to hold against a checkout of an earlier commit, where this file runs as it is.

Appends one JSON line to --out.  Not part of the test suite.

    python tests/gpu_probe/traindata_stage_time.py [--rounds 7] [--also] [--writer] [--out profiles/traindata_stage_time.jsonl]

--rounds 0 skips the stage (with --writer: the writer's figure alone).
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from inconsistencymasks_amd import evalnet_functions as E  # noqa: E402
from inconsistencymasks_amd import functions as F  # noqa: E402
from inconsistencymasks_amd import im as IM  # noqa: E402
from inconsistencymasks_amd.unet import UNet  # noqa: E402

H = W = 256
N_POOL, N_IMAGES, N_LOOPS, SEED = 10, 256, 3, 7
SHAPES = {"hela": (1, 3, 1.0, "sigmoid", True), "isic": (3, 1, 0.5, "sigmoid", False), "suim": (3, 9, 1.0, "softmax", False)}
HAS_POOLED = hasattr(E, "_LoopIM")


def make(kind):
    c, k, alpha, head, ge = SHAPES[kind]
    models = [UNet(H, W, c, k, alpha, head, seed=100 + j) for j in range(N_POOL)]
    for m in models:
        m.ready_for_inference()
    rng = np.random.default_rng(SEED)
    x = torch.from_numpy(rng.integers(0, 256, (N_IMAGES, H, W, c), dtype=np.uint8)).cuda()
    gt = torch.from_numpy((rng.random((N_IMAGES, H, W, 3 if kind == "hela" else 1)) > 0.7).astype(np.uint8) * 255).cuda()
    return models, x, gt, ge


class Stage:
    """one route of the writer's GPU path on a device-resident set"""

    def __init__(self, models, x, gt, ge, pooled):
        self.models, self.x, self.gt, self.ge, self.pooled = models, x, gt, ge, pooled
        self.loop_im = E._LoopIM(models, pooled) if HAS_POOLED else None
        self.ensembles = {}
        self.calls = 0

    def _im(self, plan, subset, idx, x):
        self.calls += 1
        if self.loop_im is not None:
            return self.loop_im.run(plan, subset, idx, x, 0.5, self.ge)
        if subset not in self.ensembles:      # a checkout without the pooled route: the grouped loop as its writers have it
            self.ensembles[subset] = F.EnsembleIM([self.models[j] for j in subset])
        r = self.ensembles[subset].run(x, 0.5, self.ge, False, False)
        return r, E._random_morph(r["im"], plan, idx)

    def chunks(self, plan):
        if self.loop_im is not None:
            return E._chunks(plan, F.INFER_BATCH, self.pooled)
        return [(s, ia[i:i + F.INFER_BATCH]) for s, ia in E._groups(plan).items() for i in range(0, len(ia), F.INFER_BATCH)]

    def one_pass(self):
        rng = random.Random(SEED)
        for _ in range(N_LOOPS):
            plan = E._draw_plan(rng, N_IMAGES, N_POOL, 2, 4)
            for subset, idx in self.chunks(plan):
                sel = torch.as_tensor(idx, device="cuda")
                x, gt = self.x[sel], self.gt[sel]
                r, im = self._im(plan, subset, idx, x)
                masks = r["masks"]
                img = x.clone()
                IM.block_apply(im, img, masks)
                pred = masks > 0
                g = gt.permute(0, 3, 1, 2) > 0
                inter = (pred & g[:, :pred.shape[1]]).sum(dim=(2, 3)).cpu().numpy()
                union = (pred | g[:, :pred.shape[1]]).sum(dim=(2, 3)).cpu().numpy()
                _ = inter / (union + 1e-7)
                img.cpu()
                (masks > 0).to(torch.uint8).cpu()


def timed(stage):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stage.one_pass()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(kind, rounds):
    models, x, gt, ge = make(kind)
    routes = {"grouped": Stage(models, x, gt, ge, False)}
    if HAS_POOLED:
        routes["pooled"] = Stage(models, x, gt, ge, True)
    for s in routes.values():
        s.one_pass()
        s.calls = 0
    t = {k: [] for k in routes}
    for _ in range(rounds):
        for k, s in routes.items():
            t[k].append(timed(s))
    rec = {}
    for k, v in t.items():
        rec[k + "_ms"] = round(statistics.median(v), 2)
        rec[k + "_min_max"] = [round(min(v), 2), round(max(v), 2)]
        rec[k + "_ensemble_calls_per_pass"] = routes[k].calls // rounds
    if not HAS_POOLED:
        rec["pooled_ms"] = "not measured"
    elif rounds >= 5:
        rec["pooled_windows_wholly_below_grouped"] = max(t["pooled"]) < min(t["grouped"])
    return rec


def writer_e2e(runs, n_images=64, n_loops=2):
    """the whole HeLa writer on PNG files in a temporary directory, `runs` times: ms per run"""
    c, k, alpha, head, _ = SHAPES["hela"]
    models = [UNet(H, W, c, k, alpha, head, seed=100 + j) for j in range(N_POOL)]
    rng = np.random.default_rng(SEED)
    out = []
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "src")
        for s in ("brightfield", "alive", "dead", "mod_position"):
            os.makedirs(os.path.join(src, s))
            for i in range(n_images):
                a = rng.integers(0, 256, (H, W), dtype=np.uint8) if s == "brightfield" else (rng.random((H, W)) > 0.7).astype(np.uint8) * 255
                F.write_png(os.path.join(src, s, f"im_{i:04d}.png"), a)
        for r in range(runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            F.create_training_data_evalnet_miou_im_hela(models, H, W, c, src, os.path.join(d, f"out{r}"), n_loops, seed=SEED)
            F.flush_writes(all_threads=True)
            torch.cuda.synchronize()
            if r:                  # the first run is the warm-up
                out.append((time.perf_counter() - t0) * 1e3)
    return {"images": n_images, "loops": n_loops, "route": "pooled" if getattr(E, "POOLED", False) else "grouped",
            "ms": round(statistics.median(out), 1), "min_max": [round(min(out), 1), round(max(out), 1)], "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--also", action="store_true")
    ap.add_argument("--writer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traindata_stage_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    rec = {"case": f"HeLa writer GPU path, {H}x{W}x1 alpha 1 K 3, pool {N_POOL}, n 2..4, {N_LOOPS} loops, {N_IMAGES} images "
                   f"(the labelled set's size is not in the reference), chunk {F.INFER_BATCH}",
           "rounds": a.rounds, "unit": "ms per pass of 3 loops, host clock between device synchronisations", "has_pooled_route": HAS_POOLED}
    rec["hela"] = measure("hela", a.rounds) if a.rounds > 0 else "not measured"
    for kind in ("isic", "suim"):
        rec[kind] = measure(kind, 1) if a.also else "not measured"
    rec["writer_end_to_end"] = writer_e2e(5) if a.writer else "not measured"
    rec["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
