"""Time the consistency-loss step's forward/backward (imk_unet_consistency_fwd_bwd) at the ISIC and HeLa bench shapes (batch 32)
with device events, from ONE process, the three alternating window by window:
  (i)   the default route: the fused two-view head kernel (consistency_head_sigmoid_kernel);
  (ii)  the composed route (head_kernel x 2 -> consistency_dlogit_kernel -> the labelled step's head dgrad per view), selected
        through the plan's materialize switch -- in training that switch changes nothing but this selection;
  (iii) two labelled imk_unet_fwd_bwd steps on the same model and batch: the comparison (the consistency step is two forwards, two
        backwards and one head).
The optimizer step is the same launch behind all three and is left out.  Medians over --reps windows of --inner calls each, with
the run-to-run spread (min .. max of the windows).  Appends one JSON line per shape to --out.

    python tests/gpu_probe/consistency_step_time.py [--only isic|hela] [--reps 7] [--inner 400] [--out profiles/consistency_step_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from inconsistencymasks_amd.unet import UNet  # noqa: E402

BATCH = 32
SHAPES = {   # name: (H, W, C, K, alpha): config.ini's first-generation models
    "isic": (256, 256, 3, 1, 0.5),
    "hela": (256, 256, 1, 3, 1.0),
}


def windows(fns, reps, inner, before):
    """per-call milliseconds of every fn: `reps` windows of `inner` calls each, the fns alternating window by window; before[i] runs
    in front of fn i's window, untimed"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for fn, pre in zip(fns, before):
        pre()
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, fn, pre in zip(times, fns, before):
            pre()
            ev[0].record()
            for _ in range(inner):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            t.append(ev[0].elapsed_time(ev[1]) / inner)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=400)     # windows of 0.7 - 1.3 s
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_step_time.jsonl"))
    a = ap.parse_args()
    for name, (h, w, c, k, alpha) in SHAPES.items():
        if a.only and name != a.only:
            continue
        model = UNet(h, w, c, k, alpha, "sigmoid", seed=1)
        rng = np.random.default_rng(0)
        base = rng.integers(0, 256, (BATCH, h, w, c))
        v1 = torch.from_numpy((base + rng.integers(-20, 21, base.shape)).clip(0, 255).astype(np.uint8)).cuda()
        v2 = torch.from_numpy((base + rng.integers(-20, 21, base.shape)).clip(0, 255).astype(np.uint8)).cuda()
        y = torch.from_numpy(rng.integers(0, 2, (BATCH, h, w, k), dtype=np.uint8)).cuda()
        model.init_train_state()

        def fused():
            model.consistency_fwd_bwd(v1, v2)

        def composed():
            model.consistency_fwd_bwd(v1, v2)

        def two_labelled():
            model.fwd_bwd(v1, y, 0)
            model.fwd_bwd(v2, y, 0)

        def route(materialize):       # switched once per window, outside the timed calls
            torch.cuda.synchronize()
            model.debug(materialize=materialize)

        fused()
        torch.cuda.synchronize()
        loss_f, g_f = float(model.stats[0]), model.grads.clone()
        route(True)
        composed()
        torch.cuda.synchronize()
        loss_c, g_c = float(model.stats[0]), model.grads.clone()
        route(False)
        t_f, t_c, t_l = windows([fused, composed, two_labelled], a.reps, a.inner, before=[lambda: route(False), lambda: route(True), lambda: route(False)])
        rel = float(((g_f - g_c).double().norm() / g_c.double().norm().clamp_min(1e-30)).item())
        rec = {"shape": name, "hw": [h, w], "c": c, "K": k, "alpha": alpha, "batch": BATCH, "reps": a.reps, "inner": a.inner,
               "fused_ms_median": round(statistics.median(t_f), 4), "fused_ms_min_max": [round(min(t_f), 4), round(max(t_f), 4)],
               "composed_ms_median": round(statistics.median(t_c), 4), "composed_ms_min_max": [round(min(t_c), 4), round(max(t_c), 4)],
               "two_labelled_ms_median": round(statistics.median(t_l), 4), "two_labelled_ms_min_max": [round(min(t_l), 4), round(max(t_l), 4)],
               "loss_fused": loss_f, "loss_composed": loss_c, "grads_rel_l2_fused_vs_composed": rel,
               "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del model


if __name__ == "__main__":
    main()
