"""Time imk_unet_fwd_bwd with the Dice loss (loss kind 4) at the ISIC and HeLa bench shapes (batch 32) with device events:
  (i)   kind 4 on the default route (ISIC: the fused variant of head_mse_fused_kernel; HeLa: dice_dlogit_kernel + the head's dgrad),
  (ii)  kind 0 ('mse') on the same build, model and batch: the yardstick, alternating with (i) window by window,
  (iii) kind 4 with IMK_DICE_FUSED=0 -- read once per process, so in a child process, again alternating with its own kind 0.
The optimizer step is the same launch behind all of them and is left out.  Medians over --reps windows of --inner calls each after a
warm-up, with the run-to-run spread (min .. max of the windows).  Appends one JSON line per shape and process to --out.

    python tests/gpu_probe/dice_step_time.py [--only isic|hela] [--reps 7] [--inner 300] [--out profiles/dice_step_time.jsonl]
    python tests/gpu_probe/dice_step_time.py --kinds 0 --label parent      # in another checkout: kind 0 alone (a build without kind 4)
"""
import argparse
import json
import os
import statistics
import subprocess
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


def windows(fns, reps, inner):
    """per-call milliseconds of every fn: `reps` windows of `inner` calls each, the fns alternating window by window"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for fn in fns:
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(times, fns):
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
    ap.add_argument("--inner", type=int, default=300)     # windows of 0.3 - 0.6 s
    ap.add_argument("--kinds", default="4,0")
    ap.add_argument("--label", default=None)
    ap.add_argument("--no-child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dice_step_time.jsonl"))
    a = ap.parse_args()
    kinds = [int(k) for k in a.kinds.split(",")]
    route = a.label or ("composed (IMK_DICE_FUSED=0)" if os.environ.get("IMK_DICE_FUSED", "1")[0] == "0" else "default")
    for name, (h, w, c, k, alpha) in SHAPES.items():
        if a.only and name != a.only:
            continue
        model = UNet(h, w, c, k, alpha, "sigmoid", seed=1)
        rng = np.random.default_rng(0)
        x = torch.from_numpy(rng.integers(0, 256, (BATCH, h, w, c), dtype=np.uint8)).cuda()
        y = torch.from_numpy((rng.random((BATCH, h, w, k)) < 0.3).astype(np.uint8)).cuda()
        model.init_train_state()
        fns = [lambda kind=kind: model.fwd_bwd(x, y, kind) for kind in kinds]
        times = windows(fns, a.reps, a.inner)
        rec = {"shape": name, "hw": [h, w], "c": c, "K": k, "alpha": alpha, "batch": BATCH, "reps": a.reps, "inner": a.inner, "route": route}
        for kind, t in zip(kinds, times):
            model.fwd_bwd(x, y, kind)
            torch.cuda.synchronize()
            rec[f"kind{kind}_ms_median"] = round(statistics.median(t), 4)
            rec[f"kind{kind}_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
            rec[f"kind{kind}_loss"] = float(model.stats[0])
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del model
    if 4 in kinds and not a.no_child and route == "default":      # the composed route: a fresh process, the switch is read once
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--inner", str(a.inner), "--out", a.out, "--no-child"]
        if a.only:
            cmd += ["--only", a.only]
        torch.cuda.synchronize()
        subprocess.run(cmd, env=dict(os.environ, IMK_DICE_FUSED="0"), check=True)


if __name__ == "__main__":
    main()
