"""What the depth-map family's IM pass costs beside an ensemble's forwards: 256 x 256 x 3 images, alpha 0.5, N = 2 models, batch 128, on
one GPU.  Four calls on the same plans and buffers, timed with device events around `--reps` back-to-back calls per window, the four
taken in turn inside every window round (so that a drift of the clocks or a neighbour on the host meets all of them alike), after an
untimed warm-up of every call:

  fused        imk_unet_forward_im_depth (the std launch reads the two last decoder activations)
  unfused      imk_unet_forward x 2 into the fp32 stack + imk_im_depth (the same build's other route)
  forward_im   imk_unet_forward_im on the same plans: what a voting IM pass costs here, the yardstick
  rule         imk_im_depth alone on a stored stack
Medians over the windows with min .. max, in microseconds per call.  The rule's split into its three launches comes from a kernel
trace taken in a child process of its own (rocprofv3 --kernel-trace --stats around `--rule-only`); without rocprofv3 it is recorded
as not measured.  Appends one JSON line to --out.  Not part of the test suite.

    python tests/gpu_probe/depth_im_stage_time.py [--windows 7] [--reps 20] [--out profiles/depth_im_stage_time.jsonl]
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from inconsistencymasks_amd._lib import check, lib  # noqa: E402
from inconsistencymasks_amd.unet import UNet  # noqa: E402

H = W = 256
ALPHA, N, B = 0.5, 2, 128
KERNELS = ("depth_std_kernel", "depth_thr_kernel", "depth_mask_kernel")


def setup():
    models = [UNet(H, W, 3, 1, ALPHA, "sigmoid", seed=100 + j) for j in range(N)]
    for m in models:
        m.ready_for_inference()
    plan = models[0].plan
    dev = "cuda"
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
    o = dict(img_out=e(x.shape, torch.uint8), im=e((B, H, W), torch.uint8), masks=e((B, 1, H, W), torch.uint8),
             im_size=e((B, 1), torch.int64), pred_size=e((B, 1), torch.int64), thr=e((B,), torch.float32),
             stack=e((N, B, H, W), torch.float32))
    k = min(N, 3)
    ws_depth = e((lib.imk_unet_forward_im_depth_workspace_bytes(plan.ptr, N, B, k),), torch.uint8)
    ws_im = e((lib.imk_unet_forward_im_workspace_bytes(plan.ptr, N, B, k),), torch.uint8)
    ws_fwd = e((plan.workspace_bytes(B, 0),), torch.uint8)
    ws_rule = e((lib.imk_im_depth_workspace_bytes(B, H, W),), torch.uint8)
    params = (ctypes.c_void_p * N)(*[m.params.data_ptr() for m in models])
    packed = (ctypes.c_void_p * N)(*[m.packed.data_ptr() for m in models])
    s = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731

    def rule():
        check(lib.imk_im_depth(o["stack"].data_ptr(), N, B, H, W, 2.0, x.data_ptr(), 3, 1, o["img_out"].data_ptr(), o["im"].data_ptr(),
                               o["im_size"].data_ptr(), o["thr"].data_ptr(), None, ws_rule.data_ptr(), ws_rule.numel(), s()), "imk_im_depth")

    def fused():
        check(lib.imk_unet_forward_im_depth(plan.ptr, N, params, packed, x.data_ptr(), B, 2.0, x.data_ptr(), 1, o["img_out"].data_ptr(),
                                            o["im"].data_ptr(), o["im_size"].data_ptr(), o["thr"].data_ptr(), None, ws_depth.data_ptr(),
                                            ws_depth.numel(), s()), "imk_unet_forward_im_depth")

    def unfused():
        for j, m in enumerate(models):
            check(lib.imk_unet_forward(plan.ptr, m.params.data_ptr(), m.packed.data_ptr(), x.data_ptr(), B, o["stack"][j].data_ptr(),
                                       ws_fwd.data_ptr(), ws_fwd.numel(), s()), "imk_unet_forward")
        rule()

    def forward_im():
        check(lib.imk_unet_forward_im(plan.ptr, N, params, packed, x.data_ptr(), B, 0.5, 0, x.data_ptr(), 1, 1, o["img_out"].data_ptr(),
                                      o["masks"].data_ptr(), o["im"].data_ptr(), o["im_size"].data_ptr(), o["pred_size"].data_ptr(), None,
                                      ws_im.data_ptr(), ws_im.numel(), s()), "imk_unet_forward_im")
    return {"fused": fused, "unfused": unfused, "forward_im": forward_im, "rule": rule}, o


def window_us(call, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def rule_launches(reps):
    """{kernel: mean microseconds per launch} from a kernel trace of `--rule-only` in a child of its own, or None"""
    tool = shutil.which("rocprofv3")
    if not tool:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--rule-only", "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        if r.returncode != 0:
            return None
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    for k in KERNELS:
                        if k in row.get("Name", ""):
                            out[k] = round(float(row["AverageNs"]) / 1e3, 2)
        return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rule-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_im_stage_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    calls, o = setup()
    o["stack"].uniform_(0, 1)
    if a.rule_only:
        for _ in range(a.reps):
            calls["rule"]()
        torch.cuda.synchronize()
        return
    assert a.windows >= 5
    for c in calls.values():      # warm-up: code objects, the pool's side streams
        for _ in range(3):
            c()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(a.windows):
        for k, c in calls.items():
            t[k].append(window_us(c, a.reps))
    rec = {"case": f"{H}x{W}x3 alpha {ALPHA} N {N} batch {B}", "windows": a.windows, "reps_per_window": a.reps, "unit": "us per call"}
    for k, v in t.items():
        rec[k + "_median"] = round(statistics.median(v), 1)
        rec[k + "_min_max"] = [round(min(v), 1), round(max(v), 1)]
    rec["fused_beats_unfused_ranges_apart"] = max(t["fused"]) < min(t["unfused"])
    launches = rule_launches(a.reps)
    rec["rule_launches_us"] = launches if launches else "not measured"
    rec["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
