"""Where a data-preparation stage spends its time: decode, upload, kernel, download and encode of
  (i)  64 Cityscapes-sized pairs (1024 x 2048 RGB image, linear, and label map, nearest + 1) -> 208 x 416, PNG in and out;
  (ii) 64 ragged ISIC-like JPEGs (540 x 720 ... 2000 x 3008) -> 256 x 256, one ragged batch.
The files are generated from a seed into a temporary directory and go through the directory stages' own path (prep.stage_batches /
prep.resize_batch: batches of at most 256 MB of decoded sources).  Decode is host wall time of the header pass plus the pool threads'
decode straight into the pinned staging buffer (a grey label file as one plane), so nothing is packed outside a timed stage; encode
is host wall time of functions.write_png on the same pool (IMK_IO_THREADS threads); upload, kernel and download are device events.
One untimed pass first (code objects, the pinned staging buffer, the pools' threads), then --reps timed passes; medians with min .. max.  Appends one JSON line per case to --out.  Not part of the test suite.

    python tests/gpu_probe/prep_stage_time.py [--only cityscapes|isic] [--reps 5] [--out profiles/prep_stage_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from inconsistencymasks_amd import functions as F  # noqa: E402
from inconsistencymasks_amd import prep  # noqa: E402

N = 64
ISIC_SIZES = [(540, 720), (768, 1024), (1129, 1504), (1536, 2048), (2000, 3008)]


def scene(rng, h, w):
    """blocks of colour with a little noise on top: compresses like a photograph rather than like noise"""
    base = rng.integers(0, 256, (h // 32 + 1, w // 32 + 1, 3), dtype=np.uint8).repeat(32, 0).repeat(32, 1)[:h, :w]
    return (base.astype(np.int16) + rng.integers(-6, 7, (h, w, 3))).clip(0, 255).astype(np.uint8)


def generate(root, case, rng):
    jobs = []
    for i in range(N):
        if case == "cityscapes":
            img, lab = os.path.join(root, f"c_{i:03d}_leftImg8bit.png"), os.path.join(root, f"c_{i:03d}_gtFine_labelIds.png")
            F.write_png(img, scene(rng, 1024, 2048))
            F.write_png(lab, rng.integers(0, 34, (1024 // 64, 2048 // 64), dtype=np.uint8).repeat(64, 0).repeat(64, 1))
            size = lambda h, w: prep.cityscapes_size(h, w, 0.2)
            jobs += [prep.ResizeJob(img, 3, size, prep.IMK_PREP_LINEAR, 0, os.path.join(root, "out", f"c_{i:03d}_image.png")),
                     prep.ResizeJob(lab, 3, size, prep.IMK_PREP_NEAREST, prep.IMK_PREP_LABEL_PLUS1, os.path.join(root, "out", f"c_{i:03d}_mask.png"))]
        else:
            h, w = ISIC_SIZES[i % len(ISIC_SIZES)]
            path = os.path.join(root, f"ISIC_{i:07d}.jpg")
            Image.fromarray(scene(rng, h, w)).save(path, quality=95)
            jobs.append(prep.ResizeJob(path, 3, lambda h, w: (256, 256), prep.IMK_PREP_LINEAR, 0, os.path.join(root, "out", f"ISIC_{i:07d}.png")))
    return jobs


def one_pass(jobs, out_dir):
    """the product path of a directory stage (prep.stage_batches / prep.resize_batch) with its writes timed instead of queued"""
    t = {"encode_ms": 0.0, "batches": 0}
    with F._pool() as pool:
        for batch in prep.stage_batches(pool, jobs, timing=t):      # headers, then per batch: decode INTO the pinned buffer (decode_ms)
            writes = prep.resize_batch(pool, batch, timing=t)       # upload / kernel / download: device events
            t0 = time.perf_counter()
            pool.map(lambda w: F.write_png(*w), writes)
            t["encode_ms"] += (time.perf_counter() - t0) * 1e3
            t["batches"] += 1
            t["source_mb"] = t.get("source_mb", 0.0) + batch[0] / 1e6
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("cityscapes", "isic"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep_stage_time.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    for case in ("cityscapes", "isic"):
        if a.only and case != a.only:
            continue
        with tempfile.TemporaryDirectory() as root:
            out_dir = os.path.join(root, "out")
            os.makedirs(out_dir)
            jobs = generate(root, case, np.random.default_rng(20261019))
            one_pass(jobs, out_dir)
            runs = [one_pass(jobs, out_dir) for _ in range(a.reps)]
        stages = ("decode_ms", "upload_ms", "kernel_ms", "download_ms", "encode_ms")
        rec = {"case": case, "files": len(jobs), "source_mb": round(runs[0]["source_mb"], 1), "batches": runs[0]["batches"], "reps": a.reps,
               "io_threads": F._IO_THREADS}
        for s in stages:
            v = [r[s] for r in runs]
            rec[s.replace("_ms", "_ms_median")] = round(statistics.median(v), 3)
            rec[s.replace("_ms", "_ms_min_max")] = [round(min(v), 3), round(max(v), 3)]
        rec["dominant"] = max(stages, key=lambda s: rec[s.replace("_ms", "_ms_median")])[:-3]
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
