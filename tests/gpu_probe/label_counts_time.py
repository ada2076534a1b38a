"""Time imk_label_counts alone at the writers' shape -- 256 x 256 x 3, B = 128 -- with device events after warm-up, in a fresh
process, on segmentation-like maps (blocks of 16 x 16 pixels with stray pixels, 9 classes) and on uniformly random ones (no runs of
equal pixels: every pixel pays its LDS atomics):
  counts_ms      pred, gt -> counts (im NULL)
  blocked_ms     pred, gt, im, image in place, pred_blocked -> counts (the IM writer's one call per chunk)
  block_apply_ms imk_block_apply on the same im / image / prediction (what the call replaces on the device, without its counts)
Each is the median over --reps windows of --inner calls with its min .. max, next to its byte floor: the bytes the call has to read
and write at 8 TB/s (the maps once; of the image only the blocked pixels' bytes are written, counted here as the blocked share of it).
A record, not a gate.

    python tests/gpu_probe/label_counts_time.py [--batch 128] [--reps 7] [--inner 200] [--out profiles/label_counts_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from inconsistencymasks_amd import evaluate
    from inconsistencymasks_amd import im as IM
    from inconsistencymasks_amd._lib import lib
    from inconsistencymasks_amd.build import source_id
    assert torch.cuda.is_available(), "a timing needs the GPU"
    b, h, w, c, k = a.batch, 256, 256, 3, 9
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lines = []
    for maps in ("blocks", "random"):
        rng = np.random.default_rng(1)
        if maps == "blocks":
            gt = rng.integers(0, k, (b, h // 16, w // 16), dtype=np.uint8).repeat(16, 1).repeat(16, 2)
            pred = np.where(rng.random((b, h, w)) < 0.02, rng.integers(0, k, (b, h, w), dtype=np.uint8), gt).astype(np.uint8)
            im_np = (rng.random((b, h // 8, w // 8)) < 0.1).repeat(8, 1).repeat(8, 2).astype(np.uint8) * 255
        else:
            gt, pred = rng.integers(0, k, (b, h, w), dtype=np.uint8), rng.integers(0, k, (b, h, w), dtype=np.uint8)
            im_np = (rng.random((b, h, w)) < 0.1).astype(np.uint8) * 255
        gt, pred, im = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (gt, pred, im_np))
        image = torch.from_numpy(rng.integers(1, 256, (b, h, w, c), dtype=np.uint8)).cuda()
        out = torch.empty_like(pred)
        masks = pred.clone()[:, None].contiguous()
        share = float(im_np.mean() / 255)
        n = b * h * w
        floors = {"counts_ms": 2 * n + b * 8192, "blocked_ms": 4 * n + share * n * c + b * 8192, "block_apply_ms": n + share * n * (c + 1)}
        # evaluate.label_counts downloads the counts (a synchronise per call): the timed calls go to the C ABI directly
        counts = torch.empty((b, 4, 256), dtype=torch.int64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        arms = {"counts_ms": lambda: lib.imk_label_counts(pred.data_ptr(), gt.data_ptr(), None, None, 0, b, h, w, None, counts.data_ptr(), s),
                "blocked_ms": lambda: lib.imk_label_counts(pred.data_ptr(), gt.data_ptr(), im.data_ptr(), image.data_ptr(), c, b, h, w,
                                                           out.data_ptr(), counts.data_ptr(), s),
                "block_apply_ms": lambda: IM.block_apply(im, image, masks)}
        for f in arms.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for _ in range(a.reps):
            for name, f in arms.items():      # alternating: the arms share whatever else the machine is doing
                ev[0].record()
                for _ in range(a.inner):
                    f()
                ev[1].record()
                torch.cuda.synchronize()
                times[name].append(ev[0].elapsed_time(ev[1]) / a.inner)
        want = evaluate.label_counts(pred, gt, im, None, True)[1]
        rec = {"maps": maps, "hw": [h, w], "c": c, "batch": b, "classes": k, "blocked_share": round(share, 4), "windows": a.reps,
               "inner": a.inner, "source_id": source_id(), "counts_ok": bool((counts.cpu().numpy() == want).all())}
        for name, v in times.items():
            rec[name + "_median"] = round(statistics.median(v), 5)
            rec[name + "_min_max"] = [round(min(v), 5), round(max(v), 5)]
            rec[name.replace("_ms", "_floor_ms")] = round(floors[name] / HBM_BYTES_PER_S * 1e3, 5)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
