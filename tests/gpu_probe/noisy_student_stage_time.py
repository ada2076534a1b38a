"""Time the noisy-student teacher pass per call at the real shapes (batch 32) and at the first and last generation's strength, with
device events, both routes from ONE process, alternating:
  (i)  the sequence the library offered before imk_unet_forward_student, on one stream: imk_unet_forward (fp32 probabilities), the
       label step (the single-member vote kernels), imk_augment with the label as its mask;
  (ii) imk_unet_forward_student: head + label + geometry in one kernel, the image path on a side stream.
Medians over --reps timed windows of --inner calls each, with the run-to-run spread (min .. max of the windows) beside them; the
outputs of both routes are compared.  Prints one JSON line per shape and strength.  The label kernel of (ii) is also timed alone
through the library's profiling hook, against its algorithmic bytes (the fp16 activation read once + the label written once).

    python tests/gpu_probe/noisy_student_stage_time.py [--only isic|hela|suim|cityscapes] [--reps 7] [--inner 200] [--single-stream] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from inconsistencymasks_amd import noisy_student as ns  # noqa: E402
from inconsistencymasks_amd import prof  # noqa: E402
from inconsistencymasks_amd.augment import augment_batch, draw_params  # noqa: E402
from inconsistencymasks_amd.im_driver import NOISY_STUDENT  # noqa: E402
from inconsistencymasks_amd.input_ensemble import vote_views_binary  # noqa: E402
from inconsistencymasks_amd.unet import UNet  # noqa: E402
from inconsistencymasks_amd.vote import vote_multiclass  # noqa: E402

BATCH = 32
PF_IM = 15      # the profiling family of the label kernels (imk_common.h)
SHAPES = {   # name: (dataset, H, W, C, K, act, cmp_ge, free rotation as config.ini has it)
    "isic": ("ISIC_2018", 256, 256, 3, 1, "sigmoid", False, True),
    "hela": ("HeLa", 256, 256, 1, 3, "sigmoid", True, True),
    "suim": ("SUIM", 256, 256, 3, 9, "softmax", False, False),
    "cityscapes": ("Cityscapes", 208, 416, 3, 35, "softmax", False, False),
}


def windows(fns, reps, inner):
    """per-call milliseconds of every fn: `reps` windows of `inner` calls each, the fns alternating window by window"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for fn in fns:
        for _ in range(3):
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
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--single-stream", action="store_true", help="also time (ii) without its side stream")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []
    for name, (ds, h, w, c, k, act, cmp_ge, free) in SHAPES.items():
        if a.only and name != a.only:
            continue
        sched = NOISY_STUDENT[ds]
        for gen in (0, 4):
            alpha = sched["alphas"][gen]
            model = UNet(h, w, c, k, alpha, act, seed=1)
            rng = np.random.default_rng(gen)
            x = torch.from_numpy(rng.integers(0, 256, (BATCH, h, w, c), dtype=np.uint8)).cuda()
            img = x.flip(-1).contiguous() if c == 3 else x
            import random
            prm = draw_params(BATCH, sched["bra"][gen], sched["brb"][gen], sched["max_blurs"][gen], sched["max_noises"][gen], free,
                              rng=random.Random(gen), np_rng=np.random.RandomState(gen))
            tl = ns.TeacherLabel(model, act == "sigmoid")

            def fused():
                return tl.run(x, img, prm, 0.5, cmp_ge)

            def sequence():
                p = model.predict_device(x)
                if act == "sigmoid":
                    lab = vote_views_binary(p[None], None, 0.5, cmp_ge)                 # [B,K,H,W]
                    lab = lab.permute(0, 2, 3, 1).contiguous() if k > 1 else lab.reshape(BATCH, h, w, 1)
                else:
                    lab = vote_multiclass(p[None], soft=False)[..., None]
                return augment_batch(img, lab, prm)

            t_seq, t_fused = windows([sequence, fused], a.reps, a.inner)
            t_single = None
            if a.single_stream:      # (ii) with the image path on the caller's stream: what the fork / join costs or hides
                model.debug(single_stream=True)
                t_single = windows([fused], a.reps, a.inner)[0]
                model.debug(single_stream=False)
            o1, l1 = fused()
            o2, l2 = sequence()
            l2 = l2.permute(0, 3, 1, 2) if act == "sigmoid" else l2[..., 0]
            torch.cuda.synchronize()
            # the label kernel's floor: the fp16 activation [B,H,W,cs] read once + the label map(s) written once
            cs = -(-int(round(16 * alpha)) // 8) * 8
            label_bytes = BATCH * h * w * (cs * 2 + (k if act == "sigmoid" else 1))
            rec = {"shape": name, "hw": [h, w], "K": k, "gen": gen, "alpha": alpha, "batch": BATCH, "max_blur": sched["max_blurs"][gen],
                   "free_rotation": free, "quarter_turns": int(sum(q.rot in (1, 3) for q in prm)),
                   "sequence_ms_median": round(statistics.median(t_seq), 4), "sequence_ms_min_max": [round(min(t_seq), 4), round(max(t_seq), 4)],
                   "student_ms_median": round(statistics.median(t_fused), 4), "student_ms_min_max": [round(min(t_fused), 4), round(max(t_fused), 4)],
                   "label_kernel_floor_bytes": label_bytes,
                   "same_image": bool(torch.equal(o1, o2)), "same_labels": bool(torch.equal(l1, l2))}
            if t_single:
                rec["student_single_stream_ms_median"] = round(statistics.median(t_single), 4)
                rec["student_single_stream_ms_min_max"] = [round(min(t_single), 4), round(max(t_single), 4)]
            # the label kernel alone: every launch of the family timed by the library's own device events (it is the only kernel of the
            # fused call in that family; the forward's kernels and imk_augment are in others or in none)
            pf = prof.Profiler(1)
            try:
                for _ in range(10):
                    fused()
                torch.cuda.synchronize()
                n, ms, by, _ = pf.collect()
            finally:
                pf.close()
            if n[PF_IM]:
                rec["label_kernel_us"] = round(1e3 * ms[PF_IM] / n[PF_IM], 2)
                rec["label_kernel_TBps"] = round(by[PF_IM] / n[PF_IM] / (ms[PF_IM] / n[PF_IM] * 1e-3) / 1e12, 3)
                assert by[PF_IM] / n[PF_IM] == label_bytes, (by[PF_IM] / n[PF_IM], label_bytes)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del model, tl
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
