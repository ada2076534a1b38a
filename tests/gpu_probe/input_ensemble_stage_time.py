"""Time the input-ensemble pseudo-label stage at real sizes with device events: view generation (imk_views), the fused route
(imk_unet_forward_views_vote: one forward over the B*M views + the vote fused with the head) and the unfused route at the same shapes
(the same forward writing fp32 probabilities, then the stack vote), per call and summed over the set.  Prints one JSON line per shape
and checks that both routes give the same labels.  Kernel times come from a separate run under rocprofv3 --kernel-trace --stats.

    python tests/gpu_probe/input_ensemble_stage_time.py [--only isic|cityscapes] [--reps 3]
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from inconsistencymasks_amd import input_ensemble as ie  # noqa: E402
from inconsistencymasks_amd import vote  # noqa: E402
from inconsistencymasks_amd.functions import infer_batch_size  # noqa: E402
from inconsistencymasks_amd.unet import UNet  # noqa: E402

SHAPES = {   # name: (images, H, W, C, K, alpha, act, chain, views per image)
    "isic": [(2335, 256, 256, 3, 1, 0.5, "sigmoid", False, m) for m in (3, 5, 7)],
    "cityscapes": [(500, 208, 416, 3, 35, 1.0, "softmax", True, m) for m in (4, 6, 8)],
}


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        best = min(best, ev[0].elapsed_time(ev[1]))
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for name, shapes in SHAPES.items():
        if a.only and name != a.only:
            continue
        for n_img, h, w, c, k, alpha, act, chain, m in shapes:
            model = UNet(h, w, c, k, alpha, act, seed=1)
            vv = ie.ViewVote(model, act == "sigmoid")
            b = max(1, infer_batch_size(alpha) // m)
            rng = np.random.default_rng(0)
            x = torch.from_numpy(rng.integers(0, 256, (b, h, w, c), dtype=np.uint8)).cuda()
            random.seed(0)
            if chain:
                per = [ie.draw_chain_views(m - 1, np_rng=np.random.RandomState(i)) for i in range(b)]
            else:
                per = [ie.draw_random_views(m, np_rng=np.random.RandomState(i)) for i in range(b)]
            plan = ie.ViewPlan(per, chain=chain, restore=not chain)
            mode, cmp_ge = (vote.VOTE_HARD, True) if act == "sigmoid" else (vote.VOTE_SOFT, False)
            t_views, views = timed(lambda: ie.make_views(x, plan), a.reps)
            p = model.plan
            nbytes = int(ie.lib.imk_unet_forward_views_vote_workspace_bytes(p.ptr, m, b))
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            ops = torch.from_numpy(plan.ops).cuda() if plan.restore else None
            shape = (b, p.n_out, h, w) if act == "sigmoid" else (b, h, w)
            out = torch.empty(shape, dtype=torch.uint8, device="cuda")

            def fused():
                ie.check(ie.lib.imk_unet_forward_views_vote(p.ptr, model.params.data_ptr(), model.packed.data_ptr(), views.data_ptr(), m, b,
                                                            ops.data_ptr() if ops is not None else None, plan.quarter, 0.5, mode, int(cmp_ge),
                                                            out.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream),
                         "imk_unet_forward_views_vote")
                return out.clone()

            def unfused():
                pr = model.predict_device(views.reshape(m * b, h, w, c))
                pr = pr.reshape(m, b, *pr.shape[1:])
                if plan.restore:
                    return ie.vote_views_binary(pr, plan.ops.reshape(m, b), 0.5, True)
                return vote.vote_multiclass(pr, True)

            t_fused, o1 = timed(fused, a.reps)
            t_unfused, o2 = timed(unfused, a.reps)
            calls = -(-n_img // b)
            view_bytes = 2.0 * m * b * h * w * c
            print(json.dumps({"shape": name, "images": n_img, "hw": [h, w], "alpha": alpha, "views": m, "images_per_call": b,
                              "calls": calls, "views_ms": round(t_views, 3), "fused_ms": round(t_fused, 3),
                              "unfused_ms": round(t_unfused, 3), "stage_fused_ms": round(calls * (t_views + t_fused), 1),
                              "stage_unfused_ms": round(calls * (t_views + t_unfused), 1),
                              "views_TBps_event": round(view_bytes / (t_views * 1e-3) / 1e12, 3), "same_labels": bool(torch.equal(o1, o2))}),
                  flush=True)
            del ws, views, out


if __name__ == "__main__":
    main()
