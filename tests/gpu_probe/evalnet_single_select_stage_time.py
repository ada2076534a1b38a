"""Time the selection stage of the single-EvalNet baseline per call at the real shapes, with device events after warm-up: B images
with M candidate masks each, scored by ONE EvalNet, then the rule + gather.
  isic_m10   256 x 256, one sigmoid unit, IMK_SELECT_IOU
  suim_m10   256 x 256, 9 classes, IMK_SELECT_CONF_GATED (the gate over the image's candidates, the score from the detection units)
Per shape three timings, each the median over --reps windows of --inner calls (the rule alone: 50 x --inner calls, it is microseconds
long) with its min .. max:
  fused_ms   imk_evalnet_forward_select (scoring + rule + gather, what the writers call per batch)
  scores_ms  imk_evalnet_forward_candidates alone
  rule_ms    imk_evalnet_select alone on those scores (the rule kernel: rule + gather of B x H x W bytes)
so that rule_ms / fused_ms says how much of the stage the rule kernel is.  A record, not a gate.

    python tests/gpu_probe/evalnet_single_select_stage_time.py [--batch 8] [--reps 5] [--inner 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {   # name: (H, W, ca, cb, n_out, two_heads, normalize_b, b_onehot, alpha of the EvalNet, M, mode)
    "isic_m10": (256, 256, 3, 1, 1, False, True, False, 1.0, 10, 0),
    "suim_m10": (256, 256, 3, 9, 9, True, False, True, 2.0, 10, 2),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from inconsistencymasks_amd import evalnet as E
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lines = []
    for name, (h, w, ca, cb, n_out, two, norm_b, onehot, alpha, m, mode) in SHAPES.items():
        b = a.batch
        model = E.EvalNet(h, w, ca, cb, n_out, alpha, two, True, norm_b, seed=40, b_onehot=onehot)
        rng = np.random.default_rng(3)
        xa = torch.from_numpy(rng.integers(0, 256, (b, h, w, ca), dtype=np.uint8)).cuda()
        if onehot:
            xb = torch.from_numpy(rng.integers(0, cb, (b, m, h, w), dtype=np.uint8)).cuda()
        else:
            xb = torch.from_numpy((rng.integers(0, 2, (b, m, h, w, cb), dtype=np.uint8) * 255).astype(np.uint8)).cuda()
        cand = xb.reshape(b, m, -1)
        scorer = E.CandidateScorer([model])
        scores = scorer.scores(xa, xb)
        thr = float(scores[0, :, :, -1].max(1).values.median())
        arms = {"fused_ms": lambda: scorer.run(xa, xb, cand, thr, None, mode), "scores_ms": lambda: scorer.scores(xa, xb),
                "rule_ms": lambda: E.select_candidates(scores, cand, thr, mode)}
        for f in arms.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, f in arms.items():
                inner = a.inner * (50 if k == "rule_ms" else 1)
                ev[0].record()
                for _ in range(inner):
                    out = f()
                ev[1].record()
                torch.cuda.synchronize()
                times[k].append(ev[0].elapsed_time(ev[1]) / inner)
        fused, alone = scorer.run(xa, xb, cand, thr, None, mode), E.select_candidates(scores, cand, thr, mode)
        rec = {"shape": name, "hw": [h, w], "alpha": alpha, "batch": b, "M": m, "n": 1, "mode": mode, "windows": a.reps, "inner": a.inner,
               "kept": int(fused[2].sum()), "same_outputs": all(torch.equal(x, y) for x, y in zip(fused, alone))}
        for k, v in times.items():
            rec[k + "_median"] = round(statistics.median(v), 4)
            rec[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
        rec["rule_share_of_fused"] = round(rec["rule_ms_median"] / rec["fused_ms_median"], 4)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        del model, scorer, out
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
