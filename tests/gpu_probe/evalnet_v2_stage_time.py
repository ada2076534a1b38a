"""Time the EvalNet scoring stage with the late-fusion network (get_evalnet_miou_v2) at the HeLa shape, with device events after warm-up:
256 x 256, brightfield + 3 masks, alpha 2, N = 3 EvalNets, B = 32 images x M = 10 candidates through imk_evalnet_forward_select.
  a  v2, the image tower (input block + four conv blocks) once per image
  b  v2 with IMK_SELECT_SHARED=0: imk_evalnet_forward's launches on a device-side repeat of the images
  c  v1 (get_evalnet_miou), shared tower: the network the scripts build today
  step_v2 / step_v1  one training step (fwd_bwd + AdamW) at batch 32
Every arm runs in a fresh child process of this script (the switch is read once per process), the arms alternating over --rounds; a
child warms up, then times --reps windows of --inner calls.  The parent process never touches the GPU.  Per arm the median over all
windows is printed with its min .. max, one JSON line each; arms a and b must give the same outputs (digest).

    python tests/gpu_probe/evalnet_v2_stage_time.py [--rounds 2] [--reps 5] [--inner 10] [--out profiles/evalnet_v2_stage_time.jsonl]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H = W = 256
CA, CB, ALPHA, N, B, M, TRAIN_B = 1, 3, 2.0, 3, 32, 10, 32
ARMS = {"a": ("v2", "1"), "b": ("v2", "0"), "c": ("v1", "1"), "step_v2": ("v2", "1"), "step_v1": ("v1", "1")}


def child(a):
    import numpy as np
    import torch
    from inconsistencymasks_amd import evalnet as E
    arch = ARMS[a.arm][0]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rng = np.random.default_rng(3)
    make = lambda seed: E.EvalNet(H, W, CA, CB, CB, ALPHA, True, True, False, seed=seed, arch=arch)
    if a.arm.startswith("step"):
        m = make(40)
        xa = torch.from_numpy(rng.integers(0, 256, (TRAIN_B, H, W, CA), dtype=np.uint8)).cuda()
        xb = torch.from_numpy(rng.integers(0, 2, (TRAIN_B, H, W, CB), dtype=np.uint8)).cuda()
        y = torch.from_numpy(rng.random((TRAIN_B, 2 * CB)).astype(np.float32)).cuda()
        y[:, CB:] = (y[:, CB:] > 0.5).float()
        m.init_train_state()
        call = lambda: m.train_step(xa, xb, y, 3e-3, 1e-4)
        tail = lambda: [m.stats[:1].clone()]
    else:
        models = [make(40 + j) for j in range(N)]
        xa = torch.from_numpy(rng.integers(0, 256, (B, H, W, CA), dtype=np.uint8)).cuda()
        xb = torch.from_numpy(rng.integers(0, 2, (B, M, H, W, CB), dtype=np.uint8)).cuda()
        cand = (xb * 255).reshape(B, M, H * W * CB)
        scorer = E.CandidateScorer(models)
        res = {}

        def call():
            res["out"] = scorer.run(xa, xb, cand, 0.5, None)
        tail = lambda: list(res["out"]) + [scorer.last_scores]
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        ev[0].record()
        for _ in range(a.inner):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]) / a.inner)
    dig = hashlib.sha256()
    for t in tail():
        dig.update(t.cpu().numpy().tobytes())
    print(json.dumps({"arm": a.arm, "ms": ms, "digest": dig.hexdigest()[:16]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--arm", choices=sorted(ARMS))
    a = ap.parse_args()
    if a.arm:
        return child(a)
    acc = {}
    for _ in range(a.rounds):
        for arm, (_, shared) in ARMS.items():
            argv = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--reps", str(a.reps), "--inner", str(a.inner), "--warmup",
                    str(a.warmup)]
            r = subprocess.run(argv, env=dict(os.environ, IMK_SELECT_SHARED=shared), capture_output=True, text=True, timeout=600, cwd=ROOT)
            if r.returncode != 0:      # a child that failed ends the measurement: nothing more is started on the GPU
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return r.returncode
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    rec = json.loads(line)
                    e = acc.setdefault(rec["arm"], {"ms": [], "digests": set()})
                    e["ms"] += rec["ms"]
                    e["digests"].add(rec["digest"])
    lines = []
    for arm, e in acc.items():
        rec = {"arm": arm, "arch": ARMS[arm][0], "hw": [H, W], "alpha": ALPHA, "windows": len(e["ms"]), "inner": a.inner,
               "ms_median": round(statistics.median(e["ms"]), 3), "ms_min_max": [round(min(e["ms"]), 3), round(max(e["ms"]), 3)]}
        if arm.startswith("step"):
            rec["batch"] = TRAIN_B
        else:
            rec.update(n=N, batch=B, M=M, shared=ARMS[arm][1] == "1", one_digest_per_arm=len(e["digests"]) == 1)
        lines.append(rec)
    if "a" in acc and "b" in acc:
        same = acc["a"]["digests"] == acc["b"]["digests"] and len(acc["a"]["digests"]) == 1
        med = {r["arm"]: r["ms_median"] for r in lines}
        lines.append({"a_and_b_same_outputs": same, "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / med["c"], 4),
                      "step_v2_over_step_v1": round(med["step_v2"] / med["step_v1"], 4)})
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
