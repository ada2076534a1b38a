"""Time the pseudo-label stage of the EvalNet-ensemble baseline per call at the real shapes, with device events after warm-up:
B images with M candidate masks each, scored by the n EvalNets of the ensemble, arg-max, threshold, gather.
  shared    imk_evalnet_forward_select: the image tower once per image
  repeated  the same call with IMK_SELECT_SHARED=0: imk_evalnet_forward per model on a device-side repeat of the images
  parent    what the library offered before: n x imk_evalnet_forward on the repeated images, the scores to the host, the rule in numpy,
            a torch gather of the chosen candidates (timed on the host clock around a synchronise: it has a host step in it)
The switch is read once per process, so the two arms run in child processes of this script, alternating (--rounds of each); every
child times every shape in --reps windows of --inner calls.  The parent process never touches the GPU.  Per shape the medians over all
windows of an arm are printed with their min .. max, one JSON line each, and the children's outputs are compared through a digest.

    python tests/gpu_probe/evalnet_select_stage_time.py [--only NAME] [--batch 8] [--rounds 2] [--reps 5] [--inner 40] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {   # name: (H, W, ca, cb, n_out, two_heads, normalize_b, b_onehot, alpha of the EvalNet, M, n)
    "isic_m10": (256, 256, 3, 1, 1, False, True, False, 1.0, 10, 4),
    "hela_m10": (256, 256, 1, 3, 3, True, False, False, 2.0, 10, 4),
    "hela_m6": (256, 256, 1, 3, 3, True, False, False, 2.0, 6, 4),
    "suim_m10": (256, 256, 3, 9, 9, True, False, True, 2.0, 10, 4),
    "suim_m6": (256, 256, 3, 9, 9, True, False, True, 2.0, 6, 4),
    "cityscapes_m10": (208, 416, 3, 35, 35, True, False, True, 2.0, 10, 4),
    "cityscapes_m6": (208, 416, 3, 35, 35, True, False, True, 2.0, 6, 4),
}


def child(a):
    import numpy as np
    import torch
    from inconsistencymasks_amd import evalnet as E
    shared = os.environ.get("IMK_SELECT_SHARED", "1") != "0"
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for name, (h, w, ca, cb, n_out, two, norm_b, onehot, alpha, m, n) in SHAPES.items():
        if a.only and name != a.only:
            continue
        b = a.batch
        models = [E.EvalNet(h, w, ca, cb, n_out, alpha, two, True, norm_b, seed=40 + j, b_onehot=onehot) for j in range(n)]
        rng = np.random.default_rng(3)
        xa = torch.from_numpy(rng.integers(0, 256, (b, h, w, ca), dtype=np.uint8)).cuda()
        if onehot:
            xb = torch.from_numpy(rng.integers(0, cb, (b, m, h, w), dtype=np.uint8)).cuda()
            cand = xb.reshape(b, m, h * w)
        else:
            xb = torch.from_numpy((rng.integers(0, 2, (b, m, h, w, cb), dtype=np.uint8) * (255 if norm_b else 1)).astype(np.uint8)).cuda()
            cand = (xb * (1 if norm_b else 255)).reshape(b, m, h * w * cb)
        counts = torch.from_numpy(np.array([m - (i % 2) for i in range(b)], np.int32)).cuda() if m in (6, 11) else None
        scorer = E.CandidateScorer(models)
        thr = 0.5

        def fused():
            return scorer.run(xa, xb, cand, thr, counts)

        def parent_style():
            rep = xa.repeat_interleave(m, 0)
            flat = xb.reshape((b * m,) + tuple(xb.shape[2:]))
            flat = flat if flat.dim() == 4 else flat[..., None]
            sc = torch.stack([mod.predict_device(rep, flat).reshape(b, m, -1) for mod in models], 0).cpu().numpy()
            mean = sc[0].copy()
            for q in range(1, n):
                mean = mean + sc[q]
            mean = mean / np.float32(n)
            if two:
                ok = mean[..., n_out:] >= np.float32(0.5)
                cnt = ok.sum(-1)
                score = np.where(cnt > 0, (mean[..., :n_out] * ok).sum(-1) / np.maximum(cnt, 1), 0).astype(np.float32)
            else:
                score = mean[..., 0]
            if counts is not None:
                score = np.where(np.arange(m)[None] < counts.cpu().numpy()[:, None], score, -np.inf)
            best = torch.from_numpy(np.argmax(score, 1)).cuda()
            return cand[torch.arange(b, device="cuda"), best]

        for _ in range(3):
            out = fused()
            parent_style()
        torch.cuda.synchronize()
        t_fused, t_parent = [], []
        for _ in range(a.reps):
            ev[0].record()
            for _ in range(a.inner):
                out = fused()
            ev[1].record()
            torch.cuda.synchronize()
            t_fused.append(ev[0].elapsed_time(ev[1]) / a.inner)
            if shared:
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    parent_style()
                torch.cuda.synchronize()
                t_parent.append((time.perf_counter() - t0) * 1e3 / a.inner)
        dig = hashlib.sha256()
        for t in list(out) + [scorer.last_scores]:
            dig.update(t.cpu().numpy().tobytes())
        print(json.dumps({"shape": name, "shared": shared, "ms": t_fused, "parent_ms": t_parent, "digest": dig.hexdigest()[:16],
                          "kept": int(out[2].sum())}), flush=True)
        del models, scorer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=40)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    acc = {}
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch), "--reps", str(a.reps), "--inner", str(a.inner)]
    if a.only:
        argv += ["--only", a.only]
    for _ in range(a.rounds):
        for arm in ("1", "0"):
            r = subprocess.run(argv, env=dict(os.environ, IMK_SELECT_SHARED=arm), capture_output=True, text=True, timeout=900, cwd=ROOT)
            if r.returncode != 0:      # a child that failed ends the measurement: nothing more is started on the GPU
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return r.returncode
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    rec = json.loads(line)
                    e = acc.setdefault(rec["shape"], {"shared": [], "repeated": [], "parent": [], "digests": set(), "kept": rec["kept"]})
                    e["shared" if rec["shared"] else "repeated"] += rec["ms"]
                    e["parent"] += rec["parent_ms"]
                    e["digests"].add(rec["digest"])
    lines = []
    for name, e in acc.items():
        h, w, ca, cb, n_out, two, norm_b, onehot, alpha, m, n = SHAPES[name]
        rec = {"shape": name, "hw": [h, w], "alpha": alpha, "batch": a.batch, "M": m, "n": n, "kept": e["kept"],
               "same_outputs": len(e["digests"]) == 1, "windows_per_arm": len(e["shared"])}
        for arm in ("shared", "repeated", "parent"):
            rec[arm + "_ms_median"] = round(statistics.median(e[arm]), 3)
            rec[arm + "_ms_min_max"] = [round(min(e[arm]), 3), round(max(e[arm]), 3)]
        rec["shared_over_repeated"] = round(rec["shared_ms_median"] / rec["repeated_ms_median"], 4)
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
