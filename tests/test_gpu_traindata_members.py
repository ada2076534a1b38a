"""The EvalNet training-data writers of the IM++ family on their two routes, at toy size (5 pool models, 12 images of 32 x 32 or
32 x 48, 2 loops, a fixed seed): IMK_TRAINDATA_POOLED=1 (one model pool with per-image member sets, one ensemble call per chunk of
the file list, one imk_morph_var per operation) against IMK_TRAINDATA_POOLED=0 (the images grouped by sub-ensemble).  Every PNG file
and labels.csv have to be byte-identical, and the pooled run has to make exactly one ensemble call per chunk.

The switch is read once per process, so every run is a fresh child (tests/traindata_members_runner.py), started one after another,
each under its own timeout; after a child that ended by a signal, a timeout or an error, no further child is started."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import traindata_members_runner as R  # noqa: E402

CHILD_TIMEOUT_S = 120
INFER_BATCH = 5                       # 12 images: chunks of 5, 5 and 2
_DIED = []


def run_child(kind, pooled, data_dir, out_dir):
    assert not _DIED, f"earlier child died: {_DIED[0]}"
    cmd = [sys.executable, os.path.join(HERE, "traindata_members_runner.py"), kind, data_dir, out_dir]
    env = dict(os.environ, IMK_TRAINDATA_POOLED=str(int(pooled)), IMK_INFER_BATCH=str(INFER_BATCH))
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        _DIED.append(f"{kind}, pooled={pooled}: ran into its {CHILD_TIMEOUT_S} s timeout")
        raise AssertionError(_DIED[0] + "\n" + str(e.stderr or "")[-3000:])
    if r.returncode != 0:
        _DIED.append(f"{kind}, pooled={pooled}: ended with return code {r.returncode}")
        raise AssertionError(_DIED[0] + "\n" + r.stdout[-2000:] + r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


@pytest.mark.parametrize("kind", sorted(R.KINDS))
def test_pooled_route_writes_the_grouped_route_s_bytes(kind, tmp_path):
    data = str(tmp_path / "data")
    pooled = run_child(kind, True, data, str(tmp_path / "pooled"))
    grouped = run_child(kind, False, data, str(tmp_path / "grouped"))
    a, b = tree(str(tmp_path / "pooled")), tree(str(tmp_path / "grouped"))
    n_dirs = 4 if kind == "hela" else 2
    assert sorted(a) == sorted(b) and len(a) == n_dirs * R.N_IMAGES * R.N_LOOPS + 1 and "labels.csv" in a
    diff = [name for name in sorted(a) if a[name] != b[name]]
    assert not diff, f"{len(diff)} of {len(a)} files differ between the routes: {diff[:6]}"
    assert len(a["labels.csv"].splitlines()) == R.N_IMAGES * R.N_LOOPS
    chunks = -(-R.N_IMAGES // INFER_BATCH)
    assert pooled["infer_batch"] == grouped["infer_batch"] == INFER_BATCH
    assert pooled == {"pool_calls": R.N_LOOPS * chunks, "ensemble_calls": 0, "infer_batch": INFER_BATCH}, pooled
    assert grouped["pool_calls"] == 0 and grouped["ensemble_calls"] > R.N_LOOPS * chunks, grouped
