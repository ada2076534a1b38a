"""The C ABI's stream contract (include/imk.h, Conventions): every call leaves all of its work -- the part on the pool's side
streams included -- ordered after prior work on `stream` and before later work on `stream`.

The six entry points with fork / join logic of their own (imk_unet_fwd_bwd, imk_unet_consistency_fwd_bwd, imk_evalnet_fwd_bwd,
imk_unet_forward_im, imk_unet_forward_vote, imk_unet_forward_student) run under skewed streams with poison in every buffer a
premature reader could touch (tests/stream_skew.py; its planted defects: tests/test_gpu_stream_skew_harness.py), and every result
has to be bit-identical

  1. within a process and plan configuration, between every skew and the unskewed run, and between the two poison fills;
  2. between debug(single_stream=True) and the default;
  3. between IMK_SIDE_STREAMS = 0, 1 and 2 (the drivers' "no side stream of its own (results identical)" rests on this);
  4. with IMK_SIDE_STREAMS=0, whether or not the pool's side streams are held (part of 1 in that process).

IMK_SIDE_STREAMS is read once per process, so the runs live in tests/stream_order_runner.py, started here as a fresh child once
per value, one after another, each under its own timeout.  After a child that ended by a signal, a timeout or an error, no further
child is started: the remaining tests fail with "earlier child died".  The three `test_child_ran` items carry the children's run
time (holds of at least 50 ms each dominate it: 10-35 s per child); every other item only compares digests.
"""
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

import stream_order_runner as R  # noqa: E402

SIDE_STREAMS = (0, 1, 2)
CHILD_TIMEOUT_S = 240
_DOCS, _DIED = {}, []


def child(n, tmp_path_factory):
    """the finished run of the child with IMK_SIDE_STREAMS=n (children 0 .. n are started in order, each once)"""
    for k in SIDE_STREAMS[:SIDE_STREAMS.index(n) + 1]:
        if k in _DOCS:
            continue
        if _DIED:
            _DOCS[k] = f"earlier child died: {_DIED[0]}"
            continue
        out = str(tmp_path_factory.mktemp(f"stream_order_{k}") / "digests.json")
        cmd = [sys.executable, os.path.join(HERE, "stream_order_runner.py"), out]
        try:
            r = subprocess.run(cmd, env=dict(os.environ, IMK_SIDE_STREAMS=str(k)), capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT_S, cwd=ROOT)
        except subprocess.TimeoutExpired as e:
            _DIED.append(f"IMK_SIDE_STREAMS={k} ran into its {CHILD_TIMEOUT_S} s timeout")
            _DOCS[k] = _DIED[0] + "\n" + str(e.stderr or "")[-3000:]
            continue
        if r.returncode != 0:
            _DIED.append(f"IMK_SIDE_STREAMS={k} ended with return code {r.returncode}")
            _DOCS[k] = _DIED[0] + "\n" + r.stdout[-2000:] + r.stderr[-3000:]
            continue
        with open(out) as f:
            _DOCS[k] = json.load(f)
    doc = _DOCS[n]
    assert isinstance(doc, dict), doc
    return doc


@pytest.mark.parametrize("n", SIDE_STREAMS)
def test_child_ran(n, tmp_path_factory):
    doc = child(n, tmp_path_factory)
    assert doc["side_streams"] == n
    print(f"IMK_SIDE_STREAMS={n}: {doc['elapsed_s']} s, torch.cuda._sleep at {doc['cycles_per_ms']:.0f} cycles per ms")
    for case_id in sorted(doc["meta"]):
        print(f"  {case_id}: " + ", ".join(f"{c}: wall {v['wall_ms']} ms, holds {v['hold_ms']} ms" for c, v in sorted(doc["meta"][case_id].items())))
    assert sorted(doc["results"]) == sorted(R.training_case_ids() + R.inference_case_ids())


@pytest.mark.parametrize("n", SIDE_STREAMS)
def test_every_skew_was_real(n, tmp_path_factory):
    """no hold had been released when the call under it returned (run_skewed fails such a run; the child records the failure), and
    the caller's stream and the side streams do not share a hardware queue, so a held one leaves the others free to run ahead"""
    doc = child(n, tmp_path_factory)
    bad = [(case_id, config, skew, fill, d) for case_id, configs in doc["results"].items() for config, skews in configs.items()
           for skew, fills in skews.items() for fill, d in fills.items() if len(d) != 64]
    assert not bad, bad[:5]
    # ... and every hold sat in front of work the call waits for: under the hold of the caller's stream, or of a side stream the
    # call forks onto and joins, the caller's stream cannot be through before the hold is (0.8: the sleep's calibration).  A hold
    # that the call's work slipped past would let it finish in the undisturbed time.
    for case_id, configs in doc["meta"].items():
        for config, m in configs.items():
            used = {"main"} | {f"side{i}" for i in range(R.sides_in_use(case_id, n, config))}
            for skew, ms in m["synced_ms"].items():
                if skew != "none" and set(skew.replace(">", "+").split("+")) & used:
                    assert ms >= 0.8 * m["hold_ms"], (f"{case_id}, {config}, skew {skew!r}: the caller's stream was through after {ms} ms, "
                                                      f"the hold lasts {m['hold_ms']} ms")
    assert doc["caller_stream_runs_beside_the_side_streams"], "no caller stream off the side streams' hardware queues was found"
    assert doc["side_streams_run_beside_each_other"], "the pool's two side streams share a hardware queue"


def expected_skews(case_id, n):
    if case_id.endswith("/fwd_bwd"):
        return R.training_skews(n)
    if case_id.endswith("/steps"):
        return R.steps_skews(n)
    if case_id.startswith("student/"):
        return R.inference_skews(2)
    return R.inference_skews(int(case_id.rsplit("/k", 1)[1]))


def base_digest(doc, case_id, config="default"):
    return doc["results"][case_id][config]["none"]["FF"]


def check_case(case_id, tmp_path_factory):
    docs = {n: child(n, tmp_path_factory) for n in SIDE_STREAMS}
    for n, doc in docs.items():
        res = doc["results"][case_id]
        for config, skews in res.items():
            assert sorted(skews) == sorted(R.skew_name(s) for s in expected_skews(case_id, n)), (n, config, sorted(skews))
            want = skews["none"]["FF"]
            for skew, fills in skews.items():                                                # 1 (and 4 in the child with 0)
                assert sorted(fills) == ["3C", "FF"]
                for fill, d in fills.items():
                    assert d == want, (f"{case_id}, IMK_SIDE_STREAMS={n}, {config}: skew {skew!r} with fill 0x{fill} gives {d}, "
                                       f"the unskewed run with fill 0xFF {want}")
        if len(res) == 2:                                                                    # 2
            assert base_digest(doc, case_id, "single_stream") == base_digest(doc, case_id), \
                f"{case_id}, IMK_SIDE_STREAMS={n}: single_stream differs from the default"
    config = "default" if "default" in docs[0]["results"][case_id] else "single_stream"
    got = {n: base_digest(doc, case_id, config) for n, doc in docs.items()}                  # 3
    assert len(set(got.values())) == 1, f"{case_id}: the results depend on IMK_SIDE_STREAMS: {got}"


@pytest.mark.parametrize("case_id", R.training_case_ids())
def test_training_call_is_bit_identical_under_every_skew(case_id, tmp_path_factory):
    check_case(case_id, tmp_path_factory)


@pytest.mark.parametrize("case_id", R.inference_case_ids())
def test_inference_call_is_bit_identical_under_every_skew(case_id, tmp_path_factory):
    check_case(case_id, tmp_path_factory)


@pytest.mark.parametrize("call", ("im", "vote"))
@pytest.mark.parametrize("name", R.ENSEMBLE_CASES)
def test_ensemble_on_more_streams_equals_one_stream(name, call, tmp_path_factory):
    """every output of the ensemble calls on 2 and 3 streams against the unskewed run on one (with check_case: under every skew)"""
    for n in SIDE_STREAMS:
        doc = child(n, tmp_path_factory)
        want = base_digest(doc, f"{call}/{name}/k1")
        for k in R.N_STREAMS[1:]:
            assert base_digest(doc, f"{call}/{name}/k{k}") == want, (call, name, k, n)
