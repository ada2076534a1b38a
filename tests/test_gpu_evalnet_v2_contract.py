"""The C ABI's buffer and stream contracts (include/imk.h) for the imk_evalnet_* calls on a late-fusion plan
(imk_evalnet_v2_plan_create): inside tests/arena.py's guard bands under its three poison fills (0x00 / 0xFF / 0x3C), results bit-exact
across the fills and against the Python wrappers, a workspace one byte short refused with nothing written -- forward, fwd_bwd (two
consecutive steps), forward_candidates and forward_select; and imk_evalnet_fwd_bwd under tests/stream_skew.py's skewed streams (the
caller's stream, side stream 0, side stream 1, both side streams held), bit-exact against the unskewed run and against
debug(single_stream).  Both helper modules are imported as they are; the small helpers are tests/test_gpu_buffer_contract.py's and the
pattern is tests/test_gpu_dice_contract.py's."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import arena as A  # noqa: E402
import evalnet_v2_cases as V  # noqa: E402
import stream_skew as SK  # noqa: E402
import test_gpu_buffer_contract as BC  # noqa: E402  (Arena ordering, refused, same, model_specs, ptr_arrays)

L, S, dev = BC.L, BC.S, BC.dev
NAMES = ["hela", "odd"]
EB = 2


def net(name, seed=21, train=False):
    from inconsistencymasks_amd.evalnet import get_evalnet_miou_v2
    cfg = V.CASES[name]
    key = ("evalnet_v2", name, seed)
    if train or key not in BC._CACHE:
        m = get_evalnet_miou_v2(cfg["h"], cfg["w"], cfg["ca"], cfg["cb"], cfg["alpha"], seed=seed, onehot_B=cfg.get("onehot", False))
        m.load_state_dict(BC.randomize_bn(m.state_dict(), seed + 1))
        m.repack()
        if train:
            m.init_train_state()
            torch.cuda.synchronize()
            return m, cfg
        BC._CACHE[key] = m
    return BC._CACHE[key], cfg


def inputs(cfg, b, m_cand=None, seed=0):
    """xa [B,H,W,ca], xb [B,(M,)H,W,cb] or class ids [B,(M,)H,W,1], y [B,2*cb]"""
    rng = np.random.default_rng(seed + cfg["h"] + b)
    lead = (b,) if m_cand is None else (b, m_cand)
    xa = rng.integers(0, 256, (b, cfg["h"], cfg["w"], cfg["ca"]), dtype=np.uint8)
    if cfg.get("onehot"):
        xb = rng.integers(0, cfg["cb"], lead + (cfg["h"], cfg["w"], 1), dtype=np.uint8)
    else:
        xb = (rng.integers(0, 2, lead + (cfg["h"], cfg["w"], cfg["cb"]), dtype=np.uint8) * 255).astype(np.uint8)
    y = rng.random((b, 2 * cfg["cb"])).astype(np.float32)
    y[:, cfg["cb"]:] = y[:, cfg["cb"]:] > 0.5
    return dev(xa), dev(xb), dev(y)


def settle(m, xa, xb, y):
    """dynamic loss scaling as in training: a pass that overflows is followed by its (skipped) optimizer step, which halves the loss
    scale and leaves the weights alone -- until a pass on these inputs is finite.  What the tests then compare are finite gradients."""
    for _ in range(14):
        m.fwd_bwd(xa, xb, y)
        if float(m.stats[1]) == 0.0:
            break
        before = m.params[:m.plan.n_trainable].clone()
        m.adamw_step(3e-3, 1e-4)
        assert torch.equal(before, m.params[:m.plan.n_trainable])
    assert float(m.stats[1]) == 0.0, "no finite pass within 14 halvings of the loss scale"
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", NAMES)
def test_forward(name):
    m, cfg = net(name)
    xa, xb, _ = inputs(cfg, EB)
    u = 2 * m.plan.n_out
    n = m.plan.workspace_bytes(EB, 0)

    def arena(ws_bytes):
        return BC.Arena([("params", m.params, "in"), ("packed", m.packed, "in"), ("xa", xa, "in"), ("xb", xb, "in"),
                         ("out", EB * u * 4, "out"), ("ws", ws_bytes, "scratch")], "cuda")

    def call(ws_bytes):
        return lambda p: L().imk_evalnet_forward(m.plan.ptr, p["params"], p["packed"], p["xa"], p["xb"], EB, p["out"], p["ws"], ws_bytes, S())
    out = arena(n).check(call(n))
    BC.same(out["out"], m.predict_device(xa, xb), "out")
    BC.refused(arena(n - 1), call(n - 1))


@pytest.mark.parametrize("name", NAMES)
def test_fwd_bwd_two_steps(name):
    m, cfg = net(name, seed=31, train=True)
    xa, xb, y = inputs(cfg, EB, seed=3)
    settle(m, xa, xb, y)
    u, nt = 2 * m.plan.n_out, m.plan.n_trainable
    n = m.plan.workspace_bytes(EB, 1)
    params0 = m.params.clone()

    def arena(ws_bytes):
        return BC.Arena([("params", params0, "inout"), ("packed", m.packed, "inout"), ("state", m.train_state, "inout"), ("xa", xa, "in"),
                         ("xb", xb, "in"), ("y", y, "in"), ("out", EB * u * 4, "out"), ("grads", nt * 4, "out"), ("stats", 32, "out"),
                         ("ws", ws_bytes, "scratch")], "cuda")

    def step(ws_bytes):
        def call(p):
            for _ in range(2):      # the second step sees the first one's workspace as its stale content
                rc = L().imk_evalnet_fwd_bwd(m.plan.ptr, p["params"], p["packed"], p["state"], p["xa"], p["xb"], p["y"], EB, p["out"],
                                             p["grads"], p["stats"], p["ws"], ws_bytes, S())
                if rc:
                    return rc
            return 0
        return call
    out = arena(n).check(step(n), ranges={"stats": (0, 4 * 6)})      # include/imk.h: six values of stats are defined
    assert torch.equal(out["params"][:nt * 4], A.as_bytes(params0)[:nt * 4]), "imk_evalnet_fwd_bwd changed a trainable parameter"
    assert not torch.equal(out["params"][nt * 4:], A.as_bytes(params0)[nt * 4:]), "the moving statistics did not move"
    BC.refused(arena(n - 1), step(n - 1))
    m.fwd_bwd(xa, xb, y)
    w_out = m.fwd_bwd(xa, xb, y)
    torch.cuda.synchronize()
    BC.same(out["out"], w_out, "out")
    BC.same(out["grads"], m.grads, "grads")
    BC.same(out["stats"], m.stats[:6], "stats")
    BC.same(out["params"], m.params, "params")
    BC.same(out["state"], m.train_state, "state")
    assert float(m.stats[1]) == 0.0 and int((m.grads != 0).sum()) > nt // 2


@pytest.mark.parametrize("name", NAMES)
def test_forward_candidates_and_select(name):
    from inconsistencymasks_amd import evalnet as EV
    models = [net(name, seed=21 + 9 * j)[0] for j in range(2)]
    cfg = V.CASES[name]
    plan, mc, n = models[0].plan, 3, len(models)
    xa, xb, _ = inputs(cfg, EB, mc, seed=5)
    if cfg.get("onehot"):
        xb = xb[..., 0].contiguous()
    u = 2 * plan.n_out
    cand_bytes = cfg["h"] * cfg["w"]
    cand = dev(np.random.default_rng(8).integers(0, 256, (EB, mc, cand_bytes), dtype=np.uint8))
    nws = L().imk_evalnet_forward_candidates_workspace_bytes(plan.ptr, EB, mc)
    assert nws == plan.workspace_bytes(EB * mc, 0)      # one model's activations at batch B*M: the shared tower needs nothing more
    scorer = EV.CandidateScorer(models)
    w_scores = scorer.scores(xa, xb)
    torch.cuda.synchronize()
    thr = float(w_scores.mean(0)[..., :plan.n_out].mean())

    def arena(ws_bytes, select):
        specs = BC.model_specs(models) + [("xa", xa, "in"), ("xb", xb, "in")]
        if select:
            specs += [("cand", cand, "in")]
        specs += [("scores", n * EB * mc * u * 4, "out")]
        if select:
            specs += [("best_idx", EB * 4, "out"), ("best_score", EB * 4, "out"), ("keep", EB, "out"), ("chosen", EB * cand_bytes, "out")]
        return BC.Arena(specs + [("ws", ws_bytes, "scratch")], "cuda")

    def call_cand(ws_bytes):
        def call(p):
            pa, pk = BC.ptr_arrays(p, n)
            return L().imk_evalnet_forward_candidates(plan.ptr, n, pa, pk, p["xa"], p["xb"], EB, mc, p["scores"], p["ws"], ws_bytes, S())
        return call

    def call_sel(ws_bytes, mode):
        def call(p):
            pa, pk = BC.ptr_arrays(p, n)
            return L().imk_evalnet_forward_select(plan.ptr, n, pa, pk, p["xa"], p["xb"], EB, mc, None, p["cand"], cand_bytes, thr, mode,
                                                  p["scores"], p["best_idx"], p["best_score"], p["keep"], p["chosen"], p["ws"], ws_bytes, S())
        return call
    out = arena(nws, False).check(call_cand(nws))
    BC.same(out["scores"], w_scores, "scores")
    BC.refused(arena(nws - 1, False), call_cand(nws - 1))
    for mode in (EV.SELECT_MIOU, EV.SELECT_CONF_GATED):
        out = arena(nws, True).check(call_sel(nws, mode))
        bi, bs, keep, chosen = scorer.run(xa, xb, cand, thr, None, mode)
        torch.cuda.synchronize()
        for key, want in (("scores", scorer.last_scores), ("best_idx", bi), ("best_score", bs), ("keep", keep), ("chosen", chosen)):
            BC.same(out[key], want, f"mode {mode}: {key}")
    BC.refused(arena(nws - 1, True), call_sel(nws - 1, EV.SELECT_MIOU))


def test_fwd_bwd_under_skewed_streams():
    """both towers' last BatchNorm backward read ONE gradient buffer, the towers' weight gradients fork to the side streams block by block
    and the step joins them at its end: with the caller's stream or a side stream held while every buffer a premature reader could touch
    holds poison, outputs, gradients, statistics and moving statistics are the unskewed run's bit for bit, under both fills -- and so
    are they with no side stream at all"""
    name, b = "hela", 2
    m, cfg = net(name, seed=61, train=True)
    xa0, xb0, y0 = inputs(cfg, b, seed=7)
    nt = m.plan.n_trainable
    settle(m, xa0, xb0, y0)
    start, state0, packed0 = m.params.clone(), m.train_state.clone(), m.packed.clone()

    def restore():
        m.params.copy_(start), m.train_state.copy_(state0), m.packed.copy_(packed0)
        m._packed_ok, m._fold_ok = True, False
    restore()
    out0 = m.fwd_bwd(xa0, xb0, y0).clone()
    torch.cuda.synchronize()
    want = {"out": out0, "grads": m.grads.clone(), "stats": m.stats[:6].clone(), "moving": m.params[nt:].clone()}
    assert float(want["stats"][1]) == 0.0 and torch.isfinite(want["grads"]).all()

    restore()
    m.debug(single_stream=True)
    try:
        out1 = m.fwd_bwd(xa0, xb0, y0)
        torch.cuda.synchronize()
    finally:
        m.debug(single_stream=False)
    for key, got in (("out", out1), ("grads", m.grads), ("stats", m.stats[:6]), ("moving", m.params[nt:])):
        assert torch.equal(got, want[key]), f"single_stream: {key}"

    restore()
    sides = {"side0": SK.side_stream(m, 0), "side1": SK.side_stream(m, 1)}
    caller, beside = SK.caller_stream_beside(list(sides.values()))
    assert beside, "no caller stream off the side streams' hardware queues was found"
    xa, xb, y = torch.empty_like(xa0), torch.empty_like(xb0), torch.empty_like(y0)
    out = torch.empty_like(out0)
    inputs_ = {"xa": (xa, xa0), "xb": (xb, xb0), "y": (y, y0), "params": (m.params, start), "packed": (m.packed, packed0),
               "state": (m.train_state, state0)}
    outputs = {"out": out, "grads": m.grads, "stats": m.stats[:6], "moving": m.params[nt:]}
    ws = m.workspace(b, 1)

    def call():
        from inconsistencymasks_amd._lib import check
        check(L().imk_evalnet_fwd_bwd(m.plan.ptr, m.params.data_ptr(), m.packed.data_ptr(), m.train_state.data_ptr(), xa.data_ptr(),
                                      xb.data_ptr(), y.data_ptr(), b, out.data_ptr(), m.grads.data_ptr(), m.stats.data_ptr(),
                                      ws.data_ptr(), ws.numel(), S()), "imk_evalnet_fwd_bwd")
    hold_ms = SK.hold_ms_for(SK.wall_ms(call, inputs_, caller))
    digests = {}
    for skew in ((), ("main",), ("side0",), ("side1",), ("side0", "side1")):
        for fill in SK.FILLS:
            snaps = SK.run_skewed(call, inputs_, outputs, [ws, m.grads_and_stats, out], skew, caller, fill=fill, hold_ms=hold_ms, sides=sides)
            digests[("+".join(skew) or "none", f"{fill:02X}")] = SK.digest(snaps)
            if not skew:
                for key in outputs:
                    BC.same(snaps[key], want[key], f"unskewed, fill 0x{fill:02X}: {key}")
    assert len(set(digests.values())) == 1, digests
