"""The C ABI's buffer and stream contracts (include/imk.h) for the depth-map family's entry points: imk_im_depth, imk_eval_depth,
imk_unet_forward_im_depth and loss kinds 2 / 3 of imk_unet_fwd_bwd inside tests/arena.py's guard bands under its three poison fills,
and imk_unet_forward_im_depth under tests/stream_skew.py's skews.  Both helper modules are imported as they are; the shapes and small
helpers are tests/test_gpu_buffer_contract.py's.  Every comparison is bit-exact: across the fills, across the skews, and against the
Python wrappers (the product path)."""
import ctypes
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
import stream_skew as SK  # noqa: E402
import test_gpu_buffer_contract as BC  # noqa: E402  (Arena ordering, refused, same, cached models, images)
from inconsistencymasks_amd import depth as D  # noqa: E402

L, S, dev = BC.L, BC.S, BC.dev
DEPTH_CFG = (48, 80, 3, 1, 0.5, "sigmoid")      # BC.SHAPES[1]: the fused head's width (8 channels); H*W = 3840: a short last workgroup
WIDE_CFG = (32, 48, 3, 1, 2.0, "sigmoid")       # BC.SHAPES[4]: 32 channels


# ---- imk_im_depth ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,b,h,w", [(3, 2, 37, 51), (2, 3, 96, 96), (9, 1, 48, 80)])
def test_im_depth(n, b, h, w):
    rng = np.random.default_rng(n * h)
    preds = dev(rng.random((n, b, h, w), dtype=np.float32))
    img = dev(rng.integers(1, 256, (b, h, w, 3), dtype=np.uint8))
    want = D.im_depth(preds, 1.5, img, True, want_std=True)
    torch.cuda.synchronize()
    assert 0 < int(want["im_size"].sum()) < b * h * w
    nws = L().imk_im_depth_workspace_bytes(b, h, w)
    outs = [("img_out", img.numel(), "out"), ("im", b * h * w, "out"), ("im_size", b * 8, "out"), ("thr", b * 4, "out")]

    def arena(ws_bytes, with_std):
        return BC.Arena([("preds", preds, "in"), ("img", img, "in")] + outs + ([("std", b * h * w * 4, "out")] if with_std else []) +
                        [("ws", ws_bytes, "scratch")])

    def call(ws_bytes, with_std):
        return lambda p: L().imk_im_depth(p["preds"], n, b, h, w, 1.5, p["img"], 3, 1, p["img_out"], p["im"], p["im_size"], p["thr"],
                                          p["std"] if with_std else None, p["ws"], ws_bytes, S())
    for with_std in (True, False):
        out = arena(nws, with_std).check(call(nws, with_std))
        for key in ("img_out", "im", "im_size", "thr") + (("std",) if with_std else ()):
            BC.same(out[key], want[key], f"std_out {with_std}: {key}")
    BC.refused(arena(nws - 1, False), call(nws - 1, False))
    # with std_out given the workspace is not touched at all: one byte of it is enough, and it stays the fill
    ar = arena(1, True)
    snap = ar.run(0x3C, call(1, True))
    BC.same(snap["thr"], want["thr"], "one-byte workspace: thr")
    assert int(ar.view("ws")[0]) == 0x3C


# ---- imk_eval_depth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w", [(3, 37, 51), (2, 64, 64)])
def test_eval_depth(b, h, w):
    rng = np.random.default_rng(b * h)
    probs = dev(rng.random((b, h, w), dtype=np.float32))
    gt = dev(rng.integers(0, 256, (b, h, w), dtype=np.uint8))
    pred, sums = D.eval_depth(probs, gt)
    ar = BC.Arena([("probs", probs, "in"), ("gt", gt, "in"), ("pred", b * h * w, "out"), ("sums", b * 16, "out")])
    out = ar.check(lambda p: L().imk_eval_depth(p["probs"], p["gt"], b, h, w, p["pred"], p["sums"], S()))
    BC.same(out["pred"], pred, "pred")
    BC.same(out["sums"], torch.from_numpy(sums), "sums")
    ar = BC.Arena([("probs", probs, "in"), ("gt", gt, "in"), ("sums", b * 16, "out")])
    out = ar.check(lambda p: L().imk_eval_depth(p["probs"], p["gt"], b, h, w, None, p["sums"], S()))
    BC.same(out["sums"], torch.from_numpy(sums), "sums without pred_out")


# ---- loss kinds 2 and 3 of imk_unet_fwd_bwd -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("cfg,b", [(DEPTH_CFG, 3), (WIDE_CFG, 1)], ids=["a0.5-b3", "a2.0-b1"])
def test_fwd_bwd_two_steps(cfg, b, kind):
    """tests/test_gpu_buffer_contract.py::check_fwd_bwd with continuous targets and the new loss kinds (kind 3 adds a launch over grads
    and stats behind everything else)"""
    m = BC.fresh_trainee(cfg)
    x = BC.images(cfg, b, 1)
    y = dev(np.random.default_rng(b + kind).integers(0, 256, (b, cfg[0], cfg[1], 1), dtype=np.uint8))
    nt, n = m.plan.n_trainable, m.plan.workspace_bytes(b, 1)
    params0 = m.params.clone()

    def arena(ws_bytes):
        return BC.Arena([("params", params0, "inout"), ("packed", m.packed, "inout"), ("state", m.train_state, "inout"), ("x", x, "in"),
                         ("y", y, "in"), ("grads", nt * 4, "out"), ("stats", 16, "out"), ("ws", ws_bytes, "scratch")])

    def step(ws_bytes):
        def call(p):
            for _ in range(2):
                rc = L().imk_unet_fwd_bwd(m.plan.ptr, p["params"], p["packed"], p["state"], p["x"], p["y"], b, kind, p["grads"],
                                          p["stats"], p["ws"], ws_bytes, S())
                if rc:
                    return rc
            return 0
        return call
    out = arena(n).check(step(n), ranges={"stats": (0, 12)})           # stats[3] is reserved
    assert torch.equal(out["params"][:nt * 4], A.as_bytes(params0)[:nt * 4]), "imk_unet_fwd_bwd changed a trainable parameter"
    BC.refused(arena(n - 1), step(n - 1))
    m.fwd_bwd(x, y, kind)
    m.fwd_bwd(x, y, kind)
    torch.cuda.synchronize()
    BC.same(out["grads"], m.grads, "grads")
    BC.same(out["stats"], m.stats[:3], "stats[0:3]")
    BC.same(out["params"], m.params, "params")


# ---- imk_unet_forward_im_depth --------------------------------------------------------------------------------------------------------
def ensemble(cfg, n=3):
    return [BC.unet(cfg, seed=11 + 10 * j) for j in range(n)]


def depth_arena(models, x, b, ws_bytes, with_std=True):
    p = models[0].plan
    specs = BC.model_specs(models) + [("x", x, "in"), ("img_out", x.numel(), "out"), ("im", b * p.h * p.w, "out"), ("im_size", b * 8, "out"),
                                      ("thr", b * 4, "out")] + ([("std", b * p.h * p.w * 4, "out")] if with_std else [])
    return BC.Arena(specs + [("ws", ws_bytes, "scratch")])


def depth_call(models, b, ws_bytes, with_std=True):
    plan, n = models[0].plan, len(models)

    def call(p):
        pa, pk = BC.ptr_arrays(p, n)
        return L().imk_unet_forward_im_depth(plan.ptr, n, pa, pk, p["x"], b, 1.0, p["x"], 1, p["img_out"], p["im"], p["im_size"],
                                             p["thr"], p["std"] if with_std else None, p["ws"], ws_bytes, torch.cuda.current_stream().cuda_stream)
    return call


@pytest.mark.parametrize("n_streams", [1, 2, 3])
@pytest.mark.parametrize("cfg,b", [(DEPTH_CFG, 3), (WIDE_CFG, 1)], ids=["a0.5-b3", "a2.0-b1"])
def test_forward_im_depth(cfg, b, n_streams):
    models, x = ensemble(cfg), BC.images(cfg, b)
    plan = models[0].plan
    n = L().imk_unet_forward_im_depth_workspace_bytes(plan.ptr, 3, b, n_streams)
    keys = ("img_out", "im", "im_size", "thr", "std")
    def product_path():      # imk_unet_forward x N + imk_im_depth
        probs = torch.stack([m.predict_device(x) for m in models], 0)[..., 0].contiguous()
        r = D.im_depth(probs, 1.0, x, True, want_std=True)
        torch.cuda.synchronize()
        return r
    for route in ("fused", "unfused"):      # the product path under the same switch: it changes which conv kernels run as well
        for m in models:
            m.debug(materialize=route == "unfused")
        try:
            want = product_path()
            out = depth_arena(models, x, b, n).check(depth_call(models, b, n))
        finally:
            for m in models:
                m.debug(materialize=False)
        for key in keys:
            BC.same(out[key], want[key], f"{route} {key}")
    want = product_path()
    assert 0 < int(want["im_size"].sum()) < b * plan.h * plan.w
    out = depth_arena(models, x, b, n, False).check(depth_call(models, b, n, False))      # the map in the workspace
    for key in keys[:-1]:
        BC.same(out[key], want[key], f"std_out NULL: {key}")
    if n_streams == 1:
        map_bytes = BC.up256(b * plan.h * plan.w * 4)
        lo = map_bytes + BC.im_min_bytes(plan, 3, b)
        BC.refused(depth_arena(models, x, b, lo - 1), depth_call(models, b, lo - 1))
        if lo < n:       # the smaller workspace: the unfused route, with the guard right behind it
            out = depth_arena(models, x, b, lo).check(depth_call(models, b, lo))
            for key in keys:
                BC.same(out[key], want[key], f"small-workspace {key}")


def test_forward_im_depth_under_skewed_streams():
    """three models on three streams (the caller's and the pool's two side streams), each stream held in turn while every buffer a
    premature reader could touch holds poison: every output is bit-identical to the unskewed run, under both fills"""
    cfg, b = DEPTH_CFG, 3
    models, x0 = ensemble(cfg), BC.images(cfg, b)
    plan = models[0].plan
    nws = L().imk_unet_forward_im_depth_workspace_bytes(plan.ptr, 3, b, 3)
    probs = torch.stack([m.predict_device(x0) for m in models], 0)[..., 0].contiguous()
    want = D.im_depth(probs, 1.0, x0, True, want_std=True)
    torch.cuda.synchronize()
    sides = {f"side{i}": SK.side_stream(models[0], i) for i in range(2)}
    caller, beside = SK.caller_stream_beside(list(sides.values()))
    assert beside, "no caller stream off the side streams' hardware queues was found"
    x = torch.empty_like(x0)
    bufs = {"img_out": torch.empty_like(x0), "im": torch.empty((b, plan.h, plan.w), dtype=torch.uint8, device="cuda"),
            "im_size": torch.empty(b, dtype=torch.int64, device="cuda"), "thr": torch.empty(b, dtype=torch.float32, device="cuda"),
            "std": torch.empty((b, plan.h, plan.w), dtype=torch.float32, device="cuda")}
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    ptrs = {f"params{j}": m.params.data_ptr() for j, m in enumerate(models)}
    ptrs.update({f"packed{j}": m.packed.data_ptr() for j, m in enumerate(models)})
    ptrs.update({k: v.data_ptr() for k, v in bufs.items()})
    ptrs.update(x=x.data_ptr(), ws=ws.data_ptr())
    fn = depth_call(models, b, nws)

    def call():
        assert fn(ptrs) == 0
    inputs = {"x": (x, x0)}
    hold_ms = SK.hold_ms_for(SK.wall_ms(call, inputs, caller))
    digests = {}
    for skew in ((), ("main",), ("side0",), ("side1",), ("side0", "side1")):
        for fill in SK.FILLS:
            snaps = SK.run_skewed(call, inputs, bufs, [ws], skew, caller, fill=fill, hold_ms=hold_ms, sides=sides)
            digests[("+".join(skew) or "none", f"{fill:02X}")] = SK.digest(snaps)
            if not skew:
                for key in bufs:
                    BC.same(snaps[key], want[key], f"unskewed, fill 0x{fill:02X}: {key}")
    assert len(set(digests.values())) == 1, digests
