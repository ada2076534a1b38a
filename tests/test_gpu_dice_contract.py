"""The C ABI's buffer and stream contracts (include/imk.h) for loss kind 4 of imk_unet_fwd_bwd on both gradient routes and for
imk_eval_dice_sums: inside tests/arena.py's guard bands under its three poison fills, a workspace one byte short refused with nothing
written, and kind 4 under tests/stream_skew.py's skewed streams.  Both helper modules are imported as they are; the shapes and small
helpers are tests/test_gpu_buffer_contract.py's.  Every comparison is bit-exact: across the fills, across the skews, and against the
Python wrappers (the product path)."""
import os
import subprocess
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
import test_gpu_buffer_contract as BC  # noqa: E402  (Arena ordering, refused, same, fresh_trainee, images)
from inconsistencymasks_amd import evaluate as E  # noqa: E402

L, S, dev = BC.L, BC.S, BC.dev
FUSED_CFG = (48, 80, 3, 1, 0.5, "sigmoid")      # BC.SHAPES[1]: 8 channels, 1 map -- the fused variant; H*W = 3840: a short last workgroup
HELA_CFG = (48, 32, 1, 2, 1.75, "sigmoid")      # BC.SHAPES[3]: 28 channels padded to 32, 2 maps -- dice_dlogit_kernel + the head's dgrad
WIDE_CFG = (32, 48, 3, 1, 2.0, "sigmoid")       # BC.SHAPES[4]: 32 channels
CASES = [(FUSED_CFG, 3), (HELA_CFG, 3), (WIDE_CFG, 1)]
IDS = ["a0.5-b3", "a1.75k2-b3", "a2.0-b1"]


def targets(cfg, b):
    """every image its own foreground share; the last plane of a multi-map head is 0 / 3 (HeLa's position plane)"""
    rng = np.random.default_rng(cfg[0] + b)
    y = np.stack([(rng.random((cfg[0], cfg[1], cfg[3])) < s).astype(np.uint8) for s in (0.05, 0.5, 0.95)[:b]], 0)
    if cfg[3] > 1:
        y[..., -1] *= 3
    return dev(y)


def check_fwd_bwd_kind4(cfg, b):
    """tests/test_gpu_buffer_contract.py::check_fwd_bwd with loss kind 4: two consecutive steps inside one arena run, the second sees the
    first one's workspace (partial rows, coefficients) as its stale content"""
    m = BC.fresh_trainee(cfg)
    x, y = BC.images(cfg, b, 1), targets(cfg, b)
    nt, n = m.plan.n_trainable, m.plan.workspace_bytes(b, 1)
    params0 = m.params.clone()

    def arena(ws_bytes):
        return BC.Arena([("params", params0, "inout"), ("packed", m.packed, "inout"), ("state", m.train_state, "inout"), ("x", x, "in"),
                         ("y", y, "in"), ("grads", nt * 4, "out"), ("stats", 16, "out"), ("ws", ws_bytes, "scratch")])

    def step(ws_bytes):
        def call(p):
            for _ in range(2):
                rc = L().imk_unet_fwd_bwd(m.plan.ptr, p["params"], p["packed"], p["state"], p["x"], p["y"], b, 4, p["grads"],
                                          p["stats"], p["ws"], ws_bytes, S())
                if rc:
                    return rc
            return 0
        return call
    out = arena(n).check(step(n), ranges={"stats": (0, 12)})           # stats[3] is reserved
    assert torch.equal(out["params"][:nt * 4], A.as_bytes(params0)[:nt * 4]), "imk_unet_fwd_bwd changed a trainable parameter"
    assert not torch.equal(out["params"][nt * 4:], A.as_bytes(params0)[nt * 4:]), "the moving statistics did not move"
    BC.refused(arena(n - 1), step(n - 1))
    m.fwd_bwd(x, y, 4)
    m.fwd_bwd(x, y, 4)
    torch.cuda.synchronize()
    BC.same(out["grads"], m.grads, "grads")
    BC.same(out["stats"], m.stats[:3], "stats[0:3]")
    BC.same(out["params"], m.params, "params")
    BC.same(out["state"], m.train_state, "state")
    BC.same(out["packed"], m.packed, "packed")
    loss = float(m.stats[0])
    assert 0.0 < loss < 1.0 and int((m.grads != 0).sum()) > nt // 2, loss
    return out


@pytest.mark.parametrize("cfg,b", CASES, ids=IDS)
def test_fwd_bwd_kind4_two_steps(cfg, b):
    assert os.environ.get("IMK_DICE_FUSED", "1") != "0", "this process must run the default routes"
    check_fwd_bwd_kind4(cfg, b)


def test_fwd_bwd_kind4_composed_route_of_the_fused_shape(tmp_path):
    """IMK_DICE_FUSED=0 is read once per process: the same arena check in a child; its loss is this process's bit for bit (the sums and
    coefficient launches are shared), its gradients are not (another dgrad)"""
    child = ("import sys, torch\n"
             "sys.path[:0] = [%r, %r]\n"
             "import test_gpu_dice_contract as T\n"
             "out = T.check_fwd_bwd_kind4(T.FUSED_CFG, 3)\n"
             "torch.save({k: out[k].cpu() for k in ('grads', 'stats')}, sys.argv[1])\n") % (ROOT, HERE)
    path = str(tmp_path / "composed.pt")
    r = subprocess.run([sys.executable, "-c", child, path], env=dict(os.environ, IMK_DICE_FUSED="0"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    composed = torch.load(path)
    fused = check_fwd_bwd_kind4(FUSED_CFG, 3)
    assert torch.equal(fused["stats"].cpu(), composed["stats"])
    assert not torch.equal(fused["grads"].cpu(), composed["grads"]), "this process did not take the fused route"


@pytest.mark.parametrize("b,h,w,k", [(3, 37, 51, 1), (5, 16, 16, 3), (1, 64, 48, 2)])
def test_eval_dice_sums(b, h, w, k):
    rng = np.random.default_rng(b * h + k)
    probs = dev(rng.random((b, h, w, k), dtype=np.float32))
    gt = dev(rng.integers(0, 4, (b, h, w, k), dtype=np.uint8))
    want = E.dice_sums(probs, gt)
    ar = BC.Arena([("probs", probs, "in"), ("gt", gt, "in"), ("out", b * 3 * 8, "out")])
    out = ar.check(lambda p: L().imk_eval_dice_sums(p["probs"], p["gt"], b, h, w, k, p["out"], S()))
    BC.same(out["out"], torch.from_numpy(want), "sums")


def test_fwd_bwd_kind4_under_skewed_streams():
    """the three head launches run in order on the caller's stream and the weight-gradient forks stay what they are: with the caller's
    stream or the side stream held while every buffer a premature reader could touch holds poison, gradients, statistics and moving
    statistics are bit-identical to the unskewed run, under both fills, on the fused and on the composed shape"""
    for cfg, b in ((FUSED_CFG, 3), (WIDE_CFG, 2)):
        m = BC.fresh_trainee(cfg)
        x0, y0 = BC.images(cfg, b, 1), targets(cfg, b)
        nt = m.plan.n_trainable
        m.fwd_bwd(x0, y0, 4)
        torch.cuda.synchronize()
        want = {"grads": m.grads.clone(), "stats": m.stats[:3].clone(), "moving": m.params[nt:].clone()}
        m = BC.fresh_trainee(cfg)
        sides = {"side0": SK.side_stream(m, 0)}
        caller, beside = SK.caller_stream_beside(list(sides.values()))
        assert beside, "no caller stream off the side stream's hardware queue was found"
        x, y = torch.empty_like(x0), torch.empty_like(y0)
        inputs = {"x": (x, x0), "y": (y, y0), "params": (m.params, m.params.clone()), "packed": (m.packed, m.packed.clone()),
                  "state": (m.train_state, m.train_state.clone())}
        outputs = {"grads": m.grads, "stats": m.stats[:3], "moving": m.params[nt:]}
        ws = m.workspace(b, 1)

        def call():
            m._packed_ok, m._fold_ok = True, False      # the device state was restored to the packed weights of `params`
            m.fwd_bwd(x, y, 4)
        hold_ms = SK.hold_ms_for(SK.wall_ms(call, inputs, caller))
        digests = {}
        for skew in ((), ("main",), ("side0",)):
            for fill in SK.FILLS:
                snaps = SK.run_skewed(call, inputs, outputs, [ws, m.grads_and_stats], skew, caller, fill=fill, hold_ms=hold_ms, sides=sides)
                digests[("+".join(skew) or "none", f"{fill:02X}")] = SK.digest(snaps)
                if not skew:
                    for key in outputs:
                        BC.same(snaps[key], want[key], f"{cfg}: unskewed, fill 0x{fill:02X}: {key}")
        assert len(set(digests.values())) == 1, (cfg, digests)
