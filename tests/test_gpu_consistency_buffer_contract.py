"""The C ABI's buffer contract (include/imk.h, "Buffers") for imk_unet_consistency_fwd_bwd, with the guard bands and poison fills of
tests/arena.py: nothing outside the arguments is written, the inputs stay as they are, every output byte is written and none depends
on what the workspace or the outputs held (bit-exact across the three fills), the result is bit for bit the Python wrapper's, and a
workspace one byte short is refused with nothing written.  Both routes: the default one here, IMK_CONSISTENCY_FUSED=0 in a child.
"""
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import arena as A  # noqa: E402
import consistency_cases as C  # noqa: E402

IMK_EWORKSPACE = -3


def L():
    from inconsistencymasks_amd._lib import lib
    return lib


def S():
    return torch.cuda.current_stream().cuda_stream


def same(snap, want, what):
    w = A.as_bytes(want).to(snap.device)
    assert snap.numel() == w.numel(), (what, snap.numel(), w.numel())
    if not torch.equal(snap, w):
        d = torch.nonzero(snap != w)[:, 0]
        raise AssertionError(f"{what}: {d.numel()} byte(s) differ from the wrapper path, first at +{int(d[0])}")


def check_consistency(name):
    """two consecutive calls inside one arena run: the second sees the first one's workspace as its stale content"""
    from inconsistencymasks_amd.unet import UNet
    cfg = C.CASES[name]
    b = cfg["b"]
    m = UNet(cfg["h"], cfg["w"], cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], seed=3)
    m.load_state_dict(C.randomize_bn(m.state_dict(), 4))
    m.repack()
    m.init_train_state()
    v1, v2 = C.make_views(cfg, 5)
    x1, x2 = torch.from_numpy(v1).cuda(), torch.from_numpy(v2).cuda()
    torch.cuda.synchronize()
    nt = m.plan.n_trainable
    n = L().imk_unet_consistency_workspace_bytes(m.plan.ptr, b)
    assert n >= 2 * m.plan.workspace_bytes(b, 1) + 4 * nt
    params0 = m.params.clone()

    def arena(ws_bytes):
        # the workspace first, then the outputs, the inputs last (tests/test_gpu_buffer_contract.py::Arena)
        return A.Arena([("ws", ws_bytes, "scratch"), ("grads", nt * 4, "out"), ("stats", 16, "out"), ("params", params0, "inout"),
                        ("packed", m.packed, "inout"), ("state", m.train_state, "inout"), ("x1", x1, "in"), ("x2", x2, "in")], "cuda")

    def step(ws_bytes):
        def call(p):
            for _ in range(2):
                rc = L().imk_unet_consistency_fwd_bwd(m.plan.ptr, p["params"], p["packed"], p["state"], p["x1"], p["x2"], b, p["grads"],
                                                      p["stats"], p["ws"], ws_bytes, S())
                if rc:
                    return rc
            return 0
        return call
    out = arena(n).check(step(n), ranges={"stats": (0, 12)})           # stats[3] is reserved
    assert torch.equal(out["params"][:nt * 4], A.as_bytes(params0)[:nt * 4]), "a trainable parameter changed"
    assert not torch.equal(out["params"][nt * 4:], A.as_bytes(params0)[nt * 4:]), "the moving statistics did not move"
    arena(n - 1).run(0x3C, step(n - 1), want_rc=IMK_EWORKSPACE, untouched=True)
    m.consistency_fwd_bwd(x1, x2)
    m.consistency_fwd_bwd(x1, x2)
    torch.cuda.synchronize()
    same(out["grads"], m.grads, "grads")
    same(out["stats"], m.stats[:3], "stats[0:3]")
    same(out["params"], m.params, "params")
    same(out["state"], m.train_state, "state")
    same(out["packed"], m.packed, "packed")


@pytest.mark.parametrize("name", list(C.CASES))
def test_consistency_fwd_bwd_two_calls(name):
    assert os.environ.get("IMK_CONSISTENCY_FUSED", "1") != "0", "this process must run the default routes"
    check_consistency(name)


def test_composed_route_in_a_child_process():
    """IMK_CONSISTENCY_FUSED=0 is read once per process: the same checks in a child, for the cases the fused kernel takes"""
    env = {**os.environ, "IMK_CONSISTENCY_FUSED": "0"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "composed"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "composed ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


if __name__ == "__main__":
    assert sys.argv[1:] == ["composed"] and os.environ.get("IMK_CONSISTENCY_FUSED") == "0"
    for case in C.FUSED:
        check_consistency(case)
    print("composed ok")
