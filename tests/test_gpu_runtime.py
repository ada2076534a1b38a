"""GPU: process-level behaviour of libimk.so -- the one side-stream pool per device, the hardware-queue check a bare C-ABI caller
gets, the profiler's totals / marker hooks, and the data-parallel BatchNorm momentum reaching the plan on every rank."""
import ctypes
import json
import os
import socket
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_unet_and_evalnet_plans_share_the_side_stream_pool():
    """imk_net.h is compiled into two translation units; the pool must live in one (an IM++ process held two sets
    of side streams, one idle -- enough to put the weight gradients in line behind the main chain on 4 hardware queues)."""
    import torch
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd._lib import check, lib
    from inconsistencymasks_amd.evalnet import EvalNet
    from inconsistencymasks_amd.unet import UNet
    torch.cuda.set_device(0)
    u = UNet(32, 32, 3, 1, 0.5, "sigmoid", seed=1)
    e = EvalNet(64, 64, 3, 1, 1, 0.5, False, seed=2)
    got = []
    for m in (u, e):
        for i in (0, 1):
            s = ctypes.c_void_p()
            check(lib.imk_unet_plan_side_stream(m.plan.ptr, i, ctypes.byref(s)), "imk_unet_plan_side_stream")
            assert s.value
            got.append(s.value)
    assert got[0] == got[2] and got[1] == got[3] and got[0] != got[1]
    # a process whose caller chose no queue count: the package exported GPU_MAX_HW_QUEUES=8 before the runtime started, so a side
    # stream raises no warning (a fresh child -- this one's count is whatever the environment running the suite chose)
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    r = subprocess.run([sys.executable, "-c", CHILD_PACKAGE_HWQ, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "WARN 0 8", r.stdout + r.stderr


CHILD_PACKAGE_HWQ = textwrap.dedent("""
    import ctypes, sys
    sys.path.insert(0, sys.argv[1])
    import inconsistencymasks_amd, os
    import torch
    from inconsistencymasks_amd._lib import check, lib
    from inconsistencymasks_amd.unet import UNet
    torch.cuda.set_device(0)
    u = UNet(32, 32, 3, 1, 0.5, "sigmoid", seed=1)
    s = ctypes.c_void_p()
    check(lib.imk_unet_plan_side_stream(u.plan.ptr, 0, ctypes.byref(s)), "imk_unet_plan_side_stream")
    assert s.value
    print("WARN", lib.imk_runtime_warnings(), os.environ["GPU_MAX_HW_QUEUES"])
""")


CHILD_HWQ = textwrap.dedent("""
    import ctypes, os, sys
    import torch                                  # torch's HIP runtime first (see _lib.py), WITHOUT importing the package
    lib = ctypes.CDLL(os.path.join(sys.argv[1], "inconsistencymasks_amd", "libimk.so"))
    class Cfg(ctypes.Structure):
        _fields_ = [("h", ctypes.c_int), ("w", ctypes.c_int), ("c_in", ctypes.c_int), ("n_out", ctypes.c_int),
                    ("ch", ctypes.c_int * 5), ("act_out", ctypes.c_int)]
    cfg = Cfg(32, 32, 3, 1, (ctypes.c_int * 5)(8, 16, 32, 64, 128), 0)
    plan = ctypes.c_void_p()
    assert lib.imk_unet_plan_create(ctypes.byref(cfg), ctypes.byref(plan)) == 0
    torch.zeros(1, device="cuda")
    before = lib.imk_runtime_warnings()
    s = ctypes.c_void_p()
    assert lib.imk_unet_plan_side_stream(plan, 0, ctypes.byref(s)) == 0 and s.value
    print("WARN", before, lib.imk_runtime_warnings())
""")


@pytest.mark.parametrize("queues,expect", [(None, 1), ("4", 1), ("8", 0)])
def test_hw_queue_check_tells_a_bare_c_abi_caller(tmp_path, queues, expect):
    """A caller that binds libimk.so without the Python package and asks for a side stream with fewer than 8
    hardware queues is told: the IMK_WARN_HW_QUEUES bit and one line on stderr."""
    script = tmp_path / "c.py"
    script.write_text(CHILD_HWQ)
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    if queues:
        env["GPU_MAX_HW_QUEUES"] = queues
    r = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    before, after = [int(v) for v in r.stdout.strip().splitlines()[-1].split()[1:]]
    assert before == 0 and after == expect
    assert ("GPU_MAX_HW_QUEUES" in r.stderr) == bool(expect)


def test_profiler_totals_marker_and_unbind():
    import torch
    sys.path.insert(0, ROOT)
    from inconsistencymasks_amd._lib import lib
    from inconsistencymasks_amd.prof import Profiler
    from inconsistencymasks_amd.unet import UNet
    torch.cuda.set_device(0)
    m = UNet(64, 64, 3, 1, 0.5, "sigmoid", seed=1)
    x = torch.randint(0, 256, (4, 64, 64, 3), dtype=torch.uint8, device="cuda")
    old = Profiler(0)
    pr = Profiler(0)             # binds itself: `old` is no longer the bound context
    old.close()                  # must NOT unbind `pr`
    pr.totals(True)
    Profiler.mark(1)
    for _ in range(3):
        m.predict_device(x)
    Profiler.mark(2)
    torch.cuda.synchronize()
    t = pr.totals_dump()
    pipe = {k: v for k, v in t.items() if k.startswith("conv_pipe_kernel<")}
    assert pipe and all(v["launches"] % 3 == 0 and v["bytes"] > 0 for v in pipe.values()), t
    assert any(k.endswith(", 0, 1>") for k in pipe) or len(pipe) >= 2        # template arguments spelled as rocprofv3 prints them
    # round 6: EVERY launch is counted under its own kernel name (resolved from the launched function), priced or not
    assert t["imk_mark_kernel"] == {"launches": 2, "bytes": 0.0, "flops": 0.0}, t
    assert not any("(" in k or k.startswith("void ") or "anonymous" in k for k in t), list(t)
    heads = {k: v for k, v in t.items() if k.startswith("head_")}
    assert heads and all(v["launches"] == 3 and v["bytes"] > 0 for v in heads.values()), t
    m.train_step(x, (torch.rand((4, 64, 64, 1), device="cuda") > 0.5).to(torch.uint8), 0, 3e-3, 1e-4)
    torch.cuda.synchronize()
    t = pr.totals_dump()
    for name in ("wgf_stage1_kernel", "wgf_stage2_kernel", "adamw_kernel", "bn_bwd_coef_kernel"):
        assert t[name]["launches"] >= 1 and t[name]["bytes"] > 0, (name, t.get(name))
    pr.totals(False)
    assert pr.totals_dump() == {}
    assert lib.imk_prof_unbind(pr._p) == 1 and lib.imk_prof_unbind(pr._p) == 0
    pr.close()


WORKER_DP = textwrap.dedent("""
    import json, os, sys
    sys.path.insert(0, sys.argv[1])
    import torch, torch.distributed as dist
    torch.cuda.set_device(0)                                   # two ranks time-slicing one GPU
    dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    from inconsistencymasks_amd import functions as F
    from inconsistencymasks_amd.unet import UNet
    m = UNet(32, 32, 3, 1, 0.5, "sigmoid", seed=3)
    x = torch.randint(0, 256, (8, 32, 32, 3), dtype=torch.uint8, device="cuda")
    y = (torch.rand((8, 32, 32, 1), device="cuda") > 0.5).to(torch.uint8)
    class L:
        def next_batch(self): return x, y
    before = m.get_bn_momentum()
    F.fit(m, L(), 2, 1, 0)
    with open(os.path.join(sys.argv[2], f"rank{dist.get_rank()}.json"), "w") as f:      # (two ranks share one stdout: lines can interleave)
        json.dump({"rank": dist.get_rank(), "before": before, "after": m.get_bn_momentum(), "rule": F.dp_bn_momentum_rule()[0],
                   "moving": float(m.params[m.plan.n_trainable:].double().sum())}, f)
    dist.destroy_process_group()
""")


@pytest.mark.parametrize("mode,expect", [(None, 0.99), ("scaled", 0.99 ** 2)])
def test_dp_bn_momentum_reaches_the_plan_on_every_rank(tmp_path, mode, expect):
    """fit() under a 2-rank process group: the library's plan trains with Keras' 0.99 on BOTH ranks by default (the reference's
    recipe at any world size: ADVICE round 4), with 0.99^2 under IMK_DP_BN_MOMENTUM=scaled."""
    script = tmp_path / "w.py"
    script.write_text(WORKER_DP)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k != "IMK_DP_BN_MOMENTUM"}
    env.update(IMK_DIST_BACKEND="gloo", IMK_ONE_GPU="1", MASTER_ADDR="127.0.0.1")
    if mode:
        env["IMK_DP_BN_MOMENTUM"] = mode
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script), ROOT, str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    outs = [json.load(open(tmp_path / f"rank{k}.json")) for k in (0, 1)]
    assert sorted(o["rank"] for o in outs) == [0, 1]
    for o in outs:
        assert abs(o["before"] - 0.99) < 1e-7 and abs(o["after"] - expect) < 1e-6, o
        assert o["rule"] == ("scaled" if mode else "reference")
    assert outs[0]["moving"] == outs[1]["moving"]              # moving statistics averaged over the replicas at the epoch's end
