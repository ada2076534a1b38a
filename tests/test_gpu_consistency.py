"""The consistency-loss training step (imk_unet_consistency_fwd_bwd, csrc/imk_consist.hip) on the GPU against the torch-CPU oracle
composed in tests/consistency_cases.py, on both routes (the fused two-view head kernel; head_kernel x 2 -> consistency_dlogit_kernel
-> the labelled step's head dgrad), and the step's structural properties.

Bounds:
  * loss: 1e-4 relative, the labelled step's bound (tests/test_gpu_unet.py);
  * moving statistics after the step: 1e-5 of two sequential momentum updates, view 1 first;
  * every gradient tensor, with the oracle's forward values pinned to each view's stored tensors: rel-L2 <= max(2e-2, 1.5 x d),
    d = the distance between the oracle's fp16-emulating and fp32 forms of the same gradient on the same pins (the gradient is a sum
    of two contributions that partly cancel, so the labelled step's 2e-2 cannot simply be assumed; tests/test_cpu_consistency_yardstick.py
    checks d itself).  The distances measured on the MI355X are recorded in tests/measured/consistency_grad_gap.json.
  * fused against composed: both meet the bounds, loss equal within 1e-6 relative; no bit-identity between the routes.
"""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import consistency_cases as C  # noqa: E402

_RUNS, _REFS = {}, {}


def build_model(name, seed=C.MODEL_SEED):
    from inconsistencymasks_amd.unet import UNet
    cfg = C.CASES[name]
    m = UNet(cfg["h"], cfg["w"], cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], seed=seed)
    sd = C.randomize_bn(m.state_dict(), C.BN_SEED)
    m.load_state_dict(sd)
    return m, sd


def views(name, seed=C.INPUT_SEED):
    v1, v2 = C.make_views(C.CASES[name], seed)
    return v1, v2, torch.from_numpy(v1).cuda(), torch.from_numpy(v2).cuda()


def run_case(name):
    """one consistency forward/backward of the case on this process's route -> everything the checks read (numpy)"""
    cfg = C.CASES[name]
    m, sd = build_model(name)
    v1, v2, d1, d2 = views(name)
    m.init_train_state()
    for attempt in range(12):   # dynamic loss scaling: an overflowing step is skipped and the scale halved
        m.consistency_fwd_bwd(d1, d2)
        torch.cuda.synchronize()
        stats = m.stats.cpu().numpy().copy()
        assert stats[2] == 32768.0 / 2 ** attempt
        if stats[1] == 0.0:
            break
        before = m.params.clone()
        m.adamw_step(3e-3, 1e-4)
        assert torch.equal(before, m.params)
        m.load_state_dict(sd)
    assert stats[1] == 0.0
    g1 = m.grads.clone()
    moving = {k: v.numpy() for k, v in m.state_dict().items() if k.endswith(".mean") or k.endswith(".var")}
    m.consistency_fwd_bwd(d1, d2)          # a second call from the same trainable state: bit-identical gradients
    torch.cuda.synchronize()
    assert torch.equal(g1, m.grads), "the consistency step is not bit-reproducible"
    assert m.stats.cpu().numpy()[0] == stats[0]
    out = {"stats": stats, "grads": g1.cpu().numpy()}
    for k, v in moving.items():
        out["moving/" + k] = v
    for view in (0, 1):
        for l in m.plan.layers:
            if l["kind"] == 0 and l["name"] != "out":
                out[f"ov{view}/" + l["name"]] = m.intermediate(l["name"], cfg["b"], 1, view=view).numpy()
    out["layers"] = np.array([(l["name"], l["kind"], l["ksize"], l["cin"], l["cout"], l["off_w"], l["off_b"]) for l in m.plan.layers], dtype=object)
    return out


def run_of(name):
    if name not in _RUNS:
        _RUNS[name] = run_case(name)
    return _RUNS[name]


def reference_of(name, run):
    """the oracle on the pins of `run`, computed once per case and left unchanged"""
    if name not in _REFS:
        cfg = C.CASES[name]
        _, sd = build_model(name)
        v1, v2 = C.make_views(cfg)
        ov = [{k.split("/", 1)[1]: torch.from_numpy(v) for k, v in run.items() if k.startswith(f"ov{view}/")} for view in (0, 1)]
        _REFS[name] = C.yardstick(sd, v1, v2, cfg, ov[0], ov[1], loss_scale=float(run["stats"][2]))
    return _REFS[name]


def grad_errors(run, g_ref):
    g, errs = run["grads"], {}
    for name, kind, ks, ci, co, off_w, off_b in run["layers"]:
        if kind == 0:
            errs[name + ".w"] = C.rel_l2(g[off_w:off_w + ks * ks * ci * co].reshape(ks, ks, ci, co), g_ref[name + ".w"].numpy())
            errs[name + ".b"] = C.rel_l2(g[off_b:off_b + co], g_ref[name + ".b"].numpy())
        else:
            errs[name + ".gamma"] = C.rel_l2(g[off_w:off_w + co], g_ref[name + ".gamma"].numpy())
            errs[name + ".beta"] = C.rel_l2(g[off_b:off_b + co], g_ref[name + ".beta"].numpy())
    return errs


def check_against_oracle(name, run, route):
    loss_ref, g_ref, moving_ref, dist, _ = reference_of(name, run)
    stats = run["stats"]
    print(f"{name} ({route}): loss {stats[0]:.6g} oracle {loss_ref:.6g} rel {abs(stats[0] - loss_ref) / abs(loss_ref):.2g}")
    errs = grad_errors(run, g_ref)
    worst = max(errs, key=lambda k: errs[k] / C.grad_bound(dist[k]))
    print(f"{name} ({route}): gradient rel-L2 max {max(errs.values()):.3g}; closest to its bound: {worst} {errs[worst]:.3g} of "
          f"{C.grad_bound(dist[worst]):.3g} (yardstick {dist[worst]:.3g}); GPU_GAP {name} {route} "
          f"{ {k: float('%.3g' % v) for k, v in errs.items()} }")
    assert abs(stats[0] - loss_ref) <= 1e-4 * abs(loss_ref)
    for k, v in moving_ref.items():
        assert np.allclose(run["moving/" + k], v.numpy(), atol=1e-5, rtol=1e-5), k
    bad = {k: (round(v, 4), round(C.grad_bound(dist[k]), 4)) for k, v in errs.items() if not v <= C.grad_bound(dist[k])}
    assert not bad, f"{name} ({route}): gradient tensors beyond max(2e-2, 1.5 x yardstick) (rel-L2, bound): {bad}"
    return errs


@pytest.mark.parametrize("name", list(C.CASES))
def test_consistency_step_parity(name):
    assert os.environ.get("IMK_CONSISTENCY_FUSED", "1") != "0", "this process must run the default routes"
    check_against_oracle(name, run_of(name), "fused" if name in C.FUSED else "composed")


def test_composed_route_in_a_child_process(tmp_path):
    """IMK_CONSISTENCY_FUSED=0 is read once per process: the cases the fused kernel takes, run composed in a child.  The forwards are
    the same launches on both routes, so the pins -- and with them the oracle -- are the parent's."""
    child = ("import sys, numpy as np\n"
             "sys.path[:0] = [%r, %r]\n"
             "import test_gpu_consistency as T\n"
             "for name in T.C.FUSED:\n"
             "    np.savez(sys.argv[1] + name + '.npz', **T.run_case(name))\n") % (ROOT, HERE)
    env = dict(os.environ, IMK_CONSISTENCY_FUSED="0")
    r = subprocess.run([sys.executable, "-c", child, str(tmp_path) + os.sep], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name in C.FUSED:
        fused = run_of(name)
        with np.load(str(tmp_path / (name + ".npz")), allow_pickle=True) as z:
            composed = {k: z[k] for k in z.files}
        for k in fused:
            if k.startswith("ov") or k.startswith("moving/"):
                assert np.array_equal(fused[k], composed[k]), f"{name}: {k} differs between the routes' forwards"
        check_against_oracle(name, composed, "composed")
        check_against_oracle(name, fused, "fused")
        lf, lc = float(fused["stats"][0]), float(composed["stats"][0])
        print(f"{name}: loss fused {lf!r} composed {lc!r}")
        assert abs(lf - lc) <= 1e-6 * abs(lc)
        # which route ran: the routes round in different places (fp32 sums in another order), so the parent's gradients are the child's
        # bit for bit only if the parent took the composed route too
        assert not np.array_equal(fused["grads"], composed["grads"]), f"{name}: this process did not take the fused route"


# ---- structural properties ------------------------------------------------------------------------------------------------------------
STRUCT = ["isic", "hela", "suim"]      # fused one lane per pixel, fused two lanes per pixel, composed softmax


def _ctl(m):
    """(loss_scale, inv_loss_scale, good_steps, step) of the model's optimizer state (ImkCtl, csrc/imk_elem.h)"""
    off = m.plan.state_bytes - 256
    return struct.unpack("ffii", bytes(m.train_state[off:off + 16].cpu().tolist()))


@pytest.mark.parametrize("name", STRUCT)
def test_identical_views_give_zero(name):
    m, _ = build_model(name)
    _, _, d1, _ = views(name)
    m.init_train_state()
    m.grads_and_stats.fill_(float("nan"))      # every gradient and the statistics are written, not left over
    m.consistency_fwd_bwd(d1, d1.clone())
    torch.cuda.synchronize()
    st = m.stats.cpu().numpy()
    assert st[0] == 0.0 and st[1] == 0.0, st
    assert int((m.grads != 0).sum()) == 0, "identical views must give an all-zero gradient"


@pytest.mark.parametrize("name", STRUCT)
def test_swapping_the_views_keeps_the_loss_bits(name):
    m, sd = build_model(name)
    _, _, d1, d2 = views(name)
    m.consistency_fwd_bwd(d1, d2)
    torch.cuda.synchronize()
    a = m.stats.cpu().numpy()[0]
    m.load_state_dict(sd)
    m.consistency_fwd_bwd(d2, d1)
    torch.cuda.synchronize()
    b = m.stats.cpu().numpy()[0]
    assert a > 0 and a.tobytes() == b.tobytes(), (a, b)


def _labelled(name, seed):
    cfg = C.CASES[name]
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(0, 256, (cfg["b"], cfg["h"], cfg["w"], cfg["c"]), dtype=np.uint8)).cuda()
    if cfg["act"] == "sigmoid":
        return x, torch.from_numpy(rng.integers(0, 2, (cfg["b"], cfg["h"], cfg["w"], cfg["k"]), dtype=np.uint8)).cuda(), 0
    return x, torch.from_numpy(rng.integers(0, cfg["k"], (cfg["b"], cfg["h"], cfg["w"]), dtype=np.uint8)).cuda(), 1


@pytest.mark.parametrize("name", ["isic", "suim"])
def test_labelled_and_consistency_steps_share_the_optimizer_state(name):
    """labelled, consistency, labelled: Adam's step counter advances by 3 (one state buffer, one imk_unet_adamw_step)"""
    m, _ = build_model(name)
    _, _, d1, d2 = views(name)
    x, y, kind = _labelled(name, 7)
    m.init_train_state()
    assert _ctl(m)[3] == 0
    scales = []
    for what in ("labelled", "consistency", "labelled"):
        before = m.params[:m.plan.n_trainable].clone()
        if what == "labelled":
            m.train_step(x, y, kind, 3e-3, 1e-4)
        else:
            m.consistency_step(d1, d2, 3e-3, 1e-4)
        torch.cuda.synchronize()
        st = m.stats.cpu().numpy()
        scales.append(st[2])
        assert st[1] == 0.0 and np.isfinite(st[0]), (what, st)
        assert not torch.equal(before, m.params[:m.plan.n_trainable]), what
    assert _ctl(m)[3] == 3 and _ctl(m)[2] == 3
    assert scales == [32768.0] * 3


@pytest.mark.parametrize("name", ["isic", "suim"])
def test_overflowing_consistency_step_is_skipped(name):
    """as tests/test_gpu_unet.py::test_overflow_skips_step_and_halves_scale: params untouched apart from the moving statistics"""
    m, _ = build_model(name)
    _, _, d1, d2 = views(name)
    m.init_train_state()
    ctl_off = m.plan.state_bytes - 256
    m.train_state[ctl_off:ctl_off + 8] = torch.tensor(list(struct.pack("ff", 2.0 ** 40, 2.0 ** -40)), dtype=torch.uint8).cuda()
    before = m.params.clone()
    m.consistency_step(d1, d2, 3e-3, 1e-4)
    torch.cuda.synchronize()
    st = m.stats.cpu().numpy()
    nt = m.plan.n_trainable
    assert st[1] == 1.0, st
    assert torch.equal(before[:nt], m.params[:nt])
    assert not torch.equal(before[nt:], m.params[nt:]), "the moving statistics move in a skipped step too"
    assert _ctl(m)[0] == 2.0 ** 39 and _ctl(m)[3] == 0


@pytest.mark.parametrize("name", ["isic", "suim"])
def test_labelled_step_is_untouched_by_a_consistency_call(name):
    """the labelled fwd_bwd on the same model, bit for bit, before and after a consistency call: the workspaces do not bleed"""
    m, sd = build_model(name)
    _, _, d1, d2 = views(name)
    x, y, kind = _labelled(name, 9)
    m.fwd_bwd(x, y, kind)
    torch.cuda.synchronize()
    g0, s0 = m.grads.clone(), m.stats.clone()
    m.load_state_dict(sd)
    m.consistency_fwd_bwd(d1, d2)
    m.load_state_dict(sd)          # the moving statistics of the call above
    m.fwd_bwd(x, y, kind)
    torch.cuda.synchronize()
    assert torch.equal(g0, m.grads) and torch.equal(s0[:3], m.stats[:3])
