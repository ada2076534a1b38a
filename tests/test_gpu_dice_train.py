"""Loss kind 4 of imk_unet_fwd_bwd (the reference's dice_loss on sigmoid heads, csrc/imk_dice.hip) and imk_eval_dice_sums on the GPU.

  * against the oracle, by the procedure of test_gpu_depth_train.py::test_kind2_against_the_oracle: oracle/unet_oracle.forward in
    training mode with the conv outputs pinned to the GPU's, the Dice loss written in torch (tests/dice_cases.py).  Bounds: loss 1e-4
    relative; every gradient tensor rel-L2 <= max(2e-2, 1.5 x d), d = the distance between the oracle's fp16-emulating and fp32 forms
    of that gradient on the same pins (the yardstick tests/test_gpu_consistency.py forms);
  * image boundaries: 1536 pixels per image are no multiple of the fused kernel's 4 x 256-pixel iteration, three images of ~2 % / 50 % /
    98 % foreground -- a coefficient taken from the neighbouring image moves out.b's gradient far outside the bound; the same at
    16 x 16 x 5 (one workgroup per image) on the composed route;
  * imk_eval_dice_sums: a batch of 5 equals the five single-image calls bit for bit and numpy float64 within 1e-12 relative;
  * stats[0] equals 1 - mean dice_b formed in float64 from imk_eval_dice_sums on the training-mode probabilities (the head of the
    oracle on the GPU's own last activation under its batch statistics) within 1e-5 relative;
  * both routes (IMK_DICE_FUSED=0 in a child process) pass the oracle check with bit-identical losses;
  * bit-reproducible; Dice on a fixed batch falls over 20 applied steps; a non-finite probability skips the step; refusals."""
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

import dice_cases as DC  # noqa: E402
import test_gpu_unet as TU  # noqa: E402  (make_input, randomize_bn, first_finite_step, rel_l2)
from inconsistencymasks_amd import evaluate as E  # noqa: E402
from inconsistencymasks_amd.unet import UNet  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402

F32 = np.float32
# name -> (configuration, the gradient route it takes by default)
CASES = {
    "isic": (TU.CFGS["isic"], "fused"),                                                     # 64 x 64, K 1, 8 channels, B 4
    "hela": (TU.CFGS["hela"], "composed"),                                                  # 32 x 48, K 3, 16 channels, B 3
    "alpha2": (TU.CFGS["alpha2"], "composed"),                                              # 32 channels
    "bound_fused": (dict(h=32, w=48, c=3, k=1, alpha=0.5, act="sigmoid", loss="mse", b=3), "fused"),
    "bound_composed": (dict(h=16, w=16, c=3, k=1, alpha=1.0, act="sigmoid", loss="mse", b=5), "composed"),
}
FUSED = [n for n, (_, r) in CASES.items() if r == "fused"]
SHARES = [0.02, 0.5, 0.98, 0.25, 0.75]
_RUNS, _REFS = {}, {}


def batch_of(name):
    cfg = CASES[name][0]
    x, y, _ = TU.make_input(cfg, 13)
    if name.startswith("bound"):      # every image its own foreground share
        rng = np.random.default_rng(17)
        y = np.stack([(rng.random((cfg["h"], cfg["w"], cfg["k"])) < SHARES[i]).astype(np.uint8) for i in range(cfg["b"])], 0)
    if name == "hela":
        y[..., 2] *= 3                # the position plane is 0 / 3
    return x, y


def build_model(name, seed=11):
    cfg = CASES[name][0]
    m = UNet(cfg["h"], cfg["w"], cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], seed=seed)
    sd = TU.randomize_bn(m.state_dict(), seed + 1)
    m.load_state_dict(sd)
    return m, sd


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_case(name, scale=32768.0):
    """one finite kind-4 step of the case on this process's route, run twice -> everything the checks read (numpy)"""
    cfg = CASES[name][0]
    m, sd = build_model(name)
    x, y = batch_of(name)
    stats = TU.first_finite_step(m, sd, x, y, 4, scale)
    g1, s1 = m.grads.clone(), m.stats.clone()
    m.fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 4)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g1), _bits(m.grads)) and torch.equal(_bits(s1), _bits(m.stats)), "kind 4 is not bit-reproducible"
    out = {"stats": stats.copy(), "grads": g1.cpu().numpy()}
    for l in m.plan.layers:
        if l["kind"] == 0 and l["name"] != "out":
            out["ov/" + l["name"]] = m.intermediate(l["name"], cfg["b"], 1).numpy()
    out["layers"] = np.array([(l["name"], l["kind"], l["ksize"], l["cin"], l["cout"], l["off_w"], l["off_b"]) for l in m.plan.layers], dtype=object)
    return out


def run_of(name):
    if name not in _RUNS:
        _RUNS[name] = run_case(name)
    return _RUNS[name]


def reference_of(name, run):
    """the oracle on the pins of `run` in its fp16-emulating and fp32 forms, computed once per case and left unchanged
    -> (loss, gradients, {tensor: rel-L2 between the two forms})"""
    if name not in _REFS:
        cfg = CASES[name][0]
        _, sd = build_model(name)
        x, y = batch_of(name)
        tgt = y.astype(F32)
        ov = {k.split("/", 1)[1]: torch.from_numpy(v) for k, v in run.items() if k.startswith("ov/")}
        loss16, g16 = DC.oracle_step(U, sd, x, tgt, cfg, True, float(run["stats"][2]), ov)
        _, g32 = DC.oracle_step(U, sd, x, tgt, cfg, False, 1.0, ov)
        assert all(bool(torch.isfinite(v).all()) for v in g16.values()), "the oracle's step overflows at the GPU's loss scale"
        _REFS[name] = (loss16, g16, {n: TU.rel_l2(g16[n].numpy(), g32[n].numpy()) for n in g16})
    return _REFS[name]


def grad_errors(run, g_ref):
    g, errs = run["grads"], {}
    for name, kind, ks, ci, co, off_w, off_b in run["layers"]:
        if kind == 0:
            errs[name + ".w"] = TU.rel_l2(g[off_w:off_w + ks * ks * ci * co].reshape(ks, ks, ci, co), g_ref[name + ".w"].numpy())
            errs[name + ".b"] = TU.rel_l2(g[off_b:off_b + co], g_ref[name + ".b"].numpy())
        else:
            errs[name + ".gamma"] = TU.rel_l2(g[off_w:off_w + co], g_ref[name + ".gamma"].numpy())
            errs[name + ".beta"] = TU.rel_l2(g[off_b:off_b + co], g_ref[name + ".beta"].numpy())
    return errs


def bound(d):
    return max(2e-2, 1.5 * d)


def check_against_oracle(name, run, route):
    loss_ref, g_ref, dist = reference_of(name, run)
    stats = run["stats"]
    errs = grad_errors(run, g_ref)
    worst = max(errs, key=lambda k: errs[k] / bound(dist[k]))
    print(f"{name} ({route}): loss {stats[0]!r} oracle {loss_ref!r} rel {abs(stats[0] - loss_ref) / abs(loss_ref):.2g}; gradient rel-L2 max "
          f"{max(errs.values()):.3g}; closest to its bound: {worst} {errs[worst]:.3g} of {bound(dist[worst]):.3g} (yardstick {dist[worst]:.3g}); "
          f"out.b {errs['out.b']:.3g}")
    assert abs(stats[0] - loss_ref) <= 1e-4 * abs(loss_ref)
    bad = {k: (round(v, 4), round(bound(dist[k]), 4)) for k, v in errs.items() if not v <= bound(dist[k])}
    assert not bad, f"{name} ({route}): gradient tensors beyond max(2e-2, 1.5 x yardstick) (rel-L2, bound): {bad}"


@pytest.mark.parametrize("name", list(CASES))
def test_kind4_against_the_oracle(name):
    assert os.environ.get("IMK_DICE_FUSED", "1") != "0", "this process must run the default routes"
    check_against_oracle(name, run_of(name), CASES[name][1])


def test_a_neighbouring_images_coefficients_would_be_caught():
    """what the boundary cases rest on: with the coefficients of image b + 1 the float64 rule's out.b gradient (the sum of dL/dlogit)
    leaves the bound by far at these foreground shares"""
    for name in ("bound_fused", "bound_composed"):
        _, y = batch_of(name)
        t = y.astype(np.float64)
        p = np.random.default_rng(3).random(t.shape)
        c0, c1 = DC.coefficients(t, p)
        right = DC.dloss_dlogit(t, p).sum()
        wrong = ((np.roll(c0, -1)[:, None, None, None] - np.roll(c1, -1)[:, None, None, None] * t) * p * (1 - p)).sum()
        assert abs(wrong - right) > 10 * 2e-2 * abs(right), name


def test_both_routes_in_a_child_process(tmp_path):
    """IMK_DICE_FUSED=0 is read once per process: the cases the fused variant takes, run composed in a child.  The forward and the sums
    and coefficient launches are the same on both routes: the pins and the loss are the parent's bit for bit."""
    child = ("import sys, numpy as np\n"
             "sys.path[:0] = [%r, %r]\n"
             "import test_gpu_dice_train as T\n"
             "for name in T.FUSED:\n"
             "    np.savez(sys.argv[1] + name + '.npz', **T.run_case(name))\n") % (ROOT, HERE)
    env = dict(os.environ, IMK_DICE_FUSED="0")
    r = subprocess.run([sys.executable, "-c", child, str(tmp_path) + os.sep], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for name in FUSED:
        fused = run_of(name)
        with np.load(str(tmp_path / (name + ".npz")), allow_pickle=True) as z:
            composed = {k: z[k] for k in z.files}
        for k in fused:
            if k.startswith("ov/"):
                assert np.array_equal(fused[k], composed[k]), f"{name}: {k} differs between the routes' forwards"
        check_against_oracle(name, composed, "composed")
        check_against_oracle(name, fused, "fused")
        assert fused["stats"].tobytes() == composed["stats"].tobytes(), (name, fused["stats"], composed["stats"])
        # which route ran: the routes round their dgrad and weight-gradient sums in different places
        assert not np.array_equal(fused["grads"], composed["grads"]), f"{name}: this process did not take the fused route"


def test_eval_dice_sums_per_image_independence():
    rng = np.random.default_rng(5)
    b, h, w, k = 5, 24, 20, 3
    p = rng.random((b, h, w, k)).astype(F32)
    g = (rng.random((b, h, w, k)) < np.array(SHARES)[:, None, None, None]).astype(np.uint8)
    g[..., 2] *= 3
    pd, gd = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    whole = E.dice_sums(pd, gd)
    assert whole.shape == (b, 3) and whole.dtype == np.float64
    for i in range(b):
        one = E.dice_sums(pd[i:i + 1], gd[i:i + 1])
        assert one.tobytes() == whole[i:i + 1].tobytes(), i
    want = DC.sums(g, p)
    assert np.abs(whole - want).max() <= 1e-12 * np.abs(want).max() and (np.abs(whole - want) <= 1e-12 * np.abs(want)).all()
    assert np.array_equal(E.dice_from_sums(whole), DC.dice_from_sums(whole))


@pytest.mark.parametrize("name", ["isic", "hela"])
def test_loss_value_is_the_monitor_on_the_training_probabilities(name):
    """the head of the oracle (BatchNorm with batch statistics rounded once to fp16, the fp32 output layer, sigmoid) on the GPU's own
    last decoder activation -> imk_eval_dice_sums -> 1 - mean dice_b in float64"""
    cfg = CASES[name][0]
    run = run_of(name)
    _, sd = build_model(name)
    _, y = batch_of(name)
    z = torch.from_numpy(run["ov/d9.c1"]).float().permute(0, 3, 1, 2)
    with torch.no_grad():
        probs, _ = U.head(U._bn(z, sd, "d9.bnb", True, True, None), sd["out.w"], sd["out.b"], cfg["act"])
    probs = probs.permute(0, 2, 3, 1).contiguous()
    s = E.dice_sums(probs.cuda(), torch.from_numpy(y).cuda())
    want = 1.0 - float(np.mean(E.dice_from_sums(s)))
    got = float(run["stats"][0])
    print(f"{name}: stats[0] {got!r} monitor {want!r} rel {abs(got - want) / abs(want):.2g}")
    assert abs(got - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize("name", ["isic", "hela"])
def test_training_moves(name):
    m, _ = build_model(name)
    x, y = batch_of(name)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m.init_train_state()
    losses, applied = [], 0
    while applied < 20 and len(losses) < 40:
        m.train_step(xd, yd, 4, 3e-3, 1e-4)
        st = m.stats.cpu().numpy()
        losses.append(float(st[0]))
        applied += int(st[1] == 0.0)
    m.fwd_bwd(xd, yd, 4)
    last = float(m.stats[0])
    print(f"{name}: Dice loss {losses[0]:.5f} -> {last:.5f} over {applied} applied steps")
    assert applied == 20 and np.isfinite(losses).all() and last < losses[0]


@pytest.mark.parametrize("name", ["isic", "hela"])
def test_a_non_finite_probability_skips_the_step(name):
    m, sd = build_model(name)
    x, y = batch_of(name)
    sd = dict(sd)
    sd["out.b"] = torch.full_like(sd["out.b"], float("nan"))
    m.load_state_dict(sd)
    m.init_train_state()
    m.fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 4)
    st = m.stats.cpu().numpy()
    assert np.isnan(st[0]) and st[1] == 1.0, st
    nt = m.plan.n_trainable
    before = m.params[:nt].clone()
    m.adamw_step(3e-3, 1e-4)
    assert torch.equal(_bits(before), _bits(m.params[:nt]))


def test_refusals():
    from inconsistencymasks_amd._lib import ImkError
    soft = UNet(32, 32, 3, 4, 0.5, "softmax", seed=1)
    x = torch.zeros((1, 32, 32, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ImkError):
        soft.fwd_bwd(x, torch.zeros((1, 32, 32, 4), dtype=torch.uint8, device="cuda"), 4)
    sig = UNet(32, 32, 3, 1, 0.5, "sigmoid", seed=1)
    y = torch.zeros((1, 32, 32, 1), dtype=torch.uint8, device="cuda")
    with pytest.raises(ImkError):
        sig.fwd_bwd(x, y, 5)
    sig.fwd_bwd(x, y, 4)
    assert float(sig.stats[1]) in (0.0, 1.0)
