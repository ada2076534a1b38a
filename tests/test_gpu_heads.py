"""The output heads (unet.py:63, the reference's one float32 layer) held to a float64 reference of the head ALONE, at every edge of their
16-class tiles and on every channel stride.  The whole-network tests (tests/test_gpu_unet.py) need rel-L2 1e-2 / max |dp| 3e-2 for the
fp16 towers in front of the head; a head that dropped the `lo` half of its split weights, took a coarser exponential or added its bias in
fp16 sits 50 times inside those.  oracle/head_oracle.py is the reference, tests/test_cpu_head_oracle.py holds the yardsticks, their
reasoning and the planted defects that show they have teeth.

All cases: 32 x 32 images at batch 2 = 2048 pixels = 8 workgroups of the head kernels = 32 groups of 64 pixels; channel strides 8 / 16 / 24 /
32 from alpha 0.5 / 1 / 1.25 / 2 (real widths 8 / 16 / 20 / 32).

(a) inference heads in isolation: max |p_gpu - p_64| <= 8 x max |p_32 - p_64| per case, p_64 = head_oracle fed the stored d9.c1, p_32 the
    numpy float32 head on the same data.  The BatchNorm fold is made exact (moving variance float32(0.999): var + eps == 1.0f; mean 0; gamma,
    beta multiples of 1/64), so the reference sees bit for bit the x the kernel sees.  Both stores of head_softmax_kernel (16-byte and
    4-byte, the latter through a `probs` pointer 4 bytes off alignment): bit-identical.
(b) the fused heads (IM, vote hard / soft, teacher label) at K = 16, 17, 48, 49, 64: bit-identical to their unfused routes, by the
    comparisons of the existing fused-vs-unfused tests.
(c) training: every head_cce_fused_kernel<CSV,KT> form and four sigmoid + mse shapes through the procedure and the bounds of
    test_train_step_parity.  The fused route needs imk_loss_blocks(2048) = 8 partial rows <= the last BatchNorm's n_bwd_rows, which is at
    least B * ceil(h / 8) * ceil(w / 16) = 16 (csrc/imk_net.h), so it is taken.
(d) training heads in isolation: loss and the gradients of out.w, out.b, d9.bnb.gamma, d9.bnb.beta against head_oracle in training mode on
    the stored d9.c1 and its float64 batch statistics, within 2 x (d_round + d_stat) of the nearer reference.

Measured on the MI355X: tests/measured/head_isolation.json (written when IMK_HEAD_MEASURED_OUT names a file)."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_cpu_head_oracle as C  # noqa: E402
import test_gpu_unet as TU  # noqa: E402

H, W, B = 32, 32, 2
MEASURED = {"about": "tests/test_gpu_heads.py on the MI355X.  inference: max |p - p_64| of the GPU and of numpy float32, the bound (8 x the "
                     "latter) and their ratio, per (channel stride, activation, K).  training: per (channel stride, K, activation) the kernel "
                     "form, the step's loss scale, the GPU's rel-L2 distance to the nearer reference per quantity, the yardsticks d_round and "
                     "d_stat, the bound 2 x (d_round + d_stat), and the loss gap with its bound (absolute).",
            "inference": {}, "training": {}}


@pytest.fixture(scope="module")
def UNet():
    assert torch.cuda.is_available()
    from inconsistencymasks_amd.unet import UNet as cls
    yield cls
    out = os.environ.get("IMK_HEAD_MEASURED_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _cfg(cs, k, act):
    return dict(h=H, w=W, c=3, k=k, alpha=C.WIDTHS[cs][0], act=act, loss="mse" if act == "sigmoid" else "cce", b=B)


# ---- (a) inference heads in isolation ---------------------------------------------------------------------------------------------------
def _isolated_model(UNet, cs, act, k):
    alpha, cin = C.WIDTHS[cs]
    m = UNet(H, W, 3, k, alpha, act, seed=1000 + cs + k)
    sd = TU.randomize_bn(m.state_dict(), 7)
    gamma, beta, w, b = C.draw_head_params(cin, k, 2000 + 100 * cs + k)
    assert sd["d9.bnb.gamma"].shape == (cin,) and sd["out.w"].shape == (1, 1, cin, k)
    sd["d9.bnb.gamma"], sd["d9.bnb.beta"] = torch.from_numpy(gamma), torch.from_numpy(beta)
    sd["d9.bnb.mean"], sd["d9.bnb.var"] = torch.zeros(cin), torch.full((cin,), 0.999)
    sd["out.w"], sd["out.b"] = torch.from_numpy(w).reshape(1, 1, cin, k), torch.from_numpy(b)
    m.load_state_dict(sd)
    return m, gamma, beta, w, b


@pytest.mark.parametrize("case", C.INFER_CASES, ids=C.case_id)
def test_inference_head_in_isolation(UNet, case):
    from inconsistencymasks_amd._lib import check, lib
    cs, act, k = case
    cin = C.WIDTHS[cs][1]
    # the exact fold: bn_fold_batched_kernel's gamma / sqrtf(var + 1e-3f) and beta - mean * scale give gamma and beta themselves
    assert np.float32(np.float32(0.999) + np.float32(1e-3)) == np.float32(1.0)
    m, gamma, beta, w, b = _isolated_model(UNet, cs, act, k)
    assert m.plan.layers[-1]["name"] == "out" and m.plan.layers[-1]["cin"] == cin
    x, _, _ = TU.make_input(_cfg(cs, k, act), 40 + k)
    xd = torch.from_numpy(x).cuda()
    pd = m.predict_device(xd)
    probs = pd.cpu().numpy().reshape(-1, k)
    z = m.intermediate("d9.c1", B, 0).numpy().reshape(-1, cin)
    assert z.shape[0] == 2048 and z.min() >= 0 and z.std() > 0.05        # a live post-ReLU activation, not a constant
    p64, d32, bound = C.infer_yardstick(z, gamma, beta, w, b, act)
    d = C.infer_distance(probs, p64)
    rec = dict(gpu_vs_f64=d, f32_vs_f64=d32, bound=bound, factor=d / d32)
    if act == "softmax":
        rec["row_sum_gap"] = float(np.abs(probs.astype(np.float64).sum(-1) - 1).max())
    MEASURED["inference"][C.case_id(case)] = rec
    print(f"head {C.case_id(case)}: GPU {d:.3e} from float64, float32 {d32:.3e} ({d / d32:.2f} x; bound {C.INFER_FACTOR:g} x)")
    assert np.isfinite(probs).all()
    assert d <= bound, f"max |p_gpu - p_64| = {d:.3e} is {d / d32:.2f} x float32's own {d32:.3e} (bound {C.INFER_FACTOR:g} x)"
    if act == "softmax":
        assert rec["row_sum_gap"] <= k * bound
    # the other store of head_softmax_kernel: a probability buffer 4 bytes off 16-byte alignment takes the 4-byte stores
    n = probs.size
    buf = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[1:1 + n]
    assert pd.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4
    ws = m.workspace(B, 0)
    check(lib.imk_unet_forward(m.plan.ptr, m.params.data_ptr(), m.packed.data_ptr(), xd.data_ptr(), B, out.data_ptr(), ws.data_ptr(),
                               ws.numel(), torch.cuda.current_stream().cuda_stream), "imk_unet_forward")
    torch.cuda.synchronize()
    assert torch.equal(out, pd.reshape(-1))
    assert bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[1 + n:]).all())


# ---- (b) the fused heads at the new class counts ------------------------------------------------------------------------------------------
FUSED_K = (16, 17, 48, 49, 64)
FUSED_CASES = [(cs, k) for cs in (16, 32) for k in FUSED_K]
_fused_ids = [f"{cs}-{k}" for cs, k in FUSED_CASES]


def _ensemble(UNet, cs, k, n=2):
    models = [UNet(H, W, 3, k, C.WIDTHS[cs][0], "softmax", seed=300 + 7 * k + j) for j in range(n)]
    for j, mm in enumerate(models):
        mm.load_state_dict(TU.randomize_bn(mm.state_dict(), 900 + k + j))
    x = np.random.default_rng(k + cs).integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    return models, x


@pytest.mark.parametrize("cs,k", FUSED_CASES, ids=_fused_ids)
def test_forward_im_matches_unfused(UNet, cs, k):
    """as test_randomized_ensembles_fused_vs_unfused: imk_unet_forward_im against imk_unet_forward's probabilities through the oracle's IM
    chain (np.argmax of every model's probabilities), bit for bit"""
    from inconsistencymasks_amd import functions as F
    from oracle import im_oracle as O
    models, x = _ensemble(UNet, cs, k)
    xd = torch.from_numpy(x).cuda()
    r = F.EnsembleIM(models).run(xd, 0.5, False, True, True, want_presence=True)
    pn = torch.stack([mm.predict_device(xd) for mm in models], 0).cpu().numpy()
    assert len({int(v) for v in pn.argmax(-1).ravel()}) > 1
    for i in range(B):
        e = O.im_multiclass(pn[:, i])
        eimg, (ef,) = O.block(x[i], [e["final"]], e["im"], True, True)
        assert np.array_equal(r["masks"][i, 0].cpu().numpy(), ef)
        assert int(r["im_size"][i, 0]) == int(e["im_size"])
        assert np.array_equal(r["presence"][:, i].cpu().numpy(), e["presence"])
        assert np.array_equal(r["im"][i].cpu().numpy(), e["im"])
        assert np.array_equal(r["img_out"][i].cpu().numpy(), eimg)


@pytest.mark.parametrize("cs,k", FUSED_CASES, ids=_fused_ids)
def test_forward_vote_matches_unfused(UNet, cs, k):
    """as tests/test_gpu_model_ensemble.py::test_forward_vote_is_bit_identical_to_forward_plus_vote, hard and soft; the hard vote of one
    model is np.argmax of the probabilities imk_unet_forward returns"""
    import test_gpu_model_ensemble as ME
    models, x = _ensemble(UNet, cs, k)
    xd = torch.from_numpy(x).cuda()
    for soft in (False, True):
        want = ME._unfused(models, xd, 0.5, soft)
        got = ME._forward_vote(models, xd, 0.5, soft, 2)
        torch.cuda.synchronize()
        assert torch.equal(got, want), (soft, int((got != want).sum()))
        assert torch.equal(ME.V.EnsembleVote(models).run(xd, 0.5, soft), want)          # the Python entry point
    one = ME._forward_vote(models[:1], xd, 0.5, False, 1)
    torch.cuda.synchronize()
    assert np.array_equal(one.cpu().numpy(), models[0].predict_device(xd).cpu().numpy().argmax(-1).astype(np.uint8))


@pytest.mark.parametrize("cs,k", FUSED_CASES, ids=_fused_ids)
def test_forward_student_matches_unfused(cs, k):
    """as tests/test_gpu_noisy_student.py: imk_unet_forward_student against imk_unet_forward -> np.argmax -> the augmentation oracle, and
    the unfused route under the materialize switch, bit for bit"""
    import test_gpu_noisy_student as NS
    from inconsistencymasks_amd import noisy_student
    NS.run_case(noisy_student, f"heads-{cs}-{k}", H, W, 3, k, C.WIDTHS[cs][0], "softmax", [(0, 0, 0), (0, 1, 0), (1, 0, 1), (1, 1, 2)], False)


# ---- (c) training heads: every form against the whole-step oracle ----------------------------------------------------------------------------
def _train_batch(case):
    """the case's configuration and batch: tests/test_cpu_head_oracle.py::training_batch (the first seed on which the oracle alone is
    conditioned; class 0 and class K - 1 labelled)"""
    cfg, batch, _ = C.training_batch(case)
    return cfg, batch


def test_the_table_names_the_form_the_launcher_picks():
    """imk_launch_head_cce_fused: CSV = 16 for cs <= 16, else 32; KT = ceil(K / 16).  All eight forms are reached."""
    forms = set()
    for cs, k, act, loss, form in C.TRAIN_CASES:
        if loss == "cce":
            assert form == f"head_cce_fused_kernel<{16 if cs <= 16 else 32},{(k + 15) // 16}>"
            forms.add(form)
    assert len(forms) == 8


@pytest.mark.parametrize("case", C.TRAIN_CASES, ids=C.case_id)
def test_training_step_against_the_whole_step_oracle(UNet, case):
    cfg, batch = _train_batch(case)
    TU.train_step_parity(UNet, cfg, batch)


# ---- (d) training heads in isolation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.TRAIN_CASES, ids=C.case_id)
def test_training_head_in_isolation(UNet, case):
    cs, k, act, loss, form = case
    cin = C.WIDTHS[cs][1]
    cfg, (x, y, tgt) = _train_batch(case)
    m = UNet(H, W, 3, k, cfg["alpha"], act, seed=11)
    sd = TU.randomize_bn(m.state_dict(), 12)
    m.load_state_dict(sd)
    stats = TU.first_finite_step(m, sd, x, y, 0 if loss == "mse" else 1)
    z = m.intermediate("d9.c1", B, 1).numpy().reshape(-1, cin)
    g = m.grads.cpu().numpy()
    lay = {l["name"]: l for l in m.plan.layers}
    lo, lb = lay["out"], lay["d9.bnb"]
    assert (lo["cin"], lo["cout"], lb["cout"]) == (cin, k, cin)
    got = {"loss": float(stats[0]), "out.w": g[lo["off_w"]:lo["off_w"] + cin * k].reshape(cin, k), "out.b": g[lo["off_b"]:lo["off_b"] + k],
           "gamma": g[lb["off_w"]:lb["off_w"] + cin], "beta": g[lb["off_b"]:lb["off_b"] + cin]}
    yd = C.train_yardsticks(z, sd["d9.bnb.gamma"].numpy(), sd["d9.bnb.beta"].numpy(), sd["out.w"][0, 0].numpy(), sd["out.b"].numpy(),
                            act, loss, tgt.reshape(-1, k), float(stats[2]))
    d, dl = C.train_distances(got, yd)
    MEASURED["training"][C.case_id(case)] = dict(form=form, loss_scale=float(stats[2]), gpu=d, d_round=yd["d_round"], d_stat=yd["d_stat"],
                                                 bound=yd["bound"], loss_gap=dl, loss_bound=yd["loss_bound"], loss=yd["on"]["loss"])
    print(f"training head {C.case_id(case)} ({form}), scale {stats[2]:g}: " +
          "; ".join(f"{q} {d[q]:.2e} (round {yd['d_round'][q]:.2e}, stat {yd['d_stat'][q]:.2e})" for q in C.TRAIN_QUANTITIES) +
          f"; loss gap {dl:.2e} (bound {yd['loss_bound']:.2e})")
    bad = {q: (d[q], yd["bound"][q]) for q in C.TRAIN_QUANTITIES if not d[q] <= yd["bound"][q]}
    assert not bad, f"(distance, bound) outside {C.TRAIN_MARGIN:g} x (d_round + d_stat): {bad}"
    assert dl <= yd["loss_bound"], (dl, yd["loss_bound"])
