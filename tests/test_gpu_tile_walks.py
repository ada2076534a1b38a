"""The persistent kernels' multi-tile walks, pinned to the same kernels' one-tile-per-workgroup launches.

In every oracle-parity case of tests/test_gpu_unet.py, tests/test_gpu_heads.py and tests/test_gpu_evalnet.py each workgroup of a persistent
kernel (conv_pipe_kernel, conv_wide_kernel, bwd1x1_kernel, wgrad_mfma_kernel, wgrad_gemm_kernel) processes exactly one tile: grid ==
n_tiles.  The loop-carried half of those kernels -- the register prefetch of the next tile, the q / r step across image boundaries
(ptile_next, ImkWalk), the last iteration's re-read of the current tile, the ticket taking of the dynamic walk, accumulators and
BatchNorm-statistics rows carried from tile to tile -- runs only in launches with more tiles than workgroups.  Here small images at large
batches make every level-0 and level-1 launch walk (tests/tile_walk_cases.py; the conditions are checked in
tests/test_cpu_tile_walk_cases.py), with no change to how anything is launched, and the reference of a walked launch is the same kernel's
one-tile launch, which the suites above pin to the oracle:

  * inference is bit-exact batch-invariant, so a 768-image forward equals its 16-image sub-batches (at most 256 tiles at every level: one
    tile per workgroup whatever the occupancy) bit for bit -- probabilities, every stored layer, the fused consumers' outputs;
  * a training batch of 96 identical replicas of a 4-image batch makes the training forward comparable bit for bit (replica r against
    replica 0), and its mean loss and mean-loss gradients are those of the 4 images, which the whole-step oracle can compute.

Nothing here is an allclose: a failing identity is a finding, reported as (layer, image, tile row / column, tile index in the launch).
Measured on the MI355X: tests/measured/tile_walks.json (written when IMK_TILE_WALK_MEASURED_OUT names a file)."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_gpu_unet as TU  # noqa: E402
import tile_walk_cases as T  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402

MEASURED = {"about": "tests/test_gpu_tile_walks.py on the MI355X.  layers: per case and resolution the 16 x 16 tile count of a persistent "
                     "launch at the test's batch, what that count says about the walk (a condition: tests/tile_walk_cases.py::walk_class; "
                     "which kernel class runs a deep layer is the library's choice) and the stored layers of that resolution.  training: the step's loss scale and, per "
                     "gradient tensor, the rel-L2 distance between the 384-image replica step and a plain GPU step on the 4 images -- two "
                     "implementations of the code under test, recorded, not a bound.",
            "layers": {"inference": {}, "training": {}}, "training": {}}


@pytest.fixture(scope="module")
def UNet():
    assert torch.cuda.is_available()
    from inconsistencymasks_amd.unet import UNet as cls
    yield cls
    out = os.environ.get("IMK_TILE_WALK_MEASURED_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)
            f.write("\n")


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def layer_views(m, batch, mode, names):
    """name -> the stored conv output as an fp16 DEVICE view [batch, h, w, c] into the model's workspace of (batch, mode), as
    imk_unet_tensor_info / imk_evalnet_tensor_info describe it (UNet.intermediate copies to CPU float32: minutes at these batches)"""
    from inconsistencymasks_amd._lib import check, lib
    from inconsistencymasks_amd.evalnet import EvalNet
    fn = lib.imk_evalnet_tensor_info if isinstance(m, EvalNet) else lib.imk_unet_tensor_info
    ws = [v for k, v in m._ws.items() if k[0] == batch and k[1] == mode][0]
    index = {l["name"]: i for i, l in enumerate(m.plan.layers)}
    out = {}
    for n in names:
        off, h, w, c, cs = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check(fn(m.plan.ptr, batch, mode, index[n], 0, ctypes.byref(off), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c), ctypes.byref(cs)),
              "tensor_info " + n)
        cnt = batch * h.value * w.value * cs.value
        out[n] = ws[off.value:off.value + 2 * cnt].view(torch.float16).reshape(batch, h.value, w.value, cs.value)[..., :c.value]
    return out


def stored_names(m, materialize, skip=("out",)):
    """the conv outputs a forward stores: all of them under the materialize switch (and in training), the block outputs *.c1 and the
    decoder's *.ca on the default inference path (tests/test_gpu_unet.py::test_inference_parity)"""
    names = [l["name"] for l in m.plan.layers if l["kind"] == 0 and l["name"] not in skip]
    return names if materialize else [n for n in names if n.endswith(".c1") or n.endswith(".ca")]


def record_layers(kind, case, views):
    """per resolution: the 16 x 16 tile count of a persistent launch over it at this batch, what the count says about the walk
    (a condition, tests/tile_walk_cases.py::walk_class) and the stored layers of that resolution"""
    levels = {}
    for n, v in views.items():
        b, h, w = v.shape[:3]
        tiles = b * math.ceil(h / T.TILE) * math.ceil(w / T.TILE)
        levels.setdefault(f"{h}x{w}", dict(batch=b, tiles=tiles, walk=T.walk_class(tiles), layers=[]))["layers"].append(n)
    MEASURED["layers"][kind][case] = {k: dict(v, layers=" ".join(v["layers"])) for k, v in levels.items()}


assert_equals_sub_batches = T.assert_equals_sub_batches


def build(UNet, cfg, seed=1):
    m = UNet(cfg["h"], cfg["w"], cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], seed=seed)
    sd = TU.randomize_bn(m.state_dict(), seed + 1)
    m.load_state_dict(sd)
    return m, sd


def images(cfg, batch, seed=3):
    """make_input's texture plus its per-image noise: distinct per index (a constant image would hide a wrong tile address)"""
    x, _, _ = TU.make_input(dict(cfg, b=batch), seed)
    assert not np.array_equal(x[0], x[1]) and not np.array_equal(x[0], x[batch - 1])
    return x


def forward_with_layers(m, xd, names, drop_unwritten=False):
    """imk_unet_forward (as predict_device calls it) + clones of the stored layers (the next forward of another batch size replaces
    the workspace).  The probability buffer and the slots of the stored layers are filled with NaN first, which compares unequal to
    itself: a tile the forward did not write fails every comparison, and stale activations of an earlier call cannot pass as fresh
    ones.  The REST of the workspace is left as the previous call left it -- the tile counters of the dynamic walk live there, at
    their end values.  drop_unwritten: layers the forward did not write at all are left out (on the default path a fused first stage,
    PRE, keeps the decoder's *.ca on the chip; tensor_info still names its slot); the block outputs *.c1 are always written."""
    from inconsistencymasks_amd._lib import check, lib
    m.ready_for_inference()
    b, p = xd.shape[0], m.plan
    assert xd.is_contiguous() and xd.dtype == torch.uint8
    ws = m.workspace(b, 0)
    for v in layer_views(m, b, 0, names).values():
        v.fill_(float("nan"))
    probs = torch.full((b, p.h, p.w, p.n_out), float("nan"), dtype=torch.float32, device=xd.device)
    check(lib.imk_unet_forward(p.ptr, m.params.data_ptr(), m.packed.data_ptr(), xd.data_ptr(), b, probs.data_ptr(), ws.data_ptr(), ws.numel(),
                               torch.cuda.current_stream().cuda_stream), "imk_unet_forward")
    out = {"probs": probs}
    for n, v in layer_views(m, b, 0, names).items():
        if drop_unwritten and bool(torch.isnan(v).all()):
            assert not n.endswith(".c1"), n
            continue
        out[n] = v.clone()
    return out


# ---- inference, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("materialize", [False, True], ids=["default", "materialize"])
@pytest.mark.parametrize("name", list(T.CASES))
def test_inference_walks_equal_one_tile_launches(UNet, name, materialize):
    """predict_device on 768 images == the concatenation of predict_device on their 48 sub-batches of 16, probabilities and every stored
    layer, on the default path (chains, LM_STEM, PRE; the *.c1 / *.ca layers) and under the materialize switch (every layer).  The first
    4 images of the WHOLE-batch result then go through test_inference_parity's bounds against the oracle: a reference run that is itself
    wrong cannot vouch for the walked one."""
    cfg = T.CASES[name]
    m, sd = build(UNet, cfg)
    x = images(cfg, T.INFER_BATCH)
    xd = torch.from_numpy(x).cuda()
    m.debug(materialize=materialize)
    try:
        names = stored_names(m, materialize)
        whole = forward_with_layers(m, xd, names, drop_unwritten=not materialize)
        names = [n for n in whole if n != "probs"]
        if not materialize:
            MEASURED["layers"].setdefault("default_path_keeps_on_chip", {})[name] = " ".join(sorted(set(stored_names(m, False)) - set(names)))
        if materialize:
            record_layers("inference", name, {n: whole[n] for n in names})
        assert_equals_sub_batches(whole, lambda lo, hi: forward_with_layers(m, xd[lo:hi], names), T.INFER_BATCH, T.SUB_BATCH,
                                  f"{name}, {'materialize' if materialize else 'default path'}")
    finally:
        m.debug(materialize=False)
    taps = {}
    ref = U.forward(sd, x[:4], cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], emulate_fp16=True, taps=taps).numpy()
    TU.assert_probability_bounds(whole["probs"][:4].cpu().numpy(), ref, cfg["act"])
    for n in names:       # ... and the stored layers of those 4 images, by the layer bound of test_inference_parity
        TU.assert_layer_bound(whole[n][:4].float().cpu().numpy(), taps[n].numpy(), n)


@pytest.mark.parametrize("name", list(T.CASES) + ["one_tile"])
def test_tile_counters_start_at_zero_each_call(UNet, name):
    """Three whole-batch forwards in a row on the same workspace give identical results, a fourth on a second stream does too: the
    dynamic walk's tile counters are zeroed by every call on its own stream (csrc/imk_unet.hip, "the tile counters of this forward's
    launches").  Between the calls the workspace is left alone, so every counter sits at its end value when the next call starts, and only
    the output and the stored layers' slots are filled with NaN (forward_with_layers): without the reset the tickets of the second call
    start past the end of every group's range, the tiles behind the statically assigned first ones stay unwritten, and the NaNs
    fail the comparison."""
    if name == "one_tile":
        cfg, batch = dict(T.ONE_TILE, alpha=1.0), T.ONE_TILE_BATCHES[-1]
    else:
        cfg, batch = T.CASES[name], T.INFER_BATCH
    m, _ = build(UNet, cfg)
    xd = torch.from_numpy(images(cfg, batch)).cuda()
    names = stored_names(m, False)
    first = forward_with_layers(m, xd, names, drop_unwritten=True)
    names = [n for n in first if n != "probs"]
    ws = m.workspace(batch, 0)
    for call in (2, 3):
        again = forward_with_layers(m, xd, names)
        assert m.workspace(batch, 0) is ws
        for n in first:
            assert torch.equal(first[n], again[n]), (call, T.first_mismatch(n, again[n], first[n]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fourth = forward_with_layers(m, xd, names)
    side.synchronize()
    for n in first:
        assert torch.equal(first[n], fourth[n]), ("second stream", T.first_mismatch(n, fourth[n], first[n]))


@pytest.mark.parametrize("batch", T.ONE_TILE_BATCHES)
@pytest.mark.parametrize("alpha", T.ONE_TILE_ALPHAS)
def test_one_tile_images_around_the_dynamic_walks_threshold(UNet, alpha, batch):
    """16 x 16 images: n_tiles == batch at levels 0 and 1.  2040 and 2047 tiles take the static walk, 2048, 2049 and 2080 the dynamic one
    (32 groups of ceil(n / 32) tiles, the grid rounded down to a multiple of 32: at 2048 tiles and full occupancy every tile is a
    statically assigned first one and the tickets hand out none, at 2049 and 2080 each group's range has one more tile than that, and
    below full occupancy the tickets hand out the larger part).  Each equals
    its sub-batches of 256 (B = 2049: eight of 256 and one of 1), on both paths, and the first 4 images meet the oracle."""
    cfg = dict(T.ONE_TILE, alpha=alpha)
    m, sd = build(UNet, cfg)
    x = images(cfg, T.ONE_TILE_BATCHES[-1])[:batch]
    xd = torch.from_numpy(x).cuda()
    ref = U.forward(sd, x[:4], cfg["c"], cfg["k"], alpha, cfg["act"], emulate_fp16=True).numpy()
    for materialize in (False, True):
        m.debug(materialize=materialize)
        try:
            names = stored_names(m, materialize)
            whole = forward_with_layers(m, xd, names, drop_unwritten=not materialize)
            names = [n for n in whole if n != "probs"]
            assert_equals_sub_batches(whole, lambda lo, hi: forward_with_layers(m, xd[lo:hi], names), batch, T.ONE_TILE_SUB,
                                      f"one_tile alpha {alpha} batch {batch} materialize {materialize}")
        finally:
            m.debug(materialize=False)
        # the oracle ties in: the first 4 images of the whole-batch result, by test_inference_parity's bounds
        TU.assert_probability_bounds(whole["probs"][:4].cpu().numpy(), ref, cfg["act"])


# ---- the fused consumers of the same forward -----------------------------------------------------------------------------------------------
def _ensemble_im(models, batch, n_streams):
    """functions.EnsembleIM with a workspace sized for n_streams concurrent models (imk_unet_forward_im takes the stream count from it)"""
    from inconsistencymasks_amd import functions as F
    from inconsistencymasks_amd._lib import lib
    ens = F.EnsembleIM(models)
    nbytes = lib.imk_unet_forward_im_workspace_bytes(ens.plan.ptr, len(models), batch, n_streams)
    assert nbytes > 0
    ens._ws, ens._ws_batch = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), batch
    ens.sized_for = (nbytes, ens._ws.data_ptr())          # im_outputs checks that run() kept this workspace, i.e. this stream count
    return ens


@pytest.mark.parametrize("name", ["pair", "plain16"])
def test_fused_consumers_walk_like_their_sub_batches(UNet, name):
    """imk_unet_forward_im (through functions.EnsembleIM, 1 and 2 streams), imk_unet_forward_vote (hard and soft) and
    imk_unet_forward_student run the same forward; two models, B = 768: every output equals its 16-image sub-batch outputs."""
    import test_gpu_model_ensemble as ME
    import test_gpu_noisy_student as NS
    from inconsistencymasks_amd import noisy_student
    cfg = T.CASES[name]
    models = [build(UNet, cfg, seed=50 + 3 * j)[0] for j in range(2)]
    B, S = T.INFER_BATCH, T.SUB_BATCH
    xd = torch.from_numpy(images(cfg, B, seed=51)).cuda()
    soft = cfg["act"] == "softmax"
    keys = ["img_out", "masks", "im", "im_size"] + (["presence"] if soft else ["pred_size"])

    def im_outputs(ens, lo, hi):
        r = ens.run(xd[lo:hi], 0.5, False, True, True, want_presence=soft)
        assert (ens._ws.numel(), ens._ws.data_ptr()) == ens.sized_for, "EnsembleIM replaced the workspace: the stream count is no longer the test's"
        out = {k: r[k] for k in keys}
        out["masks"] = r["masks"].permute(0, 2, 3, 1)                # [b, Kb, h, w] -> pixels first, as first_mismatch reads them
        if soft:
            out["presence"] = r["presence"].permute(1, 0, 2)       # [n, b, K] -> image first
        return out
    for n_streams in (1, 2):
        whole = im_outputs(_ensemble_im(models, B, n_streams), 0, B)
        assert 0 < int(whole["im_size"].sum()) < B * cfg["h"] * cfg["w"]          # the models disagree somewhere, not everywhere
        sub = _ensemble_im(models, S, n_streams)
        assert_equals_sub_batches(whole, lambda lo, hi: im_outputs(sub, lo, hi), B, S, f"{name}: forward_im, {n_streams} stream(s)")
    pixels_first = (lambda t: t) if soft else (lambda t: t.permute(0, 2, 3, 1))      # sigmoid heads: labels [b, K, h, w]
    for soft_vote in (False, True):
        vote = lambda lo, hi: {"labels": pixels_first(ME._forward_vote(models, xd[lo:hi], 0.5, soft_vote, 2))}  # noqa: E731
        assert_equals_sub_batches(vote(0, B), vote, B, S, f"{name}: forward_vote, soft {soft_vote}")
    from inconsistencymasks_amd import _lib
    prm = NS.params([(0, i % 2, 0) for i in range(B)], 77)
    img = xd.flip(-1).contiguous() if cfg["c"] == 3 else xd
    for j, model in enumerate(models):
        tl = noisy_student.TeacherLabel(model, not soft)

        def student(lo, hi):
            out, lab = tl.run(xd[lo:hi], img[lo:hi], (_lib.AugParams * (hi - lo))(*prm[lo:hi]), 0.5, False)
            return {"img_out": out, "labels": pixels_first(lab)}
        whole = student(0, B)
        assert len(torch.unique(whole["labels"])) > 1
        assert_equals_sub_batches(whole, student, B, S, f"{name}: forward_student, model {j}")


def test_evalnet_walks_equal_one_tile_launches():
    """EvalNet `isic` of tests/test_gpu_evalnet.py (64 x 64: 16 tiles per image) at B = 320 = 5120 tiles against sub-batches of 16 = 256
    tiles: the stored tower layers bit for bit, the outputs within the 1e-6 test_inference_parity there uses for batch invariance."""
    from tests import test_gpu_evalnet as TE
    cfg = dict(TE.CFGS[T.EVALNET_CASE], b=T.EVALNET_BATCH)
    assert (cfg["h"], cfg["w"]) == T.EVALNET_HW           # the size the case table's tile counts are for
    m, _, xa, xb, _ = TE.make(cfg, 21)
    assert not np.array_equal(xa[0], xa[1])
    xa, xb = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    names = stored_names(m, True, skip=("dense", "iou", "detection"))

    def run(lo, hi):
        out = m.predict_device(xa[lo:hi], xb[lo:hi])
        layers = {n: v.clone() for n, v in layer_views(m, hi - lo, 0, names).items()}
        return out, layers
    m.debug(materialize=True)
    try:
        out, whole = run(0, T.EVALNET_BATCH)
        outs = []

        def sub(lo, hi):
            o, layers = run(lo, hi)
            outs.append(o)
            return layers
        assert_equals_sub_batches(whole, sub, T.EVALNET_BATCH, T.EVALNET_SUB, "EvalNet isic")
    finally:
        m.debug(materialize=False)
    gap = float((torch.cat(outs[:T.EVALNET_BATCH // T.EVALNET_SUB]) - out).abs().max())
    assert bool(torch.isfinite(out).all()) and gap <= 1e-6, gap


# ---- training: replicas ----------------------------------------------------------------------------------------------------------------------
def _bn_input(bn_name):
    """the conv whose output a BatchNorm layer normalises (unet.py: in.c -> in.bn, X.c1 -> X.bn / X.bnb, X.ca -> X.bna)"""
    stem, kind = bn_name.rsplit(".", 1)
    return stem + {"bn": ".c" if stem == "in" else ".c1", "bna": ".ca", "bnb": ".c1"}[kind]


def _tensor_gaps(m, ga, gb):
    out = {}
    for l in m.plan.layers:
        n = l["cout"] if l["kind"] else l["ksize"] ** 2 * l["cin"] * l["cout"]
        a, b = ("gamma", "beta") if l["kind"] else ("w", "b")
        out[f"{l['name']}.{a}"] = TU.rel_l2(ga[l["off_w"]:l["off_w"] + n].numpy(), gb[l["off_w"]:l["off_w"] + n].numpy())
        out[f"{l['name']}.{b}"] = TU.rel_l2(ga[l["off_b"]:l["off_b"] + l["cout"]].numpy(), gb[l["off_b"]:l["off_b"] + l["cout"]].numpy())
    return out


@pytest.mark.parametrize("name", list(T.CASES))
def test_training_step_on_replicas(UNet, name):
    """x, y = 96 copies of a 4-image batch b0; one fwd_bwd from a fresh state under the dynamic loss scale (first_finite_step).

    Forward, bit for bit.  A tile's conv output depends only on its input tile, the weights and the batch statistics, and the statistics
    are shared by the whole batch, so every stored training-mode conv output of replica r equals replica 0's, for every layer and r.
    This does not hide a defect of the loop-carried path: within a group's tile range the first `step` tiles are first iterations and
    all others are later ones, and with 15 tiles per image and 96 replicas every in-image tile position occurs both as a first and as a
    later iteration (tests/test_cpu_tile_walk_cases.py), so a stale prefetch or a wrong q / r step breaks the identity.

    Against the oracle on b0.  The mean loss and the mean-loss gradients of 96 identical replicas are those of b0: unet_oracle.train_step
    on b0, its forward values pinned to replica 0's stored activations, at the GPU step's loss scale (halved for both while the
    oracle's 96 x larger per-pixel gradients overflow fp16), through the bounds of train_step_parity.  One term does depend on the pixel
    count: the moving variance takes the Bessel-corrected batch variance, n / (n - 1), and n is 96 x larger here --
    1.7 % of the batch variance at the bottom level's 60 pixels.  The oracle's moving variance is restated for 96 n before it is compared.

    What this does not pin.  Sums over tiles -- the weight gradients, the statistics rows, the dgrad's effect on earlier layers -- are
    checked in aggregate only, at 2e-2 rel-L2 per tensor: a defect touching one tile in 5760 stays invisible; one tied to a walk position
    (every workgroup's second tile, its last one, the tile after an image boundary) touches at least a 1 / 8 share here and does not.
    The per-element sharpness is in the forward.  Recorded, not asserted: the per-tensor rel-L2 between this step's gradients and a
    plain GPU step on b0 (two implementations of the code under test cannot bound each other)."""
    cfg = dict(T.CASES[name], b=T.TRAIN_B0)
    c, k, alpha, act = cfg["c"], cfg["k"], cfg["alpha"], cfg["act"]
    m = UNet(cfg["h"], cfg["w"], c, k, alpha, act, seed=11)
    sd = TU.randomize_bn(m.state_dict(), 12)
    m.load_state_dict(sd)
    x0, y0, tgt0 = TU.make_input(cfg, 13)
    R, B = T.TRAIN_REPLICAS, T.TRAIN_BATCH
    x, y = np.tile(x0, (R, 1, 1, 1)), np.tile(y0, (R,) + (1,) * (y0.ndim - 1))
    assert x.shape[0] == B and np.array_equal(x[4 * 37:4 * 38], x0) and np.array_equal(y[4 * 95:], y0)
    kind = 0 if cfg["loss"] == "mse" else 1
    names = stored_names(m, True)
    scale = 32768.0
    while True:
        stats = TU.first_finite_step(m, sd, x, y, kind, scale)
        g1 = m.grads.clone()
        moving_after_1 = m.state_dict()
        views = layer_views(m, B, 1, names)
        record_layers("training", name, views)
        reps = {n: v.reshape(R, T.TRAIN_B0, *v.shape[1:]) for n, v in views.items()}
        bad = torch.stack([(reps[n] != reps[n][:1]).any() for n in names]).cpu().numpy()
        if bad.any():
            n = names[int(np.argmax(bad))]
            pytest.fail(f"{name}: training-mode {n} differs between replicas: "
                        f"{T.first_mismatch(n, views[n], views[n][:T.TRAIN_B0].repeat(R, 1, 1, 1))}; layers: {[q for q, f in zip(names, bad) if f]}")
        ov = {n: v[:T.TRAIN_B0].float().cpu() for n, v in views.items()}
        assert all(float(t.abs().max()) > 0 for t in ov.values())
        # deterministic: a second pass from the same state gives bit-identical gradients
        m.fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), kind)
        assert torch.equal(g1, m.grads)
        sd_ref = {kk: v.clone() for kk, v in sd.items()}
        loss_ref, grads_ref = U.train_step(sd_ref, U.new_opt_state(sd_ref), x0, tgt0, c, k, alpha, act, cfg["loss"], emulate_fp16=True,
                                           loss_scale=float(stats[2]), return_grads=True, override=ov)
        if all(bool(torch.isfinite(v).all()) for v in grads_ref.values()):
            break
        scale = float(stats[2]) / 2       # as train_step_parity: a step the oracle cannot follow is skipped by both
        assert scale >= 1.0
        m.load_state_dict(sd)
    for kk in sd_ref:                     # the moving variance for 96 n pixels instead of n
        if kk.endswith(".var"):
            n_px = int(np.prod(ov[_bn_input(kk[:-4])].shape[:3]))
            r = (R * n_px / (R * n_px - 1)) / (n_px / (n_px - 1))
            v_ref, v_0 = sd_ref[kk].double(), sd[kk].double()
            sd_ref[kk] = (v_ref + (v_ref - U.BN_MOMENTUM * v_0) * (r - 1)).float()
    # recorded first, so that a failing bound still leaves the figures: a plain GPU step on b0 at the same loss scale
    m0 = UNet(cfg["h"], cfg["w"], c, k, alpha, act, seed=11)
    m0.load_state_dict(sd)
    stats0 = TU.first_finite_step(m0, sd, x0, y0, kind, float(stats[2]))
    gaps = _tensor_gaps(m, g1.cpu(), m0.grads.cpu())
    MEASURED["training"][name] = dict(loss_scale=float(stats[2]), loss_scale_b0=float(stats0[2]), loss=float(stats[0]), loss_b0=float(stats0[0]),
                                      loss_oracle=float(loss_ref), grads_vs_plain_b0_step=gaps)
    print(f"tile walks, training {name}: scale {stats[2]:g}, loss {stats[0]:.6f} (b0 step {stats0[0]:.6f}, oracle {loss_ref:.6f}); "
          f"gradients vs the plain b0 step, worst rel-L2 {max(gaps.values()):.3e} ({max(gaps, key=gaps.get)})")
    TU.assert_step_bounds(m, stats, g1, moving_after_1, loss_ref, grads_ref, sd_ref)
