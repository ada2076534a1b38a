"""The C ABI's buffer contract (include/imk.h, "Buffers"), checked on the GPU with guard bands and poisoned workspaces (tests/arena.py):

  * nothing outside [ptr, ptr + bytes) of any argument is written (64 KiB guards on both sides of every buffer, every size exactly
    what the library's *_bytes query returns);
  * `const` arguments are not modified;
  * outputs do not depend on what workspaces and outputs held on entry (three fills: 0x00, 0xFF, 0x3C), which also proves that
    every output byte is written;
  * a workspace one byte too small is refused with IMK_EWORKSPACE before anything is written;
  * the 0x00-fill outputs equal what the Python wrappers (the product path) return for the same inputs.

Every comparison is bit-exact; these are self-comparisons, there is no oracle and no tolerance.  The calls go through
inconsistencymasks_amd._lib.lib with arena pointers: the wrappers allocate their own buffers.

Not visible to this method: out-of-range READS whose values never reach an output (a clamped or speculative load whose result is
masked away), and an overrun that jumps a whole 64 KiB guard and lands inside the workspace, which is exempt from the comparison.

Where the header lets a call get along with less than the query returns (imk_unet_forward_im / _vote: the unfused route's smaller
slabs, fewer streams; imk_unet_forward_views_vote: smaller image chunks), "one byte too small" is one byte below the smallest
size the header states."""
import ctypes
import hashlib
import os
import random
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

import arena as A  # noqa: E402

IMK_OK, IMK_EWORKSPACE = 0, -3
_CACHE = {}


def L():
    from inconsistencymasks_amd._lib import lib
    return lib


def S():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).cuda().contiguous()


def up256(n):
    return (n + 255) // 256 * 256


def same(snap, want, what):
    """a snapshot (uint8) against a product-path tensor of any dtype, bit for bit"""
    w = A.as_bytes(want).to(snap.device)
    assert snap.numel() == w.numel(), (what, snap.numel(), w.numel())
    if not torch.equal(snap, w):
        d = torch.nonzero(snap != w)[:, 0]
        raise AssertionError(f"{what}: {d.numel()} byte(s) differ from the wrapper path, first at +{int(d[0])}")


def randomize_bn(sd, seed):
    """tests/test_gpu_unet.py::randomize_bn"""
    from tests.test_gpu_unet import randomize_bn as r
    return r(sd, seed)


# ---- U-Net shapes: (h, w, c, k, alpha, head), the smallest that reach every conv family and edge ------------------------------------
SHAPES = [
    (16, 16, 3, 3, 1.0, "softmax"),      # one tile per image, 1 x 1 pixels at the bottom
    (48, 80, 3, 1, 0.5, "sigmoid"),      # pair layout, LM_STEM, prestage, partial tiles below full resolution
    (48, 80, 3, 35, 1.25, "softmax"),    # 20 / 40 / ... channels, two class tiles
    (48, 32, 1, 2, 1.75, "sigmoid"),     # wide kernel with a partly filled channel tile, one input channel
    (32, 48, 3, 1, 2.0, "sigmoid"),      # GEMM-class kernels, 512-channel bottleneck
    (32, 32, 3, 19, 2.0, "softmax"),
]
BATCHES = (1, 3)
SB = [(s, b) for s in SHAPES for b in BATCHES]
SB_IDS = [f"{s[0]}x{s[1]}c{s[2]}k{s[3]}a{s[4]}-b{b}" for s, b in SB]
S_IDS = [f"{s[0]}x{s[1]}c{s[2]}k{s[3]}a{s[4]}" for s in SHAPES]
ISIC = (256, 256, 3, 1, 0.5, "sigmoid")


def unet(cfg, seed=1):
    """a model with perturbed BatchNorm statistics, ready for inference (cached: the tests never change a cached model's weights)"""
    from inconsistencymasks_amd.unet import UNet
    key = ("unet", cfg, seed)
    if key not in _CACHE:
        m = UNet(*cfg, seed=seed)
        m.load_state_dict(randomize_bn(m.state_dict(), seed + 1))
        m.ready_for_inference()
        torch.cuda.synchronize()
        _CACHE[key] = m
    return _CACHE[key]


def images(cfg, b, seed=0):
    rng = np.random.default_rng(1000 * seed + cfg[0] * 7 + cfg[3] + b)
    return dev(rng.integers(0, 256, (b, cfg[0], cfg[1], cfg[2]), dtype=np.uint8))


def model_specs(models):
    specs = []
    for j, m in enumerate(models):
        specs += [(f"params{j}", m.params, "in"), (f"packed{j}", m.packed, "in")]
    return specs


def ptr_arrays(p, n):
    return ((ctypes.c_void_p * n)(*[p[f"params{j}"] for j in range(n)]), (ctypes.c_void_p * n)(*[p[f"packed{j}"] for j in range(n)]))


def Arena(specs, device="cuda"):
    """the workspace first, then the outputs, the inputs last: what runs past the end of the workspace's last tensor or of an
    output by more than a guard lands in a buffer that is compared or checked, not in the exempt workspace"""
    order = {"scratch": 0, "out": 1, "inout": 2, "in": 3}
    return A.Arena(sorted(specs, key=lambda t: order[t[2]]), device)


def refused(ar, call):
    """the call with a workspace one byte too small: IMK_EWORKSPACE and an arena that is entirely unchanged"""
    ar.run(0x3C, call, want_rc=IMK_EWORKSPACE, untouched=True)


# ---- imk_unet_pack_weights / imk_unet_forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", SHAPES, ids=S_IDS)
def test_pack_weights(cfg):
    """imk_unet_pack_weights, and a forward on what it packed in the same run: no byte of `packed` that a kernel reads is left
    to the fill"""
    b = 2
    m, x = unet(cfg), images(cfg, b)
    n = m.plan.workspace_bytes(b, 0)
    ar = Arena([("params", m.params, "in"), ("x", x, "in"), ("packed", m.plan.packed_bytes, "out"),
                  ("probs", b * cfg[0] * cfg[1] * cfg[3] * 4, "out"), ("ws", n, "scratch")], "cuda")

    def call(p):
        rc = L().imk_unet_pack_weights(m.plan.ptr, p["params"], p["packed"], S())
        return rc or L().imk_unet_forward(m.plan.ptr, p["params"], p["packed"], p["x"], b, p["probs"], p["ws"], n, S())
    out = ar.check(call)
    same(out["packed"], m.packed, "packed")
    same(out["probs"], m.predict_device(x), "probs")


def forward_arena(m, x, b, ws_bytes):
    return Arena([("params", m.params, "in"), ("packed", m.packed, "in"), ("x", x, "in"),
                    ("probs", b * m.plan.h * m.plan.w * m.plan.n_out * 4, "out"), ("ws", ws_bytes, "scratch")], "cuda")


def forward_call(m, b, ws_bytes):
    return lambda p: L().imk_unet_forward(m.plan.ptr, p["params"], p["packed"], p["x"], b, p["probs"], p["ws"], ws_bytes, S())


@pytest.mark.parametrize("cfg,b", SB, ids=SB_IDS)
def test_forward(cfg, b):
    m, x = unet(cfg), images(cfg, b)
    n = m.plan.workspace_bytes(b, 0)
    out = forward_arena(m, x, b, n).check(forward_call(m, b, n))
    same(out["probs"], m.predict_device(x), "probs")
    refused(forward_arena(m, x, b, n - 1), forward_call(m, b, n - 1))


@pytest.mark.parametrize("cfg", [SHAPES[1], SHAPES[2], SHAPES[4]], ids=[S_IDS[1], S_IDS[2], S_IDS[4]])
def test_forward_materialize(cfg):
    """inference with the plan's materialize switch: the fused kernels' intermediates are stored too"""
    b = 3
    m, x = unet(cfg), images(cfg, b)
    m.debug(materialize=True)
    try:
        want = m.predict_device(x)
        torch.cuda.synchronize()
        n = m.plan.workspace_bytes(b, 0)
        out = forward_arena(m, x, b, n).check(forward_call(m, b, n))
    finally:
        m.debug(materialize=False)
    same(out["probs"], want, "probs")


def test_forward_many_tiles():
    """ISIC 256 x 256, alpha 0.5, batch 8: 2048 tiles, the dynamic walk with its tile counters"""
    b = 8
    m, x = unet(ISIC), images(ISIC, b)
    n = m.plan.workspace_bytes(b, 0)
    out = forward_arena(m, x, b, n).check(forward_call(m, b, n))
    same(out["probs"], m.predict_device(x), "probs")


# ---- training: imk_unet_state_init / imk_unet_fwd_bwd / imk_unet_adamw_step ---------------------------------------------------------
@pytest.mark.parametrize("cfg", [SHAPES[0], SHAPES[4]], ids=[S_IDS[0], S_IDS[4]])
def test_state_init(cfg):
    m = unet(cfg)
    ar = Arena([("state", m.plan.state_bytes, "out")], "cuda")
    out = ar.check(lambda p: L().imk_unet_state_init(m.plan.ptr, p["state"], S()))
    st = torch.empty(m.plan.state_bytes, dtype=torch.uint8, device="cuda")
    assert L().imk_unet_state_init(m.plan.ptr, st.data_ptr(), S()) == 0
    same(out["state"], st, "state")


def fresh_trainee(cfg, seed=3):
    """a model of its own (training changes it), packed, with an initialised optimizer state"""
    from inconsistencymasks_amd.unet import UNet
    m = UNet(*cfg, seed=seed)
    m.load_state_dict(randomize_bn(m.state_dict(), seed + 1))
    m.repack()
    m.init_train_state()
    torch.cuda.synchronize()
    return m


def targets(cfg, b, seed=0):
    rng = np.random.default_rng(77 + seed + cfg[0] + b)
    if cfg[5] == "sigmoid":
        return dev(rng.integers(0, 2, (b, cfg[0], cfg[1], cfg[3]), dtype=np.uint8)), 0
    return dev(rng.integers(0, cfg[3], (b, cfg[0], cfg[1]), dtype=np.uint8)), 1


def check_fwd_bwd(cfg, b):
    """two consecutive steps inside one arena run: the second sees the first one's workspace as its stale content.  grads is an
    output like any other: the header states no precondition on it, so it gets the fill."""
    m = fresh_trainee(cfg)
    x = images(cfg, b, 1)
    y, kind = targets(cfg, b)
    nt, n = m.plan.n_trainable, m.plan.workspace_bytes(b, 1)
    params0 = m.params.clone()

    def arena(ws_bytes):
        return Arena([("params", params0, "inout"), ("packed", m.packed, "inout"), ("state", m.train_state, "inout"), ("x", x, "in"),
                        ("y", y, "in"), ("grads", nt * 4, "out"), ("stats", 16, "out"), ("ws", ws_bytes, "scratch")], "cuda")

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
    # only the moving statistics move
    assert torch.equal(out["params"][:nt * 4], A.as_bytes(params0)[:nt * 4]), "imk_unet_fwd_bwd changed a trainable parameter"
    assert not torch.equal(out["params"][nt * 4:], A.as_bytes(params0)[nt * 4:]), "the moving statistics did not move"
    refused(arena(n - 1), step(n - 1))
    m.fwd_bwd(x, y, kind)
    m.fwd_bwd(x, y, kind)
    torch.cuda.synchronize()
    same(out["grads"], m.grads, "grads")
    same(out["stats"], m.stats[:3], "stats[0:3]")
    same(out["params"], m.params, "params")
    same(out["state"], m.train_state, "state")
    same(out["packed"], m.packed, "packed")
    return m


@pytest.mark.parametrize("cfg,b", SB, ids=SB_IDS)
def test_fwd_bwd_two_steps(cfg, b):
    check_fwd_bwd(cfg, b)


def test_fwd_bwd_many_tiles():
    """ISIC 256 x 256, alpha 0.5, batch 12: 3072 tiles, more than any launch grid -- workgroups walk several tiles and write
    several partial rows"""
    check_fwd_bwd(ISIC, 12)


@pytest.mark.parametrize("cfg", SHAPES, ids=S_IDS)
def test_adamw_step(cfg):
    b = 3
    m = fresh_trainee(cfg, seed=5)
    x = images(cfg, b, 2)
    y, kind = targets(cfg, b, 1)
    for _ in range(16):          # until the dynamic loss scale lets a step through
        m.fwd_bwd(x, y, kind)
        torch.cuda.synchronize()
        if float(m.stats[1]) == 0.0:
            break
        m.adamw_step(3e-3, 1e-4)
    assert float(m.stats[1]) == 0.0
    ar = Arena([("params", m.params, "inout"), ("packed", m.packed, "inout"), ("state", m.train_state, "inout"),
                  ("grads", m.grads.clone(), "in"), ("stats", m.stats.clone(), "in")], "cuda")
    out = ar.check(lambda p: L().imk_unet_adamw_step(m.plan.ptr, p["params"], p["packed"], p["state"], p["grads"], p["stats"], 1.0,
                                                     3e-3, 1e-4, 0.9, 0.999, 1e-7, S()))
    before = m.params.clone()
    m.adamw_step(3e-3, 1e-4)
    torch.cuda.synchronize()
    assert not torch.equal(before, m.params)
    same(out["params"], m.params, "params")
    same(out["packed"], m.packed, "packed")
    same(out["state"], m.train_state, "state")


# ---- ensembles: imk_unet_forward_im / imk_unet_forward_vote ------------------------------------------------------------------------
N_MODELS = 3


def ensemble(cfg):
    return [unet(cfg, seed=11 + 10 * j) for j in range(N_MODELS)]


def im_min_bytes(plan, n, b):
    """the smallest workspace the header states for imk_unet_forward_im / _vote: n probability slabs (or the fused route's
    activation slabs where those are not larger) + one activation workspace"""
    fused = L().imk_unet_forward_im_workspace_bytes(plan.ptr, n, b, 1)
    unfused = n * up256(b * plan.h * plan.w * plan.n_out * 4) + plan.workspace_bytes(b, 0)
    return min(fused, unfused)


def im_arena(models, x, b, ws_bytes, binary):
    p = models[0].plan
    kb = p.n_out if binary else 1
    specs = model_specs(models) + [("x", x, "in"), ("img_out", x.numel(), "out"), ("masks", b * kb * p.h * p.w, "out"),
                                   ("im", b * p.h * p.w, "out"), ("im_size", b * kb * 8, "out"), ("pred_size", b * kb * 8, "out")]
    if not binary:
        specs.append(("presence", len(models) * b * p.n_out, "out"))
    return Arena(specs + [("ws", ws_bytes, "scratch")], "cuda")


def im_call(models, b, ws_bytes, binary):
    plan, n = models[0].plan, len(models)

    def call(p):
        pa, pk = ptr_arrays(p, n)
        return L().imk_unet_forward_im(plan.ptr, n, pa, pk, p["x"], b, 0.5, 0, p["x"], 1, 1, p["img_out"], p["masks"], p["im"],
                                       p["im_size"], p["pred_size"], None if binary else p["presence"], p["ws"], ws_bytes, S())
    return call


@pytest.mark.parametrize("n_streams", [1, 2, 3])
@pytest.mark.parametrize("cfg,b", SB, ids=SB_IDS)
def test_forward_im(cfg, b, n_streams):
    from inconsistencymasks_amd import functions as F
    models, x = ensemble(cfg), images(cfg, b)
    plan, binary = models[0].plan, cfg[5] == "sigmoid"
    n = L().imk_unet_forward_im_workspace_bytes(plan.ptr, N_MODELS, b, n_streams)
    unwritten = () if binary else ("pred_size",)          # include/imk.h: pred_size unused for softmax heads
    keys = ("img_out", "masks", "im", "im_size") + (("pred_size",) if binary else ("presence",))
    for route in ("fused", "unfused"):      # the wrapper under the same switch: it changes which conv kernels run as well
        for m in models:
            m.debug(materialize=route == "unfused")
        try:
            want = F.EnsembleIM(models).run(x, 0.5, False, True, True, want_presence=not binary)
            torch.cuda.synchronize()
            out = im_arena(models, x, b, n, binary).check(im_call(models, b, n, binary), unwritten=unwritten)
        finally:
            for m in models:
                m.debug(materialize=False)
        for key in keys:
            same(out[key], want[key], f"{route} {key}")
    want = F.EnsembleIM(models).run(x, 0.5, False, True, True, want_presence=not binary)
    torch.cuda.synchronize()
    if n_streams == 1:
        lo = im_min_bytes(plan, N_MODELS, b)
        refused(im_arena(models, x, b, lo - 1, binary), im_call(models, b, lo - 1, binary))
        if lo < n:       # the smaller workspace the header allows: the unfused route, with the guard right behind it
            out = im_arena(models, x, b, lo, binary).check(im_call(models, b, lo, binary), unwritten=unwritten)
            for key in keys:     # bit-identical to the fused route (include/imk.h)
                same(out[key], want[key], f"small-workspace {key}")


def vote_arena(models, x, b, ws_bytes, binary):
    p = models[0].plan
    return Arena(model_specs(models) + [("x", x, "in"), ("masks", b * (p.n_out if binary else 1) * p.h * p.w, "out"),
                                          ("ws", ws_bytes, "scratch")], "cuda")


def vote_call(models, b, ws_bytes, mode):
    plan, n = models[0].plan, len(models)

    def call(p):
        pa, pk = ptr_arrays(p, n)
        return L().imk_unet_forward_vote(plan.ptr, n, pa, pk, p["x"], b, 0.5, mode, p["masks"], p["ws"], ws_bytes, S())
    return call


@pytest.mark.parametrize("cfg,b", SB, ids=SB_IDS)
def test_forward_vote(cfg, b):
    from inconsistencymasks_amd import vote as V
    models, x = ensemble(cfg), images(cfg, b)
    plan, binary = models[0].plan, cfg[5] == "sigmoid"
    n = L().imk_unet_forward_im_workspace_bytes(plan.ptr, N_MODELS, b, 3)
    ev = V.EnsembleVote(models)
    for mode in (0, 1):
        for route in ("fused", "unfused"):
            for m in models:
                m.debug(materialize=route == "unfused")
            try:
                want = ev.run(x, 0.5, bool(mode))
                torch.cuda.synchronize()
                out = vote_arena(models, x, b, n, binary).check(vote_call(models, b, n, mode))
            finally:
                for m in models:
                    m.debug(materialize=False)
            same(out["masks"], want, f"{route} mode {mode}")
    lo = im_min_bytes(plan, N_MODELS, b)
    refused(vote_arena(models, x, b, lo - 1, binary), vote_call(models, b, lo - 1, 0))


# ---- imk_unet_forward_views_vote ----------------------------------------------------------------------------------------------------
def view_plan(cfg, b, m_views, restore):
    from inconsistencymasks_amd import input_ensemble as IE
    random.seed(m_views + b)
    if restore:
        square = cfg[0] == cfg[1]
        per = []
        for i in range(b):
            views = IE.draw_random_views(m_views, np_rng=np.random.RandomState(i))
            for j, q in enumerate(views):      # rectangles cannot take a quarter turn: identity, the flips and the half turns
                if not square:
                    q.op = (0, 2, 5, 8, 11)[(i + j) % 5]
            per.append(views)
        return IE.ViewPlan(per, chain=False, restore=True)
    return IE.ViewPlan([IE.draw_chain_views(m_views - 1, np_rng=np.random.RandomState(i)) for i in range(b)], chain=True, restore=False)


@pytest.mark.parametrize("cfg,b", SB, ids=SB_IDS)
def test_forward_views_vote(cfg, b):
    from inconsistencymasks_amd import input_ensemble as IE
    m, x = unet(cfg), images(cfg, b)
    plan, binary, mv = m.plan, cfg[5] == "sigmoid", 4
    # (restore, mode, cmp_ge): ISIC's D4-restoring hard vote, the chain's hard / soft votes, the majority
    variants = [(True, 0, True), (False, 0, False), (False, 1, False)] if binary else [(False, 1, False), (False, 2, False)]
    n = L().imk_unet_forward_views_vote_workspace_bytes(plan.ptr, mv, b)
    lo = up256(mv * plan.h * plan.w * plan.n_out * 4) + plan.workspace_bytes(1, 0)      # one image per chunk
    vv = IE.ViewVote(m, binary)
    for restore, mode, ge in variants:
        vp = view_plan(cfg, b, mv, restore)
        views = IE.make_views(x, vp)
        want = vv.run(x, vp, 0.5, mode, ge)
        torch.cuda.synchronize()
        ops = dev(vp.ops) if restore else None

        def arena(ws_bytes):
            specs = [("params", m.params, "in"), ("packed", m.packed, "in"), ("views", views, "in")]
            if restore:
                specs.append(("ops", ops, "in"))
            return Arena(specs + [("masks", want.numel(), "out"), ("ws", ws_bytes, "scratch")], "cuda")

        def call(ws_bytes):
            return lambda p: L().imk_unet_forward_views_vote(plan.ptr, p["params"], p["packed"], p["views"], mv, b,
                                                             p["ops"] if restore else None, vp.quarter, 0.5, mode, int(ge), p["masks"],
                                                             p["ws"], ws_bytes, S())
        for ws_bytes in (n, n - 1, lo):       # the query's size; one byte less: smaller chunks; the least: one image per chunk
            if ws_bytes <= n:
                out = arena(ws_bytes).check(call(ws_bytes))
                same(out["masks"], want, f"restore {restore} mode {mode} workspace {ws_bytes}")
        m.debug(materialize=True)
        try:
            want_m = vv.run(x, vp, 0.5, mode, ge)
            torch.cuda.synchronize()
            out = arena(n).check(call(n))
        finally:
            m.debug(materialize=False)
        same(out["masks"], want_m, f"materialize, restore {restore} mode {mode}")
        if lo <= n:
            refused(arena(lo - 1), call(lo - 1))


# ---- imk_unet_forward_student -------------------------------------------------------------------------------------------------------
def student_inputs(cfg, b):
    from inconsistencymasks_amd import augment
    x = images(cfg, b)
    img = x.flip(-1).contiguous() if cfg[2] == 3 else images(cfg, b, 5)
    prm = augment.draw_params(b, rng=random.Random(b + cfg[3]), np_rng=np.random.RandomState(b), free_rotation=cfg[0] == cfg[1])
    return x, img, prm


def check_student(cfg, b, materialize=False):
    """-> the 0x00-fill outputs (img_out, labels) as uint8 tensors"""
    m = unet(cfg)
    plan, binary = m.plan, cfg[5] == "sigmoid"
    x, img, prm = student_inputs(cfg, b)
    quarter = int(any(q.rot in (1, 3) for q in prm))
    aug = torch.frombuffer(bytearray(bytes(prm)), dtype=torch.uint8).cuda()
    n = L().imk_unet_forward_student_workspace_bytes(plan.ptr, b)
    n_lab = b * (plan.n_out if binary else 1) * plan.h * plan.w

    def arena(ws_bytes):
        return Arena([("params", m.params, "in"), ("packed", m.packed, "in"), ("x", x, "in"), ("img", img, "in"), ("aug", aug, "in"),
                        ("img_out", img.numel(), "out"), ("labels", n_lab, "out"), ("ws", ws_bytes, "scratch")], "cuda")

    def call(ws_bytes):
        return lambda p: L().imk_unet_forward_student(plan.ptr, p["params"], p["packed"], p["x"], p["img"], b, 0.5, 0, p["aug"], quarter,
                                                      p["img_out"], p["labels"], p["ws"], ws_bytes, S())
    m.debug(materialize=materialize)
    try:
        out = arena(n).check(call(n))
    finally:
        m.debug(materialize=False)
    refused(arena(n - 1), call(n - 1))
    return out


@pytest.mark.parametrize("cfg,b", SB, ids=SB_IDS)
def test_forward_student(cfg, b):
    from inconsistencymasks_amd import noisy_student as NS
    m = unet(cfg)
    x, img, prm = student_inputs(cfg, b)
    for materialize in ((False, True) if b == 3 else (False,)):      # the fused route; the unfused one under the debug switch
        out = check_student(cfg, b, materialize)
        m.debug(materialize=materialize)
        try:
            w_img, w_lab = NS.TeacherLabel(m, cfg[5] == "sigmoid").run(x, img, prm, 0.5, False)
            torch.cuda.synchronize()
        finally:
            m.debug(materialize=False)
        same(out["img_out"], w_img, f"img_out (materialize {materialize})")
        same(out["labels"], w_lab, f"labels (materialize {materialize})")


def student_digest():
    h = hashlib.sha256()
    for cfg, b in SB:
        out = check_student(cfg, b)
        h.update(out["img_out"].cpu().numpy().tobytes())
        h.update(out["labels"].cpu().numpy().tobytes())
    return h.hexdigest()


def test_forward_student_unfused_switch_in_a_child_process():
    """IMK_STUDENT_FUSED=0 is read once per process: the same guard / poison checks in a child, and the same output bytes"""
    env = {**os.environ, "IMK_STUDENT_FUSED": "0"}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "student"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("student-digest ")]
    assert line and line[-1].split()[1] == student_digest(), r.stdout[-500:]


# ---- EvalNet ------------------------------------------------------------------------------------------------------------------------
EVAL = ["isic", "hela", "city"]
EB = 2


def evalnet(name, seed=21):
    from inconsistencymasks_amd.evalnet import EvalNet
    from tests.test_gpu_evalnet import CFGS
    cfg = CFGS[name]
    key = ("evalnet", name, seed)
    if key not in _CACHE:
        m = EvalNet(cfg["h"], cfg["w"], cfg["ca"], cfg["cb"], cfg["k"], cfg["alpha"], cfg["two"], cfg["na"], cfg["nb"], seed=seed,
                    b_onehot=cfg.get("onehot", False))
        m.load_state_dict(randomize_bn(m.state_dict(), seed + 1))
        m.ready_for_inference()
        torch.cuda.synchronize()
        _CACHE[key] = m
    return _CACHE[key], cfg


def eval_inputs(cfg, b, m_cand=None, seed=0):
    """xa [B,H,W,ca], xb [B,(M,)H,W,cb] or class ids [B,(M,)H,W,1], y [B,U]"""
    rng = np.random.default_rng(seed + cfg["h"] + b)
    lead = (b,) if m_cand is None else (b, m_cand)
    xa = rng.integers(0, 256, (b, cfg["h"], cfg["w"], cfg["ca"]), dtype=np.uint8)
    if cfg.get("onehot"):
        xb = rng.integers(0, cfg["cb"], lead + (cfg["h"], cfg["w"], 1), dtype=np.uint8)
    else:
        xb = (rng.integers(0, 2, lead + (cfg["h"], cfg["w"], cfg["cb"]), dtype=np.uint8) * 255).astype(np.uint8)
    u = (2 if cfg["two"] else 1) * cfg["k"]
    y = rng.random((b, u)).astype(np.float32)
    if cfg["two"]:
        y[:, cfg["k"]:] = y[:, cfg["k"]:] > 0.5
    return dev(xa), dev(xb), dev(y)


@pytest.mark.parametrize("name", EVAL)
def test_evalnet_forward(name):
    m, cfg = evalnet(name)
    xa, xb, _ = eval_inputs(cfg, EB)
    u = m.n_heads * m.plan.n_out
    n = m.plan.workspace_bytes(EB, 0)

    def arena(ws_bytes):
        return Arena([("params", m.params, "in"), ("packed", m.packed, "in"), ("xa", xa, "in"), ("xb", xb, "in"),
                        ("out", EB * u * 4, "out"), ("ws", ws_bytes, "scratch")], "cuda")

    def call(ws_bytes):
        return lambda p: L().imk_evalnet_forward(m.plan.ptr, p["params"], p["packed"], p["xa"], p["xb"], EB, p["out"], p["ws"], ws_bytes, S())
    out = arena(n).check(call(n))
    same(out["out"], m.predict_device(xa, xb), "out")
    refused(arena(n - 1), call(n - 1))
    m.debug(materialize=True)
    try:
        n2 = m.plan.workspace_bytes(EB, 0)
        out2 = arena(n2).check(call(n2))
        same(out2["out"], m.predict_device(xa, xb), "out under materialize")
    finally:
        m.debug(materialize=False)


@pytest.mark.parametrize("name", EVAL)
def test_evalnet_fwd_bwd_two_steps(name):
    from inconsistencymasks_amd.evalnet import EvalNet
    from tests.test_gpu_evalnet import CFGS
    cfg = CFGS[name]
    m = EvalNet(cfg["h"], cfg["w"], cfg["ca"], cfg["cb"], cfg["k"], cfg["alpha"], cfg["two"], cfg["na"], cfg["nb"], seed=31,
                b_onehot=cfg.get("onehot", False))
    m.load_state_dict(randomize_bn(m.state_dict(), 32))
    m.repack()
    m.init_train_state()
    torch.cuda.synchronize()
    xa, xb, y = eval_inputs(cfg, EB, seed=3)
    u, nt = m.n_heads * m.plan.n_out, m.plan.n_trainable
    n = m.plan.workspace_bytes(EB, 1)
    params0 = m.params.clone()

    def arena(ws_bytes):
        return Arena([("params", params0, "inout"), ("packed", m.packed, "inout"), ("state", m.train_state, "inout"), ("xa", xa, "in"),
                        ("xb", xb, "in"), ("y", y, "in"), ("out", EB * u * 4, "out"), ("grads", nt * 4, "out"), ("stats", 32, "out"),
                        ("ws", ws_bytes, "scratch")], "cuda")

    def step(ws_bytes):
        def call(p):
            for _ in range(2):
                rc = L().imk_evalnet_fwd_bwd(m.plan.ptr, p["params"], p["packed"], p["state"], p["xa"], p["xb"], p["y"], EB, p["out"],
                                             p["grads"], p["stats"], p["ws"], ws_bytes, S())
                if rc:
                    return rc
            return 0
        return call
    n_stats = 6 if cfg["two"] else 5       # include/imk.h: {total loss, overflow flag, loss scale, step, loss of head 0, loss of head 1}
    out = arena(n).check(step(n), ranges={"stats": (0, 4 * n_stats)})
    assert torch.equal(out["params"][:nt * 4], A.as_bytes(params0)[:nt * 4]), "imk_evalnet_fwd_bwd changed a trainable parameter"
    refused(arena(n - 1), step(n - 1))
    m.fwd_bwd(xa, xb, y)
    w_out = m.fwd_bwd(xa, xb, y)
    torch.cuda.synchronize()
    same(out["out"], w_out, "out")
    same(out["grads"], m.grads, "grads")
    same(out["stats"], m.stats[:n_stats], "stats")
    same(out["params"], m.params, "params")
    same(out["state"], m.train_state, "state")


def scorer_models(name):
    return [evalnet(name, seed=21 + 9 * j)[0] for j in range(2)]


@pytest.mark.parametrize("name", EVAL)
def test_evalnet_forward_candidates_and_select(name):
    from inconsistencymasks_amd import evalnet as EV
    models = scorer_models(name)
    _, cfg = evalnet(name)
    plan, mc, n = models[0].plan, 3, len(models)
    xa, xb, _ = eval_inputs(cfg, EB, mc, seed=5)
    if cfg.get("onehot"):
        xb = xb[..., 0].contiguous()
    u = models[0].n_heads * plan.n_out
    cand_bytes = cfg["h"] * cfg["w"]
    cand = dev(np.random.default_rng(8).integers(0, 256, (EB, mc, cand_bytes), dtype=np.uint8))
    nws = L().imk_evalnet_forward_candidates_workspace_bytes(plan.ptr, EB, mc)
    scorer = EV.CandidateScorer(models)
    w_scores = scorer.scores(xa, xb)
    torch.cuda.synchronize()
    mode = EV.SELECT_MIOU if cfg["two"] else EV.SELECT_IOU
    mean = w_scores.mean(0)
    thr = float(mean[..., :plan.n_out].mean())

    def arena(ws_bytes, select):
        specs = model_specs(models) + [("xa", xa, "in"), ("xb", xb, "in")]
        if select:
            specs += [("cand", cand, "in")]
        specs += [("scores", n * EB * mc * u * 4, "out")]
        if select:
            specs += [("best_idx", EB * 4, "out"), ("best_score", EB * 4, "out"), ("keep", EB, "out"), ("chosen", EB * cand_bytes, "out")]
        return Arena(specs + [("ws", ws_bytes, "scratch")], "cuda")

    def call_cand(ws_bytes):
        def call(p):
            pa, pk = ptr_arrays(p, n)
            return L().imk_evalnet_forward_candidates(plan.ptr, n, pa, pk, p["xa"], p["xb"], EB, mc, p["scores"], p["ws"], ws_bytes, S())
        return call

    def call_sel(ws_bytes):
        def call(p):
            pa, pk = ptr_arrays(p, n)
            return L().imk_evalnet_forward_select(plan.ptr, n, pa, pk, p["xa"], p["xb"], EB, mc, None, p["cand"], cand_bytes, thr, mode,
                                                  p["scores"], p["best_idx"], p["best_score"], p["keep"], p["chosen"], p["ws"], ws_bytes, S())
        return call
    out = arena(nws, False).check(call_cand(nws))
    same(out["scores"], w_scores, "scores")
    refused(arena(nws - 1, False), call_cand(nws - 1))
    out = arena(nws, True).check(call_sel(nws))
    bi, bs, keep, chosen = scorer.run(xa, xb, cand, thr, None, mode)
    torch.cuda.synchronize()
    for key, want in (("scores", scorer.last_scores), ("best_idx", bi), ("best_score", bs), ("keep", keep), ("chosen", chosen)):
        same(out[key], want, key)
    refused(arena(nws - 1, True), call_sel(nws - 1))


# ---- standalone kernels, at ragged sizes where the 16-byte store paths have tails ---------------------------------------------------
@pytest.mark.parametrize("n,b,h,w,kb,c", [(4, 2, 35, 21, 1, 3), (2, 3, 64, 48, 3, 1)])
def test_im_binary(n, b, h, w, kb, c):
    from inconsistencymasks_amd import im as IM
    rng = np.random.default_rng(h * w + n)
    base = rng.random((1, b, h, w, kb), dtype=np.float32)
    preds = np.clip(base + (rng.random((n, b, h, w, kb), dtype=np.float32) - 0.5) * 0.3, 0, 1).astype(np.float32)
    preds[0, 0, 0, :4, 0] = [0.5, np.nan, 0.50000006, 0.49999997]
    pd, img = dev(preds), dev(rng.integers(1, 256, (b, h, w, c), dtype=np.uint8))
    ge = int(kb == 3)
    ar = Arena([("preds", pd, "in"), ("img", img, "in"), ("img_out", img.numel(), "out"), ("masks", b * kb * h * w, "out"),
                  ("im", b * h * w, "out"), ("im_size", b * kb * 8, "out"), ("pred_size", b * kb * 8, "out")], "cuda")
    out = ar.check(lambda p: L().imk_im_binary(p["preds"], n, b, h, w, kb, 0.5, ge, p["img"], c, 1, 1, p["img_out"], p["masks"], p["im"],
                                               p["im_size"], p["pred_size"], S()))
    want = IM.im_binary(pd, 0.5, bool(ge), img, True, True)
    for key in ("img_out", "masks", "im", "im_size", "pred_size"):
        same(out[key], want[key], key)
    # no image: img_out is ignored
    ar = Arena([("preds", pd, "in"), ("masks", b * kb * h * w, "out"), ("im", b * h * w, "out"), ("im_size", b * kb * 8, "out"),
                  ("pred_size", b * kb * 8, "out")], "cuda")
    out = ar.check(lambda p: L().imk_im_binary(p["preds"], n, b, h, w, kb, 0.5, ge, None, 0, 1, 0, None, p["masks"], p["im"],
                                               p["im_size"], p["pred_size"], S()))
    same(out["masks"], IM.im_binary(pd, 0.5, bool(ge), None, True, False)["masks"], "masks without an image")


@pytest.mark.parametrize("n,b,h,w,k,c", [(3, 1, 17, 9, 4, 1), (2, 3, 13, 26, 35, 3)])
def test_im_multiclass(n, b, h, w, k, c):
    from inconsistencymasks_amd import im as IM
    rng = np.random.default_rng(k * 7 + h)
    base = rng.random((1, b, h, w, k), dtype=np.float32)
    probs = (base + 0.2 * rng.random((n, b, h, w, k), dtype=np.float32)).astype(np.float32)
    probs[:, :, : h // 3] = np.round(probs[:, :, : h // 3] * 3) / 3
    pd, img = dev(probs), dev(rng.integers(1, 256, (b, h, w, c), dtype=np.uint8))
    ar = Arena([("probs", pd, "in"), ("img", img, "in"), ("img_out", img.numel(), "out"), ("final", b * h * w, "out"),
                  ("im", b * h * w, "out"), ("im_size", b * 8, "out"), ("presence", n * b * k, "out")], "cuda")
    out = ar.check(lambda p: L().imk_im_multiclass(p["probs"], n, b, h, w, k, p["img"], c, 1, 1, p["img_out"], p["final"], p["im"],
                                                   p["im_size"], p["presence"], S()))
    want = IM.im_multiclass(pd, img, True, True)
    for key in ("img_out", "final", "im", "im_size", "presence"):
        same(out[key], want[key], key)


@pytest.mark.parametrize("k", [2, 5])
def test_morph(k):
    from inconsistencymasks_amd import im as IM
    rng = np.random.default_rng(10 + k)
    src = dev((rng.random((4, 61, 83)) > 0.5).astype(np.uint8) * 255)
    for op in (0, 1):
        ar = Arena([("src", src, "in"), ("dst", src.numel(), "out")], "cuda")
        out = ar.check(lambda p: L().imk_morph(p["src"], p["dst"], 4, 61, 83, k, op, S()))
        same(out["dst"], IM.morph(src, k, "erode" if op == 0 else "dilate"), f"op {op}")


def test_block_apply():
    """in place: img and masks are inout"""
    from inconsistencymasks_amd import im as IM
    rng = np.random.default_rng(3)
    im = dev((rng.random((3, 40, 56)) > 0.6).astype(np.uint8) * 255)
    img, masks = dev(rng.integers(1, 256, (3, 40, 56, 3), dtype=np.uint8)), dev(rng.integers(1, 256, (3, 2, 40, 56), dtype=np.uint8))
    ar = Arena([("im", im, "in"), ("img", img, "inout"), ("masks", masks, "inout")], "cuda")
    out = ar.check(lambda p: L().imk_block_apply(p["im"], p["img"], 3, p["masks"], 2, 3, 40, 56, S()))
    wi, wm = img.clone(), masks.clone()
    IM.block_apply(im, wi, wm)
    same(out["img"], wi, "img")
    same(out["masks"], wm, "masks")


def golden(name):
    with np.load(os.path.join(ROOT, "tests", "golden", name)) as d:
        return {k: d[k] for k in d.files}


def first_case(d, kind):
    return sorted({k.split("_")[0] for k in d if k.startswith(kind) and k[len(kind)].isdigit()})[0]


def test_vote_binary_and_multiclass():
    """the shapes of tests/test_gpu_model_ensemble.py: the recorded reference stacks"""
    from inconsistencymasks_amd import vote as V
    d = golden("model_ensemble.npz")
    for kind, soft in (("bin", 0), ("hela", 1)):
        c = first_case(d, kind)
        preds = dev(d[c + "_preds"])
        n, b, h, w, kb = preds.shape
        thr = float(d[c + "_thr"])
        ar = Arena([("preds", preds, "in"), ("masks", b * kb * h * w, "out")], "cuda")
        out = ar.check(lambda p: L().imk_vote_binary(p["preds"], n, b, h, w, kb, thr, soft, p["masks"], S()))
        same(out["masks"], V.vote_binary(preds, thr, bool(soft)), kind)
    c = first_case(d, "mc")
    probs = dev(d[c + "_probs"])
    n, b, h, w, k = probs.shape
    for soft in (0, 1):
        ar = Arena([("probs", probs, "in"), ("final", b * h * w, "out")], "cuda")
        out = ar.check(lambda p: L().imk_vote_multiclass(p["probs"], n, b, h, w, k, soft, p["final"], S()))
        same(out["final"], V.vote_multiclass(probs, bool(soft)), f"mc soft {soft}")


def test_vote_views_binary_and_majority():
    """the shapes of tests/test_gpu_input_ensemble.py: the recorded reference stacks"""
    from inconsistencymasks_amd import input_ensemble as IE
    sys.path.insert(0, HERE)
    from test_golden_input_ensemble import load
    d = load()
    c = first_case(d, "isic")
    preds = dev(d[c + "_preds"][:, None])
    m, b, h, w, k = preds.shape
    ops_np = np.ascontiguousarray(d[c + "_ops"][:, None].astype(np.int32))
    ops = dev(ops_np)
    quarter = int(any(IE.is_quarter_turn(int(o)) for o in ops_np.ravel()))
    thr = float(d[c + "_thr"])
    ar = Arena([("preds", preds, "in"), ("ops", ops, "in"), ("masks", b * k * h * w, "out")], "cuda")
    out = ar.check(lambda p: L().imk_vote_views_binary(p["preds"], m, b, h, w, k, p["ops"], quarter, thr, 1, p["masks"], S()))
    same(out["masks"], IE.vote_views_binary(preds, ops_np, thr, True), "views binary")
    c = first_case(d, "mc")
    probs = dev(d[c + "_probs"][:, None])
    m, b, h, w, k = probs.shape
    ar = Arena([("probs", probs, "in"), ("final", b * h * w, "out")], "cuda")
    out = ar.check(lambda p: L().imk_vote_views_majority(p["probs"], m, b, h, w, k, p["final"], S()))
    same(out["final"], IE.vote_views_majority(probs), "majority")


@pytest.mark.parametrize("chain", [0, 1])
def test_views(chain):
    from inconsistencymasks_amd import input_ensemble as IE
    rng = np.random.default_rng(11)
    b, h, w, c = 3, 32, 32, 3
    x = dev(rng.integers(0, 256, (b, h, w, c), dtype=np.uint8))
    random.seed(5)
    if chain:
        per = [IE.draw_chain_views(4, np_rng=np.random.RandomState(i)) for i in range(b)]
    else:
        per = [IE.draw_random_views(7, np_rng=np.random.RandomState(i)) for i in range(b)]
    vp = IE.ViewPlan(per, chain=bool(chain))
    prm = torch.frombuffer(bytearray(bytes(vp.params)), dtype=torch.uint8).cuda()
    ar = Arena([("img", x, "in"), ("prm", prm, "in"), ("views", vp.n_views * x.numel(), "out")], "cuda")
    out = ar.check(lambda p: L().imk_views(p["img"], b, h, w, c, vp.n_views, p["prm"], chain, vp.quarter, p["views"], S()))
    same(out["views"], IE.make_views(x, vp), "views")


@pytest.mark.parametrize("shape,cm,free", [((5, 48, 80, 3), 1, False), ((4, 32, 32, 1), 3, True), ((3, 7, 7, 3), 1, True)])
def test_augment(shape, cm, free):
    from inconsistencymasks_amd import augment
    rng = np.random.default_rng(0)
    b, h, w, c = shape
    img, msk = dev(rng.integers(0, 256, shape, dtype=np.uint8)), dev(rng.integers(0, 256, (b, h, w, cm), dtype=np.uint8))
    prm = augment.draw_params(b, rng=random.Random(100), np_rng=np.random.RandomState(100), free_rotation=free, max_blur=3, max_noise=25)
    quarter = int(any(q.rot in (1, 3) for q in prm))
    aug = torch.frombuffer(bytearray(bytes(prm)), dtype=torch.uint8).cuda()
    ar = Arena([("img", img, "in"), ("mask", msk, "in"), ("aug", aug, "in"), ("img_out", img.numel(), "out"),
                  ("mask_out", msk.numel(), "out")], "cuda")
    out = ar.check(lambda p: L().imk_augment(p["img"], p["mask"], b, h, w, c, cm, p["aug"], p["img_out"], p["mask_out"], quarter, S()))
    wi, wm = augment.augment_batch(img, msk, prm)
    same(out["img_out"], wi, "img_out")
    same(out["mask_out"], wm, "mask_out")


@pytest.mark.parametrize("planes,hw,c", [(1, (16, 16), 3), (3, (24, 40), 1), (1, (5, 7), 3)])
def test_gather_pairs(planes, hw, c):
    from inconsistencymasks_amd import functions as F
    g = torch.Generator(device="cuda").manual_seed(5)
    h, w = hw
    x = torch.randint(0, 256, (37, h, w, c), dtype=torch.uint8, device="cuda", generator=g)
    m = torch.randint(0, 2, (37, planes, h, w), dtype=torch.uint8, device="cuda", generator=g) * 255
    idx = torch.randperm(37, device="cuda", generator=g)[:29].contiguous()
    mul = torch.tensor([1, 1, 3][:planes], dtype=torch.uint8, device="cuda") if planes == 3 else None
    specs = [("img", x, "in"), ("mask", m, "in"), ("idx", idx, "in")] + ([("mul", mul, "in")] if mul is not None else [])
    ar = Arena(specs + [("img_out", 29 * h * w * c, "out"), ("mask_out", 29 * h * w * planes, "out")], "cuda")
    out = ar.check(lambda p: L().imk_gather_pairs(p["img"], h * w * c, p["mask"], planes, h * w, 1, p["mul"] if mul is not None else None,
                                                  p["idx"], 29, p["img_out"], p["mask_out"], S()))
    gx, gm = F.gather_pairs(idx, img=x, mask_planar=m, div255=True, mul=mul)
    same(out["img_out"], gx, "img_out")
    same(out["mask_out"], gm, "mask_out")


@pytest.mark.parametrize("shape", [(5, 17, 23), (2, 1, 1), (3, 256, 256)])
def test_eval_binary(shape):
    rng = np.random.default_rng(1)
    probs = rng.random(shape, dtype=np.float32)
    probs.ravel()[::7] = 0.5
    gt = rng.choice(np.array([0, 1, 127, 128, 255], np.uint8), shape)
    pd, gd = dev(probs), dev(gt)
    b, h, w = shape
    ar = Arena([("probs", pd, "in"), ("gt", gd, "in"), ("pred", b * h * w, "out"), ("counts", b * 5 * 8, "out")], "cuda")
    out = ar.check(lambda p: L().imk_eval_binary(p["probs"], 0.5, 0, p["gt"], b, h, w, p["pred"], p["counts"], S()))
    from inconsistencymasks_amd import evaluate as E
    pred, counts = E.eval_binary(pd, gd, 0.5, False)
    same(out["pred"], pred, "pred")
    same(out["counts"], torch.from_numpy(counts), "counts")


@pytest.mark.parametrize("shape,k", [((4, 5, 7), 3), ((3, 64, 64), 9), ((1, 32, 32), 1)])
def test_eval_multiclass(shape, k):
    rng = np.random.default_rng(2)
    probs = rng.random(shape + (k,), dtype=np.float32)
    gt = rng.integers(0, k + 1, shape).astype(np.uint8)
    pd, gd = dev(probs), dev(gt)
    b, h, w = shape
    ar = Arena([("probs", pd, "in"), ("gt", gd, "in"), ("pred", b * h * w, "out"), ("counts", b * 4 * 256 * 8, "out")], "cuda")
    out = ar.check(lambda p: L().imk_eval_multiclass(p["probs"], p["gt"], b, h, w, k, p["pred"], p["counts"], S()))
    from inconsistencymasks_amd import evaluate as E
    pred, counts = E.eval_multiclass(pd, gd)
    same(out["pred"], pred, "pred")
    same(out["counts"], torch.from_numpy(counts), "counts")


@pytest.mark.parametrize("b,h,w,k,mode", [(3, 32, 48, 9, 0), (2, 16, 16, 35, 0), (1, 16, 16, 64, 0), (4, 32, 32, 3, 1)])
def test_eval_soft_sums(b, h, w, k, mode):
    from inconsistencymasks_amd import evaluate as E
    rng = np.random.default_rng(4)
    probs = rng.random((b, h, w, k)).astype(np.float32)
    gt = rng.integers(0, k if mode == 0 else 4, (b, h, w) if mode == 0 else (b, h, w, k)).astype(np.uint8)
    pd, gd = dev(probs), dev(gt)
    nd = L().imk_eval_soft_out_doubles(k)
    n_res = 3 * k if mode == 0 else 1       # the results come first; the block partials behind them are scratch
    ar = Arena([("probs", pd, "in"), ("gt", gd, "in"), ("out", nd * 8, "out")], "cuda")
    out = ar.check(lambda p: L().imk_eval_soft_sums(p["probs"], p["gt"], b * h * w, k, mode, p["out"], S()), ranges={"out": (0, n_res * 8)})
    want = E.soft_sums(pd, gd, mode)
    got = out["out"].view(torch.float64).cpu().numpy()
    assert np.array_equal(got, np.asarray(want, np.float64).reshape(-1)[:n_res])


@pytest.mark.parametrize("m", [5, 11])
def test_evalnet_select(m):
    from inconsistencymasks_amd import evalnet as EV
    rng = np.random.default_rng(m)
    n, b, k = 3, 4, 3
    for mode, u in ((EV.SELECT_IOU, 1), (EV.SELECT_MIOU, 2 * k)):
        scores = dev(rng.random((n, b, m, u)).astype(np.float32))
        counts = dev(np.array([m, 1, m - 2, 3], np.int32))
        for cand_bytes in (16, 64 * 64):
            cand = dev(rng.integers(0, 256, (b, m, cand_bytes), dtype=np.uint8))
            for cnt in (None, counts):
                specs = [("scores", scores, "in"), ("cand", cand, "in")] + ([("counts", cnt, "in")] if cnt is not None else [])
                ar = Arena(specs + [("best_idx", b * 4, "out"), ("best_score", b * 4, "out"), ("keep", b, "out"),
                                      ("chosen", b * cand_bytes, "out")], "cuda")
                out = ar.check(lambda p: L().imk_evalnet_select(p["scores"], n, b, m, 2 if mode else 1, k if mode else 1,
                                                                p["counts"] if cnt is not None else None, p["cand"], cand_bytes, 0.5, mode,
                                                                p["best_idx"], p["best_score"], p["keep"], p["chosen"], S()))
                bi, bs, keep, chosen = EV.select_candidates(scores, cand, 0.5, mode, cnt)
                for key, want in (("best_idx", bi), ("best_score", bs), ("keep", keep), ("chosen", chosen)):
                    same(out[key], want, key)


if __name__ == "__main__":
    if sys.argv[1:] == ["student"]:
        print("student-digest", student_digest())
