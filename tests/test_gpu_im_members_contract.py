"""The C ABI's buffer and stream contracts (include/imk.h) for the per-image sub-ensemble entry points: imk_im_binary_members,
imk_im_multiclass_members, imk_morph_var and imk_unet_forward_im_members inside tests/arena.py's guard bands under its three poison
fills, a workspace one byte short refused with nothing written, and imk_unet_forward_im_members under tests/stream_skew.py's skews.
Both helper modules are imported as they are; the small helpers are tests/test_gpu_buffer_contract.py's.  Every comparison is
bit-exact: across the fills, across the skews, and against the Python wrappers (the product path)."""
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

import stream_skew as SK  # noqa: E402
import test_gpu_buffer_contract as BC  # noqa: E402  (Arena ordering, refused, same, cached models, images)

L, S, dev = BC.L, BC.S, BC.dev
IMK_EWORKSPACE = -3


def words_dev(words):
    return dev(np.asarray(words, np.uint32).view(np.int32))


# ---- the rule on a stack, at ragged sizes where the 16-byte store paths have tails ---------------------------------------------------
@pytest.mark.parametrize("n,b,h,w,kb,c", [(5, 3, 35, 21, 1, 3), (10, 4, 64, 48, 3, 1)])
def test_im_binary_members(n, b, h, w, kb, c):
    from inconsistencymasks_amd import im as IM
    rng = np.random.default_rng(h * w + n)
    base = rng.random((1, b, h, w, kb), dtype=np.float32)
    preds = np.clip(base + (rng.random((n, b, h, w, kb), dtype=np.float32) - 0.5) * 0.3, 0, 1).astype(np.float32)
    preds[0, 0, 0, :4, 0] = [0.5, np.nan, 0.50000006, 0.49999997]
    words = [0b101, (1 << n) - 1, 0, 1 << (n - 1)][:b]
    pd, img, wd = dev(preds), dev(rng.integers(1, 256, (b, h, w, c), dtype=np.uint8)), words_dev(words)
    ge = int(kb == 3)
    ar = BC.Arena([("preds", pd, "in"), ("members", wd, "in"), ("img", img, "in"), ("img_out", img.numel(), "out"),
                   ("masks", b * kb * h * w, "out"), ("im", b * h * w, "out"), ("im_size", b * kb * 8, "out"), ("pred_size", b * kb * 8, "out")])
    out = ar.check(lambda p: L().imk_im_binary_members(p["preds"], p["members"], n, b, h, w, kb, 0.5, ge, p["img"], c, 1, 1, p["img_out"],
                                                       p["masks"], p["im"], p["im_size"], p["pred_size"], S()))
    want = IM.im_binary_members(pd, words, 0.5, bool(ge), img, True, True)
    for key in ("img_out", "masks", "im", "im_size", "pred_size"):
        BC.same(out[key], want[key], key)
    # no image: img_out is ignored
    ar = BC.Arena([("preds", pd, "in"), ("members", wd, "in"), ("masks", b * kb * h * w, "out"), ("im", b * h * w, "out"),
                   ("im_size", b * kb * 8, "out"), ("pred_size", b * kb * 8, "out")])
    out = ar.check(lambda p: L().imk_im_binary_members(p["preds"], p["members"], n, b, h, w, kb, 0.5, ge, None, 0, 1, 0, None, p["masks"],
                                                       p["im"], p["im_size"], p["pred_size"], S()))
    BC.same(out["masks"], IM.im_binary_members(pd, words, 0.5, bool(ge), None, True, False)["masks"], "masks without an image")


@pytest.mark.parametrize("n,b,h,w,k,c", [(5, 3, 17, 9, 4, 1), (16, 4, 13, 26, 35, 3)])
def test_im_multiclass_members(n, b, h, w, k, c):
    from inconsistencymasks_amd import im as IM
    rng = np.random.default_rng(k * 7 + h)
    base = rng.random((1, b, h, w, k), dtype=np.float32)
    probs = (base + 0.2 * rng.random((n, b, h, w, k), dtype=np.float32)).astype(np.float32)
    probs[:, :, : h // 3] = np.round(probs[:, :, : h // 3] * 3) / 3
    words = [0b110, (1 << n) - 1, 0, 1 << (n - 1)][:b]
    pd, img, wd = dev(probs), dev(rng.integers(1, 256, (b, h, w, c), dtype=np.uint8)), words_dev(words)
    ar = BC.Arena([("probs", pd, "in"), ("members", wd, "in"), ("img", img, "in"), ("img_out", img.numel(), "out"), ("final", b * h * w, "out"),
                   ("im", b * h * w, "out"), ("im_size", b * 8, "out"), ("presence", n * b * k, "out")])
    out = ar.check(lambda p: L().imk_im_multiclass_members(p["probs"], p["members"], n, b, h, w, k, p["img"], c, 1, 1, p["img_out"],
                                                           p["final"], p["im"], p["im_size"], p["presence"], S()))
    want = IM.im_multiclass_members(pd, words, img, True, True)
    for key in ("img_out", "final", "im", "im_size", "presence"):
        BC.same(out[key], want[key], key)


def test_morph_var():
    from inconsistencymasks_amd import im as IM
    rng = np.random.default_rng(17)
    ks = [0, 3, 5, 7, 3]
    src = dev((rng.random((5, 61, 83)) > 0.5).astype(np.uint8) * 255)
    kd = dev(np.asarray(ks, np.int32))
    for op in (0, 1):
        ar = BC.Arena([("src", src, "in"), ("ksizes", kd, "in"), ("dst", src.numel(), "out")])
        out = ar.check(lambda p: L().imk_morph_var(p["src"], p["dst"], 5, 61, 83, p["ksizes"], op, S()))
        BC.same(out["dst"], IM.morph_var(src, ks, "erode" if op == 0 else "dilate"), f"op {op}")


# ---- imk_unet_forward_im_members -----------------------------------------------------------------------------------------------------
N_POOL = 5
POOL_SHAPES = [BC.SHAPES[0], BC.SHAPES[1], BC.SHAPES[3]]      # softmax 16 x 16; sigmoid 48 x 80, 8 channels; sigmoid K 2, 28 channels
POOL_IDS = [BC.S_IDS[0], BC.S_IDS[1], BC.S_IDS[3]]
WORDS = {3: [0b00110, 0b10001, 0b00110], 4: [0b00110, 0b10001, 0, 0b11100]}


def pool(cfg):
    return [BC.unet(cfg, seed=11 + 10 * j) for j in range(N_POOL)]


def members_arena(models, x, b, ws_bytes, binary):
    p = models[0].plan
    kb = p.n_out if binary else 1
    specs = BC.model_specs(models) + [("x", x, "in"), ("img_out", x.numel(), "out"), ("masks", b * kb * p.h * p.w, "out"),
                                      ("im", b * p.h * p.w, "out"), ("im_size", b * kb * 8, "out"), ("pred_size", b * kb * 8, "out")]
    if not binary:
        specs.append(("presence", len(models) * b * p.n_out, "out"))
    return BC.Arena(specs + [("ws", ws_bytes, "scratch")])


def members_call(models, b, words, ws_bytes, binary):
    plan, n = models[0].plan, len(models)
    host = (ctypes.c_uint32 * b)(*words)

    def call(p):
        pa, pk = BC.ptr_arrays(p, n)
        return L().imk_unet_forward_im_members(plan.ptr, n, pa, pk, p["x"], b, host, 0.5, 0, p["x"], 1, 1, p["img_out"], p["masks"],
                                               p["im"], p["im_size"], p["pred_size"], None if binary else p["presence"], p["ws"],
                                               ws_bytes, S())
    return call


@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("cfg", POOL_SHAPES, ids=POOL_IDS)
def test_forward_im_members(cfg, b, n_streams):
    from inconsistencymasks_amd import functions as F
    models, x = pool(cfg), BC.images(cfg, b)
    plan, binary = models[0].plan, cfg[5] == "sigmoid"
    words = WORDS[b]
    n = L().imk_unet_forward_im_members_workspace_bytes(plan.ptr, N_POOL, b, n_streams)
    assert n > 0
    unwritten = () if binary else ("pred_size",)          # include/imk.h: pred_size unused for softmax heads
    keys = ("img_out", "masks", "im", "im_size") + (("pred_size",) if binary else ("presence",))
    for route in ("fused", "unfused"):      # the wrapper under the same switch: it changes which conv kernels run as well
        for m in models:
            m.debug(materialize=route == "unfused")
        try:
            want = F.PoolIM(models).run(x, words, 0.5, False, True, True, want_presence=not binary)
            torch.cuda.synchronize()
            out = members_arena(models, x, b, n, binary).check(members_call(models, b, words, n, binary), unwritten=unwritten)
        finally:
            for m in models:
                m.debug(materialize=False)
        for key in keys:
            BC.same(out[key], want[key], f"{route} {key}")
    if n_streams == 1:      # the size for one stream is the least the call accepts
        BC.refused(members_arena(models, x, b, n - 1, binary), members_call(models, b, words, n - 1, binary))


def test_forward_im_members_under_skewed_streams():
    """five models on three streams (the caller's and the pool's two side streams), each stream held in turn while every buffer a
    premature reader could touch holds poison: every output is bit-identical to the unskewed run, under both fills.  The member
    words travel as kernel arguments, so the call returns while its stream is held."""
    from inconsistencymasks_amd import functions as F
    cfg, b = BC.SHAPES[1], 4
    models, x0 = pool(cfg), BC.images(cfg, b)
    plan = models[0].plan
    words = WORDS[b]
    nws = L().imk_unet_forward_im_members_workspace_bytes(plan.ptr, N_POOL, b, 3)
    want = F.PoolIM(models).run(x0, words, 0.5, False, True, True)
    torch.cuda.synchronize()
    sides = {f"side{i}": SK.side_stream(models[0], i) for i in range(2)}
    caller, beside = SK.caller_stream_beside(list(sides.values()))
    assert beside, "no caller stream off the side streams' hardware queues was found"
    x = torch.empty_like(x0)
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
    bufs = {"img_out": torch.empty_like(x0), "masks": u8(b, 1, plan.h, plan.w), "im": u8(b, plan.h, plan.w),
            "im_size": torch.empty((b, 1), dtype=torch.int64, device="cuda"), "pred_size": torch.empty((b, 1), dtype=torch.int64, device="cuda")}
    ws = u8(nws)
    ptrs = {f"params{j}": m.params.data_ptr() for j, m in enumerate(models)}
    ptrs.update({f"packed{j}": m.packed.data_ptr() for j, m in enumerate(models)})
    ptrs.update({k: v.data_ptr() for k, v in bufs.items()})
    ptrs.update(x=x.data_ptr(), ws=ws.data_ptr())
    fn = members_call(models, b, words, nws, True)

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
