"""GPU parity of the late-fusion EvalNet (get_evalnet_miou_v2; imk_evalnet_v2_plan_create and the imk_evalnet_* calls on such a plan)
against its CPU restatement (tests/evalnet_v2_cases.py, parity unpinned: evalnet.py runs inside Keras).  The checks and tolerances are
tests/test_gpu_evalnet.py's:
  * stored conv outputs, layer by layer: relative L2 <= 1e-2 (inference), 3e-2 (training-mode batch statistics)
  * outputs: |dp| <= 2e-2 (inference), 2e-3 (training, forward pinned);  losses 1e-3 relative with the forward values pinned to the GPU's
  * gradients with pinned forward values, per tensor: relative L2 <= max(2e-2, 1.5 x the restatement's own fp16-vs-fp32 distance on
    that case) -- the yardstick of the consistency and Dice tests; the distances measured on the MI355X are recorded in
    tests/measured/evalnet_v2_yardstick.json (IMK_WRITE_MEASURED=1 rewrites it)
  * the add on its own: the stored sum is bit for bit fp16(a + b) of the two pooled maps computed here from the stored tower outputs
    and the scale / shift pairs the kernels applied (imk_evalnet_tensor_info, which 3 and 4)."""
import ctypes
import json
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

import evalnet_v2_cases as V  # noqa: E402
from tests.test_gpu_unet import randomize_bn, rel_l2  # noqa: E402

CFGS = V.CASES
MEASURED = os.path.join(HERE, "measured", "evalnet_v2_yardstick.json")


def make(cfg, seed):
    from inconsistencymasks_amd.evalnet import get_evalnet_miou_v2
    m = get_evalnet_miou_v2(cfg["h"], cfg["w"], cfg["ca"], cfg["cb"], cfg["alpha"], seed=seed, onehot_B=cfg.get("onehot", False))
    sd = randomize_bn(m.state_dict(), seed + 1)
    m.load_state_dict(sd)
    xa, xb, y = V.make_inputs(cfg, seed + 2)
    return m, sd, xa, xb, y


def raw(m, layer, batch, mode, which):
    """a stored tensor as it lies in the workspace: fp16 [B,h,w,c_stride] and its channel count"""
    from inconsistencymasks_amd._lib import check, lib
    idx = [l["name"] for l in m.plan.layers].index(layer)
    off, h, w, c, cs = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib.imk_evalnet_tensor_info(m.plan.ptr, batch, mode, idx, which, ctypes.byref(off), ctypes.byref(h), ctypes.byref(w),
                                      ctypes.byref(c), ctypes.byref(cs)), "imk_evalnet_tensor_info")
    ws = [v for k, v in m._ws.items() if k[0] == batch and k[1] == mode][0]
    if which == 4:      # fp32 scale | shift: the packed buffer in inference, the workspace in training
        buf = ws if mode == 1 else m.packed
        return buf[off.value:off.value + 8 * cs.value].view(torch.float32).reshape(2, cs.value).cpu().numpy(), c.value
    n = batch * h.value * w.value * cs.value
    return ws[off.value:off.value + 2 * n].view(torch.float16).reshape(batch, h.value, w.value, cs.value).cpu().numpy(), c.value


def check_add(m, batch, mode):
    """sum == fp16(pool(affine(a4.c1)) + pool(affine(b4.c1))), every value rounded once: the affine and the sum are formed exactly in
    float64 (an fp16 times an fp32 has 35 significant bits; two fp16 span 51) and numpy's float64 -> float16 is correctly rounded"""
    pooled = []
    for tw in ("a", "b"):
        z, c = raw(m, f"{tw}4.c1", batch, mode, 0)
        ss, _ = raw(m, f"{tw}4.bn", batch, mode, 4)
        v = (z.astype(np.float64) * ss[0].astype(np.float64) + ss[1].astype(np.float64)).astype(np.float16)
        hh, wh = v.shape[1] // 2, v.shape[2] // 2
        v = v[:, :2 * hh, :2 * wh].reshape(batch, hh, 2, wh, 2, v.shape[3]).max(axis=(2, 4))      # the odd last row / column dropped
        pooled.append(v[..., :c])
    got, c = raw(m, "m1.c3", batch, mode, 3)
    assert got.shape[1:3] == pooled[0].shape[1:3] and c == pooled[0].shape[3]
    want = (pooled[0].astype(np.float64) + pooled[1].astype(np.float64)).astype(np.float16)
    assert np.isfinite(want.astype(np.float32)).all()
    assert np.array_equal(got[..., :c].view(np.uint16), want.view(np.uint16)), int((got[..., :c].view(np.uint16) != want.view(np.uint16)).sum())
    return pooled, want


def test_param_count_and_order():
    from inconsistencymasks_amd.evalnet import get_evalnet_miou_v2
    for name, cfg in CFGS.items():
        m = get_evalnet_miou_v2(cfg["h"], cfg["w"], cfg["ca"], cfg["cb"], cfg["alpha"], seed=1, onehot_B=cfg.get("onehot", False))
        assert (m.plan.n_total, m.plan.n_trainable) == V.count_params(cfg["ca"], cfg["cb"], cfg["cb"], cfg["alpha"]), name
        table = V.layer_table(cfg["ca"], cfg["cb"], cfg["cb"], cfg["alpha"])
        assert [(l["name"], l["ksize"], l["cin"], l["cout"]) for l in m.plan.layers] == [(t[0], t[2], t[3], t[4]) for t in table], name
        assert m.plan.arch == "v2" and m.n_heads == 2


def test_plan_limits():
    from inconsistencymasks_amd.evalnet import EvalNet, get_evalnet_miou_v2
    from inconsistencymasks_amd._lib import ImkError
    for h, w in ((64, 128), (128, 64), (130, 129)):      # seven poolings; even sizes
        with pytest.raises(ImkError):
            get_evalnet_miou_v2(h, w, 1, 3, 0.5, seed=1)
    with pytest.raises(ImkError):      # the single head has no v2
        EvalNet(128, 128, 3, 1, 1, 0.5, False, arch="v2", seed=1)


@pytest.mark.parametrize("name", list(CFGS))
def test_inference_parity(name):
    cfg = CFGS[name]
    m, sd, xa, xb, _ = make(cfg, 21)
    m.debug(materialize=True)
    try:
        out = m.predict([xa, xb])
    finally:
        m.debug(materialize=False)
    taps, sums = {}, {}
    with torch.no_grad():
        ref, _ = V.forward(sd, xa, V.oracle_b(cfg, xb), True, True, False, emulate_fp16=True, taps=taps, sums=sums)
    for n, t in taps.items():
        assert rel_l2(m.intermediate(n, cfg["b"], 0).numpy(), t.numpy()) <= 1e-2, n
    pooled, got_sum = check_add(m, cfg["b"], 0)
    assert rel_l2(got_sum.astype(np.float32), sums["sum"].numpy()) <= 1e-2
    got = np.concatenate(out, 1)
    assert np.abs(got - ref.numpy()).max() <= 2e-2
    plain = np.concatenate(m.predict([xa, xb]), 1)      # the fused launches of the product path
    check_add(m, cfg["b"], 0)
    assert np.abs(plain - ref.numpy()).max() <= 2e-2
    if cfg.get("onehot"):    # the reference's call sites pass the one-hot stack itself: same result
        oh = m.predict([xa, V.one_hot(xb, cfg["cb"])])
        assert np.array_equal(np.concatenate(oh, 1), plain)
    one = np.concatenate(m.predict([xa[:1], xb[:1]]), 1)      # batch invariance of inference
    assert np.abs(one - plain[:1]).max() <= 1e-6
    assert np.array_equal(np.concatenate(m.predict([xa, xb]), 1), plain)      # bit-identical repeats


def _record(name, dist):
    if os.environ.get("IMK_WRITE_MEASURED") != "1":
        return
    rec = json.load(open(MEASURED)) if os.path.exists(MEASURED) else {"what": "", "cases": {}}
    rec["what"] = ("rel-L2 per gradient tensor between the restatement's fp16-emulating and fp32 forms on the forward values of the "
                   "MI355X run (yardstick), and between the MI355X gradients and the fp16 form (gpu)")
    rec["cases"][name] = dist
    with open(MEASURED, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("name", list(CFGS))
def test_train_pass_parity(name):
    cfg = CFGS[name]
    m, sd, xa, xb, y = make(cfg, 31)
    m.init_train_state()
    dev = lambda a: torch.from_numpy(a).cuda()
    for attempt in range(14):
        out = m.fwd_bwd(dev(xa), dev(xb), dev(y))
        torch.cuda.synchronize()
        stats = m.stats.cpu().numpy()
        assert stats[2] == 32768.0 / 2 ** attempt
        if stats[1] == 0.0:
            break
        before = m.params.clone()
        m.adamw_step(3e-3, 1e-4)
        assert torch.equal(before, m.params)
        m.load_state_dict(sd)
    assert stats[1] == 0.0
    g1 = m.grads.clone()
    moving_after_1 = m.state_dict()
    out2 = m.fwd_bwd(dev(xa), dev(xb), dev(y))
    assert torch.equal(g1, m.grads) and torch.equal(out, out2)          # deterministic: no float atomics anywhere in the step
    check_add(m, cfg["b"], 1)
    ov = {l["name"]: m.intermediate(l["name"], cfg["b"], 1) for l in m.plan.layers if l["kind"] == 0 and l["name"] not in V.HEADS}
    taps = {}
    xbo = V.oracle_b(cfg, xb)
    with torch.no_grad():
        V.forward(sd, xa, xbo, True, True, False, training=True, emulate_fp16=True, taps=taps)
    for n, t in taps.items():
        assert rel_l2(ov[n].numpy(), t.numpy()) <= 3e-2, n
    losses, out_ref, grads_ref, bstats = V.grads(sd, xa, xbo, y, True, True, False, emulate_fp16=True, loss_scale=float(stats[2]),
                                                 override=ov)
    _, _, grads32, _ = V.grads(sd, xa, xbo, y, True, True, False, emulate_fp16=False, override=ov)
    assert np.abs(out.cpu().numpy() - out_ref.numpy()).max() <= 2e-3
    assert abs(stats[0] - losses[0]) <= 1e-3 * max(1.0, abs(losses[0]))
    assert abs(stats[4] - losses[1]) <= 1e-3 * max(1.0, abs(losses[1]))
    assert abs(stats[5] - losses[2]) <= 1e-3 * max(1.0, abs(losses[2]))
    g = g1.cpu()
    errs = {}
    for l in m.plan.layers:
        n = l["name"]
        if l["kind"] == 0:
            kk, ci, co = l["ksize"], l["cin"], l["cout"]
            errs[n + ".w"] = rel_l2(g[l["off_w"]:l["off_w"] + kk * kk * ci * co].reshape(kk, kk, ci, co).numpy(), grads_ref[n + ".w"].numpy())
            errs[n + ".b"] = rel_l2(g[l["off_b"]:l["off_b"] + co].numpy(), grads_ref[n + ".b"].numpy())
        else:
            cc = l["cout"]
            errs[n + ".gamma"] = rel_l2(g[l["off_w"]:l["off_w"] + cc].numpy(), grads_ref[n + ".gamma"].numpy())
            errs[n + ".beta"] = rel_l2(g[l["off_b"]:l["off_b"] + cc].numpy(), grads_ref[n + ".beta"].numpy())
    yard = {k: rel_l2(grads_ref[k].numpy(), grads32[k].numpy()) for k in errs}
    bound = {k: max(2e-2, 1.5 * yard[k]) for k in errs}
    worst = max(errs, key=lambda k: errs[k] / bound[k])
    print(f"GPU_GAP {name}: worst {worst} {errs[worst]:.3g} of {bound[worst]:.3g} (yardstick {yard[worst]:.3g}); "
          f"largest yardstick {max(yard.values()):.3g}, largest gap {max(errs.values()):.3g}")
    _record(name, {k: {"yardstick": float(f"{yard[k]:.3g}"), "gpu": float(f"{errs[k]:.3g}")} for k in sorted(errs)})
    bad = {k: (round(v, 4), round(bound[k], 4)) for k, v in errs.items() if not v <= bound[k]}
    assert not bad, f"gradient tensors beyond max(2e-2, 1.5 x yardstick) (rel-L2, bound): {bad}"
    for name_, (mean, var) in bstats.items():       # moving = 0.99 * moving + 0.01 * batch
        assert torch.allclose(moving_after_1[name_ + ".mean"], 0.99 * sd[name_ + ".mean"] + 0.01 * mean, atol=1e-4, rtol=1e-3), name_
        assert torch.allclose(moving_after_1[name_ + ".var"], 0.99 * sd[name_ + ".var"] + 0.01 * var, atol=1e-4, rtol=1e-3), name_


def test_training_reduces_loss():
    cfg = CFGS["hela"]
    m, sd, xa, xb, y = make(cfg, 41)
    dev = lambda a: torch.from_numpy(a).cuda()
    xa, xb, y = dev(xa), dev(xb), dev(y)
    losses = []
    for _ in range(40):
        m.train_step(xa, xb, y, 3e-3, 1e-4)
        losses.append(float(m.stats[0]))
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < 0.9 * np.mean(losses[:5]), losses
    out = m.predict([xa, xb])
    assert out[0].shape == (cfg["b"], cfg["cb"]) and out[1].shape == (cfg["b"], cfg["cb"])
