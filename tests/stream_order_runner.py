"""The runs of tests/test_gpu_stream_order.py (a plain module with main(), started by that test as a fresh child process once per
value of IMK_SIDE_STREAMS -- the switch table is read once per process -- and importable for its case lists).

Every case runs its call(s) through tests/stream_skew.py::run_skewed under every skew and both poison fills, in two configurations
of the plan (default, debug(single_stream=True)), and leaves one sha256 digest of the outputs per (case, configuration, skew,
fill) in a JSON file, with the measured undisturbed wall time and the hold length of every (case, configuration).  The parent
compares digests; nothing is compared here.

    python tests/stream_order_runner.py OUT.json [unet/isic | evalnet/ | ensemble/hela | student/ ...]
"""
import ctypes
import json
import os
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# ---- the cases (names only: importable without a GPU) -----------------------------------------------------------------------------
UNET_CASES = ("isic", "suim", "alpha175", "odd", "alpha2", "tiny16")      # tests/test_gpu_unet.py::CFGS
EVALNET_CASES = ("isic", "alpha2")                                        # tests/test_gpu_evalnet.py::CFGS
CONSISTENCY_CASES = ("isic", "suim")                                      # tests/consistency_cases.py::CASES (fused, composed)
ENSEMBLE_CASES = ("hela", "suim")                                         # tests/test_gpu_unet.py::CFGS, N_MODELS models each
STUDENT_CASES = ("hela-small", "suim-small")                              # tests/test_gpu_noisy_student.py::SMALL, last width 16
N_MODELS = 3
N_STREAMS = (1, 2, 3)
CONFIGS = ("default", "single_stream")
LR, WD = 3e-3, 1e-4


def training_case_ids():
    ids = [f"unet/{n}" for n in UNET_CASES] + [f"evalnet/{n}" for n in EVALNET_CASES] + [f"consistency/{n}" for n in CONSISTENCY_CASES]
    return [f"{i}/{kind}" for i in ids for kind in ("fwd_bwd", "steps")]


def inference_case_ids():
    return ([f"{call}/{n}/k{k}" for call in ("im", "vote") for n in ENSEMBLE_CASES for k in N_STREAMS]
            + [f"student/{n}" for n in STUDENT_CASES])


def skew_name(skew):
    if isinstance(skew, dict):
        return ">".join("+".join(skew[i]) for i in sorted(skew))
    return "+".join(skew) or "none"


def training_skews(n_side):
    """the skews of one training call: with IMK_SIDE_STREAMS=0 the pool's two side streams are held together (nothing may change)"""
    if n_side == 0:
        return [(), ("main",), ("side0", "side1")]
    if n_side == 1:
        return [(), ("main",), ("side0",)]
    return [(), ("main",), ("side0",), ("side1",), ("side0", "side1")]


def steps_skews(n_side):
    """three steps back to back: the caller's stream held before the first, a side stream before the second (call index 2: a
    poison fill of the dead buffers sits between two steps)"""
    return [()] + [{0: ("main",), 2: (f"side{i}",)} for i in range(max(1, n_side))]


def inference_skews(n_streams):
    return training_skews(max(1, n_streams - 1))


def sides_in_use(case_id, n_side, config="default"):
    """how many of the pool's side streams the case's call forks onto: the training steps IMK_SIDE_STREAMS, the ensemble calls one
    per stream beyond the first, the student pass one; none under single_stream"""
    if config == "single_stream":
        return 0
    if case_id.startswith("student/"):
        return 1
    if case_id.startswith(("im/", "vote/")):
        return int(case_id.rsplit("/k", 1)[1]) - 1
    return n_side


# ---- everything below needs the GPU -----------------------------------------------------------------------------------------------
def _imports():
    global torch, np, K, lib, check
    import numpy as np
    import torch
    import stream_skew as K
    from inconsistencymasks_amd._lib import check, lib


def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).cuda().contiguous()


class Spec:
    """one call under test: what run_skewed needs, the models whose plans take the configuration switch, and the skews"""

    def __init__(self, case_id, call, inputs, outputs, scratch, skews, models, configs=CONFIGS, box=None):
        self.case_id, self.call, self.inputs, self.outputs, self.scratch = case_id, call, inputs, outputs, scratch
        self.skews, self.models, self.configs, self.box = skews, models, configs, box if box is not None else {}


def state_inputs(m):
    """the model's device state as inputs: restored from these copies behind the hold, so every run starts from the same bits"""
    return {"params": (m.params, m.params.clone()), "packed": (m.packed, m.packed.clone()),
            "state": (m.train_state, m.train_state.clone())}


def settle_loss_scale(m, fwd_bwd, sd):
    """the dynamic loss scale starts at 32768: overflowing passes are skipped and halve it (tests/test_gpu_unet.py::
    test_train_step_parity); the runs start from the first scale that does not overflow, with the weights as loaded"""
    m.init_train_state()
    for _ in range(14):
        fwd_bwd()
        torch.cuda.synchronize()
        if float(m.stats[1]) == 0.0:
            break
        m.adamw_step(LR, WD)
        m.load_state_dict(sd)
    else:
        raise AssertionError("no loss scale without overflow")
    m.load_state_dict(sd)          # undo the moving-statistics update
    m.repack()
    torch.cuda.synchronize()


def training_specs(prefix, m, data, fwd_bwd, predict, ws_train, extra_out, n_side):
    """(a) one fwd_bwd; (b) three train steps back to back, dead buffers poisoned in between, then a forward on a fixed batch"""
    nt = m.plan.n_trainable
    b = next(iter(data.values()))[0].shape[0]
    ws_inf = m.workspace(b, 0)
    probs = predict().clone()
    torch.cuda.synchronize()
    state = state_inputs(m)
    inputs = dict(data, **state)
    box = {"fill": 0xFF}

    def first_fwd_bwd():
        m._packed_ok, m._fold_ok = True, False      # the device state was restored to the packed weights of `params`
        fwd_bwd()
    outs_a = dict({"grads": m.grads, "stats": m.stats[:3], "moving": m.params[nt:]}, **extra_out)
    a = Spec(prefix + "/fwd_bwd", first_fwd_bwd, inputs, outs_a, [ws_train, m.grads_and_stats], training_skews(n_side), [m])

    def first_step():
        first_fwd_bwd()
        m.adamw_step(LR, WD)

    def step():
        fwd_bwd()
        m.adamw_step(LR, WD)

    def between():      # the caller reusing what is dead between two steps: the workspace, the gradients, the statistics
        K.poison(ws_train, box["fill"])
        K.poison(m.grads_and_stats, box["fill"])

    def forward():
        probs.copy_(predict())
    outs_b = {"params": m.params, "state": m.train_state, "stats": m.stats[:3], "probs": probs}
    s = Spec(prefix + "/steps", [first_step, between, step, between, step, forward], inputs, outs_b,
             [ws_train, ws_inf, m.grads_and_stats, probs], steps_skews(n_side), [m], box=box)
    return [a, s]


def unet_training(name, n_side):
    from tests.test_gpu_unet import CFGS, make_input, randomize_bn
    from inconsistencymasks_amd.unet import UNet
    cfg = CFGS[name]
    m = UNet(cfg["h"], cfg["w"], cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], seed=11)
    sd = randomize_bn(m.state_dict(), 12)
    m.load_state_dict(sd)
    x, y, _ = make_input(cfg, 13)
    xd, yd = dev(x), dev(y)
    kind = 0 if cfg["loss"] == "mse" else 1
    fb = lambda: m.fwd_bwd(xd, yd, kind)  # noqa: E731
    settle_loss_scale(m, fb, sd)
    data = {"x": (xd, xd.clone()), "y": (yd, yd.clone())}
    return training_specs(f"unet/{name}", m, data, fb, lambda: m.predict_device(xd), m.workspace(cfg["b"], 1), {}, n_side)


def evalnet_training(name, n_side):
    from tests.test_gpu_evalnet import CFGS, make
    cfg = CFGS[name]
    m, sd, xa, xb, y = make(cfg, 31)
    xa, xb, y = dev(xa), dev(xb), dev(y)
    out = torch.empty((cfg["b"], m.n_heads * m.plan.n_out), dtype=torch.float32, device="cuda")
    fb = lambda: out.copy_(m.fwd_bwd(xa, xb, y))  # noqa: E731
    settle_loss_scale(m, fb, sd)
    data = {"xa": (xa, xa.clone()), "xb": (xb, xb.clone()), "y": (y, y.clone())}
    extra = {"out": out, "head_losses": m.stats[4:6]}
    return training_specs(f"evalnet/{name}", m, data, fb, lambda: m.predict_device(xa, xb), m.workspace(cfg["b"], 1), extra, n_side)


def consistency_training(name, n_side):
    import consistency_cases as C
    from inconsistencymasks_amd.unet import UNet
    cfg = C.CASES[name]
    m = UNet(cfg["h"], cfg["w"], cfg["c"], cfg["k"], cfg["alpha"], cfg["act"], seed=C.MODEL_SEED)
    sd = C.randomize_bn(m.state_dict(), C.BN_SEED)
    m.load_state_dict(sd)
    v1, v2 = C.make_views(cfg)
    d1, d2 = dev(v1), dev(v2)
    fb = lambda: m.consistency_fwd_bwd(d1, d2)  # noqa: E731
    settle_loss_scale(m, fb, sd)
    data = {"x1": (d1, d1.clone()), "x2": (d2, d2.clone())}
    return training_specs(f"consistency/{name}", m, data, fb, lambda: m.predict_device(d1), m.consistency_workspace(cfg["b"]), {},
                          n_side)


def ensemble_specs(name):
    """imk_unet_forward_im and imk_unet_forward_vote through the C ABI on n_streams = 1, 2, 3; the models' weights are inputs like
    the images: a model that starts on a side stream before the caller's stream has produced them reads poison"""
    from tests.test_gpu_unet import CFGS, make_input, randomize_bn
    from inconsistencymasks_amd.unet import UNet
    cfg = CFGS[name]
    h, w, c, k, b = cfg["h"], cfg["w"], cfg["c"], cfg["k"], cfg["b"]
    binary = cfg["act"] == "sigmoid"
    models = []
    for j in range(N_MODELS):
        m = UNet(h, w, c, k, cfg["alpha"], cfg["act"], seed=41 + j)
        m.load_state_dict(randomize_bn(m.state_dict(), 51 + j))
        m.ready_for_inference()
        models.append(m)
    torch.cuda.synchronize()
    plan = models[0].plan
    x = dev(make_input(cfg, 61)[0])
    inputs = {"x": (x, x.clone())}
    for j, m in enumerate(models):
        inputs[f"params{j}"] = (m.params, m.params.clone())
        inputs[f"packed{j}"] = (m.packed, m.packed.clone())
    pa = (ctypes.c_void_p * N_MODELS)(*[m.params.data_ptr() for m in models])
    pk = (ctypes.c_void_p * N_MODELS)(*[m.packed.data_ptr() for m in models])
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device="cuda")  # noqa: E731
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")  # noqa: E731
    if binary:
        im_out = {"img_out": u8(b, h, w, c), "masks": u8(b, k, h, w), "im": u8(b, h, w), "im_size": i64(b, k), "pred_size": i64(b, k)}
        vote_out = {"masks": u8(b, k, h, w)}
    else:
        im_out = {"img_out": u8(b, h, w, c), "masks": u8(b, h, w), "im": u8(b, h, w), "im_size": i64(b), "presence": u8(N_MODELS, b, k)}
        vote_out = {"masks": u8(b, h, w)}
    ptr = lambda d, n: d[n].data_ptr() if n in d else None  # noqa: E731
    specs = []
    for n_streams in N_STREAMS:
        nbytes = lib.imk_unet_forward_im_workspace_bytes(plan.ptr, N_MODELS, b, n_streams)
        assert nbytes > 0, nbytes
        ws = u8(nbytes)

        def im(ws=ws, nbytes=nbytes):
            check(lib.imk_unet_forward_im(plan.ptr, N_MODELS, pa, pk, x.data_ptr(), b, 0.5, 0, x.data_ptr(), 1, 1,
                                          ptr(im_out, "img_out"), ptr(im_out, "masks"), ptr(im_out, "im"), ptr(im_out, "im_size"),
                                          ptr(im_out, "pred_size"), ptr(im_out, "presence"), ws.data_ptr(), nbytes,
                                          torch.cuda.current_stream().cuda_stream), "imk_unet_forward_im")

        def vote(ws=ws, nbytes=nbytes):      # the soft vote for sigmoid heads (fp64 mean), the hard one for softmax heads
            check(lib.imk_unet_forward_vote(plan.ptr, N_MODELS, pa, pk, x.data_ptr(), b, 0.5, 1 if binary else 0,
                                            vote_out["masks"].data_ptr(), ws.data_ptr(), nbytes,
                                            torch.cuda.current_stream().cuda_stream), "imk_unet_forward_vote")
        # single_stream runs the models back to back whatever the workspace allows: one workspace size is enough for it
        configs = CONFIGS if n_streams == N_STREAMS[-1] else CONFIGS[:1]
        specs.append(Spec(f"im/{name}/k{n_streams}", im, inputs, im_out, [ws], inference_skews(n_streams), models, configs))
        specs.append(Spec(f"vote/{name}/k{n_streams}", vote, inputs, vote_out, [ws], inference_skews(n_streams), models, configs))
    return specs


def student_spec(name):
    """imk_unet_forward_student through the C ABI (the wrapper uploads the draws inside the call, which waits for the stream): last
    decoder width 16, so the image path forks; every blur size occurs"""
    from tests.test_gpu_noisy_student import SMALL, params
    from inconsistencymasks_amd.unet import UNet
    _, h, w, c, k, alpha, act, geoms, cmp_ge = [s for s in SMALL if s[0] == name][0]
    assert int(16 * alpha) > 8
    m = UNet(h, w, c, k, alpha, act, seed=11)
    m.ready_for_inference()
    seed = zlib.crc32(name.encode())
    rng = np.random.default_rng(seed)
    b = len(geoms)
    x = dev(rng.integers(0, 256, (b, h, w, c), dtype=np.uint8))
    img = x.flip(-1).contiguous() if c == 3 else x.clone()
    prm = params(geoms, seed)
    assert any(q.blur_k for q in prm)
    quarter = int(any(q.rot in (1, 3) for q in prm))
    aug = torch.frombuffer(bytearray(bytes(prm)), dtype=torch.uint8).cuda()
    nbytes = lib.imk_unet_forward_student_workspace_bytes(m.plan.ptr, b)
    assert nbytes > 0, nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = {"img_out": torch.empty_like(img),
           "labels": torch.empty((b, k, h, w) if act == "sigmoid" else (b, h, w), dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    inputs = {"x": (x, x.clone()), "img": (img, img.clone()), "aug": (aug, aug.clone()),
              "params": (m.params, m.params.clone()), "packed": (m.packed, m.packed.clone())}

    def call():
        check(lib.imk_unet_forward_student(m.plan.ptr, m.params.data_ptr(), m.packed.data_ptr(), x.data_ptr(), img.data_ptr(), b, 0.5,
                                           int(cmp_ge), aug.data_ptr(), quarter, out["img_out"].data_ptr(), out["labels"].data_ptr(),
                                           ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "imk_unet_forward_student")
    return Spec(f"student/{name}", call, inputs, out, [ws], inference_skews(2), [m])


def run_spec(spec, S, sides, results, meta):
    for config in spec.configs:
        for m in spec.models:
            m.debug(single_stream=(config == "single_stream"))
        wall = K.wall_ms(spec.call, spec.inputs, S)
        hold_ms = K.hold_ms_for(wall)
        waited = {}
        meta[spec.case_id][config] = {"wall_ms": round(wall, 3), "hold_ms": round(hold_ms, 1), "synced_ms": waited}
        for skew in spec.skews:
            for fill in K.FILLS:
                spec.box["fill"] = fill
                timing = {}
                try:
                    got = K.digest(K.run_skewed(spec.call, spec.inputs, spec.outputs, spec.scratch, skew, S, fill=fill,
                                                hold_ms=hold_ms, sides=sides, timing=timing))
                    name = skew_name(skew)      # the earliest the caller's stream was through, over the fills
                    waited[name] = round(min(waited.get(name, 1e9), timing["synced_ms"]), 2)
                except AssertionError as e:      # a hold that was too short: this slot fails in the parent, the run goes on
                    got = f"FAILED: {e}"
                results[spec.case_id][config].setdefault(skew_name(skew), {})[f"{fill:02X}"] = got
    for m in spec.models:
        m.debug(single_stream=False)


def main(argv):
    out_path, only = argv[1], argv[2:]
    _imports()
    t0 = time.perf_counter()
    n_side = int(os.environ.get("IMK_SIDE_STREAMS", "1"))
    assert n_side in (0, 1, 2), n_side
    want = lambda case_id: not only or any(case_id.startswith(p) for p in only)  # noqa: E731
    builders = ([(f"unet/{n}", lambda n=n: unet_training(n, n_side)) for n in UNET_CASES]
                + [(f"evalnet/{n}", lambda n=n: evalnet_training(n, n_side)) for n in EVALNET_CASES]
                + [(f"consistency/{n}", lambda n=n: consistency_training(n, n_side)) for n in CONSISTENCY_CASES]
                + [(f"ensemble/{n}", lambda n=n: ensemble_specs(n)) for n in ENSEMBLE_CASES]
                + [(f"student/{n}", lambda n=n: [student_spec(n)]) for n in STUDENT_CASES])
    from inconsistencymasks_amd.unet import UNet
    probe = UNet(16, 16, 3, 1, 0.5, "sigmoid", seed=1)
    sides = {"side0": K.side_stream(probe, 0), "side1": K.side_stream(probe, 1)}
    S, beside = K.caller_stream_beside(list(sides.values()))
    doc = {"side_streams": n_side, "cycles_per_ms": K.cycles_per_ms(), "caller_stream_runs_beside_the_side_streams": beside,
           "side_streams_run_beside_each_other": K.runs_ahead(sides["side0"], sides["side1"]) and K.runs_ahead(sides["side1"], sides["side0"]),
           "results": {}, "meta": {}}
    for key, build in builders:
        if not want(key):
            continue
        with torch.cuda.stream(S):
            specs = build()
        torch.cuda.synchronize()
        for spec in specs:
            doc["results"][spec.case_id] = {c: {} for c in spec.configs}
            doc["meta"][spec.case_id] = {}
            run_spec(spec, S, sides, doc["results"], doc["meta"])
        del specs
    torch.cuda.synchronize()
    doc["elapsed_s"] = round(time.perf_counter() - t0, 1)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
