"""GPU tests of the noisy-student label pass: imk_unet_forward_student against imk_unet_forward -> numpy threshold / np.argmax ->
oracle/aug_oracle.py (bit for bit, every pixel), the fused route against the unfused one, the three writers against the reference's
recorded label files (tests/golden/noisy_student.npz), the refusal of quarter turns on rectangles, and the fork / join of the image
path's side stream."""
import os
import random
import zlib

import numpy as np
import pytest
import torch

from oracle import aug_oracle as A

pytestmark = pytest.mark.gpu

GEOMETRIES = [(fv, fh, rot) for fv in range(2) for fh in range(2) for rot in range(4)]      # all 16 combinations
FLIPS = [(0, fh, 0) for fh in range(2)]                                                     # FREE_ROTATION = False


@pytest.fixture(scope="module")
def ns():
    from inconsistencymasks_amd import noisy_student
    return noisy_student


@pytest.fixture(scope="module")
def gold():
    from test_golden_noisy_student import load
    return load()


def params(geoms, seed, max_blur=3, max_noise=25):
    """one AugParams per geometry: the pixel part random (every blur size occurs), the geometry as given"""
    from inconsistencymasks_amd import _lib
    rng = np.random.default_rng(seed)
    arr = (_lib.AugParams * len(geoms))()
    for i, (q, (fv, fh, rot)) in enumerate(zip(arr, geoms)):
        q.flip_v, q.flip_h, q.rot = fv, fh, rot
        q.bright_on, q.alpha, q.beta = int(rng.integers(0, 2)), float(rng.uniform(0.5, 1.5)), float(rng.uniform(-25, 25))
        b = (i % (max_blur + 1)) if max_blur else 0
        q.blur_k = 2 * b + 1 if b else 0
        q.noise_max, q.seed = max_noise, int(rng.integers(0, 2 ** 32))
    return arr


def expected(model, x, img, prm, thr, cmp_ge):
    """imk_unet_forward -> the label rule in numpy -> aug_oracle, per image"""
    p = model.predict_device(x).cpu().numpy()
    img = img.cpu().numpy()
    sigmoid = model.plan.act_out == "sigmoid"
    imgs, labs = [], []
    for i, q in enumerate(prm):
        if sigmoid:
            with np.errstate(invalid="ignore"):
                lab = np.where(p[i] >= np.float32(thr) if cmp_ge else p[i] > np.float32(thr), 255, 0).astype(np.uint8)      # [H,W,K]
        else:
            lab = np.argmax(p[i], -1).astype(np.uint8)[..., None]
        moved = A.geometric(lab, q.flip_v, q.flip_h, q.rot)
        labs.append(np.moveaxis(moved, -1, 0) if sigmoid else moved[..., 0])
        imgs.append(A.augment(img[i], None, q.flip_v, q.flip_h, q.rot, q.bright_on, q.alpha, q.beta, q.blur_k, q.noise_max, q.seed)[0])
    return np.stack(imgs), np.stack(labs)


def run_case(ns, name, h, w, c, k, alpha, act, geoms, cmp_ge, max_blur=3, max_noise=25, dump=None):
    from inconsistencymasks_amd.unet import UNet
    model = UNet(h, w, c, k, alpha, act, seed=11)
    seed = zlib.crc32(name.encode())
    rng = np.random.default_rng(seed)
    b = len(geoms)
    x = torch.from_numpy(rng.integers(0, 256, (b, h, w, c), dtype=np.uint8)).cuda()
    img = x.flip(-1).contiguous() if c == 3 else x        # what is written differs from what the net is fed (ISIC: BGR)
    prm = params(geoms, seed, max_blur, max_noise)
    tl = ns.TeacherLabel(model, act == "sigmoid")
    out, lab = tl.run(x, img, prm, 0.5, cmp_ge)
    torch.cuda.synchronize()
    want_img, want_lab = expected(model, x, img, prm, 0.5, cmp_ge)
    lab, out = lab.cpu().numpy(), out.cpu().numpy()
    assert lab.shape == want_lab.shape and lab.dtype == np.uint8
    bad = int((lab != want_lab).sum())
    print(f"{name}: {bad} of {lab.size} label bytes differ, {int((out != want_img).sum())} of {out.size} image bytes differ, "
          f"label mean {float(want_lab.mean()):.2f}")
    assert np.array_equal(lab, want_lab), name          # total: no pixel excluded, none within an ulp of the threshold either
    assert np.array_equal(out, want_img), name
    # the unfused route under the materialize debug switch.  That switch also runs the forward's stored input block, whose fp32 sums are
    # taken in another order (tests/test_gpu_unet.py::test_fused_input_block_matches_stored_one: probabilities agree to 2e-3), so the
    # route is held to ITS forward: imk_unet_forward under the same switch -> the rule -> aug_oracle, bit for bit.  The two routes on
    # the SAME forward are compared bit for bit in test_fused_route_equals_unfused_route (IMK_STUDENT_FUSED=0).
    model.debug(materialize=True)
    try:
        out2, lab2 = ns.TeacherLabel(model, act == "sigmoid").run(x, img, prm, 0.5, cmp_ge)
        torch.cuda.synchronize()
        want_img2, want_lab2 = expected(model, x, img, prm, 0.5, cmp_ge)
    finally:
        model.debug(materialize=False)
    lab2 = lab2.cpu().numpy()
    print(f"{name}: unfused under materialize: {int((lab2 != want_lab2).sum())} label bytes differ from its own forward's labels, "
          f"{int((lab2 != lab).sum())} from the fused route's")
    assert np.array_equal(lab2, want_lab2) and np.array_equal(out2.cpu().numpy(), want_img2), name + " (unfused, materialize)"
    assert np.array_equal(want_img2, want_img)
    if dump is not None:
        dump[name + "_img"], dump[name + "_lab"] = out, lab
    return model, x, img


SMALL = [  # (name, h, w, c, K, alpha, act, geometries, cmp_ge)
    ("isic-small", 32, 32, 3, 1, 0.5, "sigmoid", GEOMETRIES, False),
    ("hela-small", 32, 32, 1, 3, 1.0, "sigmoid", GEOMETRIES, True),
    ("suim-small", 32, 32, 3, 9, 1.0, "softmax", GEOMETRIES, False),
    ("cityscapes-rect", 16, 48, 3, 35, 1.0, "softmax", FLIPS * 2, False),
    ("isic-rect", 48, 80, 3, 1, 0.5, "sigmoid", FLIPS + [(1, 1, 2), (1, 0, 0)], False),
    ("suim-narrow", 32, 16, 3, 9, 0.5, "softmax", FLIPS + [(1, 1, 2)], False),
    ("hela-partial-tiles", 48, 48, 1, 3, 0.5, "sigmoid", GEOMETRIES, True),            # W % 64 != 0: partial 64 x 16 tiles
]
# the real sizes at the widths of the schedules' first and last generation (im_driver.NOISY_STUDENT)
REAL = [
    ("isic-a0.5", 256, 256, 3, 1, 0.5, "sigmoid", [(1, 0, 1), (0, 1, 0)], False),
    ("isic-a1.5", 256, 256, 3, 1, 1.5, "sigmoid", [(0, 1, 3), (1, 1, 2)], False),
    ("hela-a1", 256, 256, 1, 3, 1.0, "sigmoid", [(1, 1, 3), (0, 0, 0)], True),
    ("hela-a2", 256, 256, 1, 3, 2.0, "sigmoid", [(0, 0, 1), (1, 0, 2)], True),
    ("suim-a1", 256, 256, 3, 9, 1.0, "softmax", [(0, 1, 0), (0, 0, 0)], False),
    ("suim-a2", 256, 256, 3, 9, 2.0, "softmax", [(0, 1, 0), (0, 0, 0)], False),
    ("cityscapes-a1", 208, 416, 3, 35, 1.0, "softmax", [(0, 1, 0), (0, 0, 0)], False),
    ("cityscapes-a2", 208, 416, 3, 35, 2.0, "softmax", [(0, 0, 0), (0, 1, 0)], False),
]


@pytest.mark.parametrize("case", SMALL + REAL, ids=[c[0] for c in SMALL + REAL])
def test_student_pass_is_bit_identical_to_forward_label_oracle(ns, case):
    run_case(ns, *case)


ROUTE_CASES = SMALL + [REAL[0], REAL[3], REAL[4], REAL[7]]


def test_fused_route_equals_unfused_route(ns, tmp_path):
    """fused == unfused bit for bit on the same forward: a child process with IMK_STUDENT_FUSED=0 (the switch table is read once per
    process) runs the cases through forward -> label -> imk_augment and stores every output; this process runs them fused"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = ("import sys, numpy as np\n"
             "sys.path[:0] = [%r, %r]\n"
             "import test_gpu_noisy_student as T\n"
             "from inconsistencymasks_amd import noisy_student\n"
             "dump = {}\n"
             "for case in T.ROUTE_CASES:\n"
             "    T.run_case(noisy_student, *case, dump=dump)\n"
             "np.savez(sys.argv[1], **dump)\n") % (root, os.path.join(root, "tests"))
    path = str(tmp_path / "unfused.npz")
    env = dict(os.environ, IMK_STUDENT_FUSED="0")
    r = subprocess.run([sys.executable, "-c", child, path], env=env, capture_output=True, text=True, timeout=420, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.environ.get("IMK_STUDENT_FUSED", "1") != "0", "this process must run the fused route"
    fused = {}
    for case in ROUTE_CASES:
        run_case(ns, *case, dump=fused)
    with np.load(path) as unfused:
        assert sorted(unfused.files) == sorted(fused)
        for k in fused:
            assert np.array_equal(fused[k], unfused[k]), k


def test_unfused_shapes_take_the_same_rules(ns):
    """a shape the fused head does not cover (more than 4 sigmoid maps; a plan's H and W are multiples of 16 and its last decoder
    width at most 32, so the other exclusions cannot be reached through a plan)"""
    run_case(ns, "sigmoid-5-maps", 16, 16, 3, 5, 0.5, "sigmoid", GEOMETRIES, True)
    run_case(ns, "sigmoid-5-maps-rect", 16, 32, 3, 5, 0.5, "sigmoid", FLIPS + [(1, 1, 2)], False)


def test_quarter_turn_on_a_rectangle_is_refused(ns):
    from inconsistencymasks_amd._lib import ImkError
    from inconsistencymasks_amd.unet import UNet
    model = UNet(16, 32, 3, 1, 0.5, "sigmoid", seed=1)
    x = torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device="cuda")
    tl = ns.TeacherLabel(model, True)
    with pytest.raises(ImkError) as e:
        tl.run(x, x, params([(0, 0, 1)], 0), 0.5, False)
    assert "-4" in str(e.value) or "unsupported" in str(e.value).lower()
    out, lab = tl.run(x, x, params([(1, 1, 2)], 0), 0.5, False)      # 180 degrees keeps the shape
    assert out.shape == x.shape and lab.shape == (1, 1, 16, 32)


def test_two_calls_on_one_stream_then_one_sync(ns):
    """the call is asynchronous and leaves the stream joined: a second call on the same stream, with other draws and other buffers,
    then ONE synchronisation, gives both results right"""
    from inconsistencymasks_amd.unet import UNet
    h = w = 128
    model = UNet(h, w, 3, 1, 1.0, "sigmoid", seed=5)      # last decoder width 16: the image path forks (width 8 stays on the stream)
    rng = np.random.default_rng(77)
    x = torch.from_numpy(rng.integers(0, 256, (8, h, w, 3), dtype=np.uint8)).cuda()
    img = x.flip(-1).contiguous()
    g1, g2 = GEOMETRIES[:8], GEOMETRIES[8:]
    p1, p2 = params(g1, 1), params(g2, 2)
    for q in list(p1) + list(p2):
        q.blur_k = 7                                   # the long image path: it is still running when the next call is issued
    tl = ns.TeacherLabel(model, True)
    tl.run(x, img, p1, 0.5, False)                     # warm: plans, streams, workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        o1, l1 = tl.run(x, img, p1, 0.5, False)
        o2, l2 = tl.run(x, img, p2, 0.5, False)
        dep = o2.sum() + l2.sum() + o1.sum() + l1.sum()      # work queued on the SAME stream right behind the calls
    s.synchronize()
    w1, wl1 = expected(model, x, img, p1, 0.5, False)
    w2, wl2 = expected(model, x, img, p2, 0.5, False)
    assert np.array_equal(o1.cpu().numpy(), w1) and np.array_equal(l1.cpu().numpy(), wl1)
    assert np.array_equal(o2.cpu().numpy(), w2) and np.array_equal(l2.cpu().numpy(), wl2)
    assert int(dep) == int(w1.sum(dtype=np.int64) + wl1.sum(dtype=np.int64) + w2.sum(dtype=np.int64) + wl2.sum(dtype=np.int64))


# ---- the writers with .predict fakes against the reference's recorded label files ---------------------------------------------
class Fixed:
    def __init__(self, arr):
        self.arr = arr

    def predict(self, x):
        assert x.shape[0] == self.arr.shape[0]
        return self.arr.copy()


def _cases(d, kind):
    return sorted({k.split("_")[0] for k in d if k.startswith(kind) and k[len(kind)].isdigit()})


def _write_inputs(tmp_path, name, h, w, c):
    from inconsistencymasks_amd import functions as F
    src = tmp_path / ("in_" + name)
    src.mkdir(exist_ok=True)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    F.write_png(str(src / name), rng.integers(0, 256, (h, w, c) if c > 1 else (h, w), dtype=np.uint8))
    return str(src)


def _recorded_draws(monkeypatch, draws):
    """the writers draw per file name; the golden cases were drawn from a seeded global stream: hand the recorded geometry in"""
    from inconsistencymasks_amd import noisy_student
    real = noisy_student.draw_for

    def fixed(rngs, *a, **k):
        q = real(rngs, *a, **k)
        q.flip_v, q.flip_h, q.rot = int(draws[0]), int(draws[1]), int(draws[2])
        return q
    monkeypatch.setattr(noisy_student, "draw_for", fixed)


@pytest.mark.parametrize("kind", ["isic", "hela", "mc"])
def test_writers_label_files_equal_the_reference(kind, gold, tmp_path, monkeypatch):
    from inconsistencymasks_amd import functions as F
    d = gold
    for c in _cases(d, kind):
        files = d[c + "_files"].tolist()
        name = files[0].split("/")[1].replace("_aug", "")
        out = tmp_path / c
        _recorded_draws(monkeypatch, d[c + "_draws"])
        free = bool(d[c + "_free"])
        if kind == "isic":
            p = d[c + "_preds"]
            h, w = p.shape[1:3]
            F.create_pseudo_labels_noisy_student_ISIC_2018(Fixed(p), h, w, 3, _write_inputs(tmp_path, name, h, w, 3), str(out), True,
                                                           (0.9, 1.1), (-5, 5), 3, 5, free)
            want = {files[1]: d[c + "_mask"]}
        elif kind == "hela":
            p = d[c + "_preds"]
            h, w = p.shape[1:3]
            F.create_pseudo_labels_noisy_student_hela(Fixed(p), h, w, 1, _write_inputs(tmp_path, name, h, w, 1), str(out), (0.9, 1.1),
                                                      (-3, 3), 2, 10, free)
            want = {files[1]: d[c + "_alive"], files[2]: d[c + "_dead"]}
            assert all(f.endswith("_aug.png") for f in files)
        else:
            p = d[c + "_probs"]
            h, w = p.shape[1:3]
            F.create_pseudo_labels_noisy_student_multiclass(Fixed(p), h, w, 3, _write_inputs(tmp_path, name, h, w, 3), str(out), True,
                                                            (0.9, 1.1), (-5, 5), 1, 5, free)
            want = {files[1]: d[c + "_mask"]}
        F.flush_writes()
        got_files = sorted(os.path.relpath(os.path.join(r, f), out).replace(os.sep, "/") for r, _, fs in os.walk(out) for f in fs)
        assert got_files == sorted(files), c
        for rel, arr in want.items():
            got = F.read_png(str(out / rel), 1)
            assert np.array_equal(np.squeeze(got).astype(np.int64), np.asarray(arr).astype(np.int64)), (c, rel)
        img = F.read_png(str(out / files[0]), 3 if kind != "hela" else 1)
        assert img.shape[:2] == (h, w)
