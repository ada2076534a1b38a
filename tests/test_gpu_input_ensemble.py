"""GPU tests of the input-ensemble baseline: imk_views against oracle/aug_oracle.py's pieces composed in data_augmentation_image's
order, the unfused view votes and the functions of record against the reference's recorded outputs
(tests/golden/input_ensemble.npz), and the fused route of imk_unet_forward_views_vote against forward + unfused vote."""
import random
import zlib

import numpy as np
import pytest
import torch

from oracle import aug_oracle as A

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def ie():
    from inconsistencymasks_amd import input_ensemble
    return input_ensemble


@pytest.fixture(scope="module")
def gold():
    from test_golden_input_ensemble import load
    return load()


def _cases(d, kind):
    return sorted({k.split("_")[0] for k in d if k.startswith(kind) and k[len(kind)].isdigit()})


def view_oracle(ie, img, q):
    """data_augmentation_image after the op, from aug_oracle's pieces: geometry -> blur -> noise -> convertScaleAbs"""
    a = ie.apply_op(img, q.op)
    a = A.gaussian_blur(a, q.blur_k)
    if q.noise_max > 0:
        a = A.apply_noise(a, A.noise_field(a.shape, q.noise_max, q.seed))
    if q.bright_on:
        a = A.convert_scale_abs(a, q.alpha, q.beta)
    return a


def params(ie, op=0, blur=0, noise=0, seed=0, coin=0, alpha=1.0, beta=0.0):
    from inconsistencymasks_amd import _lib
    q = _lib.ViewParams()
    q.op, q.blur_k, q.noise_max, q.seed, q.bright_on, q.alpha, q.beta = op, blur, noise, seed, coin, alpha, beta
    return q


# ---- view generator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_views_geometry_all_ops(ie, c):
    rng = np.random.default_rng(c)
    x = rng.integers(0, 256, (2, 24, 24, c), dtype=np.uint8)
    per = [[params(ie, op) for op in range(13)] for _ in range(2)]
    v = ie.make_views(torch.from_numpy(x).cuda(), ie.ViewPlan(per)).cpu().numpy()
    for b in range(2):
        for op in range(13):
            assert np.array_equal(v[op, b], ie.apply_op(x[b], op)), (b, op)


@pytest.mark.parametrize("c", [1, 3])
def test_views_pixel_chain(ie, c):
    rng = np.random.default_rng(10 + c)
    h = w = 32
    x = rng.integers(0, 256, (3, h, w, c), dtype=np.uint8)
    per = []
    for b in range(3):
        views = []
        for blur in (0, 3, 5, 7):
            for coin in (0, 1):
                for noise in (0, 25):
                    views.append(params(ie, int(rng.integers(0, 13)), blur, noise, int(rng.integers(0, 2 ** 32)), coin,
                                        float(rng.uniform(0.5, 1.5)), float(rng.uniform(-25, 25))))
        per.append(views)
    v = ie.make_views(torch.from_numpy(x).cuda(), ie.ViewPlan(per)).cpu().numpy()
    for b in range(3):
        for m, q in enumerate(per[b]):
            assert np.array_equal(v[m, b], view_oracle(ie, x[b], q)), (b, m, q.op, q.blur_k, q.noise_max, q.bright_on)


def test_views_large_identity(ie):
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, (1, 208, 416, 3), dtype=np.uint8)
    q = params(ie, 0, 5, 15, 1234, 1, 1.2, -7.5)
    v = ie.make_views(torch.from_numpy(x).cuda(), ie.ViewPlan([[q]])).cpu().numpy()
    assert np.array_equal(v[0, 0], view_oracle(ie, x[0], q))


def test_views_chain_equals_single_steps(ie):
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, (2, 16, 48, 1), dtype=np.uint8)
    random.seed(5)
    per = [ie.draw_chain_views(4, np_rng=np.random.RandomState(b)) for b in range(2)]
    v = ie.make_views(torch.from_numpy(x).cuda(), ie.ViewPlan(per, chain=True)).cpu().numpy()
    for b in range(2):
        cur = x[b]
        for m, q in enumerate(per[b]):
            cur = view_oracle(ie, cur, q)
            assert np.array_equal(v[m, b], cur), (b, m)


def test_views_refuse_quarter_turn_on_rectangles(ie):
    from inconsistencymasks_amd._lib import ImkError
    x = torch.zeros((1, 16, 32, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ImkError):
        ie.make_views(x, ie.ViewPlan([[params(ie, 1)]]))
    v = ie.make_views(x, ie.ViewPlan([[params(ie, 2)]]))       # 180 degrees keeps the shape
    assert v.shape == (1, 1, 16, 32, 3)


# ---- unfused votes against the reference -------------------------------------------------------------------------------------
def test_unfused_votes_match_golden(ie, gold):
    from inconsistencymasks_amd import vote
    d = gold
    for c in _cases(d, "isic"):
        p = torch.from_numpy(d[c + "_preds"][:, None]).cuda()
        out = ie.vote_views_binary(p, d[c + "_ops"][:, None], float(d[c + "_thr"]), True)[0, 0].cpu().numpy()
        assert np.array_equal(out, d[c + "_out"]), c
    for c in _cases(d, "hela"):
        p = torch.from_numpy(d[c + "_preds"][:, None]).cuda()
        m = vote.vote_binary(p, float(d[c + "_thr"]), bool(d[c + "_soft"]))[0].cpu().numpy()
        assert np.array_equal(m[0], d[c + "_alive"]) and np.array_equal(m[1], d[c + "_dead"]) and np.array_equal(m[2], d[c + "_pos"]), c
    for c in _cases(d, "mc"):
        p = torch.from_numpy(d[c + "_probs"][:, None]).cuda()
        assert np.array_equal(vote.vote_multiclass(p, True)[0].cpu().numpy(), d[c + "_soft"]), c
        assert np.array_equal(ie.vote_views_majority(p)[0].cpu().numpy(), d[c + "_major"]), c


# ---- functions of record with .predict fakes ---------------------------------------------------------------------------------
class Fixed:
    def __init__(self, arr):
        self.arr = arr

    def predict(self, x):
        assert x.shape[0] == self.arr.shape[0]
        return self.arr.copy()


def test_functions_of_record_match_golden(gold):
    from inconsistencymasks_amd import functions as F
    d = gold
    for c in _cases(d, "isic"):
        preds = d[c + "_preds"]
        n, h, w = preds.shape[:3]
        random.seed(int(d[c + "_seed"]))
        out = F.get_input_ensemble_prediction_ISIC_2018(Fixed(preds), np.zeros((h, w, 3), np.uint8), h, w, 3, float(d[c + "_thr"]), n,
                                                        use_n_rnd_transformations=n != 13)
        assert out.dtype == np.uint8 and np.array_equal(out, d[c + "_out"]), c
        if n == 13:
            assert np.array_equal(F.input_ensemble_prediction(Fixed(preds), np.zeros((h, w, 3), np.uint8), h, w, 3, 0.5), d[c + "_out"])
    for c in _cases(d, "hela"):
        preds = d[c + "_preds"]
        n, h, w = preds.shape[0] - 1, preds.shape[1], preds.shape[2]
        fn = F.get_input_ensemble_prediction_hela_soft if d[c + "_soft"] else F.get_input_ensemble_prediction_hela_hard
        random.seed(int(d[c + "_seed"]))
        alive, dead, pos = fn(Fixed(preds), np.zeros((h, w), np.uint8), h, w, 1, n, threshold=float(d[c + "_thr"]))
        assert np.array_equal(alive, d[c + "_alive"]) and np.array_equal(dead, d[c + "_dead"]), c
        assert pos.shape == (h, w, 3)
    for c in _cases(d, "mc"):
        probs = d[c + "_probs"]
        n, h, w = probs.shape[0] - 1, probs.shape[1], probs.shape[2]
        random.seed(int(d[c + "_seed"]))
        assert np.array_equal(F.get_input_ensemble_prediction_multiclass_soft(Fixed(probs), np.zeros((h, w, 3), np.uint8), h, w, 3, n),
                              d[c + "_soft"]), c
        assert np.array_equal(F.get_input_ensemble_prediction_multiclass(Fixed(probs), np.zeros((h, w, 3), np.uint8), h, w, 3, n),
                              d[c + "_major"]), c


def test_data_augmentation_image_shape():
    from inconsistencymasks_amd import functions as F
    x = np.random.default_rng(0).integers(0, 256, (32, 32), dtype=np.uint8)
    random.seed(0)
    y = F.data_augmentation_image(x, 1, 15, (0.7, 1.3), (-15, 15))
    assert y.shape == x.shape and y.dtype == np.uint8


# ---- fused route against forward + unfused vote ------------------------------------------------------------------------------
def _unfused(ie, model, x, plan, thr, mode, cmp_ge):
    from inconsistencymasks_amd import vote
    views = ie.make_views(x, plan)
    m, b = plan.n_views, plan.batch
    p = model.predict_device(views.reshape(m * b, *views.shape[2:]))
    preds = p.reshape(m, b, *p.shape[1:]).contiguous()
    if plan.restore:
        return ie.vote_views_binary(preds, plan.ops.reshape(m, b), thr, cmp_ge)
    if mode == ie.VOTE_MAJORITY:
        return ie.vote_views_majority(preds)
    if model.plan.act_out == "sigmoid":
        if cmp_ge and mode == vote.VOTE_HARD:
            return ie.vote_views_binary(preds, None, thr, True)
        return vote.vote_binary(preds, thr, mode == vote.VOTE_SOFT)
    return vote.vote_multiclass(preds, mode == vote.VOTE_SOFT)


FUSED = [  # (h, w, c, K, alpha, act, chain, mode, cmp_ge, M list, batch)
    ("isic", 64, 64, 3, 1, 0.5, "sigmoid", False, 0, True, (1, 3, 7, 13, 16, 17), 3),
    ("isic-a1", 32, 32, 3, 1, 1.0, "sigmoid", False, 0, True, (5,), 2),
    ("isic-a1.5", 32, 32, 3, 1, 1.5, "sigmoid", False, 0, True, (3,), 3),
    ("isic-a2", 32, 32, 3, 1, 2.0, "sigmoid", False, 0, True, (7,), 1),
    ("hela-hard", 32, 32, 1, 3, 0.5, "sigmoid", True, 0, False, (3, 8, 9), 3),
    ("hela-soft", 32, 32, 1, 3, 0.5, "sigmoid", True, 1, False, (4,), 2),
    ("suim", 32, 48, 3, 8, 0.5, "softmax", True, 1, False, (4, 9), 3),
    ("suim-major", 32, 48, 3, 8, 0.5, "softmax", True, 2, False, (6,), 2),
    ("cityscapes", 208, 416, 3, 35, 0.5, "softmax", True, 1, False, (4,), 1),
]


@pytest.mark.parametrize("case", FUSED, ids=[f[0] for f in FUSED])
def test_fused_route_equals_forward_plus_vote(ie, case):
    from inconsistencymasks_amd.unet import UNet
    name, h, w, c, k, alpha, act, chain, mode, cmp_ge, ms, b = case
    model = UNet(h, w, c, k, alpha, act, seed=7)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = torch.from_numpy(rng.integers(0, 256, (b, h, w, c), dtype=np.uint8)).cuda()
    vv = ie.ViewVote(model, act == "sigmoid")
    for m in ms:
        random.seed(m)
        if chain:
            per = [ie.draw_chain_views(m - 1, np_rng=np.random.RandomState(i)) for i in range(b)]
        else:
            per = [ie.all_views()[:m] if m <= 13 else ie.draw_random_views(m, np_rng=np.random.RandomState(i)) for i in range(b)]
            per = [ie.draw_random_views(m, np_rng=np.random.RandomState(i)) if i % 2 else per[i] for i in range(b)]
        plan = ie.ViewPlan(per, chain=chain, restore=not chain)
        got = vv.run(x, plan, 0.5, mode, cmp_ge)
        want = _unfused(ie, model, x, plan, 0.5, mode, cmp_ge)
        torch.cuda.synchronize()
        assert got.shape == want.shape
        assert torch.equal(got, want), (name, m)
