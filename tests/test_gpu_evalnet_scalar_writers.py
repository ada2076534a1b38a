"""The writers of the scalar-IoU multiclass EvalNet family on the GPU.

Fed the recorded reference run (tests/golden/evalnet_scalar.npz: probabilities, agreement masks and IMs, EvalNet scores) through
`.predict` fakes, they must write the reference's files, masks, labels.csv lines and kept sets.  Then the selection identities for
class-id candidates (fused == scores + select == the repeated-image route of IMK_SELECT_SHARED=0), and one toy chain of native models
end to end at 64 x 64 with 4 and 9 classes: three U-Nets, both training-data writers (the IM writer on both routes of
IMK_TRAINDATA_POOLED, byte for byte), train_evalnet_multiclass, the ensemble selection writer, the augmentation writer -- each held
to the restated rules (tests/label_cases.py) on the same models' outputs."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import label_cases as LC  # noqa: E402
from inconsistencymasks_amd import evalnet_functions as EF  # noqa: E402
from inconsistencymasks_amd import functions as F  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "evalnet_scalar.npz")) as d:
        return {k: d[k] for k in d.files}


def _lines(path):
    with open(os.path.join(path, "labels.csv"), newline="") as f:
        return [";".join(row) for row in csv.reader(f, delimiter=";")]


def _write_set(root, names, images, masks):
    for sub in ("images", "masks"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for n, img, m in zip(names, images, masks):
        F.write_png(os.path.join(root, "images", n), img)
        F.write_png(os.path.join(root, "masks", n), m)


class RecordedSeg:
    """.predict(x) -> the recorded probabilities of the images of x, found by the index in pixel (0, 0)"""

    def __init__(self, probs):
        self.probs = probs

    def predict(self, x):
        return np.stack([self.probs[int(img[0, 0, 0])] for img in x])


def test_single_writer_on_the_recorded_run(gold, tmp_path):
    names, gt, probs = [str(n) for n in gold["sw_names"]], gold["sw_gt"], gold["sw_probs"]
    h, w = gt.shape[1:]
    images = np.zeros((len(names), h, w, 3), np.uint8)
    images[:, 0, 0] = np.arange(len(names))[:, None]
    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    _write_set(src, names, images, gt)
    for step in (0, 11):
        F.create_training_data_evalnet_multiclass(RecordedSeg(probs), h, w, 3, os.path.join(src, "images"), os.path.join(src, "masks"), out, step,
                                                  rgb=step == 0)
    assert _lines(out) == [str(s) for s in gold["sw_labels"]]
    want = {str(f).split("/", 2)[2] for f in gold["sw_files"]}
    assert {f"{sub}/{n}" for sub in ("images", "masks") for n in os.listdir(os.path.join(out, sub))} == want
    for si, step in enumerate((0, 11)):
        for j, n in enumerate(names):
            assert np.array_equal(F.read_png(os.path.join(out, "masks", LC.pred_name(n, step)), 1)[..., 0], gold["sw_masks"][si, j]), (step, n)
    for n in names:      # the i == 0 copies
        for sub in ("images", "masks"):
            assert open(os.path.join(out, sub, n), "rb").read() == open(os.path.join(src, sub, n), "rb").read()


def test_im_writer_on_the_recorded_run(gold, tmp_path, monkeypatch):
    """the recorded draws, agreement masks and IMs (after the recorded morphology) in the ensemble stage's place: blocking and labels are
    the one imk_label_counts call; the samples the recorded coin does not augment must be the reference's bytes"""
    names, draws = [str(n) for n in gold["imw_names"]], gold["imw_draws"]
    loops, n, h, w = gold["imw_pred"].shape
    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    _write_set(src, names, gold["imw_images"], gold["imw_gt"])
    state = {"loop": -1}

    def plan(rng, n_images, n_models, n_min, n_max):
        state["loop"] += 1
        rows = draws[state["loop"] * n:(state["loop"] + 1) * n]
        return [(tuple(j for j in range(n_models) if int(r[1]) >> j & 1), int(r[2]), int(r[3]), bool(r[4] < 0.5)) for r in rows]

    class Stage:
        def __init__(self, models, pooled):
            self.pooled = True

        def run(self, plan_, subset, idx, x, thr, cmp_ge):
            nl = state["loop"]
            assert (thr, cmp_ge) == (F.THRESHOLD, False)
            return ({"masks": torch.from_numpy(gold["imw_pred"][nl][idx][:, None].copy()).cuda()},
                    torch.from_numpy(gold["imw_im"][nl][idx].copy()).cuda())

    monkeypatch.setattr(EF, "_draw_plan", plan)
    monkeypatch.setattr(EF, "_LoopIM", Stage)
    F.create_training_data_evalnet_im_multiclass([None] * 5, h, w, 3, os.path.join(src, "images"), os.path.join(src, "masks"), out, loops)
    assert _lines(out) == [str(s) for s in gold["imw_labels"]]
    plain = 0
    for nl in range(loops):
        for j, nme in enumerate(names):
            name = f"{nme[:-4]}_aug_{nl}.png"
            img, msk = F.read_png(os.path.join(out, "images", name), 3), F.read_png(os.path.join(out, "masks", name), 1)[..., 0]
            if draws[nl * n + j, 4] >= 0.5:
                plain += 1
                assert np.array_equal(img, gold["imw_out_images"][nl, j]) and np.array_equal(msk, gold["imw_out_masks"][nl, j]), name
    assert 0 < plain < loops * n
    assert sorted(os.listdir(os.path.join(out, "masks"))) == sorted(os.listdir(os.path.join(out, "images")))
    assert len(os.listdir(os.path.join(out, "masks"))) == loops * n


class RecordedEvalNet:
    """.predict([images, one-hot masks]) -> the recorded scores [M,1] of one image's candidates"""

    def __init__(self, scores, k):
        self.scores, self.k = scores, k

    def predict(self, x):
        assert len(x[0]) == len(x[1]) == len(self.scores) and x[1].shape[-1] == self.k and x[1].max() <= 1
        return self.scores.reshape(-1, 1).copy()


def test_selection_writers_on_the_recorded_run(gold, tmp_path):
    k = 4
    for i in range(int(gold["sel_count"])):
        scores, cands, (thr, last, best, keep, n) = gold[f"sel{i}_scores"], gold[f"sel{i}_cands"], gold[f"sel{i}_meta"]
        m, h, w = cands.shape
        root = str(tmp_path / f"c{i}")
        name = f"u_{i:03d}.png"
        os.makedirs(os.path.join(root, "in"))
        F.write_png(os.path.join(root, "in", name), np.full((h, w, 3), i, np.uint8))
        dirs = [os.path.join(root, f"d{j}") for j in range(m - int(last))]
        for j, d in enumerate(dirs):
            os.makedirs(d)
            F.write_png(os.path.join(d, name), cands[j])
        out = os.path.join(root, "out")
        if last:      # the last generation's mask is already in the output's masks/
            os.makedirs(os.path.join(out, "masks"))
            F.write_png(os.path.join(out, "masks", name), cands[-1])
        nets = [RecordedEvalNet(scores[q], k) for q in range(int(n))]
        args = (h, w, 3, k, os.path.join(root, "in"), dirs, out, float(thr))
        if n == 1:
            F.create_training_data_for_segnet_multiclass(nets[0], *args, rgb=bool(i % 2))
        else:
            F.create_training_data_for_segnet_with_ensemble_multiclass(nets, *args, rgb=bool(i % 2))
        assert os.path.isfile(os.path.join(out, "images", name)) == bool(keep), i
        if keep:
            assert np.array_equal(F.read_png(os.path.join(out, "masks", name), 1)[..., 0], gold[f"sel{i}_mask"]), i
            assert open(os.path.join(out, "images", name), "rb").read() == open(os.path.join(root, "in", name), "rb").read()
        elif last:
            assert np.array_equal(F.read_png(os.path.join(out, "masks", name), 1)[..., 0], cands[-1]), i
        else:
            assert os.listdir(os.path.join(out, "masks")) == [], i


# ---- selection identities for class-id candidates ------------------------------------------------------------------------------------
def run_identity_case(dump):
    """N = 3 one-head one-hot EvalNets, M = 6 class-id candidates: fused == scores + select, and the restated rule on those scores"""
    from inconsistencymasks_amd import evalnet as ev
    b, m, h, w, k = 3, 6, 64, 64, 9
    models = [ev.get_evalnet(h, w, 3, k, 0.5, seed=70 + j) for j in range(3)]
    rng = np.random.default_rng(8)
    xa = torch.from_numpy(np.stack([np.clip(rng.integers(0, 60, (h, w, 3)) + 90 * i, 0, 255) for i in range(b)]).astype(np.uint8)).cuda()
    xb = torch.from_numpy(rng.integers(0, k, (b, m, h // 8, w // 8), dtype=np.uint8).repeat(8, 2).repeat(8, 3)).cuda().contiguous()
    cand = xb.reshape(b, m, h * w).contiguous()
    counts = torch.tensor([m, m - 1, 1], dtype=torch.int32, device="cuda")
    scorer = ev.CandidateScorer(models)
    assert scorer.shared
    composed_scores = scorer.scores(xa, xb)
    thr = float(composed_scores[..., 0].mean(0).max(1).values.median())
    for tag, cnt in (("counts", counts), ("all", None)):
        fused = scorer.run(xa, xb, cand, thr, cnt, ev.SELECT_IOU)
        composed = ev.select_candidates(composed_scores, cand, thr, ev.SELECT_IOU, cnt)
        torch.cuda.synchronize()
        assert torch.equal(scorer.last_scores.view(torch.int32), composed_scores.view(torch.int32)), tag
        s = composed_scores.cpu().numpy()[..., 0]
        for f, c, what in zip(fused, composed, ("best_idx", "best_score", "keep", "out")):
            assert f.cpu().numpy().tobytes() == c.cpu().numpy().tobytes(), (tag, what)
            dump[f"{tag}_{what}"] = f.cpu().numpy()
        for i in range(b):
            n_c = m if cnt is None else int(cnt[i])
            best, score, keep = LC.select(s[:, i, :n_c], thr)
            assert (int(fused[0][i]), bool(fused[2][i])) == (best, keep) and fused[1][i].cpu().numpy().tobytes() == score.tobytes(), (tag, i)
            assert torch.equal(fused[3][i], cand[i, best])
    dump["scores"] = composed_scores.cpu().numpy()


def test_fused_equals_composed_and_repeated_route(tmp_path):
    child = ("import sys, numpy as np\n"
             "sys.path[:0] = [%r, %r]\n"
             "import test_gpu_evalnet_scalar_writers as T\n"
             "dump = {}\n"
             "T.run_identity_case(dump)\n"
             "np.savez(sys.argv[1], **dump)\n") % (ROOT, os.path.join(ROOT, "tests"))
    path = str(tmp_path / "repeated.npz")
    r = subprocess.run([sys.executable, "-c", child, path], env=dict(os.environ, IMK_SELECT_SHARED="0"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.environ.get("IMK_SELECT_SHARED", "1") != "0", "this process must run the shared-tower route"
    fused = {}
    run_identity_case(fused)
    with np.load(path) as rep:
        assert sorted(rep.files) == sorted(fused)
        for key in fused:
            assert rep[key].tobytes() == fused[key].tobytes(), key
    assert set(np.concatenate([fused["counts_keep"], fused["all_keep"]]).tolist()) == {0, 1}, "both keep values must occur"


# ---- one toy chain end to end -----------------------------------------------------------------------------------------------------------
def _blobs(rng, h, w, k):
    m = np.zeros((h, w), np.uint8)
    for c in range(1, k):
        y, x = int(rng.integers(0, h - 16)), int(rng.integers(0, w - 16))
        m[y:y + int(rng.integers(8, 24)), x:x + int(rng.integers(8, 24))] = c
    return m


def _tree_bytes(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(root) for f in fs}


@pytest.mark.parametrize("k", [4, 9])
def test_toy_chain(tmp_path, monkeypatch, k):
    from inconsistencymasks_amd.evalnet import get_evalnet
    from inconsistencymasks_amd.unet import UNet
    h = w = 64
    rng = np.random.default_rng(k)
    names = [f"l_{i:03d}.png" for i in range(6)]
    images = rng.integers(0, 256, (len(names), h, w, 3)).astype(np.uint8)
    gts = np.stack([_blobs(rng, h, w, k) for _ in names])
    src = str(tmp_path / "labelled")
    _write_set(src, names, images, gts)
    simg, smsk = os.path.join(src, "images"), os.path.join(src, "masks")
    unets = [UNet(h, w, 3, k, 0.5, "softmax", seed=11 + j) for j in range(3)]

    # 2a. the single-model writer, against the restated label on the model's own probabilities
    data = str(tmp_path / "evalnet_data")
    for i, net in enumerate(unets[:2]):
        F.create_training_data_evalnet_multiclass(net, h, w, 3, simg, smsk, data, i)
    want = []
    for i, net in enumerate(unets[:2]):
        pred = np.argmax(net.predict_device(torch.from_numpy(images).cuda()).cpu().numpy(), -1).astype(np.uint8)
        for j, n in enumerate(names):
            want.append(f"{LC.pred_name(n, i)};{LC.rounded(LC.counts(pred[j], gts[j]))}")
            assert np.array_equal(F.read_png(os.path.join(data, "masks", LC.pred_name(n, i)), 1)[..., 0], pred[j])
        if i == 0:
            want += [f"{n};1.0" for n in names]
    assert _lines(data) == want

    # 2b. the IM writer: one fused call per chunk on the pooled route and on the grouped one, byte for byte; labels restated
    routes = {}
    for pooled in (True, False):
        monkeypatch.setattr(EF, "POOLED", pooled)
        routes[pooled] = str(tmp_path / f"im_data_{int(pooled)}")
        F.create_training_data_evalnet_im_multiclass(unets, h, w, 3, simg, smsk, routes[pooled], 2, n_min_models=2, n_max_models=3, seed=5)
    monkeypatch.setattr(EF, "POOLED", True)
    assert _tree_bytes(routes[True]) == _tree_bytes(routes[False]) and len(_lines(routes[True])) == 2 * len(names)
    labels = [float(line.split(";")[1]) for line in _lines(routes[True])]
    assert all(0.0 <= v <= 1.0 for v in labels) and len(set(labels)) > 1
    F.create_training_data_evalnet_im_multiclass(unets, h, w, 3, simg, smsk, data, 1, n_min_models=2, n_max_models=3, seed=6)
    assert len(_lines(data)) == 4 * len(names)

    # 3. train_evalnet_multiclass: finite (mse, mae), a checkpoint that loads and scores
    evalnet = get_evalnet(h, w, 3, k, 0.5, seed=21)
    assert evalnet.plan.b_onehot == (k > 4)
    ckpt = str(tmp_path / "evalnet.h5")
    mse, mae = F.train_evalnet_multiclass(evalnet, data, data, ckpt, 4, k, 2, seed=1)
    assert np.isfinite([mse, mae]).all() and mse >= 0 and mae >= 0
    nets = [F.load_evalnet(ckpt), get_evalnet(h, w, 3, k, 0.5, seed=22)]

    # 4. the ensemble selection writer against the restated rule on the nets' predict outputs
    dirs = [os.path.join(data, "cand0"), os.path.join(data, "cand1"), os.path.join(data, "cand2")]
    cands = rng.integers(0, k, (3, len(names), h // 8, w // 8), dtype=np.uint8).repeat(8, 2).repeat(8, 3)
    for d, stack in zip(dirs, cands):
        os.makedirs(d)
        for n, m in zip(names, stack):
            F.write_png(os.path.join(d, n), m)
    onehot = lambda ids: np.stack([ids == c for c in range(k)], -1).astype(np.uint8)
    scores = np.stack([np.stack([e.predict([images, ids if e.plan.b_onehot else onehot(ids)])[:, 0] for ids in cands], 1) for e in nets])
    best = [LC.select(scores[:, j], 0.0) for j in range(len(names))]
    thr = float(np.sort([b[1] for b in best])[len(names) // 2])
    selected = str(tmp_path / "selected")
    F.create_training_data_for_segnet_with_ensemble_multiclass(nets, h, w, 3, k, simg, dirs, selected, thr)
    kept = {n for j, n in enumerate(names) if LC.select(scores[:, j], thr)[2]}
    assert 0 < len(kept) and set(os.listdir(os.path.join(selected, "images"))) == set(os.listdir(os.path.join(selected, "masks"))) == kept
    for j, n in enumerate(names):
        if n in kept:
            assert np.array_equal(F.read_png(os.path.join(selected, "masks", n), 1)[..., 0], cands[best[j][0], j]), n

    # 5. the augmentation writer: the number of copies follows the one net's predicted IoU of (image, chosen mask)
    aug = str(tmp_path / "augmented")
    one = nets[0]
    chosen = np.stack([F.read_png(os.path.join(selected, "masks", n), 1)[..., 0] for n in sorted(kept)])
    pred_iou = one.predict([np.stack([images[names.index(n)] for n in sorted(kept)]), chosen if one.plan.b_onehot else onehot(chosen)])[:, 0]
    lo, hi = float(pred_iou.min()) - 0.01, float(pred_iou.max()) + 0.01
    F.create_augment_images_and_masks_with_evalnet_multiclass(one, h, w, 3, k, lo, hi, selected, aug)
    want_files = {f"{n[:-4]}___{j}.png" for n, v in zip(sorted(kept), pred_iou) for j in range(LC.num_augs(v, lo, hi))}
    assert set(os.listdir(os.path.join(aug, "images"))) == set(os.listdir(os.path.join(aug, "masks"))) == want_files
    for f in want_files:      # geometry and photometry leave a class-id mask a class-id mask
        assert F.read_png(os.path.join(aug, "masks", f), 1).max() < k
