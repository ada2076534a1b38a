"""The IM over per-image sub-ensembles of a model pool, restated in numpy (a plain helper module): what imk_im_binary_members and
imk_im_multiclass_members (include/imk.h) compute.  Image b carries a member word, bit n set = model n of the pool votes for it.
tests/golden/make_golden_im_members.py records the reference's own get_im_prediction_binary / _hela / _multiclass on the sub-list of
models of every image; tests/test_cpu_im_members.py holds this restatement to those records, tests/test_gpu_im_members.py the kernels.

`defect` plants one of three mistakes a kernel over member words can make, so that the fixture can be shown to tell them apart:
  "nonmembers"  the votes of non-members are counted (binary) / non-members have to agree too (multi-class)
  "n_models"    the vote sum is compared with the size of the pool instead of the number of members
  "anchor0"     the multi-class comparison is anchored on model 0 even where it is not a member
"""
import numpy as np

DEFECTS = ("nonmembers", "n_models", "anchor0")


def member_list(word, n_models):
    """the pool models of a member word, ascending; bits at and above n_models are ignored"""
    return [n for n in range(n_models) if (int(word) >> n) & 1]


def binary(preds, words, thr=0.5, cmp_ge=False, block_out=False, defect=None):
    """preds [N,B,H,W,Kb] float32, words [B] -> masks [B,Kb,H,W] u8 {0,255}, im [B,H,W] u8 {0,255} (max over the maps),
    im_size [B,Kb] i64, pred_size [B,Kb] i64 (counted before blocking)"""
    n_models, b, h, w, kb = preds.shape
    thr = np.float32(thr)
    with np.errstate(invalid="ignore"):
        hit = (preds >= thr) if cmp_ge else (preds > thr)            # NaN votes 0
    masks = np.zeros((b, kb, h, w), np.uint8)
    im = np.zeros((b, h, w), np.uint8)
    im_size, pred_size = np.zeros((b, kb), np.int64), np.zeros((b, kb), np.int64)
    for i in range(b):
        mem = member_list(words[i], n_models)
        cnt = n_models if defect == "n_models" else len(mem)
        voters = list(range(n_models)) if defect == "nonmembers" else mem
        if not mem:
            continue                                                  # nobody votes: no label, no IM, sizes 0
        s = hit[voters, i].sum(0).transpose(2, 0, 1)                  # [Kb,H,W]
        fg = s == cnt
        mx = (s != 0) & ~fg
        pred_size[i], im_size[i] = fg.sum((1, 2)), mx.sum((1, 2))
        any_mx = mx.any(0)
        im[i] = any_mx * np.uint8(255)
        masks[i] = (fg & ~(any_mx[None] & bool(block_out))) * np.uint8(255)
    return masks, im, im_size, pred_size


def multiclass(probs, words, block_out=False, defect=None):
    """probs [N,B,H,W,K] float32, words [B] -> final [B,H,W] u8 class ids, im [B,H,W] u8 {0,255}, im_size [B] i64,
    presence [N,B,K] u8 (0 in the rows of non-members).  np.argmax: the first maximum wins, the first NaN wins."""
    n_models, b, h, w, k = probs.shape
    labels = np.argmax(probs, axis=-1)                                # [N,B,H,W]
    final = np.zeros((b, h, w), np.uint8)
    im = np.zeros((b, h, w), np.uint8)
    im_size = np.zeros((b,), np.int64)
    presence = np.zeros((n_models, b, k), np.uint8)
    for i in range(b):
        mem = member_list(words[i], n_models)
        if not mem:
            continue
        for n in mem:
            presence[n, i, np.unique(labels[n, i])] = 1
        voters = list(range(n_models)) if defect == "nonmembers" else mem
        anchor = labels[0, i] if defect == "anchor0" else labels[voters[0], i]
        agree = np.all(labels[voters, i] == anchor[None], axis=0)
        final[i] = np.where(agree, anchor, 0)
        im[i] = np.where(agree, 0, 255)
        im_size[i] = (~agree).sum()
    return final, im, im_size, presence


def load(path):
    """the fixture as a list of case dicts: kind ('binary' | 'hela' | 'multi'), preds, words and the reference's records"""
    out = []
    with np.load(path) as d:
        for name in d["names"]:
            name = str(name)
            c = {"name": name, "kind": name.split("_")[0]}
            for key in d.files:
                if key.startswith(name + "/"):
                    c[key[len(name) + 1:]] = d[key]
            out.append(c)
    return out


def check_case(c, defect=None):
    """the restatement (with `defect` planted) against the records of one case: the list of images it misses"""
    missed = []
    words = c["words"]
    if c["kind"] in ("binary", "hela"):
        masks, im, im_size, pred_size = binary(c["preds"], words, 0.5, c["kind"] == "hela", False, defect)
        for i in range(len(words)):
            ok = np.array_equal(masks[i], c["masks"][i]) and np.array_equal(im[i], c["im"][i])
            if c["kind"] == "hela":      # the reference returns the summed IM size and no prediction size
                ok = ok and int(im_size[i].sum()) == int(c["im_size"][i])
            else:
                ok = ok and int(im_size[i, 0]) == int(c["im_size"][i]) and int(pred_size[i, 0]) == int(c["pred_size"][i])
            if not ok:
                missed.append(i)
    else:
        final, im, im_size, presence = multiclass(c["preds"], words, False, defect)
        n_models = c["preds"].shape[0]
        for i in range(len(words)):
            mem = member_list(words[i], n_models)
            equal = all(np.array_equal(presence[n, i], presence[mem[0], i]) for n in mem) if mem else True
            ok = (np.array_equal(final[i], c["final"][i]) and np.array_equal(im[i], c["im"][i]) and int(im_size[i]) == int(c["im_size"][i])
                  and bool(equal) == bool(c["lists_equal"][i]))
            if not ok:
                missed.append(i)
    return missed
