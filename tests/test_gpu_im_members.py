"""The IM over per-image sub-ensembles on the GPU, bit-exact:

  1. imk_im_binary_members / imk_im_multiclass_members against tests/golden/im_members.npz (the reference's own functions on the
     sub-list of models of every image), with blocking on and off against tests/im_members_cases.py, and with every bit set against
     imk_im_binary / imk_im_multiclass;
  2. imk_unet_forward_im_members (functions.PoolIM) == the models' own forwards + the kernels of 1 == functions.EnsembleIM on every
     group of images that share a member set, on the fused route and on the unfused one (an image with more than 8 members);
  3. imk_morph_var against imk_morph, image by image.

Every comparison is an equality of bytes; there is no tolerance."""
import os
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

import im_members_cases as MC  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "im_members.npz")
_CACHE = {}


def cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = {c["name"]: c for c in MC.load(GOLDEN)}
    return _CACHE["cases"]


CASE_NAMES = ("binary_n5", "binary_n16", "binary_n2", "hela_n10", "multi_k3_n5", "multi_k9_n10", "multi_k35_n16", "multi_k3_n2")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def eq(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {got.size} element(s) differ"


# ---- 1. the rule on a probability stack ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_stack_rule_against_the_reference_records(name):
    from inconsistencymasks_amd import im as IM
    c = cases()[name]
    preds, words = dev(c["preds"]), c["words"]
    b = len(words)
    if c["kind"] == "multi":
        r = IM.im_multiclass_members(preds, words, None, False, False, want_presence=True)
        eq(r["final"], c["final"], "final")
        eq(r["im"], c["im"], "im")
        eq(r["im_size"], c["im_size"], "im_size")
        pres = r["presence"].cpu().numpy()
        n = preds.shape[0]
        for i in range(b):
            mem = MC.member_list(words[i], n)
            assert not pres[[j for j in range(n) if j not in mem], i].any(), "presence of a non-member"
            equal = all(np.array_equal(pres[j, i], pres[mem[0], i]) for j in mem) if mem else True
            assert equal == bool(c["lists_equal"][i]), (i, "unique-set filter")
    else:
        hela = c["kind"] == "hela"
        r = IM.im_binary_members(preds, words, 0.5, hela, None, False, False)
        eq(r["masks"], c["masks"], "masks")
        eq(r["im"], c["im"], "im")
        if hela:
            eq(r["im_size"].sum(1), c["im_size"], "summed im_size")
        else:
            eq(r["im_size"][:, 0], c["im_size"], "im_size")
            eq(r["pred_size"][:, 0], c["pred_size"], "pred_size")


@pytest.mark.parametrize("block_in,block_out", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_stack_rule_with_blocking_and_both_comparisons(name, block_in, block_out):
    from inconsistencymasks_amd import im as IM
    c = cases()[name]
    preds, words = dev(c["preds"]), c["words"]
    _, b, h, w, _ = c["preds"].shape
    rng = np.random.default_rng(h * w + b)
    for ch in (1, 3):
        img = rng.integers(1, 256, (b, h, w, ch), dtype=np.uint8)

        def image_and_im(r, im):
            eq(r["im"], im, "im")
            eq(r["img_out"], np.where((im > 0)[..., None] & block_in, 0, img), "img_out")
        if c["kind"] == "multi":
            r = IM.im_multiclass_members(preds, words, dev(img), block_in, block_out, want_presence=True)
            final, im, size, pres = MC.multiclass(c["preds"], words, block_out)
            eq(r["final"], final, "final")
            eq(r["presence"], pres, "presence")
            eq(r["im_size"], size, "im_size")
            image_and_im(r, im)
        else:
            for ge in (False, True):
                r = IM.im_binary_members(preds, words, 0.5, ge, dev(img), block_in, block_out)
                masks, im, im_size, pred_size = MC.binary(c["preds"], words, 0.5, ge, block_out)
                eq(r["masks"], masks, f"masks ge={ge}")
                eq(r["im_size"], im_size, "im_size")
                eq(r["pred_size"], pred_size, "pred_size")
                image_and_im(r, im)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_bit_set_is_the_whole_ensemble_kernel(name):
    from inconsistencymasks_amd import im as IM
    c = cases()[name]
    preds = dev(c["preds"])
    n, b, h, w, _ = c["preds"].shape
    img = dev(np.random.default_rng(n).integers(1, 256, (b, h, w, 3), dtype=np.uint8))
    full = np.full(b, 0xFFFFFFFF, np.uint32)                 # the bits above the pool are ignored
    if c["kind"] == "multi":
        got, want = IM.im_multiclass_members(preds, full, img, True, True), IM.im_multiclass(preds, img, True, True)
    else:
        ge = c["kind"] == "hela"
        got, want = IM.im_binary_members(preds, full, 0.5, ge, img, True, True), IM.im_binary(preds, 0.5, ge, img, True, True)
    for key in want:
        eq(got[key], want[key], key)


# The generic (odd-size) kernels: 35 x 21 and 17 x 9 are no multiple of 4 pixels, and Kb 2 takes the generic kernel at any size.
@pytest.mark.parametrize("kind,n,b,h,w,k", [("binary", 5, 3, 35, 21, 1), ("binary", 5, 3, 35, 21, 2), ("multi", 5, 3, 17, 9, 4)])
def test_ragged_stacks_are_the_whole_ensemble_kernel_on_the_members(kind, n, b, h, w, k):
    from inconsistencymasks_amd import im as IM
    rng = np.random.default_rng(1000 * h + 10 * w + k)
    # the models share a base so that agreement and disagreement both occur
    stack = (0.6 * rng.random((1, b, h, w, k)) + 0.4 * rng.random((n, b, h, w, k))).astype(np.float32)
    img_np = rng.integers(1, 256, (b, h, w, 3), dtype=np.uint8)
    img = dev(img_np)

    def whole(s):
        return IM.im_multiclass(dev(s), img, True, True) if kind == "multi" else IM.im_binary(dev(s), 0.5, k == 2, img, True, True)

    def members(words):
        if kind == "multi":
            return IM.im_multiclass_members(dev(stack), words, img, True, True)
        return IM.im_binary_members(dev(stack), words, 0.5, k == 2, img, True, True)
    got, want = members(np.full(b, (1 << n) - 1, np.uint32)), whole(stack)
    assert set(got) == set(want)
    for key in want:
        eq(got[key], want[key], f"all bits: {key}")
    # every image under every word: the whole-ensemble kernel on the word's models, image by image
    words = [0b101, 1 << (n - 1), 0]
    sub = {word: (MC.member_list(word, n), whole(stack[MC.member_list(word, n)])) for word in words if word}
    for shift in range(b):
        per_image = [words[(i + shift) % len(words)] for i in range(b)]
        got = members(np.array(per_image, np.uint32))
        for i, word in enumerate(per_image):
            for key in got:
                row = got[key][:, i] if key == "presence" else got[key][i]
                if word == 0:                                # nobody votes: all zero, the image copied
                    eq(row, img_np[i] if key == "img_out" else torch.zeros_like(row), f"word 0, image {i}: {key}")
                    continue
                mem, ref = sub[word]
                if key == "presence":
                    eq(row[mem], ref[key][:, i], f"word {word:#b}, image {i}: presence of the members")
                    assert not row[[j for j in range(n) if j not in mem]].any(), "presence of a non-member"
                else:
                    eq(row, ref[key][i], f"word {word:#b}, image {i}: {key}")


def test_wrappers_refuse_bad_members_before_upload():
    from inconsistencymasks_amd import im as IM
    with pytest.raises(ValueError):
        IM.member_words([[0, 5]], 1, 5)                      # member 5 of a pool of 5
    with pytest.raises(ValueError):
        IM.member_words([1, 2], 3, 4)                        # two sets for three images
    with pytest.raises(ValueError):
        IM.member_words([1], 1, 17)
    assert IM.member_words([[0, 2], 6, []], 3, 4).tolist() == [5, 6, 0]


# ---- 2. the fused ensemble call -----------------------------------------------------------------------------------------------------
# (h, w, c, k, alpha, head), pool, batch, cmp_ge: 32 x 32 is one 1024-pixel chunk exactly, 16 x 48 a partial one, 48 x 80 several and a
# partial one; alpha 0.5 and 1; sigmoid K 1 and 3 with both comparisons; softmax K 3, 9 and 35; pools of 2, 5, 10 and 16; batch 5 .. 7
POOLS = [
    ((32, 32, 3, 1, 0.5, "sigmoid"), 5, 5, False),
    ((16, 48, 1, 3, 1.0, "sigmoid"), 10, 6, True),
    ((48, 80, 3, 1, 1.0, "sigmoid"), 16, 7, True),
    ((32, 32, 1, 3, 0.5, "sigmoid"), 2, 5, False),
    ((16, 48, 3, 3, 0.5, "softmax"), 5, 7, False),
    ((48, 80, 3, 9, 1.0, "softmax"), 10, 5, False),
    ((32, 32, 3, 35, 1.0, "softmax"), 16, 6, False),
    ((32, 32, 3, 9, 0.5, "softmax"), 2, 5, False),
]
POOL_IDS = [f"{c[0]}x{c[1]}c{c[2]}k{c[3]}a{c[4]}-n{n}-b{b}" for c, n, b, _ in POOLS]


def pool_models(cfg, n):
    from inconsistencymasks_amd.unet import UNet
    from tests.test_gpu_unet import randomize_bn
    key = (cfg, n)
    if key not in _CACHE:
        models = []
        for j in range(n):
            m = UNet(*cfg, seed=101 + 7 * j)
            m.load_state_dict(randomize_bn(m.state_dict(), 201 + j))
            m.ready_for_inference()
            models.append(m)
        torch.cuda.synchronize()
        _CACHE[key] = models
    return _CACHE[key]


def member_sets(n, batch, many):
    """many = False: at most 8 members everywhere (the fused route): disjoint sets in neighbouring images, nobody, bits above the
    pool, only the highest bit (one member), all members (pools of up to 8; batch 6 and 7), a set shared by two images (batch 7).
    many = True: image 0 has more than 8 members (pools of 10 and 16) or the whole pool: the call takes the unfused route."""
    full = (1 << n) - 1
    even = sum(1 << j for j in range(0, n, 2))
    small = lambda v: v if bin(v).count("1") <= 8 else v & 0xFF    # noqa: E731
    above = (0b11 & full) | ((0x5A5 << n) & 0xFFFFFFFF)
    words = [small(even), small(full & ~even), 0, above, 1 << (n - 1), small(full), small(even)]
    if many:
        words = [full if n <= 8 else full & ~1] + words
    return np.array(words[:batch], np.uint32)


@pytest.mark.parametrize("block", [True, False])
@pytest.mark.parametrize("many", [False, True], ids=["fused", "over8"])
@pytest.mark.parametrize("cfg,n,b,ge", POOLS, ids=POOL_IDS)
def test_pool_call_equals_own_forwards_and_group_ensembles(cfg, n, b, ge, many, block):
    from inconsistencymasks_amd import functions as F
    from inconsistencymasks_amd import im as IM
    models = pool_models(cfg, n)
    h, w, c, k, _, head = cfg
    binary = head == "sigmoid"
    rng = np.random.default_rng(h + 3 * w + n + b)
    x = dev(rng.integers(0, 256, (b, h, w, c), dtype=np.uint8))
    words = member_sets(n, b, many)
    got = F.PoolIM(models).run(x, words, 0.5, ge, block, block, want_presence=True)
    torch.cuda.synchronize()
    # the models' own forwards on the whole batch + the rule on the stack
    stack = torch.stack([m.predict_device(x) for m in models], 0).contiguous()
    if binary:
        want = IM.im_binary_members(stack, words, 0.5, ge, x, block, block)
        for key in ("masks", "im", "im_size", "pred_size", "img_out"):
            eq(got[key], want[key], f"own forwards: {key}")
    else:
        want = IM.im_multiclass_members(stack, words, x, block, block, want_presence=True)
        eq(got["masks"][:, 0], want["final"], "own forwards: final")
        eq(got["im_size"][:, 0], want["im_size"], "own forwards: im_size")
        for key in ("im", "presence", "img_out"):
            eq(got[key], want[key], f"own forwards: {key}")
    # every group of images that share a member set: the whole-batch ensemble call on that set
    groups = {}
    for i, word in enumerate(words):
        groups.setdefault(tuple(MC.member_list(word, n)), []).append(i)
    for mem, idx in groups.items():
        if not mem:
            assert not got["masks"][idx].any() and not got["im"][idx].any() and not got["im_size"][idx].any()
            eq(got["img_out"][idx], x[idx], "nobody votes: the image is copied")
            continue
        r = F.EnsembleIM([models[j] for j in mem]).run(x[idx].contiguous(), 0.5, ge, block, block, want_presence=True)
        for key in ("masks", "im", "im_size", "img_out") + (("pred_size",) if binary else ()):
            eq(got[key][idx], r[key], f"group {mem}: {key}")
        if not binary:
            eq(got["presence"][list(mem)][:, idx], r["presence"], f"group {mem}: presence")


def test_pool_call_takes_the_unfused_route_under_materialize():
    from inconsistencymasks_amd import functions as F
    cfg, n, b, ge = POOLS[1]
    models = pool_models(cfg, n)
    x = dev(np.random.default_rng(5).integers(0, 256, (b, cfg[0], cfg[1], cfg[2]), dtype=np.uint8))
    words = member_sets(n, b, False)
    want = F.PoolIM(models).run(x, words, 0.5, ge, True, True)
    for m in models:
        m.debug(materialize=True)
    try:
        got = F.PoolIM(models).run(x, words, 0.5, ge, True, True)
        torch.cuda.synchronize()
    finally:
        for m in models:
            m.debug(materialize=False)
    for key in ("masks", "im", "im_size", "pred_size", "img_out"):
        eq(got[key], want[key], key)


def test_routes_run_their_kernels_and_each_model_only_its_images():
    """by kernel name (the library's per-kernel launch totals): the fused route is the head + IM kernel over members with one input
    gather per model that sees a part of the batch and no stack kernel; a model nobody uses does not run; an image with more than 8
    members sends the call to the stack kernel"""
    from inconsistencymasks_amd import functions as F
    from inconsistencymasks_amd.prof import Profiler
    cfg, n, b, ge = POOLS[1]                              # a pool of 10
    models = pool_models(cfg, n)
    x = dev(np.random.default_rng(9).integers(0, 256, (b, cfg[0], cfg[1], cfg[2]), dtype=np.uint8))
    pool = F.PoolIM(models)
    prof = Profiler()
    try:
        def kernels(words):
            pool.run(x, words, 0.5, ge, True, True)       # workspace and code objects
            torch.cuda.synchronize()
            prof.totals(True)
            pool.run(x, words, 0.5, ge, True, True)
            torch.cuda.synchronize()
            t = prof.totals_dump()
            prof.totals(False)
            return t

        def launches(t, part):
            return sum(v["launches"] for name, v in t.items() if part in name)
        one = kernels([0b1, 0b1, 0b1, 0b1, 0b1, 0b1])                        # model 0 on every image: no gather, one forward
        two = kernels([0b11, 0b10, 0b10, 0b10, 0b10, 0b10])                  # model 0 on one image, model 1 on all
        three = kernels([0b111, 0b10, 0b10, 0b10, 0b10, 0b10])               # a third model on one image
        over8 = kernels([0b1111111110] + [0b11] * 5)
    finally:
        prof.close()
    for t in (one, two, three):
        assert launches(t, "head_im_members_sigmoid_kernel") == 1 and launches(t, "im_binary_members") == 0, sorted(t)
        assert launches(t, "members_lists_kernel") == 1 and launches(t, "members_upload_kernel") == 1
    assert launches(one, "gather_rows_kernel") == 0 and launches(two, "gather_rows_kernel") == 1 and launches(three, "gather_rows_kernel") == 2
    total = lambda t: sum(v["launches"] for v in t.values())  # noqa: E731
    per_model = total(two) - total(one) - 1               # one more model's forward; the gather is the "- 1"
    assert per_model > 0 and total(three) - total(two) == per_model + 1, (total(one), total(two), total(three))
    assert launches(over8, "head_im_members") == 0 and launches(over8, "im_binary_members_vec") == 1 and launches(over8, "gather_rows_kernel") == 0


def test_pool_of_predict_style_models_goes_through_the_stack():
    from inconsistencymasks_amd import functions as F
    c = cases()["binary_n5"]
    n, b, h, w, _ = c["preds"].shape

    class Fixed:
        def __init__(self, table):
            self.table, self.i = table, 0

        def predict(self, x):                      # called once per image, in order
            self.i += 1
            return self.table[(self.i - 1) % b][None]

    got = F.PoolIM([Fixed(c["preds"][j]) for j in range(n)], binary=True).run(torch.zeros((b, h, w, 1), dtype=torch.uint8, device="cuda"),
                                                                                 c["words"], 0.5, False, False, False)
    eq(got["masks"], c["masks"], "masks")
    eq(got["im"], c["im"], "im")


# ---- 3. imk_morph_var ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(37, 70), (8, 200)])
def test_morph_var_equals_morph_image_by_image(h, w):
    from inconsistencymasks_amd import im as IM
    rng = np.random.default_rng(h * w)
    ks = [0, 3, 5, 7, 7, 0, 5, 3, 3]
    src = np.zeros((len(ks), h, w), np.uint8)
    for i in range(len(ks)):                       # blobs, some of them on the image's edges and corners
        src[i] = (rng.random((h, w)) > 0.93) * 255
        src[i, :3, :5] = 255
        src[i, h - 2:, w // 2:w // 2 + 9] = 255
        src[i, h // 3:h // 3 + 6, w - 4:] = 255
        src[i, h // 2:h // 2 + 7, 0] = 255
    sd = dev(src)
    for op in ("erode", "dilate"):
        got = IM.morph_var(sd, ks, op)
        for i, k in enumerate(ks):
            want = sd[i:i + 1] if k == 0 else IM.morph(sd[i:i + 1].contiguous(), k, op)
            eq(got[i:i + 1], want, f"{op}, image {i}, window {k}")
    for bad in ([4] + ks[1:], [33] + ks[1:], [-1] + ks[1:], ks[1:]):
        with pytest.raises(ValueError):
            IM.morph_var(sd, bad, "erode")
