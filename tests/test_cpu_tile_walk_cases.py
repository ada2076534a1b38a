"""The conditions under which tests/test_gpu_tile_walks.py means what it says, checked without a GPU: the tile counts of every case as
the launchers compute them against the launchers' own grid caps (conditions, not measurements), and the comparison helper's self-test."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import tile_walk_cases as T  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "inconsistencymasks_amd", "csrc")
GRID_MAX, GRID_MIN = T.CAPS["conv_grid_max"][0], T.CAPS["conv_grid_min"][0]


def test_the_caps_are_the_launchers_own():
    """every cap the table compares with is restated from a line of the launcher that sets it; the line must still be there"""
    for name, (value, fname, lines) in T.CAPS.items():
        text = open(os.path.join(CSRC, fname)).read()
        for line in lines:
            assert line in text, f"{name} = {value}: csrc/{fname} no longer has `{line}`"
    assert GRID_MAX == 256 * 8 and GRID_MIN == 256 * 1
    assert T.CAPS["bwd1_small"][0] == 256 * 3 and T.CAPS["bwd1_large"][0] == 512


@pytest.mark.parametrize("name", list(T.CASES))
def test_tile_counts_per_image(name):
    cfg = T.CASES[name]
    assert T.tiles_per_image(cfg["h"], cfg["w"], 0) == 15 and T.tiles_per_image(cfg["h"], cfg["w"], 1) == 6
    assert T.tiles_per_image(cfg["h"], cfg["w"], 2) == 2
    # cfg_ok (csrc/imk_unet.hip) admits multiples of 16 only: FULL tiles at level 0, partial last row and column at level 1
    assert "if (c->h <= 0 || c->w <= 0 || (c->h % 16) || (c->w % 16)) return false;" in open(os.path.join(CSRC, "imk_unet.hip")).read()
    assert cfg["h"] % 16 == 0 and cfg["w"] % 16 == 0
    h1, w1 = T.level_hw(cfg["h"], cfg["w"], 1)
    assert h1 % 16 and w1 % 16
    assert T.widths(cfg["alpha"])[0] == {"pair": 8, "plain16": 16, "wide20": 20, "wide32": 32}[name]


@pytest.mark.parametrize("name", list(T.CASES))
def test_inference_batch_walks_and_its_reference_does_not(name):
    """B = 768: levels 0 and 1 of every case have at least twice the largest possible grid of launch_conv_pipe_k / launch_conv_wide_k
    (2048 workgroups), and at least the 2048 tiles from which conv_pipe_kernel takes the dynamic walk; a 16-image sub-batch has at most
    256 tiles at every level, which is at most the SMALLEST possible grid, so there grid == n_tiles."""
    cfg = T.CASES[name]
    h, w = cfg["h"], cfg["w"]
    assert (T.conv_tiles(T.INFER_BATCH, h, w, 0), T.conv_tiles(T.INFER_BATCH, h, w, 1)) == (11520, 4608)
    for level in (0, 1):
        n = T.conv_tiles(T.INFER_BATCH, h, w, level)
        assert n >= 2 * GRID_MAX and n >= T.CAPS["dyn_min_tiles"][0], (level, n)
        assert T.walk_class(n) == "every workgroup walks"
    # level 2 (12 x 20 pixels: 2 tiles per image) has 1536 tiles: it walks only if the instantiation's occupancy is below 6
    # workgroups per compute unit, which nobody has measured.  Stated, not relied upon.
    assert T.conv_tiles(T.INFER_BATCH, h, w, 2) == 1536 and GRID_MIN < 1536 <= GRID_MAX
    assert T.walk_class(1536) == "walks only below 6 workgroups per compute unit"
    for level in range(5):
        assert T.conv_tiles(T.SUB_BATCH, h, w, level) <= GRID_MIN, level
    assert T.conv_tiles(T.SUB_BATCH, h, w, 0) == 240
    assert T.INFER_BATCH % T.SUB_BATCH == 0 and len(T.sub_ranges(T.INFER_BATCH, T.SUB_BATCH)) == 48


@pytest.mark.parametrize("name", list(T.CASES))
def test_training_batch_walks(name):
    """B = 384 = 96 replicas of 4 images: 5760 tiles at level 0 (>= 2 x 2048), 11520 bwd1x1 tiles of 128 pixels (>= 2 x 768), and 768 /
    n_pairs weight-gradient splits of at least 2 tiles each at levels 0 and 1.  The level-1 conv launches have 2304 tiles against a
    grid of at most 2048: some workgroups walk at any occupancy, every one only below full occupancy -- stated, not relied upon."""
    cfg = T.CASES[name]
    h, w, ch = cfg["h"], cfg["w"], T.widths(cfg["alpha"])
    assert T.TRAIN_BATCH == 384
    n0, n1 = T.conv_tiles(T.TRAIN_BATCH, h, w, 0), T.conv_tiles(T.TRAIN_BATCH, h, w, 1)
    assert (n0, n1) == (5760, 2304)
    assert n0 >= 2 * GRID_MAX
    assert GRID_MAX < n1 < 2 * GRID_MAX and T.walk_class(n1).startswith("some workgroups walk")
    for level in (0, 1):
        cs = T.pad8(ch[level])
        n_tiles = T.conv_tiles(T.TRAIN_BATCH, h, w, level)
        # the block's Conv1x1 (cs -> cs) through bwd1x1_kernel where imk_bwd1x1_ok admits it
        if T.bwd1_applies(cs, cs):
            rows = T.bwd1_tiles(T.TRAIN_BATCH, h, w, level)
            assert rows >= 2 * T.bwd1_cap(cs, cs), (level, rows)
            if (name, level) == ("wide20", 0):
                assert (cs, rows, T.bwd1_cap(cs, cs)) == (24, 11520, 768)            # bwd1x1_kernel<SMALL>
        # the split weight-gradient kernels: every same-width conv of the level, 3x3 and 1x1
        splits = T.wgrad_splits(T.TRAIN_BATCH, h, w, ch[level], ch[level], level)
        assert n_tiles >= 2 * splits, (level, n_tiles, splits)
    if name == "pair":      # one channel-tile pair: 768 splits of 7.5 tiles
        assert T.wgrad_splits(T.TRAIN_BATCH, h, w, 8, 8, 0) == 768 and n0 / 768 == 7.5
    # every in-image tile position occurs as a first and as a later iteration: a group's range (1 / 8 of the launch, 720 tiles = 48
    # images) starts on an image boundary, its first `step` <= 256 tiles cover at most 17 images, the rest the other 31
    assert n0 % 8 == 0 and (n0 // 8) % T.tiles_per_image(h, w) == 0 and (n0 // 8) - GRID_MAX // 8 >= 2 * T.tiles_per_image(h, w)


def test_one_tile_batches_straddle_the_dynamic_threshold():
    c = T.ONE_TILE
    assert T.tiles_per_image(c["h"], c["w"], 0) == 1 and T.tiles_per_image(c["h"], c["w"], 1) == 1
    thr = T.CAPS["dyn_min_tiles"][0]
    n = [T.conv_tiles(b, c["h"], c["w"]) for b in T.ONE_TILE_BATCHES]
    assert n == list(T.ONE_TILE_BATCHES)
    assert [b for b in n if b < thr] == [2040, 2047] and thr in n and thr + 1 in n
    assert 2080 % 32 == 0 and 2080 > thr and 2049 % 32 == 1           # the 32-group walk rounds the grid down to a multiple of 32
    assert T.conv_tiles(T.ONE_TILE_SUB, c["h"], c["w"]) <= GRID_MIN
    assert T.sub_ranges(2049, 256) == [(i * 256, (i + 1) * 256) for i in range(8)] + [(2048, 2049)]
    assert T.sub_ranges(2040, 256)[-1] == (1792, 2040)


def test_evalnet_batch_walks():
    assert T.EVALNET_HW == (64, 64) and T.tiles_per_image(64, 64) == 16
    assert T.conv_tiles(T.EVALNET_BATCH, 64, 64) == 5120 >= 2 * GRID_MAX
    assert T.conv_tiles(T.EVALNET_SUB, 64, 64) == 256 <= GRID_MIN
    assert T.EVALNET_BATCH % T.EVALNET_SUB == 0


# ---- the comparison helper has teeth -------------------------------------------------------------------------------------------------
def test_first_mismatch_names_the_element():
    torch = pytest.importorskip("torch")
    g = torch.Generator().manual_seed(0)
    b, h, w, c = 5, 40, 72, 3                                  # 3 x 5 tiles per image, partial last row and column
    ref = torch.rand((b, h, w, c), generator=g).to(torch.float16)
    assert T.first_mismatch("e1.c3", ref.clone(), ref) is None
    got = ref.clone()
    # one fp16 element, by one ulp: image 3 of this slice, pixel (37, 50) -> tile row 2, tile column 3
    v = got[3, 37, 50, 1].view(torch.int16)
    got[3, 37, 50, 1] = (v + 1).view(torch.float16)
    assert int((got != ref).sum()) == 1
    m = T.first_mismatch("e1.c3", got, ref, first_image=32)      # the slice is images 32 ... 36 of the launch
    assert m == dict(layer="e1.c3", image=35, tile_row=2, tile_col=3, launch_tile=35 * 15 + 2 * 5 + 3, y=37, x=50, channel=1, n_diff=1)
    # two differing elements: the first in launch order is named, both are counted
    got[1, 0, 71, 0] = got[1, 0, 71, 0] + 1
    m = T.first_mismatch("e1.c3", got, ref)
    assert (m["image"], m["tile_row"], m["tile_col"], m["launch_tile"], m["n_diff"]) == (1, 0, 4, 15 + 4, 2)
    # label maps [b, h, w] go through the same helper
    lab = torch.zeros((2, 16, 32), dtype=torch.uint8)
    other = lab.clone()
    other[1, 5, 20] = 1
    assert T.first_mismatch("labels", other, lab)["launch_tile"] == 2 + 1
    # a loop that compares a tensor with itself is an error, not a pass; so are two shapes
    with pytest.raises(ValueError):
        T.first_mismatch("e1.c3", ref, ref)
    with pytest.raises(ValueError):
        T.first_mismatch("e1.c3", ref[:2], ref)


def test_sub_batch_comparison_fails_on_one_element():
    """assert_equals_sub_batches on CPU tensors: equal runs pass; one fp16 element of one sub-batch's layer fails it, the message naming
    the layer, the image in the launch and the tile"""
    torch = pytest.importorskip("torch")
    g = torch.Generator().manual_seed(1)
    whole = {"probs": torch.rand((40, 48, 80, 2), generator=g), "e1.c1": torch.rand((40, 48, 80, 8), generator=g).to(torch.float16)}
    calls = []

    def run_sub(lo, hi, tamper=None):
        calls.append((lo, hi))
        out = {n: v[lo:hi].clone() for n, v in whole.items()}
        if tamper is not None and lo <= tamper < hi:
            out["e1.c1"][tamper - lo, 20, 70, 5] += 1
        return out
    T.assert_equals_sub_batches(whole, run_sub, 40, 16, "self-test")
    assert calls == [(0, 16), (16, 32), (32, 40)]
    with pytest.raises(pytest.fail.Exception) as e:
        T.assert_equals_sub_batches(whole, lambda lo, hi: run_sub(lo, hi, tamper=35), 40, 16, "self-test")
    msg = str(e.value)
    assert "1 of 3 sub-batches" in msg and "['e1.c1']" in msg
    assert "'image': 35" in msg and "'tile_row': 1" in msg and "'tile_col': 4" in msg and f"'launch_tile': {35 * 15 + 5 + 4}" in msg
