"""Case table of tests/test_gpu_tile_walks.py: small images at batches large enough that every workgroup of a persistent kernel
walks several tiles, and the arithmetic that says so.  Plain data and helpers; imports without a GPU (tests/test_cpu_tile_walk_cases.py).

What makes a launch walk is the batch, never a switch: the launchers size their grids from the tile count and fixed caps
(CAPS below, each with the source text it restates), so a launch with at least twice its largest possible grid walks in every
workgroup, and one with at most 256 tiles runs one tile per workgroup whatever the occupancy query returns."""
import math

TILE = 16                      # csrc/imk_stage.h: `constexpr int TW = 16;`, tile rows of 16 in the persistent kernels
BWD1_PIXELS = 128              # csrc/imk_bwd1.hip, imk_bwd1x1_rows: `(n_pix + 127) / 128`

# name -> (value, file under inconsistencymasks_amd/csrc, the source text that sets it)
CAPS = {
    # launch_conv_pipe_k / launch_conv_wide_k: grid = min(256 * blocks_per_cu, n_tiles), blocks_per_cu <= 8
    "conv_grid_max": (2048, "imk_conv.hip", ["constexpr int PIPE_BLOCKS_PER_CU = 8;", "blocks_per_cu = nb > PIPE_BLOCKS_PER_CU ? PIPE_BLOCKS_PER_CU : nb;",
                                             "blocks_per_cu = nb > 8 ? 8 : nb;", "int grid = 256 * blocks_per_cu;", "if (grid > n_tiles) grid = n_tiles;"]),
    # ... and never fewer than min(256, n_tiles): the occupancy query returns at least 1
    "conv_grid_min": (256, "imk_conv.hip", ["int grid = 256 * blocks_per_cu;"]),
    # the dynamic walk (DYN): inference launches from 2048 tiles up
    "dyn_min_tiles": (2048, "imk_conv.hip", ["if (a.sched && !a.stats_partial && a.B * imk_cdiv(a.H, 16) * imk_cdiv(a.W, TW) >= 2048)"]),
    # imk_bwd1x1_rows: min(ceil(n_pix / 128), 768 or 512)
    "bwd1_small": (768, "imk_bwd1.hip", ["#define BWD1_SMALL_WGS 3", "const int cap = (cs_in <= 32 && cs_out <= 32) ? 256 * BWD1_SMALL_WGS : 512;"]),
    "bwd1_large": (512, "imk_bwd1.hip", ["const int cap = (cs_in <= 32 && cs_out <= 32) ? 256 * BWD1_SMALL_WGS : 512;"]),
    # imk_wgrad_splits: min(768 / n_pairs, n_tiles)
    "wgrad_target": (768, "imk_conv.hip", ["constexpr int target = 768;", "int s = target / n_pairs;", "if (s > n_tiles) s = n_tiles;"]),
}

# Every U-Net plan needs h and w to be multiples of 16 (cfg_ok, csrc/imk_unet.hip: four poolings), so level 0 of a U-Net has FULL tiles
# only; the partial edge tiles (not FULL) are those of level 1, 24 x 40 pixels = 2 x 3 tiles with a half last row and column, which
# walks at the inference batch in every case, and of the levels below.
CASES = {
    # pair layout, FULL tiles at level 0, LM_STEM, the decoder's PRE stage, the fused weight-gradient forms WG
    "pair": dict(h=48, w=80, c=3, k=1, act="sigmoid", loss="mse", alpha=0.5),
    # plain 16-channel layout, one input channel, 32 channels at level 1
    "plain16": dict(h=48, w=80, c=1, k=3, act="softmax", loss="cce", alpha=1.0),
    # conv_wide_kernel at level 0, CHAIN2, bwd1x1_kernel<SMALL> (channel stride 24)
    "wide20": dict(h=48, w=80, c=3, k=5, act="softmax", loss="cce", alpha=1.25),
    # 32 channels at level 0 (two channel tiles), the GEMM-class kernel from level 1 down
    "wide32": dict(h=48, w=80, c=3, k=1, act="sigmoid", loss="mse", alpha=2.0),
}
INFER_BATCH, SUB_BATCH = 768, 16
TRAIN_B0, TRAIN_REPLICAS = 4, 96
TRAIN_BATCH = TRAIN_B0 * TRAIN_REPLICAS

# one tile per image: n_tiles equals the batch -- the edges of the dynamic walk's threshold
ONE_TILE = dict(h=16, w=16, c=3, k=3, act="softmax", loss="cce")
ONE_TILE_ALPHAS = (0.5, 1.0)
ONE_TILE_BATCHES = (2040, 2047, 2048, 2049, 2080)      # below the threshold; at it; above; a multiple of 32 above
ONE_TILE_SUB = 256

EVALNET_CASE, EVALNET_BATCH, EVALNET_SUB = "isic", 320, 16      # tests/test_gpu_evalnet.py CFGS: 64 x 64, 16 tiles per image
EVALNET_HW = (64, 64)                                           # checked against CFGS where the GPU test builds the net


def pad8(c):
    return (c + 7) // 8 * 8


def widths(alpha):
    """channels per level, unet.py:49-56"""
    return [int(v * alpha) for v in (16, 32, 64, 128, 256)]


def level_hw(h, w, level):
    """MaxPooling2D halves, dropping an odd last row / column"""
    return h >> level, w >> level


def tiles_per_image(h, w, level=0):
    hh, ww = level_hw(h, w, level)
    return math.ceil(hh / TILE) * math.ceil(ww / TILE)


def conv_tiles(batch, h, w, level=0):
    """n_tiles of launch_conv_pipe_k / launch_conv_wide_k: B * ceil(h / 16) * ceil(w / 16)"""
    return batch * tiles_per_image(h, w, level)


def bwd1_tiles(batch, h, w, level=0):
    """imk_bwd1x1_rows: ceil(n_pix / 128)"""
    hh, ww = level_hw(h, w, level)
    return math.ceil(batch * hh * ww / BWD1_PIXELS)


def bwd1_applies(cs_in, cs_out):
    """imk_bwd1x1_ok: 24 ... 64 padded channels on both sides"""
    return 24 <= cs_in <= 64 and 24 <= cs_out <= 64


def bwd1_cap(cs_in, cs_out):
    return CAPS["bwd1_small"][0] if cs_in <= 32 and cs_out <= 32 else CAPS["bwd1_large"][0]


def wgrad_splits(batch, h, w, cin, cout, level=0):
    """imk_wgrad_splits: min(768 / n_pairs, n_tiles), at least 1"""
    n_tiles = conv_tiles(batch, h, w, level)
    n_pairs = ((pad8(cin) + 15) // 16) * ((pad8(cout) + 15) // 16)
    return min(max(CAPS["wgrad_target"][0] // n_pairs, 1), n_tiles)


def sub_ranges(batch, sub):
    """[lo, hi) of the reference sub-batches: full ones and the remainder"""
    return [(lo, min(lo + sub, batch)) for lo in range(0, batch, sub)]


def walk_class(n_tiles):
    """what the tile count of a persistent conv launch says about its walk, without knowing the occupancy"""
    if n_tiles >= 2 * CAPS["conv_grid_max"][0]:
        return "every workgroup walks"
    if n_tiles > CAPS["conv_grid_max"][0]:
        return "some workgroups walk; all of them below full occupancy"
    if n_tiles > CAPS["conv_grid_min"][0]:
        return "walks only below %d workgroups per compute unit" % math.ceil(n_tiles / 256)
    return "one tile per workgroup"


# ---- the comparison helper ---------------------------------------------------------------------------------------------------------
def first_mismatch(layer, got, ref, first_image=0):
    """got, ref: tensors [b, h, w, c] of one stored layer (any dtype compared bit for bit by value; fp16 NaNs do not occur in stored
    activations), `got` being images first_image ... first_image + b of a larger launch.  None if they are equal, else where the first
    difference lies: dict(layer, image, tile_row, tile_col, launch_tile, y, x, channel, n_diff) with image counted in the launch,
    tile_row / tile_col the 16 x 16 tile inside the image and launch_tile = image * tiles per image + tile_row * tiles_x + tile_col --
    the index the persistent kernels walk."""
    import torch
    if got.shape != ref.shape or got.dtype != ref.dtype:
        raise ValueError(f"{layer}: comparing {tuple(got.shape)} {got.dtype} with {tuple(ref.shape)} {ref.dtype}")
    if got.data_ptr() == ref.data_ptr() and got.numel():
        raise ValueError(f"{layer}: a tensor compared with itself")
    if got.dim() == 3:
        got, ref = got[..., None], ref[..., None]
    elif got.dim() < 3:            # per-image scalars (sizes, scores): only the image is meaningful
        got, ref = got.reshape(got.shape[0], 1, 1, -1), ref.reshape(ref.shape[0], 1, 1, -1)
    ne = got != ref
    n_diff = int(ne.sum())
    if n_diff == 0:
        return None
    _, h, w, c = got.shape
    flat = int(torch.nonzero(ne.reshape(-1))[0])
    i, rest = divmod(flat, h * w * c)
    y, rest = divmod(rest, w * c)
    x, ch = divmod(rest, c)
    tiles_x, tiles_y = math.ceil(w / TILE), math.ceil(h / TILE)
    image, tr, tc = first_image + i, y // TILE, x // TILE
    return dict(layer=layer, image=image, tile_row=tr, tile_col=tc, launch_tile=image * tiles_x * tiles_y + tr * tiles_x + tc,
                y=y, x=x, channel=ch, n_diff=n_diff)


def assert_equals_sub_batches(whole, run_sub, batch, sub, what):
    """whole: name -> tensor [batch, ...] of the whole-batch run; run_sub(lo, hi) -> the same dict for images lo ... hi run on their own.
    Every tensor of every sub-batch equals the whole run's slice bit for bit.  The flags stay on the device until the end (one
    synchronisation); a sub-batch that differs is run again and the first difference located."""
    import numpy as np
    import pytest
    import torch
    ranges = sub_ranges(batch, sub)
    names = list(whole)
    flags = []
    for lo, hi in ranges:
        got = run_sub(lo, hi)
        assert list(got) == names
        flags.append(torch.stack([(whole[n][lo:hi] != got[n]).any() for n in names]))
    bad = torch.stack(flags).cpu().numpy()
    if bad.any():
        r = int(np.argwhere(bad.any(1))[0, 0])
        lo, hi = ranges[r]
        got = run_sub(lo, hi)
        where = [first_mismatch(n, whole[n][lo:hi], got[n], lo) for n in names if bad[r, names.index(n)]]
        pytest.fail(f"{what}: the batch-{batch} run differs from its sub-batches of {sub} in {int(bad.any(1).sum())} of {len(ranges)} sub-batches, "
                    f"tensors {[n for i, n in enumerate(names) if bad[:, i].any()]}; first: {where}")
