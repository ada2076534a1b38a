"""Data preparation: the host side of csrc/imk_prep.hip and the counterparts of the functions the reference's 00_* / 01_* /
SUIM 02_* scripts define (same names, positional arguments and defaults; file:line cited per function).

The reference goes through cv2.imread / cv2.resize / cv2.cvtColor / cv2.imwrite one file at a time.  Here a directory stage reads
the files' headers, gives every source of a batch its slice of one pinned staging buffer, and the reader pool's threads decode straight
into those slices (a grey file as one plane); the batch is uploaded once, ONE imk_prep_resize runs per rule (or one imk_prep_crops per
source), the results come back in one download and the PNG encodes are queued on the writer pool.  There is no CPU path for the pixel rules: without libimk.so
the import fails.  Arrays are held in RGB order where the reference holds BGR; files come out the same, because both write back
the order they read.

What differs from the reference, by design:
  * create_random_crops seeds its draws per file from (SEED, output directory, file name), like the other writers of this package, so
    the files do not depend on the rank count.  The reference's crops are unseeded.  random_crop itself uses the global generators in
    the reference's order.
  * SUIM's split copies the JPEG bytes; the reference re-encodes them with cv2.imwrite (lossy, quality 95).
  * With several ranks the 00 / 02 stages shard their file list (functions.shard_list) and end in a barrier.
"""
import collections
import ctypes
import math
import os
import random
import shutil
import time
import zlib

import numpy as np
import torch
from PIL import Image, ImageOps

from . import _lib
from . import functions as F
from ._lib import check, lib

IMK_PREP_LINEAR, IMK_PREP_NEAREST = 0, 1
IMK_PREP_LABEL_PLUS1 = 1
IMK_PREP_GRAY, IMK_PREP_GRAY_THRESH, IMK_PREP_CLASS8 = 0, 1, 2

SEED = F.SEED
STAGE_BYTES = int(os.environ.get("IMK_PREP_STAGE_MB", 256)) << 20      # decoded sources per batch


# ---------------------------------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def make_item(src_off, src_h, src_w, dh, dw, rect=None):
    """one imk_prep_item; rect = (x0, y0, cw, ch), default the whole source.  The scales are 1 / inv_scale as cv::resize forms them."""
    x0, y0, cw, ch = rect if rect is not None else (0, 0, src_w, src_h)
    if not (0 <= x0 and 0 <= y0 and cw > 0 and ch > 0 and x0 + cw <= src_w and y0 + ch <= src_h):
        raise ValueError(f"rectangle {(x0, y0, cw, ch)} leaves its {src_h} x {src_w} source")
    return _lib.PrepItem(int(src_off), int(src_h), int(src_w), int(x0), int(y0), int(cw), int(ch),
                         1.0 / (float(dw) / float(cw)), 1.0 / (float(dh) / float(ch)))


def items_to_device(items, device="cuda"):
    arr = (_lib.PrepItem * len(items))(*items)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def prep_resize(src, items, c, dh, dw, interp=IMK_PREP_LINEAR, post=0, out=None):
    """src: uint8 cuda tensor holding the decoded sources back to back; items: list of imk_prep_item (make_item) or their device
    bytes (items_to_device) -> uint8 cuda [n, dh, dw, c]"""
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous()
    n = len(items) if not torch.is_tensor(items) else items.numel() // ctypes.sizeof(_lib.PrepItem)
    dev = items if torch.is_tensor(items) else items_to_device(items, src.device)
    if out is None:
        out = torch.empty((n, dh, dw, c), dtype=torch.uint8, device=src.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n * dh * dw * c
    check(lib.imk_prep_resize(src.data_ptr(), src.numel(), dev.data_ptr(), n, c, dh, dw, int(interp), int(post), out.data_ptr(),
                              _stream()), "imk_prep_resize")
    return out


def prep_crops(src, positions, ch, cw, rule, class_table=None, b_first=False, out=None):
    """src: uint8 cuda [h, w, c]; positions: [(x, y)] or an int32 cuda tensor [P, 2] -> uint8 cuda [P, ch, cw]"""
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 3
    h, w, c = src.shape
    pos = positions if torch.is_tensor(positions) else torch.tensor(list(positions), dtype=torch.int32).reshape(-1, 2).to(src.device)
    assert pos.is_cuda and pos.dtype == torch.int32 and pos.is_contiguous()
    n = pos.shape[0]
    if out is None:
        out = torch.empty((n, ch, cw), dtype=torch.uint8, device=src.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == n * ch * cw
    table = None
    if class_table is not None:
        table = np.ascontiguousarray(class_table, dtype=np.uint8)
        assert table.shape == (8,)
    check(lib.imk_prep_crops(src.data_ptr(), h, w, c, pos.data_ptr(), n, ch, cw, int(rule),
                             table.ctypes.data if table is not None else None, int(bool(b_first)), out.data_ptr(), _stream()),
          "imk_prep_crops")
    return out


# ---------------------------------------------------------------------------------------------------
# readers
# ---------------------------------------------------------------------------------------------------
# what a file that is no (whole) image raises: Pillow's UnidentifiedImageError and truncated-file errors are OSErrors, a broken
# stream inside a decoder is a ValueError / SyntaxError / EOFError there
_DECODE_ERRORS = (OSError, ValueError, SyntaxError, EOFError, Image.DecompressionBombError)


def read_image(path, channels=3):
    """uint8 [h, w, channels] (RGB or grey) or None where the file does not decode -- cv2.imread's `None`.  PNG goes through the
    native codec (functions.read_png; Pillow for what it declines); JPEG, BMP and the rest through Pillow with the EXIF orientation
    applied, as cv2.imread does by default."""
    try:
        if path.lower().endswith(".png"):
            return F.read_png(path, channels)
        with Image.open(path) as im:
            im = ImageOps.exif_transpose(im).convert("RGB" if channels == 3 else "L")
            a = np.array(im, dtype=np.uint8)      # a copy of its own: Pillow's buffer is read-only
        return a if a.ndim == 3 else a[..., None]
    except _DECODE_ERRORS:      # text files, truncated downloads: reported by the caller and skipped; anything else is a bug and raises
        return None


# ---------------------------------------------------------------------------------------------------
# the ragged resize stage
# ---------------------------------------------------------------------------------------------------
class _Staging:
    """one pinned host buffer, grown on demand and reused by every batch of the process"""

    def __init__(self):
        self.buf = None

    def view(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return self.buf


_STAGING = _Staging()

# one output file of a resize stage: the file at `path`, wanted with `channels` (1 or 3), its rectangle rect(h, w) (None: the whole
# image) resized to dsize(h, w) and written to out_path with `channels` channels
ResizeJob = collections.namedtuple("ResizeJob", "path channels dsize interp post out_path rect", defaults=(None,))


def probe_image(path, channels=3):
    """(h, w, c) as the file will be decoded, from its header alone, or None where it is no image.  c is 1 where one channel is wanted
    or the file is 8-bit grey: a grey source is staged, uploaded and resized as one plane and replicated behind the kernel, which
    gives what the three equal channels would have given."""
    try:
        if path.lower().endswith(".png") and F._NATIVE_PNG:
            h, w, ct, bd = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            if lib.imk_png_info(os.fsencode(path), ctypes.byref(h), ctypes.byref(w), ctypes.byref(ct), ctypes.byref(bd)) == 0:
                return h.value, w.value, 1 if channels == 1 or (ct.value == 0 and bd.value == 8) else 3
        with Image.open(path) as im:
            w, h = im.size
            if im.getexif().get(0x0112, 1) in (5, 6, 7, 8):      # the orientations that swap the axes (read_image applies them)
                w, h = h, w
            return h, w, 1 if channels == 1 or im.mode == "L" else 3
    except _DECODE_ERRORS:
        return None


def decode_into(path, row):
    """decode `path` straight into `row`, a uint8 [h, w, c] view (of the pinned staging buffer) shaped as probe_image said; False where
    the file does not decode after all (a truncated download)"""
    c = row.shape[2]
    try:
        if path.lower().endswith(".png"):
            F._read_png_into(path, c, row)
        else:
            with Image.open(path) as im:
                im = ImageOps.exif_transpose(im).convert("RGB" if c == 3 else "L")
                row[...] = np.asarray(im, dtype=np.uint8).reshape(row.shape)
        return True
    except _DECODE_ERRORS as e:
        print(f"Failed to decode {path}: {type(e).__name__}: {e}")
        return False


def _launch_staged(stage, total, entries, timing=None):
    """entries: (offset, h, w, c, rect, (dh, dw), interp, post) over the first `total` bytes of the pinned tensor `stage` -> one output
    array per entry.  One upload, one imk_prep_resize per (c, dh, dw, interp, post), one download per launch."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timing is not None else None
    if ev:
        ev[0].record()
    dev = stage[:total].cuda(non_blocking=True)
    if ev:
        ev[1].record()
    groups = {}
    for i, (off, h, w, c, rect, (dh, dw), interp, post) in enumerate(entries):
        groups.setdefault((c, int(dh), int(dw), interp, post), []).append(i)
    outs_dev = []
    for (c, dh, dw, interp, post), idx in groups.items():
        items = [make_item(entries[i][0], entries[i][1], entries[i][2], dh, dw, entries[i][4]) for i in idx]
        outs_dev.append(prep_resize(dev, items, c, dh, dw, interp, post))
    if ev:
        ev[2].record()
    outs = [None] * len(entries)
    for idx, o in zip(groups.values(), outs_dev):
        o = o.cpu().numpy()
        for row, i in enumerate(idx):
            outs[i] = o[row]
    if ev:
        ev[3].record()
        ev[3].synchronize()
        for k, name in enumerate(("upload_ms", "kernel_ms", "download_ms")):
            timing[name] = timing.get(name, 0.0) + ev[k].elapsed_time(ev[k + 1])
    return outs


def resize_arrays(arrays, dsizes, interp, post=0, rects=None):
    """[h_i, w_i, c_i] uint8 arrays already in memory -> list of [dh_i, dw_i, c_i] arrays (the single-image functions' route; the
    directory stages decode straight into the staging buffer instead: stage_batches / resize_batch)"""
    if not arrays:
        return []
    entries, total = [], 0
    for i, a in enumerate(arrays):
        assert a.dtype == np.uint8 and a.ndim == 3
        entries.append((total, a.shape[0], a.shape[1], a.shape[2], rects[i] if rects else None, dsizes[i], interp, post))
        total += a.size
    stage = _STAGING.view(total)
    host = stage.numpy()
    for a, e in zip(arrays, entries):
        host[e[0]:e[0] + a.size] = a.reshape(-1)
    return _launch_staged(stage, total, entries)


def stage_batches(pool, jobs, what="image", timing=None):
    """Read the headers of the jobs' files on the pool and cut the jobs into batches: a batch closes at INFER_BATCH files or at
    STAGE_BYTES of decoded sources, whichever comes first (a source larger than that is a batch of its own).  Jobs on one file share
    one decode.  -> list of batches, a batch = (total bytes, [(path, offset, (h, w, c))], [(job, source index, rect)])"""
    t0 = time.perf_counter()
    jobs = list(jobs)
    keys = list(dict.fromkeys((j.path, j.channels) for j in jobs))
    shapes = dict(zip(keys, pool.map(lambda k: probe_image(*k), keys)))
    batches, sources, index, entries, total, reported = [], [], {}, [], 0, set()
    for job in jobs:
        key = (job.path, job.channels)
        shape = shapes[key]
        if shape is None:
            if key not in reported:
                reported.add(key)
                print(f"Failed to load {what}: {job.path}")
            continue
        nbytes = shape[0] * shape[1] * shape[2]
        if key not in index and sources and (len(sources) >= F.INFER_BATCH or total + nbytes > STAGE_BYTES):
            batches.append((total, sources, entries))
            sources, index, entries, total = [], {}, [], 0
        if key not in index:
            index[key] = len(sources)
            sources.append((job.path, total, shape))
            total += nbytes
        entries.append((job, index[key], job.rect(shape[0], shape[1]) if job.rect else None))
    if sources:
        batches.append((total, sources, entries))
    if timing is not None:
        timing["decode_ms"] = timing.get("decode_ms", 0.0) + (time.perf_counter() - t0) * 1e3
    return batches


def resize_batch(pool, batch, timing=None):
    """One batch: the pool threads decode every source straight into its slice of the pinned staging buffer, then one upload, one
    imk_prep_resize per rule, one download -> [(out_path, array)] with the channels each job asked for"""
    total, sources, entries = batch
    stage = _STAGING.view(total)
    host = stage.numpy()
    t0 = time.perf_counter()
    ok = pool.map(lambda s: decode_into(s[0], host[s[1]:s[1] + s[2][0] * s[2][1] * s[2][2]].reshape(s[2])), sources)
    if timing is not None:
        timing["decode_ms"] = timing.get("decode_ms", 0.0) + (time.perf_counter() - t0) * 1e3
    live = [(job, si, rect) for job, si, rect in entries if ok[si]]
    outs = _launch_staged(stage, total, [(sources[si][1],) + sources[si][2] + (rect, job.dsize(*sources[si][2][:2]), job.interp, job.post)
                                         for job, si, rect in live], timing)
    return [(job.out_path, np.repeat(o, 3, 2) if job.channels == 3 and o.shape[2] == 1 else o) for (job, _, _), o in zip(live, outs)]


def _run_resize_stage(jobs, what="image"):
    """a directory stage: per batch the decode into the staging buffer, one upload, one launch per rule, one download and one
    write-pool submit"""
    with F._pool() as pool:
        for batch in stage_batches(pool, jobs, what):
            F.write_pngs_async(resize_batch(pool, batch))
    F.flush_writes()


def _barrier():
    d = F._dist()
    if d:
        d.barrier()


# ---------------------------------------------------------------------------------------------------
# ISIC_2018/00_ISIC_2018_preprocess_images.py
# ---------------------------------------------------------------------------------------------------
def isic_out_name(filename, is_mask=False):
    """:50-52: the mask name drops its 17-character `_segmentation.png` tail, the image name its extension"""
    return f"{filename[:-17]}.png" if is_mask else f"{filename[:-4]}.png"


def preprocess_data(dir_pairs, is_mask=False):
    """ISIC_2018/00_ISIC_2018_preprocess_images.py:33-56: every file of in_dir resized to IMAGE_WIDTH x IMAGE_HEIGHT with cv2.resize's
    default (linear, masks included: the reference passes no flag) and written as a 3-channel PNG.  Files that do not decode (the
    download folders hold text files) are reported and skipped."""
    S = F.config["ISIC_2018"]
    dw, dh = int(S["IMAGE_WIDTH"]), int(S["IMAGE_HEIGHT"])
    for in_dir, out_dir in dir_pairs:
        if not os.path.exists(in_dir):
            continue
        os.makedirs(out_dir, exist_ok=True)
        jobs = [ResizeJob(os.path.join(in_dir, n), 3, lambda h, w: (dh, dw), IMK_PREP_LINEAR, 0,
                          os.path.join(out_dir, isic_out_name(n, is_mask)))
                for n in F.shard_list(os.listdir(in_dir))]
        _run_resize_stage(jobs, "mask" if is_mask else "image")
        _barrier()


# ---------------------------------------------------------------------------------------------------
# Cityscapes/00_Cityscapes_resize_images_and_masks.py
# ---------------------------------------------------------------------------------------------------
def cityscapes_size(h, w, factor, base=16):
    """:25-29 -> (dh, dw): int(dim * factor), then up to the next multiple of `base` (1024 x 2048 at 0.2: 208 x 416)"""
    return base * int(np.ceil(int(h * factor) / base)), base * int(np.ceil(int(w * factor) / base))


def cityscapes_pairs(img_dir, mask_dir):
    """:43-53: (image path, mask path, common name) of every `.png` below img_dir whose `{city}/{common}_gtFine_labelIds.png` exists;
    the city is the directory's own name"""
    pairs = []
    for root, _, files in os.walk(img_dir):
        _, city = os.path.split(root)
        for file in files:
            if file.endswith(".png"):
                common_name = "_".join(file.split("_")[:-1])
                mask_path = os.path.join(mask_dir, city, common_name + "_gtFine_labelIds.png")
                if os.path.exists(mask_path):
                    pairs.append((os.path.join(root, file), mask_path, common_name))
    return pairs


def resize_image(image_path, factor, base=16, is_mask=False):
    """:21-36 for one file -> [dh, dw, 3] (RGB where the reference returns BGR).  Masks: INTER_NEAREST; the +1 is process_images'."""
    image = read_image(image_path, 3)
    dh, dw = cityscapes_size(image.shape[0], image.shape[1], factor, base)
    return resize_arrays([image], [(dh, dw)], IMK_PREP_NEAREST if is_mask else IMK_PREP_LINEAR)[0]


def process_images(img_dir, mask_dir, save_img_dir, save_mask_dir, factor, base=16):
    """:38-66: images linear, masks nearest then np.where(m > 0, m + 1, m), both as `{common}.png` with 3 channels"""
    os.makedirs(save_img_dir, exist_ok=True)
    os.makedirs(save_mask_dir, exist_ok=True)
    size = lambda h, w: cityscapes_size(h, w, factor, base)
    jobs = []
    for img_path, mask_path, common in F.shard_list(cityscapes_pairs(img_dir, mask_dir)):
        jobs.append(ResizeJob(img_path, 3, size, IMK_PREP_LINEAR, 0, os.path.join(save_img_dir, common + ".png")))
        jobs.append(ResizeJob(mask_path, 3, size, IMK_PREP_NEAREST, IMK_PREP_LABEL_PLUS1, os.path.join(save_mask_dir, common + ".png")))
    _run_resize_stage(jobs)
    _barrier()


# ---------------------------------------------------------------------------------------------------
# HeLa/00_HeLa_create_crops.py
# ---------------------------------------------------------------------------------------------------
def hela_crop_name(img_name, count):
    """:123, :145: crop `count` of every channel of `img_name`"""
    return f"{img_name[:-4]}_{count}.png"


class ImagePreprocessor:
    """HeLa/00_HeLa_create_crops.py:20-194.  process_image reads every channel image once, uploads it once and cuts all its crops
    with one imk_prep_crops (the reference reads and converts every channel image again for every crop)."""

    def __init__(self, img_path, crop_path, crop_size, overlap, use_mod_pos_size=True):
        self.img_path = img_path
        self.crop_path = crop_path
        self.crop_size = crop_size
        self.overlap = overlap
        self.use_mod_pos_size = use_mod_pos_size
        self.channels = ["brightfield", "alive", "dead"]
        self.channels.append("mod_position" if use_mod_pos_size else "position")

    def get_positions(self, img_height, img_width):
        """:33-80, with Python's round / int / min exactly"""
        assert img_height > 0 and img_width > 0, "Image dimensions should be positive."
        assert 0 <= self.overlap < 1, "Overlap should be between 0 and 1."
        x_count = round(img_width / (self.crop_size * (1 - self.overlap)))
        y_count = round(img_height / (self.crop_size * (1 - self.overlap)))
        x_move = img_width / x_count
        y_move = img_height / y_count
        positions = []
        for i in range(x_count):
            for j in range(y_count):
                x = min(int(i * x_move), img_width - self.crop_size)
                y = min(int(j * y_move), img_height - self.crop_size)
                positions.append((x, y))
        return positions

    def _channel_file(self, channel, img_name):
        return os.path.join(self.img_path, channel, f"{img_name[:-4]}.png" if channel != "brightfield" else img_name)

    def _cut(self, positions, img_name, counts):
        for channel in self.channels:
            path = self._channel_file(channel, img_name)
            if not os.path.exists(path):
                continue
            shape = probe_image(path, 3)      # a grey file is read, uploaded and cut as one plane (BGR2GRAY of R = G = B is the identity)
            img = read_image(path, shape[2]) if shape else None
            if img is None:
                raise FileNotFoundError(f"Image file {os.path.basename(path)} not found in {path}.")
            rule = IMK_PREP_GRAY if channel == "brightfield" else IMK_PREP_GRAY_THRESH
            planes = prep_crops(torch.from_numpy(np.ascontiguousarray(img)).cuda(), positions, self.crop_size, self.crop_size,
                                rule).cpu().numpy()
            out_dir = os.path.join(self.crop_path, channel)
            os.makedirs(out_dir, exist_ok=True)
            F.write_pngs_async([(os.path.join(out_dir, hela_crop_name(img_name, count)), planes[k])
                                for k, count in enumerate(counts)])

    def process_image(self, img_name):
        """:84-98"""
        bf = os.path.join(self.img_path, "brightfield", img_name)
        size = None
        try:
            with Image.open(bf) as im:
                size = ImageOps.exif_transpose(im).size
        except Exception:      # noqa: BLE001
            pass
        if size is None:
            raise FileNotFoundError(f"Image file {img_name} not found in {self.img_path}/brightfield.")
        positions = self.get_positions(size[1], size[0])
        if positions:
            self._cut(positions, img_name, range(len(positions)))

    def process_crops(self, position, img_name, count):
        """:102-145 for one position"""
        self._cut([tuple(position)], img_name, [count])
        F.flush_writes()

    def mod_pos_size(self, in_path, out_path, max_pos_circle_size=8, min_pos_circle_size=3):
        """:149-194: every position image of in_path redrawn by functions.mod_pos_size (imk_mod_pos_size), 3 channels as the
        reference writes them"""
        if not os.path.exists(in_path):
            raise FileNotFoundError(f"Input directory {in_path} does not exist.")
        os.makedirs(out_path, exist_ok=True)
        for posimg in os.listdir(in_path):
            shape = probe_image(os.path.join(in_path, posimg), 3)
            img = read_image(os.path.join(in_path, posimg), shape[2]) if shape else None
            if img is None:
                raise FileNotFoundError(f"Image file {posimg} not found in {in_path}.")
            out = F.mod_pos_size(img[..., ::-1] if img.shape[2] == 3 else img[..., 0], max_pos_circle_size, min_pos_circle_size)
            F.write_png(os.path.join(out_path, posimg), np.repeat(out[..., None], 3, 2))


def hela_create_crops(base_img_path, base_crop_path, use_mod_pos_size, crop_size=256, overlap=0.6,
                      data_sets=("train_full", "val", "test")):
    """:198-218 main()"""
    for data_set in data_sets:
        img_path = os.path.join(base_img_path, data_set)
        pre = ImagePreprocessor(img_path, os.path.join(base_crop_path, data_set), crop_size=crop_size, overlap=overlap,
                                use_mod_pos_size=use_mod_pos_size)
        bf_path = os.path.join(img_path, "brightfield")
        if os.path.exists(bf_path):
            for img_name in F.shard_list(os.listdir(bf_path)):
                try:
                    pre.process_image(img_name)
                except Exception as e:      # noqa: BLE001 -- the reference prints and goes on
                    print(e)
        F.flush_writes()
        _barrier()


def hela_split(root_dir, labeled_dir, unlabeled_dir, use_mod_pos_size, seed=SEED):
    """HeLa/01_HeLa_split_train_in_labeled_and_unlabeled.py:28-59: random.seed(SEED); random.shuffle of the brightfield listing, the
    first int(0.10 n) names labelled; shutil.copy of every channel's file"""
    folders = ["brightfield", "alive", "dead", "mod_position" if use_mod_pos_size else "position"]
    bf_img_names = os.listdir(os.path.join(root_dir, "brightfield"))
    rng = random.Random(seed)      # random.seed(SEED); random.shuffle: the same generator, without touching the global one
    rng.shuffle(bf_img_names)
    split_idx = int(len(bf_img_names) * 0.10)
    parts = ((labeled_dir, bf_img_names[:split_idx]), (unlabeled_dir, bf_img_names[split_idx:]))
    for folder in folders:
        for d, _ in parts:
            os.makedirs(os.path.join(d, folder), exist_ok=True)
    for folder in folders:
        for d, names in parts:
            for imagename in names:
                src = os.path.join(root_dir, folder, imagename)
                if os.path.exists(src):
                    shutil.copy(src, os.path.join(d, folder, imagename))
                else:
                    print(f"Source file {src} does not exist.")
    return parts[0][1], parts[1][1]


# ---------------------------------------------------------------------------------------------------
# SUIM/00_SUIM_convert_bmp_to_png_masks.py
# ---------------------------------------------------------------------------------------------------
def class_table(color_to_class_mapping):
    """the 8 entries of IMK_PREP_CLASS8: after np.where(image < 128, 0, 255) (:21) a pixel can only equal a mapping colour whose
    components are all 0 or 255; colours the mapping lacks stay 0 (:24)"""
    t = np.zeros(8, np.uint8)
    for rgb, class_id in color_to_class_mapping.items():
        if all(v in (0, 255) for v in rgb):
            t[((rgb[0] == 255) << 2) | ((rgb[1] == 255) << 1) | (rgb[2] == 255)] = class_id
    return t


def suim_mask_png_name(bmp_file):
    """:47"""
    return f"{os.path.splitext(bmp_file)[0]}.png"


def convert_color_bmp_to_class_mask_png(bmp_file_path, output_path, color_to_class_mapping):
    """:15-32"""
    image = read_image(bmp_file_path, 3)
    h, w = image.shape[:2]
    plane = prep_crops(torch.from_numpy(np.ascontiguousarray(image)).cuda(), [(0, 0)], h, w, IMK_PREP_CLASS8,
                       class_table(color_to_class_mapping))[0].cpu().numpy()
    F.write_png(output_path, plane)


def convert_all_masks_in_folder(input_folder, output_folder, color_to_class_mapping):
    """:36-50"""
    os.makedirs(output_folder, exist_ok=True)
    bmp_files = [f for f in os.listdir(input_folder) if f.endswith(".bmp")]
    table = class_table(color_to_class_mapping)
    with F._pool() as pool:
        mine = F.shard_list(bmp_files)
        for i in range(0, len(mine), F.INFER_BATCH):
            chunk = mine[i:i + F.INFER_BATCH]
            for name, image in zip(chunk, pool.map(lambda n: read_image(os.path.join(input_folder, n), 3), chunk)):
                if image is None:
                    print(f"Failed to load mask: {os.path.join(input_folder, name)}")
                    continue
                h, w = image.shape[:2]
                plane = prep_crops(torch.from_numpy(np.ascontiguousarray(image)).cuda(), [(0, 0)], h, w, IMK_PREP_CLASS8, table)
                F.write_png_async(os.path.join(output_folder, suim_mask_png_name(name)), plane[0].cpu().numpy())
    F.flush_writes()
    _barrier()


# ---------------------------------------------------------------------------------------------------
# SUIM/02_SUIM_create_crops.py
# ---------------------------------------------------------------------------------------------------
def _draw_crop(height, width, min_crop_size, max_crop_size, rng, np_rng):
    """:17-21: the reference's draws in its order -> (x, y, size, size) or None (the whole image is resized)"""
    crop_size = int(np_rng.randint(min_crop_size, min(max_crop_size, max(height, width))))
    if height >= crop_size and width >= crop_size:
        x = rng.randint(0, width - crop_size)
        y = rng.randint(0, height - crop_size)
        return (x, y, crop_size, crop_size)
    return None


def random_crop(img, mask, target_crop_size=256, min_crop_size=256, max_crop_size=512):
    """:13-37 with the global generators (np.random.randint, then random.randint for x, then y).  img linear, mask nearest."""
    img, mask = np.asarray(img, np.uint8), np.asarray(mask, np.uint8)
    rect = _draw_crop(img.shape[0], img.shape[1], min_crop_size, max_crop_size, random, np.random)
    i3, m3 = (img if img.ndim == 3 else img[..., None]), (mask if mask.ndim == 3 else mask[..., None])
    t = (target_crop_size, target_crop_size)
    o = resize_arrays([np.ascontiguousarray(i3)], [t], IMK_PREP_LINEAR, 0, [rect])[0]
    m = resize_arrays([np.ascontiguousarray(m3)], [t], IMK_PREP_NEAREST, 0, [rect])[0]
    return (o if img.ndim == 3 else o[..., 0]), (m if mask.ndim == 3 else m[..., 0])


def crop_rngs(main_output_path, image_file):
    """the generators of one file's crops: seeded by (SEED, output directory, file name) like functions._view_rngs"""
    key = f"{SEED}|{os.path.basename(os.path.normpath(main_output_path))}|{image_file}"
    return random.Random(key), np.random.RandomState(zlib.crc32(key.encode()))


def create_random_crops(image_folder, mask_folder, main_output_path, num_crops_per_image):
    """:40-61: `{stem}_{i}_{j}.png` with i the index in the `.jpg` listing; random_crop's default sizes, as the reference calls it"""
    _create_random_crops(image_folder, mask_folder, main_output_path, num_crops_per_image, 256, 256, 512)


def _create_random_crops(image_folder, mask_folder, main_output_path, num_crops_per_image, target_crop_size, min_crop_size,
                         max_crop_size):
    image_files = [f for f in os.listdir(image_folder) if f.endswith(".jpg")]
    images_path_out = os.path.join(main_output_path, "images")
    masks_path_out = os.path.join(main_output_path, "masks")
    os.makedirs(images_path_out, exist_ok=True)
    os.makedirs(masks_path_out, exist_ok=True)
    t = lambda h, w: (target_crop_size, target_crop_size)
    jobs = []
    for image_file, i in F.shard_list([(f, i) for i, f in enumerate(image_files)]):
        ipath, mpath = os.path.join(image_folder, image_file), os.path.join(mask_folder, f"{image_file[:-4]}.png")
        rng, np_rng = crop_rngs(main_output_path, image_file)
        drawn = {}

        def rect(h, w, j, drawn=drawn, rng=rng, np_rng=np_rng):      # image and mask of crop j share one draw, made in order of j
            for k in range(len(drawn), j + 1):
                drawn[k] = _draw_crop(h, w, min_crop_size, max_crop_size, rng, np_rng)
            return drawn[j]

        for j in range(num_crops_per_image):
            name = f"{image_file[:-4]}_{i}_{j}.png"
            jobs.append(ResizeJob(ipath, 3, t, IMK_PREP_LINEAR, 0, os.path.join(images_path_out, name),
                                  lambda h, w, j=j, r=rect: r(h, w, j)))
            jobs.append(ResizeJob(mpath, 1, t, IMK_PREP_NEAREST, 0, os.path.join(masks_path_out, name),
                                  lambda h, w, j=j, r=rect: r(h, w, j)))
    _run_resize_stage(jobs)
    _barrier()


# ---------------------------------------------------------------------------------------------------
# the 01_* splits
# ---------------------------------------------------------------------------------------------------
def train_test_split(items, test_size, random_state):
    """scikit-learn's train_test_split(list, test_size=float, random_state=int) restated: n_test = ceil(test_size n), the test part
    is the head of RandomState(seed).permutation(n), the train part its tail; an empty part is a ValueError"""
    items = list(items)
    n = len(items)
    n_test = int(math.ceil(test_size * n))
    if n_test <= 0 or n - n_test <= 0:
        raise ValueError(f"With n_samples={n} and test_size={test_size}, one of the two parts would be empty.")
    perm = np.random.RandomState(random_state).permutation(n)
    return [items[i] for i in perm[n_test:]], [items[i] for i in perm[:n_test]]


def _rewrite_png(src, dst):
    """cv2.imread + cv2.imwrite of a PNG: the same pixels with 3 channels"""
    a = read_image(src, 3)
    if a is None:
        raise FileNotFoundError(src)
    F.write_png(dst, a)


def _write_subsets(subsets, output_dir, copy_pair):
    with F._pool() as pool:
        for subset, files in subsets.items():
            print(f"Processing {subset} data...")
            img_subset_dir = os.path.join(output_dir, subset, "images")
            mask_subset_dir = os.path.join(output_dir, subset, "masks")
            os.makedirs(img_subset_dir, exist_ok=True)
            os.makedirs(mask_subset_dir, exist_ok=True)
            pool.map(lambda f: copy_pair(f, img_subset_dir, mask_subset_dir), files)


def split_and_resize_dataset(images_dir, masks_dir, output_dir, subset_names, split_ratio, seed=SEED):
    """ISIC_2018/01_ISIC_2018_split_original_train.py:20-44 and Cityscapes/01_Cityscapes_split_original_train_val.py:20-44: the
    os.listdir order (unsorted, as the reference feeds it) split by train_test_split; every PNG rewritten with 3 channels"""
    image_files = os.listdir(images_dir)
    mask_files = os.listdir(masks_dir)
    assert set(image_files) == set(mask_files), "Images and masks don't match"
    part_a, part_b = train_test_split(image_files, test_size=split_ratio, random_state=seed)

    def copy_pair(f, img_dir, mask_dir):
        _rewrite_png(os.path.join(images_dir, f), os.path.join(img_dir, f))
        _rewrite_png(os.path.join(masks_dir, f), os.path.join(mask_dir, f))

    _write_subsets({subset_names[0]: part_a, subset_names[1]: part_b}, output_dir, copy_pair)
    return part_a, part_b


def split_and_resize_dataset_suim(images_dir, masks_dir, output_dir, subset_names, test_size=0.1):
    """SUIM/01_SUIM_split_original_train_val.py:13-47 (its split_and_resize_dataset; random_state is 42 there, not SEED).  The JPEG
    is copied byte for byte where the reference re-encodes it; the mask PNG is rewritten with 3 channels."""
    assert isinstance(subset_names, list), "subset_names must be a list"
    assert len(subset_names) == 2, "subset_names must have exactly two elements"
    assert all(isinstance(item, str) for item in subset_names), "all elements in subset_names must be strings"
    image_files_no_ext = [os.path.splitext(f)[0] for f in os.listdir(images_dir)]
    mask_files_no_ext = [os.path.splitext(f)[0] for f in os.listdir(masks_dir)]
    assert set(image_files_no_ext) == set(mask_files_no_ext), "Images and masks don't match"
    train_files, val_files = train_test_split(image_files_no_ext, test_size=test_size, random_state=42)

    def copy_pair(f, img_dir, mask_dir):
        shutil.copy(os.path.join(images_dir, f + ".jpg"), os.path.join(img_dir, f + ".jpg"))
        _rewrite_png(os.path.join(masks_dir, f + ".png"), os.path.join(mask_dir, f + ".png"))

    _write_subsets({subset_names[0]: train_files, subset_names[1]: val_files}, output_dir, copy_pair)
    return train_files, val_files
