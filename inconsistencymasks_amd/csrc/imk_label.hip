// Label counts of the scalar-IoU multiclass EvalNet family (functions.py:3496-3567, 3673-3769): every training-data writer of that
// family labels a sample with get_IoU_multi_unique (functions.py:1791-1816) of two class-id maps, the prediction with its IM pixels
// set to class 0.  One streaming pass over the maps applies the blocking (prediction, optionally the image) and leaves, per image,
// the INTEGER pixel counts every such label is a ratio of; the host forms the ratios with the reference's own float expressions
// (evaluate.iou_multi_unique_from_counts), so the labels are bit-identical to the numpy loop and do not depend on the grid.
// HBM-bound: each map read once in 16-byte pieces, the blocked prediction written once, counts via one LDS histogram per workgroup
// (integer LDS atomics, one per run of equal pixels) and one 64-bit global atomic per non-zero bin per workgroup.
#include "imk_common.h"

namespace {

struct LabelRun {      // a run of pixels with the same (gt, blocked prediction, blocked) along a thread's walk
    int key = -1, n = 0;
};

__device__ __forceinline__ void label_flush(unsigned int *hist, const LabelRun &r, bool has_im) {
    if (!r.n) return;
    const int g = r.key & 255, p = (r.key >> 8) & 255;
    atomicAdd(&hist[g], (unsigned)r.n);
    atomicAdd(&hist[256 + p], (unsigned)r.n);
    if (g == p) atomicAdd(&hist[512 + g], (unsigned)r.n);
    if (has_im && !(r.key >> 16)) atomicAdd(&hist[768 + g], (unsigned)r.n);
}

// one pixel: -> the blocked prediction; zeroes the image's pixel where blocked (the bytes imk_block_apply writes, and no others)
__device__ __forceinline__ int label_pixel(unsigned int *hist, LabelRun &run, bool has_im, int g, int p, int m,
                                           uint8_t *image, int c, size_t px) {
    const bool blocked = m != 0;
    if (blocked) {
        p = 0;
        if (image)
            for (int ch = 0; ch < c; ++ch) image[px * c + ch] = 0;
    }
    const int key = g | (p << 8) | ((int)blocked << 16);
    if (key != run.key) { label_flush(hist, run, has_im); run.key = key; run.n = 0; }
    ++run.n;
    return p;
}

// grid (workgroups per image, B): workgroup x of an image owns a contiguous range of the image's 16-byte pieces, and a share of the
// pixels in front of / behind them (unaligned image base, ragged end; all pixels where the maps' addresses differ modulo 16).
// pred_blocked may alias pred: a thread reads a piece completely before it writes it, and no other thread touches that piece.
__global__ __launch_bounds__(256) void label_counts_kernel(const uint8_t *pred, const uint8_t *__restrict__ gt,
                                                           const uint8_t *__restrict__ im, uint8_t *__restrict__ image, int c, int hw,
                                                           uint8_t *pred_blocked, unsigned long long *__restrict__ counts) {
    __shared__ unsigned int hist[4 * 256];
    for (int i = threadIdx.x; i < 4 * 256; i += 256) hist[i] = 0;
    __syncthreads();
    const int b = blockIdx.y;
    const size_t base = (size_t)b * hw;
    const bool has_im = im != nullptr;
    const uint8_t *pp = pred + base, *gp = gt + base, *mp = has_im ? im + base : nullptr;
    uint8_t *op = pred_blocked ? pred_blocked + base : nullptr;

    // the image's split into head bytes, 16-byte pieces and tail bytes (uniform over the workgroup)
    const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(pp) & 15);
    bool same = (reinterpret_cast<uintptr_t>(gp) & 15) == a;
    if (has_im) same = same && (reinterpret_cast<uintptr_t>(mp) & 15) == a;
    if (op) same = same && (reinterpret_cast<uintptr_t>(op) & 15) == a;
    int n_head = same ? min((int)((16 - a) & 15), hw) : 0;
    const int n_vec = same ? (hw - n_head) / 16 : 0;
    const int tail0 = n_head + 16 * n_vec, n_bytes = n_head + (hw - tail0);

    LabelRun run;
    const int per = (n_vec + gridDim.x - 1) / gridDim.x;
    const int v_end = min(n_vec, (int)(blockIdx.x + 1) * per);
    for (int v = blockIdx.x * per + threadIdx.x; v < v_end; v += 256) {
        const int p0 = n_head + 16 * v;
        const uint4 pv = *reinterpret_cast<const uint4 *>(pp + p0), gv = *reinterpret_cast<const uint4 *>(gp + p0);
        const uint4 mv = has_im ? *reinterpret_cast<const uint4 *>(mp + p0) : uint4{0, 0, 0, 0};
        const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w}, gw[4] = {gv.x, gv.y, gv.z, gv.w}, mw[4] = {mv.x, mv.y, mv.z, mv.w};
        uint32_t ow[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t o = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = label_pixel(hist, run, has_im, (gw[q] >> (8 * j)) & 255, (pw[q] >> (8 * j)) & 255, (mw[q] >> (8 * j)) & 255,
                                          image, c, base + p0 + 4 * q + j);
                o |= (uint32_t)r << (8 * j);
            }
            ow[q] = o;
        }
        if (op) *reinterpret_cast<uint4 *>(op + p0) = uint4{ow[0], ow[1], ow[2], ow[3]};
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_bytes; i += gridDim.x * 256) {
        const int p = i < n_head ? i : tail0 + (i - n_head);
        const int r = label_pixel(hist, run, has_im, gp[p], pp[p], has_im ? mp[p] : 0, image, c, base + p);
        if (op) op[p] = (uint8_t)r;
    }
    label_flush(hist, run, has_im);
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * 256; i += 256) {
        const unsigned int n = (i >= 768 && !has_im) ? hist[i - 768] : hist[i];      // no IM: nothing is blocked, row 3 is row 0
        if (n) atomicAdd(counts + (size_t)b * 1024 + i, (unsigned long long)n);
    }
}

}  // namespace

extern "C" int imk_label_counts(const uint8_t *pred, const uint8_t *gt, const uint8_t *im, uint8_t *image, int c, int batch, int h,
                                int w, uint8_t *pred_blocked, int64_t *counts, void *stream_) {
    IMK_CHECK_ARG(pred && gt && counts && batch > 0 && h > 0 && w > 0);
    IMK_CHECK_ARG(!image || c == 1 || c == 3);
    if ((int64_t)h * w >= ((int64_t)1 << 31) || batch > 65535) return IMK_EUNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    IMK_HIP(hipMemsetAsync(counts, 0, (size_t)batch * 1024 * sizeof(int64_t), stream));
    const int hw = h * w;
    // two 16-byte pieces per thread and workgroup; an image of 64 pieces or more is spread over at least two workgroups
    const int n_vec = hw / 16;
    int bx = imk_cdiv(n_vec, 512);
    if (bx < 2 && n_vec >= 64) bx = 2;
    if (bx < 1) bx = 1;
    if (bx > 64) bx = 64;
    imk_klaunch(label_counts_kernel, dim3(bx, batch), dim3(256), 0, stream, pred, gt, im, image, c, hw, pred_blocked,
                (unsigned long long *)counts);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
