// Input-ensemble baseline for gfx950 (MI355X): one model voting with itself over augmented views of each image -- the pseudo-label
// rules of the reference's get_input_ensemble_prediction_* (functions.py:1409-1459, 1570-1764, 2127-2407).
//
// D4 ops: 0 = identity, 1..12 = the reference's enumeration (generate_random_transformations, functions.py:1675-1726):
//   op = 1 + 6 * flip_horizontal + 3 * flip_vertical + (rotation - 1), where flip_horizontal is cv2.flip(., 0) (the rows
//   reversed), flip_vertical cv2.flip(., 1) (the columns), rotation 1 = 90 CW, 2 = 180, 3 = 90 CCW, applied in that order.
//   Several of the 12 repeat another D4 element; they stay distinct ops because random.choice indexes into the list of 12.
//   The restore (restore_random_transformations, :1729-1764) is the exact inverse, so a view's prediction at view pixel v is
//   the vote of source pixel src_of(op, v).
//
// views_kernel:        B uint8 NHWC images -> M views per image [M,B,H,W,C] with data_augmentation_image's chain (:1570-1594):
//                      geometry -> GaussianBlur 3/5/7 -> uniform integer noise, clipped -> convertScaleAbs.  The pixel
//                      arithmetic is imk_aug.hip's (the same blur weights, BORDER_REFLECT_101, rounding, noise hash and
//                      saturate(rint|a x + b|)); only the order differs.  16 output bytes per thread, stored as one uint4.
// views_vote_sigmoid:  the ISIC hard vote fused with the sigmoid head: the last decoder activations of the M views of ONE model,
//                      head weights staged once, head_sigmoid(head_logit) exactly as imk_unet_forward's head; each member is
//                      read in its own row order over a 16x16 view tile and its votes land in LDS at output coordinates.
// vote_views_binary:   the same rule on an fp32 prediction stack [M,B,H,W,K] (duck-typed models, the unfused route).
// vote_views_majority: the most common per-view arg-max (np.argmax(np.bincount(.)): ties go to the smallest label).
#include "imk_common.h"
#include "imk_head.h"

namespace {

__device__ __forceinline__ uint32_t hash32(uint32_t x) {   // lowbias32 (imk_aug.hip)
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// saturate(rint(|x * alpha + beta|)) with the product rounded on its own: aug_oracle.convert_scale_abs's float32 arithmetic.  With
// contraction on (the HIP default) the expression may become one FMA, which moves values that land on a half (beta = -7.5) by one.
__device__ __forceinline__ int scale_abs(int x, float alpha, float beta) {
#pragma clang fp contract(off)
    const int o = __float2int_rn(fabsf((float)x * alpha + beta));
    return o > 255 ? 255 : o;
}

// view pixel (yo, xo) of op -> source pixel (quarter turns only with H == W: the host refuses the others)
__device__ __forceinline__ void view_src(int op, int H, int W, int yo, int xo, int &ys, int &xs) {
    if (op <= 0) { ys = yo; xs = xo; return; }
    const int o = op - 1, fr = o / 6, fc = (o / 3) & 1, rot = o % 3 + 1;
    switch (rot) {                     // undo the rotation (imk_aug.hip's src_index)
        case 1: ys = H - 1 - xo; xs = yo; break;
        case 2: ys = H - 1 - yo; xs = W - 1 - xo; break;
        default: ys = xo; xs = W - 1 - yo; break;
    }
    if (fc) xs = W - 1 - xs;
    if (fr) ys = H - 1 - ys;
}

// source pixel (y, x) -> the view pixel that holds it (the inverse of view_src)
__device__ __forceinline__ void view_dst(int op, int H, int W, int y, int x, int &yo, int &xo) {
    if (op <= 0) { yo = y; xo = x; return; }
    const int o = op - 1, fr = o / 6, fc = (o / 3) & 1, rot = o % 3 + 1;
    const int y2 = fr ? H - 1 - y : y, x2 = fc ? W - 1 - x : x;
    switch (rot) {
        case 1: yo = x2; xo = H - 1 - y2; break;
        case 2: yo = H - 1 - y2; xo = W - 1 - x2; break;
        default: yo = W - 1 - x2; xo = y2; break;
    }
}

// OpenCV's small Gaussian kernels for sigma = 0 (x/64), by radius: imk_aug.hip's weights
__constant__ int c_gauss[4][7] = {{64, 0, 0, 0, 0, 0, 0}, {16, 32, 16, 0, 0, 0, 0}, {4, 16, 24, 16, 4, 0, 0}, {2, 7, 14, 18, 14, 7, 2}};

// grid (ceil(H*W*C / 4096), B, M): view m0 + z of image b from src + b * HWC (chain: one launch per view, src = the view before)
__global__ __launch_bounds__(256) void views_kernel(const uint8_t *__restrict__ src, int H, int W, int C,
                                                    const imk_view_params *__restrict__ prm, int batch, int m0,
                                                    uint8_t *__restrict__ out) {
    const int b = blockIdx.y, m = m0 + blockIdx.z;
    const int64_t hwc = (int64_t)H * W * C;
    const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (e0 >= hwc) return;
    const imk_view_params q = prm[(size_t)m * batch + b];
    const uint8_t *img = src + (size_t)b * hwc;
    uint8_t *dst = out + ((size_t)m * batch + b) * hwc;
    const int k = q.blur_k, r = k > 1 ? k / 2 : 0;           // 0/1 = none, 3, 5, 7
    const uint32_t nkey = hash32(q.seed ^ 0x9e3779b9u);
    uint8_t v16[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t e = e0 + i;
        if (e >= hwc) { v16[i] = 0; continue; }
        const int p = (int)(e / C), c = (int)(e - (int64_t)p * C);
        const int yo = p / W, xo = p - yo * W;
        int ys, xs;
        view_src(q.op, H, W, yo, xo, ys, xs);
        int val;
        if (r == 0) {
            val = img[((size_t)ys * W + xs) * C + c];
        } else {
            // The blur acts on the view, but a symmetric kernel with BORDER_REFLECT_101 commutes with every flip and quarter turn,
            // and the sum is exact integer arithmetic: the taps are taken around the source pixel in source space.
            const int *wg = c_gauss[r];
            int acc = 0;
            for (int dy = -r; dy <= r; ++dy) {
                const uint8_t *row_p = img + (size_t)reflect101(ys + dy, H) * W * C + c;
                int row = 0;
                for (int dx = -r; dx <= r; ++dx) row += wg[dx + r] * row_p[(size_t)reflect101(xs + dx, W) * C];
                acc += wg[dy + r] * row;
            }
            val = (acc + 2048) >> 12;                         // weights sum to 64 per axis
        }
        if (q.noise_max > 0) {
            const uint32_t h = hash32(nkey + (uint32_t)e);
            const int noise = (int)(((uint64_t)h * (uint32_t)(2 * q.noise_max)) >> 32) - q.noise_max;
            val = min(255, max(0, val + noise));
        }
        if (q.bright_on) val = scale_abs(val, q.alpha, q.beta);
        v16[i] = (uint8_t)val;
    }
    if (e0 + 16 <= hwc && (reinterpret_cast<uintptr_t>(dst + e0) & 15) == 0) {
        uint4 w;
        uint32_t *w32 = reinterpret_cast<uint32_t *>(&w);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            w32[j] = v16[4 * j] | (v16[4 * j + 1] << 8) | (v16[4 * j + 2] << 16) | ((uint32_t)v16[4 * j + 3] << 24);
        *reinterpret_cast<uint4 *>(dst + e0) = w;
    } else {
        for (int i = 0; i < 16 && e0 + i < hwc; ++i) dst[e0 + i] = v16[i];
    }
}

template <bool GE>
__device__ __forceinline__ bool vote_cmp(float p, float thr) { return GE ? p >= thr : p > thr; }     // NaN votes 0 under both

// grid (W/16, H/16, B), 256 threads = one 16x16 tile.  The M members' last decoder activations z + m * B*H*W*CS; masks [B,K,H,W].
template <int CS, int KB, bool GE>
__global__ __launch_bounds__(256) void views_vote_sigmoid_kernel(ImkViewVoteArgs a) {
    __shared__ float s_w[KB * CS + KB + 2 * CS];
    __shared__ uint8_t s_cnt[KB][256];
    const int t = threadIdx.x, b = blockIdx.z, H = a.h, W = a.w, M = a.n_views;
    const int ty0 = blockIdx.y * 16, tx0 = blockIdx.x * 16;
    head_stage<CS>(a.wt, a.bias, a.sc, a.sh, a.cin, KB, s_w);
#pragma unroll
    for (int k = 0; k < KB; ++k) s_cnt[k][t] = 0;
    __syncthreads();
    const float thr = (float)a.thr;
    for (int m = 0; m < M; ++m) {
        const int op = a.ops[(size_t)m * a.ops_ld + b];
        // the view tile that holds this output tile: the image of its corners, an aligned 16x16 square (H, W multiples of 16)
        int vy0, vx0, vy1, vx1;
        view_dst(op, H, W, ty0, tx0, vy0, vx0);
        view_dst(op, H, W, ty0 + 15, tx0 + 15, vy1, vx1);
        const int vy = min(vy0, vy1) + (t >> 4), vx = min(vx0, vx1) + (t & 15);     // this thread's view pixel, row order
        int y, x;
        view_src(op, H, W, vy, vx, y, x);
        const long long p = ((long long)m * a.batch + b) * H * W + (long long)vy * W + vx;
        float xin[CS];
        head_input<CS>(a.z, p, s_w, KB, xin);
        const int slot = (y - ty0) * 16 + (x - tx0);
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (vote_cmp<GE>(head_sigmoid(head_logit<CS>(xin, s_w, KB, k)), thr)) s_cnt[k][slot] += 1;
        __syncthreads();                                      // the next member writes other threads' slots
    }
    const int y = ty0 + (t >> 4), x = tx0 + (t & 15);
#pragma unroll
    for (int k = 0; k < KB; ++k) a.out[(((size_t)b * KB + k) * H + y) * W + x] = s_cnt[k][t] == M ? 255 : 0;
}

// one thread per output pixel: preds [M,B,H,W,K] fp32 (member m of image b at row m * ld + b), masks [B,K,H,W]
template <bool GE>
__global__ __launch_bounds__(256) void vote_views_binary_kernel(const float *__restrict__ preds, int M, int batch, int H, int W, int K,
                                                                const int *__restrict__ ops, int ops_ld, float thr,
                                                                uint8_t *__restrict__ out) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= H * W) return;
    const int y = q / W, x = q - y * W;
    for (int k = 0; k < K; ++k) {
        int votes = 0;
        for (int m = 0; m < M; ++m) {
            int vy = y, vx = x;
            if (ops) view_dst(ops[(size_t)m * ops_ld + b], H, W, y, x, vy, vx);
            votes += vote_cmp<GE>(preds[((((size_t)m * batch + b) * H + vy) * W + vx) * K + k], thr) ? 1 : 0;
        }
        out[((size_t)b * K + k) * H * W + q] = votes == M ? 255 : 0;
    }
}

// np.argmax per view (first maximum; the first NaN wins), then np.argmax(np.bincount(labels)): the most common label, ties to
// the smallest.  probs [M,B,H,W,K] fp32, M <= IMK_VIEWS_MAX -> labels [B,H,W]
__global__ __launch_bounds__(256) void vote_views_majority_kernel(const float *__restrict__ probs, int M, long long n_pix, int K,
                                                                  uint8_t *__restrict__ out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pix) return;
    int lab[IMK_VIEWS_MAX];
#pragma unroll
    for (int m = 0; m < IMK_VIEWS_MAX; ++m) {
        lab[m] = 0x7fff;
        if (m < M) {
            const float *row = probs + ((size_t)m * n_pix + p) * K;
            float bv = row[0];
            int bk = 0;
            for (int k = 1; k < K && !__builtin_isnan(bv); ++k) {
                const float v = row[k];
                if (__builtin_isnan(v) || v > bv) { bv = v; bk = k; }
            }
            lab[m] = bk;
        }
    }
    int best = 0, best_n = 0;
#pragma unroll
    for (int i = 0; i < IMK_VIEWS_MAX; ++i) {
        int n = 0;
#pragma unroll
        for (int j = 0; j < IMK_VIEWS_MAX; ++j) n += (j < M && lab[j] == lab[i]) ? 1 : 0;
        if (i < M && (n > best_n || (n == best_n && lab[i] < best))) { best = lab[i]; best_n = n; }
    }
    out[p] = (uint8_t)best;
}

}  // namespace

extern "C" int imk_views(const uint8_t *img, int batch, int h, int w, int c, int n_views, const imk_view_params *params,
                         int chain, int any_quarter_turn, uint8_t *views_out, void *stream_) {
    IMK_CHECK_ARG(img && params && views_out && batch > 0 && h > 0 && w > 0 && c > 0 && n_views > 0);
    IMK_CHECK_ARG(batch <= 65535 && n_views <= 65535);
    if (any_quarter_turn && h != w) return IMK_EUNSUPPORTED;   // the view would change shape
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t hwc = (int64_t)h * w * c;
    IMK_CHECK_ARG(hwc < (1ll << 31));
    const unsigned gx = (unsigned)imk_cdiv(hwc, 16 * 256);
    // algorithmic bytes: every view read once from its source and written once
    ImkProfScope prof(PF_IM, 2.0 * (double)hwc * batch * n_views, stream, 0.0);
    if (!chain) {
        imk_klaunch(views_kernel, dim3(gx, batch, n_views), dim3(256), 0, stream, img, h, w, c, params, batch, 0, views_out);
        IMK_LAUNCH_CHECK();
        return IMK_OK;
    }
    for (int m = 0; m < n_views; ++m) {     // view m = aug(view m - 1): dependent launches on one stream
        const uint8_t *src = m == 0 ? img : views_out + (size_t)(m - 1) * batch * hwc;
        imk_klaunch(views_kernel, dim3(gx, batch, 1), dim3(256), 0, stream, src, h, w, c, params, batch, m, views_out);
        IMK_LAUNCH_CHECK();
    }
    return IMK_OK;
}

bool imk_views_vote_head_supported(const ImkViewVoteArgs &a) {
    if (a.n_views < 1 || a.n_views > IMK_VIEWS_MAX || a.K < 1 || a.K > 4) return false;
    if (a.cs != 8 && a.cs != 16 && a.cs != 24 && a.cs != 32) return false;
    return a.h % 16 == 0 && a.w % 16 == 0 && a.batch <= 65535;
}

int imk_launch_views_vote_head(const ImkViewVoteArgs &a, hipStream_t stream) {
    IMK_CHECK_ARG(a.z && a.ops && a.out && a.batch > 0);
    if (!imk_views_vote_head_supported(a)) return IMK_EUNSUPPORTED;
    const long long n_pix = (long long)a.batch * a.h * a.w;
    ImkProfScope prof(PF_IM, (double)n_pix * ((double)a.n_views * a.cs * 2 + a.K), stream,
                      (double)n_pix * a.n_views * a.K * (2.0 * a.cin + 1.0));
    const dim3 grid(a.w / 16, a.h / 16, a.batch);
#define IMK_VV(CSV, KBV)                                                                                                     \
    do {                                                                                                                     \
        if (a.cmp_ge) imk_klaunch(views_vote_sigmoid_kernel<CSV, KBV, true>, grid, dim3(256), 0, stream, a);                 \
        else imk_klaunch(views_vote_sigmoid_kernel<CSV, KBV, false>, grid, dim3(256), 0, stream, a);                         \
    } while (0)
#define IMK_VV_KB(CSV)                                                                                                       \
    switch (a.K) {                                                                                                           \
        case 1: IMK_VV(CSV, 1); break;                                                                                       \
        case 2: IMK_VV(CSV, 2); break;                                                                                       \
        case 3: IMK_VV(CSV, 3); break;                                                                                       \
        default: IMK_VV(CSV, 4); break;                                                                                      \
    }
    switch (a.cs) {
        case 8: IMK_VV_KB(8); break;
        case 16: IMK_VV_KB(16); break;
        case 24: IMK_VV_KB(24); break;
        default: IMK_VV_KB(32); break;
    }
#undef IMK_VV_KB
#undef IMK_VV
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

int imk_vote_views_binary_ld(const float *preds, int n_views, int batch, int h, int w, int k, const int *ops, int ops_ld,
                             double thr, int cmp_ge, uint8_t *masks_out, hipStream_t stream) {
    const int64_t hw = (int64_t)h * w;
    const long long n_pix = (long long)batch * hw;
    ImkProfScope prof(PF_IM, (double)n_pix * ((double)n_views * k * 4 + k), stream, (double)n_pix * n_views * k);
    const dim3 grid(imk_cdiv(hw, 256), batch);
    if (cmp_ge)
        imk_klaunch(vote_views_binary_kernel<true>, grid, dim3(256), 0, stream, preds, n_views, batch, h, w, k, ops, ops_ld,
                    (float)thr, masks_out);
    else
        imk_klaunch(vote_views_binary_kernel<false>, grid, dim3(256), 0, stream, preds, n_views, batch, h, w, k, ops, ops_ld,
                    (float)thr, masks_out);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_vote_views_binary(const float *preds, int n_views, int batch, int h, int w, int k, const int *ops,
                                     int any_quarter_turn, double thr, int cmp_ge, uint8_t *masks_out, void *stream_) {
    IMK_CHECK_ARG(preds && masks_out && n_views > 0 && batch > 0 && h > 0 && w > 0 && k > 0);
    IMK_CHECK_ARG(batch <= 65535 && (int64_t)h * w < (1ll << 30));
    if (ops && any_quarter_turn && h != w) return IMK_EUNSUPPORTED;
    return imk_vote_views_binary_ld(preds, n_views, batch, h, w, k, ops, batch, thr, cmp_ge, masks_out, (hipStream_t)stream_);
}

extern "C" int imk_vote_views_majority(const float *probs, int n_views, int batch, int h, int w, int k, uint8_t *final_out,
                                       void *stream_) {
    IMK_CHECK_ARG(probs && final_out && n_views > 0 && batch > 0 && h > 0 && w > 0 && k > 0);
    if (n_views > IMK_VIEWS_MAX || k > 256) return IMK_EUNSUPPORTED;
    const long long n_pix = (long long)batch * h * w;
    hipStream_t stream = (hipStream_t)stream_;
    ImkProfScope prof(PF_IM, (double)n_pix * ((double)n_views * k * 4 + 1), stream, (double)n_pix * n_views * k);
    imk_klaunch(vote_views_majority_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, stream, probs, n_views, n_pix, k,
                final_out);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
