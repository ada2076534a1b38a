// The Inconsistency-Mask rule, ONE device body per kernel of imk_im.hip, over a "model set": who votes for the image of this
// workgroup.  The whole-ensemble kernels (im_binary_vec, ..., head_im_softmax_kernel) pass AllModels, the per-image sub-ensemble
// kernels (im_binary_members_vec, ..., head_im_members_softmax_kernel) pass MemberBits; the __global__ entry points are shells that
// build the set and call the body, so with every bit set the members kernels run the arithmetic of the whole-ensemble kernels in the
// same order by construction.  A set is walked with `for (auto it = set.begin(); it.more(); it.next())` (a callback form cost 10 % more
// instructions in im_binary_vec), it.n() is the model, it.first() holds for the first one; all(votes): everybody voted foreground;
// row(n, b): the image of model n's slab that holds image b (fused kernels); POOL: the largest model index + 1 (LDS sizing).
#pragma once
#include "imk_common.h"
#include "imk_head.h"
#include "imk_imfin.h"

namespace {

// models 0 .. n_models - 1, every slab holding the whole batch
struct AllModels {
    static constexpr int POOL = IMK_HEAD_IM_MAX_MODELS;
    static constexpr bool PEEL_FIRST = false;      // head_im_softmax_body
    int n_models;
    struct It {
        int i, end;
        __device__ __forceinline__ bool more() const { return i < end; }
        __device__ __forceinline__ void next() { ++i; }
        __device__ __forceinline__ int n() const { return i; }
        __device__ __forceinline__ bool first() const { return i == 0; }
    };
    __device__ __forceinline__ It begin() const { return It{0, n_models}; }
    __device__ __forceinline__ bool all(int votes) const { return votes == n_models; }
    __device__ __forceinline__ int row(int, int b) const { return b; }
};

// The set bits of image b's member word, lowest first.  A workgroup never straddles two images, so the word is wave-uniform: it is
// read once into a scalar register and the walk is scalar code (s_ff1 / s_and), the votes vector code as before.  Bits at and above
// n_models are ignored.  rows [n_models][batch]: image b's position in model n's compacted batch (members only; fused kernels).
struct MemberBits {
    static constexpr int POOL = IMK_MEMBERS_MAX_POOL;
    static constexpr bool PEEL_FIRST = true;
    uint32_t word;
    int cnt;
    const int *rows;
    int batch;
    __device__ __forceinline__ MemberBits(const uint32_t *__restrict__ members, int b, int n_models, const int *rows_ = nullptr,
                                          int batch_ = 0) : rows(rows_), batch(batch_) {
        const uint32_t pool = n_models >= 32 ? 0xffffffffu : ((1u << n_models) - 1u);
        word = __builtin_amdgcn_readfirstlane(members[b] & pool);
        cnt = __builtin_popcount(word);
    }
    struct It {
        uint32_t m;
        bool head;      // a flag, not `m == word`: the compiler peels the first member off the loop for it
        __device__ __forceinline__ bool more() const { return m != 0; }
        __device__ __forceinline__ void next() { m &= m - 1; head = false; }
        __device__ __forceinline__ int n() const { return __builtin_ctz(m); }
        __device__ __forceinline__ bool first() const { return head; }
    };
    __device__ __forceinline__ It begin() const { return It{word, true}; }
    __device__ __forceinline__ bool all(int votes) const { return cnt != 0 && votes == cnt; }      // nobody votes: no label, no IM
    __device__ __forceinline__ int row(int n, int b) const { return rows[(size_t)n * batch + b]; }
};

// ---- binary / HeLa -----------------------------------------------------------------------------
// the votes of a thread's 4 pixels -> label / IM bytes in LDS at px0 and the thread's share of the per-image sizes
template <int KB, class Set>
__device__ __forceinline__ void im_votes_finish(const Set &set, const int (&votes)[4][KB], int block_out, int (&cnt_fg)[KB],
                                                int (&cnt_mx)[KB], uint8_t (*s_final)[BIN_CHUNK], uint8_t *s_im, int px0) {
    uint32_t fin[KB], im4 = 0;
#pragma unroll
    for (int k = 0; k < KB; ++k) fin[k] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bool any = false, fg[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            fg[k] = set.all(votes[j][k]);
            const bool mx = (votes[j][k] != 0) && !fg[k];
            cnt_fg[k] += fg[k];
            cnt_mx[k] += mx;
            any |= mx;
        }
        if (any) im4 |= 0xffu << (8 * j);
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (fg[k] && !(block_out && any)) fin[k] |= 0xffu << (8 * j);
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) *reinterpret_cast<uint32_t *>(&s_final[k][px0]) = fin[k];
    *reinterpret_cast<uint32_t *>(&s_im[px0]) = im4;
}

// grid (ceil(HW/1024), B); requires HW % 4 == 0 and 16-byte aligned preds (host checks), else the generic body below runs.
template <int KB, class Set>
__device__ __forceinline__ void im_binary_vec_body(
    const Set set, const float *__restrict__ preds, int batch, int hw, float thr, int cmp_ge,
    const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ masks_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, unsigned long long *__restrict__ pred_size, int vec_out, int vec_img) {
    __shared__ __attribute__((aligned(16))) uint8_t s_final[KB][BIN_CHUNK];
    __shared__ __attribute__((aligned(16))) uint8_t s_im[BIN_CHUNK];
    __shared__ int s_cnt[2 * KB];
    const int b = blockIdx.y;
    const int p_base = blockIdx.x * BIN_CHUNK;
    const int t = threadIdx.x;
    const int p0 = p_base + 4 * t;
    if (t < 2 * KB) s_cnt[t] = 0;
    int cnt_fg[KB], cnt_mx[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) cnt_fg[k] = cnt_mx[k] = 0;

    if (p0 < hw) {
        int s[4][KB];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < KB; ++k) s[j][k] = 0;
        for (auto it = set.begin(); it.more(); it.next()) {
            const float4 *src = reinterpret_cast<const float4 *>(preds + ((size_t)(it.n() * batch + b) * hw + p0) * KB);
            float v[4 * KB];
#pragma unroll
            for (int q = 0; q < KB; ++q) {
                const float4 f = src[q];
                v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
            }
#pragma unroll
            for (int i = 0; i < 4 * KB; ++i) {
                const bool hit = cmp_ge ? (v[i] >= thr) : (v[i] > thr);  // NaN compares false
                s[i / KB][i % KB] += hit ? 1 : 0;
            }
        }
        im_votes_finish<KB>(set, s, block_out, cnt_fg, cnt_mx, s_final, s_im, 4 * t);
    }
    __syncthreads();
    // per-image sizes: wave reduction, one LDS atomic per wave, one global atomic per workgroup
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        int a = cnt_fg[k], m = cnt_mx[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); m += __shfl_xor(m, o, 64); }
        if ((t & 63) == 0) { atomicAdd(&s_cnt[2 * k], a); atomicAdd(&s_cnt[2 * k + 1], m); }
    }
    __syncthreads();
    if (t < KB) {
        if (s_cnt[2 * t]) atomicAdd(&pred_size[(size_t)b * KB + t], (unsigned long long)s_cnt[2 * t]);
        if (s_cnt[2 * t + 1]) atomicAdd(&im_size[(size_t)b * KB + t], (unsigned long long)s_cnt[2 * t + 1]);
    }
    const int n_px = min(BIN_CHUNK, hw - p_base);
#pragma unroll
    for (int k = 0; k < KB; ++k)
        store_bytes<BIN_CHUNK>(masks_out + ((size_t)b * KB + k) * hw + p_base, s_final[k], n_px, vec_out);
    store_bytes<BIN_CHUNK>(im_out + (size_t)b * hw + p_base, s_im, n_px, vec_out);
    if (img) {
        const size_t off = ((size_t)b * hw + p_base) * c;
        block_image(img + off, img_out + off, s_im, n_px, c, block_in, vec_img);
    }
}

// Any shape / alignment: one pixel per thread.  Used for odd sizes only.
template <class Set>
__device__ __forceinline__ void im_binary_generic_body(
    const Set set, const float *__restrict__ preds, int batch, int hw, int kb, float thr, int cmp_ge,
    const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ masks_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, unsigned long long *__restrict__ pred_size) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    bool any = false;
    for (int k = 0; k < kb; ++k) {
        int s = 0;
        for (auto it = set.begin(); it.more(); it.next()) {
            const float v = preds[((size_t)(it.n() * batch + b) * hw + p) * kb + k];
            s += cmp_ge ? (v >= thr) : (v > thr);
        }
        const bool fg = set.all(s);
        const bool mx = (s != 0) && !fg;
        any |= mx;
        if (fg) atomicAdd(&pred_size[(size_t)b * kb + k], 1ull);
        if (mx) atomicAdd(&im_size[(size_t)b * kb + k], 1ull);
        masks_out[((size_t)b * kb + k) * hw + p] = fg ? 255 : 0;
    }
    im_out[(size_t)b * hw + p] = any ? 255 : 0;
    if (block_out && any)
        for (int k = 0; k < kb; ++k) masks_out[((size_t)b * kb + k) * hw + p] = 0;
    if (img)
        for (int ch = 0; ch < c; ++ch) {
            const size_t i = ((size_t)b * hw + p) * c + ch;
            img_out[i] = (block_in && any) ? 0 : img[i];
        }
}

// ---- multiclass ----------------------------------------------------------------------------------
// grid (ceil(HW/256), B), dynamic LDS = 256 * (K|1) floats.  Each model's [256 px][K] slab is read
// with coalesced 16-byte loads into LDS (odd row stride: conflict-free column walks), then one thread
// per pixel takes np.argmax (np_argmax_step, imk_head.h: the first maximum wins, and a NaN counts as the maximum -- the
// first NaN wins).
// The reference anchors the comparison on the first sampled model (functions.py:3128); agreement of all members is symmetric, so
// the lowest member is the anchor here, whatever the sampling order was.
template <class Set>
__device__ __forceinline__ void im_multi_body(
    const Set set, const float *__restrict__ probs, int batch, int hw, int k_classes, uint32_t magic_k,
    const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ final_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, uint8_t *__restrict__ presence, int vec_in, int vec_out, int vec_img) {
    extern __shared__ __attribute__((aligned(16))) float s_p[];
    __shared__ __attribute__((aligned(16))) uint8_t s_final[MC_CHUNK];
    __shared__ __attribute__((aligned(16))) uint8_t s_im[MC_CHUNK];
    __shared__ uint32_t s_pres[64];
    __shared__ int s_cnt;
    const int ks = k_classes | 1;
    const int b = blockIdx.y;
    const int p_base = blockIdx.x * MC_CHUNK;
    const int n_px = min(MC_CHUNK, hw - p_base);
    const int t = threadIdx.x;
    if (t == 0) s_cnt = 0;
    int label0 = 0;
    bool agree = true;
    for (auto it = set.begin(); it.more(); it.next()) {
        const int n = it.n();
        if (t < 64) s_pres[t] = 0;
        const float *src = probs + ((size_t)(n * batch + b) * hw + p_base) * k_classes;
        const int total = n_px * k_classes;
        if (vec_in && (total & 3) == 0) {
            for (int i = t; i < total / 4; i += 256) {
                const float4 v = reinterpret_cast<const float4 *>(src)[i];
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t idx = 4u * i + q;
                    const uint32_t px = __umulhi(idx, magic_k);  // idx / K, exact for idx*K < 2^32
                    s_p[px * ks + (idx - px * k_classes)] = e[q];
                }
            }
        } else {
            for (int i = t; i < total; i += 256) {
                const int px = i / k_classes;
                s_p[px * ks + (i - px * k_classes)] = src[i];
            }
        }
        __syncthreads();
        if (t < n_px) {
            const float *row = s_p + t * ks;
            int best = -1;
            float bv = 0.f;
            for (int k = 0; k < k_classes; ++k) np_argmax_step(row[k], k, bv, best);
            s_pres[best] = 1;
            if (it.first()) label0 = best; else agree = agree && (best == label0);
        }
        __syncthreads();
        if (presence && t < k_classes && s_pres[t]) presence[((size_t)n * batch + b) * k_classes + t] = 1;
    }
    int dis = 0;
    if (t < n_px) {
        const uint8_t im = agree ? 0 : 255;
        s_im[t] = im;
        s_final[t] = (agree && !(block_out && im)) ? (uint8_t)label0 : 0;
        dis = agree ? 0 : 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dis += __shfl_xor(dis, o, 64);
    if ((t & 63) == 0 && dis) atomicAdd(&s_cnt, dis);
    __syncthreads();
    if (t == 0 && s_cnt) atomicAdd(&im_size[b], (unsigned long long)s_cnt);
    store_bytes<MC_CHUNK>(final_out + (size_t)b * hw + p_base, s_final, n_px, vec_out);
    store_bytes<MC_CHUNK>(im_out + (size_t)b * hw + p_base, s_im, n_px, vec_out);
    if (img) {
        const size_t off = ((size_t)b * hw + p_base) * c;
        block_image(img + off, img_out + off, s_im, n_px, c, block_in, vec_img);
    }
}

// ---- head + IM in one pass (ensemble inference: imk_unet_forward_im, imk_unet_forward_im_members) ---------------------------------
// The probability stack [N,B,H,W,K] fp32 never exists: every model's output layer (BatchNorm on load, fp32 1x1 conv,
// sigmoid / softmax -- the arithmetic of head_kernel, imk_head.h) is evaluated per pixel in registers / LDS and goes
// straight into the vote.  Per pixel it reads N x cs fp16 + the image and writes image + label map(s) + IM:
// ISIC 2 x 16 + 3 B in, 5 B out (SURVEY 8d's fused figure) instead of 8 + 3 in / 5 out behind 2 x (16 in, 4 out).
// A workgroup never straddles two images.  Sigmoid heads: 4 consecutive pixels per thread (1024 per workgroup); with a
// compile-time model count (NM > 0, AllModels) all N x 4 activation loads of a thread are issued before the first use, otherwise
// each model's four-pixel loads go out before its votes.  Only the set's head images are staged (slot n of the LDS image = model n).
// Softmax heads: the matrix-core arithmetic of imk_head.h (HeadMfma), four lanes per pixel.
template <int CS, int KB, int NM /* models, compile-time (0: run-time) */, class Set, class Args>
__device__ __forceinline__ void head_im_sigmoid_body(const Set set, const Args &a, int vec_out, int vec_img) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];   // POOL x head image (imk_head.h)
    __shared__ __attribute__((aligned(16))) uint8_t s_final[KB][BIN_CHUNK];
    __shared__ __attribute__((aligned(16))) uint8_t s_im[BIN_CHUNK];
    __shared__ int s_cnt[2 * KB];
    const int K = a.K, hw = a.hw;
    const int per_model = head_lds_floats<CS>(K);
    const int b = blockIdx.y, t = threadIdx.x;
    const int p_base = blockIdx.x * BIN_CHUNK;
    const int n_px = min(BIN_CHUNK, hw - p_base);
    for (auto it = set.begin(); it.more(); it.next()) {
        const int n = it.n();
        head_stage<CS>(a.w[n], a.bias[n], a.sc[n], a.sh[n], a.cin, K, s_dyn + n * per_model);
    }
    if (t < 2 * KB) s_cnt[t] = 0;
    int cnt_a[KB], cnt_m[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) cnt_a[k] = cnt_m[k] = 0;
    const int p0 = 4 * t;                                   // hw % 16 == 0: a thread's 4 pixels are all in or all out
    constexpr int NMR = NM > 0 ? NM : 1;
    f16x8 raw[NMR][4][CS / 8];
    if (NM > 0 && p0 < n_px) {                               // every activation load of this thread goes out first
#pragma unroll
        for (int n = 0; n < NMR; ++n) {
            const long long p = (long long)set.row(n, b) * hw + p_base + p0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < CS / 8; ++q) raw[n][j][q] = *reinterpret_cast<const f16x8 *>(a.z[n] + (p + j) * CS + q * 8);
        }
    }
    __syncthreads();                                         // head images staged
    if (p0 < n_px) {
        int votes[4][KB];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < KB; ++k) votes[j][k] = 0;
        auto vote = [&](const float *hw_n, const f16x8 (&r)[CS / 8], int j) {
            float xin[CS];
            head_input_regs<CS>(r, hw_n, K, xin);
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const float v = head_sigmoid(head_logit<CS>(xin, hw_n, K, k));
                votes[j][k] += (a.cmp_ge ? (v >= a.thr) : (v > a.thr)) ? 1 : 0;      // NaN compares false
            }
        };
        if constexpr (NM > 0) {
#pragma unroll
            for (int n = 0; n < NMR; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) vote(s_dyn + n * per_model, raw[n][j], j);
        } else {
            for (auto it = set.begin(); it.more(); it.next()) {
                const int n = it.n();
                const long long p = (long long)set.row(n, b) * hw + p_base + p0;
                f16x8 r[4][CS / 8];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int q = 0; q < CS / 8; ++q) r[j][q] = *reinterpret_cast<const f16x8 *>(a.z[n] + (p + j) * CS + q * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) vote(s_dyn + n * per_model, r[j], j);
            }
        }
        im_votes_finish<KB>(set, votes, a.block_out, cnt_a, cnt_m, s_final, s_im, p0);
    }
    __syncthreads();
    head_im_finish<KB>(a, s_final, s_im, s_cnt, cnt_a, cnt_m, true, b, p_base, n_px, vec_out, vec_img);
}

// Softmax heads: HeadMfma (imk_head.h) gives every group of 4 lanes the K probabilities of one pixel; a wave takes 64 of
// the workgroup's 256 pixels (4 units of 16), model after model of the set (a model's fragments are loaded for the set only), and
// keeps label / agreement per unit in registers.
template <int KT, class Set, class Args>
__device__ __forceinline__ void head_im_softmax_body(const Set set, const Args &a, int vec_out, int vec_img) {
    __shared__ __attribute__((aligned(16))) uint8_t s_final[1][BIN_CHUNK];   // MC_CHUNK bytes used
    __shared__ __attribute__((aligned(16))) uint8_t s_im[BIN_CHUNK];
    __shared__ uint32_t s_pres[Set::POOL][64];
    __shared__ int s_cnt[2];
    const int K = a.K, hw = a.hw, cs = a.cs;
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, p16 = lane & 15, g = lane >> 4;
    const int p_base = blockIdx.x * MC_CHUNK;
    const int n_px = min(MC_CHUNK, hw - p_base);
    for (int i = t; i < Set::POOL * 64; i += 256) (&s_pres[0][0])[i] = 0;
    if (t < 2) s_cnt[t] = 0;
    __syncthreads();
    int cnt_a[1] = {0}, cnt_m[1] = {0};
    int label0[4] = {0, 0, 0, 0};
    bool agree[4] = {true, true, true, true};
    auto model = [&](const typename Set::It &it) {
        const int n = it.n();
        const int row = set.row(n, b);
        HeadMfma<KT> h;
        h.load(a.w[n], a.bias[n], a.sc[n], a.sh[n], a.cin, cs, K);
        f16x8 zr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = 64 * wave + 16 * u + p16;
            zr[u] = h.load_z(a.z[n], (long long)row * hw + p_base + (q < n_px ? q : 0), cs);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f32x4 pr[KT];
            h.probs(zr[u], K, pr);
            const int best = h.argmax(pr, K);
            if (g == 0 && 64 * wave + 16 * u + p16 < n_px) s_pres[n][best] = 1;
            if (it.first()) label0[u] = best; else agree[u] = agree[u] && (best == label0[u]);
        }
    };
    // Left alone the compiler peels the first model off the loop at some KT.  The choice below reproduces, for KT >= 2, the code both
    // kernels had as separate copies: peeled for the member bits (K 19: 125 registers; unpeeled 130 and a wave less per SIMD), one copy
    // of the body for all models (K 19: 128 registers).  The timings of the other choices are in DESIGN.md, "EvalNet training data".
    if constexpr (Set::PEEL_FIRST) {
        for (auto it = set.begin(); it.more(); it.next()) model(it);
    } else {
#pragma clang loop unroll(disable)
        for (auto it = set.begin(); it.more(); it.next()) model(it);
    }
    if (g == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = 64 * wave + 16 * u + p16;
            if (q < n_px) {
                const uint8_t im = agree[u] ? 0 : 255;
                s_im[q] = im;
                s_final[0][q] = (agree[u] && !(a.block_out && im)) ? (uint8_t)label0[u] : 0;
                cnt_m[0] += agree[u] ? 0 : 1;
            }
        }
    }
    __syncthreads();
    if (a.presence)
        for (int i = t; i < a.n_models * 64; i += 256) {
            const int n = i >> 6, k = i & 63;
            if (k < K && s_pres[n][k]) a.presence[((size_t)n * a.batch + b) * K + k] = 1;
        }
    head_im_finish<1>(a, s_final, s_im, s_cnt, cnt_a, cnt_m, false, b, p_base, n_px, vec_out, vec_img);
}

// ---- morphology (cold path: EK = DK = 0 in every shipped config) ---------------------------------------------------------------
// ksize: the window of image blockIdx.z.  COPY0 (imk_morph_var): a window of 0 copies the image.
template <bool COPY0>
__device__ __forceinline__ void morph_body(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int h, int w, int ksize,
                                           int op) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t *s = src + (size_t)b * h * w;
    if (COPY0 && ksize <= 0) {
        dst[(size_t)b * h * w + (size_t)y * w + x] = s[(size_t)y * w + x];
        return;
    }
    const int a = ksize / 2;
    int acc = op ? 0 : 255;
    for (int dy = -a; dy < ksize - a; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= h) continue;
        for (int dx = -a; dx < ksize - a; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= w) continue;
            const int v = s[(size_t)yy * w + xx];
            acc = op ? max(acc, v) : min(acc, v);
        }
    }
    dst[(size_t)b * h * w + (size_t)y * w + x] = (uint8_t)acc;
}

}  // namespace
