// The depth-map (regression) family on the GPU: the standard-deviation inconsistency mask of get_im_prediction_depth_map
// (functions.py:6155-6177) and the evaluation sums of benchmark_depth_map / delta_metric / rmse (functions.py:36-48, 1345-1384).
//
// The IM rule is not a vote: a pixel is inconsistent where the ensemble's per-pixel standard deviation exceeds threshold_multiplier
// times the IMAGE's mean standard deviation, so the threshold of an image hangs on a reduction over the whole image -- and the
// project's contract for IM masks is bit-exactness given identical predictions, so that reduction is numpy's, in numpy's order:
//
//   S(a[0..n)), numpy's float32 add.reduce of a contiguous run (pairwise_sum, numpy/core/src/umath/loops_utils.h.src):
//     n < 8           sequential from the left
//     8 <= n <= 128   r[j] = a[j] (j < 8); r[j] += a[i + j] for i = 8, 16, .. below n - n % 8;
//                     ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then the n % 8 remaining elements, sequentially
//     n > 128         S(a[0..n2)) + S(a[n2..n)),  n2 = n / 2, n2 -= n2 % 8
//   and a whole-array reduction is cut into chunks of 8192 elements (numpy's default buffer size): S(chunk 0), then + S(chunk 1),
//   + S(chunk 2) ... sequentially; the last chunk may be short and follows the recursion with its own leaf sizes.
//
//   per pixel over the N models (np.std(axis=-1)):  m = S(p) / N,  d_n = p_n - m,  std = sqrt(S(d_n * d_n) / N)
//   per image (np.mean):                            mean = S_chunked(std over H*W) / (H*W),  thr = float32(mult) * mean,  im = std > thr
//
// float32 throughout, every operation rounded on its own: `#pragma clang fp contract(off)` in every function that forms these values
// (hipcc would turn a + d * d into one FMA, which changes bits), and plain `/` and sqrtf, which hipcc compiles correctly rounded
// (-fhip-fp32-correctly-rounded-divide-sqrt, its default).  The __f*_rn spellings are NOT used: without OCML_BASIC_ROUNDED_OPERATIONS
// the compiler's header defines __fadd_rn as a plain (contractable) `x + y` and __fsqrt_rn as the native, not correctly rounded, sqrt.
// IEEE addition is commutative, so a butterfly (v += shfl_xor(v, 1), 2, 4, ...) forms exactly the balanced trees above in every lane.
// `2 * np.float32` is float32 under numpy >= 2; under numpy < 2 the product is formed in double and rounded once, which is the same
// value for every multiplier that is representable in float32 (a 24 x 24 bit product is exact in double).
// NaN propagates: one NaN prediction makes thr NaN and the image's whole IM zero.
//
// Three launches: (1) std per pixel -> an fp32 map, 4 pixels per thread; (2) one workgroup per image: a wave per 8192-chunk (eight
// lanes per 128-leaf, eight leaves per pass, the chunk's balanced tree in registers), the short last chunk through a leaf table the
// host derives from H*W (kernel argument), the chunk chain by one thread; (3) mask + blocking + im_size, byte outputs staged through
// LDS, one integer atomic per workgroup, a workgroup never straddles two images.  No float atomics anywhere.
#include "imk_common.h"
#include "imk_head.h"

namespace {

constexpr int DEPTH_MIN_MODELS = 2, DEPTH_MAX_MODELS = 16;
constexpr int NP_CHUNK = 8192;     // numpy's default ufunc buffer, in elements
constexpr int NP_LEAF = 128;       // pairwise_sum's PW_BLOCKSIZE
constexpr int PX_CHUNK = 1024;     // pixels per workgroup of launches 1 and 3 (4 per thread)
constexpr int MAX_LEAVES = 128;    // a run of fewer than 8192 elements has at most 127 leaves (every leaf of a split run has >= 64)
constexpr int MAX_CHUNKS = 2048;   // H*W <= 2^24

struct DepthLeaves {               // the short last chunk's leaves in order, with their depth in the recursion
    int n;
    uint16_t off[MAX_LEAVES], len[MAX_LEAVES];
    uint8_t depth[MAX_LEAVES];
};

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// S over the N models of one pixel
template <int N>
__device__ __forceinline__ float sum_models(const float (&a)[N]) {
#pragma clang fp contract(off)
    if constexpr (N < 8) {
        float r = a[0];
#pragma unroll
        for (int i = 1; i < N; ++i) r = r + a[i];
        return r;
    } else {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        if constexpr (N == 16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = r[j] + a[8 + j];
        }
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int i = N - N % 8; i < N; ++i) res = res + a[i];
        return res;
    }
}

template <int N>
__device__ __forceinline__ float std_models(const float (&p)[N]) {
#pragma clang fp contract(off)
    const float fn = (float)N;
    const float m = sum_models<N>(p) / fn;
    float d[N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const float e = p[n] - m;
        d[n] = e * e;
    }
    return sqrtf(sum_models<N>(d) / fn);
}

// launch 1: grid (ceil(HW / 1024), B).  VEC: HW % 4 == 0 and 16-byte aligned preds / map.
template <int N, bool VEC>
__global__ __launch_bounds__(256) void depth_std_kernel(const float *__restrict__ preds, int batch, int hw, float *__restrict__ map) {
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * PX_CHUNK + 4 * threadIdx.x;
    if (p0 >= hw) return;
    float v[4][N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const float *src = preds + ((size_t)n * batch + b) * hw + p0;
        if constexpr (VEC) {
            const float4 f = *reinterpret_cast<const float4 *>(src);
            v[0][n] = f.x; v[1][n] = f.y; v[2][n] = f.z; v[3][n] = f.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j][n] = (p0 + j < hw) ? src[j] : 0.f;
        }
    }
    float s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = std_models<N>(v[j]);
    float *dst = map + (size_t)b * hw + p0;
    if constexpr (VEC) {
        *reinterpret_cast<float4 *>(dst) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < hw) dst[j] = s[j];
    }
}

// launch 1 fused with the ensemble's heads (imk_unet_forward_im_depth): every model's probability comes from the code of imk_head.h
// (head_stage / head_input / head_logit / head_sigmoid, the arithmetic of head_kernel) on its last decoder activation and goes straight
// into the standard deviation -- the fp32 probability stack is never written, and the map holds the bits launch 1 above writes for the
// stack imk_unet_forward would have written.  Which of the logit's products the compiler fuses into the running sum is its choice, made
// per loop body (head_kernel at 16 channels: the first eight fused, the last eight rounded on their own); with several pixels unrolled
// into one body it chose differently for one of them, and a fifth of the standard deviations moved by an ulp.  So the head runs here in
// head_kernel's own shape: ONE pixel per loop body, K a run-time value, nothing unrolled around it (models and the thread's four pixels
// are loops that stay loops; thread t takes pixels t, t + 256, ... of the workgroup's 1024, so neighbouring lanes read neighbouring
// activation rows).  The probabilities wait in LDS, [model][pixel]; behind a barrier thread t takes pixels 4t .. 4t + 3 for the
// standard deviation and the 16-byte store.  tests/test_gpu_im_depth.py holds all four widths to bit-identity with the unfused route.
// grid (ceil(HW / 1024), B); HW % 16 == 0.
template <int CS>
__device__ __forceinline__ void depth_head_probs(const ImkDepthHeadArgs &a, const float *s_dyn, float *s_p, long long img_base, int n_px) {
    const int K = a.K;
    const int per_model = head_lds_floats<CS>(K);
#pragma unroll 1
    for (int n = 0; n < a.n_models; ++n) {
        const float *hw_n = s_dyn + n * per_model;
#pragma unroll 1
        for (int px = threadIdx.x; px < n_px; px += 256) {
            float xin[CS];
            head_input<CS>(a.z[n], img_base + px, hw_n, K, xin);
            s_p[n * PX_CHUNK + px] = head_sigmoid(head_logit<CS>(xin, hw_n, K, 0));
        }
    }
}

template <int CS, int N>
__global__ __launch_bounds__(256) void depth_head_std_kernel(ImkDepthHeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];   // N x head image (imk_head.h), then N x 1024 probabilities
    const int per_model = head_lds_floats<CS>(a.K);
    float *s_p = s_dyn + ((N * per_model + 3) & ~3);
    const int b = blockIdx.y, t = threadIdx.x;
    const int p_base = blockIdx.x * PX_CHUNK;
    const int n_px = min(PX_CHUNK, a.hw - p_base);
    for (int n = 0; n < N; ++n) head_stage<CS>(a.w[n], a.bias[n], a.sc[n], a.sh[n], a.cin, a.K, s_dyn + n * per_model);
    __syncthreads();
    const long long img_base = (long long)b * a.hw + p_base;
    depth_head_probs<CS>(a, s_dyn, s_p, img_base, n_px);
    __syncthreads();
    if (4 * t >= n_px) return;
    float v[4][N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const float4 f = *reinterpret_cast<const float4 *>(s_p + n * PX_CHUNK + 4 * t);
        v[0][n] = f.x; v[1][n] = f.y; v[2][n] = f.z; v[3][n] = f.w;
    }
    float s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = std_models<N>(v[j]);
    *reinterpret_cast<float4 *>(a.map + img_base + 4 * t) = make_float4(s[0], s[1], s[2], s[3]);
}

// launch 2: grid (B), 1024 threads.  thr_out[b] = mult * (S_chunked(map[b]) / HW)
__global__ __launch_bounds__(1024) void depth_thr_kernel(const float *__restrict__ map, int hw, float mult, DepthLeaves lv,
                                                         float *__restrict__ thr_out) {
#pragma clang fp contract(off)
    __shared__ float s_chunk[MAX_CHUNKS];
    __shared__ float s_leaf[MAX_LEAVES];
    __shared__ float s_stack[16];
    __shared__ int s_depth[16];
    __shared__ float s_part[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float *a = map + (size_t)blockIdx.x * hw;
    const int n_full = hw / NP_CHUNK;
    const int j = lane & 7;
    // the short last chunk: eight lanes per leaf, all leaves at once (at most 128 leaves = 1024 lanes)
    {
        const int leaf = t >> 3;
        const bool on = leaf < lv.n;
        const float *q = a + (size_t)n_full * NP_CHUNK + (on ? lv.off[leaf] : 0);
        const int len = on ? lv.len[leaf] : 0;
        const int m = len - (len & 7);
        float r = 0.f;
        if (m > 0) {
            r = q[j];
            for (int i = 8; i < m; i += 8) r = r + q[i + j];
        }
        r = r + __shfl_xor(r, 1, 64);
        r = r + __shfl_xor(r, 2, 64);
        r = r + __shfl_xor(r, 4, 64);
        if (on && j == 0) {
            int i = m;
            if (m == 0) { r = q[0]; i = 1; }                   // fewer than 8 elements: sequential from the left
            for (; i < len; ++i) r = r + q[i];
            s_leaf[leaf] = r;
        }
    }
    // the full chunks: a wave per chunk; a pass takes eight 128-leaves (eight lanes each), the butterfly over all 64 lanes is the
    // balanced tree over those eight leaves, and the eight pass results meet in the tree's upper three levels
    for (int c = wave; c < n_full; c += 16) {
        const float *q = a + (size_t)c * NP_CHUNK + (lane >> 3) * NP_LEAF + j;
        float g[8];
#pragma unroll
        for (int pass = 0; pass < 8; ++pass) {
            const float *qq = q + pass * 8 * NP_LEAF;
            float x[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] = qq[8 * i];
            float r = x[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) r = r + x[i];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) r = r + __shfl_xor(r, o, 64);
            g[pass] = r;
        }
        if (lane == 0) s_chunk[c] = ((g[0] + g[1]) + (g[2] + g[3])) + ((g[4] + g[5]) + (g[6] + g[7]));
    }
    __syncthreads();
    if (t == 64 && lv.n > 0) {
        // the recursion's additions in post-order: two neighbours of one depth are the halves of one run
        int sp = 0;
        for (int i = 0; i < lv.n; ++i) {
            float v = s_leaf[i];
            int d = lv.depth[i];
            while (sp > 0 && s_depth[sp - 1] == d) {
                v = s_stack[sp - 1] + v;
                --sp;
                --d;
            }
            s_stack[sp] = v;
            s_depth[sp] = d;
            ++sp;
        }
        s_part[1] = s_stack[0];
    }
    if (t == 0 && n_full > 0) {
        float r = s_chunk[0];
        for (int c = 1; c < n_full; ++c) r = r + s_chunk[c];
        s_part[0] = r;
    }
    __syncthreads();
    if (t == 0) {
        const float total = n_full > 0 ? (lv.n > 0 ? s_part[0] + s_part[1] : s_part[0]) : s_part[1];
        const float mean = total / (float)hw;
        thr_out[blockIdx.x] = mult * mean;
    }
}

// launch 3: grid (ceil(HW / 1024), B)
template <bool VEC>
__global__ __launch_bounds__(256) void depth_mask_kernel(const float *__restrict__ map, const float *__restrict__ thr_in, int hw,
                                                         const uint8_t *__restrict__ img, int c, int block_in,
                                                         uint8_t *__restrict__ img_out, uint8_t *__restrict__ im_out,
                                                         unsigned long long *__restrict__ im_size, int vec_out, int vec_img) {
    __shared__ __attribute__((aligned(16))) uint8_t s_im[PX_CHUNK];
    __shared__ int s_cnt;
    const int b = blockIdx.y, t = threadIdx.x;
    const int p_base = blockIdx.x * PX_CHUNK;
    const int n_px = min(PX_CHUNK, hw - p_base);
    const int p0 = 4 * t;
    const float thr = thr_in[b];
    if (t == 0) s_cnt = 0;
    int cnt = 0;
    if (p0 < n_px) {
        const float *src = map + (size_t)b * hw + p_base + p0;
        float v[4];
        if constexpr (VEC) {
            const float4 f = *reinterpret_cast<const float4 *>(src);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = (p0 + q < n_px) ? src[q] : 0.f;
        }
        uint32_t im4 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool hit = (p0 + q < n_px) && (v[q] > thr);      // NaN on either side compares false
            cnt += hit;
            if (hit) im4 |= 0xffu << (8 * q);
        }
        *reinterpret_cast<uint32_t *>(&s_im[p0]) = im4;
    }
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((t & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (t == 0 && s_cnt) atomicAdd(&im_size[b], (unsigned long long)s_cnt);
    uint8_t *dst = im_out + (size_t)b * hw + p_base;
    if (vec_out) {
        for (int i = t; i < n_px / 16; i += 256) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(s_im)[i];
    } else {
        for (int i = t; i < n_px; i += 256) dst[i] = s_im[i];
    }
    if (img) {
        const size_t off = ((size_t)b * hw + p_base) * c;
        const uint8_t *isrc = img + off;
        uint8_t *idst = img_out + off;
        const int nbytes = n_px * c;
        if (vec_img) {
            for (int i = t; i < nbytes / 16; i += 256) {
                uint4 v = reinterpret_cast<const uint4 *>(isrc)[i];
                if (block_in) {
                    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t keep = 0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int idx = i * 16 + q * 4 + k;
                            const int px = (c == 3) ? idx / 3 : (c == 1 ? idx : idx / c);
                            keep |= (s_im[px] ? 0u : 0xffu) << (8 * k);
                        }
                        w[q] &= keep;
                    }
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                reinterpret_cast<uint4 *>(idst)[i] = v;
            }
        } else {
            for (int i = t; i < nbytes; i += 256) idst[i] = (block_in && s_im[i / c]) ? 0 : isrc[i];
        }
    }
}

// ---- evaluation ------------------------------------------------------------------------------------------------------------
// grid (B), 1024 threads: a thread owns the pixels t, t + 1024, ... of its image and adds them in that order, the 1024 partial sums
// meet in a fixed balanced tree -- the summation order is a function of H*W alone.
__global__ __launch_bounds__(1024) void eval_depth_kernel(const float *__restrict__ probs, const uint8_t *__restrict__ gt, int hw,
                                                          uint8_t *__restrict__ pred_out, double *__restrict__ sums) {
#pragma clang fp contract(off)
    __shared__ double s_sq[1024];
    __shared__ int s_n[16];
    const int b = blockIdx.x, t = threadIdx.x;
    const float *p = probs + (size_t)b * hw;
    const uint8_t *g = gt + (size_t)b * hw;
    double sq = 0.0;
    int cnt = 0;
    for (int i = t; i < hw; i += 1024) {
        const float v = p[i];
        const float y = (float)g[i] / 255.0f;
        const float e = v - y;
        sq = sq + (double)e * (double)e;
        const float r1 = v / y, r2 = y / v;                     // tf.maximum hands a NaN on, `<` is false on it
        cnt += (r1 < 1.25f) && (r2 < 1.25f);
        if (pred_out) {
            const float s = v * 255.0f;                         // clip(p * 255, 0, 255) truncated; NaN -> 0
            pred_out[(size_t)b * hw + i] = s > 0.f ? (s < 255.f ? (uint8_t)s : (uint8_t)255) : (uint8_t)0;
        }
    }
    s_sq[t] = sq;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((t & 63) == 0) s_n[t >> 6] = cnt;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) s_sq[t] = s_sq[t] + s_sq[t + o];
        __syncthreads();
    }
    if (t == 0) {
        int n = 0;
        for (int i = 0; i < 16; ++i) n += s_n[i];
        sums[2 * b] = s_sq[0];
        sums[2 * b + 1] = (double)n;
    }
}

// the recursion of pairwise_sum on a run of n < 8192 elements: its leaves in order, with their depth
void depth_leaves(int off, int n, int depth, DepthLeaves &lv) {
    if (n <= NP_LEAF) {
        lv.off[lv.n] = (uint16_t)off; lv.len[lv.n] = (uint16_t)n; lv.depth[lv.n] = (uint8_t)depth;
        ++lv.n;
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    depth_leaves(off, n2, depth + 1, lv);
    depth_leaves(off + n2, n - n2, depth + 1, lv);
}

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

template <int N>
void launch_std(const float *preds, int batch, int hw, float *map, bool vec, hipStream_t stream) {
    const dim3 grid(imk_cdiv(hw, PX_CHUNK), batch);
    if (vec) imk_klaunch(depth_std_kernel<N, true>, dim3(grid), dim3(256), 0, stream, preds, batch, hw, map);
    else imk_klaunch(depth_std_kernel<N, false>, dim3(grid), dim3(256), 0, stream, preds, batch, hw, map);
}

}  // namespace

extern "C" int64_t imk_im_depth_workspace_bytes(int batch, int h, int w) {
    if (batch <= 0 || h <= 0 || w <= 0) return IMK_EINVAL;
    if ((int64_t)h * w > (int64_t)MAX_CHUNKS * NP_CHUNK || batch > 65535) return IMK_EUNSUPPORTED;
    return align256((int64_t)batch * h * w * (int64_t)sizeof(float));
}

extern "C" int imk_im_depth(const float *preds, int n_models, int batch, int h, int w, float mult, const uint8_t *img, int c,
                            int block_in, uint8_t *img_out, uint8_t *im_out, int64_t *im_size, float *thr_out, float *std_out,
                            void *workspace, int64_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    IMK_CHECK_ARG(preds && im_out && im_size && thr_out && batch > 0 && h > 0 && w > 0);
    IMK_CHECK_ARG(!img || (img_out && c > 0));
    if (n_models < DEPTH_MIN_MODELS || n_models > DEPTH_MAX_MODELS) return IMK_EUNSUPPORTED;
    const int64_t need = imk_im_depth_workspace_bytes(batch, h, w);
    if (need < 0) return (int)need;
    float *map = std_out;                                      // the caller's map is the map; the workspace is not touched then
    if (!map) {
        IMK_CHECK_ARG(workspace);
        if (workspace_bytes < need) return IMK_EWORKSPACE;
        map = static_cast<float *>(workspace);
    }
    const int hw = h * w;
    const bool vec = (hw % 4 == 0) && aligned16(preds) && aligned16(map);
    ImkProfScope prof(PF_IM, (double)batch * hw * ((double)n_models * 4 + (img ? 2.0 * c : 0.0) + 1), stream);
    switch (n_models) {
#define IMK_DEPTH_N(NV) case NV: launch_std<NV>(preds, batch, hw, map, vec, stream); break;
        IMK_DEPTH_N(2) IMK_DEPTH_N(3) IMK_DEPTH_N(4) IMK_DEPTH_N(5) IMK_DEPTH_N(6) IMK_DEPTH_N(7) IMK_DEPTH_N(8) IMK_DEPTH_N(9)
        IMK_DEPTH_N(10) IMK_DEPTH_N(11) IMK_DEPTH_N(12) IMK_DEPTH_N(13) IMK_DEPTH_N(14) IMK_DEPTH_N(15) IMK_DEPTH_N(16)
#undef IMK_DEPTH_N
    }
    IMK_LAUNCH_CHECK();
    return imk_depth_finish(map, batch, hw, mult, img, c, block_in, img_out, im_out, im_size, thr_out, stream);
}

int imk_depth_finish(const float *map, int batch, int hw, float mult, const uint8_t *img, int c, int block_in, uint8_t *img_out,
                     uint8_t *im_out, int64_t *im_size, float *thr_out, hipStream_t stream) {
    IMK_HIP(hipMemsetAsync(im_size, 0, sizeof(int64_t) * batch, stream));
    const bool vec = (hw % 4 == 0) && aligned16(map);
    DepthLeaves lv;
    lv.n = 0;
    if (hw % NP_CHUNK) depth_leaves(0, hw % NP_CHUNK, 0, lv);
    imk_klaunch(depth_thr_kernel, dim3(batch), dim3(1024), 0, stream, map, hw, mult, lv, thr_out);
    IMK_LAUNCH_CHECK();
    const int vec_out = (hw % 16 == 0) && aligned16(im_out);
    const int vec_img = img && ((int64_t)hw * c % 16 == 0) && aligned16(img) && aligned16(img_out);
    const dim3 grid(imk_cdiv(hw, PX_CHUNK), batch);
    auto *ims = reinterpret_cast<unsigned long long *>(im_size);
    if (vec) imk_klaunch(depth_mask_kernel<true>, dim3(grid), dim3(256), 0, stream, map, (const float *)thr_out, hw, img, c, block_in, img_out, im_out, ims, vec_out, vec_img);
    else imk_klaunch(depth_mask_kernel<false>, dim3(grid), dim3(256), 0, stream, map, (const float *)thr_out, hw, img, c, block_in, img_out, im_out, ims, vec_out, vec_img);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

bool imk_depth_head_supported(const ImkDepthHeadArgs &a) {
    if (a.softmax || a.K != 1) return false;
    if (a.n_models < DEPTH_MIN_MODELS || a.n_models > IMK_HEAD_IM_MAX_MODELS) return false;
    if (a.cs != 8 && a.cs != 16 && a.cs != 24 && a.cs != 32) return false;
    return a.hw % 16 == 0 && aligned16(a.map);
}

int imk_launch_depth_head_std(const ImkDepthHeadArgs &a, hipStream_t stream) {
    IMK_CHECK_ARG(a.batch > 0 && a.hw > 0 && a.map);
    if (!imk_depth_head_supported(a)) return IMK_EUNSUPPORTED;
    // N head images (at most 8 x 97 floats), then N x 1024 probabilities: at most 35 KB
    const size_t lds = ((((size_t)a.n_models * (a.K * a.cs + a.K + 2 * a.cs) + 3) & ~(size_t)3) + (size_t)a.n_models * PX_CHUNK) * sizeof(float);
    const dim3 grid(imk_cdiv(a.hw, PX_CHUNK), a.batch);
    ImkProfScope prof(PF_IM, (double)a.batch * a.hw * ((double)a.n_models * a.cs * 2 + 4), stream);
#define IMK_DH(CSV, NV) case NV: imk_klaunch((depth_head_std_kernel<CSV, NV>), dim3(grid), dim3(256), lds, stream, a); break;
#define IMK_DH_N(CSV) switch (a.n_models) { IMK_DH(CSV, 2) IMK_DH(CSV, 3) IMK_DH(CSV, 4) IMK_DH(CSV, 5) IMK_DH(CSV, 6) IMK_DH(CSV, 7) IMK_DH(CSV, 8) }
    switch (a.cs) {
        case 8: IMK_DH_N(8) break;
        case 16: IMK_DH_N(16) break;
        case 24: IMK_DH_N(24) break;
        default: IMK_DH_N(32) break;
    }
#undef IMK_DH_N
#undef IMK_DH
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_eval_depth(const float *probs, const uint8_t *gt, int batch, int h, int w, uint8_t *pred_out, double *sums,
                              void *stream_) {
    IMK_CHECK_ARG(probs && gt && sums && batch > 0 && h > 0 && w > 0);
    IMK_CHECK_ARG((int64_t)h * w < (1ll << 30));
    imk_klaunch(eval_depth_kernel, dim3(batch), dim3(1024), 0, (hipStream_t)stream_, probs, gt, h * w, pred_out, sums);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
