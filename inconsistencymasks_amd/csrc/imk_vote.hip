// Model-ensemble voting for gfx950 (MI355X): the pseudo-label rules of the reference's model-ensemble baseline
// (get_model_ensemble_prediction_*, functions.py:2409-2566), which the IM kernels do not compute.
//   binary, hard      255 where every model has p > thr                              (ISIC, functions.py:2409-2435)
//   binary, soft      255 where (sum_n (double)p_n) / N > thr (fp64), summed in model order (HeLa, functions.py:2474-2528)
//   multiclass, hard  the label where all N arg-maxes agree, else 0                  (functions.py:2438-2469)
//   multiclass, soft  argmax_k of fl32(fl32(p_0k + p_1k) + ...) / N, divide correctly rounded (SUIM / Cityscapes,
//                     functions.py:2534-2566: np.mean(axis=0) of the float32 stack is exactly this)
// Arg-maxes follow np.argmax: the first maximum wins, and a NaN counts as the maximum (the first NaN wins).
//
// imk_vote_binary / imk_vote_multiclass read the fp32 probability stack (one thread per pixel: the duck-typed-model path and the
// route of imk_unet_forward_vote).  vote_head_sigmoid_kernel (ISIC, HeLa) and vote_head_softmax_kernel (SUIM, Cityscapes) read only
// the N last decoder activations and evaluate every model's output layer with the code of imk_unet_forward's head (imk_head.h), so
// the fused result is bit-identical to imk_unet_forward + imk_vote_*, and only the uint8 labels are written.
#include "imk_common.h"
#include "imk_head.h"

namespace {

// ---- unfused: probability stack -> labels ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vote_binary_kernel(const float *__restrict__ preds, int n_models, long long n_pix, int hw,
                                                          int kb, double thr, int soft, uint8_t *__restrict__ masks_out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pix) return;
    const long long b = p / hw, q = p - b * hw;
    for (int k = 0; k < kb; ++k) {
        bool on;
        if (soft) {
            double s = 0.0;
            for (int n = 0; n < n_models; ++n) s += (double)preds[((size_t)n * n_pix + p) * kb + k];
            on = s / (double)n_models > thr;                  // NaN compares false
        } else {
            int votes = 0;
            for (int n = 0; n < n_models; ++n) votes += preds[((size_t)n * n_pix + p) * kb + k] > (float)thr ? 1 : 0;
            on = votes == n_models;
        }
        masks_out[((size_t)b * kb + k) * hw + q] = on ? 255 : 0;
    }
}

__global__ __launch_bounds__(256) void vote_multi_kernel(const float *__restrict__ probs, int n_models, long long n_pix, int K,
                                                         int soft, uint8_t *__restrict__ final_out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pix) return;
    int label = 0;
    if (soft) {
        const float fn = (float)n_models;
        float bv = 0.f;
        int bk = -1;
        for (int k = 0; k < K; ++k) {
            float s = probs[(size_t)p * K + k];
            for (int n = 1; n < n_models; ++n) s += probs[((size_t)n * n_pix + p) * K + k];
            np_argmax_step(__fdiv_rn(s, fn), k, bv, bk);
        }
        label = bk;
    } else {
        bool agree = true;
        for (int n = 0; n < n_models; ++n) {
            float bv = 0.f;
            int bk = -1;
            for (int k = 0; k < K; ++k) np_argmax_step(probs[((size_t)n * n_pix + p) * K + k], k, bv, bk);
            if (n == 0) label = bk; else agree = agree && bk == label;
        }
        if (!agree) label = 0;
    }
    final_out[p] = (uint8_t)label;
}

// ---- fused: last decoder activations -> labels ------------------------------------------------------------------------------
constexpr int VOTE_BIN_CHUNK = 1024;    // sigmoid heads: pixels per workgroup (4 per thread), never straddling two images

// LDS -> global as 16-byte stores: n is a multiple of 16 and dst 16-byte aligned (imk_vote_head_supported: hw % 16 == 0, aligned out)
__device__ __forceinline__ void vote_store(uint8_t *__restrict__ dst, const uint8_t *s, int n) {
    for (int i = threadIdx.x; i < n / 16; i += 256) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(s)[i];
}

// a + b rounded on its own: HeadMfma::probs ends in p = e * inv, and with contraction on (the HIP default) `acc + e * inv` may become
// one FMA that never rounds p -- not the sum of the probabilities imk_unet_forward stores
__device__ __forceinline__ float add_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// Sigmoid heads (K <= 4): the N models' head images in LDS (imk_head.h), 4 consecutive pixels per thread; the probability of
// model n is head_sigmoid(head_logit) -- head_kernel's and head_im_sigmoid_kernel's expression -- and goes into a vote count
// (hard) or an fp64 sum (soft) in registers.  grid (ceil(HW / 1024), B); masks [B,K,H,W].
template <int CS, int KB, bool SOFT>
__global__ __launch_bounds__(256) void vote_head_sigmoid_kernel(ImkVoteHeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[KB][VOTE_BIN_CHUNK];
    const int K = a.K, hw = a.hw, n_models = a.n_models;
    const int per_model = head_lds_floats<CS>(K);
    const int b = blockIdx.y, t = threadIdx.x;
    const int p_base = blockIdx.x * VOTE_BIN_CHUNK;
    const int n_px = min(VOTE_BIN_CHUNK, hw - p_base);
    for (int n = 0; n < n_models; ++n) head_stage<CS>(a.w[n], a.bias[n], a.sc[n], a.sh[n], a.cin, K, s_dyn + n * per_model);
    __syncthreads();
    const int p0 = 4 * t;                                       // hw % 16 == 0: a thread's 4 pixels are all in or all out
    if (p0 < n_px) {
        const long long p = (long long)b * hw + p_base + p0;
        double sum[4][KB];
        int votes[4][KB];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < KB; ++k) { sum[j][k] = 0.0; votes[j][k] = 0; }
        for (int n = 0; n < n_models; ++n) {
            const float *hn = s_dyn + n * per_model;
            f16x8 r[4][CS / 8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < CS / 8; ++q) r[j][q] = *reinterpret_cast<const f16x8 *>(a.z[n] + (p + j) * CS + q * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float xin[CS];
                head_input_regs<CS>(r[j], hn, K, xin);
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    const float v = head_sigmoid(head_logit<CS>(xin, hn, K, k));
                    if constexpr (SOFT) sum[j][k] += (double)v;
                    else votes[j][k] += v > (float)a.thr ? 1 : 0;         // NaN compares false
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            uint32_t o = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool on = SOFT ? (sum[j][k] / (double)n_models > a.thr) : (votes[j][k] == n_models);
                if (on) o |= 0xffu << (8 * j);
            }
            *reinterpret_cast<uint32_t *>(&s_out[k][p0]) = o;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KB; ++k) vote_store(a.out + ((size_t)b * KB + k) * hw + p_base, s_out[k], n_px);
}

// Softmax heads (K <= 64): HeadMfma::probs -- the code of imk_unet_forward's softmax head (head_softmax_kernel) -- gives every group
// of 4 lanes the K probabilities of one pixel.  A wave owns U units of 16 pixels and walks the models in order: one fragment build
// per model and wave serves U units.  Hard: the label / agreement per unit stay in registers.  Soft: each lane keeps the running sums
// of its own classes ((p_0 + p_1) + p_2) + ..., each add rounded on its own) in a wave-private LDS slab [U*16 pixels][16*KT classes],
// read and written as f32x4 by the lane that owns them, then divides by N (correctly rounded).  A register-resident form of the sums
// (KT f32x4 per unit held across the model loop) gave arg-maxes that differed from the same kernel's per-model arg-max even at N = 1,
// for every class count tried, and was replaced by the slab.  The arg-max is np.argmax's over the 4 lanes of a pixel.  Labels leave
// through LDS as 16-byte stores; flat over the B*H*W pixels.
template <int KT>
struct VoteUnits { static constexpr int U = KT == 1 ? 8 : (KT == 4 ? 4 : 5); };

template <int KT, bool SOFT>
__host__ __device__ constexpr size_t vote_softmax_lds() {
    return (SOFT ? (size_t)4 * VoteUnits<KT>::U * 16 * 16 * KT * sizeof(float) : 0) + (size_t)4 * VoteUnits<KT>::U * 16;
}

template <int KT, bool SOFT>
__global__ __launch_bounds__(256) void vote_head_softmax_kernel(ImkVoteHeadArgs a, long long n_pix) {
    constexpr int U = VoteUnits<KT>::U, CHUNK = 4 * U * 16, KP = 16 * KT;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int K = a.K, cs = a.cs, n_models = a.n_models;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, p16 = lane & 15, g = lane >> 4;
    f32x4 *s_acc = reinterpret_cast<f32x4 *>(smem) + (size_t)wave * U * 16 * KT * 4;     // [U*16][KP] floats of this wave
    uint8_t *s_out = smem + (SOFT ? (size_t)4 * U * 16 * KP * sizeof(float) : 0);
    const long long p_base = (long long)blockIdx.x * CHUNK;
    const int n_px = (int)(n_pix - p_base < CHUNK ? n_pix - p_base : CHUNK);     // a multiple of 16
    int label[U];
    bool agree[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { label[u] = 0; agree[u] = true; }
    // the lane's f32x4 of class tile kt, unit u: classes 16 kt + 4 g .. + 3 of pixel u * 16 + p16
    auto slot = [&](int u, int kt) { return s_acc + ((u * 16 + p16) * KP + 16 * kt + 4 * g) / 4; };
    for (int n = 0; n < n_models; ++n) {
        HeadMfma<KT> h;
        h.load(a.w[n], a.bias[n], a.sc[n], a.sh[n], a.cin, cs, K);
        f16x8 zr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = (wave * U + u) * 16 + p16;
            zr[u] = h.load_z(a.z[n], p_base + (q < n_px ? q : 0), cs);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            f32x4 pr[KT];
            h.probs(zr[u], K, pr);
            if constexpr (SOFT) {
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    f32x4 s = pr[kt];                                      // np.add.reduce: the first model's row, then + in order
                    if (n > 0) {
                        const f32x4 o = *slot(u, kt);
#pragma unroll
                        for (int r = 0; r < 4; ++r) s[r] = add_rounded(o[r], pr[kt][r]);
                    }
                    *slot(u, kt) = s;
                }
            } else {
                const int bk = vote_argmax<KT>(pr, K);
                if (n == 0) label[u] = bk; else agree[u] = agree[u] && bk == label[u];
            }
        }
    }
    if constexpr (SOFT) {
        const float fn = (float)n_models;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            f32x4 m[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                m[kt] = *slot(u, kt);
#pragma unroll
                for (int r = 0; r < 4; ++r) m[kt][r] = m[kt][r] / fn;      // correctly rounded (v_div_scale / fmas / fixup)
            }
            label[u] = vote_argmax<KT>(m, K);
        }
    }
    if (g == 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = (wave * U + u) * 16 + p16;
            if (q < n_px) s_out[q] = (uint8_t)((SOFT || agree[u]) ? label[u] : 0);
        }
    }
    __syncthreads();
    vote_store(a.out + p_base, s_out, n_px);
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

static size_t vote_head_lds(const ImkVoteHeadArgs &a) {
    if (a.softmax) return 0;      // weights live in registers (HeadMfma)
    return (size_t)a.n_models * (a.K * a.cs + a.K + 2 * a.cs) * sizeof(float);
}

bool imk_vote_head_supported(const ImkVoteHeadArgs &a) {
    if (a.n_models < 1 || a.n_models > IMK_HEAD_IM_MAX_MODELS) return false;
    if (a.softmax ? a.K > 64 : a.K > 4) return false;
    if (a.cs != 8 && a.cs != 16 && a.cs != 24 && a.cs != 32) return false;
    if (a.hw % 16 != 0 || !aligned16(a.out)) return false;
    return vote_head_lds(a) <= 150 * 1024;
}

int imk_launch_vote_head(const ImkVoteHeadArgs &a, hipStream_t stream) {
    IMK_CHECK_ARG(a.n_models > 0 && a.batch > 0 && a.hw > 0 && a.K > 0 && a.out && (a.mode == IMK_VOTE_HARD || a.mode == IMK_VOTE_SOFT));
    if (!imk_vote_head_supported(a)) return IMK_EUNSUPPORTED;
    const bool soft = a.mode == IMK_VOTE_SOFT;
    const long long n_pix = (long long)a.batch * a.hw;
    const int nf = a.softmax ? 1 : a.K;
    // algorithmic bytes: N last activations read, the label map(s) written; flops: the N output layers (2 cin K) + the vote
    ImkProfScope prof(PF_IM, (double)n_pix * ((double)a.n_models * a.cs * 2 + nf), stream,
                      (double)n_pix * a.n_models * a.K * (2.0 * a.cin + 1.0));
    if (a.softmax) {
        const int kt = (a.K + 15) / 16;
#define IMK_VS(KT)                                                                                                          \
        do {                                                                                                                \
            constexpr int CHUNK = 4 * VoteUnits<KT>::U * 16;                                                                \
            const dim3 grid((unsigned)((n_pix + CHUNK - 1) / CHUNK));                                                       \
            if (soft) {                                                                                                     \
                constexpr size_t lds = vote_softmax_lds<KT, true>();                                                        \
                if (lds > 64 * 1024)                                                                                        \
                    IMK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(vote_head_softmax_kernel<KT, true>),         \
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                     \
                imk_klaunch(vote_head_softmax_kernel<KT, true>, grid, dim3(256), lds, stream, a, n_pix);                    \
            } else {                                                                                                        \
                imk_klaunch(vote_head_softmax_kernel<KT, false>, grid, dim3(256), vote_softmax_lds<KT, false>(), stream, a, n_pix); \
            }                                                                                                               \
        } while (0)
        switch (kt) {
            case 1: IMK_VS(1); break;
            case 2: IMK_VS(2); break;
            case 3: IMK_VS(3); break;
            default: IMK_VS(4); break;
        }
#undef IMK_VS
    } else {
        const size_t lds = vote_head_lds(a);
        const dim3 grid(imk_cdiv(a.hw, VOTE_BIN_CHUNK), a.batch);
#define IMK_VB_LAUNCH(KERN)                                                                                                 \
        do {                                                                                                                \
            if (lds > 64 * 1024)                                                                                            \
                IMK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
            imk_klaunch(KERN, grid, dim3(256), lds, stream, a);                                                             \
        } while (0)
#define IMK_VB(CSV, KBV) do { if (soft) IMK_VB_LAUNCH((vote_head_sigmoid_kernel<CSV, KBV, true>)); else IMK_VB_LAUNCH((vote_head_sigmoid_kernel<CSV, KBV, false>)); } while (0)
#define IMK_VB_KB(CSV)                                                                                                      \
        switch (a.K) {                                                                                                      \
            case 1: IMK_VB(CSV, 1); break;                                                                                  \
            case 2: IMK_VB(CSV, 2); break;                                                                                  \
            case 3: IMK_VB(CSV, 3); break;                                                                                  \
            default: IMK_VB(CSV, 4); break;                                                                                 \
        }
        switch (a.cs) {
            case 8: IMK_VB_KB(8); break;
            case 16: IMK_VB_KB(16); break;
            case 24: IMK_VB_KB(24); break;
            default: IMK_VB_KB(32); break;
        }
#undef IMK_VB_KB
#undef IMK_VB
#undef IMK_VB_LAUNCH
    }
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_vote_binary(const float *preds, int n_models, int batch, int h, int w, int kb, double thr, int mode,
                               uint8_t *masks_out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    IMK_CHECK_ARG(preds && masks_out && n_models > 0 && batch > 0 && h > 0 && w > 0 && kb > 0);
    IMK_CHECK_ARG(mode == IMK_VOTE_HARD || mode == IMK_VOTE_SOFT);
    const int64_t hw64 = (int64_t)h * w;
    IMK_CHECK_ARG(hw64 < (1ll << 30));
    const long long n_pix = (long long)batch * hw64;
    ImkProfScope prof(PF_IM, (double)n_pix * ((double)n_models * kb * 4 + kb), stream, (double)n_pix * n_models * kb);
    imk_klaunch(vote_binary_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, stream, preds, n_models, n_pix, (int)hw64, kb,
                thr, mode, masks_out);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_vote_multiclass(const float *probs, int n_models, int batch, int h, int w, int k, int mode, uint8_t *final_out,
                                   void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    IMK_CHECK_ARG(probs && final_out && n_models > 0 && batch > 0 && h > 0 && w > 0 && k > 0);
    IMK_CHECK_ARG(mode == IMK_VOTE_HARD || mode == IMK_VOTE_SOFT);
    if (k > 64) return IMK_EUNSUPPORTED;
    const int64_t hw64 = (int64_t)h * w;
    IMK_CHECK_ARG(hw64 < (1ll << 30));
    const long long n_pix = (long long)batch * hw64;
    ImkProfScope prof(PF_IM, (double)n_pix * ((double)n_models * k * 4 + 1), stream, (double)n_pix * n_models * k);
    imk_klaunch(vote_multi_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, stream, probs, n_models, n_pix, k, mode,
                final_out);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
