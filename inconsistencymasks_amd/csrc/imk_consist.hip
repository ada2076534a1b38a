// The head of the consistency-loss step (functions.py:367-474 of the reference): L = mean over B*H*W*K of (pA - pB)^2 with pA, pB the
// fp32 outputs of the sigmoid / softmax head on two augmented views of one unlabelled batch, both forwards in training mode (each
// view's last BatchNorm normalises with its own batch statistics), and the gradient of loss_scale * L w.r.t. both views' logits.
//
// Fused route (consistency_head_sigmoid_kernel: sigmoid heads with 1 or 3 maps on 8 or 16 padded channels -- ISIC, HeLa), one pass in
// head_mse_fused_kernel's layout (imk_headf.hip): both last decoder activations read once, each under its own BatchNorm scale / shift,
// the fp32 output layer + sigmoid of imk_head.h, the loss partial, both logit gradients rounded to fp16 (what the composed route
// stores), dy = W . dlogit per view (fp16 weights like the packed dgrad operand, fp32 sums, fp16 result) with each view's
// BatchNorm-backward statistics rows, and ONE set of weight / bias gradient rows for the output layer, summed over both views.
// The wide form of head_mse_fused_kernel lost to its 2 CS + CS K + K + 1 accumulators per thread (215-256 registers at 16 channels);
// two views would double that, so here a pixel belongs to CS / 8 neighbouring lanes, each with 8 channels of both views: one 16-byte
// load and one 16-byte store per view and lane, consecutive lanes on consecutive 16 bytes, and 32 + 9 K + 1 accumulators per thread
// (42 / 60; the compiler's totals: 146 VGPRs for <8,1>, 132 for <16,1>, 173 for <16,3>, 236 for <8,3>, no spills).  The logit's sum
// runs through the lanes of a pixel in head_logit's order (bias, then channels ascending).
//
// Composed route (every shape, softmax heads included): head_kernel's arithmetic stores both fp32 probability stacks, then
// consistency_dlogit_kernel turns them into the two fp16 logit-gradient tensors and the loss partials; the head's dgrad /
// weight-gradient launches of the labelled step follow per view.
//
// No atomics: per-thread fp32 accumulators, lanes by butterfly, waves 0..3 in order -> one partial row per workgroup.
#include "imk_elem.h"
#include "imk_head.h"

namespace {

struct ConsistHeadArgs {
    const f16 *z[2];              // [n_pix][CS] last decoder activation of view A / B (pre-BatchNorm)
    const float *sc[2], *sh[2];   // that view's BatchNorm scale / shift (its own batch statistics) [CS]
    const float *w, *bias;        // output layer: kernel [cin][K] fp32, bias [K]
    int cin;
    long long n_pix;
    const ImkCtl *ctl;
    float *stats;
    f16 *dy[2];                   // [n_pix][CS] gradient w.r.t. each view's BatchNorm output
    float *loss_partial;          // [grid]
    float *dystat_partial[2];     // [grid][2 * CS]: sum dy, sum dy * z per channel and view
    float *wg_partial;            // [grid][2][256]: weight-gradient partials of both views in wgf_stage1's layout
};

template <int CS, int K>
__global__ __launch_bounds__(256) void consistency_head_sigmoid_kernel(ConsistHeadArgs a) {
    constexpr int TPP = CS / 8;                  // lanes per pixel
    constexpr int PPB = 256 / TPP;               // pixels per workgroup and iteration
    constexpr int O_W = 32, O_B = 32 + 8 * K, O_L = O_B + K, NA = O_L + 1;
    // acc: [view][sum dy | sum dy z][8] | dW[8][K] (both views) | db[K] | loss -- the last two on a pixel's first lane only
    __shared__ float s_w[K * CS], s_wd[K * CS], s_b[K], s_sc[2][CS], s_sh[2][CS];
    __shared__ float s_red[4][TPP][NA];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, sub = t & (TPP - 1), c0 = 8 * sub;
    for (int i = t; i < K * CS; i += 256) {
        const int k = i / CS, c = i - k * CS;
        const float w = (c < a.cin) ? a.w[(size_t)c * K + k] : 0.f;
        s_w[i] = w;                              // forward: the fp32 output layer (unet.py:63)
        s_wd[i] = (float)(f16)w;                 // dgrad: the fp16 operand the packed weights hold
    }
    if (t < K) s_b[t] = a.bias[t];
    if (t < 2 * CS) { const int v = t / CS, c = t - v * CS; s_sc[v][c] = a.sc[v][c]; s_sh[v][c] = a.sh[v][c]; }
    const float S = a.ctl->loss_scale;
    if (blockIdx.x == 0 && t == 0) { a.stats[1] = 0.f; a.stats[2] = S; a.stats[3] = (float)a.ctl->step; }   // as head_loss_kernel
    __syncthreads();
    const float inv_n = 1.0f / ((float)a.n_pix * (float)K);
    float acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.f;
    for (long long p = (long long)blockIdx.x * PPB + t / TPP; p < a.n_pix; p += (long long)gridDim.x * PPB) {
        f16x8 zv[2];
#pragma unroll
        for (int v = 0; v < 2; ++v) zv[v] = *reinterpret_cast<const f16x8 *>(a.z[v] + p * CS + c0);
        float xin[2][8], pk[2][K];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xin[v][j] = (float)imk_affine1(zv[v][j], s_sc[v][c0 + j], s_sh[v][c0 + j]);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                // head_logit's sum: the pixel's first lane starts from the bias, the next one continues from its result
                float lg = s_b[k];
#pragma unroll
                for (int j = 0; j < 8; ++j) lg += xin[v][j] * s_w[k * CS + c0 + j];
                if constexpr (TPP == 2) {
                    float l1 = __shfl_xor(lg, 1, 64);        // on the second lane: the first lane's bias + channels 0..7
#pragma unroll
                    for (int j = 0; j < 8; ++j) l1 += xin[v][j] * s_w[k * CS + c0 + j];
                    const float back = __shfl_xor(l1, 1, 64);
                    lg = sub ? l1 : back;
                }
                pk[v][k] = head_sigmoid(lg);
            }
        }
        float gk[2][K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float e = pk[0][k] - pk[1][k], g = S * 2.0f * e * inv_n;
            gk[0][k] = (float)(f16)(g * pk[0][k] * (1.0f - pk[0][k]));
            gk[1][k] = (float)(f16)(-g * pk[1][k] * (1.0f - pk[1][k]));
            if (sub == 0) {
                acc[O_L] += e * e;
                acc[O_B + k] += gk[0][k] + gk[1][k];
            }
        }
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            f16x8 dv;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float d = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    d += gk[v][k] * s_wd[k * CS + c0 + j];
                    acc[O_W + j * K + k] += xin[v][j] * gk[v][k];
                }
                const f16 d16 = (f16)d;
                dv[j] = d16;
                acc[v * 16 + j] += (float)d16;
                acc[v * 16 + 8 + j] += (float)d16 * (float)zv[v][j];
            }
            *reinterpret_cast<f16x8 *>(a.dy[v] + p * CS + c0) = dv;
        }
    }
    // ---- per-workgroup partial rows, fixed order: the lanes that hold the same channels (butterfly), then waves 0..3 ------------
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        float v = acc[i];
#pragma unroll
        for (int o = 32; o >= TPP; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane < TPP) s_red[wave][lane][i] = v;
    }
    __syncthreads();
    auto tot = [&](int s, int i) { return (s_red[0][s][i] + s_red[1][s][i]) + (s_red[2][s][i] + s_red[3][s][i]); };
    if (t < 4 * CS) {             // rows of the statistics are [2][CS] per view
        const int v = t / (2 * CS), r = t - v * 2 * CS, which = r / CS, c = r - which * CS;
        a.dystat_partial[v][(size_t)blockIdx.x * 2 * CS + r] = tot(c >> 3, v * 16 + which * 8 + (c & 7));
    }
    if (t == 0) a.loss_partial[blockIdx.x] = tot(0, O_L);
    // weight-gradient partial row [tap 0 | bias][256] in wgf_stage1's layout: element e = r * 64 + l holds (ci = 4 (l >> 4) + r,
    // co = l & 15); the bias row keeps co in elements 0..15
    float *wp = a.wg_partial + (size_t)blockIdx.x * 2 * 256;
    {
        const int r = t >> 6, l = t & 63, ci = 4 * (l >> 4) + r, co = l & 15;
        wp[t] = (ci < CS && co < K) ? tot(ci >> 3, O_W + (ci & 7) * K + co) : 0.f;
        wp[256 + t] = (t < K) ? tot(0, O_B + t) : 0.f;
    }
}

// Composed route: both fp32 probability stacks [n_pix][K] -> both fp16 logit gradients [n_pix][cs_out] (channels beyond K zero) and
// the loss partials.  sigmoid: dlogitA = g pA (1 - pA), dlogitB = -g pB (1 - pB) with g = S 2 (pA - pB) / (n_pix K); softmax, with
// g_k = 2 (pA_k - pB_k) / (n_pix K): dlogitA_k = S pA_k (g_k - sum_j g_j pA_j), dlogitB_k = S pB_k (-g_k + sum_j g_j pB_j).
__global__ __launch_bounds__(256) void consistency_dlogit_kernel(const float *__restrict__ pA, const float *__restrict__ pB, int K,
                                                                 int softmax, long long n_pix, const ImkCtl *__restrict__ ctl,
                                                                 float *__restrict__ stats, int cs_out, f16 *__restrict__ dlA,
                                                                 f16 *__restrict__ dlB, float *__restrict__ loss_partial) {
    const float S = ctl->loss_scale;
    if (blockIdx.x == 0 && threadIdx.x == 0) { stats[1] = 0.f; stats[2] = S; stats[3] = (float)ctl->step; }   // as head_loss_kernel
    const float inv_n = 1.0f / ((float)n_pix * (float)K);
    float l = 0.f;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n_pix; p += (long long)gridDim.x * 256) {
        const float *a = pA + p * K, *b = pB + p * K;
        float dotA = 0.f, dotB = 0.f;
        if (softmax)
            for (int k = 0; k < K; ++k) {
                const float g = 2.0f * (a[k] - b[k]) * inv_n;
                dotA += g * a[k];
                dotB += g * b[k];
            }
        for (int k0 = 0; k0 < cs_out; k0 += 8) {
            f16x8 ga = {0, 0, 0, 0, 0, 0, 0, 0}, gb = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + j;
                if (k < K) {
                    const float e = a[k] - b[k];
                    l += e * e;
                    if (softmax) {
                        const float g = 2.0f * e * inv_n;
                        ga[j] = (f16)(S * a[k] * (g - dotA));
                        gb[j] = (f16)(S * b[k] * (dotB - g));
                    } else {
                        const float g = S * 2.0f * e * inv_n;
                        ga[j] = (f16)(g * a[k] * (1.0f - a[k]));
                        gb[j] = (f16)(-g * b[k] * (1.0f - b[k]));
                    }
                }
            }
            *reinterpret_cast<f16x8 *>(dlA + p * cs_out + k0) = ga;
            *reinterpret_cast<f16x8 *>(dlB + p * cs_out + k0) = gb;
        }
    }
    __shared__ float s_l[4];
    l = wave_sum<64>(l);
    if ((threadIdx.x & 63) == 0) s_l[threadIdx.x >> 6] = l;
    __syncthreads();
    if (threadIdx.x == 0) loss_partial[blockIdx.x] = (s_l[0] + s_l[1]) + (s_l[2] + s_l[3]);
}

// g += g2, element by element (one fixed order: bit-reproducible); a non-finite sum raises the step's overflow flag
__global__ __launch_bounds__(256) void grad_add_kernel(float *__restrict__ g, const float *__restrict__ g2, long long n,
                                                       float *__restrict__ found_inf) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = g[i] + g2[i];
        g[i] = v;
        bad = bad || !__builtin_isfinite(v);
    }
    if (bad) *found_inf = 1.0f;
}

}  // namespace

// Sigmoid heads with 1 or 3 maps on 8 or 16 padded channels.  `rows_cap`: capacity (rows) of each view's dystat_partial.
bool imk_consistency_fused_ok(int cs, int K, int softmax, long long n_pix, int rows_cap) {
    if (softmax || (cs != 8 && cs != 16) || (K != 1 && K != 3)) return false;
    return imk_loss_blocks(n_pix) <= rows_cap;
}

int imk_launch_consistency_head(const f16 *zA, const f16 *zB, const float *scA, const float *shA, const float *scB,
                                const float *shB, const float *w, const float *bias, int cin, int cs, int K, long long n_pix,
                                const ImkCtl *ctl, float *stats, f16 *dyA, f16 *dyB, float *loss_partial, float *dystatA,
                                float *dystatB, float *wg_partial, hipStream_t stream) {
    ConsistHeadArgs a{{zA, zB}, {scA, scB}, {shA, shB}, w, bias, cin, n_pix, ctl, stats, {dyA, dyB}, loss_partial,
                      {dystatA, dystatB}, wg_partial};
    const int grid = imk_loss_blocks(n_pix);
    ImkProfScope prof(PF_HEAD_LOSS, (double)n_pix * 4 * cs * 2, stream, 2 * 6.0 * n_pix * cin * K);
    if (cs == 8 && K == 1) imk_klaunch(consistency_head_sigmoid_kernel<8, 1>, dim3(grid), dim3(256), 0, stream, a);
    else if (cs == 8 && K == 3) imk_klaunch(consistency_head_sigmoid_kernel<8, 3>, dim3(grid), dim3(256), 0, stream, a);
    else if (cs == 16 && K == 1) imk_klaunch(consistency_head_sigmoid_kernel<16, 1>, dim3(grid), dim3(256), 0, stream, a);
    else if (cs == 16 && K == 3) imk_klaunch(consistency_head_sigmoid_kernel<16, 3>, dim3(grid), dim3(256), 0, stream, a);
    else return IMK_EUNSUPPORTED;
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

int imk_launch_consistency_dlogit(const float *pA, const float *pB, int K, int softmax, long long n_pix, const ImkCtl *ctl,
                                  float *stats, f16 *dlogitA, f16 *dlogitB, float *loss_partial, hipStream_t stream) {
    if (K > 64) return IMK_EUNSUPPORTED;
    const int cs_out = imk_pad8(K);
    ImkProfScope prof(PF_HEAD_LOSS, (double)n_pix * (2 * K * 4 + 2 * cs_out * 2), stream);
    imk_klaunch(consistency_dlogit_kernel, dim3(imk_loss_blocks(n_pix)), dim3(256), 0, stream, pA, pB, K, softmax, n_pix, ctl,
                stats, cs_out, dlogitA, dlogitB, loss_partial);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

int imk_launch_grad_add(float *g, const float *g2, long long n, float *found_inf, hipStream_t stream) {
    if (n <= 0) return IMK_OK;
    const long long nb = (n + 255) / 256;
    ImkProfScope prof(PF_STEP_TAIL, (double)n * 12, stream);
    imk_klaunch(grad_add_kernel, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(256), 0, stream, g, g2, n, found_inf);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
