// Loss kind 4 of imk_unet_fwd_bwd: the reference's dice_loss (functions.py:162-184, smooth = 1) on sigmoid heads, and the
// validation monitor imk_eval_dice_sums.
//   I_b = sum t p    U_b = sum t + sum p    dice_b = (2 I_b + 1) / (U_b + 1)    over the H W K elements of image b, t = float(y)
//   L = 1 - mean_b dice_b
//   dL/dp = c0_b - c1_b t      c0_b = (2 I_b + 1) / (B (U_b + 1)^2)      c1_b = 2 / (B (U_b + 1))
//   dlogit = fp16(S (c0_b - c1_b t) p (1 - p))
// A pixel's gradient depends on two reductions over its whole image, so the head runs in three launches on the step's stream (the
// depth-map IM's pattern: a reduction launch between two streaming launches):
//   1. dice_sums_kernel    grid (workgroups per image, image): probabilities recomputed from the last decoder activation under its
//                          BatchNorm with imk_head.h's code (head_loss_kernel's arithmetic in its order), sum t p, sum t, sum p per
//                          thread in fp32, lanes (butterfly) then waves 0..3 -> one partial row per workgroup.  cs 2 + K bytes read
//                          per pixel.  First kernel of the step's gradient part: it sets stats[1..3] as head_loss_kernel does.
//   2. dice_coef_kernel    one workgroup: a wave per image adds that image's rows in double (lanes stride the rows, butterfly), forms
//                          dice_b, c0_b, c1_b in double and rounds them once; thread 0 then sums dice_b in index order -> stats[0].
//                          (imk_launch_loss_finalize is not launched for kind 4.)
//   3. the gradient pass   probabilities recomputed again (no fp32 probability tensor): dice_dlogit_kernel writes the fp16 logit
//                          gradient in head_loss_kernel's layout for the head's dgrad (every sigmoid shape); 8 channels and 1 map
//                          take head_mse_fused_kernel<8, 1, false, true> (imk_headf.hip) instead, IMK_DICE_FUSED=0 forces the former.
// No float atomics anywhere: bit-reproducible.
#include "imk_elem.h"
#include "imk_head.h"

namespace {

template <int CS>
__global__ __launch_bounds__(256) void dice_sums_kernel(const f16 *__restrict__ z, const float *__restrict__ sc,
                                                        const float *__restrict__ sh, const float *__restrict__ w,
                                                        const float *__restrict__ bias, int cin, int K, int hw,
                                                        const uint8_t *__restrict__ y, const ImkCtl *__restrict__ ctl,
                                                        float *__restrict__ stats, float *__restrict__ partial /*[B][gridDim.x][3]*/) {
    extern __shared__ float s_w[];   // head_stage's image: w^T [K][CS], bias [K], scale [CS], shift [CS]
    __shared__ float s_red[4][3];
    head_stage<CS>(w, bias, sc, sh, cin, K, s_w);
    // start of the step's gradient part, as head_loss_kernel
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { stats[1] = 0.f; stats[2] = ctl->loss_scale; stats[3] = (float)ctl->step; }
    __syncthreads();
    const long long base = (long long)blockIdx.y * hw;       // this workgroup's image: it never reads another one's pixels
    float a_tp = 0.f, a_t = 0.f, a_p = 0.f;
    auto pixel = [&](const f16x8 (&zv)[CS / 8], long long p) {
        float xin[CS];
        head_input_regs<CS>(zv, s_w, K, xin);
        for (int k = 0; k < K; ++k) {
            const float t = (float)y[p * K + k];
            const float pk = head_sigmoid(head_logit<CS>(xin, s_w, K, k));
            a_tp += t * pk; a_t += t; a_p += pk;
        }
    };
    // NP pixels per iteration with all their activation loads issued first (head_mse_fused_kernel's scheme)
    constexpr int NP = 4;
    const int stride = gridDim.x * 256;
    int q = blockIdx.x * 256 + threadIdx.x;
    for (; q + (NP - 1) * stride < hw; q += NP * stride) {
        f16x8 zz[NP][CS / 8];
#pragma unroll
        for (int u = 0; u < NP; ++u)
#pragma unroll
            for (int v = 0; v < CS / 8; ++v) zz[u][v] = *reinterpret_cast<const f16x8 *>(z + (base + q + u * stride) * CS + v * 8);
#pragma unroll
        for (int u = 0; u < NP; ++u) pixel(zz[u], base + q + u * stride);
    }
    for (; q < hw; q += stride) {
        f16x8 z0[CS / 8];
#pragma unroll
        for (int v = 0; v < CS / 8; ++v) z0[v] = *reinterpret_cast<const f16x8 *>(z + (base + q) * CS + v * 8);
        pixel(z0, base + q);
    }
    // fixed order: lanes (butterfly), then waves 0..3
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a_tp = wave_sum<64>(a_tp); a_t = wave_sum<64>(a_t); a_p = wave_sum<64>(a_p);
    if (lane == 0) { s_red[wave][0] = a_tp; s_red[wave][1] = a_t; s_red[wave][2] = a_p; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int i = threadIdx.x;
        partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + i] = (s_red[0][i] + s_red[1][i]) + (s_red[2][i] + s_red[3][i]);
    }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void dice_coef_kernel(const float *__restrict__ partial, int rows, int batch,
                                                        float *__restrict__ coef /*[B][2]*/, double *__restrict__ dice /*[B]*/,
                                                        float *__restrict__ stats) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = wave; b < batch; b += 4) {
        double s[3] = {0, 0, 0};
        for (int r = lane; r < rows; r += 64)
#pragma unroll
            for (int i = 0; i < 3; ++i) s[i] += (double)partial[((size_t)b * rows + r) * 3 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] = wave_sum_d(s[i]);
        if (lane == 0) {
            const double num = 2.0 * s[0] + 1.0, den = (s[1] + s[2]) + 1.0;
            dice[b] = num / den;
            coef[2 * b] = (float)(num / ((double)batch * den * den));
            coef[2 * b + 1] = (float)(2.0 / ((double)batch * den));
        }
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0;
        for (int b = 0; b < batch; ++b) tot += dice[b];      // images in index order
        stats[0] = (float)(1.0 - tot / (double)batch);
    }
}

// head_loss_kernel's scheme (sigmoid branch) with the Dice gradient: the fp16 logit gradient [n_pix][cs_out] for the head's dgrad
template <int CS>
__global__ __launch_bounds__(256) void dice_dlogit_kernel(const f16 *__restrict__ z, const float *__restrict__ sc,
                                                          const float *__restrict__ sh, const float *__restrict__ w,
                                                          const float *__restrict__ bias, int cin, int K, long long n_pix, int hw,
                                                          const uint8_t *__restrict__ y, const ImkCtl *__restrict__ ctl,
                                                          const float *__restrict__ coef, int cs_out, f16 *__restrict__ dlogit) {
    extern __shared__ float s_w[];
    head_stage<CS>(w, bias, sc, sh, cin, K, s_w);
    __syncthreads();
    const float S = ctl->loss_scale;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n_pix; p += (long long)gridDim.x * 256) {
        float xin[CS];
        head_input<CS>(z, p, s_w, K, xin);
        const int b = dice_image(p, hw);
        const float c0 = coef[2 * b], c1 = coef[2 * b + 1];
        f16 *d = dlogit + p * cs_out;
        for (int k0 = 0; k0 < cs_out; k0 += 8) {
            f16x8 g8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + j;
                if (k < K) {
                    const float t = (float)y[p * K + k];
                    const float pk = head_sigmoid(head_logit<CS>(xin, s_w, K, k));
                    g8[j] = (f16)dice_dlogit(S, c0, c1, t, pk);
                }
            }
            *reinterpret_cast<f16x8 *>(d + k0) = g8;
        }
    }
}

// One workgroup per image; a thread owns the elements t, t + 256, ... of the image's H W K and adds them in that order in double
// (u8 x fp32 products are exact there), then the 256 threads' sums go through one fixed tree: the result of an image depends on
// its own elements and their count alone.
__global__ __launch_bounds__(256) void eval_dice_sums_kernel(const float *__restrict__ probs, const uint8_t *__restrict__ gt,
                                                             long long n /* H W K */, double *__restrict__ out /*[B][3]*/) {
    __shared__ double s_r[3][256];
    const float *p = probs + (size_t)blockIdx.x * n;
    const uint8_t *g = gt + (size_t)blockIdx.x * n;
    double a_tp = 0, a_t = 0, a_p = 0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const double t = (double)g[i], v = (double)p[i];
        a_tp += t * v; a_t += t; a_p += v;
    }
    s_r[0][threadIdx.x] = a_tp; s_r[1][threadIdx.x] = a_t; s_r[2][threadIdx.x] = a_p;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
#pragma unroll
            for (int i = 0; i < 3; ++i) s_r[i][threadIdx.x] += s_r[i][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x < 3) out[(size_t)blockIdx.x * 3 + threadIdx.x] = s_r[threadIdx.x][0];
}

size_t head_lds_bytes(int cs, int K) { return ((size_t)K * cs + K + 2 * cs) * sizeof(float); }

}  // namespace

// workgroups per image of the sums launch = partial rows per image: at most ~1024 workgroups over the batch
int imk_dice_rows(int batch, int hw) {
    int cap = 1024 / batch;
    if (cap < 1) cap = 1;
    const int per = (hw + 255) / 256;
    return per < cap ? per : cap;
}

int imk_launch_dice_sums(const f16 *z, const float *sc, const float *sh, const float *w, const float *bias, int cin, int cs, int K,
                         int batch, int hw, const uint8_t *y, const ImkCtl *ctl, float *stats, float *partial, hipStream_t stream) {
    if (K > 64) return IMK_EUNSUPPORTED;
    const dim3 grid(imk_dice_rows(batch, hw), batch);
    const size_t lds = head_lds_bytes(cs, K);
    ImkProfScope prof(PF_HEAD_LOSS, (double)batch * hw * (cs * 2 + K), stream);
#define IMK_DS(CS) imk_klaunch(dice_sums_kernel<CS>, grid, dim3(256), lds, stream, z, sc, sh, w, bias, cin, K, hw, y, ctl, stats, partial)
    switch (cs) {
        case 8: IMK_DS(8); break;
        case 16: IMK_DS(16); break;
        case 24: IMK_DS(24); break;
        case 32: IMK_DS(32); break;
        default: return IMK_EUNSUPPORTED;
    }
#undef IMK_DS
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

int imk_launch_dice_coef(const float *partial, int batch, int hw, float *coef, double *dice, float *stats, hipStream_t stream) {
    const int rows = imk_dice_rows(batch, hw);
    ImkProfScope prof(PF_STEP_TAIL, (double)batch * rows * 12, stream);
    imk_klaunch(dice_coef_kernel, dim3(1), dim3(256), 0, stream, partial, rows, batch, coef, dice, stats);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

int imk_launch_dice_dlogit(const f16 *z, const float *sc, const float *sh, const float *w, const float *bias, int cin, int cs, int K,
                           long long n_pix, int hw, const uint8_t *y, const ImkCtl *ctl, const float *coef, f16 *dlogit,
                           hipStream_t stream) {
    if (K > 64) return IMK_EUNSUPPORTED;
    const int nb = imk_loss_blocks(n_pix), cs_out = imk_pad8(K);
    const size_t lds = head_lds_bytes(cs, K);
    ImkProfScope prof(PF_HEAD_LOSS, (double)n_pix * (cs * 2 + K + cs_out * 2), stream);
#define IMK_DD(CS) imk_klaunch(dice_dlogit_kernel<CS>, dim3(nb), dim3(256), lds, stream, z, sc, sh, w, bias, cin, K, n_pix, hw, y, ctl, coef, cs_out, dlogit)
    switch (cs) {
        case 8: IMK_DD(8); break;
        case 16: IMK_DD(16); break;
        case 24: IMK_DD(24); break;
        case 32: IMK_DD(32); break;
        default: return IMK_EUNSUPPORTED;
    }
#undef IMK_DD
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_eval_dice_sums(const float *probs, const uint8_t *gt, int batch, int h, int w, int k, double *out, void *stream_) {
    IMK_CHECK_ARG(probs && gt && out && batch > 0 && h > 0 && w > 0 && k > 0);
    imk_klaunch(eval_dice_sums_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream_, probs, gt, (long long)h * w * k, out);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
