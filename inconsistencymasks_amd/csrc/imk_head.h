// The U-Net's output layer (unet.py:63: Conv2D(num_outputmasks, (1,1), activation=actifuout, dtype='float32') on the last
// decoder block's BatchNorm output), per pixel, in fp32 -- shared by head_kernel (probabilities -> HBM) and head_im_kernel
// (probabilities -> votes -> inconsistency mask, nothing stored), so that both produce the SAME fp32 probabilities bit for
// bit: the IM chain thresholds them (`>` / `>=` 0.5, functions.py:3157 / 3187) and takes their arg-max (functions.py:3225).
#pragma once
#include "imk_common.h"

// LDS image of one model's head: w^T [K][CS] (input channels beyond cin are zero), bias [K], BN scale [CS], shift [CS]
template <int CS>
__device__ __forceinline__ int head_lds_floats(int K) { return K * CS + K + 2 * CS; }

template <int CS>
__device__ __forceinline__ void head_stage(const float *__restrict__ w /*[cin][K]*/, const float *__restrict__ bias,
                                           const float *__restrict__ sc, const float *__restrict__ sh, int cin, int K,
                                           float *s_w) {
    float *s_b = s_w + K * CS, *s_sc = s_b + K, *s_sh = s_sc + CS;
    for (int i = threadIdx.x; i < K * CS; i += 256) {
        const int k = i / CS, c = i - k * CS;
        s_w[i] = (c < cin) ? w[(size_t)c * K + k] : 0.f;
    }
    for (int i = threadIdx.x; i < K; i += 256) s_b[i] = bias[i];
    for (int i = threadIdx.x; i < CS; i += 256) { s_sc[i] = sc[i]; s_sh[i] = sh[i]; }
}

// the pixel's input: fp16(z * scale + shift) per channel (the BatchNorm of the last decoder block, applied on load)
template <int CS>
__device__ __forceinline__ void head_input(const f16 *__restrict__ z, long long p, const float *s_w, int K, float (&xin)[CS]) {
    const float *s_sc = s_w + K * CS + K, *s_sh = s_sc + CS;
#pragma unroll
    for (int q = 0; q < CS / 8; ++q) {
        const f16x8 v = *reinterpret_cast<const f16x8 *>(z + p * CS + q * 8);
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const f16x2 r2 = imk_affine2(f16x2{v[j], v[j + 1]}, f32x2{s_sc[q * 8 + j], s_sc[q * 8 + j + 1]}, f32x2{s_sh[q * 8 + j], s_sh[q * 8 + j + 1]});
            xin[q * 8 + j] = (float)r2[0]; xin[q * 8 + j + 1] = (float)r2[1];
        }
    }
}

// the same from activation vectors the caller loaded itself (several pixels' loads in flight before the first one's arithmetic)
template <int CS>
__device__ __forceinline__ void head_input_regs(const f16x8 (&v)[CS / 8], const float *s_w, int K, float (&xin)[CS]) {
    const float *s_sc = s_w + K * CS + K, *s_sh = s_sc + CS;
#pragma unroll
    for (int q = 0; q < CS / 8; ++q)
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const f16x2 r2 = imk_affine2(f16x2{v[q][j], v[q][j + 1]}, f32x2{s_sc[q * 8 + j], s_sc[q * 8 + j + 1]}, f32x2{s_sh[q * 8 + j], s_sh[q * 8 + j + 1]});
            xin[q * 8 + j] = (float)r2[0]; xin[q * 8 + j + 1] = (float)r2[1];
        }
}

template <int CS>
__device__ __forceinline__ float head_logit(const float (&xin)[CS], const float *s_w, int K, int k) {
    float acc = s_w[K * CS + k];
#pragma unroll
    for (int c = 0; c < CS; ++c) acc += xin[c] * s_w[k * CS + c];
    return acc;
}

__device__ __forceinline__ float head_sigmoid(float logit) { return 1.0f / (1.0f + expf(-logit)); }

// ---- Dice loss (loss kind 4; imk_dice.hip and head_mse_fused_kernel's Dice variant) ----------------------------------------------
// image of pixel p of a [B][hw] batch (one 32-bit divide wherever the pixel index fits)
__device__ __forceinline__ int dice_image(long long p, int hw) {
    return (p >> 32) ? (int)(p / hw) : (int)((unsigned)p / (unsigned)hw);
}
// d(loss * scale)/d(logit) of an element with target t and probability pk of an image with coefficients (c0, c1): the ONE
// expression of both gradient kernels, so that the routes differ by their dgrad alone
__device__ __forceinline__ float dice_dlogit(float S, float c0, float c1, float t, float pk) {
    return S * (c0 - c1 * t) * (pk * (1.0f - pk));
}

// softmax over the K classes into row[0..K) (an LDS row of the caller)
template <int CS>
__device__ __forceinline__ void head_softmax_row(const float (&xin)[CS], const float *s_w, int K, float *row) {
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const float acc = head_logit<CS>(xin, s_w, K, k);
        row[k] = acc;
        mx = fmaxf(mx, acc);
    }
    float sum = 0.f;
    for (int k = 0; k < K; ++k) { const float e = expf(row[k] - mx); row[k] = e; sum += e; }
    const float inv = 1.0f / sum;
    for (int k = 0; k < K; ++k) row[k] *= inv;
}

// ---- softmax heads on the matrix cores (head_softmax_kernel: probabilities -> HBM; head_im_softmax_kernel: -> votes) ------
// logits^T [class][pixel] = W^T . x^T + b on v_mfma_f32_16x16x32_f16, ONE k-step for all (<= 32) input channels, with the fp32
// weights of the reference's float32 output layer split into two fp16 halves w = hi + lo (hi = fp16(w), lo = fp16(w - hi)): the
// products with the fp16 activations are exact in fp32 and the two MFMAs carry ~22 bits of w (1e-7 relative).  A wave takes 16
// pixels per unit, lane (p16 = lane & 15, g = lane >> 4) supplies the channels 8 g + j of pixel p16 (the 16 bytes it loads
// itself) and receives the classes 16 kt + 4 g + r of the same pixel, so the softmax is registers + two shuffles over the 4
// lanes of a pixel.  History: one thread per pixel with a broadcast LDS read per product took 2.0 ms per 128 Cityscapes images
// and 2 models at alpha 2; fp32 MFMAs (16x16x4, 8 dependent steps per class tile) 1.0 ms, 40 % of it matrix-core time.
// Both kernels call probs() below and nothing else, so the stored and the voted probabilities are the same bits.
template <int KT /* 16-class tiles */>
struct HeadMfma {
    f16x8 whi[KT], wlo[KT];
    float bias_r[KT][4], sc8[8], sh8[8];

    __device__ __forceinline__ void load(const float *__restrict__ w /*[cin][K]*/, const float *__restrict__ bias,
                                         const float *__restrict__ sc, const float *__restrict__ sh, int cin, int cs, int K) {
        const int lane = threadIdx.x & 63, p16 = lane & 15, g = lane >> 4;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 8 * g + j, k = 16 * kt + p16;
                const float v = (c < cin && k < K) ? w[(size_t)c * K + k] : 0.f;
                whi[kt][j] = (f16)v;
                wlo[kt][j] = (f16)(v - (float)whi[kt][j]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) { const int k = 16 * kt + 4 * g + r; bias_r[kt][r] = k < K ? bias[k] : 0.f; }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { const int c = 8 * g + j; sc8[j] = c < cs ? sc[c] : 0.f; sh8[j] = c < cs ? sh[c] : 0.f; }
    }

    // this lane's 8 channels of pixel p (cs is a multiple of 8: they are all inside or all outside the tensor)
    __device__ __forceinline__ f16x8 load_z(const f16 *__restrict__ z, long long p, int cs) const {
        const int g = (threadIdx.x & 63) >> 4;
        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (8 * g < cs) v = *reinterpret_cast<const f16x8 *>(z + p * cs + 8 * g);
        return v;
    }

    // softmax probabilities of the lane's pixel: pr[kt][r] = class 16 kt + 4 g + r (0 for classes >= K)
    __device__ __forceinline__ void probs(const f16x8 &z8, int K, f32x4 (&pr)[KT]) const {
        const int g = (threadIdx.x & 63) >> 4;
        f16x8 x8;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {                                                  // as head_input
            const f16x2 r2 = imk_affine2(f16x2{z8[j], z8[j + 1]}, f32x2{sc8[j], sc8[j + 1]}, f32x2{sh8[j], sh8[j + 1]});
            x8[j] = r2[0]; x8[j + 1] = r2[1];
        }
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
            pr[kt] = f32x4{bias_r[kt][0], bias_r[kt][1], bias_r[kt][2], bias_r[kt][3]};
            pr[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(whi[kt], x8, pr[kt], 0, 0, 0);
            pr[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wlo[kt], x8, pr[kt], 0, 0, 0);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (16 * kt + 4 * g + r >= K) pr[kt][r] = -INFINITY;     // padding classes: exp -> 0
                mx = fmaxf(mx, pr[kt][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { pr[kt][r] = __builtin_amdgcn_exp2f((pr[kt][r] - mx) * 1.44269504088896f); sum += pr[kt][r]; }   // v_exp_f32 (1 ulp of 2^x)
        sum += __shfl_xor(sum, 16, 64);      // (s_g + s_g^1) + (s_g^2 + s_g^3): the same bits on the 4 lanes of a pixel
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) pr[kt][r] *= inv;
    }

    // arg-max over the K classes of the lane's pixel, the lowest index winning ties (numpy's argmax, functions.py:3225);
    // the same value on the 4 lanes of the pixel
    __device__ __forceinline__ int argmax(const f32x4 (&pr)[KT], int K) const {
        const int g = (threadIdx.x & 63) >> 4;
        float bv = -1.f;
        int bk = 0x7fffffff;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 16 * kt + 4 * g + r;
                if (k < K && pr[kt][r] > bv) { bv = pr[kt][r]; bk = k; }     // ascending k within a lane: strict > keeps the first
            }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int ok = __shfl_xor(bk, o, 64);
            if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
        }
        return bk == 0x7fffffff ? 0 : bk;
    }
};

// ---- np.argmax (the model-ensemble, input-ensemble and teacher-label kernels) ----------------------------------------------------------------------------------------------------------------
// candidates of ascending k: bk < 0 = none yet
__device__ __forceinline__ void np_argmax_step(float v, int k, float &bv, int &bk) {
    if (bk < 0) { bv = v; bk = k; return; }
    if (__builtin_isnan(bv)) return;                   // the first NaN holds
    if (__builtin_isnan(v) || v > bv) { bv = v; bk = k; }
}
// two partial results of disjoint class sets (any order): NaN first, then the larger value, the lower index on ties
__device__ __forceinline__ void np_argmax_merge(float ov, int ok, float &bv, int &bk) {
    if (ok < 0) return;
    if (bk < 0) { bv = ov; bk = ok; return; }
    const bool on = __builtin_isnan(ov), bn = __builtin_isnan(bv);
    const bool take = (on || bn) ? (on && (!bn || ok < bk)) : (ov > bv || (ov == bv && ok < bk));
    if (take) { bv = ov; bk = ok; }
}
// np.argmax over the K classes of the lane's pixel in HeadMfma's layout (v[kt][r] = class 16 kt + 4 g + r); the same value on the 4
// lanes of the pixel
template <int KT>
__device__ __forceinline__ int vote_argmax(const f32x4 (&v)[KT], int K) {
    const int g = (threadIdx.x & 63) >> 4;
    float bv = 0.f;
    int bk = -1;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 16 * kt + 4 * g + r;
            if (k < K) np_argmax_step(v[kt][r], k, bv, bk);
        }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) np_argmax_merge(__shfl_xor(bv, o, 64), __shfl_xor(bk, o, 64), bv, bk);
    return bk;
}

// ---- fused head + inconsistency mask (imk_im.hip) -------------------------------------------------------------------------
#define IMK_HEAD_IM_MAX_MODELS 8
struct ImkHeadImArgs {
    const f16 *z[IMK_HEAD_IM_MAX_MODELS];        // last decoder block's conv output [B,H,W,cs] of every model
    const float *sc[IMK_HEAD_IM_MAX_MODELS], *sh[IMK_HEAD_IM_MAX_MODELS];   // its folded BatchNorm
    const float *w[IMK_HEAD_IM_MAX_MODELS], *bias[IMK_HEAD_IM_MAX_MODELS];  // the head's fp32 kernel [cin][K] / bias [K]
    int n_models, cin, cs, K, softmax;
    int batch, hw;
    float thr;
    int cmp_ge;
    const uint8_t *img;
    int c, block_in, block_out;
    uint8_t *img_out, *masks_out, *im_out;
    int64_t *im_size, *pred_size;
    uint8_t *presence;
};
// sigmoid heads: K <= 4 (ISIC 1, HeLa 3); softmax heads: K <= 64.  Returns IMK_EUNSUPPORTED otherwise (the caller then
// runs head_kernel per model + imk_im_binary / imk_im_multiclass).
bool imk_head_im_supported(const ImkHeadImArgs &a);
int imk_launch_head_im(const ImkHeadImArgs &a, hipStream_t stream);

// ---- fused head + inconsistency mask over per-image members of a model pool (imk_im.hip) -----------------------------------
#define IMK_MEMBERS_MAX_POOL 16
struct ImkHeadImMembersArgs {
    const f16 *z[IMK_MEMBERS_MAX_POOL];          // model n's last decoder conv output [count_n,H,W,cs]: the images that use it
    const float *sc[IMK_MEMBERS_MAX_POOL], *sh[IMK_MEMBERS_MAX_POOL];       // its folded BatchNorm
    const float *w[IMK_MEMBERS_MAX_POOL], *bias[IMK_MEMBERS_MAX_POOL];      // the head's fp32 kernel [cin][K] / bias [K]
    const uint32_t *members;                     // device [B]: bit n = model n votes for image b
    const int *row;                              // device [n_models][B]: image b's position in model n's batch (members only)
    int n_models, cin, cs, K, softmax;
    int batch, hw;
    float thr;
    int cmp_ge;
    const uint8_t *img;
    int c, block_in, block_out;
    uint8_t *img_out, *masks_out, *im_out;
    int64_t *im_size, *pred_size;
    uint8_t *presence;
};
// The shapes of imk_head_im_supported, a pool of at most 16 models and at most 8 members per image.
bool imk_head_im_members_supported(const ImkHeadImMembersArgs &a, int max_members);
int imk_launch_head_im_members(const ImkHeadImMembersArgs &a, int max_members, hipStream_t stream);
// the host's member words into a device array [B], as kernel arguments (nothing waits for the stream)
void imk_launch_members_upload(const uint32_t *members_host, int batch, uint32_t *dst, hipStream_t stream);
// list [n_models][B] int64 (the images of model n, in order) and row [n_models][B] from the member words; one launch
void imk_launch_members_lists(const uint32_t *members, int n_models, int batch, int64_t *list, int *row, hipStream_t stream);

// ---- fused head + standard-deviation map of the depth-map IM (imk_depth.hip) ------------------------------------------------
struct ImkDepthHeadArgs {
    const f16 *z[IMK_HEAD_IM_MAX_MODELS];        // last decoder block's conv output [B,H,W,cs] of every model
    const float *sc[IMK_HEAD_IM_MAX_MODELS], *sh[IMK_HEAD_IM_MAX_MODELS];   // its folded BatchNorm
    const float *w[IMK_HEAD_IM_MAX_MODELS], *bias[IMK_HEAD_IM_MAX_MODELS];  // the head's fp32 kernel [cin][1] / bias [1]
    int n_models, cin, cs, K, softmax;
    int batch, hw;
    float *map;                                  // [B,H,W] fp32: the per-pixel standard deviation over the models
};
// Sigmoid heads with one map, last decoder widths 8 / 16 / 24 / 32, 2 .. 8 models, H*W a multiple of 16, a 16-byte aligned map.
bool imk_depth_head_supported(const ImkDepthHeadArgs &a);
int imk_launch_depth_head_std(const ImkDepthHeadArgs &a, hipStream_t stream);
// launches 2 and 3 of imk_im_depth on a finished map (image thresholds, then mask + blocking + sizes)
int imk_depth_finish(const float *map, int batch, int hw, float mult, const uint8_t *img, int c, int block_in, uint8_t *img_out,
                     uint8_t *im_out, int64_t *im_size, float *thr_out, hipStream_t stream);

// ---- fused head + model-ensemble vote (imk_vote.hip) ----------------------------------------------------------------------
struct ImkVoteHeadArgs {
    const f16 *z[IMK_HEAD_IM_MAX_MODELS];        // last decoder block's conv output [B,H,W,cs] of every model
    const float *sc[IMK_HEAD_IM_MAX_MODELS], *sh[IMK_HEAD_IM_MAX_MODELS];   // its folded BatchNorm
    const float *w[IMK_HEAD_IM_MAX_MODELS], *bias[IMK_HEAD_IM_MAX_MODELS];  // the head's fp32 kernel [cin][K] / bias [K]
    int n_models, cin, cs, K, softmax;
    int batch, hw;
    double thr;                                  // fp64 for the soft vote; the hard vote compares against (float)thr
    int mode;                                    // IMK_VOTE_HARD / IMK_VOTE_SOFT
    uint8_t *out;                                // masks [B,K,H,W] {0,255}
};
// Sigmoid heads in the shapes of imk_head_im_supported; the caller takes imk_unet_forward + imk_vote_* otherwise.
bool imk_vote_head_supported(const ImkVoteHeadArgs &a);
int imk_launch_vote_head(const ImkVoteHeadArgs &a, hipStream_t stream);

// ---- fused head + D4-restoring input-ensemble vote (imk_views.hip) --------------------------------------------------------
struct ImkViewVoteArgs {
    const f16 *z;                                // last decoder block's conv output of the M*B views [M,B,H,W,cs]
    const float *sc, *sh, *wt, *bias;            // its folded BatchNorm; the head's fp32 kernel [cin][K] / bias [K] (one model)
    const int *ops;                              // device [M][ops_ld]: the D4 op of view m of image b at m * ops_ld + b
    int ops_ld, n_views, cin, cs, K, batch, h, w;
    double thr;                                  // compared as (float)thr
    int cmp_ge;                                  // p >= thr (ISIC) or p > thr
    uint8_t *out;                                // masks [B,K,H,W] {0,255}
};
bool imk_views_vote_head_supported(const ImkViewVoteArgs &a);
int imk_launch_views_vote_head(const ImkViewVoteArgs &a, hipStream_t stream);
int imk_vote_views_binary_ld(const float *preds, int n_views, int batch, int h, int w, int k, const int *ops, int ops_ld,
                             double thr, int cmp_ge, uint8_t *masks_out, hipStream_t stream);

// ---- fused head + teacher label moved with the image (imk_student.hip) -----------------------------------------------------
struct ImkStudentArgs {
    const f16 *z;                                // last decoder block's conv output [B,H,W,cs]
    const float *sc, *sh, *wt, *bias;            // its folded BatchNorm; the head's fp32 kernel [cin][K] / bias [K]
    const imk_aug_params *aug;                   // device [B]: flip_v, flip_h, rot of every image
    int cin, cs, K, softmax, batch, h, w;
    float thr;
    int cmp_ge;                                  // sigmoid: p >= thr or p > thr
    uint8_t *out;                                // sigmoid: [B,K,H,W] {0,255}; softmax: [B,H,W] class ids -- in the moved frame
};
// The shapes of imk_vote_head_supported; the caller takes imk_unet_forward + label + imk_augment otherwise.
bool imk_student_head_supported(const ImkStudentArgs &a);
int imk_launch_student_head(const ImkStudentArgs &a, hipStream_t stream);
// planar label maps [B,P,H,W] -> the same maps moved by aug[b]'s flips / turn (the unfused route of sigmoid heads with P > 1)
int imk_student_move_planes(const uint8_t *src, int batch, int planes, int h, int w, const imk_aug_params *aug, uint8_t *out,
                            hipStream_t stream);
