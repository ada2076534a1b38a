// Inconsistency masks over per-image sub-ensembles for gfx950 (MI355X).
//
// The EvalNet training-data writers of the IM++ family draw, for every image, a random sub-ensemble of the run's model pool
// (functions.py:3621-3640, 3826, 3931-3953: random.sample(models, n)) and form the IM over those members only.  Here image b
// carries a member word: bit n set = model n of the pool votes for image b.  The kernels are the ones of imk_im.hip with the model
// loop walking the set bits of that word.  A workgroup never straddles two images, so the word is wave-uniform: it is read once
// into a scalar register and the walk is scalar code (s_ff1 / s_and), the votes vector code as before.
//   * imk_im_binary_members / imk_im_multiclass_members: the rule on an fp32 probability stack of the whole pool;
//   * imk_launch_head_im_members: head + IM in one pass on the pool's last decoder activations, each model's slab compacted to the
//     images that use it (imk_unet_forward_im_members, imk_unet.hip);
//   * imk_morph_var: imk_morph with one window per image.
// With every bit set the outputs are those of imk_im.hip's kernels bit for bit: the same arithmetic in the same order.
#include <algorithm>

#include "imk_common.h"
#include "imk_head.h"
#include "imk_imfin.h"

namespace {

// the member word of image b as a scalar: bits at and above n_models are ignored
__device__ __forceinline__ uint32_t member_word(const uint32_t *__restrict__ members, int b, int n_models) {
    const uint32_t pool = n_models >= 32 ? 0xffffffffu : ((1u << n_models) - 1u);
    return __builtin_amdgcn_readfirstlane(members[b] & pool);
}

// ---- binary / HeLa on the probability stack (im_binary_vec of imk_im.hip) ---------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(256) void im_binary_members_vec(
    const float *__restrict__ preds, const uint32_t *__restrict__ members, int n_models, int batch, int hw, float thr, int cmp_ge,
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
    const uint32_t word = member_word(members, b, n_models);
    const int cnt = __builtin_popcount(word);
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
        for (uint32_t m = word; m; m &= m - 1) {
            const int n = __builtin_ctz(m);
            const float4 *src = reinterpret_cast<const float4 *>(preds + ((size_t)(n * batch + b) * hw + p0) * KB);
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
        uint32_t fin[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) fin[k] = 0;
        uint32_t im4 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool any = false;
            bool fg[KB];
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                fg[k] = cnt != 0 && (s[j][k] == cnt);          // nobody votes: no label, no IM
                const bool mx = (s[j][k] != 0) && !fg[k];
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
        for (int k = 0; k < KB; ++k) *reinterpret_cast<uint32_t *>(&s_final[k][4 * t]) = fin[k];
        *reinterpret_cast<uint32_t *>(&s_im[4 * t]) = im4;
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

// Any shape / alignment: one pixel per thread (im_binary_generic of imk_im.hip).
__global__ __launch_bounds__(256) void im_binary_members_generic(
    const float *__restrict__ preds, const uint32_t *__restrict__ members, int n_models, int batch, int hw, int kb, float thr,
    int cmp_ge, const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ masks_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, unsigned long long *__restrict__ pred_size) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const uint32_t word = member_word(members, b, n_models);
    const int cnt = __builtin_popcount(word);
    if (p >= hw) return;
    bool any = false;
    for (int k = 0; k < kb; ++k) {
        int s = 0;
        for (uint32_t m = word; m; m &= m - 1) {
            const int n = __builtin_ctz(m);
            const float v = preds[((size_t)(n * batch + b) * hw + p) * kb + k];
            s += cmp_ge ? (v >= thr) : (v > thr);
        }
        const bool fg = cnt != 0 && s == cnt;
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

// ---- multiclass on the probability stack (im_multi_kernel of imk_im.hip) -----------------------------------------------------------
// The reference anchors the comparison on the first sampled model (functions.py:3128); agreement of all members is symmetric, so
// the lowest member is the anchor here, whatever the sampling order was.
__global__ __launch_bounds__(256) void im_multi_members_kernel(
    const float *__restrict__ probs, const uint32_t *__restrict__ members, int n_models, int batch, int hw, int k_classes,
    uint32_t magic_k, const uint8_t *__restrict__ img, int c, int block_in, int block_out,
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
    const uint32_t word = member_word(members, b, n_models);
    if (t == 0) s_cnt = 0;
    int label0 = 0;
    bool agree = true, first = true;
    for (uint32_t m = word; m; m &= m - 1) {
        const int n = __builtin_ctz(m);
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
            if (first) label0 = best; else agree = agree && (best == label0);
        }
        first = false;
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

// ---- the member words, host -> workspace ------------------------------------------------------------------------------------------
// The words travel as kernel arguments, 256 per launch: the arguments are captured when the launch is enqueued, so the caller's array
// is free as soon as the call returns and nothing waits for the stream (a copy from pageable host memory would).
struct ImkMemberChunk {
    uint32_t w[256];
};
__global__ __launch_bounds__(256) void members_upload_kernel(ImkMemberChunk c, uint32_t *__restrict__ dst, int n) {
    const int t = threadIdx.x;
    if (t < n) dst[t] = c.w[t];
}

// ---- per-model image lists -----------------------------------------------------------------------------------------------------
// Thread n walks the B member words: list[n][i] = the i-th image that uses model n (int64: the index array of the gather kernel),
// row[n][b] = the position of image b in model n's compacted batch (-1: not a member).  B is a few hundred at the most.
__global__ __launch_bounds__(64) void members_lists_kernel(const uint32_t *__restrict__ members, int n_models, int batch,
                                                           int64_t *__restrict__ list, int *__restrict__ row) {
    const int n = threadIdx.x;
    if (n >= n_models) return;
    int pos = 0;
    for (int b = 0; b < batch; ++b) {
        const bool in = (members[b] >> n) & 1u;
        if (in) list[(size_t)n * batch + pos] = b;
        row[(size_t)n * batch + b] = in ? pos : -1;
        pos += in;
    }
}

// ---- head + IM in one pass over per-image members (head_im_sigmoid_kernel / head_im_softmax_kernel of imk_im.hip) -----------------------
// Sigmoid heads: the run-time-model-count form.  Only the members' head images are staged (slot n of the LDS image = model n), and
// each member's four-pixel loads go out before its votes.
template <int CS, int KB>
__global__ __launch_bounds__(256) void head_im_members_sigmoid_kernel(ImkHeadImMembersArgs a, int vec_out, int vec_img) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];   // n_models x head image (imk_head.h)
    __shared__ __attribute__((aligned(16))) uint8_t s_final[KB][BIN_CHUNK];
    __shared__ __attribute__((aligned(16))) uint8_t s_im[BIN_CHUNK];
    __shared__ int s_cnt[2 * KB];
    const int K = a.K, hw = a.hw;
    const int per_model = head_lds_floats<CS>(K);
    const int b = blockIdx.y, t = threadIdx.x;
    const int p_base = blockIdx.x * BIN_CHUNK;
    const int n_px = min(BIN_CHUNK, hw - p_base);
    const uint32_t word = member_word(a.members, b, a.n_models);
    const int cnt = __builtin_popcount(word);
    for (uint32_t m = word; m; m &= m - 1) {
        const int n = __builtin_ctz(m);
        head_stage<CS>(a.w[n], a.bias[n], a.sc[n], a.sh[n], a.cin, K, s_dyn + n * per_model);
    }
    if (t < 2 * KB) s_cnt[t] = 0;
    int cnt_a[KB], cnt_m[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) cnt_a[k] = cnt_m[k] = 0;
    const int p0 = 4 * t;                                   // hw % 16 == 0: a thread's 4 pixels are all in or all out
    __syncthreads();                                         // head images staged
    if (p0 < n_px) {
        int votes[4][KB];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < KB; ++k) votes[j][k] = 0;
        auto vote = [&](const float *hw_n, const f16x8 (&r)[CS / 8], int j) {
            const float *s_sc = hw_n + K * CS + K, *s_sh = s_sc + CS;
            float xin[CS];
#pragma unroll
            for (int q = 0; q < CS / 8; ++q)
#pragma unroll
                for (int e = 0; e < 8; e += 2) {                                                                                  // = head_input
                    const f16x2 r2 = imk_affine2(f16x2{r[q][e], r[q][e + 1]}, f32x2{s_sc[q * 8 + e], s_sc[q * 8 + e + 1]}, f32x2{s_sh[q * 8 + e], s_sh[q * 8 + e + 1]});
                    xin[q * 8 + e] = (float)r2[0]; xin[q * 8 + e + 1] = (float)r2[1];
                }
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const float v = head_sigmoid(head_logit<CS>(xin, hw_n, K, k));
                votes[j][k] += (a.cmp_ge ? (v >= a.thr) : (v > a.thr)) ? 1 : 0;      // NaN compares false
            }
        };
        for (uint32_t m = word; m; m &= m - 1) {
            const int n = __builtin_ctz(m);
            // image b is image row[n][b] of model n's compacted batch (a member: row >= 0)
            const long long p = (long long)a.row[(size_t)n * a.batch + b] * hw + p_base + p0;
            f16x8 r[4][CS / 8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < CS / 8; ++q) r[j][q] = *reinterpret_cast<const f16x8 *>(a.z[n] + (p + j) * CS + q * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) vote(s_dyn + n * per_model, r[j], j);
        }
        uint32_t fin[KB], im4 = 0;
#pragma unroll
        for (int k = 0; k < KB; ++k) fin[k] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool any = false, fg[KB];
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                fg[k] = cnt != 0 && votes[j][k] == cnt;
                const bool mx = votes[j][k] != 0 && !fg[k];
                cnt_a[k] += fg[k]; cnt_m[k] += mx;
                any |= mx;
            }
            if (any) im4 |= 0xffu << (8 * j);
#pragma unroll
            for (int k = 0; k < KB; ++k)
                if (fg[k] && !(a.block_out && any)) fin[k] |= 0xffu << (8 * j);
        }
#pragma unroll
        for (int k = 0; k < KB; ++k) *reinterpret_cast<uint32_t *>(&s_final[k][p0]) = fin[k];
        *reinterpret_cast<uint32_t *>(&s_im[p0]) = im4;
    }
    __syncthreads();
    head_im_finish<KB>(a, s_final, s_im, s_cnt, cnt_a, cnt_m, true, b, p_base, n_px, vec_out, vec_img);
}

// Softmax heads: a member's HeadMfma fragments are loaded for members only; label / agreement per unit stay in registers.
template <int KT>
__global__ __launch_bounds__(256) void head_im_members_softmax_kernel(ImkHeadImMembersArgs a, int vec_out, int vec_img) {
    __shared__ __attribute__((aligned(16))) uint8_t s_final[1][BIN_CHUNK];   // MC_CHUNK bytes used
    __shared__ __attribute__((aligned(16))) uint8_t s_im[BIN_CHUNK];
    __shared__ uint32_t s_pres[IMK_MEMBERS_MAX_POOL][64];
    __shared__ int s_cnt[2];
    const int K = a.K, hw = a.hw, cs = a.cs;
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, p16 = lane & 15, g = lane >> 4;
    const int p_base = blockIdx.x * MC_CHUNK;
    const int n_px = min(MC_CHUNK, hw - p_base);
    const uint32_t word = member_word(a.members, b, a.n_models);
    for (int i = t; i < IMK_MEMBERS_MAX_POOL * 64; i += 256) (&s_pres[0][0])[i] = 0;
    if (t < 2) s_cnt[t] = 0;
    __syncthreads();
    int cnt_a[1] = {0}, cnt_m[1] = {0};
    int label0[4] = {0, 0, 0, 0};
    bool agree[4] = {true, true, true, true};
    bool first = true;
    for (uint32_t m = word; m; m &= m - 1) {
        const int n = __builtin_ctz(m);
        const long long base = (long long)a.row[(size_t)n * a.batch + b] * hw + p_base;
        HeadMfma<KT> h;
        h.load(a.w[n], a.bias[n], a.sc[n], a.sh[n], a.cin, cs, K);
        f16x8 zr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = 64 * wave + 16 * u + p16;
            zr[u] = h.load_z(a.z[n], base + (q < n_px ? q : 0), cs);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            f32x4 pr[KT];
            h.probs(zr[u], K, pr);
            const int best = h.argmax(pr, K);
            if (g == 0 && 64 * wave + 16 * u + p16 < n_px) s_pres[n][best] = 1;
            if (first) label0[u] = best; else agree[u] = agree[u] && (best == label0[u]);
        }
        first = false;
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

// ---- morphology with one window per image (morph_kernel of imk_im.hip) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void morph_var_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                        int h, int w, const int *__restrict__ ksizes, int op) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    int ksize = __builtin_amdgcn_readfirstlane(ksizes[b]);
    if (x >= w || y >= h) return;
    const uint8_t *s = src + (size_t)b * h * w;
    if (ksize <= 0) {                                       // 0: the image is copied
        dst[(size_t)b * h * w + (size_t)y * w + x] = s[(size_t)y * w + x];
        return;
    }
    ksize = min(ksize, 31);
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

size_t head_im_members_lds(const ImkHeadImMembersArgs &a) {
    if (a.softmax) return 0;      // weights live in registers (HeadMfma)
    return (size_t)a.n_models * (a.K * a.cs + a.K + 2 * a.cs) * sizeof(float);
}

}  // namespace

bool imk_head_im_members_supported(const ImkHeadImMembersArgs &a, int max_members) {
    if (a.n_models < 1 || a.n_models > IMK_MEMBERS_MAX_POOL || max_members > IMK_HEAD_IM_MAX_MODELS) return false;
    ImkHeadImArgs s{};      // the shapes of the whole-batch kernel (imk_im.hip), one member standing for all
    s.n_models = 1; s.cin = a.cin; s.cs = a.cs; s.K = a.K; s.softmax = a.softmax; s.batch = a.batch; s.hw = a.hw;
    s.masks_out = a.masks_out; s.im_out = a.im_out;
    return imk_head_im_supported(s) && head_im_members_lds(a) <= 64 * 1024;
}

void imk_launch_members_upload(const uint32_t *members_host, int batch, uint32_t *dst, hipStream_t stream) {
    for (int b0 = 0; b0 < batch; b0 += 256) {
        ImkMemberChunk c{};
        const int n = std::min(256, batch - b0);
        for (int i = 0; i < n; ++i) c.w[i] = members_host[b0 + i];
        imk_klaunch(members_upload_kernel, dim3(1), dim3(256), 0, stream, c, dst + b0, n);
    }
}

void imk_launch_members_lists(const uint32_t *members, int n_models, int batch, int64_t *list, int *row, hipStream_t stream) {
    imk_klaunch(members_lists_kernel, dim3(1), dim3(64), 0, stream, members, n_models, batch, list, row);
}

int imk_launch_head_im_members(const ImkHeadImMembersArgs &a, int max_members, hipStream_t stream) {
    IMK_CHECK_ARG(a.n_models > 0 && a.batch > 0 && a.hw > 0 && a.K > 0 && a.members && a.row);
    IMK_CHECK_ARG(a.masks_out && a.im_out && a.im_size && (a.softmax || a.pred_size));
    IMK_CHECK_ARG(!a.img || (a.img_out && a.c > 0));
    if (!imk_head_im_members_supported(a, max_members)) return IMK_EUNSUPPORTED;
    const int nf = a.softmax ? 1 : a.K;
    IMK_HIP(hipMemsetAsync(a.im_size, 0, sizeof(int64_t) * a.batch * nf, stream));
    if (a.pred_size && !a.softmax) IMK_HIP(hipMemsetAsync(a.pred_size, 0, sizeof(int64_t) * a.batch * nf, stream));
    if (a.softmax && a.presence) IMK_HIP(hipMemsetAsync(a.presence, 0, (size_t)a.n_models * a.batch * a.K, stream));
    const size_t lds = head_im_members_lds(a);
    const int chunk = a.softmax ? MC_CHUNK : BIN_CHUNK;
    const int vec_img2 = a.img && ((int64_t)a.hw * a.c % 16 == 0) && (chunk * a.c % 16 == 0) && aligned16(a.img) && aligned16(a.img_out);
    const dim3 grid(imk_cdiv(a.hw, chunk), a.batch);
#define IMK_HIMM_LAUNCH(KERN) imk_klaunch(KERN, dim3(grid), dim3(256), lds, stream, a, 1, vec_img2)
    if (a.softmax) {
        switch ((a.K + 15) / 16) {
            case 1: IMK_HIMM_LAUNCH(head_im_members_softmax_kernel<1>); break;
            case 2: IMK_HIMM_LAUNCH(head_im_members_softmax_kernel<2>); break;
            case 3: IMK_HIMM_LAUNCH(head_im_members_softmax_kernel<3>); break;
            default: IMK_HIMM_LAUNCH(head_im_members_softmax_kernel<4>); break;
        }
    } else {
#define IMK_HIMM_KB(CSV)                                                                                                    \
        switch (a.K) {                                                                                                      \
            case 1: IMK_HIMM_LAUNCH((head_im_members_sigmoid_kernel<CSV, 1>)); break;                                       \
            case 2: IMK_HIMM_LAUNCH((head_im_members_sigmoid_kernel<CSV, 2>)); break;                                       \
            case 3: IMK_HIMM_LAUNCH((head_im_members_sigmoid_kernel<CSV, 3>)); break;                                       \
            default: IMK_HIMM_LAUNCH((head_im_members_sigmoid_kernel<CSV, 4>)); break;                                      \
        }
        switch (a.cs) {
            case 8: IMK_HIMM_KB(8); break;
            case 16: IMK_HIMM_KB(16); break;
            case 24: IMK_HIMM_KB(24); break;
            default: IMK_HIMM_KB(32); break;
        }
#undef IMK_HIMM_KB
    }
#undef IMK_HIMM_LAUNCH
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_im_binary_members(const float *preds, const uint32_t *members, int n_models, int batch, int h, int w, int kb,
                                     float thr, int cmp_ge, const uint8_t *img, int c, int block_in, int block_out,
                                     uint8_t *img_out, uint8_t *masks_out, uint8_t *im_out,
                                     int64_t *im_size, int64_t *pred_size, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    IMK_CHECK_ARG(preds && members && masks_out && im_out && im_size && pred_size);
    IMK_CHECK_ARG(n_models > 0 && n_models <= IMK_MEMBERS_MAX_POOL && batch > 0 && batch <= 65535 && h > 0 && w > 0 && kb > 0);
    IMK_CHECK_ARG(!img || (img_out && c > 0));
    const int64_t hw64 = (int64_t)h * w;
    IMK_CHECK_ARG(hw64 < (1ll << 30));
    const int hw = (int)hw64;
    IMK_HIP(hipMemsetAsync(im_size, 0, sizeof(int64_t) * batch * kb, stream));
    IMK_HIP(hipMemsetAsync(pred_size, 0, sizeof(int64_t) * batch * kb, stream));
    auto *ims = reinterpret_cast<unsigned long long *>(im_size);
    auto *pss = reinterpret_cast<unsigned long long *>(pred_size);
    const bool vec_ok = (hw % 4 == 0) && aligned16(preds) && (kb == 1 || kb == 3);
    if (vec_ok) {
        const int vec_out = (hw % 16 == 0) && aligned16(masks_out) && aligned16(im_out);
        const int vec_img = img && ((int64_t)hw * c % 16 == 0) && aligned16(img) && aligned16(img_out);
        dim3 grid(imk_cdiv(hw, BIN_CHUNK), batch);
        if (kb == 1)
            imk_klaunch(im_binary_members_vec<1>, dim3(grid), dim3(256), 0, stream, preds, members, n_models, batch, hw, thr, cmp_ge, img, c,
                        block_in, block_out, img_out, masks_out, im_out, ims, pss, vec_out, vec_img);
        else
            imk_klaunch(im_binary_members_vec<3>, dim3(grid), dim3(256), 0, stream, preds, members, n_models, batch, hw, thr, cmp_ge, img, c,
                        block_in, block_out, img_out, masks_out, im_out, ims, pss, vec_out, vec_img);
    } else {
        dim3 grid(imk_cdiv(hw, 256), batch);
        imk_klaunch(im_binary_members_generic, dim3(grid), dim3(256), 0, stream, preds, members, n_models, batch, hw, kb, thr, cmp_ge, img,
                    c, block_in, block_out, img_out, masks_out, im_out, ims, pss);
    }
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_im_multiclass_members(const float *probs, const uint32_t *members, int n_models, int batch, int h, int w, int k,
                                         const uint8_t *img, int c, int block_in, int block_out,
                                         uint8_t *img_out, uint8_t *final_out, uint8_t *im_out,
                                         int64_t *im_size, uint8_t *presence, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    IMK_CHECK_ARG(probs && members && final_out && im_out && im_size);
    IMK_CHECK_ARG(n_models > 0 && n_models <= IMK_MEMBERS_MAX_POOL && batch > 0 && batch <= 65535 && h > 0 && w > 0 && k > 0);
    IMK_CHECK_ARG(!img || (img_out && c > 0));
    if (k > 64) return IMK_EUNSUPPORTED;
    const int64_t hw64 = (int64_t)h * w;
    IMK_CHECK_ARG(hw64 < (1ll << 30));
    const int hw = (int)hw64;
    IMK_HIP(hipMemsetAsync(im_size, 0, sizeof(int64_t) * batch, stream));
    if (presence) IMK_HIP(hipMemsetAsync(presence, 0, (size_t)n_models * batch * k, stream));
    const int vec_in = aligned16(probs) && (((int64_t)hw * k) % 4 == 0) && ((MC_CHUNK * k) % 4 == 0);
    const int vec_out = (hw % 16 == 0) && aligned16(final_out) && aligned16(im_out);
    const int vec_img = img && ((int64_t)hw * c % 16 == 0) && aligned16(img) && aligned16(img_out);
    const uint32_t magic = (uint32_t)((1ull << 32) / (uint32_t)k) + 1u;
    const size_t lds = (size_t)MC_CHUNK * (k | 1) * sizeof(float);
    dim3 grid(imk_cdiv(hw, MC_CHUNK), batch);
    imk_klaunch(im_multi_members_kernel, dim3(grid), dim3(256), lds, stream, probs, members, n_models, batch, hw, k, magic, img, c, block_in,
                block_out, img_out, final_out, im_out, reinterpret_cast<unsigned long long *>(im_size), presence, vec_in, vec_out,
                vec_img);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_morph_var(const uint8_t *src, uint8_t *dst, int batch, int h, int w, const int32_t *ksizes, int op, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    IMK_CHECK_ARG(src && dst && src != dst && ksizes && batch > 0 && batch <= 65535 && h > 0 && w > 0 && (op == 0 || op == 1));
    dim3 grid(imk_cdiv(w, 64), imk_cdiv(h, 4), batch);
    imk_klaunch(morph_var_kernel, dim3(grid), dim3(256), 0, stream, src, dst, h, w, ksizes, op);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
