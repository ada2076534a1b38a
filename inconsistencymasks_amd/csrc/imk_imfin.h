// The LDS finish of the IM kernels (the bodies of imk_imrule.h): a workgroup's label / mask bytes staged in LDS leave the CU as
// 16-byte stores, the image is blocked on the way through, and the per-image sizes take one global atomic per workgroup and map.
#pragma once
#include "imk_common.h"
#include "imk_head.h"

namespace {

constexpr int BIN_CHUNK = 1024;  // pixels per workgroup, binary kernel (4 per thread)
constexpr int MC_CHUNK = 256;    // pixels per workgroup, multiclass kernel (1 per thread)

// ---- shared phase 2: LDS results -> global, 16-byte stores when the shape allows -------------------
template <int CHUNK>
__device__ __forceinline__ void store_bytes(uint8_t *__restrict__ dst, const uint8_t *s, int n, bool vec) {
    const int t = threadIdx.x;
    if (vec) {
        for (int i = t; i < n / 16; i += 256)
            reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(s)[i];
    } else {
        for (int i = t; i < n; i += 256) dst[i] = s[i];
    }
}

__device__ __forceinline__ void block_image(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                            const uint8_t *s_im, int n_px, int c, int block_in, bool vec) {
    const int t = threadIdx.x;
    const int nbytes = n_px * c;
    if (vec) {
        for (int i = t; i < nbytes / 16; i += 256) {
            uint4 v = reinterpret_cast<const uint4 *>(src)[i];
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
            reinterpret_cast<uint4 *>(dst)[i] = v;
        }
    } else {
        for (int i = t; i < nbytes; i += 256) {
            const int px = i / c;
            dst[i] = (block_in && s_im[px]) ? 0 : src[i];
        }
    }
}

// head + IM kernels: sizes, label map(s), IM and blocked image of one workgroup (a must name hw, c, block_in and the outputs)
template <int NF, class Args>
__device__ __forceinline__ void head_im_finish(const Args &a, const uint8_t (*s_final)[BIN_CHUNK], const uint8_t *s_im,
                                               int *s_cnt, const int *cnt_a, const int *cnt_m, bool count_fg, int b, int p_base,
                                               int n_px, int vec_out, int vec_img) {
    const int t = threadIdx.x, hw = a.hw;
    // per-image sizes: wave reduction, one LDS atomic per wave, one global atomic per workgroup
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        int fa = cnt_a[k], fm = cnt_m[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { fa += __shfl_xor(fa, o, 64); fm += __shfl_xor(fm, o, 64); }
        if ((t & 63) == 0) { if (fa) atomicAdd(&s_cnt[2 * k], fa); if (fm) atomicAdd(&s_cnt[2 * k + 1], fm); }
    }
    __syncthreads();
    if (t < NF) {
        auto *ims = reinterpret_cast<unsigned long long *>(a.im_size), *pss = reinterpret_cast<unsigned long long *>(a.pred_size);
        if (count_fg && s_cnt[2 * t]) atomicAdd(&pss[(size_t)b * NF + t], (unsigned long long)s_cnt[2 * t]);
        if (s_cnt[2 * t + 1]) atomicAdd(&ims[(size_t)b * NF + t], (unsigned long long)s_cnt[2 * t + 1]);
    }
#pragma unroll
    for (int k = 0; k < NF; ++k)
        store_bytes<BIN_CHUNK>(a.masks_out + ((size_t)b * NF + k) * hw + p_base, s_final[k], n_px, vec_out);
    store_bytes<BIN_CHUNK>(a.im_out + (size_t)b * hw + p_base, s_im, n_px, vec_out);
    if (a.img) {
        const size_t off = ((size_t)b * hw + p_base) * a.c;
        block_image(a.img + off, a.img_out + off, s_im, n_px, a.c, a.block_in, vec_img);
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
