// Fused Inconsistency-Mask kernels for gfx950 (MI355X).
//
// One launch per batch turns the N-model probability stack into pseudo-label, inconsistency mask,
// blocked image and per-image sizes -- the chain the reference runs per image in numpy:
//   threshold/argmax  functions.py:3157, 3187-3189, 3225
//   agreement         functions.py:3104-3120 (binary), 3123-3137 (multiclass), 3195-3200 (HeLa combine)
//   blocking          functions.py:2867-2874
// The kernels are pure streaming (about 3 integer ops per byte): the roofline is HBM bandwidth.
// Layout choices for that: every global access is a 16-byte vector per lane (float4 probability
// loads, uint4 mask / image stores); results are staged in LDS so that the byte-granular outputs
// (3-channel images, 1-byte masks) still leave the CU as full 16-byte stores; one workgroup never
// straddles two images so the per-image sizes need one integer atomic per workgroup and channel.
//
// Every kernel comes in two forms over one body (imk_imrule.h): the whole ensemble votes for every image, or image b carries a
// member word (bit n set = model n of the pool votes for image b).  The EvalNet training-data writers of the IM++ family draw, for
// every image, a random sub-ensemble of the run's model pool (functions.py:3621-3640, 3826, 3931-3953: random.sample(models, n)) and
// form the IM over those members only:
//   * imk_im_binary_members / imk_im_multiclass_members: the rule on an fp32 probability stack of the whole pool;
//   * imk_launch_head_im_members: head + IM in one pass on the pool's last decoder activations, each model's slab compacted to the
//     images that use it (imk_unet_forward_im_members, imk_unet.hip);
//   * imk_morph_var: imk_morph with one window per image.
// With every bit set the outputs are those of the whole-ensemble kernels bit for bit: the same body, the same arithmetic in the
// same order.
#include <algorithm>
#include <optional>
#include <type_traits>

#include "imk_common.h"
#include "imk_head.h"
#include "imk_imrule.h"

namespace {

// ---- the kernels: a model set (imk_imrule.h) and the body ------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(256) void im_binary_vec(
    const float *__restrict__ preds, int n_models, int batch, int hw, float thr, int cmp_ge,
    const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ masks_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, unsigned long long *__restrict__ pred_size, int vec_out, int vec_img) {
    im_binary_vec_body<KB>(AllModels{n_models}, preds, batch, hw, thr, cmp_ge, img, c, block_in, block_out, img_out, masks_out, im_out,
                           im_size, pred_size, vec_out, vec_img);
}
template <int KB>
__global__ __launch_bounds__(256) void im_binary_members_vec(
    const float *__restrict__ preds, const uint32_t *__restrict__ members, int n_models, int batch, int hw, float thr, int cmp_ge,
    const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ masks_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, unsigned long long *__restrict__ pred_size, int vec_out, int vec_img) {
    im_binary_vec_body<KB>(MemberBits(members, blockIdx.y, n_models), preds, batch, hw, thr, cmp_ge, img, c, block_in, block_out,
                           img_out, masks_out, im_out, im_size, pred_size, vec_out, vec_img);
}

__global__ __launch_bounds__(256) void im_binary_generic(
    const float *__restrict__ preds, int n_models, int batch, int hw, int kb, float thr, int cmp_ge,
    const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ masks_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, unsigned long long *__restrict__ pred_size) {
    im_binary_generic_body(AllModels{n_models}, preds, batch, hw, kb, thr, cmp_ge, img, c, block_in, block_out, img_out, masks_out,
                           im_out, im_size, pred_size);
}
__global__ __launch_bounds__(256) void im_binary_members_generic(
    const float *__restrict__ preds, const uint32_t *__restrict__ members, int n_models, int batch, int hw, int kb, float thr,
    int cmp_ge, const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ masks_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, unsigned long long *__restrict__ pred_size) {
    im_binary_generic_body(MemberBits(members, blockIdx.y, n_models), preds, batch, hw, kb, thr, cmp_ge, img, c, block_in, block_out,
                           img_out, masks_out, im_out, im_size, pred_size);
}

__global__ __launch_bounds__(256) void im_multi_kernel(
    const float *__restrict__ probs, int n_models, int batch, int hw, int k_classes, uint32_t magic_k,
    const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ final_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, uint8_t *__restrict__ presence, int vec_in, int vec_out, int vec_img) {
    im_multi_body(AllModels{n_models}, probs, batch, hw, k_classes, magic_k, img, c, block_in, block_out, img_out, final_out, im_out,
                  im_size, presence, vec_in, vec_out, vec_img);
}
__global__ __launch_bounds__(256) void im_multi_members_kernel(
    const float *__restrict__ probs, const uint32_t *__restrict__ members, int n_models, int batch, int hw, int k_classes,
    uint32_t magic_k, const uint8_t *__restrict__ img, int c, int block_in, int block_out,
    uint8_t *__restrict__ img_out, uint8_t *__restrict__ final_out, uint8_t *__restrict__ im_out,
    unsigned long long *__restrict__ im_size, uint8_t *__restrict__ presence, int vec_in, int vec_out, int vec_img) {
    im_multi_body(MemberBits(members, blockIdx.y, n_models), probs, batch, hw, k_classes, magic_k, img, c, block_in, block_out, img_out,
                  final_out, im_out, im_size, presence, vec_in, vec_out, vec_img);
}

template <int CS, int KB, int NM /* models, compile-time (0: run-time) */>
__global__ __launch_bounds__(256) void head_im_sigmoid_kernel(ImkHeadImArgs a, int vec_out, int vec_img) {
    head_im_sigmoid_body<CS, KB, NM>(AllModels{NM > 0 ? NM : a.n_models}, a, vec_out, vec_img);
}
template <int CS, int KB>      // the run-time-model-count form
__global__ __launch_bounds__(256) void head_im_members_sigmoid_kernel(ImkHeadImMembersArgs a, int vec_out, int vec_img) {
    head_im_sigmoid_body<CS, KB, 0>(MemberBits(a.members, blockIdx.y, a.n_models, a.row, a.batch), a, vec_out, vec_img);
}

template <int KT>
__global__ __launch_bounds__(256) void head_im_softmax_kernel(ImkHeadImArgs a, int vec_out, int vec_img) {
    head_im_softmax_body<KT>(AllModels{a.n_models}, a, vec_out, vec_img);
}
template <int KT>
__global__ __launch_bounds__(256) void head_im_members_softmax_kernel(ImkHeadImMembersArgs a, int vec_out, int vec_img) {
    head_im_softmax_body<KT>(MemberBits(a.members, blockIdx.y, a.n_models, a.row, a.batch), a, vec_out, vec_img);
}

// morphology + late blocking (cold path: EK = DK = 0 in every shipped config); morph_var: one window per image, 0 copies the image
__global__ __launch_bounds__(256) void morph_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                    int h, int w, int ksize, int op) {
    morph_body<false>(src, dst, h, w, ksize, op);
}
__global__ __launch_bounds__(256) void morph_var_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                        int h, int w, const int *__restrict__ ksizes, int op) {
    morph_body<true>(src, dst, h, w, min(__builtin_amdgcn_readfirstlane(ksizes[blockIdx.z]), 31), op);
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

__global__ __launch_bounds__(256) void block_apply_kernel(const uint8_t *__restrict__ im, uint8_t *__restrict__ img, int c,
                                                          uint8_t *__restrict__ masks, int n_masks, int hw) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    if (im[(size_t)b * hw + p] == 0) return;
    if (img)
        for (int ch = 0; ch < c; ++ch) img[((size_t)b * hw + p) * c + ch] = 0;
    if (masks)
        for (int m = 0; m < n_masks; ++m) masks[((size_t)b * n_masks + m) * hw + p] = 0;
}

}  // namespace

template <class Args>
static size_t head_im_lds(const Args &a) {
    if (a.softmax) return 0;      // weights live in registers (HeadMfma)
    return (size_t)a.n_models * (a.K * a.cs + a.K + 2 * a.cs) * sizeof(float);
}

bool imk_head_im_supported(const ImkHeadImArgs &a) {
    if (a.n_models < 1 || a.n_models > IMK_HEAD_IM_MAX_MODELS) return false;
    if (a.softmax ? a.K > 64 : a.K > 4) return false;
    if (a.cs != 8 && a.cs != 16 && a.cs != 24 && a.cs != 32) return false;
    if (a.hw % 16 != 0 || !aligned16(a.masks_out) || !aligned16(a.im_out)) return false;   // odd sizes: unfused path
    return head_im_lds(a) <= 150 * 1024;
}

bool imk_head_im_members_supported(const ImkHeadImMembersArgs &a, int max_members) {
    if (a.n_models < 1 || a.n_models > IMK_MEMBERS_MAX_POOL || max_members > IMK_HEAD_IM_MAX_MODELS) return false;
    ImkHeadImArgs s{};      // the shapes of the whole-batch kernel, one member standing for all
    s.n_models = 1; s.cin = a.cin; s.cs = a.cs; s.K = a.K; s.softmax = a.softmax; s.batch = a.batch; s.hw = a.hw;
    s.masks_out = a.masks_out; s.im_out = a.im_out;
    return imk_head_im_supported(s) && head_im_lds(a) <= 64 * 1024;
}

// the head + IM kernel of a shape, whole ensemble (ImkHeadImArgs) or per-image members (ImkHeadImMembersArgs: always run-time N)
template <class Args, int CS, int KB, int NM>
static constexpr auto head_im_sigmoid_of() {
    if constexpr (std::is_same_v<Args, ImkHeadImArgs>) return &head_im_sigmoid_kernel<CS, KB, NM>;
    else return &head_im_members_sigmoid_kernel<CS, KB>;
}
template <class Args, int KT>
static constexpr auto head_im_softmax_of() {
    if constexpr (std::is_same_v<Args, ImkHeadImArgs>) return &head_im_softmax_kernel<KT>;
    else return &head_im_members_softmax_kernel<KT>;
}

template <class Args>
static int launch_head_im(const Args &a, bool supported, hipStream_t stream) {
    constexpr bool whole = std::is_same_v<Args, ImkHeadImArgs>;
    IMK_CHECK_ARG(a.n_models > 0 && a.batch > 0 && a.hw > 0 && a.K > 0);
    IMK_CHECK_ARG(a.masks_out && a.im_out && a.im_size && (a.softmax || a.pred_size));
    IMK_CHECK_ARG(!a.img || (a.img_out && a.c > 0));
    if (!supported) return IMK_EUNSUPPORTED;
    const int nf = a.softmax ? 1 : a.K;
    IMK_HIP(hipMemsetAsync(a.im_size, 0, sizeof(int64_t) * a.batch * nf, stream));
    // softmax heads have no pred_size (include/imk.h): the buffer is not touched, as on the unfused route (imk_im_multiclass)
    if (a.pred_size && !a.softmax) IMK_HIP(hipMemsetAsync(a.pred_size, 0, sizeof(int64_t) * a.batch * nf, stream));
    if (a.softmax && a.presence) IMK_HIP(hipMemsetAsync(a.presence, 0, (size_t)a.n_models * a.batch * a.K, stream));
    const size_t lds = head_im_lds(a);
    const int chunk = a.softmax ? MC_CHUNK : BIN_CHUNK;
    const int vec_img2 = a.img && ((int64_t)a.hw * a.c % 16 == 0) && (chunk * a.c % 16 == 0) && aligned16(a.img) && aligned16(a.img_out);
    const dim3 grid(imk_cdiv(a.hw, chunk), a.batch);
    // algorithmic bytes: N last activations + image read, image + label map(s) + IM written
    std::optional<ImkProfScope> prof;
    if (whole) prof.emplace(PF_IM, (double)a.batch * a.hw * ((double)a.n_models * a.cs * 2 + (a.img ? 2.0 * a.c : 0.0) + nf + 1), stream);
#define IMK_HIM_LAUNCH(KERN)                                                                                                \
    do {                                                                                                                    \
        if (whole && lds > 64 * 1024)      /* the members kernels stay within 64 KiB (imk_head_im_members_supported) */       \
            IMK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        imk_klaunch(KERN, dim3(grid), dim3(256), lds, stream, a, 1, vec_img2);                                              \
    } while (0)
    if (a.softmax) {
        switch ((a.K + 15) / 16) {
            case 1: IMK_HIM_LAUNCH((head_im_softmax_of<Args, 1>())); break;
            case 2: IMK_HIM_LAUNCH((head_im_softmax_of<Args, 2>())); break;
            case 3: IMK_HIM_LAUNCH((head_im_softmax_of<Args, 3>())); break;
            default: IMK_HIM_LAUNCH((head_im_softmax_of<Args, 4>())); break;
        }
    } else {
        // the reference's ensembles have 2-4 members: 2 and 3 get all their loads hoisted (compile-time N)
        const int nm = whole ? a.n_models : 0;
#define IMK_HIM_SIG(CSV, KBV)                                                                                               \
        do {                                                                                                                \
            if (nm == 2 && CSV <= 16) IMK_HIM_LAUNCH((head_im_sigmoid_of<Args, CSV, KBV, 2>()));                            \
            else if (nm == 3 && CSV <= 8) IMK_HIM_LAUNCH((head_im_sigmoid_of<Args, CSV, KBV, 3>()));                        \
            else IMK_HIM_LAUNCH((head_im_sigmoid_of<Args, CSV, KBV, 0>()));                                                 \
        } while (0)
#define IMK_HIM_KB(CSV)                                                                                                     \
        switch (a.K) {                                                                                                      \
            case 1: IMK_HIM_SIG(CSV, 1); break;                                                                             \
            case 2: IMK_HIM_SIG(CSV, 2); break;                                                                             \
            case 3: IMK_HIM_SIG(CSV, 3); break;                                                                             \
            default: IMK_HIM_SIG(CSV, 4); break;                                                                            \
        }
        switch (a.cs) {
            case 8: IMK_HIM_KB(8); break;
            case 16: IMK_HIM_KB(16); break;
            case 24: IMK_HIM_KB(24); break;
            default: IMK_HIM_KB(32); break;
        }
#undef IMK_HIM_KB
#undef IMK_HIM_SIG
    }
#undef IMK_HIM_LAUNCH
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

int imk_launch_head_im(const ImkHeadImArgs &a, hipStream_t stream) { return launch_head_im(a, imk_head_im_supported(a), stream); }

int imk_launch_head_im_members(const ImkHeadImMembersArgs &a, int max_members, hipStream_t stream) {
    IMK_CHECK_ARG(a.members && a.row);
    return launch_head_im(a, imk_head_im_members_supported(a, max_members), stream);
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

// ---- the rule on a probability stack: members == NULL is the whole ensemble (the entry point of record for profiles: it alone
// announces its work) ----------------------------------------------------------------------------------------------------------
#define IMK_IM_LAUNCH(WHOLE, MEMBERS, GRID, LDS, STACK, ...)                                                                \
    do {                                                                                                                    \
        if (members) imk_klaunch(MEMBERS, dim3(GRID), dim3(256), LDS, stream, STACK, members, __VA_ARGS__);                 \
        else imk_klaunch(WHOLE, dim3(GRID), dim3(256), LDS, stream, STACK, __VA_ARGS__);                                    \
    } while (0)

static int im_binary_run(const float *preds, const uint32_t *members, int n_models, int batch, int h, int w, int kb,
                         float thr, int cmp_ge, const uint8_t *img, int c, int block_in, int block_out,
                         uint8_t *img_out, uint8_t *masks_out, uint8_t *im_out,
                         int64_t *im_size, int64_t *pred_size, hipStream_t stream) {
    IMK_CHECK_ARG(preds && masks_out && im_out && im_size && pred_size);
    IMK_CHECK_ARG(n_models > 0 && batch > 0 && h > 0 && w > 0 && kb > 0);
    IMK_CHECK_ARG(!img || (img_out && c > 0));
    const int64_t hw64 = (int64_t)h * w;
    IMK_CHECK_ARG(hw64 < (1ll << 30));
    const int hw = (int)hw64;
    IMK_HIP(hipMemsetAsync(im_size, 0, sizeof(int64_t) * batch * kb, stream));
    IMK_HIP(hipMemsetAsync(pred_size, 0, sizeof(int64_t) * batch * kb, stream));
    auto *ims = reinterpret_cast<unsigned long long *>(im_size);
    auto *pss = reinterpret_cast<unsigned long long *>(pred_size);
    const bool vec_ok = (hw % 4 == 0) && aligned16(preds) && (kb == 1 || kb == 3);
    // probability stack + image read, image + masks + IM written
    std::optional<ImkProfScope> prof;
    if (!members) prof.emplace(PF_IM, (double)batch * hw * ((double)n_models * kb * 4 + (img ? 2.0 * c : 0.0) + kb + 1), stream);
    if (vec_ok) {
        const int vec_out = (hw % 16 == 0) && aligned16(masks_out) && aligned16(im_out);
        const int vec_img = img && ((int64_t)hw * c % 16 == 0) && aligned16(img) && aligned16(img_out);
        dim3 grid(imk_cdiv(hw, BIN_CHUNK), batch);
        if (kb == 1)
            IMK_IM_LAUNCH(im_binary_vec<1>, im_binary_members_vec<1>, grid, 0, preds, n_models, batch, hw, thr, cmp_ge, img, c, block_in,
                          block_out, img_out, masks_out, im_out, ims, pss, vec_out, vec_img);
        else
            IMK_IM_LAUNCH(im_binary_vec<3>, im_binary_members_vec<3>, grid, 0, preds, n_models, batch, hw, thr, cmp_ge, img, c, block_in,
                          block_out, img_out, masks_out, im_out, ims, pss, vec_out, vec_img);
    } else {
        dim3 grid(imk_cdiv(hw, 256), batch);
        IMK_IM_LAUNCH(im_binary_generic, im_binary_members_generic, grid, 0, preds, n_models, batch, hw, kb, thr, cmp_ge, img, c, block_in,
                      block_out, img_out, masks_out, im_out, ims, pss);
    }
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

static int im_multiclass_run(const float *probs, const uint32_t *members, int n_models, int batch, int h, int w, int k,
                             const uint8_t *img, int c, int block_in, int block_out,
                             uint8_t *img_out, uint8_t *final_out, uint8_t *im_out,
                             int64_t *im_size, uint8_t *presence, hipStream_t stream) {
    IMK_CHECK_ARG(probs && final_out && im_out && im_size);
    IMK_CHECK_ARG(n_models > 0 && batch > 0 && h > 0 && w > 0 && k > 0);
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
    std::optional<ImkProfScope> prof;
    if (!members) prof.emplace(PF_IM, (double)batch * hw * ((double)n_models * k * 4 + (img ? 2.0 * c : 0.0) + 2), stream);
    IMK_IM_LAUNCH(im_multi_kernel, im_multi_members_kernel, grid, lds, probs, n_models, batch, hw, k, magic, img, c, block_in, block_out,
                  img_out, final_out, im_out, reinterpret_cast<unsigned long long *>(im_size), presence, vec_in, vec_out, vec_img);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
#undef IMK_IM_LAUNCH

extern "C" int imk_im_binary(const float *preds, int n_models, int batch, int h, int w, int kb,
                             float thr, int cmp_ge, const uint8_t *img, int c, int block_in, int block_out,
                             uint8_t *img_out, uint8_t *masks_out, uint8_t *im_out,
                             int64_t *im_size, int64_t *pred_size, void *stream_) {
    return im_binary_run(preds, nullptr, n_models, batch, h, w, kb, thr, cmp_ge, img, c, block_in, block_out, img_out, masks_out, im_out,
                         im_size, pred_size, (hipStream_t)stream_);
}

extern "C" int imk_im_binary_members(const float *preds, const uint32_t *members, int n_models, int batch, int h, int w, int kb,
                                     float thr, int cmp_ge, const uint8_t *img, int c, int block_in, int block_out,
                                     uint8_t *img_out, uint8_t *masks_out, uint8_t *im_out,
                                     int64_t *im_size, int64_t *pred_size, void *stream_) {
    IMK_CHECK_ARG(members && n_models <= IMK_MEMBERS_MAX_POOL && batch <= 65535);
    return im_binary_run(preds, members, n_models, batch, h, w, kb, thr, cmp_ge, img, c, block_in, block_out, img_out, masks_out, im_out,
                         im_size, pred_size, (hipStream_t)stream_);
}

extern "C" int imk_im_multiclass(const float *probs, int n_models, int batch, int h, int w, int k,
                                 const uint8_t *img, int c, int block_in, int block_out,
                                 uint8_t *img_out, uint8_t *final_out, uint8_t *im_out,
                                 int64_t *im_size, uint8_t *presence, void *stream_) {
    return im_multiclass_run(probs, nullptr, n_models, batch, h, w, k, img, c, block_in, block_out, img_out, final_out, im_out, im_size,
                             presence, (hipStream_t)stream_);
}

extern "C" int imk_im_multiclass_members(const float *probs, const uint32_t *members, int n_models, int batch, int h, int w, int k,
                                         const uint8_t *img, int c, int block_in, int block_out,
                                         uint8_t *img_out, uint8_t *final_out, uint8_t *im_out,
                                         int64_t *im_size, uint8_t *presence, void *stream_) {
    IMK_CHECK_ARG(members && n_models <= IMK_MEMBERS_MAX_POOL && batch <= 65535);
    return im_multiclass_run(probs, members, n_models, batch, h, w, k, img, c, block_in, block_out, img_out, final_out, im_out, im_size,
                             presence, (hipStream_t)stream_);
}

// ksizes == NULL: the window `ksize` for every image; else one window per image (0: copied; clamped to 31 in the kernel)
static int morph_run(const uint8_t *src, uint8_t *dst, int batch, int h, int w, int ksize, const int32_t *ksizes, int op,
                     hipStream_t stream) {
    IMK_CHECK_ARG(src && dst && src != dst && batch > 0 && h > 0 && w > 0 && (op == 0 || op == 1));
    dim3 grid(imk_cdiv(w, 64), imk_cdiv(h, 4), batch);
    if (ksizes) imk_klaunch(morph_var_kernel, dim3(grid), dim3(256), 0, stream, src, dst, h, w, ksizes, op);
    else imk_klaunch(morph_kernel, dim3(grid), dim3(256), 0, stream, src, dst, h, w, ksize, op);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_morph(const uint8_t *src, uint8_t *dst, int batch, int h, int w, int ksize, int op, void *stream_) {
    IMK_CHECK_ARG(ksize > 0 && ksize <= 31);
    return morph_run(src, dst, batch, h, w, ksize, nullptr, op, (hipStream_t)stream_);
}

extern "C" int imk_morph_var(const uint8_t *src, uint8_t *dst, int batch, int h, int w, const int32_t *ksizes, int op, void *stream_) {
    IMK_CHECK_ARG(ksizes && batch <= 65535);
    return morph_run(src, dst, batch, h, w, 0, ksizes, op, (hipStream_t)stream_);
}

extern "C" int imk_block_apply(const uint8_t *im, uint8_t *img, int c, uint8_t *masks, int n_masks,
                               int batch, int h, int w, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    IMK_CHECK_ARG(im && batch > 0 && h > 0 && w > 0);
    IMK_CHECK_ARG(!img || c > 0);
    IMK_CHECK_ARG(!masks || n_masks > 0);
    const int hw = h * w;
    dim3 grid(imk_cdiv(hw, 256), batch);
    imk_klaunch(block_apply_kernel, dim3(grid), dim3(256), 0, stream, im, img, c, masks, n_masks, hw);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_version(void) { return IMK_VERSION; }

extern "C" const char *imk_error_string(int code) {
    switch (code) {
        case IMK_OK: return "ok";
        case IMK_EINVAL: return "invalid argument";
        case IMK_EUNSUPPORTED: return "unsupported shape";
        case IMK_EWORKSPACE: return "workspace too small";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown imk error";
    }
}
