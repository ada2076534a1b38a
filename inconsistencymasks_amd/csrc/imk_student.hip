// Noisy-Student baseline for gfx950 (MI355X): the teacher's label pass of create_pseudo_labels_noisy_student_* (functions.py:
// 3243-3417).  The reference predicts on the un-augmented image, labels it (p > 0.5 / p >= 0.5 / np.argmax) and then moves image
// and label with ONE draw of flips / quarter turn (augment_image_and_mask, :2779-2826).  Here the label is born in the moved frame:
//
// student_sigmoid_kernel:  the last decoder activations of the teacher -> head_sigmoid(head_logit) exactly as imk_unet_forward's
//                          head (imk_head.h) -> threshold -> masks [B,K,H,W] {0,255} at the pixel the image's pixel moves to.
// student_softmax_kernel:  the same with the matrix-core softmax head (HeadMfma::probs) and np.argmax -> class ids [B,H,W].
// move_planes_kernel:      the geometry alone on planar label maps (the unfused route of sigmoid heads with several maps).
//
// Form: one thread per OUTPUT pixel, gathering the 16..64-byte fp16 activation row of its source pixel (imk_pixmap.h), because the
// label is one byte per pixel and the activation 16..64: a scatter by source pixel would write single bytes H apart under a quarter
// turn, while the gather keeps every store a full dword (sigmoid: 4 pixels of a row per thread, 64 contiguous bytes per 16 lanes)
// or a 16-byte store from LDS (softmax), and its reads stay whole activation rows -- at least 16 contiguous bytes each, and under
// flips alone 64 neighbouring pixels of one image row per wave, ascending or descending.  A sigmoid workgroup covers a 64 x 16
// output tile, so under a quarter turn it reads a 16 x 64 source tile: 16 neighbouring pixels (256 B .. 1 KiB) per source row.
// The softmax head's lane map (lane = pixel p16 of a 16-pixel unit x channel group g, imk_head.h) loads 16 bytes per lane from any
// pixel already, so the gather costs it nothing but the address.
#include "imk_common.h"
#include "imk_head.h"
#include "imk_pixmap.h"

namespace {

template <bool GE>
__device__ __forceinline__ bool label_cmp(float p, float thr) { return GE ? p >= thr : p > thr; }     // NaN -> 0 under both

// grid (ceil(W / 64), ceil(H / 16), B), 256 threads: thread t labels the output pixels (y0 + t / 16, x0 + 4 (t % 16) .. + 3)
template <int CS, int KB, bool GE>
__global__ __launch_bounds__(256) void student_sigmoid_kernel(ImkStudentArgs a) {
    __shared__ float s_w[KB * CS + KB + 2 * CS];
    const int t = threadIdx.x, b = blockIdx.z, H = a.h, W = a.w;
    head_stage<CS>(a.wt, a.bias, a.sc, a.sh, a.cin, KB, s_w);
    __syncthreads();
    const imk_aug_params q = a.aug[b];
    const int yo = blockIdx.y * 16 + (t >> 4), xo0 = blockIdx.x * 64 + (t & 15) * 4;
    if (yo >= H || xo0 >= W) return;
    uint32_t word[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) word[k] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (xo0 + i >= W) break;
        int ys, xs;
        imk_aug_src(q.flip_v, q.flip_h, q.rot, H, W, yo, xo0 + i, ys, xs);
        float xin[CS];
        head_input<CS>(a.z, ((long long)b * H + ys) * W + xs, s_w, KB, xin);
#pragma unroll
        for (int k = 0; k < KB; ++k)
            if (label_cmp<GE>(head_sigmoid(head_logit<CS>(xin, s_w, KB, k)), a.thr)) word[k] |= 0xffu << (8 * i);
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        uint8_t *dst = a.out + (((size_t)b * KB + k) * H + yo) * W + xo0;
        if (xo0 + 4 <= W && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
            *reinterpret_cast<uint32_t *>(dst) = word[k];
        } else {
            for (int i = 0; i < 4 && xo0 + i < W; ++i) dst[i] = (uint8_t)(word[k] >> (8 * i));
        }
    }
}

// Flat over the B*H*W output pixels (H*W a multiple of 16: a 16-pixel unit never straddles two images).  A wave owns U units; all
// activation loads of a workgroup are issued before the first MFMA.  Labels leave through LDS as 16-byte stores.
template <int KT>
struct StudentUnits { static constexpr int U = KT == 1 ? 8 : (KT == 4 ? 4 : 5); };

template <int KT>
__global__ __launch_bounds__(256) void student_softmax_kernel(ImkStudentArgs a, long long n_pix) {
    constexpr int U = StudentUnits<KT>::U, CHUNK = 4 * U * 16;
    __shared__ __attribute__((aligned(16))) uint8_t s_out[CHUNK];
    const int K = a.K, cs = a.cs, H = a.h, W = a.w, hw = H * W;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, p16 = lane & 15, g = lane >> 4;
    const long long p_base = (long long)blockIdx.x * CHUNK;
    const int n_px = (int)(n_pix - p_base < CHUNK ? n_pix - p_base : CHUNK);     // a multiple of 16
    HeadMfma<KT> h;
    h.load(a.wt, a.bias, a.sc, a.sh, a.cin, cs, K);
    f16x8 zr[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int qi = (wave * U + u) * 16 + p16;
        const long long po = p_base + (qi < n_px ? qi : 0);
        const int b = (int)(po / hw), r = (int)(po - (long long)b * hw);
        const int yo = r / W, xo = r - yo * W;
        const imk_aug_params q = a.aug[b];
        int ys, xs;
        imk_aug_src(q.flip_v, q.flip_h, q.rot, H, W, yo, xo, ys, xs);
        zr[u] = h.load_z(a.z, (long long)b * hw + (long long)ys * W + xs, cs);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        f32x4 pr[KT];
        h.probs(zr[u], K, pr);
        const int bk = vote_argmax<KT>(pr, K);
        const int qi = (wave * U + u) * 16 + p16;
        if (g == 0 && qi < n_px) s_out[qi] = (uint8_t)bk;
    }
    __syncthreads();
    uint8_t *dst = a.out + p_base;
    for (int i = t; i < n_px / 16; i += 256) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(s_out)[i];
}

// grid (ceil(H*W / 256), B): one thread per output pixel, every plane
__global__ __launch_bounds__(256) void move_planes_kernel(const uint8_t *__restrict__ src, int P, int H, int W,
                                                          const imk_aug_params *__restrict__ aug, uint8_t *__restrict__ out) {
    const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const imk_aug_params q = aug[b];
    const int yo = p / W, xo = p - yo * W;
    int ys, xs;
    imk_aug_src(q.flip_v, q.flip_h, q.rot, H, W, yo, xo, ys, xs);
    for (int k = 0; k < P; ++k) out[((size_t)b * P + k) * H * W + p] = src[(((size_t)b * P + k) * H + ys) * W + xs];
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

bool imk_student_head_supported(const ImkStudentArgs &a) {
    if (a.softmax ? a.K > 64 : a.K > 4) return false;
    if (a.K < 1 || (a.cs != 8 && a.cs != 16 && a.cs != 24 && a.cs != 32)) return false;
    return ((long long)a.h * a.w) % 16 == 0 && aligned16(a.out) && a.batch <= 65535;
}

int imk_launch_student_head(const ImkStudentArgs &a, hipStream_t stream) {
    IMK_CHECK_ARG(a.z && a.aug && a.out && a.batch > 0 && a.h > 0 && a.w > 0);
    if (!imk_student_head_supported(a)) return IMK_EUNSUPPORTED;
    const long long n_pix = (long long)a.batch * a.h * a.w;
    const int nf = a.softmax ? 1 : a.K;
    // algorithmic bytes: the last activation read once, the label map(s) written once; flops: the output layer (2 cin K) + the rule
    ImkProfScope prof(PF_IM, (double)n_pix * ((double)a.cs * 2 + nf), stream, (double)n_pix * a.K * (2.0 * a.cin + 1.0));
    if (a.softmax) {
#define IMK_SS(KT)                                                                                                           \
    do {                                                                                                                     \
        constexpr int CHUNK = 4 * StudentUnits<KT>::U * 16;                                                                  \
        imk_klaunch(student_softmax_kernel<KT>, dim3((unsigned)((n_pix + CHUNK - 1) / CHUNK)), dim3(256), 0, stream, a, n_pix); \
    } while (0)
        switch ((a.K + 15) / 16) {
            case 1: IMK_SS(1); break;
            case 2: IMK_SS(2); break;
            case 3: IMK_SS(3); break;
            default: IMK_SS(4); break;
        }
#undef IMK_SS
        IMK_LAUNCH_CHECK();
        return IMK_OK;
    }
    const dim3 grid((a.w + 63) / 64, (a.h + 15) / 16, a.batch);
#define IMK_ST(CSV, KBV)                                                                                                     \
    do {                                                                                                                     \
        if (a.cmp_ge) imk_klaunch(student_sigmoid_kernel<CSV, KBV, true>, grid, dim3(256), 0, stream, a);                    \
        else imk_klaunch(student_sigmoid_kernel<CSV, KBV, false>, grid, dim3(256), 0, stream, a);                            \
    } while (0)
#define IMK_ST_KB(CSV)                                                                                                       \
    switch (a.K) {                                                                                                           \
        case 1: IMK_ST(CSV, 1); break;                                                                                       \
        case 2: IMK_ST(CSV, 2); break;                                                                                       \
        case 3: IMK_ST(CSV, 3); break;                                                                                       \
        default: IMK_ST(CSV, 4); break;                                                                                      \
    }
    switch (a.cs) {
        case 8: IMK_ST_KB(8); break;
        case 16: IMK_ST_KB(16); break;
        case 24: IMK_ST_KB(24); break;
        default: IMK_ST_KB(32); break;
    }
#undef IMK_ST_KB
#undef IMK_ST
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

int imk_student_move_planes(const uint8_t *src, int batch, int planes, int h, int w, const imk_aug_params *aug, uint8_t *out,
                            hipStream_t stream) {
    IMK_CHECK_ARG(src && aug && out && src != out && batch > 0 && batch <= 65535 && planes > 0 && h > 0 && w > 0);
    IMK_CHECK_ARG((int64_t)h * w < (1ll << 30));
    ImkProfScope prof(PF_IM, 2.0 * batch * planes * h * w, stream, 0.0);
    imk_klaunch(move_planes_kernel, dim3((unsigned)imk_cdiv((int64_t)h * w, 256), batch), dim3(256), 0, stream, src, planes, h, w, aug, out);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
