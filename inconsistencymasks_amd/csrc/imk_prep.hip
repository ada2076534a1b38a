// Data preparation for gfx950 (MI355X): the pixel rules behind the reference's 00_* / 01_* / SUIM 02_* scripts, which reach them
// through cv2.resize, cv2.cvtColor(BGR2GRAY) and cv2.threshold.  Restated from OpenCV 4's published sources (imgproc/src/resize.cpp:
// resizeGeneric_ / HResizeLinear / VResizeLinear<uchar, int, short>, ResizeAreaFastVec, resizeNN; imgproc/src/color_rgb.simd.hpp:
// RGB2Gray<uchar> with its 15-bit coefficients) -- no OpenCV is linked or was available to compare against (README, hand-off list).
//
// prep_resize_kernel: a ragged batch, one launch.  Every thread makes 4 consecutive bytes of one output row and gathers its own taps
//                     (four per value, whatever the source size: there is nothing to stage).  The word is stored as one dword where
//                     it lies whole inside the row at a 4-byte address, else byte by byte (rows of dw * c bytes need not be words).
// prep_crops_kernel:  P crops of one source as grey / thresholded / class planes, 4 output bytes per thread in the same way.
#include "imk_common.h"

namespace {

// (float)((d + 0.5) * scale - 0.5) with the product and the sum rounded on their own: OpenCV's x86 baseline has no FMA here,
// hipcc would contract the expression into one
__device__ __forceinline__ float src_coord(int d, double scale) {
    return (float)__dadd_rn(__dmul_rn((double)d + 0.5, scale), -0.5);
}

// saturate_cast<short>(v * INTER_RESIZE_COEF_SCALE): cvRound (half to even), then the int16 range
__device__ __forceinline__ int coef2048(float v) {
    const int r = __float2int_rn(v * 2048.f);
    return min(32767, max(-32768, r));
}

struct LinTap { int s0, s1, w0, w1; };

// x: taps zeroed at both borders; y: no zeroing, both rows clamped (resizeGeneric_'s xofs / yofs tables)
__device__ __forceinline__ LinTap lin_tap_x(int d, double scale, int n) {
    float f = src_coord(d, scale);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n - 1) { s = n - 1; f = 0.f; }
    return {s, min(s + 1, n - 1), coef2048(1.f - f), coef2048(f)};
}
__device__ __forceinline__ LinTap lin_tap_y(int d, double scale, int n) {
    float f = src_coord(d, scale);
    const int s = (int)floorf(f);
    f -= (float)s;
    return {min(max(s, 0), n - 1), min(max(s + 1, 0), n - 1), coef2048(1.f - f), coef2048(f)};
}

__device__ __forceinline__ int nearest_src(int d, double scale, int n) {
    const double v = floor(__dmul_rn((double)d, scale));
    return v >= (double)(n - 1) ? n - 1 : max((int)v, 0);
}

// 4 bytes at dst + e0 .. (row_end exclusive): one dword where possible
__device__ __forceinline__ void store4(uint8_t *row, int e0, int row_len, const uint8_t v[4]) {
    uint8_t *p = row + e0;
    if (e0 + 4 <= row_len && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<uint32_t *>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | ((uint32_t)v[3] << 24);
    } else {
        for (int i = 0; i < 4 && e0 + i < row_len; ++i) p[i] = v[i];
    }
}

// grid (ceil(dh * ceil(dw * c / 4) / 256), n)
template <int C>
__global__ __launch_bounds__(256) void prep_resize_kernel(const uint8_t *__restrict__ src, int64_t src_bytes,
                                                          const imk_prep_item *__restrict__ items, int dh, int dw, int interp,
                                                          int post, uint8_t *__restrict__ out) {
    const int row_len = dw * C, wpr = (row_len + 3) >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= dh * wpr) return;
    const int dy = q / wpr, e0 = (q - dy * wpr) * 4;
    const imk_prep_item it = items[blockIdx.y];
    uint8_t *row = out + ((size_t)blockIdx.y * dh + dy) * row_len;
    uint8_t v4[4] = {0, 0, 0, 0};
    const int64_t need = (int64_t)it.src_h * it.src_w * C;
    const bool ok = it.src_h > 0 && it.src_w > 0 && it.src_off >= 0 && need <= src_bytes && it.src_off <= src_bytes - need &&
                    it.x0 >= 0 && it.y0 >= 0 && it.cw > 0 && it.ch > 0 && it.cw <= it.src_w - it.x0 && it.ch <= it.src_h - it.y0;
    if (ok) {
        const size_t pitch = (size_t)it.src_w * C;
        const uint8_t *rect = src + it.src_off + (size_t)it.y0 * pitch + (size_t)it.x0 * C;
        const bool half = interp == IMK_PREP_LINEAR && it.cw == 2 * dw && it.ch == 2 * dh;
        LinTap ty = {0, 0, 0, 0};
        int ny = 0;
        if (interp == IMK_PREP_NEAREST) ny = nearest_src(dy, it.scale_y, it.ch);
        else if (!half) ty = lin_tap_y(dy, it.scale_y, it.ch);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = e0 + i;
            if (e >= row_len) break;
            const int dx = e / C, k = e - dx * C;
            int val;
            if (interp == IMK_PREP_NEAREST) {
                val = rect[(size_t)ny * pitch + (size_t)nearest_src(dx, it.scale_x, it.cw) * C + k];
            } else if (half) {
                const uint8_t *p = rect + (size_t)(2 * dy) * pitch + (size_t)(2 * dx) * C + k;
                val = (p[0] + p[C] + p[pitch] + p[pitch + C] + 2) >> 2;
            } else {
                const LinTap tx = lin_tap_x(dx, it.scale_x, it.cw);
                const uint8_t *r0 = rect + (size_t)ty.s0 * pitch + k, *r1 = rect + (size_t)ty.s1 * pitch + k;
                const int h0 = r0[(size_t)tx.s0 * C] * tx.w0 + r0[(size_t)tx.s1 * C] * tx.w1;
                const int h1 = r1[(size_t)tx.s0 * C] * tx.w0 + r1[(size_t)tx.s1 * C] * tx.w1;
                val = (((ty.w0 * (h0 >> 4)) >> 16) + ((ty.w1 * (h1 >> 4)) >> 16) + 2) >> 2;
            }
            uint8_t b = (uint8_t)val;
            if (post == IMK_PREP_LABEL_PLUS1 && b > 0) b = (uint8_t)(b + 1);
            v4[i] = b;
        }
    }
    store4(row, e0, row_len, v4);
}

struct ClassTable { uint8_t v[8]; };

// grid (ceil(ch * ceil(cw / 4) / 256), P)
template <int C>
__global__ __launch_bounds__(256) void prep_crops_kernel(const uint8_t *__restrict__ src, int h, int w,
                                                         const int32_t *__restrict__ pos, int ch, int cw, int rule,
                                                         ClassTable table, int b_first, uint8_t *__restrict__ out) {
    const int wpr = (cw + 3) >> 2;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= ch * wpr) return;
    const int cy = q / wpr, e0 = (q - cy * wpr) * 4;
    const int x0 = pos[2 * blockIdx.y], y0 = pos[2 * blockIdx.y + 1];
    uint8_t *row = out + ((size_t)blockIdx.y * ch + cy) * cw;
    uint8_t v4[4] = {0, 0, 0, 0};
    const int64_t y = (int64_t)y0 + cy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t x = (int64_t)x0 + e0 + i;
        if (e0 + i >= cw || x < 0 || x >= w || y < 0 || y >= h) continue;
        const uint8_t *p = src + ((size_t)y * w + (size_t)x) * C;
        int g;
        if (C == 1) {
            g = p[0];
        } else {
            const int r = b_first ? p[2] : p[0], gr = p[1], b = b_first ? p[0] : p[2];
            if (rule == IMK_PREP_CLASS8) g = table.v[((r >= 128) << 2) | ((gr >= 128) << 1) | (b >= 128)];
            else g = (r * 9798 + gr * 19235 + b * 3735 + 16384) >> 15;
        }
        if (rule == IMK_PREP_GRAY_THRESH) g = g > 10 ? 255 : 0;
        v4[i] = (uint8_t)g;
    }
    store4(row, e0, cw, v4);
}

}  // namespace

extern "C" int imk_prep_resize(const uint8_t *src, int64_t src_bytes, const imk_prep_item *items, int n, int c, int dh, int dw,
                               int interp, int post, uint8_t *out, void *stream_) {
    IMK_CHECK_ARG(src && items && out && src_bytes > 0 && n > 0 && dh > 0 && dw > 0 && n <= 65535);
    IMK_CHECK_ARG(interp == IMK_PREP_LINEAR || interp == IMK_PREP_NEAREST);
    IMK_CHECK_ARG(post == 0 || post == IMK_PREP_LABEL_PLUS1);
    if (c != 1 && c != 3) return IMK_EUNSUPPORTED;
    const int64_t px = (int64_t)dh * dw * c;
    IMK_CHECK_ARG(px < (1ll << 31));
    hipStream_t stream = (hipStream_t)stream_;
    const int wpr = (dw * c + 3) / 4;
    const dim3 grid((unsigned)imk_cdiv((int64_t)dh * wpr, 256), n);
    // algorithmic bytes: every output written once, four taps read per value
    ImkProfScope prof(PF_IM, 5.0 * (double)px * n, stream, 0.0);
    if (c == 1) imk_klaunch(prep_resize_kernel<1>, grid, dim3(256), 0, stream, src, src_bytes, items, dh, dw, interp, post, out);
    else imk_klaunch(prep_resize_kernel<3>, grid, dim3(256), 0, stream, src, src_bytes, items, dh, dw, interp, post, out);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

extern "C" int imk_prep_crops(const uint8_t *src, int h, int w, int c, const int32_t *pos, int n_crops, int ch, int cw, int rule,
                              const uint8_t *class_table, int b_first, uint8_t *out, void *stream_) {
    IMK_CHECK_ARG(src && pos && out && h > 0 && w > 0 && n_crops > 0 && ch > 0 && cw > 0 && n_crops <= 65535);
    IMK_CHECK_ARG(rule == IMK_PREP_GRAY || rule == IMK_PREP_GRAY_THRESH || rule == IMK_PREP_CLASS8);
    if (c != 1 && c != 3) return IMK_EUNSUPPORTED;
    if (rule == IMK_PREP_CLASS8) {
        IMK_CHECK_ARG(class_table);
        if (c != 3) return IMK_EUNSUPPORTED;
    }
    IMK_CHECK_ARG((int64_t)h * w * c < (1ll << 31) && (int64_t)ch * cw < (1ll << 31));
    hipStream_t stream = (hipStream_t)stream_;
    ClassTable table = {};
    if (class_table) for (int i = 0; i < 8; ++i) table.v[i] = class_table[i];
    const int wpr = (cw + 3) / 4;
    const dim3 grid((unsigned)imk_cdiv((int64_t)ch * wpr, 256), n_crops);
    ImkProfScope prof(PF_IM, (double)ch * cw * n_crops * (c + 1.0), stream, 0.0);
    if (c == 1) imk_klaunch(prep_crops_kernel<1>, grid, dim3(256), 0, stream, src, h, w, pos, ch, cw, rule, table, b_first, out);
    else imk_klaunch(prep_crops_kernel<3>, grid, dim3(256), 0, stream, src, h, w, pos, ch, cw, rule, table, b_first, out);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}
