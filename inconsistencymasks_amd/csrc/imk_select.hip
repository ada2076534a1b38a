// EvalNet-ensemble selection for gfx950 (MI355X): the rule by which the reference's EvalNet-ensemble baseline picks one of the M
// candidate masks of an unlabeled image (create_training_data_for_segnet_with_ensemble_binary, functions.py:5132-5152;
// ..._with_miou_ensemble_hela, :5399-5442; ..._with_miou_ensemble_multiclass, :5531-5574), and the gather of the chosen candidate.
//   mean over the N EvalNets   fl32(fl32(p_0 + p_1) + ...) / N, the divide correctly rounded: np.mean(axis=0) of the float32 stack
//   IMK_SELECT_IOU             score = that mean of the single unit
//   IMK_SELECT_MIOU            classes whose mean detection is >= 0.5f count; score = their mean ious summed in class order (Python's
//                              sum() over np.float32: the first addend as it is), divided by their number; 0.0 if none counts
//   IMK_SELECT_CONF_GATED      the single-EvalNet rule of create_training_data_by_evalnet_miou_for_segnet_multiclass (:5649-5672): class k
//                              counts for every candidate of the image if the mean of its detection values over the image's candidates
//                              (summed in candidate order, one divide: np.mean(axis=0) of the float32 [M,K]) is >= 0.03f; score = the
//                              candidate's detection values of the counting classes summed in class order, divided by their number;
//                              0.0 if none counts.  The iou units are not read.  A kernel of its own (evalnet_select_gated_kernel).
//   best                       np.argmax: the first maximum wins, the first NaN wins;  keep = best >= (float)thr (NaN: no)
// One workgroup per (16 KB chunk of the candidate, image): every workgroup of an image evaluates the rule itself -- at most
// N * M * units = 8 * 16 * 128 floats, cache hits after the first -- and copies its chunk of the winner with 16-byte accesses.
#include "imk_kernels.h"
#include "imk_head.h"
#include <vector>

namespace {

constexpr int SEL_VEC_PER_THREAD = 4;
constexpr int SEL_CHUNK_VECS = 256 * SEL_VEC_PER_THREAD;      // 16-byte vectors a workgroup copies
constexpr int SEL_MAX_OUT = 64;                               // units per head (imk_evalnet_cfg::n_out)

__global__ __launch_bounds__(256) void evalnet_select_kernel(ImkSelectArgs a) {
    __shared__ float s_iou[IMK_SELECT_MAX_CAND * SEL_MAX_OUT], s_det[IMK_SELECT_MAX_CAND * SEL_MAX_OUT];
    __shared__ float s_score[IMK_SELECT_MAX_CAND];
    __shared__ int s_best;
    const int b = blockIdx.y, t = threadIdx.x;
    const int M = a.n_cand, K = a.n_out, U = a.n_heads * K, N = a.n_models;
    int cnt = a.counts ? a.counts[b] : M;
    cnt = cnt < 1 ? 1 : (cnt > M ? M : cnt);                  // the host refuses such counts; never index outside the image's rows
    const float fn = (float)N;
    const size_t model_stride = (size_t)a.batch * M * U;
    const float *sb = a.scores + (size_t)b * M * U;
    for (int i = t; i < cnt * K; i += 256) {                  // (candidate, class): the means over the models, in model order
        const int m = i / K, k = i - m * K;
        const float *p = sb + (size_t)m * U + k;
        float si = p[0];
        for (int n = 1; n < N; ++n) si += p[n * model_stride];
        s_iou[i] = __fdiv_rn(si, fn);
        if (a.miou) {
            float sd = p[K];
            for (int n = 1; n < N; ++n) sd += p[n * model_stride + K];
            s_det[i] = __fdiv_rn(sd, fn);
        }
    }
    __syncthreads();
    if (t < cnt) {
        float sc;
        if (!a.miou) {
            sc = s_iou[t];                                    // K == 1
        } else {
            float s = 0.f;
            int c = 0;
            for (int k = 0; k < K; ++k)
                if (s_det[t * K + k] >= 0.5f) {               // NaN compares false
                    s = c ? s + s_iou[t * K + k] : s_iou[t * K + k];
                    ++c;
                }
            sc = c ? __fdiv_rn(s, (float)c) : 0.f;
        }
        s_score[t] = sc;
    }
    __syncthreads();
    if (t == 0) {
        float bv = 0.f;
        int bk = -1;
        for (int m = 0; m < cnt; ++m) np_argmax_step(s_score[m], m, bv, bk);
        s_best = bk;
        if (blockIdx.x == 0) {
            a.best_idx[b] = bk;
            a.best_score[b] = bv;
            a.keep[b] = bv >= a.thr ? 1 : 0;                  // NaN compares false
        }
    }
    __syncthreads();
    const long long n_vec = a.cand_bytes / 16;
    const uint4 *src = reinterpret_cast<const uint4 *>(a.cand + ((size_t)b * M + s_best) * a.cand_bytes);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + (size_t)b * a.cand_bytes);
    const long long v0 = (long long)blockIdx.x * SEL_CHUNK_VECS + t;
    uint4 r[SEL_VEC_PER_THREAD];
#pragma unroll
    for (int j = 0; j < SEL_VEC_PER_THREAD; ++j) if (v0 + j * 256 < n_vec) r[j] = src[v0 + j * 256];
#pragma unroll
    for (int j = 0; j < SEL_VEC_PER_THREAD; ++j) if (v0 + j * 256 < n_vec) dst[v0 + j * 256] = r[j];
}

// IMK_SELECT_CONF_GATED: as above, with one reduction across the candidates of the image (the gate) between the means over the
// models and the scores.  Reads the detection units only.
__global__ __launch_bounds__(256) void evalnet_select_gated_kernel(ImkSelectArgs a) {
    __shared__ float s_det[IMK_SELECT_MAX_CAND * SEL_MAX_OUT];
    __shared__ float s_gate[SEL_MAX_OUT];
    __shared__ float s_score[IMK_SELECT_MAX_CAND];
    __shared__ int s_best;
    const int b = blockIdx.y, t = threadIdx.x;
    const int M = a.n_cand, K = a.n_out, U = 2 * K, N = a.n_models;
    int cnt = a.counts ? a.counts[b] : M;
    cnt = cnt < 1 ? 1 : (cnt > M ? M : cnt);                  // the host refuses such counts; never index outside the image's rows
    const float fn = (float)N;
    const size_t model_stride = (size_t)a.batch * M * U;
    const float *sb = a.scores + (size_t)b * M * U + K;       // the detection units follow the K iou units
    for (int i = t; i < cnt * K; i += 256) {                  // (candidate, class): the means over the models, in model order
        const int m = i / K, k = i - m * K;
        const float *p = sb + (size_t)m * U + k;
        float sd = p[0];
        for (int n = 1; n < N; ++n) sd += p[n * model_stride];
        s_det[i] = __fdiv_rn(sd, fn);
    }
    __syncthreads();
    if (t < K) {                                              // the gate: the class's mean over the image's candidates, in candidate order
        float g = s_det[t];
        for (int m = 1; m < cnt; ++m) g += s_det[m * K + t];
        s_gate[t] = __fdiv_rn(g, (float)cnt);
    }
    __syncthreads();
    if (t < cnt) {
        float s = 0.f;
        int c = 0;
        for (int k = 0; k < K; ++k)
            if (s_gate[k] >= 0.03f) {                         // NaN compares false
                s = c ? s + s_det[t * K + k] : s_det[t * K + k];
                ++c;
            }
        s_score[t] = c ? __fdiv_rn(s, (float)c) : 0.f;
    }
    __syncthreads();
    if (t == 0) {
        float bv = 0.f;
        int bk = -1;
        for (int m = 0; m < cnt; ++m) np_argmax_step(s_score[m], m, bv, bk);
        s_best = bk;
        if (blockIdx.x == 0) {
            a.best_idx[b] = bk;
            a.best_score[b] = bv;
            a.keep[b] = bv >= a.thr ? 1 : 0;                  // NaN compares false
        }
    }
    __syncthreads();
    const long long n_vec = a.cand_bytes / 16;
    const uint4 *src = reinterpret_cast<const uint4 *>(a.cand + ((size_t)b * M + s_best) * a.cand_bytes);
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + (size_t)b * a.cand_bytes);
    const long long v0 = (long long)blockIdx.x * SEL_CHUNK_VECS + t;
    uint4 r[SEL_VEC_PER_THREAD];
#pragma unroll
    for (int j = 0; j < SEL_VEC_PER_THREAD; ++j) if (v0 + j * 256 < n_vec) r[j] = src[v0 + j * 256];
#pragma unroll
    for (int j = 0; j < SEL_VEC_PER_THREAD; ++j) if (v0 + j * 256 < n_vec) dst[v0 + j * 256] = r[j];
}

// [B][n_vec] -> [B][n_rep][n_vec]: one load, n_rep stores per vector
template <typename V>
__global__ __launch_bounds__(256) void repeat_rows_kernel(const V *__restrict__ src, long long n_vec, int n_rep, V *__restrict__ dst) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vec) return;
    const int b = blockIdx.y;
    const V v = src[(size_t)b * n_vec + i];
    for (int r = 0; r < n_rep; ++r) dst[((size_t)b * n_rep + r) * n_vec + i] = v;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int imk_launch_evalnet_select(const ImkSelectArgs &a, hipStream_t stream) {
    const long long n_vec = a.cand_bytes / 16;
    const dim3 grid((unsigned)((n_vec + SEL_CHUNK_VECS - 1) / SEL_CHUNK_VECS), a.batch);
    ImkProfScope prof(PF_IM, (double)a.batch * (2.0 * a.cand_bytes + 4.0 * a.n_models * a.n_cand * a.n_heads * a.n_out), stream);
    if (a.gated) imk_klaunch(evalnet_select_gated_kernel, grid, dim3(256), 0, stream, a);
    else imk_klaunch(evalnet_select_kernel, grid, dim3(256), 0, stream, a);
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

int imk_launch_repeat_rows(const uint8_t *src, int batch, int n_rep, long long row_bytes, uint8_t *dst, hipStream_t stream) {
    IMK_CHECK_ARG(src && dst && batch > 0 && batch <= 65535 && n_rep > 0 && row_bytes > 0 && row_bytes % 4 == 0);
    if (row_bytes % 16 == 0 && aligned16(src) && aligned16(dst)) {
        const long long n = row_bytes / 16;
        imk_klaunch(repeat_rows_kernel<uint4>, dim3((unsigned)((n + 255) / 256), batch), dim3(256), 0, stream,
                    reinterpret_cast<const uint4 *>(src), n, n_rep, reinterpret_cast<uint4 *>(dst));
    } else {
        IMK_CHECK_ARG((reinterpret_cast<uintptr_t>(src) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0);
        const long long n = row_bytes / 4;
        imk_klaunch(repeat_rows_kernel<uint32_t>, dim3((unsigned)((n + 255) / 256), batch), dim3(256), 0, stream,
                    reinterpret_cast<const uint32_t *>(src), n, n_rep, reinterpret_cast<uint32_t *>(dst));
    }
    IMK_LAUNCH_CHECK();
    return IMK_OK;
}

// the argument rules of imk_evalnet_select, shared with imk_evalnet_forward_select (imk_evalnet.hip)
int imk_select_check(int n_models, int batch, int n_cand, int n_heads, int n_out, const int32_t *counts, const uint8_t *cand,
                     int64_t cand_bytes, int mode, const uint8_t *out, hipStream_t stream) {
    IMK_CHECK_ARG(n_models > 0 && batch > 0 && n_cand > 0 && n_out > 0 && cand && out);
    IMK_CHECK_ARG(mode == IMK_SELECT_IOU || mode == IMK_SELECT_MIOU || mode == IMK_SELECT_CONF_GATED);
    IMK_CHECK_ARG(mode == IMK_SELECT_IOU ? (n_heads == 1 && n_out == 1) : n_heads == 2);
    IMK_CHECK_ARG(cand_bytes > 0 && cand_bytes % 16 == 0 && aligned16(cand) && aligned16(out));
    if (n_models > IMK_SELECT_MAX_MODELS || n_cand > IMK_SELECT_MAX_CAND || n_out > SEL_MAX_OUT || batch > 65535) return IMK_EUNSUPPORTED;
    if (counts) {     // device memory: read back before anything is launched
        std::vector<int32_t> h(batch);
        IMK_HIP(hipMemcpyAsync(h.data(), counts, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, stream));
        IMK_HIP(hipStreamSynchronize(stream));
        for (int32_t c : h) IMK_CHECK_ARG(c >= 1 && c <= n_cand);
    }
    return IMK_OK;
}

extern "C" int imk_evalnet_select(const float *scores, int n_models, int batch, int n_cand, int n_heads, int n_out,
                                  const int32_t *counts, const uint8_t *cand, int64_t cand_bytes, double thr, int mode,
                                  int32_t *best_idx, float *best_score, uint8_t *keep, uint8_t *out, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    IMK_CHECK_ARG(scores && best_idx && best_score && keep);
    int rc = imk_select_check(n_models, batch, n_cand, n_heads, n_out, counts, cand, cand_bytes, mode, out, stream);
    if (rc) return rc;
    const ImkSelectArgs a{scores, counts, cand, n_models, batch, n_cand, n_heads, n_out, mode == IMK_SELECT_MIOU, cand_bytes,
                          (float)thr, best_idx, best_score, keep, out, mode == IMK_SELECT_CONF_GATED};
    return imk_launch_evalnet_select(a, stream);
}
