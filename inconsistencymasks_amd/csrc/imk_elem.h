// Launchers of the streaming kernels in imk_elem.hip.
#pragma once
#include "imk_common.h"

// Device-resident control block of the training state (no host round trips inside a step).
struct ImkCtl {
    float loss_scale;      // dynamic loss scale (Keras LossScaleOptimizer semantics)
    float inv_loss_scale;
    int good_steps;        // consecutive finite steps since the last scale change
    int step;              // number of applied optimizer steps
    float found_inf;       // unused (the overflow flag of a step lives in its stats[1], where the all-reduce sees it)
    float pad[3];
};

int imk_launch_bn_finalize(const float *partial, int n_part, int c, int cs, double count, const float *gamma,
                           const float *beta, float *mov_mean, float *mov_var, float *scale, float *shift,
                           float *save_mean, float *save_invstd, hipStream_t stream, float momentum = 0.99f);   // Keras default momentum
int imk_bn_prep_blocks(int B, int H, int W, int cs);
int imk_launch_bn_bwd_prep(int mode, const f16 *g_direct, const f16 *g_other, const f16 *z, const float *sc,
                           const float *sh, f16 *dy_out, float *partial, int B, int H, int W, int cs, hipStream_t stream,
                           int g_other_cs = 0);   // mode 1 without g_direct: channel stride of g_other (0: cs)
int imk_launch_bn_bwd_coef(const float *partial, int n_part, int c, int cs, double count, const float *gamma,
                           const float *save_mean, const float *save_invstd, const float *inv_scale_ptr, float *coef,
                           float *dgamma, float *dbeta, float *found_inf, hipStream_t stream);
int imk_launch_head(const f16 *z, const float *sc, const float *sh, const float *w, const float *bias, int cin, int cs,
                    int K, int softmax, long long n_pix, float *probs, hipStream_t stream);
int imk_loss_blocks(long long n_pix);
// training: head (BN on load, fp32 1x1 conv, sigmoid / softmax) + loss + d(loss * scale)/d(logits), no probability tensor
int imk_launch_head_loss(const f16 *z, const float *sc, const float *sh, const float *w, const float *bias, int cin, int cs,
                         int K, int softmax, long long n_pix, const uint8_t *y, const ImkCtl *ctl, float *stats,
                         f16 *dlogit, float *loss_partial, hipStream_t stream, int y255 = 0);   // y255: targets y / 255.0f (sigmoid heads)
// softmax heads, training: head + loss + gradient of the last BatchNorm's output (+ its statistics) + the output layer's
// weight / bias gradient partials in ONE pass (imk_headf.hip); rows = workgroups = rows of every partial buffer it writes
bool imk_head_cce_fused_ok(int cs, int K, long long n_pix, int rows_cap);
int imk_head_cce_fused_rows(long long n_pix);
int imk_launch_head_cce_fused(const f16 *z, const float *sc, const float *sh, const float *w, const float *bias, int cin, int cs,
                              int K, long long n_pix, const uint8_t *y, const ImkCtl *ctl, float *stats, f16 *dy,
                              float *loss_partial, float *dystat_partial, float *wg_partial, hipStream_t stream);
// the same for sigmoid heads (mse) with 1 or 3 maps and <= 16 input channels (imk_headf.hip: head_mse_fused_kernel)
bool imk_head_mse_fused_ok(int cs, int K, long long n_pix, int rows_cap);
int imk_launch_head_mse_fused(const f16 *z, const float *sc, const float *sh, const float *w, const float *bias, int cin, int cs,
                              int K, long long n_pix, const uint8_t *y, const ImkCtl *ctl, float *stats, f16 *dy,
                              float *loss_partial, float *dystat_partial, float *wg_partial, hipStream_t stream, int y255 = 0,
                              const float *dice_coef = nullptr, int hw = 0);   // dice_coef: the Dice variant (loss kind 4), see below
// loss kind 4, the reference's dice_loss on sigmoid heads (imk_dice.hip): per-image sums (rows = imk_dice_rows(batch, hw) partial rows
// of 3 floats per image; sets stats[1..3] like head_loss_kernel), then the images' coefficients coef [batch][2], their Dice values
// dice [batch] and stats[0] = the loss, then the fp16 logit gradient in head_loss_kernel's layout (or imk_launch_head_mse_fused with
// dice_coef where imk_head_mse_fused_ok)
int imk_dice_rows(int batch, int hw);
int imk_launch_dice_sums(const f16 *z, const float *sc, const float *sh, const float *w, const float *bias, int cin, int cs, int K,
                         int batch, int hw, const uint8_t *y, const ImkCtl *ctl, float *stats, float *partial, hipStream_t stream);
int imk_launch_dice_coef(const float *partial, int batch, int hw, float *coef, double *dice, float *stats, hipStream_t stream);
int imk_launch_dice_dlogit(const f16 *z, const float *sc, const float *sh, const float *w, const float *bias, int cin, int cs, int K,
                           long long n_pix, int hw, const uint8_t *y, const ImkCtl *ctl, const float *coef, f16 *dlogit,
                           hipStream_t stream);
// loss kind 3 (the reference's rmse = sqrt(mse)), behind the mse step's loss finalize: every gradient is linear in the head's logit
// gradient, so grads[i] *= 0.5f / sqrtf(mse) and stats[0] = sqrtf(mse); mse == 0 sets the overflow flag stats[1] (the step is skipped)
int imk_launch_rmse_scale(const float *loss_partial, long long n_pix, int K, float *grads, long long n_grads, float *stats,
                          hipStream_t stream);
int imk_launch_loss_finalize(const float *loss_partial, long long n_pix, int K, int kind, float *stats, hipStream_t stream);
// consistency-loss step (imk_consist.hip): L = mean (pA - pB)^2 over two views' head outputs.  Fused (sigmoid heads, 1 or 3 maps on
// 8 / 16 padded channels): head of both views + loss + both BatchNorm-output gradients with their statistics rows + one set of
// weight-gradient rows for the output layer, imk_loss_blocks(n_pix) rows each.  Composed: both fp32 probability stacks -> both fp16
// logit gradients [n_pix][pad8(K)] + loss partials.  imk_launch_grad_add: g += g2 in one fixed order (non-finite sums set *found_inf).
bool imk_consistency_fused_ok(int cs, int K, int softmax, long long n_pix, int rows_cap);
int imk_launch_consistency_head(const f16 *zA, const f16 *zB, const float *scA, const float *shA, const float *scB,
                                const float *shB, const float *w, const float *bias, int cin, int cs, int K, long long n_pix,
                                const ImkCtl *ctl, float *stats, f16 *dyA, f16 *dyB, float *loss_partial, float *dystatA,
                                float *dystatB, float *wg_partial, hipStream_t stream);
int imk_launch_consistency_dlogit(const float *pA, const float *pB, int K, int softmax, long long n_pix, const ImkCtl *ctl,
                                  float *stats, f16 *dlogitA, f16 *dlogitB, float *loss_partial, hipStream_t stream);
int imk_launch_grad_add(float *g, const float *g2, long long n, float *found_inf, hipStream_t stream);
int imk_launch_ctl_init(ImkCtl *ctl, hipStream_t stream);
int imk_launch_adamw(float *p, float *m, float *v, const float *g, long long n, ImkCtl *ctl, const float *stats,
                     float grad_scale, float lr, float wd, float b1, float b2, float eps, hipStream_t stream);

// EvalNet (evalnet.py:24-47): concatenation of the towers' pooled BatchNorm outputs; the tail (BN + pool on load, global
// average pool, Dense + sigmoid head(s), and in training the losses, the gradient of the pooled map and the per-sample
// Dense gradients) and the batch reduction of the latter
// a_div > 1: tower A holds B / a_div images and row b of the concatenation reads image b / a_div of it (one image scored
// with a_div candidate masks: imk_evalnet_forward_candidates)
int imk_launch_concat_pool(const f16 *za, const float *sca, const float *sha, int csa, const f16 *zb, const float *scb,
                           const float *shb, int csb, int B, int Hh, int Wh, f16 *cat, hipStream_t stream, int a_div = 1);
// get_evalnet_miou_v2 (evalnet.py:96): add() of the towers' pooled BatchNorm outputs, both cs channels wide.  H, W: the size of
// the towers' last Conv1x1 outputs (the sum is H/2 x W/2, an odd last row / column dropped); a_div as above
int imk_launch_add_pool(const f16 *za, const float *sca, const float *sha, const f16 *zb, const float *scb, const float *shb,
                        int cs, int B, int H, int W, f16 *sum, hipStream_t stream, int a_div = 1);
int imk_launch_onehot(const uint8_t *cls, long long n_pix, int cs, bool div255, f16 *out, hipStream_t stream);
size_t imk_evalnet_head_partial_floats(int B, int n_heads, int K, int C);
int imk_launch_evalnet_head(const f16 *z, const float *sc, const float *sh, const float *const *w, const float *const *bias,
                            int n_heads, int K, int C, int cs, int B, int H, int W, float *out, const float *y,
                            const ImkCtl *ctl, float *stats, f16 *dP, float *partial, hipStream_t stream);
int imk_launch_evalnet_head_reduce(const float *partial, int B, int n_heads, int K, int C, const float *inv_scale_ptr,
                                   float *dw0, float *db0, float *dw1, float *db1, float *found_inf, float *stats,
                                   hipStream_t stream);

// End of an optimizer step (Keras dynamic loss scale: halve on overflow, double after 2000 consecutive finite steps;
// step counter).  Called by one thread of the weight re-packing kernel, which runs right after adamw_kernel.
__device__ __forceinline__ void imk_ctl_end_step(ImkCtl *ctl, const float *stats) {
    if (stats[1] != 0.f) {
        ctl->loss_scale = fmaxf(ctl->loss_scale * 0.5f, 1.0f);
        ctl->good_steps = 0;
    } else {
        ctl->step += 1;
        if (++ctl->good_steps >= 2000) { ctl->loss_scale *= 2.0f; ctl->good_steps = 0; }
    }
    ctl->inv_loss_scale = 1.0f / ctl->loss_scale;
}

// all BatchNorm layers of a model folded (moving statistics -> scale | shift) in one launch
#define IMK_FOLD_MAX_JOBS 32
struct ImkFoldJob { const float *gamma, *beta, *mean, *var; float *scale; int c, cs; };
struct ImkFoldJobs { ImkFoldJob j[IMK_FOLD_MAX_JOBS]; int n; };
int imk_launch_bn_fold_jobs(const ImkFoldJobs &jobs, hipStream_t stream);
