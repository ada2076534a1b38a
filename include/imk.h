/* imk.h -- C ABI of libimk.so: the MI355X (gfx950) implementation of the Inconsistency-Mask hot path.
 *
 * The reference (MichaelVorndran/InconsistencyMasks) is pure Python and has no FFI/plugin layer; the
 * boundary it offers for this path is a set of Python functions.  Each entry
 * point below names the reference call site(s) whose arithmetic it replaces (file:line relative to the
 * reference checkout).  The Python host layer (inconsistencymasks_amd/) binds these with ctypes and
 * presents the reference's own function names on top (functions.py / unet.py mirrors).
 *
 * Conventions (all entry points):
 *   - return 0 on success, a negative IMK_E* code for bad arguments, a positive value = hipError_t;
 *   - never throw, never allocate or free caller memory, never synchronise: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream) and the caller owns every buffer until
 *     it has synchronised that stream;
 *   - all pointers are DEVICE pointers unless a parameter says "host";
 *   - compute entry points keep no mutable global state; a PLAN owns its fork / join events, so one plan must not be
 *     driven from two host threads at the same time (use one plan per thread; plans are cheap).  The side streams the
 *     training step and the ensemble forward fork onto are created once per device and shared by every plan of the
 *     process (more streams than the runtime has hardware queues serialise behind each other); they are never destroyed.
 *     The debug switches at the end of this file act on ONE plan (imk_unet_plan_debug); the measurement context
 *     (imk_prof_*) is created and owned by the caller and bound to the launching thread.
 *   - images and masks are uint8, NHWC; probabilities float32 NHWC; sizes int64.
 *
 * Buffers (all entry points; tests/test_gpu_buffer_contract.py holds every one of them to this with guard bands and poison fills):
 *   - what workspaces and outputs hold on entry is arbitrary: the library initialises what it needs on `stream` inside the call
 *     (counters, sums, tile schedules), and no result depends on what a workspace or an output held before -- a workspace may be
 *     shared between calls on one stream and need never be cleared;
 *   - nothing outside [ptr, ptr + bytes) of any argument is written, where bytes is the size this header gives for the argument
 *     (for workspaces, packed weights and optimizer state: what the matching *_bytes query returns);
 *   - `const` arguments are not modified;
 *   - every byte of an output is written, except where an output is stated to be unused on a route: such a buffer is not touched
 *     and may be NULL;
 *   - a workspace smaller than the call needs is refused with IMK_EWORKSPACE before anything is launched or written.
 *
 * Streams (all entry points; tests/test_gpu_stream_order.py holds the six that fork to this with skewed streams and poison fills):
 *   - every call leaves all of its work, including work on the pool's side streams, ordered after prior work on `stream` and
 *     before later work on `stream`: what the caller enqueued on `stream` before the call is visible to every kernel of the call, and
 *     what it enqueues on `stream` behind the call (reading an output, overwriting an input or the workspace) sees the call finished.
 */
#ifndef IMK_H
#define IMK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMK_VERSION 100 /* 0.1.0 */

/* libimk.so is built with -fvisibility=hidden: only the entry points declared here are exported. */
#define IMK_API __attribute__((visibility("default")))

enum {
    IMK_OK = 0,
    IMK_EINVAL = -1,      /* null pointer / non-positive size / unsupported combination */
    IMK_EUNSUPPORTED = -2,/* shape outside what the kernels cover (e.g. more than 64 classes) */
    IMK_EWORKSPACE = -3,  /* workspace too small */
};

IMK_API int imk_version(void);
IMK_API const char *imk_error_string(int code);

/* ------------------------------------------------------------------------------------------------
 * Inconsistency-mask kernels
 * ---------------------------------------------------------------------------------------------- */

/* Binary / HeLa IM.  Replaces get_im_prediction_binary (functions.py:3140-3162: `> thr`, Kb = 1),
 * get_im_prediction_hela (functions.py:3165-3202: `>= thr`, Kb = 3, combined IM = max, size = sum),
 * pred_masks_to_im_binary (functions.py:3104-3120) and the blocking of functions.py:2867-2874, for a
 * whole batch in one launch.
 *   preds      [N,B,H,W,Kb] float32   probabilities of the N ensemble members
 *   img        [B,H,W,C] uint8 or NULL (no image blocking)
 *   img_out    [B,H,W,C] uint8 (ignored when img == NULL); = img with IM pixels zeroed if block_in
 *   masks_out  [B,Kb,H,W] uint8 {0,255}; IM pixels zeroed if block_out
 *   im_out     [B,H,W]   uint8 {0,255}  (max over the Kb channel IMs)
 *   im_size    [B,Kb] int64, pred_size [B,Kb] int64   -- counted BEFORE blocking, like the reference
 * NaN votes 0 under both comparison operators.                                                        */
IMK_API int imk_im_binary(const float *preds, int n_models, int batch, int h, int w, int kb,
                  float thr, int cmp_ge,
                  const uint8_t *img, int c, int block_in, int block_out,
                  uint8_t *img_out, uint8_t *masks_out, uint8_t *im_out,
                  int64_t *im_size, int64_t *pred_size, void *stream);

/* Multi-class IM.  Replaces get_im_prediction_multiclass (functions.py:3206-3238), pred_masks_to_im_multiclass
 * (functions.py:3123-3137) and the blocking of functions.py:3055-3062.  The arg-max is np.argmax's: the first maximum
 * wins, and a NaN counts as the maximum (the first NaN wins).
 *   probs      [N,B,H,W,K] float32, K <= 64
 *   final_out  [B,H,W] uint8 class ids (0 where the models disagree; zeroed on IM pixels if block_out --
 *              the same thing, kept for symmetry with the reference's order of operations)
 *   im_out     [B,H,W] uint8 {0,255}
 *   im_size    [B] int64
 *   presence   [N,B,K] uint8 or NULL: 1 where model n predicts class k somewhere in image b (the
 *              `np.unique` sets of functions.py:3226, for the unique-set filter of :3231-3234)        */
IMK_API int imk_im_multiclass(const float *probs, int n_models, int batch, int h, int w, int k,
                      const uint8_t *img, int c, int block_in, int block_out,
                      uint8_t *img_out, uint8_t *final_out, uint8_t *im_out,
                      int64_t *im_size, uint8_t *presence, void *stream);

/* The IM over per-image sub-ensembles of a model pool: the rule the EvalNet training-data writers of the IM++ family apply to
 * `random.sample(models, n)` per image (create_training_data_evalnet_im_binary, functions.py:3621-3640;
 * create_training_data_evalnet_miou_im_multiclass, :3826; create_training_data_evalnet_miou_im_hela, :3931-3953).  The arguments
 * of imk_im_binary / imk_im_multiclass, whose stack holds the whole pool (n_models <= 16), and
 *   members    [B] uint32: bit n set = model n of the pool votes for image b; bits at and above n_models are ignored.
 * With cnt_b the number of members of image b:
 *   binary: s = the members' votes; masks_out = 255 where s == cnt_b; IM where s != 0 and s != cnt_b; sizes before blocking;
 *   multi-class: final_out = the label where all members' arg-maxes agree, else 0 (the reference anchors on the first sampled
 *     model; agreement is symmetric, so the sampling order does not matter); presence rows of non-members are 0.
 *   cnt_b == 0: labels 0, IM 0, sizes 0, the image copied.
 * Non-members' probabilities are not read.  With every bit set the outputs equal imk_im_binary / imk_im_multiclass bit for bit.
 * batch <= 65535.                                                                                             */
IMK_API int imk_im_binary_members(const float *preds, const uint32_t *members, int n_models, int batch, int h, int w, int kb,
                  float thr, int cmp_ge,
                  const uint8_t *img, int c, int block_in, int block_out,
                  uint8_t *img_out, uint8_t *masks_out, uint8_t *im_out,
                  int64_t *im_size, int64_t *pred_size, void *stream);
IMK_API int imk_im_multiclass_members(const float *probs, const uint32_t *members, int n_models, int batch, int h, int w, int k,
                      const uint8_t *img, int c, int block_in, int block_out,
                      uint8_t *img_out, uint8_t *final_out, uint8_t *im_out,
                      int64_t *im_size, uint8_t *presence, void *stream);

/* k x k all-ones erosion (op = 0) / dilation (op = 1) of [B,H,W] uint8 masks, out-of-image taps ignored.
 * Replaces cv2.erode / cv2.dilate at functions.py:2858-2864 (dead in every shipped config: EK = DK = 0). */
IMK_API int imk_morph(const uint8_t *src, uint8_t *dst, int batch, int h, int w, int ksize, int op, void *stream);

/* imk_morph with one window per image: ksizes [B] int32 (device), image b gets a ksizes[b] x ksizes[b] window and is bit-identical
 * to imk_morph(ksize = ksizes[b]) on that image; 0 (or less) copies the image, sizes above 31 count as 31.  One launch for the
 * per-image random erosion / dilation of the writers above (functions.py:3626-3634, 3946-3954).  batch <= 65535.            */
IMK_API int imk_morph_var(const uint8_t *src, uint8_t *dst, int batch, int h, int w, const int32_t *ksizes, int op, void *stream);

/* image[im>0] = 0 (all C channels) and mask[im>0] = 0 for n_masks [B,H,W] masks packed as [B,n_masks,H,W]:
 * the blocking step of functions.py:2867-2874 when it has to run AFTER morphology changed the IM.
 * In place.  img or masks may be NULL.                                                                */
IMK_API int imk_block_apply(const uint8_t *im, uint8_t *img, int c, uint8_t *masks, int n_masks,
                    int batch, int h, int w, void *stream);

/* Model-ensemble voting: the pseudo-label rules of the model-ensemble baseline (get_model_ensemble_prediction_*,
 * functions.py:2409-2566), for a whole batch in one launch.  mode IMK_VOTE_HARD / IMK_VOTE_SOFT.
 *   preds      [N,B,H,W,Kb] float32   probabilities of the N ensemble members
 *   masks_out  [B,Kb,H,W] uint8 {0,255}
 *     hard: 255 where every model has p > (float)thr: numpy compares the float32 predictions with the Python threshold in
 *           float32 (get_model_ensemble_prediction_ISIC_2018, functions.py:2409-2435);
 *     soft: 255 where ((double)p_0 + (double)p_1 + ...) / (double)N > thr, summed in model order with an IEEE fp64 divide and
 *           compared in fp64 -- the float64 accumulator of get_model_ensemble_prediction_hela_soft (functions.py:2474-2528).
 *           thr is a double so that thresholds that are not exact in fp32 (0.3) compare as the reference's Python float does.
 *   NaN votes 0 (hard); it makes the soft average NaN, so the pixel is 0.                                              */
enum { IMK_VOTE_HARD = 0, IMK_VOTE_SOFT = 1 };
IMK_API int imk_vote_binary(const float *preds, int n_models, int batch, int h, int w, int kb, double thr, int mode,
                    uint8_t *masks_out, void *stream);

/* Multi-class model-ensemble vote.  probs [N,B,H,W,K] float32, K <= 64 -> final_out [B,H,W] uint8 class ids.
 *   hard: the label where all N arg-maxes agree, else 0 (get_model_ensemble_prediction_multiclass_hard, functions.py:2438-2469);
 *   soft: argmax_k fl32(fl32(((p_0k + p_1k) + p_2k) + ...) / N): fp32 sums in model order and a correctly rounded fp32
 *         divide, what np.mean(axis=0) of the float32 stack computes (get_model_ensemble_prediction_multiclass_soft,
 *         functions.py:2534-2566).
 * Every arg-max is np.argmax's: the first maximum wins, and a NaN counts as the maximum (the first NaN wins).             */
IMK_API int imk_vote_multiclass(const float *probs, int n_models, int batch, int h, int w, int k, int mode,
                        uint8_t *final_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Tiny U-Net (unet.py:4-67): plan, parameters, forward, fused forward+IM, training step
 * ---------------------------------------------------------------------------------------------- */

typedef struct imk_unet_cfg {
    int h, w;        /* input height / width; multiples of 16 (4 poolings); h * w < 2^24 and w < 2^16, else IMK_EUNSUPPORTED */
    int c_in;        /* image channels (1 or 3)                              */
    int n_out;       /* output maps K (unet.py:63)                           */
    int ch[5];       /* int(16a), int(32a), int(64a), int(128a), int(256a)   (unet.py:49-56) */
    int act_out;     /* 0 = sigmoid, 1 = softmax                             */
} imk_unet_cfg;

typedef struct imk_unet_plan imk_unet_plan; /* opaque, host memory (U-Net and EvalNet plans) */

/* EvalNet (evalnet.py:24-73), see the section at the end of this file */
typedef struct imk_evalnet_cfg {
    int h, w;            /* input height / width: even, >= 64 (6 poolings; odd rows / columns are dropped like Keras does);
                            h * w < 2^24 and w < 2^16, else IMK_EUNSUPPORTED */
    int ca, cb;          /* channels of input A (image) and input B (mask stack); 1..4 each, cb up to 64 with b_onehot */
    int n_out;           /* units per Dense head: 1 (get_evalnet) or inputB_channels (get_evalnet_miou) */
    int two_heads;       /* 0: one sigmoid head (evalnet.py:45); 1: 'iou' + 'detection' (evalnet.py:70-71) */
    int normalize_a, normalize_b;   /* the x/255 Lambda of each input block (evalnet.py:5-6)            */
    int ch[5];           /* int(16a), int(32a), int(64a), int(128a), int(256a)  (evalnet.py:28-41)      */
    int b_onehot;        /* 1: input B is a class-id map [B,H,W] u8, expanded on the device to the one-hot stack over cb
                            classes that the reference feeds (functions.py:4978, 5990); no x/255 on it */
} imk_evalnet_cfg;

IMK_API int imk_unet_plan_create(const imk_unet_cfg *cfg, imk_unet_plan **out);
IMK_API void imk_unet_plan_destroy(imk_unet_plan *plan);

/* Flat fp32 parameter vector.  Trainable section first (what AdamW and the gradient all-reduce see),
 * in unet.py creation order: per Conv2D kernel [kh][kw][cin][cout] (Keras HWIO) then bias [cout]; per
 * BatchNormalization gamma then beta.  Then the non-trainable section: per BN moving_mean, moving_var. */
IMK_API int imk_unet_param_count(const imk_unet_plan *plan, int64_t *total, int64_t *trainable);

typedef struct imk_layer_info {
    char name[16];   /* "in.c", "e1.c3", "e1.c1", "e1.bn", "b.c3", ..., "d6.ca", "d6.bna", ..., "out" */
    int kind;        /* 0 = conv, 1 = batch-norm */
    int ksize, cin, cout;
    int64_t off_w, off_b;         /* conv: kernel, bias;   bn: gamma, beta   (offsets in floats) */
    int64_t off_mean, off_var;    /* bn only */
} imk_layer_info;
IMK_API int imk_unet_num_layers(const imk_unet_plan *plan);
IMK_API int imk_unet_layer_info(const imk_unet_plan *plan, int idx, imk_layer_info *out);

/* fp16 copies of the conv kernels in MFMA-fragment order (forward and transposed/flipped for dgrad),
 * folded BN scale/shift.  Re-run after every change of `params`.  train = 0 folds the moving statistics
 * into scale/shift (inference); in training the batch statistics are produced by the step itself.
 * Every byte of `packed` is written (the gaps of its layout are zeroed): it is a function of `params` alone. */
IMK_API int64_t imk_unet_packed_bytes(const imk_unet_plan *plan);
IMK_API int imk_unet_pack_weights(const imk_unet_plan *plan, const float *params, void *packed, void *stream);

/* Workspace (activations, gradients, reduction scratch).  mode 0 = inference, 1 = training. */
IMK_API int64_t imk_unet_workspace_bytes(const imk_unet_plan *plan, int batch, int mode);

/* Batched inference: replaces model.predict at functions.py:3157, 3184, 3224 (and the batch-64 form at
 * :1120).  x [B,H,W,c_in] uint8 (the model divides by 255 itself, unet.py:5) -> probs [B,H,W,n_out] f32. */
IMK_API int imk_unet_forward(const imk_unet_plan *plan, const float *params, const void *packed,
                     const uint8_t *x, int batch, float *probs, void *workspace, int64_t workspace_bytes,
                     void *stream);

/* Debug/parity: after imk_unet_forward or a training step, byte offset/shape of a stored intermediate
 * inside the workspace (fp16, NHWC with the channel count padded to a multiple of 8).
 * which: 0 = conv output of layer `layer_idx` (post-ReLU, pre-BN).  Returns IMK_EINVAL if not stored. */
IMK_API int imk_unet_tensor_info(const imk_unet_plan *plan, int batch, int mode, int layer_idx, int which,
                         int64_t *byte_offset, int *h, int *w, int *c, int *c_stride);

/* Ensemble inference fused with the IM chain: N models' forward passes, then head -> threshold/argmax ->
 * agreement -> IM -> blocking in ONE kernel that reads the N last decoder activations (fp16) and never writes the
 * probability stack: the head's fp32 arithmetic is the same code as imk_unet_forward's, so the outputs are bit-identical
 * to imk_unet_forward + imk_im_binary / imk_im_multiclass.  One call = functions.py:2844-2887 minus file I/O, for a batch.
 * `params`/`packed` are arrays (host) of n_models device pointers.
 * binary heads (act_out = 0): outputs as imk_im_binary;  softmax heads: as imk_im_multiclass
 * (masks_out = final_out [B,H,W]; pred_size unused: not written on either route, may be NULL; presence optional).
 * workspace: imk_unet_forward_im_workspace_bytes(plan, n_models, B, k), 1 <= k <= min(n_models, 3): with k > 1 the models
 * run on k streams side by side (forked from and joined to `stream` with events; the call stays asynchronous), with
 * k = 1 back to back.  Shapes the fused kernel does not cover (sigmoid heads with more than 4 maps, H*W not a multiple
 * of 16, more than 8 models) and plans with the materialize debug switch take the unfused route through the fp32 probability stack
 * (n_models * align256(B*H*W*n_out*4) + k * imk_unet_workspace_bytes(plan, B, 0) bytes are enough for that one).      */
IMK_API int64_t imk_unet_forward_im_workspace_bytes(const imk_unet_plan *plan, int n_models, int batch, int n_streams);
IMK_API int imk_unet_forward_im(const imk_unet_plan *plan, int n_models,
                        const float *const *params, const void *const *packed,
                        const uint8_t *x, int batch, float thr, int cmp_ge,
                        const uint8_t *img, int block_in, int block_out,
                        uint8_t *img_out, uint8_t *masks_out, uint8_t *im_out,
                        int64_t *im_size, int64_t *pred_size, uint8_t *presence,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* imk_unet_forward_im over per-image sub-ensembles of a pool of n_models <= 16 models: image b is judged by the models whose bit
 * is set in members_host[b] (a HOST array [B], like `params` and `packed`; bits at and above n_models are ignored; the call copies
 * it into the workspace as kernel arguments: the array is the caller's again when the call returns, and nothing waits for `stream`).  Each model runs once, on the images that use it (a model nobody uses does not run), and one head + IM
 * kernel reads, for every image, its members' last decoder activations.  Outputs as imk_unet_forward_im, with the rule and the
 * `presence` layout [n_models,B,K] of imk_im_binary_members / imk_im_multiclass_members.
 * Bit-identical to imk_unet_forward per pool model + imk_im_*_members; for images that share a member set, bit-identical to
 * imk_unet_forward_im on that set (the forward does not depend on the batch an image sits in).
 * workspace: imk_unet_forward_im_members_workspace_bytes(plan, n_models, B, k), 1 <= k <= 3 concurrent streams as for
 * imk_unet_forward_im; the size for k = 1 is the least the call accepts.  Shapes the fused kernel does not cover (those of
 * imk_unet_forward_im), an image with more than 8 members and plans with the materialize debug switch take the unfused route
 * inside the same workspace: every used model on the whole batch -> fp32 stack -> imk_im_*_members.  batch <= 65535. */
IMK_API int64_t imk_unet_forward_im_members_workspace_bytes(const imk_unet_plan *plan, int n_models, int batch, int n_streams);
IMK_API int imk_unet_forward_im_members(const imk_unet_plan *plan, int n_models,
                        const float *const *params, const void *const *packed,
                        const uint8_t *x, int batch, const uint32_t *members_host, float thr, int cmp_ge,
                        const uint8_t *img, int block_in, int block_out,
                        uint8_t *img_out, uint8_t *masks_out, uint8_t *im_out,
                        int64_t *im_size, int64_t *pred_size, uint8_t *presence,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* Ensemble inference + model-ensemble vote: N models' forward passes, then head -> vote in ONE kernel that reads the N last
 * decoder activations (fp16) and writes only the uint8 labels (softmax heads: the soft sums in a wave-private LDS slab).  The per-model probabilities come from the code of
 * imk_unet_forward's head, so the outputs are bit-identical to imk_unet_forward x N + imk_vote_binary (sigmoid heads: masks_out
 * [B,K,H,W]) / imk_vote_multiclass (softmax heads: masks_out [B,H,W]; thr unused).  mode IMK_VOTE_HARD / IMK_VOTE_SOFT.
 * `params`/`packed` are arrays (host) of n_models device pointers.  Streams and workspace as imk_unet_forward_im: the workspace is
 * sized by imk_unet_forward_im_workspace_bytes(plan, n_models, B, k), 1 <= k <= min(n_models, 3) concurrent streams.  Shapes the
 * fused kernel does not cover (more than 8 models, sigmoid heads with more than 4 maps, last decoder widths other than 8, 16,
 * 24 or 32 channels, a masks_out that is not 16-byte aligned) and plans with the materialize debug switch take the unfused route
 * through the fp32 probability stack.                                                                              */
IMK_API int imk_unet_forward_vote(const imk_unet_plan *plan, int n_models,
                          const float *const *params, const void *const *packed,
                          const uint8_t *x, int batch, double thr, int mode, uint8_t *masks_out,
                          void *workspace, int64_t workspace_bytes, void *stream);

/* Training (functions.py:207-218, one step of model.fit): forward with batch statistics, loss,
 * backward, optimizer.  Split in two so that a data-parallel caller can all-reduce `grads` in between.
 *   loss_kind 0 = 'mse' on {0,1} targets y u8 [B,H,W,n_out]   (ISIC, HeLa)
 *             1 = categorical cross-entropy, y u8 [B,H,W] class ids (one-hot formed on the fly)
 *             2 = 'mse' on the continuous targets float32(y) / 255.0f (a correctly rounded divide), y u8 [B,H,W,n_out] as
 *                 parse_image_depth_map builds it (functions.py:1051-1073); sigmoid heads.  With y in {0,255} it is kind 0 with
 *                 y in {0,1}, bit for bit.
 *             3 = the reference's rmse (functions.py:36-37), sqrt(mean (p - y)^2) on the targets of kind 2: kind 2, then one launch
 *                 over the gradient vector behind the loss finalize, on `stream`: grads[i] *= 0.5f / sqrtf(mse), stats[0] =
 *                 sqrtf(mse).  A batch with mse == 0 sets the overflow flag stats[1] and is skipped by imk_unet_adamw_step (Keras'
 *                 loss-scale optimizer skips the NaN gradient TensorFlow produces there).  A rank's rmse is not the batch's: do
 *                 not average kind-3 gradients over data-parallel ranks.
 *             4 = the reference's dice_loss (functions.py:162-184, smooth = 1) on the targets of kind 0, t = float(y) (HeLa's position
 *                 plane is 0 / 3); sigmoid heads only, a softmax plan is an argument error.  Per image b of the batch, over its
 *                 H*W*n_out elements: I_b = sum t p, U_b = sum t + sum p, dice_b = (2 I_b + 1) / (U_b + 1), loss = 1 - mean_b dice_b,
 *                 d loss / d p = c0_b - c1_b t with c0_b = (2 I_b + 1) / (B (U_b + 1)^2), c1_b = 2 / (B (U_b + 1)).  Three launches
 *                 in order on `stream`: the per-image sums (fp32 per thread, fixed-order partial rows in the workspace), one
 *                 workgroup that adds them in double and writes the coefficients and stats[0], and the gradient pass, which
 *                 recomputes the probabilities (no atomics: bit-reproducible; nothing depends on what the workspace held).  The
 *                 gradient pass is one fused kernel for 8 padded channels and 1 map; IMK_DICE_FUSED=0 forces the general route
 *                 (logit gradient, then the output layer's dgrad).  Every rank's loss is a mean over its own images: with equal
 *                 batch sizes, averaging kind-4 gradients over data-parallel ranks is the batch's gradient.
 *   grads     [trainable] float32, UNSCALED gradient of the mean loss
 *   stats     device float[4]: {loss, found_inf (0/1), loss_scale used, reserved}
 *   state     device buffer of imk_unet_state_bytes(): Adam m, v, step counter, dynamic loss scale
 * imk_unet_fwd_bwd also updates the BN moving statistics in `params` (momentum 0.99).                  */
IMK_API int64_t imk_unet_state_bytes(const imk_unet_plan *plan);
IMK_API int imk_unet_state_init(const imk_unet_plan *plan, void *state, void *stream);
IMK_API int imk_unet_fwd_bwd(const imk_unet_plan *plan, float *params, void *packed, void *state,
                     const uint8_t *x, const uint8_t *y, int batch, int loss_kind,
                     float *grads, float *stats, void *workspace, int64_t workspace_bytes, void *stream);

/* tensorflow_addons AdamW (functions.py:215): var -= wd*var; Adam(b1,b2,eps) with bias-corrected lr.
 * Skips the update (and halves the dynamic loss scale) when stats[1] != 0; re-packs the conv weights for the next
 * training step.  It does NOT refresh the folded inference BatchNorm statistics (training never reads them):
 * call imk_unet_pack_weights before the next imk_unet_forward / imk_unet_forward_im.
 * grad_scale multiplies grads first (1/world_size after a sum all-reduce).                            */
IMK_API int imk_unet_adamw_step(const imk_unet_plan *plan, float *params, void *packed, void *state,
                        const float *grads, const float *stats, float grad_scale,
                        float lr, float wd, float beta1, float beta2, float eps, void *stream);

/* Consistency-loss step (functions.py:367-474 of the reference; the unlabelled half of an epoch of the consistency-loss
 * baseline): x1, x2 u8 [B,H,W,c_in] are two views of one unlabelled batch (imk_views with two views); both forwards run in training
 * mode, each BatchNorm normalising with the statistics of its own view's batch, and the moving statistics in `params` move twice,
 * view 1 first.  L = mean over B*H*W*n_out of (p1 - p2)^2 on the fp32 outputs of the sigmoid / softmax head, the gradient taken
 * through both forwards (and through the softmax).  grads, stats, state: as imk_unet_fwd_bwd, stats[0] = L; follow with
 * imk_unet_adamw_step, so that labelled and consistency steps share Adam's slots, the step counter and the dynamic loss scale
 * (the fp16 gradient tensors carry the state's loss scale; an overflowing step is skipped like a labelled one).
 * Order on `stream`: forward of view 1, forward of view 2, the consistency head, backward of view 1 into `grads`, backward of
 * view 2 into a second vector inside the workspace, one fixed-order grads += second.  No float atomics: bit-reproducible.
 * Sigmoid heads with 1 or 3 maps on a last decoder width of 8 or 16 (padded) channels take one fused head kernel that reads both
 * last activations once; every other shape, plans with the materialize debug switch and IMK_CONSISTENCY_FUSED=0 take the composed
 * route (both fp32 probability stacks -> both logit gradients -> the labelled step's head dgrad per view).
 * workspace: imk_unet_consistency_workspace_bytes(plan, B) = two training workspaces, the second gradient vector and the head's
 * scratch; view v's training workspace starts at byte v * imk_unet_workspace_bytes(plan, B, 1), so imk_unet_tensor_info(mode 1)
 * offsets are valid relative to that.                                                                                   */
IMK_API int64_t imk_unet_consistency_workspace_bytes(const imk_unet_plan *plan, int batch);
IMK_API int imk_unet_consistency_fwd_bwd(const imk_unet_plan *plan, float *params, void *packed, void *state,
                                 const uint8_t *x1, const uint8_t *x2, int batch,
                                 float *grads, float *stats, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Noisy-Student augmentation (IM+ / AIM+ drivers)
 * ---------------------------------------------------------------------------------------------- */
typedef struct imk_aug_params {   /* one per image, device array */
    int flip_v, flip_h;           /* cv2.flip(.., 0) / cv2.flip(.., 1)                (functions.py:2796-2803) */
    int rot;                      /* 0 none, 1 = 90 CW, 2 = 180, 3 = 90 CCW           (functions.py:2805-2818) */
    int bright_on;                /* apply convertScaleAbs(alpha, beta)               (functions.py:2820-2824) */
    float alpha, beta;
    int blur_k;                   /* 0/1 none, 3, 5, 7: GaussianBlur((k,k), 0)        (functions.py:1495-1501) */
    int noise_max;                /* uniform integer noise in [-m, m), then clip      (functions.py:1463-1478) */
    uint32_t seed;                /* per-image seed of the counter-based noise generator */
} imk_aug_params;

/* Epoch assembly of a training set that lives in HBM: row r of the outputs = row idx[r] of the inputs -- the shuffle + batch of
 * the reference's tf.data pipeline (functions.py:207-209) with the mask normalisation of its parsers folded in
 * (parse_image_ISIC_2018: mask / 255, functions.py:975; parse_image_hela: / 255 and position x Position_weight,
 * functions.py:1001-1011).
 *   img   [n_src, row_img] uint8 (any layout; a row is copied as it is)            -> img_out  [n, row_img]     (img may be NULL)
 *   mask  [n_src, planes, hw] uint8, planar (as imk_im_binary / imk_unet_forward_im write label maps)
 *                                                                                   -> mask_out [n, hw, planes], interleaved,
 *         every value v -> (div255 ? v / 255 : v) * (mul ? mul[plane] : 1)  (mul: device, [planes])   (mask may be NULL)
 *   idx   device, int64 [n]; n <= 65535.  Outputs must not alias inputs. */
IMK_API int imk_gather_pairs(const uint8_t *img, int64_t row_img, const uint8_t *mask, int planes, int64_t hw, int div255,
                             const uint8_t *mul, const int64_t *idx, int64_t n, uint8_t *img_out, uint8_t *mask_out,
                             void *stream);

/* Replaces augment_image_and_mask (functions.py:2779-2826) + add_noise_and_blur (:1481-1506) for a batch.
 *   img  [B,H,W,C] u8 -> img_out;  mask [B,H,W,Cm] u8 (or NULL) -> mask_out (geometric part only).
 * 90-degree turns need h == w (set any_quarter_turn if any params[i].rot is 1 or 3).  Not in place. */
IMK_API int imk_augment(const uint8_t *img, const uint8_t *mask, int batch, int h, int w, int c, int cm,
                const imk_aug_params *params, uint8_t *img_out, uint8_t *mask_out, int any_quarter_turn, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Input-ensemble baseline: one model voting with itself over augmented views of each image
 * (get_input_ensemble_prediction_*, functions.py:1409-1459, 1570-1764, 2127-2407)
 * ---------------------------------------------------------------------------------------------- */
#define IMK_VIEWS_MAX 16          /* views per image the fused and unfused view votes take (the 13-view form fits) */
typedef struct imk_view_params {  /* one per (view, image), device array [M][B] */
    int op;                       /* D4 op: 0 identity, 1..12 = 1 + 6 fh + 3 fv + (rot - 1), the order of
                                     generate_random_transformations (functions.py:1675-1726): fh = cv2.flip(., 0),
                                     fv = cv2.flip(., 1), rot 1 = 90 CW, 2 = 180, 3 = 90 CCW, applied in that order */
    int blur_k;                   /* 0/1 none, 3, 5, 7: GaussianBlur((k,k), 0)        (functions.py:1494-1501) */
    int noise_max;                /* uniform integer noise in [-m, m), then clip      (functions.py:1463-1478) */
    uint32_t seed;                /* seed of the counter-based noise generator (imk_augment's) */
    int bright_on;                /* convertScaleAbs(alpha, beta)                     (functions.py:1589-1593) */
    float alpha, beta;
} imk_view_params;

/* M views per image: img [B,H,W,C] u8 -> views_out [M,B,H,W,C] u8 (member-major), each
 * geometry(op) -> blur -> noise -> brightness (data_augmentation_image, functions.py:1570-1594), with imk_augment's pixel
 * arithmetic.  chain = 0: every view is made from the image (ISIC); chain = 1: view m is made from view m-1 and view 0 from the
 * image (the HeLa / multi-class loops), as M dependent launches.  Quarter turns need h == w (set any_quarter_turn if any op is
 * a quarter turn), else IMK_EUNSUPPORTED.  Not in place. */
IMK_API int imk_views(const uint8_t *img, int batch, int h, int w, int c, int n_views, const imk_view_params *params,
                      int chain, int any_quarter_turn, uint8_t *views_out, void *stream);

/* The D4-restoring hard vote on an fp32 stack.  preds [M,B,H,W,K] float32 (views of image b at rows m*B + b), ops device int32
 * [M,B] (NULL: identity) -> masks_out [B,K,H,W] {0,255}: 255 where every view, read at the pixel its op moved (y, x) to, has
 * p >= (float)thr (cmp_ge = 1, the ISIC rule) or p > (float)thr (cmp_ge = 0).  NaN votes 0.  Quarter turns need h == w. */
IMK_API int imk_vote_views_binary(const float *preds, int n_views, int batch, int h, int w, int k, const int *ops,
                                  int any_quarter_turn, double thr, int cmp_ge, uint8_t *masks_out, void *stream);

/* The majority of the per-view arg-maxes (get_input_ensemble_prediction_multiclass, functions.py:2182-2218): np.argmax per view
 * (the first maximum; the first NaN wins), then np.argmax(np.bincount(.)), so ties go to the smallest label.
 * probs [M,B,H,W,K] float32, M <= IMK_VIEWS_MAX -> final_out [B,H,W] u8. */
IMK_API int imk_vote_views_majority(const float *probs, int n_views, int batch, int h, int w, int k, uint8_t *final_out,
                                    void *stream);

enum { IMK_VOTE_MAJORITY = 2 };
/* One model's forward over the B*M views [M,B,H,W,C] as one batch, then the input-ensemble vote -> masks_out:
 *   sigmoid head, ops != NULL:  the D4-restoring hard vote of imk_vote_views_binary (mode IMK_VOTE_HARD), fused with the head
 *                               for M <= IMK_VIEWS_MAX, K <= 4 and last decoder widths 8/16/24/32;
 *   sigmoid head, ops == NULL:  imk_vote_binary's rules (mode IMK_VOTE_HARD: p > thr; IMK_VOTE_SOFT: the fp64 mean), fused
 *                               through the model-ensemble head kernel with every member's weights the same;
 *   softmax head:               IMK_VOTE_SOFT (argmax of the fp32 mean, fused likewise) or IMK_VOTE_MAJORITY.
 * Outputs are bit-identical to imk_unet_forward over the views + imk_vote_views_binary / imk_vote_binary / imk_vote_multiclass /
 * imk_vote_views_majority, which is the route for the shapes the fused kernels do not cover: there the forwards run per view
 * and image chunk so that the fp32 stack of the whole batch is never held.  The workspace is sized by
 * imk_unet_forward_views_vote_workspace_bytes(plan, M, B).  A smaller one is accepted down to
 * align256(M*H*W*n_out*4) + imk_unet_workspace_bytes(plan, 1, 0): the call then takes the unfused route in image chunks that fit
 * (one image per chunk at that size), with the same outputs; below that, IMK_EWORKSPACE. */
IMK_API int64_t imk_unet_forward_views_vote_workspace_bytes(const imk_unet_plan *plan, int n_views, int batch);
IMK_API int imk_unet_forward_views_vote(const imk_unet_plan *plan, const float *params, const void *packed,
                                        const uint8_t *views, int n_views, int batch, const int *ops, int any_quarter_turn,
                                        double thr, int mode, int cmp_ge, uint8_t *masks_out, void *workspace,
                                        int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Noisy-student baseline: the teacher labels an image, then image and label take the same flips / turn
 * (create_pseudo_labels_noisy_student_*, functions.py:3243-3417; augment_image_and_mask(s), :2725-2826)
 * ---------------------------------------------------------------------------------------------- */
/* One call = predict, label and augment for a batch:
 *   x   [B,H,W,C] u8: what the model is fed;   img [B,H,W,C] u8: what is augmented and written (ISIC: the BGR copy)
 *   aug device imk_aug_params[B]: image i and its label take aug[i]'s flip_v / flip_h / rot, the image alone the rest
 *   img_out    [B,H,W,C] u8 = imk_augment(img) (image path)
 *   labels_out sigmoid head: [B,K,H,W] {0,255}, 255 where p > thr (cmp_ge = 0) or p >= thr (cmp_ge = 1), NaN -> 0;
 *              softmax head: [B,H,W] class ids by np.argmax's rule (the first maximum; the first NaN wins)
 *              -- both at the pixel the image's pixel moved to; p are the bits imk_unet_forward writes.
 * Sigmoid heads with K <= 4 and softmax heads with K <= 64, last decoder widths 8/16/24/32 and H*W a multiple of 16 take one
 * fused head + label kernel (no fp32 probabilities, no un-moved label) with the image path on a side stream, forked from and
 * joined to `stream`; the other shapes and imk_unet_plan_debug(materialize) take imk_unet_forward -> label -> imk_augment on
 * `stream`, with bit-identical outputs.  Asynchronous.  Quarter turns need h == w (set any_quarter_turn if any aug[i].rot is 1
 * or 3): IMK_EUNSUPPORTED otherwise, before any launch.  The workspace is sized by imk_unet_forward_student_workspace_bytes. */
IMK_API int64_t imk_unet_forward_student_workspace_bytes(const imk_unet_plan *plan, int batch);
IMK_API int imk_unet_forward_student(const imk_unet_plan *plan, const float *params, const void *packed, const uint8_t *x,
                                     const uint8_t *img, int batch, float thr, int cmp_ge, const imk_aug_params *aug,
                                     int any_quarter_turn, uint8_t *img_out, uint8_t *labels_out, void *workspace,
                                     int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation reductions (benchmark_ISIC2018 / benchmark_multiclass)
 * ---------------------------------------------------------------------------------------------- */
/* Replaces the threshold + per-image numpy metric loop of benchmark_ISIC2018 (functions.py:1120-1140) with
 * get_IoU_binary (:1767-1788) and dice_score_numpy_binary (:1837-1861):
 *   probs [B,H,W] f32, gt [B,H,W] u8 -> pred_out [B,H,W] u8 in {0,255} (may be NULL), counts [B,5] int64 =
 *   { #(gt!=0 & pred), #(gt!=0 | pred), #(gt>=128), #pred, #(gt>=128 & pred) };  pred = p > thr (cmp_ge: >=). */
IMK_API int imk_eval_binary(const float *probs, float thr, int cmp_ge, const uint8_t *gt, int batch, int h, int w,
                    uint8_t *pred_out, int64_t *counts, void *stream);

/* Replaces argmax + pixel_accuracy (functions.py:1820-1834) + get_IoU_multi_unique (:1791-1816) of
 * benchmark_multiclass (:1308-1330):  probs [B,H,W,K] f32, gt [B,H,W] u8 class ids -> pred_out [B,H,W] u8 (may be
 * NULL), counts [B,4,256] int64: [0][v] = #(gt==v), [1][v] = #(pred==v), [2][v] = #(gt==v & pred==v),
 * [3][0] = #(pred==gt).  k <= 256.  The arg-max is np.argmax's: the first maximum wins, and a NaN counts as the maximum
 * (the first NaN wins). */
IMK_API int imk_eval_multiclass(const float *probs, const uint8_t *gt, int batch, int h, int w, int k, uint8_t *pred_out,
                        int64_t *counts, void *stream);

/* Reductions of the validation monitors of train_multiclass / train_hela (the ModelCheckpoint criteria, functions.py:
 * 255-258, 303-306), deterministic (fixed summation order):
 *   mode 0 -- MeanIoU.update_state (functions.py:75-86): probs [n_pix,K] f32, gt [n_pix] u8 class ids ->
 *             out[0..K) = sum_p [gt == k] p_k,  out[K..2K) = sum_p [gt == k],  out[2K..3K) = sum_p p_k
 *   mode 1 -- squared error of Keras' val_loss for 'mse': gt [n_pix,K] u8 targets -> out[0] = sum (p - y)^2
 * out: device buffer of imk_eval_soft_out_doubles(K) doubles (results first, block partials behind them); K <= 64. */
IMK_API int64_t imk_eval_soft_out_doubles(int k);
IMK_API int imk_eval_soft_sums(const float *probs, const uint8_t *gt, int64_t n_pix, int k, int mode, double *out, void *stream);

/* The sums of the reference's dice_loss (functions.py:162-184) per image: probs [B,H,W,K] f32, gt [B,H,W,K] u8 targets ->
 * out [B,3] double = (sum t p, sum t, sum p) with t = double(gt).  One workgroup per image, double accumulators in an order fixed
 * by H*W*K alone: an image's row does not depend on the batch it is in.  The loss of a prediction is
 * 1 - mean_b (2 out[b][0] + 1) / (out[b][1] + out[b][2] + 1); train_hela's val_loss monitor under dice_loss is that over all
 * validation images. */
IMK_API int imk_eval_dice_sums(const float *probs, const uint8_t *gt, int batch, int h, int w, int k, double *out, void *stream);

/* The label of the scalar-IoU multiclass EvalNet family (csrc/imk_label.hip): the writers' `image[im > 0] = 0; pred[im > 0] = 0`
 * and the per-class pixel counts get_IoU_multi_unique (functions.py:1791-1816) is a ratio of, in one pass.
 *   pred, gt [B,H,W] u8 class ids 0..255; im [B,H,W] u8 or NULL: a pixel with im > 0 is blocked -- its prediction counts as class 0,
 *   pred_blocked [B,H,W] u8 (may be NULL, may alias pred) stores p' = the blocked prediction, image [B,H,W,c] u8 (may be NULL;
 *   c = 1 or 3) is zeroed there in place: the bytes imk_block_apply and a copy leave.
 *   counts [B,4,256] int64: [0][v] = #(gt == v), [1][v] = #(p' == v), [2][v] = #(gt == v & p' == v), [3][v] = #(gt == v & im == 0)
 *   (im NULL: row 3 = row 0).  Zeroed by the call on `stream`; integer arithmetic only, so the result does not depend on the grid.
 * Asynchronous, allocates nothing.  IMK_EINVAL (before any launch): a NULL pred / gt / counts, non-positive sizes, image given with
 * c other than 1 or 3.  IMK_EUNSUPPORTED: h * w >= 2^31, batch > 65535. */
IMK_API int imk_label_counts(const uint8_t *pred, const uint8_t *gt, const uint8_t *im, uint8_t *image, int c, int batch, int h, int w,
                     uint8_t *pred_blocked, int64_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Depth-map (regression) family (csrc/imk_depth.hip): get_im_prediction_depth_map (functions.py:6155-6177), benchmark_depth_map
 * (:1345-1384), rmse / delta_metric (:36-48)
 * ---------------------------------------------------------------------------------------------- */
/* The standard-deviation IM: a pixel is inconsistent where the ensemble's per-pixel standard deviation exceeds mult times the
 * image's mean standard deviation.  Every image of the batch gets its own threshold (the reference works on one prepared image; one
 * threshold over a whole batch, as it forms when handed one, is this call with batch 1 and height B*H: the element order is the same).
 *   preds    [N,B,H,W] float32 (one output map), 2 <= N <= 16, else IMK_EUNSUPPORTED; H*W <= 2^24 and B <= 65535, else IMK_EUNSUPPORTED
 *   img      [B,H,W,C] uint8 or NULL;  img_out = img with IM pixels zeroed if block_in (ignored when img == NULL)
 *   im_out   [B,H,W] uint8 {0,255};  im_size [B] int64;  thr_out [B] float32, the thresholds
 *   std_out  [B,H,W] float32 or NULL: the standard-deviation map.  Given, it serves as the call's map and the workspace is not touched
 *            (it may be NULL then); otherwise the map lives in the workspace, imk_im_depth_workspace_bytes(B, H, W) bytes.
 * Bit-exact against numpy's float32 np.std(axis=-1) -> mult * np.mean -> `>` given identical predictions: float32 throughout, every
 * operation rounded on its own (no fused multiply-add; correctly rounded divides and square roots), sums in numpy's order -- over the
 * models eight strided accumulators from N = 8 on, over the image the pairwise recursion down to leaves of at most 128 elements inside
 * chunks of 8192 elements that are added sequentially (csrc/imk_depth.hip states the order in full).  mult is the float32 multiplier:
 * numpy >= 2 forms float32(mult) * mean in float32; numpy < 2 forms the product in double and rounds once, the same value for every
 * multiplier representable in float32.  NaN propagates: one NaN prediction makes the image's threshold NaN and its whole IM zero. */
IMK_API int64_t imk_im_depth_workspace_bytes(int batch, int h, int w);
IMK_API int imk_im_depth(const float *preds, int n_models, int batch, int h, int w, float mult, const uint8_t *img, int c,
                         int block_in, uint8_t *img_out, uint8_t *im_out, int64_t *im_size, float *thr_out, float *std_out,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* Ensemble inference fused with the standard-deviation IM, in the shape of imk_unet_forward_im: N models' forward passes (sigmoid
 * heads with one map; `params` / `packed` host arrays of N device pointers; the models on k <= min(N, 3) streams forked from and
 * joined to `stream`), then imk_im_depth's rule on their probabilities; outputs as imk_im_depth (std_out may be NULL; img = the
 * plan's c_in channels).  The first launch of the rule reads the N last decoder activations (fp16) and forms every model's probability
 * with the code of imk_unet_forward's head, so the fp32 probability stack is never written and the outputs are bit-identical to
 * imk_unet_forward x N + imk_im_depth.  The fused launch covers last decoder widths 8 / 16 / 24 / 32 and N <= 8; other shapes (N up
 * to 16) and plans with the materialize debug switch take the unfused route through the stack inside the same call.
 * workspace: imk_unet_forward_im_depth_workspace_bytes(plan, N, B, k) = imk_unet_forward_im_workspace_bytes + the std map. */
IMK_API int64_t imk_unet_forward_im_depth_workspace_bytes(const imk_unet_plan *plan, int n_models, int batch, int n_streams);
IMK_API int imk_unet_forward_im_depth(const imk_unet_plan *plan, int n_models, const float *const *params,
                                      const void *const *packed, const uint8_t *x, int batch, float mult, const uint8_t *img,
                                      int block_in, uint8_t *img_out, uint8_t *im_out, int64_t *im_size, float *thr_out,
                                      float *std_out, void *workspace, int64_t workspace_bytes, void *stream);

/* Evaluation of a depth-map model: probs [B,H,W] f32, gt [B,H,W] u8 ->
 *   pred_out [B,H,W] u8 (may be NULL): clip(p * 255.0f, 0, 255) truncated toward zero, NaN -> 0 (benchmark_depth_map's PNG rule)
 *   sums     [B,2] double, per image and in a summation order fixed by H*W:
 *            [0] sum (p - y)^2 with y = float32(gt) / 255.0f (a correctly rounded divide), the difference formed in float32 and
 *                squared and added in double;
 *            [1] the number of pixels with max(p / y, y / p) < 1.25f in float32; y = 0 and NaN count as false, as tf.maximum and `<`
 *                leave them.
 * Per image, so that the host can form Keras' per-batch, batch-size-weighted means (rmse: the mean of per-batch square roots). */
IMK_API int imk_eval_depth(const float *probs, const uint8_t *gt, int batch, int h, int w, uint8_t *pred_out, double *sums,
                           void *stream);

/* ------------------------------------------------------------------------------------------------
 * EvalNet (evalnet.py:24-73): the quality-scoring network of IM++ / AIM++
 * ----------------------------------------------------------------------------------------------
 * Replaces get_evalnet / get_evalnet_miou + model.predict([A, B]) (functions.py:5837-5941 call sites) and the
 * model.fit step of train_evalnet_ISIC_2018 / train_evalnet_miou_model_hela (functions.py:4464-4506, 4673-4722).
 * Two uint8 inputs A [B,H,W,ca] (image) and B [B,H,W,cb] (mask stack, or [B,H,W] class ids with b_onehot); each tower is input_block + conv_block, the
 * towers are concatenated, five conv_blocks follow, then GlobalAvgPool2D and the Dense sigmoid head(s).
 * The plan is an imk_unet_plan: imk_unet_param_count / _num_layers / _layer_info / _packed_bytes / _pack_weights /
 * _state_bytes / _state_init / _adamw_step / _plan_destroy apply unchanged.  Layer names: "a.in.c", "a.in.bn", "a.c3",
 * "a.c1", "a.bn", the same with "b.", "m1.c3", "m1.c1", "m1.bn" ... "m5.bn", then "dense" or "iou", "detection"
 * (Dense kernels [C, n_out] + bias, reported as 1x1 convs); parameter order = Keras creation order. */
IMK_API int imk_evalnet_plan_create(const imk_evalnet_cfg *cfg, imk_unet_plan **out);
/* The late-fusion EvalNet, get_evalnet_miou_v2 (evalnet.py:76-106).  Same blocks, other wiring: each tower is input_block at
 * ch[0] + FOUR conv_blocks at ch[0..3]; the towers' pooled outputs (H/16 x W/16, ch[3] channels) are ADDED -- two fp16 tensors,
 * the exact sum rounded to fp16 once, as Keras' Add layer does under mixed_float16; three conv_blocks at ch[2], ch[3], ch[4]
 * follow, then GlobalAvgPool2D and the heads 'iou' and 'detection'.  The cfg struct is the one above: two_heads must be 1, h and w
 * even and >= 128 (seven poolings; odd rows / columns dropped), ch[3] a multiple of 8; every other limit as
 * imk_evalnet_plan_create.  Layer names: "a.in.c", "a.in.bn", "a1.c3", "a1.c1", "a1.bn" ... "a4.bn", the same with "b",
 * "m1.c3" ... "m3.bn", "iou", "detection"; parameter order = Keras creation order (tower A completely, tower B, trunk, heads).
 * Every imk_evalnet_* call below takes such a plan and does the same job for it; imk_evalnet_forward_candidates then runs ALL of
 * the image tower (about half of the network) once per image.  Plans made by imk_evalnet_plan_create run the launches they always ran. */
IMK_API int imk_evalnet_v2_plan_create(const imk_evalnet_cfg *cfg, imk_unet_plan **out);
IMK_API int64_t imk_evalnet_workspace_bytes(const imk_unet_plan *plan, int batch, int mode /* 0 inference, 1 training */);

/* out [B, n_heads*n_out] f32 sigmoid outputs (two heads: iou units first, then detection units); inference-mode BN */
IMK_API int imk_evalnet_forward(const imk_unet_plan *plan, const float *params, const void *packed, const uint8_t *xa,
                        const uint8_t *xb, int batch, float *out, void *workspace, int64_t workspace_bytes, void *stream);

/* Training pass: forward with batch statistics (moving statistics updated in params), losses, backward.
 *   y [B, n_heads*n_out] f32 targets.  Loss: head 0 mean squared error; head 1 binary cross-entropy (functions.py:4708
 *   loss=['mse','binary_crossentropy'], summed);  a single head: mean squared error (functions.py:4492).
 *   out (may be NULL): the training-mode outputs;  grads [n_trainable] f32 (unscaled);
 *   stats [8] f32: {total loss, overflow flag, loss scale, step, loss of head 0, loss of head 1, -, -}.
 * Follow with imk_unet_adamw_step. */
IMK_API int imk_evalnet_fwd_bwd(const imk_unet_plan *plan, float *params, void *packed, void *state, const uint8_t *xa,
                        const uint8_t *xb, const float *y, int batch, float *out, float *grads, float *stats,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* Debug/parity: like imk_unet_tensor_info, for EvalNet plans.  Two more values of `which`:
 *   3  the INPUT of the trunk's first conv ("m1.c3"): the towers' concatenation, or for a v2 plan their sum (c = its channels)
 *   4  a BatchNorm layer's fp32 scale[c_stride] | shift[c_stride] as the kernels apply them (h = 1, w = 2): mode 0 the folded
 *      moving statistics, and byte_offset is into the PACKED buffer; mode 1 the last pass's batch statistics, in the workspace */
IMK_API int imk_evalnet_tensor_info(const imk_unet_plan *plan, int batch, int mode, int layer_idx, int which,
                            int64_t *byte_offset, int *h, int *w, int *c, int *c_stride);

/* ------------------------------------------------------------------------------------------------
 * EvalNet-ensemble selection baseline (create_training_data_for_segnet_with_ensemble_binary,
 * ..._with_miou_ensemble_hela, ..._with_miou_ensemble_multiclass: functions.py:5070-5155, 5323-5577) and the single-EvalNet
 * baseline (create_training_data_for_segnet_ISIC_2018, :4991-5063 = IMK_SELECT_IOU with N = 1;
 * create_training_data_by_evalnet_miou_for_segnet_multiclass, :5583-5677 = IMK_SELECT_CONF_GATED)
 * ----------------------------------------------------------------------------------------------
 * For every unlabeled image the reference stacks M candidate masks, scores the (image, mask) pairs with the N EvalNets of the
 * ensemble, averages over the EvalNets, takes the arg-max candidate and keeps the pair if its score reaches a threshold.  */
#define IMK_SELECT_MAX_CAND 16    /* candidates per image */
#define IMK_SELECT_MAX_MODELS 8   /* EvalNets per ensemble */
enum { IMK_SELECT_IOU = 0, IMK_SELECT_MIOU = 1, IMK_SELECT_CONF_GATED = 2 };

/* The selection rule and the gather of the chosen candidate, one kernel.
 *   scores     [N,B,M,n_heads*n_out] f32, unit order of imk_evalnet_forward (iou units first, then detection units)
 *   counts     device int32 [B] or NULL (= every image has M candidates); candidates m >= counts[b] do not exist for image b and
 *              influence nothing.  1 <= counts[b] <= M, else IMK_EINVAL (the array is read back before the launch: the call
 *              waits for `stream` when counts is given)
 *   cand       [B,M,cand_bytes] u8: what is written out for a chosen candidate; cand_bytes a multiple of 16, cand / out 16-byte aligned
 *   best_idx [B] int32, best_score [B] f32, keep [B] u8 (0/1), out [B,cand_bytes] u8 = the best candidate's bytes, kept or not
 * Mean over the models (every mode): ((p_0 + p_1) + p_2) + ... in fp32, then one correctly rounded fp32 divide by N -- np.mean(axis=0)
 * of the float32 stack, as imk_vote_multiclass.
 *   IMK_SELECT_IOU  (n_heads = 1, n_out = 1): score = that mean.
 *   IMK_SELECT_MIOU (n_heads = 2): class k counts if its mean detection >= 0.5f (NaN does not); score = the fp32 sum of the counting
 *                   classes' mean ious in class order (the first addend as it is), divided by their number (correctly rounded);
 *                   0 if no class counts.
 *   IMK_SELECT_CONF_GATED (n_heads = 2): the rule of the single-EvalNet writer create_training_data_by_evalnet_miou_for_segnet_multiclass
 *                   (functions.py:5649-5672; the reference runs it with N = 1, where the mean over the models is the value itself).
 *                   Gate: g_k = the fp32 sum of class k's mean detection over the image's candidates m = 0 .. cnt-1 in candidate order,
 *                   divided by cnt (correctly rounded) -- np.mean(axis=0) of the float32 [M,K]; class k counts, for every candidate of
 *                   the image, iff g_k >= 0.03f (NaN does not).  cnt = counts[b], or M.  Score of candidate m = the fp32 sum of its
 *                   mean DETECTION values over the counting classes in class order (the first addend as it is), divided by their
 *                   number (correctly rounded); 0 if no class counts.  The iou units (the first K of every row) are read by nobody
 *                   in this mode, as in the reference.  Its own kernel; modes 0 and 1 run the code they ran before.
 * best_idx = np.argmax of the scores (the first maximum; the first NaN wins); keep = best >= (float)thr (NaN keeps nothing): numpy
 * compares the float32 score with the Python threshold in float32.
 * N > IMK_SELECT_MAX_MODELS or M > IMK_SELECT_MAX_CAND (or n_out > 64): IMK_EUNSUPPORTED, before any launch.               */
IMK_API int imk_evalnet_select(const float *scores, int n_models, int batch, int n_cand, int n_heads, int n_out,
                               const int32_t *counts, const uint8_t *cand, int64_t cand_bytes, double thr, int mode,
                               int32_t *best_idx, float *best_score, uint8_t *keep, uint8_t *out, void *stream);

/* N EvalNets of one plan score B images with M candidates each: xa [B,H,W,ca], xb [B,M,H,W,cb] (b_onehot: class ids [B,M,H,W])
 * -> scores [N,B,M,n_heads*n_out].  Per model the image tower runs once at batch B, the mask tower and the trunk at batch B*M, and
 * row r of the concatenation reads image r / M of the image tower.  Bit-identical to imk_evalnet_forward on the image repeated M
 * times.  `params`/`packed` are arrays (host) of n_models device pointers; the models run one after another on `stream`.
 * Asynchronous; nothing is allocated.  Limits as imk_evalnet_select.  The workspace is one model's activations at batch B*M; under
 * IMK_SELECT_SHARED=0 it also holds the repeated images, so size it with the function below in the process that makes the call. */
IMK_API int64_t imk_evalnet_forward_candidates_workspace_bytes(const imk_unet_plan *plan, int batch, int n_cand);
IMK_API int imk_evalnet_forward_candidates(const imk_unet_plan *plan, int n_models, const float *const *params,
                                           const void *const *packed, const uint8_t *xa, const uint8_t *xb, int batch, int n_cand,
                                           float *scores, void *workspace, int64_t workspace_bytes, void *stream);

/* imk_evalnet_forward_candidates + imk_evalnet_select on one stream, the scores staying on the device ([N,B,M,n_heads*n_out], the
 * caller's buffer) and no host synchronisation between scoring and gather.  Asynchronous with counts = NULL.  With counts given the
 * call (like imk_evalnet_select) first copies counts to the host and waits for `stream`, so that a count outside 1..M is IMK_EINVAL
 * rather than a clamp: it then blocks the host once, before its first launch, and cannot be captured into a graph.
 * Outputs bit-identical to the two calls.  Same workspace.  IMK_SELECT_SHARED=0 (environment) scores through imk_evalnet_forward
 * per model on a device-side repeat of the images instead: the comparison arm of the tests and the measurement.             */
IMK_API int imk_evalnet_forward_select(const imk_unet_plan *plan, int n_models, const float *const *params,
                                       const void *const *packed, const uint8_t *xa, const uint8_t *xb, int batch, int n_cand,
                                       const int32_t *counts, const uint8_t *cand, int64_t cand_bytes, double thr, int mode,
                                       float *scores, int32_t *best_idx, float *best_score, uint8_t *keep, uint8_t *out,
                                       void *workspace, int64_t workspace_bytes, void *stream);

/* Momentum of the BatchNorm moving statistics in the training steps of ONE plan (U-Net or EvalNet).  Default 0.99 = Keras'
 * BatchNormalization default, which the reference never overrides (unet.py:7).  Data-parallel runs with per-GPU batch 32 make
 * N times fewer optimizer steps per epoch: 0.99^N keeps the moving average's memory the same in SAMPLES (functions.py of this
 * repository: IMK_DP_BN_MOMENTUM=scaled; off by default, it is a deviation from the reference's recipe). */
IMK_API int imk_unet_plan_set_bn_momentum(imk_unet_plan *plan, float momentum);
IMK_API int imk_unet_plan_get_bn_momentum(const imk_unet_plan *plan, float *momentum);

/* Debug / measurement switches of ONE plan (U-Net or EvalNet); -1 leaves a switch as it is.  The library keeps no global state:
 * the caller owns the plan and these two flags in it.
 *   materialize = 1: inference also stores the intermediates that fused kernels normally keep on chip (the Conv3x3 output
 *     inside a fused Conv3x3 -> Conv1x1 kernel, the input block's output), so that imk_unet_tensor_info works on every layer.
 *     Training always stores them (the backward pass needs them).
 *   single_stream = 1: every kernel runs on the caller's stream (no side stream for the weight gradients, the ensemble's models
 *     back to back), so that per-kernel timings are exclusive.  Results are identical either way. */
IMK_API int imk_unet_plan_debug(imk_unet_plan *plan, int materialize, int single_stream);

/* ------------------------------------------------------------------------------------------------
 * Host-side PNG codec of the directory API (csrc/imk_png.cpp).  Replaces cv2.imread / cv2.imwrite of the
 * reference's writers and parsers (functions.py:2846, 2885-2887, 955-1048) for the files this path reads and writes.  ALL
 * pointers are HOST pointers; no GPU call is made; thread-safe and re-entrant (one file per call: callers parallelise over files,
 * ctypes drops the interpreter lock around the call).  Decoder: 8-bit greyscale / RGB / palette / greyscale + alpha / RGBA,
 * non-interlaced; anything else returns IMK_EUNSUPPORTED (the Python layer then uses Pillow).  want_c = 3: RGB (alpha dropped,
 * palette expanded, grey replicated); want_c = 1: Pillow's convert("L").  Encoder: 8-bit greyscale (c = 1) or RGB (c = 3),
 * deflate level 0-9.
 * ---------------------------------------------------------------------------------------------- */
IMK_API int imk_png_info(const char *path, int *h, int *w, int *color_type, int *bit_depth);
IMK_API int imk_png_read_file(const char *path, int want_c, uint8_t *out, int64_t out_cap, int *h_out, int *w_out);
IMK_API int imk_png_decode(const uint8_t *data, int64_t len, int want_c, uint8_t *out, int64_t out_cap, int *h_out, int *w_out);
IMK_API int imk_png_encode(const uint8_t *pixels, int h, int w, int c, int level, uint8_t *out, int64_t out_cap, int64_t *out_len);
IMK_API int imk_png_write_file(const char *path, const uint8_t *pixels, int h, int w, int c, int level);

/* ------------------------------------------------------------------------------------------------
 * Host-side geometry of the HeLa position masks (csrc/imk_geom.cpp).  HOST pointers, no GPU call,
 * thread-safe and re-entrant (one image per call).  Replace the reference's OpenCV calls:
 *   imk_pos_contours  functions.py:6181-6218 get_pos_contours: cv2.erode (erode_kernel x erode_kernel, odd or 0/1 for none) ->
 *                     threshold > 10 -> cv2.findContours(RETR_TREE) -> cv2.moments -> (int(m10 / m00) + 1, int(m01 / m00) + 1)
 *                     for every contour with m00 != 0 (blobs in raster order of their first pixel, each followed by its holes).
 *                     Writes up to `cap` (x, y) pairs, returns the number found (> cap: call again with a larger buffer) or a
 *                     negative IMK_E* code.
 *   imk_mod_pos_size  functions.py:6255-6292 mod_pos_size: blobs (3 x 3 erosion) re-drawn with cv2.circle of radius
 *                     clamp(min_dist // 4, min_r, max_r); blur2 != 0: cv2.blur (2, 2), < 254 -> 0.  lone_dist: the distance
 *                     used when the mask holds exactly one position (0 in mod_pos_size; 99 and blur2 = 0 in the pseudo-label
 *                     writer, functions.py:2952-2966).  out: h x w uint8 in {0, 255}.
 *   imk_cell_count    functions.py:6298-6371 get_cell_count: counts = {alive, dead, unclear} over the positions.
 * ---------------------------------------------------------------------------------------------- */
IMK_API int imk_pos_contours(const uint8_t *img, int h, int w, int erode_kernel, int32_t *xy, int cap);
IMK_API int imk_mod_pos_size(const uint8_t *img, int h, int w, int max_r, int min_r, int lone_dist, int blur2, uint8_t *out);
IMK_API int imk_cell_count(const int32_t *xy, int n, const uint8_t *alive, const uint8_t *dead, int h, int w,
                           int measuring_range, int32_t counts[3]);

/* ------------------------------------------------------------------------------------------------
 * Data preparation (csrc/imk_prep.hip): the pixel rules of the reference's 00_* / 01_* / SUIM 02_* scripts, which go through
 * cv2.resize, cv2.cvtColor and cv2.threshold.  The rules are restated from OpenCV 4's published sources (imgproc/src/resize.cpp,
 * imgproc/src/color_rgb.simd.hpp as of 4.x: 8-bit grey with 15-bit coefficients); they are not pinned against OpenCV itself.
 * DEVICE pointers unless stated; not in place.
 *
 * imk_prep_resize: a ragged batch in one launch.  src holds n decoded sources [src_h, src_w, c] u8 back to back (src_bytes in
 * all); item i resizes the rectangle (x0, y0, cw, ch) of the source at src + src_off to out[i] [dh, dw, c].  scale_x / scale_y
 * are 1.0 / ((double)dw / cw) and 1.0 / ((double)dh / ch), formed by the host as cv::resize forms 1 / inv_scale.  An item whose
 * rectangle leaves its source, or whose source leaves [0, src_bytes), is written as zeros (nothing is read for it).
 *   IMK_PREP_LINEAR   cv2.resize's default for 8-bit data: per axis f = (float)((d + 0.5) * scale - 0.5) (product and sum rounded
 *                     separately in double), s = floor(f), f -= s; on x, s < 0 -> (0, 0) and s >= cw - 1 -> (cw - 1, 0); on y the
 *                     rows s, s + 1 are clamped into the rectangle; weights rint(. * 2048) (half to even, saturated to int16);
 *                     H = S[s] a0 + S[s + 1] a1; out = (((b0 (H0 >> 4)) >> 16) + ((b1 (H1 >> 4)) >> 16) + 2) >> 2.
 *                     cw == 2 dw and ch == 2 dh: (p00 + p01 + p10 + p11 + 2) >> 2, as cv::resize switches to its area rule.
 *   IMK_PREP_NEAREST  sx = min((int)floor(dx * scale_x), cw - 1) in double, the same on y.
 *   post = IMK_PREP_LABEL_PLUS1: v > 0 ? (uint8)(v + 1) : v  (np.where(m > 0, m + 1, m) on uint8: 255 wraps to 0).
 * c is 1 or 3 (else IMK_EUNSUPPORTED); n <= 65535; dh * dw * c < 2^31.
 * ---------------------------------------------------------------------------------------------- */
enum { IMK_PREP_LINEAR = 0, IMK_PREP_NEAREST = 1 };
enum { IMK_PREP_LABEL_PLUS1 = 1 };
typedef struct imk_prep_item {    /* one per output image, device array [n] */
    int64_t src_off;              /* byte offset of the decoded source inside src */
    int src_h, src_w;
    int x0, y0, cw, ch;           /* the crop rectangle inside the source; the whole image is (0, 0, src_w, src_h) */
    double scale_x, scale_y;
} imk_prep_item;
IMK_API int imk_prep_resize(const uint8_t *src, int64_t src_bytes, const imk_prep_item *items, int n, int c, int dh, int dw,
                            int interp, int post, uint8_t *out, void *stream);

/* imk_prep_crops: one source [h, w, c] u8 (c = 1 or 3) -> P planes out [P, ch, cw] u8; pos device int32 [P, 2] of (x, y), the
 * crop's top-left corner.  The whole image is the one crop at (0, 0) with cw = w, ch = h.  A crop pixel outside the source is
 * written as 0 (nothing is read for it).  b_first != 0: byte 0 of a pixel is B (cv2.imread's order), else R.
 *   IMK_PREP_GRAY         c == 3: (R 9798 + G 19235 + B 3735 + 16384) >> 15 (cv2.cvtColor(BGR2GRAY), 8 bit); c == 1: a copy
 *   IMK_PREP_GRAY_THRESH  the grey value > 10 ? 255 : 0                                  (cv2.threshold(., 10, 255, THRESH_BINARY))
 *   IMK_PREP_CLASS8       c == 3 only: class_table[(R >= 128) << 2 | (G >= 128) << 1 | (B >= 128)]; class_table is a HOST
 *                         pointer to 8 bytes, read during the call (NULL for the other rules)
 * ---------------------------------------------------------------------------------------------- */
enum { IMK_PREP_GRAY = 0, IMK_PREP_GRAY_THRESH = 1, IMK_PREP_CLASS8 = 2 };
IMK_API int imk_prep_crops(const uint8_t *src, int h, int w, int c, const int32_t *pos, int n_crops, int ch, int cw, int rule,
                           const uint8_t *class_table, int b_first, uint8_t *out, void *stream);

/* Runtime environment checks.  imk_runtime_warnings() returns a bit mask of conditions the library has noticed so far in this
 * process (it also prints each once to stderr):
 *   IMK_WARN_HW_QUEUES  a side stream was requested (training step, ensemble forward) while GPU_MAX_HW_QUEUES is unset or
 *                       below 8: the HIP runtime's default of 4 hardware queues lets a side stream share the queue of the
 *                       stream it should run beside (measured: -14 % per generation).  Export GPU_MAX_HW_QUEUES=8 before the
 *                       first HIP call of the process (the Python package does so at import).
 * imk_unet_plan_side_stream returns side stream i (0 .. 1) of `plan` as a hipStream_t, creating it if needed -- the streams
 * belong to ONE pool per device shared by every plan (U-Net or EvalNet) of the process. */
#define IMK_WARN_HW_QUEUES 1
IMK_API int imk_runtime_warnings(void);
IMK_API int imk_unet_plan_side_stream(const imk_unet_plan *plan, int i, void **stream_out);

/* ------------------------------------------------------------------------------------------------
 * Measurement hook (bench.py): per-launch HIP-event timing of every kernel family of the path, on the stream the
 * kernel is launched on.  A context is created and owned by the caller and bound to the calling thread: while bound, every
 * period-th hooked launch made by THAT thread records an event pair into it (period 0 = off).  imk_prof_collect synchronises
 * those events and returns, per family v (0..IMK_PROF_VARIANTS-1), the number of sampled launches, their summed duration in
 * ms, their summed ALGORITHMIC bytes (every input tensor read once + every output tensor written once) and -- flops may be
 * NULL -- the summed FLOPs (2 x multiply-adds, logical channel counts; 0 for families that are not convolutions), then
 * resets the records.  Families:
 *   0..5  conv_mfma_kernel<TH,MT>: v = 3*(TH==8) + log2(MT)      6  conv_pipe_kernel
 *   7  wgrad_mfma_kernel      8  bn_bwd_prep(_pool)_kernel       9  bn_bwd_coef_kernel     10  bn_finalize_kernel
 *   11 wgf_stage1 + wgf_stage2 (one bracket)                     12 head_kernel            13  head_loss_kernel / head_cce_fused_kernel
 *   14 loss_finalize / adamw / pack_conv_batched / bn_fold_batched                         15  im_binary_* / im_multi_kernel
 *   16 conv_gemm_kernel (wide layers, forward / dgrad)           17 wgrad_gemm_kernel (wide layers, weight gradient)
 * A context must not be shared between threads that launch concurrently (two hipEventRecord per sampled launch while bound).
 * ---------------------------------------------------------------------------------------------- */
#define IMK_PROF_VARIANTS 18
typedef struct imk_prof imk_prof;   /* opaque, host memory */
IMK_API int imk_prof_create(int period, imk_prof **out);
IMK_API void imk_prof_destroy(imk_prof *ctx);
IMK_API int imk_prof_bind(imk_prof *ctx);              /* ctx or NULL (unbind) for the calling thread */
IMK_API int imk_prof_unbind(imk_prof *ctx);            /* unbinds the calling thread only if `ctx` is what it has bound (1 if it did, else 0) */
IMK_API int imk_prof_set_period(imk_prof *ctx, int period);
/* Totals for rocprofv3 cross-checks: while enabled, EVERY hooked launch of the bound thread adds its launch count, algorithmic
 * bytes and flops to a per-kernel-name sum (the conv_pipe / conv_wide families by template variant, spelled as rocprofv3 prints
 * them; the others by family).  imk_prof_totals_enable(ctx, on) clears the sums and switches them on / off;
 * imk_prof_totals_dump writes "name;launches;bytes;flops" lines into buf (cap bytes) and returns the size needed.
 * imk_prof_mark enqueues an empty marker kernel (imk_mark_kernel, 64 * id work-items) on `stream`: bench.py brackets its timed
 * region with ids 1 and 2 so that profiles/summarize.py can cut a kernel trace there. */
IMK_API int imk_prof_totals_enable(imk_prof *ctx, int on);
IMK_API int64_t imk_prof_totals_dump(imk_prof *ctx, char *buf, int64_t cap);
IMK_API int imk_prof_mark(int id, void *stream);
IMK_API int imk_prof_collect(imk_prof *ctx, int64_t *count, double *ms, double *bytes, double *flops);

#ifdef __cplusplus
}
#endif
#endif /* IMK_H */
