// Host orchestration of the tiny U-Net (unet.py:4-67) on top of the kernels in imk_conv.hip /
// imk_elem.hip: topology, workspace layout, batched inference, ensemble inference + IM, and the training step
// (forward with batch statistics, loss, backward, AdamW).  The layer-level helpers are shared with EvalNet (imk_net.h).
// Everything is enqueued on the caller's stream; nothing here allocates or synchronises.
#include <atomic>
#include <cstdio>
#include <vector>
#include "imk_net.h"
#include "imk_head.h"
#include "imk_switches.h"

namespace {

// ---- topology ------------------------------------------------------------------------------------
// index of every layer by role

struct Topo {
    int in_c, in_bn;
    int e_c3[4], e_c1[4], e_bn[4];
    int b_c3, b_c1, b_bn;
    int d_ca[4], d_bna[4], d_c3[4], d_c1[4], d_bnb[4];
    int out;
};

Topo make_topo(const imk_unet_plan *p) {
    Topo t{};
    t.in_c = p->find("in.c"); t.in_bn = p->find("in.bn");
    char nm[16];
    for (int i = 0; i < 4; ++i) {
        snprintf(nm, sizeof nm, "e%d.c3", i + 1); t.e_c3[i] = p->find(nm);
        snprintf(nm, sizeof nm, "e%d.c1", i + 1); t.e_c1[i] = p->find(nm);
        snprintf(nm, sizeof nm, "e%d.bn", i + 1); t.e_bn[i] = p->find(nm);
    }
    t.b_c3 = p->find("b.c3"); t.b_c1 = p->find("b.c1"); t.b_bn = p->find("b.bn");
    for (int j = 0; j < 4; ++j) {
        snprintf(nm, sizeof nm, "d%d.ca", j + 6); t.d_ca[j] = p->find(nm);
        snprintf(nm, sizeof nm, "d%d.bna", j + 6); t.d_bna[j] = p->find(nm);
        snprintf(nm, sizeof nm, "d%d.c3", j + 6); t.d_c3[j] = p->find(nm);
        snprintf(nm, sizeof nm, "d%d.c1", j + 6); t.d_c1[j] = p->find(nm);
        snprintf(nm, sizeof nm, "d%d.bnb", j + 6); t.d_bnb[j] = p->find(nm);
    }
    t.out = p->find("out");
    return t;
}

void build_layers(imk_unet_plan *p) {
    const int *ch = p->cfg.ch;  // 16a 32a 64a 128a 256a
    int c = add_conv(p, "in.c", 1, p->cfg.c_in, ch[0], 0);
    add_bn(p, "in.bn", ch[0], 0, c);
    const int enc_in[4] = {ch[0], ch[0], ch[1], ch[2]};
    const int enc_f[4] = {ch[0], ch[1], ch[2], ch[3]};
    char nm[16];
    for (int i = 0; i < 4; ++i) {
        snprintf(nm, sizeof nm, "e%d.c3", i + 1); add_conv(p, nm, 3, enc_in[i], enc_f[i], i);
        snprintf(nm, sizeof nm, "e%d.c1", i + 1); c = add_conv(p, nm, 1, enc_f[i], enc_f[i], i);
        snprintf(nm, sizeof nm, "e%d.bn", i + 1); add_bn(p, nm, enc_f[i], i, c);
    }
    add_conv(p, "b.c3", 3, ch[3], ch[4], 4);
    c = add_conv(p, "b.c1", 1, ch[4], ch[3], 4);
    add_bn(p, "b.bn", ch[3], 4, c);
    const int dec_in[4] = {ch[3], ch[2], ch[1], ch[0]};
    const int dec_f1[4] = {ch[3], ch[2], ch[1], ch[0]};
    const int dec_f2[4] = {ch[2], ch[1], ch[0], ch[0]};
    for (int j = 0; j < 4; ++j) {
        const int res = 3 - j;
        snprintf(nm, sizeof nm, "d%d.ca", j + 6); c = add_conv(p, nm, 1, dec_in[j], dec_f1[j], res);
        snprintf(nm, sizeof nm, "d%d.bna", j + 6); add_bn(p, nm, dec_f1[j], res, c);
        snprintf(nm, sizeof nm, "d%d.c3", j + 6); add_conv(p, nm, 3, dec_f1[j], dec_f1[j], res);
        snprintf(nm, sizeof nm, "d%d.c1", j + 6); c = add_conv(p, nm, 1, dec_f1[j], dec_f2[j], res);
        snprintf(nm, sizeof nm, "d%d.bnb", j + 6); add_bn(p, nm, dec_f2[j], res, c);
    }
    c = add_conv(p, "out", 1, ch[0], p->cfg.n_out, 0);
    p->layers[c].flags = IMK_LF_HEAD;

    // where every conv reads its input (the producer's BatchNorm, pooling and upsample+add are applied on load)
    const Topo t = make_topo(p);
    set_src(p, t.in_c, LM_U8, IMK_SRC_XA);
    set_src(p, t.e_c3[0], LM_AFFINE, t.in_c, t.in_bn);
    for (int i = 1; i < 4; ++i) set_src(p, t.e_c3[i], LM_POOL, t.e_c1[i - 1], t.e_bn[i - 1]);
    for (int i = 0; i < 4; ++i) set_src(p, t.e_c1[i], LM_RAW, t.e_c3[i]);
    set_src(p, t.b_c3, LM_POOL, t.e_c1[3], t.e_bn[3]);
    set_src(p, t.b_c1, LM_RAW, t.b_c3);
    for (int j = 0; j < 4; ++j) {
        const int lo_c = j == 0 ? t.b_c1 : t.d_c1[j - 1], lo_bn = j == 0 ? t.b_bn : t.d_bnb[j - 1];
        set_src(p, t.d_ca[j], LM_UPADD, lo_c, lo_bn, t.e_c1[3 - j], t.e_bn[3 - j]);
        set_src(p, t.d_c3[j], LM_AFFINE, t.d_ca[j], t.d_bna[j]);
        set_src(p, t.d_c1[j], LM_RAW, t.d_c3[j]);
    }
    set_src(p, t.out, LM_AFFINE, t.d_c1[3], t.d_bnb[3]);
    finish_layout(p);
}

Ws make_ws(const imk_unet_plan *p, int B, int mode) {
    Ws w;
    const Topo t = make_topo(p);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = up(off + bytes); return o; };
    make_ws_layers(p, B, mode, w, take);
    if (mode == 0) { w.sched = take(IMK_SCHED_BYTES * p->layers.size()); w.has_sched = true; }

    if (mode == 1) {
        for (int j = 0; j < 4; ++j) {  // decoder j+6 at res 3-j; u has the channels of ca's input
            const ImkLayer &ca = p->layers[t.d_ca[j]];
            const Dim d = res_dim(p->cfg, ca.res);
            w.dU[j] = take((size_t)B * d.h * d.w * imk_pad8(ca.cin) * 2);
        }
        for (int i = 0; i < 4; ++i) {  // pooled output of encoder i+1, at res i+1
            const ImkLayer &e = p->layers[t.e_c1[i]];
            const Dim d = res_dim(p->cfg, i + 1);
            w.dP[i] = take((size_t)B * d.h * d.w * imk_pad8(e.cout) * 2);
        }
        const size_t px = (size_t)B * p->cfg.h * p->cfg.w;
        w.dlogit = take(px * imk_pad8(p->cfg.n_out) * 2);
        w.loss_partial = take((size_t)imk_loss_blocks((long long)px) * sizeof(float));
        w.probs = take(px * p->cfg.n_out * sizeof(float));
        w.dice_partial = take((size_t)B * imk_dice_rows(B, p->cfg.h * p->cfg.w) * 3 * sizeof(float));
        w.dice_coef = take((size_t)B * 2 * sizeof(float));
        w.dice_val = take((size_t)B * sizeof(double));
    }
    w.total = off;
    return w;
}

int run_forward(Ctx &c, const Topo &t, float *probs, float *params_rw) {
    int rc;
    // inference: the tile counters of this forward's launches (dynamic walk of the persistent conv kernels) start at zero
    if (!c.train && c.ws.has_sched) IMK_HIP(hipMemsetAsync(c.base + c.ws.sched, 0, IMK_SCHED_BYTES * c.p->layers.size(), c.stream));
#define RUN(conv) do { rc = run_conv_fwd(c, (conv), params_rw); if (rc) return rc; } while (0)
    // Conv3x3+ReLU -> Conv1x1+ReLU pairs run as one kernel where the channel counts allow it
#define RUN_PAIR(c3, c1) do { rc = run_conv_pair(c, (c3), (c1), params_rw); if (rc) return rc; } while (0)
    // Inference: the input block (x/255 -> Conv1x1+ReLU -> BN, unet.py:4-9) is computed by the first encoder conv while it
    // stages its tile (LM_STEM), so the full-resolution stem tensor is neither written nor read.
    bool stem_fused = false;
    {
        const ImkLayer &st = c.p->layers[t.in_c], &c3 = c.p->layers[t.e_c3[0]];
        if (!c.train && !c.p->dbg_materialize && imk_conv_stem_fusable(st.cin, st.cout, c3.cout)) {
            ImkInput x{};
            x.in = c.x_in[0]; x.lmode = LM_STEM; x.cin = c3.cin; x.cs_in = imk_pad8(c3.cin); x.u8_c = st.cin;
            x.sc = c.bn_scale(t.in_bn); x.sh = c.bn_shift(t.in_bn);
            x.sc2 = c.params + st.off_w; x.sh2 = c.params + st.off_b;
            bool f = false;
            rc = run_conv_fwd(c, t.e_c3[0], params_rw, t.e_c1[0], &f, &x);
            if (rc == IMK_OK) stem_fused = true;
            else if (rc != IMK_EUNSUPPORTED) return rc;
        }
    }
    if (!stem_fused) { RUN(t.in_c); RUN_PAIR(t.e_c3[0], t.e_c1[0]); }
    for (int i = 1; i < 4; ++i) RUN_PAIR(t.e_c3[i], t.e_c1[i]);
    RUN_PAIR(t.b_c3, t.b_c1);
    for (int j = 0; j < 4; ++j) {
        rc = run_conv_pre_pair(c, t.d_ca[j], t.d_c3[j], t.d_c1[j]);      // inference, shallow levels: one launch per decoder block
        if (rc == IMK_OK) continue;
        if (rc != IMK_EUNSUPPORTED) return rc;
        RUN(t.d_ca[j]); RUN_PAIR(t.d_c3[j], t.d_c1[j]);
    }
#undef RUN_PAIR
#undef RUN
    if (!probs) return IMK_OK;   // training: the caller runs the fused head + loss kernel
    const ImkLayer &o = c.p->layers[t.out];
    const int bn = t.d_bnb[3];
    return imk_launch_head(c.act(t.d_c1[3]), c.bn_scale(bn), c.bn_shift(bn), c.params + o.off_w, c.params + o.off_b,
                           o.cin, imk_pad8(o.cin), o.cout, c.p->cfg.act_out, (long long)c.B * c.p->cfg.h * c.p->cfg.w,
                           probs, c.stream);
}

bool cfg_ok(const imk_unet_cfg *c) {
    if (!c) return false;
    if (c->h <= 0 || c->w <= 0 || (c->h % 16) || (c->w % 16)) return false;
    if (c->c_in < 1 || c->c_in > 8 || c->n_out < 1 || c->n_out > 64) return false;
    for (int i = 0; i < 5; ++i) if (c->ch[i] < 1 || c->ch[i] > 512) return false;
    if (imk_pad8(c->ch[0]) > 32) return false;  // head kernel instantiations
    return c->act_out == 0 || c->act_out == 1;
}

}  // namespace

// =====================================================================================================
// The process-wide side-stream pool (see imk_net.h: why one pool and not one pair of streams per plan).
static std::atomic<int> g_runtime_warnings{0};
hipStream_t imk_side_pool_stream(int i) {
    struct Pool { std::mutex mu; hipStream_t s[imk_unet_plan::MAX_SIDE] = {}; };
    static Pool pools[64];
    if (i < 0 || i >= imk_unet_plan::MAX_SIDE) return nullptr;
    // The HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), read when it starts.  With fewer than 8, a
    // side stream can land on the queue of the stream it is meant to run beside and the "concurrent" weight gradients queue up
    // behind barrier packets (-14 % on the ISIC generation with an RCCL stream in the process).  The Python package
    // exports 8 before the runtime starts; a bare C-ABI caller is told here, once.
    static std::once_flag hwq_once;
    std::call_once(hwq_once, []() {
        const char *e = getenv("GPU_MAX_HW_QUEUES");
        if (!e || atoi(e) < 8) {
            g_runtime_warnings.fetch_or(IMK_WARN_HW_QUEUES);
            fprintf(stderr, "libimk: GPU_MAX_HW_QUEUES=%s (< 8): side streams may serialise behind the caller's stream; "
                            "export GPU_MAX_HW_QUEUES=8 before the HIP runtime starts\n", e ? e : "unset");
        }
    });
    int dev = 0;
    (void)hipGetDevice(&dev);
    Pool &pool = pools[dev & 63];
    std::lock_guard<std::mutex> lock(pool.mu);
    if (!pool.s[i] && hipStreamCreateWithFlags(&pool.s[i], hipStreamNonBlocking) != hipSuccess) pool.s[i] = nullptr;
    return pool.s[i];
}

extern "C" int imk_runtime_warnings(void) { return g_runtime_warnings.load(); }

extern "C" int imk_unet_plan_side_stream(const imk_unet_plan *plan, int i, void **stream_out) {
    IMK_CHECK_ARG(plan && stream_out && i >= 0 && i < imk_unet_plan::MAX_SIDE);
    if (!ensure_side_streams(plan, i + 1)) return IMK_EINVAL;
    *stream_out = (void *)plan->side[i];
    return IMK_OK;
}

extern "C" int imk_unet_plan_create(const imk_unet_cfg *cfg, imk_unet_plan **out) {
    IMK_CHECK_ARG(out);
    if (!cfg_ok(cfg)) return IMK_EINVAL;
    if ((long long)cfg->h * cfg->w >= imk_conv_max_pixels() || cfg->w >= (1 << 16)) return IMK_EUNSUPPORTED;   // include/imk.h: image size limit
    imk_unet_plan *p = new (std::nothrow) imk_unet_plan();
    if (!p) return IMK_EINVAL;
    p->cfg = *cfg;
    build_layers(p);
    *out = p;
    return IMK_OK;
}

extern "C" void imk_unet_plan_destroy(imk_unet_plan *plan) {
    if (!plan) return;
    for (int i = 0; i < imk_unet_plan::MAX_SIDE; ++i) {
        if (!plan->side[i]) continue;
        (void)hipStreamSynchronize(plan->side[i]);      // the streams belong to the process-wide pool (imk_net.h)
        if (plan->ev_join[i]) (void)hipEventDestroy(plan->ev_join[i]);
    }
    for (auto &e : plan->ev_fork) if (e) (void)hipEventDestroy(e);
    for (auto &e : plan->ev_ring) if (e) (void)hipEventDestroy(e);
    delete plan;
}

extern "C" int imk_unet_param_count(const imk_unet_plan *plan, int64_t *total, int64_t *trainable) {
    IMK_CHECK_ARG(plan);
    if (total) *total = plan->n_total;
    if (trainable) *trainable = plan->n_trainable;
    return IMK_OK;
}

extern "C" int imk_unet_num_layers(const imk_unet_plan *plan) { return plan ? (int)plan->layers.size() : IMK_EINVAL; }

extern "C" int imk_unet_layer_info(const imk_unet_plan *plan, int idx, imk_layer_info *out) {
    IMK_CHECK_ARG(plan && out && idx >= 0 && idx < (int)plan->layers.size());
    const ImkLayer &l = plan->layers[idx];
    memset(out, 0, sizeof *out);
    strncpy(out->name, l.name.c_str(), sizeof(out->name) - 1);
    out->kind = l.kind; out->ksize = l.ksize; out->cin = l.cin; out->cout = l.cout;
    out->off_w = l.off_w; out->off_b = l.off_b; out->off_mean = l.off_mean; out->off_var = l.off_var;
    return IMK_OK;
}

extern "C" int imk_unet_plan_set_bn_momentum(imk_unet_plan *plan, float momentum) {
    IMK_CHECK_ARG(plan && momentum >= 0.f && momentum < 1.f);
    plan->bn_momentum = momentum;
    return IMK_OK;
}

extern "C" int imk_unet_plan_get_bn_momentum(const imk_unet_plan *plan, float *momentum) {
    IMK_CHECK_ARG(plan && momentum);
    *momentum = plan->bn_momentum;
    return IMK_OK;
}

extern "C" int imk_unet_plan_debug(imk_unet_plan *plan, int materialize, int single_stream) {
    IMK_CHECK_ARG(plan);
    if (materialize >= 0) plan->dbg_materialize = materialize != 0;
    if (single_stream >= 0) plan->dbg_single_stream = single_stream != 0;
    return IMK_OK;
}

extern "C" int64_t imk_unet_packed_bytes(const imk_unet_plan *plan) { return plan ? plan->packed_bytes : IMK_EINVAL; }


extern "C" int imk_unet_pack_weights(const imk_unet_plan *plan, const float *params, void *packed, void *stream_) {
    IMK_CHECK_ARG(plan && params && packed);
    // The layout has bytes no packing job writes (alignment gaps, the unused tail of a chain slot, the output layer's forward copy:
    // the head reads `params`).  They are zeroed so that `packed` is a function of `params` alone, whatever the buffer held.
    IMK_HIP(hipMemsetAsync(packed, 0, (size_t)plan->packed_bytes, (hipStream_t)stream_));
    return pack_weights(plan, params, packed, (hipStream_t)stream_, nullptr, nullptr, true);
}

extern "C" int64_t imk_unet_workspace_bytes(const imk_unet_plan *plan, int batch, int mode) {
    if (!plan || batch <= 0 || (mode != 0 && mode != 1)) return IMK_EINVAL;
    return (int64_t)make_ws(plan, batch, mode).total;
}

extern "C" int imk_unet_forward(const imk_unet_plan *plan, const float *params, const void *packed, const uint8_t *x,
                                int batch, float *probs, void *workspace, int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && params && packed && x && probs && workspace && batch > 0);
    Ctx c{plan, make_ws(plan, batch, 0), (uint8_t *)workspace, params, (const uint8_t *)packed, batch, false,
          (hipStream_t)stream_};
    if ((int64_t)c.ws.total > workspace_bytes) return IMK_EWORKSPACE;
    c.x_in[0] = x;
    return run_forward(c, make_topo(plan), probs, nullptr);
}

extern "C" int imk_unet_tensor_info(const imk_unet_plan *plan, int batch, int mode, int layer_idx, int which,
                                    int64_t *byte_offset, int *h, int *w, int *c, int *c_stride) {
    IMK_CHECK_ARG(plan && batch > 0 && layer_idx >= 0 && layer_idx < (int)plan->layers.size());
    IMK_CHECK_ARG(mode == 0 || mode == 1);
    const Ws ws = make_ws(plan, batch, mode);
    const ImkLayer &l = plan->layers[layer_idx];
    const Dim d = res_dim(plan->cfg, l.res);
    size_t off = 0;
    if (which == 0 && l.kind == 0 && layer_idx != plan->find("out")) off = ws.L[layer_idx].out;
    else if (which == 1 && l.kind == 0 && mode == 1) off = ws.L[layer_idx].dA;
    else if (which == 2 && l.kind == 1 && mode == 1) off = ws.L[layer_idx].dy;
    else return IMK_EINVAL;
    if (byte_offset) *byte_offset = (int64_t)off;
    if (h) *h = d.h;
    if (w) *w = d.w;
    if (c) *c = l.cout;
    if (c_stride) *c_stride = imk_pad8(l.cout);
    return IMK_OK;
}

// Ensemble inference + IM.  Workspace: n_models head slabs, then one activation workspace per concurrent stream.  A head
// slab holds what the IM stage reads of one model: its last decoder activation [B,H,W,cs] fp16 (fused head + IM kernel,
// the default) or its fp32 probabilities [B,H,W,K] (unfused: head_kernel per model + imk_im_*; taken for shapes the fused
// kernel does not cover, under imk_debug_materialize(1), and when the caller sized the slabs for probabilities only).
static size_t head_slab_bytes(const imk_unet_plan *plan, int batch, bool fused) {
    const imk_unet_cfg &cf = plan->cfg;
    const size_t px = (size_t)batch * cf.h * cf.w;
    const size_t probs = px * cf.n_out * sizeof(float), zlast = px * imk_pad8(cf.ch[0]) * sizeof(f16);
    return up(fused && zlast > probs ? zlast : probs);
}

extern "C" int64_t imk_unet_forward_im_workspace_bytes(const imk_unet_plan *plan, int n_models, int batch, int n_streams) {
    if (!plan || plan->net != 0 || n_models <= 0 || batch <= 0 || n_streams <= 0) return IMK_EINVAL;
    return (int64_t)(head_slab_bytes(plan, batch, true) * n_models + make_ws(plan, batch, 0).total * n_streams);
}

// Where the fused head of an ensemble finds each model: its last decoder activation and folded BatchNorm, its output layer.
struct EnsembleHeads {
    const f16 **z;
    const float **sc, **sh, **w, **bias;
};

// One forward of an ensemble call: model `model` (its index in params / packed / heads) on `batch` images -- the caller's input
// batch, or, with `gather`, the rows gather[0 .. batch) of it, compacted into the stream's input buffer first.
struct ForwardJob {
    int model, batch;
    const int64_t *gather;
    const Ws *ws;        // the activation workspace at this batch
    f16 *slab;           // fused: the model's head slab (its last decoder activation)
    float *probs;        // unfused: its fp32 probabilities
};

// The forward passes of an ensemble (imk_unet_forward_im, _im_members, _im_depth, _vote), a model nobody uses simply absent.  `regions`:
// per concurrent stream `per_stream` bytes, an input buffer of `xbuf` bytes (jobs with a gather list) and then an activation workspace.
// heads != NULL (fused): the last decoder activation of a job goes to its head slab and `heads` receives the pointers the fused
// kernel reads; no head launch.  heads == NULL: its fp32 probabilities go to `probs`.  Everything ends joined to `main_stream`.
static int run_ensemble_forwards(const imk_unet_plan *plan, const Topo &topo, const ForwardJob *jobs, int n_jobs,
                                 const float *const *params, const void *const *packed, const uint8_t *x, uint8_t *regions,
                                 size_t per_stream, size_t xbuf, int64_t regions_bytes, const EnsembleHeads *heads,
                                 hipStream_t main_stream) {
    const imk_unet_cfg &cf = plan->cfg;
    // The models are independent until the IM stage: with room for one region per stream (the caller passes its fixed part
    // + k regions, k <= 1 + MAX_SIDE) they run on k streams side by side -- the deep layers of one model fill the gaps of the
    // other's.  With room for one only, they run back to back.
    const int max_streams = 1 + imk_unet_plan::MAX_SIDE;
    int n_slabs = (int)((size_t)regions_bytes / per_stream);
    if (n_slabs > n_jobs) n_slabs = n_jobs;
    if (n_slabs > max_streams) n_slabs = max_streams;
    if (n_slabs > 1 && (plan->dbg_single_stream || !ensure_side_streams(plan, n_slabs - 1))) n_slabs = 1;
    if (n_slabs > 1) {
        IMK_HIP(hipEventRecord(plan->ev_fork[0], main_stream));
        for (int s = 1; s < n_slabs; ++s) IMK_HIP(hipStreamWaitEvent(plan->side[s - 1], plan->ev_fork[0], 0));
    }
    const ImkLayer &o = plan->layers[topo.out];
    const int64_t row_img = (int64_t)cf.h * cf.w * cf.c_in;
    for (int i = 0; i < n_jobs; ++i) {
        const ForwardJob &j = jobs[i];
        const int sl = i % n_slabs, m = j.model;
        hipStream_t st = sl == 0 ? main_stream : plan->side[sl - 1];
        uint8_t *region = regions + per_stream * sl;
        if (j.gather) {
            int rc = imk_gather_pairs(x, row_img, nullptr, 0, 0, 0, nullptr, j.gather, j.batch, region, nullptr, st);
            if (rc) return rc;
        }
        Ctx c{plan, *j.ws, region + xbuf, params[m], (const uint8_t *)packed[m], j.batch, false, st};
        c.x_in[0] = j.gather ? region : x;
        if (heads) {    // the last decoder activation goes to the model's head slab; no head launch
            c.ovr_conv = topo.d_c1[3];
            c.ovr_out = j.slab;
            heads->z[m] = c.ovr_out;
            heads->sc[m] = c.bn_scale(topo.d_bnb[3]); heads->sh[m] = c.bn_shift(topo.d_bnb[3]);
            heads->w[m] = params[m] + o.off_w; heads->bias[m] = params[m] + o.off_b;
        }
        int rc = run_forward(c, topo, heads ? nullptr : j.probs, nullptr);
        if (rc) return rc;
    }
    for (int s = 1; s < n_slabs; ++s) {
        IMK_HIP(hipEventRecord(plan->ev_join[s - 1], plan->side[s - 1]));
        IMK_HIP(hipStreamWaitEvent(main_stream, plan->ev_join[s - 1], 0));
    }
    return IMK_OK;
}

// Every model on the whole batch.  `slab` bytes per model at the start of the workspace, then one activation workspace per concurrent
// stream; unfused, model m's probabilities go to base + m * B*H*W*K*4 (the contiguous stack [N,B,H,W,K]: only the last slab may be
// padded).
static int run_ensemble_forwards(const imk_unet_plan *plan, const Topo &topo, const Ws &ws, int n_models, const float *const *params,
                                 const void *const *packed, const uint8_t *x, int batch, size_t slab, uint8_t *base,
                                 int64_t workspace_bytes, const EnsembleHeads *heads, hipStream_t main_stream) {
    const imk_unet_cfg &cf = plan->cfg;
    const size_t probs_exact = (size_t)batch * cf.h * cf.w * cf.n_out * sizeof(float);
    std::vector<ForwardJob> jobs;
    jobs.reserve(n_models);
    for (int m = 0; m < n_models; ++m)
        jobs.push_back({m, batch, nullptr, &ws, reinterpret_cast<f16 *>(base + slab * m), (float *)(base + probs_exact * m)});
    return run_ensemble_forwards(plan, topo, jobs.data(), n_models, params, packed, x, base + slab * n_models, ws.total, 0,
                                 workspace_bytes - (int64_t)(slab * n_models), heads, main_stream);
}

extern "C" int imk_unet_forward_im(const imk_unet_plan *plan, int n_models, const float *const *params,
                                   const void *const *packed, const uint8_t *x, int batch, float thr, int cmp_ge,
                                   const uint8_t *img, int block_in, int block_out, uint8_t *img_out, uint8_t *masks_out,
                                   uint8_t *im_out, int64_t *im_size, int64_t *pred_size, uint8_t *presence,
                                   void *workspace, int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && params && packed && x && workspace && batch > 0 && n_models > 0);
    const imk_unet_cfg &cf = plan->cfg;
    const Ws ws = make_ws(plan, batch, 0);
    const Topo topo = make_topo(plan);
    // fused head + IM?  (the kernel's shape limits, and room for the activation slabs)
    ImkHeadImArgs ha{};
    ha.n_models = n_models; ha.cin = cf.ch[0]; ha.cs = imk_pad8(cf.ch[0]); ha.K = cf.n_out; ha.softmax = cf.act_out;
    ha.batch = batch; ha.hw = cf.h * cf.w; ha.thr = thr; ha.cmp_ge = cmp_ge; ha.img = img; ha.c = cf.c_in;
    ha.block_in = block_in; ha.block_out = block_out; ha.img_out = img_out; ha.masks_out = masks_out; ha.im_out = im_out;
    ha.im_size = im_size; ha.pred_size = pred_size; ha.presence = presence;
    bool fused = !plan->dbg_materialize && imk_head_im_supported(ha) &&
                 (int64_t)(head_slab_bytes(plan, batch, true) * n_models + ws.total) <= workspace_bytes;
    const size_t slab = head_slab_bytes(plan, batch, fused);
    if ((int64_t)(slab * n_models + ws.total) > workspace_bytes) return IMK_EWORKSPACE;
    uint8_t *base = (uint8_t *)workspace;
    hipStream_t main_stream = (hipStream_t)stream_;
    const EnsembleHeads heads{ha.z, ha.sc, ha.sh, ha.w, ha.bias};
    int rc = run_ensemble_forwards(plan, topo, ws, n_models, params, packed, x, batch, slab, base, workspace_bytes,
                                   fused ? &heads : nullptr, main_stream);
    if (rc) return rc;
    if (fused) return imk_launch_head_im(ha, main_stream);
    if (cf.act_out == 0)
        return imk_im_binary((const float *)base, n_models, batch, cf.h, cf.w, cf.n_out, thr, cmp_ge, img, cf.c_in, block_in,
                             block_out, img_out, masks_out, im_out, im_size, pred_size, stream_);
    return imk_im_multiclass((const float *)base, n_models, batch, cf.h, cf.w, cf.n_out, img, cf.c_in, block_in, block_out,
                             img_out, masks_out, im_out, im_size, presence, stream_);
}

// Ensemble inference + IM over per-image members of a model pool.  Workspace: [member words u32 [B] | image lists int64 [N][B] |
// rows int32 [N][B] | N head slabs | per concurrent stream: a compacted input batch and an activation workspace].  Fused: model n
// runs on the images that use it (gathered by its list) and leaves their last decoder activations in its slab; one head + IM kernel
// (imk_im.hip) reads, for image b, the slabs of b's members at row[n][b].  Unfused (shapes the kernel does not cover, more than
// 8 members in some image, imk_debug_materialize(1)): every model that anybody uses runs on the whole batch into the fp32 stack
// [N,B,H,W,K] at the start of the slabs, then imk_im_*_members.
struct MembersLayout {
    size_t list, row, slabs, slab, xbuf, per_stream, fixed;
};
static MembersLayout members_layout(const imk_unet_plan *plan, int n_models, int batch) {
    const imk_unet_cfg &cf = plan->cfg;
    MembersLayout l;
    l.list = up((size_t)batch * sizeof(uint32_t));
    l.row = l.list + up((size_t)n_models * batch * sizeof(int64_t));
    l.slabs = l.row + up((size_t)n_models * batch * sizeof(int));
    l.slab = head_slab_bytes(plan, batch, true);
    l.xbuf = up((size_t)batch * cf.h * cf.w * cf.c_in);
    l.per_stream = l.xbuf + make_ws(plan, batch, 0).total;
    l.fixed = l.slabs + l.slab * n_models;
    return l;
}

extern "C" int64_t imk_unet_forward_im_members_workspace_bytes(const imk_unet_plan *plan, int n_models, int batch, int n_streams) {
    if (!plan || plan->net != 0 || n_models <= 0 || n_models > IMK_MEMBERS_MAX_POOL || batch <= 0 || n_streams <= 0) return IMK_EINVAL;
    const MembersLayout l = members_layout(plan, n_models, batch);
    return (int64_t)(l.fixed + l.per_stream * n_streams);
}

extern "C" int imk_unet_forward_im_members(const imk_unet_plan *plan, int n_models, const float *const *params,
                                           const void *const *packed, const uint8_t *x, int batch, const uint32_t *members_host,
                                           float thr, int cmp_ge, const uint8_t *img, int block_in, int block_out, uint8_t *img_out,
                                           uint8_t *masks_out, uint8_t *im_out, int64_t *im_size, int64_t *pred_size,
                                           uint8_t *presence, void *workspace, int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && plan->net == 0 && params && packed && x && members_host && workspace && batch > 0 && batch <= 65535);
    IMK_CHECK_ARG(n_models > 0 && n_models <= IMK_MEMBERS_MAX_POOL);
    IMK_CHECK_ARG(masks_out && im_out && im_size && (plan->cfg.act_out != 0 || pred_size) && (!img || img_out));
    const imk_unet_cfg &cf = plan->cfg;
    const MembersLayout lay = members_layout(plan, n_models, batch);
    if ((int64_t)(lay.fixed + lay.per_stream) > workspace_bytes) return IMK_EWORKSPACE;
    // each model's images, counted on the host
    const uint32_t pool = (n_models >= 32) ? 0xffffffffu : ((1u << n_models) - 1u);
    int count[IMK_MEMBERS_MAX_POOL] = {0}, max_members = 0;
    for (int b = 0; b < batch; ++b) {
        const uint32_t word = members_host[b] & pool;
        max_members = std::max(max_members, __builtin_popcount(word));
        for (int n = 0; n < n_models; ++n) count[n] += (word >> n) & 1u;
    }
    uint8_t *base = (uint8_t *)workspace;
    uint32_t *d_members = (uint32_t *)base;
    int64_t *d_list = (int64_t *)(base + lay.list);
    int *d_row = (int *)(base + lay.row);
    hipStream_t main_stream = (hipStream_t)stream_;
    const Topo topo = make_topo(plan);
    ImkHeadImMembersArgs ha{};
    ha.members = d_members; ha.row = d_row;
    ha.n_models = n_models; ha.cin = cf.ch[0]; ha.cs = imk_pad8(cf.ch[0]); ha.K = cf.n_out; ha.softmax = cf.act_out;
    ha.batch = batch; ha.hw = cf.h * cf.w; ha.thr = thr; ha.cmp_ge = cmp_ge; ha.img = img; ha.c = cf.c_in;
    ha.block_in = block_in; ha.block_out = block_out; ha.img_out = img_out; ha.masks_out = masks_out; ha.im_out = im_out;
    ha.im_size = im_size; ha.pred_size = pred_size; ha.presence = presence;
    const bool fused = !plan->dbg_materialize && imk_head_im_members_supported(ha, max_members);
    // Every model that somebody uses, fused on its own images (gathered by its list unless it has them all; the activation
    // workspace of a smaller batch fits the full batch's), unfused on the whole batch.
    Ws ws_of[IMK_MEMBERS_MAX_POOL];
    const Ws ws_full = make_ws(plan, batch, 0);
    const size_t probs_exact = (size_t)batch * cf.h * cf.w * cf.n_out * sizeof(float);
    ForwardJob jobs[IMK_MEMBERS_MAX_POOL];
    int n_jobs = 0;
    for (int n = 0; n < n_models; ++n) {
        if (!count[n]) continue;        // nobody uses this model
        const int nb = fused ? count[n] : batch;
        ws_of[n] = nb < batch ? make_ws(plan, nb, 0) : ws_full;
        if (ws_of[n].total > ws_full.total) return IMK_EWORKSPACE;
        jobs[n_jobs++] = {n, nb, nb < batch ? d_list + (size_t)n * batch : nullptr, &ws_of[n],
                          reinterpret_cast<f16 *>(base + lay.slabs + lay.slab * n), (float *)(base + lay.slabs + probs_exact * n)};
    }
    imk_launch_members_upload(members_host, batch, d_members, main_stream);
    IMK_LAUNCH_CHECK();
    if (fused) {
        imk_launch_members_lists(d_members, n_models, batch, d_list, d_row, main_stream);
        IMK_LAUNCH_CHECK();
    }
    const EnsembleHeads heads{ha.z, ha.sc, ha.sh, ha.w, ha.bias};
    int rc = run_ensemble_forwards(plan, topo, jobs, n_jobs, params, packed, x, base + lay.fixed, lay.per_stream, lay.xbuf,
                                   workspace_bytes - (int64_t)lay.fixed, fused ? &heads : nullptr, main_stream);
    if (rc) return rc;
    if (fused) return imk_launch_head_im_members(ha, max_members, main_stream);
    const float *stack = (const float *)(base + lay.slabs);
    if (cf.act_out == 0)
        return imk_im_binary_members(stack, d_members, n_models, batch, cf.h, cf.w, cf.n_out, thr, cmp_ge, img, cf.c_in, block_in,
                                     block_out, img_out, masks_out, im_out, im_size, pred_size, stream_);
    return imk_im_multiclass_members(stack, d_members, n_models, batch, cf.h, cf.w, cf.n_out, img, cf.c_in, block_in, block_out,
                                     img_out, masks_out, im_out, im_size, presence, stream_);
}

// Ensemble inference + the depth-map family's standard-deviation IM.  Workspace: [the std map, B*H*W fp32 | imk_unet_forward_im's
// workspace]: the model loop of imk_unet_forward_im, then the fused head + std kernel on the activation slabs (imk_depth.hip), or --
// for the shapes it does not cover -- imk_im_depth's first launch on the probability stack; the thresholds and the mask either way.
static size_t depth_map_bytes(const imk_unet_plan *plan, int batch) {
    return up((size_t)batch * plan->cfg.h * plan->cfg.w * sizeof(float));
}

extern "C" int64_t imk_unet_forward_im_depth_workspace_bytes(const imk_unet_plan *plan, int n_models, int batch, int n_streams) {
    const int64_t fwd = imk_unet_forward_im_workspace_bytes(plan, n_models, batch, n_streams);
    return fwd < 0 ? fwd : fwd + (int64_t)depth_map_bytes(plan, batch);
}

extern "C" int imk_unet_forward_im_depth(const imk_unet_plan *plan, int n_models, const float *const *params,
                                         const void *const *packed, const uint8_t *x, int batch, float mult, const uint8_t *img,
                                         int block_in, uint8_t *img_out, uint8_t *im_out, int64_t *im_size, float *thr_out,
                                         float *std_out, void *workspace, int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && plan->net == 0 && params && packed && x && workspace && batch > 0);
    IMK_CHECK_ARG(im_out && im_size && thr_out && (!img || img_out));
    const imk_unet_cfg &cf = plan->cfg;
    if (n_models < 2 || n_models > 16 || cf.act_out != 0 || cf.n_out != 1 || batch > 65535) return IMK_EUNSUPPORTED;
    const Ws ws = make_ws(plan, batch, 0);
    const Topo topo = make_topo(plan);
    const size_t map_bytes = depth_map_bytes(plan, batch);
    uint8_t *base = (uint8_t *)workspace + map_bytes;
    const int64_t fwd_bytes = workspace_bytes - (int64_t)map_bytes;
    float *map = std_out ? std_out : (float *)workspace;
    ImkDepthHeadArgs da{};
    da.n_models = n_models; da.cin = cf.ch[0]; da.cs = imk_pad8(cf.ch[0]); da.K = cf.n_out; da.softmax = cf.act_out;
    da.batch = batch; da.hw = cf.h * cf.w; da.map = map;
    const bool fused = !plan->dbg_materialize && imk_depth_head_supported(da) &&
                       (int64_t)(head_slab_bytes(plan, batch, true) * n_models + ws.total) <= fwd_bytes;
    const size_t slab = head_slab_bytes(plan, batch, fused);
    if (fwd_bytes < 0 || (int64_t)(slab * n_models + ws.total) > fwd_bytes) return IMK_EWORKSPACE;
    hipStream_t main_stream = (hipStream_t)stream_;
    const EnsembleHeads heads{da.z, da.sc, da.sh, da.w, da.bias};
    int rc = run_ensemble_forwards(plan, topo, ws, n_models, params, packed, x, batch, slab, base, fwd_bytes,
                                   fused ? &heads : nullptr, main_stream);
    if (rc) return rc;
    if (!fused)      // the stack [N,B,H,W] at the start of the slabs; its map is `map` (never the workspace imk_im_depth would take)
        return imk_im_depth((const float *)base, n_models, batch, cf.h, cf.w, mult, img, cf.c_in, block_in, img_out, im_out, im_size,
                            thr_out, map, nullptr, 0, stream_);
    rc = imk_launch_depth_head_std(da, main_stream);
    if (rc) return rc;
    return imk_depth_finish(map, batch, da.hw, mult, img, cf.c_in, block_in, img_out, im_out, im_size, thr_out, main_stream);
}

// Ensemble inference + model-ensemble vote: the model loop of imk_unet_forward_im, then the fused head + vote kernel
// (imk_vote.hip) on the activation slabs, or -- for the shapes it does not cover -- imk_vote_* on the probability stack.
// Workspace: imk_unet_forward_im_workspace_bytes.
extern "C" int imk_unet_forward_vote(const imk_unet_plan *plan, int n_models, const float *const *params,
                                     const void *const *packed, const uint8_t *x, int batch, double thr, int mode,
                                     uint8_t *masks_out, void *workspace, int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && plan->net == 0 && params && packed && x && masks_out && workspace && batch > 0 && n_models > 0);
    IMK_CHECK_ARG(mode == IMK_VOTE_HARD || mode == IMK_VOTE_SOFT);
    const imk_unet_cfg &cf = plan->cfg;
    const Ws ws = make_ws(plan, batch, 0);
    const Topo topo = make_topo(plan);
    ImkVoteHeadArgs va{};
    va.n_models = n_models; va.cin = cf.ch[0]; va.cs = imk_pad8(cf.ch[0]); va.K = cf.n_out; va.softmax = cf.act_out;
    va.batch = batch; va.hw = cf.h * cf.w; va.thr = thr; va.mode = mode; va.out = masks_out;
    const bool fused = !plan->dbg_materialize && imk_vote_head_supported(va) &&
                       (int64_t)(head_slab_bytes(plan, batch, true) * n_models + ws.total) <= workspace_bytes;
    const size_t slab = head_slab_bytes(plan, batch, fused);
    if ((int64_t)(slab * n_models + ws.total) > workspace_bytes) return IMK_EWORKSPACE;
    uint8_t *base = (uint8_t *)workspace;
    hipStream_t main_stream = (hipStream_t)stream_;
    const EnsembleHeads heads{va.z, va.sc, va.sh, va.w, va.bias};
    int rc = run_ensemble_forwards(plan, topo, ws, n_models, params, packed, x, batch, slab, base, workspace_bytes,
                                   fused ? &heads : nullptr, main_stream);
    if (rc) return rc;
    if (fused) return imk_launch_vote_head(va, main_stream);
    if (cf.act_out == 0) return imk_vote_binary((const float *)base, n_models, batch, cf.h, cf.w, cf.n_out, thr, mode, masks_out, stream_);
    return imk_vote_multiclass((const float *)base, n_models, batch, cf.h, cf.w, cf.n_out, mode, masks_out, stream_);
}

// Input ensemble: one model's forward over the B*M views as one batch.  Fused: the last decoder activation of the whole batch goes
// to a head slab and one vote kernel reads it -- the D4-restoring kernel (imk_views.hip) for ops != NULL, the model-ensemble head
// kernel (imk_vote.hip) with member m = slice m of the slab and the same weights for every member otherwise.  Unfused: per image
// chunk, one forward per view into an fp32 stack [M,bc,H,W,K], then the stack vote; bc is the largest chunk whose stack and
// activation workspace fit the fused route's workspace.
extern "C" int64_t imk_unet_forward_views_vote_workspace_bytes(const imk_unet_plan *plan, int n_views, int batch) {
    if (!plan || plan->net != 0 || n_views <= 0 || batch <= 0) return IMK_EINVAL;
    const int mb = n_views * batch;
    return (int64_t)(head_slab_bytes(plan, mb, true) + make_ws(plan, mb, 0).total);
}

extern "C" int imk_unet_forward_views_vote(const imk_unet_plan *plan, const float *params, const void *packed,
                                           const uint8_t *views, int n_views, int batch, const int *ops, int any_quarter_turn,
                                           double thr, int mode, int cmp_ge, uint8_t *masks_out, void *workspace,
                                           int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && plan->net == 0 && params && packed && views && masks_out && workspace && batch > 0 && n_views > 0);
    const imk_unet_cfg &cf = plan->cfg;
    const bool sigmoid = cf.act_out == 0;
    IMK_CHECK_ARG(mode == IMK_VOTE_HARD || mode == IMK_VOTE_SOFT || (!sigmoid && mode == IMK_VOTE_MAJORITY));
    IMK_CHECK_ARG(!ops || (sigmoid && mode == IMK_VOTE_HARD));
    if (ops && any_quarter_turn && cf.h != cf.w) return IMK_EUNSUPPORTED;
    const int mb = n_views * batch;
    IMK_CHECK_ARG(mb <= 65535);
    const Topo topo = make_topo(plan);
    const ImkLayer &o = plan->layers[topo.out];
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t *base = (uint8_t *)workspace;
    const int hw = cf.h * cf.w, cs = imk_pad8(cf.ch[0]);
    ImkViewVoteArgs da{};     // D4-restoring (ops)
    da.ops = ops; da.ops_ld = batch; da.n_views = n_views; da.cin = cf.ch[0]; da.cs = cs; da.K = cf.n_out; da.batch = batch;
    da.h = cf.h; da.w = cf.w; da.thr = thr; da.cmp_ge = cmp_ge; da.out = masks_out;
    ImkVoteHeadArgs va{};     // identity maps
    va.n_models = n_views; va.cin = cf.ch[0]; va.cs = cs; va.K = cf.n_out; va.softmax = cf.act_out; va.batch = batch; va.hw = hw;
    va.thr = thr; va.mode = mode; va.out = masks_out;
    const bool kernel_ok = ops ? imk_views_vote_head_supported(da)
                               : (mode != IMK_VOTE_MAJORITY && !(sigmoid && cmp_ge) && imk_vote_head_supported(va));
    const Ws ws = make_ws(plan, mb, 0);
    const size_t slab = head_slab_bytes(plan, mb, true);
    if (!plan->dbg_materialize && kernel_ok && (int64_t)(slab + ws.total) <= workspace_bytes) {
        Ctx c{plan, ws, base + slab, params, (const uint8_t *)packed, mb, false, stream};
        c.x_in[0] = views;
        c.ovr_conv = topo.d_c1[3];
        c.ovr_out = reinterpret_cast<f16 *>(base);
        const float *sc = c.bn_scale(topo.d_bnb[3]), *sh = c.bn_shift(topo.d_bnb[3]);
        int rc = run_forward(c, topo, nullptr, nullptr);
        if (rc) return rc;
        if (ops) {
            da.z = c.ovr_out; da.sc = sc; da.sh = sh; da.wt = params + o.off_w; da.bias = params + o.off_b;
            return imk_launch_views_vote_head(da, stream);
        }
        for (int m = 0; m < n_views; ++m) {
            va.z[m] = c.ovr_out + (size_t)m * batch * hw * cs;
            va.sc[m] = sc; va.sh[m] = sh; va.w[m] = params + o.off_w; va.bias[m] = params + o.off_b;
        }
        return imk_launch_vote_head(va, stream);
    }
    // unfused: image chunks of bc, the stack [M,bc,H,W,K] at the start of the workspace
    const size_t img_probs = (size_t)hw * cf.n_out * sizeof(float);
    int bc = batch;
    while (bc > 0 && (int64_t)(up(img_probs * n_views * bc) + make_ws(plan, bc, 0).total) > workspace_bytes) bc = bc > 8 ? bc * 3 / 4 : bc - 1;
    if (bc <= 0) return IMK_EWORKSPACE;
    float *stack = (float *)base;
    const size_t hwc = (size_t)hw * cf.c_in;
    for (int b0 = 0; b0 < batch; b0 += bc) {
        const int n = batch - b0 < bc ? batch - b0 : bc;
        const Ws wsc = make_ws(plan, n, 0);
        for (int m = 0; m < n_views; ++m) {
            Ctx c{plan, wsc, base + up(img_probs * n_views * bc), params, (const uint8_t *)packed, n, false, stream};
            c.x_in[0] = views + ((size_t)m * batch + b0) * hwc;
            int rc = run_forward(c, topo, stack + (size_t)m * n * hw * cf.n_out, nullptr);
            if (rc) return rc;
        }
        int rc;
        if (ops)
            rc = imk_vote_views_binary_ld(stack, n_views, n, cf.h, cf.w, cf.n_out, ops + b0, batch, thr, cmp_ge,
                                          masks_out + (size_t)b0 * cf.n_out * hw, stream);
        else if (sigmoid && cmp_ge && mode == IMK_VOTE_HARD)
            rc = imk_vote_views_binary_ld(stack, n_views, n, cf.h, cf.w, cf.n_out, nullptr, 0, thr, 1,
                                          masks_out + (size_t)b0 * cf.n_out * hw, stream);
        else if (sigmoid)
            rc = imk_vote_binary(stack, n_views, n, cf.h, cf.w, cf.n_out, thr, mode, masks_out + (size_t)b0 * cf.n_out * hw, stream_);
        else if (mode == IMK_VOTE_MAJORITY)
            rc = imk_vote_views_majority(stack, n_views, n, cf.h, cf.w, cf.n_out, masks_out + (size_t)b0 * hw, stream_);
        else
            rc = imk_vote_multiclass(stack, n_views, n, cf.h, cf.w, cf.n_out, mode, masks_out + (size_t)b0 * hw, stream_);
        if (rc) return rc;
    }
    return IMK_OK;
}

// Noisy student: the teacher's forward, the label, and the SAME flips / quarter turn on image and label.  Fused: the last decoder
// activation goes to a head slab and one kernel (imk_student.hip) applies the output layer, thresholds or arg-maxes, and stores
// the label in the moved frame, while imk_augment's image path runs on a side stream forked from and joined to `stream`.
// Unfused (shapes the kernel does not cover, imk_unet_plan_debug(materialize), IMK_STUDENT_FUSED=0): imk_unet_forward -> the single-member vote kernels
// as the label rule -> imk_augment with the label as its mask (planar maps of a several-map sigmoid head: image alone + the plane
// mover), all on `stream`.  Workspace: [head slab | un-moved label | activations].
static size_t student_label_bytes(const imk_unet_plan *plan, int batch) {
    const imk_unet_cfg &cf = plan->cfg;
    return up((size_t)batch * cf.h * cf.w * (cf.act_out == 0 ? cf.n_out : 1));
}

extern "C" int64_t imk_unet_forward_student_workspace_bytes(const imk_unet_plan *plan, int batch) {
    if (!plan || plan->net != 0 || batch <= 0) return IMK_EINVAL;
    return (int64_t)(head_slab_bytes(plan, batch, true) + student_label_bytes(plan, batch) + make_ws(plan, batch, 0).total);
}

extern "C" int imk_unet_forward_student(const imk_unet_plan *plan, const float *params, const void *packed, const uint8_t *x,
                                        const uint8_t *img, int batch, float thr, int cmp_ge, const imk_aug_params *aug,
                                        int any_quarter_turn, uint8_t *img_out, uint8_t *labels_out, void *workspace,
                                        int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && plan->net == 0 && params && packed && x && img && aug && img_out && labels_out && workspace && batch > 0);
    IMK_CHECK_ARG(img != img_out && batch <= 65535);
    const imk_unet_cfg &cf = plan->cfg;
    if (any_quarter_turn && cf.h != cf.w) return IMK_EUNSUPPORTED;   // the outputs would change shape: refused before any launch
    const Ws ws = make_ws(plan, batch, 0);
    const size_t slab = head_slab_bytes(plan, batch, true), lab = student_label_bytes(plan, batch);
    if ((int64_t)(slab + lab + ws.total) > workspace_bytes) return IMK_EWORKSPACE;
    const Topo topo = make_topo(plan);
    const ImkLayer &o = plan->layers[topo.out];
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t *base = (uint8_t *)workspace;
    const bool sigmoid = cf.act_out == 0;
    ImkStudentArgs sa{};
    sa.aug = aug; sa.cin = cf.ch[0]; sa.cs = imk_pad8(cf.ch[0]); sa.K = cf.n_out; sa.softmax = cf.act_out; sa.batch = batch;
    sa.h = cf.h; sa.w = cf.w; sa.thr = thr; sa.cmp_ge = cmp_ge; sa.out = labels_out;
    Ctx c{plan, ws, base + slab + lab, params, (const uint8_t *)packed, batch, false, stream};
    c.x_in[0] = x;
    if (!plan->dbg_materialize && imk_switches().student_fused && imk_student_head_supported(sa)) {
        // The augmented image needs only img and the draws: on a side stream beside the forward (blur is the expensive part).  Not for
        // the narrowest nets (last decoder width 8, ISIC's alpha 0.5): their forward of 32 images takes 0.23 ms, the schedules pair
        // that width with no blur, and the fork + join then cost more than the image path hides (noisy student).
        const bool side = sa.cs > 8 && !plan->dbg_single_stream && ensure_side_streams(plan, 1);
        hipStream_t s_img = side ? plan->side[0] : stream;
        if (side) {
            IMK_HIP(hipEventRecord(plan->ev_fork[0], stream));
            IMK_HIP(hipStreamWaitEvent(s_img, plan->ev_fork[0], 0));
        }
        int rc = imk_augment(img, nullptr, batch, cf.h, cf.w, cf.c_in, 0, aug, img_out, nullptr, any_quarter_turn, s_img);
        if (side) IMK_HIP(hipEventRecord(plan->ev_join[0], s_img));      // recorded even after an error: `stream` is always joined
        c.ovr_conv = topo.d_c1[3];
        c.ovr_out = reinterpret_cast<f16 *>(base);
        sa.z = c.ovr_out; sa.sc = c.bn_scale(topo.d_bnb[3]); sa.sh = c.bn_shift(topo.d_bnb[3]);
        sa.wt = params + o.off_w; sa.bias = params + o.off_b;
        if (!rc) rc = run_forward(c, topo, nullptr, nullptr);
        if (!rc) rc = imk_launch_student_head(sa, stream);
        if (side) IMK_HIP(hipStreamWaitEvent(stream, plan->ev_join[0], 0));
        return rc;
    }
    float *probs = (float *)base;
    uint8_t *label = base + slab;
    int rc = run_forward(c, topo, probs, nullptr);
    if (rc) return rc;
    if (sigmoid) rc = imk_vote_views_binary_ld(probs, 1, batch, cf.h, cf.w, cf.n_out, nullptr, 0, thr, cmp_ge, label, stream);
    else rc = imk_vote_multiclass(probs, 1, batch, cf.h, cf.w, cf.n_out, IMK_VOTE_HARD, label, stream_);
    if (rc) return rc;
    if (!sigmoid || cf.n_out == 1)      // one label plane: [B,H,W] is imk_augment's [B,H,W,1] mask
        return imk_augment(img, label, batch, cf.h, cf.w, cf.c_in, 1, aug, img_out, labels_out, any_quarter_turn, stream_);
    rc = imk_augment(img, nullptr, batch, cf.h, cf.w, cf.c_in, 0, aug, img_out, nullptr, any_quarter_turn, stream_);
    if (rc) return rc;
    return imk_student_move_planes(label, batch, cf.n_out, cf.h, cf.w, aug, labels_out, stream);
}

// =====================================================================================================
// training
// =====================================================================================================

extern "C" int64_t imk_unet_state_bytes(const imk_unet_plan *plan) {
    if (!plan) return IMK_EINVAL;
    return (int64_t)(2 * up((size_t)plan->n_trainable * sizeof(float)) + up(sizeof(ImkCtl)));
}

extern "C" int imk_unet_state_init(const imk_unet_plan *plan, void *state, void *stream_) {
    IMK_CHECK_ARG(plan && state);
    hipStream_t stream = (hipStream_t)stream_;
    IMK_HIP(hipMemsetAsync(state, 0, (size_t)imk_unet_state_bytes(plan), stream));
    return imk_launch_ctl_init(state_view(plan, state).ctl, stream);
}

namespace {

// The output layer's weight / bias gradient as partial rows some head kernel has already written (run_backward queues their reduction).
struct HeadWgJob { float *partial; int rows; };

// The head's dgrad / weight-gradient launches of a step whose logit gradient is a stored tensor (the labelled step where no one-pass
// head kernel covers the shape; both views of the consistency step's composed route).  *rows: statistics rows of the last BatchNorm's
// dy; *job: set where the dgrad launch produced the weight-gradient rows itself.
template <typename LossHook>
int head_dgrad(Bwd &b, const Topo &t, f16 *dlogit, LossHook &&loss_on_side, int *head_rows, HeadWgJob *job) {
    Ctx &c = b.c;
    const imk_unet_cfg &cf = c.p->cfg;
    const ImkLayer &ol = c.p->layers[t.out];
    const int obn = t.d_bnb[3];
    int rc;
#define OK(e) do { rc = (e); if (rc) return rc; } while (0)
    // head: its "dA" is dlogit.  Its dgrad (dlogit -> dy of the last BatchNorm, with that BN's gradient statistics) reads
    // exactly the operands of its weight gradient (dlogit, and z = the last decoder activation, whose BatchNorm output is
    // the head's input): where the pipelined kernel covers the shape, one launch produces both.
    ImkConvArgs ha{};
    ha.x.in = dlogit; ha.x.lmode = LM_RAW; ha.x.cin = ol.cout; ha.x.cs_in = imk_pad8(ol.cout);
    ha.B = c.B; ha.H = cf.h; ha.W = cf.w; ha.ksize = 1; ha.cout = ol.cin; ha.cs_out = imk_pad8(ol.cin);
    ha.wpk = c.wbwd(t.out); ha.out = c.dy(obn); ha.epi = EP_PLAIN;
    ha.dystat_z = c.act(t.d_c1[3]);
    ha.stats_partial = reinterpret_cast<float *>(c.base + c.ws.L[obn].bwd_partial);
    const bool head_fused = imk_conv_can_fuse_wgrad(ha);
    if (!head_fused) OK(b.wgrad(t.out, dlogit));
    // the loss value only needs head_loss_kernel's partials: its reduction rides on the side stream, behind the head's
    // weight gradient, instead of sitting at the end of the step
    OK(loss_on_side());
    int rows = 0;
    ha.stats_rows = &rows;
    if (head_fused) {
        ha.wg_partial = reinterpret_cast<float *>(c.base + c.ws.L[t.out].wg_partial);
        ha.wg_sc = c.bn_scale(obn); ha.wg_sh = c.bn_shift(obn);
    }
    OK(imk_launch_conv(ha, c.stream));
    if (rows <= 0 || rows > c.ws.L[obn].n_bwd_rows) return IMK_EWORKSPACE;
    *head_rows = rows;
    if (head_fused) {
        if (rows > imk_conv_fused_wgrad_rows_max()) return IMK_EWORKSPACE;
        *job = HeadWgJob{ha.wg_partial, rows};
    }
#undef OK
    return IMK_OK;
}

// Everything of a backward pass below the head: decoders 9..6, bottleneck, encoders 4..1, input block, and the reduction of every
// weight gradient into b.grads.  On entry the last BatchNorm's dy is stored with `head_rows` rows of its gradient statistics, and
// `head_job` (optional) holds the output layer's weight-gradient rows.  loss_on_side: called wherever a fork to the side stream exists.
template <typename LossHook>
int run_backward(Bwd &b, const Topo &t, int head_rows, const HeadWgJob *head_job, LossHook &&loss_on_side) {
    Ctx &c = b.c;
    const ImkLayer &ol = c.p->layers[t.out];
    int rc;
#define OK(e) do { rc = (e); if (rc) return rc; } while (0)
    b.dy_rows[t.d_bnb[3]] = head_rows;
    if (head_job)
        OK(imk_wgf_add_job(b.jobs, head_job->partial, head_job->rows, ol.ksize, ol.cin, ol.cout, b.grads + ol.off_w, b.grads + ol.off_b));
    // decoders 9..6
    for (int j = 3; j >= 0; --j) {
        f16 *dU = reinterpret_cast<f16 *>(c.base + c.ws.dU[j]);
        if (j == 3) OK(b.bn_bwd(t.d_bnb[j], 0, nullptr, nullptr));
        else OK(b.bn_bwd(t.d_bnb[j], 2, nullptr, reinterpret_cast<f16 *>(c.base + c.ws.dU[j + 1])));
        OK(b.wgrad_dgrad(t.d_c1[j], c.dA(t.d_c3[j]), c.act(t.d_c3[j])));
        OK(b.wgrad_dgrad(t.d_c3[j], c.dy(t.d_bna[j]), nullptr, t.d_bna[j]));
        OK(b.bn_bwd(t.d_bna[j], 0, nullptr, nullptr));
        b.sum2_bn = j > 0 ? t.d_bnb[j - 1] : t.b_bn;     // dU's 2x2 sums = dy of the block below: assembled by this dgrad where it can
        OK(b.wgrad_dgrad(t.d_ca[j], dU, nullptr));
        OK(b.flush_block());    // the block's weight gradients (and the head's, for the first block) -> side stream
        OK(loss_on_side());
    }
    // bottleneck: dy = 2x2 sum of dU[decoder 6]
    OK(b.bn_bwd(t.b_bn, 2, nullptr, reinterpret_cast<f16 *>(c.base + c.ws.dU[0])));
    OK(b.wgrad_dgrad(t.b_c1, c.dA(t.b_c3), c.act(t.b_c3)));
    OK(b.wgrad_dgrad(t.b_c3, reinterpret_cast<f16 *>(c.base + c.ws.dP[3]), nullptr));
    OK(b.flush_block());
    // encoders 4..1: dy = skip gradient (dU of decoder 6+(3-i)) + max-pool scatter of dP[i]
    for (int i = 3; i >= 0; --i) {
        if (i == 0) {
            b.defer_finalize = true;   // last block: nothing left to hide its split reductions behind
            b.hold_conv = t.e_c3[0];
        }
        OK(b.bn_bwd(t.e_bn[i], 1, reinterpret_cast<f16 *>(c.base + c.ws.dU[3 - i]),
                    reinterpret_cast<f16 *>(c.base + c.ws.dP[i])));
        OK(b.wgrad_dgrad(t.e_c1[i], c.dA(t.e_c3[i]), c.act(t.e_c3[i])));
        f16 *dst = i > 0 ? reinterpret_cast<f16 *>(c.base + c.ws.dP[i - 1]) : c.dy(t.in_bn);
        OK(b.wgrad_dgrad(t.e_c3[i], dst, nullptr, i > 0 ? -1 : t.in_bn));
        OK(i > 0 ? b.flush_block() : b.flush_wgrads());
    }
    OK(b.bn_bwd(t.in_bn, 0, nullptr, nullptr));
    if (b.has_held) {
        OK(b.wgrad(t.in_c));                        // full resolution: forked onto the side stream at once
        b.pending[b.n_pending++] = b.held;          // launched on the main stream by finish_wgrads
    } else {
        OK(b.wgrad(t.in_c, nullptr, true));
    }
    OK(b.finish_wgrads());
#undef OK
    return IMK_OK;
}

}  // namespace

extern "C" int imk_unet_fwd_bwd(const imk_unet_plan *plan, float *params, void *packed, void *state, const uint8_t *x,
                                const uint8_t *y, int batch, int loss_kind, float *grads, float *stats, void *workspace,
                                int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && params && packed && state && x && y && grads && stats && workspace && batch > 0);
    IMK_CHECK_ARG(loss_kind >= 0 && loss_kind <= 4);
    IMK_CHECK_ARG((loss_kind != 1) == (plan->cfg.act_out == 0));  // mse / rmse / Dice <-> sigmoid head, cce <-> softmax head
    const int y255 = loss_kind == 2 || loss_kind == 3;            // kinds 2, 3: continuous targets y / 255.0f
    const bool dice = loss_kind == 4;                             // the per-image Dice loss: sums -> coefficients -> gradient (imk_dice.hip)
    const int fin_kind = loss_kind == 1 ? 1 : 0;                  // the loss finalize's denominator: every element, or every pixel
    hipStream_t stream = (hipStream_t)stream_;
    Ctx c{plan, make_ws(plan, batch, 1), (uint8_t *)workspace, params, (const uint8_t *)packed, batch, true, stream};
    if ((int64_t)c.ws.total > workspace_bytes) return IMK_EWORKSPACE;
    c.x_in[0] = x;
    const StateView sv = state_view(plan, state);
    const imk_unet_cfg &cf = plan->cfg;
    const Topo t = make_topo(plan);
    const long long n_pix = (long long)batch * cf.h * cf.w;
    int rc;
#define OK(e) do { rc = (e); if (rc) return rc; } while (0)
    OK(run_forward(c, t, nullptr, params));

    // head + loss + d(loss*scale)/d(logits) in one pass over the last activation
    f16 *dlogit = reinterpret_cast<f16 *>(c.base + c.ws.dlogit);
    float *loss_partial = reinterpret_cast<float *>(c.base + c.ws.loss_partial);
    const ImkLayer &ol = plan->layers[t.out];
    const int obn = t.d_bnb[3];
    // softmax heads: the loss, the gradient of the last BatchNorm's output (with its statistics) and the output layer's weight
    // gradient come out of ONE kernel that reads the last activation once (imk_headf.hip); sigmoid heads: head_loss_kernel,
    // then the output layer's dgrad (+ fused weight gradient where the pipelined kernel covers the shape)
    const bool head_one_pass = cf.act_out == 1 &&
                               imk_head_cce_fused_ok(imk_pad8(ol.cin), ol.cout, n_pix, c.ws.L[obn].n_bwd_rows);
    // sigmoid heads with 1 / 3 maps on <= 16 channels (ISIC, HeLa): the same in one pass (head_mse_fused_kernel, round 4)
    const bool head_mse_pass = cf.act_out == 0 && imk_head_mse_fused_ok(imk_pad8(ol.cin), ol.cout, n_pix, c.ws.L[obn].n_bwd_rows) &&
                               (!dice || imk_switches().dice_fused);
    float *dice_coef = reinterpret_cast<float *>(c.base + c.ws.dice_coef);
    if (dice) {
        float *rows = reinterpret_cast<float *>(c.base + c.ws.dice_partial);
        OK(imk_launch_dice_sums(c.act(t.d_c1[3]), c.bn_scale(obn), c.bn_shift(obn), params + ol.off_w, params + ol.off_b, ol.cin,
                                imk_pad8(ol.cin), ol.cout, batch, cf.h * cf.w, y, sv.ctl, stats, rows, stream));
        OK(imk_launch_dice_coef(rows, batch, cf.h * cf.w, dice_coef, reinterpret_cast<double *>(c.base + c.ws.dice_val), stats, stream));
        if (!head_mse_pass)
            OK(imk_launch_dice_dlogit(c.act(t.d_c1[3]), c.bn_scale(obn), c.bn_shift(obn), params + ol.off_w, params + ol.off_b, ol.cin,
                                      imk_pad8(ol.cin), ol.cout, n_pix, cf.h * cf.w, y, sv.ctl, dice_coef, dlogit, stream));
    } else if (!head_one_pass && !head_mse_pass)
        OK(imk_launch_head_loss(c.act(t.d_c1[3]), c.bn_scale(obn), c.bn_shift(obn), params + ol.off_w, params + ol.off_b, ol.cin,
                                imk_pad8(ol.cin), ol.cout, cf.act_out, n_pix, y, sv.ctl, stats, dlogit, loss_partial, stream, y255));

    // The weight-gradient kernels run on a side stream, forked after the kernel that produced their gradient operand and
    // joined before the final reduction: nothing on the backward chain depends on them, and they fill the gaps that the
    // latency-bound kernels of the chain leave (1.280 vs 1.365 ms per step with all 24 on the side stream; forking only
    // the deep layers' was neutral).
    const int n_side = imk_switches().side_streams;
    const bool side_on = !plan->dbg_single_stream && n_side > 0 && ensure_side_streams(plan, n_side);
    Bwd b{c, grads, sv.ctl, stats + 1, side_on ? n_side : 0};
    ImkStopRingScope stop_ring(plan, stream, b.n_side);      // from here on: the backward pass's launches carry their own events
    bool loss_done = dice;                  // kind 4: dice_coef_kernel wrote stats[0]
    auto loss_on_side = [&]() -> int {      // once, as soon as a fork exists (every fork event is younger than the head's kernel)
        if (loss_done || b.n_side <= 0 || b.n_fork <= 0 || loss_kind == 3) return IMK_OK;      // kind 3: on `stream`, in front of its scaling launch
        loss_done = true;
        return imk_launch_loss_finalize(loss_partial, n_pix, cf.n_out, fin_kind, stats, plan->side[(b.n_fork - 1) % b.n_side]);
    };
    int head_rows = 0;
    HeadWgJob head_job{};
    if (head_mse_pass) {
        const int rows = imk_head_cce_fused_rows(n_pix);
        float *wgp = reinterpret_cast<float *>(c.base + c.ws.L[t.out].wg_partial);
        OK(imk_launch_head_mse_fused(c.act(t.d_c1[3]), c.bn_scale(obn), c.bn_shift(obn), params + ol.off_w, params + ol.off_b,
                                     ol.cin, imk_pad8(ol.cin), ol.cout, n_pix, y, sv.ctl, stats, c.dy(obn), loss_partial,
                                     reinterpret_cast<float *>(c.base + c.ws.L[obn].bwd_partial), wgp, stream, y255,
                                     dice ? dice_coef : nullptr, cf.h * cf.w));
        head_rows = rows;
        head_job = HeadWgJob{wgp, rows};
    } else if (head_one_pass) {
        const int rows = imk_head_cce_fused_rows(n_pix);
        float *wgp = reinterpret_cast<float *>(c.base + c.ws.L[t.out].wg_partial);
        OK(imk_launch_head_cce_fused(c.act(t.d_c1[3]), c.bn_scale(obn), c.bn_shift(obn), params + ol.off_w, params + ol.off_b,
                                     ol.cin, imk_pad8(ol.cin), ol.cout, n_pix, y, sv.ctl, stats, c.dy(obn), loss_partial,
                                     reinterpret_cast<float *>(c.base + c.ws.L[obn].bwd_partial), wgp, stream));
        head_rows = rows;
        head_job = HeadWgJob{wgp, rows};
    } else {
        OK(head_dgrad(b, t, dlogit, loss_on_side, &head_rows, &head_job));
    }
    OK(run_backward(b, t, head_rows, head_job.partial ? &head_job : nullptr, loss_on_side));
    if (!loss_done) OK(imk_launch_loss_finalize(loss_partial, n_pix, cf.n_out, fin_kind, stats, stream));
    if (loss_kind == 3) {      // rmse: the mse step's gradients times 0.5 / sqrt(mse), behind the finalize and every gradient's reduction
        int64_t n_total = 0, n_train = 0;
        OK(imk_unet_param_count(plan, &n_total, &n_train));
        OK(imk_launch_rmse_scale(loss_partial, n_pix, cf.n_out, grads, n_train, stats, stream));
    }
#undef OK
    return IMK_OK;
}

// Consistency-loss step (functions.py:367-474 of the reference): two training-mode forwards on two views of one unlabelled batch,
// L = mean (p1 - p2)^2, the gradient through both forwards.  Workspace: [view 1's training workspace | view 2's | the second
// gradient vector | the head's loss partials]; the fused head's weight-gradient rows (both views in one set) take the output layer's
// own partial buffer in view 1's workspace, which is sized for one row per head workgroup plus the reduction's scratch behind them.
// Everything runs in order on `stream` (the weight gradients inside each backward pass fork to the side stream as in the labelled step).
namespace {
struct ConsistLayout {
    Ws ws;
    size_t view[2], grads2, loss_partial, total;
};
ConsistLayout consist_layout(const imk_unet_plan *plan, int batch) {
    ConsistLayout l{make_ws(plan, batch, 1), {0, 0}, 0, 0, 0};
    const int rows = imk_loss_blocks((long long)batch * plan->cfg.h * plan->cfg.w);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = up(off + bytes); return o; };
    l.view[0] = take(l.ws.total);
    l.view[1] = take(l.ws.total);
    l.grads2 = take((size_t)plan->n_trainable * sizeof(float));
    l.loss_partial = take((size_t)rows * sizeof(float));
    l.total = off;
    return l;
}
}  // namespace

extern "C" int64_t imk_unet_consistency_workspace_bytes(const imk_unet_plan *plan, int batch) {
    if (!plan || plan->net != 0 || batch <= 0) return IMK_EINVAL;
    return (int64_t)consist_layout(plan, batch).total;
}

extern "C" int imk_unet_consistency_fwd_bwd(const imk_unet_plan *plan, float *params, void *packed, void *state,
                                            const uint8_t *x1, const uint8_t *x2, int batch, float *grads, float *stats,
                                            void *workspace, int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && plan->net == 0 && params && packed && state && x1 && x2 && grads && stats && workspace && batch > 0);
    const ConsistLayout lay = consist_layout(plan, batch);
    if ((int64_t)lay.total > workspace_bytes) return IMK_EWORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t *base = (uint8_t *)workspace;
    Ctx c1{plan, lay.ws, base + lay.view[0], params, (const uint8_t *)packed, batch, true, stream};
    Ctx c2{plan, lay.ws, base + lay.view[1], params, (const uint8_t *)packed, batch, true, stream};
    c1.x_in[0] = x1;
    c2.x_in[0] = x2;
    const StateView sv = state_view(plan, state);
    const imk_unet_cfg &cf = plan->cfg;
    const Topo t = make_topo(plan);
    const long long n_pix = (long long)batch * cf.h * cf.w;
    const ImkLayer &ol = plan->layers[t.out];
    const int obn = t.d_bnb[3], cs = imk_pad8(ol.cin);
    float *grads2 = reinterpret_cast<float *>(base + lay.grads2);
    float *loss_partial = reinterpret_cast<float *>(base + lay.loss_partial);
    int rc;
#define OK(e) do { rc = (e); if (rc) return rc; } while (0)
    // both forwards with batch statistics; each BatchNorm's finalize moves the moving statistics, view 1 first
    OK(run_forward(c1, t, nullptr, params));
    OK(run_forward(c2, t, nullptr, params));

    // the fused head's weight-gradient rows carry both views and are reduced into `grads` alone: the output layer is the last entry
    // of the trainable section, and the final sum then stops in front of it
    const bool fused = !plan->dbg_materialize && imk_switches().consistency_fused &&
                       ol.off_b + ol.cout == plan->n_trainable &&
                       imk_consistency_fused_ok(cs, ol.cout, cf.act_out, n_pix, lay.ws.L[obn].n_bwd_rows);
    const int head_rows = imk_loss_blocks(n_pix);
    HeadWgJob fused_job{reinterpret_cast<float *>(c1.base + lay.ws.L[t.out].wg_partial), head_rows};
    f16 *dlogit1 = reinterpret_cast<f16 *>(c1.base + lay.ws.dlogit), *dlogit2 = reinterpret_cast<f16 *>(c2.base + lay.ws.dlogit);
    if (fused) {
        OK(imk_launch_consistency_head(c1.act(t.d_c1[3]), c2.act(t.d_c1[3]), c1.bn_scale(obn), c1.bn_shift(obn), c2.bn_scale(obn),
                                       c2.bn_shift(obn), params + ol.off_w, params + ol.off_b, ol.cin, cs, ol.cout, n_pix, sv.ctl,
                                       stats, c1.dy(obn), c2.dy(obn), loss_partial,
                                       reinterpret_cast<float *>(c1.base + lay.ws.L[obn].bwd_partial),
                                       reinterpret_cast<float *>(c2.base + lay.ws.L[obn].bwd_partial), fused_job.partial, stream));
    } else {
        float *p1 = reinterpret_cast<float *>(c1.base + lay.ws.probs), *p2 = reinterpret_cast<float *>(c2.base + lay.ws.probs);
        OK(imk_launch_head(c1.act(t.d_c1[3]), c1.bn_scale(obn), c1.bn_shift(obn), params + ol.off_w, params + ol.off_b, ol.cin, cs,
                           ol.cout, cf.act_out, n_pix, p1, stream));
        OK(imk_launch_head(c2.act(t.d_c1[3]), c2.bn_scale(obn), c2.bn_shift(obn), params + ol.off_w, params + ol.off_b, ol.cin, cs,
                           ol.cout, cf.act_out, n_pix, p2, stream));
        OK(imk_launch_consistency_dlogit(p1, p2, ol.cout, cf.act_out, n_pix, sv.ctl, stats, dlogit1, dlogit2, loss_partial, stream));
    }

    const int n_side = imk_switches().side_streams;
    const bool side_on = !plan->dbg_single_stream && n_side > 0 && ensure_side_streams(plan, n_side);
    {   // backward of view 1 into `grads`; the loss value rides on its first fork, as in the labelled step
        Bwd b{c1, grads, sv.ctl, stats + 1, side_on ? n_side : 0};
        ImkStopRingScope stop_ring(plan, stream, b.n_side);
        bool loss_done = false;
        auto loss_on_side = [&]() -> int {
            if (loss_done || b.n_side <= 0 || b.n_fork <= 0) return IMK_OK;
            loss_done = true;
            return imk_launch_loss_finalize(loss_partial, n_pix, cf.n_out, 0, stats, plan->side[(b.n_fork - 1) % b.n_side]);
        };
        int rows = head_rows;
        HeadWgJob job = fused ? fused_job : HeadWgJob{};
        if (!fused) OK(head_dgrad(b, t, dlogit1, loss_on_side, &rows, &job));
        OK(run_backward(b, t, rows, job.partial ? &job : nullptr, loss_on_side));
        if (!loss_done) OK(imk_launch_loss_finalize(loss_partial, n_pix, cf.n_out, 0, stats, stream));
    }
    {   // backward of view 2 into the second vector
        Bwd b{c2, grads2, sv.ctl, stats + 1, side_on ? n_side : 0};
        ImkStopRingScope stop_ring(plan, stream, b.n_side);
        auto no_loss = []() -> int { return IMK_OK; };
        int rows = head_rows;
        HeadWgJob job{};
        if (!fused) OK(head_dgrad(b, t, dlogit2, no_loss, &rows, &job));
        OK(run_backward(b, t, rows, job.partial ? &job : nullptr, no_loss));
    }
    OK(imk_launch_grad_add(grads, grads2, fused ? ol.off_w : plan->n_trainable, stats + 1, stream));
#undef OK
    return IMK_OK;
}

extern "C" int imk_unet_adamw_step(const imk_unet_plan *plan, float *params, void *packed, void *state,
                                   const float *grads, const float *stats, float grad_scale, float lr, float wd,
                                   float beta1, float beta2, float eps, void *stream_) {
    IMK_CHECK_ARG(plan && params && packed && state && grads && stats);
    const StateView sv = state_view(plan, state);
    int rc = imk_launch_adamw(params, sv.m, sv.v, grads, plan->n_trainable, sv.ctl, stats, grad_scale, lr, wd, beta1, beta2,
                              eps, (hipStream_t)stream_);
    if (rc) return rc;
    // conv weights only: training does not read the folded inference statistics (imk_unet_pack_weights refreshes them)
    return pack_weights(plan, params, packed, (hipStream_t)stream_, sv.ctl, stats, false);
}
