// Host orchestration of EvalNet (evalnet.py:24-73: get_evalnet, get_evalnet_miou) on top of the same conv / BatchNorm
// kernels as the U-Net: two towers (input block + one conv block each), concatenate, five conv blocks, GlobalAvgPool2D,
// Dense sigmoid head(s).  get_evalnet_miou_v2 (evalnet.py:76-106, plan->ev2) is the late-fusion form of the same blocks: input
// block + FOUR conv blocks per tower, add() of the towers' pooled outputs at 1/16 resolution, three trunk blocks, the two heads.  A conv block is Conv3x3+ReLU -> Conv1x1+ReLU -> BatchNorm -> MaxPooling2D (evalnet.py:14-21),
// i.e. the U-Net's encoder block: its BatchNorm and pooling are applied by the consumer on load.
// Plans are imk_unet_plan objects: parameter layout, packing, optimizer state and AdamW step are the imk_unet_* calls.
#include "imk_net.h"
#include "imk_switches.h"

namespace {

struct ETopo {
    int in_c[2], in_bn[2], t_c3[2], t_c1[2], t_bn[2];   // towers A, B
    int m_c3[5], m_c1[5], m_bn[5];                      // trunk blocks
    int dense[2];
    // v2: tower blocks 1..4 ("a1.c3" ...), trunk blocks m1..m3 in m_*[0..2]
    int v_c3[2][4], v_c1[2][4], v_bn[2][4];
    int n_trunk;                                        // 5, v2: 3
};

ETopo make_etopo(const imk_unet_plan *p) {
    ETopo t{};
    const char tw[2] = {'a', 'b'};
    char nm[16];
    t.n_trunk = p->ev2 ? 3 : 5;
    for (int s = 0; s < 2; ++s) {
        snprintf(nm, sizeof nm, "%c.in.c", tw[s]); t.in_c[s] = p->find(nm);
        snprintf(nm, sizeof nm, "%c.in.bn", tw[s]); t.in_bn[s] = p->find(nm);
        snprintf(nm, sizeof nm, "%c.c3", tw[s]); t.t_c3[s] = p->find(nm);
        snprintf(nm, sizeof nm, "%c.c1", tw[s]); t.t_c1[s] = p->find(nm);
        snprintf(nm, sizeof nm, "%c.bn", tw[s]); t.t_bn[s] = p->find(nm);
        for (int j = 0; j < 4; ++j) {
            snprintf(nm, sizeof nm, "%c%d.c3", tw[s], j + 1); t.v_c3[s][j] = p->find(nm);
            snprintf(nm, sizeof nm, "%c%d.c1", tw[s], j + 1); t.v_c1[s][j] = p->find(nm);
            snprintf(nm, sizeof nm, "%c%d.bn", tw[s], j + 1); t.v_bn[s][j] = p->find(nm);
        }
    }
    for (int i = 0; i < t.n_trunk; ++i) {
        snprintf(nm, sizeof nm, "m%d.c3", i + 1); t.m_c3[i] = p->find(nm);
        snprintf(nm, sizeof nm, "m%d.c1", i + 1); t.m_c1[i] = p->find(nm);
        snprintf(nm, sizeof nm, "m%d.bn", i + 1); t.m_bn[i] = p->find(nm);
    }
    t.dense[0] = p->find(p->ecfg.two_heads ? "iou" : "dense");
    t.dense[1] = p->ecfg.two_heads ? p->find("detection") : -1;
    return t;
}

// Layer (= parameter) order is Keras' creation order of evalnet.py:24-45: tower A (input block, conv block), tower B,
// the five trunk blocks, the Dense head(s).
void build_layers(imk_unet_plan *p) {
    const imk_evalnet_cfg &e = p->ecfg;
    const int F = e.ch[0];
    const char tw[2] = {'a', 'b'};
    const int cin[2] = {e.ca, e.cb};
    const int norm[2] = {e.normalize_a, e.normalize_b};
    char nm[16];
    for (int s = 0; s < 2; ++s) {
        snprintf(nm, sizeof nm, "%c.in.c", tw[s]);
        const int ic = add_conv(p, nm, 1, cin[s], F, 0);
        if (!norm[s] && !(s == 1 && e.b_onehot)) p->layers[ic].flags |= IMK_LF_U8_RAW;
        snprintf(nm, sizeof nm, "%c.in.bn", tw[s]);
        const int ib = add_bn(p, nm, F, 0, ic);
        snprintf(nm, sizeof nm, "%c.c3", tw[s]);
        const int c3 = add_conv(p, nm, 3, F, F, 0);
        snprintf(nm, sizeof nm, "%c.c1", tw[s]);
        const int c1 = add_conv(p, nm, 1, F, F, 0);
        snprintf(nm, sizeof nm, "%c.bn", tw[s]);
        add_bn(p, nm, F, 0, c1);
        if (s == 1 && e.b_onehot) set_src(p, ic, LM_RAW, IMK_SRC_ONEHOT);   // 1x1 conv over the one-hot stack
        else set_src(p, ic, LM_U8, s ? IMK_SRC_XB : IMK_SRC_XA);
        set_src(p, c3, LM_AFFINE, ic, ib);
        set_src(p, c1, LM_RAW, c3);
    }
    int prev_c1 = -1, prev_bn = -1, prev_f = 2 * F;
    for (int i = 0; i < 5; ++i) {
        const int f = e.ch[i], res = i + 1;
        snprintf(nm, sizeof nm, "m%d.c3", i + 1);
        const int c3 = add_conv(p, nm, 3, prev_f, f, res);
        snprintf(nm, sizeof nm, "m%d.c1", i + 1);
        const int c1 = add_conv(p, nm, 1, f, f, res);
        snprintf(nm, sizeof nm, "m%d.bn", i + 1);
        const int bn = add_bn(p, nm, f, res, c1);
        if (i == 0) set_src(p, c3, LM_RAW, IMK_SRC_CAT);
        else set_src(p, c3, LM_POOL, prev_c1, prev_bn);
        set_src(p, c1, LM_RAW, c3);
        prev_c1 = c1; prev_bn = bn; prev_f = f;
    }
    for (int h = 0; h < (e.two_heads ? 2 : 1); ++h) {
        const int d = add_conv(p, e.two_heads ? (h ? "detection" : "iou") : "dense", 1, e.ch[4], e.n_out, 6);
        p->layers[d].flags = IMK_LF_DENSE;
    }
    finish_layout(p);
}

// v2 (evalnet.py:76-106): Keras' creation order is tower A completely (input block, blocks 1..4 at int(16a) .. int(128a)), tower B,
// the trunk (int(64a), int(128a), int(256a)), the heads.  Tower block j+1 runs at resolution level j and reads the pooled output of
// the block before it on load; the trunk's first conv reads the materialised sum of the towers' pooled outputs (level 4).
void build_layers_v2(imk_unet_plan *p) {
    const imk_evalnet_cfg &e = p->ecfg;
    const char tw[2] = {'a', 'b'};
    const int cin[2] = {e.ca, e.cb};
    const int norm[2] = {e.normalize_a, e.normalize_b};
    char nm[16];
    int prev_c1 = -1, prev_bn = -1, prev_f = 0;
    auto block = [&](const char *prefix, int f, int res, int lmode, int src, int src_bn) {
        snprintf(nm, sizeof nm, "%s.c3", prefix);
        const int c3 = add_conv(p, nm, 3, prev_f, f, res);
        snprintf(nm, sizeof nm, "%s.c1", prefix);
        const int c1 = add_conv(p, nm, 1, f, f, res);
        snprintf(nm, sizeof nm, "%s.bn", prefix);
        const int bn = add_bn(p, nm, f, res, c1);
        set_src(p, c3, lmode, src, src_bn);
        set_src(p, c1, LM_RAW, c3);
        prev_c1 = c1; prev_bn = bn; prev_f = f;
    };
    char pre[8];
    for (int s = 0; s < 2; ++s) {
        snprintf(nm, sizeof nm, "%c.in.c", tw[s]);
        const int ic = add_conv(p, nm, 1, cin[s], e.ch[0], 0);
        if (!norm[s] && !(s == 1 && e.b_onehot)) p->layers[ic].flags |= IMK_LF_U8_RAW;
        snprintf(nm, sizeof nm, "%c.in.bn", tw[s]);
        const int ib = add_bn(p, nm, e.ch[0], 0, ic);
        if (s == 1 && e.b_onehot) set_src(p, ic, LM_RAW, IMK_SRC_ONEHOT);   // 1x1 conv over the one-hot stack
        else set_src(p, ic, LM_U8, s ? IMK_SRC_XB : IMK_SRC_XA);
        prev_f = e.ch[0];
        for (int j = 0; j < 4; ++j) {
            snprintf(pre, sizeof pre, "%c%d", tw[s], j + 1);
            if (j == 0) block(pre, e.ch[0], 0, LM_AFFINE, ic, ib);
            else block(pre, e.ch[j], j, LM_POOL, prev_c1, prev_bn);
        }
    }
    for (int i = 0; i < 3; ++i) {
        snprintf(pre, sizeof pre, "m%d", i + 1);
        if (i == 0) block(pre, e.ch[2], 4, LM_RAW, IMK_SRC_CAT, -1);
        else block(pre, e.ch[2 + i], 4 + i, LM_POOL, prev_c1, prev_bn);
    }
    for (int h = 0; h < 2; ++h) {
        const int d = add_conv(p, h ? "detection" : "iou", 1, e.ch[4], e.n_out, 7);
        p->layers[d].flags = IMK_LF_DENSE;
    }
    finish_layout(p);
}

Ws make_ews_v2(const imk_unet_plan *p, int B, int mode) {
    Ws w;
    const imk_evalnet_cfg &e = p->ecfg;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = up(off + bytes); return o; };
    make_ws_layers(p, B, mode, w, take);
    auto pooled = [&](int res, int c) { const Dim d = res_dim(p->cfg, res); return (size_t)B * d.h * d.w * imk_pad8(c) * 2; };
    w.cat = take(pooled(4, e.ch[3]));
    if (e.b_onehot) w.onehot = take((size_t)B * e.h * e.w * imk_pad8(e.cb) * 2);
    w.probs = take((size_t)B * 2 * e.n_out * sizeof(float));
    if (mode == 1) {
        w.dcat = take(pooled(4, e.ch[3]));
        for (int i = 0; i < 3; ++i) w.dP[i] = take(pooled(5 + i, e.ch[2 + i]));   // pooled output of trunk block i+1 ([2]: the head writes it)
        for (int s = 0; s < 2; ++s)
            for (int j = 0; j < 3; ++j) w.dT[s][j] = take(pooled(j + 1, e.ch[j]));   // pooled output of tower block j+1
        w.head_partial = take(imk_evalnet_head_partial_floats(B, 2, e.n_out, e.ch[4]) * sizeof(float));
    }
    w.total = off;
    return w;
}

Ws make_ews(const imk_unet_plan *p, int B, int mode) {
    if (p->ev2) return make_ews_v2(p, B, mode);
    Ws w;
    const imk_evalnet_cfg &e = p->ecfg;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = up(off + bytes); return o; };
    make_ws_layers(p, B, mode, w, take);
    const size_t px1 = (size_t)B * (e.h / 2) * (e.w / 2);
    const int cat_cs = 2 * imk_pad8(e.ch[0]);
    w.cat = take(px1 * cat_cs * 2);
    if (e.b_onehot) w.onehot = take((size_t)B * e.h * e.w * imk_pad8(e.cb) * 2);
    w.probs = take((size_t)B * 2 * e.n_out * sizeof(float));   // training: the head's outputs of the batch
    if (mode == 1) {
        w.dcat = take(px1 * cat_cs * 2);
        for (int i = 0; i < 5; ++i) {   // gradient w.r.t. the pooled output of trunk block i+1, at res i+2
            const Dim d = res_dim(p->cfg, i + 2);
            w.dP[i] = take((size_t)B * d.h * d.w * imk_pad8(e.ch[i]) * 2);
        }
        w.head_partial = take(imk_evalnet_head_partial_floats(B, e.two_heads ? 2 : 1, e.n_out, e.ch[4]) * sizeof(float));
    }
    w.total = off;
    return w;
}

// a_div > 1 (inference, imk_evalnet_forward_candidates): c.B = B * a_div rows, x_in[0] holds B images -- tower A runs at batch B in
// the front of its B * a_div sized buffers, and row r of the concatenation reads its image r / a_div
int run_forward(Ctx &c, const ETopo &t, float *params_rw, int a_div = 1) {
    int rc;
#define OK(e) do { rc = (e); if (rc) return rc; } while (0)
    const imk_evalnet_cfg &e = c.p->ecfg;
    if (e.b_onehot)
        OK(imk_launch_onehot(c.x_in[1], (long long)c.B * e.h * e.w, imk_pad8(e.cb), e.normalize_b != 0, reinterpret_cast<f16 *>(c.base + c.ws.onehot),
                             c.stream));
    const int B_rows = c.B;
    if (c.p->ev2) {   // all of tower A (input block + four blocks) at batch B_rows / a_div; tower B and the trunk at B_rows
        for (int s = 0; s < 2; ++s) {
            c.B = s == 0 ? B_rows / a_div : B_rows;
            OK(run_conv_fwd(c, t.in_c[s], params_rw));
            for (int j = 0; j < 4; ++j) OK(run_conv_pair(c, t.v_c3[s][j], t.v_c1[s][j], params_rw));
        }
        const Dim d3 = res_dim(c.p->cfg, 3);
        OK(imk_launch_add_pool(c.act(t.v_c1[0][3]), c.bn_scale(t.v_bn[0][3]), c.bn_shift(t.v_bn[0][3]), c.act(t.v_c1[1][3]),
                               c.bn_scale(t.v_bn[1][3]), c.bn_shift(t.v_bn[1][3]), imk_pad8(e.ch[3]), c.B, d3.h, d3.w,
                               reinterpret_cast<f16 *>(c.base + c.ws.cat), c.stream, a_div));
        for (int i = 0; i < 3; ++i) OK(run_conv_pair(c, t.m_c3[i], t.m_c1[i], params_rw));
        return IMK_OK;
    }
    for (int s = 0; s < 2; ++s) {
        c.B = s == 0 ? B_rows / a_div : B_rows;
        OK(run_conv_fwd(c, t.in_c[s], params_rw));
        OK(run_conv_pair(c, t.t_c3[s], t.t_c1[s], params_rw));
    }
    const int csF = imk_pad8(e.ch[0]);
    OK(imk_launch_concat_pool(c.act(t.t_c1[0]), c.bn_scale(t.t_bn[0]), c.bn_shift(t.t_bn[0]), csF, c.act(t.t_c1[1]),
                              c.bn_scale(t.t_bn[1]), c.bn_shift(t.t_bn[1]), csF, c.B, e.h / 2, e.w / 2,
                              reinterpret_cast<f16 *>(c.base + c.ws.cat), c.stream, a_div));
    for (int i = 0; i < 5; ++i) OK(run_conv_pair(c, t.m_c3[i], t.m_c1[i], params_rw));
#undef OK
    return IMK_OK;
}

// the tail: BN + pool of the last block, global average pool, Dense head(s); with targets also loss and gradients
int run_head(Ctx &c, const ETopo &t, float *out, const float *y, const ImkCtl *ctl, float *stats) {
    const imk_evalnet_cfg &e = c.p->ecfg;
    const int nh = e.two_heads ? 2 : 1;
    const float *w[2] = {nullptr, nullptr}, *b[2] = {nullptr, nullptr};
    for (int h = 0; h < nh; ++h) { const ImkLayer &d = c.p->layers[t.dense[h]]; w[h] = c.params + d.off_w; b[h] = c.params + d.off_b; }
    const int last = t.n_trunk - 1;                                 // the last trunk block, at level 5 (v2: 6)
    const Dim d5 = res_dim(c.p->cfg, c.p->layers[t.m_c1[last]].res);
    return imk_launch_evalnet_head(c.act(t.m_c1[last]), c.bn_scale(t.m_bn[last]), c.bn_shift(t.m_bn[last]), w, b, nh, e.n_out, e.ch[4],
                                   imk_pad8(e.ch[4]), c.B, d5.h, d5.w, out, y, ctl, stats,
                                   y ? reinterpret_cast<f16 *>(c.base + c.ws.dP[last]) : nullptr,
                                   y ? reinterpret_cast<float *>(c.base + c.ws.head_partial) : nullptr, c.stream);
}

bool ecfg_ok(const imk_evalnet_cfg *c) {
    if (!c) return false;
    // six 2x2 poolings; sizes that are not multiples of 64 lose odd last rows / columns like Keras' 'valid' pooling
    // (208 x 416: 13 -> 6 -> 3).  Full resolution itself must be even (the towers' pooled outputs are concatenated).
    if (c->h < 64 || c->w < 64 || (c->h % 2) || (c->w % 2)) return false;
    if (c->ca < 1 || c->ca > 4 || c->cb < 1 || c->cb > (c->b_onehot ? 64 : 4)) return false;   // uint8 stems of the pipelined conv kernel
    if (c->n_out < 1 || c->n_out > 64) return false;
    for (int i = 0; i < 5; ++i) if (c->ch[i] < 1 || c->ch[i] > 512) return false;
    if (c->ch[0] % 8) return false;   // the towers' channels sit side by side in the concatenated tensor
    return true;
}

int plan_create(const imk_evalnet_cfg *cfg, imk_unet_plan **out, bool v2) {
    IMK_CHECK_ARG(out);
    if (!ecfg_ok(cfg)) return IMK_EINVAL;
    // v2: seven 2x2 poolings; the two heads only; the towers' last level is summed in 8-channel chunks
    if (v2 && (cfg->h < 128 || cfg->w < 128 || cfg->two_heads != 1 || cfg->ch[3] % 8)) return IMK_EINVAL;
    if ((long long)cfg->h * cfg->w >= imk_conv_max_pixels() || cfg->w >= (1 << 16)) return IMK_EUNSUPPORTED;   // include/imk.h: image size limit
    imk_unet_plan *p = new (std::nothrow) imk_unet_plan();
    if (!p) return IMK_EINVAL;
    p->net = 1;
    p->ev2 = v2 ? 1 : 0;
    p->ecfg = *cfg;
    p->cfg = imk_unet_cfg{cfg->h, cfg->w, cfg->ca, cfg->n_out, {cfg->ch[0], cfg->ch[1], cfg->ch[2], cfg->ch[3], cfg->ch[4]}, 0};
    if (v2) build_layers_v2(p);
    else build_layers(p);
    *out = p;
    return IMK_OK;
}

}  // namespace

// =====================================================================================================
extern "C" int imk_evalnet_plan_create(const imk_evalnet_cfg *cfg, imk_unet_plan **out) { return plan_create(cfg, out, false); }
extern "C" int imk_evalnet_v2_plan_create(const imk_evalnet_cfg *cfg, imk_unet_plan **out) { return plan_create(cfg, out, true); }

extern "C" int64_t imk_evalnet_workspace_bytes(const imk_unet_plan *plan, int batch, int mode) {
    if (!plan || plan->net != 1 || batch <= 0 || (mode != 0 && mode != 1)) return IMK_EINVAL;
    return (int64_t)make_ews(plan, batch, mode).total;
}

extern "C" int imk_evalnet_forward(const imk_unet_plan *plan, const float *params, const void *packed, const uint8_t *xa,
                                   const uint8_t *xb, int batch, float *out, void *workspace, int64_t workspace_bytes,
                                   void *stream_) {
    IMK_CHECK_ARG(plan && plan->net == 1 && params && packed && xa && xb && out && workspace && batch > 0);
    Ctx c{plan, make_ews(plan, batch, 0), (uint8_t *)workspace, params, (const uint8_t *)packed, batch, false,
          (hipStream_t)stream_};
    if ((int64_t)c.ws.total > workspace_bytes) return IMK_EWORKSPACE;
    c.x_in[0] = xa; c.x_in[1] = xb;
    const ETopo t = make_etopo(plan);
    int rc = run_forward(c, t, nullptr);
    if (rc) return rc;
    return run_head(c, t, out, nullptr, nullptr, nullptr);
}

// ---- EvalNet-ensemble scoring: N models of one plan, B images with M candidate masks each (include/imk.h) -------------------
namespace {

// Workspace: one model's inference activations at batch B * M (tower A uses the first B images' worth of its buffers).  Only under
// IMK_SELECT_SHARED=0 (read once per process) the images repeated M times follow: the comparison route alone pays for them.
struct CandWs { Ws ws; size_t rep = 0, total = 0; };
CandWs make_cand_ws(const imk_unet_plan *p, int B, int M) {
    CandWs w;
    w.ws = make_ews(p, B * M, 0);
    w.rep = w.ws.total;
    w.total = w.rep + (imk_switches().select_shared ? 0 : up((size_t)B * M * p->ecfg.h * p->ecfg.w * p->ecfg.ca));
    return w;
}

int cand_limits(const imk_unet_plan *plan, int n_models, int batch, int n_cand) {
    IMK_CHECK_ARG(plan && plan->net == 1 && n_models > 0 && batch > 0 && n_cand > 0);
    if (n_models > IMK_SELECT_MAX_MODELS || n_cand > IMK_SELECT_MAX_CAND || batch > 65535) return IMK_EUNSUPPORTED;
    return IMK_OK;
}

// shared: tower A once per image (run_forward's a_div); else imk_evalnet_forward's launches on the repeated images
int forward_candidates(const imk_unet_plan *plan, int n_models, const float *const *params, const void *const *packed,
                       const uint8_t *xa, const uint8_t *xb, int batch, int n_cand, float *scores, void *workspace,
                       int64_t workspace_bytes, hipStream_t stream, bool shared) {
    int rc = cand_limits(plan, n_models, batch, n_cand);
    if (rc) return rc;
    IMK_CHECK_ARG(params && packed && xa && xb && scores && workspace);
    for (int n = 0; n < n_models; ++n) IMK_CHECK_ARG(params[n] && packed[n]);
    const CandWs cw = make_cand_ws(plan, batch, n_cand);
    if ((int64_t)cw.total > workspace_bytes) return IMK_EWORKSPACE;
    const imk_evalnet_cfg &e = plan->ecfg;
    uint8_t *base = (uint8_t *)workspace;
    if (!shared) {
        rc = imk_launch_repeat_rows(xa, batch, n_cand, (long long)e.h * e.w * e.ca, base + cw.rep, stream);
        if (rc) return rc;
    }
    const ETopo t = make_etopo(plan);
    const int rows = batch * n_cand, units = (e.two_heads ? 2 : 1) * e.n_out;
    for (int n = 0; n < n_models; ++n) {
        Ctx c{plan, cw.ws, base, params[n], (const uint8_t *)packed[n], rows, false, stream};
        c.x_in[0] = shared ? xa : base + cw.rep;
        c.x_in[1] = xb;
        rc = run_forward(c, t, nullptr, shared ? n_cand : 1);
        if (rc) return rc;
        rc = run_head(c, t, scores + (size_t)n * rows * units, nullptr, nullptr, nullptr);
        if (rc) return rc;
    }
    return IMK_OK;
}

}  // namespace

extern "C" int64_t imk_evalnet_forward_candidates_workspace_bytes(const imk_unet_plan *plan, int batch, int n_cand) {
    int rc = cand_limits(plan, 1, batch, n_cand);
    if (rc) return rc;
    return (int64_t)make_cand_ws(plan, batch, n_cand).total;
}

extern "C" int imk_evalnet_forward_candidates(const imk_unet_plan *plan, int n_models, const float *const *params,
                                              const void *const *packed, const uint8_t *xa, const uint8_t *xb, int batch,
                                              int n_cand, float *scores, void *workspace, int64_t workspace_bytes, void *stream_) {
    return forward_candidates(plan, n_models, params, packed, xa, xb, batch, n_cand, scores, workspace, workspace_bytes,
                              (hipStream_t)stream_, true);
}

extern "C" int imk_evalnet_forward_select(const imk_unet_plan *plan, int n_models, const float *const *params,
                                          const void *const *packed, const uint8_t *xa, const uint8_t *xb, int batch, int n_cand,
                                          const int32_t *counts, const uint8_t *cand, int64_t cand_bytes, double thr, int mode,
                                          float *scores, int32_t *best_idx, float *best_score, uint8_t *keep, uint8_t *out,
                                          void *workspace, int64_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int rc = cand_limits(plan, n_models, batch, n_cand);
    if (rc) return rc;
    IMK_CHECK_ARG(scores && best_idx && best_score && keep);
    const imk_evalnet_cfg &e = plan->ecfg;
    const int n_heads = e.two_heads ? 2 : 1;
    rc = imk_select_check(n_models, batch, n_cand, n_heads, e.n_out, counts, cand, cand_bytes, mode, out, stream);
    if (rc) return rc;
    rc = forward_candidates(plan, n_models, params, packed, xa, xb, batch, n_cand, scores, workspace, workspace_bytes, stream,
                            imk_switches().select_shared);
    if (rc) return rc;
    const ImkSelectArgs a{scores, counts, cand, n_models, batch, n_cand, n_heads, e.n_out, mode == IMK_SELECT_MIOU, cand_bytes,
                          (float)thr, best_idx, best_score, keep, out, mode == IMK_SELECT_CONF_GATED};
    return imk_launch_evalnet_select(a, stream);
}

extern "C" int imk_evalnet_tensor_info(const imk_unet_plan *plan, int batch, int mode, int layer_idx, int which,
                                       int64_t *byte_offset, int *h, int *w, int *c, int *c_stride) {
    IMK_CHECK_ARG(plan && plan->net == 1 && batch > 0 && layer_idx >= 0 && layer_idx < (int)plan->layers.size());
    IMK_CHECK_ARG(mode == 0 || mode == 1);
    const Ws ws = make_ews(plan, batch, mode);
    const ImkLayer &l = plan->layers[layer_idx];
    IMK_CHECK_ARG(!(l.flags & IMK_LF_DENSE));
    const Dim d = res_dim(plan->cfg, l.res);
    size_t off = 0;
    if (which == 0 && l.kind == 0) off = ws.L[layer_idx].out;
    else if (which == 1 && l.kind == 0 && mode == 1) off = ws.L[layer_idx].dA;
    else if (which == 2 && l.kind == 1 && mode == 1) off = ws.L[layer_idx].dy;
    else if (which == 3 && l.kind == 0 && l.src == IMK_SRC_CAT) {   // the conv's INPUT: the towers' concatenation (v2: their sum)
        if (byte_offset) *byte_offset = (int64_t)ws.cat;
        if (h) *h = d.h;
        if (w) *w = d.w;
        if (c) *c = l.cin;
        if (c_stride) *c_stride = plan->ev2 ? imk_pad8(l.cin) : 2 * imk_pad8(plan->ecfg.ch[0]);
        return IMK_OK;
    } else if (which == 4 && l.kind == 1) {   // fp32 scale[c_stride] | shift[c_stride]: mode 0 in the PACKED buffer, mode 1 in the workspace
        if (byte_offset) *byte_offset = mode == 1 ? (int64_t)ws.L[layer_idx].scale : l.pk_scale;
        if (h) *h = 1;
        if (w) *w = 2;
        if (c) *c = l.cout;
        if (c_stride) *c_stride = imk_pad8(l.cout);
        return IMK_OK;
    } else return IMK_EINVAL;
    if (byte_offset) *byte_offset = (int64_t)off;
    if (h) *h = d.h;
    if (w) *w = d.w;
    if (c) *c = l.cout;
    if (c_stride) *c_stride = imk_pad8(l.cout);
    return IMK_OK;
}

// One training pass: forward with batch statistics, losses (head 0 mean squared error; head 1 binary cross-entropy,
// functions.py:4708 `loss=['mse', 'binary_crossentropy']`; the single head of get_evalnet: mse, functions.py:4492),
// backward.  grads [n_trainable]; stats [8]: loss, overflow flag, loss scale, step, loss of head 0, loss of head 1.
// out [B, n_heads*n_out]: the sigmoid outputs of this (training-mode) pass.
extern "C" int imk_evalnet_fwd_bwd(const imk_unet_plan *plan, float *params, void *packed, void *state, const uint8_t *xa,
                                   const uint8_t *xb, const float *y, int batch, float *out, float *grads, float *stats,
                                   void *workspace, int64_t workspace_bytes, void *stream_) {
    IMK_CHECK_ARG(plan && plan->net == 1 && params && packed && state && xa && xb && y && grads && stats && workspace);
    IMK_CHECK_ARG(batch > 0);
    hipStream_t stream = (hipStream_t)stream_;
    Ctx c{plan, make_ews(plan, batch, 1), (uint8_t *)workspace, params, (const uint8_t *)packed, batch, true, stream};
    if ((int64_t)c.ws.total > workspace_bytes) return IMK_EWORKSPACE;
    c.x_in[0] = xa; c.x_in[1] = xb;
    const StateView sv = state_view(plan, state);
    const ETopo t = make_etopo(plan);
    const imk_evalnet_cfg &e = plan->ecfg;
    const int nh = e.two_heads ? 2 : 1;
    int rc;
#define OK(e_) do { rc = (e_); if (rc) return rc; } while (0)
    OK(run_forward(c, t, params));
    float *head_out = out ? out : reinterpret_cast<float *>(c.base + c.ws.probs);
    OK(run_head(c, t, head_out, y, sv.ctl, stats));

    const int n_side = imk_switches().side_streams;
    const bool side_on = !plan->dbg_single_stream && n_side > 0 && ensure_side_streams(plan, n_side);
    Bwd b{c, grads, sv.ctl, stats + 1, side_on ? n_side : 0};
    ImkStopRingScope stop_ring(plan, stream, b.n_side);      // the backward pass's launches carry their own events (imk_common.h)
    {   // Dense gradients and the loss values: batch reduction of the head kernel's per-sample terms
        const ImkLayer &d0 = plan->layers[t.dense[0]];
        const ImkLayer *d1 = nh > 1 ? &plan->layers[t.dense[1]] : nullptr;
        OK(imk_launch_evalnet_head_reduce(reinterpret_cast<const float *>(c.base + c.ws.head_partial), batch, nh, e.n_out,
                                          e.ch[4], &sv.ctl->inv_loss_scale, grads + d0.off_w, grads + d0.off_b,
                                          d1 ? grads + d1->off_w : nullptr, d1 ? grads + d1->off_b : nullptr, stats + 1, stats,
                                          stream));
    }
    // trunk blocks 5..1 (v2: 3..1): dy of the block's BatchNorm = max-pool scatter of the gradient of its pooled output
    for (int i = t.n_trunk - 1; i >= 0; --i) {
        OK(b.bn_bwd(t.m_bn[i], 1, nullptr, reinterpret_cast<f16 *>(c.base + c.ws.dP[i])));
        OK(b.wgrad_dgrad(t.m_c1[i], c.dA(t.m_c3[i]), c.act(t.m_c3[i])));
        f16 *dst = i > 0 ? reinterpret_cast<f16 *>(c.base + c.ws.dP[i - 1]) : reinterpret_cast<f16 *>(c.base + c.ws.dcat);
        OK(b.wgrad_dgrad(t.m_c3[i], dst, nullptr));
        OK(b.flush_wgrads());
    }
    if (plan->ev2) {
        // The gradient of the sum is the gradient of both addends: both towers' last BatchNorm scatter the SAME tensor.  Blocks 4..2 of
        // a tower follow the trunk's pattern, block 1 and the input block v1's tower; tower A comes last, as in v1.
        const f16 *dsum = reinterpret_cast<const f16 *>(c.base + c.ws.dcat);
        for (int s = 1; s >= 0; --s) {
            for (int j = 3; j >= 1; --j) {
                const f16 *g = j == 3 ? dsum : reinterpret_cast<const f16 *>(c.base + c.ws.dT[s][j]);
                OK(b.bn_bwd(t.v_bn[s][j], 1, nullptr, g));
                OK(b.wgrad_dgrad(t.v_c1[s][j], c.dA(t.v_c3[s][j]), c.act(t.v_c3[s][j])));
                OK(b.wgrad_dgrad(t.v_c3[s][j], reinterpret_cast<f16 *>(c.base + c.ws.dT[s][j - 1]), nullptr));
                OK(b.flush_wgrads());
            }
            b.tail_early = true;
            if (s == 0) b.defer_finalize = true;
            OK(b.bn_bwd(t.v_bn[s][0], 1, nullptr, reinterpret_cast<const f16 *>(c.base + c.ws.dT[s][0])));
            OK(b.wgrad_dgrad(t.v_c1[s][0], c.dA(t.v_c3[s][0]), c.act(t.v_c3[s][0])));
            OK(b.wgrad_dgrad(t.v_c3[s][0], c.dy(t.in_bn[s]), nullptr, t.in_bn[s]));
            OK(b.bn_bwd(t.in_bn[s], 0, nullptr, nullptr));
            OK(b.wgrad(t.in_c[s], nullptr, s == 0));
        }
        OK(b.finish_wgrads());
        return IMK_OK;
    }
    // towers: each takes its channel slice of the concatenated gradient
    const int csF = imk_pad8(e.ch[0]);
    for (int s = 1; s >= 0; --s) {
        const f16 *dcat = reinterpret_cast<const f16 *>(c.base + c.ws.dcat) + s * csF;
        // both towers' weight gradients released with their dgrads (Bwd::tail_early), the last tower's split reductions left to
        // the end of the step (Bwd::defer_finalize)
        b.tail_early = true;
        if (s == 0) b.defer_finalize = true;
        OK(b.bn_bwd(t.t_bn[s], 1, nullptr, dcat, 2 * csF));
        OK(b.wgrad_dgrad(t.t_c1[s], c.dA(t.t_c3[s]), c.act(t.t_c3[s])));
        OK(b.wgrad_dgrad(t.t_c3[s], c.dy(t.in_bn[s]), nullptr, t.in_bn[s]));
        OK(b.bn_bwd(t.in_bn[s], 0, nullptr, nullptr));
        OK(b.wgrad(t.in_c[s], nullptr, s == 0));      // the very last one stays on the main stream (Bwd::wgrad)
    }
    OK(b.finish_wgrads());
#undef OK
    return IMK_OK;
}
