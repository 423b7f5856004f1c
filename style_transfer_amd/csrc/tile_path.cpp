// libstx host side: the tile evaluation -- stx_features_tile and stx_sc_grad_tile (the reference's
// CaffeModel.eval_features_tile / eval_sc_grad_tile, style_transfer.py:421-427,556-612): the forward pass
// over the blobs on the path, the backward walk to the image; the loss terms of the tapped blobs are tile_terms.cpp's.

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "engine.h"

namespace stx {

ConvProblem conv_fwd_problem(const float *x, float *y, const float *bias, int Cin, int Cout, int H, int W,
                             int ks, int relu) {
    ConvProblem p{};
    p.x = x;
    p.y = y;
    p.bias = bias;
    p.K = Cin;
    p.M = Cout;
    p.H = H;
    p.W = W;
    p.ksize = ks;
    p.relu = relu;
    p.epilogue = kEpiForward;
    return p;
}

// (backward data: the reduction runs over the layer's OUTPUT channels; mask = post-ReLU data of dx's blob, or null)
ConvProblem conv_bwd_problem(const float *dy, float *dx, const float *mask, int Cout, int Cin, int H, int W,
                             int ks) {
    ConvProblem p{};
    p.x = dy;
    p.y = dx;
    p.mask = mask;
    p.K = Cout;
    p.M = Cin;
    p.H = H;
    p.W = W;
    p.ksize = ks;
    p.epilogue = kEpiDgrad;
    return p;
}

static double conv_flops(int K, int M, int H, int W, int ks) {
    return 2.0 * K * M * ks * ks * (double)H * W;
}

// Sets blob shapes for a th x tw tile and makes sure data buffers exist for `needed` blobs.
static int shape_blobs(stx_engine *e, int th, int tw, const std::vector<char> &needed, bool with_diff) {
    Blob &in = e->blobs[e->layers[0].top_blob];
    in.h = th;
    in.w = tw;
    for (size_t li = 1; li < e->layers.size(); ++li) {
        const Layer &L = e->layers[li];
        if (L.type == STX_LAYER_RELU) continue;
        const Blob &b = e->blobs[L.bottom_blob];
        Blob &t = e->blobs[L.top_blob];
        if (L.type == STX_LAYER_CONV) {
            t.h = b.h;
            t.w = b.w;
        } else {
            t.h = pooled_len(b.h);
            t.w = pooled_len(b.w);
        }
    }
    for (size_t bi = 0; bi < e->blobs.size(); ++bi) {
        if (!needed[bi]) continue;
        Blob &b = e->blobs[bi];
        STX_TRY(b.data.ensure(b.count() * sizeof(float)));
        if (with_diff) STX_TRY(b.diff.ensure(b.count() * sizeof(float)));
    }
    return STX_OK;
}

// Marks `blob` and everything it depends on.
static void mark_ancestors(const stx_engine *e, int blob, std::vector<char> &needed) {
    while (blob >= 0 && !needed[blob]) {
        needed[blob] = 1;
        const int p = e->blobs[blob].producer;
        if (p <= 0) break;
        blob = e->layers[p].bottom_blob;
    }
}

// The bank of layer `layer`, packed from its weights the first time it is asked for.
static int get_bank(stx_engine *e, int layer, const ConvBank &bank, const float **out) {
    std::lock_guard<std::mutex> lock(e->sh->mutex);
    ConvParams &cp = e->sh->conv[layer];
    if (!cp.set) {
        set_error("weights of layer %s were never set", e->layers[layer].name.c_str());
        return STX_ERR_STATE;
    }
    auto it = cp.packed.find(bank.key);
    if (it == cp.packed.end()) {
        std::unique_ptr<DevBuf> buf(new DevBuf);
        STX_TRY(buf->ensure(bank.floats * sizeof(float)));
        STX_TRY(bank.pack(e->stream, cp.w.f(), buf->f()));
        // the other engines of this GPU will read the bank from their own streams
        if (e->sh->members.size() > 1) STX_HIP(hipStreamSynchronize(e->stream));
        it = cp.packed.emplace(bank.key, std::move(buf)).first;
    }
    *out = it->second->f();
    return STX_OK;
}

static int get_packed(stx_engine *e, int layer, int dir, const ConvConfig &cfg, const float **out) {
    const ConvParams &cp = e->sh->conv[layer];
    return get_bank(e, layer, conv_bank(cfg, dir, cp.cout, cp.cin, cp.ks), out);
}

// The configuration of convolution li in direction dir (conv_choose), tuned where the engine tunes.
static int choose_conv(stx_engine *e, int li, int dir, const ConvProblem &p, ConvConfig *out) {
    const ConvTuner tuner{e->device, e->stream, e->ev_tune0, e->ev_tune1, [=](const ConvConfig &cfg, const float **w) {
                              return get_packed(e, li, dir, cfg, w);
                          }};
    return conv_choose(p, e->winograd, e->autotune ? &tuner : nullptr, out);
}

// Gives the problem a split-K scratch buffer when conv_launch will slice the reduction.
int attach_splitk(stx_engine *e, const ConvConfig &cfg, ConvProblem &p) {
    const size_t need = conv_splitk_floats(cfg, p);
    if (!need) return STX_OK;
    STX_TRY(e->splitk.ensure(need * sizeof(float)));
    p.splitk_ws = e->splitk.f();
    p.splitk_ws_floats = e->splitk.bytes / sizeof(float);
    return STX_OK;
}

int launch_conv(stx_engine *e, const ConvConfig &cfg, const ConvProblem &problem) {
    ConvProblem p = problem;
    e->last_mark = -1;
    if (e->clock_marks && conv_takes_clock(cfg) && e->marks_used < kMaxClockMarks) {
        e->last_mark = e->marks_used++;
        p.clock_out = static_cast<long long *>(e->marks_buf.ptr) + 2 * (size_t)e->last_mark;
    }
    int var = 0;     // the specialised injecting body the launch took, as h2_launch itself reports it
    p.variant_out = &var;
    // (bookkeeping for stx_last_tile_flops)
    const int rc = conv_dispatch(e->stream, cfg, p, &e->flop_algorithmic, &e->flop_issued);
    if (var) {
        ++e->n_inject_specialised;
        e->inject_variants |= 1u << var;
    }
    return rc;
}

// The slots with max |x| of a blob's data / diff for a kernel that is about to read it: what its
// producer left (Blob::amax_data / amax_diff), else a pass over the array now.
// `consumer`: the launch group that will read it (stx_amax_audit).
static int amax_for(stx_engine *e, int blob, bool diff, const std::string &consumer, const unsigned **out) {
    Blob &b = e->blobs[blob];
    int &src = diff ? b.amax_diff : b.amax_data;
    if (src < 0) {
        ProfScope scope(e, std::string("absmax ") + b.name, 0.0);
        STX_TRY(absmax_launch(e->stream, diff ? b.diff.f() : b.data.f(), b.count(), e->amax_slots(blob, diff)));
        src = blob;
    } else if (e->amax_audit) {
        STX_TRY(amax_audit_note(e, e->stream, consumer, b.name, diff, e->amax_slots(src, diff),
                                diff ? b.diff.f() : b.data.f(), b.count()));
    }
    *out = e->amax_slots(src, diff);
    return STX_OK;
}

int amax_audit_note(stx_engine *e, hipStream_t stream, const std::string &consumer, const std::string &blob,
                    bool diff, const unsigned *slots, const float *x, size_t n) {
    if (!e->amax_audit) return STX_OK;
    if (e->audit.size() >= kMaxAmaxAudit) {
        set_error("stx_amax_audit: more than %zu hand-offs since the last stx_amax_audit_read", kMaxAmaxAudit);
        return STX_ERR_STATE;
    }
    // whose slots: a group of the engine's table (data groups, diff groups, then the scratch groups)
    const size_t group = (size_t)(slots - static_cast<const unsigned *>(e->amax.ptr)) / kAmaxSlots;
    const size_t nb = e->blobs.size();
    const std::string source = group < 2 * nb ? e->blobs[group % nb].name : "(scratch)";
    unsigned *const rec = static_cast<unsigned *>(e->audit_buf.ptr) + 2 * e->audit.size() * kAmaxSlots;
    STX_HIP(hipMemcpyAsync(rec, slots, kAmaxSlots * sizeof(unsigned), hipMemcpyDeviceToDevice, stream));
    STX_TRY(absmax_launch(stream, x, n, rec + kAmaxSlots));
    e->audit.push_back(stx_engine::AuditEntry{consumer, blob, source, diff});
    return STX_OK;
}

// Two groups of the maxima table behind the blobs' own slots, for a pass over an array that is no blob's
// (and, in a stand-alone operator call, for what the launch leaves).
int amax_scratch(stx_engine *e, unsigned **out) {
    STX_TRY(e->amax_ensure());
    *out = e->amax_slots((int)e->blobs.size(), true);
    return STX_OK;
}

// What the forward pass knows about a convolution from the layers behind it (plan_fwd_conv).
struct FwdConvPlan {
    bool force_relu;        // rectify the output though no ReLU layer follows (forward's relu_blob)
    const Layer *pool;      // the 2x2/2 pooling layer that can ride on this convolution's epilogue, or null
    int pool_li;            // ... and its layer index, or -1
    bool top_unobserved;    // with `pool`: nobody but that layer reads the full-resolution output
    bool conv_reader;       // a convolution on the path reads the output: its backward pass masks with its signs
    bool relu_codes;        // a backward pass will follow: leave ReLU sign nibbles where a kernel can
};

// One scan of the layers behind convolution li.
static FwdConvPlan plan_fwd_conv(const stx_engine *e, size_t li, const std::vector<char> &needed, int relu_blob,
                                 bool relu_codes, const std::vector<char> &observed) {
    const Layer &L = e->layers[li];
    FwdConvPlan plan{L.top_blob == relu_blob, nullptr, -1, false, false, relu_codes};
    int readers = 0;
    for (size_t lj = li + 1; lj < e->layers.size(); ++lj) {
        const Layer &P = e->layers[lj];
        if (P.type == STX_LAYER_RELU || P.bottom_blob != L.top_blob) continue;
        ++readers;
        // a convolution on the path reads this blob: its backward pass masks with the blob's signs
        plan.conv_reader |= P.type == STX_LAYER_CONV && needed[P.top_blob];
        // a 2x2/2 pooling layer fed by this blob (and nothing rectifying the pooled blob, which would
        // have to come after the pooling) can ride on the convolution's epilogue: the first such layer
        if (!plan.pool && P.type == STX_LAYER_POOL && needed[P.top_blob] && P.ksize == 2 && P.stride == 2 &&
            P.pad == 0 && !e->blobs[P.top_blob].relu && P.top_blob != relu_blob) {
            plan.pool = &P;
            plan.pool_li = (int)lj;
        }
    }
    plan.top_unobserved = plan.pool && !observed[L.top_blob] && L.top_blob != relu_blob && readers == 1;
    return plan;
}

// *pooled tells the caller whether the convolution wrote the output of plan.pool too.
static int run_conv_forward(stx_engine *e, int li, const FwdConvPlan &plan, bool *pooled) {
    const Layer &L = e->layers[li];
    const Layer *const pool = plan.pool;
    Blob &b = e->blobs[L.bottom_blob];
    Blob &t = e->blobs[L.top_blob];
    const ConvParams &cp = e->sh->conv[li];
    ConvProblem p = conv_fwd_problem(b.data.f(), t.data.f(), cp.b.f(), cp.cin, cp.cout, b.h, b.w, cp.ks,
                                     (t.relu || plan.force_relu) ? 1 : 0);
    const double direct = conv_flops(cp.cin, cp.cout, b.h, b.w, cp.ks);
    *pooled = false;
    if (conv_first_usable(cp.cin, cp.cout, cp.ks) && !pool) {
        // the first layer: its own kernel, straight from the Caffe-layout bank; with the Gram
        // partials of the blob when it is a style tap of this call
        b.relu_codes_valid = false;
        b.relu_codes_wanted = false;
        t.relu_codes_valid = false;
        unsigned *y_amax = nullptr;
        t.amax_data = -1;
        if (conv_h2_enabled()) {
            y_amax = e->amax_slots(L.top_blob, false);
            t.amax_data = L.top_blob;
        }
        float *gram = nullptr;
        if (L.top_blob == e->first_gram_blob) {
            const int parts = conv_first_workgroups(b.h, b.w);
            // (+ room for gram_finish's per-block sums of squares behind the partial tiles)
            STX_TRY(e->first_gram.ensure(((size_t)parts * 64 * 64 + 64 * 64 / 64 + 64) * sizeof(float)));
            gram = e->first_gram.f();
            e->first_gram_parts = parts;
            e->first_gram_valid = true;
        }
        ProfScope scope(e, "fwd " + L.name, direct);
        e->flop_algorithmic += direct;
        e->flop_issued += direct;
        return conv_first_launch(e->stream, p.x, cp.w.f(), cp.b.f(), p.y, cp.cin, b.h, b.w, p.relu, gram, y_amax);
    }
    ConvConfig cfg;
    STX_TRY(choose_conv(e, li, 0, p, &cfg));
    // (a blob whose producer already left its nibbles needs none from its consumer; the fp16-split kernel
    // reads the maximum of its input instead)
    b.relu_codes_wanted = !conv_reads_x_amax(cfg) && !b.relu_codes_valid && plan.relu_codes && b.relu && b.channels <= 128;  // (see below)
    p.wants_codes = b.relu_codes_wanted;
    t.amax_data = -1;
    if (conv_reads_x_amax(cfg)) STX_TRY(amax_for(e, L.bottom_blob, false, "fwd " + L.name, &p.x_amax));
    if (conv_leaves_y_amax(cfg)) {
        p.y_amax = e->amax_slots(L.top_blob, false);
        t.amax_data = L.top_blob;          // (a K-sliced launch leaves it through its reduce pass)
    }
    STX_TRY(get_packed(e, li, 0, cfg, &p.w));
    STX_TRY(attach_splitk(e, cfg, p));
    // a backward pass will follow: let this layer leave the sign nibbles of its (rectified) input
    // (up to 128 input channels -- conv1_2 and conv2_2 of a VGG: their backward pass is co-limited
    // by HBM and gains 40 / 24 us from the byte masks on a 1024^2 tile, while emitting them costs
    // the forward pass 10 / 16 us; from 256 channels on the backward pass is matrix-bound, gains
    // 0-7 us and the forward pass pays 5-10: measured, profiles/r03_relu_codes_ab.txt)
    if (b.relu_codes_wanted) {
        const size_t bytes = (size_t)b.channels * ((b.h + 1) / 2) * ((b.w + 1) / 2);
        STX_TRY(b.relu_codes.ensure(bytes));
        p.in_codes = static_cast<unsigned char *>(b.relu_codes.ptr);
        b.relu_codes_valid = conv_uses_relu_codes(cfg, p, conv_splitk_factor(cfg, p));
        if (!b.relu_codes_valid) p.in_codes = nullptr;
    }
    if (pool) {
        Blob &pt = e->blobs[pool->top_blob];
        p.pool_out = pt.data.f();
        p.pool_mode = pool->pool_mode;
        pt.codes_valid = false;
        pt.amax_data = -1;
        if (conv_fuses_pool(cfg, p)) {
            *pooled = true;
            pt.amax_data = t.amax_data;    // max (or mean) of 2x2 windows: the same bound
            if (conv_writes_pool_codes(cfg) && e->pool_codes) {
                STX_TRY(pt.codes.ensure(pt.count() + 4));    // (+ 4: conv_h2.hip fetches three codes as one dword)
                p.pool_codes = static_cast<unsigned char *>(pt.codes.ptr);
                pt.codes_valid = true;
                // the full-resolution blob is then dead weight unless somebody looks at it: the
                // next layer reads the pooled blob, the backward pooling the codes (conv1_2 of a
                // 1024^2 tile: 268 MB that were written and never read)
                p.skip_y = plan.top_unobserved;
            }
        } else {
            p.pool_out = nullptr;
        }
    }
    // ... and the nibbles of its own (rectified) output, when a convolution reads it and its backward
    // pass will mask with it: the epilogue holds one 2x2 window per lane and channel, so the byte
    // costs a handful of compares -- and the consumer's backward epilogue reads 1 byte instead of
    // 16 per lane and channel (the epilogues of one round all run at the same moment: their reads
    // and stores are a bandwidth-bound burst)
    t.relu_codes_valid = false;
    // (only beside the fp16-split kernels: STX_CONV_H2=0 keeps round 4's schedule to the letter)
    if (plan.relu_codes && t.relu && plan.conv_reader && conv_h2_enabled()) {
        const size_t bytes = (size_t)t.channels * ((t.h + 1) / 2) * ((t.w + 1) / 2);
        STX_TRY(t.relu_codes.ensure(bytes));
        p.out_codes = static_cast<unsigned char *>(t.relu_codes.ptr);
        t.relu_codes_valid = conv_writes_out_codes(cfg, p, conv_splitk_factor(cfg, p));
        if (!t.relu_codes_valid) p.out_codes = nullptr;
    }
    ProfScope scope(e, "fwd " + L.name, direct);
    return launch_conv(e, cfg, p);
}

// The backward problem of convolution layer li, as far as the choice of kernel depends on it.
static ConvProblem conv_backward_shape(stx_engine *e, int li) {
    const Layer &L = e->layers[li];
    const Blob &b = e->blobs[L.bottom_blob];
    const ConvParams &cp = e->sh->conv[li];
    return conv_bwd_problem(nullptr, nullptr, nullptr, cp.cout, cp.cin, b.h, b.w, cp.ks);
}

// Can the backward pass of convolution li take the gradient of the 2x2/2 pooling layer behind it as it
// stands -- pooled, with the window codes -- and route it inside its own patch staging (conv_h2.hip, PIN)?
// Then the pooling layer's backward kernel does not run, and the gradient of the convolution's output
// blob (four times the pooled one) is neither written nor read.  STX_POOL_BWD_FUSE=0 keeps the kernel.
static bool conv_backward_takes_pooled(stx_engine *e, int li) {
    const char *env = sw_env("STX_POOL_BWD_FUSE");
    if (env && atoi(env) == 0) return false;
    const ConvProblem p = conv_backward_shape(e, li);
    ConvConfig cfg;
    return p.ksize == 3 && p.M > 4 && conv_choose(p, e->winograd, nullptr, &cfg) == STX_OK &&
           conv_takes_pooled_input(cfg, p);
}

// Will the backward pass of convolution li scale its incoming gradient by a recorded maximum (run_conv_backward)?
static bool conv_backward_reads_amax(stx_engine *e, int li) {
    const ConvProblem p = conv_backward_shape(e, li);
    ConvConfig cfg;
    return !(p.ksize == 3 && p.M <= 4) && conv_choose(p, e->winograd, nullptr, &cfg) == STX_OK && conv_reads_x_amax(cfg);
}

// `pooled` (or null): the pooling layer behind this convolution whose backward pass the caller skipped
// (conv_backward_takes_pooled): the incoming gradient is that of the pooled blob.
static int run_conv_backward(stx_engine *e, int li, const ConvInject *inj, bool *fused, const Layer *pooled) {
    const Layer &L = e->layers[li];
    Blob &b = e->blobs[L.bottom_blob];
    const Blob &t = e->blobs[L.top_blob];
    const ConvParams &cp = e->sh->conv[li];
    ConvProblem p = conv_backward_shape(e, li);
    p.x = t.diff.f();
    p.y = b.diff.f();
    p.mask = b.relu ? b.data.f() : nullptr;
    // (kernels that cannot read the nibbles use the fp32 blob: conv_uses_relu_codes)
    p.mask_codes = b.relu && b.relu_codes_valid ? static_cast<const unsigned char *>(b.relu_codes.ptr) : nullptr;
    p.wants_codes = b.relu && b.relu_codes_wanted;
    if (cp.ks == 3 && cp.cin <= 4) {
        // backward into a <= 4-channel blob (the image): dedicated 4x4x1-MFMA kernel
        if (fused) *fused = false;
        const float *packed = nullptr;
        STX_TRY(get_bank(e, li, conv_small_bank(cp.cout, cp.cin), &packed));
        const double direct = conv_flops(cp.cout, cp.cin, b.h, b.w, cp.ks);
        ProfScope scope(e, "bwd " + L.name, direct);
        e->flop_algorithmic += direct;
        e->flop_issued += direct * 4.0 / p.M;    // the 4x4x1 MFMA computes four output channels
        return conv_small_launch(e->stream, p.x, packed, p.y, p.mask, p.K, p.M, p.H, p.W);
    }
    ConvConfig cfg;
    STX_TRY(choose_conv(e, li, 1, p, &cfg));   // (tuned without the injection terms)
    const bool can_fuse = inj && conv_takes_inject(cfg);
    if (fused) *fused = can_fuse;
    if (can_fuse) p.inject = *inj;
    b.amax_diff = -1;
    if (pooled) {
        const Blob &pt = e->blobs[pooled->top_blob];
        if (!conv_takes_pooled_input(cfg, p) || !pt.codes_valid) {
            set_error("run_conv_backward: %s cannot take the gradient of %s pooled", L.name.c_str(), pt.name.c_str());
            return STX_ERR_UNSUPPORTED;
        }
        p.x = pt.diff.f();
        p.pin_codes = static_cast<const unsigned char *>(pt.codes.ptr);
        p.pin_mode = pooled->pool_mode;
        p.pin_mask = t.relu;
        STX_TRY(amax_for(e, pooled->top_blob, true, "bwd " + L.name, &p.x_amax));    // (routing / averaging never raises the maximum)
    } else if (conv_reads_x_amax(cfg)) {
        STX_TRY(amax_for(e, L.top_blob, true, "bwd " + L.name, &p.x_amax));
    }
    if (conv_leaves_y_amax(cfg)) {
        p.y_amax = e->amax_slots(L.bottom_blob, true);
        b.amax_diff = L.bottom_blob;
    }
    STX_TRY(get_packed(e, li, 1, cfg, &p.w));
    STX_TRY(attach_splitk(e, cfg, p));
    ProfScope scope(e, "bwd " + L.name, conv_flops(cp.cout, cp.cin, b.h, b.w, cp.ks));
    return launch_conv(e, cfg, p);
}

static int begin_timing(stx_engine *e) {
    e->ev_cur = (e->ev_cur + 1) % stx_engine::kTimed;
    STX_HIP(hipEventRecord(e->ev_start[e->ev_cur], e->stream));
    e->flop_algorithmic = e->flop_issued = 0;
    return STX_OK;
}

static int end_timing(stx_engine *e) {
    STX_HIP(hipEventRecord(e->ev_stop[e->ev_cur], e->stream));
    if (e->ev_recorded < stx_engine::kTimed) ++e->ev_recorded;
    e->timed = true;
    return STX_OK;
}

// Validates the taps against the graph and the targets, orders them, shapes the blobs and plans the loss
// terms (plan_terms): a call that cannot be evaluated fails here, before its first launch.
static int sc_grad_prepare(stx_engine *e, const TileCall &c, TilePlan &plan) {
    // ---- taps in deep -> shallow order (style_transfer.py:231-233)
    std::vector<Tap> &order = plan.order;
    const stx_tap *taps = c.taps;
    const int n_taps = c.n_taps;
    const auto tapped = [&](int blob) {
        return std::any_of(order.begin(), order.end(), [=](const Tap &o) { return o.blob == blob; });
    };
    const auto has_layer_target = [&](int blob) {   // a per-layer target makes the layer part of the call
        bool any = false;
        for_each_layer_kind(*e->sh, [&](const auto &targets) { any |= target_at(targets, blob) != nullptr; });
        return any;
    };
    for (int i = 0; i < n_taps; ++i) {
        const int blob = e->find_blob(taps[i].layer);
        if (blob <= 0) {
            set_error("stx_sc_grad_tile: unknown tap layer '%s'",
                      taps[i].layer ? taps[i].layer : "(null)");
            return STX_ERR_ARG;
        }
        if (tapped(blob)) {
            set_error("stx_sc_grad_tile: layer '%s' is tapped twice", taps[i].layer);
            return STX_ERR_ARG;
        }
        if (!taps[i].is_content && !taps[i].is_style && !taps[i].is_dd && !has_layer_target(blob)) continue;
        order.push_back(Tap{blob, &taps[i]});
    }
    // a layer with a per-layer target of any kind is part of every evaluation, tapped or not
    for_each_layer_kind(*e->sh, [&](const auto &targets) {
        for (const auto &target : targets) {
            if (tapped(target.blob)) continue;
            stx_tap t{};
            t.layer_weight = 1.0;
            plan.extra.push_back(t);
            order.push_back(Tap{target.blob, &plan.extra.back()});
        }
    });
    if (order.empty()) {
        set_error("stx_sc_grad_tile: no content, style or Deep-Dream layer");
        return STX_ERR_ARG;
    }
    std::sort(order.begin(), order.end(), [](const Tap &a, const Tap &b) { return a.blob > b.blob; });
    std::vector<char> &needed = plan.needed;
    needed.assign(e->blobs.size(), 0);
    mark_ancestors(e, order[0].blob, needed);
    std::vector<int> &tap_of = plan.tap_of;
    tap_of.assign(e->blobs.size(), -1);
    for (size_t i = 0; i < order.size(); ++i) {
        if (!needed[order[i].blob]) {
            set_error("stx_sc_grad_tile: tapped layers must lie on one path through the network "
                      "('%s' does not feed '%s')", e->blobs[order[i].blob].name.c_str(),
                      e->blobs[order[0].blob].name.c_str());
            return STX_ERR_UNSUPPORTED;
        }
        tap_of[order[i].blob] = (int)i;
    }
    for (const Tap &tp : order) {
        if (tp.t->is_content && e->sh->n_contents == 0) {
            set_error("stx_sc_grad_tile: no content targets set");
            return STX_ERR_STATE;
        }
        if (tp.t->is_style && e->sh->n_styles == 0) {
            set_error("stx_sc_grad_tile: no style targets set");
            return STX_ERR_STATE;
        }
    }
    STX_TRY(shape_blobs(e, c.th, c.tw, needed, true));
    plan.sums_late = !(sw_env("STX_SUMS_LATE") && !atoi(sw_env("STX_SUMS_LATE")));
    plan.interleave = !(sw_env("STX_TERMS_LATE") && atoi(sw_env("STX_TERMS_LATE")));
    return plan_terms(e, c, plan);
}

// `blob` is complete: the loss terms of its tap, for a run that wants them inside the forward pass.
static int blob_done(TileRun *run, int blob) {
    const int k = run ? run->plan.tap_of[blob] : -1;
    return k >= 0 ? queue_tap_terms(*run, (size_t)k) : STX_OK;
}

// Runs the layers needed for `needed` blobs, in graph order.  `relu_blob` (or -1) is rectified
// even when no ReLU layer follows it (np.maximum(0, .) at style_transfer.py:426,567).
// `run` (or null): the evaluation whose loss terms are queued as soon as a tapped blob is complete, before
// the next layer is queued.  `relu_codes`: a backward pass will follow (FwdConvPlan).
// `observed`: blobs whose data somebody reads after the pass (taps, requested maps);
// a convolution whose only consumer is a pooling layer fused into it need not store the others.
static int forward(stx_engine *e, const std::vector<char> &needed, int relu_blob, TileRun *run,
                   bool relu_codes, const std::vector<char> &observed) {
    int pooled_layer = -1;      // pooling layer whose output the producing convolution wrote
    // the maxima the fp16-split convolutions leave for each other (Blob::amax_data): none yet
    STX_TRY(e->amax_ensure());
    // (the data slots and, behind them, the diff slots of a backward walk that may follow: one fill)
    STX_HIP(hipMemsetAsync(e->amax_slots(0, false), 0, 2 * e->blobs.size() * kAmaxSlots * sizeof(unsigned), e->stream));
    for (Blob &b : e->blobs) {
        b.amax_data = -1;
        b.relu_codes_valid = false;
    }
    for (size_t li = 1; li < e->layers.size(); ++li) {
        const Layer &L = e->layers[li];
        if (L.type == STX_LAYER_RELU || !needed[L.top_blob]) continue;
        const Blob &b = e->blobs[L.bottom_blob];
        Blob &t = e->blobs[L.top_blob];
        if (L.type == STX_LAYER_CONV) {
            const FwdConvPlan plan = plan_fwd_conv(e, li, needed, relu_blob, relu_codes, observed);
            bool pooled = false;
            STX_TRY(run_conv_forward(e, (int)li, plan, &pooled));
            if (pooled) pooled_layer = plan.pool_li;
            STX_TRY(blob_done(run, L.top_blob));
            if (pooled) STX_TRY(blob_done(run, plan.pool->top_blob));
        } else if ((int)li == pooled_layer) {
            continue;
        } else {
            {
                ProfScope scope(e, "fwd " + L.name, 0.0);
                unsigned char *codes = nullptr;
                t.codes_valid = false;
                if (e->pool_codes) {
                    STX_TRY(t.codes.ensure(t.count() + 4));      // (see run_conv_forward)
                    codes = static_cast<unsigned char *>(t.codes.ptr);
                    t.codes_valid = true;
                }
                STX_TRY(pool_forward_launch(e->stream, b.data.f(), b.channels, b.h, b.w, L.pool_mode,
                                            t.data.f(), codes));
                t.amax_data = b.amax_data;      // (a ReLU behind it only lowers the maximum)
                if (t.relu || L.top_blob == relu_blob)
                    STX_TRY(relu_inplace_launch(e->stream, t.data.f(), t.count()));
            }   // (the loss terms of a tapped pooled blob are timed under their own labels)
            STX_TRY(blob_done(run, L.top_blob));
        }
    }
    return STX_OK;
}

// The backward walk from the deepest tap to the image (style_transfer.py:569-610).
static int backward_walk(TileRun &run) {
    stx_engine *e = run.e;
    const int data_blob = e->layers[0].top_blob;
    int cur = run.plan.order[0].blob;
    // (the diff slots were zeroed with the data slots when the forward pass began)
    for (Blob &b : e->blobs) b.amax_diff = -1;
    {
        bool written = false;
        STX_TRY(inject_terms(run, 0, written));
        if (!written)
            STX_HIP(hipMemsetAsync(e->blobs[cur].diff.ptr, 0, e->blobs[cur].count() * sizeof(float),
                                   e->stream));
    }
    const Layer *pooled = nullptr;      // a pooling layer whose backward pass rides in the next convolution's
    while (cur != data_blob) {
        const int li = e->blobs[cur].producer;
        const Layer &L = e->layers[li];
        Blob &bot = e->blobs[L.bottom_blob];
        const Blob &top = e->blobs[cur];
        const int k = run.plan.tap_of[L.bottom_blob];
        bool fused = false;
        if (L.type == STX_LAYER_POOL && top.codes_valid && k < 0 && L.ksize == 2 && L.stride == 2 && L.pad == 0 &&
            e->layers[bot.producer].type == STX_LAYER_CONV && conv_backward_takes_pooled(e, bot.producer)) {
            // the convolution under the pooling layer un-pools inside its patch staging: nothing to launch,
            // the gradient of `bot` never exists (nobody else wants it: no loss term taps that blob)
            pooled = &L;
            cur = L.bottom_blob;
            continue;
        }
        if (L.type == STX_LAYER_CONV) {
            ConvInject inj{};
            if (k >= 0 && tap_fusable(run, (size_t)k)) {
                inj = make_inject(run, (size_t)k, bot);
                fused = true;
            }
            STX_TRY(run_conv_backward(e, li, fused ? &inj : nullptr, &fused, pooled));
            pooled = nullptr;
        } else {
            // Nobody recorded the pooled gradient's maximum (a 1x1 or few-channel layer wrote it: the direct family
            // leaves none) and the fp16-split convolution under the pooling layer will ask for one: take it from the
            // pooled gradient, a quarter of the elements -- the bound the pooled-gradient route scales by, so that
            // the two routes split their operand alike and stay bit-identical (AVE spreads a window's gradient
            // over its elements: the un-pooled array's own maximum is up to four times smaller).
            if (top.amax_diff < 0 && e->layers[bot.producer].type == STX_LAYER_CONV &&
                conv_backward_reads_amax(e, bot.producer)) {
                const unsigned *unused;
                STX_TRY(amax_for(e, cur, true, "bwd " + L.name, &unused));
            }
            ProfScope scope(e, "bwd " + L.name, 0.0);
            if (top.codes_valid)
                STX_TRY(pool_backward_codes_launch(
                    e->stream, top.diff.f(), static_cast<const unsigned char *>(top.codes.ptr),
                    bot.channels, bot.h, bot.w, L.pool_mode, bot.relu, bot.diff.f()));
            else
                STX_TRY(pool_backward_launch(e->stream, top.diff.f(), bot.data.f(), bot.channels,
                                             bot.h, bot.w, L.pool_mode, bot.relu, bot.diff.f()));
            bot.amax_diff = top.amax_diff;     // routing / averaging never raises the maximum
        }
        cur = L.bottom_blob;
        if (k >= 0 && !fused) {
            bool written = true;   // the upstream gradient is already in diff
            // (the terms are added behind the kernel that left a maximum; the slots hold that one, and
            // max is monotone: zero them so that the last term's kernel leaves the new one)
            STX_HIP(hipMemsetAsync(e->amax_slots(L.bottom_blob, true), 0, kAmaxSlots * sizeof(unsigned), e->stream));
            STX_TRY(inject_terms(run, (size_t)k, written));
        }
    }
    return STX_OK;
}

// An unmasked style term on the first layer's blob: that layer's kernel leaves its Gram partials.
// (A masked style takes the Gram of F . m: the partials are for the unmasked targets of the blob.)
static void first_gram_setup(stx_engine *e, const TilePlan &plan) {
    const int data_blob = e->layers[0].top_blob;
    e->first_gram_blob = -1;
    e->first_gram_valid = false;
    for (const PlannedTerm &t : plan.terms) {
        const int blob = plan.order[t.tap].blob, pl = e->blobs[blob].producer;
        if (t.kind == TermKind::Style && e->first_gram_blob < 0 && pl > 0 && e->layers[pl].type == STX_LAYER_CONV &&
            e->layers[pl].bottom_blob == data_blob && e->blobs[blob].channels == 64)
            e->first_gram_blob = blob;
    }
}

// Enqueues the evaluation proper: forward pass with the loss terms of the tapped blobs, backward
// walk, the mirror copy of the loss scalars.  The tile is already in the input blob; the gradient
// is left in its diff.
static int sc_grad_run(stx_engine *e, const TilePlan &plan, PendingLoss &pl) {
    const std::vector<Tap> &order = plan.order;
    TileRun run{e, plan, pl, std::vector<std::vector<Term>>(order.size()), {}};
    while (e->sgrad.size() < order.size()) e->sgrad.emplace_back(new DevBuf);
    for (size_t k = 0; k < order.size(); ++k) STX_TRY(e->sgrad[k]->ensure(plan.sgrad_floats[k] * sizeof(float)));
    STX_TRY(e->term_scratch.ensure(plan.scratch_floats * sizeof(float)));
    STX_TRY(begin_timing(e));
    std::vector<char> observed(e->blobs.size(), 0);
    for (const Tap &tp : order) observed[tp.blob] = 1;
    first_gram_setup(e, plan);
    STX_TRY(forward(e, plan.needed, order[0].blob, plan.interleave ? &run : nullptr, true, observed));
    if (!plan.interleave) {
        // (shallowest tap first, the order the interleaved schedule queues them in: the host adds
        // the loss terms up in queueing order, in double precision, and must get the same bits)
        for (size_t k = order.size(); k-- > 0;) STX_TRY(queue_tap_terms(run, k));
    }
    if (!run.sum_jobs.empty()) {
        ProfScope scope(e, "sums", 0.0);
        STX_TRY(sum_jobs_launch(e->stream, run.sum_jobs.data(), (int)run.sum_jobs.size()));
    }
    STX_TRY(backward_walk(run));
    STX_TRY(end_timing(e));
    // mirror the scalars used so far (small) for the loss
    STX_HIP(hipMemcpyAsync(e->A().host, e->A().scalars.ptr, e->A().used * sizeof(float),
                           hipMemcpyDeviceToHost, e->stream));
    return STX_OK;
}

// Is [p, p + bytes) device memory of the engine's own GPU, float-aligned?  (Host memory, managed memory and another
// GPU's memory keep the copies: hipMemcpyDefault finds its way to them, a kernel of this GPU need not.)
static bool local_device_floats(const stx_engine *e, const void *p, int mem) {
    if (mem == STX_HOST || (reinterpret_cast<uintptr_t>(p) & 3) != 0) return false;
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();     // (a pointer the runtime does not know: not an error of this call)
        return false;
    }
    return attr.type == hipMemoryTypeDevice && attr.device == e->device;
}

static bool ranges_overlap(const void *a, const void *b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bytes && y < x + bytes;
}

// Which ends of a tile evaluation can work on the caller's own buffers, with the input blob's data / diff as
// non-owning views of them while the call is queued (TileIoView) -- the kernels whose reads of the blob's data
// and whose writes of its diff have been checked against a caller's allocation, which ends with the tile
// (DevBuf rounds up to 256 bytes) and is float-aligned, not 256-byte aligned:
//   data  read by the first-layer kernel alone (conv_first.hip: dword buffer loads inside K H W floats; nobody asks
//         for the blob's maximum, no pooling layer reads it, no convolution fuses a pooling layer over it);
//   diff  written by the backward-into-image kernel alone (conv3x3_m4_kernel: one dword store per element of
//         [M][H][W], every element; its vector loads are of the OTHER blob's gradient).
// Every other graph keeps the copy at that end.  The input blob carries no loss term (sc_grad_prepare refuses a
// tap on it), so nothing else reads its data or adds to its diff.
static void tile_io_direct(stx_engine *e, const TileCall &c, const TilePlan &plan, bool *in_direct, bool *out_direct) {
    const int data_blob = e->layers[0].top_blob;
    const Blob &in = e->blobs[data_blob];
    const size_t bytes = in.count() * sizeof(float);
    *in_direct = *out_direct = false;
    if (const char *env = sw_env("STX_TILE_IO_DIRECT"))
        if (atoi(env) == 0) return;
    if (plan.tap_of[data_blob] >= 0 || in.relu) return;
    // (distinct buffers, and neither of them one of the blob's own: the engine's buffers keep today's path)
    if (ranges_overlap(c.img, c.grad_out, bytes) || ranges_overlap(c.img, in.data.ptr, in.data.bytes) ||
        ranges_overlap(c.img, in.diff.ptr, in.diff.bytes) || ranges_overlap(c.grad_out, in.data.ptr, in.data.bytes) ||
        ranges_overlap(c.grad_out, in.diff.ptr, in.diff.bytes))
        return;
    std::vector<char> observed(e->blobs.size(), 0);
    for (const Tap &tp : plan.order) observed[tp.blob] = 1;
    int readers = 0;
    bool first_only = true, small_only = true;
    for (size_t li = 1; li < e->layers.size(); ++li) {
        const Layer &L = e->layers[li];
        if (L.type == STX_LAYER_RELU || L.bottom_blob != data_blob || !plan.needed[L.top_blob]) continue;
        ++readers;
        if (L.type != STX_LAYER_CONV) {
            first_only = small_only = false;
            continue;
        }
        const ConvParams &cp = e->sh->conv[li];
        first_only &= conv_first_usable(cp.cin, cp.cout, cp.ks) &&
                      !plan_fwd_conv(e, li, plan.needed, plan.order[0].blob, true, observed).pool;
        small_only &= cp.ks == 3 && cp.cin <= 4;      // (run_conv_backward: conv_small_launch)
    }
    if (readers != 1) return;
    *in_direct = first_only && local_device_floats(e, c.img, c.img_mem);
    *out_direct = small_only && local_device_floats(e, c.grad_out, c.grad_mem);
}

// The input blob's data / diff pointed at the caller's buffers for as long as this object lives; the blob's own
// buffers come back when it goes, on the error paths too.  Launches capture pointers when they are queued.
struct TileIoView {
    Blob &in;
    void *const data, *const diff;
    TileIoView(Blob &blob, const void *img, void *grad) : in(blob), data(blob.data.ptr), diff(blob.diff.ptr) {
        if (img) in.data.ptr = const_cast<void *>(img);      // (read only: tile_io_direct)
        if (grad) in.diff.ptr = grad;
    }
    ~TileIoView() {
        in.data.ptr = data;
        in.diff.ptr = diff;
    }
    TileIoView(const TileIoView &) = delete;
    TileIoView &operator=(const TileIoView &) = delete;
};

static int sc_grad_eager(stx_engine *e, const TileCall &c, double *loss_out) {
    TilePlan plan;
    STX_TRY(sc_grad_prepare(e, c, plan));
    // the scalar arena holds the reductions of every call queued since the last stx_sync; drain
    // it (publishing the pending losses) before this call's terms could overflow it
    if (e->A().used + plan.scalars > e->scalars_cap) STX_TRY(do_sync(e));
    if (plan.scalars > e->scalars_cap) {
        set_error("stx_sc_grad_tile: %d taps need more scalar space than the arena holds", c.n_taps);
        return STX_ERR_NOMEM;
    }
    Blob &in = e->blobs[e->layers[0].top_blob];
    // (a tile handed over in the engine's own buffers, stx_tile_buffers, needs no copies; nor does one in device
    // buffers of the caller's that the first and the last kernel can work on where they are)
    bool in_direct, out_direct;
    tile_io_direct(e, c, plan, &in_direct, &out_direct);
    if (c.img != in.data.ptr && !in_direct)
        STX_TRY(copy_in(e, in.data.ptr, c.img, c.img_mem, in.count() * sizeof(float)));
    PendingLoss pl;
    pl.out = loss_out;
    {
        const TileIoView view(in, in_direct ? c.img : nullptr, out_direct ? c.grad_out : nullptr);
        STX_TRY(sc_grad_run(e, plan, pl));
    }
    if (c.grad_out != in.diff.ptr && !out_direct)
        STX_TRY(copy_out(e, c.grad_out, c.grad_mem, in.diff.ptr, in.count() * sizeof(float)));
    e->A().pending.push_back(std::move(pl));
    ++e->n_tile_evals;
    e->n_tile_io_direct += (in_direct ? 1 : 0) + (out_direct ? 1 : 0);
    return STX_OK;
}

}  // namespace stx

extern "C" {

int stx_features_tile(stx_engine *e, const float *img, int img_mem, int th, int tw,
                      const char *const *layers, int n_layers, float *const *out, int out_mem) {
    if (!e || !img || th <= 0 || tw <= 0 || n_layers <= 0 || !layers || !out) {
        set_error("stx_features_tile: bad arguments");
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    std::vector<char> needed(e->blobs.size(), 0);
    std::vector<int> want(n_layers);
    for (int i = 0; i < n_layers; ++i) {
        want[i] = e->find_blob(layers[i]);
        if (want[i] < 0 || !out[i]) {
            set_error("stx_features_tile: unknown layer '%s'", layers[i] ? layers[i] : "(null)");
            return STX_ERR_ARG;
        }
        mark_ancestors(e, want[i], needed);
    }
    STX_TRY(shape_blobs(e, th, tw, needed, false));
    Blob &in = e->blobs[e->layers[0].top_blob];
    STX_TRY(copy_in(e, in.data.ptr, img, img_mem, in.count() * sizeof(float)));
    STX_TRY(begin_timing(e));
    e->first_gram_blob = -1;       // (no loss terms here: the first layer computes no Gram partials)
    e->first_gram_valid = false;
    // the reference rectifies the net's last blob (style_transfer.py:426)
    const int last_blob = (int)e->blobs.size() - 1;
    std::vector<char> observed(e->blobs.size(), 0);
    for (int i = 0; i < n_layers; ++i) observed[want[i]] = 1;
    STX_TRY(forward(e, needed, needed[last_blob] ? last_blob : -1, nullptr, false, observed));
    STX_TRY(end_timing(e));
    for (int i = 0; i < n_layers; ++i) {
        const Blob &b = e->blobs[want[i]];
        STX_TRY(copy_out(e, out[i], out_mem, b.data.ptr, b.count() * sizeof(float)));
    }
    return STX_OK;
}

int stx_sc_grad_tile(stx_engine *e, const float *img, int img_mem, int th, int tw,
                     const int roll_xy[2], const int start_yx[2], const stx_tap *taps, int n_taps,
                     double *loss_out, float *grad_out, int grad_mem, int sync_now) {
    // (n_taps = 0: the layers of the statistics targets alone; without such targets sc_grad_prepare refuses it)
    if (!e || !img || th <= 0 || tw <= 0 || n_taps < 0 || (!taps && n_taps > 0) || !grad_out || !start_yx) {
        set_error("stx_sc_grad_tile: bad arguments");
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    const TileCall c{img, img_mem, th, tw, roll_xy ? roll_xy[0] : 0, roll_xy ? roll_xy[1] : 0,
                     {start_yx[0], start_yx[1]}, taps, n_taps, grad_out, grad_mem};
    STX_TRY(sc_grad_eager(e, c, loss_out));
    if (sync_now) return do_sync(e);
    return STX_OK;
}

int stx_tile_buffers(stx_engine *e, int th, int tw, float **tile_in, float **grad_out) {
    if (!e || th <= 0 || tw <= 0 || !tile_in || !grad_out) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    Blob &in = e->blobs[e->layers[0].top_blob];
    const size_t bytes = (size_t)in.channels * th * tw * sizeof(float);
    STX_TRY(in.data.ensure(bytes));
    STX_TRY(in.diff.ensure(bytes));
    *tile_in = in.data.f();
    *grad_out = in.diff.f();
    return STX_OK;
}

int stx_gram_matrix(stx_engine *e, const float *feat, int feat_mem, int channels, int hw,
                    float *gram_out, int gram_mem) {
    if (!e || !feat || !gram_out || channels <= 0 || hw <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    const float *src = feat;
    if (feat_mem == STX_HOST) {
        STX_TRY(e->upload.ensure((size_t)channels * hw * sizeof(float)));
        STX_TRY(copy_in(e, e->upload.ptr, feat, STX_HOST, (size_t)channels * hw * sizeof(float)));
        src = e->upload.f();
    }
    const GramPlan plan = gram_plan(channels, hw);
    STX_TRY(e->gram_partials.ensure(plan.partial_floats * sizeof(float)));
    STX_TRY(e->gram.ensure((size_t)channels * channels * sizeof(float)));
    const unsigned *f_amax = nullptr;
    if (gram_h2_usable(src, channels, hw)) {       // the fp16 two-piece kernel: scaled by the array's maximum
        unsigned *scratch;
        STX_TRY(amax_scratch(e, &scratch));
        STX_TRY(absmax_launch(e->stream, src, (size_t)channels * hw, scratch));
        f_amax = scratch;
    }
    STX_TRY(gram_partials_launch(e->stream, src, plan, e->gram_partials.f(), f_amax));
    STX_TRY(gram_finish_launch(e->stream, e->gram_partials.f(), plan, e->gram.f(), nullptr, nullptr,
                               nullptr, nullptr, f_amax));
    STX_TRY(copy_out(e, gram_out, gram_mem, e->gram.ptr, (size_t)channels * channels * sizeof(float)));
    if (feat_mem == STX_HOST || gram_mem == STX_HOST) STX_HIP(hipStreamSynchronize(e->stream));
    return STX_OK;
}

int stx_feature_stats(stx_engine *e, const float *feat, int feat_mem, int channels, int hw, float *mean_out,
                      float *sd_out, int out_mem) {
    if (!e || !feat || !mean_out || !sd_out || channels <= 0 || hw <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    const float *src = feat;
    if (feat_mem == STX_HOST) {
        STX_TRY(e->upload.ensure((size_t)channels * hw * sizeof(float)));
        STX_TRY(copy_in(e, e->upload.ptr, feat, STX_HOST, (size_t)channels * hw * sizeof(float)));
        src = e->upload.f();
    }
    const size_t parts = 4 * (size_t)channels * stat_slices(hw);
    STX_TRY(e->stat_scratch.ensure((parts + 2 * (size_t)channels) * sizeof(float)));
    float *mu = e->stat_scratch.f() + parts, *sd = mu + channels;
    // the first two launches of the term itself (launch_stat_terms): a tile's own statistics are its targets
    STX_TRY(stat_partials_launch(e->stream, src, channels, hw, e->stat_scratch.f()));
    STX_TRY(stat_finish_launch(e->stream, e->stat_scratch.f(), channels, hw, nullptr, nullptr, nullptr, nullptr, mu, sd));
    STX_TRY(copy_out(e, mean_out, out_mem, mu, (size_t)channels * sizeof(float)));
    STX_TRY(copy_out(e, sd_out, out_mem, sd, (size_t)channels * sizeof(float)));
    if (feat_mem == STX_HOST || out_mem == STX_HOST) STX_HIP(hipStreamSynchronize(e->stream));
    return STX_OK;
}

int stx_shift_gram(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, const int *offsets,
                   int n_offsets, float *out) {
    if (!e || !feat || !out) {
        set_error("stx_shift_gram: bad arguments");
        return STX_ERR_ARG;
    }
    ShiftOffsets off;
    STX_TRY(shift_check_offsets("stx_shift_gram", channels, offsets, n_offsets, &off));
    STX_TRY(shift_check_map("stx_shift_gram", channels, h, w, off));
    STX_TRY(e->set_device());
    const int n = h * w;
    const float *src = feat;
    if (feat_mem == STX_HOST) {
        STX_TRY(e->upload.ensure((size_t)channels * n * sizeof(float)));
        STX_TRY(copy_in(e, e->upload.ptr, feat, STX_HOST, (size_t)channels * n * sizeof(float)));
        src = e->upload.f();
    }
    const size_t x_floats = (size_t)n_offsets * channels * channels;
    const size_t scratch_floats = shift_scratch_floats(channels, n, n_offsets);
    STX_TRY(e->shift_io.ensure((scratch_floats + x_floats) * sizeof(float)));
    const ShiftScratch x = shift_scratch(e->shift_io.f(), channels, n, n_offsets);
    float *const x_dev = e->shift_io.f() + scratch_floats;
    // the first two launches of the term itself (launch_shift_terms): a tile's own X are its targets
    STX_TRY(shift_cross_launch(e->stream, src, channels, h, w, off, x));
    STX_TRY(shift_merge_launch(e->stream, channels, h, w, off, x, nullptr, x_dev, nullptr));
    STX_TRY(copy_out(e, out, STX_HOST, x_dev, x_floats * sizeof(float)));
    STX_HIP(hipStreamSynchronize(e->stream));
    return STX_OK;
}

int stx_swd_target(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, const float *V,
                   int dirs, int quantiles, float *out) {
    if (!e || !feat || !V || !out || h <= 0 || w <= 0) {
        set_error("stx_swd_target: bad arguments");
        return STX_ERR_ARG;
    }
    STX_TRY(swd_check("stx_swd_target", channels, (long long)h * w, dirs, quantiles));
    STX_TRY(e->set_device());
    const int n = h * w;
    const float *src = feat;
    if (feat_mem == STX_HOST) {
        STX_TRY(e->upload.ensure((size_t)channels * n * sizeof(float)));
        STX_TRY(copy_in(e, e->upload.ptr, feat, STX_HOST, (size_t)channels * n * sizeof(float)));
        src = e->upload.f();
    }
    const size_t v_floats = ((size_t)dirs * channels + 63) & ~(size_t)63;
    STX_TRY(e->swd_io.ensure((v_floats + (size_t)dirs * quantiles) * sizeof(float)));
    STX_TRY(e->swd_work.ensure(2 * (size_t)dirs * swd_padded(n) * sizeof(float)));
    float *const v_dev = e->swd_io.f(), *const q_dev = v_dev + v_floats;
    STX_TRY(copy_in(e, v_dev, V, STX_HOST, (size_t)dirs * channels * sizeof(float)));
    // the first two steps of the term itself (launch_swd_terms), the sorted rows kept, then their resampling
    STX_TRY(swd_project_launch(e->stream, src, channels, n, v_dev, dirs, e->swd_work.ptr));
    STX_TRY(swd_sort_launch(e->stream, e->swd_work.ptr, n, dirs));
    STX_TRY(swd_finish_launch(e->stream, e->swd_work.ptr, n, dirs, nullptr, 0, nullptr, nullptr, nullptr));
    STX_TRY(swd_quantiles_launch(e->stream, e->swd_work.ptr, n, dirs, quantiles, q_dev));
    STX_TRY(copy_out(e, out, STX_HOST, q_dev, (size_t)dirs * quantiles * sizeof(float)));
    STX_HIP(hipStreamSynchronize(e->stream));
    return STX_OK;
}

int stx_cx_rows(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, int rows, float *rows_out,
                int out_mem) {
    if (!e || !feat || !rows_out || channels <= 0 || h <= 0 || w <= 0 || rows < 1) {
        set_error("stx_cx_rows: bad arguments (%d channels, a %dx%d map, %d rows)", channels, h, w, rows);
        return STX_ERR_ARG;
    }
    if (channels % 64 != 0) {       // (the gather walks the channels in whole blocks of 64, as the term does)
        set_error("stx_cx_rows: %d channels (a multiple of 64 is expected)", channels);
        return STX_ERR_UNSUPPORTED;
    }
    STX_TRY(e->set_device());
    const SelfsimGrid gr = selfsim_grid(h, w, rows);
    const size_t in_bytes = (size_t)channels * h * w * sizeof(float), out_floats = (size_t)gr.N * channels;
    const float *src = feat;
    if (feat_mem == STX_HOST) {
        STX_TRY(e->upload.ensure(in_bytes));
        STX_TRY(copy_in(e, e->upload.ptr, feat, STX_HOST, in_bytes));
        src = e->upload.f();
    }
    float *dst = rows_out;
    if (out_mem == STX_HOST) {
        STX_TRY(e->cx_io.ensure(out_floats * sizeof(float)));
        dst = e->cx_io.f();
    }
    STX_TRY(cx_rows_launch(e->stream, src, channels, h, w, gr, dst));
    if (out_mem == STX_HOST) STX_TRY(copy_out(e, rows_out, STX_HOST, dst, out_floats * sizeof(float)));
    if (feat_mem == STX_HOST || out_mem == STX_HOST) STX_HIP(hipStreamSynchronize(e->stream));
    return STX_OK;
}

int stx_cx_bank(stx_engine *e, const float *raw_rows, int mem, int channels, int rows, float *mu_out, float *bank_out,
                int out_mem) {
    if (!e || !raw_rows || !mu_out || !bank_out) {
        set_error("stx_cx_bank: bad arguments");
        return STX_ERR_ARG;
    }
    STX_TRY(cx_check("stx_cx_bank", channels, 2, rows, 1.0));
    STX_TRY(e->set_device());
    // the staged rows, then (a host destination) the bank and mu
    const size_t floats = (size_t)rows * channels, staged = mem == STX_HOST ? floats : 0;
    STX_TRY(e->cx_io.ensure((staged + (out_mem == STX_HOST ? floats + channels : 0)) * sizeof(float)));
    const float *src = raw_rows;
    if (mem == STX_HOST) {
        STX_TRY(copy_in(e, e->cx_io.ptr, raw_rows, STX_HOST, floats * sizeof(float)));
        src = e->cx_io.f();
    }
    float *bank = out_mem == STX_HOST ? e->cx_io.f() + staged : bank_out;
    float *mu = out_mem == STX_HOST ? bank + floats : mu_out;
    STX_TRY(cx_bank_launch(e->stream, src, channels, rows, mu, bank));
    if (out_mem == STX_HOST) {
        STX_TRY(copy_out(e, bank_out, STX_HOST, bank, floats * sizeof(float)));
        STX_TRY(copy_out(e, mu_out, STX_HOST, mu, (size_t)channels * sizeof(float)));
    }
    STX_HIP(hipStreamSynchronize(e->stream));
    return STX_OK;
}

// Both bank entries, their arguments accepted: the pass (patch 3: the passes) that prepares a tile's blob for the
// search (nnfm.hip), with the float32 rows as the output.  The engine's nnfm_scratch holds the rows of a host
// destination, then the work area of patch 3.
static int nnfm_bank_rows(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, int patch,
                          int stride, float *bank_out, int out_mem) {
    STX_TRY(e->set_device());
    const size_t in_bytes = (size_t)channels * h * w * sizeof(float);
    const size_t out_floats = (size_t)ceil_div(h, stride) * ceil_div(w, stride) * patch * patch * channels;
    const float *src = feat;
    if (feat_mem == STX_HOST) {
        STX_TRY(e->upload.ensure(in_bytes));
        STX_TRY(copy_in(e, e->upload.ptr, feat, STX_HOST, in_bytes));
        src = e->upload.f();
    }
    const size_t staged = out_mem == STX_HOST ? (out_floats + 63) & ~(size_t)63 : 0;
    const size_t work = patch == 3 ? nnfm_patch_work_floats(h * w) : 0;
    STX_TRY(e->nnfm_scratch.ensure((staged + work) * sizeof(float)));
    float *dst = out_mem == STX_HOST ? e->nnfm_scratch.f() : bank_out;
    STX_TRY(nnfm_prepare_launch(e->stream, src, channels, h, w, patch, stride,
                                work ? reinterpret_cast<double *>(e->nnfm_scratch.f() + staged) : nullptr, nullptr,
                                nullptr, nullptr, dst));
    if (out_mem == STX_HOST) STX_TRY(copy_out(e, bank_out, STX_HOST, dst, out_floats * sizeof(float)));
    // (a side on the host; or the work area, which is the engine's: the rows are complete before another call may
    // reuse it)
    if (work || feat_mem == STX_HOST || out_mem == STX_HOST) STX_HIP(hipStreamSynchronize(e->stream));
    return STX_OK;
}

int stx_nnfm_bank(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, int stride,
                  float *bank_out, int out_mem) {
    if (!e || !feat || !bank_out || channels <= 0 || h <= 0 || w <= 0 || stride < 1) return STX_ERR_ARG;
    return nnfm_bank_rows(e, feat, feat_mem, channels, h, w, 1, stride, bank_out, out_mem);
}

int stx_nnfm_patch_bank(stx_engine *e, const float *feat, int feat_mem, int channels, int h, int w, int patch,
                        int stride, float *bank_out, int out_mem) {
    if (patch == 1) return stx_nnfm_bank(e, feat, feat_mem, channels, h, w, stride, bank_out, out_mem);
    if (patch != 3 || !e || !feat || !bank_out || channels <= 0 || h <= 0 || w <= 0 || stride < 1) {
        set_error("stx_nnfm_patch_bank: bad arguments (patch %d; 1 or 3 is expected)", patch);
        return STX_ERR_ARG;
    }
    const long long rows = (long long)ceil_div(h, stride) * ceil_div(w, stride);
    if (channels % 64 != 0 || (long long)h * w >= (1ll << 31) / channels || rows >= (1ll << 31) / (9ll * channels)) {
        set_error("stx_nnfm_patch_bank: %lld rows of 9 x %d channels from a %dx%d map (a multiple of 64 and rows x 9 "
                  "channels below 2^31 are expected)", rows, channels, h, w);
        return STX_ERR_UNSUPPORTED;
    }
    return nnfm_bank_rows(e, feat, feat_mem, channels, h, w, 3, stride, bank_out, out_mem);
}

}  // extern "C"
