// libstx host side: the tile evaluation -- stx_features_tile and stx_sc_grad_tile (the reference's
// CaffeModel.eval_features_tile / eval_sc_grad_tile, style_transfer.py:421-427,556-612): the forward pass
// over the blobs on the path, the loss terms of the tapped blobs, the backward walk to the image.

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <deque>

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
    // (bookkeeping for stx_last_tile_flops)
    return conv_dispatch(e->stream, cfg, p, &e->flop_algorithmic, &e->flop_issued);
}

// The slots with max |x| of a blob's data / diff for a kernel that is about to read it: what its
// producer left (Blob::amax_data / amax_diff), else a pass over the array now.
static int amax_for(stx_engine *e, int blob, bool diff, const unsigned **out) {
    Blob &b = e->blobs[blob];
    int &src = diff ? b.amax_diff : b.amax_data;
    if (src < 0) {
        ProfScope scope(e, std::string("absmax ") + b.name, 0.0);
        STX_TRY(absmax_launch(e->stream, diff ? b.diff.f() : b.data.f(), b.count(), e->amax_slots(blob, diff)));
        src = blob;
    }
    *out = e->amax_slots(src, diff);
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
    if (conv_reads_x_amax(cfg)) STX_TRY(amax_for(e, L.bottom_blob, false, &p.x_amax));
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
        STX_TRY(amax_for(e, pooled->top_blob, true, &p.x_amax));    // (routing / averaging never raises the maximum)
    } else if (conv_reads_x_amax(cfg)) {
        STX_TRY(amax_for(e, L.top_blob, true, &p.x_amax));
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

// Floats of the engine's term_scratch that one style term of a C-channel, HW-pixel blob takes when its
// final sums are deferred: 2 x gram_finish's blocks + the SYMM kernel's workgroups, which outlive the call.
static size_t style_term_scratch_floats(int C, int HW) {
    return 2 * (size_t)ceil_div(C * C, 64) + (size_t)symm_num_workgroups(C, HW) + 64;
}

// Style terms of one tapped blob, the launches of style_transfer.py:584-593 in order: Gram of
// `feat` -> D = G - target (fp32 + bf16 pieces) -> S = sym(D) feat into `sgrad`;
// sc[0] = sum of squares of tril(D), sc[1] = sum |S| (one small launch for both).
// f_amax (or null): the kAmaxSlots words bounding |feat| that its producer left -- the fp16 two-piece
// Gram and SYMM kernels (f16x2.h) scale by them; without them a pass over `feat` comes first.
// term_scratch + defer (or null: sc[0], sc[1] are final when this returns): style_term_scratch_floats
// floats, and the list that receives the two final sums for ONE launch behind the forward pass
// (sum_jobs_launch).
int launch_style_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w,
                       const float *target, float *sgrad, float *sc, const std::string &name,
                       const unsigned *f_amax, float *term_scratch, std::vector<SumJob> *defer) {
    const int HW = h * w;
    // the first layer's kernel may have left this blob's Gram partials already (conv_first.hip)
    const bool fused = e->first_gram_valid && e->first_gram_blob >= 0 &&
                       feat == e->blobs[e->first_gram_blob].data.f() && C == 64;
    GramPlan plan = gram_plan(C, HW);
    if (fused) {
        plan.splits = e->first_gram_parts;
        plan.tiles = 1;
        plan.parts = 1;
        plan.partial_floats = (size_t)plan.splits * 64 * 64;
    }
    const int fin_blocks = gram_finish_blocks(plan);
    float *const partials = fused ? e->first_gram.f() : nullptr;
    // (behind the partial tiles: gram_finish's per-block sums of squares and maxima)
    if (!fused) STX_TRY(e->gram_partials.ensure((plan.partial_floats + 2 * fin_blocks) * sizeof(float)));
    STX_TRY(e->dsym.ensure((size_t)C * C * sizeof(float)));
    const bool gram_h2 = !fused && gram_h2_usable(feat, C, HW);
    const bool symm_h2 = symm_h2_usable(feat, sgrad, C, HW);
    const bool bf3 = !symm_h2 && symm_bf3_usable(feat, sgrad, C, HW);
    if ((gram_h2 || symm_h2) && !f_amax) {
        unsigned *scratch;
        STX_TRY(amax_scratch(e, &scratch));
        ProfScope scope(e, "absmax " + name, 0.0, stream);
        STX_TRY(absmax_launch(stream, feat, (size_t)C * HW, scratch));
        f_amax = scratch;
    }
    if (bf3) STX_TRY(e->dsym_pieces.ensure(symm_pieces_elems(C) * sizeof(unsigned short)));
    unsigned short *pieces = bf3 && C % 64 == 0 ? static_cast<unsigned short *>(e->dsym_pieces.ptr) : nullptr;
    {
        ProfScope scope(e, "gram " + name, 2.0 * C * C * (double)HW, stream);
        if (!fused) STX_TRY(gram_partials_launch(stream, feat, plan, e->gram_partials.f(), gram_h2 ? f_amax : nullptr));
        STX_TRY(gram_finish_launch(stream, fused ? partials : e->gram_partials.f(), plan, nullptr, target,
                                   e->dsym.f(), nullptr, pieces, gram_h2 ? f_amax : nullptr,
                                   defer ? term_scratch : nullptr));
    }
    ProfScope scope(e, "symm " + name, 2.0 * C * C * (double)HW, stream);
    const float *block_sumsq = defer ? term_scratch : (fused ? partials : e->gram_partials.f()) + plan.partial_floats;
    // the two final sums: now, or as two jobs of the caller's one launch
    auto finish = [&](float *symm_partials, int n_wg) -> int {
        if (!defer) return sum_partials2_launch(stream, block_sumsq, fin_blocks, sc, symm_partials, n_wg, sc + 1);
        defer->push_back(SumJob{block_sumsq, fin_blocks, sc});
        defer->push_back(SumJob{symm_partials, n_wg, sc + 1});
        return STX_OK;
    };
    if (symm_h2 || bf3) {
        const int n_wg = symm_num_workgroups(C, HW);
        float *symm_partials = defer ? term_scratch + 2 * fin_blocks : nullptr;
        if (!defer) {
            STX_TRY(e->symm_partials.ensure((size_t)n_wg * sizeof(float)));
            symm_partials = e->symm_partials.f();
        }
        if (symm_h2)
            STX_TRY(symm_h2_launch(stream, feat, e->dsym.f(), reinterpret_cast<const unsigned *>(block_sumsq + fin_blocks),
                                   fin_blocks, f_amax, sgrad, symm_partials, C, HW));
        else
            STX_TRY(symm_bf3_launch(stream, feat, e->dsym.f(), static_cast<unsigned short *>(e->dsym_pieces.ptr),
                                    pieces != nullptr, sgrad, symm_partials, C, HW));
        return finish(symm_partials, n_wg);
    }
    const ConvConfig cfg = conv_pick_config(1, C, C, h, w);
    const int n_wg = conv_num_workgroups(cfg, C, h, w);
    STX_TRY(e->symm_partials.ensure((size_t)n_wg * sizeof(float)));
    ConvProblem p{};
    p.x = feat;
    p.w = e->dsym.f();
    p.y = sgrad;
    p.partials = e->symm_partials.f();
    p.K = C;
    p.M = C;
    p.H = h;
    p.W = w;
    p.ksize = 1;
    p.epilogue = kEpiSymm;
    STX_TRY(conv_launch(stream, cfg, p, false));
    // (this path keeps its SYMM partials in the engine's shared buffer: its two sums are launched here)
    return sum_partials2_launch(stream, block_sumsq, fin_blocks, sc, e->symm_partials.f(), n_wg, sc + 1);
}

// The style term of a masked style (style_mask.hip), around launch_style_terms as it stands:
//   Fm = feat . m with the partials of sum m^2  ->  T' = a target, a = sum m^2 / HW  ->  Gram / SYMM on (Fm, T')
//   ->  S <- a m . S with the partials of sum |m . S|, whose final sum joins `defer` or is launched here.
// |Fm| <= |feat|: the producer's f_amax stays a valid bound for the fp16-split kernels.  Fm is not the
// first layer's blob, so that layer's fused Gram partials are never taken for it.
int launch_masked_style_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w,
                              const float *mask_map, const ContentWindow &win, const float *target,
                              float *sgrad, float *sc, const std::string &name, const unsigned *f_amax,
                              float *term_scratch, float *mask_scratch, std::vector<SumJob> *defer) {
    STX_TRY(e->masked_feat.ensure((size_t)C * h * w * sizeof(float)));
    STX_TRY(e->masked_target.ensure((size_t)C * C * sizeof(float)));
    float *const m2_partials = mask_scratch, *const ms_partials = mask_scratch + kMaskParts;
    {
        ProfScope scope(e, "mask " + name, 0.0, stream);
        int n_m2 = 0;
        STX_TRY(mask_apply_launch(stream, feat, mask_map, win, e->masked_feat.f(), m2_partials, &n_m2));
        STX_TRY(mask_target_launch(stream, target, C, m2_partials, n_m2, h * w, e->masked_target.f(), sc + 3));
    }
    STX_TRY(launch_style_terms(e, stream, e->masked_feat.f(), C, h, w, e->masked_target.f(), sgrad, sc, name,
                               f_amax, term_scratch, defer));
    ProfScope scope(e, "smask " + name, 0.0, stream);
    int n_ms = 0;
    STX_TRY(mask_sgrad_launch(stream, sgrad, mask_map, win, sc + 3, ms_partials, &n_ms));
    if (!defer) return sum_partials_launch(stream, ms_partials, n_ms, sc + 2);
    defer->push_back(SumJob{ms_partials, n_ms, sc + 2});
    return STX_OK;
}

// The mean / std term of one tapped blob (stat.hip): the slices' partials, their merge against the targets
// (table and E), S with the partials of sum |S|.  Everything in stat_scratch outlives the call.
int launch_stat_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w, const float *MU,
                      const float *SD, float *sgrad, float *sc, const std::string &name, float *stat_scratch,
                      std::vector<SumJob> *defer) {
    const int HW = h * w;
    float *const partials = stat_scratch;
    float *const table = partials + 4 * (size_t)C * stat_slices(HW);
    float *const abs_partials = table + 4 * (size_t)C;
    ProfScope scope(e, "stat " + name, 0.0, stream);
    STX_TRY(stat_partials_launch(stream, feat, C, HW, partials));
    STX_TRY(stat_finish_launch(stream, partials, C, HW, MU, SD, table, sc, nullptr, nullptr));
    int n_parts = 0;
    STX_TRY(stat_grad_launch(stream, feat, C, HW, table, sgrad, abs_partials, &n_parts));
    if (!defer) return sum_partials_launch(stream, abs_partials, n_parts, sc + 1);
    defer->push_back(SumJob{abs_partials, n_parts, sc + 1});
    return STX_OK;
}

// A content term through a weight map (content_mask.hip): the window's mean weight, then the pass that writes
// S = a (m d) with the partials of sum m d^2 and sum |m d|, added like content_sums_launch's.
int launch_masked_content_terms(stx_engine *e, hipStream_t stream, const float *feat, const float *content,
                                const float *mask_map, const ContentWindow &win, float *sgrad, float *sc,
                                const std::string &name, float *partials, std::vector<SumJob> *defer) {
    ProfScope scope(e, "cmask " + name, 0.0, stream);
    STX_TRY(content_mask_mean_launch(stream, mask_map, win, sc + 2));
    int n = 0;
    STX_TRY(content_mask_term_launch(stream, feat, content, mask_map, win, sc + 2, sgrad, partials, &n));
    if (!defer) return sum_partials2_launch(stream, partials, n, sc, partials + n, n, sc + 1);
    defer->push_back(SumJob{partials, n, sc});
    defer->push_back(SumJob{partials + n, n, sc + 1});
    return STX_OK;
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

namespace {

struct Tap {
    int blob;
    const stx_tap *t;
};

// One stx_sc_grad_tile call.
struct TileCall {
    const float *img;
    int img_mem, th, tw, rx, ry, start[2];
    const stx_tap *taps;
    int n_taps;
    float *grad_out;
    int grad_mem;
};

struct TilePlan {
    std::vector<Tap> order;         // taps, deepest first
    std::vector<char> needed;       // blobs on the path
    std::vector<int> tap_of;        // blob -> index into order, or -1
    std::deque<stx_tap> extra;      // taps of the layers that only a statistics target names (lw = 1);
                                    // `order` points into it: a deque's elements stay where they are
};

// One loss term of a tapped blob, as the backward walk adds it to the blob's gradient.
struct Term {
    bool style;
    const float *src;        // style: S = sym(tril(G - Gs)) F;  content: the content map
    const float *sums;       // style: &sum|S|;  content: {sum c^2, sum |c|}
    float coef;
    ContentWindow win;
};

// One evaluation (sc_grad_run): what its steps share.
struct TileRun {
    stx_engine *e;
    const TileCall &c;
    const TilePlan &plan;
    PendingLoss &pl;
    // The final sums of the loss terms (two per style term, two per content term) are collected and run
    // as ONE launch behind the forward pass (STX_SUMS_LATE=0: each where it arises, as rounds 1-4 did);
    // what they add up must outlive the term's own launches: one scratch region per style term.
    bool sums_late;
    bool interleave;         // (STX_TERMS_LATE=1: all loss terms after the forward pass, for A/B measurements)
    std::vector<std::vector<Term>> terms;     // per tap, in plan.order
    std::vector<SumJob> sum_jobs;
    size_t scratch_used;     // floats of the engine's term_scratch that style terms have taken
    std::vector<SumJob> *defer() { return sums_late ? &sum_jobs : nullptr; }
};

}  // namespace

// The mean / std target of `blob` (stx_set_stat_targets), or null.
static const StatTarget *stat_target_of(const stx_engine *e, int blob) {
    for (const StatTarget &t : e->sh->stats)
        if (t.blob == blob) return &t;
    return nullptr;
}

// Validates the taps against the graph and the targets, orders them and shapes the blobs.
static int sc_grad_prepare(stx_engine *e, const TileCall &c, TilePlan &plan) {
    // ---- taps in deep -> shallow order (style_transfer.py:231-233)
    std::vector<Tap> &order = plan.order;
    const stx_tap *taps = c.taps;
    const int n_taps = c.n_taps;
    for (int i = 0; i < n_taps; ++i) {
        const int blob = e->find_blob(taps[i].layer);
        if (blob <= 0) {
            set_error("stx_sc_grad_tile: unknown tap layer '%s'",
                      taps[i].layer ? taps[i].layer : "(null)");
            return STX_ERR_ARG;
        }
        for (const Tap &o : order)
            if (o.blob == blob) {
                set_error("stx_sc_grad_tile: layer '%s' is tapped twice", taps[i].layer);
                return STX_ERR_ARG;
            }
        if (!taps[i].is_content && !taps[i].is_style && !taps[i].is_dd && !stat_target_of(e, blob)) continue;
        order.push_back(Tap{blob, &taps[i]});
    }
    // a layer with a statistics target is part of every evaluation, tapped or not
    for (const StatTarget &st : e->sh->stats) {
        bool tapped = false;
        for (const Tap &o : order) tapped |= o.blob == st.blob;
        if (tapped) continue;
        stx_tap t{};
        t.layer_weight = 1.0;
        plan.extra.push_back(t);
        order.push_back(Tap{st.blob, &plan.extra.back()});
    }
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

    return shape_blobs(e, c.th, c.tw, needed, true);
}

// The window of blob b's tile in a ch x cw content map: start_ = start // scale (style_transfer.py:572);
// roll // scale per layer (:647-655)
static ContentWindow content_window(const Blob &b, int ch, int cw, const int start[2], int rx, int ry) {
    ContentWindow win;
    win.C = b.channels;
    win.fh = b.h;
    win.fw = b.w;
    win.ch = ch;
    win.cw = cw;
    win.oy = (int)std::floor((double)start[0] / b.scale);
    win.ox = (int)std::floor((double)start[1] / b.scale);
    win.sx = (int)std::floor((double)rx / b.scale);
    win.sy = (int)std::floor((double)ry / b.scale);
    return win;
}

// ... and its Deep-Dream form: a map of the blob's own size, nothing shifted.
static ContentWindow dream_window(const Blob &b) {
    const int origin[2] = {0, 0};
    return content_window(b, b.h, b.w, origin, 0, 0);
}

// The sums of tap k's residual against `target` (null: a zero map) under `label`, as a loss term of
// weight / 2 and a gradient term of weight.
static int queue_residual_term(TileRun &run, size_t k, const char *label, const float *target,
                               const ContentWindow &win, double weight) {
    stx_engine *e = run.e;
    const Blob &b = e->blobs[run.plan.order[k].blob];
    size_t si;
    STX_TRY(alloc_scalars(e, 2 + 2 * 1024, &si));
    float *sums = e->A().scalars.f() + si;
    {
        ProfScope scope(e, label + b.name, 0.0, e->stream);
        STX_TRY(content_sums_launch(e->stream, b.data.f(), target, win, sums, run.defer()));
    }
    run.pl.terms.push_back(LossTerm{si, weight * 0.5});
    run.terms[k].push_back(Term{false, target, sums, (float)weight, win});
    return STX_OK;
}

// The content mask map at `blob` (stx_set_content_mask), or null.
static const ContentMask *content_mask_of(const stx_engine *e, int blob) {
    for (const ContentMask &m : e->sh->cmasks)
        if (m.blob == blob) return &m;
    return nullptr;
}

// The term of content target `ct` of tap k through the mask map (its size is the content map's: `win` is the
// window of both): launch_masked_content_terms into `sgrad`, which then rides as a gradient blob.
static int queue_masked_content_term(TileRun &run, size_t k, const ContentTarget &ct, const ContentMask &mk,
                                     const ContentWindow &win, float *sgrad) {
    stx_engine *e = run.e;
    const Tap &tp = run.plan.order[k];
    const Blob &b = e->blobs[tp.blob];
    if (win.oy < 0 || win.ox < 0) {
        set_error("content mask window [%d+%d, %d+%d] exceeds the %dx%d mask map of layer %s",
                  win.oy, win.fh, win.ox, win.fw, win.ch, win.cw, b.name.c_str());
        return STX_ERR_ARG;
    }
    size_t si;
    STX_TRY(alloc_scalars(e, 4, &si));
    float *sc = e->A().scalars.f() + si;   // [0] = sum m d^2, [1] = sum |m d|, [2] = a
    float *partials = e->term_scratch.f() + run.scratch_used;
    run.scratch_used += kContentMaskScratchFloats;
    STX_TRY(launch_masked_content_terms(e, e->stream, b.data.f(), ct.feat->f(), mk.map->f(), win, sgrad, sc,
                                        b.name, partials, run.defer()));
    const double weight = tp.t->layer_weight * tp.t->content_weight;
    run.pl.terms.push_back(LossTerm{si, weight * 0.5});
    run.terms[k].push_back(Term{true, sgrad, sc + 1, (float)weight, ContentWindow{}});
    return STX_OK;
}

static int queue_content_terms(TileRun &run, size_t k) {
    stx_engine *e = run.e;
    const Tap &tp = run.plan.order[k];
    const Blob &b = e->blobs[tp.blob];
    bool any = false;
    const ContentMask *mk = e->sh->cmasks.empty() ? nullptr : content_mask_of(e, tp.blob);
    int slot = 0;
    if (mk) {
        int n_here = 0;
        for (const ContentTarget &ct : e->sh->contents) n_here += ct.blob == tp.blob;
        STX_TRY(e->sgrad_content[k]->ensure((size_t)n_here * b.count() * sizeof(float)));
    }
    for (const ContentTarget &ct : e->sh->contents) {
        if (ct.blob != tp.blob) continue;
        any = true;
        const ContentWindow win = content_window(b, ct.h, ct.w, run.c.start, run.c.rx, run.c.ry);
        if (win.oy + win.fh > win.ch || win.ox + win.fw > win.cw) {
            set_error("content window [%d+%d, %d+%d] exceeds the %dx%d map of layer %s",
                      win.oy, win.fh, win.ox, win.fw, win.ch, win.cw, b.name.c_str());
            return STX_ERR_ARG;
        }
        if (mk) {
            STX_TRY(queue_masked_content_term(run, k, ct, *mk, win,
                                              e->sgrad_content[k]->f() + (size_t)slot++ * b.count()));
            continue;
        }
        STX_TRY(queue_residual_term(run, k, "content ", ct.feat->f(), win, tp.t->layer_weight * tp.t->content_weight));
    }
    if (!any) {
        set_error("no content target for layer %s", b.name.c_str());
        return STX_ERR_STATE;
    }
    return STX_OK;
}

// The mask map of style `index` at `blob` (stx_set_style_masks), or null.
static const StyleMask *style_mask_of(const stx_engine *e, int index, int blob) {
    for (const StyleMask &m : e->sh->masks)
        if (m.index == index && m.blob == blob) return &m;
    return nullptr;
}

// The term of a masked style target of tap k: the tile's window of the mask map, taken as a content
// map's is, then launch_masked_style_terms.
static int queue_masked_style_term(TileRun &run, size_t k, const StyleTarget &st, const StyleMask &mk, float *sgrad) {
    stx_engine *e = run.e;
    const Tap &tp = run.plan.order[k];
    const Blob &b = e->blobs[tp.blob];
    const ContentWindow win = content_window(b, mk.h, mk.w, run.c.start, run.c.rx, run.c.ry);
    if (win.oy < 0 || win.ox < 0 || win.oy + win.fh > win.ch || win.ox + win.fw > win.cw) {
        set_error("style mask window [%d+%d, %d+%d] exceeds the %dx%d mask map of layer %s",
                  win.oy, win.fh, win.ox, win.fw, win.ch, win.cw, b.name.c_str());
        return STX_ERR_ARG;
    }
    size_t si;
    STX_TRY(alloc_scalars(e, 4, &si));
    float *sc = e->A().scalars.f() + si;   // [0] = sum tril(D)^2, [2] = sum |m . S|, [3] = a
    const unsigned *f_amax = b.amax_data >= 0 ? e->amax_slots(b.amax_data, false) : nullptr;
    float *scratch = nullptr;
    if (run.sums_late) {
        scratch = e->term_scratch.f() + run.scratch_used;
        run.scratch_used += style_term_scratch_floats(b.channels, b.h * b.w);
    }
    float *mask_scratch = e->term_scratch.f() + run.scratch_used;
    run.scratch_used += kMaskScratchFloats;
    STX_TRY(launch_masked_style_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, mk.map->f(), win,
                                      st.gram->f(), sgrad, sc, b.name, f_amax, scratch, mask_scratch, run.defer()));
    const double lw = tp.t->layer_weight;
    run.pl.terms.push_back(LossTerm{si, lw * tp.t->style_weight * 0.5 / e->sh->n_styles});
    run.terms[k].push_back(Term{true, sgrad, sc + 2, (float)(lw * tp.t->style_weight / e->sh->n_styles),
                                ContentWindow{}});
    return STX_OK;
}

// Gram -> G - Gs -> SYMM against every style target of tap k (launch_style_terms).
static int queue_style_terms(TileRun &run, size_t k) {
    stx_engine *e = run.e;
    const Tap &tp = run.plan.order[k];
    const Blob &b = e->blobs[tp.blob];
    const double lw = tp.t->layer_weight;
    int n_here = 0;
    for (const StyleTarget &st : e->sh->styles) n_here += st.blob == tp.blob;
    if (!n_here) {
        set_error("no style target for layer %s", b.name.c_str());
        return STX_ERR_STATE;
    }
    STX_TRY(e->sgrad_tap[k]->ensure((size_t)n_here * b.count() * sizeof(float)));
    int slot = 0;
    for (const StyleTarget &st : e->sh->styles) {
        if (st.blob != tp.blob) continue;
        const int C = b.channels, HW = b.h * b.w;
        if (C % 4 != 0) {
            set_error("style layer %s: channel count %d is not a multiple of 4", b.name.c_str(),
                      C);
            return STX_ERR_UNSUPPORTED;
        }
        float *sgrad = e->sgrad_tap[k]->f() + (size_t)slot++ * b.count();
        if (const StyleMask *mk = style_mask_of(e, st.index, tp.blob)) {
            STX_TRY(queue_masked_style_term(run, k, st, *mk, sgrad));
            continue;
        }
        size_t si;
        STX_TRY(alloc_scalars(e, 2, &si));
        float *sc = e->A().scalars.f() + si;   // [0] = sum tril(D)^2, [1] = sum |S|
        // (the maximum the blob's producer left, if it left one: the fp16-split kernels' scale)
        const unsigned *f_amax = b.amax_data >= 0 ? e->amax_slots(b.amax_data, false) : nullptr;
        float *scratch = nullptr;
        if (run.sums_late) {
            scratch = e->term_scratch.f() + run.scratch_used;
            run.scratch_used += style_term_scratch_floats(C, HW);
        }
        STX_TRY(launch_style_terms(e, e->stream, b.data.f(), C, b.h, b.w, st.gram->f(), sgrad, sc,
                                   b.name, f_amax, scratch, run.defer()));
        run.pl.terms.push_back(LossTerm{si, lw * tp.t->style_weight * 0.5 / e->sh->n_styles});
        run.terms[k].push_back(Term{true, sgrad, sc + 1,
                                    (float)(lw * tp.t->style_weight / e->sh->n_styles), ContentWindow{}});
    }
    return STX_OK;
}

// The mean / std term of tap k against the blob's statistics target (launch_stat_terms).
static int queue_stat_term(TileRun &run, size_t k, const StatTarget &st) {
    stx_engine *e = run.e;
    const Tap &tp = run.plan.order[k];
    const Blob &b = e->blobs[tp.blob];
    STX_TRY(e->sgrad_stat[k]->ensure(b.count() * sizeof(float)));
    float *sgrad = e->sgrad_stat[k]->f();
    size_t si;
    STX_TRY(alloc_scalars(e, 2, &si));
    float *sc = e->A().scalars.f() + si;   // [0] = E, [1] = sum |S|
    float *scratch = e->term_scratch.f() + run.scratch_used;
    run.scratch_used += stat_scratch_floats(b.channels, b.h * b.w);
    STX_TRY(launch_stat_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, st.ms->f(), st.ms->f() + st.C,
                              sgrad, sc, b.name, scratch, run.defer()));
    const double coef = tp.t->layer_weight * st.weight;
    run.pl.terms.push_back(LossTerm{si, coef * 0.5});
    run.terms[k].push_back(Term{true, sgrad, sc + 1, (float)coef, ContentWindow{}});
    return STX_OK;
}

// Deep-Dream term (style_transfer.py:602-604): the content term against a zero map with a negative
// weight -- loss -= lw*dd*1/2|F|^2, diff -= lw*dd*normalize(F)
static int queue_dream_term(TileRun &run, size_t k) {
    const Tap &tp = run.plan.order[k];
    return queue_residual_term(run, k, "dream ", nullptr, dream_window(run.e->blobs[tp.blob]),
                               -tp.t->layer_weight * tp.t->dd_weight);
}

// Loss terms of tap k (Gram -> G - Gs -> SYMM, content residual sums).  They are queued the
// moment the tapped blob is complete, in the middle of the forward pass, while the blob is
// still in the L2 / Infinity Cache the convolution just wrote it through (the shallow blobs
// were re-fetched from HBM when all taps ran after the forward pass: 1.1 GB per tile by PMC).
static int queue_tap_terms(TileRun &run, size_t k) {
    const stx_tap *t = run.plan.order[k].t;
    if (t->is_content) STX_TRY(queue_content_terms(run, k));
    if (t->is_style) STX_TRY(queue_style_terms(run, k));
    if (const StatTarget *st = stat_target_of(run.e, run.plan.order[k].blob)) STX_TRY(queue_stat_term(run, k, *st));
    if (t->is_dd) STX_TRY(queue_dream_term(run, k));
    return STX_OK;
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

// Adds the terms of tap k to its blob's diff with stand-alone kernels (used for the deepest
// tap, for blobs produced by a pooling backward, and when a tap has more than one content or
// style term; otherwise the terms ride in the epilogue of the convolution backward above).
static int inject_terms(TileRun &run, size_t k, bool &diff_written) {
    stx_engine *e = run.e;
    const int blob = run.plan.order[k].blob;
    const std::vector<Term> &terms = run.terms[k];
    Blob &b = e->blobs[blob];
    ProfScope scope(e, "inject " + b.name, 0.0);
    b.amax_diff = -1;
    for (size_t ti = 0; ti < terms.size(); ++ti) {       // content terms come first, like the reference
        const Term &t = terms[ti];
        // the last term's kernel writes the blob's final gradient: it leaves its maximum for the
        // fp16-split convolution that reads it next (the slots were zeroed when the walk began)
        unsigned *amax = nullptr;
        if (ti + 1 == terms.size() && conv_h2_enabled()) {
            amax = e->amax_slots(blob, true);
            b.amax_diff = blob;
        }
        if (t.style)
            STX_TRY(inject_style_launch(e->stream, b.diff.f(), t.src, b.count(), t.sums, t.coef,
                                        diff_written, amax));
        else
            STX_TRY(inject_content_launch(e->stream, b.diff.f(), b.data.f(), t.src, t.win,
                                          t.sums, t.coef, diff_written, amax));
        diff_written = true;
    }
    return STX_OK;
}

// Can the terms of tap k ride in the epilogue of the convolution backward that produces its blob's gradient?
static bool tap_fusable(const TileRun &run, size_t k) {
    int ns = 0, nc = 0;
    for (const Term &t : run.terms[k]) {
        if (!t.style && !t.src) return false;      // Deep-Dream terms take the stand-alone path
        (t.style ? ns : nc)++;
    }
    return ns <= 1 && nc <= 1;
}

// ... and what that epilogue needs of them (`bot`: the tapped blob).
static ConvInject make_inject(const TileRun &run, size_t k, const Blob &bot) {
    ConvInject inj{};
    for (const Term &t : run.terms[k]) {
        if (t.style) {
            inj.sgrad = t.src;
            inj.s_abs_sum = t.sums;
            inj.s_coef = t.coef;
        } else {
            inj.content = t.src;
            inj.c_sums = t.sums;
            inj.c_coef = t.coef;
            inj.win = t.win;
            inj.feat = bot.data.f();
        }
    }
    return inj;
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

// A style tap on the first layer's blob: that layer's kernel leaves its Gram partials.
static void first_gram_setup(stx_engine *e, const TilePlan &plan) {
    const int data_blob = e->layers[0].top_blob;
    e->first_gram_blob = -1;
    e->first_gram_valid = false;
    for (const Tap &tp : plan.order) {
        const int pl = e->blobs[tp.blob].producer;
        // (a masked style takes the Gram of F . m: the partials are for the unmasked targets of the blob)
        bool unmasked = e->sh->masks.empty();
        for (const StyleTarget &st : e->sh->styles)
            unmasked |= st.blob == tp.blob && !style_mask_of(e, st.index, tp.blob);
        if (tp.t->is_style && unmasked && pl > 0 && e->layers[pl].type == STX_LAYER_CONV &&
            e->layers[pl].bottom_blob == data_blob && e->blobs[tp.blob].channels == 64)
            e->first_gram_blob = tp.blob;
    }
}

// Enqueues the evaluation proper: forward pass with the loss terms of the tapped blobs, backward
// walk, the mirror copy of the loss scalars.  The tile is already in the input blob; the gradient
// is left in its diff.
static int sc_grad_run(stx_engine *e, const TileCall &c, const TilePlan &plan, PendingLoss &pl) {
    const std::vector<Tap> &order = plan.order;
    TileRun run{e, c, plan, pl, !(sw_env("STX_SUMS_LATE") && !atoi(sw_env("STX_SUMS_LATE"))),
                !(sw_env("STX_TERMS_LATE") && atoi(sw_env("STX_TERMS_LATE"))),
                std::vector<std::vector<Term>>(order.size()), {}, 0};
    while (e->sgrad_tap.size() < order.size()) e->sgrad_tap.emplace_back(new DevBuf);
    if (!e->sh->stats.empty())
        while (e->sgrad_stat.size() < order.size()) e->sgrad_stat.emplace_back(new DevBuf);
    if (!e->sh->cmasks.empty())
        while (e->sgrad_content.size() < order.size()) e->sgrad_content.emplace_back(new DevBuf);
    {
        size_t need = 0;
        for (const Tap &tp : order) {
            const Blob &b = e->blobs[tp.blob];
            // (a statistics term's partials and table live there, with or without the late sums)
            if (stat_target_of(e, tp.blob)) need += stat_scratch_floats(b.channels, b.h * b.w);
            // (and a masked content term's partials)
            if (tp.t->is_content && !e->sh->cmasks.empty() && content_mask_of(e, tp.blob))
                for (const ContentTarget &ct : e->sh->contents)
                    if (ct.blob == tp.blob) need += kContentMaskScratchFloats;
            if (!tp.t->is_style) continue;
            for (const StyleTarget &st : e->sh->styles) {
                if (st.blob != tp.blob) continue;
                if (run.sums_late) need += style_term_scratch_floats(b.channels, b.h * b.w);
                // (a masked term's partials live there too, with or without the late sums)
                if (style_mask_of(e, st.index, tp.blob)) need += kMaskScratchFloats;
            }
        }
        STX_TRY(e->term_scratch.ensure(need * sizeof(float)));
    }
    STX_TRY(begin_timing(e));
    std::vector<char> observed(e->blobs.size(), 0);
    for (const Tap &tp : order) observed[tp.blob] = 1;
    first_gram_setup(e, plan);
    STX_TRY(forward(e, plan.needed, order[0].blob, run.interleave ? &run : nullptr, true, observed));
    if (!run.interleave) {
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

static int sc_grad_eager(stx_engine *e, const TileCall &c, double *loss_out) {
    // the scalar arena holds the reductions of every call queued since the last stx_sync; drain
    // it (publishing the pending losses) before it could overflow
    {
        const size_t per_call = ((size_t)c.n_taps + e->sh->stats.size()) * 2100 *
                                (size_t)std::max(1, e->sh->n_contents + e->sh->n_styles);
        if (e->A().used + per_call > e->scalars_cap) STX_TRY(do_sync(e));
        if (per_call > e->scalars_cap) {
            set_error("stx_sc_grad_tile: %d taps need more scalar space than the arena holds", c.n_taps);
            return STX_ERR_NOMEM;
        }
    }
    TilePlan plan;
    STX_TRY(sc_grad_prepare(e, c, plan));
    Blob &in = e->blobs[e->layers[0].top_blob];
    // (a tile handed over in the engine's own buffers, stx_tile_buffers, needs no copies)
    if (c.img != in.data.ptr) STX_TRY(copy_in(e, in.data.ptr, c.img, c.img_mem, in.count() * sizeof(float)));
    PendingLoss pl;
    pl.out = loss_out;
    STX_TRY(sc_grad_run(e, c, plan, pl));
    if (c.grad_out != in.diff.ptr)
        STX_TRY(copy_out(e, c.grad_out, c.grad_mem, in.diff.ptr, in.count() * sizeof(float)));
    e->A().pending.push_back(std::move(pl));
    ++e->n_tile_evals;
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

}  // extern "C"
