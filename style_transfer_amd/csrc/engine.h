// The engine's state and the few helpers that more than one host file uses.  Internal: not installed.
//   engine.cpp     engine life cycle, weights, scalar arenas and fences, profiling readers
//   targets.cpp    stx_set_*: the group's targets (contents, styles, masks, statistics, banks) and their swap
//   tile_path.cpp  the tile evaluation: shaping, forward pass, backward walk
//   tile_terms.cpp the loss terms of a tile evaluation: their plan, their launches, their injection
//   image_api.cpp  whole-image and vector entries, the SWT regulariser's tables, the Laplacian loss
//   op_hooks.cpp   stx_op_*: single operators for the tests
#pragma once

#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"

namespace stx {

// Growable device buffer.  Growth frees and reallocates (hipFree synchronises the device, so
// kernels still reading the old allocation have finished); it happens only when a larger tile
// than ever before arrives.
struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return STX_OK;
        if (ptr) STX_HIP(hipFree(ptr));
        ptr = nullptr;
        bytes = 0;
        const size_t want = (need + 255) & ~(size_t)255;
        hipError_t err = hipMalloc(&ptr, want);
        if (err != hipSuccess) {
            set_error("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(err));
            ptr = nullptr;
            return STX_ERR_NOMEM;
        }
        bytes = want;
        return STX_OK;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    float *f() const { return static_cast<float *>(ptr); }
};

struct Layer {
    std::string name, bottom, top;
    int type = 0, num_output = 0, ksize = 0, pad = 0, stride = 1, pool_mode = 0;
    int bottom_blob = -1, top_blob = -1;
};

struct Blob {
    std::string name;
    int channels = 0;
    int producer = -1;   // layer index that writes it (conv / pool / input)
    bool relu = false;   // an in-place ReLU layer follows the producer
    int scale = 1;       // 224 // height at a 224 input (CaffeModel.layer_info, style_transfer.py:415-419)
    int h = 0, w = 0;    // current tile
    DevBuf data, diff;
    DevBuf codes;             // pooled blobs: one window code per element (pool.hip), written by the
    bool codes_valid = false; // forward pass that produced `data` if its kernel can
    DevBuf relu_codes;        // rectified blobs: sign nibbles per 2x2 window (ConvProblem::out_codes / in_codes),
    bool relu_codes_valid = false;   // written by the convolution that produces the blob, or by the one that reads it
    bool relu_codes_wanted = false;  // ... or would have been, had its kernel taken them (ConvProblem::wants_codes)
    // max |data| / max |diff| (or an upper bound of it) on the device, for the fp16-split convolution
    // that reads the blob (conv_h2.hip): the slot group (a blob index) of the engine's table that
    // holds it -- the blob's own when its producer tracked it, the blob's below / above when a
    // pooling layer passed the bound on -- or -1 when nobody has left one in this pass
    int amax_data = -1, amax_diff = -1;
    size_t count() const { return (size_t)channels * h * w; }
};

struct ConvParams {
    int cin = 0, cout = 0, ks = 0;
    DevBuf w, b;                              // Caffe layout on the device
    bool set = false;
    std::map<int, std::unique_ptr<DevBuf>> packed;  // key: ConvBank::key
};

struct ContentTarget {
    int index, blob, C, h, w;
    std::unique_ptr<DevBuf> feat;
    void release() { feat->release(); }
};

struct StyleTarget {
    int index, blob, C;
    std::unique_ptr<DevBuf> gram;
    void release() { gram->release(); }
};

// The mask of style `index` at one tapped blob (stx_set_style_masks): the block means of the
// image-resolution mask at the blob's scale, [h][w], addressed like a content map.
struct StyleMask {
    int index, blob, h, w;
    std::unique_ptr<DevBuf> map;
    void release() { map->release(); }
};

// The content mask at one blob that has a content target (stx_set_content_mask): the block means of the
// image-resolution mask at the blob's scale, [h][w] -- the size of the blob's content maps.
struct ContentMask {
    int blob, h, w;
    std::unique_ptr<DevBuf> map;
    void release() { map->release(); }
};

// The mean / std targets of one tapped blob (stx_set_stat_targets): MU [C] then SD [C] on the device.
struct StatTarget {
    int blob, C;
    double weight;
    std::unique_ptr<DevBuf> ms;
    void release() { ms->release(); }
};

// The bank of one tapped blob's nearest-neighbour term (stx_set_nnfm_targets): float32 rows [rows][C] on the
// device and, built once when the targets are set, their fp16 hi / lo pieces for the search (nnfm.hip).
// patch 3 (stx_set_nnfm_patch_targets): rows of 3 x 3 patches, 9 C channels each.  k (stx_set_nnfm_knn_targets):
// the rows a query is matched to, 1 .. kNnfmMaxK; the bank does not depend on it.  cover
// (stx_set_nnfm_cover_targets): the factor of the coverage part, 0: none (patch 1 only).
struct NnfmTarget {
    int blob, C, rows;
    double weight;
    std::unique_ptr<DevBuf> bank, pieces;
    int patch = 1, k = 1;
    float cover = 0.f;
    // guided (stx_set_nnfm_guided_targets; segs.count > 0): the bank's segments and the block means of every
    // segment's image-resolution mask at the blob's scale, maps [segments][mh][mw], addressed like a content map
    NnfmSegments segs{};
    int mh = 0, mw = 0;
    std::unique_ptr<DevBuf> maps;
    // [rows][patch^2 C] hi, then as many lo
    const unsigned short *pieces_hi_lo() const { return static_cast<const unsigned short *>(pieces->ptr); }
    void release() {
        bank->release();
        pieces->release();
        if (maps) maps->release();
    }
};

// The sliced Wasserstein target of one tapped blob (stx_set_swd_targets): V [D][C] then Tq [D][Q] on the device.
struct SwdTarget {
    int blob, C, D, Q;
    double weight;
    std::unique_ptr<DevBuf> vt;
    const float *V() const { return vt->f(); }
    const float *Tq() const { return vt->f() + (size_t)D * C; }
    void release() { vt->release(); }
};

// The self-similarity target of one tapped blob (stx_set_selfsim_targets): it reads the layer's content map of
// content_index 0 and carries no data of its own.
struct SelfsimTarget {
    int blob, points;
    double weight;
    void release() {}
};

// The shifted-Gram targets of one tapped blob (stx_set_shift_targets): the offsets and T [n][C][C] on the device.
struct ShiftTarget {
    int blob, C;
    ShiftOffsets off;
    double weight;
    std::unique_ptr<DevBuf> grams;
    void release() { grams->release(); }
};

// The contextual target of one tapped blob (stx_set_cx_targets): the bank's centred unit rows [rows][C], then the
// mean mu [C] of the raw rows, on the device.
struct CxTarget {
    int blob, C, rows, points;
    float eta;
    double weight;
    std::unique_ptr<DevBuf> data;
    const float *bank() const { return data->f(); }
    const float *mu() const { return data->f() + (size_t)rows * C; }
    void release() { data->release(); }
};

struct LossTerm {
    size_t scalar_index;   // float in the host mirror of the scalar buffer
    double coef;
};

struct PendingLoss {
    double *out;
    std::vector<LossTerm> terms;       // sum coef * scalar
    std::vector<LossTerm> dterms;      // sum coef * double scalar (image ops)
};

// What the engines of one GPU have in common: the network's weights, the banks packed for the
// kernels and the current targets.  A farm runs several engines (HIP streams + activation
// buffers) per GPU; each holding its own copy cost 4 x (80 MB of weights + ~200 MB of packed
// banks + the per-scale content maps: 537 MB at 4096^2) per GPU and as many uploads over xGMI.
struct SharedState {
    std::map<int, ConvParams> conv;    // layer index -> params
    std::vector<ContentTarget> contents;
    std::vector<StyleTarget> styles;
    std::vector<StyleMask> masks;      // (cleared with the targets)
    std::vector<StatTarget> stats;     // (cleared with the targets)
    std::vector<ContentMask> cmasks;   // (cleared with the targets)
    std::vector<NnfmTarget> nnfms;     // (cleared with the targets)
    std::vector<SwdTarget> swds;       // (cleared with the targets)
    std::vector<SelfsimTarget> selfsims;   // (cleared with the targets)
    std::vector<ShiftTarget> shifts;   // (cleared with the targets)
    std::vector<CxTarget> cxs;         // (cleared with the targets)
    int n_contents = 0, n_styles = 0;
    std::vector<stx_engine *> members;
    std::mutex mutex;                  // packs and target swaps (members may be driven by different threads)
    size_t target_uploads = 0;         // stx_set_contents_and_styles calls that copied data
    double target_bytes = 0;           // bytes those calls copied (cumulative)
};

}  // namespace stx

using namespace stx;   // (an internal header: every file that includes it is the library's own host code)

struct stx_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    bool clock_marks = false;              // stx_clock_marks: one mark per 2-D Winograd launch
    DevBuf marks_buf;
    int marks_used = 0, last_mark = -1;    // (last_mark: the slot of the launch just queued, or -1)
    std::vector<std::unique_ptr<DevBuf>> sgrad;       // per tap: the gradient blobs S of its terms (PlannedTerm::sgrad_off)
    // start / stop of the last few tile calls (a ring: stx_last_tile_ms reports the newest call
    // that has finished, so a host that runs ahead does not wait for the call it just queued)
    static constexpr int kTimed = 4;
    hipEvent_t ev_start[kTimed] = {}, ev_stop[kTimed] = {};
    int ev_cur = 0;
    int ev_recorded = 0;               // ring slots that hold a recorded pair (at most kTimed)
    hipEvent_t ev_tune0 = nullptr, ev_tune1 = nullptr;
    bool timed = false;
    double flop_algorithmic = 0, flop_issued = 0;   // matrix work of the current / last tile call
    std::vector<Layer> layers;
    std::vector<Blob> blobs;
    std::map<std::string, int> blob_index, layer_index;
    std::shared_ptr<SharedState> sh;   // weights, packed banks, targets (shared per GPU)

    DevBuf splitk;                     // split-K partial sums of small-plane convolutions
    DevBuf amax;                       // [data | diff][blob][kAmaxSlots] words of float bits (Blob::amax_data)
    unsigned *amax_slots(int blob, bool diff) const {
        return static_cast<unsigned *>(amax.ptr) + ((size_t)(diff ? blobs.size() : 0) + blob) * kAmaxSlots;
    }
    int amax_ensure() {     // (+ 2: the scratch groups behind the blobs' own, see amax_scratch)
        return amax.ensure((2 * blobs.size() + 2) * kAmaxSlots * sizeof(unsigned));
    }
    // the first layer leaves the Gram partials of its own output when that blob is a style tap of
    // the call (conv_first.hip): which blob, whether this call's forward pass wrote them, how many
    DevBuf first_gram;
    int first_gram_blob = -1, first_gram_parts = 0;
    bool first_gram_valid = false;
    DevBuf gram_partials, gram, dsym, dsym_pieces, symm_partials, upload;
    DevBuf term_scratch;               // per term of a tile call: what its launches leave for the sum jobs (TilePlan)
    DevBuf masked_feat, masked_target; // a masked style term's F . m and a Gs (style_mask.hip), one term at a time
    DevBuf stat_scratch;               // stx_feature_stats / stx_op_stat_terms: partials, table, outputs
    DevBuf nnfm_scratch;               // stx_nnfm_bank / stx_op_nnfm_terms: rows, bank pieces, the term's scratch
    DevBuf swd_work;                   // a sliced Wasserstein term's sort records and G (swd_work_floats), one term at a time
    DevBuf swd_io;                     // stx_swd_target / stx_op_swd_terms: V, the quantiles, the term's scratch
    DevBuf selfsim_io;                 // stx_op_selfsim_terms: the term's scratch
    DevBuf shift_io;                   // stx_shift_gram / stx_op_shift_terms: the term's scratch, X
    DevBuf cx_io;                      // stx_cx_rows / stx_cx_bank / stx_op_cx_terms: staged rows, the term's scratch
    // Loss scalars of the calls queued so far: device floats (tile terms) and doubles (image-op
    // reductions), each with a pinned host mirror, and the losses that will be published from
    // them.  TWO arenas: stx_fence closes the current one behind an event and opens the other, so
    // that a step loop can queue iteration i + 1 before it waits (stx_fence_wait) for the
    // scalars of iteration i -- the host runs one iteration ahead of the GPU instead of letting
    // it idle while the statistics of a step travel home.
    struct ScalarArena {
        DevBuf scalars;                    // device floats
        float *host = nullptr;             // pinned mirror
        size_t used = 0;
        DevBuf dscalars;                   // device doubles (image-op reductions)
        double *dhost = nullptr;
        size_t dused = 0;
        std::vector<PendingLoss> pending;
        hipEvent_t fence = nullptr;
        unsigned long long ticket = 0;     // 0: open; else closed by stx_fence and not yet published
    };
    ScalarArena arena[2];
    int cur = 0;
    unsigned long long next_ticket = 1;
    ScalarArena &A() { return arena[cur]; }
    size_t scalars_cap = 0;
    size_t n_tile_evals = 0;               // stx_sc_grad_tile calls (STX_Q_TILE_EVALS)
    size_t n_tile_io_direct = 0;           // ... and their ends that needed no copy (STX_Q_TILE_IO_DIRECT)
    size_t n_inject_specialised = 0;       // launches of conv_h2's specialised injecting bodies (STX_Q_INJECT_SPECIALISED)
    unsigned inject_variants = 0;          // ... and which: bit h2_variant (STX_Q_INJECT_VARIANTS)
    std::vector<hipEvent_t> fence_events;     // stx_engine_wait: ring of events recorded on this stream
    size_t fence_next = 0;
    size_t dscalars_cap = 64;
    DevBuf red_scratch;                // float partials for image-op reductions
    DevBuf color_sums;                 // stx_image_color_stats: its nine sums (made at first use)
    DevBuf swt_scratch;                // stx_image_swt_haar_levels: row-filtered image + its partials
    struct SwtTable {                  // stx_image_swt_daub_levels: the taps of one (order, levels, N)
        int order, levels, N, ntaps, hl;
        DevBuf taps;
    };
    std::vector<SwtTable> swt_tables;  // built at first use, kept: a step uploads nothing
    DevBuf lap_scratch;                // stx_image_lap / _target: pooled maps, cell values, partials
    DevBuf flow_work;                  // stx_image_flow_estimate: pyramid and planes; released at the next sync
    DevBuf poisson_work;               // stx_image_poisson: e and b of every level; released at the next sync

    bool winograd = true;   // 1-D Winograd F(2,3) for the 3x3 layers (STX_WINOGRAD=0: direct only)
    bool autotune = true;   // tile-config autotuning (process-wide cache, see conv_choose)
    bool pool_codes = true; // forward pooling leaves window codes for the backward pass (STX_POOL_CODES=0: off)

    // optional per-kernel-group timing (stx_profile_enable): event pairs around launch groups
    bool profiling = false;
    struct ProfEntry {
        std::string label;
        double flops;
        hipEvent_t start, stop;
        int mark = -1;      // clock mark of the group's convolution launch (stx_clock_marks), or -1
    };
    std::vector<ProfEntry> prof;
    std::vector<hipEvent_t> event_pool;

    // optional audit of the maxima handed from kernel to kernel (stx_amax_audit): per hand-off the recorded
    // slots and a measured maximum, kAmaxSlots words each, in audit_buf
    bool amax_audit = false;
    struct AuditEntry {
        std::string consumer, blob, source;
        bool diff;
    };
    std::vector<AuditEntry> audit;
    DevBuf audit_buf;

    int set_device() {
        STX_HIP(hipSetDevice(device));
        return STX_OK;
    }
    int find_blob(const char *name) const {
        if (!name) return -1;
        auto it = blob_index.find(name);
        return it == blob_index.end() ? -1 : it->second;
    }
};

namespace stx {
#pragma GCC visibility push(hidden)     // what follows is internal to the library: not exported

// RAII timing of one launch group when profiling is on (no-op otherwise).
struct ProfScope {
    stx_engine *e;
    int index = -1;
    hipStream_t stream;
    ProfScope(stx_engine *eng, const std::string &label, double flops, hipStream_t on = nullptr)
        : e(eng), stream(on ? on : eng->stream) {
        if (!e->profiling) return;
        auto take = [&]() {
            hipEvent_t ev = nullptr;
            if (!e->event_pool.empty()) {
                ev = e->event_pool.back();
                e->event_pool.pop_back();
            } else if (hipEventCreate(&ev) != hipSuccess) {
                ev = nullptr;
            }
            return ev;
        };
        stx_engine::ProfEntry pe{label, flops, take(), take()};
        if (!pe.start || !pe.stop) return;
        (void)hipEventRecord(pe.start, stream);
        e->prof.push_back(pe);
        index = (int)e->prof.size() - 1;
    }
    ~ProfScope() {
        if (index < 0) return;
        (void)hipEventRecord(e->prof[index].stop, stream);
        e->prof[index].mark = e->last_mark;
        e->last_mark = -1;
    }
};

constexpr int kMaxClockMarks = 16384;   // stx_clock_marks: launches that can leave a mark between two reads

// ---- helpers that more than one host file uses
// engine.cpp
int alloc_scalars(stx_engine *e, size_t n, size_t *index);
int alloc_dscalars(stx_engine *e, size_t n, size_t *index);
int copy_in(stx_engine *e, void *dst, const void *src, int mem, size_t bytes);
int copy_out(stx_engine *e, void *dst, int mem, const void *src, size_t bytes);
int do_sync(stx_engine *e);
int quiesce_members(stx_engine *e);
// Frees the device memory of every target of one kind and forgets them: the one place that releases targets.
// (The caller has made sure that no queued kernel still reads them: quiesce_members.)
template <class T>
inline void clear_targets(std::vector<T> &targets) {
    for (T &t : targets) t.release();
    targets.clear();
}
// THE list of the per-layer kinds: the targets that hang on one layer each and make it part of every evaluation,
// in planning order (plan_terms).  `visit` sees every kind's vector; whoever must know the kinds goes through here.
template <class State, class Visit>
inline void for_each_layer_kind(State &sh, Visit visit) {
    visit(sh.stats);
    visit(sh.nnfms);
    visit(sh.swds);
    visit(sh.selfsims);
    visit(sh.shifts);
    visit(sh.cxs);
}
// The element of `targets` that hangs on `blob`, or null.
template <class T>
inline const T *target_at(const std::vector<T> &targets, int blob) {
    for (const T &t : targets)
        if (t.blob == blob) return &t;
    return nullptr;
}
inline void clear_dependent_targets(SharedState &sh) {   // what is set behind the contents and styles, and goes with them
    clear_targets(sh.masks);
    clear_targets(sh.cmasks);
    for_each_layer_kind(sh, [](auto &targets) { clear_targets(targets); });
}
inline void clear_all_targets(SharedState &sh) {
    clear_targets(sh.contents);
    clear_targets(sh.styles);
    sh.n_contents = sh.n_styles = 0;
    clear_dependent_targets(sh);
}
// tile_path.cpp
ConvProblem conv_fwd_problem(const float *x, float *y, const float *bias, int Cin, int Cout, int H, int W,
                             int ks, int relu);
ConvProblem conv_bwd_problem(const float *dy, float *dx, const float *mask, int Cout, int Cin, int H, int W,
                             int ks);
int attach_splitk(stx_engine *e, const ConvConfig &cfg, ConvProblem &p);
int launch_conv(stx_engine *e, const ConvConfig &cfg, const ConvProblem &problem);
int amax_scratch(stx_engine *e, unsigned **out);
constexpr size_t kMaxAmaxAudit = 2048;   // stx_amax_audit: hand-offs kept between two reads
// With the audit on: records that `consumer` is about to read the n floats at x scaled by `slots` (a group of
// the engine's table) -- a copy of the slots and a measured max |x| into the audit's storage, on `stream`.
int amax_audit_note(stx_engine *e, hipStream_t stream, const std::string &consumer, const std::string &blob,
                    bool diff, const unsigned *slots, const float *x, size_t n);
// ---- tile_terms.cpp: the loss terms of one tile evaluation
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

enum class TermKind { Content, MaskedContent, Style, MaskedStyle, Stat, Nnfm, NnfmGuided, Swd, Selfsim, Shift, Cx, Dream };
constexpr size_t kNoSlot = ~(size_t)0;
constexpr size_t kResidualScalars = 2 + 2 * 1024;   // content_sums_launch: two sums and their partials

// One loss term of a call, planned before the first launch (plan_terms).
struct PlannedTerm {
    TermKind kind;
    int tap;                         // index into TilePlan::order
    const float *target, *mask;      // content map / Gram / MU then SD / null (dream); the mask map or null
    ContentWindow win;               // the tile's window of the content or mask map (with the map's size)
    double coef;                     // of the gradient term; the loss term takes half of it
    size_t scalars;                  // floats of the scalar arena
    size_t scratch_off, scratch_len; // its region of the engine's term_scratch, in floats
    size_t sgrad_off;                // its blob S in the tap's gradient buffer (stx_engine::sgrad), in floats, or kNoSlot
    const NnfmTarget *nnfm = nullptr; // TermKind::Nnfm: the bank with its pieces
    const SwdTarget *swd = nullptr;   // TermKind::Swd: the directions and quantiles
    int points = 0;                   // TermKind::Selfsim: the most grid positions (target = the content map, win its window)
    const ShiftTarget *shift = nullptr;   // TermKind::Shift: the offsets (target = T)
    const CxTarget *cx = nullptr;     // TermKind::Cx: the bank with mu, the points and the bandwidth
};

struct TilePlan {
    std::vector<Tap> order;         // taps, deepest first
    std::vector<char> needed;       // blobs on the path
    std::vector<int> tap_of;        // blob -> index into order, or -1
    std::deque<stx_tap> extra;      // taps of the layers that only a per-layer target (for_each_layer_kind) names (lw = 1);
                                    // `order` points into it: a deque's elements stay where they are
    // The final sums of the loss terms are collected and run as ONE launch behind the forward pass
    // (STX_SUMS_LATE=0: each where it arises, as rounds 1-4 did); what they add up must outlive the term's
    // own launches: its region of term_scratch.
    bool sums_late;
    bool interleave;                // (STX_TERMS_LATE=1: all loss terms after the forward pass, for A/B measurements)
    // The terms in queueing order -- shallowest tap first; per tap the content targets in sh->contents order,
    // the style targets in sh->styles order, the per-layer kinds' terms in for_each_layer_kind's order, Deep-Dream -- which is the order of
    // PendingLoss::terms: the host adds the loss up in it.
    std::vector<PlannedTerm> terms;
    std::vector<size_t> first_term;     // per tap: its first record
    std::vector<size_t> sgrad_floats;   // per tap: the size of its gradient buffer
    size_t scratch_floats = 0, scalars = 0;     // what the call takes of term_scratch and of the scalar arena
};

// One loss term of a tapped blob, as the backward walk adds it to the blob's gradient.
struct Term {
    enum Kind { Gradient, Residual } kind;
    const float *src;        // Gradient: a ready blob S;  Residual: the map F is held against (null: Deep-Dream)
    const float *sums;       // Gradient: &sum|S|;  Residual: {sum d^2, sum |d|}
    float coef;
    ContentWindow win;
};

// One evaluation (sc_grad_run): what its steps share.
struct TileRun {
    stx_engine *e;
    const TilePlan &plan;
    PendingLoss &pl;
    std::vector<std::vector<Term>> terms;     // per tap, in plan.order
    std::vector<SumJob> sum_jobs;
    std::vector<SumJob> *defer() { return plan.sums_late ? &sum_jobs : nullptr; }
};

// Validates the targets of the taps (shaped blobs) and lists the terms with what each takes.
int plan_terms(stx_engine *e, const TileCall &c, TilePlan &plan);
// Loss terms of tap k: launches them and records them for the backward walk and the host's sum.
int queue_tap_terms(TileRun &run, size_t k);
int inject_terms(TileRun &run, size_t k, bool &diff_written);
bool tap_fusable(const TileRun &run, size_t k);
ConvInject make_inject(const TileRun &run, size_t k, const Blob &bot);
int launch_style_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w,
                       const float *target, float *sgrad, float *sc, const std::string &name,
                       const unsigned *f_amax = nullptr, float *term_scratch = nullptr,
                       std::vector<SumJob> *defer = nullptr);
// The same term through a mask (style_mask.hip): F . m and a Gs, launch_style_terms on them, S <- a m . S.
// sc[4] = {sum tril(D)^2, (sum |S| before the mask), sum |m . S|, a}; mask_scratch: kMaskScratchFloats floats
// that outlive the call like term_scratch.
constexpr size_t kMaskScratchFloats = kMaskParts + kMaskSgradParts;
int launch_masked_style_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w,
                              const float *mask_map, const ContentWindow &win, const float *target,
                              float *sgrad, float *sc, const std::string &name, const unsigned *f_amax,
                              float *term_scratch, float *mask_scratch, std::vector<SumJob> *defer);
// The mean / std term of a blob (stat.hip): partials -> finish against MU, SD -> S into sgrad.
// sc[2] = {E, sum |S|}; the final sum of sum |S| joins `defer` or is launched here.  stat_scratch:
// stat_scratch_floats(C, h * w) floats that outlive the call like term_scratch.
int launch_stat_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w, const float *MU,
                      const float *SD, float *sgrad, float *sc, const std::string &name, float *stat_scratch,
                      std::vector<SumJob> *defer);
// The nearest-neighbour term of a blob (nnfm.hip): prepare -> search (-> merge) -> S into sgrad.
// sc[2] = {E, sum |S|}, both from partials whose final sums join `defer` or are launched here.  scratch:
// nnfm_scratch_floats(C, h * w, rows, patch, k) floats that outlive the call like term_scratch.  idx_out (or null):
// the winning rows [k][h * w].  patch 1, or 3: the 3 x 3 patch form, bank rows of 9 C channels.  pieces: the bank's
// fp16 pieces, [rows][patch^2 C] hi then lo (nnfm_split_rows_launch).  k: the rows per query, 1 .. kNnfmMaxK.
// cover != 0 (patch 1 only; the scratch sized with it): E and S gain cover times the coverage part; winner_out (or
// null): every bank row's best column [rows]; e_cov_out (or null): E_cov alone, summed here.
int launch_nnfm_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w, int patch,
                      const float *bank, const unsigned short *pieces, int rows, float *sgrad, int *idx_out, float *sc,
                      const std::string &name, float *scratch, std::vector<SumJob> *defer, int k = 1, float cover = 0.f,
                      int *winner_out = nullptr, float *e_cov_out = nullptr);
// The guided nearest-neighbour term of a blob (nnfm.hip): prepare -> mask windows and a -> search per segment
// (-> merge) -> S into sgrad.  sc[3] = {E, sum |S|, a}; a is final behind the window pass, the two others come from
// partials whose final sums join `defer` or are launched here.  scratch: nnfm_guided_scratch_floats(C, h * w, segs, k)
// floats that outlive the call like term_scratch.  maps [segments][win.ch][win.cw] and `win` the tile's window of
// them.  idx_out (or null): the lists [segments][k][h * w].  scale_by_a: sgrad = a S (the tile path), else S itself.
int launch_nnfm_guided_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w,
                             const float *bank, const unsigned short *pieces, const NnfmSegments &segs,
                             const float *maps, const ContentWindow &win, float *sgrad, int *idx_out, float *sc,
                             const std::string &name, float *scratch, std::vector<SumJob> *defer, int k,
                             bool scale_by_a);
// The sliced Wasserstein term of a blob (swd.hip): projection -> sort with the rank pass -> S = V^T G / D into sgrad.
// sc[2] = {E, sum |S|}, both from partials whose final sums join `defer` or are launched here.  scratch:
// swd_scratch_floats(C, h * w, D) floats that outlive the call like term_scratch; the records and G live in the
// engine's swd_work, which the next term may reuse.  rank_out (or null): r_d(i) [D][h * w].
int launch_swd_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w, const float *V, int D,
                     const float *Tq, int Q, float *sgrad, int *rank_out, float *sc, const std::string &name,
                     float *scratch, std::vector<SumJob> *defer);
// The self-similarity content term of a blob (selfsim.hip): prepare -> distances -> column pass -> gradient into sgrad.
// feat is the blob [C][h][w], content the other side (a plain array or a content map's window).  sc[2] = {E, sum |S|},
// both from partials whose final sums join `defer` or are launched here.  scratch: selfsim_scratch_floats(C, N)
// floats that outlive the call like term_scratch.  signs_out (or null): T int8 [N][N].
int launch_selfsim_terms(stx_engine *e, hipStream_t stream, const float *feat, const SelfsimSource &content, int C,
                         int h, int w, int points, float *sgrad, signed char *signs_out, float *sc,
                         const std::string &name, float *scratch, std::vector<SumJob> *defer);
// The shifted-Gram term of a blob (shiftgram.hip): cross-Gram partials -> merge against the targets -> S into sgrad.
// sc[2] = {E, sum |S|}, both from partials whose final sums join `defer` or are launched here.  scratch:
// shift_scratch_floats(C, h * w, off.n) floats that outlive the call like term_scratch.  targets [off.n][C][C].
int launch_shift_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w,
                       const ShiftOffsets &off, const float *targets, float *sgrad, float *sc, const std::string &name,
                       float *scratch, std::vector<SumJob> *defer);
// The contextual term of a blob (cx.hip): prepare -> scores -> row pass -> column pass -> gradient into sgrad.
// sc[2] = {E, sum |S|}: E enters the loss whole (LossTerm: the full coefficient), sum |S| from partials; both final
// sums join `defer` or are launched here.  scratch: cx_scratch_floats(C, N, rows) floats that outlive the call like
// term_scratch.  kbest_out [N], winner_out [rows] (device, or null): the decisions k*, i*.
int launch_cx_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w, int points,
                    const float *bank, const float *mu, int rows, float eta, float *sgrad, int *kbest_out,
                    int *winner_out, float *sc, const std::string &name, float *scratch, std::vector<SumJob> *defer);
// A content term through a weight map (content_mask.hip): a from the window of the map, then S = a (m d) into
// sgrad.  sc[3] = {sum m d^2, sum |m d|, a}; the two final sums join `defer` or are launched here.  partials:
// kContentMaskScratchFloats floats that outlive the call like term_scratch.
constexpr size_t kContentMaskScratchFloats = 2 * kContentMaskParts;
int launch_masked_content_terms(stx_engine *e, hipStream_t stream, const float *feat, const float *content,
                                const float *mask_map, const ContentWindow &win, float *sgrad, float *sc,
                                const std::string &name, float *partials, std::vector<SumJob> *defer);
#pragma GCC visibility pop

}  // namespace stx
