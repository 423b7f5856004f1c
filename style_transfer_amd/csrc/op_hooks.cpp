// libstx host side: the stx_op_* test hooks -- single operators of the tile path, launched the way the
// tile path launches them, on caller-owned device arrays.

#include <cmath>

#include "engine.h"

extern "C" {

// Packs `bank` from the Caffe-layout weights w into the upload buffer.
static int scratch_pack(stx_engine *e, const ConvBank &bank, const float *w, const float **packed) {
    STX_TRY(e->upload.ensure(bank.floats * sizeof(float)));
    STX_TRY(bank.pack(e->stream, w, e->upload.f()));
    *packed = e->upload.f();
    return STX_OK;
}

// A stand-alone operator call: the tile path's choice without the tuner; the input's maximum (where the kernel
// reads it) comes from a pass over it, the output's goes to a scratch group of the table.
static int hook_conv(stx_engine *e, ConvProblem &p, const float *w, int Mo, int Ko, int dir) {
    ConvConfig cfg;
    STX_TRY(conv_choose(p, e->winograd, nullptr, &cfg));
    if (conv_reads_x_amax(cfg)) {
        unsigned *scratch;
        STX_TRY(amax_scratch(e, &scratch));
        STX_TRY(absmax_launch(e->stream, p.x, (size_t)p.K * p.H * p.W, scratch));
        STX_HIP(hipMemsetAsync(scratch + kAmaxSlots, 0, kAmaxSlots * sizeof(unsigned), e->stream));
        p.x_amax = scratch;
        p.y_amax = scratch + kAmaxSlots;
    }
    STX_TRY(scratch_pack(e, conv_bank(cfg, dir, Mo, Ko, p.ksize), w, &p.w));
    STX_TRY(attach_splitk(e, cfg, p));
    return launch_conv(e, cfg, p);
}

int stx_op_conv_forward(stx_engine *e, const float *x, int Cin, int H, int W, const float *w,
                        const float *b, int Cout, int ksize, int relu, float *y) {
    if (!e || !x || !w || !y) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    if (conv_first_usable(Cin, Cout, ksize))      // the tile path's first-layer kernel
        return conv_first_launch(e->stream, x, w, b, y, Cin, H, W, relu, nullptr);
    ConvProblem p = conv_fwd_problem(x, y, b, Cin, Cout, H, W, ksize, relu);
    return hook_conv(e, p, w, Cout, Cin, 0);
}

int stx_op_conv_backward_data(stx_engine *e, const float *dy, int Cout, int H, int W, const float *w,
                              int Cin, int ksize, const float *relu_mask_data, float *dx) {
    if (!e || !dy || !w || !dx) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    if (ksize == 3 && Cin <= 4) {
        const float *packed = nullptr;
        STX_TRY(scratch_pack(e, conv_small_bank(Cout, Cin), w, &packed));
        return conv_small_launch(e->stream, dy, packed, dx, relu_mask_data, Cout, Cin, H, W);
    }
    ConvProblem p = conv_bwd_problem(dy, dx, relu_mask_data, Cout, Cin, H, W, ksize);
    return hook_conv(e, p, w, Cout, Cin, 1);
}

int stx_op_pool_forward(stx_engine *e, const float *x, int C, int H, int W, int mode, float *y) {
    if (!e || !x || !y) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return pool_forward_launch(e->stream, x, C, H, W, mode, y);
}

int stx_op_pool_backward(stx_engine *e, const float *dy, const float *x, int C, int H, int W,
                         int mode, const float *relu_mask_data, float *dx) {
    if (!e || !dy || !x || !dx) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    // the mask source is the pool input itself (post-ReLU data of the blob below)
    return pool_backward_launch(e->stream, dy, x, C, H, W, mode, relu_mask_data != nullptr, dx);
}

// The window of an h x w tile at (oy, ox) of a map_h x map_w map behind a roll: the caller gives all of them in
// the map's own pixels, so nothing is divided by a scale.
static ContentWindow hook_window(int C, int h, int w, int map_h, int map_w, int oy, int ox, const int roll_xy[2]) {
    ContentWindow win;
    win.C = C;
    win.fh = h;
    win.fw = w;
    win.ch = map_h;
    win.cw = map_w;
    win.oy = oy;
    win.ox = ox;
    win.sx = roll_xy ? roll_xy[0] : 0;
    win.sy = roll_xy ? roll_xy[1] : 0;
    return win;
}

// The scalars of one term hook: take() drains the arena and hands out n device floats of it, fetch() mirrors
// them, waits and hands out their host copies; the arena is empty again when the hook returns.
namespace {
struct HookScalars {
    stx_engine *e;
    size_t si = 0;
    explicit HookScalars(stx_engine *eng) : e(eng) {}
    ~HookScalars() { e->A().used = 0; }
    int take(size_t n, float **sc) {
        STX_TRY(do_sync(e));
        STX_TRY(alloc_scalars(e, n, &si));
        *sc = e->A().scalars.f() + si;
        return STX_OK;
    }
    int fetch(const float **host) {
        STX_HIP(hipMemcpyAsync(e->A().host, e->A().scalars.ptr, e->A().used * sizeof(float), hipMemcpyDeviceToHost,
                               e->stream));
        STX_HIP(hipStreamSynchronize(e->stream));
        *host = e->A().host + si;
        return STX_OK;
    }
};
}  // namespace

int stx_op_style_terms(stx_engine *e, const float *feat, int C, int h, int w,
                       const float *gram_target, float *s_out, float *normalized_out,
                       double *half_sumsq, double *abs_sum) {
    if (!e || !feat || !gram_target || C <= 0 || C % 4 || h <= 0 || w <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    const size_t count = (size_t)C * h * w;
    STX_TRY(e->upload.ensure(count * sizeof(float)));
    float *sgrad = s_out ? s_out : e->upload.f();
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(2, &sc));
    // the launches of the style branch of stx_sc_grad_tile, in the same order
    STX_TRY(launch_style_terms(e, e->stream, feat, C, h, w, gram_target, sgrad, sc, "op"));
    if (normalized_out)
        STX_TRY(inject_style_launch(e->stream, normalized_out, sgrad, count, sc + 1, 1.0f, false));
    STX_TRY(scalars.fetch(&host));
    if (half_sumsq) *half_sumsq = 0.5 * (double)host[0];
    if (abs_sum) *abs_sum = (double)host[1];
    return STX_OK;
}

int stx_op_masked_style_terms(stx_engine *e, const float *feat, int C, int h, int w, const float *mask_map,
                              int mh, int mw, int oy, int ox, const int roll_xy[2], const float *gram_target,
                              float *sgrad_out, double out[3]) {
    if (!e || !feat || !mask_map || !gram_target || !sgrad_out || !out || C <= 0 || C % 4 || h <= 0 || w <= 0)
        return STX_ERR_ARG;
    if (oy < 0 || ox < 0 || oy + h > mh || ox + w > mw) {
        set_error("stx_op_masked_style_terms: window exceeds the mask map");
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(4, &sc));
    STX_TRY(e->term_scratch.ensure(kMaskScratchFloats * sizeof(float)));
    // the launches of a masked style target of stx_sc_grad_tile, in the same order
    STX_TRY(launch_masked_style_terms(e, e->stream, feat, C, h, w, mask_map, hook_window(C, h, w, mh, mw, oy, ox, roll_xy),
                                      gram_target, sgrad_out, sc, "op", nullptr, nullptr, e->term_scratch.f(), nullptr));
    STX_TRY(scalars.fetch(&host));
    out[0] = 0.5 * (double)host[0];
    out[1] = (double)host[2];
    out[2] = (double)host[3];
    return STX_OK;
}

int stx_op_stat_terms(stx_engine *e, const float *feat, int C, int h, int w, const float *MU, const float *SD,
                      float *s_out, double out[2]) {
    if (!e || !feat || !MU || !SD || !s_out || !out || C <= 0 || h <= 0 || w <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(2, &sc));
    STX_TRY(e->stat_scratch.ensure(stat_scratch_floats(C, h * w) * sizeof(float)));
    // the launches of a statistics target of stx_sc_grad_tile, in the same order
    STX_TRY(launch_stat_terms(e, e->stream, feat, C, h, w, MU, SD, s_out, sc, "op", e->stat_scratch.f(), nullptr));
    STX_TRY(scalars.fetch(&host));
    out[0] = 0.5 * (double)host[0];
    out[1] = (double)host[1];
    return STX_OK;
}

int stx_op_swd_terms(stx_engine *e, const float *feat, int C, int h, int w, const float *V, int D, const float *Tq,
                     int Q, float *s_out, int *rank_out, double out[2]) {
    if (!e || !feat || !V || !Tq || !s_out || !out || h <= 0 || w <= 0) {
        set_error("stx_op_swd_terms: bad arguments");
        return STX_ERR_ARG;
    }
    STX_TRY(swd_check("stx_op_swd_terms", C, (long long)h * w, D, Q));
    STX_TRY(e->set_device());
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(2, &sc));
    STX_TRY(e->swd_io.ensure(swd_scratch_floats(C, h * w, D) * sizeof(float)));
    // the launches of a sliced Wasserstein target of stx_sc_grad_tile, in the same order
    STX_TRY(launch_swd_terms(e, e->stream, feat, C, h, w, V, D, Tq, Q, s_out, rank_out, sc, "op", e->swd_io.f(),
                             nullptr));
    STX_TRY(scalars.fetch(&host));
    out[0] = 0.5 * (double)host[0];
    out[1] = (double)host[1];
    return STX_OK;
}

int stx_op_selfsim_terms(stx_engine *e, const float *feat, const float *content, int C, int h, int w, int points,
                         float *sgrad, double sc_out[2], signed char *signs_out) {
    if (!e || !feat || !content || !sgrad || !sc_out || h <= 0 || w <= 0) {
        set_error("stx_op_selfsim_terms: bad arguments");
        return STX_ERR_ARG;
    }
    STX_TRY(selfsim_check("stx_op_selfsim_terms", C, points));
    STX_TRY(e->set_device());
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(2, &sc));
    STX_TRY(e->selfsim_io.ensure(selfsim_scratch_floats(C, selfsim_grid(h, w, points).N) * sizeof(float)));
    // the launches of a self-similarity target of stx_sc_grad_tile, in the same order
    STX_TRY(launch_selfsim_terms(e, e->stream, feat, SelfsimSource{content, h, w, 0, 0}, C, h, w, points, sgrad,
                                 signs_out, sc, "op", e->selfsim_io.f(), nullptr));
    STX_TRY(scalars.fetch(&host));
    sc_out[0] = (double)host[0];
    sc_out[1] = (double)host[1];
    return STX_OK;
}

int stx_op_shift_terms(stx_engine *e, const float *feat, int C, int h, int w, const int *offsets, int n_offsets,
                       const float *grams, float *s_out, double out[2]) {
    if (!e || !feat || !grams || !s_out || !out) {
        set_error("stx_op_shift_terms: bad arguments");
        return STX_ERR_ARG;
    }
    ShiftOffsets off;
    STX_TRY(shift_check_offsets("stx_op_shift_terms", C, offsets, n_offsets, &off));
    STX_TRY(shift_check_map("stx_op_shift_terms", C, h, w, off));
    STX_TRY(e->set_device());
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(2, &sc));
    STX_TRY(e->shift_io.ensure(shift_scratch_floats(C, h * w, n_offsets) * sizeof(float)));
    // the launches of a shifted-Gram target of stx_sc_grad_tile, in the same order
    STX_TRY(launch_shift_terms(e, e->stream, feat, C, h, w, off, grams, s_out, sc, "op", e->shift_io.f(), nullptr));
    STX_TRY(scalars.fetch(&host));
    out[0] = 0.5 * (double)host[0];
    out[1] = (double)host[1];
    return STX_OK;
}

int stx_op_cx_terms(stx_engine *e, const float *feat, int C, int h, int w, int points, const float *bank,
                    const float *mu, int rows, double eta, float *sgrad, double sc_out[2], int *kbest_out,
                    int *winner_out) {
    if (!e || !feat || !bank || !mu || !sgrad || !sc_out || h <= 0 || w <= 0) {
        set_error("stx_op_cx_terms: bad arguments");
        return STX_ERR_ARG;
    }
    STX_TRY(cx_check("stx_op_cx_terms", C, points, rows, (double)(float)eta));
    STX_TRY(e->set_device());
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(2, &sc));
    STX_TRY(e->cx_io.ensure(cx_scratch_floats(C, selfsim_grid(h, w, points).N, rows) * sizeof(float)));
    // the launches of a contextual target of stx_sc_grad_tile, in the same order
    STX_TRY(launch_cx_terms(e, e->stream, feat, C, h, w, points, bank, mu, rows, (float)eta, sgrad, kbest_out,
                            winner_out, sc, "op", e->cx_io.f(), nullptr));
    STX_TRY(scalars.fetch(&host));
    sc_out[0] = (double)host[0];
    sc_out[1] = (double)host[1];
    return STX_OK;
}

int stx_op_masked_content_terms(stx_engine *e, const float *feat, int C, int h, int w, const float *content,
                                int content_h, int content_w, const float *mask_map, int oy, int ox,
                                const int roll_xy[2], float *sgrad_out, double out[3]) {
    if (!e || !feat || !content || !mask_map || !sgrad_out || !out || C <= 0 || h <= 0 || w <= 0) return STX_ERR_ARG;
    if (oy < 0 || ox < 0 || oy + h > content_h || ox + w > content_w) {
        set_error("stx_op_masked_content_terms: window exceeds the content map");
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(4, &sc));
    STX_TRY(e->term_scratch.ensure(kContentMaskScratchFloats * sizeof(float)));
    // the launches of a masked content target of stx_sc_grad_tile, in the same order
    STX_TRY(launch_masked_content_terms(e, e->stream, feat, content, mask_map,
                                        hook_window(C, h, w, content_h, content_w, oy, ox, roll_xy), sgrad_out, sc, "op",
                                        e->term_scratch.f(), nullptr));
    STX_TRY(scalars.fetch(&host));
    out[0] = 0.5 * (double)host[0];
    out[1] = (double)host[1];
    out[2] = (double)host[2];
    return STX_OK;
}

// The NNFM hooks.  k = 1 through stx_op_nnfm_knn_terms is the patch call; k > 1 speaks as stx_op_nnfm_knn_terms and
// index_out holds [k][h w].  Patch 1 is the plain term and speaks as stx_op_nnfm_terms through either entry point; every
// other patch size speaks as stx_op_nnfm_patch_terms: `plain` picks between the two entry points' messages, which
// are the ones they had as two functions.  Nothing is written before the arguments are accepted.  (An error behind
// take() leaves the scalar arena empty, as in the other term hooks.)
static int hook_nnfm_terms(stx_engine *e, const float *feat, int C, int h, int w, int patch, const float *bank, int rows,
                           float *s_out, int *index_out, double out[2], int k = 1, float cover = 0.f,
                           int *winner_out = nullptr) {
    const bool plain = patch == 1, covered = cover != 0.f;      // covered: out[3] = {E, sum |S|, E_cov}
    const char *const who = covered ? "stx_op_nnfm_cover_terms"
                            : k > 1 ? "stx_op_nnfm_knn_terms"
                            : plain ? "stx_op_nnfm_terms"
                                    : "stx_op_nnfm_patch_terms";
    if ((!plain && patch != 3) || !e || !feat || !bank || !s_out || !index_out || !out || C <= 0 || h <= 0 || w <= 0 ||
        rows <= 0) {
        if (plain)
            set_error("%s: bad arguments", who);
        else
            set_error("%s: bad arguments (patch %d; 1 or 3 is expected)", who, patch);
        return STX_ERR_ARG;
    }
    if (C % 64 != 0) {
        set_error("%s: the channel count %d is not a multiple of 64", who, C);
        return STX_ERR_UNSUPPORTED;
    }
    const long long n = (long long)h * w, width = (long long)patch * patch * C;
    if (n >= (1ll << 31) / C || rows >= (1ll << 31) / width || (!plain && reinterpret_cast<uintptr_t>(bank) % 16 != 0)) {
        if (plain)
            set_error("%s: %lld columns against %d rows of %d channels exceed 32-bit offsets", who, n, rows, C);
        else
            set_error("%s: %lld patches against %d rows of 9 x %d channels exceed 32-bit offsets, or the bank is not "
                      "aligned to 16 bytes", who, n, rows, C);
        return STX_ERR_UNSUPPORTED;
    }
    STX_TRY(e->set_device());
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(covered ? 3 : 2, &sc));
    const size_t pieces = nnfm_pieces_floats(rows, (int)width);
    STX_TRY(e->nnfm_scratch.ensure((pieces + nnfm_scratch_floats(C, h * w, rows, patch, k, covered)) * sizeof(float)));
    unsigned short *bhi = static_cast<unsigned short *>(e->nnfm_scratch.ptr);
    // what the targets' setter does once, then the launches of an NNFM target of stx_sc_grad_tile, in the same order
    STX_TRY(nnfm_split_rows_launch(e->stream, bank, rows, (int)width, bhi, bhi + (size_t)rows * width));
    STX_TRY(launch_nnfm_terms(e, e->stream, feat, C, h, w, patch, bank, bhi, rows, s_out, index_out, sc, "op",
                              e->nnfm_scratch.f() + pieces, nullptr, k, cover, winner_out, covered ? sc + 2 : nullptr));
    STX_TRY(scalars.fetch(&host));
    out[0] = (double)host[0];
    out[1] = (double)host[1];
    if (covered) out[2] = (double)host[2];
    return STX_OK;
}

int stx_op_nnfm_terms(stx_engine *e, const float *feat, int C, int h, int w, const float *bank, int rows,
                      float *s_out, int *index_out, double out[2]) {
    return hook_nnfm_terms(e, feat, C, h, w, 1, bank, rows, s_out, index_out, out);
}

int stx_op_nnfm_patch_terms(stx_engine *e, const float *feat, int C, int h, int w, int patch, const float *bank,
                            int rows, float *s_out, int *index_out, double out[2]) {
    return hook_nnfm_terms(e, feat, C, h, w, patch, bank, rows, s_out, index_out, out);
}

int stx_op_nnfm_knn_terms(stx_engine *e, const float *feat, int C, int h, int w, int patch, int k, const float *bank,
                          int rows, float *s_out, int *index_out, double out[2]) {
    if (k < 1 || k > kNnfmMaxK) {
        set_error("stx_op_nnfm_knn_terms: k %d (1 to %d is expected)", k, kNnfmMaxK);
        return STX_ERR_ARG;
    }
    return hook_nnfm_terms(e, feat, C, h, w, patch, bank, rows, s_out, index_out, out, k);
}

int stx_op_nnfm_cover_terms(stx_engine *e, const float *feat, int C, int h, int w, int patch, int k, float cover,
                            const float *bank, int rows, float *s_out, int *index_out, int *winner_out, double out[3]) {
    if (!(cover >= 0.f) || !std::isfinite(cover)) {
        set_error("stx_op_nnfm_cover_terms: cover %g (a finite factor, 0 or more, is expected)", (double)cover);
        return STX_ERR_ARG;
    }
    if (cover == 0.f) return stx_op_nnfm_knn_terms(e, feat, C, h, w, patch, k, bank, rows, s_out, index_out, out);
    if (patch != 1 || !winner_out) {
        set_error("stx_op_nnfm_cover_terms: cover %g with patch %d%s (the coverage part has no patch form)", (double)cover,
                  patch, winner_out ? "" : " and no place for the winners");
        return STX_ERR_ARG;
    }
    if (k < 1 || k > kNnfmMaxK) {
        set_error("stx_op_nnfm_cover_terms: k %d (1 to %d is expected)", k, kNnfmMaxK);
        return STX_ERR_ARG;
    }
    return hook_nnfm_terms(e, feat, C, h, w, patch, bank, rows, s_out, index_out, out, k, cover, winner_out);
}

int stx_op_nnfm_guided_terms(stx_engine *e, const float *feat, int C, int h, int w, int k, const float *bank,
                             const int *seg_rows, int segments, const float *mask_maps, int mh, int mw, int oy, int ox,
                             const int roll_xy[2], float *s_out, int *index_out, double out[3]) {
    const char *const who = "stx_op_nnfm_guided_terms";
    if (!e || !feat || !bank || !seg_rows || !mask_maps || !s_out || !index_out || !out || C <= 0 || h <= 0 || w <= 0) {
        set_error("%s: bad arguments", who);
        return STX_ERR_ARG;
    }
    if (segments < 1 || segments > kNnfmMaxSegments) {
        set_error("%s: %d segments (1 to %d are expected)", who, segments, kNnfmMaxSegments);
        return STX_ERR_ARG;
    }
    if (k < 1 || k > kNnfmMaxK) {
        set_error("%s: k %d (1 to %d is expected)", who, k, kNnfmMaxK);
        return STX_ERR_ARG;
    }
    long long rows = 0;
    for (int s = 0; s < segments; ++s) {
        if (seg_rows[s] < k) {
            set_error("%s: segment %d has %d rows, fewer than k = %d", who, s, seg_rows[s], k);
            return STX_ERR_ARG;
        }
        rows += seg_rows[s];
    }
    if (oy < 0 || ox < 0 || oy + h > mh || ox + w > mw) {
        set_error("%s: window exceeds the mask maps", who);
        return STX_ERR_ARG;
    }
    if (C % 64 != 0) {
        set_error("%s: the channel count %d is not a multiple of 64", who, C);
        return STX_ERR_UNSUPPORTED;
    }
    const long long n = (long long)h * w;
    if (n >= (1ll << 31) / C || rows >= (1ll << 31) / C) {
        set_error("%s: %lld columns against %lld rows of %d channels exceed 32-bit offsets", who, n, rows, C);
        return STX_ERR_UNSUPPORTED;
    }
    const NnfmSegments segs = nnfm_segments(seg_rows, segments);
    STX_TRY(e->set_device());
    HookScalars scalars(e);
    float *sc;
    const float *host;
    STX_TRY(scalars.take(3, &sc));
    const size_t pieces = nnfm_pieces_floats((int)rows, C);
    STX_TRY(e->nnfm_scratch.ensure((pieces + nnfm_guided_scratch_floats(C, h * w, segs, k)) * sizeof(float)));
    unsigned short *bhi = static_cast<unsigned short *>(e->nnfm_scratch.ptr);
    // what the targets' setter does once, then the launches of a guided target of stx_sc_grad_tile, in the same order
    STX_TRY(nnfm_split_rows_launch(e->stream, bank, (int)rows, C, bhi, bhi + (size_t)rows * C));
    STX_TRY(launch_nnfm_guided_terms(e, e->stream, feat, C, h, w, bank, bhi, segs, mask_maps,
                                     hook_window(C, h, w, mh, mw, oy, ox, roll_xy), s_out, index_out, sc, "op",
                                     e->nnfm_scratch.f() + pieces, nullptr, k, false));
    STX_TRY(scalars.fetch(&host));
    out[0] = (double)host[0];
    out[1] = (double)host[1];
    out[2] = (double)host[2];
    return STX_OK;
}

int stx_op_content_terms(stx_engine *e, const float *feat, int C, int h, int w,
                         const float *content, int content_h, int content_w, int oy, int ox,
                         const int roll_xy[2], float *normalized_out, double sums[2]) {
    if (!e || !feat || !content || C <= 0 || h <= 0 || w <= 0) return STX_ERR_ARG;
    if (oy < 0 || ox < 0 || oy + h > content_h || ox + w > content_w) {
        set_error("stx_op_content_terms: window exceeds the content map");
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    const ContentWindow win = hook_window(C, h, w, content_h, content_w, oy, ox, roll_xy);
    HookScalars scalars(e);
    float *s;
    const float *host;
    STX_TRY(scalars.take(kResidualScalars, &s));
    STX_TRY(content_sums_launch(e->stream, feat, content, win, s));
    if (normalized_out)
        STX_TRY(inject_content_launch(e->stream, normalized_out, feat, content, win, s, 1.0f, false));
    STX_TRY(scalars.fetch(&host));
    if (sums) {
        sums[0] = (double)host[0];
        sums[1] = (double)host[1];
    }
    return STX_OK;
}

}  // extern "C"
