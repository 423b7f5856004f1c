// libstx host side: the loss terms of a tile evaluation (tile_path.cpp) -- the launches of each kind of term,
// the list of a call's terms planned before its first launch, their queueing behind a tapped blob and their
// injection into the blob's gradient on the way back.

#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.h"

namespace stx {

// Floats of the engine's term_scratch that one style term of a C-channel, HW-pixel blob takes when its
// final sums are deferred: 2 x gram_finish's blocks + the SYMM kernel's workgroups, which outlive the call.
static size_t style_term_scratch_floats(int C, int HW) {
    return 2 * (size_t)ceil_div(C * C, 64) + (size_t)symm_num_workgroups(C, HW) + 64;
}

// The tail of every launch_*_terms: the final sums of a term's partials, launched now on `stream` or, with `defer`,
// left as jobs of the caller's ONE launch behind the forward pass (sum_jobs_launch) -- two sums, or one.
static int finish_sums(hipStream_t stream, std::vector<SumJob> *defer, const SumJob &a, const SumJob &b) {
    if (!defer) return sum_partials2_launch(stream, a.src, a.n, a.dst, b.src, b.n, b.dst);
    defer->push_back(a);
    defer->push_back(b);
    return STX_OK;
}
static int finish_sums(hipStream_t stream, std::vector<SumJob> *defer, const SumJob &a) {
    if (!defer) return sum_partials_launch(stream, a.src, a.n, a.dst);
    defer->push_back(a);
    return STX_OK;
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
    } else if ((gram_h2 || symm_h2) && e->amax_audit) {    // (a maximum somebody else left: stx_amax_audit)
        STX_TRY(amax_audit_note(e, stream, (feat == e->masked_feat.f() ? "masked style " : "style ") + name, name,
                                false, f_amax, feat, (size_t)C * HW));
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
        return finish_sums(stream, defer, SumJob{block_sumsq, fin_blocks, sc}, SumJob{symm_partials, n_wg, sc + 1});
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
    return finish_sums(stream, defer, SumJob{ms_partials, n_ms, sc + 2});
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
    return finish_sums(stream, defer, SumJob{abs_partials, n_parts, sc + 1});
}

// The nearest-neighbour term of one tapped blob (nnfm.hip): 1 / |f_i| and the pieces of the unit columns, the
// search over the bank (with the slices' merge when the bank was cut), S with the partials of E and sum |S|.
// patch 3: 1 / |P_p| and the pieces of the columns under one scale, the gathered search, c_p and S.
// k > 1: the search keeps the k best rows of a column and S pulls towards their mean (the profile names say so).
// cover != 0 (patch 1): behind those, the reverse search (bank rows look for their best column), the inverted index
// and the pass that adds cover S_cov to S; sc[0] is then the sum of ONE list of partials, E_fwd's and cover E_cov's,
// and sc[1] that of the final S's.
int launch_nnfm_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w, int patch,
                      const float *bank, const unsigned short *pieces, int rows, float *sgrad, int *idx_out, float *sc,
                      const std::string &name, float *scratch, std::vector<SumJob> *defer, int k, float cover,
                      int *winner_out, float *e_cov_out) {
    const int n = h * w;
    const bool covered = cover != 0.f;
    if (covered && patch != 1) {
        set_error("launch_nnfm_terms: the coverage part with patch %d", patch);
        return STX_ERR_ARG;
    }
    const NnfmScratch x = nnfm_carve(scratch, C, n, rows, patch, k, covered);
    const NnfmPlan plan = nnfm_plan(n, rows);
    int *const idx = idx_out ? idx_out : x.idx;
    const std::string tag = std::string(patch == 3 ? "nnfm patch " : "nnfm ") + (k > 1 ? "k" + std::to_string(k) + " " : "");
    {
        ProfScope scope(e, tag + "prepare " + name, 0.0, stream);
        STX_TRY(nnfm_prepare_launch(stream, feat, C, h, w, patch, 1, x.work, x.inv_r, x.xhi, x.xlo, nullptr));
    }
    {
        ProfScope scope(e, tag + "search " + name + " x" + std::to_string(plan.slices),
                        6.0 * n * (double)rows * C * (patch * patch), stream);
        STX_TRY(nnfm_search_launch(stream, x, h, w, patch, pieces, rows, C, idx, k));
    }
    int n_parts = 0;
    {
        ProfScope scope(e, tag + "grad " + name, 0.0, stream);
        STX_TRY(nnfm_grad_launch(stream, feat, C, h, w, patch, x, bank, rows, idx, sgrad, &n_parts, k));
    }
    if (covered) {
        int *const winner = winner_out ? winner_out : x.cov.winner;
        int n_e = 0, n_abs = 0;
        {
            ProfScope scope(e, "nnfm cover search " + name + " x" + std::to_string(nnfm_plan(rows, n).slices),
                            6.0 * n * (double)rows * C, stream);
            STX_TRY(nnfm_cover_search_launch(stream, x, n, pieces, rows, C, winner));
        }
        {
            ProfScope scope(e, "nnfm cover index " + name, 0.0, stream);
            STX_TRY(nnfm_cover_index_launch(stream, feat, C, n, x, bank, rows, winner, cover));
        }
        {
            ProfScope scope(e, "nnfm cover grad " + name, 0.0, stream);
            STX_TRY(nnfm_cover_grad_launch(stream, feat, C, n, x, bank, rows, cover, sgrad, &n_e, &n_abs));
        }
        if (e_cov_out) STX_TRY(sum_partials_launch(stream, x.cov.e_cov_parts, ceil_div(rows, 64), e_cov_out));
        return finish_sums(stream, defer, SumJob{x.cov.e_parts, n_e, sc}, SumJob{x.cov.abs_parts, n_abs, sc + 1});
    }
    return finish_sums(stream, defer, SumJob{x.partials, n_parts, sc}, SumJob{x.partials + n_parts, n_parts, sc + 1});
}

// The guided nearest-neighbour term of one tapped blob (nnfm.hip; patch 1): as above, with the mask windows and a
// between prepare and search, the search per (query block, slice, segment) and the gradient weighted by the masks.
int launch_nnfm_guided_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w,
                             const float *bank, const unsigned short *pieces, const NnfmSegments &segs,
                             const float *maps, const ContentWindow &win, float *sgrad, int *idx_out, float *sc,
                             const std::string &name, float *scratch, std::vector<SumJob> *defer, int k,
                             bool scale_by_a) {
    const int n = h * w;
    const NnfmGuidedScratch x = nnfm_guided_carve(scratch, C, n, segs, k);
    const NnfmPlan plan = nnfm_plan(n, segs.largest());
    int *const idx = idx_out ? idx_out : x.idx;
    const std::string tag = "nnfm guided " + (k > 1 ? "k" + std::to_string(k) + " " : std::string());
    {
        ProfScope scope(e, tag + "prepare " + name, 0.0, stream);
        STX_TRY(nnfm_prepare_launch(stream, feat, C, h, w, 1, 1, nullptr, x.inv_r, x.xhi, x.xlo, nullptr));
    }
    {
        ProfScope scope(e, tag + "window " + name, 0.0, stream);
        STX_TRY(nnfm_mask_window_launch(stream, maps, win, segs, k, x, idx, sc + 2));
    }
    {       // (the flops of a search of every pair: what the activity bytes leave out is the gain)
        ProfScope scope(e, tag + "search " + name + " x" + std::to_string(plan.slices) + " s" + std::to_string(segs.count),
                        6.0 * n * (double)segs.total() * C, stream);
        STX_TRY(nnfm_guided_search_launch(stream, x, n, pieces, segs, C, idx, k));
    }
    ProfScope scope(e, tag + "grad " + name, 0.0, stream);
    int n_parts = 0;
    STX_TRY(nnfm_guided_grad_launch(stream, feat, C, n, x, bank, segs, idx, scale_by_a ? sc + 2 : nullptr, sgrad,
                                    &n_parts, k));
    return finish_sums(stream, defer, SumJob{x.partials, n_parts, sc}, SumJob{x.partials + n_parts, n_parts, sc + 1});
}

// The sliced Wasserstein term of one tapped blob (swd.hip): the projections as sort records, the segmented sort
// whose last launch is the rank pass (G with the partials of E), S = V^T G / D with the partials of sum |S|.
int launch_swd_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w, const float *V, int D,
                     const float *Tq, int Q, float *sgrad, int *rank_out, float *sc, const std::string &name,
                     float *scratch, std::vector<SumJob> *defer) {
    const int n = h * w;
    STX_TRY(swd_check("launch_swd_terms", C, (long long)h * w, D, Q));
    // (grows when a larger blob than ever arrives; the stream orders the terms that share it)
    STX_TRY(e->swd_work.ensure(swd_work_floats(n, D) * sizeof(float)));
    void *const records = e->swd_work.ptr;
    float *const G = e->swd_work.f() + 2 * (size_t)D * swd_padded(n);
    const int n_e = swd_e_parts(n, D);
    float *const e_parts = scratch, *const abs_parts = scratch + (((size_t)n_e + 63) & ~(size_t)63);
    {
        ProfScope scope(e, "swd project " + name, 2.0 * D * (double)C * n, stream);
        STX_TRY(swd_project_launch(stream, feat, C, n, V, D, records));
    }
    {
        ProfScope scope(e, "swd sort " + name + " x" + std::to_string(swd_sort_passes(n) - 1), 0.0, stream);
        STX_TRY(swd_sort_launch(stream, records, n, D));
    }
    {       // (the sort's last launch: the steps left inside a block, then the rank pass from LDS)
        ProfScope scope(e, "swd rank " + name, 0.0, stream);
        STX_TRY(swd_finish_launch(stream, records, n, D, Tq, Q, G, rank_out, e_parts));
    }
    ProfScope scope(e, "swd grad " + name, 2.0 * D * (double)C * n, stream);
    int n_abs = 0;
    STX_TRY(swd_grad_launch(stream, V, G, C, n, D, sgrad, abs_parts, &n_abs));
    return finish_sums(stream, defer, SumJob{e_parts, n_e, sc}, SumJob{abs_parts, n_abs, sc + 1});
}

// The self-similarity content term of one tapped blob (selfsim.hip): both sides' unit columns on the sample grid,
// the two distance matrices in one launch, the column pass (T, the partials of E, A), q = -(A + A^T) X with its
// projection into the blob's layout (the partials of sum |S|).
int launch_selfsim_terms(stx_engine *e, hipStream_t stream, const float *feat, const SelfsimSource &content, int C,
                         int h, int w, int points, float *sgrad, signed char *signs_out, float *sc,
                         const std::string &name, float *scratch, std::vector<SumJob> *defer) {
    STX_TRY(selfsim_check("launch_selfsim_terms", C, points));
    const SelfsimGrid gr = selfsim_grid(h, w, points);
    const SelfsimScratch x = selfsim_scratch(scratch, C, gr.N);
    const double product = 2.0 * (double)gr.N * gr.N * C;
    {
        ProfScope scope(e, "selfsim prepare " + name, 0.0, stream);
        STX_TRY(selfsim_prepare_launch(stream, SelfsimSource{feat, h, w, 0, 0}, content, C, gr, x));
    }
    {
        ProfScope scope(e, "selfsim dist " + name, 2.0 * product, stream);
        STX_TRY(selfsim_dist_launch(stream, C, gr.N, x));
    }
    int n_e = 0, n_abs = 0;
    {
        ProfScope scope(e, "selfsim cols " + name, 0.0, stream);
        STX_TRY(selfsim_cols_launch(stream, gr.N, x, signs_out ? signs_out : x.T, &n_e));
    }
    ProfScope scope(e, "selfsim grad " + name, product, stream);
    STX_TRY(selfsim_grad_launch(stream, C, h, w, gr, x, sgrad, &n_abs));
    return finish_sums(stream, defer, SumJob{x.e_parts, n_e, sc}, SumJob{x.abs_parts, n_abs, sc + 1});
}

// The shifted-Gram term of one tapped blob (shiftgram.hip): the slices' partials of every offset's cross-Gram, their
// merge against the targets (the gradient's weights and the partials of E), S with the partials of sum |S|.
int launch_shift_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w,
                       const ShiftOffsets &off, const float *targets, float *sgrad, float *sc, const std::string &name,
                       float *scratch, std::vector<SumJob> *defer) {
    STX_TRY(shift_check_map("launch_shift_terms", C, h, w, off));
    const ShiftScratch x = shift_scratch(scratch, C, h * w, off.n);
    const double product = 2.0 * off.n * (double)C * C * h * w;
    int n_e = 0, n_abs = 0;
    {
        ProfScope scope(e, "shift cross " + name, product, stream);
        STX_TRY(shift_cross_launch(stream, feat, C, h, w, off, x));
    }
    {
        ProfScope scope(e, "shift merge " + name, 0.0, stream);
        STX_TRY(shift_merge_launch(stream, C, h, w, off, x, targets, nullptr, &n_e));
    }
    ProfScope scope(e, "shift grad " + name, 2.0 * product, stream);
    STX_TRY(shift_grad_launch(stream, feat, C, h, w, off, x, sgrad, &n_abs));
    return finish_sums(stream, defer, SumJob{x.e_parts, n_e, sc}, SumJob{x.abs_parts, n_abs, sc + 1});
}

// The contextual term of one tapped blob (cx.hip): the unit columns of F - mu on the sample grid, the scores with
// the slots of the row maxima, the row pass (k*, tau, p), the column pass (i*, the partials of CX) with the second
// row pass (g, E), q = g B in K slices with its projection into the blob's layout (the partials of sum |S|).
int launch_cx_terms(stx_engine *e, hipStream_t stream, const float *feat, int C, int h, int w, int points,
                    const float *bank, const float *mu, int rows, float eta, float *sgrad, int *kbest_out,
                    int *winner_out, float *sc, const std::string &name, float *scratch, std::vector<SumJob> *defer) {
    STX_TRY(cx_check("launch_cx_terms", C, points, rows, eta));
    const SelfsimGrid gr = selfsim_grid(h, w, points);
    const CxScratch x = cx_scratch(scratch, C, gr.N, rows);
    const double product = 2.0 * (double)gr.N * rows * C;
    {
        ProfScope scope(e, "cx prepare " + name, 0.0, stream);
        STX_TRY(cx_prepare_launch(stream, feat, C, h, w, gr, mu, x));
    }
    {
        ProfScope scope(e, "cx score " + name, product, stream);
        STX_TRY(cx_score_launch(stream, C, gr.N, rows, bank, x));
    }
    {
        ProfScope scope(e, "cx rows " + name, 0.0, stream);
        STX_TRY(cx_rows_pass_launch(stream, gr.N, rows, eta, x));
    }
    {
        ProfScope scope(e, "cx cols " + name, 0.0, stream);
        STX_TRY(cx_cols_pass_launch(stream, gr.N, rows, eta, x, kbest_out, winner_out));
    }
    int n_abs = 0;
    ProfScope scope(e, "cx grad " + name, product, stream);
    STX_TRY(cx_grad_launch(stream, C, h, w, gr, rows, bank, x, sgrad, &n_abs));
    return finish_sums(stream, defer, SumJob{x.e_part, 1, sc}, SumJob{x.abs_parts, n_abs, sc + 1});
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
    return finish_sums(stream, defer, SumJob{partials, n, sc}, SumJob{partials + n, n, sc + 1});
}

// The mask map of style `index` at `blob` (stx_set_style_masks), or null.
static const StyleMask *style_mask_of(const stx_engine *e, int index, int blob) {
    for (const StyleMask &m : e->sh->masks)
        if (m.index == index && m.blob == blob) return &m;
    return nullptr;
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

// The tile's window must lie inside its map; `what`: "content", "content mask" or "style mask".
static int check_window(const ContentWindow &win, const char *what, const Blob &b) {
    if (win.oy >= 0 && win.ox >= 0 && win.oy + win.fh <= win.ch && win.ox + win.fw <= win.cw) return STX_OK;
    set_error("%s window [%d+%d, %d+%d] exceeds the %dx%d %s of layer %s", what, win.oy, win.fh, win.ox, win.fw,
              win.ch, win.cw, strchr(what, ' ') ? "mask map" : "map", b.name.c_str());
    return STX_ERR_ARG;
}

int plan_terms(stx_engine *e, const TileCall &c, TilePlan &plan) {
    const SharedState &sh = *e->sh;
    const size_t n_taps = plan.order.size();
    plan.first_term.assign(n_taps, 0);
    plan.sgrad_floats.assign(n_taps, 0);
    const auto align = [](size_t floats) { return (floats + 63) & ~(size_t)63; };     // 256 bytes, like a DevBuf
    for (size_t k = n_taps; k-- > 0;) {       // shallowest tap first: the order the forward pass completes them in
        const Tap &tp = plan.order[k];
        const Blob &b = e->blobs[tp.blob];
        const double lw = tp.t->layer_weight;
        plan.first_term[k] = plan.terms.size();
        // The tap's gradient buffer: the style slots, then (each group from a 256-byte boundary) the masked
        // content slots and one slot per per-layer kind that is present, in planning order (take_slot).
        size_t styles_here = 0;
        for (const StyleTarget &st : sh.styles) styles_here += tp.t->is_style && st.blob == tp.blob;
        size_t style_slot = 0, content_slot = align(styles_here * b.count());
        const auto add = [&](TermKind kind, const float *target, const float *mask, const ContentWindow &win,
                             double coef, size_t scalars, size_t scratch, size_t slot) {
            plan.terms.push_back(PlannedTerm{kind, (int)k, target, mask, win, coef, scalars, plan.scratch_floats,
                                             scratch, slot});
            plan.scalars += scalars;
            plan.scratch_floats += scratch;
            if (slot != kNoSlot) plan.sgrad_floats[k] = std::max(plan.sgrad_floats[k], slot + b.count());
        };
        if (tp.t->is_content) {
            const ContentMask *mk = target_at(sh.cmasks, tp.blob);
            bool any = false;
            for (const ContentTarget &ct : sh.contents) {
                if (ct.blob != tp.blob) continue;
                any = true;
                // (the mask map has the content map's size: `win` is the window of both)
                const ContentWindow win = content_window(b, ct.h, ct.w, c.start, c.rx, c.ry);
                STX_TRY(check_window(win, mk ? "content mask" : "content", b));
                const double coef = lw * tp.t->content_weight;
                if (mk) {
                    add(TermKind::MaskedContent, ct.feat->f(), mk->map->f(), win, coef, 4, kContentMaskScratchFloats,
                        content_slot);
                    content_slot += b.count();
                } else {
                    add(TermKind::Content, ct.feat->f(), nullptr, win, coef, kResidualScalars, 0, kNoSlot);
                }
            }
            if (!any) {
                set_error("no content target for layer %s", b.name.c_str());
                return STX_ERR_STATE;
            }
        }
        if (tp.t->is_style) {
            if (!styles_here) {
                set_error("no style target for layer %s", b.name.c_str());
                return STX_ERR_STATE;
            }
            if (b.channels % 4 != 0) {
                set_error("style layer %s: channel count %d is not a multiple of 4", b.name.c_str(), b.channels);
                return STX_ERR_UNSUPPORTED;
            }
            const size_t late = plan.sums_late ? style_term_scratch_floats(b.channels, b.h * b.w) : 0;
            for (const StyleTarget &st : sh.styles) {
                if (st.blob != tp.blob) continue;
                const double coef = lw * tp.t->style_weight / sh.n_styles;
                if (const StyleMask *mk = style_mask_of(e, st.index, tp.blob)) {
                    // (the tile's window of the mask map, taken as a content map's is; its partials follow the
                    // deferred sums' region)
                    const ContentWindow win = content_window(b, mk->h, mk->w, c.start, c.rx, c.ry);
                    STX_TRY(check_window(win, "style mask", b));
                    add(TermKind::MaskedStyle, st.gram->f(), mk->map->f(), win, coef, 4, late + kMaskScratchFloats,
                        style_slot);
                } else {
                    add(TermKind::Style, st.gram->f(), nullptr, ContentWindow{}, coef, 2, late, style_slot);
                }
                style_slot += b.count();
            }
        }
        // The per-layer kinds (for_each_layer_kind), each behind whatever came before it: ONE cursor, which a kind
        // that is present moves on by its slot -- no kind asks which of the others are there.
        size_t cursor = align(content_slot);
        const auto take_slot = [&]() {
            const size_t slot = cursor;
            cursor = align(cursor + b.count());
            return slot;
        };
        if (const StatTarget *st = target_at(sh.stats, tp.blob)) {
            add(TermKind::Stat, st->ms->f(), nullptr, ContentWindow{}, lw * st->weight, 2,
                stat_scratch_floats(b.channels, b.h * b.w), take_slot());
        }
        if (const NnfmTarget *nt = target_at(sh.nnfms, tp.blob)) {
            if (nt->segs.count) {       // guided: the tile's window of the mask maps, taken as a content map's is
                const ContentWindow win = content_window(b, nt->mh, nt->mw, c.start, c.rx, c.ry);
                STX_TRY(check_window(win, "NNFM mask", b));
                add(TermKind::NnfmGuided, nt->bank->f(), nt->maps->f(), win, lw * nt->weight, 3,
                    nnfm_guided_scratch_floats(b.channels, b.h * b.w, nt->segs, nt->k), take_slot());
            } else {
                add(TermKind::Nnfm, nt->bank->f(), nullptr, ContentWindow{}, lw * nt->weight, 2,
                    nnfm_scratch_floats(b.channels, b.h * b.w, nt->rows, nt->patch, nt->k, nt->cover != 0.f),
                    take_slot());
            }
            plan.terms.back().nnfm = nt;
        }
        if (const SwdTarget *wt = target_at(sh.swds, tp.blob)) {
            STX_TRY(swd_check(("sliced Wasserstein target of layer " + b.name).c_str(), b.channels,
                              (long long)b.h * b.w, wt->D, wt->Q));
            add(TermKind::Swd, wt->Tq(), nullptr, ContentWindow{}, lw * wt->weight, 2,
                swd_scratch_floats(b.channels, b.h * b.w, wt->D), take_slot());
            plan.terms.back().swd = wt;
        }
        if (const SelfsimTarget *ft = target_at(sh.selfsims, tp.blob)) {
            STX_TRY(selfsim_check(("self-similarity target of layer " + b.name).c_str(), b.channels, ft->points));
            const ContentTarget *map = nullptr;     // the layer's content map of content_index 0, whatever the tap says
            for (const ContentTarget &ct : sh.contents)
                if (ct.blob == tp.blob && ct.index == 0 && !map) map = &ct;
            if (!map) {
                set_error("self-similarity target of layer %s: no content map of content_index 0 there", b.name.c_str());
                return STX_ERR_STATE;
            }
            const ContentWindow win = content_window(b, map->h, map->w, c.start, c.rx, c.ry);
            STX_TRY(check_window(win, "content", b));
            add(TermKind::Selfsim, map->feat->f(), nullptr, win, lw * ft->weight, 2,
                selfsim_scratch_floats(b.channels, selfsim_grid(b.h, b.w, ft->points).N), take_slot());
            plan.terms.back().points = ft->points;
        }
        if (const ShiftTarget *ht = target_at(sh.shifts, tp.blob)) {
            STX_TRY(shift_check_map(("shifted-Gram target of layer " + b.name).c_str(), b.channels, b.h, b.w, ht->off));
            add(TermKind::Shift, ht->grams->f(), nullptr, ContentWindow{}, lw * ht->weight, 2,
                shift_scratch_floats(b.channels, b.h * b.w, ht->off.n), take_slot());
            plan.terms.back().shift = ht;
        }
        if (const CxTarget *xt = target_at(sh.cxs, tp.blob)) {
            STX_TRY(cx_check(("contextual target of layer " + b.name).c_str(), b.channels, xt->points, xt->rows, xt->eta));
            add(TermKind::Cx, xt->bank(), nullptr, ContentWindow{}, lw * xt->weight, 2,
                cx_scratch_floats(b.channels, selfsim_grid(b.h, b.w, xt->points).N, xt->rows), take_slot());
            plan.terms.back().cx = xt;
        }
        // Deep-Dream (style_transfer.py:602-604): the content term against a zero map with a negative
        // weight -- loss -= lw*dd*1/2|F|^2, diff -= lw*dd*normalize(F)
        if (tp.t->is_dd)
            add(TermKind::Dream, nullptr, nullptr, dream_window(b), -lw * tp.t->dd_weight, kResidualScalars, 0, kNoSlot);
    }
    return STX_OK;
}

// Loss terms of tap k (Gram -> G - Gs -> SYMM, content residual sums, ...).  They are queued the
// moment the tapped blob is complete, in the middle of the forward pass, while the blob is
// still in the L2 / Infinity Cache the convolution just wrote it through (the shallow blobs
// were re-fetched from HBM when all taps ran after the forward pass: 1.1 GB per tile by PMC).
// Each enters the loss with half its coefficient (the contextual term, whose E is no square: with all of it) and
// the tap's gradient with all of it.
int queue_tap_terms(TileRun &run, size_t k) {
    stx_engine *e = run.e;
    const TilePlan &plan = run.plan;
    const Blob &b = e->blobs[plan.order[k].blob];
    for (size_t i = plan.first_term[k]; i < plan.terms.size() && plan.terms[i].tap == (int)k; ++i) {
        const PlannedTerm &t = plan.terms[i];
        size_t si;
        STX_TRY(alloc_scalars(e, t.scalars, &si));
        float *const sc = e->A().scalars.f() + si;
        float *const scratch = e->term_scratch.f() + t.scratch_off;
        float *const late = plan.sums_late ? scratch : nullptr;       // (a style term's deferred sums)
        float *const sgrad = t.sgrad_off == kNoSlot ? nullptr : e->sgrad[k]->f() + t.sgrad_off;
        // (the maximum the blob's producer left, if it left one: the fp16-split kernels' scale)
        const unsigned *f_amax = b.amax_data >= 0 ? e->amax_slots(b.amax_data, false) : nullptr;
        const float *abs_sum = sc + 1;
        switch (t.kind) {
        case TermKind::Content:
        case TermKind::Dream: {       // sc[0] = sum d^2, sc[1] = sum |d|, then their partials
            ProfScope scope(e, (t.kind == TermKind::Dream ? "dream " : "content ") + b.name, 0.0, e->stream);
            STX_TRY(content_sums_launch(e->stream, b.data.f(), t.target, t.win, sc, run.defer()));
            break;
        }
        case TermKind::MaskedContent: // sc[0] = sum m d^2, sc[1] = sum |m d|, sc[2] = a
            STX_TRY(launch_masked_content_terms(e, e->stream, b.data.f(), t.target, t.mask, t.win, sgrad, sc, b.name,
                                                scratch, run.defer()));
            break;
        case TermKind::Style:         // sc[0] = sum tril(D)^2, sc[1] = sum |S|
            STX_TRY(launch_style_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, t.target, sgrad, sc, b.name,
                                       f_amax, late, run.defer()));
            break;
        case TermKind::MaskedStyle:   // sc[0] = sum tril(D)^2, sc[2] = sum |m . S|, sc[3] = a
            STX_TRY(launch_masked_style_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, t.mask, t.win, t.target,
                                              sgrad, sc, b.name, f_amax, late,
                                              scratch + t.scratch_len - kMaskScratchFloats, run.defer()));
            abs_sum = sc + 2;
            break;
        case TermKind::Stat:          // sc[0] = E, sc[1] = sum |S|
            STX_TRY(launch_stat_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, t.target, t.target + b.channels,
                                      sgrad, sc, b.name, scratch, run.defer()));
            break;
        case TermKind::Nnfm:          // sc[0] = E, sc[1] = sum |S|
            STX_TRY(launch_nnfm_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, t.nnfm->patch, t.target,
                                      t.nnfm->pieces_hi_lo(), t.nnfm->rows, sgrad, nullptr, sc, b.name, scratch,
                                      run.defer(), t.nnfm->k, t.nnfm->cover));
            break;
        case TermKind::NnfmGuided:    // sc[0] = E, sc[1] = sum |S| (of S without a), sc[2] = a; sgrad = a S
            STX_TRY(launch_nnfm_guided_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, t.target,
                                             t.nnfm->pieces_hi_lo(), t.nnfm->segs, t.mask, t.win, sgrad, nullptr, sc,
                                             b.name, scratch, run.defer(), t.nnfm->k, true));
            break;
        case TermKind::Swd:           // sc[0] = E, sc[1] = sum |S|
            STX_TRY(launch_swd_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, t.swd->V(), t.swd->D, t.target,
                                     t.swd->Q, sgrad, nullptr, sc, b.name, scratch, run.defer()));
            break;
        case TermKind::Selfsim:       // sc[0] = E, sc[1] = sum |S|; the window as the content term addresses it
            STX_TRY(launch_selfsim_terms(e, e->stream, b.data.f(),
                                         SelfsimSource{t.target, t.win.ch, t.win.cw, t.win.oy - t.win.sy,
                                                       t.win.ox - t.win.sx},
                                         b.channels, b.h, b.w, t.points, sgrad, nullptr, sc, b.name, scratch,
                                         run.defer()));
            break;
        case TermKind::Shift:         // sc[0] = E, sc[1] = sum |S|
            STX_TRY(launch_shift_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, t.shift->off, t.target, sgrad, sc,
                                       b.name, scratch, run.defer()));
            break;
        case TermKind::Cx:            // sc[0] = E (which enters the loss whole), sc[1] = sum |S|
            STX_TRY(launch_cx_terms(e, e->stream, b.data.f(), b.channels, b.h, b.w, t.cx->points, t.target, t.cx->mu(),
                                    t.cx->rows, t.cx->eta, sgrad, nullptr, nullptr, sc, b.name, scratch, run.defer()));
            break;
        }
        run.pl.terms.push_back(LossTerm{si, t.kind == TermKind::Cx ? t.coef : t.coef * 0.5});
        run.terms[k].push_back(sgrad ? Term{Term::Gradient, sgrad, abs_sum, (float)t.coef, ContentWindow{}}
                                     : Term{Term::Residual, t.target, sc, (float)t.coef, t.win});
    }
    return STX_OK;
}

// Adds the terms of tap k to its blob's diff with stand-alone kernels (used for the deepest
// tap, for blobs produced by a pooling backward, and when a tap has more than one content or
// style term; otherwise the terms ride in the epilogue of the convolution backward above).
int inject_terms(TileRun &run, size_t k, bool &diff_written) {
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
        if (t.kind == Term::Gradient)
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
bool tap_fusable(const TileRun &run, size_t k) {
    int ns = 0, nc = 0;
    for (const Term &t : run.terms[k]) {
        if (t.kind == Term::Residual && !t.src) return false;      // Deep-Dream terms take the stand-alone path
        (t.kind == Term::Gradient ? ns : nc)++;
    }
    return ns <= 1 && nc <= 1;
}

// ... and what that epilogue needs of them (`bot`: the tapped blob).
ConvInject make_inject(const TileRun &run, size_t k, const Blob &bot) {
    ConvInject inj{};
    for (const Term &t : run.terms[k]) {
        if (t.kind == Term::Gradient) {
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

}  // namespace stx
