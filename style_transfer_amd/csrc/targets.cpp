// libstx host side: the targets of an engine group (stx_set_*).
//
// The engines of one GPU share their targets (SharedState): the content maps and style Grams, and behind them
// the style masks, the content mask and the targets of every per-layer kind (engine.h: for_each_layer_kind), which
// go when new contents and styles arrive.  Every setter is one swap (swap_targets) around a body that validates and
// copies.

#include <cmath>

#include "engine.h"

namespace {

// One swap of the group's targets: nothing that any member has queued still reads the old ones when `body`
// runs, and the copies and launches that `body` queued have finished when this returns -- a source on either
// side may be reused or freed right away, and the sharing engines read the new targets from their own streams.
// `body(wait)` returns a status; it may clear `wait` when nothing needs the host to wait.  On any failure
// `rollback` runs, so that no half-made target stays behind.
template <class Body, class Rollback>
static int swap_targets(stx_engine *e, const char *who, Body body, Rollback rollback) {
    STX_TRY(e->set_device());
    std::lock_guard<std::mutex> lock(e->sh->mutex);
    STX_TRY(quiesce_members(e));
    bool wait = true;
    int rc = body(wait);
    if (wait || rc != STX_OK) {
        const hipError_t err = hipStreamSynchronize(e->stream);
        if (rc == STX_OK && err != hipSuccess) {
            set_error("%s: %s", who, hipGetErrorString(err));
            rc = STX_ERR_HIP;
        }
    }
    if (rc != STX_OK) rollback();
    return rc;
}

// A caller's image-resolution mask [H][W] for the two mask setters: a host mask is staged on the device (in a
// buffer that goes with this object, behind the swap's wait), and map_at makes the block means at one scale.
struct MaskSource {
    DevBuf staged;
    const float *src = nullptr;
    int H = 0, W = 0;
    ~MaskSource() { staged.release(); }
    int stage(stx_engine *e, const float *mask, int h, int w, int mem) {
        src = mask, H = h, W = w;
        if (mem != STX_HOST) return STX_OK;
        const size_t bytes = (size_t)H * W * sizeof(float);
        STX_TRY(staged.ensure(bytes));
        src = staged.f();
        return copy_in(e, staged.ptr, mask, STX_HOST, bytes);
    }
    // (the map is allocated even when the launch fails: the caller keeps it where its rollback finds it)
    int map_at(stx_engine *e, int scale, int h, int w, std::unique_ptr<DevBuf> &map) const {
        map.reset(new DevBuf);
        STX_TRY(map->ensure((size_t)h * w * sizeof(float)));
        return mask_map_launch(e->stream, src, H, W, scale, map->f());
    }
};

// The opening of every per-layer setter's loop: target i of `kind` names `layer`, whose blob goes to *blob.  Refused:
// an unknown layer, the input, a layer that `have` holds already and -- under the same message, which ends in
// `or_no` -- a target without its data.  channels (or null: the kind has none) must be the blob's.
template <class T>
static int open_target(const stx_engine *e, const std::vector<T> &have, const char *kind, int i, const char *layer,
                       bool has_data, const char *or_no, const int *channels, int *blob) {
    *blob = e->find_blob(layer);
    if (*blob <= 0 || !has_data || target_at(have, *blob)) {
        set_error("%s target %d: bad layer '%s' (unknown, the input, or given twice)%s", kind, i,
                  layer ? layer : "(null)", or_no);
        return STX_ERR_ARG;
    }
    if (channels && *channels != e->blobs[*blob].channels) {
        set_error("%s target %d: layer %s has %d channels, not %d", kind, i, layer, e->blobs[*blob].channels, *channels);
        return STX_ERR_ARG;
    }
    return STX_OK;
}

// The banks of the four NNFM setters: a plain bank is a patch target with patch 1, both match k = 1 row, and all
// three have no coverage part (cover 0).
static int set_nnfm_banks(stx_engine *e, const stx_nnfm_cover_target *targets, int n, const char *who) {
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    for (int i = 0; i < n; ++i) {
        if (targets[i].patch != 1 && targets[i].patch != 3) {
            set_error("NNFM target %d: patch %d (1 or 3 is expected)", i, targets[i].patch);
            return STX_ERR_ARG;
        }
        if (targets[i].k < 1 || targets[i].k > kNnfmMaxK) {
            set_error("NNFM target %d: k %d (1 to %d is expected)", i, targets[i].k, kNnfmMaxK);
            return STX_ERR_ARG;
        }
        if (!(targets[i].cover >= 0.f) || !std::isfinite(targets[i].cover)) {
            set_error("NNFM target %d: cover %g (a finite factor, 0 or more, is expected)", i, (double)targets[i].cover);
            return STX_ERR_ARG;
        }
        if (targets[i].cover != 0.f && targets[i].patch != 1) {
            set_error("NNFM target %d: cover %g with patch %d (the coverage part has no patch form)", i,
                      (double)targets[i].cover, targets[i].patch);
            return STX_ERR_ARG;
        }
    }
    auto &nnfms = e->sh->nnfms;
    return swap_targets(e, who, [&](bool &) -> int {
        clear_targets(nnfms);
        for (int i = 0; i < n; ++i) {
            const stx_nnfm_cover_target &nt = targets[i];
            int blob;
            STX_TRY(open_target(e, nnfms, "NNFM", i, nt.layer, nt.bank && nt.rows > 0, " or no bank", &nt.channels, &blob));
            const int width = nt.patch * nt.patch * nt.channels;
            if (nt.channels % 64 != 0 || nt.rows >= (1ll << 31) / width) {
                set_error("NNFM target %d: %d rows of %d channels (a multiple of 64 and rows x channels below 2^31 "
                          "are expected)", i, nt.rows, width);
                return STX_ERR_UNSUPPORTED;
            }
            nnfms.push_back(NnfmTarget{blob, nt.channels, nt.rows, nt.weight, std::unique_ptr<DevBuf>(new DevBuf),
                                       std::unique_ptr<DevBuf>(new DevBuf), nt.patch, nt.k, nt.cover});
            NnfmTarget &t = nnfms.back();
            const size_t bytes = (size_t)t.rows * width * sizeof(float);
            STX_TRY(t.bank->ensure(bytes));
            STX_TRY(t.pieces->ensure(nnfm_pieces_floats(t.rows, width) * sizeof(float)));
            STX_TRY(copy_in(e, t.bank->ptr, nt.bank, nt.mem, bytes));
            // the fp16 pieces the search reads, once
            unsigned short *hi = static_cast<unsigned short *>(t.pieces->ptr);
            STX_TRY(nnfm_split_rows_launch(e->stream, t.bank->f(), t.rows, width, hi, hi + (size_t)t.rows * width));
        }
        return STX_OK;
    }, [&]() { clear_targets(nnfms); });
}

}  // namespace

extern "C" {

int stx_set_contents_and_styles(stx_engine *e, const stx_content_target *contents, int n_contents,
                                const stx_style_target *styles, int n_styles) {
    if (!e || (n_contents && !contents) || (n_styles && !styles)) return STX_ERR_ARG;
    SharedState &sh = *e->sh;
    return swap_targets(e, "stx_set_contents_and_styles", [&](bool &wait) -> int {
        clear_all_targets(sh);     // (with the masks, statistics and banks that were set behind the old ones)
        double copied = 0;
        bool host_src = false;
        for (int i = 0; i < n_contents; ++i) {
            const stx_content_target &c = contents[i];
            const int blob = e->find_blob(c.layer);
            if (blob < 0 || !c.features || c.channels != e->blobs[blob].channels || c.height <= 0 ||
                c.width <= 0 || c.content_index < 0) {
                set_error("content target %d: bad layer '%s' or shape", i, c.layer ? c.layer : "(null)");
                return STX_ERR_ARG;
            }
            sh.contents.push_back(ContentTarget{c.content_index, blob, c.channels, c.height, c.width,
                                                std::unique_ptr<DevBuf>(new DevBuf)});
            ContentTarget &t = sh.contents.back();
            const size_t bytes = (size_t)t.C * t.h * t.w * sizeof(float);
            STX_TRY(t.feat->ensure(bytes));
            STX_TRY(copy_in(e, t.feat->ptr, c.features, c.mem, bytes));
            copied += (double)bytes;
            host_src |= c.mem == STX_HOST;
            sh.n_contents = std::max(sh.n_contents, t.index + 1);
        }
        for (int i = 0; i < n_styles; ++i) {
            const stx_style_target &s = styles[i];
            const int blob = e->find_blob(s.layer);
            if (blob < 0 || !s.gram || s.channels != e->blobs[blob].channels || s.style_index < 0) {
                set_error("style target %d: bad layer '%s' or shape", i, s.layer ? s.layer : "(null)");
                return STX_ERR_ARG;
            }
            sh.styles.push_back(StyleTarget{s.style_index, blob, s.channels, std::unique_ptr<DevBuf>(new DevBuf)});
            StyleTarget &t = sh.styles.back();
            const size_t bytes = (size_t)t.C * t.C * sizeof(float);
            STX_TRY(t.gram->ensure(bytes));
            STX_TRY(copy_in(e, t.gram->ptr, s.gram, s.mem, bytes));
            copied += (double)bytes;
            host_src |= s.mem == STX_HOST;
            sh.n_styles = std::max(sh.n_styles, t.index + 1);
        }
        // (device sources of an engine that shares with nobody: its own stream orders the copies before the
        // next tile, and a --jitter step sets targets without a host wait)
        wait = host_src || sh.members.size() > 1;
        sh.target_uploads += 1;
        sh.target_bytes += copied;
        return STX_OK;
    }, [&]() { clear_all_targets(sh); });
}

int stx_set_style_masks(stx_engine *e, const stx_style_mask *masks, int n) {
    if (!e || n < 0 || (n && !masks)) return STX_ERR_ARG;
    SharedState &sh = *e->sh;
    MaskSource source;
    return swap_targets(e, "stx_set_style_masks", [&](bool &) -> int {
        clear_targets(sh.masks);
        for (int i = 0; i < n; ++i) {
            const stx_style_mask &sm = masks[i];
            bool any = false;
            for (const StyleTarget &st : sh.styles) any |= st.index == sm.style_index;
            if (!sm.mask || sm.H <= 0 || sm.W <= 0 || !any) {
                set_error("style mask %d: no mask, a bad size or no style target of index %d", i, sm.style_index);
                return STX_ERR_ARG;
            }
            STX_TRY(source.stage(e, sm.mask, sm.H, sm.W, sm.mem));
            for (const StyleTarget &st : sh.styles) {
                if (st.index != sm.style_index) continue;
                bool have = false;
                for (const StyleMask &m : sh.masks) have |= m.index == st.index && m.blob == st.blob;
                if (have) continue;
                const int scale = e->blobs[st.blob].scale;
                sh.masks.push_back(StyleMask{st.index, st.blob, ceil_div(sm.H, scale), ceil_div(sm.W, scale), nullptr});
                StyleMask &m = sh.masks.back();
                STX_TRY(source.map_at(e, scale, m.h, m.w, m.map));
            }
        }
        return STX_OK;
    }, [&]() { clear_targets(sh.masks); });
}

int stx_set_content_mask(stx_engine *e, const float *mask, int H, int W, int mem) {
    if (!e || (mask && (H <= 0 || W <= 0))) return STX_ERR_ARG;
    SharedState &sh = *e->sh;
    MaskSource source;
    return swap_targets(e, "stx_set_content_mask", [&](bool &) -> int {
        clear_targets(sh.cmasks);
        if (!mask) return STX_OK;
        if (sh.contents.empty()) {
            set_error("stx_set_content_mask: no content targets set (call it after stx_set_contents_and_styles)");
            return STX_ERR_STATE;
        }
        // the map of a blob has the size of the blob's content maps: the tile's window is taken from both alike
        for (const ContentTarget &ct : sh.contents) {
            const int scale = e->blobs[ct.blob].scale;
            if (ceil_div(H, scale) != ct.h || ceil_div(W, scale) != ct.w) {
                set_error("stx_set_content_mask: a %dx%d mask gives a %dx%d map at layer %s, whose content map is "
                          "%dx%d; the mask must have the content picture's size", H, W, ceil_div(H, scale),
                          ceil_div(W, scale), e->blobs[ct.blob].name.c_str(), ct.h, ct.w);
                return STX_ERR_ARG;
            }
        }
        STX_TRY(source.stage(e, mask, H, W, mem));
        for (const ContentTarget &ct : sh.contents) {
            bool have = false;
            for (const ContentMask &m : sh.cmasks) have |= m.blob == ct.blob;
            if (have) continue;
            sh.cmasks.push_back(ContentMask{ct.blob, ct.h, ct.w, nullptr});
            STX_TRY(source.map_at(e, e->blobs[ct.blob].scale, ct.h, ct.w, sh.cmasks.back().map));
        }
        return STX_OK;
    }, [&]() { clear_targets(sh.cmasks); });
}

int stx_set_stat_targets(stx_engine *e, const stx_stat_target *targets, int n) {
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    auto &stats = e->sh->stats;
    return swap_targets(e, "stx_set_stat_targets", [&](bool &) -> int {
        clear_targets(stats);
        for (int i = 0; i < n; ++i) {
            const stx_stat_target &st = targets[i];
            int blob;
            STX_TRY(open_target(e, stats, "statistics", i, st.layer, st.mean && st.sd, " or no data", &st.channels, &blob));
            stats.push_back(StatTarget{blob, st.channels, st.weight, std::unique_ptr<DevBuf>(new DevBuf)});
            StatTarget &t = stats.back();
            const size_t bytes = (size_t)t.C * sizeof(float);
            STX_TRY(t.ms->ensure(2 * bytes));
            STX_TRY(copy_in(e, t.ms->ptr, st.mean, st.mem, bytes));
            STX_TRY(copy_in(e, t.ms->f() + t.C, st.sd, st.mem, bytes));
        }
        return STX_OK;
    }, [&]() { clear_targets(stats); });
}

int stx_set_swd_targets(stx_engine *e, const struct stx_swd_target *targets, int n) {
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    auto &swds = e->sh->swds;
    return swap_targets(e, "stx_set_swd_targets", [&](bool &) -> int {
        clear_targets(swds);
        for (int i = 0; i < n; ++i) {
            const struct stx_swd_target &wt = targets[i];
            int blob;
            STX_TRY(open_target(e, swds, "sliced Wasserstein", i, wt.layer, wt.V && wt.Tq, " or no data", &wt.channels,
                                &blob));
            STX_TRY(swd_check("stx_set_swd_targets", wt.channels, 1, wt.dirs, wt.quantiles));
            swds.push_back(SwdTarget{blob, wt.channels, wt.dirs, wt.quantiles, wt.weight,
                                     std::unique_ptr<DevBuf>(new DevBuf)});
            SwdTarget &t = swds.back();
            const size_t v_bytes = (size_t)t.D * t.C * sizeof(float), q_bytes = (size_t)t.D * t.Q * sizeof(float);
            STX_TRY(t.vt->ensure(v_bytes + q_bytes));
            STX_TRY(copy_in(e, t.vt->ptr, wt.V, wt.mem, v_bytes));
            STX_TRY(copy_in(e, t.vt->f() + (size_t)t.D * t.C, wt.Tq, wt.mem, q_bytes));
        }
        return STX_OK;
    }, [&]() { clear_targets(swds); });
}

int stx_set_selfsim_targets(stx_engine *e, const struct stx_selfsim_target *targets, int n) {
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    auto &selfsims = e->sh->selfsims;
    return swap_targets(e, "stx_set_selfsim_targets", [&](bool &) -> int {
        clear_targets(selfsims);
        for (int i = 0; i < n; ++i) {
            const struct stx_selfsim_target &ft = targets[i];
            int blob;
            STX_TRY(open_target(e, selfsims, "self-similarity", i, ft.layer, true, "", nullptr, &blob));
            bool has_map = false;
            for (const ContentTarget &ct : e->sh->contents) has_map |= ct.blob == blob && ct.index == 0;
            if (!has_map) {
                set_error("self-similarity target %d: layer %s holds no content map of content_index 0", i, ft.layer);
                return STX_ERR_ARG;
            }
            STX_TRY(selfsim_check("stx_set_selfsim_targets", e->blobs[blob].channels, ft.points));
            selfsims.push_back(SelfsimTarget{blob, ft.points, ft.weight});
        }
        return STX_OK;
    }, [&]() { clear_targets(selfsims); });
}

int stx_set_shift_targets(stx_engine *e, const struct stx_shift_target *targets, int n) {
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    auto &shifts = e->sh->shifts;
    return swap_targets(e, "stx_set_shift_targets", [&](bool &) -> int {
        clear_targets(shifts);
        for (int i = 0; i < n; ++i) {
            const struct stx_shift_target &ht = targets[i];
            int blob;
            STX_TRY(open_target(e, shifts, "shifted-Gram", i, ht.layer, ht.grams && ht.offsets, " or no data",
                                &ht.channels, &blob));
            ShiftOffsets off;
            STX_TRY(shift_check_offsets("stx_set_shift_targets", ht.channels, ht.offsets, ht.n_offsets, &off));
            shifts.push_back(ShiftTarget{blob, ht.channels, off, ht.weight, std::unique_ptr<DevBuf>(new DevBuf)});
            ShiftTarget &t = shifts.back();
            const size_t bytes = (size_t)off.n * t.C * t.C * sizeof(float);
            STX_TRY(t.grams->ensure(bytes));
            STX_TRY(copy_in(e, t.grams->ptr, ht.grams, ht.mem, bytes));
        }
        return STX_OK;
    }, [&]() { clear_targets(shifts); });
}

int stx_set_cx_targets(stx_engine *e, const struct stx_cx_target *targets, int n) {
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    auto &cxs = e->sh->cxs;
    std::vector<std::unique_ptr<DevBuf>> raws;      // the copied raw rows; they go behind the swap's wait
    const int rc = swap_targets(e, "stx_set_cx_targets", [&](bool &) -> int {
        clear_targets(cxs);
        for (int i = 0; i < n; ++i) {
            const struct stx_cx_target &xt = targets[i];
            int blob;
            STX_TRY(open_target(e, cxs, "contextual", i, xt.layer, xt.raw_rows != nullptr, " or no rows", &xt.channels,
                                &blob));
            STX_TRY(cx_check("stx_set_cx_targets", xt.channels, xt.points, xt.rows, (double)(float)xt.h));
            cxs.push_back(CxTarget{blob, xt.channels, xt.rows, xt.points, (float)xt.h, xt.weight,
                                   std::unique_ptr<DevBuf>(new DevBuf)});
            CxTarget &t = cxs.back();
            const size_t floats = (size_t)t.rows * t.C;
            STX_TRY(t.data->ensure((floats + t.C) * sizeof(float)));
            raws.emplace_back(new DevBuf);
            DevBuf &raw = *raws.back();
            STX_TRY(raw.ensure(floats * sizeof(float)));
            STX_TRY(copy_in(e, raw.ptr, xt.raw_rows, xt.mem, floats * sizeof(float)));
            STX_TRY(cx_bank_launch(e->stream, raw.f(), t.C, t.rows, t.data->f() + floats, t.data->f()));
        }
        return STX_OK;
    }, [&]() { clear_targets(cxs); });
    for (auto &raw : raws) raw->release();
    return rc;
}

int stx_set_nnfm_targets(stx_engine *e, const stx_nnfm_target *targets, int n) {
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    std::vector<stx_nnfm_cover_target> as_knn;
    for (int i = 0; i < n; ++i) {
        const stx_nnfm_target &t = targets[i];
        as_knn.push_back(stx_nnfm_cover_target{t.layer, t.channels, 1, 1, t.rows, t.bank, t.mem, t.weight, 0.f});
    }
    return set_nnfm_banks(e, as_knn.data(), n, "stx_set_nnfm_targets");
}

int stx_set_nnfm_patch_targets(stx_engine *e, const stx_nnfm_patch_target *targets, int n) {
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    std::vector<stx_nnfm_cover_target> as_knn;
    for (int i = 0; i < n; ++i) {
        const stx_nnfm_patch_target &t = targets[i];
        as_knn.push_back(stx_nnfm_cover_target{t.layer, t.channels, t.patch, 1, t.rows, t.bank, t.mem, t.weight, 0.f});
    }
    return set_nnfm_banks(e, as_knn.data(), n, "stx_set_nnfm_patch_targets");
}

int stx_set_nnfm_knn_targets(stx_engine *e, const stx_nnfm_knn_target *targets, int n) {
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    std::vector<stx_nnfm_cover_target> as_cover;
    for (int i = 0; i < n; ++i) {
        const stx_nnfm_knn_target &t = targets[i];
        as_cover.push_back(stx_nnfm_cover_target{t.layer, t.channels, t.patch, t.k, t.rows, t.bank, t.mem, t.weight, 0.f});
    }
    return set_nnfm_banks(e, as_cover.data(), n, "stx_set_nnfm_knn_targets");
}

int stx_set_nnfm_cover_targets(stx_engine *e, const stx_nnfm_cover_target *targets, int n) {
    return set_nnfm_banks(e, targets, n, "stx_set_nnfm_cover_targets");
}

int stx_set_nnfm_guided_targets(stx_engine *e, const stx_nnfm_guided_target *targets, int n,
                                const float *const *masks, int segments, int H, int W, int mask_mem) {
    const char *const who = "stx_set_nnfm_guided_targets";
    if (!e || n < 0 || (n && !targets)) return STX_ERR_ARG;
    if (segments < 1 || segments > STX_NNFM_MAX_SEGMENTS) {
        set_error("%s: %d segments (1 to %d are expected)", who, segments, STX_NNFM_MAX_SEGMENTS);
        return STX_ERR_ARG;
    }
    if (!masks || H <= 0 || W <= 0) {
        set_error("%s: no masks or a bad mask size %dx%d", who, H, W);
        return STX_ERR_ARG;
    }
    for (int s = 0; s < segments; ++s) {
        if (masks[s]) continue;
        set_error("%s: no mask for segment %d", who, s);
        return STX_ERR_ARG;
    }
    std::vector<stx_nnfm_cover_target> as_cover;
    for (int i = 0; i < n; ++i) {
        const stx_nnfm_guided_target &t = targets[i];
        if (t.k < 1 || t.k > kNnfmMaxK) {
            set_error("NNFM target %d: k %d (1 to %d is expected)", i, t.k, kNnfmMaxK);
            return STX_ERR_ARG;
        }
        if (t.segments != segments || !t.seg_rows) {
            set_error("NNFM target %d: %d segments for %d masks", i, t.segments, segments);
            return STX_ERR_ARG;
        }
        long long rows = 0;
        for (int s = 0; s < segments; ++s) {
            if (t.seg_rows[s] < t.k) {
                set_error("NNFM target %d: segment %d has %d rows, fewer than k = %d", i, s, t.seg_rows[s], t.k);
                return STX_ERR_ARG;
            }
            rows += t.seg_rows[s];
        }
        if (rows >= (1ll << 31) / std::max(t.channels, 1)) {
            set_error("NNFM target %d: %lld rows of %d channels (rows x channels below 2^31 are expected)", i, rows,
                      t.channels);
            return STX_ERR_UNSUPPORTED;
        }
        as_cover.push_back(stx_nnfm_cover_target{t.layer, t.channels, 1, t.k, (int)rows, t.bank, t.mem, t.weight, 0.f});
    }
    // the banks as the other setters make them; then, in a swap of its own, every bank's segments and mask maps
    STX_TRY(set_nnfm_banks(e, as_cover.data(), n, who));
    auto &nnfms = e->sh->nnfms;
    MaskSource source;
    return swap_targets(e, who, [&](bool &) -> int {
        for (int i = 0; i < n; ++i) {
            NnfmTarget &t = nnfms[i];
            const int scale = e->blobs[t.blob].scale;
            t.segs = nnfm_segments(targets[i].seg_rows, segments);
            t.mh = ceil_div(H, scale);
            t.mw = ceil_div(W, scale);
            t.maps.reset(new DevBuf);
            STX_TRY(t.maps->ensure((size_t)segments * t.mh * t.mw * sizeof(float)));
        }
        for (int s = 0; s < segments; ++s) {       // (one staging of a host mask serves every layer)
            STX_TRY(source.stage(e, masks[s], H, W, mask_mem));
            for (int i = 0; i < n; ++i) {
                NnfmTarget &t = nnfms[i];
                STX_TRY(mask_map_launch(e->stream, source.src, H, W, e->blobs[t.blob].scale,
                                        t.maps->f() + (size_t)s * t.mh * t.mw));
            }
            // (the staging buffer is reused by the next mask: its launches must have read it)
            if (mask_mem == STX_HOST) STX_HIP(hipStreamSynchronize(e->stream));
        }
        return STX_OK;
    }, [&]() { clear_targets(nnfms); });
}

}  // extern "C"
