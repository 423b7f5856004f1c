// libstx host side: the entries that work on whole images, feature maps and parameter vectors
// (stx_image_*, stx_map_*, stx_vec_*, stx_adam_step) -- thin wrappers that check their arguments and
// queue a few launches of image_ops.hip / reduce.hip / swt.hip / lap.hip / photo.hip / temporal.hip /
// flow.hip on the engine's stream.

#include <cmath>
#include <cstdint>
#include <functional>
#include <initializer_list>

#include "engine.h"

extern "C" {

int stx_image_cut_tile(stx_engine *e, const float *img, int H, int W, const int roll_xy[2], int y0,
                       int x0, int th, int tw, float *tile) {
    if (!e || !img || !tile || H <= 0 || W <= 0 || th <= 0 || tw <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return cut_tile_launch(e->stream, img, H, W, roll_xy ? roll_xy[0] : 0, roll_xy ? roll_xy[1] : 0,
                           y0, x0, th, tw, tile);
}

int stx_image_put_tile(stx_engine *e, float *grad, int H, int W, const int roll_xy[2], int y0,
                       int x0, int th, int tw, const float *tile_grad) {
    if (!e || !grad || !tile_grad || H <= 0 || W <= 0 || th <= 0 || tw <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return put_tile_launch(e->stream, grad, H, W, roll_xy ? roll_xy[0] : 0,
                           roll_xy ? roll_xy[1] : 0, y0, x0, th, tw, tile_grad);
}

int stx_image_mask_map(stx_engine *e, const float *mask, int H, int W, int scale, float *out) {
    if (!e || !mask || !out || H <= 0 || W <= 0 || scale <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return mask_map_launch(e->stream, mask, H, W, scale, out);
}

int stx_map_place(stx_engine *e, float *dst, int channels, int dst_h, int dst_w, int y0, int x0,
                  const float *src, int h, int w) {
    if (!e || !dst || !src || channels <= 0 || h <= 0 || w <= 0 || y0 < 0 || x0 < 0 ||
        y0 + h > dst_h || x0 + w > dst_w) {
        set_error("stx_map_place: window [%d+%d, %d+%d] does not fit a %dx%d map", y0, h, x0, w,
                  dst_h, dst_w);
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    return place_window_launch(e->stream, dst, dst_h, dst_w, y0, x0, src, channels, h, w);
}

int stx_map_roll_add(stx_engine *e, float *acc, const float *src, int channels, int h, int w,
                     const int roll_xy[2], double alpha, double init_divisor) {
    if (!e || !acc || !src || channels <= 0 || h <= 0 || w <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    const bool init = init_divisor != 0.0;
    return roll_add_launch(e->stream, acc, src, channels, h, w, roll_xy ? roll_xy[0] : 0,
                           roll_xy ? roll_xy[1] : 0, (float)(init ? init_divisor : alpha), init);
}

int stx_image_resample(stx_engine *e, const float *src, int channels, int H, int W, float *dst,
                       int out_h, int out_w, const int *bounds_x, const double *weights_x,
                       int ksize_x, const int *bounds_y, const double *weights_y, int ksize_y,
                       int clamp_min_zero) {
    if (!e || !src || !dst || !bounds_x || !weights_x || !bounds_y || !weights_y || channels <= 0 ||
        H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || ksize_x <= 0 || ksize_y <= 0)
        return STX_ERR_ARG;
    STX_TRY(e->set_device());
    // device scratch: [bounds_x | bounds_y] ints, [kx | ky] doubles, horizontal-pass image
    const size_t nbx = 2 * (size_t)out_w, nby = 2 * (size_t)out_h;
    const size_t nkx = (size_t)out_w * ksize_x, nky = (size_t)out_h * ksize_y;
    const size_t tmp_floats = (size_t)channels * H * out_w;
    const size_t k_off = ((nbx + nby) * sizeof(int) + 7) & ~(size_t)7;
    const size_t t_off = (k_off + (nkx + nky) * sizeof(double) + 255) & ~(size_t)255;
    STX_TRY(e->upload.ensure(t_off + tmp_floats * sizeof(float)));
    char *base = static_cast<char *>(e->upload.ptr);
    int *d_bx = reinterpret_cast<int *>(base), *d_by = d_bx + nbx;
    double *d_kx = reinterpret_cast<double *>(base + k_off), *d_ky = d_kx + nkx;
    float *tmp = reinterpret_cast<float *>(base + t_off);
    STX_HIP(hipMemcpyAsync(d_bx, bounds_x, nbx * sizeof(int), hipMemcpyHostToDevice, e->stream));
    STX_HIP(hipMemcpyAsync(d_by, bounds_y, nby * sizeof(int), hipMemcpyHostToDevice, e->stream));
    STX_HIP(hipMemcpyAsync(d_kx, weights_x, nkx * sizeof(double), hipMemcpyHostToDevice, e->stream));
    STX_HIP(hipMemcpyAsync(d_ky, weights_y, nky * sizeof(double), hipMemcpyHostToDevice, e->stream));
    // Pillow runs the horizontal pass first, then the vertical pass on its float32 result
    STX_TRY(resample_launch(e->stream, 0, src, channels, H, W, tmp, H, out_w, d_bx, d_kx, ksize_x, 0));
    STX_TRY(resample_launch(e->stream, 1, tmp, channels, H, out_w, dst, out_h, out_w, d_by, d_ky,
                            ksize_y, clamp_min_zero));
    // the coefficient tables are host memory of the caller: finish the copies before returning
    STX_HIP(hipStreamSynchronize(e->stream));
    return STX_OK;
}

// Queues n double-precision loss terms: `launch` enqueues the kernels that leave them at the device
// pointer it is handed, they are mirrored to the host arena, and at the next sync *loss_out becomes
// sum coefs[i] * term[i].
static int queue_dterms(stx_engine *e, const double *coefs, size_t n, double *loss_out,
                        const std::function<int(double *)> &launch) {
    size_t di;
    STX_TRY(alloc_dscalars(e, n, &di));
    double *terms = static_cast<double *>(e->A().dscalars.ptr) + di;
    STX_TRY(launch(terms));
    STX_HIP(hipMemcpyAsync(e->A().dhost + di, terms, n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    PendingLoss pl;
    pl.out = loss_out;
    for (size_t i = 0; i < n; ++i) pl.dterms.push_back(LossTerm{di + i, coefs[i]});
    e->A().pending.push_back(std::move(pl));
    return STX_OK;
}

static int queue_dterms(stx_engine *e, std::initializer_list<double> coefs, double *loss_out,
                        const std::function<int(double *)> &launch) {
    return queue_dterms(e, coefs.begin(), coefs.size(), loss_out, launch);
}

int stx_image_regularizers(stx_engine *e, const float *img, float *grad, int H, int W,
                           const float mean_bgr[3], double tv_scale, double tv_power, double p_scale,
                           double p_power, const float *aux, double aux_scale,
                           const int aux_roll_xy[2], double *loss_out) {
    if (!e || !img || !grad || !mean_bgr || H <= 0 || W <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return queue_dterms(e, {tv_scale, p_scale, aux ? aux_scale * 0.5 : 0.0}, loss_out, [&](double *terms) {
        return regularizers_launch(e->stream, img, grad, H, W, mean_bgr, (float)tv_scale,
                                   (float)tv_power, (float)p_scale, (float)p_power, aux,
                                   (float)aux_scale, aux_roll_xy ? aux_roll_xy[0] : 0,
                                   aux_roll_xy ? aux_roll_xy[1] : 0, terms, e->red_scratch.f(),
                                   e->red_scratch.bytes / sizeof(float));
    });
}

// ---- the SWT term (swt.hip): order 1 is Haar and goes to the Haar levels entry, one level of it to the
// one-level kernel, so that the three entries agree bit for bit where they overlap ----

// pywt.swt2 takes 1 to log2(padded side) levels
static int swt_check_levels(const char *name, int H, int W, int levels) {
    const int N = swt_padded_side(H, W);
    if (levels < 1 || levels > 30 || (1 << levels) > N) {
        set_error("%s: levels = %d, but a %d x %d image (padded side %d) takes 1 to %d levels", name,
                  levels, H, W, N, (int)std::lround(std::log2((double)N)));
        return STX_ERR_ARG;
    }
    return STX_OK;
}

// The scratch of the two separable passes: the row-filtered image and the column pass's partials.
static int swt_scratch_for(stx_engine *e, int H, int W, float **tmp, float **partials) {
    size_t tmp_floats, partial_floats;
    swt_levels_scratch(H, W, &tmp_floats, &partial_floats);
    // growing frees the old buffer, which waits for the kernels that still read it
    STX_TRY(e->swt_scratch.ensure((tmp_floats + partial_floats) * sizeof(float)));
    *tmp = e->swt_scratch.f();
    *partials = *tmp + tmp_floats;
    return STX_OK;
}

// The device copy of swt_daub_table(order, levels, N): built and uploaded at first use, then kept.
static int swt_table_for(stx_engine *e, int order, int levels, int N, const stx_engine::SwtTable **out) {
    for (const stx_engine::SwtTable &t : e->swt_tables)
        if (t.order == order && t.levels == levels && t.N == N) {
            *out = &t;
            return STX_OK;
        }
    std::vector<float> taps;
    int hl;
    swt_daub_table(order, levels, N, &taps, &hl);
    stx_engine::SwtTable t{order, levels, N, (int)taps.size(), hl, DevBuf()};
    STX_TRY(t.taps.ensure(taps.size() * sizeof(float)));
    // once per table and synchronous: the host copy does not outlive this call
    hipError_t err = hipMemcpy(t.taps.ptr, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        t.taps.release();
        set_error("stx_image_swt_daub_levels: hipMemcpy of %zu taps failed: %s", taps.size(),
                  hipGetErrorString(err));
        return STX_ERR_HIP;
    }
    e->swt_tables.push_back(t);
    *out = &e->swt_tables.back();
    return STX_OK;
}

int stx_image_swt_haar(stx_engine *e, const float *img, float *grad, int H, int W,
                       const int roll_xy[2], double scale, double power, double *loss_out) {
    if (!e || !img || !grad || H <= 0 || W <= 0 || power <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return queue_dterms(e, {scale}, loss_out, [&](double *term) {
        return swt_haar_launch(e->stream, img, grad, H, W, roll_xy ? roll_xy[0] : 0,
                               roll_xy ? roll_xy[1] : 0, (float)scale, (float)power, term,
                               e->red_scratch.f(), e->red_scratch.bytes / sizeof(float));
    });
}

int stx_image_swt_haar_levels(stx_engine *e, const float *img, float *grad, int H, int W, int levels,
                              const int roll_xy[2], double scale, double power, double *loss_out) {
    if (!e || !img || !grad || H <= 0 || W <= 0 || power <= 0) return STX_ERR_ARG;
    STX_TRY(swt_check_levels("stx_image_swt_haar_levels", H, W, levels));
    if (levels == 1) return stx_image_swt_haar(e, img, grad, H, W, roll_xy, scale, power, loss_out);
    STX_TRY(e->set_device());
    float *tmp, *partials;
    STX_TRY(swt_scratch_for(e, H, W, &tmp, &partials));
    return queue_dterms(e, {scale}, loss_out, [&](double *term) {
        return swt_haar_levels_launch(e->stream, img, grad, H, W, levels, roll_xy ? roll_xy[0] : 0,
                                      roll_xy ? roll_xy[1] : 0, (float)scale, (float)power, term, tmp,
                                      partials);
    });
}

int stx_image_swt_daub_levels(stx_engine *e, const float *img, float *grad, int H, int W, int order,
                              int levels, const int roll_xy[2], double scale, double power,
                              double *loss_out) {
    if (!e || !img || !grad || H <= 0 || W <= 0 || power <= 0) return STX_ERR_ARG;
    if (order < 1 || order > 38) {
        set_error("stx_image_swt_daub_levels: order = %d, but db1 to db38 exist", order);
        return STX_ERR_ARG;
    }
    if (order == 1)     // (the Haar entry checks the level count)
        return stx_image_swt_haar_levels(e, img, grad, H, W, levels, roll_xy, scale, power, loss_out);
    STX_TRY(swt_check_levels("stx_image_swt_daub_levels", H, W, levels));
    STX_TRY(e->set_device());
    const stx_engine::SwtTable *tab;
    STX_TRY(swt_table_for(e, order, levels, swt_padded_side(H, W), &tab));
    float *tmp, *partials;
    STX_TRY(swt_scratch_for(e, H, W, &tmp, &partials));
    return queue_dterms(e, {scale}, loss_out, [&](double *term) {
        return swt_table_launch(e->stream, img, grad, H, W, tab->taps.f(), tab->ntaps, tab->hl,
                                roll_xy ? roll_xy[0] : 0, roll_xy ? roll_xy[1] : 0, (float)scale,
                                (float)power, term, tmp, partials);
    });
}

// ---- the Laplacian loss (lap.hip) ----

// 1..4 distinct powers of two in 1..64; on success *lv describes the grids and *floats is their size
static int lap_check(const char *name, int H, int W, int n_pools, const int *pools, LapLevels *lv,
                     size_t *floats) {
    if (!pools) {
        set_error("%s: pools is null", name);
        return STX_ERR_ARG;
    }
    if (H <= 0 || W <= 0) {
        set_error("%s: a %d x %d picture", name, H, W);
        return STX_ERR_ARG;
    }
    if (n_pools < 1 || n_pools > kLapMaxPools) {
        set_error("%s: n_pools = %d, but 1 to %d pool sizes are taken", name, n_pools, kLapMaxPools);
        return STX_ERR_ARG;
    }
    for (int k = 0; k < n_pools; ++k) {
        const int p = pools[k];
        if (p < 1 || p > 64 || (p & (p - 1))) {
            set_error("%s: pool size %d is not a power of two in 1..64", name, p);
            return STX_ERR_ARG;
        }
        for (int j = 0; j < k; ++j)
            if (pools[j] == p) {
                set_error("%s: pool size %d is given twice", name, p);
                return STX_ERR_ARG;
            }
    }
    *floats = lap_levels(H, W, n_pools, pools, lv);
    if (*floats > (size_t)INT32_MAX) {
        set_error("%s: %zu cells on the pooled grids of a %d x %d picture (at most 2^31 - 1)", name, *floats,
                  H, W);
        return STX_ERR_ARG;
    }
    return STX_OK;
}

static int lap_scratch_for(stx_engine *e, size_t floats, float **scratch) {
    // growing frees the old buffer, which waits for the kernels that still read it
    STX_TRY(e->lap_scratch.ensure(lap_scratch_floats(floats) * sizeof(float)));
    *scratch = e->lap_scratch.f();
    return STX_OK;
}

size_t stx_image_lap_floats(int H, int W, int n_pools, const int *pools) {
    LapLevels lv;
    size_t floats;
    return lap_check("stx_image_lap_floats", H, W, n_pools, pools, &lv, &floats) == STX_OK ? floats : 0;
}

int stx_image_lap_target(stx_engine *e, const float *content, int H, int W, int n_pools, const int *pools,
                         float *target_out) {
    if (!e || !content || !target_out) {
        set_error("stx_image_lap_target: %s is null", !e ? "the engine" : !content ? "content" : "target_out");
        return STX_ERR_ARG;
    }
    LapLevels lv;
    size_t floats;
    STX_TRY(lap_check("stx_image_lap_target", H, W, n_pools, pools, &lv, &floats));
    STX_TRY(e->set_device());
    float *scratch;
    STX_TRY(lap_scratch_for(e, floats, &scratch));
    return lap_target_launch(e->stream, content, H, W, lv, target_out, scratch);
}

int stx_image_lap(stx_engine *e, const float *img, float *grad, int H, int W, int n_pools, const int *pools,
                  const double *weights, const float *target, double scale, double *loss_out) {
    if (!e || !img || !grad || !weights || !target || !loss_out) {
        set_error("stx_image_lap: %s is null", !e ? "the engine" : !img ? "img" : !grad ? "grad" :
                  !weights ? "weights" : !target ? "target" : "loss_out");
        return STX_ERR_ARG;
    }
    LapLevels lv;
    size_t floats;
    STX_TRY(lap_check("stx_image_lap", H, W, n_pools, pools, &lv, &floats));
    STX_TRY(e->set_device());
    float *scratch;
    STX_TRY(lap_scratch_for(e, floats, &scratch));
    // one loss term per pool size, sum e_p^2, with coefficient scale * w_p; the cells get 2 scale w_p (D e_p)
    double coefs[kLapMaxPools];
    float cell_coefs[kLapMaxPools];
    for (int k = 0; k < n_pools; ++k) {
        coefs[k] = scale * weights[k];
        cell_coefs[k] = (float)(2.0 * coefs[k]);
    }
    return queue_dterms(e, coefs, (size_t)n_pools, loss_out, [&](double *terms) {
        return lap_launch(e->stream, img, grad, H, W, lv, floats, cell_coefs, target, terms, scratch);
    });
}

// ---- the photorealism regulariser (photo.hip) ----

int stx_image_photo(stx_engine *e, const float *img, const float *content, float *grad, int H, int W,
                    double eps, double scale, double *loss_out) {
    if (!e || !img || !content || !grad || !loss_out) {
        set_error("stx_image_photo: %s is null", !e ? "the engine" : !img ? "img" : !content ? "content" :
                  !grad ? "grad" : "loss_out");
        return STX_ERR_ARG;
    }
    if (H < 3 || W < 3) {
        set_error("stx_image_photo: a %d x %d picture holds no 3 x 3 window", H, W);
        return STX_ERR_ARG;
    }
    if (!std::isfinite(eps) || !(eps > 0.0)) {
        set_error("stx_image_photo: eps = %g, but a finite positive value is needed", eps);
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    // (the engine's reduction scratch holds kBlocks floats and more: one partial per workgroup)
    return queue_dterms(e, {scale}, loss_out, [&](double *term) {
        return photo_launch(e->stream, img, content, grad, H, W, eps, scale, term, e->red_scratch.f());
    });
}

// ---- the temporal-consistency term (temporal.hip) ----

int stx_image_flow_warp(stx_engine *e, const float *prev, const float *flow_b, const float *flow_f, int H, int W,
                        double su, double sv, int first, float *target, float *weight) {
    if (!e || !prev || !flow_b || !target || !weight) {
        set_error("stx_image_flow_warp: %s is null", !e ? "the engine" : !prev ? "prev" : !flow_b ? "flow_b" :
                  !target ? "target" : "weight");
        return STX_ERR_ARG;
    }
    if (H < 2 || W < 2) {
        set_error("stx_image_flow_warp: a %d x %d picture holds no 2 x 2 taps", H, W);
        return STX_ERR_ARG;
    }
    if (!std::isfinite(su) || !std::isfinite(sv)) {
        set_error("stx_image_flow_warp: scale factors (%g, %g), but finite values are needed", su, sv);
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    return flow_warp_launch(e->stream, prev, flow_b, flow_f, H, W, su, sv, first, target, weight);
}

int stx_image_temporal(stx_engine *e, const float *img, float *grad, const float *target, const float *weight,
                       int H, int W, double scale, double *loss_out) {
    if (!e || !img || !grad || !target || !weight || !loss_out) {
        set_error("stx_image_temporal: %s is null", !e ? "the engine" : !img ? "img" : !grad ? "grad" :
                  !target ? "target" : !weight ? "weight" : "loss_out");
        return STX_ERR_ARG;
    }
    if (H <= 0 || W <= 0) {
        set_error("stx_image_temporal: a %d x %d picture", H, W);
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    // (the engine's reduction scratch holds kBlocks floats and more: one partial per workgroup)
    return queue_dterms(e, {scale * 63.75}, loss_out, [&](double *term) {
        return temporal_launch(e->stream, img, grad, target, weight, H, W, scale, term, e->red_scratch.f());
    });
}

// ---- the optical-flow estimator of --prev-contents (flow.hip) ----

int stx_image_flow_estimate(stx_engine *e, const float *I1, const float *I2, int H, int W,
                            const stx_flow_params *p, float *flow_out) {
    if (!e || !I1 || !I2 || !p || !flow_out) {
        set_error("stx_image_flow_estimate: %s is null", !e ? "the engine" : !I1 ? "I1" : !I2 ? "I2" :
                  !p ? "the parameters" : "flow_out");
        return STX_ERR_ARG;
    }
    if (H < 16 || W < 16 || H > 32768 || W > 32768) {
        set_error("stx_image_flow_estimate: a %d x %d picture, but sides from 16 to 32768 are needed", H, W);
        return STX_ERR_ARG;
    }
    const struct { const char *name; double value; bool ok; } reals[] = {
        {"alpha", p->alpha, p->alpha > 0},
        {"gamma", p->gamma, p->gamma >= 0},
        {"eta", p->eta, p->eta > 0.25 && p->eta < 0.95},
        {"omega", p->omega, p->omega > 0 && p->omega < 2},
        {"eps", p->eps, p->eps > 0},
    };
    for (const auto &r : reals)
        if (!std::isfinite(r.value) || !r.ok) {
            set_error("stx_image_flow_estimate: %s = %g, but %s is needed", r.name, r.value,
                      "alpha > 0, gamma >= 0, 0.25 < eta < 0.95, 0 < omega < 2, eps > 0, all finite");
            return STX_ERR_ARG;
        }
    const struct { const char *name; int value; } counts[] = {
        {"levels", p->levels}, {"outer", p->outer}, {"inner", p->inner}, {"sor", p->sor}};
    for (const auto &c : counts)
        if (c.value < 1) {
            set_error("stx_image_flow_estimate: %s = %d, but a count of at least 1 is needed", c.name, c.value);
            return STX_ERR_ARG;
        }
    STX_TRY(e->set_device());
    // The workspace is the engine's: it grows here if it has to and goes back at the next stx_sync, when the
    // launches queued here are done (engine.cpp, do_sync) -- the call itself waits for nothing.
    STX_TRY(e->flow_work.ensure(flow_workspace_doubles(H, W, p->eta, p->levels) * sizeof(double)));
    return flow_estimate_launch(e->stream, I1, I2, H, W, *p, flow_out, static_cast<double *>(e->flow_work.ptr));
}

// ---- the screened-Poisson output stage of --poisson-lambda (poisson.hip) ----

int stx_image_poisson(stx_engine *e, const float *img, const float *content, float *out, int H, int W,
                      double lambda, int cycles) {
    if (!e || !img || !content || !out) {
        set_error("stx_image_poisson: %s is null", !e ? "the engine" : !img ? "img" : !content ? "content" : "out");
        return STX_ERR_ARG;
    }
    if (H < 1 || W < 1 || H > 32768 || W > 32768) {
        set_error("stx_image_poisson: a %d x %d picture, but sides from 1 to 32768 are needed", H, W);
        return STX_ERR_ARG;
    }
    if (!std::isfinite(lambda) || !(lambda > 0.0) || lambda > 1000.0) {
        set_error("stx_image_poisson: lambda = %g, but a finite value above 0 and up to 1000 is needed", lambda);
        return STX_ERR_ARG;
    }
    if (cycles < 1 || cycles > 32) {
        set_error("stx_image_poisson: cycles = %d, but a count from 1 to 32 is needed", cycles);
        return STX_ERR_ARG;
    }
    const size_t n = 3 * (size_t)H * W;
    const auto overlaps = [&](const float *in) {
        return reinterpret_cast<uintptr_t>(out) < reinterpret_cast<uintptr_t>(in + n) &&
               reinterpret_cast<uintptr_t>(in) < reinterpret_cast<uintptr_t>(out + n);
    };
    if (overlaps(img) || overlaps(content)) {
        set_error("stx_image_poisson: out overlaps %s; a buffer of its own is needed", overlaps(img) ? "img" : "content");
        return STX_ERR_ARG;
    }
    STX_TRY(e->set_device());
    // The workspace is the engine's: it grows here if it has to and goes back at the next stx_sync, when the
    // launches queued here are done (engine.cpp, do_sync) -- the call itself waits for nothing.
    STX_TRY(e->poisson_work.ensure(poisson_workspace_doubles(H, W, lambda) * sizeof(double)));
    return poisson_launch(e->stream, img, content, out, H, W, lambda, cycles, static_cast<double *>(e->poisson_work.ptr));
}

int stx_adam_step(stx_engine *e, float *params, const float *grad, float *g1, float *g2, float *p1,
                  float *avg_out, size_t n, double lr, double b1, double b2, double bp1, double corr1,
                  double corr2, double corrp) {
    if (!e || !params || !grad || !g1 || !g2 || !p1 || !avg_out || !n) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return adam_launch(e->stream, params, grad, g1, g2, p1, avg_out, n, lr, b1, b2, bp1, corr1,
                       corr2, corrp);
}

static int sync_scalar(stx_engine *e, size_t di, int n, double *out) {
    STX_HIP(hipMemcpyAsync(e->A().dhost + di, static_cast<double *>(e->A().dscalars.ptr) + di,
                           n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    STX_HIP(hipStreamSynchronize(e->stream));
    for (int i = 0; i < n; ++i) out[i] = e->A().dhost[di + i];
    return STX_OK;
}

int stx_vec_dot(stx_engine *e, const float *x, const float *y, size_t n, double *out) {
    if (!e || !x || !y || !out || !n) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    const size_t di = e->dscalars_cap - 2;   // reserved slot for synchronous scalar results
    STX_TRY(dot_launch(e->stream, x, y, n, static_cast<double *>(e->A().dscalars.ptr) + di,
                       e->red_scratch.f(), e->red_scratch.bytes / sizeof(float)));
    return sync_scalar(e, di, 1, out);
}

int stx_vec_mean_abs(stx_engine *e, const float *x, size_t n, double *out) {
    if (!e || !x || !out || !n) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    const size_t di = e->dscalars_cap - 2;
    STX_TRY(abs_sum_launch(e->stream, x, n, static_cast<double *>(e->A().dscalars.ptr) + di,
                           e->red_scratch.f(), e->red_scratch.bytes / sizeof(float)));
    STX_TRY(sync_scalar(e, di, 1, out));
    *out /= (double)n;
    return STX_OK;
}

int stx_vec_dot_async(stx_engine *e, const float *x, const float *y, size_t n, double *out_dev) {
    if (!e || !x || !y || !out_dev || !n) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return dot_launch(e->stream, x, y, n, out_dev, e->red_scratch.f(),
                      e->red_scratch.bytes / sizeof(float));
}

int stx_vec_abs_sum_async(stx_engine *e, const float *x, size_t n, double *out_dev) {
    if (!e || !x || !out_dev || !n) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return abs_sum_launch(e->stream, x, n, out_dev, e->red_scratch.f(),
                          e->red_scratch.bytes / sizeof(float));
}

int stx_vec_axpy_dev(stx_engine *e, double c1, const double *a_dev, double da, double c2,
                     const double *b_dev, double db, const float *x, float *y, size_t n) {
    if (!e || !a_dev || !x || !y || !n || da == 0.0 || (b_dev && db == 0.0)) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return axpy_dev_launch(e->stream, c1, a_dev, da, c2, b_dev, db, x, y, n);
}

int stx_vec_scale_dev(stx_engine *e, double c, const double *den_dev, double den_div, float *x,
                      size_t n) {
    if (!e || !den_dev || !x || !n || den_div == 0.0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return scale_dev_launch(e->stream, c, den_dev, den_div, x, n);
}

int stx_vec_axpy_dot_dev(stx_engine *e, double c1, const double *a_dev, double da, double c2,
                         const double *b_dev, double db, double scale_c, const double *scale_den_dev,
                         double scale_div, const float *x, const float *src, float *y, const float *z,
                         size_t n, double *out_dev) {
    if (!e || !a_dev || !x || !src || !y || !z || !out_dev || !n || da == 0.0 || (b_dev && db == 0.0) ||
        (scale_den_dev && scale_div == 0.0))
        return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return axpy_dot_dev_launch(e->stream, c1, a_dev, da, c2, b_dev, db, scale_c, scale_den_dev, scale_div, x,
                               src, y, z, n, out_dev, e->red_scratch.f(), e->red_scratch.bytes / sizeof(float));
}

int stx_vec_lbfgs_pair(stx_engine *e, const float *g_new, float *g_old, const float *s, float *y, size_t n,
                       double *out_dev2, double *sy_host_sync) {
    if (!e || !g_new || !g_old || !s || !y || !out_dev2 || !sy_host_sync || !n) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    STX_TRY(lbfgs_pair_launch(e->stream, g_new, g_old, s, y, n, out_dev2, e->red_scratch.f(),
                              e->red_scratch.bytes / sizeof(float)));
    const size_t di = e->dscalars_cap - 2;   // the pinned mirror's slot for synchronous scalar results
    STX_HIP(hipMemcpyAsync(e->A().dhost + di, out_dev2, sizeof(double), hipMemcpyDeviceToHost, e->stream));
    STX_HIP(hipStreamSynchronize(e->stream));
    *sy_host_sync = e->A().dhost[di];
    return STX_OK;
}

int stx_vec_scale2_axpy(stx_engine *e, double c1, double c2, float *s, float *params, size_t n) {
    if (!e || !s || !params || !n) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return scale2_axpy_launch(e->stream, (float)c1, (float)c2, s, params, n);
}

int stx_vec_axpy(stx_engine *e, double a, const float *x, float *y, size_t n) {
    if (!e || !x || !y || !n) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return axpy_launch(e->stream, (float)a, x, y, n);
}

int stx_vec_scale(stx_engine *e, double a, float *x, size_t n) {
    if (!e || !x || !n) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return scale_launch(e->stream, (float)a, x, n);
}

int stx_image_step_stats(stx_engine *e, const float *avg, float *old, int H, int W, double stats[2]) {
    if (!e || !avg || !old || !stats || H <= 0 || W <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    const size_t di = e->dscalars_cap - 2;
    STX_TRY(step_stats_launch(e->stream, avg, old, H, W, static_cast<double *>(e->A().dscalars.ptr) + di,
                              e->red_scratch.f(), e->red_scratch.bytes / sizeof(float)));
    double raw[2];
    STX_TRY(sync_scalar(e, di, 2, raw));
    const double n = 3.0 * H * W;
    stats[0] = raw[0] / n;
    stats[1] = std::sqrt(raw[1] / n);
    return STX_OK;
}

int stx_image_step_stats_async(stx_engine *e, const float *avg, float *old, int H, int W,
                               double raw_sums[2]) {
    if (!e || !avg || !old || !raw_sums || H <= 0 || W <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    size_t di;
    STX_TRY(alloc_dscalars(e, 2, &di));
    double *dev = static_cast<double *>(e->A().dscalars.ptr) + di;
    STX_TRY(step_stats_launch(e->stream, avg, old, H, W, dev, e->red_scratch.f(),
                              e->red_scratch.bytes / sizeof(float)));
    STX_HIP(hipMemcpyAsync(e->A().dhost + di, dev, 2 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    for (int i = 0; i < 2; ++i) {
        PendingLoss pl;
        pl.out = raw_sums + i;
        pl.dterms.push_back(LossTerm{di + (size_t)i, 1.0});
        e->A().pending.push_back(std::move(pl));
    }
    return STX_OK;
}

int stx_image_to_u8(stx_engine *e, const float *img, int H, int W, const float mean_bgr[3],
                    uint8_t *out_rgb_u8) {
    if (!e || !img || !mean_bgr || !out_rgb_u8 || H <= 0 || W <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return to_u8_launch(e->stream, img, H, W, mean_bgr, out_rgb_u8);
}

int stx_image_to_u8_luma(stx_engine *e, const float *img, const float *content, int H, int W,
                         const float mean_bgr[3], uint8_t *out_rgb_u8) {
    if (!e || !img || !content || !mean_bgr || !out_rgb_u8 || H <= 0 || W <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return to_u8_luma_launch(e->stream, img, content, H, W, mean_bgr, out_rgb_u8);
}

int stx_image_color_stats(stx_engine *e, const float *img, int H, int W, double out_host_sync[9]) {
    if (!e || !img || !out_host_sync || H <= 0 || W <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    STX_TRY(e->color_sums.ensure(9 * sizeof(double)));
    double *dev = static_cast<double *>(e->color_sums.ptr);
    STX_TRY(color_stats_launch(e->stream, img, H, W, dev, e->red_scratch.f(),
                               e->red_scratch.bytes / sizeof(float)));
    STX_HIP(hipMemcpyAsync(out_host_sync, dev, 9 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    STX_HIP(hipStreamSynchronize(e->stream));
    return STX_OK;
}

int stx_image_color_affine(stx_engine *e, const float *src, float *dst, int H, int W, const double A[9],
                           const double b[3], const float mean_bgr[3]) {
    if (!e || !src || !dst || !A || !b || !mean_bgr || H <= 0 || W <= 0) return STX_ERR_ARG;
    STX_TRY(e->set_device());
    return color_affine_launch(e->stream, src, dst, H, W, A, b, mean_bgr);
}

}  // extern "C"
