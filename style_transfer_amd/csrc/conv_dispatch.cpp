// The packed-weight convolutions by kernel family (common.h: ConvFamily): the choice of a configuration, its
// filter bank, its launch and its capabilities.  The one place that dispatches on the family; host code only.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "common.h"

namespace stx {

// The fp16-split kernel (conv_h2.hip) for this problem?  By shape and epilogue only -- never by timing:
// it rounds differently from the fp32 kernels, and a given shape must always take the same path.
//   forward: layers with at least STX_CONV_H2 input channels (default 64; 0: never);
//   backward: at least STX_CONV_H2_BWD channels of incoming gradient (default 64).
// A forward blob that differs in its last bits flips ReLU / max-pooling near-ties, and the two 64-channel
// layers hold most of a tile's decisions.  Every bound of tests/ holds with them on this kernel; the one
// chaotic fixture -- the reference's L-BFGS run of BASELINE config 4 in miniature, tiles of 30 x 33 pixels
// -- follows another of the REFERENCE'S OWN branches (tests/golden/cfg4_sensitivity.py: the reference with
// its convolutions rounded at this level takes that branch in half of its runs).
// The backward pass decides nothing: its rounding moves the gradient by 1e-7 and no further.
// STX_CONV_ALGO=h2|h2a|h2b|h2c forces the kernel (any / the 64- / the 128-channel / the two-patch tiling)
// wherever it applies.
// (with STX_CONV_H2=0 and no STX_CONV_H2_BWD neither direction takes the kernel)
static int h2_min_k(bool forward) {
    const char *env = sw_env("STX_CONV_H2"), *envb = sw_env("STX_CONV_H2_BWD");
    return forward ? (env ? atoi(env) : 64) : envb ? atoi(envb) : env && atoi(env) <= 0 ? 0 : 64;
}

bool conv_h2_enabled() {
    const char *algo = sw_env("STX_CONV_ALGO");
    if (algo && *algo) return !strncmp(algo, "h2", 2);
    return h2_min_k(true) > 0 || h2_min_k(false) > 0;
}

static bool h2_choice(const ConvProblem &p, ConvConfig *out) {
    const char *algo = sw_env("STX_CONV_ALGO");
    int force = 0;
    if (algo && *algo) {
        if (!strcmp(algo, "h2")) force = 4;
        else if (!strcmp(algo, "h2a")) force = 1;
        else if (!strcmp(algo, "h2b")) force = 2;
        else if (!strcmp(algo, "h2c")) force = 3;
        else return false;             // some other kernel family was asked for
    }
    const int min_k = h2_min_k(p.epilogue == kEpiForward);
    if (!force && (min_k <= 0 || p.K < min_k || p.M < 64)) return false;
    if (!h2_usable(p)) return false;
    *out = force == 1 ? h2_config(1) : force == 2 ? h2_config(2) : force == 3 ? h2_config(1, 2) : h2_pick_config(p);
    return true;
}

// 3x3 layers with more than 32 output channels that the fp16-split kernel does not take (h2_choice) run the
// fp32 2-D Winograd kernel F(2x2,3x3) (4/9 of the direct kernel's MFMAs); everything else the direct kernel.
// The choice depends on the shape only, never on timing: the rounding differs between the kernels, and a
// given shape must always take the same path.  STX_CONV_ALGO=direct|wino2|wino2a|wino2b|wino2c overrides it
// for tests and measurements (a / b / c: one patch geometry only).
static bool wino_choice(const ConvProblem &p, bool winograd, ConvConfig *out) {
    if (p.ksize != 3 || p.K < 8 || p.M <= 4) return false;
    const char *algo = sw_env("STX_CONV_ALGO");
    if (algo && *algo) {
        if (!strcmp(algo, "direct")) return false;
        if (!strcmp(algo, "wino2")) { *out = wino2_config(wino2_pick_geometry(p.H, p.W)); return true; }
        if (!strcmp(algo, "wino2a")) { *out = wino2_config(0); return true; }   // one geometry only
        if (!strcmp(algo, "wino2b")) { *out = wino2_config(1); return true; }
        if (!strcmp(algo, "wino2c")) { *out = wino2_config(2); return true; }
    }
    if (!winograd || p.M <= 32) return false;
    *out = wino2_config(wino2_pick_geometry(p.H, p.W));
    return true;
}

// All direct configurations accumulate k in the same order, so they produce bit-identical results; which
// one is fastest depends on how many workgroups the plane yields (co-resident workgroups hide each other's
// stage swaps and epilogues).  The first time a shape is seen every candidate is timed with HIP events on
// the tuner's stream (a few launches, once per shape and scale) and the winner is cached.  The cache is
// shared by all engines of the process (several engines drive the same GPU as separate streams; they must
// agree, and later ones need not re-measure).  Key: device + shape.
static std::mutex g_tuned_mutex;
static std::map<std::vector<int>, int> g_tuned;

static int direct_tune(const ConvTuner &t, ConvProblem p, ConvConfig *out) {
    if (p.ksize != 3 || p.K <= 4 || p.M <= 32) return STX_OK;
    // planes too small to fill the chip run the small-tile config with a K split that depends on
    // the shape only (split results differ in rounding from unsplit ones, so no timing here)
    if (conv_splitk_factor(*out, p) > 1 || conv_num_workgroups(conv_config_by_id(5), p.M, p.H, p.W) < 256)
        return STX_OK;
    const std::vector<int> key = {t.device, p.ksize, p.K, p.M, p.H, p.W, p.epilogue};
    {
        std::lock_guard<std::mutex> lock(g_tuned_mutex);
        auto it = g_tuned.find(key);
        if (it != g_tuned.end()) {
            *out = conv_config_by_id(it->second);
            return STX_OK;
        }
    }
    const int candidates[] = {0, 1, 2, 5};
    float best_ms = 1e30f;
    int best = out->id;
    for (int id : candidates) {
        const ConvConfig cfg = conv_config_by_id(id);
        if (cfg.bm > 64 && p.M <= 64) continue;            // half-empty channel tiles
        STX_TRY(t.bank(cfg, &p.w));
        STX_TRY(conv_launch(t.stream, cfg, p, true));     // warm (also builds nothing lazily)
        STX_HIP(hipEventRecord(t.ev0, t.stream));
        for (int r = 0; r < 2; ++r) STX_TRY(conv_launch(t.stream, cfg, p, true));
        STX_HIP(hipEventRecord(t.ev1, t.stream));
        STX_HIP(hipEventSynchronize(t.ev1));
        float ms = 0.f;
        STX_HIP(hipEventElapsedTime(&ms, t.ev0, t.ev1));
        if (ms < best_ms) {
            best_ms = ms;
            best = id;
        }
    }
    {
        std::lock_guard<std::mutex> lock(g_tuned_mutex);
        g_tuned[key] = best;
    }
    *out = conv_config_by_id(best);
    return STX_OK;
}

int conv_choose(const ConvProblem &p, bool winograd, const ConvTuner *tuner, ConvConfig *out) {
    if (h2_choice(p, out) || wino_choice(p, winograd, out)) return STX_OK;
    *out = conv_pick_config(p.ksize, p.K, p.M, p.H, p.W);
    return tuner ? direct_tune(*tuner, p, out) : STX_OK;
}

// Bank keys: dir * 1024 + the direct variant's id, or the slot the configurations of a Winograd family share.
enum { kSlotWino2 = 256, kSlotH2 = 512, kSlotSmall = 768 };

ConvBank conv_bank(const ConvConfig &cfg, int dir, int Mo, int Ko, int ks) {
    const int M = dir ? Ko : Mo, K = dir ? Mo : Ko;
    switch (cfg.family) {
        case ConvFamily::Direct:
            return {dir * 1024 + cfg.id, conv_packed_floats(cfg, K, M, ks),
                    [=](hipStream_t s, const float *w, float *out) { return conv_pack_weights(s, w, Mo, Ko, ks, dir, cfg, out); }};
        case ConvFamily::Wino2:
            return {dir * 1024 + kSlotWino2, wino2_packed_floats(K, M),
                    [=](hipStream_t s, const float *w, float *out) { return wino2_pack_weights(s, w, Mo, Ko, dir, out); }};
        case ConvFamily::H2:
            return {dir * 1024 + kSlotH2, h2_packed_floats(K, M),
                    [=](hipStream_t s, const float *w, float *out) { return h2_pack_weights(s, w, Mo, Ko, dir, out); }};
    }
    return {};
}

ConvBank conv_small_bank(int Mo, int Ko) {
    return {1024 + kSlotSmall, conv_small_packed_floats(Mo),
            [=](hipStream_t s, const float *w, float *out) { return conv_small_pack(s, w, Mo, Ko, 1, out); }};
}

// ------------------------------------------------------------------------------------------------
// Launch and capabilities
// ------------------------------------------------------------------------------------------------

int conv_dispatch(hipStream_t s, const ConvConfig &cfg, const ConvProblem &p, double *flop_algorithmic,
                  double *flop_issued) {
    const double direct = 2.0 * p.M * p.K * p.ksize * p.ksize * (double)p.H * p.W;
    *flop_algorithmic += direct;
    switch (cfg.family) {
        case ConvFamily::Direct:
            *flop_issued += direct;
            return conv_launch(s, cfg, p, true);
        case ConvFamily::Wino2:
            *flop_issued += direct * 4.0 / 9.0;
            return wino2_launch(s, cfg, p, conv_splitk_factor(cfg, p));
        case ConvFamily::H2:   // 6 of 9 multiplies, each as three fp16 products of 1/16 of an fp32 MFMA's time per k
            *flop_issued += direct * (6.0 / 9.0) * (3.0 / 16.0);
            return h2_launch(s, cfg, p, conv_splitk_factor(cfg, p));
    }
    return STX_ERR_ARG;
}

int conv_splitk_factor(const ConvConfig &cfg, const ConvProblem &p) {
    if (p.ksize != 3 || (p.epilogue != kEpiForward && p.epilogue != kEpiDgrad)) return 1;
    return cfg.family == ConvFamily::Wino2 ? wino2_splitk_factor(cfg, p)
           : cfg.family == ConvFamily::H2  ? h2_splitk_factor(cfg, p)
                                           : direct_splitk_factor(cfg, p, true);
}

size_t conv_splitk_floats(const ConvConfig &cfg, const ConvProblem &p) {
    int f = conv_splitk_factor(cfg, p);
    if (cfg.family == ConvFamily::Wino2 && p.ksize == 3)     // (the tail split's slices are whole planes too)
        f = std::max(f, wino2_max_slices(cfg, p));
    return f > 1 ? (size_t)f * p.M * p.H * p.W : 0;
}

// stx_clock_marks: the Winograd kernels time the chunk loop of one of their workgroups
bool conv_takes_clock(const ConvConfig &cfg) { return cfg.family != ConvFamily::Direct; }

// (STX_POOL_FWD_FUSE=0: the stand-alone pooling kernel everywhere, for A/B measurements and tests)
bool conv_fuses_pool(const ConvConfig &cfg, const ConvProblem &p) {
    const char *env = sw_env("STX_POOL_FWD_FUSE");
    if ((env && atoi(env) == 0) || cfg.family == ConvFamily::Direct || conv_splitk_factor(cfg, p) != 1) return false;
    return cfg.family == ConvFamily::H2 ? h2_fuses_pool(p) : wino2_fuses_pool(p);
}

bool conv_writes_pool_codes(const ConvConfig &cfg) { return cfg.family != ConvFamily::Direct; }

bool conv_reads_x_amax(const ConvConfig &cfg) { return cfg.family == ConvFamily::H2; }

// the eight-wave fp32 kernel leaves its output's maximum too, wherever the fp16-split kernel may read it
bool conv_leaves_y_amax(const ConvConfig &cfg) {
    return cfg.family == ConvFamily::H2 || (cfg.family == ConvFamily::Wino2 && conv_h2_enabled());
}

bool conv_takes_inject(const ConvConfig &cfg) { return cfg.family != ConvFamily::Direct || direct_takes_inject(cfg); }

bool conv_takes_pooled_input(const ConvConfig &cfg, const ConvProblem &p) {
    return cfg.family == ConvFamily::H2 && h2_takes_pooled_input(cfg, p);
}

bool conv_uses_relu_codes(const ConvConfig &cfg, const ConvProblem &p, int ksplit) {
    return cfg.family == ConvFamily::Wino2 && wino2_uses_relu_codes(p, ksplit);
}

// The unsplit eight-wave fp32 kernel and the unsplit fp16-split kernel leave the sign nibbles of their
// (rectified) output.  STX_RELU_CODES=0: nowhere.
bool conv_writes_out_codes(const ConvConfig &cfg, const ConvProblem &p, int ksplit) {
    const char *env = sw_env("STX_RELU_CODES");
    if ((env && atoi(env) == 0) || cfg.family == ConvFamily::Direct) return false;
    if (p.epilogue != kEpiForward || !p.relu || !p.out_codes || ksplit > 1) return false;
    return cfg.family == ConvFamily::H2 || wino2_writes_out_codes(cfg, p);
}

}  // namespace stx
