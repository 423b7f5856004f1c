// Internal declarations shared by the libstx translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include <cstdarg>
#include <cstdio>
#include <functional>
#include <string>

#include "stx.h"

namespace stx {

// float32 machine epsilon: num_utils.py:14 (EPS), used by normalize / tv_norm / Adam.
constexpr float kEps = 1.1920928955078125e-07f;

void set_error(const char *fmt, ...);

// The library's STX_* switches (A/B levers and test hooks: INTEGRATION.md lists them).  They are read from a
// SNAPSHOT of the process environment -- taken when the library is first asked for one and again at every
// stx_reread_env() -- never with getenv() at a call site: the launch paths run on several host threads (one per
// engine of a farm), and getenv() beside a setenv() of the host program is a data race.  A caller that changes a
// switch inside a process (the tests do, bench.py's fp32 leg does) calls stx_reread_env() afterwards.  Returns
// the value or null, like getenv(); the pointer stays valid for the life of the process.
const char *sw_env(const char *name);
void sw_reread();

#define STX_HIP(call)                                                                       \
    do {                                                                                    \
        hipError_t err__ = (call);                                                          \
        if (err__ != hipSuccess) {                                                          \
            ::stx::set_error("%s:%d: %s failed: %s", __FILE__, __LINE__, #call,            \
                             hipGetErrorString(err__));                                     \
            return STX_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

#define STX_CHECK_LAUNCH()                                                                  \
    do {                                                                                    \
        hipError_t err__ = hipGetLastError();                                               \
        if (err__ != hipSuccess) {                                                          \
            ::stx::set_error("%s:%d: kernel launch failed: %s", __FILE__, __LINE__,        \
                             hipGetErrorString(err__));                                     \
            return STX_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

#define STX_TRY(expr)                                                                       \
    do {                                                                                    \
        int rc__ = (expr);                                                                  \
        if (rc__ != STX_OK) return rc__;                                                    \
    } while (0)

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int pooled_len(int n) { return n >= 2 ? (n - 2 + 1) / 2 + 1 : 1; }  // ceil((n-2)/2)+1
// Workgroups of a grid-stride reduction over n elements (image_ops.hip, swt.hip): at most kBlocks,
// which the engine's reduction scratch is sized for.
constexpr int kBlocks = 1024;
inline int blocks_for(size_t n) {
    const size_t b = (n + 255) / 256;
    return b < (size_t)kBlocks ? (int)b : kBlocks;
}
#ifdef __HIPCC__
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Block-reduces up to NV values (256 threads) and writes partials[v * gridDim.x + blockIdx.x].
template <int NV>
__device__ __forceinline__ void block_partials(float (&v)[NV], float *partials) {
    __shared__ float red[NV][4];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const float s = wave_sum_f(v[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k)
            partials[k * gridDim.x + blockIdx.x] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
    }
}

// Window codes of the 2x2/2 pooling (pool.hip): what the backward pass needs to know about a window.
// MAX: index of the FIRST maximum in row-major order (strict '>' scan, as Caffe's) | 4 if it is > 0.
__device__ __forceinline__ unsigned pool_max_code(float v00, float v01, float v10, float v11, bool hx,
                                                  bool hy) {
    unsigned arg = 0;
    float best = v00;
    if (hx && v01 > best) best = v01, arg = 1;
    if (hy && v10 > best) best = v10, arg = 2;
    if (hx && hy && v11 > best) best = v11, arg = 3;
    return arg | (best > 0.f ? 4u : 0u);
}
// AVE: bit k set if element k of the window is > 0 (the ReLU mask of the blob below).
__device__ __forceinline__ unsigned pool_ave_code(float v00, float v01, float v10, float v11, bool hx,
                                                  bool hy) {
    return (v00 > 0.f ? 1u : 0u) | (hx && v01 > 0.f ? 2u : 0u) | (hy && v10 > 0.f ? 4u : 0u) |
           (hx && hy && v11 > 0.f ? 8u : 0u);
}
#endif

// ------------------------------------------------------------------------------------------------
// Kernel launchers (each enqueues on `stream` and returns STX_OK / STX_ERR_*).
// ------------------------------------------------------------------------------------------------

// Epilogue selection for the implicit-GEMM MFMA kernel.
enum ConvEpilogue {
    kEpiForward = 0,      // y = [relu](acc + bias)
    kEpiDgrad = 1,        // y = acc * (mask > 0)      (mask optional)
    kEpiSymm = 2,         // y = acc, plus per-workgroup sum|y| partials
    kEpiDgradInject = 3,  // kEpiDgrad plus the loss-gradient terms of the produced blob (internal)
    kEpiPartial = 4       // raw accumulators of one K slice (split-K, internal)
};

struct ContentWindow {
    int C, fh, fw;          // tile feature size
    int ch, cw;             // full content map size
    int oy, ox;             // window origin in the rolled map
    int sy, sx;             // roll shifts (rows, cols)
};

// Loss-gradient terms added by the backward-data epilogue to the gradient it produces (the
// reference's saxpy(lw*w, normalize(x), diff[layer]), style_transfer.py:580,592-593):
//   y += c_coef / (c_sums[1]/n + EPS) * (feat - content[window])     (content term, first)
//   y += s_coef / (s_abs_sum[0]/n + EPS) * sgrad                     (style term)
struct ConvInject {
    const float *sgrad = nullptr, *s_abs_sum = nullptr;
    float s_coef = 0.f;
    const float *content = nullptr, *c_sums = nullptr, *feat = nullptr;
    float c_coef = 0.f;
    ContentWindow win{};
};

struct ConvProblem {
    const float *x;        // [K][H][W] input planes (activations or upstream gradient)
    const float *w;        // weight rows, see conv_mfma.hip (packed tiles or a dense symmetric matrix)
    float *y;              // [M][H][W]
    const float *bias;     // kEpiForward: [M] or null
    const float *mask;     // kEpiDgrad: [M][H][W] post-ReLU data of the output blob, or null
    float *partials;       // kEpiSymm: one float per workgroup
    int K, M, H, W;        // reduction channels, output channels, plane size
    int ksize;             // 3 (pad 1) or 1 (pad 0)
    int relu;              // kEpiForward
    int epilogue;
    ConvInject inject;     // kEpiDgrad, optional
    unsigned char *pool_codes = nullptr;   // with pool_out: one window code per pooled element (pool.hip)
    // ReLU sign nibbles of a [C][H][W] blob, one byte per 2x2 window ([C][ceil(H/2)][ceil(W/2)],
    // bit 2*dy+dx = element (2y+dy, 2x+dx) > 0).  kEpiForward: in_codes (optional) receives the
    // nibbles of the INPUT planes x -- the forward pass of the layer that consumes a rectified blob
    // writes them as a by-product of staging its patches; kEpiDgrad: mask_codes (optional) replaces
    // the fp32 `mask` array, 1 byte instead of 16 per lane and channel.  Kernels that cannot use
    // them ignore them (conv_uses_relu_codes).
    unsigned char *in_codes = nullptr;
    const unsigned char *mask_codes = nullptr;
    // kEpiForward with relu: out_codes (optional) receives the nibbles of the OUTPUT planes y -- the
    // producer's epilogue holds exactly one 2x2 window per lane and channel (round 5: the fp16-split
    // kernel and the eight-wave fp32 kernel; unsplit launches only: conv_writes_out_codes)
    unsigned char *out_codes = nullptr;
    // the caller attaches ReLU nibbles to this launch wherever the kernel takes them (it does not under
    // STX_WINO_BIG=1, for one): launches that want them keep out of the tail split either way, so
    // that the schedule -- and with it the rounding -- does not depend on whether they were taken
    bool wants_codes = false;
    // kEpiForward with a fused pooling that also writes window codes: nobody will read y itself
    // (the pooled blob feeds the next layer, the backward pooling runs from the codes) -- skip
    // its stores.  Only honoured by the kernels that fuse (conv_fuses_pool); ignored otherwise.
    bool skip_y = false;
    float *pool_out = nullptr;       // kEpiForward: also write the 2x2/2 ceil-mode pooling of y here
    int pool_mode = 0;               // (kernels that cannot do it leave it to the caller: see
                                     // conv_fuses_pool)
    float *splitk_ws = nullptr;      // scratch for split-K partial sums (optional)
    size_t splitk_ws_floats = 0;
    // stx_clock_marks: one workgroup of the launch (the eight-wave Winograd kernel only) stores
    // {core-clock cycles, 100 MHz ticks} spent in its chunk loop here -- the shader clock the part
    // sustains INSIDE the kernel that does 80 % of the work (null: nothing is read or stored)
    long long *clock_out = nullptr;
    // conv_h2.hip (fp16 two-piece split): max |x| of the input planes as kAmaxSlots words of float
    // bits (the largest one counts), left by the kernel that wrote them or by absmax_launch; y_amax
    // (optional, zeroed by the caller): where this launch leaves max |y| of its own output
    const unsigned *x_amax = nullptr;
    unsigned *y_amax = nullptr;
    // kEpiDgrad, conv_h2.hip only (h2_takes_pooled_input): the upstream gradient arrives as the gradient
    // of a 2x2/2 pooling layer's OUTPUT -- x is [K][ceil(H/2)][ceil(W/2)] -- together with that layer's
    // window codes (pool.hip; the array must be readable 3 bytes past its end).  The patch staging
    // routes / spreads it exactly as pool_bwd_codes_kernel would have: the gradient of the pooling
    // layer's input (four times the size) is never written or read.
    const unsigned char *pin_codes = nullptr;
    int pin_mode = 0;            // STX_POOL_MAX / STX_POOL_AVE
    bool pin_mask = false;       // the blob under the pooling layer is rectified (the codes carry its signs)
    // conv_h2.hip (optional): receives the specialised body of the injecting epilogue that the launch took
    // (h2_variant's code), or 0 -- written by h2_launch where it picks the kernel
    int *variant_out = nullptr;
#ifdef STX_EXPERIMENT_BF3
    const void *x_split = nullptr;   // tools/experiments/conv_bf3.hip only
#endif
};

// The kernel families of the packed-weight 3x3 / 1x1 convolutions: the direct implicit GEMM (conv_mfma.hip),
// the fp32 2-D Winograd F(2x2,3x3) (conv_wino2.hip) and the fp16-split 1-D Winograd F(2,3) (conv_h2.hip).
// conv_dispatch.cpp is the one place that dispatches on the family.
enum class ConvFamily { Direct, Wino2, H2 };

// Tile configuration chosen for a problem; weights must be packed for the same configuration (conv_bank).
struct ConvConfig {
    ConvFamily family;
    int id;        // the variant within its family (direct: index into the instantiation table)
    int bm;        // output channels per workgroup
    int kc;        // reduction channels per LDS stage
    int pr, pc;    // pixel tile rows x cols
    int threads;
    size_t lds_bytes;
};

ConvConfig conv_pick_config(int ksize, int K, int M, int H, int W);
ConvConfig conv_config_by_id(int id);
bool direct_takes_inject(const ConvConfig &cfg);     // kEpiDgradInject is instantiated for it
int conv_num_workgroups(const ConvConfig &cfg, int M, int H, int W);
// Packed weight buffer size (floats) for a [M][K][ks][ks] filter bank under cfg.
size_t conv_packed_floats(const ConvConfig &cfg, int K, int M, int ksize);
// Packs Caffe-layout weights w[Mo][Ko][ks][ks] (device) into the kernel's tile layout.
// transpose_flip = 0: forward (M = Mo, K = Ko).  1: backward-data (M = Ko, K = Mo, taps rotated 180).
int conv_pack_weights(hipStream_t s, const float *w_caffe, int Mo, int Ko, int ksize,
                      int transpose_flip, const ConvConfig &cfg, float *packed);
int conv_launch(hipStream_t s, const ConvConfig &cfg, const ConvProblem &p, bool packed_weights);
// Number of K slices conv_launch will use for this problem (1 = no split).  Small planes yield fewer
// workgroups than the chip has CUs; slicing the reduction over several workgroups and adding the slices
// in a fixed order fills the machine.
int direct_splitk_factor(const ConvConfig &cfg, const ConvProblem &p, bool packed_weights);

int splitk_reduce_launch(hipStream_t s, const ConvProblem &p, int ksplit);
// The same for the work items item_base .. item_base + items - 1 of a 2-D Winograd launch only (64
// channels x one pr x pc pixel patch each, in the kernel's own item order): conv_wino2's tail split.
int splitk_reduce_items_launch(hipStream_t s, const ConvProblem &p, const ConvConfig &cfg, int slices,
                               int item_base, int items);
// Work item lt of a 2-D Winograd launch -> (pixel patch, channel tile); conv_wino2.hip's order.
__host__ __device__ inline void wino2_item_tiles(int lt, int m_tiles, int n_patches, int &pt, int &mt) {
    pt = lt / m_tiles;
    mt = lt - pt * m_tiles;
    if (m_tiles == 8 && (n_patches & 7) == 0) {
        const int g = lt >> 5, r = lt & 31;
        mt = (g & 1) * 4 + (r & 3);
        pt = (g >> 1) * 8 + (r >> 2);
    }
}

// Kernel arguments shared by the Winograd kernels.
struct WinoArgs {
    const float *x;
    const float *w;        // transformed filter bank in the kernel's own tile layout
    float *y;
    const float *bias;
    const float *mask;
    int K, M, H, W;
    int n_chunks, tiles_x, tiles_y, m_tiles, ksplit;
    int w_tile_stride;     // floats between consecutive output-channel tiles
    int x_bytes, w_bytes;
    int relu;
    ConvInject inj;
    float *pool_out;       // forward only: 2x2/2 pooling of the output, or null
    int pool_mode;
    unsigned char *pool_codes;   // with pool_out: window codes for the backward pass, or null
    int skip_y = 0;                             // forward + fused pooling with codes: y is not stored
    unsigned char *out_codes = nullptr;         // forward: ReLU nibbles of y to write (ConvProblem)
    unsigned char *in_codes = nullptr;          // forward: ReLU nibbles of x to write (ConvProblem)
    const unsigned char *mask_codes = nullptr;  // backward: ReLU nibbles of the output blob to read
    long long *clock_out = nullptr;             // ConvProblem::clock_out
    int item_base = 0;                          // conv_wino2, K slices: first work item of the launch (tail split)
    const unsigned *x_amax = nullptr;           // conv_h2: ConvProblem::x_amax / y_amax
    unsigned *y_amax = nullptr;
    const unsigned char *pin_codes = nullptr;   // conv_h2: ConvProblem::pin_codes / pin_mode / pin_mask
    int pin_mode = 0, pin_mask = 0;
#ifdef STX_EXPERIMENT_BF3
    int vp_rows = 0, vp_tp = 0;                 // tools/experiments/conv_bf3.hip only
#endif
};

// First layer (at most 3 planes -> 64 channels, 3x3) with the Gram partials of its own output
// (conv_first.hip).  gram_partials (or null): conv_first_workgroups(H, W) partial tiles of 64 x 64
// floats, finished by gram_finish_launch with {C 64, HW, splits = that count, tiles 1, parts 1}.
bool conv_first_usable(int K, int M, int ksize);
int conv_first_workgroups(int H, int W);
int conv_first_launch(hipStream_t s, const float *x, const float *w_caffe, const float *bias, float *y,
                      int K, int H, int W, int relu, float *gram_partials, unsigned *y_amax = nullptr);

// 2-D Winograd F(2x2,3x3) (conv_wino2.hip); the config id is the patch geometry.
ConvConfig wino2_config(int geometry = 0);     // 0: 4 x 64 pixel patches, 1: 16 x 16, 2: 8 x 32
int wino2_pick_geometry(int H, int W);
size_t wino2_packed_floats(int K, int M);
int wino2_pack_weights(hipStream_t s, const float *w_caffe, int Mo, int Ko, int transpose_flip,
                       float *packed);
int wino2_launch(hipStream_t s, const ConvConfig &cfg, const ConvProblem &p, int ksplit);
bool wino2_fuses_pool(const ConvProblem &p);
bool wino2_uses_relu_codes(const ConvProblem &p, int ksplit);           // see conv_uses_relu_codes
bool wino2_writes_out_codes(const ConvConfig &cfg, const ConvProblem &p);   // see conv_writes_out_codes
int wino2_splitk_factor(const ConvConfig &cfg, const ConvProblem &p);
// Tail split: a launch of n = 256 q + r work items (q >= 1) runs its last r items as r x slices K
// slices -- one short round instead of a mostly empty full one -- and a reduce pass over those r
// patches only.  {0, 1}: not for this problem.  Shape and epilogue only, like the K split.
struct Wino2Tail { int items, slices; };
Wino2Tail wino2_tail_split(const ConvConfig &cfg, const ConvProblem &p);
int wino2_max_slices(const ConvConfig &cfg, const ConvProblem &p);

// 1-D Winograd F(2,3) on the fp16 matrix cores with two-piece operands (conv_h2.hip): fp32-class
// accuracy at 0.28 of the fp32 2-D form's matrix time.  Config ids 0 (64 channels x 8 x 32 pixels per
// workgroup), 1 (128 channels) and 2 (64 channels x 16 x 32 pixels); all read the same packed bank.
constexpr int kAmaxSlots = 64;
ConvConfig h2_config(int mb, int pb = 1);     // (1, 1), (2, 1) or (1, 2): ids 0 / 1 / 2
ConvConfig h2_pick_config(const ConvProblem &p);    // the cheaper tiling by the round model (shape only)
bool h2_usable(const ConvProblem &p);       // what the kernel takes (shape, epilogue, addressing)
size_t h2_packed_floats(int K, int M);
int h2_pack_weights(hipStream_t s, const float *w_caffe, int Mo, int Ko, int transpose_flip, float *packed);
int h2_launch(hipStream_t s, const ConvConfig &cfg, const ConvProblem &p, int ksplit);
// The injecting epilogue's specialised bodies (conv_h2_inject.hip): what a launch injects | where its mask comes from
enum { kH2Style = 1, kH2Content = 2, kH2MaskNibbles = 4, kH2MaskBlob = 8 };
int h2_variant(const ConvProblem &p, int pin, bool split);      // the body a launch takes, or 0: the generic one
int h2_launch_variant(hipStream_t s, const WinoArgs &a, int n_wg, int cfg_id, int pin, int var);
int h2_splitk_factor(const ConvConfig &cfg, const ConvProblem &p);
bool h2_fuses_pool(const ConvProblem &p);
bool h2_takes_pooled_input(const ConvConfig &cfg, const ConvProblem &p);   // ConvProblem::pin_codes
// slots[0 .. kAmaxSlots) = 0, then max |x| as float bits into them (the largest slot counts)
int absmax_launch(hipStream_t s, const float *x, size_t n, unsigned *slots);

// 3x3 convolution with <= 4 output channels (backward into the image) on the 4x4x1 MFMA.
size_t conv_small_packed_floats(int K);
int conv_small_pack(hipStream_t s, const float *w_caffe, int Mo, int Ko, int transpose_flip,
                    float *packed);
int conv_small_launch(hipStream_t s, const float *x, const float *packed, float *y,
                      const float *mask, int K, int M, int H, int W);

// ------------------------------------------------------------------------------------------------
// The packed-weight convolutions by family (conv_dispatch.cpp): choice, filter bank, launch, capabilities.
// ------------------------------------------------------------------------------------------------
bool conv_h2_enabled();    // some problem may take the fp16-split kernel (STX_CONV_H2 / _H2_BWD / STX_CONV_ALGO)
// Times the direct candidates on `stream` with the two events, from the banks `bank` gives.
struct ConvTuner { int device; hipStream_t stream; hipEvent_t ev0, ev1; std::function<int(const ConvConfig &, const float **)> bank; };
// The fp16-split kernel, else the fp32 2-D Winograd one (`winograd`: the engine's switch), else a direct
// variant -- by shape; tuner (or null) then times the direct variants, which all round alike.
int conv_choose(const ConvProblem &p, bool winograd, const ConvTuner *tuner, ConvConfig *out);
// Configurations with the same key read the same bank (one per direct variant, one for the Winograd
// geometries, one for the fp16-split tilings; per direction).  pack: Caffe-layout weights -> `floats` floats.
struct ConvBank { int key; size_t floats; std::function<int(hipStream_t, const float *w_caffe, float *packed)> pack; };
ConvBank conv_bank(const ConvConfig &cfg, int dir, int Mo, int Ko, int ksize);   // dir: as conv_pack_weights
ConvBank conv_small_bank(int Mo, int Ko);     // conv_small_launch's (backward)
// Enqueues p; adds a direct convolution's FLOPs and those the kernel issues to the two counters.
int conv_dispatch(hipStream_t s, const ConvConfig &cfg, const ConvProblem &p, double *flop_algorithmic,
                  double *flop_issued);
// What a launch of p under cfg does (shape and epilogue only):
int conv_splitk_factor(const ConvConfig &cfg, const ConvProblem &p);     // K slices (1: none)
size_t conv_splitk_floats(const ConvConfig &cfg, const ConvProblem &p);  // scratch floats of its splits
bool conv_takes_clock(const ConvConfig &cfg);                            // ConvProblem::clock_out
bool conv_fuses_pool(const ConvConfig &cfg, const ConvProblem &p);       // writes p.pool_out itself
bool conv_writes_pool_codes(const ConvConfig &cfg);                      // ... and p.pool_codes
bool conv_reads_x_amax(const ConvConfig &cfg);                           // ConvProblem::x_amax
bool conv_leaves_y_amax(const ConvConfig &cfg);                          // ConvProblem::y_amax
bool conv_takes_inject(const ConvConfig &cfg);                           // ConvProblem::inject
bool conv_takes_pooled_input(const ConvConfig &cfg, const ConvProblem &p);            // ConvProblem::pin_codes
bool conv_uses_relu_codes(const ConvConfig &cfg, const ConvProblem &p, int ksplit);   // p.in_codes / mask_codes
bool conv_writes_out_codes(const ConvConfig &cfg, const ConvProblem &p, int ksplit);  // p.out_codes

int pool_forward_launch(hipStream_t s, const float *x, int C, int H, int W, int mode, float *y,
                        unsigned char *codes = nullptr);
int pool_backward_codes_launch(hipStream_t s, const float *dy, const unsigned char *codes, int C,
                               int H, int W, int mode, bool relu_mask, float *dx);
// dx = route(dy) [* (x > 0) when masked]; x is the pool input data (post-ReLU).
int pool_backward_launch(hipStream_t s, const float *dy, const float *x, int C, int H, int W,
                         int mode, bool relu_mask, float *dx);

// Gram: partial products over split-K slices, then a fixed-order reduction.
struct GramPlan {
    int C, HW, splits, tiles;      // tiles = lower-triangular 64x64 tiles
    int parts;                     // partial tiles written per slice (4: one per wave)
    size_t partial_floats;
};
GramPlan gram_plan(int C, int HW);
// f_amax (or null): kAmaxSlots words of float bits bounding |feat| -> the fp16 two-piece kernel
// (f16x2.h; ask gram_h2_usable first), whose partial tiles carry the square of the input scale:
// hand the same slots to gram_finish_launch.
bool gram_h2_usable(const float *feat, int C, int HW);
int gram_partials_launch(hipStream_t s, const float *feat, const GramPlan &plan, float *partials,
                         const unsigned *f_amax = nullptr);
// gram_out (lower-tri, upper zero) = sum_s partials * 1/(C*HW).  If target != null also writes
// dsym = sym(tril(gram - target)) and sumsq[0] = sum over the lower triangle of (gram-target)^2.
// `pieces` (optional, with target): dsym split into three bf16 matrices [3][C][C] for symm_bf3_launch
// (C a multiple of 64).  sumsq == null: the per-block sums of squares are left behind the Gram
// partials (gram_finish_blocks(plan) floats at partials + plan.partial_floats) for the caller to add.
int gram_finish_blocks(const GramPlan &plan);
// With a target, gram_finish_blocks(plan) words of float bits follow the block sums: max |dsym| per
// block (symm_h2_launch's d_amax).  f_amax: see gram_partials_launch.
// block_out (or null: behind the Gram partials): where the 2 x gram_finish_blocks(plan) block words go.
int gram_finish_launch(hipStream_t s, const float *partials, const GramPlan &plan, float *gram_out,
                       const float *target, float *dsym, float *sumsq, unsigned short *pieces = nullptr,
                       const unsigned *f_amax = nullptr, float *block_out = nullptr);

// S = dsym F (+ per-workgroup partial sums of |S|) on the bf16 matrix cores, three-piece split
// (symm.hip).  `pieces` is scratch for the split dsym: symm_pieces_elems(C) 16-bit words.
size_t symm_pieces_elems(int C);
int symm_num_workgroups(int C, int HW);
bool symm_bf3_usable(const float *feat, const float *out, int C, int HW);
// pieces_ready: gram_finish_launch already wrote them (else they are made from dsym here)
// The same product with two fp16 pieces per operand, three products (f16x2.h): dsym is read as it
// is; d_amax = n_damax words of float bits whose largest is max |dsym|, f_amax = kAmaxSlots words
// bounding |feat|.
bool symm_h2_usable(const float *feat, const float *out, int C, int HW);
int symm_h2_launch(hipStream_t s, const float *feat, const float *dsym, const unsigned *d_amax, int n_damax,
                   const unsigned *f_amax, float *out, float *partials, int C, int HW);
int symm_bf3_launch(hipStream_t s, const float *feat, const float *dsym, unsigned short *pieces,
                    bool pieces_ready, float *out, float *partials, int C, int HW);

// sums[0] = sum (F - Fc)^2, sums[1] = sum |F - Fc| over the tile window of the (virtually rolled)
// content map.
#ifdef __HIPCC__
// Window origin in the un-rolled content map, before wrapping: (oy - sy, ox - sx).
__device__ __forceinline__ int content_origin_y(const ContentWindow &w) { return w.oy - w.sy; }
__device__ __forceinline__ int content_origin_x(const ContentWindow &w) { return w.ox - w.sx; }
// Rolled content value at tile-feature position (c, y, x):
// roll2(Fc, (sx, sy))[c][oy + y][ox + x] = Fc[c][(oy + y - sy) mod ch][(ox + x - sx) mod cw]
__device__ __forceinline__ size_t content_index(const ContentWindow &w, int c, int y, int x) {
    int yy = (content_origin_y(w) + y) % w.ch;
    int xx = (content_origin_x(w) + x) % w.cw;
    if (yy < 0) yy += w.ch;
    if (xx < 0) xx += w.cw;
    return ((size_t)c * w.ch + yy) * w.cw + xx;
}
#endif

// A final sum a caller may postpone: dst[0] = the n floats at src, added in the fixed order of
// sum_partials_kernel.  The tile path collects the jobs of all its loss terms and runs them as ONE
// launch behind the forward pass (sum_jobs_launch) -- a dispatch costs ~5 us however little it does.
struct SumJob {
    const float *src;
    int n;
    float *dst;
};
int sum_jobs_launch(hipStream_t s, const SumJob *jobs, int n_jobs);
// defer (or null: the two sums are launched here): receives the two jobs instead
int content_sums_launch(hipStream_t s, const float *feat, const float *content,
                        const ContentWindow &win, float *sums /*[2]*/, std::vector<SumJob> *defer = nullptr);
// diff (=|+=) coef / (abs_sum/n + EPS) * term, term = S (style) or F - Fc (content).
// y_amax (optional, zeroed by the caller): max |value written| for a conv_h2 launch that reads diff next
int inject_style_launch(hipStream_t s, float *diff, const float *sgrad, size_t n,
                        const float *abs_sum, float coef, bool accumulate, unsigned *y_amax = nullptr);
int inject_content_launch(hipStream_t s, float *diff, const float *feat, const float *content,
                          const ContentWindow &win, const float *sums, float coef, bool accumulate,
                          unsigned *y_amax = nullptr);
int relu_inplace_launch(hipStream_t s, float *x, size_t n);
int sum_partials_launch(hipStream_t s, const float *partials, int n, float *out);
int sum_partials2_launch(hipStream_t s, const float *a, int na, float *out_a, const float *b, int nb,
                         float *out_b);

// style_mask.hip: a style term restricted to a region by a mask map m (values in [0, 1]; the tile's
// window of it is addressed like a content map's).  Partials are added in sum_partials_kernel's order.
constexpr int kMaskParts = 1024;         // most partials of sum m^2 (mask_apply_launch)
constexpr int kMaskSgradParts = 2048;    // most partials of sum |m . S| (mask_sgrad_launch)
// out [ceil(H/scale)][ceil(W/scale)] = block means of the H x W mask (edge blocks over what exists)
int mask_map_launch(hipStream_t s, const float *mask, int H, int W, int scale, float *out);
// fm = feat . m (every channel); *n_parts partials of sum m^2 over the window into m2_partials
int mask_apply_launch(hipStream_t s, const float *feat, const float *map, const ContentWindow &win, float *fm,
                      float *m2_partials, int *n_parts);
// a = sum m^2 / HW from the partials; out = a gs (C x C), a_out[0] = a
int mask_target_launch(hipStream_t s, const float *gs, int C, const float *m2_partials, int n_parts, int HW,
                       float *out, float *a_out);
// sgrad <- a[0] (m . sgrad) in place; *n_parts partials of sum |m . sgrad| (without a) into partials
int mask_sgrad_launch(hipStream_t s, float *sgrad, const float *map, const ContentWindow &win, const float *a,
                      float *partials, int *n_parts);

// content_mask.hip: a content term weighted by a map m (values in [0, 1]; the tile's window of it is the
// content map's own).  The pass takes content_sums_launch's grid, so that m == 1 leaves its partials.
constexpr int kContentMaskParts = 1024;      // most workgroups of content_mask_term_launch (reduce.hip's cap)
// a_out[0] = sum m / (fh fw) over the window, in double in a fixed order
int content_mask_mean_launch(hipStream_t s, const float *map, const ContentWindow &win, float *a_out);
// sgrad = a[0] (m . (feat - content[window])); *n_parts partials of sum m d^2, then as many of sum |m d|
int content_mask_term_launch(hipStream_t s, const float *feat, const float *content, const float *map,
                             const ContentWindow &win, const float *a, float *sgrad, float *partials,
                             int *n_parts);

// stat.hip: the mean / std style term of a blob [C][HW] against per-channel targets (include/stx.h,
// stx_set_stat_targets).  A workgroup owns kStatSlice pixels of one channel; everything the three
// launches hand to each other lives in stat_scratch_floats(C, HW) floats of the caller's.
constexpr int kStatSlice = 16384;
constexpr float kStatEps = 1e-5f;        // sd = sqrt(var + kStatEps)
int stat_slices(int HW);
size_t stat_scratch_floats(int C, int HW);
// partials [C][slices][4] = (count, mean as two floats, M2 about that mean) of every slice
int stat_partials_launch(hipStream_t s, const float *feat, int C, int HW, float *partials);
// Chan's merge in double, in slice order.  MU, SD given: table [C][4] = (mu, a = mu - MU, b = (sd - SD) / sd, 0)
// and e_out[0] = E; null: mean_out[c] = mu, sd_out[c] = sd
int stat_finish_launch(hipStream_t s, const float *partials, int C, int HW, const float *MU, const float *SD,
                       float *table, float *e_out, float *mean_out, float *sd_out);
// sgrad = a + b (feat - mu) per channel; *n_parts partials of sum |sgrad| into abs_partials
int stat_grad_launch(hipStream_t s, const float *feat, int C, int HW, const float *table, float *sgrad,
                     float *abs_partials, int *n_parts);

// swd.hip: the sliced Wasserstein style term of a blob [C][n] along D directions V [D][C] against quantile
// targets Tq [D][Q] (include/stx.h, stx_set_swd_targets).  The sort works on records of 64 bits, in rows padded
// to swd_padded(n) -- a power of two, 2 at least -- and in LDS blocks of kSwdBlock records.
constexpr int kSwdBlock = 8192;
constexpr int kSwdMaxDirs = 4096, kSwdMaxQuantiles = 65536, kSwdMaxPixels = 1 << 22;
int swd_padded(int n);
// STX_ERR_ARG / STX_ERR_UNSUPPORTED with the message, as include/stx.h lists them (n = 1 where no blob is known yet)
int swd_check(const char *who, int C, long long n, int D, int Q);
// floats of the caller's that outlive the term's launches: the partials of E (swd_e_parts), then those of sum |S|
// from the next multiple of 64
int swd_e_parts(int n, int D);
size_t swd_scratch_floats(int C, int n, int D);
// floats of the work area, free again behind the term's last launch: the records [D][swd_padded(n)], then G [D][n]
size_t swd_work_floats(int n, int D);
// records [D][swd_padded(n)] = (order-preserving image of v_d . f_i, i), padded with sentinels that order last
int swd_project_launch(hipStream_t s, const float *feat, int C, int n, const float *V, int D, void *records);
// Sorts every row, in two calls: all launches but the last, then the last one.  Tq null: the last launch leaves
// the sorted records in place.  Otherwise it ends in the rank pass and writes no records: G [D][n] = g, rank_out
// [D][n] (or null), e_parts = the blocks' sums of g^2 / (D n).  swd_sort_passes: launches of both, each of which
// reads and writes every record once.
int swd_sort_launch(hipStream_t s, void *records, int n, int D);
int swd_finish_launch(hipStream_t s, void *records, int n, int D, const float *Tq, int Q, float *G, int *rank_out,
                      float *e_parts);
int swd_sort_passes(int n);
// sgrad [C][n] = V^T G / D; *n_parts partials of sum |sgrad| into abs_parts
int swd_grad_launch(hipStream_t s, const float *V, const float *G, int C, int n, int D, float *sgrad, float *abs_parts,
                    int *n_parts);
// out [D][Q] = resample(sorted row, n -> Q)
int swd_quantiles_launch(hipStream_t s, const void *records, int n, int D, int Q, float *out);

// selfsim.hip: the self-similarity content term of a blob [C][h][w] against the tile's window of a content map
// (include/stx.h, stx_set_selfsim_targets), on a sample grid of at most `points` positions.
constexpr int kSelfsimMaxPoints = 4096;
constexpr float kSelfsimEps = 1e-6f;
// g = the smallest integer >= 1 with ceil(h / g) ceil(w / g) <= points; the positions (a g, b g), a < gh, b < gw,
// in raster order; N = gh gw
struct SelfsimGrid {
    int g, gh, gw, N;
};
SelfsimGrid selfsim_grid(int h, int w, int points);
// STX_ERR_ARG for points outside 2 .. kSelfsimMaxPoints, STX_ERR_UNSUPPORTED for channels not a multiple of 64
int selfsim_check(const char *who, int C, int points);
// One side of the term: planes [C][mh][mw] at p, the sampled pixel (y, x) read at ((oy + y) mod mh, (ox + x) mod mw).
// A plain [C][h][w] array is {p, h, w, 0, 0}; a content map's window is the map with origin (oy - sy, ox - sx).
struct SelfsimSource {
    const float *p;
    int mh, mw, oy, ox;
};
// The term's scratch, all of which outlives its launches (the final sums of e_parts and abs_parts may be deferred).
struct SelfsimScratch {
    float *rows;            // [2][N][C]: the unit columns of F, then of the window
    float *inv_r;           // [2][N]
    float *D;               // [2][N][N]: DX then DC; the column pass leaves A where DX was
    float *col_parts;       // [2][ceil(N / 64)][N]: column sums of D per block of 64 rows
    float *u_parts;         // [ceil(N / 64)][N]
    float *q;               // [N][C]
    signed char *T;         // [N][N]
    float *e_parts;         // ceil(N / 64)^2 partials of E
    float *abs_parts;       // ceil(N / 64) partials of sum |S|
    size_t floats;
};
SelfsimScratch selfsim_scratch(float *base, int C, int N);
size_t selfsim_scratch_floats(int C, int N);
int selfsim_prepare_launch(hipStream_t s, const SelfsimSource &feat, const SelfsimSource &content, int C,
                           const SelfsimGrid &gr, const SelfsimScratch &x);
int selfsim_dist_launch(hipStream_t s, int C, int N, const SelfsimScratch &x);
// signs: T int8 [N][N] (x.T, or the caller's array); *n_e partials of E in x.e_parts
int selfsim_cols_launch(hipStream_t s, int N, const SelfsimScratch &x, signed char *signs, int *n_e);
// sgrad [C][h][w] = S (cleared first when the grid skips pixels); *n_abs partials of sum |S| in x.abs_parts
int selfsim_grad_launch(hipStream_t s, int C, int h, int w, const SelfsimGrid &gr, const SelfsimScratch &x,
                        float *sgrad, int *n_abs);

// cx.hip: the contextual style term of a blob [C][h][w], sampled on the grid of selfsim_grid, against a bank [M][C]
// of centred unit rows with the mean mu [C] of the raw rows (include/stx.h, stx_set_cx_targets).
constexpr int kCxMaxPoints = 4096;
constexpr int kCxMaxRows = 16384;
constexpr long long kCxMaxCells = 1ll << 24;    // points x M: the two score matrices exist in memory
constexpr float kCxEps = 1e-5f;
// STX_ERR_ARG for points outside 2 .. kCxMaxPoints, M outside 1 .. kCxMaxRows, eta <= 0 or not finite;
// STX_ERR_UNSUPPORTED for channels not a multiple of 64 and for points x M > kCxMaxCells
int cx_check(const char *who, int C, int points, long long M, double eta);
// rows of the bank per K slice of the gradient product (a multiple of 32); ceil(M / it) slices
int cx_slice_len(int C, int N, int M);
// The term's scratch, all of which outlives its launches (the final sums of e_part and abs_parts may be deferred).
struct CxScratch {
    float *rows;            // [N][C]: the unit columns of F - mu
    float *inv_r;           // [N]
    float *S;               // [N][M]: the scores; the second row pass leaves g there
    float *P;               // [N][M]
    float *best_val;        // [ceil(M / 64)][N]: a row's best score per block of 64 columns ...
    int *best_idx;          // ... and its lowest column
    int *kstar;             // [N]
    float *tau, *u, *row_p; // [N] each: tau_i, u_i, P_i
    float *col_val;         // [ceil(N / 64)][M]: a column's best p per block of 64 rows ...
    int *col_idx;           // ... and its lowest row
    int *winner;            // [M]: i*_k
    float *m_parts;         // ceil(M / 256) partials of sum_k m_k
    float *qp;              // [slices][N][C]: the gradient product's partial tiles
    float *e_part;          // E, one "partial"
    float *dot_parts;       // [C / 64][N]: a channel block's share of q_i . x_i
    float *abs_parts;       // (C / 64) ceil(N / 64) partials of sum |S|
    size_t floats;
};
CxScratch cx_scratch(float *base, int C, int N, int M);
size_t cx_scratch_floats(int C, int N, int M);
// rows [N][C] = the raw columns of feat on the grid
int cx_rows_launch(hipStream_t s, const float *feat, int C, int h, int w, const SelfsimGrid &gr, float *rows);
// mu [C] and bank [M][C] from raw rows [M][C] (all on the device)
int cx_bank_launch(hipStream_t s, const float *raw, int C, int M, float *mu, float *bank);
int cx_prepare_launch(hipStream_t s, const float *feat, int C, int h, int w, const SelfsimGrid &gr, const float *mu,
                      const CxScratch &x);
int cx_score_launch(hipStream_t s, int C, int N, int M, const float *bank, const CxScratch &x);
int cx_rows_pass_launch(hipStream_t s, int N, int M, float eta, const CxScratch &x);
// the column pass and the second row pass; kbest_out [N], winner_out [M] (device, or null): the decisions
int cx_cols_pass_launch(hipStream_t s, int N, int M, float eta, const CxScratch &x, int *kbest_out, int *winner_out);
// sgrad [C][h][w] = S (cleared first when the grid skips pixels); *n_abs partials of sum |S| in x.abs_parts
int cx_grad_launch(hipStream_t s, int C, int h, int w, const SelfsimGrid &gr, int M, const float *bank,
                   const CxScratch &x, float *sgrad, int *n_abs);

// shiftgram.hip: the shifted-Gram style term of a blob [C][h][w] for a list of axis-aligned offsets against targets
// [offsets][C][C] (include/stx.h, stx_set_shift_targets).  P_d, the pairs of an offset in raster order, is cut into
// slices of shift_slice_len(h w) pairs; a map has shift_slices(h w) of them at most.
constexpr int kShiftMaxOffsets = 16;
struct ShiftOffsets {       // (a kernel argument)
    int n;
    int dy[kShiftMaxOffsets], dx[kShiftMaxOffsets];
};
int shift_slice_len(int HW);
int shift_slices(int HW);
// STX_ERR_ARG for a count outside 1 .. kShiftMaxOffsets or an offset that is not (0, d) or (d, 0) with d >= 1,
// STX_ERR_UNSUPPORTED for channels not a multiple of 32; `out` (or null) receives the list
int shift_check_offsets(const char *who, int C, const int *offsets /*[n][2] = dy, dx*/, int n_offsets,
                        ShiftOffsets *out);
// STX_ERR_ARG when an offset leaves an h x w map without a pair (the message names `who` and the offset)
int shift_check_map(const char *who, int C, int h, int w, const ShiftOffsets &off);
// The term's scratch, all of which outlives its launches (the final sums of e_parts and abs_parts may be deferred).
struct ShiftScratch {
    float *partials;        // [offsets][shift_slices][C][C]
    float *weights;         // [offsets][2][C][C]: (n / (n_d |Delta|)) D_d, then its transpose
    float *e_parts;         // [offsets][ceil(C C / 256)] partials of E
    float *abs_parts;       // [ceil(C / 64)][ceil(h w / 64)] partials of sum |S|
    size_t floats;
};
ShiftScratch shift_scratch(float *base, int C, int HW, int n_offsets);
size_t shift_scratch_floats(int C, int HW, int n_offsets);
int shift_cross_launch(hipStream_t s, const float *feat, int C, int h, int w, const ShiftOffsets &off,
                       const ShiftScratch &x);
// targets [offsets][C][C]: the weights and *n_e partials of E in x.e_parts.  Or, targets null: x_out [offsets][C][C] = X.
int shift_merge_launch(hipStream_t s, int C, int h, int w, const ShiftOffsets &off, const ShiftScratch &x,
                       const float *targets, float *x_out, int *n_e);
// sgrad [C][h][w] = S; *n_abs partials of sum |S| in x.abs_parts
int shift_grad_launch(hipStream_t s, const float *feat, int C, int h, int w, const ShiftOffsets &off,
                      const ShiftScratch &x, float *sgrad, int *n_abs);

// nnfm.hip: the nearest-neighbour feature matching term of a blob [C][n] against a bank [M][C] of unit rows
// (include/stx.h, stx_set_nnfm_targets).  The search multiplies kNnfmQ query columns by kNnfmB bank rows per
// workgroup, kNnfmK channels per LDS stage; with few query blocks the bank is cut into slices.
constexpr int kNnfmQ = 128, kNnfmB = 128, kNnfmK = 32, kNnfmMaxSlices = 64;
constexpr int kNnfmMaxK = 4;        // the k best rows per query (stx_set_nnfm_knn_targets): 1 .. 4
struct NnfmPlan {
    int q_blocks, b_blocks, slices, blocks_per_slice;
};
NnfmPlan nnfm_plan(int n, int M);
// floats that hold the fp16 hi / lo pieces of `rows` rows of C channels ([rows][C] hi, then [rows][C] lo)
size_t nnfm_pieces_floats(int rows, int C);
// floats of the caller's that one term takes, and their division (from the next 256-byte boundary)
// (patch 3: the 3 x 3 patch term, whose bank rows have 9 C channels -- O(n) floats more; k rows per query: k - 1
// further index planes and k-fold slice pairs; cover: the arrays of NnfmCover behind everything else, so that a
// term without the coverage part keeps its size and layout)
size_t nnfm_scratch_floats(int C, int n, int M, int patch = 1, int k = 1, bool cover = false);
// The coverage part (stx_set_nnfm_cover_targets): every bank row j looks for its best column i*_j.  All null
// without it.
struct NnfmCover {
    int *winner = nullptr;          // [M]: i*_j
    float *part_score = nullptr;    // [slices of nnfm_plan(M, n)][M], or null with one slice
    int *part_idx = nullptr;
    int *cursor = nullptr;          // [n]: rows per column, then each column's fill cursor
    int *offsets = nullptr;         // [n + 1]: column i owns list[offsets[i] .. offsets[i + 1])
    int *unordered = nullptr;       // [M]: the lists as the cursors filled them
    int *list = nullptr;            // [M]: the lists, ascending j within a column
    float *cprime = nullptr;        // [M]: c'_j
    float *e_parts = nullptr;       // ceil(n / 64) partials of E_fwd, then ceil(M / 64) of cover E_cov: ONE list of E
    float *e_cov_parts = nullptr;   // ceil(M / 64) partials of E_cov alone
    float *abs_parts = nullptr;     // (C / 64) ceil(n / 64) partials of sum |S| of the final S
};
struct NnfmScratch {
    unsigned short *xhi, *xlo;      // pieces of x_i 2^13 (patch 3: of f_i under the blob's common scale), [n][C] each
    float *inv_r;                   // [n]
    int *idx;                       // [k][n], rank-major
    float *part_score;              // [slices][k][n], or null with one slice
    int *part_idx;
    float *partials;                // ceil(n / 64) of (2/n) sum (1 - c_i), then as many of sum |S|
    double *work;                   // patch 3: nnfm_patch_work_floats(n) floats of nnfm_prepare_launch, else null
    float *cosv;                    // patch 3: c_p [n], else null
    NnfmCover cov;                  // the coverage part, or nulls
};
NnfmScratch nnfm_carve(float *scratch, int C, int n, int M, int patch = 1, int k = 1, bool cover = false);
// The term's three steps, for both forms.  patch 1: columns of C channels against bank rows of C.  patch 3
// (stx_set_nnfm_patch_targets): pixel p's patch is the 9 C vector of the columns at p + tap, tap-major (dy outer,
// dx inner, (-1, -1) first), zero outside the map, against bank rows [M][9 C] of unit or zero rows.
// floats (8-byte aligned) that nnfm_prepare_launch works in at patch 3: the column norms^2 and their block maxima
size_t nnfm_patch_work_floats(int n);
// feat [C][h][w], outputs per picked position (y % stride == 0 and x % stride == 0, raster order).
// patch 1, one pass, each output optional (hi and lo together): 1 / |f| (0 for a zero column) into inv_r, the
// pieces of f / |f| 2^13 into hi / lo, f / |f| as float32 rows into rows_out; work is not used.
// patch 3, two passes through work, one of the two: hi / lo (stride 1 only) -- 1 / |P_p| into inv_r and the pieces
// of the COLUMNS [n][C] under one power of two for the whole blob; or rows_out -- the unit patches as float32 rows
// [rows][9 C] (a zero patch stays a zero row).
int nnfm_prepare_launch(hipStream_t s, const float *feat, int C, int h, int w, int patch, int stride, double *work,
                        float *inv_r, unsigned short *hi, unsigned short *lo, float *rows_out);
// the pieces of bank 2^13, bank [M][C] given as rows (C: the whole width of a row)
int nnfm_split_rows_launch(hipStream_t s, const float *bank, int M, int C, unsigned short *hi, unsigned short *lo);
// idx_out[i] = argmax_j x_i . b_j (patch 3: P_p . b_j, the query operand gathered from x's [n][C] pieces), the
// lowest j among equal scores.  pieces: the bank's, [M][patch^2 C] hi then lo (nnfm_split_rows_launch).
// k > 1: idx_out [k][n], the k best rows by (score descending, index ascending), -1 from rank min(k, M) on.
int nnfm_search_launch(hipStream_t s, const NnfmScratch &x, int h, int w, int patch, const unsigned short *pieces,
                       int M, int C, int *idx_out, int k = 1);
// sgrad = S [C][n] (patch 3: x.cosv = c_p first, then S in the gather form; the bank aligned to 16 bytes);
// *n_parts partials of E in x.partials, then as many of sum |S|.  k > 1: idx [k][n], and the target of a column is
// the mean of its min(k, M) rows
int nnfm_grad_launch(hipStream_t s, const float *feat, int C, int h, int w, int patch, const NnfmScratch &x,
                     const float *bank, int M, const int *idx, float *sgrad, int *n_parts, int k = 1);
// The coverage part of the plain term (patch 1), behind nnfm_prepare_launch and nnfm_grad_launch, in three steps.
// winner_out[j] = argmax_i x_i . b_j, the lowest i among equal scores: nnfm_search_kernel<false, 1> with the
// operands exchanged -- the bank's pieces are the queries, x's pieces the bank -- under nnfm_plan(M, n).
int nnfm_cover_search_launch(hipStream_t s, const NnfmScratch &x, int n, const unsigned short *pieces, int M, int C,
                             int *winner_out);
// c'_j into x.cov.cprime with the partials of E_cov (and of cover E_cov behind E_fwd's place in x.cov.e_parts), then
// the inverted index: x.cov.offsets and x.cov.list, ascending j within a column.
int nnfm_cover_index_launch(hipStream_t s, const float *feat, int C, int n, const NnfmScratch &x, const float *bank,
                            int M, const int *winner, float cover);
// sgrad = S_fwd + cover S_cov in place, the lists added in their order; E_fwd's partials join x.cov.e_parts:
// *n_e partials of E = E_fwd + cover E_cov there, *n_abs of sum |S| in x.cov.abs_parts.
int nnfm_cover_grad_launch(hipStream_t s, const float *feat, int C, int n, const NnfmScratch &x, const float *bank,
                           int M, float cover, float *sgrad, int *n_e, int *n_abs);
// The guided term (stx_set_nnfm_guided_targets; patch 1): the bank is cut into segments, one per style picture,
// and column i looks into segment s with the weight m_s(i) of that picture's mask map.  Segment s holds the rows
// [off[s], off[s] + rows[s]) of the bank; indices are local to a segment.
constexpr int kNnfmMaxSegments = 8;     // (STX_NNFM_MAX_SEGMENTS)
struct NnfmSegments {
    int count;
    int off[kNnfmMaxSegments], rows[kNnfmMaxSegments];
    int total() const { return count ? off[count - 1] + rows[count - 1] : 0; }
    int largest() const {
        int m = 0;
        for (int s = 0; s < count; ++s) m = rows[s] > m ? rows[s] : m;
        return m;
    }
};
// count segments of seg_rows[s] rows, one after the other
NnfmSegments nnfm_segments(const int *seg_rows, int count);
// floats of the caller's that one guided term takes (slices: nnfm_plan(n, the largest segment)), and their division
size_t nnfm_guided_scratch_floats(int C, int n, const NnfmSegments &segs, int k);
struct NnfmGuidedScratch {
    unsigned short *xhi, *xlo;      // as NnfmScratch's
    float *inv_r;                   // [n]
    float *m;                       // [segments][n]: the tile's windows of the mask maps
    unsigned char *active;          // [segments][query blocks]: some column of the block has m_s > 0
    float *m_parts;                 // [segments][query blocks]: the blocks' sums of m_s
    int *idx;                       // [segments][k][n], -1 in the blocks of a pair that is not searched
    float *part_score;              // [segments][slices][k][n], or null with one slice
    int *part_idx;
    float *partials;                // ceil(n / 64) of E, then as many of sum |S|
};
NnfmGuidedScratch nnfm_guided_carve(float *scratch, int C, int n, const NnfmSegments &segs, int k);
// One pass over the windows `win` (fh x fw = the blob's map) of maps [segments][win.ch][win.cw]: x.m, x.active,
// x.m_parts and -1 into idx [segments][k][n] for the pairs that will not be searched; then, a launch behind it,
// a_out[0] = sum m / n in double in a fixed order.
int nnfm_mask_window_launch(hipStream_t s, const float *maps, const ContentWindow &win, const NnfmSegments &segs, int k,
                            const NnfmGuidedScratch &x, int *idx, float *a_out);
// nnfm_search_launch per (query block, slice, segment): idx_out [segments][k][n], written for the active pairs only.
// pieces: of the whole bank, [total rows][C] hi then lo.
int nnfm_guided_search_launch(hipStream_t s, const NnfmGuidedScratch &x, int n, const unsigned short *pieces,
                              const NnfmSegments &segs, int C, int *idx_out, int k);
// sgrad = a S [C][n], S_i = sum_s m_s(i) S_{i,s} over the segments with m_s(i) > 0 in ascending s (a: a_ptr[0], or 1
// when null); *n_parts partials of E in x.partials, then as many of sum |S| (without a)
int nnfm_guided_grad_launch(hipStream_t s, const float *feat, int C, int n, const NnfmGuidedScratch &x, const float *bank,
                            const NnfmSegments &segs, const int *idx, const float *a_ptr, float *sgrad, int *n_parts,
                            int k);

// image_ops.hip
int cut_tile_launch(hipStream_t s, const float *img, int H, int W, int rx, int ry, int y0, int x0,
                    int th, int tw, float *tile);
int put_tile_launch(hipStream_t s, float *grad, int H, int W, int rx, int ry, int y0, int x0,
                    int th, int tw, const float *tile);
int place_window_launch(hipStream_t s, float *dst, int dh, int dw, int y0, int x0, const float *src,
                        int C, int h, int w);
int roll_add_launch(hipStream_t s, float *acc, const float *src, int C, int h, int w, int sx, int sy,
                    float alpha, bool init);
int resample_launch(hipStream_t s, int axis, const float *src, int C, int H, int W, float *dst,
                    int OH, int OW, const int *bounds, const double *k, int ksize, int clamp);
// *out_dev = sum of n float partials, added in double in a fixed order
int finish_partials_launch(hipStream_t s, const float *partials, int n, double *out_dev);
// the same for nv = 1..4 values: out_dev[k] = sum of partials[k * n .. k * n + n)
int finish_partials_n_launch(hipStream_t s, const float *partials, int n, int nv, double *out_dev);
int regularizers_launch(hipStream_t s, const float *img, float *grad, int H, int W,
                        const float mean[3], float tv_scale, float tv_power, float p_scale,
                        float p_power, const float *aux, float aux_scale, int aux_rx, int aux_ry,
                        double *loss_terms /*[3]*/, float *scratch, size_t scratch_floats);

// swt.hip: the SWT term.  One Haar level is a single pass over `scratch` (blocks_for(3 H W) floats);
// more levels and the table form are two separable passes: tmp and partials hold what
// swt_levels_scratch asks for, N = swt_padded_side(H, W) bounds the level count (2^levels <= N).
int swt_padded_side(int H, int W);
int swt_haar_launch(hipStream_t s, const float *img, float *grad, int H, int W, int rx, int ry,
                    float scale, float power, double *loss_term, float *scratch,
                    size_t scratch_floats);
void swt_levels_scratch(int H, int W, size_t *tmp_floats, size_t *partial_floats);
int swt_haar_levels_launch(hipStream_t s, const float *img, float *grad, int H, int W, int levels,
                           int rx, int ry, float scale, float power, double *loss_term, float *tmp,
                           float *partials);
// The same term for the orthogonal Daubechies / symlet filter with `order` vanishing moments.
// swt_daub_table builds, in double on the host, the per-axis taps of `levels` levels folded onto the
// periodic square of side N (at most N taps; tap i weighs padded coordinate q + i - *hl) and
// rounds them to float once; swt_table_launch runs the two passes with a device copy of them.
void swt_daub_table(int order, int levels, int N, std::vector<float> *taps, int *hl);
int swt_table_launch(hipStream_t s, const float *img, float *grad, int H, int W, const float *table,
                     int ntaps, int hl, int rx, int ry, float scale, float power,
                     double *loss_term, float *tmp, float *partials);

// lap.hip: the Laplacian loss.  lap_levels describes the pooled grids of the pool sizes (distinct powers
// of two, 1..64, at most kLapMaxPools: the caller has checked) and returns their floats in all, which is
// the size of a target; map k starts at off[k].  scratch holds lap_scratch_floats(that count) floats.
constexpr int kLapMaxPools = 4;
struct LapLevels {
    int n;
    int lp[kLapMaxPools], hp[kLapMaxPools], wp[kLapMaxPools], off[kLapMaxPools];    // log2 p, grid, offset
};
size_t lap_levels(int H, int W, int n_pools, const int *pools, LapLevels *lv);
size_t lap_scratch_floats(size_t map_floats);
// target = [D P_p u(content) for p in pools]
int lap_target_launch(hipStream_t s, const float *content, int H, int W, const LapLevels &lv,
                      float *target, float *scratch);
// grad += sum_p 2 coefs[p] (D e_p) / (n_cell 382.5) per pixel, loss_terms[p] = sum e_p^2
int lap_launch(hipStream_t s, const float *img, float *grad, int H, int W, const LapLevels &lv,
               size_t map_floats, const float *coefs, const float *target, double *loss_terms,
               float *scratch);

// photo.hip: the photorealism regulariser (the matting Laplacian's quadratic form, matrix-free).
// grad += 2 scale (L v_c) / 255 per plane, *loss_term = sum over planes and windows of
// [sum r^2 + eps |a|^2] (without scale); scratch holds photo_blocks(H, W) <= kBlocks floats.
int photo_blocks(int H, int W);
int photo_launch(hipStream_t s, const float *img, const float *content, float *grad, int H, int W,
                 double eps, double scale, double *loss_term, float *scratch);

// temporal.hip: the temporal-consistency term.  flow_warp_launch composites one earlier frame warped by a flow
// into target / weight (H, W >= 2; flow_f may be null); temporal_launch adds the masked term's gradient and leaves
// *loss_term = sum w' d^2 (without scale * 63.75); scratch holds kBlocks floats.
int flow_warp_launch(hipStream_t s, const float *prev, const float *flow_b, const float *flow_f, int H, int W,
                     double su, double sv, int first, float *target, float *weight);
int temporal_launch(hipStream_t s, const float *img, float *grad, const float *target, const float *weight,
                    int H, int W, double scale, double *loss_term, float *scratch);

// flow.hip: the optical-flow estimator (stx_image_flow_estimate; the caller has checked the parameters).
// flow_levels fills the pyramid's sizes (kFlowMaxLevels entries at most) and returns their count; `work` holds
// flow_workspace_doubles(...) doubles and is read and written by the queued launches only.
constexpr int kFlowMaxLevels = 256;
int flow_levels(int H, int W, double eta, int levels, int *hs, int *ws);
size_t flow_workspace_doubles(int H, int W, double eta, int levels);
int flow_estimate_launch(hipStream_t s, const float *I1, const float *I2, int H, int W, const stx_flow_params &p,
                         float *flow_out, double *work);

// poisson.hip: the screened-Poisson output stage (stx_image_poisson; the caller has checked the arguments).
// poisson_levels fills the levels' sizes and lambdas (kPoissonMaxLevels entries at most) and returns their count;
// `work` holds poisson_workspace_doubles(...) doubles and is read and written by the queued launches only.
constexpr int kPoissonMaxLevels = 16;
int poisson_levels(int H, int W, double lambda, int *hs, int *ws, double *lambdas);
size_t poisson_workspace_doubles(int H, int W, double lambda);
int poisson_launch(hipStream_t s, const float *img, const float *content, float *out, int H, int W, double lambda,
                   int cycles, double *work);

// image_ops.hip
int adam_launch(hipStream_t s, float *params, const float *grad, float *g1, float *g2, float *p1,
                float *avg, size_t n, double lr, double b1, double b2, double bp1, double c1,
                double c2, double cp);
int dot_launch(hipStream_t s, const float *x, const float *y, size_t n, double *out_dev,
               float *scratch, size_t scratch_floats);
int abs_sum_launch(hipStream_t s, const float *x, size_t n, double *out_dev, float *scratch,
                   size_t scratch_floats);
int axpy_launch(hipStream_t s, float a, const float *x, float *y, size_t n);
int scale_launch(hipStream_t s, float a, float *x, size_t n);
int axpy_dev_launch(hipStream_t s, double c1, const double *a, double da, double c2, const double *b,
                    double db, const float *x, float *y, size_t n);
int scale_dev_launch(hipStream_t s, double c, const double *den, double den_div, float *x, size_t n);
// fused passes of the L-BFGS step (image_ops.hip): bit for bit the separate launches they replace
int axpy_dot_dev_launch(hipStream_t s, double c1, const double *a, double da, double c2, const double *b,
                        double db, double c_s, const double *den_s, double div_s, const float *x,
                        const float *src, float *y, const float *z, size_t n, double *out_dev, float *scratch,
                        size_t scratch_floats);
int lbfgs_pair_launch(hipStream_t s, const float *g_new, float *g_old, const float *sv, float *y, size_t n,
                      double *out_dev2, float *scratch, size_t scratch_floats);
int scale2_axpy_launch(hipStream_t s, float c1, float c2, float *sv, float *params, size_t n);
int step_stats_launch(hipStream_t s, const float *avg, float *old, int H, int W,
                      double *out_dev /*[2]*/, float *scratch, size_t scratch_floats);
int to_u8_launch(hipStream_t s, const float *img, int H, int W, const float mean[3], uint8_t *out);
// --preserve-color: the luminance of img on the chroma of content as RGB HWC bytes; the nine colour sums
// (b, g, r, bb, bg, br, gg, gr, rr) of img into out_dev; dst = clip(A src + b + mean, 0, 255) - mean
int to_u8_luma_launch(hipStream_t s, const float *img, const float *content, int H, int W,
                      const float mean[3], uint8_t *out);
int color_stats_launch(hipStream_t s, const float *img, int H, int W, double *out_dev /*[9]*/,
                       float *scratch, size_t scratch_floats);
int color_affine_launch(hipStream_t s, const float *src, float *dst, int H, int W, const double A[9],
                        const double b[3], const float mean[3]);

}  // namespace stx
