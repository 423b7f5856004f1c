// The screened-Poisson output stage of --poisson-lambda (Mechrez, Shechtman, Zelnik-Manor, BMVC 2017): per
// channel, e + lambda * (graph Laplacian) e = lambda * (graph Laplacian) (c - s) on the 4-connected grid, solved for
// the correction e from zero by a fixed count of multigrid W-cycles, and out = s + e.  stx.h states the definition
// operation by operation; tests/poisson_ref.py restates it in numpy.
//
// Every value between the float32 inputs and the float32 output is float64, and the file is compiled with
// -ffp-contract=off: each operation rounds once, in the order written, so the result is the reference's.  No
// atomics, no reductions, no stopping test: the same inputs give the same bits, and the host waits for nothing.
//
// Kernels (256 threads as 64 x 4 pixels; a thread owns one pixel of the level it writes, no grid-stride loop;
// blockIdx.z is the channel):
//   poisson_rhs_kernel         b = lambda (n d - S(d)) with d = c - s formed on the fly, e = 0        (level 0)
//   poisson_sweep_kernel       one red-black half-sweep
//   poisson_restrict_kernel    a thread owns a coarse pixel: the residuals of its up to four children, their mean
//                              as the coarse b, and the coarse e = 0 -- the residual is never stored
//   poisson_prolong_kernel     e += the cell-centred bilinear interpolation of the coarse e
//   poisson_out_kernel         out = float32(double(s) + e)
//
// Bytes per pixel and channel of the half-sweep (the hot kernel: 8 launches per visit of a level, 40 at the
// coarsest): an active pixel reads b and its four neighbours' e and writes e.  The neighbours are the other
// colour's pixels, so a half-sweep touches every 128-byte line of e twice (read, written) and of b once: counted
// per pixel of the level (both colours) 24 B; DESIGN.md 3.26 holds this against what was measured.

#include <cmath>
#include <cstdint>

#include "common.h"

namespace stx {

namespace {

constexpr int kPoissonPre = 2, kPoissonPost = 2, kPoissonCoarsest = 20;
constexpr double kPoissonCoarsestLambda = 0.05;

// ((left + right) + up) + down around (x, y) of one plane, +0.0 for a neighbour outside.
__device__ __forceinline__ double neighbour_sum(const double *a, int H, int W, int x, int y, size_t i) {
    const double l = x > 0 ? a[i - 1] : 0.0, r = x < W - 1 ? a[i + 1] : 0.0;
    const double u = y > 0 ? a[i - W] : 0.0, d = y < H - 1 ? a[i + W] : 0.0;
    return ((l + r) + u) + d;
}

__device__ __forceinline__ double neighbour_count(int H, int W, int x, int y) {
    return (double)((x > 0) + (x < W - 1) + (y > 0) + (y < H - 1));
}

__global__ __launch_bounds__(256) void poisson_rhs_kernel(const float *__restrict__ img, const float *__restrict__ content,
                                                          int H, int W, double lambda, double *__restrict__ e,
                                                          double *__restrict__ b) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t plane = (size_t)H * W, i = (size_t)y * W + x;
    const float *s = img + blockIdx.z * plane, *c = content + blockIdx.z * plane;
    const double d = (double)c[i] - (double)s[i];
    const double dl = x > 0 ? (double)c[i - 1] - (double)s[i - 1] : 0.0;
    const double dr = x < W - 1 ? (double)c[i + 1] - (double)s[i + 1] : 0.0;
    const double du = y > 0 ? (double)c[i - W] - (double)s[i - W] : 0.0;
    const double dd = y < H - 1 ? (double)c[i + W] - (double)s[i + W] : 0.0;
    b[blockIdx.z * plane + i] = lambda * (neighbour_count(H, W, x, y) * d - (((dl + dr) + du) + dd));
    e[blockIdx.z * plane + i] = 0.0;
}

// One half-sweep: the pixels with ((y + x) & 1) == colour.  A thread owns the pixel 2 * slot + parity of its row;
// its neighbours are of the other colour, which this launch only reads.
__global__ __launch_bounds__(256) void poisson_sweep_kernel(double *e_, const double *__restrict__ b_, int H, int W,
                                                            double lambda, int colour) {
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (y >= H) return;
    const int x = 2 * (blockIdx.x * 64 + threadIdx.x) + ((y + colour) & 1);
    if (x >= W) return;
    const size_t plane = (size_t)H * W, i = (size_t)y * W + x;
    double *e = e_ + blockIdx.z * plane;
    e[i] = (b_[blockIdx.z * plane + i] + lambda * neighbour_sum(e, H, W, x, y, i)) /
           (1.0 + lambda * neighbour_count(H, W, x, y));
}

__device__ __forceinline__ double residual_at(const double *e, const double *b, int H, int W,
                                              double lambda, int x, int y) {
    if (x >= W || y >= H) return 0.0;
    const size_t i = (size_t)y * W + x;
    return (b[i] + lambda * neighbour_sum(e, H, W, x, y, i)) - (1.0 + lambda * neighbour_count(H, W, x, y)) * e[i];
}

// e, b: level l [H][W]; ec, bc: level l + 1 [h][w] with h = ceil(H / 2), w = ceil(W / 2).
__global__ __launch_bounds__(256) void poisson_restrict_kernel(const double *__restrict__ e_, const double *__restrict__ b_,
                                                               int H, int W, double lambda, int h, int w,
                                                               double *__restrict__ ec, double *__restrict__ bc) {
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y;
    if (X >= w || Y >= h) return;
    const size_t plane = (size_t)H * W;
    const double *e = e_ + blockIdx.z * plane, *b = b_ + blockIdx.z * plane;
    const int x = 2 * X, y = 2 * Y;
    const double r00 = residual_at(e, b, H, W, lambda, x, y), r01 = residual_at(e, b, H, W, lambda, x + 1, y);
    const double r10 = residual_at(e, b, H, W, lambda, x, y + 1), r11 = residual_at(e, b, H, W, lambda, x + 1, y + 1);
    const double count = (double)((1 + (x + 1 < W)) * (1 + (y + 1 < H)));
    const size_t o = blockIdx.z * ((size_t)h * w) + (size_t)Y * w + X;
    bc[o] = (((r00 + r01) + r10) + r11) / count;
    ec[o] = 0.0;
}

// e: level l [H][W]; ec: level l + 1 [h][w].
__global__ __launch_bounds__(256) void poisson_prolong_kernel(double *__restrict__ e, const double *__restrict__ ec_, int H,
                                                              int W, int h, int w) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const double *ec = ec_ + blockIdx.z * ((size_t)h * w);
    const int X = x >> 1, Y = y >> 1;
    int Xn = (x & 1) ? X + 1 : X - 1, Yn = (y & 1) ? Y + 1 : Y - 1;
    Xn = Xn < 0 ? 0 : (Xn > w - 1 ? w - 1 : Xn);
    Yn = Yn < 0 ? 0 : (Yn > h - 1 ? h - 1 : Yn);
    const double top = 0.75 * ec[(size_t)Y * w + X] + 0.25 * ec[(size_t)Y * w + Xn];
    const double other = 0.75 * ec[(size_t)Yn * w + X] + 0.25 * ec[(size_t)Yn * w + Xn];
    const size_t i = blockIdx.z * ((size_t)H * W) + (size_t)y * W + x;
    e[i] = e[i] + (0.75 * top + 0.25 * other);
}

__global__ __launch_bounds__(256) void poisson_out_kernel(const float *__restrict__ img, const double *__restrict__ e, int H,
                                                          int W, float *__restrict__ out) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t i = blockIdx.z * ((size_t)H * W) + (size_t)y * W + x;
    out[i] = (float)((double)img[i] + e[i]);
}

inline dim3 grid_for(int H, int W) { return dim3((unsigned)ceil_div(W, 64), (unsigned)ceil_div(H, 4), 3u); }

struct PoissonLevel {
    int H, W;
    double lambda;
    double *e, *b;      // [3][H][W] each
};

int sweeps(hipStream_t s, const PoissonLevel &l, int count, int first) {
    const dim3 half = grid_for(l.H, (l.W + 1) / 2), block(64, 4);
    for (int k = 0; k < count; ++k) {
        poisson_sweep_kernel<<<half, block, 0, s>>>(l.e, l.b, l.H, l.W, l.lambda, first);
        poisson_sweep_kernel<<<half, block, 0, s>>>(l.e, l.b, l.H, l.W, l.lambda, first ^ 1);
    }
    STX_CHECK_LAUNCH();
    return STX_OK;
}

// One visit of level k (stx.h): the W-cycle visits level k + 1 twice, the first time from zero.
int visit(hipStream_t s, const PoissonLevel *lv, int n, int k) {
    const PoissonLevel &l = lv[k];
    if (k == n - 1) return sweeps(s, l, kPoissonCoarsest, 0);
    const PoissonLevel &c = lv[k + 1];
    const dim3 block(64, 4);
    STX_TRY(sweeps(s, l, kPoissonPre, 0));
    poisson_restrict_kernel<<<grid_for(c.H, c.W), block, 0, s>>>(l.e, l.b, l.H, l.W, l.lambda, c.H, c.W, c.e, c.b);
    STX_CHECK_LAUNCH();
    STX_TRY(visit(s, lv, n, k + 1));
    STX_TRY(visit(s, lv, n, k + 1));
    poisson_prolong_kernel<<<grid_for(l.H, l.W), block, 0, s>>>(l.e, c.e, l.H, l.W, c.H, c.W);
    STX_CHECK_LAUNCH();
    return sweeps(s, l, kPoissonPost, 1);
}

}  // namespace

int poisson_levels(int H, int W, double lambda, int *hs, int *ws, double *lambdas) {
    int n = 1;
    hs[0] = H;
    ws[0] = W;
    lambdas[0] = lambda;
    while (n < kPoissonMaxLevels &&
           !((hs[n - 1] < ws[n - 1] ? hs[n - 1] : ws[n - 1]) <= 2 || lambdas[n - 1] <= kPoissonCoarsestLambda)) {
        hs[n] = (hs[n - 1] + 1) / 2;
        ws[n] = (ws[n - 1] + 1) / 2;
        lambdas[n] = lambdas[n - 1] / 4.0;
        ++n;
    }
    return n;
}

size_t poisson_workspace_doubles(int H, int W, double lambda) {
    int hs[kPoissonMaxLevels], ws[kPoissonMaxLevels];
    double lambdas[kPoissonMaxLevels];
    const int n = poisson_levels(H, W, lambda, hs, ws, lambdas);
    size_t total = 0;
    for (int k = 0; k < n; ++k) total += 2 * 3 * (size_t)hs[k] * ws[k];
    return total;
}

int poisson_launch(hipStream_t s, const float *img, const float *content, float *out, int H, int W, double lambda,
                   int cycles, double *work) {
    int hs[kPoissonMaxLevels], ws[kPoissonMaxLevels];
    double lambdas[kPoissonMaxLevels];
    const int n = poisson_levels(H, W, lambda, hs, ws, lambdas);
    PoissonLevel lv[kPoissonMaxLevels];
    double *at = work;
    for (int k = 0; k < n; ++k) {
        const size_t planes = 3 * (size_t)hs[k] * ws[k];
        lv[k] = {hs[k], ws[k], lambdas[k], at, at + planes};
        at += 2 * planes;
    }
    const dim3 block(64, 4);
    poisson_rhs_kernel<<<grid_for(H, W), block, 0, s>>>(img, content, H, W, lambda, lv[0].e, lv[0].b);
    STX_CHECK_LAUNCH();
    for (int c = 0; c < cycles; ++c) STX_TRY(visit(s, lv, n, 0));
    poisson_out_kernel<<<grid_for(H, W), block, 0, s>>>(img, lv[0].e, H, W, out);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

}  // namespace stx
