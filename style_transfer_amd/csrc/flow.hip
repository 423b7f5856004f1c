// Optical flow for the temporal term's --prev-contents: the robust variational method of Brox, Bruhn,
// Papenberg, Weickert (ECCV 2004) in the discretisation of Sanchez, Monzon, Salgado ("Robust Optical Flow
// Estimation", IPOL 2013) -- coarse to fine with warping, a lagged nonlinearity and red-black SOR with fixed
// iteration counts.  stx.h states the definition operation by operation; tests/flow_ref.py restates it in numpy.
//
// Every value between the float32 inputs and the float32 output is float64, and the file is compiled with
// -ffp-contract=off: each operation rounds once, in the order written, so the result is the reference's.  No
// atomics, no reductions, no stopping test: the same inputs give the same bits, and the host waits for nothing.
//
// Kernels (256 threads as 64 x 4 pixels; a thread owns one pixel, no grid-stride loop):
//   flow_to_double_kernel      I1, I2 float32 -> level 0 of the pyramid
//   flow_gauss_rows_kernel     the Gaussian along x, both pictures in one launch
//   flow_gauss_cols_resample_kernel   the Gaussian along y evaluated at the four taps of each pixel of the
//                              next level, and their bilinear mix: the column-filtered picture is never stored
//   flow_zero_kernel           u = v = 0 at the coarsest level
//   flow_derivatives_kernel    Ax, Ay, Bx, By, Bxx, Bxy, Byy (the second differences nest the first)
//   flow_warp_kernel           six planes of B sampled at p + (u, v) in one pass; leaves Iz, Ix, Iy, Ixz, Iyz,
//                              Ixx, Ixy, Iyy, du = dv = 0 and S = (u, v)
//   flow_psi_kernel            psiS from the central differences of S = (u + du, v + dv)
//   flow_coeff_kernel          psiD, the four neighbour weights, A11, A12, A22, c1, c2
//   flow_sweep_kernel          one red-black half-sweep
//   flow_up_kernel             the flow's way up a level
//   flow_out_kernel            float32 of the finest level's flow
// `u += du` needs no kernel: a half-sweep keeps S = u + du beside du, so that a neighbour costs one read per
// component instead of two, and after the last sweep S *is* the new u -- the host swaps the two pointers.
//
// Bytes per pixel of the half-sweep (the hot kernel: outer * inner * sor * 2 launches per level).  An active
// pixel reads du, dv, u, v (32 B), four neighbours' Su and Sv (64 B), four weights (32 B), A11, A12, A22, c1, c2
// (40 B) and writes du, dv, Su, Sv (32 B): 200 B.  The neighbours are the other colour's pixels and the own
// planes are read with a stride of two doubles, so a half-sweep touches every 128-byte line of the 17 planes
// once: counted per pixel of the level (both colours) that is 17 * 8 = 136 B read and 32 B written, 168 B, for
// one half-sweep; DESIGN.md 3.25 holds this against what was measured.

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"

namespace stx {

namespace {

constexpr int kFlowMaxTaps = 15;    // eta > 0.25: sigma < 2.33, radius <= 7

struct FlowTaps {
    double w[kFlowMaxTaps];
    int n;                          // 2 r + 1
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The bilinear mix, exact at fx, fy in {0, 1} (a zero flow samples a picture's own values, the last row and
// column included, where the taps start one pixel before).
__device__ __forceinline__ double mix(double p00, double p01, double p10, double p11, double fx, double fy) {
    const double top = (1.0 - fx) * p00 + fx * p01, bottom = (1.0 - fx) * p10 + fx * p11;
    return (1.0 - fy) * top + fy * bottom;
}

// Clamped coordinate -> first tap and fraction: x0 = min(floor(q), n - 2) (n >= 2).
__device__ __forceinline__ void tap(double q, int n, int &i0, double &f) {
    q = fmin(fmax(q, 0.0), (double)(n - 1));
    const int fl = (int)floor(q);
    i0 = fl < n - 2 ? fl : n - 2;
    f = q - (double)i0;
}

__device__ __forceinline__ bool pixel(int H, int W, int &x, int &y) {
    x = blockIdx.x * 64 + threadIdx.x;
    y = blockIdx.y * 4 + threadIdx.y;
    return x < W && y < H;
}

__global__ __launch_bounds__(256) void flow_to_double_kernel(const float *__restrict__ I1, const float *__restrict__ I2,
                                                             int H, int W, double *__restrict__ A,
                                                             double *__restrict__ B) {
    int x, y;
    if (!pixel(H, W, x, y)) return;
    const size_t i = (size_t)y * W + x;
    A[i] = (double)I1[i];
    B[i] = (double)I2[i];
}

__global__ __launch_bounds__(256) void flow_zero_kernel(int H, int W, double *__restrict__ u, double *__restrict__ v) {
    int x, y;
    if (!pixel(H, W, x, y)) return;
    const size_t i = (size_t)y * W + x;
    u[i] = 0.0;
    v[i] = 0.0;
}

// blockIdx.z: the picture (A or B).
__global__ __launch_bounds__(256) void flow_gauss_rows_kernel(const double *__restrict__ src0, const double *__restrict__ src1,
                                                              int H, int W, FlowTaps k, double *__restrict__ dst0,
                                                              double *__restrict__ dst1) {
    int x, y;
    if (!pixel(H, W, x, y)) return;
    const double *src = (blockIdx.z ? src1 : src0) + (size_t)y * W;
    const int r = k.n >> 1;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < kFlowMaxTaps; ++i)
        if (i < k.n) acc = acc + k.w[i] * src[clampi(x + i - r, W - 1)];
    (blockIdx.z ? dst1 : dst0)[(size_t)y * W + x] = acc;
}

__device__ __forceinline__ double gauss_col(const double *__restrict__ rows, int H, int W, int x, int y,
                                            const FlowTaps &k) {
    const int r = k.n >> 1;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < kFlowMaxTaps; ++i)
        if (i < k.n) acc = acc + k.w[i] * rows[(size_t)clampi(y + i - r, H - 1) * W + x];
    return acc;
}

// rows: the row-filtered pictures [H][W]; dst: the next level [h][w].
__global__ __launch_bounds__(256) void flow_gauss_cols_resample_kernel(const double *__restrict__ rows0,
                                                                       const double *__restrict__ rows1, int H, int W,
                                                                       FlowTaps k, int h, int w, double sx, double sy,
                                                                       double *__restrict__ dst0,
                                                                       double *__restrict__ dst1) {
    int x, y;
    if (!pixel(h, w, x, y)) return;
    const double *rows = blockIdx.z ? rows1 : rows0;
    int x0, y0;
    double fx, fy;
    tap(((double)x + 0.5) * sx - 0.5, W, x0, fx);
    tap(((double)y + 0.5) * sy - 0.5, H, y0, fy);
    const double p00 = gauss_col(rows, H, W, x0, y0, k), p01 = gauss_col(rows, H, W, x0 + 1, y0, k);
    const double p10 = gauss_col(rows, H, W, x0, y0 + 1, k), p11 = gauss_col(rows, H, W, x0 + 1, y0 + 1, k);
    (blockIdx.z ? dst1 : dst0)[(size_t)y * w + x] = mix(p00, p01, p10, p11, fx, fy);
}

// Central differences over a replicated border, halved.
__device__ __forceinline__ double dx_at(const double *__restrict__ p, int W, int x, int y) {
    const double *row = p + (size_t)y * W;
    return (row[x < W - 1 ? x + 1 : W - 1] - row[x > 0 ? x - 1 : 0]) / 2.0;
}

__device__ __forceinline__ double dy_at(const double *__restrict__ p, int H, int W, int x, int y) {
    return (p[(size_t)(y < H - 1 ? y + 1 : H - 1) * W + x] - p[(size_t)(y > 0 ? y - 1 : 0) * W + x]) / 2.0;
}

struct FlowDerivs {
    double *Ax, *Ay, *Bx, *By, *Bxx, *Bxy, *Byy;
};

__global__ __launch_bounds__(256) void flow_derivatives_kernel(const double *__restrict__ A, const double *__restrict__ B,
                                                               int H, int W, FlowDerivs d) {
    int x, y;
    if (!pixel(H, W, x, y)) return;
    const size_t i = (size_t)y * W + x;
    const int xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1;
    const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1;
    d.Ax[i] = dx_at(A, W, x, y);
    d.Ay[i] = dy_at(A, H, W, x, y);
    d.Bx[i] = dx_at(B, W, x, y);
    d.By[i] = dy_at(B, H, W, x, y);
    d.Bxx[i] = (dx_at(B, W, xp, y) - dx_at(B, W, xm, y)) / 2.0;
    d.Bxy[i] = (dx_at(B, W, x, yp) - dx_at(B, W, x, ym)) / 2.0;
    d.Byy[i] = (dy_at(B, H, W, x, yp) - dy_at(B, H, W, x, ym)) / 2.0;
}

struct FlowWarped {
    double *Iz, *Ix, *Iy, *Ixz, *Iyz, *Ixx, *Ixy, *Iyy;
};

struct FlowIterate {
    double *u, *v, *du, *dv, *Su, *Sv;
};

__device__ __forceinline__ double sample(const double *__restrict__ p, size_t t00, int W, double fx, double fy) {
    return mix(p[t00], p[t00 + 1], p[t00 + W], p[t00 + W + 1], fx, fy);
}

__global__ __launch_bounds__(256) void flow_warp_kernel(const double *__restrict__ A, const double *__restrict__ B, int H,
                                                        int W, FlowDerivs d, FlowIterate it, FlowWarped o) {
    int x, y;
    if (!pixel(H, W, x, y)) return;
    const size_t i = (size_t)y * W + x;
    const double u = it.u[i], v = it.v[i];
    int x0, y0;
    double fx, fy;
    tap((double)x + u, W, x0, fx);
    tap((double)y + v, H, y0, fy);
    const size_t t00 = (size_t)y0 * W + x0;
    const double Ix = sample(d.Bx, t00, W, fx, fy), Iy = sample(d.By, t00, W, fx, fy);
    o.Iz[i] = sample(B, t00, W, fx, fy) - A[i];
    o.Ix[i] = Ix;
    o.Iy[i] = Iy;
    o.Ixz[i] = Ix - d.Ax[i];
    o.Iyz[i] = Iy - d.Ay[i];
    o.Ixx[i] = sample(d.Bxx, t00, W, fx, fy);
    o.Ixy[i] = sample(d.Bxy, t00, W, fx, fy);
    o.Iyy[i] = sample(d.Byy, t00, W, fx, fy);
    it.du[i] = 0.0;
    it.dv[i] = 0.0;
    it.Su[i] = u;       // (u + 0)
    it.Sv[i] = v;
}

__global__ __launch_bounds__(256) void flow_psi_kernel(const double *__restrict__ Su, const double *__restrict__ Sv, int H,
                                                       int W, double eps2, double *__restrict__ psi_s) {
    int x, y;
    if (!pixel(H, W, x, y)) return;
    const double ux = dx_at(Su, W, x, y), uy = dy_at(Su, H, W, x, y);
    const double vx = dx_at(Sv, W, x, y), vy = dy_at(Sv, H, W, x, y);
    psi_s[(size_t)y * W + x] = 0.5 / sqrt((((ux * ux + uy * uy) + vx * vx) + vy * vy) + eps2);
}

struct FlowSystem {
    double *gl, *gr, *gu, *gd, *A11, *A12, *A22, *c1, *c2;
};

__global__ __launch_bounds__(256) void flow_coeff_kernel(FlowWarped in, const double *__restrict__ du_,
                                                         const double *__restrict__ dv_,
                                                         const double *__restrict__ psi_s, int H, int W, double alpha,
                                                         double gamma, double eps2, FlowSystem o) {
    int x, y;
    if (!pixel(H, W, x, y)) return;
    const size_t i = (size_t)y * W + x;
    const double du = du_[i], dv = dv_[i];
    const double Iz = in.Iz[i], Ix = in.Ix[i], Iy = in.Iy[i], Ixz = in.Ixz[i], Iyz = in.Iyz[i];
    const double Ixx = in.Ixx[i], Ixy = in.Ixy[i], Iyy = in.Iyy[i];
    const double b = (Iz + Ix * du) + Iy * dv;
    const double gx = (Ixz + Ixx * du) + Ixy * dv;
    const double gy = (Iyz + Ixy * du) + Iyy * dv;
    const double psi_d = 0.5 / sqrt((b * b + gamma * (gx * gx + gy * gy)) + eps2);
    const double ps = psi_s[i];
    o.gl[i] = x > 0 ? (alpha * (ps + psi_s[i - 1])) / 2.0 : 0.0;
    o.gr[i] = x < W - 1 ? (alpha * (ps + psi_s[i + 1])) / 2.0 : 0.0;
    o.gu[i] = y > 0 ? (alpha * (ps + psi_s[i - W])) / 2.0 : 0.0;
    o.gd[i] = y < H - 1 ? (alpha * (ps + psi_s[i + W])) / 2.0 : 0.0;
    o.A11[i] = psi_d * (Ix * Ix + gamma * (Ixx * Ixx + Ixy * Ixy));
    o.A12[i] = psi_d * (Ix * Iy + gamma * (Ixx * Ixy + Ixy * Iyy));
    o.A22[i] = psi_d * (Iy * Iy + gamma * (Ixy * Ixy + Iyy * Iyy));
    o.c1[i] = psi_d * (Ix * Iz + gamma * (Ixx * Ixz + Ixy * Iyz));
    o.c2[i] = psi_d * (Iy * Iz + gamma * (Ixy * Ixz + Iyy * Iyz));
}

// One half-sweep: the pixels with (x + y + colour) even.  A thread owns the pixel 2 * slot + parity of its row;
// its neighbours are of the other colour, which this launch only reads.
__global__ __launch_bounds__(256) void flow_sweep_kernel(FlowSystem s, FlowIterate it, int H, int W, int colour,
                                                         double omega, double om1) {
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (y >= H) return;
    const int x = 2 * (blockIdx.x * 64 + threadIdx.x) + ((y + colour) & 1);
    if (x >= W) return;
    const size_t i = (size_t)y * W + x;
    const size_t l = x > 0 ? i - 1 : i, r = x < W - 1 ? i + 1 : i;      // (a neighbour outside has weight 0)
    const size_t a = y > 0 ? i - W : i, b = y < H - 1 ? i + W : i;
    const double gl = s.gl[i], gr = s.gr[i], gu = s.gu[i], gd = s.gd[i];
    const double gs = ((gl + gr) + gu) + gd;
    const double u = it.u[i], v = it.v[i], du = it.du[i], dv = it.dv[i];
    const double A12 = s.A12[i];
    const double su = ((gl * it.Su[l] + gr * it.Su[r]) + gu * it.Su[a]) + gd * it.Su[b];
    const double new_du = om1 * du + omega * ((((su - gs * u) - A12 * dv) - s.c1[i]) / (s.A11[i] + gs));
    const double sv = ((gl * it.Sv[l] + gr * it.Sv[r]) + gu * it.Sv[a]) + gd * it.Sv[b];
    const double new_dv = om1 * dv + omega * ((((sv - gs * v) - A12 * new_du) - s.c2[i]) / (s.A22[i] + gs));
    it.du[i] = new_du;
    it.dv[i] = new_dv;
    it.Su[i] = u + new_du;
    it.Sv[i] = v + new_dv;
}

// The coarser level's flow [h][w] sampled on this level's grid [H][W], times (W / w, H / h).
__global__ __launch_bounds__(256) void flow_up_kernel(const double *__restrict__ cu, const double *__restrict__ cv, int h,
                                                      int w, int H, int W, double sx, double sy, double mx, double my,
                                                      double *__restrict__ u, double *__restrict__ v) {
    int x, y;
    if (!pixel(H, W, x, y)) return;
    int x0, y0;
    double fx, fy;
    tap(((double)x + 0.5) * sx - 0.5, w, x0, fx);
    tap(((double)y + 0.5) * sy - 0.5, h, y0, fy);
    const size_t t00 = (size_t)y0 * w + x0, i = (size_t)y * W + x;
    u[i] = sample(cu, t00, w, fx, fy) * mx;
    v[i] = sample(cv, t00, w, fx, fy) * my;
}

__global__ __launch_bounds__(256) void flow_out_kernel(const double *__restrict__ u, const double *__restrict__ v, int H,
                                                       int W, float *__restrict__ out) {
    int x, y;
    if (!pixel(H, W, x, y)) return;
    const size_t i = (size_t)y * W + x, plane = (size_t)H * W;
    out[i] = (float)u[i];
    out[plane + i] = (float)v[i];
}

inline dim3 grid_for(int H, int W, int z = 1) { return dim3((unsigned)ceil_div(W, 64), (unsigned)ceil_div(H, 4), (unsigned)z); }

constexpr int kFullPlanes = 33;     // what a level needs beside the pyramid, each of the input's size

}  // namespace

int flow_levels(int H, int W, double eta, int levels, int *hs, int *ws) {
    int n = 1;
    hs[0] = H;
    ws[0] = W;
    while (n < levels && n < kFlowMaxLevels) {
        const int h = (int)std::floor((double)hs[n - 1] * eta + 0.5), w = (int)std::floor((double)ws[n - 1] * eta + 0.5);
        if ((h < w ? h : w) < 16) break;
        hs[n] = h;
        ws[n] = w;
        ++n;
    }
    return n;
}

size_t flow_workspace_doubles(int H, int W, double eta, int levels) {
    int hs[kFlowMaxLevels], ws[kFlowMaxLevels];
    const int n = flow_levels(H, W, eta, levels, hs, ws);
    size_t pyramid = 0;
    for (int k = 0; k < n; ++k) pyramid += 2 * (size_t)hs[k] * ws[k];
    return pyramid + (size_t)kFullPlanes * H * W;
}

int flow_estimate_launch(hipStream_t s, const float *I1, const float *I2, int H, int W, const stx_flow_params &p,
                         float *flow_out, double *work) {
    int hs[kFlowMaxLevels], ws[kFlowMaxLevels];
    const int n = flow_levels(H, W, p.eta, p.levels, hs, ws);
    const size_t plane = (size_t)H * W;
    // ---- the workspace: the pyramid, then kFullPlanes planes of the input's size
    double *A[kFlowMaxLevels], *B[kFlowMaxLevels];
    double *at = work;
    for (int k = 0; k < n; ++k) {
        A[k] = at;
        B[k] = at + (size_t)hs[k] * ws[k];
        at += 2 * (size_t)hs[k] * ws[k];
    }
    double *planes[kFullPlanes];
    for (int k = 0; k < kFullPlanes; ++k) planes[k] = at + k * plane;
    FlowDerivs d = {planes[0], planes[1], planes[2], planes[3], planes[4], planes[5], planes[6]};
    FlowWarped wp = {planes[7], planes[8], planes[9], planes[10], planes[11], planes[12], planes[13], planes[14]};
    FlowSystem sys = {planes[15], planes[16], planes[17], planes[18], planes[19], planes[20], planes[21], planes[22],
                      planes[23]};
    FlowIterate it = {planes[24], planes[25], planes[26], planes[27], planes[28], planes[29]};
    double *psi_s = planes[30], *cu = planes[31], *cv = planes[32];
    double *rows0 = sys.gl, *rows1 = sys.gr;        // (the Gaussian's row pass: free until the first level is solved)

    // ---- the Gaussian's weights: sigma = 0.6 sqrt(eta^-2 - 1), radius ceil(3 sigma), normalised
    FlowTaps taps;
    const double sigma = 0.6 * std::sqrt(1.0 / (p.eta * p.eta) - 1.0);
    const int radius = (int)std::ceil(3.0 * sigma);
    taps.n = 2 * radius + 1;
    if (taps.n > kFlowMaxTaps) {
        set_error("stx_image_flow_estimate: eta %g gives a Gaussian of %d taps, above %d", p.eta, taps.n, kFlowMaxTaps);
        return STX_ERR_ARG;
    }
    double total = 0.0;
    for (int i = 0; i < kFlowMaxTaps; ++i) {
        const int o = i - radius;
        taps.w[i] = i < taps.n ? std::exp(-(double)(o * o) / (2.0 * sigma * sigma)) : 0.0;
        if (i < taps.n) total = total + taps.w[i];
    }
    for (int i = 0; i < taps.n; ++i) taps.w[i] = taps.w[i] / total;

    const dim3 block(64, 4);
    flow_to_double_kernel<<<grid_for(H, W), block, 0, s>>>(I1, I2, H, W, A[0], B[0]);
    STX_CHECK_LAUNCH();
    for (int k = 1; k < n; ++k) {
        const int sh = hs[k - 1], sw = ws[k - 1];
        flow_gauss_rows_kernel<<<grid_for(sh, sw, 2), block, 0, s>>>(A[k - 1], B[k - 1], sh, sw, taps, rows0, rows1);
        STX_CHECK_LAUNCH();
        flow_gauss_cols_resample_kernel<<<grid_for(hs[k], ws[k], 2), block, 0, s>>>(
            rows0, rows1, sh, sw, taps, hs[k], ws[k], (double)sw / (double)ws[k], (double)sh / (double)hs[k], A[k], B[k]);
        STX_CHECK_LAUNCH();
    }
    const double eps2 = p.eps * p.eps, om1 = 1.0 - p.omega;
    for (int k = n - 1; k >= 0; --k) {
        const int h = hs[k], w = ws[k];
        const dim3 grid = grid_for(h, w), half = grid_for(h, (w + 1) / 2);
        if (k == n - 1) {
            flow_zero_kernel<<<grid, block, 0, s>>>(h, w, it.u, it.v);
            STX_CHECK_LAUNCH();
        } else {
            const int ch = hs[k + 1], cw = ws[k + 1];
            // (the coarser level's result is in it.u / it.v, which this level writes: it moves aside first)
            std::swap(it.u, cu);
            std::swap(it.v, cv);
            flow_up_kernel<<<grid, block, 0, s>>>(cu, cv, ch, cw, h, w, (double)cw / (double)w, (double)ch / (double)h,
                                                  (double)w / (double)cw, (double)h / (double)ch, it.u, it.v);
            STX_CHECK_LAUNCH();
        }
        flow_derivatives_kernel<<<grid, block, 0, s>>>(A[k], B[k], h, w, d);
        STX_CHECK_LAUNCH();
        for (int outer = 0; outer < p.outer; ++outer) {
            flow_warp_kernel<<<grid, block, 0, s>>>(A[k], B[k], h, w, d, it, wp);
            STX_CHECK_LAUNCH();
            for (int inner = 0; inner < p.inner; ++inner) {
                flow_psi_kernel<<<grid, block, 0, s>>>(it.Su, it.Sv, h, w, eps2, psi_s);
                STX_CHECK_LAUNCH();
                flow_coeff_kernel<<<grid, block, 0, s>>>(wp, it.du, it.dv, psi_s, h, w, p.alpha, p.gamma, eps2, sys);
                STX_CHECK_LAUNCH();
                for (int sweep = 0; sweep < p.sor; ++sweep) {
                    flow_sweep_kernel<<<half, block, 0, s>>>(sys, it, h, w, 0, p.omega, om1);
                    flow_sweep_kernel<<<half, block, 0, s>>>(sys, it, h, w, 1, p.omega, om1);
                }
                STX_CHECK_LAUNCH();
            }
            // u += du: S holds u + du already
            std::swap(it.u, it.Su);
            std::swap(it.v, it.Sv);
        }
    }
    flow_out_kernel<<<grid_for(H, W), block, 0, s>>>(it.u, it.v, H, W, flow_out);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

}  // namespace stx
