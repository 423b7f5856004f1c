// The photorealism regulariser (Luan, Paris, Shechtman, Bala, "Deep Photo Style Transfer", 2017): the
// iterate is held to what is locally an affine function of the content picture's colours, the
// quadratic form of the matting Laplacian (Levin, Lischinski, Weiss, "A Closed-Form Solution to
// Natural Image Matting", 2008) without the matrix.  Pictures are [3][H][W] planes, un-rolled;
// I = content / 255 (a constant offset of I changes nothing, so the mean stays off), v = x_c / 255
// for a plane c of the iterate, and for every 3 x 3 window w_k that lies inside the picture
//     mu_k = mean_w I               m_k = mean_w v
//     S_k  = mean_w (I - mu_k)(I - mu_k)^T           (3 x 3, shared by the three planes)
//     q_k  = mean_w (I - mu_k)(v - m_k)
//     a_k  = (S_k + (eps / 9) Id)^-1 q_k
//     r_ki = (v_i - m_k) - a_k . (I_i - mu_k)        for the nine pixels i of w_k
//     loss = scale * sum_c sum_k [ sum_i r_ki^2 + eps |a_k|^2 ]
//     grad[c][i] += scale * 2 * (sum over the windows k that hold i of r_ki) / 255
// A corner pixel is in one window, an interior pixel in nine.
//
// The kernel works in the pictures' own units: with I' = 255 I and v' = 255 v, S' = 255^2 S and
// q' = 255^2 q, so a_k = (S' + (255^2 eps / 9) Id)^-1 q' is unchanged and r' = 255 r; no pixel is divided.
//
// Precision is the design.  At eps = 1e-7 the regularised covariance has a condition number near 1e7
// wherever a window's colours lie on a line, which is the rule in a photograph, and window algebra in
// float32 is off by 2.6e-3 of max|Lv|.  So everything between the float32 pictures and the float32
// gradient is float64: the means, the covariance, an LDL^T factorisation (the adjugate loses
// cond^2 * 2^-53 in the determinant), a_k, the centred residuals and their nine-term sums; b_k = m_k -
// a_k . mu_k, which cancels, is never formed.  The sum of a pixel is rounded to float32 once and added
// once to the gradient element.
//
// One pass, nothing stored between calls (S_k^-1 is recomputed from the content picture: 48 B / pixel of
// stored inverses would double the traffic of the call).  A workgroup of 256 threads owns a 30 x 6
// tile of pixels at a time (grid-stride over the tiles):
//   stage    the six planes of the 34 x 10 pixels within 2 of the tile -> LDS (zero outside the picture)
//   windows  thread t owns the window centred at tile column (t & 31) - 1, row (t >> 5) - 1: the
//            32 x 8 windows within 1 of the tile.  mu, S, the factorisation once; m, q, a per plane;
//            mu (3), m (3) and a (9) as doubles -> LDS, one array per coefficient so that neighbouring
//            lanes read neighbouring doubles.  The window adds eps |a|^2 if its centre is in the tile.
//   pixels   thread t < 180 owns a pixel: the residuals of the (up to) nine windows around it in a fixed
//            order, their squares into the loss, their sum into the gradient.
// Every (window, pixel) pair and every window is counted by exactly one workgroup.  The loss is kept
// per thread in double across its tiles, reduced per workgroup in float and finished in double by
// finish_partials_kernel.  No atomics: the same inputs give the same bits.
//
// The file is compiled with -ffp-contract=off, like lap.hip: what is fused is written as fma().

#include <algorithm>
#include <cstdint>

#include "common.h"

namespace stx {

namespace {

constexpr int kTileW = 30, kTileH = 6;              // pixels a workgroup owns at a time
constexpr int kWinW = kTileW + 2, kWinH = kTileH + 2;   // windows within 1 of them: 32 x 8 = 256
constexpr int kPixW = kTileW + 4, kPixH = kTileH + 4;   // pixels within 2 of them: 34 x 10
constexpr int kWins = kWinW * kWinH;
constexpr int kPixRow = kPixW + 1;                  // (row stride of the staged planes, odd)
static_assert(kWins == 256, "one window per thread");

__global__ __launch_bounds__(256) void photo_kernel(const float *__restrict__ img,
                                                    const float *__restrict__ content,
                                                    float *__restrict__ grad, int H, int W, int tiles_x,
                                                    int tiles, double eps, double eps_units,
                                                    double grad_coef, float *__restrict__ partials) {
    __shared__ float s_px[6][kPixH][kPixRow];       // planes 0..2: content, 3..5: the iterate
    __shared__ double s_mu[3][kWins], s_m[3][kWins], s_a[9][kWins];
    const int t = threadIdx.x;
    const size_t plane = (size_t)H * W;
    double acc = 0.0;                               // sum r'^2 of this thread's pixels, in units^2
    double acc_a = 0.0;                             // sum |a|^2 of this thread's windows
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int X0 = (tile % tiles_x) * kTileW, Y0 = (tile / tiles_x) * kTileH;
        // ---- stage
        for (int i = t; i < 6 * kPixH * kPixW; i += 256) {
            const int p = i / (kPixH * kPixW), rem = i - p * (kPixH * kPixW);
            const int ly = rem / kPixW, lx = rem - ly * kPixW;
            const int y = Y0 - 2 + ly, x = X0 - 2 + lx;
            float val = 0.f;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const float *src = p < 3 ? content + p * plane : img + (p - 3) * plane;
                val = src[(size_t)y * W + x];
            }
            s_px[p][ly][lx] = val;
        }
        __syncthreads();
        // ---- windows
        {
            const int wx = t & (kWinW - 1), wy = t / kWinW;
            const int cx = X0 - 1 + wx, cy = Y0 - 1 + wy;
            if (cx >= 1 && cx <= W - 2 && cy >= 1 && cy <= H - 2) {
                double d[3][9], mu[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double s = 0.0;
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        d[c][j] = (double)s_px[c][wy + j / 3][wx + j % 3];
                        s += d[c][j];
                    }
                    mu[c] = s / 9.0;
#pragma unroll
                    for (int j = 0; j < 9; ++j) d[c][j] -= mu[c];
                    s_mu[c][t] = mu[c];
                }
                double s00 = 0, s10 = 0, s11 = 0, s20 = 0, s21 = 0, s22 = 0;
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    s00 = fma(d[0][j], d[0][j], s00);
                    s10 = fma(d[1][j], d[0][j], s10);
                    s11 = fma(d[1][j], d[1][j], s11);
                    s20 = fma(d[2][j], d[0][j], s20);
                    s21 = fma(d[2][j], d[1][j], s21);
                    s22 = fma(d[2][j], d[2][j], s22);
                }
                // S' + eps' Id = L D L^T (positive definite: every pivot is at least eps')
                const double d0 = s00 / 9.0 + eps_units;
                const double l10 = (s10 / 9.0) / d0, l20 = (s20 / 9.0) / d0;
                const double d1 = fma(-l10, s10 / 9.0, s11 / 9.0 + eps_units);
                const double u21 = fma(-l20, s10 / 9.0, s21 / 9.0);
                const double l21 = u21 / d1;
                const double d2 = fma(-l21, u21, fma(-l20, s20 / 9.0, s22 / 9.0 + eps_units));
                const bool mine = wx >= 1 && wx <= kTileW && wy >= 1 && wy <= kTileH;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double v[9], s = 0.0;
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        v[j] = (double)s_px[3 + c][wy + j / 3][wx + j % 3];
                        s += v[j];
                    }
                    const double m = s / 9.0;
                    double q0 = 0, q1 = 0, q2 = 0;
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        const double dv = v[j] - m;
                        q0 = fma(d[0][j], dv, q0);
                        q1 = fma(d[1][j], dv, q1);
                        q2 = fma(d[2][j], dv, q2);
                    }
                    const double y0 = q0 / 9.0;
                    const double y1 = fma(-l10, y0, q1 / 9.0);
                    const double y2 = fma(-l21, y1, fma(-l20, y0, q2 / 9.0));
                    const double a2 = y2 / d2;
                    const double a1 = fma(-l21, a2, y1 / d1);
                    const double a0 = fma(-l20, a2, fma(-l10, a1, y0 / d0));
                    s_m[c][t] = m;
                    s_a[3 * c + 0][t] = a0;
                    s_a[3 * c + 1][t] = a1;
                    s_a[3 * c + 2][t] = a2;
                    if (mine) acc_a += fma(a0, a0, fma(a1, a1, a2 * a2));
                }
            }
        }
        __syncthreads();
        // ---- pixels
        if (t < kTileW * kTileH) {
            const int ty = t / kTileW, tx = t - ty * kTileW;
            const int x = X0 + tx, y = Y0 + ty;
            if (x < W && y < H) {
                double ci[3], vi[3], sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    ci[c] = (double)s_px[c][ty + 2][tx + 2];
                    vi[c] = (double)s_px[3 + c][ty + 2][tx + 2];
                }
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int cx = x + dx, cy = y + dy;
                        if (cx < 1 || cx > W - 2 || cy < 1 || cy > H - 2) continue;
                        const int k = (ty + 1 + dy) * kWinW + tx + 1 + dx;
                        const double e0 = ci[0] - s_mu[0][k], e1 = ci[1] - s_mu[1][k], e2 = ci[2] - s_mu[2][k];
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const double fit = fma(s_a[3 * c + 2][k], e2,
                                                   fma(s_a[3 * c + 1][k], e1, s_a[3 * c][k] * e0));
                            const double r = (vi[c] - s_m[c][k]) - fit;
                            sum[c] += r;
                            acc = fma(r, r, acc);
                        }
                    }
                }
                const size_t at = (size_t)y * W + x;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float g = (float)(sum[c] * grad_coef);
                    grad[c * plane + at] = grad[c * plane + at] + g;
                }
            }
        }
        __syncthreads();        // (the next tile's staging overwrites what the pixels read)
    }
    float term[1] = {(float)(acc / 65025.0 + eps * acc_a)};
    block_partials<1>(term, partials);
}

}  // namespace

int photo_blocks(int H, int W) {
    const size_t tiles = (size_t)ceil_div(W, kTileW) * ceil_div(H, kTileH);
    return (int)std::min<size_t>(tiles, (size_t)kBlocks);
}

int photo_launch(hipStream_t s, const float *img, const float *content, float *grad, int H, int W,
                 double eps, double scale, double *loss_term, float *scratch) {
    const int tiles_x = ceil_div(W, kTileW);
    const size_t tiles = (size_t)tiles_x * ceil_div(H, kTileH);
    if (tiles > (size_t)INT32_MAX) {
        set_error("photo: %zu tiles in a %d x %d picture (at most 2^31 - 1)", tiles, H, W);
        return STX_ERR_ARG;
    }
    const int blocks = photo_blocks(H, W);
    photo_kernel<<<blocks, 256, 0, s>>>(img, content, grad, H, W, tiles_x, (int)tiles, eps,
                                        eps * 65025.0 / 9.0, 2.0 * scale / 65025.0, scratch);
    STX_CHECK_LAUNCH();
    return finish_partials_launch(s, scratch, blocks, loss_term);
}

}  // namespace stx
