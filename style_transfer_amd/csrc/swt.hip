// The SWT regularizer of the reference (style_transfer.py:716-720, num_utils.py:179-196): the whole
// term lives in this file -- one Haar level (the reference's default), Haar at L levels, and the
// orthogonal Daubechies / symlet filters from a table.
//
// Padding, roll, and D = x - B x.  Every channel of img / 127.5 is padded symmetrically to a square
// of side N = 2^ceil(log2(max(H, W))) (an odd amount puts the extra row / column behind),
// transformed with the stationary wavelet transform (periodic on the square), the approximation
// band is dropped and the rest transformed back.  For one Haar level what comes out is
//     D = x - B x,   B = [1 2 1]/4 along rows x [1 2 1]/4 along columns, circular on the square
// (oracle/num_ops.py has the derivation and a band-by-band check).  loss = sum |D|^p over the
// H x W crop; the reference adds the p-norm's OWN gradient at D to the image gradient, not its
// chain through D, and so does this.  The reference transforms the image rolled by the
// iteration's shift; here the image stays un-rolled: pixel (y, x) sits at ((y + ry) mod H,
// (x + rx) mod W) of the rolled picture.  swt_haar_kernel does all of that in one pass.
//
// The L-level triangle.  Level j (j = 1..L) of the stationary Haar transform uses the two-tap
// filters dilated by d = 2^(j-1), periodic on the padded N x N square.  Analysis followed by the
// shift-averaged synthesis of the low band alone is [1 2 1]/4 at stride d, and pywt.iswt2 uses only
// the deepest approximation band, so zeroing the approximation bands removes the path through that
// band alone:
//     D = x - B_L x,   B_L = product over j of ([1 2 1]/4 at stride 2^(j-1)), rows x columns.
// Per axis the product is the triangle T_L[k] = (2^L - |k|) / 4^L, |k| < 2^L
// (tests/swt_levels_ref.py restates it and holds it to a band-by-band filterbank).
//
// Two passes, each a direct triangle out of LDS, so the work per pixel grows like 2^L:
//   pass 1  rows:    R[c][y][x] = sum_k T[k] * x/127.5 at padded column qx + k   -> 3 x H x W floats
//   pass 2  columns: blur = sum_k T[k] * R at padded row qy + k;  D = x/127.5 - blur;
//                    sum |D|^p into per-workgroup partials;  grad += scale * dp_norm(D)
// Every padded coordinate is a copy of a picture coordinate (swt_source), so the row-filtered value
// on a padded row is the row-filtered value on its source row: the intermediate is picture-sized
// and is kept in the un-rolled frame, like the image and the gradient.
//
// A workgroup stages its strip and the halo of 2^L - 1 on either side in LDS; a halo too long for
// the LDS budget (L >= 10 along rows, L >= 7 along columns) is walked in chunks with the taps in
// the same ascending order, so the sums do not depend on the chunking.  The triangle's integer
// numerators are accumulated with one fused multiply-add per tap and scaled by the exact 4^-L at
// the end: no running sums, the rounding error of a pixel is that of its own 2^(L+1) - 1 terms.
//
// The table for dbN / symN.  Per level and axis, analysis followed by the shift-averaged synthesis
// of the low band is r/2 at stride 2^(j-1), r the autocorrelation of the low-pass filter; r depends
// on |H|^2 alone, which dbN and symN share.  The product over the levels is a table of taps built
// on the host (swt_daub_table), already normalised and already folded onto the periodic square, so
// that it never has more than N taps: tap i of `ntaps` is the weight of padded coordinate
// q + i - hl.  The passes are the two above with the weight read from the table, and both walk the
// TAPS in chunks of at most T, ascending: a chunk stages the T taps and the T + tile - 1 slots they
// reach, so every output of the tile takes every tap of the chunk and no tap range depends on the
// thread.
//
// The file is compiled with -ffp-contract=off: D and the p-norm (swt_pnorm) round once per
// operation, like the reference's numpy expressions, in all three forms of the term.

#include <algorithm>

#include "common.h"

namespace stx {

namespace {

constexpr int kRowTile = 256;     // pass 1: output columns per workgroup (one per thread)
constexpr int kRowRows = 4;       //         image rows per workgroup (share the column mapping)
constexpr int kRowChunk = 2048;   //         staged columns per row at most (32 KiB with 4 rows)
constexpr int kColTile = 64;      // pass 2: columns per workgroup (one 256-byte line per row)
constexpr int kColRows = 64;      //         output rows per workgroup, 16 per thread
constexpr int kColChunk = 192;    //         staged rows at most (48 KiB)

__device__ __forceinline__ int swt_source(int q, int pad_lo, int n) {
    // padded coordinate q in [0, N) -> coordinate of the rolled picture (numpy.pad 'symmetric')
    int t = (q - pad_lo) % (2 * n);
    if (t < 0) t += 2 * n;
    return t < n ? t : 2 * n - 1 - t;
}

// un-rolled picture coordinate behind slot `s` of a strip that starts at padded coordinate `q0`
// (q0 may be negative or beyond N: the square is periodic); shift = roll mod n, in [0, n)
__device__ __forceinline__ int swt_unrolled(int q0, int s, int N, int pad_lo, int n, int shift) {
    int q = (q0 + s) % N;
    if (q < 0) q += N;
    const int u = swt_source(q, pad_lo, n) - shift;
    return u < 0 ? u + n : u;
}

// The p-norm at one pixel: |d|^power is added to `sum`; returns the norm's own gradient at d.
__device__ __forceinline__ float swt_pnorm(float d, float power, float &sum) {
    const float ad = fabsf(d);
    float g;
    if (power == 2.f) {
        sum += d * d;
        g = 2.f * d;
    } else if (power == 1.f) {
        sum += ad;
        g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    } else {
        const float ap1 = powf(ad, power - 1.f);
        sum += ap1 * ad;
        g = power * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * ap1;
    }
    return g;
}

// The end of a column pass: one partial per workgroup of its 3-D grid, added in a fixed order
// (finish_partials_launch adds the partials in double).  red: 4 floats of LDS.
__device__ __forceinline__ void swt_cols_partial(float sum, float *red, float *partials) {
    sum = wave_sum_f(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] =
            red[0] + red[1] + red[2] + red[3];
}

// One Haar level in a single pass: a grid-stride loop over the 3 H W pixels, nine loads each.
__global__ __launch_bounds__(256) void swt_haar_kernel(const float *__restrict__ img,
                                                       float *__restrict__ grad, int H, int W, int N,
                                                       int rx, int ry, float scale, float power,
                                                       float *__restrict__ partials) {
    const size_t plane = (size_t)H * W, total = 3 * plane;
    const int pad_y = (N - H) / 2, pad_x = (N - W) / 2;
    float sums[1] = {0.f};
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = i % W;
        const int y = (i / W) % H;
        const int c = i / plane;
        const float *p = img + (size_t)c * plane;
        // position in the rolled picture and on the padded square
        int Y = (y + ry) % H, X = (x + rx) % W;
        if (Y < 0) Y += H;
        if (X < 0) X += W;
        const int qy = Y + pad_y, qx = X + pad_x;
        // rows first (vertical [1 2 1]/4), then columns, like the oracle's two passes
        int uy[3];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int sy = swt_source((qy + dy + N) % N, pad_y, H);
            uy[dy + 1] = (sy - ry) % H;
            if (uy[dy + 1] < 0) uy[dy + 1] += H;
        }
        float cols[3], centre = 0.f;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int sx = swt_source((qx + dx + N) % N, pad_x, W);
            int ux = (sx - rx) % W;
            if (ux < 0) ux += W;
            const float up = p[(size_t)uy[0] * W + ux] / 127.5f, mid = p[(size_t)uy[1] * W + ux] / 127.5f;
            const float down = p[(size_t)uy[2] * W + ux] / 127.5f;
            cols[dx + 1] = (up + 2.f * mid + down) / 4.f;
            if (dx == 0) centre = mid;
        }
        const float blur = (cols[0] + 2.f * cols[1] + cols[2]) / 4.f;
        const float d = centre - blur;
        grad[i] = scale * swt_pnorm(d, power, sums[0]) + grad[i];
    }
    block_partials<1>(sums, partials);
}

// Pass 1.  grid (ceil(W / 256), ceil(H / 4), 3).  Thread t owns column X0 + t of the ROLLED picture
// on four rows; slot s of the strip is padded column X0 + pad_x - h + s, the thread's centre slot is
// t + h.  ONE: the strip fits one chunk (every level the command line is used with).
template <bool ONE>
__global__ __launch_bounds__(256) void swt_rows_kernel(const float *__restrict__ img,
                                                       float *__restrict__ tmp, int H, int W, int N,
                                                       int P, int shift_x, int chunk) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int h = P - 1, span = kRowTile + 2 * h;
    const int X0 = blockIdx.x * kRowTile, y0 = blockIdx.y * kRowRows;
    const int pad_x = (N - W) / 2;
    const float *p = img + (size_t)blockIdx.z * H * W;
    const int t = threadIdx.x;
    float acc[kRowRows] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < span; c0 += chunk) {
        const int len = min(chunk, span - c0);
        if (!ONE) __syncthreads();      // the previous chunk has been read
        for (int s = t; s < len; s += 256) {
            const int ux = swt_unrolled(X0 + pad_x - h, c0 + s, N, pad_x, W, shift_x);
#pragma unroll
            for (int r = 0; r < kRowRows; ++r)
                lds[r * chunk + s] = y0 + r < H ? p[(size_t)(y0 + r) * W + ux] / 127.5f : 0.f;
        }
        __syncthreads();
        // taps k = -h..h whose slot t + h + k lies in [c0, c0 + len)
        const int lo = ONE ? -h : max(-h, c0 - (t + h));
        const int hi = ONE ? h : min(h, c0 + len - 1 - (t + h));
        const float *row = lds + (t + h - c0);
        for (int k = lo; k <= hi; ++k) {
            const float w = (float)(P - abs(k));
#pragma unroll
            for (int r = 0; r < kRowRows; ++r) acc[r] = __builtin_fmaf(w, row[r * chunk + k], acc[r]);
        }
    }
    const int X = X0 + t;
    if (X >= W) return;
    const int x = X - shift_x < 0 ? X - shift_x + W : X - shift_x;
    const float inv = 1.f / ((float)P * (float)P);      // 4^-L, exact
    float *out = tmp + (size_t)blockIdx.z * H * W;
#pragma unroll
    for (int r = 0; r < kRowRows; ++r)
        if (y0 + r < H) out[(size_t)(y0 + r) * W + x] = acc[r] * inv;
}

// Pass 2.  grid (ceil(W / 64), ceil(H / 64), 3).  Thread (col, g) owns column x0 + col (un-rolled:
// columns need no mapping here) and rows Y0 + g + 4 o, o = 0..15, of the ROLLED picture; slot s of
// the strip is padded row Y0 + pad_y - h + s.  A wavefront shares g, so its tap range and weights
// are uniform and its LDS reads are one 256-byte line each.
__global__ __launch_bounds__(256) void swt_cols_kernel(const float *__restrict__ img,
                                                       const float *__restrict__ tmp,
                                                       float *__restrict__ grad, int H, int W, int N,
                                                       int P, int shift_y, int chunk, float scale,
                                                       float power, float *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [chunk][64], then 4 sums
    constexpr int kPer = kColRows / 4;
    const int h = P - 1, span = kColRows + 2 * h;
    const int x0 = blockIdx.x * kColTile, Y0 = blockIdx.y * kColRows;
    const int pad_y = (N - H) / 2;
    const size_t plane = (size_t)H * W;
    const float *r = tmp + blockIdx.z * plane;
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int x = x0 + col;
    float acc[kPer];
#pragma unroll
    for (int o = 0; o < kPer; ++o) acc[o] = 0.f;
    for (int c0 = 0; c0 < span; c0 += chunk) {
        const int len = min(chunk, span - c0);
        if (c0 > 0) __syncthreads();    // the previous chunk has been read
        for (int s = g; s < len; s += 4) {
            const int uy = swt_unrolled(Y0 + pad_y - h, c0 + s, N, pad_y, H, shift_y);
            lds[s * kColTile + col] = x < W ? r[(size_t)uy * W + x] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int o = 0; o < kPer; ++o) {
            const int centre = g + 4 * o + h;       // slot of this output's own row
            const int lo = max(-h, c0 - centre), hi = min(h, c0 + len - 1 - centre);
            const float *column = lds + (centre - c0) * kColTile + col;
            float a = acc[o];
            for (int k = lo; k <= hi; ++k) a = __builtin_fmaf((float)(P - abs(k)), column[k * kColTile], a);
            acc[o] = a;
        }
    }
    const float inv = 1.f / ((float)P * (float)P);      // 4^-L, exact
    float sum = 0.f;
#pragma unroll
    for (int o = 0; o < kPer; ++o) {
        const int Y = Y0 + g + 4 * o;
        if (Y >= H || x >= W) continue;
        const int y = Y - shift_y < 0 ? Y - shift_y + H : Y - shift_y;
        const size_t i = blockIdx.z * plane + (size_t)y * W + x;
        const float d = img[i] / 127.5f - acc[o] * inv;
        grad[i] = scale * swt_pnorm(d, power, sum) + grad[i];
    }
    swt_cols_partial(sum, lds + chunk * kColTile, partials);
}

// ---- the two passes with the weights from a table (dbN / symN) ----
constexpr int kTabRowTaps = 1408;   // pass 1: 4 x (1408 + 255) strip + 1408 taps = 31.5 KiB
constexpr int kTabColTaps = 113;    // pass 2: (113 + 63) x 64 strip + 143 taps = 44.6 KiB; 16 m + 1
constexpr int kTabColOwn = 16;      //         consecutive output rows per thread

// Pass 1.  grid and thread mapping of swt_rows_kernel; slot s of a chunk that starts at tap k0 is
// padded column X0 + pad_x - hl + k0 + s, and tap k0 + j of thread t reads slot t + j.
__global__ __launch_bounds__(256) void swt_rows_table_kernel(const float *__restrict__ img,
                                                             float *__restrict__ tmp,
                                                             const float *__restrict__ table, int H,
                                                             int W, int N, int ntaps, int hl,
                                                             int shift_x, int T) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [4][T + 255], then T taps
    const int stride = T + kRowTile - 1;
    float *wl = lds + kRowRows * stride;
    const int X0 = blockIdx.x * kRowTile, y0 = blockIdx.y * kRowRows;
    const int pad_x = (N - W) / 2;
    const float *p = img + (size_t)blockIdx.z * H * W;
    const int t = threadIdx.x;
    float acc[kRowRows] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < ntaps; k0 += T) {
        const int n = min(T, ntaps - k0), len = n + kRowTile - 1;
        if (k0 > 0) __syncthreads();    // the previous chunk has been read
        for (int s = t; s < len; s += 256) {
            const int ux = swt_unrolled(X0 + pad_x - hl + k0, s, N, pad_x, W, shift_x);
#pragma unroll
            for (int r = 0; r < kRowRows; ++r)
                lds[r * stride + s] = y0 + r < H ? p[(size_t)(y0 + r) * W + ux] / 127.5f : 0.f;
        }
        for (int j = t; j < n; j += 256) wl[j] = table[k0 + j];
        __syncthreads();
        const float *row = lds + t;
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const float w = wl[j];
#pragma unroll
            for (int r = 0; r < kRowRows; ++r) acc[r] = __builtin_fmaf(w, row[r * stride + j], acc[r]);
        }
    }
    const int X = X0 + t;
    if (X >= W) return;
    const int x = X - shift_x < 0 ? X - shift_x + W : X - shift_x;
    float *out = tmp + (size_t)blockIdx.z * H * W;
#pragma unroll
    for (int r = 0; r < kRowRows; ++r)
        if (y0 + r < H) out[(size_t)(y0 + r) * W + x] = acc[r];
}

// Pass 2.  grid of swt_cols_kernel.  Thread (col, g) owns column x0 + col and the 16 consecutive
// rows Y0 + 16 g + o of the ROLLED picture, so that one staged value serves 16 outputs: at step s
// the thread reads slot 16 g + s once and adds it to output o with tap s - o, o = 0..15.  The 16
// taps in flight sit in registers, c[i & 15] = tap i, one new tap per step; 15 zero taps before
// and after the chunk's own (wz) let every output start and end inside the same loop -- a zero tap
// leaves its sum as it is, so each output still adds its own taps once, in ascending order.
// T is 16 m + 1: the T + 15 steps of a full chunk are whole blocks of 16.
__global__ __launch_bounds__(256) void swt_cols_table_kernel(
    const float *__restrict__ img, const float *__restrict__ tmp, float *__restrict__ grad,
    const float *__restrict__ table, int H, int W, int N, int ntaps, int hl, int shift_y, int T,
    float scale, float power, float *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [T + 63][64], wz[T + 30], 4 sums
    constexpr int kOwn = kTabColOwn;
    const int rows = T + kColRows - 1;
    float *wz = lds + rows * kColTile;
    float *red = wz + T + 2 * (kOwn - 1);
    const int x0 = blockIdx.x * kColTile, Y0 = blockIdx.y * kColRows;
    const int pad_y = (N - H) / 2;
    const size_t plane = (size_t)H * W;
    const float *r = tmp + blockIdx.z * plane;
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int x = x0 + col;
    float acc[kOwn];
#pragma unroll
    for (int o = 0; o < kOwn; ++o) acc[o] = 0.f;
    for (int k0 = 0; k0 < ntaps; k0 += T) {
        const int n = min(T, ntaps - k0);
        const int steps = (n + 2 * (kOwn - 1)) / kOwn * kOwn;       // n + 15 rounded up; <= T + 15
        if (k0 > 0) __syncthreads();    // the previous chunk has been read
        // slots the taps reach, and zeros up to the last slot a block of steps reads (<= rows)
        for (int s = g; s < kColRows - kOwn + steps; s += 4) {
            float v = 0.f;
            if (s < n + kColRows - 1 && x < W)
                v = r[(size_t)swt_unrolled(Y0 + pad_y - hl + k0, s, N, pad_y, H, shift_y) * W + x];
            lds[s * kColTile + col] = v;
        }
        for (int i = threadIdx.x; i < steps + kOwn - 1; i += 256)
            wz[i] = i >= kOwn - 1 && i < kOwn - 1 + n ? table[k0 + i - (kOwn - 1)] : 0.f;
        __syncthreads();
        float c[kOwn];
#pragma unroll
        for (int o = 0; o < kOwn; ++o) c[o] = 0.f;
        const float *strip = lds + g * kOwn * kColTile + col;
        for (int b = 0; b < steps; b += kOwn) {
#pragma unroll
            for (int u = 0; u < kOwn; ++u) {
                c[u] = wz[b + u + kOwn - 1];
                const float v = strip[(b + u) * kColTile];
#pragma unroll
                for (int o = 0; o < kOwn; ++o)
                    acc[o] = __builtin_fmaf(c[(u - o) & (kOwn - 1)], v, acc[o]);
            }
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int o = 0; o < kOwn; ++o) {
        const int Y = Y0 + g * kOwn + o;
        if (Y >= H || x >= W) continue;
        const int y = Y - shift_y < 0 ? Y - shift_y + H : Y - shift_y;
        const size_t i = blockIdx.z * plane + (size_t)y * W + x;
        const float d = img[i] / 127.5f - acc[o];
        grad[i] = scale * swt_pnorm(d, power, sum) + grad[i];
    }
    swt_cols_partial(sum, red, partials);
}

int wrapped(int v, int n) {
    v %= n;
    return v < 0 ? v + n : v;
}

}  // namespace

int swt_padded_side(int H, int W) {
    int N = 1;
    while (N < std::max(H, W)) N *= 2;
    return N;
}

int swt_haar_launch(hipStream_t s, const float *img, float *grad, int H, int W, int rx, int ry,
                    float scale, float power, double *loss_term, float *scratch,
                    size_t scratch_floats) {
    const int blocks = blocks_for((size_t)3 * H * W);
    if (scratch_floats < (size_t)blocks) {
        set_error("swt_haar: scratch too small");
        return STX_ERR_STATE;
    }
    swt_haar_kernel<<<blocks, 256, 0, s>>>(img, grad, H, W, swt_padded_side(H, W), rx, ry, scale,
                                           power, scratch);
    STX_CHECK_LAUNCH();
    return finish_partials_launch(s, scratch, blocks, loss_term);
}

void swt_levels_scratch(int H, int W, size_t *tmp_floats, size_t *partial_floats) {
    *tmp_floats = (size_t)3 * H * W;
    *partial_floats = (size_t)3 * ceil_div(H, kColRows) * ceil_div(W, kColTile);
}

// 1 <= levels and 2^levels <= N: the caller has checked (stx_image_swt_haar_levels)
int swt_haar_levels_launch(hipStream_t s, const float *img, float *grad, int H, int W, int levels,
                           int rx, int ry, float scale, float power, double *loss_term, float *tmp,
                           float *partials) {
    const int N = swt_padded_side(H, W);
    const int P = 1 << levels, h = P - 1;
    {
        const int chunk = std::min(kRowTile + 2 * h, kRowChunk);
        const dim3 grid(ceil_div(W, kRowTile), ceil_div(H, kRowRows), 3);
        const size_t lds = (size_t)kRowRows * chunk * sizeof(float);
        if (chunk == kRowTile + 2 * h)
            swt_rows_kernel<true><<<grid, 256, lds, s>>>(img, tmp, H, W, N, P, wrapped(rx, W), chunk);
        else
            swt_rows_kernel<false><<<grid, 256, lds, s>>>(img, tmp, H, W, N, P, wrapped(rx, W), chunk);
        STX_CHECK_LAUNCH();
    }
    const dim3 grid(ceil_div(W, kColTile), ceil_div(H, kColRows), 3);
    const int chunk = std::min(kColRows + 2 * h, kColChunk);
    swt_cols_kernel<<<grid, 256, ((size_t)chunk * kColTile + 4) * sizeof(float), s>>>(
        img, tmp, grad, H, W, N, P, wrapped(ry, H), chunk, scale, power, partials);
    STX_CHECK_LAUNCH();
    return finish_partials_launch(s, partials, (int)(grid.x * grid.y * grid.z), loss_term);
}

void swt_daub_table(int order, int levels, int N, std::vector<float> *taps, int *hl) {
    // r[+-(2k-1)], k = 1..order: the Lagrange weight of node k at the point 1/2 among the nodes
    // -order+1 .. order (every factor of one k has the sign pattern of the others: no cancellation)
    std::vector<double> r(order + 1, 0.0);
    for (int k = 1; k <= order; ++k) {
        double w = 1.0;
        for (int m = -order + 1; m <= order; ++m)
            if (m != k) w *= (0.5 - m) / (double)(k - m);
        r[k] = w;
    }
    // cur[i] is the tap at offset i - half while the cascade fits the square, and the tap at
    // offset i modulo N from the level at which it no longer does
    std::vector<double> cur(1, 1.0);
    long half = 0;
    bool folded = false;
    for (int j = 0; j < levels; ++j) {
        const long d = 1L << j, grow = (long)(2 * order - 1) * d;
        if (!folded && 2 * (half + grow) + 1 > N) {
            std::vector<double> circ(N, 0.0);
            for (long i = 0; i < (long)cur.size(); ++i) circ[(((i - half) % N) + N) % N] += cur[i];
            cur.swap(circ);
            folded = true;
        }
        if (folded) {
            std::vector<double> nxt(N, 0.0);
            for (long i = 0; i < N; ++i) {
                double a = 0.5 * cur[i];
                for (int k = 1; k <= order; ++k) {
                    const long o = (long)(2 * k - 1) * d % N;
                    a += 0.5 * r[k] * (cur[(i + o) % N] + cur[(i - o + N) % N]);
                }
                nxt[i] = a;
            }
            cur.swap(nxt);
        } else {
            std::vector<double> nxt(cur.size() + 2 * grow, 0.0);
            for (long i = 0; i < (long)cur.size(); ++i) {
                nxt[i + grow] += 0.5 * cur[i];
                for (int k = 1; k <= order; ++k) {
                    const long o = (long)(2 * k - 1) * d;
                    nxt[i + grow + o] += 0.5 * r[k] * cur[i];
                    nxt[i + grow - o] += 0.5 * r[k] * cur[i];
                }
            }
            cur.swap(nxt);
            half += grow;
        }
    }
    if (folded) {       // offsets -N/2 .. N/2 - 1
        *hl = N / 2;
        taps->resize(N);
        for (int i = 0; i < N; ++i) (*taps)[i] = (float)cur[(i - N / 2 + N) % N];
    } else {
        *hl = (int)half;
        taps->resize(cur.size());
        for (size_t i = 0; i < cur.size(); ++i) (*taps)[i] = (float)cur[i];
    }
}

int swt_table_launch(hipStream_t s, const float *img, float *grad, int H, int W, const float *table,
                     int ntaps, int hl, int rx, int ry, float scale, float power,
                     double *loss_term, float *tmp, float *partials) {
    const int N = swt_padded_side(H, W);
    if (ntaps < 1 || ntaps > std::max(N, 1) || hl < 0 || hl >= ntaps) {
        set_error("swt_table: %d taps (centre %d) on a padded side of %d", ntaps, hl, N);
        return STX_ERR_ARG;
    }
    {
        const int T = std::min(ntaps, kTabRowTaps);
        const dim3 grid(ceil_div(W, kRowTile), ceil_div(H, kRowRows), 3);
        const size_t lds = ((size_t)kRowRows * (T + kRowTile - 1) + T) * sizeof(float);
        swt_rows_table_kernel<<<grid, 256, lds, s>>>(img, tmp, table, H, W, N, ntaps, hl,
                                                     wrapped(rx, W), T);
        STX_CHECK_LAUNCH();
    }
    const int T = std::min(ceil_div(ntaps - 1, kTabColOwn) * kTabColOwn + 1, kTabColTaps);
    const dim3 grid(ceil_div(W, kColTile), ceil_div(H, kColRows), 3);
    const size_t lds =
        ((size_t)(T + kColRows - 1) * kColTile + T + 2 * (kTabColOwn - 1) + 4) * sizeof(float);
    swt_cols_table_kernel<<<grid, 256, lds, s>>>(img, tmp, grad, table, H, W, N, ntaps, hl,
                                                 wrapped(ry, H), T, scale, power, partials);
    STX_CHECK_LAUNCH();
    return finish_partials_launch(s, partials, (int)(grid.x * grid.y * grid.z), loss_term);
}

}  // namespace stx
