// Spatial control of the content term (Gatys et al., "Controlling Perceptual Factors in Neural Style
// Transfer"): the content picture is held through a weight map m in [0, 1] on the tapped blob F [C][fh][fw].
// With c the tile's window of the content map and m the same window of the weight map (every channel):
//   d  = F - c
//   a  = sum m / (fh fw)                     (the window's mean weight)
//   E  = 1/2 sum m d^2,  sum |m d|
//   S  = a (m d)
// Two launches: a from the window of the map (one workgroup, double, a fixed order, independent of C), then one
// streaming pass over (F, c, m) that writes S and leaves per-workgroup partials of sum m d^2 and sum |m d|
// for the fixed-order final sums (SumJob / sum_partials2_launch).  No atomics.
//
// The pass walks the elements exactly as content_sums_kernel (reduce.hip) does -- one wave per 64-column row
// segment, four segments per trip, lane l of a wave owning column l of each, the same grid -- and forms the
// square as (m d) d: with m == 1 its partials are that kernel's bit for bit, and S is F - c.  That fixes which
// lane adds which element, so the accesses stay one float per lane (a wave reads 256 contiguous bytes of a
// row); 16-byte accesses would hand a lane four neighbouring columns and add them in another order.  This
// file is compiled like reduce.hip (contraction on) for the same reason.

#include <algorithm>

#include "common.h"

namespace stx {

// ------------------------------------------------------------------------------- a = mean of the window
__global__ __launch_bounds__(1024) void content_mask_mean_kernel(const float *__restrict__ m, ContentWindow w,
                                                                 float *__restrict__ a_out) {
    __shared__ double red[1024];
    const int origin_y = content_origin_y(w);
    int x_first = content_origin_x(w) % w.cw;
    if (x_first < 0) x_first += w.cw;
    const int n = w.fh * w.fw;
    double sum = 0.0;
#pragma unroll 4
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int y = i / w.fw, x = i - y * w.fw;
        int yy = (origin_y + y) % w.ch;
        if (yy < 0) yy += w.ch;
        const int xx = (x_first + x) % w.cw;
        sum += (double)m[(size_t)yy * w.cw + xx];
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) a_out[0] = (float)(red[0] / (double)n);
}

int content_mask_mean_launch(hipStream_t s, const float *map, const ContentWindow &win, float *a_out) {
    content_mask_mean_kernel<<<1, 1024, 0, s>>>(map, win, a_out);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

// ------------------------------------------------------------- S = a (m d), partials of the two sums
// partials[blockIdx.x] = this workgroup's share of sum m d^2, partials[gridDim.x + blockIdx.x] of sum |m d|.
__global__ __launch_bounds__(256) void content_mask_term_kernel(const float *__restrict__ feat,
                                                                const float *__restrict__ content,
                                                                const float *__restrict__ m, ContentWindow w,
                                                                const float *__restrict__ a_ptr,
                                                                float *__restrict__ S,
                                                                float *__restrict__ partials) {
    __shared__ float red[2][4];
    const float a = a_ptr[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int segs = (w.fw + 63) >> 6;
    const int total_segs = w.C * w.fh * segs;
    const int origin_y = content_origin_y(w);
    int x_first = content_origin_x(w) % w.cw;
    if (x_first < 0) x_first += w.cw;
    // four segments per trip: twelve loads in flight per lane (content_sums_kernel: with one segment per trip
    // the walk is bound by load latency)
    float sq4[4] = {0.f, 0.f, 0.f, 0.f}, ab4[4] = {0.f, 0.f, 0.f, 0.f};
    const int step = gridDim.x * 4;
    for (int g0 = blockIdx.x * 4 + wave; g0 < total_segs; g0 += 4 * step) {
        float f[4], t[4], mv[4];
        size_t at[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = g0 + u * step;
            const int gg = g < total_segs ? g : g0;
            const int row = gg / segs, x0 = (gg - row * segs) * 64;
            const int c = row / w.fh, y = row - c * w.fh;
            int yy = (origin_y + y) % w.ch;
            if (yy < 0) yy += w.ch;
            const int x = x0 + lane;
            ok[u] = g < total_segs && x < w.fw;
            const int xc = x < w.fw ? x : 0;
            const int xx = (x_first + xc) % w.cw;
            at[u] = ((size_t)c * w.fh + y) * w.fw + xc;
            f[u] = feat[at[u]];
            t[u] = content[((size_t)c * w.ch + yy) * w.cw + xx];
            mv[u] = m[(size_t)yy * w.cw + xx];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float d = ok[u] ? f[u] - t[u] : 0.f;
            const float md = mv[u] * d;
            sq4[u] += md * d;
            ab4[u] += fabsf(md);
            if (ok[u]) S[at[u]] = a * md;
        }
    }
    float sq = (sq4[0] + sq4[1]) + (sq4[2] + sq4[3]), ab = (ab4[0] + ab4[1]) + (ab4[2] + ab4[3]);
    sq = wave_sum_f(sq);
    ab = wave_sum_f(ab);
    if (lane == 0) {
        red[0][wave] = sq;
        red[1][wave] = ab;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        partials[gridDim.x + blockIdx.x] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

int content_mask_term_launch(hipStream_t s, const float *feat, const float *content, const float *map,
                             const ContentWindow &win, const float *a, float *sgrad, float *partials,
                             int *n_parts) {
    const size_t total = (size_t)win.C * win.fh * win.fw;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, kContentMaskParts);
    content_mask_term_kernel<<<blocks, 256, 0, s>>>(feat, content, map, win, a, sgrad, partials);
    STX_CHECK_LAUNCH();
    *n_parts = blocks;
    return STX_OK;
}

}  // namespace stx
