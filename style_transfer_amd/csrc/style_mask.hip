// Spatial control of the style term (Gatys et al., "Controlling Perceptual Factors in Neural Style
// Transfer"): a style acts through a mask m in [0, 1] on the tapped blob F [C][fh][fw] --
//   a  = sum m^2 / HW
//   Fm = F . m                                  (every channel)
//   D  = gram_lower(Fm) - a Gs                  (the existing Gram / SYMM kernels, on Fm and a Gs)
//   S  = a m . (sym(D) Fm),  sum |m . (sym(D) Fm)|
// The four passes here stand beside those kernels: the mask map of a layer (block means of the
// image-resolution mask), Fm with the partials of sum m^2, a Gs, and the masking of S in place with
// the partials of sum |m . S|.  All are bandwidth-bound: a thread owns FOUR consecutive pixels of a
// row (one 16-byte access per channel; rows whose length is no multiple of four take the one-pixel
// form), computes the wrapped window address of its mask values once and walks the channels with
// them.  The window is the content map's (ContentWindow: origin start // scale, the roll as an
// index offset with wrap).  No float atomics: per-workgroup partials, added later in a fixed order.

#include <algorithm>

#include "common.h"

namespace stx {

// ---------------------------------------------------------------------------------- the mask map
// out[y][x] = mean of M over [y s, min((y + 1) s, H)) x [x s, min((x + 1) s, W)), summed in double.
__global__ __launch_bounds__(256) void mask_map_kernel(const float *__restrict__ M, int H, int W, int s,
                                                       float *__restrict__ out, int mh, int mw, int vec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= mh * mw) return;
    const int y = i / mw, x = i - y * mw;
    const int y0 = y * s, y1 = min(y0 + s, H), x0 = x * s, x1 = min(x0 + s, W);
    double sum = 0.0;
    if (vec && x1 - x0 == s) {      // (W and s multiples of four: every row of the block starts on 16 bytes)
        for (int yy = y0; yy < y1; ++yy) {
            const float4 *row = reinterpret_cast<const float4 *>(M + (size_t)yy * W + x0);
            for (int k = 0; k < s / 4; ++k) {
                const float4 v = row[k];
                sum += (double)v.x;
                sum += (double)v.y;
                sum += (double)v.z;
                sum += (double)v.w;
            }
        }
    } else {
        for (int yy = y0; yy < y1; ++yy) {
            const float *row = M + (size_t)yy * W;
            for (int xx = x0; xx < x1; ++xx) sum += (double)row[xx];
        }
    }
    out[i] = (float)(sum / (double)((y1 - y0) * (x1 - x0)));
}

int mask_map_launch(hipStream_t s, const float *mask, int H, int W, int scale, float *out) {
    const int mh = ceil_div(H, scale), mw = ceil_div(W, scale);
    const int vec = W % 4 == 0 && scale % 4 == 0 && reinterpret_cast<uintptr_t>(mask) % 16 == 0;
    mask_map_kernel<<<ceil_div(mh * mw, 256), 256, 0, s>>>(mask, H, W, scale, out, mh, mw, vec);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

// ------------------------------------------------------------------------- the window of a thread
// The V mask values of pixel group g (V consecutive pixels of one row of the tile's feature plane).
template <int V>
__device__ __forceinline__ void mask_values(const float *__restrict__ m, const ContentWindow &w, int origin_y,
                                            int x_first, int g, int gpr, float (&mv)[V]) {
    const int y = g / gpr, x = (g - y * gpr) * V;
    int yy = (origin_y + y) % w.ch;
    if (yy < 0) yy += w.ch;
    const float *row = m + (size_t)yy * w.cw;
    int xx = (x_first + x) % w.cw;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        mv[j] = row[xx];
        if (++xx == w.cw) xx = 0;
    }
}

template <int V> struct PixelVec;
template <> struct PixelVec<4> { using type = float4; };
template <> struct PixelVec<1> { using type = float; };

template <int V>
__device__ __forceinline__ void vec_to_array(const typename PixelVec<V>::type &v, float (&a)[V]);
template <> __device__ __forceinline__ void vec_to_array<4>(const float4 &v, float (&a)[4]) {
    a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
}
template <> __device__ __forceinline__ void vec_to_array<1>(const float &v, float (&a)[1]) { a[0] = v; }
template <int V>
__device__ __forceinline__ typename PixelVec<V>::type array_to_vec(const float (&a)[V]);
template <> __device__ __forceinline__ float4 array_to_vec<4>(const float (&a)[4]) {
    return make_float4(a[0], a[1], a[2], a[3]);
}
template <> __device__ __forceinline__ float array_to_vec<1>(const float (&a)[1]) { return a[0]; }

// Grid of the two blob passes: x over pixel groups (grid-stride), y over channels (stride gridDim.y).
struct MaskGrid {
    int vec, gx, gy;
};
static MaskGrid mask_grid(const ContentWindow &w, const void *a, const void *b) {
    MaskGrid g;
    g.vec = w.fw % 4 == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0 ? 4 : 1;
    const int groups = w.fh * (w.fw / g.vec);
    g.gx = std::min(ceil_div(groups, 256), kMaskParts);
    g.gy = std::max(1, std::min(w.C, kMaskSgradParts / g.gx));
    return g;
}

// ------------------------------------------------------------------------------------- Fm = F . m
// partials[blockIdx.x] (the workgroups of channel slice 0 only) = this workgroup's share of sum m^2.
template <int V>
__global__ __launch_bounds__(256) void mask_apply_kernel(const float *__restrict__ F, const float *__restrict__ m,
                                                         ContentWindow w, float *__restrict__ Fm,
                                                         float *__restrict__ partials) {
    using Vec = typename PixelVec<V>::type;
    const int gpr = w.fw / V, groups = w.fh * gpr;
    const size_t plane = (size_t)w.fh * w.fw;
    const int origin_y = content_origin_y(w);
    int x_first = content_origin_x(w) % w.cw;
    if (x_first < 0) x_first += w.cw;
    float acc[1] = {0.f};
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        float mv[V];
        mask_values<V>(m, w, origin_y, x_first, g, gpr, mv);
        if (blockIdx.y == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) acc[0] += mv[j] * mv[j];
        }
        const size_t off = (size_t)g * V;       // rows are contiguous: y fw + x = g V
#pragma unroll 4
        for (int c = blockIdx.y; c < w.C; c += gridDim.y) {
            float f[V];
            vec_to_array<V>(*reinterpret_cast<const Vec *>(F + c * plane + off), f);
#pragma unroll
            for (int j = 0; j < V; ++j) f[j] *= mv[j];
            *reinterpret_cast<Vec *>(Fm + c * plane + off) = array_to_vec<V>(f);
        }
    }
    if (blockIdx.y == 0) block_partials<1>(acc, partials);      // (uniform per workgroup)
}

int mask_apply_launch(hipStream_t s, const float *feat, const float *map, const ContentWindow &win, float *fm,
                      float *m2_partials, int *n_parts) {
    const MaskGrid g = mask_grid(win, feat, fm);
    if (g.vec == 4)
        mask_apply_kernel<4><<<dim3(g.gx, g.gy), 256, 0, s>>>(feat, map, win, fm, m2_partials);
    else
        mask_apply_kernel<1><<<dim3(g.gx, g.gy), 256, 0, s>>>(feat, map, win, fm, m2_partials);
    STX_CHECK_LAUNCH();
    *n_parts = g.gx;
    return STX_OK;
}

// ------------------------------------------------------------------------------------ T' = a Gs
// Every workgroup adds the partials of sum m^2 up itself, in sum_partials_kernel's order (the same
// a in all of them); workgroup 0 leaves a in a_out for the pass over S.  n = C * C, a multiple of 16.
__global__ __launch_bounds__(256) void mask_target_kernel(const float *__restrict__ gs, int n,
                                                          const float *__restrict__ m2_partials, int n_parts,
                                                          float hw, float *__restrict__ out,
                                                          float *__restrict__ a_out) {
    __shared__ float red[256];
    float sum = 0.f;
    for (int i = threadIdx.x; i < n_parts; i += 256) sum += m2_partials[i];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    const float a = red[0] / hw;
    if (blockIdx.x == 0 && threadIdx.x == 0) a_out[0] = a;
    const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i < n) {
        float4 v = *reinterpret_cast<const float4 *>(gs + i);
        v.x *= a, v.y *= a, v.z *= a, v.w *= a;
        *reinterpret_cast<float4 *>(out + i) = v;
    }
}

int mask_target_launch(hipStream_t s, const float *gs, int C, const float *m2_partials, int n_parts, int HW,
                       float *out, float *a_out) {
    const int n = C * C;
    if (n % 4 || reinterpret_cast<uintptr_t>(gs) % 16 || reinterpret_cast<uintptr_t>(out) % 16) {
        set_error("mask_target_launch: a %d x %d target on 16-byte boundaries is expected", C, C);
        return STX_ERR_UNSUPPORTED;
    }
    mask_target_kernel<<<ceil_div(n / 4, 256), 256, 0, s>>>(gs, n, m2_partials, n_parts, (float)HW, out, a_out);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

// ------------------------------------------------------------------------------ S <- a (m . S)
// partials[blockIdx.y * gridDim.x + blockIdx.x] = this workgroup's share of sum |m . S| (without a:
// the divisor of the injection is that of the masked gradient, a scales what is injected -- an
// all-zero mask gives 0 / EPS, not 0 * Inf).
template <int V>
__global__ __launch_bounds__(256) void mask_sgrad_kernel(float *__restrict__ S, const float *__restrict__ m,
                                                         ContentWindow w, const float *__restrict__ a_ptr,
                                                         float *__restrict__ partials) {
    using Vec = typename PixelVec<V>::type;
    const float a = a_ptr[0];
    const int gpr = w.fw / V, groups = w.fh * gpr;
    const size_t plane = (size_t)w.fh * w.fw;
    const int origin_y = content_origin_y(w);
    int x_first = content_origin_x(w) % w.cw;
    if (x_first < 0) x_first += w.cw;
    float acc[1] = {0.f};
    for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
        float mv[V];
        mask_values<V>(m, w, origin_y, x_first, g, gpr, mv);
        const size_t off = (size_t)g * V;
#pragma unroll 4
        for (int c = blockIdx.y; c < w.C; c += gridDim.y) {
            float v[V];
            Vec *p = reinterpret_cast<Vec *>(S + c * plane + off);
            vec_to_array<V>(*p, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                v[j] *= mv[j];
                acc[0] += fabsf(v[j]);
                v[j] *= a;
            }
            *p = array_to_vec<V>(v);
        }
    }
    block_partials<1>(acc, partials + (size_t)blockIdx.y * gridDim.x);
}

int mask_sgrad_launch(hipStream_t s, float *sgrad, const float *map, const ContentWindow &win, const float *a,
                      float *partials, int *n_parts) {
    const MaskGrid g = mask_grid(win, sgrad, sgrad);
    if (g.vec == 4)
        mask_sgrad_kernel<4><<<dim3(g.gx, g.gy), 256, 0, s>>>(sgrad, map, win, a, partials);
    else
        mask_sgrad_kernel<1><<<dim3(g.gx, g.gy), 256, 0, s>>>(sgrad, map, win, a, partials);
    STX_CHECK_LAUNCH();
    *n_parts = g.gx * g.gy;
    return STX_OK;
}

}  // namespace stx
