// The temporal-consistency term for video (Ruder, Dosovitskiy, Brox, "Artistic Style Transfer for
// Videos", 2016): earlier stylised frames are warped to the current frame by optical flow, composited
// into one target, and the iterate is held to that target wherever the flow is reliable.  Pictures
// are [3][H][W] planes, un-rolled; flows are [2][H][W] (plane 0 horizontal, 1 vertical), in pixels of
// the resolution they were estimated at; weight is [H][W].
//
// ---- flow_warp_kernel: one earlier frame into the composite (once per scale and frame)
// Every value between the float32 inputs and the float32 outputs is float64, as in photo.hip: the
// kernel decides on thresholds, and a decision taken in float32 would flip for pixels that float64
// puts 1e-6 from one.  The file is compiled with -ffp-contract=off, so every double operation below
// rounds once, in the order written; stx.h states that order.  For pixel (x, y):
//   u = su * flow_b[0], v = sv * flow_b[1]; unknown: a component that is not finite or above 1e9 in
//   magnitude before scaling (Middlebury's marker)
//   q = (x + u, y + v); inside: 0 <= qx <= W - 1 and 0 <= qy <= H - 1
//   x0 = min(floor(qx), W - 2), fx = qx - x0 (y likewise); value = the bilinear mix of prev at
//   (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
//   (fu, fv) = (su, sv) * the same mix of flow_f; a tap that is unknown makes the pixel unreliable
//   consistent: (u + fu)^2 + (v + fv)^2 <= 0.01 (u^2 + v^2 + fu^2 + fv^2) + 0.5
//   boundary: ux^2 + uy^2 + vx^2 + vy^2 > 0.01 (u^2 + v^2) + 0.002 with central differences over a
//   replicated border, or an unknown neighbour
//   c = known and inside and consistent and not boundary
// Composite (first-wins): weight before == 0 (always, with `first`) and c -> target = value on the
// three planes, weight = 1; else with `first` both are zeroed; else both stay.  A pixel whose weight
// is already set returns before it reads a flow.
//
// Bytes per pixel with a forward flow and `first`: flow_b 8 (the stencil's neighbours are the next
// lanes' and rows' own reads), flow_f 8 and prev 12 (gathered, but a smooth flow moves whole rows
// together), target 12 and weight 4 written: 44 B.  Without `first` the weight is read too (48 B) and
// settled pixels cost 4 B.
//
// ---- temporal_kernel: the term (every evaluation)
//   w' = min(max(weight, 0), 1), NaN as 0;  d = (img - target) / 127.5f
//   grad = (scale w') d + grad;  loss = scale * 63.75 * sum w' d^2
// One pass, grid-stride over the pixels in fp32: a thread reads a pixel's weight once and walks the
// three planes, so the call moves img 12 + target 12 + weight 4 + grad 24 = 52 B per pixel at most.  A
// pixel with w' = 0 reads nothing else, and an element whose addend is zero is not written (grad
// keeps its bits, a negative zero included).  With H * W a multiple of 4 and 16-byte aligned arrays
// a thread takes four neighbouring pixels with 16-byte loads.  Sums go through block partials and
// are finished in double (finish_partials_kernel).  No atomics: the same inputs give the same bits.

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"

namespace stx {

namespace {

__device__ __forceinline__ bool flow_known(float a, float b) {
    return fabsf(a) <= 1e9f && fabsf(b) <= 1e9f;    // (false for NaN and infinity)
}

__device__ __forceinline__ double bilinear(double p00, double p01, double p10, double p11, double fx,
                                           double fy) {
    const double top = p00 + fx * (p01 - p00), bottom = p10 + fx * (p11 - p10);
    return top + fy * (bottom - top);
}

__global__ __launch_bounds__(256) void flow_warp_kernel(const float *__restrict__ prev,
                                                        const float *__restrict__ flow_b,
                                                        const float *__restrict__ flow_f, int H, int W,
                                                        double su, double sv, int first,
                                                        float *__restrict__ target,
                                                        float *__restrict__ weight) {
    const size_t plane = (size_t)H * W;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < plane; i += (size_t)gridDim.x * 256) {
        if (!first && weight[i] != 0.f) continue;   // an earlier (closer) frame has this pixel
        const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * W);
        const float fb0 = flow_b[i], fb1 = flow_b[plane + i];
        bool c = flow_known(fb0, fb1);
        double value[3] = {0.0, 0.0, 0.0};
        if (c) {
            const double u = su * (double)fb0, v = sv * (double)fb1;
            const double qx = (double)x + u, qy = (double)y + v;
            c = qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1);
            if (c) {
                // ---- motion boundary: central differences of the scaled flow, replicated border
                const int xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1;
                const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1;
                const size_t l = (size_t)y * W + xm, r = (size_t)y * W + xp;
                const size_t a = (size_t)ym * W + x, b = (size_t)yp * W + x;
                const float ul = flow_b[l], ur = flow_b[r], ua = flow_b[a], ub = flow_b[b];
                const float vl = flow_b[plane + l], vr = flow_b[plane + r];
                const float va = flow_b[plane + a], vb = flow_b[plane + b];
                c = flow_known(ul, vl) && flow_known(ur, vr) && flow_known(ua, va) && flow_known(ub, vb);
                if (c) {
                    const double ux = (su * (double)ur - su * (double)ul) / 2.0;
                    const double uy = (su * (double)ub - su * (double)ua) / 2.0;
                    const double vx = (sv * (double)vr - sv * (double)vl) / 2.0;
                    const double vy = (sv * (double)vb - sv * (double)va) / 2.0;
                    const double lhs = ((ux * ux + uy * uy) + vx * vx) + vy * vy;
                    c = !(lhs > 0.01 * (u * u + v * v) + 0.002);
                }
            }
            if (c) {
                // (inside: 0 <= floor(q) <= size - 1, so the taps below are in the picture; H, W >= 2)
                const int fx0 = (int)floor(qx), fy0 = (int)floor(qy);
                const int x0 = fx0 < W - 2 ? fx0 : W - 2, y0 = fy0 < H - 2 ? fy0 : H - 2;
                const double fx = qx - (double)x0, fy = qy - (double)y0;
                const size_t t00 = (size_t)y0 * W + x0, t10 = t00 + W;
                if (flow_f != nullptr) {
                    const float f00 = flow_f[t00], f01 = flow_f[t00 + 1], f10 = flow_f[t10], f11 = flow_f[t10 + 1];
                    const float g00 = flow_f[plane + t00], g01 = flow_f[plane + t00 + 1];
                    const float g10 = flow_f[plane + t10], g11 = flow_f[plane + t10 + 1];
                    c = flow_known(f00, g00) && flow_known(f01, g01) && flow_known(f10, g10) && flow_known(f11, g11);
                    if (c) {
                        const double fu = su * bilinear(f00, f01, f10, f11, fx, fy);
                        const double fv = sv * bilinear(g00, g01, g10, g11, fx, fy);
                        const double du = u + fu, dv = v + fv;
                        c = du * du + dv * dv <= 0.01 * (((u * u + v * v) + fu * fu) + fv * fv) + 0.5;
                    }
                }
                if (c) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float *p = prev + ch * plane;
                        value[ch] = bilinear(p[t00], p[t00 + 1], p[t10], p[t10 + 1], fx, fy);
                    }
                }
            }
        }
        if (c || first) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) target[ch * plane + i] = c ? (float)value[ch] : 0.f;
            weight[i] = c ? 1.f : 0.f;
        }
    }
}

// One element: the addend into grad (not written when it is zero) and w' d^2 into the sum.
__device__ __forceinline__ void temporal_element(float x, float t, float sw, float w, float *g, float &sum) {
    if (w == 0.f) return;
    const float d = (x - t) / 127.5f;
    const float add = sw * d;
    sum += w * (d * d);
    if (add != 0.f) *g = add + *g;
}

__device__ __forceinline__ float clamp01(float w) { return w > 0.f ? (w < 1.f ? w : 1.f) : 0.f; }  // NaN -> 0

template <bool VEC4>
__global__ __launch_bounds__(256) void temporal_kernel(const float *__restrict__ img, float *__restrict__ grad,
                                                       const float *__restrict__ target,
                                                       const float *__restrict__ weight, size_t plane,
                                                       float scale, float *__restrict__ partials) {
    float sums[1] = {0.f};
    const size_t i0 = blockIdx.x * (size_t)256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (VEC4) {
        const size_t quads = plane / 4;
        for (size_t q = i0; q < quads; q += stride) {
            const float4 w4 = reinterpret_cast<const float4 *>(weight)[q];
            const float w[4] = {clamp01(w4.x), clamp01(w4.y), clamp01(w4.z), clamp01(w4.w)};
            if (w[0] == 0.f && w[1] == 0.f && w[2] == 0.f && w[3] == 0.f) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t at = c * quads + q;
                const float4 x4 = reinterpret_cast<const float4 *>(img)[at];
                const float4 t4 = reinterpret_cast<const float4 *>(target)[at];
                float4 g4 = reinterpret_cast<float4 *>(grad)[at];
                const float4 before = g4;
                temporal_element(x4.x, t4.x, scale * w[0], w[0], &g4.x, sums[0]);
                temporal_element(x4.y, t4.y, scale * w[1], w[1], &g4.y, sums[0]);
                temporal_element(x4.z, t4.z, scale * w[2], w[2], &g4.z, sums[0]);
                temporal_element(x4.w, t4.w, scale * w[3], w[3], &g4.w, sums[0]);
                // (compared as bits: a NaN must be written, and an untouched quad is not)
                if (__float_as_uint(g4.x) != __float_as_uint(before.x) ||
                    __float_as_uint(g4.y) != __float_as_uint(before.y) ||
                    __float_as_uint(g4.z) != __float_as_uint(before.z) ||
                    __float_as_uint(g4.w) != __float_as_uint(before.w))
                    reinterpret_cast<float4 *>(grad)[at] = g4;
            }
        }
    } else {
        for (size_t i = i0; i < plane; i += stride) {
            const float w = clamp01(weight[i]);
            if (w == 0.f) continue;
            const float sw = scale * w;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t at = c * plane + i;
                temporal_element(img[at], target[at], sw, w, grad + at, sums[0]);
            }
        }
    }
    block_partials<1>(sums, partials);
}

}  // namespace

int flow_warp_launch(hipStream_t s, const float *prev, const float *flow_b, const float *flow_f, int H, int W,
                     double su, double sv, int first, float *target, float *weight) {
    const size_t plane = (size_t)H * W;
    const size_t blocks = std::min<size_t>((plane + 255) / 256, (size_t)65536);
    flow_warp_kernel<<<(unsigned)blocks, 256, 0, s>>>(prev, flow_b, flow_f, H, W, su, sv, first, target, weight);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int temporal_launch(hipStream_t s, const float *img, float *grad, const float *target, const float *weight,
                    int H, int W, double scale, double *loss_term, float *scratch) {
    const size_t plane = (size_t)H * W;
    const bool aligned = ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(grad) |
                           reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(weight)) & 15) == 0;
    int blocks;
    if (plane % 4 == 0 && aligned) {
        blocks = blocks_for(plane / 4);
        temporal_kernel<true><<<blocks, 256, 0, s>>>(img, grad, target, weight, plane, (float)scale, scratch);
    } else {
        blocks = blocks_for(plane);
        temporal_kernel<false><<<blocks, 256, 0, s>>>(img, grad, target, weight, plane, (float)scale, scratch);
    }
    STX_CHECK_LAUNCH();
    return finish_partials_launch(s, scratch, blocks, loss_term);
}

}  // namespace stx
