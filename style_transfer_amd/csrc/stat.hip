// The mean / std style term (the BN-statistics loss of Li et al., "Demystifying Neural Style Transfer";
// the quantity AdaIN aligns): a tapped blob F [C][HW] is held to per-channel targets MU, SD --
//   mu_c = mean F_c,  sd_c = sqrt(var_c + 1e-5)  (population variance)
//   E    = sum_c (mu_c - MU_c)^2 + (sd_c - SD_c)^2
//   S_c  = a_c + b_c (F_c - mu_c),  a = mu - MU,  b = (sd - SD) / sd          ( = HW d(E/2)/dF )
// Three streaming launches, O(C HW), no matrix product and no atomics:
//   1. stat_partials_kernel   grid (slices of HW, C): a workgroup sums its slice, re-reads it (64 KB: it
//                             is still in L2) for the sums of d and d^2 about that mean, and writes
//                             (count, mean, M2 about its own mean).  Never sum F^2 - n mu^2.
//   2. stat_finish_kernel     one workgroup: Chan's merge of a channel's partials in double, in slice
//                             order; mu and sd are rounded to float32 ONCE and a, b, E are formed from the
//                             rounded values, so statistics that equal their targets give exactly 0.
//   3. stat_grad_kernel       grid as 1: S with the per-workgroup partials of sum |S|.
// A slice is read with 16-byte loads between a scalar head (up to the first 16-byte boundary: h w is
// odd as often as not, so a channel starts anywhere) and a scalar tail.

#include <algorithm>

#include "common.h"

namespace stx {

int stat_slices(int HW) { return ceil_div(HW, kStatSlice); }

size_t stat_scratch_floats(int C, int HW) {
    // 4 floats per partial, the (mu, a, b) table padded to 4 per channel, the partials of sum |S|
    return (size_t)C * (5 * (size_t)stat_slices(HW) + 4);
}

namespace {

// How the 256 threads of a workgroup walk `len` floats at p: [head scalars][nvec float4][tail scalars].
struct SliceSpan {
    int head, nvec, tail;
};

__device__ __forceinline__ SliceSpan slice_span(const float *p, int len, int vec) {
    SliceSpan s;
    const int to_boundary = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
    s.head = vec ? min(len, to_boundary) : len;
    s.nvec = (len - s.head) >> 2;
    s.tail = len - s.head - 4 * s.nvec;
    return s;
}

// f(value, offset from p) for every element this thread owns.
template <class Fn>
__device__ __forceinline__ void slice_for_each(const float *__restrict__ p, const SliceSpan &s, Fn f) {
    for (int i = threadIdx.x; i < s.head; i += 256) f(p[i], i);
    const float4 *v = reinterpret_cast<const float4 *>(p + s.head);
#pragma unroll 4
    for (int i = threadIdx.x; i < s.nvec; i += 256) {
        const float4 x = v[i];
        const int o = s.head + 4 * i;
        f(x.x, o);
        f(x.y, o + 1);
        f(x.z, o + 2);
        f(x.w, o + 3);
    }
    const int t0 = s.head + 4 * s.nvec;
    for (int i = threadIdx.x; i < s.tail; i += 256) f(p[t0 + i], t0 + i);
}

// The workgroup's sum of v, in every thread (fixed order: wave shuffles, then the four waves in turn).
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum_f(v);
    __syncthreads();        // (red may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void stat_partials_kernel(const float *__restrict__ F, int HW, int vec,
                                                            float *__restrict__ partials) {
    __shared__ float red[4];
    const int c = blockIdx.y, e0 = blockIdx.x * kStatSlice;
    const int len = min(kStatSlice, HW - e0);
    const float *p = F + (size_t)c * HW + e0;
    const SliceSpan span = slice_span(p, len, vec);
    float sum = 0.f;
    slice_for_each(p, span, [&](float x, int) { sum += x; });
    const float m = block_sum(sum, red) / (float)len;
    // the centred second sweep; d1 = sum (x - m) is what the float sum above left of the mean
    float d1 = 0.f, d2 = 0.f;
    slice_for_each(p, span, [&](float x, int) {
        const float d = x - m;
        d1 += d;
        d2 += d * d;
    });
    d1 = block_sum(d1, red);
    d2 = block_sum(d2, red);
    if (threadIdx.x == 0) {
        const double r = (double)d1 / (double)len;
        const double mean = (double)m + r;
        const double m2 = fmax((double)d2 - (double)d1 * r, 0.0);
        const float hi = (float)mean;
        float *o = partials + ((size_t)c * gridDim.x + blockIdx.x) * 4;
        o[0] = (float)len;
        o[1] = hi;                              // (the mean as two floats: the merge runs in double)
        o[2] = (float)(mean - (double)hi);
        o[3] = (float)m2;
    }
}

// MU / SD given: table[c] = (mu, a, b, 0), e_out[0] = E.  Otherwise mean_out[c] = mu, sd_out[c] = sd.
__global__ __launch_bounds__(256) void stat_finish_kernel(const float *__restrict__ partials, int C, int slices,
                                                          const float *__restrict__ MU, const float *__restrict__ SD,
                                                          float *__restrict__ table, float *__restrict__ e_out,
                                                          float *__restrict__ mean_out, float *__restrict__ sd_out) {
    __shared__ double red[256];
    double e = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float *q = partials + (size_t)c * slices * 4;
        double n = q[0], mean = (double)q[1] + (double)q[2], m2 = q[3];
        for (int s = 1; s < slices; ++s) {      // Chan et al., pairwise update, in slice order
            const float *b = q + 4 * s;
            const double nb = b[0], mb = (double)b[1] + (double)b[2];
            const double nn = n + nb, delta = mb - mean;
            mean += delta * (nb / nn);
            m2 += (double)b[3] + delta * delta * (n * nb / nn);
            n = nn;
        }
        const float mu = (float)mean, sd = (float)sqrt(m2 / n + (double)kStatEps);
        if (MU) {
            const float a = mu - MU[c], d = sd - SD[c];
            table[4 * c] = mu;
            table[4 * c + 1] = a;
            table[4 * c + 2] = d / sd;
            table[4 * c + 3] = 0.f;
            e += (double)a * (double)a + (double)d * (double)d;
        } else {
            mean_out[c] = mu;
            sd_out[c] = sd;
        }
    }
    if (!MU) return;        // (uniform)
    red[threadIdx.x] = e;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) e_out[0] = (float)red[0];
}

// (vec: F and S start on the same offset from a 16-byte boundary -- one span serves both)
__global__ __launch_bounds__(256) void stat_grad_kernel(const float *__restrict__ F, int HW, int vec,
                                                        const float *__restrict__ table, float *__restrict__ S,
                                                        float *__restrict__ partials) {
    __shared__ float red[4];
    const int c = blockIdx.y, e0 = blockIdx.x * kStatSlice;
    const int len = min(kStatSlice, HW - e0);
    const float mu = table[4 * c], a = table[4 * c + 1], b = table[4 * c + 2];
    const float *p = F + (size_t)c * HW + e0;
    float *o = S + (size_t)c * HW + e0;
    const SliceSpan s = slice_span(p, len, vec);
    float acc = 0.f;
    for (int i = threadIdx.x; i < s.head; i += 256) {
        const float v = a + b * (p[i] - mu);
        o[i] = v;
        acc += fabsf(v);
    }
    const float4 *pv = reinterpret_cast<const float4 *>(p + s.head);
    float4 *ov = reinterpret_cast<float4 *>(o + s.head);
#pragma unroll 4
    for (int i = threadIdx.x; i < s.nvec; i += 256) {
        const float4 x = pv[i];
        float4 v;
        v.x = a + b * (x.x - mu);
        v.y = a + b * (x.y - mu);
        v.z = a + b * (x.z - mu);
        v.w = a + b * (x.w - mu);
        ov[i] = v;
        acc += (fabsf(v.x) + fabsf(v.y)) + (fabsf(v.z) + fabsf(v.w));
    }
    const int t0 = s.head + 4 * s.nvec;
    for (int i = threadIdx.x; i < s.tail; i += 256) {
        const float v = a + b * (p[t0 + i] - mu);
        o[t0 + i] = v;
        acc += fabsf(v);
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) partials[(size_t)c * gridDim.x + blockIdx.x] = acc;
}

int check_shape(const char *who, int C, int HW) {
    if (C <= 0 || HW <= 0 || C > 65535) {
        set_error("%s: %d channels of %d pixels cannot be launched", who, C, HW);
        return STX_ERR_ARG;
    }
    return STX_OK;
}

}  // namespace

int stat_partials_launch(hipStream_t s, const float *feat, int C, int HW, float *partials) {
    STX_TRY(check_shape("stat_partials_launch", C, HW));
    const int vec = reinterpret_cast<uintptr_t>(feat) % 4 == 0;
    stat_partials_kernel<<<dim3(stat_slices(HW), C), 256, 0, s>>>(feat, HW, vec, partials);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int stat_finish_launch(hipStream_t s, const float *partials, int C, int HW, const float *MU, const float *SD,
                       float *table, float *e_out, float *mean_out, float *sd_out) {
    STX_TRY(check_shape("stat_finish_launch", C, HW));
    if (MU ? (!SD || !table || !e_out) : (!mean_out || !sd_out)) {
        set_error("stat_finish_launch: targets with a table and a scalar, or two outputs, are expected");
        return STX_ERR_ARG;
    }
    stat_finish_kernel<<<1, 256, 0, s>>>(partials, C, stat_slices(HW), MU, SD, table, e_out, mean_out, sd_out);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int stat_grad_launch(hipStream_t s, const float *feat, int C, int HW, const float *table, float *sgrad,
                     float *abs_partials, int *n_parts) {
    STX_TRY(check_shape("stat_grad_launch", C, HW));
    const uintptr_t f = reinterpret_cast<uintptr_t>(feat), g = reinterpret_cast<uintptr_t>(sgrad);
    const int vec = f % 4 == 0 && g % 4 == 0 && f % 16 == g % 16;
    stat_grad_kernel<<<dim3(stat_slices(HW), C), 256, 0, s>>>(feat, HW, vec, table, sgrad, abs_partials);
    STX_CHECK_LAUNCH();
    *n_parts = stat_slices(HW) * C;
    return STX_OK;
}

}  // namespace stx
