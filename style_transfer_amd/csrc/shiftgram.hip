// The shifted-Gram style term (Berger & Memisevic, "Incorporating long-range consistency in CNN-based texture
// generation", ICLR 2017): the Gram matrix of a tapped blob F [C][h][w] against a copy of itself translated by
// delta = (dy, dx) is held to the style picture's, for a few delta along each axis (include/stx.h,
// stx_set_shift_targets).  With P = {p : p and p + delta in the map}, n_d = (h - dy)(w - dx), n = h w:
//   X_d[a][b] = (1 / (C n_d)) sum_{p in P} F_a(p) F_b(p + delta)            (full C x C, not symmetric)
//   D_d = X_d - T_d,   E = (1 / |Delta|) sum_d sum_ab D_d[a][b]^2
//   S_a(p) = (1 / |Delta|) sum_d (n / n_d) [ sum_b D_d[a][b] F_b(p + delta) + sum_b D_d[b][a] F_b(p - delta) ]
// (terms outside the map are 0).  Three launches, v_mfma_f32_32x32x2_f32 products, no atomics:
//   1. shift_cross_kernel   grid (K slices of P, pairs of 64-channel blocks, offsets): a 64 x 64 partial of X_d
//                           over one slice of P in raster order.  Both operands come from F itself: the pair
//                           index q = y (w - dx) + x reads F_a at y w + x and F_b at (y + dy) w + x + dx.  The
//                           float32 chain of the matrix core is cut every kShiftChain pairs (a second register
//                           accumulator takes it over), so no chain is longer than that whatever the map's size.
//   2. shift_merge_kernel   adds an element's slices in slice order in double, scales by 1 / (C n_d) and rounds
//                           to float32 ONCE.  Without targets that is the output (stx_shift_gram).  With targets:
//                           D = X - T from the rounded values, the weights W_d = (n / (n_d |Delta|)) D_d and their
//                           transposes for the gradient, and the blocks' partials of E.
//   3. shift_grad_kernel    grid (64-pixel blocks, 64-channel blocks): S as ONE product over K = 2 |Delta| C --
//                           per (offset, sign) the operand rows are F at p + delta or p - delta, zero outside the
//                           map, against W_d or its transpose -- with the partials of sum |S| in its epilogue.
// X that equals T gives D = +0, W = 0 and S = 0: the term then adds exactly nothing to the loss and the gradient.

#include <algorithm>

#include "common.h"

namespace stx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

static size_t shift_round64(size_t v) { return (v + 63) & ~(size_t)63; }

int shift_slice_len(int HW) {
    // at most 64 slices of a map, none shorter than 2048 pairs, a multiple of the K tile
    const int len = std::max(2048, (HW + 63) / 64);
    return (len + 31) & ~31;
}

int shift_slices(int HW) { return ceil_div(HW, shift_slice_len(HW)); }

int shift_check_offsets(const char *who, int C, const int *offsets, int n_offsets, ShiftOffsets *out) {
    if (C <= 0 || !offsets || n_offsets < 1 || n_offsets > kShiftMaxOffsets) {
        set_error("%s: %d channels, %d offsets (1 to %d offsets are expected)", who, C, n_offsets, kShiftMaxOffsets);
        return STX_ERR_ARG;
    }
    if (C % 32 != 0) {
        set_error("%s: %d channels (a multiple of 32 is expected)", who, C);
        return STX_ERR_UNSUPPORTED;
    }
    ShiftOffsets o{};
    o.n = n_offsets;
    for (int i = 0; i < n_offsets; ++i) {
        const int dy = offsets[2 * i], dx = offsets[2 * i + 1];
        if (!((dy == 0 && dx >= 1) || (dx == 0 && dy >= 1))) {
            set_error("%s: offset %d is (%d, %d); (0, d) or (d, 0) with d >= 1 is expected", who, i, dy, dx);
            return STX_ERR_ARG;
        }
        o.dy[i] = dy;
        o.dx[i] = dx;
    }
    if (out) *out = o;
    return STX_OK;
}

int shift_check_map(const char *who, int C, int h, int w, const ShiftOffsets &off) {
    if (h <= 0 || w <= 0 || (long long)h * w > (1ll << 30) || (long long)C * h * w >= (1ll << 40)) {
        set_error("%s: a %d x %d map of %d channels cannot be launched", who, h, w, C);
        return STX_ERR_ARG;
    }
    for (int i = 0; i < off.n; ++i) {
        if (h - off.dy[i] >= 1 && w - off.dx[i] >= 1) continue;
        set_error("%s: offset (%d, %d) leaves a %d x %d map without a pair of pixels", who, off.dy[i], off.dx[i], h, w);
        return STX_ERR_ARG;
    }
    return STX_OK;
}

ShiftScratch shift_scratch(float *base, int C, int HW, int n_offsets) {
    const size_t cc = (size_t)C * C;
    ShiftScratch x;
    size_t at = 0;
    const auto take = [&](size_t floats) {      // (base null: only the size is asked for)
        float *p = base ? base + at : nullptr;
        at += shift_round64(floats);
        return p;
    };
    x.partials = take((size_t)n_offsets * shift_slices(HW) * cc);
    x.weights = take(2 * (size_t)n_offsets * cc);
    x.e_parts = take((size_t)n_offsets * ((cc + 255) / 256));
    x.abs_parts = take((size_t)ceil_div(HW, 64) * ceil_div(C, 64));
    x.floats = at;
    return x;
}

size_t shift_scratch_floats(int C, int HW, int n_offsets) { return shift_scratch(nullptr, C, HW, n_offsets).floats; }

namespace {

constexpr int kLd = 33;             // a 32-float LDS row and one of padding: the 32 lanes of an operand read hit 32 banks
constexpr int kShiftChain = 1024;   // pairs (or operand rows) that one float32 accumulation chain takes at most

// ------------------------------------------------------------------------------------------ cross-Gram
// partials[offset][slice][a][b] = sum over the slice's pairs of F_a(p) F_b(p + delta); a wave owns a 32 x 32 block
// of the 64 x 64 tile.  Slices past an offset's last pair leave nothing (the merge never reads them).
__global__ __launch_bounds__(256) void shift_cross_kernel(const float *__restrict__ F, int C, int h, int w,
                                                          ShiftOffsets off, int slice_len, int max_slices,
                                                          float *__restrict__ partials) {
    __shared__ float At[64 * kLd];
    __shared__ float Bt[64 * kLd];
    const int d = blockIdx.z;
    const int dy = off.dy[d], dx = off.dx[d];
    const int wd = w - dx, nd = (h - dy) * wd;
    const int q0 = blockIdx.x * slice_len;
    if (q0 >= nd) return;       // (uniform)
    const int q1 = min(q0 + slice_len, nd);
    const int nb = (C + 63) >> 6;
    const int a0 = (blockIdx.y / nb) * 64, b0 = (blockIdx.y % nb) * 64;
    const size_t n = (size_t)h * w;
    const int shift = dy * w + dx;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int bi = wave >> 1, bj = wave & 1;
    const int k = tid & 31, m0 = tid >> 5;
    f32x16 acc, tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = tot[r] = 0.f;
    const float *ap = At + (bi * 32 + l31) * kLd + half;
    const float *bp = Bt + (bj * 32 + l31) * kLd + half;
    int chain = 0;
    for (int kt = q0; kt < q1; kt += 32) {
        const bool ok = kt + k < q1;
        const int q = ok ? kt + k : q0;
        const int y = q / wd, x = q - y * wd;
        const size_t at = (size_t)y * w + x;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int m = m0 + 8 * r;
            const bool oka = ok && a0 + m < C, okb = ok && b0 + m < C;
            const float a = F[oka ? (size_t)(a0 + m) * n + at : 0];
            const float b = F[okb ? (size_t)(b0 + m) * n + at + shift : 0];
            At[m * kLd + k] = oka ? a : 0.f;
            Bt[m * kLd + k] = okb ? b : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 32; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], acc, 0, 0, 0);
        __syncthreads();
        chain += 32;
        if (chain == kShiftChain) {     // (uniform)
            chain = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                tot[r] += acc[r];
                acc[r] = 0.f;
            }
        }
    }
    float *out = partials + ((size_t)d * max_slices + blockIdx.x) * C * C;
    const int j = b0 + bj * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = a0 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (i < C && j < C) out[(size_t)i * C + j] = tot[r] + acc[r];
    }
}

// ---------------------------------------------------------------------------------------------- merge
// A thread owns one element (a, b) of one offset.  T null: x_out [offset][C][C] = X.  Otherwise weights
// [offset][2][C][C] = (n / (n_d |Delta|)) D_d and its transpose, e_parts [offset][blocks] = the block's sum of D^2
// over |Delta|.
__global__ __launch_bounds__(256) void shift_merge_kernel(const float *__restrict__ partials, int C, int h, int w,
                                                          ShiftOffsets off, int slice_len, int max_slices,
                                                          const float *__restrict__ T, float *__restrict__ x_out,
                                                          float *__restrict__ weights, float *__restrict__ e_parts) {
    __shared__ double red[256];
    const int d = blockIdx.y;
    const int nd = (h - off.dy[d]) * (w - off.dx[d]);
    const int slices = (nd + slice_len - 1) / slice_len;
    const size_t cc = (size_t)C * C, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    double e = 0.0;
    if (idx < cc) {
        const float *p = partials + (size_t)d * max_slices * cc + idx;
        double sum = 0.0;
        for (int s = 0; s < slices; ++s) sum += (double)p[(size_t)s * cc];
        const float x = (float)(sum / ((double)C * (double)nd));
        if (T) {
            const float diff = x - T[(size_t)d * cc + idx];
            const float scale = (float)((double)h * (double)w / ((double)nd * (double)off.n));
            const float wv = scale * diff;
            const size_t a = idx / C, b = idx - a * C;
            weights[(size_t)(2 * d) * cc + idx] = wv;
            weights[(size_t)(2 * d + 1) * cc + b * C + a] = wv;
            e = (double)diff * (double)diff;
        } else {
            x_out[(size_t)d * cc + idx] = x;
        }
    }
    if (!T) return;     // (uniform)
    red[threadIdx.x] = e;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) e_parts[(size_t)d * gridDim.x + blockIdx.x] = (float)(red[0] / (double)off.n);
}

// ------------------------------------------------------------------------------------------- gradient
// S (a, p) = sum over (offset, sign, b) of W[offset][sign][a][b] F_b(p +- delta); a wave owns a 32 x 32 block of the
// 64 channels x 64 pixels tile.  abs_parts[channel block][pixel block] = the tile's sum of |S|.
__global__ __launch_bounds__(256) void shift_grad_kernel(const float *__restrict__ F, const float *__restrict__ weights,
                                                         int C, int h, int w, ShiftOffsets off, float *__restrict__ S,
                                                         float *__restrict__ abs_parts) {
    __shared__ float At[64 * kLd];
    __shared__ float Bt[64 * kLd];
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int bi = wave >> 1, bj = wave & 1;
    const int n = h * w;
    const int p0 = blockIdx.x * 64, a0 = blockIdx.y * 64;
    const size_t cc = (size_t)C * C;
    // the operand rows a thread stages: pixel p0 + pp of channels kb0, kb0 + 4, ...; weights row m0 + 8 r, column k
    const int pp = tid & 63, kb0 = tid >> 6;
    const int k = tid & 31, m0 = tid >> 5;
    const int p = p0 + pp;
    const bool okp = p < n;
    const int y = okp ? p / w : 0, x = okp ? p - y * w : 0;
    f32x16 acc, tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = tot[r] = 0.f;
    const float *ap = At + (bi * 32 + l31) * kLd + half;
    const float *bp = Bt + (bj * 32 + l31) * kLd + half;
    int chain = 0;
    for (int ds = 0; ds < 2 * off.n; ++ds) {
        const int d = ds >> 1, sign = ds & 1;
        const int yy = sign ? y - off.dy[d] : y + off.dy[d];
        const int xx = sign ? x - off.dx[d] : x + off.dx[d];
        const bool okd = okp && yy >= 0 && yy < h && xx >= 0 && xx < w;
        const size_t src = okd ? (size_t)yy * w + xx : 0;
        const float *__restrict__ Wd = weights + (size_t)ds * cc;
        for (int bk = 0; bk < C; bk += 32) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int m = m0 + 8 * r, kb = kb0 + 4 * r;
                const bool oka = a0 + m < C;
                const float a = Wd[oka ? (size_t)(a0 + m) * C + bk + k : 0];
                const float b = F[okd ? (size_t)(bk + kb) * n + src : 0];
                At[m * kLd + k] = oka ? a : 0.f;
                Bt[pp * kLd + kb] = okd ? b : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < 32; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], acc, 0, 0, 0);
            __syncthreads();
            chain += 32;
            if (chain == kShiftChain) {     // (uniform)
                chain = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tot[r] += acc[r];
                    acc[r] = 0.f;
                }
            }
        }
    }
    const int col = p0 + bj * 32 + l31;
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = a0 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float v = tot[r] + acc[r];
        if (i < C && col < n) {
            S[(size_t)i * n + col] = v;
            sum += fabsf(v);
        }
    }
    sum = wave_sum_f(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) abs_parts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace

int shift_cross_launch(hipStream_t s, const float *feat, int C, int h, int w, const ShiftOffsets &off,
                       const ShiftScratch &x) {
    const int nb = ceil_div(C, 64), HW = h * w;
    shift_cross_kernel<<<dim3(shift_slices(HW), nb * nb, off.n), 256, 0, s>>>(feat, C, h, w, off, shift_slice_len(HW),
                                                                             shift_slices(HW), x.partials);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int shift_merge_launch(hipStream_t s, int C, int h, int w, const ShiftOffsets &off, const ShiftScratch &x,
                       const float *targets, float *x_out, int *n_e) {
    if (targets ? x_out != nullptr : !x_out) {
        set_error("shift_merge_launch: targets, or an output for X, are expected");
        return STX_ERR_ARG;
    }
    const int HW = h * w, blocks = (int)(((size_t)C * C + 255) / 256);
    shift_merge_kernel<<<dim3(blocks, off.n), 256, 0, s>>>(x.partials, C, h, w, off, shift_slice_len(HW),
                                                          shift_slices(HW), targets, x_out, x.weights, x.e_parts);
    STX_CHECK_LAUNCH();
    if (n_e) *n_e = blocks * off.n;
    return STX_OK;
}

int shift_grad_launch(hipStream_t s, const float *feat, int C, int h, int w, const ShiftOffsets &off,
                      const ShiftScratch &x, float *sgrad, int *n_abs) {
    const int pb = ceil_div(h * w, 64), cb = ceil_div(C, 64);
    shift_grad_kernel<<<dim3(pb, cb), 256, 0, s>>>(feat, x.weights, C, h, w, off, sgrad, x.abs_parts);
    STX_CHECK_LAUNCH();
    *n_abs = pb * cb;
    return STX_OK;
}

}  // namespace stx
