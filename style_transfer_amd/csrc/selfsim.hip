// The self-similarity content term (STROTSS; NNST uses the same term): it holds the PATTERN of similarities between
// positions of the content picture, not the feature values (include/stx.h, stx_set_selfsim_targets).  A tapped
// blob F [C][h][w] and the tile's window c of the layer's content map are sampled on the grid of selfsim_grid --
// N positions (a g, b g) in raster order -- and with unit columns x_i of F, y_i of c:
//   DX_ij = 1 - x_i . x_j (0 on the diagonal),  sX_j = sum_i DX_ij + N 1e-6,  PX = DX / sX (columns);  DC, sC, PC from y
//   d = PX - PC,  T = sign d,  E = sum |d| / N,  u_j = sum_k T_kj PX_kj,  A_ij = (T_ij - u_j) / sX_j (0 on the diagonal)
//   q_i = - sum_j (A_ij + A_ji) x_j,   S_i = (q_i - (q_i . x_i) x_i) / (2 r_i) at the grid positions, 0 elsewhere.
// The launches, O(N^2 C), no atomics, every sum in a fixed order:
//   1. selfsim_prepare_kernel  both sides as a batch of 2: the sampled columns' norms in double, 1 / r_i and the
//                              unit columns as float32 rows [N][C].  One kernel reads F and the window: a side is a
//                              pointer with a map size and an origin, and the origin wraps (a plain array is a map
//                              of its own size at origin 0), so equal values give equal bits on both sides.
//   2. selfsim_dist_kernel     D = 1 - R R^T by v_mfma_f32_32x32x2_f32 (64 x 64 outputs per workgroup, float32
//                              accumulation in channel order), both sides in one launch.  The epilogue forces the
//                              diagonal to 0, masks rows and columns >= N, writes D [N][N] and leaves the tile's
//                              column sums in slot [row block][column].  The whole matrix is formed: no symmetric
//                              half is skipped, so the column sums have one order on both sides.
//   3. the column pass         two sweeps over 64 x 64 tiles.  selfsim_sign_kernel finishes sX and sC from the
//                              slots, forms d and T (int8 [N][N]) and leaves the partials of E and of u_j;
//                              selfsim_weight_kernel finishes u_j and writes A over DX.
//   4. selfsim_grad_kernel     q = -(A + A^T) R by the same MFMA, K = N: the operand tile A_ij + A_ji is formed
//                              in LDS from two coalesced reads, ragged K padded with zeros there.
//      selfsim_project_kernel  projects q_i off x_i, scales by 1 / (2 r_i), writes S into the blob's [C][h][w]
//                              layout at the grid positions and leaves the partials of sum |S|.  With g > 1 the
//                              gradient array is cleared first (the injection reads the whole array).
// A blob that equals its window has DX = DC and sX = sC bit for bit, so d = 0, T = 0, A = +0 and S = +0: the term
// then adds exactly nothing to the loss and to the gradient.

#include <algorithm>

#include "common.h"

namespace stx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

SelfsimGrid selfsim_grid(int h, int w, int points) {
    int g = 1;
    while ((long long)ceil_div(h, g) * ceil_div(w, g) > points) ++g;
    return SelfsimGrid{g, ceil_div(h, g), ceil_div(w, g), ceil_div(h, g) * ceil_div(w, g)};
}

int selfsim_check(const char *who, int C, int points) {
    if (C <= 0 || points < 2 || points > kSelfsimMaxPoints) {
        set_error("%s: %d channels, %d points (2 to %d points are expected)", who, C, points, kSelfsimMaxPoints);
        return STX_ERR_ARG;
    }
    if (C % 64 != 0) {
        set_error("%s: %d channels (a multiple of 64 is expected)", who, C);
        return STX_ERR_UNSUPPORTED;
    }
    return STX_OK;
}

static size_t selfsim_round64(size_t v) { return (v + 63) & ~(size_t)63; }

SelfsimScratch selfsim_scratch(float *base, int C, int N) {
    const size_t n = (size_t)N, nb = (size_t)ceil_div(N, 64);
    SelfsimScratch x;
    size_t off = 0;
    const auto take = [&](size_t floats) {      // (base null: only the size is asked for)
        float *at = base ? base + off : nullptr;
        off += selfsim_round64(floats);
        return at;
    };
    x.rows = take(2 * n * C);
    x.inv_r = take(2 * n);
    x.D = take(2 * n * n);
    x.col_parts = take(2 * nb * n);
    x.u_parts = take(nb * n);
    x.q = take(n * C);
    x.T = reinterpret_cast<signed char *>(take((n * n + 3) / 4));
    x.e_parts = take(nb * nb);
    x.abs_parts = take(nb);
    x.floats = off;
    return x;
}

size_t selfsim_scratch_floats(int C, int N) { return selfsim_scratch(nullptr, C, N).floats; }

namespace {

constexpr int kLd = 33;         // a 32-float LDS row and one of padding: the 32 lanes of an operand read hit 32 banks

// ------------------------------------------------------------------------------------------- prepare
// A workgroup owns 64 grid positions of one side (blockIdx.y); position o is the pixel ((o / gw) g, (o % gw) g).
__global__ __launch_bounds__(256) void selfsim_prepare_kernel(SelfsimSource sf, SelfsimSource sc, int C, int g, int gw,
                                                              int N, float *__restrict__ rows,
                                                              float *__restrict__ inv_r) {
    __shared__ double red[4][64];
    __shared__ float sinv[64];
    __shared__ float tile[64][65];
    const SelfsimSource src = blockIdx.y ? sc : sf;
    const float *__restrict__ F = src.p;
    rows += (size_t)blockIdx.y * N * C;
    inv_r += (size_t)blockIdx.y * N;
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int o = min(blockIdx.x * 64 + col, N - 1);        // (positions past the end re-read the last one)
    int yy = (src.oy + (o / gw) * g) % src.mh, xx = (src.ox + (o % gw) * g) % src.mw;
    if (yy < 0) yy += src.mh;
    if (xx < 0) xx += src.mw;
    const size_t plane = (size_t)src.mh * src.mw, at0 = (size_t)yy * src.mw + xx;
    double acc = 0.0;
    for (int c = grp; c < C; c += 4) {
        const double v = (double)F[(size_t)c * plane + at0];
        acc += v * v;
    }
    red[grp][col] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        const double ss = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
        const float inv = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f;
        sinv[col] = inv;
        if (blockIdx.x * 64 + col < N) inv_r[o] = inv;
    }
    for (int c0 = 0; c0 < C; c0 += 64) {
        __syncthreads();        // (sinv is written; the tile of the round before is read)
        for (int cc = grp; cc < 64; cc += 4) tile[cc][col] = F[(size_t)(c0 + cc) * plane + at0];
        __syncthreads();
        for (int u = 0; u < 16; ++u) {
            const int item = threadIdx.x + 256 * u, col2 = item >> 6, cc = item & 63;
            const int o2 = blockIdx.x * 64 + col2;
            if (o2 < N) rows[(size_t)o2 * C + c0 + cc] = tile[cc][col2] * sinv[col2];
        }
    }
}

// ------------------------------------------------------------------------------------------ distances
// D (i, j) = 1 - sum_c R[i][c] R[j][c] of side blockIdx.z; a wave owns a 32 x 32 block of the 64 x 64 tile.
__global__ __launch_bounds__(256) void selfsim_dist_kernel(const float *__restrict__ rows, int C, int N,
                                                           float *__restrict__ D, float *__restrict__ col_parts) {
    __shared__ float At[64 * kLd];
    __shared__ float Bt[64 * kLd];
    __shared__ float csum[4][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int bi = wave >> 1, bj = wave & 1;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const float *__restrict__ R = rows + (size_t)blockIdx.z * N * C;
    D += (size_t)blockIdx.z * N * N;
    col_parts += ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * N;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *ap = At + (bi * 32 + l31) * kLd + half;
    const float *bp = Bt + (bj * 32 + l31) * kLd + half;
    for (int k0 = 0; k0 < C; k0 += 32) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * q, m = e >> 5, k = e & 31;
            const bool oka = i0 + m < N, okb = j0 + m < N;
            const float a = R[oka ? (size_t)(i0 + m) * C + k0 + k : 0];
            const float b = R[okb ? (size_t)(j0 + m) * C + k0 + k : 0];
            At[m * kLd + k] = oka ? a : 0.f;
            Bt[m * kLd + k] = okb ? b : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k], bp[k], acc, 0, 0, 0);
        __syncthreads();
    }
    // the tile's column sums in a fixed order: a lane's 16 rows, then the four (row half, lane half) pieces in turn
    const int j = j0 + bj * 32 + l31;
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const bool in = i < N && j < N;
        const float v = in && i != j ? 1.f - acc[r] : 0.f;
        if (in) D[(size_t)i * N + j] = v;
        sum += v;
    }
    csum[bi * 2 + half][bj * 32 + l31] = sum;
    __syncthreads();
    if (tid < 64 && j0 + tid < N)
        col_parts[j0 + tid] = ((csum[0][tid] + csum[1][tid]) + csum[2][tid]) + csum[3][tid];
}

// (the partials of E, u_j and sum |S| are added in double inside a workgroup and rounded once: a float32 result's
// own rounding is then all that a partial adds to the error)
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// sX_j (or sC_j): the row blocks' slots in turn, then N 1e-6
__device__ __forceinline__ float selfsim_col_sum(const float *__restrict__ parts, int nb, int N, int j) {
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s += parts[(size_t)b * N + j];
    return s + (float)N * kSelfsimEps;
}

// ---------------------------------------------------------------------------------------- column pass
// First sweep, a 64 x 64 tile per workgroup: d = PX - PC, T = sign d, the tile's sum of |d| / N and, per column,
// its sum of T PX.  A thread owns a column and every fourth row.
__global__ __launch_bounds__(256) void selfsim_sign_kernel(const float *__restrict__ D, const float *__restrict__ col_parts,
                                                           int N, signed char *__restrict__ T,
                                                           float *__restrict__ u_parts, float *__restrict__ e_parts) {
    __shared__ double red[2][4][64];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int nb = gridDim.y, i0 = blockIdx.y * 64, j = blockIdx.x * 64 + col;
    const float *__restrict__ DX = D, *__restrict__ DC = D + (size_t)N * N;
    double e = 0.0, u = 0.0;
    if (j < N) {
        const float sx = selfsim_col_sum(col_parts, nb, N, j);
        const float sc = selfsim_col_sum(col_parts + (size_t)nb * N, nb, N, j);
        for (int t = 0; t < 16; ++t) {
            const int i = i0 + grp + 4 * t;
            if (i >= N) break;
            const size_t at = (size_t)i * N + j;
            const float px = DX[at] / sx, pc = DC[at] / sc;
            const float d = px - pc;
            const float sign = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            T[at] = (signed char)sign;
            e += (double)fabsf(d);
            u += (double)(sign * px);
        }
    }
    red[0][grp][col] = e;
    red[1][grp][col] = u;
    __syncthreads();
    if (threadIdx.x < 64) {
        const double ec = ((red[0][0][col] + red[0][1][col]) + red[0][2][col]) + red[0][3][col];
        const double uc = ((red[1][0][col] + red[1][1][col]) + red[1][2][col]) + red[1][3][col];
        if (j < N) u_parts[(size_t)blockIdx.y * N + j] = (float)uc;
        const double et = wave_sum_d(ec);
        if (threadIdx.x == 0) e_parts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (float)(et / (double)N);
    }
}

// Second sweep: u_j from its slots in turn, A_ij = (T_ij - u_j) / sX_j, 0 on the diagonal, written where DX was.
__global__ __launch_bounds__(256) void selfsim_weight_kernel(const signed char *__restrict__ T,
                                                             const float *__restrict__ col_parts,
                                                             const float *__restrict__ u_parts, int N,
                                                             float *__restrict__ A) {
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int nb = gridDim.y, i0 = blockIdx.y * 64, j = blockIdx.x * 64 + col;
    if (j >= N) return;
    const float sx = selfsim_col_sum(col_parts, nb, N, j);
    float u = 0.f;
    for (int b = 0; b < nb; ++b) u += u_parts[(size_t)b * N + j];
    for (int t = 0; t < 16; ++t) {
        const int i = i0 + grp + 4 * t;
        if (i >= N) break;
        const size_t at = (size_t)i * N + j;
        A[at] = i != j ? ((float)T[at] - u) / sx : 0.f;
    }
}

// ------------------------------------------------------------------------------------------- gradient
// q (i, c) = - sum_j (A_ij + A_ji) R[j][c]; a wave owns a 32 x 32 block of the 64 x 64 tile.
__global__ __launch_bounds__(256) void selfsim_grad_kernel(const float *__restrict__ A, const float *__restrict__ R, int C,
                                                           int N, float *__restrict__ q) {
    __shared__ float At[64 * kLd];
    __shared__ float Bt[64 * kLd];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int bi = wave >> 1, bj = wave & 1;
    const int i0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *ap = At + (bi * 32 + l31) * kLd + half;
    const float *bp = Bt + (bj * 32 + l31) * kLd + half;
    for (int k0 = 0; k0 < N; k0 += 32) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {       // A_ij read along j, and the rows R[j] along c
            const int e = tid + 256 * p, m = e >> 5, k = e & 31;
            const bool ok = i0 + m < N && k0 + k < N;
            const float a = A[ok ? (size_t)(i0 + m) * N + k0 + k : 0];
            At[m * kLd + k] = ok ? a : 0.f;
            const int kb = e >> 6, c = e & 63;
            const bool okb = k0 + kb < N;
            const float b = R[okb ? (size_t)(k0 + kb) * C + c0 + c : 0];
            Bt[c * kLd + kb] = okb ? b : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 8; ++p) {       // ... plus A_ji, read along i
            const int e = tid + 256 * p, k = e >> 6, m = e & 63;
            const bool ok = i0 + m < N && k0 + k < N;
            const float a = A[ok ? (size_t)(k0 + k) * N + i0 + m : 0];
            At[m * kLd + k] += ok ? a : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k], bp[k], acc, 0, 0, 0);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (i < N) q[(size_t)i * C + c0 + bj * 32 + l31] = 0.f - acc[r];       // (+0 where the sum is +0)
    }
}

// S_i = (q_i - (q_i . x_i) x_i) / (2 r_i) into the blob's layout; a workgroup owns 64 grid positions.
__global__ __launch_bounds__(256) void selfsim_project_kernel(const float *__restrict__ q, const float *__restrict__ R,
                                                              const float *__restrict__ inv_r, int C, int h, int w, int g,
                                                              int gw, int N, float *__restrict__ sgrad,
                                                              float *__restrict__ abs_parts) {
    __shared__ float tq[64][65];
    __shared__ float tx[64][65];
    __shared__ float red[4][64];
    __shared__ double ared[4][64];
    __shared__ float sdot[64];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int o0 = blockIdx.x * 64, o = o0 + col;
    const size_t HW = (size_t)h * w;
    float dot = 0.f;
    for (int c0 = 0; c0 < C; c0 += 64) {
        __syncthreads();
        for (int u = 0; u < 16; ++u) {
            const int item = threadIdx.x + 256 * u, row = item >> 6, cc = item & 63;
            const bool ok = o0 + row < N;
            const size_t at = ok ? (size_t)(o0 + row) * C + c0 + cc : 0;
            tq[row][cc] = ok ? q[at] : 0.f;
            tx[row][cc] = ok ? R[at] : 0.f;
        }
        __syncthreads();
        for (int cc = grp; cc < 64; cc += 4) dot += tq[col][cc] * tx[col][cc];
    }
    red[grp][col] = dot;
    __syncthreads();
    if (threadIdx.x < 64) sdot[col] = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
    const float scale = o < N ? 0.5f * inv_r[o] : 0.f;
    const size_t dst = o < N ? (size_t)(o / gw) * g * w + (size_t)(o % gw) * g : 0;
    double sum = 0.0;
    for (int c0 = 0; c0 < C; c0 += 64) {
        __syncthreads();        // (sdot is written; the tiles of the round before are read)
        for (int u = 0; u < 16; ++u) {
            const int item = threadIdx.x + 256 * u, row = item >> 6, cc = item & 63;
            const bool ok = o0 + row < N;
            const size_t at = ok ? (size_t)(o0 + row) * C + c0 + cc : 0;
            tq[row][cc] = ok ? q[at] : 0.f;
            tx[row][cc] = ok ? R[at] : 0.f;
        }
        __syncthreads();
        if (o < N) {
            const float d = sdot[col];
            for (int cc = grp; cc < 64; cc += 4) {
                const float v = (tq[col][cc] - d * tx[col][cc]) * scale;
                sgrad[(size_t)(c0 + cc) * HW + dst] = v;
                sum += (double)fabsf(v);
            }
        }
    }
    ared[grp][col] = sum;
    __syncthreads();
    if (threadIdx.x < 64) {
        const double t = wave_sum_d(((ared[0][col] + ared[1][col]) + ared[2][col]) + ared[3][col]);
        if (threadIdx.x == 0) abs_parts[blockIdx.x] = (float)t;
    }
}

}  // namespace

int selfsim_prepare_launch(hipStream_t s, const SelfsimSource &feat, const SelfsimSource &content, int C,
                           const SelfsimGrid &gr, const SelfsimScratch &x) {
    selfsim_prepare_kernel<<<dim3(ceil_div(gr.N, 64), 2), 256, 0, s>>>(feat, content, C, gr.g, gr.gw, gr.N, x.rows,
                                                                      x.inv_r);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int selfsim_dist_launch(hipStream_t s, int C, int N, const SelfsimScratch &x) {
    const int nb = ceil_div(N, 64);
    selfsim_dist_kernel<<<dim3(nb, nb, 2), 256, 0, s>>>(x.rows, C, N, x.D, x.col_parts);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int selfsim_cols_launch(hipStream_t s, int N, const SelfsimScratch &x, signed char *signs, int *n_e) {
    const int nb = ceil_div(N, 64);
    selfsim_sign_kernel<<<dim3(nb, nb), 256, 0, s>>>(x.D, x.col_parts, N, signs, x.u_parts, x.e_parts);
    STX_CHECK_LAUNCH();
    selfsim_weight_kernel<<<dim3(nb, nb), 256, 0, s>>>(signs, x.col_parts, x.u_parts, N, x.D);
    STX_CHECK_LAUNCH();
    *n_e = nb * nb;
    return STX_OK;
}

int selfsim_grad_launch(hipStream_t s, int C, int h, int w, const SelfsimGrid &gr, const SelfsimScratch &x,
                        float *sgrad, int *n_abs) {
    const int nb = ceil_div(gr.N, 64);
    if (gr.g > 1) STX_HIP(hipMemsetAsync(sgrad, 0, (size_t)C * h * w * sizeof(float), s));
    selfsim_grad_kernel<<<dim3(C / 64, nb), 256, 0, s>>>(x.D, x.rows, C, gr.N, x.q);
    STX_CHECK_LAUNCH();
    selfsim_project_kernel<<<nb, 256, 0, s>>>(x.q, x.rows, x.inv_r, C, h, w, gr.g, gr.gw, gr.N, sgrad, x.abs_parts);
    STX_CHECK_LAUNCH();
    *n_abs = nb;
    return STX_OK;
}

}  // namespace stx
