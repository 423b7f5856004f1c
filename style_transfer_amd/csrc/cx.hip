// The contextual loss as a style term (Mechrez, Talmi, Zelnik-Manor, ECCV 2018; include/stx.h, stx_set_cx_targets):
// soft, scale-free matching of a blob's feature vectors against a style bank.  A tapped blob F [C][h][w] is sampled
// on the grid of selfsim_grid -- N positions (a g, b g) in raster order -- and the bank is M centred unit rows b_k
// with the mean mu of the raw rows they came from.  With x_i the unit vector of f_i - mu and s_ik = x_i . b_k:
//   k*_i = argmax_k s_ik (lowest k),  tau_i = eta (1 - s_ik* + 1e-5),  p_ik = softmax_k (s_ik - s_ik*) / tau_i
//   i*_k = argmax_i p_ik (lowest i),  CX = (1/M) sum_k p_{i*_k k},  E = -log CX
//   g_ik = dE/ds_ik with k*, i* held,  q_i = sum_k g_ik b_k,  S_i = (q_i - (q_i . x_i) x_i) / r_i on the grid, 0 elsewhere.
// The launches, O(N M C), no atomics, every sum in a fixed order:
//   1. cx_prepare_kernel   the sampled columns minus mu, their norms in double (nnfm_prepare_kernel's order), 1 / r_i
//                          and the unit columns as float32 rows [N][C].  The same kernel makes a bank from raw rows
//                          (stx_cx_bank) and, without mu, gathers raw rows from a map (stx_cx_rows).
//   2. cx_score_kernel     s = X B^T by v_mfma_f32_32x32x2_f32 (64 x 64 outputs per workgroup, float32 accumulation in
//                          channel order; selfsim_dist_kernel's tiling and LDS layout, rectangular).  Rows >= N and
//                          columns >= M are masked; the epilogue leaves per row the tile's best (score, lowest k) in
//                          slot [column block][row].
//   3. cx_row_kernel       a workgroup per row: k* from the slots in block order, tau, e = expf(.) (the accurate
//                          expf, not a fast intrinsic), Z and sum e s in double in a fixed order, p = e / Z.
//   4. cx_col_kernel       64 x 64 tiles: per column the tile's best (p, lowest i); cx_col_finish_kernel merges the
//                          row blocks' bests in block order ("greater value, else lower index") into i*_k and leaves
//                          the partials of sum_k m_k.
//   5. cx_weight_kernel    a workgroup per row: CX from the partials in block order, P_i and Q_i in double, g over s;
//                          row 0 leaves E.
//   6. cx_grad_kernel      q = g B by the same MFMA with K = M cut into slices over workgroups (cx_slice_len); the
//                          loads of step t + 1 are issued before the MFMAs of step t.  A block of 64 rows none of
//                          which owns a column (P_i = 0 throughout) has g = +0 and is written as zeros without the
//                          product: the same bits.
//      cx_reduce_kernel    adds the slices' partial tiles in slice order and leaves each 64-channel block's share of
//                          q_i . x_i; cx_project_kernel adds the shares in block order, projects q_i off x_i, scales
//                          by 1 / r_i, writes S into the blob's [C][h][w] layout and leaves the partials of sum |S|.
//                          Both run (C / 64) x ceil(N / 64) workgroups.  With g > 1 the gradient array is cleared
//                          first.

#include <algorithm>
#include <cmath>

#include "common.h"

namespace stx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

int cx_check(const char *who, int C, int points, long long M, double eta) {
    if (C <= 0 || points < 2 || points > kCxMaxPoints) {
        set_error("%s: %d channels, %d points (2 to %d points are expected)", who, C, points, kCxMaxPoints);
        return STX_ERR_ARG;
    }
    if (M < 1 || M > kCxMaxRows) {
        set_error("%s: %lld bank rows (1 to %d are expected)", who, M, kCxMaxRows);
        return STX_ERR_ARG;
    }
    if (!(eta > 0.0) || !std::isfinite(eta)) {
        set_error("%s: bandwidth %g (a finite number above 0 is expected)", who, eta);
        return STX_ERR_ARG;
    }
    if (C % 64 != 0) {
        set_error("%s: %d channels (a multiple of 64 is expected)", who, C);
        return STX_ERR_UNSUPPORTED;
    }
    if ((long long)points * M > kCxMaxCells) {
        set_error("%s: %d points against %lld bank rows (points x rows up to 2^24 is expected)", who, points, M);
        return STX_ERR_UNSUPPORTED;
    }
    return STX_OK;
}

// The gradient product's K slice: enough workgroups to fill the device (about 1024), at most ceil(M / 128) slices --
// about 128 rows each or more (M = 129: two of 96) --, a multiple of the 32-row LDS stage.
int cx_slice_len(int C, int N, int M) {
    const int base = (C / 64) * ceil_div(N, 64);
    const int slices = std::min(std::max(ceil_div(1024, base), 1), ceil_div(M, 128));
    return ceil_div(ceil_div(M, slices), 32) * 32;
}

static size_t cx_round64(size_t v) { return (v + 63) & ~(size_t)63; }

CxScratch cx_scratch(float *base, int C, int N, int M) {
    const size_t n = (size_t)N, m = (size_t)M, nb = (size_t)ceil_div(N, 64), mb = (size_t)ceil_div(M, 64);
    CxScratch x;
    size_t off = 0;
    const auto take = [&](size_t floats) {      // (base null: only the size is asked for)
        float *at = base ? base + off : nullptr;
        off += cx_round64(floats);
        return at;
    };
    x.rows = take(n * C);
    x.inv_r = take(n);
    x.S = take(n * m);
    x.P = take(n * m);
    x.best_val = take(mb * n);
    x.best_idx = reinterpret_cast<int *>(take(mb * n));
    x.kstar = reinterpret_cast<int *>(take(n));
    x.tau = take(n);
    x.u = take(n);
    x.row_p = take(n);
    x.col_val = take(nb * m);
    x.col_idx = reinterpret_cast<int *>(take(nb * m));
    x.winner = reinterpret_cast<int *>(take(m));
    x.m_parts = take((size_t)ceil_div(M, 256));
    x.qp = take((size_t)ceil_div(M, cx_slice_len(C, N, M)) * n * C);
    x.e_part = take(1);
    x.dot_parts = take((size_t)(C / 64) * n);
    x.abs_parts = take(nb * (C / 64));
    x.floats = off;
    return x;
}

size_t cx_scratch_floats(int C, int N, int M) { return cx_scratch(nullptr, C, N, M).floats; }

namespace {

constexpr int kLd = 33;         // a 32-float LDS row and one of padding: the 32 lanes of an operand read hit 32 banks

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// The workgroup's sum of v in a fixed order (a wave's tree, then the four waves in turn), on every thread.
__device__ __forceinline__ double block_sum_d(double v, double *red /*[4]*/) {
    const double t = wave_sum_d(v);
    __syncthreads();            // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ------------------------------------------------------------------------------------------- prepare
// A workgroup owns 64 positions.  kFromRows: position o is row o of raw rows [N][C]; otherwise the pixel
// ((o / gw) g, (o % gw) g) of planes [C][h][w].  mu null: the raw values as rows, nothing else.
template <bool kFromRows>
__global__ __launch_bounds__(256) void cx_prepare_kernel(const float *__restrict__ F, int C, int h, int w, int g, int gw,
                                                         int N, const float *__restrict__ mu, float *__restrict__ rows,
                                                         float *__restrict__ inv_r) {
    __shared__ double red[4][64];
    __shared__ float sinv[64];
    __shared__ float tile[64][65];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int o = min(blockIdx.x * 64 + col, N - 1);        // (positions past the end re-read the last one)
    const size_t step = kFromRows ? (size_t)1 : (size_t)h * w;
    const size_t at0 = kFromRows ? (size_t)o * C : (size_t)(o / gw) * g * w + (size_t)(o % gw) * g;
    if (mu) {
        double acc = 0.0;
        for (int c = grp; c < C; c += 4) {
            const double v = (double)(F[(size_t)c * step + at0] - mu[c]);
            acc += v * v;
        }
        red[grp][col] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        float inv = 1.f;
        if (mu) {
            const double ss = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
            inv = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f;
        }
        sinv[col] = inv;
        if (inv_r && blockIdx.x * 64 + col < N) inv_r[o] = inv;
    }
    for (int c0 = 0; c0 < C; c0 += 64) {
        __syncthreads();        // (sinv is written; the tile of the round before is read)
        for (int cc = grp; cc < 64; cc += 4) {
            const float v = F[(size_t)(c0 + cc) * step + at0];
            tile[cc][col] = mu ? v - mu[c0 + cc] : v;
        }
        __syncthreads();
        for (int u = 0; u < 16; ++u) {
            const int item = threadIdx.x + 256 * u, col2 = item >> 6, cc = item & 63;
            const int o2 = blockIdx.x * 64 + col2;
            if (o2 < N) rows[(size_t)o2 * C + c0 + cc] = mu ? tile[cc][col2] * sinv[col2] : tile[cc][col2];
        }
    }
}

// mu[c] = (1/M) sum_k Y[k][c] in double: a thread owns a channel and every fourth row, the four in turn.
__global__ __launch_bounds__(256) void cx_mean_kernel(const float *__restrict__ Y, int C, int M, float *__restrict__ mu) {
    __shared__ double red[4][64];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + col;
    double acc = 0.0;
    for (int k = grp; k < M; k += 4) acc += (double)Y[(size_t)k * C + c];
    red[grp][col] = acc;
    __syncthreads();
    if (threadIdx.x < 64)
        mu[c] = (float)((((red[0][col] + red[1][col]) + red[2][col]) + red[3][col]) / (double)M);
}

// --------------------------------------------------------------------------------------------- scores
// s (i, k) = sum_c X[i][c] B[k][c]; a wave owns a 32 x 32 block of the 64 x 64 tile.
__global__ __launch_bounds__(256) void cx_score_kernel(const float *__restrict__ X, const float *__restrict__ B, int C,
                                                       int N, int M, float *__restrict__ S,
                                                       float *__restrict__ best_val, int *__restrict__ best_idx) {
    __shared__ float At[64 * kLd];
    __shared__ float Bt[64 * kLd];
    __shared__ float tile[64][65];
    __shared__ float qv[4][64];
    __shared__ int qi[4][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int bi = wave >> 1, bj = wave & 1;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *ap = At + (bi * 32 + l31) * kLd + half;
    const float *bp = Bt + (bj * 32 + l31) * kLd + half;
    for (int k0 = 0; k0 < C; k0 += 32) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int e = tid + 256 * q, m = e >> 5, k = e & 31;
            const bool oka = i0 + m < N, okb = j0 + m < M;
            const float a = X[oka ? (size_t)(i0 + m) * C + k0 + k : 0];
            const float b = B[okb ? (size_t)(j0 + m) * C + k0 + k : 0];
            At[m * kLd + k] = oka ? a : 0.f;
            Bt[m * kLd + k] = okb ? b : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k], bp[k], acc, 0, 0, 0);
        __syncthreads();
    }
    const int jt = bj * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int it = bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (i0 + it < N && j0 + jt < M) S[(size_t)(i0 + it) * M + j0 + jt] = acc[r];
        tile[it][jt] = acc[r];
    }
    __syncthreads();
    // the tile's best per row: a thread scans 16 columns in order, then the four quarters in order (strict >:
    // the lowest index among equal scores)
    {
        const int row = tid & 63, quarter = tid >> 6;
        float best = -INFINITY;
        int at = -1;
        for (int t = 0; t < 16; ++t) {
            const int j = quarter * 16 + t;
            if (j0 + j >= M) break;
            const float v = tile[row][j];
            if (v > best) best = v, at = j0 + j;
        }
        qv[quarter][row] = best;
        qi[quarter][row] = at;
    }
    __syncthreads();
    if (tid < 64 && i0 + tid < N) {
        float best = qv[0][tid];
        int at = qi[0][tid];
#pragma unroll
        for (int quarter = 1; quarter < 4; ++quarter)
            if (qv[quarter][tid] > best) best = qv[quarter][tid], at = qi[quarter][tid];
        best_val[(size_t)blockIdx.x * N + i0 + tid] = best;
        best_idx[(size_t)blockIdx.x * N + i0 + tid] = at;
    }
}

// ------------------------------------------------------------------------------------------- row pass
// A workgroup owns row i: k*_i, tau_i, e_ik, Z_i, u_i, p_ik.
__global__ __launch_bounds__(256) void cx_row_kernel(const float *__restrict__ S, const float *__restrict__ best_val,
                                                     const int *__restrict__ best_idx, int N, int M, int mb, float eta,
                                                     float *__restrict__ P, int *__restrict__ kstar,
                                                     float *__restrict__ tau_out, float *__restrict__ u_out) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ double red[4];
    const int tid = threadIdx.x, i = blockIdx.x;
    if (tid < mb) {
        sv[tid] = best_val[(size_t)tid * N + i];
        si[tid] = best_idx[(size_t)tid * N + i];
    }
    __syncthreads();
    float best = sv[0];
    int kb = si[0];
    for (int b = 1; b < mb; ++b)        // the column blocks in order: the lowest k among equal scores
        if (sv[b] > best) best = sv[b], kb = si[b];
    const float tau = eta * ((1.f - best) + kCxEps);
    const float *__restrict__ s_row = S + (size_t)i * M;
    float *__restrict__ p_row = P + (size_t)i * M;
    double z = 0.0, us = 0.0;
    for (int k = tid; k < M; k += 256) {
        const float s = s_row[k];
        const float e = expf((s - best) / tau);
        p_row[k] = e;
        z += (double)e;
        us += (double)e * (double)s;
    }
    z = block_sum_d(z, red);
    us = block_sum_d(us, red);
    const float zf = (float)z;
    for (int k = tid; k < M; k += 256) p_row[k] = p_row[k] / zf;      // (a thread's own e)
    if (tid == 0) {
        kstar[i] = kb;
        tau_out[i] = tau;
        u_out[i] = (float)(us / z);
    }
}

// ---------------------------------------------------------------------------------------- column pass
__device__ __forceinline__ void cx_take(float v, int at, float &best, int &best_at) {     // greater value, else lower index
    if (v > best || (v == best && at < best_at)) best = v, best_at = at;
}

// A 64 x 64 tile per workgroup: per column the tile's best (p, lowest i).  A thread owns a column and every fourth row.
__global__ __launch_bounds__(256) void cx_col_kernel(const float *__restrict__ P, int N, int M, float *__restrict__ col_val,
                                                     int *__restrict__ col_idx) {
    __shared__ float cv[4][64];
    __shared__ int ci[4][64];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int i0 = blockIdx.y * 64, k = blockIdx.x * 64 + col;
    float best = -1.f;
    int at = 0x7fffffff;
    if (k < M) {
        for (int t = 0; t < 16; ++t) {
            const int i = i0 + grp + 4 * t;
            if (i >= N) break;
            const float v = P[(size_t)i * M + k];
            if (v > best) best = v, at = i;
        }
    }
    cv[grp][col] = best;
    ci[grp][col] = at;
    __syncthreads();
    if (threadIdx.x < 64 && k < M) {
        best = cv[0][col], at = ci[0][col];
#pragma unroll
        for (int q = 1; q < 4; ++q) cx_take(cv[q][col], ci[q][col], best, at);
        col_val[(size_t)blockIdx.y * M + k] = best;
        col_idx[(size_t)blockIdx.y * M + k] = at;
    }
}

// m_k and i*_k from the row blocks' bests in block order; the workgroup's sum of m_k over its 256 columns.
__global__ __launch_bounds__(256) void cx_col_finish_kernel(const float *__restrict__ col_val, const int *__restrict__ col_idx,
                                                            int nb, int M, int *__restrict__ winner,
                                                            int *__restrict__ winner_out, float *__restrict__ m_parts) {
    __shared__ double red[4];
    const int k = blockIdx.x * 256 + threadIdx.x;
    float best = 0.f;
    if (k < M) {
        best = col_val[k];
        int at = col_idx[k];
        for (int b = 1; b < nb; ++b) cx_take(col_val[(size_t)b * M + k], col_idx[(size_t)b * M + k], best, at);
        winner[k] = at;
        if (winner_out) winner_out[k] = at;
    }
    const double sum = block_sum_d((double)best, red);
    if (threadIdx.x == 0) m_parts[blockIdx.x] = (float)sum;
}

// A workgroup owns row i: P_i, Q_i over the columns the row owns, then g over s.
__global__ __launch_bounds__(256) void cx_weight_kernel(float *__restrict__ S, const float *__restrict__ P,
                                                        const int *__restrict__ winner, const float *__restrict__ m_parts,
                                                        int n_mparts, const int *__restrict__ kstar,
                                                        const float *__restrict__ tau_in, const float *__restrict__ u_in,
                                                        int M, float eta, float *__restrict__ row_p,
                                                        int *__restrict__ kbest_out, float *__restrict__ e_part) {
    __shared__ double red[4];
    const int tid = threadIdx.x, i = blockIdx.x;
    double msum = 0.0;
    for (int b = 0; b < n_mparts; ++b) msum += (double)m_parts[b];      // in block order
    const float cx = (float)(msum / (double)M);
    float *__restrict__ s_row = S + (size_t)i * M;
    const float *__restrict__ p_row = P + (size_t)i * M;
    double pp = 0.0, qq = 0.0;
    for (int k = tid; k < M; k += 256) {
        if (winner[k] != i) continue;
        const float p = p_row[k];
        pp += (double)p;
        qq += (double)p * (double)s_row[k];
    }
    const float Pi = (float)block_sum_d(pp, red);
    const float Qi = (float)block_sum_d(qq, red);
    if (Pi > 0.f) {
        const float coef = 1.f / ((float)M * cx), tau = tau_in[i];
        const float through_min = eta * (Qi - Pi * u_in[i]) / (tau * tau);
        const int kb = kstar[i];
        for (int k = tid; k < M; k += 256) {
            float v = p_row[k] * ((winner[k] == i ? 1.f : 0.f) - Pi) / tau;
            if (k == kb) v += through_min;
            s_row[k] = 0.f - coef * v;
        }
    } else {
        for (int k = tid; k < M; k += 256) s_row[k] = 0.f;      // (a row that owns no column: g = +0 throughout)
    }
    if (tid == 0) {
        row_p[i] = Pi;
        if (kbest_out) kbest_out[i] = kstar[i];
        if (i == 0) e_part[0] = (float)(0.0 - log((double)cx));
    }
}

// ------------------------------------------------------------------------------------------- gradient
// One K slice of q (i, c) = sum_k g_ik B[k][c]; a wave owns a 32 x 32 block of the 64 x 64 tile.
__global__ __launch_bounds__(256) void cx_grad_kernel(const float *__restrict__ G, const float *__restrict__ B,
                                                      const float *__restrict__ row_p, int C, int N, int M,
                                                      int slice_len, int skip, float *__restrict__ qp) {
    __shared__ float At[64 * kLd];
    __shared__ float Bt[64 * kLd];
    __shared__ int any;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int bi = wave >> 1, bj = wave & 1;
    const int i0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int ks = blockIdx.z * slice_len, ke = min(M, ks + slice_len);
    float *__restrict__ out = qp + (size_t)blockIdx.z * N * C;
    if (tid == 0) any = !skip;      // (STX_CX_SKIP=0: every block runs the product)
    __syncthreads();
    if (tid < 64 && i0 + tid < N && row_p[i0 + tid] > 0.f) any = 1;
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (any) {      // (uniform over the workgroup)
        const float *ap = At + (bi * 32 + l31) * kLd + half;
        const float *bp = Bt + (bj * 32 + l31) * kLd + half;
        float ra[8], rb[8];
        const auto load = [&](int k0) {     // g_ik read along k, and the rows B[k] along c
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int e = tid + 256 * p, m = e >> 5, k = e & 31;
                const bool ok = i0 + m < N && k0 + k < ke;
                const float a = G[ok ? (size_t)(i0 + m) * M + k0 + k : 0];
                ra[p] = ok ? a : 0.f;
                const int kb = e >> 6, c = e & 63;
                const bool okb = k0 + kb < ke;
                const float b = B[okb ? (size_t)(k0 + kb) * C + c0 + c : 0];
                rb[p] = okb ? b : 0.f;
            }
        };
        load(ks);
        for (int k0 = ks; k0 < ke; k0 += 32) {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int e = tid + 256 * p;
                At[(e >> 5) * kLd + (e & 31)] = ra[p];
                Bt[(e & 63) * kLd + (e >> 6)] = rb[p];
            }
            __syncthreads();
            if (k0 + 32 < ke) load(k0 + 32);        // (in flight while the MFMAs run)
#pragma unroll
            for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k], bp[k], acc, 0, 0, 0);
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (i < N) out[(size_t)i * C + c0 + bj * 32 + l31] = acc[r] + 0.f;     // (+0 where the sum is -0)
    }
}

// q = the slices' partial tiles added in slice order, left in slice 0, and the tile's share of q_i . x_i: a
// workgroup owns 64 grid positions x 64 channels, a wave one position at a time.
__global__ __launch_bounds__(256) void cx_reduce_kernel(float *__restrict__ qp, int slices, const float *__restrict__ R,
                                                        int C, int N, float *__restrict__ dot_parts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, o0 = blockIdx.y * 64;
    const size_t slice = (size_t)N * C;
    for (int u = 0; u < 16; ++u) {
        const int o = o0 + wave + 4 * u;
        if (o >= N) break;      // (uniform over the wave)
        const size_t at = (size_t)o * C + c;
        float q = qp[at];
#pragma unroll 4
        for (int s = 1; s < slices; ++s) q += qp[(size_t)s * slice + at];
        if (slices > 1) qp[at] = q;
        const float dot = wave_sum_f(q * R[at]);
        if (lane == 0) dot_parts[(size_t)blockIdx.x * N + o] = dot;
    }
}

// S_i = (q_i - (q_i . x_i) x_i) / r_i into the blob's layout, the dot from the channel blocks' shares in block order;
// a workgroup owns 64 grid positions x 64 channels and leaves its partial of sum |S|.
__global__ __launch_bounds__(256) void cx_project_kernel(const float *__restrict__ q, const float *__restrict__ R,
                                                         const float *__restrict__ inv_r,
                                                         const float *__restrict__ dot_parts, int C, int h, int w, int g,
                                                         int gw, int N, float *__restrict__ sgrad,
                                                         float *__restrict__ abs_parts) {
    __shared__ float tile[64][65];
    __shared__ double ared[4][64];
    const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 64, o0 = blockIdx.y * 64, cblocks = gridDim.x;
    const size_t HW = (size_t)h * w;
    for (int u = 0; u < 16; ++u) {      // a wave per position, a lane per channel
        const int row = grp + 4 * u, o = o0 + row;
        float v = 0.f;
        if (o < N) {
            float d = 0.f;
            for (int b = 0; b < cblocks; ++b) d += dot_parts[(size_t)b * N + o];
            const size_t at = (size_t)o * C + c0 + col;
            v = (q[at] - d * R[at]) * inv_r[o];
        }
        tile[col][row] = v;
    }
    __syncthreads();
    const int o = o0 + col;             // a lane per position, a wave per channel
    double sum = 0.0;
    if (o < N) {
        const size_t dst = (size_t)(o / gw) * g * w + (size_t)(o % gw) * g;
        for (int cc = grp; cc < 64; cc += 4) {
            const float v = tile[cc][col];
            sgrad[(size_t)(c0 + cc) * HW + dst] = v;
            sum += (double)fabsf(v);
        }
    }
    ared[grp][col] = sum;
    __syncthreads();
    if (threadIdx.x < 64) {
        const double t = wave_sum_d(((ared[0][col] + ared[1][col]) + ared[2][col]) + ared[3][col]);
        if (threadIdx.x == 0) abs_parts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (float)t;
    }
}

}  // namespace

int cx_rows_launch(hipStream_t s, const float *feat, int C, int h, int w, const SelfsimGrid &gr, float *rows) {
    cx_prepare_kernel<false><<<ceil_div(gr.N, 64), 256, 0, s>>>(feat, C, h, w, gr.g, gr.gw, gr.N, nullptr, rows, nullptr);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int cx_bank_launch(hipStream_t s, const float *raw, int C, int M, float *mu, float *bank) {
    cx_mean_kernel<<<C / 64, 256, 0, s>>>(raw, C, M, mu);
    STX_CHECK_LAUNCH();
    cx_prepare_kernel<true><<<ceil_div(M, 64), 256, 0, s>>>(raw, C, 0, 0, 0, 0, M, mu, bank, nullptr);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int cx_prepare_launch(hipStream_t s, const float *feat, int C, int h, int w, const SelfsimGrid &gr, const float *mu,
                      const CxScratch &x) {
    cx_prepare_kernel<false><<<ceil_div(gr.N, 64), 256, 0, s>>>(feat, C, h, w, gr.g, gr.gw, gr.N, mu, x.rows, x.inv_r);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int cx_score_launch(hipStream_t s, int C, int N, int M, const float *bank, const CxScratch &x) {
    cx_score_kernel<<<dim3(ceil_div(M, 64), ceil_div(N, 64)), 256, 0, s>>>(x.rows, bank, C, N, M, x.S, x.best_val,
                                                                           x.best_idx);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int cx_rows_pass_launch(hipStream_t s, int N, int M, float eta, const CxScratch &x) {
    cx_row_kernel<<<N, 256, 0, s>>>(x.S, x.best_val, x.best_idx, N, M, ceil_div(M, 64), eta, x.P, x.kstar, x.tau, x.u);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int cx_cols_pass_launch(hipStream_t s, int N, int M, float eta, const CxScratch &x, int *kbest_out, int *winner_out) {
    const int nb = ceil_div(N, 64), parts = ceil_div(M, 256);
    cx_col_kernel<<<dim3(ceil_div(M, 64), nb), 256, 0, s>>>(x.P, N, M, x.col_val, x.col_idx);
    STX_CHECK_LAUNCH();
    cx_col_finish_kernel<<<parts, 256, 0, s>>>(x.col_val, x.col_idx, nb, M, x.winner, winner_out, x.m_parts);
    STX_CHECK_LAUNCH();
    cx_weight_kernel<<<N, 256, 0, s>>>(x.S, x.P, x.winner, x.m_parts, parts, x.kstar, x.tau, x.u, M, eta, x.row_p,
                                       kbest_out, x.e_part);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int cx_grad_launch(hipStream_t s, int C, int h, int w, const SelfsimGrid &gr, int M, const float *bank,
                   const CxScratch &x, float *sgrad, int *n_abs) {
    const int nb = ceil_div(gr.N, 64), len = cx_slice_len(C, gr.N, M), slices = ceil_div(M, len);
    if (gr.g > 1) STX_HIP(hipMemsetAsync(sgrad, 0, (size_t)C * h * w * sizeof(float), s));
    const char *env = sw_env("STX_CX_SKIP");        // (0: the row blocks that own no column run the product too)
    const int skip = !(env && env[0] == '0');
    cx_grad_kernel<<<dim3(C / 64, nb, slices), 256, 0, s>>>(x.S, bank, x.row_p, C, gr.N, M, len, skip, x.qp);
    STX_CHECK_LAUNCH();
    cx_reduce_kernel<<<dim3(C / 64, nb), 256, 0, s>>>(x.qp, slices, x.rows, C, gr.N, x.dot_parts);
    STX_CHECK_LAUNCH();
    cx_project_kernel<<<dim3(C / 64, nb), 256, 0, s>>>(x.qp, x.rows, x.inv_r, x.dot_parts, C, h, w, gr.g, gr.gw, gr.N, sgrad,
                                                       x.abs_parts);
    STX_CHECK_LAUNCH();
    *n_abs = nb * (C / 64);
    return STX_OK;
}

}  // namespace stx
