// The sliced Wasserstein style term (Heitz et al., "A Sliced Wasserstein Loss for Neural Texture Synthesis"):
// a tapped blob F [C][n] is projected on D unit directions V [D][C]; every direction's n projections are
// sorted and held, rank by rank, to the direction's target quantile function Tq [D][Q] (include/stx.h,
// stx_set_swd_targets):
//   p[d][i] = v_d . f_i,   g[d][i] = p[d][i] - resample(Tq[d], Q -> n)[rank of i],
//   E = sum g^2 / (D n),   S = V^T g / D.
// The launches, O(D n (C + log^2 n)), no atomics:
//   1. swd_gemm_kernel<false>   P = V F by v_mfma_f32_32x32x2_f32 (64 x 64 outputs per workgroup, float32
//                               accumulation in k order).  Its epilogue writes the SORT RECORDS, not P: one
//                               64-bit word per (direction, pixel) -- the order-preserving image of the float
//                               in the high half, the pixel index in the low half -- and the sentinels
//                               (key ~0, index >= n: they order last) that pad a row to a power of two N.
//   2. the segmented sort       of D rows of N words, ascending as unsigned 64-bit integers: value first,
//                               -0 as +0, equal values by index -- a strict total order, so the result is the
//                               same whatever network sorts it.  A bitonic network: swd_block_kernel sorts
//                               blocks of kSwdBlock = 8192 words (64 KiB, 68 KiB with its bank padding) in LDS; above that size the steps
//                               with a partner distance j >= 8192 run in global memory (swd_merge_global_kernel)
//                               and the steps below it again in LDS.  Everywhere a thread takes up to three
//                               consecutive steps at once, on the eight words they connect, in registers: a
//                               third of the LDS round trips, barriers and global passes.
//   3. the rank pass            is the epilogue of the LAST block launch (the sorted block is in LDS): at rank r
//                               it forms t by the resample rule, scatters g = p - t to G[d][index], writes the
//                               rank when asked and leaves the block's sum of g^2 (scaled by 1 / (D n)) -- one
//                               partial per block, in rank order.
//   4. swd_gemm_kernel<true>    S = V^T G / D with the per-workgroup partials of sum |S|.
// The target of a style picture (stx_swd_target) is launches 1 and 2 with the sorted rows stored, and
// swd_quantiles_kernel, which resamples them n -> Q.

#include <algorithm>

#include "common.h"

namespace stx {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

int swd_padded(int n) {
    int N = 2;
    while (N < n) N <<= 1;
    return N;
}

static int swd_block_of(int N) { return std::min(N, kSwdBlock); }
static size_t swd_round64(size_t v) { return (v + 63) & ~(size_t)63; }

int swd_e_parts(int n, int D) {
    const int N = swd_padded(n);
    return D * (N / swd_block_of(N));
}

int swd_abs_parts(int C, int n) { return ceil_div(C, 64) * ceil_div(n, 64); }

size_t swd_scratch_floats(int C, int n, int D) {
    return swd_round64((size_t)swd_e_parts(n, D)) + swd_round64((size_t)swd_abs_parts(C, n));
}

size_t swd_work_floats(int n, int D) {
    // the sort records (two floats each), then G [D][n]
    return 2 * (size_t)D * swd_padded(n) + swd_round64((size_t)D * n);
}

int swd_check(const char *who, int C, long long n, int D, int Q) {
    if (C <= 0 || n < 1 || D < 1 || Q < 2) {
        set_error("%s: %d channels, %lld pixels, %d directions, %d quantiles (at least one direction and two "
                  "quantiles are expected)", who, C, n, D, Q);
        return STX_ERR_ARG;
    }
    if (C % 4 != 0 || D > kSwdMaxDirs || Q > kSwdMaxQuantiles || n > kSwdMaxPixels ||
        (long long)D * swd_padded((int)n) >= (1ll << 31)) {
        set_error("%s: %d channels, %lld pixels, %d directions, %d quantiles (a channel count that is a multiple of "
                  "4, at most %d directions, %d quantiles and %d pixels, and directions x padded pixels below 2^31 "
                  "are expected)", who, C, n, D, Q, kSwdMaxDirs, kSwdMaxQuantiles, kSwdMaxPixels);
        return STX_ERR_UNSUPPORTED;
    }
    return STX_OK;
}

namespace {

constexpr int kSortThreads = 1024;
constexpr int kLd = 33;         // a 32-float LDS row and one of padding: the 32 lanes of an operand read hit 32 banks

// float -> unsigned, order-preserving; -0 counts as +0
__device__ __forceinline__ unsigned key_of(float p) {
    const unsigned u = __builtin_bit_cast(unsigned, p + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float value_of(unsigned key) {
    return __builtin_bit_cast(float, (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// resample(s[0 .. M-1], M -> K)[k] of include/stx.h; s(j) reads element j
template <class Read>
__device__ __forceinline__ float resample_at(Read s, int M, int K, int k) {
    if (K == M) return s(k);        // (what the rule gives: j = k, a = 0)
    const long long num = (2ll * k + 1) * M - K;
    if (num <= 0) return s(0);
    const long long two_k = 2ll * K;
    // num < 2^40: the double quotient is off by one at most, which the remainder shows
    long long j = (long long)((double)num / (double)two_k);
    long long rem = num - j * two_k;
    if (rem < 0) {
        --j;
        rem += two_k;
    } else if (rem >= two_k) {
        ++j;
        rem -= two_k;
    }
    if (j >= M - 1) return s(M - 1);
    const float a = (float)rem / (float)two_k;
    const float lo = s((int)j);
    return fmaf(a, s((int)j + 1) - lo, lo);
}

// The two matrix products.  GRAD = false: out (m, col) = sum_k A[m][k] B[k][col], A = V [M = D][K = C], written
// as sort records into rows of N words.  GRAD = true: A is read transposed, A[k][m] = V [K = D][M = C],
// B = G [D][ncols]; S = scale * product with the partials of sum |S|.  A wave owns a 32 x 32 block.
template <bool GRAD>
__global__ __launch_bounds__(256) void swd_gemm_kernel(const float *__restrict__ A, const float *__restrict__ B, int M,
                                                       int K, int ncols, u64 *__restrict__ records, int N,
                                                       float *__restrict__ S, float scale,
                                                       float *__restrict__ abs_parts) {
    __shared__ float At[64 * kLd];
    __shared__ float Bt[64 * kLd];
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int bi = wave >> 1, bj = wave & 1;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float *ap = At + (bi * 32 + l31) * kLd + half;
    const float *bp = Bt + (bj * 32 + l31) * kLd + half;
    if (n0 < ncols) {       // (uniform; a workgroup past the last pixel only pads its rows)
        for (int k0 = 0; k0 < K; k0 += 32) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int e = tid + 256 * q;
                int m, k;
                size_t at;
                if (GRAD) {
                    k = e >> 6, m = e & 63;
                    at = (size_t)(k0 + k) * M + m0 + m;
                } else {
                    m = e >> 5, k = e & 31;
                    at = (size_t)(m0 + m) * K + k0 + k;
                }
                const bool ok = m0 + m < M && k0 + k < K;
                const float v = A[ok ? at : 0];
                At[m * kLd + k] = ok ? v : 0.f;
                const int kb = e >> 6, c = e & 63;
                const bool okb = k0 + kb < K && n0 + c < ncols;
                const float b = B[okb ? (size_t)(k0 + kb) * ncols + n0 + c : 0];
                Bt[c * kLd + kb] = okb ? b : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[k], bp[k], acc, 0, 0, 0);
            __syncthreads();
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const int col = n0 + bj * 32 + l31;
        if (GRAD) {
            const float v = acc[r] * scale;
            if (row < M && col < ncols) {
                S[(size_t)row * ncols + col] = v;
                sum += fabsf(v);
            }
        } else if (row < M && col < N) {
            const unsigned key = col < ncols ? key_of(acc[r]) : 0xffffffffu;
            records[(size_t)row * N + col] = ((u64)key << 32) | (unsigned)col;
        }
    }
    if (GRAD) {     // the workgroup's sum in a fixed order: wave shuffles, then the four waves in turn
        sum = wave_sum_f(sum);
        if (lane == 0) red[wave] = sum;
        __syncthreads();
        if (tid == 0) abs_parts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

struct SwdRank {
    const float *Tq;
    int Q;
    float *G;
    int *rank_out;      // or null
    float *e_parts;
    float scale;        // 1 / (D n)
};

// R consecutive steps of the merge of size k -- partner distances j, j / 2, ..., j >> (R - 1) -- on the 2^R words
// that they connect, in registers: group t of the row part at p, whose word 0 is word `base` of the row.  Word i of
// the row is in an ascending sequence of size k when bit k of i is clear; k >= 2 j, so the 2^R words agree on it.
// PAD: p is an LDS block in which record i lives at lds_at(i).
// One spare word per 16 records: the 64 lanes of a round's read or write, which lie 8 h records apart in groups of
// h (h = 2 ... 32 between the block-wide and the thread-local rounds), then spread over all banks -- two lanes per
// 8-byte bank pair, the least there is -- where unpadded they would meet in 8 h / 32 of them.
__device__ __forceinline__ int lds_at(int i) { return i + (i >> 4); }
constexpr int kSwdLdsWords = kSwdBlock + (kSwdBlock >> 4);

template <int R, bool PAD>
__device__ __forceinline__ void bitonic_round(u64 *p, int base, int t, int k, int j) {
    const int h = j >> (R - 1);
    const int i0 = ((t & ~(h - 1)) << R) | (t & (h - 1));
    const bool up = ((base + i0) & k) == 0;
    u64 x[1 << R];
#pragma unroll
    for (int m = 0; m < (1 << R); ++m) x[m] = p[PAD ? lds_at(i0 + m * h) : i0 + m * h];
#pragma unroll
    for (int d = 1 << (R - 1); d > 0; d >>= 1) {
#pragma unroll
        for (int m = 0; m < (1 << R); ++m) {
            if (m & d) continue;
            const u64 a = x[m], b = x[m + d];
            const bool swap = (a > b) == up;
            x[m] = swap ? b : a;
            x[m + d] = swap ? a : b;
        }
    }
#pragma unroll
    for (int m = 0; m < (1 << R); ++m) p[PAD ? lds_at(i0 + m * h) : i0 + m * h] = x[m];
}

// How many steps the next round takes when the partner distance is j and the steps down to distance `least` are
// left: three where there are three.  (The host and the kernels cut a merge into rounds by this one rule.)
__host__ __device__ __forceinline__ int round_steps(int j, int least) {
    int left = 0;
    for (int d = j; d >= least; d >>= 1) ++left;
    return left < 3 ? left : 3;
}

// The bitonic steps of the sequence sizes k_lo .. k_hi that stay inside a block of B words (B = min(N, kSwdBlock)):
// k_lo = 2, k_hi = B sorts the block; k_lo = k_hi = k > B finishes the merge of size k below distance B.  RANK: the
// block is final -- the rank pass reads it from LDS and the records are not written back.
template <bool RANK>
__global__ __launch_bounds__(kSortThreads) void swd_block_kernel(u64 *__restrict__ records, int N, int n, int B, int k_lo,
                                                                 int k_hi, SwdRank rk) {
    __shared__ u64 s[kSwdLdsWords];
    __shared__ float red[kSortThreads / 64];
    const int tid = threadIdx.x, row = blockIdx.y, g0 = blockIdx.x * B;
    u64 *const mine = records + (size_t)row * N + g0;
    for (int t = tid; t < B; t += kSortThreads) s[lds_at(t)] = mine[t];
    __syncthreads();
    for (int k = k_lo; k <= k_hi; k <<= 1) {
        int j = min(k >> 1, B >> 1);
        while (j > 0) {
            const int steps = round_steps(j, 1);        // (uniform)
            if (steps == 3) {
                for (int t = tid; t < (B >> 3); t += kSortThreads) bitonic_round<3, true>(s, g0, t, k, j);
            } else if (steps == 2) {
                for (int t = tid; t < (B >> 2); t += kSortThreads) bitonic_round<2, true>(s, g0, t, k, j);
            } else {
                for (int t = tid; t < (B >> 1); t += kSortThreads) bitonic_round<1, true>(s, g0, t, k, j);
            }
            j >>= steps;
            __syncthreads();
        }
    }
    if (!RANK) {
        for (int t = tid; t < B; t += kSortThreads) mine[t] = s[lds_at(t)];
        return;
    }
    const float *const tq = rk.Tq + (size_t)row * rk.Q;
    float acc = 0.f;
    for (int t = tid; t < B; t += kSortThreads) {
        const int r = g0 + t;
        if (r >= n) break;          // (the sentinels order last)
        const u64 v = s[lds_at(t)];
        const unsigned idx = (unsigned)v;
        if (idx >= (unsigned)n) continue;       // (never: the first n ranks are the row's own words)
        const float g = value_of((unsigned)(v >> 32)) - resample_at([&](int j) { return tq[j]; }, rk.Q, n, r);
        rk.G[(size_t)row * n + idx] = g;
        if (rk.rank_out) rk.rank_out[(size_t)row * n + idx] = r;
        acc += g * g;
    }
    acc = wave_sum_f(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        float sum = red[0];
        for (int w = 1; w < kSortThreads / 64; ++w) sum += red[w];
        rk.e_parts[(size_t)row * gridDim.x + blockIdx.x] = sum * rk.scale;
    }
}

// R steps of the merge of size k from distance j down (all >= kSwdBlock) in one pass over global memory: a thread
// owns the 2^R words that the steps connect.
template <int R>
__global__ __launch_bounds__(256) void swd_merge_global_kernel(u64 *__restrict__ records, int N, int k, int j) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (N >> R)) return;
    bitonic_round<R, false>(records + (size_t)blockIdx.y * N, 0, t, k, j);
}

// out [D][Q] = resample(the sorted projections of a row, n -> Q)
__global__ __launch_bounds__(256) void swd_quantiles_kernel(const u64 *__restrict__ records, int N, int n, int Q,
                                                            float *__restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const u64 *const row = records + (size_t)blockIdx.y * N;
    out[(size_t)blockIdx.y * Q + q] =
        resample_at([&](int j) { return value_of((unsigned)(row[j] >> 32)); }, n, Q, q);
}

}  // namespace

int swd_project_launch(hipStream_t s, const float *feat, int C, int n, const float *V, int D, void *records) {
    const int N = swd_padded(n);
    swd_gemm_kernel<false><<<dim3(ceil_div(N, 64), ceil_div(D, 64)), 256, 0, s>>>(
        V, feat, D, C, n, static_cast<u64 *>(records), N, nullptr, 0.f, nullptr);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

// The launches of the sort but the last; swd_finish_launch is the last.  (The order of the steps is fixed: k, then
// j, descending.)
int swd_sort_launch(hipStream_t s, void *records_, int n, int D) {
    u64 *const records = static_cast<u64 *>(records_);
    const int N = swd_padded(n), B = swd_block_of(N);
    if (B == N) return STX_OK;      // (one block per row: its sort is the last launch)
    const dim3 blocks(N / B, D);
    swd_block_kernel<false><<<blocks, kSortThreads, 0, s>>>(records, N, n, B, 2, B, SwdRank{});
    STX_CHECK_LAUNCH();
    for (long long k = 2ll * B; k <= N; k <<= 1) {
        int j = (int)(k >> 1);
        while (j >= B) {
            const int steps = round_steps(j, B);
            const dim3 grid(ceil_div(N >> steps, 256), D);
            if (steps == 3)
                swd_merge_global_kernel<3><<<grid, 256, 0, s>>>(records, N, (int)k, j);
            else if (steps == 2)
                swd_merge_global_kernel<2><<<grid, 256, 0, s>>>(records, N, (int)k, j);
            else
                swd_merge_global_kernel<1><<<grid, 256, 0, s>>>(records, N, (int)k, j);
            STX_CHECK_LAUNCH();
            j >>= steps;
        }
        if (k == N) break;
        swd_block_kernel<false><<<blocks, kSortThreads, 0, s>>>(records, N, n, B, (int)k, (int)k, SwdRank{});
        STX_CHECK_LAUNCH();
    }
    return STX_OK;
}

int swd_finish_launch(hipStream_t s, void *records_, int n, int D, const float *Tq, int Q, float *G, int *rank_out,
                      float *e_parts) {
    u64 *const records = static_cast<u64 *>(records_);
    const int N = swd_padded(n), B = swd_block_of(N);
    const SwdRank rk{Tq, Q, G, rank_out, e_parts, (float)(1.0 / ((double)D * (double)n))};
    const dim3 blocks(N / B, D);
    const int k_lo = B == N ? 2 : N;
    if (Tq)
        swd_block_kernel<true><<<blocks, kSortThreads, 0, s>>>(records, N, n, B, k_lo, N, rk);
    else
        swd_block_kernel<false><<<blocks, kSortThreads, 0, s>>>(records, N, n, B, k_lo, N, rk);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int swd_sort_passes(int n) {
    const int N = swd_padded(n), B = swd_block_of(N);
    int passes = 1;
    for (long long k = 2ll * B; k <= N; k <<= 1) {
        for (int j = (int)(k >> 1); j >= B; j >>= round_steps(j, B)) ++passes;
        ++passes;
    }
    return passes;
}

int swd_grad_launch(hipStream_t s, const float *V, const float *G, int C, int n, int D, float *sgrad, float *abs_parts,
                    int *n_parts) {
    swd_gemm_kernel<true><<<dim3(ceil_div(n, 64), ceil_div(C, 64)), 256, 0, s>>>(V, G, C, D, n, nullptr, 0, sgrad,
                                                                                 1.f / (float)D, abs_parts);
    STX_CHECK_LAUNCH();
    *n_parts = swd_abs_parts(C, n);
    return STX_OK;
}

int swd_quantiles_launch(hipStream_t s, const void *records, int n, int D, int Q, float *out) {
    swd_quantiles_kernel<<<dim3(ceil_div(Q, 256), D), 256, 0, s>>>(static_cast<const u64 *>(records), swd_padded(n), n,
                                                                   Q, out);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

}  // namespace stx
