// The nearest-neighbour feature matching term (NNFM; ARF, NNST): every column f_i of a tapped blob F [C][n]
// is pulled towards the most similar row of a fixed bank B [M][C] of unit (or zero) rows --
//   r_i = |f_i|,  x_i = f_i / r_i,  j_i = argmax_j x_i . b_j (lowest j among equals),  c_i = x_i . b_{j_i}
//   E   = (2/n) sum_i (1 - c_i)
//   S_i = -(b_{j_i} - c_i x_i) / r_i                                   ( = n d(E/2)/d f_i with j_i held fixed )
// Four launches, no atomics, every sum in a fixed order:
//   1. nnfm_prepare_kernel   one pass over F: r_i in double, 1/r_i as a float, x_i 2^13 as fp16 hi / lo pieces
//                            (f16x2.h) transposed to [n][C].  With a stride and a float32 output it builds a
//                            bank from a feature map instead (stx_nnfm_bank).  nnfm_split_rows_kernel makes the
//                            pieces of a bank that is given as rows.
//   2. nnfm_search_kernel    the n x M x C product fused with its row-wise argmax: the score matrix never
//                            exists in memory.  A workgroup owns kNnfmQ query columns and walks kNnfmB-row
//                            blocks of (its slice of) the bank; both operands' pieces are staged through LDS
//                            kNnfmK channels at a time, the next stage's loads in flight while the current
//                            one multiplies (v_mfma_f32_32x32x16_f16, three products, smallest first).  The
//                            bank is the A operand and the queries the B operand, so a lane's 16 accumulators
//                            are 16 bank rows of ONE query: the running (score, index) is lane-local.
//                            Unit vectors need no tracked maximum: both sides are scaled by 2^13.
//   3. nnfm_merge_kernel     only when the bank was cut into slices (few query blocks): the slices'
//                            (score, index) pairs by the same rule, "greater score, else lower index".
//   4. nnfm_grad_kernel      per column: gathers the float32 row j_i, recomputes c_i with float32 fma in
//                            channel order (NOT the search's score: E and S are functions of (F, B, j)),
//                            writes S in [C][n] layout and leaves the partials of sum (1 - c_i) and sum |S|.
// The 3 x 3 patch form (stx_set_nnfm_patch_targets) is the same term over the 9 C vectors of a pixel's patch.
// There is ONE search, nnfm_search_kernel<PATCH, K>, with two fetchers of the query operand: a row of the [n][C]
// pieces (plain), or 32 channels of p + tap gathered from those pieces with zeros outside the map (patch; 9 C deep,
// no [n][9 C] array is written anywhere).  Staging, products, the order rule, the clamps and the merges exist once.
// K > 1 (stx_set_nnfm_knn_targets): a sorted list of the K best rows per query takes the place of the one winner and
// S pulls towards their mean (the *_k kernels).  Prepare and gradient are different algorithms per form and stay
// separate kernels: nnfm_patch_norms_kernel / nnfm_patch_rows_kernel split the columns under one scale for the blob,
// nnfm_patch_cos_kernel / nnfm_patch_grad_kernel gather the nine patches of a pixel.  The launches choose among them.
// The coverage part (stx_set_nnfm_cover_targets, patch 1): behind those, every bank row looks for ITS best column --
// the same search with the operands exchanged -- and the nnfm_cover_* kernels turn the winners into an inverted
// index (lists in ascending row order) and add every column's rows to S in that order.  Integer atomics only.
// The guided term (stx_set_nnfm_guided_targets, patch 1): the bank is one segment per style picture and a column looks
// into segment s with the weight m_s of that picture's mask map.  nnfm_mask_window_kernel reads the tile's windows of
// the maps and marks the (segment, query block) pairs with a weight above 0, nnfm_search_kernel<false, K, true> searches
// those pairs only, segment by segment (nnfm_merge_seg_kernel behind it when the bank was cut), and
// nnfm_guided_grad_kernel adds m_s S_{i,s} over a column's segments in ascending s.

#include <algorithm>
#include <climits>
#include <type_traits>

#include "common.h"
#include "f16x2.h"

namespace stx {

namespace {

constexpr float kNnfmScale = 8192.f;        // 2^13: |x_i| = |b_j| = 1, so every piece fits fp16 with room
constexpr int kLdsRow = 2 * kNnfmK + 16;    // bytes of a staged row: 64 of data + 16 of padding (conflict-free b128 reads)

// ------------------------------------------------------------------------------------------- prepare
// A workgroup owns 64 output columns: output column o is the pixel (oy stride, ox stride) of the h x w map,
// o = oy ow + ox in raster order.
__global__ __launch_bounds__(256) void nnfm_prepare_kernel(const float *__restrict__ F, int C, int h, int w,
                                                           int stride, int ow, int n_out,
                                                           float *__restrict__ inv_r, _Float16 *__restrict__ hi,
                                                           _Float16 *__restrict__ lo, float *__restrict__ rows_out) {
    __shared__ double red[4][64];
    __shared__ float sinv[64];
    __shared__ float tile[64][65];
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
    const size_t HW = (size_t)h * w;
    const int o = min(blockIdx.x * 64 + col, n_out - 1);        // (columns past the end re-read the last one)
    const size_t src = (size_t)(o / ow) * stride * w + (size_t)(o % ow) * stride;
    double acc = 0.0;
    for (int c = g; c < C; c += 4) {
        const double v = (double)F[(size_t)c * HW + src];
        acc += v * v;
    }
    red[g][col] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        const double ss = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
        const float inv = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f;
        sinv[col] = inv;
        if (inv_r && blockIdx.x * 64 + col < n_out) inv_r[o] = inv;
    }
    for (int c0 = 0; c0 < C; c0 += 64) {
        __syncthreads();        // (sinv is written; the tile of the round before is read)
        for (int cc = g; cc < 64; cc += 4) tile[cc][col] = F[(size_t)(c0 + cc) * HW + src];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int item = threadIdx.x + 256 * u, col2 = item >> 3, oct = item & 7;
            const int o2 = blockIdx.x * 64 + col2;
            if (o2 >= n_out) continue;
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = tile[oct * 8 + j][col2];
            const float inv = sinv[col2];
            const size_t at = (size_t)o2 * C + c0 + oct * 8;
            if (hi) {
                f16x8h ph, pl;
                split2_f16(x, inv * kNnfmScale, ph, pl);
                *reinterpret_cast<f16x8h *>(hi + at) = ph;
                *reinterpret_cast<f16x8h *>(lo + at) = pl;
            }
            if (rows_out) {
#pragma unroll
                for (int j = 0; j < 8; ++j) rows_out[at + j] = x[j] * inv;
            }
        }
    }
}

// The pieces of a bank given as float32 rows [M][C]: eight channels of one row per thread.
__global__ __launch_bounds__(256) void nnfm_split_rows_kernel(const float *__restrict__ bank, size_t octets, int vec,
                                                              _Float16 *__restrict__ hi, _Float16 *__restrict__ lo) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= octets) return;
    float x[8];
    if (vec) {
        const float4 a = reinterpret_cast<const float4 *>(bank)[2 * t], b = reinterpret_cast<const float4 *>(bank)[2 * t + 1];
        x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w, x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = bank[8 * t + j];
    }
    f16x8h ph, pl;
    split2_f16(x, kNnfmScale, ph, pl);
    reinterpret_cast<f16x8h *>(hi)[t] = ph;
    reinterpret_cast<f16x8h *>(lo)[t] = pl;
}

// ------------------------------------------------------------------------------------- patch prepare
// 3 x 3 patches (stx_set_nnfm_patch_targets): pixel p's patch P_p is the 9 C vector of its columns at
// p + tap, tap = (dy, dx) with dy outer, dx inner, (-1, -1) first, zero outside the map.  |P_p|^2 is the box
// sum of the column norms^2, and the search needs no per-patch normalisation (argmax_j P_p . b_j is that of
// P_p / |P_p|), so the columns are split once, [n][C], under ONE power of two for the whole blob: the one that
// puts the largest column norm into (2^12, 2^13].  Every piece fits fp16 and a score stays below 3 2^26.
//
// First launch: the column norms^2 in double (the order of nnfm_prepare_kernel) and each workgroup's largest.
__global__ __launch_bounds__(256) void nnfm_patch_norms_kernel(const float *__restrict__ F, int C, int n,
                                                               double *__restrict__ norm2, double *__restrict__ bmax) {
    __shared__ double red[4][64];
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int p = min(blockIdx.x * 64 + col, n - 1);            // (columns past the end re-read the last one)
    double acc = 0.0;
    for (int c = g; c < C; c += 4) {
        const double v = (double)F[(size_t)c * n + p];
        acc += v * v;
    }
    red[g][col] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        const double ss = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
        if (blockIdx.x * 64 + col < n) norm2[p] = ss;
        double m = ss;          // (a maximum: no order can change it)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
        if (col == 0) bmax[blockIdx.x] = m;
    }
}

// 2^k with max_norm 2^k in (2^12, 2^13] (a zero or denormal blob: the largest power of two, harmless)
__device__ __forceinline__ float patch_scale(double max_norm) {
    const long long bits = __double_as_longlong(max_norm);
    const int e = (int)((bits >> 52) & 0x7ff) - 1023;
    const bool pow2 = (bits & ((1ll << 52) - 1)) == 0;
    return pow2f((pow2 ? 13 : 12) - e);
}

// Second launch, grid (64-column groups, taps).  Output column o is the patch centred at (oy stride, ox stride),
// o = oy ow + ox.  One tap (the tile's blob, stride 1): 1 / |P_o| into inv_R and the pieces of the column itself
// under the common scale into hi / lo [n][C].  Nine taps (a bank): rows_out [n_out][9 C], the unit patches.
__global__ __launch_bounds__(256) void nnfm_patch_rows_kernel(const float *__restrict__ F, int C, int h, int w, int stride,
                                                              int ow, int n_out, const double *__restrict__ norm2,
                                                              const double *__restrict__ bmax, int n_bmax,
                                                              float *__restrict__ inv_R, _Float16 *__restrict__ hi,
                                                              _Float16 *__restrict__ lo, float *__restrict__ rows_out) {
    __shared__ double smax[4];
    __shared__ float sinv[64];
    __shared__ float tile[64][65];
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
    const size_t HW = (size_t)h * w;
    const int o = min(blockIdx.x * 64 + col, n_out - 1);
    const int y = (o / ow) * stride, x = (o % ow) * stride;
    const int tap = gridDim.y == 1 ? 4 : (int)blockIdx.y;
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    const bool inside = (unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w;
    const size_t src = inside ? (size_t)yy * w + xx : 0;
    float scale = 0.f;
    if (hi) {
        double m = 0.0;
        for (int i = threadIdx.x; i < n_bmax; i += 256) m = fmax(m, bmax[i]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
        if (col == 0) smax[g] = m;
        __syncthreads();
        scale = patch_scale(sqrt(fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]))));
    }
    if (threadIdx.x < 64) {
        double ss = 0.0;        // the box sum, taps in order
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ty = y + t / 3 - 1, tx = x + t % 3 - 1;
            if ((unsigned)ty < (unsigned)h && (unsigned)tx < (unsigned)w) ss += norm2[(size_t)ty * w + tx];
        }
        const float inv = ss > 0.0 ? (float)(1.0 / sqrt(ss)) : 0.f;
        sinv[col] = inv;
        if (inv_R && blockIdx.x * 64 + col < n_out) inv_R[o] = inv;
    }
    for (int c0 = 0; c0 < C; c0 += 64) {
        __syncthreads();        // (sinv is written; the tile of the round before is read)
        for (int cc = g; cc < 64; cc += 4) tile[cc][col] = inside ? F[(size_t)(c0 + cc) * HW + src] : 0.f;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int item = threadIdx.x + 256 * u, col2 = item >> 3, oct = item & 7;
            const int o2 = blockIdx.x * 64 + col2;
            if (o2 >= n_out) continue;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = tile[oct * 8 + j][col2];
            if (hi) {
                const size_t at = (size_t)o2 * C + c0 + oct * 8;
                f16x8h ph, pl;
                split2_f16(v, scale, ph, pl);
                *reinterpret_cast<f16x8h *>(hi + at) = ph;
                *reinterpret_cast<f16x8h *>(lo + at) = pl;
            }
            if (rows_out) {
                const float inv = sinv[col2];
                const size_t at = ((size_t)o2 * 9 + tap) * C + c0 + oct * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) rows_out[at + j] = v[j] * inv;
            }
        }
    }
}

// -------------------------------------------------------------------------------------------- search
// "greater score, else lower index": associative and commutative, so no merge order can change the result
__device__ __forceinline__ void take_better(float s, int j, float &best_s, int &best_j) {
    if (s > best_s || (s == best_s && j < best_j)) {
        best_s = s;
        best_j = j;
    }
}

typedef unsigned u32x4n __attribute__((ext_vector_type(4)));

// The queries of a search: n of them, and for the patch form the width of their map.  A struct of one int or of
// two so that each instantiation keeps the kernel-argument layout -- and with it the instruction sequence -- that
// its form had as a kernel of its own (int n / int n, int w in this place); the plain form's w is a constant.
template <bool PATCH>
struct NnfmQueries {
    int n;
    static constexpr int w = 0;
};
template <>
struct NnfmQueries<true> {
    int n, w;
};

// The K best of a query, K > 1 (stx_set_nnfm_knn_targets): a sorted list under the strict total order "greater
// score, else lower index" (indices are distinct).  The candidate is carried down the list and changes places with
// every entry it beats, so the list stays sorted and holds the K best of all that was offered: the top K of a union
// under a strict total order, which no order of offering or merging can change.  Empty places are
// (-inf, INT_MAX): nothing offered loses to them, and they are never offered.
template <int K>
__device__ __forceinline__ void take_k_better(float s, int j, float (&best_s)[K], int (&best_j)[K]) {
    if (!(s > best_s[K - 1] || (s == best_s[K - 1] && j < best_j[K - 1]))) return;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const bool up = s > best_s[r] || (s == best_s[r] && j < best_j[r]);
        const float ts = up ? best_s[r] : s;
        const int tj = up ? best_j[r] : j;
        best_s[r] = up ? s : best_s[r];
        best_j[r] = up ? j : best_j[r];
        s = ts;
        j = tj;
    }
}

// grid (query blocks, slices).  One slice: idx_out [K][n], rank-major, -1 where fewer than K rows exist.
// Several: part_score / part_idx [slices][K][n], empty places as (-inf, INT_MAX).  K = 1 is the plain argmax.
// A bank row has CB channels: C, and the query operand is the row of the [n][C] pieces -- or, PATCH, 9 C
// tap-major, and the query operand is gathered from those pieces of the w-wide map: stage t of a row reads 32
// channels of pixel p + tap(t), found from p's (y, x) -- the right neighbour of a row's last pixel is padding --
// and zeros outside the map.
// SEG (the guided term, stx_set_nnfm_guided_targets): grid (query blocks, slices, segments) -- the same search against
// segment blockIdx.z's rows, with that segment's idx_out [K][n] / part_* [slices][K][n] planes.  A pair (segment,
// query block) in which no column has m_s > 0 returns at once: none of the segment's rows is read.  Slices are sized
// from the largest segment; one past a shorter segment's last block walks nothing and leaves empty places.  The
// plain kernel has no such arguments (an empty struct behind the others) and keeps its instruction sequence.
template <bool SEG>
struct NnfmSegArgs {};
template <>
struct NnfmSegArgs<true> {
    NnfmSegments segs;
    const unsigned char *active;    // [segments][query blocks]
};

template <bool PATCH, int K, bool SEG = false>
__global__ __launch_bounds__(256) void nnfm_search_kernel(const _Float16 *__restrict__ xhi, const _Float16 *__restrict__ xlo,
                                                          const NnfmQueries<PATCH> queries,
                                                          const _Float16 *__restrict__ bhi_all,
                                                          const _Float16 *__restrict__ blo_all, int M_all, int C,
                                                          int b_blocks_all, int blocks_per_slice,
                                                          int *__restrict__ idx_all, float *__restrict__ part_score_all,
                                                          int *__restrict__ part_idx_all, const NnfmSegArgs<SEG> seg) {
    const _Float16 *bhi = bhi_all, *blo = blo_all;
    int M = M_all, b_blocks = b_blocks_all;
    int *idx_out = idx_all, *part_idx = part_idx_all;
    float *part_score = part_score_all;
    if constexpr (SEG) {
        const int s = blockIdx.z;
        if (!seg.active[s * gridDim.x + blockIdx.x]) return;
        M = seg.segs.rows[s];
        b_blocks = (M + kNnfmB - 1) / kNnfmB;
        const size_t first = (size_t)seg.segs.off[s] * C, plane = (size_t)K * queries.n;
        const size_t part = gridDim.y > 1 ? (size_t)s * gridDim.y * plane : 0;      // (one slice: no part_* arrays)
        bhi += first, blo += first;
        idx_out += s * plane, part_score += part, part_idx += part;
    }
    // [X hi | X lo | B hi | B lo][row][kNnfmK halves + padding]; reused for the workgroup's final merge
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * 128 * kLdsRow];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wq = wave & 1, wb = wave >> 1;        // the wave's 64 queries x 64 bank rows of the 128 x 128 block
    const int r = lane & 31, half = lane >> 5;
    const int n = queries.n, w = queries.w;
    const int q0 = blockIdx.x * kNnfmQ;
    const int bb0 = blockIdx.y * blocks_per_slice, bb1 = min(bb0 + blocks_per_slice, b_blocks);
    const int CB = PATCH ? 9 * C : C;       // channels of a bank row
    const int KC = CB / kNnfmK, T = (bb1 - bb0) * KC;

    // what this thread stages: two 16-byte chunks of each of the four arrays
    const _Float16 *const arr[4] = {xhi, xlo, bhi, blo};
    u32x4n pre[4][2];
    [[maybe_unused]] int qy[2], qx[2];      // PATCH: the pixels of this thread's two query rows
    if constexpr (PATCH) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = min(q0 + (int)((threadIdx.x + 256 * u) >> 2), n - 1);     // padding re-reads the last patch
            qy[u] = q / w;
            qx[u] = q - qy[u] * w;
        }
    }
    const auto prefetch = [&](int t) {
        const int bb = bb0 + t / KC, k0 = (t % KC) * kNnfmK;
        [[maybe_unused]] const int tap = k0 / C, c0 = k0 - tap * C;             // PATCH: the stage's neighbour
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int item = threadIdx.x + 256 * u, row = item >> 2, ch = item & 3;
            const size_t j = (size_t)min(bb * kNnfmB + row, M - 1);             // padding re-reads the last row
            if constexpr (PATCH) {
                const int yy = qy[u] + tap / 3 - 1, xx = qx[u] + tap % 3 - 1;
                const bool inside = (unsigned)xx < (unsigned)w && yy >= 0 && (size_t)yy * w + xx < (size_t)n;
                const size_t at = inside ? ((size_t)yy * w + xx) * C + c0 + ch * 8 : 0;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    pre[a][u] = *reinterpret_cast<const u32x4n *>(arr[a] + at);
                    if (!inside) pre[a][u] = u32x4n{0u, 0u, 0u, 0u};
                }
            } else {
                const size_t q = (size_t)min(q0 + row, n - 1);                  // ... and the last query
#pragma unroll
                for (int a = 0; a < 2; ++a) pre[a][u] = *reinterpret_cast<const u32x4n *>(arr[a] + q * C + k0 + ch * 8);
            }
#pragma unroll
            for (int a = 2; a < 4; ++a) pre[a][u] = *reinterpret_cast<const u32x4n *>(arr[a] + j * CB + k0 + ch * 8);
        }
    };
    const auto stage = [&]() {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int item = threadIdx.x + 256 * u, row = item >> 2, ch = item & 3;
#pragma unroll
            for (int a = 0; a < 4; ++a)
                *reinterpret_cast<u32x4n *>(lds + (a * 128 + row) * kLdsRow + ch * 16) = pre[a][u];
        }
    };
    const auto frag = [&](int a, int row, int ks) {
        return *reinterpret_cast<const f16x8h *>(lds + (a * 128 + row) * kLdsRow + ks * 32 + half * 16);
    };

    f32x16h acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][k][v] = 0.f;
    float best_s[2] = {-INFINITY, -INFINITY};
    int best_j[2] = {INT_MAX, INT_MAX};
    [[maybe_unused]] float top_s[2][K];     // K > 1: the sorted lists of this lane's two queries
    [[maybe_unused]] int top_j[2][K];
    if constexpr (K > 1) {
#pragma unroll
        for (int tq = 0; tq < 2; ++tq)
#pragma unroll
            for (int k = 0; k < K; ++k) top_s[tq][k] = -INFINITY, top_j[tq][k] = INT_MAX;
    }

    prefetch(0);
    for (int t = 0; t < T; ++t) {
        __syncthreads();        // every wave has read the stage before
        stage();
        __syncthreads();
        if (t + 1 < T) prefetch(t + 1);
#pragma unroll
        for (int ks = 0; ks < kNnfmK / 16; ++ks) {
            f16x8h a_hi[2], a_lo[2], b_hi[2], b_lo[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                b_hi[i] = frag(0, 64 * wq + 32 * i + r, ks);
                b_lo[i] = frag(1, 64 * wq + 32 * i + r, ks);
                a_hi[i] = frag(2, 64 * wb + 32 * i + r, ks);
                a_lo[i] = frag(3, 64 * wb + 32 * i + r, ks);
            }
#pragma unroll
            for (int tq = 0; tq < 2; ++tq)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb)
                    acc[tq][tb] = mfma_split3(a_hi[tb], a_lo[tb], b_hi[tq], b_lo[tq], acc[tq][tb]);
        }
        if (t % KC == KC - 1) {     // the block's scores are complete: D[row = bank][col = query]
            const int j0 = (bb0 + t / KC) * kNnfmB + 64 * wb + 4 * half;
#pragma unroll
            for (int tq = 0; tq < 2; ++tq)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb) {
                    // K > 1: a tile whose largest score lies below the list's last place offers nothing (padding
                    // repeats a real row's score, so it can only keep a tile from being passed over)
                    if constexpr (K > 1) {
                        float top = acc[tq][tb][0];
#pragma unroll
                        for (int v = 1; v < 16; ++v) top = fmaxf(top, acc[tq][tb][v]);
                        if (top >= top_s[tq][K - 1]) {
#pragma unroll
                            for (int v = 0; v < 16; ++v) {
                                const int j = j0 + 32 * tb + (v & 3) + 8 * (v >> 2);
                                if (j < M) take_k_better<K>(acc[tq][tb][v], j, top_s[tq], top_j[tq]);
                            }
                        }
#pragma unroll
                        for (int v = 0; v < 16; ++v) acc[tq][tb][v] = 0.f;
                        continue;
                    }
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int j = j0 + 32 * tb + (v & 3) + 8 * (v >> 2);
                        if (j < M) take_better(acc[tq][tb][v], j, best_s[tq], best_j[tq]);     // padding never wins
                        acc[tq][tb][v] = 0.f;
                    }
                }
        }
    }
    // a query's four candidates: two lane halves x the two waves that split the bank rows
    __syncthreads();
    if constexpr (K == 1) {
        float *const cand_s = reinterpret_cast<float *>(lds);
        int *const cand_j = reinterpret_cast<int *>(lds + kNnfmQ * 4 * sizeof(float));
#pragma unroll
        for (int tq = 0; tq < 2; ++tq) {
            const int q = 64 * wq + 32 * tq + r;
            cand_s[q * 4 + wb * 2 + half] = best_s[tq];
            cand_j[q * 4 + wb * 2 + half] = best_j[tq];
        }
        __syncthreads();
        if (threadIdx.x < kNnfmQ && q0 + (int)threadIdx.x < n) {
            float s = cand_s[threadIdx.x * 4];
            int j = cand_j[threadIdx.x * 4];
#pragma unroll
            for (int k = 1; k < 4; ++k) take_better(cand_s[threadIdx.x * 4 + k], cand_j[threadIdx.x * 4 + k], s, j);
            if (j == INT_MAX) j = 0;        // (scores that are not numbers: nothing was taken)
            if (gridDim.y == 1) {
                idx_out[q0 + threadIdx.x] = j;
            } else {
                part_score[(size_t)blockIdx.y * n + q0 + threadIdx.x] = s;
                part_idx[(size_t)blockIdx.y * n + q0 + threadIdx.x] = j;
            }
        }
    } else {        // the same four candidate places, K entries each; the best K of the 4 K
        float *const cand_s = reinterpret_cast<float *>(lds);
        int *const cand_j = reinterpret_cast<int *>(lds + kNnfmQ * 4 * K * sizeof(float));
#pragma unroll
        for (int tq = 0; tq < 2; ++tq) {
            const int q = 64 * wq + 32 * tq + r;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                cand_s[(q * 4 + wb * 2 + half) * K + k] = top_s[tq][k];
                cand_j[(q * 4 + wb * 2 + half) * K + k] = top_j[tq][k];
            }
        }
        __syncthreads();
        if (threadIdx.x < kNnfmQ && q0 + (int)threadIdx.x < n) {
            float s[K];
            int j[K];
#pragma unroll
            for (int k = 0; k < K; ++k) s[k] = -INFINITY, j[k] = INT_MAX;
#pragma unroll
            for (int k = 0; k < 4 * K; ++k)
                if (cand_j[threadIdx.x * 4 * K + k] != INT_MAX)
                    take_k_better<K>(cand_s[threadIdx.x * 4 * K + k], cand_j[threadIdx.x * 4 * K + k], s, j);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (gridDim.y == 1) {
                    idx_out[(size_t)k * n + q0 + threadIdx.x] = j[k] == INT_MAX ? -1 : j[k];
                } else {
                    part_score[((size_t)blockIdx.y * K + k) * n + q0 + threadIdx.x] = s[k];
                    part_idx[((size_t)blockIdx.y * K + k) * n + q0 + threadIdx.x] = j[k];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void nnfm_merge_kernel(const float *__restrict__ part_score,
                                                         const int *__restrict__ part_idx, int n, int slices,
                                                         int *__restrict__ idx_out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    float s = part_score[q];
    int j = part_idx[q];
    for (int k = 1; k < slices; ++k) take_better(part_score[(size_t)k * n + q], part_idx[(size_t)k * n + q], s, j);
    idx_out[q] = j;
}

// K > 1: the best K of the slices' K each, part [slices][K][n] -> idx_out [K][n] (-1: fewer than K rows)
template <int K>
__device__ __forceinline__ void merge_k_body(const float *__restrict__ part_score, const int *__restrict__ part_idx,
                                             int n, int slices, int *__restrict__ idx_out, const int q) {
    float s[K];
    int j[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = -INFINITY, j[k] = INT_MAX;
    // eight candidates' loads in flight at a time: a thread's walk is a chain of dependent selects, not of loads
    for (int k0 = 0; k0 < slices * K; k0 += 8) {
        float cs[8];
        int cj[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool there = k0 + u < slices * K;
            const size_t at = (size_t)(there ? k0 + u : 0) * n + q;
            cs[u] = part_score[at];
            cj[u] = there ? part_idx[at] : INT_MAX;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (cj[u] != INT_MAX) take_k_better<K>(cs[u], cj[u], s, j);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) idx_out[(size_t)k * n + q] = j[k] == INT_MAX ? -1 : j[k];
}

template <int K>
__global__ __launch_bounds__(256) void nnfm_merge_k_kernel(const float *__restrict__ part_score,
                                                           const int *__restrict__ part_idx, int n, int slices,
                                                           int *__restrict__ idx_out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    merge_k_body<K>(part_score, part_idx, n, slices, idx_out, q);
}

// The guided term's merge, grid (256-column groups, segments): the same walk over segment blockIdx.y's planes, for
// the pairs that were searched; the others keep the -1 that the window pass left.  (K = 1: a slice that took nothing
// leaves (-inf, 0), which loses to every score a row can have.)
template <int K>
__global__ __launch_bounds__(256) void nnfm_merge_seg_kernel(const float *__restrict__ part_score,
                                                             const int *__restrict__ part_idx, int n, int slices,
                                                             const unsigned char *__restrict__ active, int q_blocks,
                                                             int *__restrict__ idx_out) {
    const int q = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y;
    if (q >= n || !active[seg * q_blocks + q / kNnfmQ]) return;
    const size_t plane = (size_t)K * n;
    merge_k_body<K>(part_score + seg * slices * plane, part_idx + seg * slices * plane, n, slices, idx_out + seg * plane, q);
}

// ---------------------------------------------------------------------------------------------- grad
// One column per lane, one wave per workgroup.  partials [0 .. blocks) = (2/n) sum (1 - c_i),
// [blocks .. 2 blocks) = sum |S| of the workgroup's columns.
__global__ __launch_bounds__(64) void nnfm_grad_kernel(const float *__restrict__ F, int C, int n,
                                                       const float *__restrict__ inv_r, const float *__restrict__ bank,
                                                       int M, int vec, const int *__restrict__ idx, float *__restrict__ S,
                                                       float *__restrict__ partials) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < n;
    const int ii = valid ? i : n - 1;
    const unsigned ju = (unsigned)idx[ii];
    const float *__restrict__ row = bank + (size_t)(ju < (unsigned)M ? ju : 0u) * C;
    const float inv = inv_r[ii];
    const float *__restrict__ f = F + ii;
    float c = 0.f;
    if (vec) {
#pragma unroll 4
        for (int ch = 0; ch < C; ch += 4) {
            const float4 b = *reinterpret_cast<const float4 *>(row + ch);
            c = fmaf(f[(size_t)ch * n] * inv, b.x, c);
            c = fmaf(f[(size_t)(ch + 1) * n] * inv, b.y, c);
            c = fmaf(f[(size_t)(ch + 2) * n] * inv, b.z, c);
            c = fmaf(f[(size_t)(ch + 3) * n] * inv, b.w, c);
        }
    } else {
#pragma unroll 4
        for (int ch = 0; ch < C; ++ch) c = fmaf(f[(size_t)ch * n] * inv, row[ch], c);
    }
    float sum_abs = 0.f;
    if (valid) {
        float *__restrict__ out = S + i;
#pragma unroll 4
        for (int ch = 0; ch < C; ++ch) {
            const float x = f[(size_t)ch * n] * inv;
            const float s = -((row[ch] - c * x) * inv);
            out[(size_t)ch * n] = s;
            sum_abs += fabsf(s);
        }
    }
    const float one_minus = wave_sum_f(valid ? 1.f - c : 0.f);
    sum_abs = wave_sum_f(sum_abs);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = one_minus * (2.f / (float)n);
        partials[gridDim.x + blockIdx.x] = sum_abs;
    }
}

// The K nearest rows (stx_set_nnfm_knn_targets), KK = min(K, M) > 1 of them: idx [K][n], rank-major, and the
// target is their mean, t_i = (b_{j_i1} + ... + b_{j_iKK}) (1 / KK) -- float32, added in rank order, then scaled;
// formed twice, the same way (knn_mean4), since C floats do not fit a lane.  All else as nnfm_grad_kernel.
// (four channels at a time: one 16-byte load per row where the bank allows it -- the same sums either way)
template <int KK>
__device__ __forceinline__ float4 knn_mean4(const float *__restrict__ bank, const unsigned (&at)[KK], int ch, bool vec) {
    float4 t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < KK; ++r) {
        const float *__restrict__ row = bank + at[r] + ch;
        const float4 b = vec ? *reinterpret_cast<const float4 *>(row) : float4{row[0], row[1], row[2], row[3]};
        if (r == 0) {
            t = b;
        } else {
            t.x += b.x, t.y += b.y, t.z += b.z, t.w += b.w;
        }
    }
    constexpr float inv_k = 1.f / (float)KK;
    return float4{t.x * inv_k, t.y * inv_k, t.z * inv_k, t.w * inv_k};
}

template <int KK>
__global__ __launch_bounds__(64) void nnfm_grad_k_kernel(const float *__restrict__ F, int C, int n,
                                                         const float *__restrict__ inv_r, const float *__restrict__ bank,
                                                         int M, int vec, const int *__restrict__ idx,
                                                         float *__restrict__ S, float *__restrict__ partials) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < n;
    const int ii = valid ? i : n - 1;
    unsigned at[KK];        // (rows x C stays below 2^31)
#pragma unroll
    for (int r = 0; r < KK; ++r) {
        const unsigned ju = (unsigned)idx[(size_t)r * n + ii];
        at[r] = (ju < (unsigned)M ? ju : 0u) * (unsigned)C;
    }
    const float inv = inv_r[ii];
    const float *__restrict__ f = F + ii;
    float c = 0.f;
#pragma unroll 2
    for (int ch = 0; ch < C; ch += 4) {
        const float4 t = knn_mean4<KK>(bank, at, ch, vec);
        c = fmaf(f[(size_t)ch * n] * inv, t.x, c);
        c = fmaf(f[(size_t)(ch + 1) * n] * inv, t.y, c);
        c = fmaf(f[(size_t)(ch + 2) * n] * inv, t.z, c);
        c = fmaf(f[(size_t)(ch + 3) * n] * inv, t.w, c);
    }
    float sum_abs = 0.f;
    if (valid) {
        float *__restrict__ out = S + i;
#pragma unroll 2
        for (int ch = 0; ch < C; ch += 4) {
            const float4 t4 = knn_mean4<KK>(bank, at, ch, vec);
            const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float x = f[(size_t)(ch + k) * n] * inv;
                const float s = -((t[k] - c * x) * inv);
                out[(size_t)(ch + k) * n] = s;
                sum_abs += fabsf(s);
            }
        }
    }
    const float one_minus = wave_sum_f(valid ? 1.f - c : 0.f);
    sum_abs = wave_sum_f(sum_abs);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = one_minus * (2.f / (float)n);
        partials[gridDim.x + blockIdx.x] = sum_abs;
    }
}

// ------------------------------------------------------------------------------------------- guided
// The guided term (stx_set_nnfm_guided_targets): the bank is S segments, one per style picture, and m_s(i) in
// [0, 1] is the tile's window of segment s's mask map --
//   E   = (2/n) sum_i sum_s m_s(i) (1 - c_{i,s}),   S_i = sum_s m_s(i) S_{i,s},   a = sum_i sum_s m_s(i) / n
// with c_{i,s}, S_{i,s} the plain term's against segment s alone (the mean of its K best rows).
//
// The window pass, grid (query blocks, segments), one column per thread: m [S][n] read through the window exactly as
// a content map is, the block's activity byte ("some column has m_s > 0": what the search and the merge look at),
// the block's sum of m_s, and -1 into the K index planes of a block that will not be searched.
__global__ __launch_bounds__(kNnfmQ) void nnfm_mask_window_kernel(const float *__restrict__ maps, ContentWindow w, int K,
                                                                   float *__restrict__ m_out,
                                                                   unsigned char *__restrict__ active,
                                                                   float *__restrict__ m_parts, int *__restrict__ idx) {
    __shared__ float red[kNnfmQ / 64];
    const int n = w.fh * w.fw, seg = blockIdx.y;
    const int i = blockIdx.x * kNnfmQ + threadIdx.x;
    float m = 0.f;
    if (i < n) {
        const int y = i / w.fw, x = i - y * w.fw;
        m = maps[(size_t)seg * w.ch * w.cw + content_index(w, 0, y, x)];
        m_out[(size_t)seg * n + i] = m;
    }
    const int any = __syncthreads_or(m > 0.f);
    const float sum = wave_sum_f(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    if (!any && i < n)
        for (int r = 0; r < K; ++r) idx[((size_t)seg * K + r) * n + i] = -1;
    __syncthreads();
    if (threadIdx.x == 0) {
        active[seg * gridDim.x + blockIdx.x] = any ? 1 : 0;
        m_parts[seg * gridDim.x + blockIdx.x] = red[0] + red[1];
    }
}

// a = sum m / n from the blocks' sums, ONE workgroup, double, a fixed order (content_mask_mean_kernel's)
__global__ __launch_bounds__(256) void nnfm_mask_mean_kernel(const float *__restrict__ m_parts, int count, int n,
                                                             float *__restrict__ a_out) {
    __shared__ double red[256];
    double sum = 0.0;
    for (int i = threadIdx.x; i < count; i += 256) sum += (double)m_parts[i];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) a_out[0] = (float)(red[0] / (double)n);
}

// The gradient, nnfm_grad_k_kernel's geometry and arithmetic: a column walks the segments with m_s(i) > 0 in
// ascending s, forms c_{i,s} and S_{i,s} as that kernel does against the segment's rows (idx [S][KK][n], local
// indices; a -1 is never followed: a column with m_s > 0 lies in a searched block, and every index is clamped) and
// adds m_s S_{i,s} to its column of S, which it alone reads and writes.  The first segment of a column writes the
// product itself and the last one leaves sum |S| (the others add +0 to it) and the factor a, so one segment with
// m == 1 gives the plain term's bits.  A column without a segment gets zeros.
template <int KK>
__global__ __launch_bounds__(64) void nnfm_guided_grad_kernel(const float *__restrict__ F, int C, int n,
                                                              const float *__restrict__ inv_r,
                                                              const float *__restrict__ bank, const NnfmSegments segs,
                                                              int vec, const int *__restrict__ idx,
                                                              const float *__restrict__ m,
                                                              const float *__restrict__ a_ptr, float *S,
                                                              float *__restrict__ partials) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < n;
    const int ii = valid ? i : n - 1;
    const float inv = inv_r[ii];
    const float a = a_ptr ? a_ptr[0] : 1.f;
    const float *__restrict__ f = F + ii;
    float *out = S + ii;
    unsigned bits = 0;      // the column's segments
    for (int s = 0; s < segs.count; ++s)
        if (valid && m[(size_t)s * n + ii] > 0.f) bits |= 1u << s;
    const int s_first = bits ? __ffs(bits) - 1 : -1, s_last = bits ? 31 - __clz(bits) : -1;
    float e = 0.f, sum_abs = 0.f;
    for (int s = 0; s < segs.count; ++s) {
        if (!(bits >> s & 1u)) continue;
        const float mv = m[(size_t)s * n + ii];
        const bool first = s == s_first, last = s == s_last;
        unsigned at[KK];        // (rows x C stays below 2^31)
#pragma unroll
        for (int r = 0; r < KK; ++r) {
            const unsigned ju = (unsigned)idx[((size_t)s * KK + r) * n + ii];
            at[r] = ((unsigned)segs.off[s] + (ju < (unsigned)segs.rows[s] ? ju : 0u)) * (unsigned)C;
        }
        float c = 0.f;
#pragma unroll 2
        for (int ch = 0; ch < C; ch += 4) {
            const float4 t = knn_mean4<KK>(bank, at, ch, vec);
            c = fmaf(f[(size_t)ch * n] * inv, t.x, c);
            c = fmaf(f[(size_t)(ch + 1) * n] * inv, t.y, c);
            c = fmaf(f[(size_t)(ch + 2) * n] * inv, t.z, c);
            c = fmaf(f[(size_t)(ch + 3) * n] * inv, t.w, c);
        }
        const float me = mv * (1.f - c);
        e = first ? me : e + me;
        // (two loops, so that a column's first segment -- with hard masks its only one -- reads nothing of S and
        // the loop has no branch inside; a wave whose columns differ in this runs both under their masks)
        const auto add_to_column = [&](auto first_tag) {
#pragma unroll 2
            for (int ch = 0; ch < C; ch += 4) {
                const float4 t4 = knn_mean4<KK>(bank, at, ch, vec);
                const float t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float x = f[(size_t)(ch + k) * n] * inv;
                    const float ms = mv * -((t[k] - c * x) * inv);
                    const float tot = decltype(first_tag)::value ? ms : out[(size_t)(ch + k) * n] + ms;
                    sum_abs += last ? fabsf(tot) : 0.f;
                    out[(size_t)(ch + k) * n] = last ? a * tot : tot;
                }
            }
        };
        if (first)
            add_to_column(std::true_type{});
        else
            add_to_column(std::false_type{});
    }
    if (valid && !bits)
        for (int ch = 0; ch < C; ++ch) out[(size_t)ch * n] = 0.f;
    const float one_minus = wave_sum_f(e);
    sum_abs = wave_sum_f(sum_abs);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = one_minus * (2.f / (float)n);
        partials[gridDim.x + blockIdx.x] = sum_abs;
    }
}

// --------------------------------------------------------------------------------------- patch grad
// First step, one patch per lane: the float32 row j_p and c_p = X_p . b_{j_p}, float32 fma in the order tap,
// then channel (a tap outside the map adds nothing and is skipped), into cos_out [n].
__global__ __launch_bounds__(64) void nnfm_patch_cos_kernel(const float *__restrict__ F, int C, int h, int w,
                                                            const float *__restrict__ inv_R,
                                                            const float *__restrict__ bank, int M,
                                                            const int *__restrict__ idx, float *__restrict__ cos_out) {
    const int n = h * w, i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int y = i / w, x = i - y * w;
    const unsigned ju = (unsigned)idx[i];
    const float *__restrict__ row = bank + (size_t)(ju < (unsigned)M ? ju : 0u) * 9 * C;
    const float inv = inv_R[i];
    float c = 0.f;
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if ((unsigned)yy >= (unsigned)h || (unsigned)xx >= (unsigned)w) continue;
        const float *__restrict__ f = F + (size_t)yy * w + xx;
        const float *__restrict__ b = row + (size_t)t * C;
#pragma unroll 2
        for (int ch = 0; ch < C; ch += 4) {         // (a row starts at a multiple of 16 bytes: C % 64 == 0)
            const float4 b4 = *reinterpret_cast<const float4 *>(b + ch);
            c = fmaf(f[(size_t)ch * n] * inv, b4.x, c);
            c = fmaf(f[(size_t)(ch + 1) * n] * inv, b4.y, c);
            c = fmaf(f[(size_t)(ch + 2) * n] * inv, b4.z, c);
            c = fmaf(f[(size_t)(ch + 3) * n] * inv, b4.w, c);
        }
    }
    cos_out[i] = c;
}

// Second step, one pixel per lane, one wave per workgroup: the gather form
//   S[c][p] = -sum_tap b_{j_q}[tap, c] / R_q  +  F[c][p] sum_tap c_q / R_q^2,   q = p - tap inside the map,
// taps in order.  partials as nnfm_grad_kernel leaves them.
__global__ __launch_bounds__(64) void nnfm_patch_grad_kernel(const float *__restrict__ F, int C, int h, int w,
                                                             const float *__restrict__ inv_R,
                                                             const float *__restrict__ bank, int M,
                                                             const int *__restrict__ idx, const float *__restrict__ cosv,
                                                             float *__restrict__ S, float *__restrict__ partials) {
    const int n = h * w, i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < n;
    const int ii = valid ? i : n - 1;
    const int y = ii / w, x = ii - y * w;
    const float *rows[9];
    float invq[9];
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int qy = y - (t / 3 - 1), qx = x - (t % 3 - 1);
        const bool inside = (unsigned)qy < (unsigned)h && (unsigned)qx < (unsigned)w;
        const int q = inside ? qy * w + qx : ii;
        const unsigned ju = (unsigned)idx[q];
        rows[t] = bank + (size_t)(ju < (unsigned)M ? ju : 0u) * 9 * C + (size_t)t * C;
        invq[t] = inside ? inv_R[q] : 0.f;
        a = fmaf(cosv[q] * invq[t], invq[t], a);
    }
    float sum_abs = 0.f;
    if (valid) {
        const float *__restrict__ f = F + i;
        float *__restrict__ out = S + i;
        for (int ch = 0; ch < C; ch += 4) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float4 b4 = *reinterpret_cast<const float4 *>(rows[t] + ch);
                acc[0] = fmaf(b4.x, invq[t], acc[0]);
                acc[1] = fmaf(b4.y, invq[t], acc[1]);
                acc[2] = fmaf(b4.z, invq[t], acc[2]);
                acc[3] = fmaf(b4.w, invq[t], acc[3]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float s = fmaf(f[(size_t)(ch + k) * n], a, -acc[k]);
                out[(size_t)(ch + k) * n] = s;
                sum_abs += fabsf(s);
            }
        }
    }
    const float one_minus = wave_sum_f(valid ? 1.f - cosv[ii] : 0.f);
    sum_abs = wave_sum_f(sum_abs);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = one_minus * (2.f / (float)n);
        partials[gridDim.x + blockIdx.x] = sum_abs;
    }
}

// The two patch steps for the KK = min(K, M) > 1 nearest rows, idx [K][n]: b_{j_p} becomes the mean t_p of the
// rows (knn_mean4: rank order, then scaled), everything else as above.
template <int KK>
__global__ __launch_bounds__(64) void nnfm_patch_cos_k_kernel(const float *__restrict__ F, int C, int h, int w,
                                                              const float *__restrict__ inv_R,
                                                              const float *__restrict__ bank, int M,
                                                              const int *__restrict__ idx, float *__restrict__ cos_out) {
    const int n = h * w, i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int y = i / w, x = i - y * w;
    unsigned at[KK];        // (rows x 9 C stays below 2^31)
#pragma unroll
    for (int r = 0; r < KK; ++r) {
        const unsigned ju = (unsigned)idx[(size_t)r * n + i];
        at[r] = (ju < (unsigned)M ? ju : 0u) * 9u * (unsigned)C;
    }
    const float inv = inv_R[i];
    float c = 0.f;
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        if ((unsigned)yy >= (unsigned)h || (unsigned)xx >= (unsigned)w) continue;
        const float *__restrict__ f = F + (size_t)yy * w + xx;
#pragma unroll 2
        for (int ch = 0; ch < C; ch += 4) {         // (a row starts at a multiple of 16 bytes: C % 64 == 0)
            const float4 b4 = knn_mean4<KK>(bank, at, t * C + ch, true);
            c = fmaf(f[(size_t)ch * n] * inv, b4.x, c);
            c = fmaf(f[(size_t)(ch + 1) * n] * inv, b4.y, c);
            c = fmaf(f[(size_t)(ch + 2) * n] * inv, b4.z, c);
            c = fmaf(f[(size_t)(ch + 3) * n] * inv, b4.w, c);
        }
    }
    cos_out[i] = c;
}

template <int KK>
__global__ __launch_bounds__(64) void nnfm_patch_grad_k_kernel(const float *__restrict__ F, int C, int h, int w,
                                                               const float *__restrict__ inv_R,
                                                               const float *__restrict__ bank, int M,
                                                               const int *__restrict__ idx,
                                                               const float *__restrict__ cosv, float *__restrict__ S,
                                                               float *__restrict__ partials) {
    const int n = h * w, i = blockIdx.x * 64 + threadIdx.x;
    const bool valid = i < n;
    const int ii = valid ? i : n - 1;
    const int y = ii / w, x = ii - y * w;
    unsigned at[9][KK];     // tap t of the rows of the patch centred at p - tap
    float invq[9];
    float a = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int qy = y - (t / 3 - 1), qx = x - (t % 3 - 1);
        const bool inside = (unsigned)qy < (unsigned)h && (unsigned)qx < (unsigned)w;
        const int q = inside ? qy * w + qx : ii;
#pragma unroll
        for (int r = 0; r < KK; ++r) {
            const unsigned ju = (unsigned)idx[(size_t)r * n + q];
            at[t][r] = ((ju < (unsigned)M ? ju : 0u) * 9u + (unsigned)t) * (unsigned)C;
        }
        invq[t] = inside ? inv_R[q] : 0.f;
        a = fmaf(cosv[q] * invq[t], invq[t], a);
    }
    float sum_abs = 0.f;
    if (valid) {
        const float *__restrict__ f = F + i;
        float *__restrict__ out = S + i;
        for (int ch = 0; ch < C; ch += 4) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float4 b4 = knn_mean4<KK>(bank, at[t], ch, true);
                acc[0] = fmaf(b4.x, invq[t], acc[0]);
                acc[1] = fmaf(b4.y, invq[t], acc[1]);
                acc[2] = fmaf(b4.z, invq[t], acc[2]);
                acc[3] = fmaf(b4.w, invq[t], acc[3]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float s = fmaf(f[(size_t)(ch + k) * n], a, -acc[k]);
                out[(size_t)(ch + k) * n] = s;
                sum_abs += fabsf(s);
            }
        }
    }
    const float one_minus = wave_sum_f(valid ? 1.f - cosv[ii] : 0.f);
    sum_abs = wave_sum_f(sum_abs);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = one_minus * (2.f / (float)n);
        partials[gridDim.x + blockIdx.x] = sum_abs;
    }
}

// -------------------------------------------------------------------------------------------- cover
// The coverage part (stx_set_nnfm_cover_targets; STROTSS's other half): every bank row j looks for its best
// column, i*_j = argmax_i x_i . b_j (nnfm_search_kernel<false, 1> with the operands exchanged), and pulls it
// towards itself --
//   c'_j = x_{i*_j} . b_j,   E_cov = (2/M) sum_j (1 - c'_j),   S_cov,i = -(n/M) sum_{j : i*_j = i} (b_j - c'_j x_i) / r_i
// a scatter from M rows into the columns that won them, done as a gather over an inverted index: no float atomics.
//
// First step, one bank row per lane, one wave per workgroup: c'_j with float32 fma in channel order, the row count
// of the winning column (an integer atomic: a count does not depend on the order of its additions) and the
// partials of E_cov -- alone in e_cov_parts and, times the factor, in e_parts, where they follow E_fwd's.
__global__ __launch_bounds__(64) void nnfm_cover_cos_kernel(const float *__restrict__ F, int C, int n,
                                                            const float *__restrict__ inv_r,
                                                            const float *__restrict__ bank, int M, int vec,
                                                            const int *__restrict__ winner, float cover,
                                                            float *__restrict__ cprime, int *__restrict__ counts,
                                                            float *__restrict__ e_parts, float *__restrict__ e_cov_parts) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    const bool valid = j < M;
    const int jj = valid ? j : M - 1;
    const unsigned iu = (unsigned)winner[jj];
    const int i = iu < (unsigned)n ? (int)iu : 0;
    const float *__restrict__ row = bank + (size_t)jj * C;
    const float inv = inv_r[i];
    const float *__restrict__ f = F + i;
    float c = 0.f;
    if (vec) {
#pragma unroll 4
        for (int ch = 0; ch < C; ch += 4) {
            const float4 b = *reinterpret_cast<const float4 *>(row + ch);
            c = fmaf(f[(size_t)ch * n] * inv, b.x, c);
            c = fmaf(f[(size_t)(ch + 1) * n] * inv, b.y, c);
            c = fmaf(f[(size_t)(ch + 2) * n] * inv, b.z, c);
            c = fmaf(f[(size_t)(ch + 3) * n] * inv, b.w, c);
        }
    } else {
#pragma unroll 4
        for (int ch = 0; ch < C; ++ch) c = fmaf(f[(size_t)ch * n] * inv, row[ch], c);
    }
    if (valid) {
        cprime[j] = c;
        atomicAdd(counts + i, 1);
    }
    const float one_minus = wave_sum_f(valid ? 1.f - c : 0.f);
    if (threadIdx.x == 0) {
        const float e = one_minus * (2.f / (float)M);
        e_cov_parts[blockIdx.x] = e;
        e_parts[blockIdx.x] = cover * e;
    }
}

// Second step, ONE workgroup: offsets = the exclusive prefix sums of the counts, 1024 columns per round; the counts
// become each column's fill cursor (its first place).  Integers: no order can change a sum.
__global__ __launch_bounds__(256) void nnfm_cover_offsets_kernel(int *__restrict__ counts, int n,
                                                                 int *__restrict__ offsets) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int at = base + 4 * (int)threadIdx.x;
        int v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = at + u < n ? counts[at + u] : 0;
        const int t = (v[0] + v[1]) + (v[2] + v[3]);
        int inc = t;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(inc, off, 64);
            if (lane >= off) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < wave) before += wsum[k];
            total += wsum[k];
        }
        int ex = carry + before + inc - t;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (at + u < n) {
                offsets[at + u] = ex;
                counts[at + u] = ex;
            }
            ex += v[u];
        }
        carry += total;
        __syncthreads();        // (wsum is read; the next round writes it)
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}

// Third step: every row takes a place of its column's through the cursor.  WHICH place depends on the order the
// atomics retire in, so this list is only the set of a column's rows ...
__global__ __launch_bounds__(256) void nnfm_cover_fill_kernel(const int *__restrict__ winner, int M, int n,
                                                              int *__restrict__ cursor, int *__restrict__ unordered) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const unsigned iu = (unsigned)winner[j];
    const int p = atomicAdd(cursor + (iu < (unsigned)n ? (int)iu : 0), 1);
    if ((unsigned)p < (unsigned)M) unordered[p] = j;
}

// ... and the fourth puts it in order: row j's place is the number of rows of its column that are below j (rows are
// distinct), a function of the set alone.  list[offsets[i] ...) is then ascending in j whatever the third step did.
// A row walks its column's whole list: sum of squared list lengths comparisons, M^2 when one column owns every row.
__global__ __launch_bounds__(256) void nnfm_cover_order_kernel(const int *__restrict__ winner, int M, int n,
                                                               const int *__restrict__ offsets,
                                                               const int *__restrict__ unordered, int *__restrict__ list) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const unsigned iu = (unsigned)winner[j];
    const int i = iu < (unsigned)n ? (int)iu : 0;
    const int beg = offsets[i], end = min(offsets[i + 1], M);
    int rank = 0;
    for (int p = beg; p < end; ++p) rank += unordered[p] < j ? 1 : 0;
    if ((unsigned)(beg + rank) < (unsigned)M) list[beg + rank] = j;
}

// The gradient, grid (64-column groups, 64-channel groups), four waves.  A wave owns 16 of the group's columns, one
// after the other, and its lanes are the 64 channels: it walks the column's list in order and a lane adds
// b_j[ch] - c'_j x_i[ch] row by row -- 256 contiguous bytes of a bank row per step, and the order of a column's sum
// is the list's, whatever the grid.  The sums go through LDS so that S is read and written along i, like
// nnfm_grad_kernel: S = S_fwd + cover S_cov in place.  A long list is one wave's work per channel group: M steps of
// C / 64 waves when one column owns every row.
// abs_parts [channel group][column group] = sum |S|; the channel group 0 moves E_fwd's partial into e_parts.
__global__ __launch_bounds__(256) void nnfm_cover_grad_kernel(const float *__restrict__ F, int C, int n,
                                                              const float *__restrict__ inv_r,
                                                              const float *__restrict__ bank, int M,
                                                              const int *__restrict__ offsets,
                                                              const int *__restrict__ list,
                                                              const float *__restrict__ cprime, float cover, float *S,
                                                              const float *__restrict__ fwd_parts,
                                                              float *__restrict__ e_parts, float *__restrict__ abs_parts) {
    __shared__ float tile[64][65];
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int icol = min(i0 + lane, n - 1);         // (columns past the end re-read the last one)
    for (int cc = wave; cc < 64; cc += 4) tile[cc][lane] = F[(size_t)(c0 + cc) * n + icol];
    __syncthreads();
    const float n_over_m = (float)n / (float)M;
    const float *__restrict__ bch = bank + c0 + lane;
    for (int u = 0; u < 16; ++u) {
        const int col = wave * 16 + u, i = i0 + col;
        float out = 0.f;
        if (i < n) {
            const float inv = inv_r[i];
            const float x = tile[lane][col] * inv;
            const int beg = offsets[i], end = min(offsets[i + 1], M);
            float acc = 0.f;
#pragma unroll 4
            for (int p = beg; p < end; ++p) {
                const unsigned ju = (unsigned)list[p];
                const size_t j = ju < (unsigned)M ? ju : 0u;
                acc += bch[j * C] - cprime[j] * x;
            }
            out = -((n_over_m * acc) * inv);
        }
        tile[lane][col] = out;      // (the place this lane alone has read)
    }
    __syncthreads();
    float sum_abs = 0.f;
    if (i0 + lane < n) {
        for (int cc = wave; cc < 64; cc += 4) {
            const size_t at = (size_t)(c0 + cc) * n + i0 + lane;
            const float s = S[at] + cover * tile[cc][lane];
            S[at] = s;
            sum_abs += fabsf(s);
        }
    }
    sum_abs = wave_sum_f(sum_abs);
    if (lane == 0) red[wave] = sum_abs;
    __syncthreads();
    if (threadIdx.x == 0) {
        abs_parts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
        if (blockIdx.y == 0) e_parts[blockIdx.x] = fwd_parts[blockIdx.x];
    }
}

// n columns of C channels against M bank rows of patch x patch x C
int check_shape(const char *who, int C, long long n, long long M, int patch) {
    const char *const what = patch == 3 ? "patches" : "columns";
    if ((patch != 1 && patch != 3) || C <= 0 || n <= 0 || M <= 0) {
        set_error("%s: patch %d, %d channels, %lld %s, %lld bank rows", who, patch, C, n, what, M);
        return STX_ERR_ARG;
    }
    if (C % 64 != 0) {
        set_error("%s: the channel count %d is not a multiple of 64", who, C);
        return STX_ERR_UNSUPPORTED;
    }
    const long long width = (long long)patch * patch * C;
    if (n >= (1ll << 31) / C || M >= (1ll << 31) / width) {
        set_error("%s: %lld %s against %lld bank rows of %lld channels exceed 32-bit offsets", who, n, what, M, width);
        return STX_ERR_UNSUPPORTED;
    }
    return STX_OK;
}

size_t round64(size_t floats) { return (floats + 63) & ~(size_t)63; }

}  // namespace

NnfmPlan nnfm_plan(int n, int M) {
    NnfmPlan p;
    p.q_blocks = ceil_div(n, kNnfmQ);
    p.b_blocks = ceil_div(M, kNnfmB);
    // few query blocks (a small tile's deep layers): cut the bank across workgroups, about two per CU
    int slices = 1;
    if (p.q_blocks < 256) slices = std::min(p.b_blocks, std::min(kNnfmMaxSlices, ceil_div(512, p.q_blocks)));
    p.blocks_per_slice = ceil_div(p.b_blocks, slices);
    p.slices = ceil_div(p.b_blocks, p.blocks_per_slice);
    return p;
}

size_t nnfm_pieces_floats(int rows, int C) { return round64((size_t)rows * C); }

size_t nnfm_patch_work_floats(int n) { return 2 * round64(n) + 2 * round64(ceil_div(n, 64)); }

namespace {

// the floats of NnfmCover, in its order
size_t cover_floats(int C, int n, int M) {
    const NnfmPlan r = nnfm_plan(M, n);
    const size_t nb = ceil_div(n, 64), mb = ceil_div(M, 64);
    return 4 * round64(M) + (r.slices > 1 ? 2 * round64((size_t)r.slices * M) : 0) + round64(n) +
           round64((size_t)n + 1) + round64(nb + mb) + round64(mb) + round64((size_t)(C / 64) * nb);
}

}  // namespace

size_t nnfm_scratch_floats(int C, int n, int M, int patch, int k, bool cover) {
    const NnfmPlan p = nnfm_plan(n, M);
    return 64 + nnfm_pieces_floats(n, C) + round64(n) + round64((size_t)k * n) +
           (p.slices > 1 ? 2 * round64((size_t)p.slices * k * n) : 0) +
           round64(2 * (size_t)ceil_div(n, 64)) + (patch == 3 ? nnfm_patch_work_floats(n) + round64(n) : 0) +
           (cover ? cover_floats(C, n, M) : 0);
}

NnfmScratch nnfm_carve(float *scratch, int C, int n, int M, int patch, int k, bool cover) {
    const NnfmPlan p = nnfm_plan(n, M);
    NnfmScratch s;
    float *at = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~(uintptr_t)255);
    s.xhi = reinterpret_cast<unsigned short *>(at);
    s.xlo = s.xhi + (size_t)n * C;
    at += nnfm_pieces_floats(n, C);
    s.inv_r = at;
    at += round64(n);
    s.idx = reinterpret_cast<int *>(at);
    at += round64((size_t)k * n);
    s.part_score = nullptr;
    s.part_idx = nullptr;
    if (p.slices > 1) {
        s.part_score = at;
        at += round64((size_t)p.slices * k * n);
        s.part_idx = reinterpret_cast<int *>(at);
        at += round64((size_t)p.slices * k * n);
    }
    s.partials = at;
    at += round64(2 * (size_t)ceil_div(n, 64));
    s.work = nullptr;
    s.cosv = nullptr;
    if (patch == 3) {
        s.work = reinterpret_cast<double *>(at);
        at += nnfm_patch_work_floats(n);
        s.cosv = at;
        at += round64(n);
    }
    if (cover) {        // behind everything else: the layout without it does not move
        const NnfmPlan r = nnfm_plan(M, n);
        const size_t nb = ceil_div(n, 64), mb = ceil_div(M, 64);
        NnfmCover &c = s.cov;
        c.winner = reinterpret_cast<int *>(at);
        at += round64(M);
        if (r.slices > 1) {
            c.part_score = at;
            at += round64((size_t)r.slices * M);
            c.part_idx = reinterpret_cast<int *>(at);
            at += round64((size_t)r.slices * M);
        }
        c.cursor = reinterpret_cast<int *>(at);
        at += round64(n);
        c.offsets = reinterpret_cast<int *>(at);
        at += round64((size_t)n + 1);
        c.unordered = reinterpret_cast<int *>(at);
        at += round64(M);
        c.list = reinterpret_cast<int *>(at);
        at += round64(M);
        c.cprime = at;
        at += round64(M);
        c.e_parts = at;
        at += round64(nb + mb);
        c.e_cov_parts = at;
        at += round64(mb);
        c.abs_parts = at;
    }
    return s;
}

int nnfm_prepare_launch(hipStream_t s, const float *feat, int C, int h, int w, int patch, int stride, double *work,
                        float *inv_r, unsigned short *hi, unsigned short *lo, float *rows_out) {
    const bool p3 = patch == 3;
    if (stride < 1 || h <= 0 || w <= 0 || (p3 && ((rows_out && hi) || (hi && stride != 1)))) {
        set_error("nnfm_prepare_launch: a %dx%d map with stride %d", h, w, stride);
        return STX_ERR_ARG;
    }
    const int oh = ceil_div(h, stride), ow = ceil_div(w, stride);
    STX_TRY(check_shape("nnfm_prepare_launch", C, (long long)h * w, (long long)oh * ow, patch));
    const int n = h * w, n_out = oh * ow;
    _Float16 *const phi = reinterpret_cast<_Float16 *>(hi), *const plo = reinterpret_cast<_Float16 *>(lo);
    if (p3) {
        const int blocks = ceil_div(n, 64);
        double *const norm2 = work, *const bmax = work + round64(n);
        nnfm_patch_norms_kernel<<<blocks, 256, 0, s>>>(feat, C, n, norm2, bmax);
        STX_CHECK_LAUNCH();
        nnfm_patch_rows_kernel<<<dim3(ceil_div(n_out, 64), rows_out ? 9 : 1), 256, 0, s>>>(
            feat, C, h, w, stride, ow, n_out, norm2, bmax, blocks, inv_r, phi, plo, rows_out);
    } else {
        nnfm_prepare_kernel<<<ceil_div(n_out, 64), 256, 0, s>>>(feat, C, h, w, stride, ow, n_out, inv_r, phi, plo,
                                                               rows_out);
    }
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int nnfm_split_rows_launch(hipStream_t s, const float *bank, int M, int C, unsigned short *hi, unsigned short *lo) {
    STX_TRY(check_shape("nnfm_split_rows_launch", C, 1, M, 1));
    const size_t octets = (size_t)M * C / 8;
    const int vec = reinterpret_cast<uintptr_t>(bank) % 16 == 0;
    nnfm_split_rows_kernel<<<(unsigned)((octets + 255) / 256), 256, 0, s>>>(bank, octets, vec,
                                                                            reinterpret_cast<_Float16 *>(hi),
                                                                            reinterpret_cast<_Float16 *>(lo));
    STX_CHECK_LAUNCH();
    return STX_OK;
}

namespace {

template <bool PATCH, int K>
void search_k_launch(hipStream_t s, const dim3 grid, const NnfmScratch &x, int n, int w, const _Float16 *bhi,
                     const _Float16 *blo, int M, int C, const NnfmPlan &p, int *idx_out) {
    const _Float16 *const xhi = reinterpret_cast<const _Float16 *>(x.xhi);
    const _Float16 *const xlo = reinterpret_cast<const _Float16 *>(x.xlo);
    NnfmQueries<PATCH> queries;
    queries.n = n;
    if constexpr (PATCH) queries.w = w;
    nnfm_search_kernel<PATCH, K><<<grid, 256, 0, s>>>(xhi, xlo, queries, bhi, blo, M, C, p.b_blocks, p.blocks_per_slice,
                                                      idx_out, x.part_score, x.part_idx, NnfmSegArgs<false>{});
    if (p.slices > 1 && hipPeekAtLastError() == hipSuccess)
        nnfm_merge_k_kernel<K><<<ceil_div(n, 256), 256, 0, s>>>(x.part_score, x.part_idx, n, p.slices, idx_out);
}

template <int KK>
void grad_k_launch(hipStream_t s, int blocks, const float *feat, int C, int h, int w, int patch, const NnfmScratch &x,
                   const float *bank, int M, const int *idx, float *sgrad) {
    if (patch == 3) {
        nnfm_patch_cos_k_kernel<KK><<<blocks, 64, 0, s>>>(feat, C, h, w, x.inv_r, bank, M, idx, x.cosv);
        if (hipPeekAtLastError() != hipSuccess) return;
        nnfm_patch_grad_k_kernel<KK><<<blocks, 64, 0, s>>>(feat, C, h, w, x.inv_r, bank, M, idx, x.cosv, sgrad,
                                                           x.partials);
    } else {
        const int vec = reinterpret_cast<uintptr_t>(bank) % 16 == 0;
        nnfm_grad_k_kernel<KK><<<blocks, 64, 0, s>>>(feat, C, h * w, x.inv_r, bank, M, vec, idx, sgrad, x.partials);
    }
}

int check_k(const char *who, int k) {
    if (k >= 1 && k <= kNnfmMaxK) return STX_OK;
    set_error("%s: k %d (1 to %d is expected)", who, k, kNnfmMaxK);
    return STX_ERR_ARG;
}

}  // namespace

int nnfm_search_launch(hipStream_t s, const NnfmScratch &x, int h, int w, int patch, const unsigned short *pieces,
                       int M, int C, int *idx_out, int k) {
    const int n = h * w;
    STX_TRY(check_shape("nnfm_search_launch", C, n, M, patch));
    STX_TRY(check_k("nnfm_search_launch", k));
    const NnfmPlan p = nnfm_plan(n, M);
    const dim3 grid(p.q_blocks, p.slices);
    const _Float16 *const xhi = reinterpret_cast<const _Float16 *>(x.xhi);
    const _Float16 *const xlo = reinterpret_cast<const _Float16 *>(x.xlo);
    const _Float16 *const bhi = reinterpret_cast<const _Float16 *>(pieces), *const blo = bhi + (size_t)M * patch * patch * C;
    if (k > 1) {        // the K best rows: idx_out [k][n]
        const bool p3 = patch == 3;
        if (k == 2)
            p3 ? search_k_launch<true, 2>(s, grid, x, n, w, bhi, blo, M, C, p, idx_out)
               : search_k_launch<false, 2>(s, grid, x, n, w, bhi, blo, M, C, p, idx_out);
        else if (k == 3)
            p3 ? search_k_launch<true, 3>(s, grid, x, n, w, bhi, blo, M, C, p, idx_out)
               : search_k_launch<false, 3>(s, grid, x, n, w, bhi, blo, M, C, p, idx_out);
        else
            p3 ? search_k_launch<true, 4>(s, grid, x, n, w, bhi, blo, M, C, p, idx_out)
               : search_k_launch<false, 4>(s, grid, x, n, w, bhi, blo, M, C, p, idx_out);
        STX_CHECK_LAUNCH();
        return STX_OK;
    }
    if (patch == 3)
        nnfm_search_kernel<true, 1><<<grid, 256, 0, s>>>(xhi, xlo, NnfmQueries<true>{n, w}, bhi, blo, M, C, p.b_blocks,
                                                         p.blocks_per_slice, idx_out, x.part_score, x.part_idx,
                                                         NnfmSegArgs<false>{});
    else
        nnfm_search_kernel<false, 1><<<grid, 256, 0, s>>>(xhi, xlo, NnfmQueries<false>{n}, bhi, blo, M, C, p.b_blocks,
                                                          p.blocks_per_slice, idx_out, x.part_score, x.part_idx,
                                                         NnfmSegArgs<false>{});
    STX_CHECK_LAUNCH();
    if (p.slices > 1) {
        nnfm_merge_kernel<<<ceil_div(n, 256), 256, 0, s>>>(x.part_score, x.part_idx, n, p.slices, idx_out);
        STX_CHECK_LAUNCH();
    }
    return STX_OK;
}

int nnfm_grad_launch(hipStream_t s, const float *feat, int C, int h, int w, int patch, const NnfmScratch &x,
                     const float *bank, int M, const int *idx, float *sgrad, int *n_parts, int k) {
    const int n = h * w, blocks = ceil_div(n, 64);
    STX_TRY(check_shape("nnfm_grad_launch", C, n, M, patch));
    STX_TRY(check_k("nnfm_grad_launch", k));
    const int vec = reinterpret_cast<uintptr_t>(bank) % 16 == 0;
    if (patch == 3 && !vec) {
        set_error("nnfm_grad_launch: the bank is not aligned to 16 bytes");
        return STX_ERR_UNSUPPORTED;
    }
    const int kk = std::min(k, M);      // the rows there are; one row: the first index plane and today's kernels
    if (kk == 2) {
        grad_k_launch<2>(s, blocks, feat, C, h, w, patch, x, bank, M, idx, sgrad);
    } else if (kk == 3) {
        grad_k_launch<3>(s, blocks, feat, C, h, w, patch, x, bank, M, idx, sgrad);
    } else if (kk == 4) {
        grad_k_launch<4>(s, blocks, feat, C, h, w, patch, x, bank, M, idx, sgrad);
    } else if (patch == 3) {
        nnfm_patch_cos_kernel<<<blocks, 64, 0, s>>>(feat, C, h, w, x.inv_r, bank, M, idx, x.cosv);
        STX_CHECK_LAUNCH();
        nnfm_patch_grad_kernel<<<blocks, 64, 0, s>>>(feat, C, h, w, x.inv_r, bank, M, idx, x.cosv, sgrad, x.partials);
    } else {
        nnfm_grad_kernel<<<blocks, 64, 0, s>>>(feat, C, n, x.inv_r, bank, M, vec, idx, sgrad, x.partials);
    }
    STX_CHECK_LAUNCH();
    *n_parts = blocks;
    return STX_OK;
}

int nnfm_cover_search_launch(hipStream_t s, const NnfmScratch &x, int n, const unsigned short *pieces, int M, int C,
                             int *winner_out) {
    if (!x.cov.winner) {
        set_error("nnfm_cover_search_launch: a scratch without the coverage part");
        return STX_ERR_ARG;
    }
    // the roles exchanged: the bank's pieces are M queries (a map M x 1), and x's pieces, [n][C] hi with lo right
    // behind them, are a bank of n rows
    NnfmScratch r{};
    r.xhi = const_cast<unsigned short *>(pieces);
    r.xlo = r.xhi + (size_t)M * C;
    r.part_score = x.cov.part_score;
    r.part_idx = x.cov.part_idx;
    return nnfm_search_launch(s, r, M, 1, 1, x.xhi, n, C, winner_out, 1);
}

int nnfm_cover_index_launch(hipStream_t s, const float *feat, int C, int n, const NnfmScratch &x, const float *bank,
                            int M, const int *winner, float cover) {
    STX_TRY(check_shape("nnfm_cover_index_launch", C, n, M, 1));
    const NnfmCover &c = x.cov;
    const int vec = reinterpret_cast<uintptr_t>(bank) % 16 == 0;
    STX_HIP(hipMemsetAsync(c.cursor, 0, (size_t)n * sizeof(int), s));
    nnfm_cover_cos_kernel<<<ceil_div(M, 64), 64, 0, s>>>(feat, C, n, x.inv_r, bank, M, vec, winner, cover, c.cprime,
                                                         c.cursor, c.e_parts + ceil_div(n, 64), c.e_cov_parts);
    STX_CHECK_LAUNCH();
    nnfm_cover_offsets_kernel<<<1, 256, 0, s>>>(c.cursor, n, c.offsets);
    STX_CHECK_LAUNCH();
    nnfm_cover_fill_kernel<<<ceil_div(M, 256), 256, 0, s>>>(winner, M, n, c.cursor, c.unordered);
    STX_CHECK_LAUNCH();
    nnfm_cover_order_kernel<<<ceil_div(M, 256), 256, 0, s>>>(winner, M, n, c.offsets, c.unordered, c.list);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int nnfm_cover_grad_launch(hipStream_t s, const float *feat, int C, int n, const NnfmScratch &x, const float *bank,
                           int M, float cover, float *sgrad, int *n_e, int *n_abs) {
    STX_TRY(check_shape("nnfm_cover_grad_launch", C, n, M, 1));
    const NnfmCover &c = x.cov;
    const int nb = ceil_div(n, 64);
    nnfm_cover_grad_kernel<<<dim3(nb, C / 64), 256, 0, s>>>(feat, C, n, x.inv_r, bank, M, c.offsets, c.list, c.cprime,
                                                            cover, sgrad, x.partials, c.e_parts, c.abs_parts);
    STX_CHECK_LAUNCH();
    *n_e = nb + ceil_div(M, 64);
    *n_abs = (C / 64) * nb;
    return STX_OK;
}

// ------------------------------------------------------------------------------------------- guided
NnfmSegments nnfm_segments(const int *seg_rows, int count) {
    NnfmSegments segs{};
    segs.count = std::max(0, std::min(count, kNnfmMaxSegments));
    long long off = 0;
    for (int s = 0; s < segs.count; ++s) {
        segs.off[s] = (int)std::min<long long>(off, INT_MAX);
        segs.rows[s] = seg_rows[s];
        off += std::max(seg_rows[s], 0);
    }
    return segs;
}

namespace {

int check_guided(const char *who, int C, long long n, const NnfmSegments &segs, int k) {
    STX_TRY(check_k(who, k));
    long long total = 0;
    for (int s = 0; s < segs.count; ++s) {
        if (segs.rows[s] < k) {
            set_error("%s: segment %d has %d rows, fewer than k = %d", who, s, segs.rows[s], k);
            return STX_ERR_ARG;
        }
        total += segs.rows[s];
    }
    if (segs.count < 1) {
        set_error("%s: no segments", who);
        return STX_ERR_ARG;
    }
    return check_shape(who, C, n, total, 1);
}

// the floats of NnfmGuidedScratch behind the pieces and 1 / r, in its order
struct GuidedSizes {
    size_t m, active, m_parts, idx, part, partials;
};
GuidedSizes guided_sizes(int n, const NnfmSegments &segs, int k) {
    const NnfmPlan p = nnfm_plan(n, segs.largest());
    const size_t S = segs.count, pairs = S * p.q_blocks;
    return GuidedSizes{round64(S * n), round64((pairs + 3) / 4), round64(pairs), round64(S * k * n),
                       p.slices > 1 ? round64(S * p.slices * k * n) : 0, round64(2 * (size_t)ceil_div(n, 64))};
}

}  // namespace

size_t nnfm_guided_scratch_floats(int C, int n, const NnfmSegments &segs, int k) {
    const GuidedSizes z = guided_sizes(n, segs, k);
    return 64 + nnfm_pieces_floats(n, C) + round64(n) + z.m + z.active + z.m_parts + z.idx + 2 * z.part + z.partials;
}

NnfmGuidedScratch nnfm_guided_carve(float *scratch, int C, int n, const NnfmSegments &segs, int k) {
    const GuidedSizes z = guided_sizes(n, segs, k);
    NnfmGuidedScratch x;
    float *at = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(scratch) + 255) & ~(uintptr_t)255);
    x.xhi = reinterpret_cast<unsigned short *>(at);
    x.xlo = x.xhi + (size_t)n * C;
    at += nnfm_pieces_floats(n, C);
    x.inv_r = at;
    at += round64(n);
    x.m = at;
    at += z.m;
    x.active = reinterpret_cast<unsigned char *>(at);
    at += z.active;
    x.m_parts = at;
    at += z.m_parts;
    x.idx = reinterpret_cast<int *>(at);
    at += z.idx;
    x.part_score = z.part ? at : nullptr;
    at += z.part;
    x.part_idx = z.part ? reinterpret_cast<int *>(at) : nullptr;
    at += z.part;
    x.partials = at;
    return x;
}

int nnfm_mask_window_launch(hipStream_t s, const float *maps, const ContentWindow &win, const NnfmSegments &segs, int k,
                            const NnfmGuidedScratch &x, int *idx, float *a_out) {
    const int n = win.fh * win.fw, q_blocks = ceil_div(n, kNnfmQ);
    if (win.oy < 0 || win.ox < 0 || win.oy + win.fh > win.ch || win.ox + win.fw > win.cw) {
        set_error("nnfm_mask_window_launch: the window [%d+%d, %d+%d] exceeds the %dx%d mask map", win.oy, win.fh,
                  win.ox, win.fw, win.ch, win.cw);
        return STX_ERR_ARG;
    }
    nnfm_mask_window_kernel<<<dim3(q_blocks, segs.count), kNnfmQ, 0, s>>>(maps, win, k, x.m, x.active, x.m_parts, idx);
    STX_CHECK_LAUNCH();
    nnfm_mask_mean_kernel<<<1, 256, 0, s>>>(x.m_parts, segs.count * q_blocks, n, a_out);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

namespace {

template <int K>
void guided_search_k_launch(hipStream_t s, const NnfmGuidedScratch &x, int n, const _Float16 *bhi, const _Float16 *blo,
                            const NnfmSegments &segs, int C, const NnfmPlan &p, int *idx_out) {
    nnfm_search_kernel<false, K, true><<<dim3(p.q_blocks, p.slices, segs.count), 256, 0, s>>>(
        reinterpret_cast<const _Float16 *>(x.xhi), reinterpret_cast<const _Float16 *>(x.xlo), NnfmQueries<false>{n}, bhi,
        blo, 0, C, 0, p.blocks_per_slice, idx_out, x.part_score, x.part_idx, NnfmSegArgs<true>{segs, x.active});
    if (p.slices > 1 && hipPeekAtLastError() == hipSuccess)
        nnfm_merge_seg_kernel<K><<<dim3(ceil_div(n, 256), segs.count), 256, 0, s>>>(x.part_score, x.part_idx, n, p.slices,
                                                                                   x.active, p.q_blocks, idx_out);
}

}  // namespace

int nnfm_guided_search_launch(hipStream_t s, const NnfmGuidedScratch &x, int n, const unsigned short *pieces,
                              const NnfmSegments &segs, int C, int *idx_out, int k) {
    STX_TRY(check_guided("nnfm_guided_search_launch", C, n, segs, k));
    const NnfmPlan p = nnfm_plan(n, segs.largest());        // (slices sized from the largest segment)
    const _Float16 *const bhi = reinterpret_cast<const _Float16 *>(pieces), *const blo = bhi + (size_t)segs.total() * C;
    if (k == 1)
        guided_search_k_launch<1>(s, x, n, bhi, blo, segs, C, p, idx_out);
    else if (k == 2)
        guided_search_k_launch<2>(s, x, n, bhi, blo, segs, C, p, idx_out);
    else if (k == 3)
        guided_search_k_launch<3>(s, x, n, bhi, blo, segs, C, p, idx_out);
    else
        guided_search_k_launch<4>(s, x, n, bhi, blo, segs, C, p, idx_out);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int nnfm_guided_grad_launch(hipStream_t s, const float *feat, int C, int n, const NnfmGuidedScratch &x, const float *bank,
                            const NnfmSegments &segs, const int *idx, const float *a_ptr, float *sgrad, int *n_parts,
                            int k) {
    STX_TRY(check_guided("nnfm_guided_grad_launch", C, n, segs, k));
    const int blocks = ceil_div(n, 64), vec = reinterpret_cast<uintptr_t>(bank) % 16 == 0;
    if (k == 1)
        nnfm_guided_grad_kernel<1><<<blocks, 64, 0, s>>>(feat, C, n, x.inv_r, bank, segs, vec, idx, x.m, a_ptr, sgrad, x.partials);
    else if (k == 2)
        nnfm_guided_grad_kernel<2><<<blocks, 64, 0, s>>>(feat, C, n, x.inv_r, bank, segs, vec, idx, x.m, a_ptr, sgrad, x.partials);
    else if (k == 3)
        nnfm_guided_grad_kernel<3><<<blocks, 64, 0, s>>>(feat, C, n, x.inv_r, bank, segs, vec, idx, x.m, a_ptr, sgrad, x.partials);
    else
        nnfm_guided_grad_kernel<4><<<blocks, 64, 0, s>>>(feat, C, n, x.inv_r, bank, segs, vec, idx, x.m, a_ptr, sgrad, x.partials);
    STX_CHECK_LAUNCH();
    *n_parts = blocks;
    return STX_OK;
}

}  // namespace stx
