// The Laplacian loss (Li, Xu, Nie, Liu, "Laplacian-Steered Neural Style Transfer", 2017): the
// iterate is held to the content picture's edges where the VGG content layer no longer sees them.
// Pictures are [3][H][W] BGR planes, mean subtracted, un-rolled; for a pool size p (a power of two,
// 1..64) and the content picture c of the scale
//     u(x)  = (x_B + x_G + x_R) / 382.5
//     P_p u = block means over p x p blocks on a grid fixed at the origin, hp x wp = ceil(H / p) x
//             ceil(W / p) cells, edge cells over the pixels that exist (mask_map_kernel's convention)
//     D v   = sum over the 4-neighbours inside the grid of (v - v_n): the graph Laplacian of the
//             grid, [0 -1 0; -1 4 -1; 0 -1 0] with a replicated border; symmetric, kills constants
//     T_p   = D P_p u(c)                       (lap_target_launch, once per scale)
//     e_p   = D P_p u(x) - T_p
//     loss  = sum_p coef_p * sum_cells e_p^2
//     grad[ch][y][x] += sum_p 2 coef_p (D e_p)[y / p][x / p] / (n_cell * 382.5),  all three ch
//
// The traffic is the design: the image is read ONCE however many sizes are asked for, the gradient
// is read and written once, and everything between lives on the pooled grids (1/16 of a plane and
// less for p >= 4).  Four kinds of launch:
//   pool     a workgroup owns a 64 x 64 pixel region (a multiple of every p).  A thread loads a
//            4 x 4 pixel block of the three planes, twelve 16-byte loads issued together (element
//            loads with a bounds check when the width or the alignment does not allow them), forms
//            the channel sums and the 1 / 2 / 4 block sums in registers; 8 .. 64 follow through LDS,
//            each level from the 2 x 2 sums of the level below.  mean = sum / (n_cell * 382.5).
//   grid     one launch over all sizes (blockIdx.y), grid-stride over the cells of a size:
//            kTarget  out = D in                          (the target)
//            kError   out = D in - T, partials of sum out^2 per workgroup and size
//            kBack    out = coef * (D in) / (n_cell * 382.5)   (the value a pixel of the cell gets)
//            all three through lap_d, so that img == content gives e == 0 exactly.
//   finish   the partials of every size added in double in a fixed order (finish_partials_n_launch)
//   scatter  a thread owns four neighbouring pixels of a row: the cell values of all sizes are
//            added up first, by themselves, and the sum is added once to each gradient plane with
//            16-byte accesses; pixels whose sum is zero are left untouched.  The cell maps are
//            small and come out of cache.
// No atomics: the same inputs give the same bits.
//
// The file is compiled with -ffp-contract=off, like swt.hip: every sum, difference and quotient
// rounds once, so the error budget of the tests counts operations and the target and the image go
// through identical roundings whatever the compiler would have fused.

#include <algorithm>
#include <cstdint>

#include "common.h"

namespace stx {

namespace {

constexpr int kRegion = 64;         // pixels per side of a pool workgroup's region
constexpr float kUnit = 382.5f;     // 3 * 127.5: n_cell * kUnit is exact in float (n_cell <= 4096)

typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct PoolOut {
    unsigned mask;      // bit lp: pool size 2^lp is wanted
    int off[7];         // where its map starts in `out`
};

// number of pixels that exist in cell (ci, cj) of pool size p
__device__ __forceinline__ int lap_cell_pixels(int ci, int cj, int p, int H, int W) {
    return min(p, H - ci * p) * min(p, W - cj * p);
}

__device__ __forceinline__ void pool_store(float *out, const PoolOut &po, int lp, int ci, int cj, int H,
                                           int W, float sum) {
    const int p = 1 << lp;
    const int hp = (H + p - 1) >> lp, wp = (W + p - 1) >> lp;
    if (ci < hp && cj < wp)
        out[po.off[lp] + (size_t)ci * wp + cj] = sum / ((float)lap_cell_pixels(ci, cj, p, H, W) * kUnit);
}

// grid (ceil(W / 64), ceil(H / 64)).  Thread t: tx = t & 15 -> columns X0 + 4 tx .. + 3,
// ty = t >> 4 -> rows Y0 + 4 ty .. + 3.  Pixels outside the picture count as zero.
template <bool VEC>
__global__ __launch_bounds__(256) void lap_pool_kernel(const float *__restrict__ img, int H, int W,
                                                       PoolOut po, float *__restrict__ out) {
    __shared__ float l4[256], l8[64], l16[16], l32[4];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int x = blockIdx.x * kRegion + 4 * tx, y = blockIdx.y * kRegion + 4 * ty;
    const size_t plane = (size_t)H * W;
    float v[3][4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t row = (size_t)(y + r) * W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (VEC) {
                f32x4_t q = {0.f, 0.f, 0.f, 0.f};
                if (y + r < H && x < W) q = *reinterpret_cast<const f32x4_t *>(img + c * plane + row);
                v[c][r][0] = q.x, v[c][r][1] = q.y, v[c][r][2] = q.z, v[c][r][3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    v[c][r][k] = y + r < H && x + k < W ? img[c * plane + row + k] : 0.f;
            }
        }
    }
    float s[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[r][k] = (v[0][r][k] + v[1][r][k]) + v[2][r][k];
    if (po.mask & 1u) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) pool_store(out, po, 0, y + r, x + k, H, W, s[r][k]);
    }
    float q2[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int m = 0; m < 2; ++m)
            q2[a][m] = (s[2 * a][2 * m] + s[2 * a][2 * m + 1]) + (s[2 * a + 1][2 * m] + s[2 * a + 1][2 * m + 1]);
    if (po.mask & 2u) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int m = 0; m < 2; ++m) pool_store(out, po, 1, y / 2 + a, x / 2 + m, H, W, q2[a][m]);
    }
    const float q4 = (q2[0][0] + q2[0][1]) + (q2[1][0] + q2[1][1]);
    if (po.mask & 4u) pool_store(out, po, 2, y / 4, x / 4, H, W, q4);
    if (po.mask < 8u) return;       // (uniform: nothing above 4 is wanted)
    l4[t] = q4;
    // level lp from the 2 x 2 sums of the level below: side 64 >> lp cells in the region
#define STX_LAP_LEVEL(LP, SRC, DST, SIDE)                                                          \
    __syncthreads();                                                                               \
    if (t < SIDE * SIDE) {                                                                         \
        const int a = t / SIDE, b = t % SIDE;                                                      \
        const float *g = SRC + (2 * a) * (2 * SIDE) + 2 * b;                                       \
        const float q = (g[0] + g[1]) + (g[2 * SIDE] + g[2 * SIDE + 1]);                           \
        DST = q;                                                                                   \
        if (po.mask & (1u << LP))                                                                  \
            pool_store(out, po, LP, blockIdx.y * SIDE + a, blockIdx.x * SIDE + b, H, W, q);        \
    }                                                                                              \
    if (po.mask < (2u << LP)) return;
    STX_LAP_LEVEL(3, l4, l8[t], 8)
    STX_LAP_LEVEL(4, l8, l16[t], 4)
    STX_LAP_LEVEL(5, l16, l32[t], 2)
    __syncthreads();
    if (t == 0) pool_store(out, po, 6, blockIdx.y, blockIdx.x, H, W, (l32[0] + l32[1]) + (l32[2] + l32[3]));
#undef STX_LAP_LEVEL
}

// (D v)[i][j] with the border replicated: a neighbour outside the grid is the cell itself, v - v = 0
__device__ __forceinline__ float lap_d(const float *__restrict__ v, int i, int j, int hp, int wp) {
    const float c = v[(size_t)i * wp + j];
    const float up = v[(size_t)max(i - 1, 0) * wp + j], down = v[(size_t)min(i + 1, hp - 1) * wp + j];
    const float left = v[(size_t)i * wp + max(j - 1, 0)], right = v[(size_t)i * wp + min(j + 1, wp - 1)];
    return ((c - up) + (c - left)) + ((c - right) + (c - down));
}

enum { kTarget = 0, kError = 1, kBack = 2 };

struct LapCoefs {
    float c[kLapMaxPools];
};

// grid (blocks, sizes): size k = blockIdx.y reads in + off[k], writes out + off[k].
template <int MODE>
__global__ __launch_bounds__(256) void lap_grid_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                       const float *__restrict__ target, LapLevels lv,
                                                       LapCoefs coefs, int H, int W,
                                                       float *__restrict__ partials) {
    const int k = blockIdx.y;
    const int hp = lv.hp[k], wp = lv.wp[k], cells = hp * wp, p = 1 << lv.lp[k];
    const float *v = in + lv.off[k];
    float sums[1] = {0.f};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cells; i += gridDim.x * 256) {
        const int ci = i / wp, cj = i - ci * wp;
        const float d = lap_d(v, ci, cj, hp, wp);
        if (MODE == kTarget) {
            out[lv.off[k] + i] = d;
        } else if (MODE == kError) {
            const float e = d - target[lv.off[k] + i];
            sums[0] += e * e;
            out[lv.off[k] + i] = e;
        } else {
            out[lv.off[k] + i] = coefs.c[k] * d / ((float)lap_cell_pixels(ci, cj, p, H, W) * kUnit);
        }
    }
    if (MODE == kError) block_partials<1>(sums, partials + (size_t)k * gridDim.x);
}

// grid (ceil(ceil(W / 4) / 64), ceil(H / 4)), 64 x 4 threads: one group of four pixels each.
template <bool VEC>
__global__ __launch_bounds__(256) void lap_scatter_kernel(const float *__restrict__ cellv, LapLevels lv,
                                                          float *__restrict__ grad, int H, int W) {
    const int x = 4 * (blockIdx.x * 64 + (threadIdx.x & 63)), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= H || x >= W) return;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < lv.n; ++k) {
        const int lp = lv.lp[k];
        const float *row = cellv + lv.off[k] + (size_t)(y >> lp) * lv.wp[k];
        if (lp >= 2) {      // the four pixels share a cell
            const float c = row[x >> lp];
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = k ? g[i] + c : c;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float c = row[min(x + i, W - 1) >> lp];
                g[i] = k ? g[i] + c : c;
            }
        }
    }
    if (g[0] == 0.f && g[1] == 0.f && g[2] == 0.f && g[3] == 0.f) return;
    const size_t plane = (size_t)H * W, at = (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float *dst = grad + c * plane + at;
        if (VEC) {
            f32x4_t q = *reinterpret_cast<f32x4_t *>(dst);
            q.x += g[0], q.y += g[1], q.z += g[2], q.w += g[3];
            *reinterpret_cast<f32x4_t *>(dst) = q;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W && g[i] != 0.f) dst[i] += g[i];
        }
    }
}

bool lap_vec(int W, const void *p) { return W % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int lap_grid_blocks(const LapLevels &lv) {
    int cells = 0;
    for (int k = 0; k < lv.n; ++k) cells = std::max(cells, lv.hp[k] * lv.wp[k]);
    return blocks_for((size_t)cells);
}

int lap_pool_launch(hipStream_t s, const float *img, int H, int W, const LapLevels &lv, float *out) {
    PoolOut po{};
    for (int k = 0; k < lv.n; ++k) {
        po.mask |= 1u << lv.lp[k];
        po.off[lv.lp[k]] = lv.off[k];
    }
    const dim3 grid(ceil_div(W, kRegion), ceil_div(H, kRegion));
    if (lap_vec(W, img))
        lap_pool_kernel<true><<<grid, 256, 0, s>>>(img, H, W, po, out);
    else
        lap_pool_kernel<false><<<grid, 256, 0, s>>>(img, H, W, po, out);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

}  // namespace

size_t lap_levels(int H, int W, int n_pools, const int *pools, LapLevels *lv) {
    size_t total = 0;
    lv->n = n_pools;
    for (int k = 0; k < n_pools; ++k) {
        int lp = 0;
        while ((1 << lp) < pools[k]) ++lp;
        lv->lp[k] = lp;
        lv->hp[k] = ceil_div(H, pools[k]);
        lv->wp[k] = ceil_div(W, pools[k]);
        lv->off[k] = (int)total;
        total += (size_t)lv->hp[k] * lv->wp[k];
    }
    return total;
}

size_t lap_scratch_floats(size_t map_floats) { return 2 * map_floats + (size_t)kLapMaxPools * kBlocks; }

int lap_target_launch(hipStream_t s, const float *content, int H, int W, const LapLevels &lv,
                      float *target, float *scratch) {
    STX_TRY(lap_pool_launch(s, content, H, W, lv, scratch));
    lap_grid_kernel<kTarget><<<dim3(lap_grid_blocks(lv), lv.n), 256, 0, s>>>(scratch, target, nullptr, lv,
                                                                          LapCoefs{}, H, W, nullptr);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

int lap_launch(hipStream_t s, const float *img, float *grad, int H, int W, const LapLevels &lv,
               size_t map_floats, const float *coefs, const float *target, double *loss_terms,
               float *scratch) {
    // scratch: [pooled maps, then the cell values | e | partials]
    float *maps = scratch, *err = scratch + map_floats, *partials = err + map_floats;
    STX_TRY(lap_pool_launch(s, img, H, W, lv, maps));
    const int blocks = lap_grid_blocks(lv);
    LapCoefs cf{};
    for (int k = 0; k < lv.n; ++k) cf.c[k] = coefs[k];
    lap_grid_kernel<kError><<<dim3(blocks, lv.n), 256, 0, s>>>(maps, err, target, lv, cf, H, W, partials);
    STX_CHECK_LAUNCH();
    lap_grid_kernel<kBack><<<dim3(blocks, lv.n), 256, 0, s>>>(err, maps, nullptr, lv, cf, H, W, nullptr);
    STX_CHECK_LAUNCH();
    STX_TRY(finish_partials_n_launch(s, partials, blocks, lv.n, loss_terms));
    const dim3 grid(ceil_div(ceil_div(W, 4), 64), ceil_div(H, 4));
    if (lap_vec(W, grad))
        lap_scatter_kernel<true><<<grid, 256, 0, s>>>(maps, lv, grad, H, W);
    else
        lap_scatter_kernel<false><<<grid, 256, 0, s>>>(maps, lv, grad, H, W);
    STX_CHECK_LAUNCH();
    return STX_OK;
}

}  // namespace stx
