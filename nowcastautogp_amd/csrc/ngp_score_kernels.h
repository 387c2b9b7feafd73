// ngp_score_kernels.h — energy score and sample CRPS of an ensemble of paths, per window of dates
// (ngp_ensemble_scores / ngp_mixture_path_scores, include/ngp.h).  Included by ngp_kernels.hip
// behind ngp_path_kernels.h (path_inv) and ngp_mixture_kernels.h (mix_block_sum).
//
//   ES = (1 / N) sum_i |u_i - v|  -  1/2 (1 / D) sum_(i < k) |u_i - u_k|,   |.| over the window
//
// The second sum is the work: N^2 / 2 pairs, each a squared distance over the window's dates and
// one square root.  The squared distance is formed from DIFFERENCES, date by date — never as
// |a|^2 + |b|^2 - 2 a.b: paths that differ by 1e-3 at a level of 1e6 (or that a clamp made equal)
// have nothing left of their distance in that form.
//
//   score_prep_kernel     x [N][m] -> u [m][N] (lanes are paths from here on), the inverse
//                         transformation (mixture form) and the score scale applied once; a value
//                         that is not finite on the score scale flags its date (integer atomic);
//                         v = s(y) by the same device function
//   score_obs_kernel      one thread per path: |u_i - v| per window; a slice's total in a fixed
//                         order (wave shuffles, waves in order) into obs [slice][W]
//   score_pairs_kernel    one workgroup per tile pair (ti <= tk) of SCORE_TILE paths — a grid of the
//                         nt (nt + 1) / 2 pairs, in rows of at most SCORE_GRID_X workgroups (one row
//                         up to N = 524,160; a launch takes fewer than 2^32 threads per dimension,
//                         2^24 workgroups of 256, and N = 2^20 has 2^25 + 2^12 pairs), (ti, tk)
//                         decoded from the block index, which is the pair's slot in the slab; a
//                         thread owns
//                         8 x 8 pairs in registers: rows tr + 16 r, columns tc + 16 c, so a wave
//                         reads 4 row values (a broadcast each) and 16 consecutive column values
//                         per date and register step — no bank conflicts.  A window's dates are
//                         staged SCORE_DCHUNK at a time for both tiles ([date][path], 32 KiB), every
//                         window walks its OWN dates in ascending order (overlapping windows share
//                         nothing, so a window's bits cannot depend on its neighbours), then one
//                         square root per pair and window.  Pairs count where i < k < N: that is
//                         the diagonal rule and the padding rule at once.  One partial per
//                         (tile pair, window) into the slab, in (ti, tk >= ti) order.
//   score_reduce_kernel   folds SCORE_REDUCE rows of a slab into one, rows in order; launched until
//                         one row is left
//
// Chains of additions: 64 square roots in a thread, 6 + 3 in the workgroup's sum, 8 + 6 + 3 per
// fold level (at most three levels at N = 2^20), and a squared distance takes at most SCORE_FOLD
// dates before it moves to a second accumulator (a window of up to SCORE_FOLD dates: 0 + sq, the
// same bits as without one).  No floating-point atomics anywhere.
#pragma once
#include "ngp_internal.h"

namespace ngp {

static_assert(SCORE_THREADS == MIX_THREADS, "mix_block_sum adds the waves of a 256-thread workgroup");
static_assert(SCORE_TILE == 128 && SCORE_THREADS == 256, "16 x 16 threads of 8 x 8 pairs each");

__device__ __forceinline__ double score_scale(double v, int scale, double shift) {
    return scale == NGP_SCORE_LOG ? log(v + shift) : v;
}

// grid (ceil(N / 64), ceil(m / 64))
__global__ __launch_bounds__(SCORE_THREADS) void score_prep_kernel(
    int N, int m, const double *x, const double *y, ngp_inv_transform inv, int apply_inv, int scale,
    double shift, double *u, double *v, int32_t *flag) {
    __shared__ double tile[64][65];
    const int p0 = blockIdx.x * 64, d0 = blockIdx.y * 64, tid = threadIdx.x;
    for (int e = tid; e < 64 * 64; e += SCORE_THREADS) {
        const int p = e >> 6, d = e & 63;
        double val = 0.0;
        if (p0 + p < N && d0 + d < m) {
            val = x[(long)(p0 + p) * m + d0 + d];
            if (apply_inv) val = path_inv(inv, val);
            val = score_scale(val, scale, shift);
            if (!(fabs(val) <= 1.79769313486231570815e308)) atomicOr(&flag[d0 + d], 1);
        }
        tile[p][d] = val;
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += SCORE_THREADS) {
        const int d = e >> 6, p = e & 63;
        if (p0 + p < N && d0 + d < m) u[(long)(d0 + d) * N + p0 + p] = tile[p][d];
    }
    if (blockIdx.x == 0 && tid < 64 && d0 + tid < m) v[d0 + tid] = score_scale(y[d0 + tid], scale, shift);
}

// grid (score_slices(N)); part [slices][W]
__global__ __launch_bounds__(SCORE_THREADS) void score_obs_kernel(int N, int W, const int32_t *win,
                                                                   const double *u, const double *v,
                                                                   double *part) {
    __shared__ double sh[MIX_WAVES];
    const int p = blockIdx.x * SCORE_THREADS + threadIdx.x;
    for (int w = 0; w < W; ++w) {
        const int j0 = win[2 * w], j1 = win[2 * w + 1];
        double dist = 0.0;
        if (p < N) {
            double tot = 0.0, sq = 0.0;
            int n = 0;
            for (int j = j0; j <= j1; ++j) {
                const double df = u[(long)j * N + p] - v[j];
                sq = fma(df, df, sq);
                if (++n == SCORE_FOLD) { tot += sq; sq = 0.0; n = 0; }
            }
            dist = sqrt(tot + sq);
        }
        const double t = mix_block_sum(dist, sh);
        if (threadIdx.x == 0) part[(long)blockIdx.x * W + w] = t;
    }
}

// row ti of the upper triangle of nt x nt tiles starts at slot ti nt - ti (ti - 1) / 2
__host__ __device__ inline long score_row_start(long ti, long nt) { return ti * nt - ti * (ti - 1) / 2; }

// grid score_pairs_grid(N): the block index, row-major, is the slot, in (ti, tk >= ti) order; a block
// past the last slot (the grid's last row may be ragged) has nothing to do; part [slots][W].
// LONG: some window of the call is longer than SCORE_FOLD dates (the second accumulator is
// compiled in; a window up to SCORE_FOLD dates gets the same bits either way)
template <bool LONG>
__global__ __launch_bounds__(SCORE_THREADS) void score_pairs_kernel(int N, int W, const int32_t *win,
                                                                     const double *u, double *part) {
    const long slot = (long)blockIdx.y * gridDim.x + blockIdx.x, nt = (N + SCORE_TILE - 1) / SCORE_TILE;
    if (slot >= nt * (nt + 1) / 2) return;     // the whole workgroup, before its first barrier
    // the row of the slot: the root of the row-start quadratic (exact in fp64: nt <= 8,192), then settled
    const double b2 = (double)(2 * nt + 1);
    long row = (long)(0.5 * (b2 - sqrt(b2 * b2 - 8.0 * (double)slot)));
    row = row < 0 ? 0 : row > nt - 1 ? nt - 1 : row;
    while (row + 1 < nt && score_row_start(row + 1, nt) <= slot) ++row;
    while (row > 0 && score_row_start(row, nt) > slot) --row;
    const int ti = (int)row, tk = (int)(row + (slot - score_row_start(row, nt)));
    __shared__ double sa[SCORE_DCHUNK][SCORE_TILE], sb[SCORE_DCHUNK][SCORE_TILE], sh[MIX_WAVES];
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const int i0 = ti * SCORE_TILE, k0 = tk * SCORE_TILE;
    // the pairs of this thread that count: i < k (the diagonal rule) and k < N (padding)
    unsigned long long mask = 0ull;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int gi = i0 + tr + 16 * r, gk = k0 + tc + 16 * c;
            if (gi < gk && gk < N) mask |= 1ull << (r * 8 + c);
        }
    for (int w = 0; w < W; ++w) {
        const int j0 = win[2 * w], j1 = win[2 * w + 1];
        double sq[8][8], tot[8][8];
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) { sq[r][c] = 0.0; tot[r][c] = 0.0; }
        int since = 0;
        for (int jb = j0; jb <= j1; jb += SCORE_DCHUNK) {
            const int nd = j1 - jb + 1 < SCORE_DCHUNK ? j1 - jb + 1 : SCORE_DCHUNK;
            __syncthreads();                       // the chunk before this one is done with
            for (int e = tid; e < nd * SCORE_TILE; e += SCORE_THREADS) {
                const int d = e >> 7, p = e & (SCORE_TILE - 1);
                const double *row = u + (long)(jb + d) * N;
                sa[d][p] = i0 + p < N ? row[i0 + p] : 0.0;
                sb[d][p] = k0 + p < N ? row[k0 + p] : 0.0;
            }
            __syncthreads();
            for (int d = 0; d < nd; ++d) {
                double a[8], b[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) { a[r] = sa[d][tr + 16 * r]; b[r] = sb[d][tc + 16 * r]; }
#pragma unroll
                for (int r = 0; r < 8; ++r)
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const double df = a[r] - b[c];
                        sq[r][c] = fma(df, df, sq[r][c]);
                    }
            }
            if (LONG) {
                since += nd;
                if (since >= SCORE_FOLD) {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
#pragma unroll
                        for (int c = 0; c < 8; ++c) { tot[r][c] += sq[r][c]; sq[r][c] = 0.0; }
                    since = 0;
                }
            }
        }
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const double d2 = LONG ? tot[r][c] + sq[r][c] : sq[r][c];
                acc += ((mask >> (r * 8 + c)) & 1ull) ? sqrt(d2) : 0.0;
            }
        const double t = mix_block_sum(acc, sh);
        if (tid == 0) part[slot * W + w] = t;
    }
}

// grid (score_folded(rows), W): out [.][W] row b = rows b SCORE_REDUCE ... of in, in row order
__global__ __launch_bounds__(SCORE_THREADS) void score_reduce_kernel(long rows, int W, const double *in,
                                                                      double *out) {
    __shared__ double sh[MIX_WAVES];
    const long base = (long)blockIdx.x * SCORE_REDUCE;
    const int w = blockIdx.y;
    double acc = 0.0;
    for (int r = 0; r < SCORE_REDUCE / SCORE_THREADS; ++r) {
        const long i = base + threadIdx.x + (long)r * SCORE_THREADS;
        if (i < rows) acc += in[i * W + w];
    }
    const double t = mix_block_sum(acc, sh);
    if (threadIdx.x == 0) out[(long)blockIdx.x * W + w] = t;
}

// the pair kernel's grid: gridDim.x * SCORE_THREADS must stay below 2^32, so beyond SCORE_GRID_X slots
// the slots are laid out in the fewest rows that hold them, of equal length (at most y - 1 idle blocks)
static dim3 score_pairs_grid(int N) {
    const long slots = score_tile_pairs(N), y = (slots + SCORE_GRID_X - 1) / SCORE_GRID_X;
    return dim3((unsigned)((slots + y - 1) / y), (unsigned)y);
}

// folds slab[0] ([rows][W]) down to one row, ping-pong with slab[1]; returns where it is
static const double *score_fold(long rows, int W, double *const slab[2], hipStream_t s) {
    int cur = 0;
    while (rows > 1) {
        const long out = score_folded(rows);
        hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)out, (unsigned)W), dim3(SCORE_THREADS), 0,
                           s, rows, W, (const double *)slab[cur], slab[cur ^ 1]);
        rows = out;
        cur ^= 1;
    }
    return slab[cur];
}

hipError_t launch_scores(int N, int m, int W, bool long_windows, const ngp_inv_transform *inv,
                         int scale, double shift, const ScoreBufs &b, const double **obs_sum,
                         const double **pair_sum, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(b.flag, 0, 4 * (size_t)m, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(score_prep_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)((m + 63) / 64)),
                       dim3(SCORE_THREADS), 0, s, N, m, b.x, b.y, inv ? *inv : ngp_inv_transform{},
                       inv ? 1 : 0, scale, shift, b.u, b.v, b.flag);
    hipLaunchKernelGGL(score_obs_kernel, dim3((unsigned)score_slices(N)), dim3(SCORE_THREADS), 0, s, N,
                       W, b.win, (const double *)b.u, (const double *)b.v, b.obs[0]);
    const dim3 slots = score_pairs_grid(N);                    // 2^25 + 2^12 slots at N = 2^20: 5 rows
    if (long_windows)
        hipLaunchKernelGGL(score_pairs_kernel<true>, slots, dim3(SCORE_THREADS), 0, s, N, W,
                           b.win, (const double *)b.u, b.pair[0]);
    else
        hipLaunchKernelGGL(score_pairs_kernel<false>, slots, dim3(SCORE_THREADS), 0, s, N, W,
                           b.win, (const double *)b.u, b.pair[0]);
    *obs_sum = score_fold(score_slices(N), W, b.obs, s);
    *pair_sum = score_fold(score_tile_pairs(N), W, b.pair, s);
    return hipSuccess;
}

}  // namespace ngp
