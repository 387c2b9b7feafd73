// ngp_long_sample_kernels.h — ngp_factor_sample_long: paths of a horizon of up to
// NGP_MAX_LONG_HORIZON dates from the sigma the long query leaves on the device (DESIGN.md section
// 4.27).  Included from ngp_kernels.hip behind ngp_col_kernels.h (chol_diag_kernel, gemm_rows,
// solve_and_store_lds) and the sampler's philox4x32_10 / u01, which it uses as they are: path
// (s, d) is the path ngp_mixture_sample draws — same counters, same pick, same Box-Muller pairing.
//
//   ls_pick_kernel     one thread per (scenario, draw): the component
//   ls_count_kernel    one workgroup per particle: how many paths picked it
//   ls_group_kernel    one workgroup per particle: its paths, ascending, behind its offset
//   ls_normals_kernel  z of the staged paths, once per path: Z [sorted position][mpad]
//   ls_pad_kernel      rows and columns m .. mpad of sigma: a unit diagonal
//   chol_diag_kernel   (ngp_col_kernels.h) diagonal block j: C_jj - L_j L_j', its factor and inverse
//   ls_panel_kernel    row blocks i > j: L_ij = (C_ij - L_i L_j') L_jj^-T, one wave per row block —
//                      the step of long_solve_kernel with sigma's own rows as the panel
//   ls_draw_kernel     X = mu + L Z: one wave per (particle, 64-row block, 64 paths), k ascending
#pragma once
#include "ngp_internal.h"
#include "ngp_mfma.h"

namespace ngp {

__global__ __launch_bounds__(LS_THREADS) void ls_pick_kernel(LongSampleGeom g, const double *w,
                                                             unsigned k0, unsigned k1, int32_t *comp) {
    const long idx = (long)blockIdx.x * LS_THREADS + threadIdx.x;
    if (idx >= g.N) return;
    const int s = (int)(idx / g.draws), d = (int)(idx % g.draws);
    // block 0: component pick by inverse CDF over the P weights of scenario s
    const Philox4 r0 = philox4x32_10(Philox4{(unsigned)d, (unsigned)s, 0u, 0u}, k0, k1);
    const double u = u01(r0.x, r0.y);
    const double *ws = w + (long)s * g.P;
    int k = g.P - 1;
    double acc = 0.0;
    for (int i = 0; i < g.P; ++i) {
        acc += ws[i];
        if (u < acc) { k = i; break; }
    }
    comp[idx] = k;
}

__global__ __launch_bounds__(LS_THREADS) void ls_count_kernel(LongSampleGeom g, const int32_t *comp,
                                                              uint32_t *cnt) {
    __shared__ uint32_t part[LS_THREADS];
    const int k = blockIdx.x, tid = threadIdx.x;
    uint32_t c = 0;
    for (long i = tid; i < g.N; i += LS_THREADS) c += comp[i] == k ? 1u : 0u;
    part[tid] = c;
    __syncthreads();
    for (int o = LS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    if (tid == 0) cnt[k] = part[0];
}

// the paths of particle k in ascending order: a running count over slices of LS_THREADS paths, the
// place inside a slice from the waves' ballots
__global__ __launch_bounds__(LS_THREADS) void ls_group_kernel(LongSampleGeom g, const int32_t *comp,
                                                              const uint32_t *off, int32_t *order) {
    __shared__ uint32_t wcnt[LS_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t lim = off[k + 1];           // never written beyond: the counts came from comp too
    uint32_t run = off[k];
    for (long base = 0; base < g.N; base += LS_THREADS) {
        const long i = base + tid;
        const bool hit = i < g.N && comp[i] == k;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) wcnt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int v = 0; v < LS_THREADS / 64; ++v) {
            if (v < wave) before += wcnt[v];
            total += wcnt[v];
        }
        const uint32_t at = run + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (hit && at < lim) order[at] = (int32_t)i;
        run += total;
        __syncthreads();
    }
}

// Z [row][mpad], row r the path at sorted position zfirst + r: blocks 1 + j / 2 of its stream, one
// Box-Muller pair per thread; the second normal of the last pair of an odd m and the padding are 0
__global__ __launch_bounds__(LS_THREADS) void ls_normals_kernel(LongSampleGeom g, unsigned k0, unsigned k1,
                                                                const int32_t *order, long zfirst,
                                                                long zrows, double *Z) {
    const int half = g.mpad / 2;
    const long e = (long)blockIdx.x * LS_THREADS + threadIdx.x;
    if (e >= zrows * half) return;
    const long r = e / half;
    const int j0 = 2 * (int)(e % half);
    double z0 = 0.0, z1 = 0.0;
    if (j0 < g.m) {
        const long idx = order[zfirst + r];
        const int s = (int)(idx / g.draws), d = (int)(idx % g.draws);
        const Philox4 q = philox4x32_10(Philox4{(unsigned)d, (unsigned)s, (unsigned)(1 + j0 / 2), 0u}, k0, k1);
        const double u1 = u01(q.x, q.y), u2 = u01(q.z, q.w);
        const double rad = sqrt(-2.0 * log(u1)), ang = 2.0 * M_PI * u2;
        z0 = rad * cos(ang);
        if (j0 + 1 < g.m) z1 = rad * sin(ang);
    }
    f64x2 v;
    v.x = z0;
    v.y = z1;
    *reinterpret_cast<f64x2 *>(Z + r * g.mpad + j0) = v;
}

__global__ __launch_bounds__(LS_THREADS) void ls_pad_kernel(LongSampleGeom g, double *sigma) {
    double *A = sigma + (long)blockIdx.y * g.stride;
    const int m = g.m, mpad = g.mpad, w = mpad - m;
    const long right = (long)m * w, total = right + (long)w * mpad;
    for (long e = (long)blockIdx.x * LS_THREADS + threadIdx.x; e < total; e += (long)gridDim.x * LS_THREADS) {
        int i, j;
        if (e < right) { i = (int)(e / w); j = m + (int)(e % w); }
        else { i = m + (int)((e - right) / mpad); j = (int)((e - right) % mpad); }
        A[(long)i * mpad + j] = i == j ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(256, 1) void ls_panel_kernel(LongSampleGeom g, LongSamplePtrs p, int j) {
    __shared__ __attribute__((aligned(16))) char epi[EPI_LDS_BYTES];
    const int item = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = j + 1 + blockIdx.x * 4 + wave;
    const bool valid = i < g.nb;                   // wave-uniform
    const long ld = g.mpad;
    double *A = p.sigma + (long)item * g.stride;
    double *Wr = A + (long)(valid ? i : j) * NB * ld;
    const int r16 = lane & 15, q = lane >> 4;
    double acc4[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc4[a][b][r] = 0.0;
    const int kmax = j * NB;
    if (valid) gemm_rows<4>(acc4, A + ((long)j * NB + r16) * ld + 2 * q, Wr + (long)r16 * ld + 2 * q, ld, 0, kmax);
    double *lds_m = reinterpret_cast<double *>(epi);
    double *buf = reinterpret_cast<double *>(epi + EPI_M_BYTES + wave * EPI_WAVE_BYTES);
    stage_mstrips(lds_m, p.dinv + (long)item * (NB * NB), tid);
    __syncthreads();
    NoProbe probe;
    if (valid) solve_and_store_lds(acc4, Wr, lds_m, ld, kmax, lane, buf, probe);
}

// A wave owns 64 rows of L (block i) and 64 paths of one particle: acc = L_i,[0, 64 (i + 1)) Z', the
// k-steps ascending whatever tile a path sits in, so a path's bits do not depend on its neighbours.
// The tile goes through the wave's LDS rows 16 paths at a time and out as 512-byte rows of `out`,
// the mean of the path's own scenario added on the way (row s of the item's mu_rows rows; the
// item's one row where mu_own is 0).  Paths of a particle whose long query or factorisation failed
// are NaN.
__global__ __launch_bounds__(256, 1) void ls_draw_kernel(LongSampleGeom g, LongSamplePtrs p, long zfirst,
                                                         long zrows) {
    __shared__ __attribute__((aligned(16))) double tile[4][16 * EPI_PITCH];
    const int item = blockIdx.z, i = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long lo = max((long)p.off[item], zfirst), hi = min((long)p.off[item + 1], zfirst + zrows);
    const long pos0 = lo + ((long)blockIdx.y * 4 + wave) * NB;
    if (pos0 >= hi) return;                        // wave-uniform; no workgroup barrier below
    const int cntw = (int)min((long)NB, hi - pos0);
    const long ld = g.mpad;
    const double *L = p.sigma + (long)item * g.stride;
    const double *Zr = p.Z + (pos0 - zfirst) * ld;  // rows beyond cntw: the next paths or the slack rows
    const int r16 = lane & 15, q = lane >> 4;
    double acc4[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc4[a][b][r] = 0.0;
    gemm_rows<4>(acc4, L + ((long)i * NB + r16) * ld + 2 * q, Zr + (long)r16 * ld + 2 * q, ld, 0, (i + 1) * NB);
    const bool tainted = p.info[item] > 0 || p.cinfo[item] > 0;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double *mu = p.mu + (long)item * g.mu_rows * g.m;
    double *buf = tile[wave];
    const int n16 = lane & 15, isub = lane >> 4;
    const int jj0 = 4 * (n16 >> 2) + isub;         // acc4[jt][it][r]: row 16 jt + jj0 of L, path 16 it + ((n16 + 4 r) & 15)
    const int col = i * NB + lane;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        if (16 * it >= cntw) break;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[((n16 + 4 * r) & 15) * EPI_PITCH + 16 * jt + jj0] = acc4[jt][it][r];
        __builtin_amdgcn_wave_barrier();
        for (int row = 0; row < 16 && 16 * it + row < cntw; ++row) {
            const long idx = p.order[pos0 + 16 * it + row];
            const int s = g.mu_own ? (int)(idx / g.draws) : 0;
            if (col < g.m)
                p.out[idx * g.m + col] = tainted ? nan : mu[(long)s * g.m + col] + buf[row * EPI_PITCH + lane];
        }
        __builtin_amdgcn_wave_barrier();
    }
}

void launch_ls_pick(const LongSampleGeom &g, const double *w, uint64_t seed, int32_t *comp, hipStream_t s) {
    hipLaunchKernelGGL(ls_pick_kernel, dim3((unsigned)((g.N + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS),
                       0, s, g, w, (unsigned)seed, (unsigned)(seed >> 32), comp);
}
void launch_ls_count(const LongSampleGeom &g, const int32_t *comp, uint32_t *cnt, hipStream_t s) {
    hipLaunchKernelGGL(ls_count_kernel, dim3((unsigned)g.P), dim3(LS_THREADS), 0, s, g, comp, cnt);
}
void launch_ls_group(const LongSampleGeom &g, const int32_t *comp, const uint32_t *off, int32_t *order,
                     hipStream_t s) {
    hipLaunchKernelGGL(ls_group_kernel, dim3((unsigned)g.P), dim3(LS_THREADS), 0, s, g, comp, off, order);
}
void launch_ls_normals(const LongSampleGeom &g, uint64_t seed, const int32_t *order, int64_t zfirst,
                       int64_t zrows, double *Z, hipStream_t s) {
    const int64_t n = zrows * (g.mpad / 2);
    hipLaunchKernelGGL(ls_normals_kernel, dim3((unsigned)((n + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS),
                       0, s, g, (unsigned)seed, (unsigned)(seed >> 32), order, (long)zfirst, (long)zrows, Z);
}
void launch_ls_pad(const LongSampleGeom &g, double *sigma, int B, hipStream_t s) {
    if (g.mpad == g.m) return;
    const int64_t n = (int64_t)(g.mpad - g.m) * (g.m + g.mpad);
    hipLaunchKernelGGL(ls_pad_kernel, dim3((unsigned)std::min<int64_t>((n + LS_THREADS - 1) / LS_THREADS, 1024), B),
                       dim3(LS_THREADS), 0, s, g, sigma);
}
void launch_ls_diag(const LongSampleGeom &g, const LongSamplePtrs &p, int B, int j, hipStream_t s) {
    // of the sweep's geometry chol_diag_kernel reads the row stride and the item stride alone
    JobGeom jg{};
    jg.ld = g.mpad;
    jg.item_stride = g.stride;
    ChunkPtrs cp{};
    cp.L = p.sigma;
    cp.dinv = p.dinv;
    cp.logdet = p.logdet;
    cp.info = p.cinfo;
    hipLaunchKernelGGL(chol_diag_kernel<NoProbe>, dim3(B), dim3(256), 0, s, jg, cp, j, 0);
}
void launch_ls_panel(const LongSampleGeom &g, const LongSamplePtrs &p, int B, int j, hipStream_t s) {
    const int below = g.nb - j - 1;
    if (below <= 0) return;
    hipLaunchKernelGGL(ls_panel_kernel, dim3((below + 3) / 4, B), dim3(256), 0, s, g, p, j);
}
void launch_ls_draw(const LongSampleGeom &g, const LongSamplePtrs &p, int B, int64_t zfirst, int64_t zrows,
                    int tiles, hipStream_t s) {
    if (tiles <= 0) return;
    hipLaunchKernelGGL(ls_draw_kernel, dim3(g.nb, tiles, B), dim3(256), 0, s, g, p, (long)zfirst, (long)zrows);
}

}  // namespace ngp
