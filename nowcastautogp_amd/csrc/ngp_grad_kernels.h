#pragma once
#include <type_traits>

#include "ngp_internal.h"
#include "ngp_mfma.h"
#include "ngp_col_kernels.h"
#include "ngp_tree_kernels.h"

namespace ngp {

// ---------------------------------------------------------------------------------------
// gradient of the log marginal likelihood (HMC inside fit_smc! / mcmc_parameters!)
//   d logml / d theta_p = 1/2 sum_ij (alpha_i alpha_j - Kinv_ij) dK_ij / d theta_p
// The factorisation above ran with aux rows [I ; y'], so the aux block is W = [L^-T ; z'] and
//   Kinv = W_I W_I'  (MFMA Gram, upper-triangular W: k starts at the row tile),  alpha = W_I z.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void grad_kinv_kernel(JobGeom g, const double *L,
                                                           double *Kinv, int npairs) {
    const int item = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pr = blockIdx.x * 4 + wave;
    if (pr >= npairs) return;
    int I, J;   // I >= J
    tri_decode(pr, I, J);
    const long ld = g.ld;
    const double *W = L + (long)item * g.item_stride + (long)g.n0 * ld;
    const int r16 = lane & 15, q = lane >> 4;
    double acc4[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc4[a][b][r] = 0.0;
    // S'[jj][i] = sum_k W[64J + jj][k] W[64I + i][k]; W[a][k] = 0 for k < a, so k >= 64 I
    const double *pa = W + (long)(J * NB + r16) * ld + 2 * q;
    const double *pb = W + (long)(I * NB + r16) * ld + 2 * q;
    gemm_rows<4>(acc4, pa, pb, ld, I * NB, g.n0);
    double *Ko = Kinv + (long)item * g.n0 * g.n0;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const f64x4 d = to_d16(acc4[jt][it]);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                Ko[(long)(I * NB + 16 * it + r16) * g.n0 + J * NB + 16 * jt + q + 4 * s] = d[s];
        }
}

// K^-1 = W W' for long series: a workgroup takes a 2 x 2 block of 64 x 64 tiles and stages the
// four row tiles it needs (column tiles J0, J0+1 as the "panel", row tiles I0, I0+1) through LDS by
// LDS-DMA, 16 columns at a time, exactly as the fat step of the factorisation does (same layout,
// same swizzle, same mfma loop) — the wave-per-tile kernel above re-reads both row tiles of every
// tile from HBM (24.6 GB per call at n = 2048 x 64 items, 5.5 TB/s: it was bound by that).  k
// starts at 64 I0 for both row tiles; for I0 + 1 the first 64 columns are zeros of W (upper
// triangular), which add nothing.  Within a 16-column chunk the MFMAs take k in ascending groups
// of four (the fat step's order) where gemm_rows takes even then odd k of an 8-column stage: the
// two kernels agree to rounding, not bit for bit.  Block pairs with bi >= bj; the tile above the
// diagonal in a diagonal block is computed and dropped.
// Grid: 1-D, workgroups b and b + 8 share an XCD (round-robin dispatch), and all blocks of an item
// go to one XCD: the 136 blocks of an item at n = 2048 read its 18 MB of W thirteen times over
// (PMC: 200 MB of fetches per item, 3.2 TB/s) and only an L2 they share can absorb that.
__global__ __launch_bounds__(256, 2) void grad_kinv_lds_kernel(JobGeom g, const double *L,
                                                               double *Kinv, int nblk, int Bc,
                                                               double *alpha) {
    constexpr int ROWB = 128, BLKB = 8 * ROWB + 128, STAGE = 32 * BLKB;
    auto row_off = [](int row) { return (row >> 3) * BLKB + (row & 7) * ROWB; };
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];
    typedef __attribute__((address_space(3))) void *lds_ptr;
    const int wg = blockIdx.x;
    const int xcd = wg & 7, idx = wg >> 3;
    const int item = (idx / nblk) * 8 + xcd;
    const int pr = idx % nblk;
    if (item >= Bc) return;
    int bi, bj;   // bi >= bj
    tri_decode(pr, bi, bj);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ltile = wave >> 1, col = wave & 1;
    const int I0 = 2 * bi, J0 = 2 * bj;
    const int I = I0 + ltile, J = J0 + col;
    // a last, unpaired tile (odd nb0) is staged as a copy of its neighbour and not stored
    const bool valid = I < g.nb0 && J < g.nb0 && I >= J;
    const long ld = g.ld;
    const double *Wb = L + (long)item * g.item_stride + (long)g.n0 * ld;
    const int r16 = lane & 15, q = lane >> 4;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double *>(Wb), 0, (int)((long)g.n0 * ld * (long)sizeof(double)), 0x00020000);
    // stage rows: waves 0,1 the panel (column tiles J0, J0+1), waves 2,3 the row tiles I0, I0+1
    int src_tile = wave < 2 ? J0 + wave : I0 + (wave - 2);
    if (src_tile >= g.nb0) src_tile = g.nb0 - 1;
    const unsigned soff_base =
        (unsigned)__builtin_amdgcn_readfirstlane((int)((long)src_tile * NB * ld * 8));
    const unsigned row_step8 = (unsigned)(8 * ld * 8);
    const unsigned voff_even = (unsigned)(((lane >> 3) * ld + 2 * ((lane & 7) ^ ((lane >> 4) & 7))) * 8);
    const unsigned voff_odd = (unsigned)(((lane >> 3) * ld + 2 * ((lane & 7) ^ ((4 + (lane >> 4)) & 7))) * 8);
    auto stage = [&](int buf, int k) {
        const unsigned kb = (unsigned)k * 8u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            lds_ptr dst = (lds_ptr)(smem + buf * STAGE + (8 * wave + i) * BLKB);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, dst, 16, (i & 1) ? voff_odd : voff_even,
                                                     soff_base + i * row_step8 + kb, 0, 0);
        }
    };
    unsigned a_addr[4], b_addr[4][4];
    {
        const int arow = 64 * col + r16;
        const int akey = (r16 >> 1) & 7;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            a_addr[s] = (unsigned)(row_off(arow) + (((2 * s + (q >> 1)) ^ akey) << 4) + (q & 1) * 8);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rr = (r16 + 4 * r) & 15;
            const int brow = 128 + 64 * ltile + rr;
            const int bkey = (rr >> 1) & 7;
#pragma unroll
            for (int s = 0; s < 4; ++s)
                b_addr[r][s] =
                    (unsigned)(row_off(brow) + (((2 * s + (q >> 1)) ^ bkey) << 4) + (q & 1) * 8);
        }
    }
    double acc4[4][4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc4[a][b][r] = 0.0;
    const int kbeg = I0 * NB;
    // columns beyond the real points are the identity padding of the last block: the rows of W that
    // matter are zero there, so the sum stops at the chunk that holds the last real column
    const int kend = min(g.n0, (g.n_real + LDS_KC - 1) / LDS_KC * LDS_KC);
    const int nchunks = max(kend - kbeg, LDS_KC) / LDS_KC;
    // Products that are known to be nothing are not issued (the wave still stages its rows and keeps
    // the barriers; its SIMD's other wave gets the matrix pipe): a wave whose tile lies above the
    // diagonal of a diagonal block or beyond the last tile, and — W being block upper triangular —
    // the first 64 columns of the k-range for the waves of row tile I0 + 1, whose rows are the
    // stored zeros of block (I0 + 1, I0) there.  Adding those zero products changed no bit.
    const int skip_chunks = __builtin_amdgcn_readfirstlane(!valid ? nchunks : (ltile == 1 ? NB / LDS_KC : 0));
    // alpha = W_I z for the rows of this block row's two row tiles, from the rows the workgroup
    // stages anyway (block pairs with bj = 0: one per block row; W[a][k] = 0 left of a's block
    // column, so the k-range of the block pair is the whole sum): thread (row, half) takes eight
    // of a chunk's sixteen columns.  The separate kernel read every row of W once more from HBM
    // (18.5 MB per item) beside this one and cost it 22 of its 713 ms.
    const bool do_alpha = alpha != nullptr && bj == 0;   // workgroup-uniform
    const int arow = tid >> 1, ahalf = tid & 1;          // LDS row 128 + arow: row arow of (I0, I0 + 1)
    const double *zrow = Wb + (long)g.n0 * ld;           // the data row of W
    const unsigned a_off = (unsigned)row_off(128 + arow);
    const int a_key = (arow >> 1) & 7;
    double asum = 0.0;
    stage(0, kbeg);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const int cur = c & 1;
        if (c + 1 < nchunks) stage(cur ^ 1, kbeg + (c + 1) * LDS_KC);
        const char *buf = smem + cur * STAGE;
        // (the rows of tile I0 + 1 start at their own block column: what lies left of it is never
        // written — wave-uniform: waves 2, 3 hold those rows)
        if (do_alpha && (arow < NB || c >= NB / LDS_KC)) {
            const double *zc = zrow + kbeg + c * LDS_KC + 8 * ahalf;
#pragma unroll
            for (int pp = 0; pp < 4; ++pp) {
                const f64x2 w = *reinterpret_cast<const f64x2 *>(buf + a_off + (((4 * ahalf + pp) ^ a_key) << 4));
                const f64x2 zz = *reinterpret_cast<const f64x2 *>(zc + 2 * pp);
                asum = fma(w.x, zz.x, asum);
                asum = fma(w.y, zz.y, asum);
            }
        }
        if (c >= skip_chunks) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                double a[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    a[u] = *reinterpret_cast<const double *>(buf + a_addr[s] + u * 2 * BLKB);
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    Rot4 br;
                    br.r0 = *reinterpret_cast<const double *>(buf + b_addr[0][s] + it * 2 * BLKB);
                    br.r1 = *reinterpret_cast<const double *>(buf + b_addr[1][s] + it * 2 * BLKB);
                    br.r2 = *reinterpret_cast<const double *>(buf + b_addr[2][s] + it * 2 * BLKB);
                    br.r3 = *reinterpret_cast<const double *>(buf + b_addr[3][s] + it * 2 * BLKB);
#pragma unroll
                    for (int jt = 0; jt < 4; ++jt) mfma16_as_4(acc4[jt][it], a[jt], br);
                }
            }
        }
        __syncthreads();
    }
    if (do_alpha) {
        asum += __shfl_xor(asum, 1, 64);
        const int trow = (I0 + (arow >> 6)) * NB + (arow & 63);
        if (ahalf == 0 && I0 + (arow >> 6) < g.nb0) alpha[(long)item * g.n0 + trow] = asum;
    }
    if (!valid) return;
    // The tile leaves as full 512-byte rows: sixteen rows at a time through a per-wave LDS tile (the
    // stage buffers are free: every wave passed the loop's last barrier), 32 store instructions of
    // 1 KiB instead of 64 that scatter 32-byte pieces over sixteen rows each
    // (profiles/r04/kinv_experiments.txt: the stores were 30 of the kernel's 710 ms).
    double *Ko = Kinv + (long)item * g.n0 * g.n0 + (long)(I * NB) * g.n0 + J * NB;
    constexpr int PITCH = NB + 2;   // doubles: rows stay 16-byte aligned, row groups on distinct banks
    double *tl = reinterpret_cast<double *>(smem) + wave * (16 * PITCH);
#pragma unroll
    for (int it = 0; it < 4; ++it) {
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            const f64x4 d = to_d16(acc4[jt][it]);
#pragma unroll
            for (int s = 0; s < 4; ++s) tl[r16 * PITCH + 16 * jt + q + 4 * s] = d[s];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = 2 * i + (lane >> 5), c2 = 2 * (lane & 31);
            const f64x2 v = *reinterpret_cast<const f64x2 *>(tl + row * PITCH + c2);
            *reinterpret_cast<f64x2 *>(Ko + (long)(16 * it + row) * g.n0 + c2) = v;
        }
    }
}

// alpha[a] = sum_k W[a][k] z[k] (z = the data row of W), quad = z'z; one wave per row
__global__ __launch_bounds__(256) void grad_alpha_kernel(JobGeom g, const double *L, double *alpha,
                                                         double *quad, int a_first) {
    const int item = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = a_first + blockIdx.x * 4 + wave;   // a == n0: the quadratic form
    if (a > g.n0) return;
    const double *W = L + (long)item * g.item_stride + (long)g.n0 * g.ld;
    const double *wa = W + (long)a * g.ld, *z = W + (long)g.n0 * g.ld;
    // W is block upper triangular and what lies left of a row's diagonal block is never written
    // (nor read): row a starts at its own block column
    double s = 0.0;
    for (int k = (a < g.n0 ? (a / NB) * NB : 0) + lane; k < g.n0; k += 64) s += wa[k] * z[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) {
        if (a < g.n0) alpha[(long)item * g.n0 + a] = s;
        else quad[item] = s;
    }
}

// ---- what the contraction kernels share ---------------------------------------------------
// w_ij = alpha_i alpha_j - Kinv_ij on the lower triangle; the diagonal carries 1/2
__device__ __forceinline__ double contract_weight(double ai, double aj, double kinv, bool diag) {
    double w = ai * aj - kinv;
    if (diag) w *= 0.5;
    return w;
}

// lane 0: the sum over the wave, lanes added in a fixed order
__device__ __forceinline__ double wave_sum_down(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Deterministic reduction of a workgroup's accumulators gacc[0..np] into dst[0..np]: wave shuffles,
// then the four waves in order
__device__ __forceinline__ void reduce_partials(const double *gacc, int np,
                                                double (*red)[NGP_MAX_PARAMS + 1], double *dst) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int pidx = 0; pidx <= np; ++pidx) {
        const double v = wave_sum_down(gacc[pidx]);
        if (lane == 0) red[wave][pidx] = v;
    }
    __syncthreads();
    if (tid <= np) dst[tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// Reverse-mode sweep of the kernel tree per matrix element, contracted with
// w_ij = alpha_i alpha_j - Kinv_ij (lower triangle; the diagonal carries 1/2).
__global__ __launch_bounds__(256) void grad_contract_kernel(JobGeom g, const DevProgram *progs,
                                                            const double *t0, const double *Kinv,
                                                            const double *alpha, double *partials,
                                                            int ntri, DevSpec sp) {
    __shared__ DevProgram P;
    __shared__ double red[4][NGP_MAX_PARAMS + 1];
    const int item = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    load_program(&P, progs + item);
    __syncthreads();
    int r, c;
    tri_decode(tile, r, c);
    const int tx = tid & 63, ty = tid >> 6;
    const int col = c * NB + tx;
    const int np = P.n_params, nops = P.n_ops;
    double gacc[NGP_MAX_PARAMS + 1];
    for (int i = 0; i <= np; ++i) gacc[i] = 0.0;
    const double *Ki = Kinv + (long)item * g.n0 * g.n0;
    const double *al = alpha + (long)item * g.n0;
    if (col < g.n_real) {
        const double t2 = t0[col], ac = al[col];
        for (int rr = 0; rr < 16; ++rr) {
            const int row = r * NB + ty * 16 + rr;
            if (row >= g.n_real || col > row) continue;
            const double w = contract_weight(al[row], ac, Ki[(long)row * g.n0 + col], row == col);
            const double t1 = t0[row];
            const double d = fabs(t1 - t2);
            // ---- forward sweep: value of every node
            double val[NGP_MAX_OPS];
            for (int i = 0; i < nops; ++i) {
                const int op = P.ops[i], po = P.poff[i];
                double v;
                if (op < NGP_OP_PLUS)
                    v = leaf_value(op, P, sp, po, t1, t2, d);
                else   // operands: first-evaluated, second
                    v = binary_value(op, val[P.first[i]], val[i - 1], [&](double &g1, double &g2) {
                        g1 = cp_sigma(sp.cp_form, t1, P.params[po], P.params[po + 1]);
                        g2 = cp_sigma(sp.cp_form, t2, P.params[po], P.params[po + 1]);
                    });
                val[i] = v;
            }
            // ---- reverse sweep: adjoint stack mirrors the evaluation stack
            EvalStack st;
            st.s0 = w;
            for (int i = nops - 1; i >= 0; --i) {
                const int op = P.ops[i], po = P.poff[i];
                const double a = st.pop();
                if (op == NGP_OP_CONSTANT) {
                    gacc[po] += a;
                } else if (op == NGP_OP_LINEAR) {
                    const double cc = P.params[po], a1 = t1 - cc, a2 = t2 - cc;
                    gacc[po] += a * P.params[po + 2] * (-a1 - a2);
                    gacc[po + 1] += a;
                    gacc[po + 2] += a * a1 * a2;
                } else if (op == NGP_OP_SQEXP) {
                    const double l = P.params[po], am = P.params[po + 1];
                    const double e = exp(-0.5 * d * d / (sp.se_form ? l : l * l));
                    gacc[po] += a * (sp.se_form ? am * e * 0.5 * d * d / (l * l)
                                                : am * e * d * d / (l * l * l));
                    gacc[po + 1] += a * e;
                } else if (op == NGP_OP_GAMMAEXP) {
                    const double l = P.params[po], gm = P.params[po + 1], am = P.params[po + 2];
                    const double rr_ = d / l, u = pow(rr_, gm), e = exp(-u);
                    gacc[po] += a * am * e * gm * u / l;
                    gacc[po + 1] += (d > 0.0) ? -a * am * e * u * log(rr_) : 0.0;
                    gacc[po + 2] += a * e;
                } else if (op == NGP_OP_PERIODIC) {
                    const double l = P.params[po], per = P.params[po + 1], am = P.params[po + 2];
                    const double ang = M_PI * d / per, sn = sin(ang), cs = cos(ang);
                    const double cq = sp.periodic_form ? 2.0 / l : 2.0 / (l * l);
                    const double e = exp(-cq * sn * sn);
                    gacc[po] += a * (sp.periodic_form ? am * e * 2.0 * sn * sn / (l * l)
                                                      : am * e * 4.0 * sn * sn / (l * l * l));
                    gacc[po + 1] += a * am * e * cq * 2.0 * sn * cs * M_PI * d / (per * per);
                    gacc[po + 2] += a * e;
                } else {
                    const double x = val[P.first[i]], y = val[i - 1];
                    double ax, ay;   // adjoints of the first-evaluated and the second operand
                    if (op == NGP_OP_PLUS) {
                        ax = a; ay = a;
                    } else if (op == NGP_OP_TIMES) {
                        ax = a * y; ay = a * x;
                    } else {
                        const bool nat = (op == NGP_OP_CHANGEPOINT);
                        const double kl = nat ? x : y, kr = nat ? y : x;
                        const double loc = P.params[po], sc = P.params[po + 1];
                        const double sgn = sp.cp_form ? 1.0 : -1.0;   // u = sgn (t - loc) / sc
                        const double u1 = sgn * (t1 - loc) / sc, u2 = sgn * (t2 - loc) / sc;
                        const double th1 = tanh(u1), th2 = tanh(u2);
                        const double g1 = 0.5 * (1.0 + th1), g2 = 0.5 * (1.0 + th2);
                        const double q1 = 0.5 * (1.0 - th1 * th1), q2 = 0.5 * (1.0 - th2 * th2);
                        const double d1l = q1 * (-sgn / sc), d2l = q2 * (-sgn / sc);
                        const double d1s = q1 * (-u1 / sc), d2s = q2 * (-u2 / sc);
                        gacc[po] += a * (d1l * kl * g2 + g1 * kl * d2l - d1l * kr * (1.0 - g2) -
                                         (1.0 - g1) * kr * d2l);
                        gacc[po + 1] += a * (d1s * kl * g2 + g1 * kl * d2s - d1s * kr * (1.0 - g2) -
                                             (1.0 - g1) * kr * d2s);
                        const double al_ = a * g1 * g2, ar_ = a * (1.0 - g1) * (1.0 - g2);
                        ax = nat ? al_ : ar_;
                        ay = nat ? ar_ : al_;
                    }
                    st.push2(ax, ay);
                }
            }
            if (row == col) gacc[np] += w;   // d K / d noise = I (w already carries the 1/2)
        }
    }
    reduce_partials(gacc, np, red, partials + ((long)item * ntri + tile) * (NGP_MAX_PARAMS + 1));
}

// The same contraction on lattice times: every transcendental of the tree comes from the per-item
// tables (tab / dtab by integer distance, sig by point), so the n^2/2 element loop is lookups and
// FMAs only.  ChangePoint: sigma = (1 + tanh u)/2 gives d sigma / du = 2 sigma (1 - sigma).
// LDSV: the node values of the forward sweep live in LDS (one column per thread) instead of a
// runtime-indexed private array, which hipcc puts in scratch — the kernel is bound by that scratch
// traffic (3.93 -> 2.96 ms at n = 2048, 64 items).  Needs programs of at most LDSV_OPS operators;
// the launcher falls back to the private-array instantiation otherwise.
constexpr int LDSV_OPS = 16;
template <bool LDSV>
__global__ __launch_bounds__(256) void grad_contract_lattice_kernel(JobGeom g, ChunkPtrs p,
                                                                    const double *Kinv,
                                                                    const double *alpha,
                                                                    double *partials, int ntri,
                                                                    int split, DevSpec sp,
                                                                    const int32_t *items) {
    __shared__ DevProgram P;
    __shared__ double red[4][NGP_MAX_PARAMS + 1];
    // split: workgroups per 64x64 tile (1, 2 or 4).  A thread walks 16 / split rows; a small
    // launch (few items, short series) is latency-bound on that walk, so it is cut into more,
    // shorter workgroups (158 -> 60 us for 64 particles at n = 150).
    const int item = items ? items[blockIdx.y] : (int)blockIdx.y;
    const int tile = blockIdx.x / split, sub = blockIdx.x % split;
    const int tid = threadIdx.x;
    const int nrows = 16 / split;
    load_program(&P, p.progs + item);
    __syncthreads();
    // per-operator constants of the derivative formulas, once per workgroup: the element loop
    // below then has no fp64 division (twelve of them per element before)
    __shared__ double cst[NGP_MAX_OPS][2];
    __shared__ double vals[LDSV ? LDSV_OPS : 1][256];
    for (int i = tid; i < P.n_ops; i += 256) {
        const int op = P.ops[i], po = P.poff[i];
        double c0 = 0.0, c1 = 0.0;
        if (op == NGP_OP_SQEXP) {
            const double l = P.params[po], am = P.params[po + 1];
            c0 = am * (sp.se_form ? 0.5 / (l * l) : 1.0 / (l * l * l));
        } else if (op == NGP_OP_GAMMAEXP) {
            c0 = P.params[po + 2] * P.params[po + 1] / P.params[po];
            c1 = P.params[po + 2];
        } else if (op == NGP_OP_PERIODIC) {
            const double l = P.params[po], per = P.params[po + 1], am = P.params[po + 2];
            const double cq = sp.periodic_form ? 2.0 / l : 2.0 / (l * l);
            c0 = am * (sp.periodic_form ? 2.0 / (l * l) : 4.0 / (l * l * l));
            c1 = am * cq * 2.0 * M_PI / (per * per);
        } else if (op == NGP_OP_CHANGEPOINT || op == OP_CP_SWAPPED) {
            c1 = 1.0 / P.params[po + 1];
            c0 = sp.cp_form ? c1 : -c1;            // u = c0 (t - loc)
        }
        cst[i][0] = c0;
        cst[i][1] = c1;
    }
    __syncthreads();
    int r, c;
    tri_decode(tile, r, c);
    const int tx = tid & 63, ty = tid >> 6;
    const int col = c * NB + tx;
    const int np = P.n_params, nops = P.n_ops;
    const int R = g.R, npts = g.npts;
    const double *tab = p.tab + (long)item * g.maxstat * R;
    const double *dt = p.dtab + (long)item * g.maxstat * 3 * R;
    const double *sig = p.sig + (long)item * g.maxcp * npts;
    double gacc[NGP_MAX_PARAMS + 1];
    for (int i = 0; i <= np; ++i) gacc[i] = 0.0;
    const double *Ki = Kinv + (long)item * g.n0 * g.n0;
    const double *al = alpha + (long)item * g.n0;
    if (col < g.n_real) {
        const double t2 = p.t0[col], ac = al[col];
        const int q2 = p.qpts[col];
        for (int rr = 0; rr < nrows; ++rr) {
            const int row = r * NB + ty * 16 + sub * nrows + rr;
            if (row >= g.n_real || col > row) continue;
            const double w = contract_weight(al[row], ac, Ki[(long)row * g.n0 + col], row == col);
            const double t1 = p.t0[row];
            const double d = fabs(t1 - t2);
            const int dq = abs(p.qpts[row] - q2);
            // ---- forward sweep: value of every node
            double vloc[LDSV ? 1 : NGP_MAX_OPS];
            auto val = [&](int i) -> double & { return LDSV ? vals[i][tid] : vloc[i]; };
            for (int i = 0; i < nops; ++i) {
                const int op = P.ops[i], po = P.poff[i];
                double v;
                if (op == NGP_OP_CONSTANT) v = P.params[po];
                else if (op == NGP_OP_LINEAR) v = linear_value(P, po, t1, t2);
                else if (op < NGP_OP_PLUS) v = tab[(long)P.slot[i] * R + dq];
                else   // operands: first-evaluated, second
                    v = binary_value(op, val(P.first[i]), val(i - 1), [&](double &g1, double &g2) {
                        g1 = sig[(long)P.slot[i] * npts + row];
                        g2 = sig[(long)P.slot[i] * npts + col];
                    });
                val(i) = v;
            }
            // ---- reverse sweep: adjoint stack mirrors the evaluation stack
            EvalStack st;
            st.s0 = w;
            for (int i = nops - 1; i >= 0; --i) {
                const int op = P.ops[i], po = P.poff[i];
                const double a = st.pop();
                if (op == NGP_OP_CONSTANT) {
                    gacc[po] += a;
                } else if (op == NGP_OP_LINEAR) {
                    const double cc = P.params[po], a1 = t1 - cc, a2 = t2 - cc;
                    gacc[po] += a * P.params[po + 2] * (-a1 - a2);
                    gacc[po + 1] += a;
                    gacc[po + 2] += a * a1 * a2;
                } else if (op < NGP_OP_PLUS) {
                    const double *d0 = dt + (long)P.slot[i] * 3 * R + dq;
                    const double e = d0[0];
                    const double c0 = cst[i][0], c1 = cst[i][1];
                    if (op == NGP_OP_SQEXP) {
                        gacc[po] += a * e * d * d * c0;
                        gacc[po + 1] += a * e;
                    } else if (op == NGP_OP_GAMMAEXP) {
                        gacc[po] += a * c0 * d0[R];
                        gacc[po + 1] -= a * c1 * d0[2 * R];
                        gacc[po + 2] += a * e;
                    } else {
                        gacc[po] += a * c0 * d0[R];
                        gacc[po + 1] += a * c1 * d0[2 * R];
                        gacc[po + 2] += a * e;
                    }
                } else {
                    const double x = val(P.first[i]), y = val(i - 1);
                    double ax, ay;   // adjoints of the first-evaluated and the second operand
                    if (op == NGP_OP_PLUS) {
                        ax = a; ay = a;
                    } else if (op == NGP_OP_TIMES) {
                        ax = a * y; ay = a * x;
                    } else {
                        const bool nat = (op == NGP_OP_CHANGEPOINT);
                        const double kl = nat ? x : y, kr = nat ? y : x;
                        const double loc = P.params[po];
                        const double us = cst[i][0], isc = cst[i][1];   // u = us (t - loc), 1 / scale
                        const double u1 = us * (t1 - loc), u2 = us * (t2 - loc);
                        const double g1 = sig[(long)P.slot[i] * npts + row];
                        const double g2 = sig[(long)P.slot[i] * npts + col];
                        const double q1 = 2.0 * g1 * (1.0 - g1), q2_ = 2.0 * g2 * (1.0 - g2);
                        const double d1l = -q1 * us, d2l = -q2_ * us;
                        const double d1s = -q1 * u1 * isc, d2s = -q2_ * u2 * isc;
                        gacc[po] += a * (d1l * kl * g2 + g1 * kl * d2l - d1l * kr * (1.0 - g2) -
                                         (1.0 - g1) * kr * d2l);
                        gacc[po + 1] += a * (d1s * kl * g2 + g1 * kl * d2s - d1s * kr * (1.0 - g2) -
                                             (1.0 - g1) * kr * d2s);
                        const double al_ = a * g1 * g2, ar_ = a * (1.0 - g1) * (1.0 - g2);
                        ax = nat ? al_ : ar_;
                        ay = nat ? ar_ : al_;
                    }
                    st.push2(ax, ay);
                }
            }
            if (row == col) gacc[np] += w;   // d K / d noise = I (w already carries the 1/2)
        }
    }
    reduce_partials(gacc, np, red,
                    partials + ((long)item * ntri * split + blockIdx.x) * (NGP_MAX_PARAMS + 1));
}

// f(std::integral_constant<int, I>) for I = FROM, FROM - 1, ..., 0: an unrolled loop by construction
// (where `#pragma unroll` is a request hipcc may decline, indices here ARE compile-time constants)
template <int FROM, class F>
__device__ __forceinline__ void static_for_down(F &&f) {
    if constexpr (FROM >= 0) {
        f(std::integral_constant<int, FROM>{});
        static_for_down<FROM - 1>(f);
    }
}

// The lattice contraction for trees of at most NL leaves (2 NL - 1 nodes) with NOTHING
// runtime-indexed in private memory.  The runtime-indexed gacc[] of the kernel above goes to scratch
// (784 B per lane: 58 MB of HBM traffic per item and call, and every `gacc[po] +=` a dependent
// load-add-store); indexing the accumulators by node slot instead needs 3 x 16 of them and the
// unrolled sweeps then keep ~225 VGPRs + scratch.  Here the workgroup first splits the program
// into its LEAVES and its BINARY nodes (in postfix order each, which is a topological order), and
// both sweeps run leaf list / binary list separately, unrolled over the list ordinal:
//     forward:  leaves -> vals[node];  binaries ascending: vals[node] = op(vals[first], vals[node-1])
//     reverse:  vals[root] = w;  binaries descending: the adjoints of the two operands overwrite
//               their values (every node has one parent: its value is dead once the parent is
//               done);  leaves: a = vals[node], accumulate
// so the accumulators are ga[leaf ordinal][3] and gcp[binary ordinal][2] — 38 doubles for 15
// nodes, all static — and one LDS array [node][thread] carries values, then adjoints.
// `items`: the chunk's items whose trees have at most NL leaves (launch_grad_contract sorts the
// items into the instantiations by size: most trees of an ensemble are one to four leaves, and a
// launch sized for the largest tree of the batch would run all of them at its occupancy).
// NACC / PASS: trees of more than 8 leaves would need more accumulators than the register file holds
// beside the sweeps; they run the kernel several times (PASS = 0, 1, ...), every pass sweeping all
// nodes but accumulating only the leaves / binaries with ordinal in [PASS NACC, (PASS + 1) NACC) — the
// first pass writes the partial sums, the later ones add theirs (same thread, same address, stream
// order).  Twice the sweep arithmetic, still no scratch.
// DIAG (the Toeplitz gradient path, stationary trees on a regular series): the contraction runs
// over the n lattice distances instead of the n^2 / 2 elements — element d stands for the whole
// d-th diagonal, `Kinv` then holds its weight w[item][d] = sum_i (a_i a_(i-d) - Kinv_(i,i-d)) (the
// diagonal d = 0 already halved; toep_weights_kernel), evaluated at (row, col) = (d, 0); one
// distance per thread, blockIdx.x = block of 256 distances.
template <int NL, int NACC = NL, int PASS = 0, bool DIAG = false>
__global__ __launch_bounds__(256) void grad_contract_lists_kernel(JobGeom g, ChunkPtrs p,
                                                                  const double *Kinv,
                                                                  const double *alpha,
                                                                  double *partials, int ntri,
                                                                  int split, DevSpec sp,
                                                                  const int32_t *items, int tpw = 1) {
    constexpr int NBIN = NL - 1, NN = 2 * NL - 1;
    constexpr bool PREFETCH = NL <= 8;     // 4 NL + 2 NBIN more doubles in registers
    __shared__ DevProgram P;
    __shared__ double red[4][NGP_MAX_PARAMS + 1];
    __shared__ double cst[NN][2];
    // values, then adjoints, of the nodes: [node][thread] in LDS — except for trees of one or two
    // leaves (REGS), whose shape is fixed (leaf, leaf, operator: nodes 0, 1, 2): three registers, no
    // LDS round trip between the leaves, the operator and the adjoints of a row
    constexpr bool REGS = NL <= 2;
    __shared__ double vals[REGS ? 1 : NN][REGS ? 1 : 256];
    __shared__ unsigned leaf_dec[NL], bin_dec[NBIN > 0 ? NBIN : 1];
    const int item = items ? items[blockIdx.y] : (int)blockIdx.y;
    // a workgroup walks `tpw` consecutive tiles of its item (large launches: the program load, the
    // list decode and the final reduction are paid once per workgroup, a third of its life at one
    // tile) and leaves ONE row of partial sums
    const int tile_first = (int)(blockIdx.x / split) * tpw, sub = blockIdx.x % split;
    const int tid = threadIdx.x;
    const int nrows = 16 / split;
    load_program(&P, p.progs + item);
    for (int i = tid; i < 4 * (NGP_MAX_PARAMS + 1); i += 256) (&red[0][0])[i] = 0.0;
    __syncthreads();
    if (tid < 64) {   // one wave: node i -> its list and its constants
        const int i = tid;
        const bool live = i < P.n_ops;
        const int op = live ? P.ops[i] : 0, po = live ? P.poff[i] : 0;
        const bool leaf = live && op < NGP_OP_PLUS;
        const unsigned long long lm = __ballot(leaf), bm = __ballot(live && !leaf);
        const unsigned long long below = (1ull << i) - 1ull;
        // node | opcode | parameter offset | table / sigmoid slot; binaries: first operand in the top byte
        if (leaf)
            leaf_dec[__popcll(lm & below)] =
                (unsigned)i | ((unsigned)op << 5) | ((unsigned)po << 9) | ((unsigned)P.slot[i] << 17);
        else if (live)
            bin_dec[__popcll(bm & below)] = (unsigned)i | ((unsigned)op << 5) | ((unsigned)po << 9) |
                                            ((unsigned)P.slot[i] << 17) | ((unsigned)P.first[i] << 25);
        if (i < NN) {
            double c0 = 0.0, c1 = 0.0;
            if (op == NGP_OP_SQEXP) {
                const double l = P.params[po], am = P.params[po + 1];
                c0 = am * (sp.se_form ? 0.5 / (l * l) : 1.0 / (l * l * l));
            } else if (op == NGP_OP_GAMMAEXP) {
                c0 = P.params[po + 2] * P.params[po + 1] / P.params[po];
                c1 = P.params[po + 2];
            } else if (op == NGP_OP_PERIODIC) {
                const double l = P.params[po], per = P.params[po + 1], am = P.params[po + 2];
                const double cq = sp.periodic_form ? 2.0 / l : 2.0 / (l * l);
                c0 = am * (sp.periodic_form ? 2.0 / (l * l) : 4.0 / (l * l * l));
                c1 = am * cq * 2.0 * M_PI / (per * per);
            } else if (op == NGP_OP_CHANGEPOINT || op == OP_CP_SWAPPED) {
                c1 = 1.0 / P.params[po + 1];
                c0 = sp.cp_form ? c1 : -c1;            // u = c0 (t - loc)
            }
            cst[i][0] = c0;
            cst[i][1] = c1;
        }
    }
    __syncthreads();
    // a wave works on ONE row at a time (its 64 lanes are 64 columns): the row index is
    // wave-uniform, which hipcc cannot see in `tid >> 6` — said explicitly, everything that is a
    // function of the row alone (t0[row], qpts[row], alpha[row], the ChangePoint sigmoid of the row)
    // becomes a scalar load instead of a vector load that every lane repeats, and the table lookups
    // of an element no longer wait behind it (they were two dependent memory round trips per row)
    const int tx = tid & 63, ty = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int np = P.n_params;
    const int nops = __builtin_amdgcn_readfirstlane(P.n_ops);
    const int nl = (nops + 1) / 2, nbin = nops / 2;       // a binary tree: nl leaves, nl - 1 binaries
    const int R = g.R, npts = g.npts;
    const double *tab = p.tab + (long)item * g.maxstat * R;
    const double *dt = p.dtab + (long)item * g.maxstat * 3 * R;
    const double *sig = p.sig + (long)item * g.maxcp * npts;
    // The decoded lists.  Trees of one or two leaves (most items of an ensemble) read them ONCE into
    // scalar registers: every index below is a compile-time constant, so the two arrays are 2 NL - 1
    // SGPRs, never memory — read from LDS where they are used, every use is an LDS round trip on the
    // critical path of every row (the compiler barrier at the top of the row loop forbids keeping
    // them), three to four per node and row.  Larger trees keep the LDS reads: with the words in
    // registers hipcc hoists everything derived from them as well and spills SGPRs into VGPRs
    // (<8>: 232 -> 254 VGPRs, one wave per SIMD instead of two).
    constexpr bool HOIST = NL <= 2;
    unsigned ldv[HOIST ? NL : 1], bdv[HOIST && NBIN > 0 ? NBIN : 1];
    if constexpr (HOIST) {
        static_for_down<NL - 1>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            ldv[l] = l < nl ? (unsigned)__builtin_amdgcn_readfirstlane((int)leaf_dec[l]) : 0u;
        });
        static_for_down<NBIN - 1>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            bdv[b] = b < nbin ? (unsigned)__builtin_amdgcn_readfirstlane((int)bin_dec[b]) : 0u;
        });
    }
    auto LD = [&](int l) {
        if constexpr (HOIST) return ldv[l];
        else return (unsigned)__builtin_amdgcn_readfirstlane((int)leaf_dec[l]);
    };
    auto BD = [&](int b) {
        if constexpr (HOIST) return bdv[b];
        else return (unsigned)__builtin_amdgcn_readfirstlane((int)bin_dec[b]);
    };
    auto f_node = [](unsigned d) { return (int)(d & 31u); };
    auto f_op = [](unsigned d) { return (int)((d >> 5) & 15u); };
    auto f_po = [](unsigned d) { return (int)((d >> 9) & 255u); };
    auto f_slot = [](unsigned d) { return (int)((d >> 17) & 255u); };
    auto f_first = [](unsigned d) { return (int)(d >> 25); };
    double ga[NACC][3], gcp[NACC][2];
#pragma unroll
    for (int l = 0; l < NACC; ++l) ga[l][0] = ga[l][1] = ga[l][2] = gcp[l][0] = gcp[l][1] = 0.0;
    constexpr auto own = [](int ordinal) { return ordinal / NACC == PASS; };
    double gnoise = 0.0;
    const double *Ki = Kinv + (long)item * g.n0 * (DIAG ? 1 : g.n0);
    const double *al = alpha + (long)item * g.n0;
    // What depends on the row alone — its time, lattice coordinate and alpha — is loaded ONCE per
    // wave, lane rr holding the values of the wave's row rr, and handed to all lanes by v_readlane
    // where the row is processed.  Loaded inside the row loop (as until round 4) they were vector
    // loads that every lane repeats (the compiler barrier below forbids scalar loads: memory may
    // have changed), and the lattice coordinate stood between the row and its table lookups: two
    // dependent memory round trips per row where there is now one.
    for (int tile = tile_first; tile < (DIAG ? tile_first + 1 : min(tile_first + tpw, ntri)); ++tile) {
    int r = 0, c = 0;
    if constexpr (!DIAG) tri_decode(tile, r, c);
    const int col = DIAG ? 0 : c * NB + tx;
    const int row0 = DIAG ? 0 : r * NB + ty * 16 + sub * nrows;
    double t1_l = 0.0, al_l = 0.0;
    int q1_l = 0;
    if constexpr (!DIAG) {
        const int lrow = row0 + (tx < nrows ? tx : 0);      // < n0: inside every array
        t1_l = p.t0[lrow];
        q1_l = p.qpts[lrow];
        al_l = al[lrow];
    }
    // ChangePoint sigmoids (trees of up to four leaves): the column's value once per lane, the rows'
    // values once per wave (lane rr = row rr), instead of two loads per node and row
    constexpr bool SIGPRE = PREFETCH && NL <= 4 && NBIN > 0 && !DIAG;
    double sgc[SIGPRE ? NBIN : 1], sgr_l[SIGPRE ? NBIN : 1];
    if constexpr (SIGPRE) {
        const int lrow = row0 + (tx < nrows ? tx : 0), lcol = col < g.n0 ? col : 0;
        static_for_down<NBIN - 1>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            sgc[b] = sgr_l[b] = 0.0;
            if (b >= nbin) return;
            const int op = f_op(BD(b));
            if (op == NGP_OP_CHANGEPOINT || op == OP_CP_SWAPPED) {
                sgc[b] = sig[(long)f_slot(BD(b)) * npts + lcol];
                sgr_l[b] = sig[(long)f_slot(BD(b)) * npts + lrow];
            }
        });
    }
    if (col < g.n_real) {
        const double t2 = p.t0[col], ac = DIAG ? 0.0 : al[col];
        const int q2 = p.qpts[col];
        for (int rr = 0; rr < (DIAG ? 1 : nrows); ++rr) {
            const int row = DIAG ? (int)blockIdx.x * 256 + tid : row0 + rr;
            if (row >= g.n_real || col > row) continue;
            // nothing loop-invariant is to be hoisted out of this loop: with the sweeps unrolled
            // hipcc would keep every node's parameters, constants and table addresses in VGPRs
            // across the rows
            asm volatile("" ::: "memory");
            double w, t1;
            int q1;
            if constexpr (DIAG) {
                w = Ki[row];
                t1 = p.t0[row];
                q1 = p.qpts[row];
            } else {
                t1 = readlane_f64(t1_l, rr);
                q1 = __builtin_amdgcn_readlane(q1_l, rr);
                w = contract_weight(readlane_f64(al_l, rr), ac, Ki[(long)row * g.n0 + col], row == col);
            }
            const double d = fabs(t1 - t2);
            const int dq = abs(q1 - q2);
            // ---- every table value of this element requested up front (PREFETCH): read where
            //      the sweeps use them, each leaf's lookups wait out their own round trip — four or
            //      five dependent memory latencies per element, which is what the kernel's time was
            //      (2.3 us per row of a wave at two leaves).  Together they cost one.
            double tv[PREFETCH ? NL : 1], td[PREFETCH ? NL : 1][3], sg[PREFETCH && NBIN ? NBIN : 1][2];
            if constexpr (PREFETCH) {
                static_for_down<NL - 1>([&](auto lc) {
                    constexpr int l = decltype(lc)::value;
                    if (l >= nl) return;
                    const int op = f_op(LD(l));
                    if (op > NGP_OP_LINEAR) {      // a stationary leaf: value and derivative factors
                        const long sl = f_slot(LD(l));
                        const double *d0 = dt + sl * 3 * R + dq;
                        tv[l] = tab[sl * R + dq];
                        td[l][0] = d0[0];
                        td[l][1] = d0[R];
                        td[l][2] = d0[2 * R];
                    }
                });
                static_for_down<NBIN - 1>([&](auto bc) {
                    constexpr int b = decltype(bc)::value;
                    if (b >= nbin) return;
                    const int op = f_op(BD(b));
                    if (op == NGP_OP_CHANGEPOINT || op == OP_CP_SWAPPED) {
                        if constexpr (SIGPRE) {
                            sg[b][0] = readlane_f64(sgr_l[b], rr);
                            sg[b][1] = sgc[b];
                        } else {
                            sg[b][0] = sig[(long)f_slot(BD(b)) * npts + row];
                            sg[b][1] = sig[(long)f_slot(BD(b)) * npts + col];
                        }
                    }
                });
            }
            double rv[3] = {0.0, 0.0, 0.0};
            // ---- forward: leaves, then binary nodes in postfix order
            static_for_down<NL - 1>([&](auto lc) {
                constexpr int l = decltype(lc)::value;
                if (l >= nl) return;
                const int op = f_op(LD(l)), po = f_po(LD(l));
                double v;
                if (op == NGP_OP_CONSTANT) v = P.params[po];
                else if (op == NGP_OP_LINEAR)
                    v = P.params[po + 1] + P.params[po + 2] * (t1 - P.params[po]) * (t2 - P.params[po]);
                else if constexpr (PREFETCH) v = tv[l];
                else v = tab[(long)f_slot(LD(l)) * R + dq];
                if constexpr (REGS) rv[l] = v;
                else vals[f_node(LD(l))][tid] = v;
            });
            static_for_down<NBIN - 1>([&](auto bc) {
                constexpr int b = NBIN - 1 - decltype(bc)::value;       // ascending: postfix order
                if (b >= nbin) return;
                const int op = f_op(BD(b)), nd = f_node(BD(b));
                const double x = REGS ? rv[0] : vals[f_first(BD(b))][tid], y = REGS ? rv[1] : vals[nd - 1][tid];
                double v;
                if (op == NGP_OP_PLUS) v = x + y;
                else if (op == NGP_OP_TIMES) v = x * y;
                else {
                    const double kl = (op == NGP_OP_CHANGEPOINT) ? x : y;
                    const double kr = (op == NGP_OP_CHANGEPOINT) ? y : x;
                    const double g1 = PREFETCH ? sg[b][0] : sig[(long)f_slot(BD(b)) * npts + row];
                    const double g2 = PREFETCH ? sg[b][1] : sig[(long)f_slot(BD(b)) * npts + col];
                    v = g1 * kl * g2 + (1.0 - g1) * kr * (1.0 - g2);
                }
                if constexpr (REGS) rv[2] = v;
                else vals[nd][tid] = v;
            });
            // ---- reverse: the root's adjoint is w; adjoints overwrite values on the way down
            if constexpr (REGS) {
                if (nops == 1) rv[0] = w;
                else rv[2] = w;
            } else {
                vals[nops - 1][tid] = w;
            }
            static_for_down<NBIN - 1>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                if (b >= nbin) return;
                const int op = f_op(BD(b)), nd = f_node(BD(b)), fi = f_first(BD(b));
                const double a = REGS ? rv[2] : vals[nd][tid];
                const double x = REGS ? rv[0] : vals[fi][tid], y = REGS ? rv[1] : vals[nd - 1][tid];
                double ax, ay;   // adjoints of the first-evaluated and the second operand
                if (op == NGP_OP_PLUS) {
                    ax = a; ay = a;
                } else if (op == NGP_OP_TIMES) {
                    ax = a * y; ay = a * x;
                } else {
                    const bool nat = (op == NGP_OP_CHANGEPOINT);
                    const double kl = nat ? x : y, kr = nat ? y : x;
                    const int po = f_po(BD(b));
                    const double loc = P.params[po];
                    const double us = cst[nd][0], isc = cst[nd][1];   // u = us (t - loc), 1 / scale
                    const double u1 = us * (t1 - loc), u2 = us * (t2 - loc);
                    const double g1 = PREFETCH ? sg[b][0] : sig[(long)f_slot(BD(b)) * npts + row];
                    const double g2 = PREFETCH ? sg[b][1] : sig[(long)f_slot(BD(b)) * npts + col];
                    const double q1 = 2.0 * g1 * (1.0 - g1), q2_ = 2.0 * g2 * (1.0 - g2);
                    const double d1l = -q1 * us, d2l = -q2_ * us;
                    const double d1s = -q1 * u1 * isc, d2s = -q2_ * u2 * isc;
                    if (own(b)) {
                        gcp[b % NACC][0] += a * (d1l * kl * g2 + g1 * kl * d2l -
                                                 d1l * kr * (1.0 - g2) - (1.0 - g1) * kr * d2l);
                        gcp[b % NACC][1] += a * (d1s * kl * g2 + g1 * kl * d2s -
                                                 d1s * kr * (1.0 - g2) - (1.0 - g1) * kr * d2s);
                    }
                    const double al_ = a * g1 * g2, ar_ = a * (1.0 - g1) * (1.0 - g2);
                    ax = nat ? al_ : ar_;
                    ay = nat ? ar_ : al_;
                }
                if constexpr (REGS) {
                    rv[0] = ax;
                    rv[1] = ay;
                } else {
                    vals[fi][tid] = ax;
                    vals[nd - 1][tid] = ay;
                }
            });
            static_for_down<NL - 1>([&](auto lc) {
                constexpr int l = decltype(lc)::value;
                if (l >= nl || !own(l)) return;
                const int op = f_op(LD(l)), po = f_po(LD(l)), nd = f_node(LD(l));
                const double a = REGS ? rv[l] : vals[nd][tid];
                if (op == NGP_OP_CONSTANT) {
                    ga[l % NACC][0] += a;
                } else if (op == NGP_OP_LINEAR) {
                    const double cc = P.params[po], a1 = t1 - cc, a2 = t2 - cc;
                    ga[l % NACC][0] += a * P.params[po + 2] * (-a1 - a2);
                    ga[l % NACC][1] += a;
                    ga[l % NACC][2] += a * a1 * a2;
                } else {
                    const double *d0 = dt + (long)f_slot(LD(l)) * 3 * R + dq;
                    const double e = PREFETCH ? td[l][0] : d0[0];
                    const double f1 = PREFETCH ? td[l][1] : d0[R], f2 = PREFETCH ? td[l][2] : d0[2 * R];
                    const double c0 = cst[nd][0], c1 = cst[nd][1];
                    if (op == NGP_OP_SQEXP) {
                        ga[l % NACC][0] += a * e * d * d * c0;
                        ga[l % NACC][1] += a * e;
                    } else if (op == NGP_OP_GAMMAEXP) {
                        ga[l % NACC][0] += a * c0 * f1;
                        ga[l % NACC][1] -= a * c1 * f2;
                        ga[l % NACC][2] += a * e;
                    } else {
                        ga[l % NACC][0] += a * c0 * f1;
                        ga[l % NACC][1] += a * c1 * f2;
                        ga[l % NACC][2] += a * e;
                    }
                }
            });
            if (PASS == 0 && row == col) gnoise += w;   // d K / d noise = I (w carries the 1/2)
        }
    }
    }   // tiles of this workgroup
    // ---- deterministic reduction: wave shuffles per (node, parameter), then the four waves in order
    const int lane = tid & 63, wave = tid >> 6;
    static_for_down<NL - 1>([&](auto lc) {
        constexpr int l = decltype(lc)::value;
        if (l >= nl || !own(l)) return;
        const int op = f_op(LD(l));
        const int cnt = op == NGP_OP_CONSTANT ? 1 : (op == NGP_OP_SQEXP ? 2 : 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k >= cnt) break;
            const double v = wave_sum_down(ga[l % NACC][k]);
            if (lane == 0) red[wave][f_po(LD(l)) + k] = v;
        }
    });
    static_for_down<NBIN - 1>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if (b >= nbin) return;
        const int op = f_op(BD(b));
        if ((op != NGP_OP_CHANGEPOINT && op != OP_CP_SWAPPED) || !own(b)) return;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double v = wave_sum_down(gcp[b % NACC][k]);
            if (lane == 0) red[wave][f_po(BD(b)) + k] = v;
        }
    });
    if (PASS == 0) {
        const double v = wave_sum_down(gnoise);
        if (lane == 0) red[wave][np] = v;
    }
    __syncthreads();
    if (tid <= np) {
        double *dst = partials + ((long)item * gridDim.x + blockIdx.x) * (NGP_MAX_PARAMS + 1) + tid;
        const double sum = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
        if (PASS == 0) *dst = sum;
        else *dst += sum;      // a parameter of another pass adds 0.0: its bits do not change
    }
}

// ---------------------------------------------------------------------------------------
// The Toeplitz gradient path (stationary trees on a regular series).
// K is symmetric positive definite Toeplitz there, dK/dtheta depends on the lattice distance only,
// so  d logml / d theta = sum_d w(d) dk(d)/dtheta  with  w(d) = sum_i (a_i a_(i-d) - Kinv_(i,i-d))
// (halved at d = 0), and by the Gohberg-Semencul formula the diagonal sums of Kinv follow from its
// first column x = Kinv e_1 alone:
//     sum_i Kinv_(i,i-d) = (1/x_0) sum_(m=0)^(n-1-d) (n - d - m) (x_(m+d) x_m - x_(n-m) x_(n-m-d)),  x_n = 0.
// A = X Kinv for the two aux rows X = [y' ; e_1'] comes out of the ordinary factorisation and one
// backward sweep (aux_back_*): row 0 = a' (alpha), row 1 = x'.  n^3/3 flops instead of n^3, no W,
// no Kinv.  One workgroup per (item, block of 256 distances): each thread sums its distance in a
// fixed order (deterministic).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void toep_weights_kernel(JobGeom g, const double *A, double *wbuf) {
    extern __shared__ double sh[];      // a[n] | x[n + 1]
    const int item = blockIdx.y, n = g.n_real, tid = threadIdx.x;
    const double *a_g = A + (long)item * g.naux_pad * g.ld, *x_g = a_g + g.ld;
    double *a = sh, *x = sh + n;
    for (int i = tid; i < n; i += 256) {
        a[i] = a_g[i];
        x[i] = x_g[i];
    }
    if (tid == 0) x[n] = 0.0;
    __syncthreads();
    const int d = blockIdx.x * 256 + tid;
    if (d >= n) return;
    const double rx0 = 1.0 / x[0];
    double sa = 0.0, s1 = 0.0, s2 = 0.0;
    for (int m = 0; m < n - d; ++m) {
        const double wgt = (double)(n - d - m);
        sa += a[m + d] * a[m];
        s1 += wgt * (x[m + d] * x[m]);
        s2 += wgt * (x[n - m] * x[n - m - d]);
    }
    const double wv = sa - (s1 - s2) * rx0;
    wbuf[(long)item * g.n0 + d] = (d == 0) ? 0.5 * wv : wv;
}

// quad = z'z from the aux row that carries y' (row 0), before the backward sweep overwrites it
__global__ __launch_bounds__(256) void toep_quad_kernel(JobGeom g, const double *L, double *quad) {
    __shared__ double red[4];
    const int item = blockIdx.x, tid = threadIdx.x;
    const double *z = L + (long)item * g.item_stride + (long)g.n0 * g.ld;
    double s = 0.0;
    for (int i = tid; i < g.n_real; i += 256) s += z[i] * z[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) quad[item] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(128) void grad_reduce_kernel(JobGeom g, const DevProgram *progs,
                                                          const double *partials, const double *quad,
                                                          const double *logdet, double *grad,
                                                          double *logml, int ntri) {
    const int item = blockIdx.x, pidx = threadIdx.x;
    const int np = progs[item].n_params;
    if (pidx <= np) {
        // t ascending, as ever (the sum's bits do not depend on the launch); sixteen loads in
        // flight at a time — one dependent load per addition made this 0.2 ms of a 64-particle call
        const double *src = partials + (long)item * ntri * (NGP_MAX_PARAMS + 1) + pidx;
        double s = 0.0;
        int t = 0;
        for (; t + 16 <= ntri; t += 16) {
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = src[(long)(t + u) * (NGP_MAX_PARAMS + 1)];
#pragma unroll
            for (int u = 0; u < 16; ++u) s += v[u];
        }
        for (; t < ntri; ++t) s += src[(long)t * (NGP_MAX_PARAMS + 1)];
        grad[(long)item * (NGP_MAX_PARAMS + 1) + pidx] = s;
    }
    if (pidx == 0)
        logml[item] = -0.5 * quad[item] - logdet[item] - 0.5 * g.n_real * 1.8378770664093454836;
}

}  // namespace ngp
