// ngp_tree_kernels.h — everything that EVALUATES a kernel tree: the interpreters, the standalone
// covariance assembly, the lattice tables, the four fill kernels and the K-apply of the Gram
// refinement.  Included from ngp_kernels.hip.
//
// One definition per rule.  The routes below were split off each other for speed and must give the
// same bits wherever two of them can compute the same element (tests: structured storage, lockstep,
// GPU parity), so what they share is written once:
//   EvalStack            the eight-register evaluation stack and its adjoint mirror
//   cp_blend             the ChangePoint combination; binary_value: Plus / Times / ChangePoint
//   leaf_value           SqExp / GammaExp / Periodic / Linear / Constant leaves
//   chain_step           one instruction of a chain program on NR x NC elements
//                        (fill_chain_kernel, kapply_kernel<.., KA_CHAIN>)
//   fill_tile_of, fill_ctx, fill_finish_and_store
//                        tile -> (block row, block column, aux), the thread's columns and per-item
//                        pointers, and the store epilogue of the four fill kernels
// All helpers are scalars in structs or references with compile-time indices: nothing here is
// runtime-indexed (that would go to scratch).
//
//   cov_kernel            k(t1, t2) for ngp_cov_batch, direct interpreter
//   tables_kernel         per item: subtree / leaf tables by lattice distance, sigmoids by point
//   fill_kernel           direct interpreter, irregular times
//   fill_lattice_kernel   table lookups through the full (gradient jobs) or reduced program
//   fill_single_kernel    stationary trees: one lookup per element
//   fill_chain_kernel     chain programs: every instruction decoded once for 8 elements
//   kapply_kernel         R = X - A K with K re-evaluated tile by tile (NGP_PREC_MIXED refinement)
#pragma once
#include "ngp_internal.h"
#include "ngp_mfma.h"

namespace ngp {

// ---------------------------------------------------------------------------------------
// kernel-tree interpreter
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void load_program(DevProgram *dst, const DevProgram *src) {
    const unsigned long long *s = reinterpret_cast<const unsigned long long *>(src);
    unsigned long long *d = reinterpret_cast<unsigned long long *>(dst);
    for (unsigned i = threadIdx.x; i < sizeof(DevProgram) / 8; i += blockDim.x) d[i] = s[i];
}

__device__ __forceinline__ double cp_sigma(int form, double x, double loc, double scale) {
    const double u = form ? (x - loc) / scale : (loc - x) / scale;
    return 0.5 * (1.0 + tanh(u));
}

// The evaluation stack of the interpreters: a register shift file (no runtime-indexed arrays, which
// would go to scratch).  push / pop2_push evaluate; pop / push2 are their adjoint mirror (the
// reverse sweeps of the gradient contraction).
struct EvalStack {
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
    __device__ __forceinline__ void push(double v) {
        s7 = s6; s6 = s5; s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v;
    }
    // the two operands on top (s1 evaluated first, s0 second) give way to the result
    __device__ __forceinline__ void pop2_push(double v) {
        s0 = v; s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
    }
    __device__ __forceinline__ double pop() {
        const double a = s0;
        s0 = s1; s1 = s2; s2 = s3; s3 = s4; s4 = s5; s5 = s6; s6 = s7;
        return a;
    }
    // adjoints of the first-evaluated (ax) and the second operand (ay): the second operand (root at
    // i - 1) is visited next, so it goes on top
    __device__ __forceinline__ void push2(double ax, double ay) {
        s7 = s5; s6 = s4; s5 = s3; s4 = s2; s3 = s1; s2 = s0; s1 = ax; s0 = ay;
    }
};

// ChangePoint of operands a (evaluated first) and b; fwd: a is the left kernel (NGP_OP_CHANGEPOINT),
// else the operands were swapped by the flattening (OP_CP_SWAPPED)
__device__ __forceinline__ double cp_blend(bool fwd, double a, double b, double g1, double g2) {
    const double kl = fwd ? a : b;
    const double kr = fwd ? b : a;
    return g1 * kl * g2 + (1.0 - g1) * kr * (1.0 - g2);
}

// Value of a binary node from its operands x (evaluated first) and y.  sigmoids(g1, g2) supplies the
// two ChangePoint sigmoids and is called for a ChangePoint only.
template <class Sig>
__device__ __forceinline__ double binary_value(int op, double x, double y, Sig &&sigmoids) {
    if (op == NGP_OP_PLUS) return x + y;
    if (op == NGP_OP_TIMES) return x * y;
    double g1, g2;
    sigmoids(g1, g2);
    return cp_blend(op == NGP_OP_CHANGEPOINT, x, y, g1, g2);
}

__device__ __forceinline__ double linear_value(const DevProgram &P, int pi, double t1, double t2) {
    const double c = P.params[pi];
    return P.params[pi + 1] + P.params[pi + 2] * (t1 - c) * (t2 - c);
}

// Value of the leaf `op` whose parameters start at P.params[pi], d = |t1 - t2|: THE leaf formulas of
// keval, keval_stat (tables_kernel) and the forward sweep of grad_contract_kernel.  LINEAR = false
// leaves the Linear branch out (stationary subtrees have none).
template <bool LINEAR = true>
__device__ __forceinline__ double leaf_value(int op, const DevProgram &P, const DevSpec &sp, int pi,
                                             double t1, double t2, double d) {
    if (op == NGP_OP_CONSTANT) return P.params[pi];
    if (LINEAR && op == NGP_OP_LINEAR) return linear_value(P, pi, t1, t2);
    if (op == NGP_OP_SQEXP) {
        const double l = P.params[pi];
        const double den = sp.se_form ? l : l * l;
        return P.params[pi + 1] * exp(-0.5 * d * d / den);
    }
    if (op == NGP_OP_GAMMAEXP)
        return P.params[pi + 2] * exp(-pow(d / P.params[pi], P.params[pi + 1]));
    // NGP_OP_PERIODIC
    const double l = P.params[pi];
    const double sn = sin(M_PI * d / P.params[pi + 1]);
    const double c = sp.periodic_form ? 2.0 / l : 2.0 / (l * l);
    return P.params[pi + 2] * exp(-c * sn * sn);
}

// parameters a leaf / a ChangePoint takes from params[] (interpreters that walk params[] in order)
__device__ __forceinline__ int leaf_nparams(int op) {
    return op == NGP_OP_CONSTANT ? 1 : (op == NGP_OP_SQEXP ? 2 : 3);
}

// Evaluate k(t1, t2) for the program held in LDS; ops are workgroup-uniform.
__device__ double keval(const DevProgram &P, const DevSpec &sp, double t1, double t2) {
    EvalStack st;
    int pi = 0;
    const int nops = P.n_ops;
    const double d = fabs(t1 - t2);
    for (int i = 0; i < nops; ++i) {
        const int op = __builtin_amdgcn_readfirstlane((int)P.ops[i]);
        if (op < NGP_OP_PLUS) {
            st.push(leaf_value(op, P, sp, pi, t1, t2, d));
            pi += leaf_nparams(op);
        } else {
            st.pop2_push(binary_value(op, st.s1, st.s0, [&](double &g1, double &g2) {
                const double loc = P.params[pi], sc = P.params[pi + 1];
                g1 = cp_sigma(sp.cp_form, t1, loc, sc);
                g2 = cp_sigma(sp.cp_form, t2, loc, sc);
                pi += 2;
            }));
        }
    }
    return st.s0;
}

// ---------------------------------------------------------------------------------------
// standalone covariance assembly (ngp_cov_batch; also the K22-style small blocks in tests)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cov_kernel(const DevProgram *progs, const double *t1,
                                                  int n1, const double *t2, int n2, int add_diag,
                                                  double *out, DevSpec sp) {
    __shared__ DevProgram P;
    const int b = blockIdx.y;
    load_program(&P, progs + b);
    __syncthreads();
    const long total = (long)n1 * n2;
    double *o = out + (long)b * total;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int i = (int)(e / n2), j = (int)(e % n2);
        double v = keval(P, sp, t1[i], t2[j]);
        if (add_diag && i == j) v += P.noise + sp.jitter;
        o[e] = v;
    }
}

// ---------------------------------------------------------------------------------------
// fill: K lower blocks + aux rows into the factor storage, one 64x64 tile per workgroup.
// What the four fill kernels share: where a tile sits, which two columns a thread owns, and what
// is stored around the kernel values.
// ---------------------------------------------------------------------------------------
struct FillTile {
    int r, c;     // block row / block column (aux: tile row inside the aux block)
    bool aux;
};

// Tiles [0, ntri) are the lower-triangular blocks (r >= c, tile = r(r+1)/2 + c), the aux tiles
// follow row by row.  AUXID (kernels that serve gradient jobs): with g.aux_identity only the y'
// tile row and the zero blocks (a, a-1) of the identity are filled, see launch_fill.  TOEP
// (fill_single_kernel): with g.toep only the diagonal tiles (they carry the noise) and the aux rows
// are stored; the column kernels take every other tile from the table (struct_slice).
template <bool AUXID, bool TOEP = false>
__device__ __forceinline__ FillTile fill_tile_of(const JobGeom &g, int tile, int ntri) {
    FillTile t;
    const bool toep = TOEP && g.toep;
    const int nmain = toep ? g.nb0 : ntri;
    t.aux = tile >= nmain;
    if (!t.aux) {
        if (toep) t.r = t.c = tile;
        else tri_decode(tile, t.r, t.c);
    } else {
        const int a = tile - nmain;
        if (AUXID && g.aux_identity) {
            t.r = a < g.nb0 ? g.nb0 : a - g.nb0 + 1;
            t.c = a < g.nb0 ? a : a - g.nb0;
        } else {
            t.r = a / g.nb0;   // aux tile row
            t.c = a % g.nb0;
        }
    }
    return t;
}

// thread = (column pair tx, 8-row group ty): two adjacent columns per thread -> 16-byte stores
struct FillCtx {
    int item, ty, col;          // col: the first of the thread's two columns
    double *Lit;                // the item's factor storage
    const double *tab, *sig;    // the item's lattice tables (TABLES) else null
    const double *y0;
    int naux_t;                 // aux rows that carry a time; row naux_t is y'
    double diag;                // noise + jitter
};

template <bool TABLES>
__device__ __forceinline__ FillCtx fill_ctx(const JobGeom &g, const ChunkPtrs &p, int item,
                                            const FillTile &t, double noise, const DevSpec &sp) {
    FillCtx x;
    x.item = item;
    x.ty = threadIdx.x >> 5;
    x.col = t.c * NB + 2 * (threadIdx.x & 31);
    x.Lit = p.L + (long)item * g.item_stride;
    x.tab = TABLES ? p.tab + (long)item * g.maxstat * g.R : nullptr;
    x.sig = TABLES ? p.sig + (long)item * g.maxcp * g.npts : nullptr;
    x.y0 = p.y0 + (g.y_shared ? 0 : (long)item * g.n0);
    x.naux_t = g.da + g.m;
    x.diag = noise + sp.jitter;
    return x;
}

// Does row lr of the tile hold kernel values (the others are data, identity or zero rows that
// fill_finish_and_store writes)?
template <bool AUXID>
__device__ __forceinline__ bool fill_row_has_value(const JobGeom &g, const FillCtx &x,
                                                   const FillTile &t, int lr) {
    if (!t.aux) return true;
    if (AUXID && g.aux_identity) return false;
    return t.r * NB + lr < x.naux_t;
}

// Point (index into t0 then taux, qpts, sig) of row lr of the tile; rows without a kernel value:
// any valid point (0), the value is not used
__device__ __forceinline__ int fill_row_point(const JobGeom &g, const FillCtx &x, const FillTile &t,
                                              int lr) {
    const int pt = t.r * NB + lr;
    if (!t.aux) return pt;
    return pt < x.naux_t ? g.n0 + pt : 0;
}

// Store row lr of the tile: v = the kernel values of the thread's two columns (read only where
// fill_row_has_value).  Main block: + diag on the diagonal, identity padding past n_real.  Aux block:
// the y' row behind the rows that carry a time, zero rows behind it (AUXE1, the Toeplitz gradient
// path: e_1' beside y'); AUXID: [I ; y'].  16-byte store; mixed-precision jobs keep the untouched aux
// rows X in p.auxX for the refinement.
template <bool AUXID, bool AUXE1 = false>
__device__ __forceinline__ void fill_finish_and_store(const JobGeom &g, const ChunkPtrs &p,
                                                      const FillCtx &x, const FillTile &t, int lr,
                                                      f64x2 v) {
    const int col = x.col;
    long row;
    if (!t.aux) {
        row = (long)t.r * NB + lr;
        if (row == col) v.x += x.diag;
        if (row == col + 1) v.y += x.diag;
        if (row >= g.n_real || col >= g.n_real) v.x = (row == col) ? 1.0 : 0.0;
        if (row >= g.n_real || col + 1 >= g.n_real) v.y = (row == col + 1) ? 1.0 : 0.0;
    } else {
        const int ar = t.r * NB + lr;
        row = (long)g.n0 + ar;
        if (AUXID && g.aux_identity) {
            v.x = ar < g.n0 ? (ar == col ? 1.0 : 0.0) : (ar == g.n0 ? x.y0[col] : 0.0);
            v.y = ar < g.n0 ? (ar == col + 1 ? 1.0 : 0.0) : (ar == g.n0 ? x.y0[col + 1] : 0.0);
        } else if (ar == x.naux_t) {
            v.x = x.y0[col];
            v.y = x.y0[col + 1];
        } else if (AUXE1 && g.aux_e1 && ar == x.naux_t + 1) {
            v.x = (col == 0) ? 1.0 : 0.0;
            v.y = 0.0;
        } else if (ar > x.naux_t) {
            v.x = 0.0;
            v.y = 0.0;
        }
    }
    *reinterpret_cast<f64x2 *>(x.Lit + row * g.ld + col) = v;
    if (t.aux && p.auxX)
        *reinterpret_cast<f64x2 *>(p.auxX + ((long)x.item * g.naux_pad + (row - g.n0)) * g.ld + col) = v;
}

__global__ __launch_bounds__(256) void fill_kernel(JobGeom g, ChunkPtrs p, int ntri, int tile_off,
                                                   DevSpec sp) {
    __shared__ DevProgram P;
    const int item = blockIdx.y;
    load_program(&P, p.progs + item);
    __syncthreads();
    // tile_off = ntri: aux rows only (cached factor)
    const FillTile t = fill_tile_of<true>(g, blockIdx.x + tile_off, ntri);
    const FillCtx x = fill_ctx<false>(g, p, item, t, P.noise, sp);
    const double t2a = p.t0[x.col], t2b = p.t0[x.col + 1];
    for (int rr = 0; rr < 8; ++rr) {
        const int lr = x.ty * 8 + rr;
        f64x2 v = {0.0, 0.0};
        if (fill_row_has_value<true>(g, x, t, lr)) {
            const int pt = t.r * NB + lr;
            const double t1 = t.aux ? p.taux[pt] : p.t0[pt];
            v.x = keval(P, sp, t1, t2a);
            v.y = keval(P, sp, t1, t2b);
        }
        fill_finish_and_store<true>(g, p, x, t, lr, v);
    }
}

// ---------------------------------------------------------------------------------------
// table-driven fill.  Dates are integer days, so after AutoGP's [0,1] rescale every time sits on
// a lattice t = tmin + q h.  Every transcendental of the kernel grammar is then a function of
// either the integer distance |q_i - q_j| (SquaredExponential / GammaExponential / Periodic
// leaves) or of a single point (ChangePoint sigmoids): O(n) evaluations per leaf instead of
// O(n^2).  tables_kernel evaluates them once per item; fill_lattice_kernel is then pure
// lookups + FMAs and runs at the HBM-write rate.
// ---------------------------------------------------------------------------------------
__device__ double keval_stat(const DevProgram &P, const DevSpec &sp, int first, int last, double d);

__global__ __launch_bounds__(256) void tables_kernel(JobGeom g, ChunkPtrs p, DevSpec sp) {
    __shared__ DevProgram P;
    const int item = blockIdx.x;
    load_program(&P, (p.progs_src ? p.progs_src : p.progs) + item);
    __syncthreads();
    if (p.progs_src) load_program(const_cast<DevProgram *>(p.progs) + item, &P);   // see ChunkPtrs::progs_src
    double *tab = p.tab + (long)item * g.maxstat * g.R;
    double *sig = p.sig + (long)item * g.maxcp * g.npts;
    // gradient jobs: dt = [slot][3][R]: e (the leaf value without its amplitude) and the two
    // factors its lengthscale-type derivatives need, so the O(n^2) contraction is lookups + FMAs
    double *dt = p.dtab ? p.dtab + (long)item * g.maxstat * 3 * g.R : nullptr;
    if (!dt || g.tab_sub > 0) {
        // one table per maximal stationary subtree of the tree (reduced program): all a value job
        // needs; a gradient job keeps them BEHIND its per-leaf tables (slot g.tab_sub on) — its fill
        // then runs on the reduced-program kernels like a value job's, the contraction on the leaves
        // (subtree by subtree: keval_stat takes its opcodes wave-uniformly, so the lanes of a wave
        // must be in the same subtree)
        for (int k = 0; k < P.n_tab; ++k) {
            const int first = P.tb_first[k], last = P.tb_last[k];
            for (int idx = threadIdx.x; idx < g.R; idx += 256)
                tab[(long)(g.tab_sub + k) * g.R + idx] = keval_stat(P, sp, first, last, idx * g.h);
        }
    }
    // One pass over (node, lattice distance) pairs and one over (ChangePoint, point) pairs: a short
    // series (R of a few dozen — the early annealing steps of a fit) fills every leaf's table in ONE
    // round of the workgroup instead of a round per leaf, each a chain of fp64 transcendentals
    // (15 us of a 24-item call at n = 21).  Per entry the arithmetic is what it was.
    // (The leaf tables keep their own expressions: the value is a * ev with ev stored beside it for
    // the derivatives, which is not the expression of leaf_value.)
    for (int e = threadIdx.x; e < P.n_ops * g.R; e += 256) {
        const int i = e / g.R, k = e - i * g.R;
        const int op = P.ops[i], slot = P.slot[i], pi = P.poff[i];
        double *d0 = dt ? dt + (long)slot * 3 * g.R : nullptr;
        if (!d0) break;   // leaf tables: gradient jobs only (value jobs tabulate whole subtrees, above)
        if (op == NGP_OP_SQEXP) {
            const double l = P.params[pi], a = P.params[pi + 1];
            const double den = sp.se_form ? l : l * l;
            const double d = k * g.h;
            const double ev = exp(-0.5 * d * d / den);
            tab[(long)slot * g.R + k] = a * ev;
            d0[k] = ev;
        } else if (op == NGP_OP_GAMMAEXP) {
            const double l = P.params[pi], gam = P.params[pi + 1], a = P.params[pi + 2];
            const double rr = k * g.h / l, u = pow(rr, gam), ev = exp(-u);
            tab[(long)slot * g.R + k] = a * ev;
            d0[k] = ev;
            d0[g.R + k] = ev * u;                                  // -> d / d lengthscale
            d0[2 * g.R + k] = (k > 0) ? ev * u * log(rr) : 0.0;    // -> d / d gamma
        } else if (op == NGP_OP_PERIODIC) {
            const double l = P.params[pi], per = P.params[pi + 1], a = P.params[pi + 2];
            const double c = sp.periodic_form ? 2.0 / l : 2.0 / (l * l);
            const double d = k * g.h, ang = M_PI * d / per;
            const double sn = sin(ang), ev = exp(-c * sn * sn);
            tab[(long)slot * g.R + k] = a * ev;
            d0[k] = ev;
            d0[g.R + k] = ev * sn * sn;                 // -> d / d lengthscale
            d0[2 * g.R + k] = ev * sn * cos(ang) * d;   // -> d / d period
        }
    }
    for (int e = threadIdx.x; e < P.n_ops * g.npts; e += 256) {
        const int i = e / g.npts, pt = e - i * g.npts;
        const int op = P.ops[i];
        if (op == NGP_OP_CHANGEPOINT || op == OP_CP_SWAPPED) {
            const int pi = P.poff[i];
            const double loc = P.params[pi], sc = P.params[pi + 1];
            const double t = pt < g.n0 ? p.t0[pt] : p.taux[pt - g.n0];
            sig[(long)P.slot[i] * g.npts + pt] = cp_sigma(sp.cp_form, t, loc, sc);
        }
    }
}

// k(t1, t2) on lattice times through the FULL program (gradient jobs: tables per leaf)
__device__ __forceinline__ double keval_lattice(const DevProgram &P, const double *tab,
                                                const double *sig, int R, int npts, double t1,
                                                double t2, int dq, int pt1, int pt2) {
    EvalStack st;
    int pi = 0;
    const int nops = P.n_ops;
    for (int i = 0; i < nops; ++i) {
        const int op = __builtin_amdgcn_readfirstlane((int)P.ops[i]);
        if (op < NGP_OP_PLUS) {
            double v;
            if (op == NGP_OP_CONSTANT) {
                v = P.params[pi];
            } else if (op == NGP_OP_LINEAR) {
                v = linear_value(P, pi, t1, t2);
            } else {
                const int slot = __builtin_amdgcn_readfirstlane((int)P.slot[i]);
                v = tab[(long)slot * R + dq];
            }
            pi += leaf_nparams(op);
            st.push(v);
        } else {
            // (its own Plus / Times / ChangePoint branches: through binary_value,
            // fill_lattice_kernel<true> lands two VGPRs lower and on another occupancy step)
            double v;
            if (op == NGP_OP_PLUS) {
                v = st.s1 + st.s0;
            } else if (op == NGP_OP_TIMES) {
                v = st.s1 * st.s0;
            } else {
                const int slot = __builtin_amdgcn_readfirstlane((int)P.slot[i]);
                const double g1 = sig[(long)slot * npts + pt1];
                const double g2 = sig[(long)slot * npts + pt2];
                v = cp_blend(op == NGP_OP_CHANGEPOINT, st.s1, st.s0, g1, g2);
                pi += 2;
            }
            st.pop2_push(v);
        }
    }
    return st.s0;
}

// Value of the stationary subtree ops[first..last] (a postfix range of the full program) at
// distance d: leaf_value per leaf, as keval does element by element.
__device__ double keval_stat(const DevProgram &P, const DevSpec &sp, int first, int last, double d) {
    EvalStack st;
    for (int i = first; i <= last; ++i) {
        const int op = __builtin_amdgcn_readfirstlane((int)P.ops[i]);
        const int pi = __builtin_amdgcn_readfirstlane((int)P.poff[i]);
        if (op < NGP_OP_PLUS) st.push(leaf_value<false>(op, P, sp, pi, 0.0, 0.0, d));
        else st.pop2_push((op == NGP_OP_PLUS) ? st.s1 + st.s0 : st.s1 * st.s0);
    }
    return st.s0;
}

// k(t1, t2) on lattice times through the REDUCED program (DevProgram::rops): table leaves by
// lattice distance dq, Linear in closed form, ChangePoint sigmoids by point
__device__ __forceinline__ double keval_reduced(const DevProgram &P, const double *tab,
                                                const double *sig, int R, int npts, double t1,
                                                double t2, int dq, int pt1, int pt2) {
    const int nops = P.n_rops;
    if (nops == 1 && P.rops[0] == OP_TABLE) return tab[dq];   // the whole tree is stationary
    EvalStack st;
    for (int i = 0; i < nops; ++i) {
        const int code = __builtin_amdgcn_readfirstlane((int)P.rops[i]);
        const int op = code & 15, lk = code >> 4;
        if (op == OP_TABLE || op == NGP_OP_LINEAR) {
            double v;
            if (op == OP_TABLE) {
                const int slot = __builtin_amdgcn_readfirstlane((int)P.rslot[i]);
                v = tab[(long)slot * R + dq];
            } else {
                v = linear_value(P, __builtin_amdgcn_readfirstlane((int)P.rpoff[i]), t1, t2);
            }
            st.push(v);
        } else {
            // operands in evaluation order: a (first), b (second — the fused leaf if there is one)
            double a, b;
            if (lk) {
                const int lf = __builtin_amdgcn_readfirstlane((int)P.rleaf[i]);
                a = st.s0;
                b = (lk == RLEAF_TABLE) ? tab[(long)lf * R + dq] : linear_value(P, lf, t1, t2);
            } else {
                a = st.s1;
                b = st.s0;
            }
            const double v = binary_value(op, a, b, [&](double &g1, double &g2) {
                const int slot = __builtin_amdgcn_readfirstlane((int)P.rslot[i]);
                g1 = sig[(long)slot * npts + pt1];
                g2 = sig[(long)slot * npts + pt2];
            });
            if (lk) st.s0 = v;
            else st.pop2_push(v);
        }
    }
    return st.s0;
}

// split: workgroups per tile (1, 2, 4) — small launches are latency-bound on the 8 rows a thread
// walks, so they are cut into more, shorter workgroups (as in the gradient contraction)
// GRADJOB: the tables are per leaf (the contraction needs them that way) -> full program;
// otherwise per maximal stationary subtree -> reduced program
template <bool GRADJOB>
__global__ __launch_bounds__(256) void fill_lattice_kernel(JobGeom g, ChunkPtrs p, int ntri,
                                                           int tile_off, int split, DevSpec sp) {
    __shared__ DevProgram P;
    // p.fill_other (staged value jobs): the chunk's items that are not chain programs
    const int item = p.fill_other ? p.fill_other[blockIdx.y] - p.fill_base : (int)blockIdx.y;
    load_program(&P, p.progs + item);
    __syncthreads();
    const int sub = blockIdx.x % split;
    const int nrows = 8 / split;
    const FillTile t = fill_tile_of<true>(g, blockIdx.x / split + tile_off, ntri);
    const FillCtx x = fill_ctx<true>(g, p, item, t, P.noise, sp);
    const int col = x.col;
    const double t2a = p.t0[col], t2b = p.t0[col + 1];
    const int q2a = p.qpts[col], q2b = p.qpts[col + 1];
    auto kev = [&](double t1, double t2, int dq, int pt1, int pt2) -> double {
        if constexpr (GRADJOB) return keval_lattice(P, x.tab, x.sig, g.R, g.npts, t1, t2, dq, pt1, pt2);
        else return keval_reduced(P, x.tab, x.sig, g.R, g.npts, t1, t2, dq, pt1, pt2);
    };
    for (int rr = 0; rr < nrows; ++rr) {
        const int lr = x.ty * 8 + sub * nrows + rr;
        f64x2 v = {0.0, 0.0};
        if (fill_row_has_value<true>(g, x, t, lr)) {
            const int pt = fill_row_point(g, x, t, lr);
            const int q1 = p.qpts[pt];
            const double t1 = t.aux ? p.taux[pt - g.n0] : p.t0[pt];
            v.x = kev(t1, t2a, abs(q1 - q2a), pt, col);
            v.y = kev(t1, t2b, abs(q1 - q2b), pt, col + 1);
        }
        fill_finish_and_store<true, true>(g, p, x, t, lr, v);
    }
}

// Stationary trees (the whole reduced program is ONE table: 45 of the 64 base kernels of the bench
// ensemble): K[i][j] = tab[|q_i - q_j|].  No program in LDS, no interpreter: sixteen lookups in
// flight per thread at full occupancy.  `p.fill_single` lists the chunk's such items.
__global__ __launch_bounds__(256) void fill_single_kernel(JobGeom g, ChunkPtrs p, int ntri,
                                                          DevSpec sp) {
    const int item = p.fill_single[blockIdx.y] - p.fill_base;
    const FillTile t = fill_tile_of<false, true>(g, blockIdx.x, ntri);
    const FillCtx x = fill_ctx<true>(g, p, item, t, p.progs[item].noise, sp);   // tab: slot 0, the tree's only table
    const int q2a = p.qpts[x.col], q2b = p.qpts[x.col + 1];
    f64x2 v[8];
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        const int q1 = p.qpts[fill_row_point(g, x, t, x.ty * 8 + rr)];
        v[rr].x = x.tab[abs(q1 - q2a)];
        v[rr].y = x.tab[abs(q1 - q2b)];
    }
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) fill_finish_and_store<false>(g, p, x, t, x.ty * 8 + rr, v[rr]);
}

// One instruction i of a chain program (DevProgram::rchain: instruction 0 pushes, every other one
// carries its leaf) applied to the NR x NC elements kv[rr][u] of a thread: decoded once, same
// formulas and the same order of operations per element as keval_reduced — bit-identical values.
// Rows: the lattice data of row rr — q(rr), t(rr), pt(rr) — wherever the caller keeps them.
template <int NR, int NC, class Rows>
__device__ __forceinline__ void chain_step(const DevProgram &P, int i, const double *tab,
                                           const double *sig, int R, int npts, const Rows &rows,
                                           const int (&q2)[NC], const double (&t2)[NC],
                                           const int (&pt2)[NC], double (&kv)[NR][NC]) {
    const int code = __builtin_amdgcn_readfirstlane((int)P.rops[i]);
    const int op = code & 15;
    int lk = code >> 4, lf;
    if (i == 0) {
        lk = (op == OP_TABLE) ? RLEAF_TABLE : RLEAF_LINEAR;
        lf = __builtin_amdgcn_readfirstlane((int)(op == OP_TABLE ? P.rslot[0] : P.rpoff[0]));
    } else {
        lf = __builtin_amdgcn_readfirstlane((int)P.rleaf[i]);
    }
    double b[NR][NC];
    if (lk == RLEAF_TABLE) {
        const double *tb = tab + (long)lf * R;
#pragma unroll
        for (int rr = 0; rr < NR; ++rr)
#pragma unroll
            for (int u = 0; u < NC; ++u) b[rr][u] = tb[abs(rows.q(rr) - q2[u])];
    } else {
        const double cc = P.params[lf], b0 = P.params[lf + 1], b1 = P.params[lf + 2];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr)
#pragma unroll
            for (int u = 0; u < NC; ++u) b[rr][u] = b0 + b1 * (rows.t(rr) - cc) * (t2[u] - cc);
    }
    if (i == 0) {
#pragma unroll
        for (int rr = 0; rr < NR; ++rr)
#pragma unroll
            for (int u = 0; u < NC; ++u) kv[rr][u] = b[rr][u];
    } else if (op == NGP_OP_PLUS) {
#pragma unroll
        for (int rr = 0; rr < NR; ++rr)
#pragma unroll
            for (int u = 0; u < NC; ++u) kv[rr][u] = kv[rr][u] + b[rr][u];
    } else if (op == NGP_OP_TIMES) {
#pragma unroll
        for (int rr = 0; rr < NR; ++rr)
#pragma unroll
            for (int u = 0; u < NC; ++u) kv[rr][u] = kv[rr][u] * b[rr][u];
    } else {
        const int slot = __builtin_amdgcn_readfirstlane((int)P.rslot[i]);
        const double *sg = sig + (long)slot * npts;
        double g2[NC];
#pragma unroll
        for (int u = 0; u < NC; ++u) g2[u] = sg[pt2[u]];
        const bool fwd = op == NGP_OP_CHANGEPOINT;
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const double g1 = sg[rows.pt(rr)];
#pragma unroll
            for (int u = 0; u < NC; ++u) kv[rr][u] = cp_blend(fwd, kv[rr][u], b[rr][u], g1, g2[u]);
        }
    }
}

// Chain programs (DevProgram::rchain with more than one instruction: one push, then only operations
// that carry their leaf — 17 of the 19 non-stationary base kernels of the bench ensemble): every
// instruction is decoded once per thread and applied to its elements (chain_step).  A kernel of its
// own (238 VGPRs would cost the single-lookup fill of stationary kernels its occupancy); `items`
// lists the chunk's chain items (ChunkPtrs::fill_chain).
// tpw: tiles a workgroup fills one after the other (large launches: the program is loaded and the
// barrier paid once for `tpw` tiles; the values do not depend on it)
struct ChainRowsReg {   // four rows' lattice data in registers
    int q1[4], pt1[4];
    double t1[4];
    __device__ __forceinline__ int q(int rr) const { return q1[rr]; }
    __device__ __forceinline__ int pt(int rr) const { return pt1[rr]; }
    __device__ __forceinline__ double t(int rr) const { return t1[rr]; }
};

__global__ __launch_bounds__(256) void fill_chain_kernel(JobGeom g, ChunkPtrs p, int ntri,
                                                         DevSpec sp, int ntiles, int tpw) {
    __shared__ DevProgram P;
    const int item = p.fill_chain[blockIdx.y] - p.fill_base;
    load_program(&P, p.progs + item);
    __syncthreads();
    for (int tile = blockIdx.x * tpw; tile < min((int)blockIdx.x * tpw + tpw, ntiles); ++tile) {
        const FillTile t = fill_tile_of<false>(g, tile, ntri);
        const FillCtx x = fill_ctx<true>(g, p, item, t, P.noise, sp);
        const int col = x.col;
        const double t2[2] = {p.t0[col], p.t0[col + 1]};
        const int q2[2] = {p.qpts[col], p.qpts[col + 1]};
        const int pt2[2] = {col, col + 1};
        // Two passes of four rows: half the registers of one pass of eight (124 instead of 206 VGPRs:
        // four waves per SIMD instead of two) for one more decode of the program per thread.  Lattice
        // data of the rows first (aux rows past the last time point: any valid point, value unused).
        for (int half = 0; half < 2; ++half) {
            ChainRowsReg rows;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int pt = fill_row_point(g, x, t, x.ty * 8 + 4 * half + rr);
                rows.pt1[rr] = pt;
                rows.q1[rr] = p.qpts[pt];
                rows.t1[rr] = pt < g.n0 ? p.t0[pt] : p.taux[pt - g.n0];
            }
            double kv[4][2];
            const int nops = P.n_rops;
            for (int i = 0; i < nops; ++i)
                chain_step<4, 2>(P, i, x.tab, x.sig, g.R, g.npts, rows, q2, t2, pt2, kv);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                f64x2 v;
                v.x = kv[rr][0];
                v.y = kv[rr][1];
                fill_finish_and_store<false>(g, p, x, t, x.ty * 8 + 4 * half + rr, v);
            }
        }
    }   // tiles of this workgroup
}

// items of the chunk a refinement launch works on: all of them, or the compacted list of those
// that have not converged yet
__device__ __forceinline__ int map_item(const ChunkPtrs &p, int i) {
    return p.items ? p.items[i] : i;
}

// R[:, col] = X[:, col] - sum_row A[:, row] K[row][col]: one thread per column (or two), the rows of
// A it multiplies are wave-uniform (LDS broadcast), K comes from the lattice tables (or the direct
// interpreter) element by element and is never stored.  One workgroup per (64 CPT columns, item,
// NACC aux rows); rows are walked in slabs of 64 whose A block, times and lattice coordinates sit
// in LDS.
// Three instantiations; on a lattice each item is taken by exactly one of the first two (the other
// returns at once):
//   KA_SINGLE   the item's tree is stationary as a whole = ONE table (DevProgram::rops): no
//               interpreter in the loop, two columns per thread, gathers issued eight rows ahead
//   KA_REDUCED  reduced-program interpreter, one column per thread (kept apart from KA_DIRECT: the
//               transcendental code of the direct interpreter cost it half its occupancy)
//   KA_DIRECT   irregular times: direct evaluation of the full program
enum { KA_SINGLE = 0, KA_REDUCED = 1, KA_DIRECT = 2, KA_CHAIN = 3 };
// Workgroup = 64 CPT columns x 4 row quarters: wave w walks the w-th quarter of the rows for the
// same columns and the four partial sums are added in wave order through LDS.  (One wave walking
// all n0 rows was the critical path: a launch took as long as the item with the longest program.)
template <int NACC, int CPT, int MODE>
__global__ __launch_bounds__(256) void kapply_kernel(JobGeom g, ChunkPtrs p, const double *A,
                                                     const double *X, double *Rout, DevSpec sp) {
    __shared__ DevProgram P;
    __shared__ double As[4][NACC][NB];
    __shared__ double t1s[4][NB];
    __shared__ int q1s[4][NB];
    __shared__ double red[3][CPT][NACC][64];
    const int item = map_item(p, blockIdx.y), tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int a0 = blockIdx.z * NACC;
    const int rows = min(NACC, g.naux - a0);
    if (rows <= 0) return;
    if (blockIdx.x * CPT * 64 >= g.n0) return;    // whole workgroup: the grid is sized for CPT = 1
    load_program(&P, p.progs + item);
    __syncthreads();
    constexpr bool SINGLE = MODE == KA_SINGLE;
    if constexpr (MODE != KA_DIRECT) {
        // workgroup-uniform: which of the three lattice instantiations owns this item
        const bool single = P.n_rops == 1 && P.rops[0] == OP_TABLE;
        const bool chain = !single && P.rchain;
        const int mine = single ? KA_SINGLE : (chain ? KA_CHAIN : KA_REDUCED);
        if (mine != MODE) return;
    }
    const long ld = g.ld;
    const double *Ai = A + ((long)item * g.naux_pad + a0) * ld;
    const double *Xi = X + ((long)item * g.naux_pad + a0) * ld;
    double *Ri = Rout + ((long)item * g.naux_pad + a0) * ld;
    const double *tab = MODE != KA_DIRECT ? p.tab + (long)item * g.maxstat * g.R : nullptr;
    const double *sig = MODE != KA_DIRECT ? p.sig + (long)item * g.maxcp * g.npts : nullptr;
    int col[CPT], q2[CPT];
    double t2[CPT];
    bool live[CPT];
#pragma unroll
    for (int u = 0; u < CPT; ++u) {
        const int cidx = (blockIdx.x * CPT + u) * 64 + lane;
        live[u] = cidx < g.n0;
        col[u] = live[u] ? cidx : g.n0 - 1;
        t2[u] = p.t0[col[u]];
        q2[u] = MODE != KA_DIRECT ? p.qpts[col[u]] : 0;
    }
    const double diag = P.noise + sp.jitter;
    double acc[CPT][NACC];
#pragma unroll
    for (int u = 0; u < CPT; ++u)
#pragma unroll
        for (int s = 0; s < NACC; ++s) acc[u][s] = 0.0;
    const int per = (g.nb0 + 3) / 4;              // 64-row slabs per wave
    for (int sl = 0; sl < per; ++sl) {
        const int slab = w * per + sl;
        const bool on = slab < g.nb0;             // wave-uniform
        const int r0 = slab * NB;
        __syncthreads();
        if (on) {
            for (int e = lane; e < NACC * NB; e += 64) {
                const int a = e >> 6, rr = e & 63;
                As[w][a][rr] = (a < rows) ? Ai[(long)a * ld + r0 + rr] : 0.0;
            }
            t1s[w][lane] = p.t0[r0 + lane];
            q1s[w][lane] = MODE != KA_DIRECT ? p.qpts[r0 + lane] : 0;
        }
        __syncthreads();
        if (!on) continue;
        if constexpr (MODE == KA_CHAIN) {
            // chain programs: 8 rows per decode (chain_step), the rows' lattice data in LDS
            static_assert(MODE != KA_CHAIN || CPT == 1, "the chain instantiation is one column per thread");
            const int nops = P.n_rops;
            for (int r8 = 0; r8 < NB; r8 += 8) {
                struct {
                    const int *q1;
                    const double *t1;
                    int pt0;
                    __device__ __forceinline__ int q(int k) const { return q1[k]; }
                    __device__ __forceinline__ int pt(int k) const { return pt0 + k; }
                    __device__ __forceinline__ double t(int k) const { return t1[k]; }
                } rows = {&q1s[w][r8], &t1s[w][r8], r0 + r8};
                double v[8][1];
                for (int i = 0; i < nops; ++i)
                    chain_step<8, 1>(P, i, tab, sig, g.R, g.npts, rows, q2, t2, col, v);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    double vv = v[k][0];
                    if (r0 + r8 + k == col[0]) vv += diag;
#pragma unroll
                    for (int s = 0; s < NACC; ++s) acc[0][s] += As[w][s][r8 + k] * vv;
                }
            }
            continue;
        }
#pragma unroll SINGLE ? 8 : 1
        for (int rr = 0; rr < NB; ++rr) {
            const int row = r0 + rr;
#pragma unroll
            for (int u = 0; u < CPT; ++u) {
                double v;
                if constexpr (SINGLE)
                    v = tab[abs(q1s[w][rr] - q2[u])];
                else if constexpr (MODE == KA_REDUCED)
                    v = keval_reduced(P, tab, sig, g.R, g.npts, t1s[w][rr], t2[u],
                                      abs(q1s[w][rr] - q2[u]), row, col[u]);
                else
                    v = keval(P, sp, t1s[w][rr], t2[u]);
                if (row == col[u]) v += diag;
#pragma unroll
                for (int s = 0; s < NACC; ++s) acc[u][s] += As[w][s][rr] * v;
            }
        }
    }
    __syncthreads();
    if (w > 0) {
#pragma unroll
        for (int u = 0; u < CPT; ++u)
#pragma unroll
            for (int s = 0; s < NACC; ++s) red[w - 1][u][s][lane] = acc[u][s];
    }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int u = 0; u < CPT; ++u)
        if (live[u]) {
#pragma unroll
            for (int s = 0; s < NACC; ++s)   // static index: a runtime bound sends acc[] to scratch
                if (s < rows) {
                    const double sum = ((acc[u][s] + red[0][u][s][lane]) + red[1][u][s][lane]) +
                                       red[2][u][s][lane];
                    Ri[(long)s * ld + col[u]] = Xi[(long)s * ld + col[u]] - sum;
                }
        }
}

}  // namespace ngp
