// ngp_path_kernels.h — functionals of whole sample paths of a Gaussian mixture, on the original
// scale (ngp_mixture_path_targets / _indep, include/ngp.h).  Included by ngp_kernels.hip behind
// philox4x32_10, u01 and small_chol_kernel, which it uses as they are: path (s, d) is the path
// mixture_sample_kernel draws — same counters, same component pick, same Box-Muller pairing, and
// the same order of the sum  mu_i + L_i0 z_0 + L_i1 z_1 + ...
//
// No path ever reaches HBM: only its T target values do, and from those only a few hundred numbers
// go back to the host.
//
//   path_pick_kernel      one thread per path: the component from Philox block 0 (the sampler's
//                         loop over the weights), its bucket (the component; with independent
//                         mixtures the pair (scenario, component)) and its rank inside the bucket
//                         from an integer atomic — the order inside a bucket may differ from call
//                         to call, nothing below depends on it
//   path_scan_kernel      one workgroup: where every bucket starts in the sorted order and the
//                         first workgroup of path_values_kernel that works on it
//   path_scatter_kernel   order[start of bucket + rank] = path
//   path_values_kernel    a workgroup takes up to PW paths of ONE bucket, a thread owns one path.
//                         The path's state lives in LDS as [date][path] (lane-contiguous: no bank
//                         conflicts); L is staged PATH_LCHUNK doubles of whole rows at a time, from
//                         the last rows up, and read as a broadcast.  Row i only needs z_0 .. z_i,
//                         so working upwards  v_i = g(x_i)  overwrites z_i in place.  Then every
//                         target walks its window of v in LDS and ONE double per (target, path) is
//                         written, at the path's own index (so every later sum runs in path order).
//                         mu is not staged: in the shared form every path of a bucket has its
//                         own scenario's row, so a thread reads its m means from global memory
//                         (L2) inside the row loop.
//   path_reduce_kernel / path_reduce_final_kernel
//                         mean: a slice's total in a fixed order, then the slices' totals in slice
//                         order — no floating-point atomics; count and the peak histogram are
//                         integers, added with integer atomics
//   path_select_*         exact order statistics by radix select on order-preserving 64-bit keys:
//                         eight passes of 8-bit digits over values[t]; ALL levels of a target
//                         share a pass.  Levels are worked in ascending rank, so the key prefixes
//                         they have fixed so far are ascending too and the levels with equal prefix
//                         form runs ("groups", one histogram each); an element finds its group by
//                         bisection.  Histograms are built in LDS and merged with integer atomics.
//                         Ties need nothing special — a digit is chosen by counts — and the common
//                         tie (a clamp puts a whole wave at exactly 0) costs one LDS atomic per
//                         wave instead of 64 on one address.
#pragma once
#include <atomic>

#include "ngp_internal.h"

namespace ngp {

constexpr int PATH_THREADS = 256;

// ---- the inverse transformations (nowcast.get_transformations), edge rules included ----------
// numpy's maximum / minimum hand a NaN on; fmax / fmin would drop it
__device__ __forceinline__ double path_max_nan(double a, double b) { return a != a ? a : fmax(a, b); }
__device__ __forceinline__ double path_min_nan(double a, double b) { return a != a ? a : fmin(a, b); }

__device__ __forceinline__ double path_inv(const ngp_inv_transform &t, double x) {
    double r = x;
    if (t.kind == NGP_INV_EXP) {
        r = path_max_nan(exp(x) - t.offset, 0.0);
    } else if (t.kind == NGP_INV_LOGISTIC100) {
        r = path_max_nan(100.0 / (1.0 + exp(-x)) - t.offset, 0.0);
    } else if (t.kind == NGP_INV_BOXCOX) {
        const double base = t.lam * x + 1.0;
        if (t.lam > 0.0) {
            r = pow(path_max_nan(base, 1.0e-10), 1.0 / t.lam) - t.offset;
        } else if (t.lam < 0.0) {
            if (base > 1.0e-10) r = pow(base, 1.0 / t.lam) - t.offset;
            else if (base <= 0.0) r = 0.0;                       // beyond the pole: mass at zero
            else r = path_min_nan(pow(base, 1.0 / t.lam), t.cap) - t.offset;
        } else {
            r = exp(x) - t.offset;
        }
        r = path_max_nan(r, 0.0);
        if (!(fabs(r) <= 1.79769313486231570815e308)) r = 1.79769313486231570815e308;   // non-finite
    }
    return r + 0.0;      // -0.0 is stored as +0.0
}

// order-preserving map double -> uint64 (negative: all bits flipped, else the sign bit set)
__device__ __forceinline__ unsigned long long path_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double path_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)b);
}

// ---- (a) pick and counting sort ----------------------------------------------------------------
__global__ __launch_bounds__(PATH_THREADS) void path_pick_kernel(
    int P, int draws, long N, const double *w, unsigned k0, unsigned k1,
    const unsigned long long *seeds, int32_t *bkt, uint32_t *rank, uint32_t *cnt) {
    const long idx = (long)blockIdx.x * PATH_THREADS + threadIdx.x;
    if (idx >= N) return;
    const int s = (int)(idx / draws), d = (int)(idx % draws);
    unsigned cs = (unsigned)s;
    if (seeds) {
        k0 = (unsigned)seeds[s];
        k1 = (unsigned)(seeds[s] >> 32);
        cs = 0u;
    }
    const Philox4 r0 = philox4x32_10(Philox4{(unsigned)d, cs, 0u, 0u}, k0, k1);
    const double u = u01(r0.x, r0.y);
    const double *ws = w + (long)s * P;
    int k = P - 1;
    double acc = 0.0;
    for (int i = 0; i < P; ++i) {
        acc += ws[i];
        if (u < acc) { k = i; break; }
    }
    const int b = seeds ? s * P + k : k;
    bkt[idx] = b;
    rank[idx] = atomicAdd(&cnt[b], 1u);
}

// off [B + 1]: exclusive running sum of cnt; wgoff [B + 1]: of ceil(cnt / PW)
__global__ __launch_bounds__(PATH_THREADS) void path_scan_kernel(int B, int PW, const uint32_t *cnt,
                                                                 uint32_t *off, uint32_t *wgoff) {
    __shared__ uint32_t sa[PATH_THREADS], sb[PATH_THREADS], carry[2];
    const int tid = threadIdx.x;
    if (tid < 2) carry[tid] = 0u;
    __syncthreads();
    for (int base = 0; base < B; base += PATH_THREADS) {
        const int i = base + tid;
        const uint32_t c = i < B ? cnt[i] : 0u, g = (c + (uint32_t)PW - 1u) / (uint32_t)PW;
        sa[tid] = c;
        sb[tid] = g;
        __syncthreads();
        for (int o = 1; o < PATH_THREADS; o <<= 1) {
            const uint32_t a = tid >= o ? sa[tid - o] : 0u, b = tid >= o ? sb[tid - o] : 0u;
            __syncthreads();
            sa[tid] += a;
            sb[tid] += b;
            __syncthreads();
        }
        if (i < B) {
            off[i] = carry[0] + sa[tid] - c;
            wgoff[i] = carry[1] + sb[tid] - g;
        }
        __syncthreads();
        if (tid == PATH_THREADS - 1) {
            carry[0] += sa[tid];
            carry[1] += sb[tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        off[B] = carry[0];
        wgoff[B] = carry[1];
    }
}

__global__ __launch_bounds__(PATH_THREADS) void path_scatter_kernel(long N, const int32_t *bkt,
                                                                    const uint32_t *rank,
                                                                    const uint32_t *off,
                                                                    int32_t *order) {
    const long idx = (long)blockIdx.x * PATH_THREADS + threadIdx.x;
    if (idx < N) order[off[bkt[idx]] + rank[idx]] = (int32_t)idx;
}

// ---- (b) paths -> target values ----------------------------------------------------------------
// blockDim = g.PW; dynamic LDS: PATH_LCHUNK doubles of L, then the state [m][PW]
__global__ __launch_bounds__(PATH_THREADS) void path_values_kernel(
    PathGeom g, const double *mu, const double *chol, unsigned k0, unsigned k1,
    const unsigned long long *seeds, ngp_inv_transform inv, const uint32_t *off,
    const uint32_t *wgoff, const int32_t *order, const ngp_path_target *targets, double *values) {
    extern __shared__ double path_lds[];
    double *Lc = path_lds, *st = path_lds + PATH_LCHUNK;
    const int tid = threadIdx.x, PW = g.PW, m = g.m;
    const uint32_t wg = blockIdx.x;
    if (wg >= wgoff[g.B]) return;                  // the grid is an upper bound
    int lo = 0, hi = g.B;                          // first bucket whose wgoff is beyond wg, minus one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (wgoff[mid] <= wg) lo = mid + 1; else hi = mid;
    }
    const int b = lo - 1;
    const uint32_t first = off[b] + (wg - wgoff[b]) * (uint32_t)PW;
    const uint32_t left = off[b + 1] - first;
    const bool active = (uint32_t)tid < left;
    const long p = active ? (long)order[first + tid] : 0l;
    const int s = (int)(p / g.draws), d = (int)(p % g.draws);
    unsigned cs = (unsigned)s;
    if (seeds) {
        k0 = (unsigned)seeds[s];
        k1 = (unsigned)(seeds[s] >> 32);
        cs = 0u;
    }
    if (active) {
        // blocks 1..: four words -> one Box-Muller pair -> two normals (mixture_sample_kernel)
        for (int j0 = 0; j0 < m; j0 += 2) {
            const Philox4 r = philox4x32_10(Philox4{(unsigned)d, cs, (unsigned)(1 + j0 / 2), 0u},
                                            k0, k1);
            const double u1 = u01(r.x, r.y), u2 = u01(r.z, r.w);
            const double rad = sqrt(-2.0 * log(u1)), ang = 2.0 * M_PI * u2;
            st[j0 * PW + tid] = rad * cos(ang);
            if (j0 + 1 < m) st[(j0 + 1) * PW + tid] = rad * sin(ang);
        }
    }
    const double *L = chol + (long)b * m * m;
    const int k = g.indep ? b - s * g.P : b;
    const double *mk = mu + (g.indep ? (long)b : (long)k * g.S + s) * m;
    const int R = PATH_LCHUNK / m;                 // whole rows per staged chunk (m <= 192: >= 10)
    for (int i1 = m; i1 > 0; i1 -= R) {
        const int i0 = i1 > R ? i1 - R : 0;
        __syncthreads();                           // the chunk before this one is done with
        for (int e = tid; e < (i1 - i0) * m; e += PW) Lc[e] = L[(long)i0 * m + e];
        __syncthreads();
        if (active) {
            for (int i = i1 - 1; i >= i0; --i) {
                const double *row = Lc + (i - i0) * m;
                double acc = mk[i];
                for (int j = 0; j <= i; ++j) acc += row[j] * st[j * PW + tid];
                st[i * PW + tid] = path_inv(inv, acc);          // z_i is not needed above row i
            }
        }
    }
    if (!active) return;
    for (int t = 0; t < g.T; ++t) {
        const ngp_path_target tg = targets[t];
        double val;
        if (tg.kind == NGP_TARGET_DIFF) {
            val = st[tg.j1 * PW + tid] - st[tg.j0 * PW + tid];
        } else if (tg.kind == NGP_TARGET_SUM) {
            val = 0.0;
            for (int j = tg.j0; j <= tg.j1; ++j) val += st[j * PW + tid];
        } else {
            double best = st[tg.j0 * PW + tid];
            int arg = tg.j0;
            for (int j = tg.j0 + 1; j <= tg.j1; ++j) {
                const double v = st[j * PW + tid];
                if (v > best || (best != best && v == v)) { best = v; arg = j; }
            }
            val = tg.kind == NGP_TARGET_MAX ? best
                  : tg.kind == NGP_TARGET_ARGMAX ? (double)arg : (best > tg.thr ? 1.0 : 0.0);
        }
        values[(long)t * g.N + p] = val + 0.0;
    }
}

// ---- (d) mean, count, peak histogram -----------------------------------------------------------
// grid (slices, T): partial [T][slices]
__global__ __launch_bounds__(PATH_THREADS) void path_reduce_kernel(
    long N, int m, const ngp_path_target *targets, const double *values, double *partial,
    unsigned long long *count, unsigned long long *hist) {
    __shared__ double sh[PATH_THREADS / 64];
    __shared__ unsigned hs[NGP_MAX_AUX], cs[PATH_THREADS / 64];
    const int t = blockIdx.y, tid = threadIdx.x;
    const ngp_path_target tg = targets[t];
    const double *v = values + (long)t * N;
    const bool peak = tg.kind == NGP_TARGET_ARGMAX;
    if (peak) {
        for (int j = tid; j < m; j += PATH_THREADS) hs[j] = 0u;
        __syncthreads();
    }
    const long base = (long)blockIdx.x * PATH_SLICE;
    double acc = 0.0;
    unsigned c = 0u;
    for (int r = 0; r < PATH_SLICE / PATH_THREADS; ++r) {
        const long i = base + tid + (long)r * PATH_THREADS;
        if (i >= N) break;
        const double x = v[i];
        acc += x;
        if (peak) {
            if (x >= 0.0 && x < (double)m) atomicAdd(&hs[(int)x], 1u);
        } else if (tg.kind == NGP_TARGET_EXCEED) {
            c += x > 0.5 ? 1u : 0u;
        } else {
            c += x > tg.thr ? 1u : 0u;
        }
    }
    const double tot = mix_block_sum(acc, sh);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((tid & 63) == 0) cs[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        partial[(long)t * gridDim.x + blockIdx.x] = tot;
        const unsigned ct = cs[0] + cs[1] + cs[2] + cs[3];
        if (ct) atomicAdd(&count[t], (unsigned long long)ct);
    }
    if (peak)
        for (int j = tid; j < m; j += PATH_THREADS)
            if (hs[j]) atomicAdd(&hist[(long)t * m + j], (unsigned long long)hs[j]);
}

// grid (T)
__global__ __launch_bounds__(PATH_THREADS) void path_reduce_final_kernel(long N, long slices,
                                                                         const double *partial,
                                                                         double *mean) {
    __shared__ double sh[PATH_THREADS / 64];
    const int t = blockIdx.x;
    double acc = 0.0;
    for (long i = threadIdx.x; i < slices; i += PATH_THREADS) acc += partial[(long)t * slices + i];
    const double tot = mix_block_sum(acc, sh);
    if (threadIdx.x == 0) mean[t] = tot / (double)N;
}

// ---- (c) selection -----------------------------------------------------------------------------
// per real-valued target y (of Tr) and rank r (of R, ascending): prefix [Tr][R] the key bits fixed
// so far, krem [Tr][R] the rank left inside them, grp [Tr][R] the rank's group, gpre [Tr][R] the
// groups' prefixes (ng [Tr] of them), ghist [Tr][R][256]
__global__ __launch_bounds__(64) void path_select_init_kernel(int R, const long long *ranks,
                                                              unsigned long long *prefix,
                                                              long long *krem, int32_t *grp,
                                                              unsigned long long *gpre,
                                                              int32_t *ng) {
    const int y = blockIdx.x, i = threadIdx.x;
    if (i < R) {
        prefix[y * R + i] = 0ull;
        krem[y * R + i] = ranks[i];
        grp[y * R + i] = 0;
        gpre[y * R + i] = 0ull;
    }
    if (i == 0) ng[y] = 1;
}

// grid (slices, Tr), dynamic LDS: R x 256 counters
__global__ __launch_bounds__(PATH_THREADS) void path_select_hist_kernel(
    long N, int R, int pass, const int32_t *real, const double *values,
    const unsigned long long *gpre, const int32_t *ng, uint32_t *ghist) {
    extern __shared__ unsigned path_hist[];
    __shared__ unsigned long long gp[PATH_MAX_LEVELS];
    const int y = blockIdx.y, tid = threadIdx.x;
    const int G = ng[y];
    const double *v = values + (long)real[y] * N;
    for (int e = tid; e < G * 256; e += PATH_THREADS) path_hist[e] = 0u;
    if (tid < G) gp[tid] = gpre[y * R + tid];
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const long base = (long)blockIdx.x * PATH_SLICE;
    for (int r = 0; r < PATH_SLICE / PATH_THREADS; ++r) {
        const long i = base + tid + (long)r * PATH_THREADS;
        int bin = -1;
        if (i < N) {
            const unsigned long long key = path_key(v[i]);
            const unsigned long long hi = pass ? key >> (shift + 8) : 0ull;
            int lo = 0, up = G;                    // first group whose prefix is not below hi
            while (lo < up) {
                const int mid = (lo + up) >> 1;
                if (gp[mid] < hi) lo = mid + 1; else up = mid;
            }
            if (lo < G && gp[lo] == hi) bin = lo * 256 + (int)((key >> shift) & 255ull);
        }
        // a whole wave in one bin (a clamp at 0, a constant target): one add instead of 64
        const int lead = __shfl(bin, 0, 64);
        if (__all(bin == lead)) {
            if ((tid & 63) == 0 && bin >= 0) atomicAdd(&path_hist[bin], 64u);
        } else if (bin >= 0) {
            atomicAdd(&path_hist[bin], 1u);
        }
    }
    __syncthreads();
    for (int e = tid; e < G * 256; e += PATH_THREADS)
        if (path_hist[e]) atomicAdd(&ghist[(long)y * R * 256 + e], path_hist[e]);
}

// grid (Tr): every rank takes the digit its count falls into, then the groups are formed again
__global__ __launch_bounds__(PATH_THREADS) void path_select_step_kernel(
    int R, int pass, unsigned long long *prefix, long long *krem, int32_t *grp,
    unsigned long long *gpre, int32_t *ng, uint32_t *ghist, double *q) {
    const int y = blockIdx.x, tid = threadIdx.x;
    uint32_t *h = ghist + (long)y * R * 256;
    if (tid < R) {
        const uint32_t *hg = h + grp[y * R + tid] * 256;
        long long k = krem[y * R + tid], cum = 0;
        int digit = 255;
        for (int dg = 0; dg < 256; ++dg) {
            const long long c = (long long)hg[dg];
            if (cum + c >= k) { digit = dg; break; }
            cum += c;
        }
        krem[y * R + tid] = k - cum;
        const unsigned long long pf = (prefix[y * R + tid] << 8) | (unsigned long long)digit;
        prefix[y * R + tid] = pf;
        if (pass == 7) q[y * R + tid] = path_unkey(pf);
    }
    __syncthreads();
    for (int e = tid; e < R * 256; e += PATH_THREADS) h[e] = 0u;
    if (tid == 0) {
        int n = 0;
        for (int i = 0; i < R; ++i) {
            const unsigned long long pf = prefix[y * R + i];
            if (i == 0 || pf != gpre[y * R + n - 1]) gpre[y * R + n++] = pf;
            grp[y * R + i] = n - 1;
        }
        ng[y] = n;
    }
}

// ---- launcher ----------------------------------------------------------------------------------
// The first error of a memset or of raising a kernel's LDS limit is returned (nothing is launched
// behind it: a histogram that was not cleared would give counts that look right).  The two limits
// are raised once per device: path_values_kernel up to PATH_LDS_MAX, path_select_hist_kernel to
// its 64 counters x 1 KiB of dynamic LDS, which with the 512 B of static gp[] is past the 64 KiB a
// kernel gets without asking.
hipError_t launch_path_targets(const PathGeom &g, const PathBufs &p, const ngp_inv_transform &inv,
                               uint64_t seed, hipStream_t s) {
    static std::atomic<unsigned long long> lds_raised{0ull};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(lds_raised.load(std::memory_order_acquire) & bit)) {
        e = hipFuncSetAttribute((const void *)path_values_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, PATH_LDS_MAX);
        if (e == hipSuccess)
            e = hipFuncSetAttribute((const void *)path_select_hist_kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, PATH_MAX_LEVELS * 1024);
        if (e != hipSuccess) return e;
        lds_raised.fetch_or(bit, std::memory_order_release);
    }
    if ((e = hipMemsetAsync(p.cnt, 0, 4 * (size_t)g.B, s)) != hipSuccess ||
        (e = hipMemsetAsync(p.count, 0, 8 * (size_t)g.T, s)) != hipSuccess ||
        (e = hipMemsetAsync(p.hist, 0, 8 * (size_t)g.T * g.m, s)) != hipSuccess ||
        (g.Tr && (e = hipMemsetAsync(p.ghist, 0, 4 * (size_t)g.Tr * g.R * 256, s)) != hipSuccess))
        return e;
    const long mats = g.B;
    hipLaunchKernelGGL(small_chol_kernel, dim3((unsigned)mats), dim3(256), 0, s, p.chol, g.m, p.info);
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const unsigned nb = (unsigned)((g.N + PATH_THREADS - 1) / PATH_THREADS);
    const auto *seeds = (const unsigned long long *)p.seeds;
    hipLaunchKernelGGL(path_pick_kernel, dim3(nb), dim3(PATH_THREADS), 0, s, g.P, g.draws, (long)g.N,
                       p.w, k0, k1, seeds, p.bkt, p.rank, p.cnt);
    hipLaunchKernelGGL(path_scan_kernel, dim3(1), dim3(PATH_THREADS), 0, s, g.B, g.PW,
                       (const uint32_t *)p.cnt, p.off, p.wgoff);
    hipLaunchKernelGGL(path_scatter_kernel, dim3(nb), dim3(PATH_THREADS), 0, s, (long)g.N,
                       (const int32_t *)p.bkt, (const uint32_t *)p.rank, (const uint32_t *)p.off,
                       p.order);
    hipLaunchKernelGGL(path_values_kernel, dim3((unsigned)path_values_grid(g.N, g.B, g.PW)),
                       dim3(g.PW), path_lds_bytes(g.m, g.PW), s, g, p.mu, (const double *)p.chol, k0,
                       k1, seeds, inv, (const uint32_t *)p.off, (const uint32_t *)p.wgoff,
                       (const int32_t *)p.order, p.targets, p.values);
    const long slices = path_slices(g.N);
    hipLaunchKernelGGL(path_reduce_kernel, dim3((unsigned)slices, g.T), dim3(PATH_THREADS), 0, s,
                       (long)g.N, g.m, p.targets, (const double *)p.values, p.partial, p.count,
                       p.hist);
    hipLaunchKernelGGL(path_reduce_final_kernel, dim3(g.T), dim3(PATH_THREADS), 0, s, (long)g.N,
                       slices, (const double *)p.partial, p.mean);
    if (g.Tr == 0) return hipSuccess;
    hipLaunchKernelGGL(path_select_init_kernel, dim3(g.Tr), dim3(64), 0, s, g.R,
                       (const long long *)p.ranks, p.prefix, p.krem, p.grp, p.gpre, p.ng);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(path_select_hist_kernel, dim3((unsigned)slices, g.Tr), dim3(PATH_THREADS),
                           (size_t)g.R * 1024, s, (long)g.N, g.R, pass, p.real,
                           (const double *)p.values, (const unsigned long long *)p.gpre,
                           (const int32_t *)p.ng, p.ghist);
        hipLaunchKernelGGL(path_select_step_kernel, dim3(g.Tr), dim3(PATH_THREADS), 0, s, g.R, pass,
                           p.prefix, p.krem, p.grp, p.gpre, p.ng, p.ghist, p.q);
    }
    return hipSuccess;
}

}  // namespace ngp
