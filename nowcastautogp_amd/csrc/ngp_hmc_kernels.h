// ngp_hmc_kernels.h — the leapfrog step of an HMC trajectory between two gradient evaluations
// (ngp_grad_job_hmc).  Included from ngp_kernels.hip.
//
// One wave per item, four items per 256-thread workgroup.  Lane l owns the item's latents l and
// l + 64 in the CALLER's order (an item has at most NGP_MAX_PARAMS + 1 = 97); HmcDev::slot maps a
// latent to where the evaluation kernels keep it (DevProgram::params[slot], the row of d_grad; the
// noise, an item's last latent, is slot n_params).  Nothing crosses a wave: no LDS, no barrier, no
// atomics; every store is a plain vector store by the lane that owns the element.
//
// Arithmetic contract.  The update is the one of autogp._hmc_move / potential, operation for
// operation, every product and sum rounded on its own: each function below switches contraction
// off (#pragma clang fp contract(off)), so no build fuses a multiply into the add that follows it.
// exp() is the only transcendental.  The three per-item sums (z'z, mom'mom or pm'pm) add a lane's
// two elements, then run a butterfly over lane distances 32, 16, 8, 4, 2, 1 — a fixed order,
// restated by tests/hmc_reference.py (wave_sum).
#pragma once
#include "ngp_internal.h"

namespace ngp {

__device__ __forceinline__ double hmc_wave_sum(double v) {
#pragma clang fp contract(off)
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

// theta and d theta / dz of one latent: gp.FlatTransform after potential's cleaning of z, followed
// by potential's domain clamps of theta (equal to the margins of gp.clip_flat)
__device__ __forceinline__ void hmc_theta(int kind, double z, double a, double b, double *theta,
                                          double *dtheta) {
#pragma clang fp contract(off)
    double zc = z;
    if (z != z) zc = 0.0;
    else if (z == INFINITY) zc = 50.0;
    else if (z == -INFINITY) zc = -50.0;
    double th, dth;
    if (kind == 0) {
        th = zc;
        dth = 1.0;
    } else if (kind <= 2) {
        double x = a + b * zc;
        x = fmin(fmax(x, -700.0), 700.0);
        const double e = exp(-fabs(x));
        const double sg = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
        const double ssg = (kind == 2 ? 2.0 : 1.0) * sg;
        th = ssg;
        dth = ssg * (1.0 - sg) * b;
    } else {
        double x = a + b * zc;
        x = fmin(fmax(x, -300.0), 300.0);
        const double v = exp(x);
        th = v;
        dth = v * b;
    }
    th = fmin(fmax(th, -1e6), 1e6);
    if (kind >= 3) th = fmax(th, 1e-12);
    else if (kind == 2) th = fmin(fmax(th, 1e-9), 2.0 - 1e-9);
    else if (kind == 1) th = fmin(fmax(th, 1e-9), 1.0 - 1e-9);
    *theta = th;
    *dtheta = dth;
}

__global__ __launch_bounds__(256) void hmc_step_kernel(const HmcDev a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= a.B) return;   // the whole wave leaves together
    const int o0 = a.off[item], nl = a.off[item + 1] - o0;   // nl - 1 parameters and the noise
    DevProgram *P = a.progs + item;
    const double *g = a.grad + (long)item * (NGP_MAX_PARAMS + 1);

    double z[2] = {0.0, 0.0}, pm[2] = {0.0, 0.0}, ga[2] = {0.0, 0.0}, th[2], dth[2];
    int kind[2] = {0, 0}, slot[2] = {0, 0};
    bool own[2], frozen[2] = {false, false};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = lane + 64 * h;
        own[h] = q < nl;
        if (own[h]) {
            z[h] = a.z[o0 + q];
            pm[h] = a.pm[o0 + q];
            kind[h] = a.kind[o0 + q];
            frozen[h] = a.frozen[o0 + q] != 0;
            slot[h] = a.slot[o0 + q];
            if (a.phase != HMC_INIT) ga[h] = g[slot[h]];
        }
        const int kd = kind[h];
        hmc_theta(kd, z[h], a.mu[kd], a.sigma[kd], &th[h], &dth[h]);
    }

    if (a.phase != HMC_INIT) {
        // the evaluation at z: ok, U and dU as potential() forms them
        const double lm = a.logml[item];
        const int info = a.info[item];
        const bool gbad = (own[0] && !isfinite(ga[0])) || (own[1] && !isfinite(ga[1]));
        const bool ok = info == 0 && isfinite(lm) && !__any(gbad);
        const double zz = hmc_wave_sum(z[0] * z[0] + z[1] * z[1]);
        const double U = ok ? -lm + 0.5 * zz : INFINITY;
        if (a.phase == HMC_FIRST) {
            const double mm = hmc_wave_sum(pm[0] * pm[0] + pm[1] * pm[1]);
            if (lane == 0) {
                a.U0[item] = U;
                a.K0[item] = 0.5 * mm;
            }
        }
        const double step = a.phase == HMC_MIDDLE ? a.eps : 0.5 * a.eps;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double dU = ok ? -ga[h] * dth[h] + z[h] : 0.0;
            if (frozen[h]) dU = 0.0;
            pm[h] = pm[h] - step * dU;
        }
        if (a.phase == HMC_LAST) {
            const double pp = hmc_wave_sum(pm[0] * pm[0] + pm[1] * pm[1]);
            if (lane == 0) {
                a.U1[item] = U;
                a.K1[item] = 0.5 * pp;
                a.lm1[item] = lm;
                a.info1[item] = info;
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (own[h]) {
                    a.pm[o0 + lane + 64 * h] = pm[h];
                    a.theta[o0 + lane + 64 * h] = th[h];
                }
            return;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            z[h] = z[h] + a.eps * pm[h];
            const int kd = kind[h];
            hmc_theta(kd, z[h], a.mu[kd], a.sigma[kd], &th[h], &dth[h]);
        }
    }
    // the parameters of the next evaluation, where its kernels read them
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (own[h]) {
            const int q = lane + 64 * h;
            if (a.phase != HMC_INIT) {
                a.z[o0 + q] = z[h];
                a.pm[o0 + q] = pm[h];
            }
            if (a.trace) a.trace[o0 + q] = z[h];
            if (q == nl - 1) P->noise = th[h];
            else P->params[slot[h]] = th[h];
        }
}

void launch_hmc_step(const HmcDev &a, hipStream_t s) {
    hipLaunchKernelGGL(hmc_step_kernel, dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, s, a);
}

}  // namespace ngp
