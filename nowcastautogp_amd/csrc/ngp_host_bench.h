// ngp_host_bench.h — microbenchmarks and self-tests behind the C-ABI: ngp_microbench_mfma_f64 /
// _detail, ngp_microbench_hbm, ngp_selftest_mfma_layout / _f32_layout.
// Included from ngp_api.hip behind that file's own code (HIPCHK, ScopedEvent, ngp_ctx's stream,
// DevCall) and the probe launchers of ngp_internal.h (launch_mfma_bench*, launch_stream_*,
// launch_mfma_*_probe); last, nothing needs it.
#pragma once

// ---------------------------------------------------------------------------------------
// microbenchmarks / self tests
// ---------------------------------------------------------------------------------------
extern "C" ngp_status ngp_microbench_mfma_f64(ngp_ctx *c, int32_t iters, double *tflops) {
    if (!c || !tflops || iters <= 0) return NGP_ERR_ARG;
    DevCall call(c);
    iters = (iters + 3) / 4 * 4;
    const int blocks = 256 * 4;  // 4 workgroups of 4 waves per CU
    double *out = nullptr;
    call.take(&out, (size_t)blocks * 256);
    ScopedEvent a, b;
    call.run([&] {
            launch_mfma_bench(out, iters, blocks, c->stream);  // warm-up
            return hipEventRecord(a, c->stream);
        })
        .run([&] {
            launch_mfma_bench(out, iters, blocks, c->stream);
            return hipEventRecord(b, c->stream);
        });
    if (call.sync()) return call.status();
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    *tflops = (double)blocks * 4.0 * (double)iters * 2048.0 / ((double)ms * 1e-3) * 1e-12;
    return NGP_OK;
}

// out[0] TFLOP/s (wall), out[1] median shader cycles per MFMA per wave, out[2] median effective
// shader clock in GHz (s_memtime / s_memrealtime), out[3] waves per SIMD used
extern "C" ngp_status ngp_microbench_mfma_f64_detail(ngp_ctx *c, int32_t iters,
                                                     int32_t blocks_per_cu, double *out) {
    if (!c || !out || iters <= 0 || blocks_per_cu <= 0 || blocks_per_cu > 8) return NGP_ERR_ARG;
    iters = (iters + 3) / 4 * 4;
    const int blocks = 256 * blocks_per_cu;
    const int waves = blocks * 4;
    std::vector<unsigned long long> h(2 * (size_t)waves);
    DevCall call(c);
    unsigned long long *stamps = nullptr;
    call.take(&stamps, 2 * (size_t)waves);
    ScopedEvent a, b;
    call.run([&] {
            launch_mfma_bench_detail(stamps, iters, blocks, c->stream);
            return hipEventRecord(a, c->stream);
        })
        .run([&] {
            launch_mfma_bench_detail(stamps, iters, blocks, c->stream);
            return hipEventRecord(b, c->stream);
        })
        .down(h.data(), stamps, sizeof(unsigned long long) * h.size());
    if (call.sync()) return call.status();
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    std::vector<double> cyc((size_t)waves), ghz((size_t)waves);
    for (int w = 0; w < waves; ++w) {
        cyc[(size_t)w] = (double)h[2 * (size_t)w] / (double)iters;
        ghz[(size_t)w] = (double)h[2 * (size_t)w] / ((double)h[2 * (size_t)w + 1] * 10.0);
    }
    std::nth_element(cyc.begin(), cyc.begin() + waves / 2, cyc.end());
    std::nth_element(ghz.begin(), ghz.begin() + waves / 2, ghz.end());
    out[0] = (double)waves * (double)iters * 2048.0 / ((double)ms * 1e-3) * 1e-12;
    out[1] = cyc[(size_t)waves / 2];
    out[2] = ghz[(size_t)waves / 2];
    out[3] = (double)blocks_per_cu;
    return NGP_OK;
}

extern "C" ngp_status ngp_microbench_hbm(ngp_ctx *c, int64_t bytes, double *write_gbs,
                                         double *copy_gbs) {
    if (!c || bytes < 4096) return NGP_ERR_ARG;
    DevCall call(c);
    const int64_t n = bytes / 16 * 2;
    double *a = nullptr, *b = nullptr;
    call.take(&a, (size_t)n).take(&b, (size_t)n);
    ScopedEvent e0, e1, e2;
    call.run([&] {
            launch_stream_write(a, n, c->stream);
            launch_stream_copy(b, a, n, c->stream);
            return hipEventRecord(e0, c->stream);
        })
        .run([&] {
            launch_stream_write(a, n, c->stream);
            return hipEventRecord(e1, c->stream);
        })
        .run([&] {
            launch_stream_copy(b, a, n, c->stream);
            return hipEventRecord(e2, c->stream);
        });
    if (call.sync()) return call.status();
    float w = 0.f, cp = 0.f;
    HIPCHK(hipEventElapsedTime(&w, e0, e1));
    HIPCHK(hipEventElapsedTime(&cp, e1, e2));
    if (write_gbs) *write_gbs = (double)n * 8.0 / ((double)w * 1e-3) * 1e-9;
    if (copy_gbs) *copy_gbs = 2.0 * (double)n * 8.0 / ((double)cp * 1e-3) * 1e-9;
    return NGP_OK;
}

// D[0:256]   = A(16x4) B(4x16) through one v_mfma_f64_16x16x4_f64 using the operand maps the
//              kernels assume
// D[256:512] = the same product through four DPP-rotated v_mfma_f64_4x4x4_4b_f64 + the gather back
//              to the 16x16x4 C/D layout (the fast path of the k-loops)
// The caller compares both with A @ B on asymmetric data — tests/test_gpu_parity.py.
extern "C" ngp_status ngp_selftest_mfma_layout(ngp_ctx *c, const double *A, const double *Bm,
                                               double *D) {
    if (!c || !A || !Bm || !D) return NGP_ERR_ARG;
    DevCall call(c);
    double *da = nullptr, *db = nullptr, *dd = nullptr;
    call.take(&da, 64).take(&db, 64).take(&dd, 512);
    call.up(da, A, 64 * 8)
        .up(db, Bm, 64 * 8)
        .run([&] { launch_mfma_layout_probe(da, db, dd, c->stream); })
        .down(D, dd, 512 * 8);
    return call.sync();
}

// D (32 x 32, row-major) = A (32 x 2) B (2 x 32) through one v_mfma_f32_32x32x2_f32 with the operand
// and result maps the mixed-precision k-loop assumes; the caller compares with A @ B.
extern "C" ngp_status ngp_selftest_mfma_f32_layout(ngp_ctx *c, const float *A, const float *Bm,
                                                   float *D) {
    if (!c || !A || !Bm || !D) return NGP_ERR_ARG;
    DevCall call(c);
    float *da = nullptr, *db = nullptr, *dd = nullptr;
    call.take(&da, 64).take(&db, 64).take(&dd, 1024);
    call.up(da, A, 64 * 4)
        .up(db, Bm, 64 * 4)
        .run([&] { launch_mfma_f32_probe(da, db, dd, c->stream); })
        .down(D, dd, 1024 * 4);
    return call.sync();
}
