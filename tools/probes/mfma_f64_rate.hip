// Probe: issue rate of v_mfma_f64_16x16x4_f64 on gfx950 (MI355X).  The guides have no row for this instruction and the
// 78.6 TFLOP/s fp64 matrix figure is the spec sheet's; this measures both:
//   1. one wave on one SIMD: back-to-back MFMAs on 8 independent accumulators, cycles per MFMA from s_memtime
//   2. the whole chip: every SIMD busy (one or two waves each), FLOP/s from hipEvent timing (2 * 16 * 16 * 4 per MFMA)
// Build: hipcc --offload-arch=gfx950 -O3 -o mfma_f64_rate mfma_f64_rate.hip ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kAcc = 8;

__global__ void k(int iters, double seed, double *out, long long *cycles)
{
    f64x4 acc[kAcc];
    for (int i = 0; i < kAcc; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double a = seed + threadIdx.x * 1e-3, b = seed - threadIdx.x * 1e-3;
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it)
#pragma unroll
        for (int i = 0; i < kAcc; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    const long long t1 = __builtin_amdgcn_s_memtime();
    double s = 0;
    for (int i = 0; i < kAcc; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) *cycles = t1 - t0;
}

int main()
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { std::printf("no device\n"); return 1; }
    const int ncu = prop.multiProcessorCount;
    double *out;
    long long *cyc;
    if (hipMalloc(&out, (size_t)ncu * 8 * 256 * sizeof(double)) || hipMalloc(&cyc, sizeof(long long))) { std::printf("hipMalloc failed\n"); return 1; }
    // 1. one wave
    for (int iters : {256, 4096}) {
        hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, iters, 1.0, out, cyc);
        long long c = 0;
        if (hipMemcpy(&c, cyc, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) { std::printf("kernel failed\n"); return 1; }
        std::printf("one wave, %d x %d MFMAs: %.2f s_memtime cycles per v_mfma_f64_16x16x4_f64\n", iters, kAcc, (double)c / ((double)iters * kAcc));
    }
    // 2. the chip: blocks of 256 threads (one wave per SIMD), one or two blocks per CU
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    const int iters = 20000;
    for (int per_cu : {1, 2}) {
        const int blocks = ncu * per_cu;
        hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, 64, 1.0, out, cyc);       // warm-up
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(k, dim3(blocks), dim3(256), 0, 0, iters, 1.0, out, cyc);
        (void)hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) { std::printf("kernel failed\n"); return 1; }
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        long long c = 0;
        (void)hipMemcpy(&c, cyc, sizeof c, hipMemcpyDeviceToHost);
        const double flop = (double)blocks * 4 * iters * kAcc * 2.0 * 16 * 16 * 4;
        std::printf("chip, %d CUs x %d wave(s) per SIMD: %.3f ms, %.1f TFLOP/s fp64; wave 0: %.2f s_memtime cycles per MFMA\n", ncu, per_cu, ms,
                    flop / (ms * 1e-3) / 1e12, (double)c / ((double)iters * kAcc));
    }
    return 0;
}
