// Probe: the operand / result layout of v_mfma_f64_16x16x4_f64 on gfx950, checked with exact integer data (every product
// and sum is an integer far below 2^53, so any misplaced element shows as a mismatch, not as rounding).
//   A: lane l holds A[l & 15][l >> 4]     B: lane l holds B[l >> 4][l & 15]     D: register r of lane l is D[(l >> 4) + 4 r][l & 15]
// B is asymmetric (B[k][j] != B[j][k]) so that a transposed result cannot pass.  Also counts how many results the f32
// 16x16 row formula (row = 4 (l >> 4) + r) would misplace.
// Build: hipcc --offload-arch=gfx950 -O2 -o mfma_f64_layout mfma_f64_layout.hip ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ void k(const double *A, const double *B, double *D)
{
    const int l = threadIdx.x;
    f64x4 c = {0.0, 0.0, 0.0, 0.0};
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(l & 15) * 4 + (l >> 4)], B[(l >> 4) * 16 + (l & 15)], c, 0, 0, 0);
    for (int r = 0; r < 4; ++r) D[l * 4 + r] = c[r];
}

int main()
{
    double A[64], B[64], want[256], got[256];
    for (int i = 0; i < 16; ++i)
        for (int k = 0; k < 4; ++k) A[i * 4 + k] = 1 + i + 17 * k;                 // A[i][k]
    for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 16; ++j) B[k * 16 + j] = 3 + 5 * j - 11 * k + j * k;  // B[k][j]
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += A[i * 4 + k] * B[k * 16 + j];
            want[i * 16 + j] = s;
        }
    double *dA, *dB, *dD;
    if (hipMalloc(&dA, sizeof A) || hipMalloc(&dB, sizeof B) || hipMalloc(&dD, sizeof got)) { std::printf("hipMalloc failed\n"); return 1; }
    (void)hipMemcpy(dA, A, sizeof A, hipMemcpyHostToDevice);
    (void)hipMemcpy(dB, B, sizeof B, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, dA, dB, dD);
    if (hipMemcpy(got, dD, sizeof got, hipMemcpyDeviceToHost) != hipSuccess) { std::printf("kernel failed\n"); return 1; }
    int bad = 0, bad_f32_rows = 0;
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 4; ++r) {
            const int col = l & 15;
            if (got[l * 4 + r] != want[((l >> 4) + 4 * r) * 16 + col]) ++bad;
            if (got[l * 4 + r] != want[(4 * (l >> 4) + r) * 16 + col]) ++bad_f32_rows;
        }
    std::printf("v_mfma_f64_16x16x4_f64: %d of 256 results differ from row = (lane>>4) + 4*reg, col = lane&15 (%s); "
                "the f32 row formula 4*(lane>>4) + reg would misplace %d\n", bad, bad ? "LAYOUT WRONG" : "layout ok", bad_f32_rows);
    return bad ? 1 : 0;
}
