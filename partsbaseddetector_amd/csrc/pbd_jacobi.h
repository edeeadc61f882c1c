// pbd_jacobi.h -- the cyclic Jacobi eigen-decomposition of a symmetric 3x3 in double, shared by the plane fit
// (pbd_kernels_planes.hip) and the part-centre poses (pbd_kernels_publish.hip).  include/pbd.h states it op by op; the numpy
// yardstick is pointcloud.jacobi3.  Every operation is an explicitly rounded intrinsic, so nothing is contracted.
#pragma once

#include <hip/hip_runtime.h>

namespace pbd {

constexpr int kJacobiSweeps = 8;

// kJacobiSweeps cyclic sweeps over (0,1), (0,2), (1,2) from V = I: A becomes (nearly) diagonal, V holds the eigenvectors as columns
__device__ inline void jacobi3(double A[3][3], double V[3][3])
{
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) V[i][k] = i == k ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep)
        for (int pr = 0; pr < 3; ++pr) {
            const int P = pr == 2 ? 1 : 0, Q = pr == 0 ? 1 : 2;     // (0,1), (0,2), (1,2)
            const double apq = A[P][Q];
            if (apq == 0.0) continue;
            const double theta = __ddiv_rn(__dsub_rn(A[Q][Q], A[P][P]), __dmul_rn(2.0, apq));
            double t = __ddiv_rn(1.0, __dadd_rn(fabs(theta), __dsqrt_rn(__dadd_rn(__dmul_rn(theta, theta), 1.0))));
            if (theta < 0.0) t = -t;
            const double cs = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dmul_rn(t, t), 1.0))), sn = __dmul_rn(t, cs);
            for (int k = 0; k < 3; ++k) {                           // A J
                const double akp = A[k][P], akq = A[k][Q];
                A[k][P] = __dsub_rn(__dmul_rn(cs, akp), __dmul_rn(sn, akq));
                A[k][Q] = __dadd_rn(__dmul_rn(sn, akp), __dmul_rn(cs, akq));
            }
            for (int k = 0; k < 3; ++k) {                           // J^T (A J)
                const double apk = A[P][k], aqk = A[Q][k];
                A[P][k] = __dsub_rn(__dmul_rn(cs, apk), __dmul_rn(sn, aqk));
                A[Q][k] = __dadd_rn(__dmul_rn(sn, apk), __dmul_rn(cs, aqk));
            }
            for (int k = 0; k < 3; ++k) {                           // V J
                const double vkp = V[k][P], vkq = V[k][Q];
                V[k][P] = __dsub_rn(__dmul_rn(cs, vkp), __dmul_rn(sn, vkq));
                V[k][Q] = __dadd_rn(__dmul_rn(sn, vkp), __dmul_rn(cs, vkq));
            }
        }
}

}  // namespace pbd
