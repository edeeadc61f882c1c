// pbd_kernels_depth.hip -- opt-in 3-D box of each candidate record from a depth image (pbd_boxes3d): the first step of the
// callers' PointCloudClusterer::computeBoundingBoxes, Candidate::boundingBox3D(im, depth) (include/Candidate.hpp:140-216;
// include/PointCloudClusterer.hpp:53-77, cells/detect.cpp:224-255, ros/Node.cpp:183-206).
//
// One kernel, k_boxes3d, one workgroup per record (grid-stride over the records):
//   geometry   the nparts + 1 boxes: parts & frame, boundingBoxNorm() & frame (Candidate.hpp:117-130), scaled to the depth image
//   select     the values at the <= 800 ranks the resample reads, by an exact radix select over order-preserving uint32 keys (float_key) of
//              the valid samples, 4 bits per pass, 8 passes, every pass reading the boxes of the depth image in place.  Pass 0
//              also counts the samples (M) and the valid samples of the first non-empty box (the reference's early NaN box).
//              Histograms live in LDS, one row of 16 counters per needed rank (ranks that share a key prefix share a row)
//   resample   cv::resize(points, points, Size(1, 400)) INTER_LINEAR, float path (:186)
//   filter     cv::filter2D(points, dpoints, -1, dog), dog = filter2D(getGaussianKernel(35, 4, CV_32F), [-1 0 1]^T) (:190-194)
//   walk       from the median out, until |d| > 0.035 (:197-205)
// Nothing is gathered: no workspace grows with the number of samples, and a record of any size runs the same code.
// Every float / double multiply and add is written with an explicitly rounded intrinsic, so none of them is contracted.
#include "pbd_device.h"

#include <math.h>

#include <algorithm>

namespace pbd {
namespace {

constexpr int kB3Threads = 1024;
constexpr int kB3Waves = kB3Threads / 64;
constexpr int kB3Out = 400;                  // cv::Size(1, 400) (Candidate.hpp:186)
constexpr int kB3MaxRanks = 2 * kB3Out;      // r0 and r1 of every output row
constexpr int kB3Bits = 4, kB3Bins = 1 << kB3Bits, kB3Passes = 32 / kB3Bits;

// Mat_<float> assignment of one depth sample (8U / 16U exact, 64F rounded to nearest, 32F as is)
template <int D> __device__ inline float b3_load(const uint8_t *row, int x)
{
    if (D == kDepth8U) return (float)row[x];
    if (D == kDepth16U) return (float)reinterpret_cast<const uint16_t *>(row)[x];
    if (D == kDepth32F) return reinterpret_cast<const float *>(row)[x];
    return (float)reinterpret_cast<const double *>(row)[x];
}

struct B3Shared {
    union {
        uint32_t hist[kB3MaxRanks * kB3Bins];    // select: per needed rank, 16 counters of the next digit (row = first rank of its prefix)
        struct { float p[kB3Out], d[kB3Out]; };  // then: the resampled and the filtered points
    };
    uint32_t pre[kB3MaxRanks];                   // key bits resolved so far, per needed rank (non-decreasing)
    int rank[kB3MaxRanks];                       // the needed ranks, ascending, distinct
    union {
        int sy[kB3Out];                          // cvFloor(fy) per output row, while the ranks are merged
        int resid[kB3MaxRanks];                  // then: rank among the samples that share the prefix
    };
    int4 box[kB3MaxBoxes];                       // x, y, w, h in the depth image, the non-empty boxes in order
    int nbox, K;
    unsigned int M, first_valid;
};
static_assert(sizeof(B3Shared) <= 65536, "the select's LDS fits one workgroup's static limit");

// one pass over every box: the digit at `shift` of every valid sample whose key prefix (the bits above `shift + 4`) is a needed
// rank's prefix is counted in that prefix's row.  Pass 0 (all prefixes empty: one row) also counts M and the samples of box 0, the
// first non-empty box.
// Lanes of a wave that hit one counter add once (wave_add_by_key: neighbouring depth samples mostly share a digit).
template <int D>
__device__ void b3_pass(B3Shared &S, const Box3dFrame &fr, int shift, bool first_pass)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = first_pass ? 0 : S.K;
    const uint32_t lo_pre = first_pass ? 0u : S.pre[0], hi_pre = first_pass ? 0u : S.pre[K - 1];
    unsigned int nvalid = 0, nfirst = 0;
    for (int b = 0; b < S.nbox; ++b) {
        const int4 r = S.box[b];
        for (int y = wave; y < r.w; y += kB3Waves) {
            const uint8_t *row = fr.data + (size_t)(r.y + y) * (size_t)fr.pitch;
            for (int x0 = 0; x0 < r.z; x0 += 64) {
                const int x = x0 + lane;
                int slot = -1;
                if (x < r.z) {
                    const float v = b3_load<D>(row, r.x + x);
                    if (v != 0.f && !(v != v)) {       // the valid samples: neither 0 nor NaN, which float_key asks for
                        const uint32_t k = float_key(v);
                        const uint32_t kp = (uint32_t)((unsigned long long)k >> (shift + kB3Bits));
                        const int digit = (int)((k >> shift) & (kB3Bins - 1));
                        if (first_pass) {
                            ++nvalid;
                            if (b == 0) ++nfirst;
                            slot = digit;
                        } else if (kp >= lo_pre && kp <= hi_pre) {
                            const int i = lower_bound_i32(S.pre, K, kp);
                            if (i < K && S.pre[i] == kp) slot = i * kB3Bins + digit;
                        }
                    }
                }
                wave_add_by_key(S.hist, slot, slot >= 0);
            }
        }
    }
    if (first_pass) {
        nvalid = wave_sum(nvalid);
        nfirst = wave_sum(nfirst);
        if (lane == 0) {
            atomicAdd(&S.M, nvalid);
            atomicAdd(&S.first_valid, nfirst);
        }
    }
}

// fy of output row dy (cv::resize INTER_LINEAR: fy = (float)((dy + 0.5) * scale - 0.5), sy = cvFloor(fy), fy -= sy)
__device__ inline float b3_fy(int dy, double scale, int *sy)
{
    float fy = (float)__dadd_rn(__dmul_rn((double)dy + 0.5, scale), -0.5);
    const int s = (int)floorf(fy);
    *sy = s;
    return __fsub_rn(fy, (float)s);
}

template <int D>
__global__ __launch_bounds__(kB3Threads) void k_boxes3d(Boxes3dParams p)
{
    __shared__ B3Shared S;
    const int tid = threadIdx.x;
    const int n = payload_count(p.in, p.in_cap);
    const double qnan = qnan_d();
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t *r = p.in + 1 + (size_t)i * p.stride;
        double *out = p.out + 6 * (size_t)i;
        const long long f = (long long)r[kRecFrame] - p.frame_offset;
        const int np = r[kRecNparts];
        if (f < 0 || f >= p.nframes || np < 1 || np > p.max_parts) {   // not a record of this call: six NaNs
            if (tid < 6) out[tid] = qnan;
            continue;
        }
        const Box3dFrame fr = p.frames[(int)f];
        // ---- geometry (one thread: a few dozen boxes)
        if (tid == 0) {
            const long long cols = fr.im_cols, rows = fr.im_rows;
            const double sx = (double)fr.cols / (double)cols, sy = (double)fr.rows / (double)rows;
            // boundingBoxNorm: centroid = cvRound((tl + br) * 0.5) (half to even), cv::meanStdDev in double
            double s[2] = {0, 0}, sq[2] = {0, 0};
            for (int k = 0; k < np; ++k) {
                const int32_t *q = record_part(r, k);
                const double cx = rint((double)(2LL * q[0] + q[2]) * 0.5), cy = rint((double)(2LL * q[1] + q[3]) * 0.5);
                s[0] = __dadd_rn(s[0], cx); sq[0] = __dadd_rn(sq[0], __dmul_rn(cx, cx));
                s[1] = __dadd_rn(s[1], cy); sq[1] = __dadd_rn(sq[1], __dmul_rn(cy, cy));
            }
            const double scale = 1. / (double)np;
            double mean[2], sd[2];
            for (int c = 0; c < 2; ++c) {
                mean[c] = __dmul_rn(s[c], scale);
                sd[c] = sqrt(fmax(__dsub_rn(__dmul_rn(sq[c], scale), __dmul_rn(mean[c], mean[c])), 0.));
            }
            int nb = 0;
            for (int k = 0; k <= np; ++k) {
                long long x, y, w, h;
                if (k < np) {
                    const int32_t *q = record_part(r, k);
                    x = q[0]; y = q[1]; w = q[2]; h = q[3];
                } else {   // Rect(xmean - 1.5 xstd, ymean - 1.5 ystd, 3 xstd, 3 ystd): double -> int truncates
                    x = (int)__dsub_rn(mean[0], __dmul_rn(1.5, sd[0])); y = (int)__dsub_rn(mean[1], __dmul_rn(1.5, sd[1]));
                    w = (int)__dmul_rn(3., sd[0]); h = (int)__dmul_rn(3., sd[1]);
                }
                rect_and64(x, y, w, h, 0, 0, cols, rows);
                // scaled to the depth image, each member truncated; the reference's depth(r) asserts inside the image, which
                // the intersection below makes explicit (it changes nothing the reference computes)
                long long dx = (int)__dmul_rn((double)x, sx), dyy = (int)__dmul_rn((double)y, sy);
                long long dw = (int)__dmul_rn((double)w, sx), dh = (int)__dmul_rn((double)h, sy);
                rect_and64(dx, dyy, dw, dh, 0, 0, fr.cols, fr.rows);
                if (dw <= 0 || dh <= 0) continue;   // part.empty(): skipped
                S.box[nb++] = make_int4((int)dx, (int)dyy, (int)dw, (int)dh);
            }
            S.nbox = nb;
            S.M = 0; S.first_valid = 0;
        }
        for (int t = tid; t < kB3Bins; t += kB3Threads) S.hist[t] = 0;
        __syncthreads();
        // ---- pass 0: M, the first box's count, the histogram of the top digit
        b3_pass<D>(S, fr, 32 - kB3Bits, true);
        __syncthreads();
        const unsigned int M = S.M;
        if (S.nbox == 0 || S.first_valid == 0 || M == 0) {   // the reference's NaN box (all-empty: defined here)
            if (tid < 6) out[tid] = tid < 3 ? qnan : 0.;
            __syncthreads();
            continue;
        }
        // ---- the ranks the resample reads (M == 400: the copy, ranks 0..399)
        const double scale = 1.0 / (400.0 / (double)M);
        if (tid < kB3Out) {
            int sy = tid;
            if (M != kB3Out) (void)b3_fy(tid, scale, &sy);
            S.sy[tid] = sy;
        }
        __syncthreads();
        if (tid == 0) {   // merge the two non-decreasing sequences clamp(sy) and clamp(sy + 1), distinct values
            const int last = (int)M - 1;
            int K = 0, a = 0, b = 0, prev = -1;
            while (a < kB3Out || b < kB3Out) {
                const int va = a < kB3Out ? min(max(S.sy[a], 0), last) : 0x7fffffff;
                const int vb = b < kB3Out ? min(max(S.sy[b] + 1, 0), last) : 0x7fffffff;
                int v;
                if (va <= vb) { v = va; ++a; } else { v = vb; ++b; }
                if (v != prev) { S.rank[K++] = v; prev = v; }
            }
            S.K = K;
        }
        __syncthreads();
        const int K = S.K;
        for (int t = tid; t < K; t += kB3Threads) { S.pre[t] = 0u; S.resid[t] = S.rank[t]; }
        __syncthreads();
        // ---- resolve one digit per pass: rank u's digit is the bin of its row where its residual rank falls
        for (int pass = 0; pass < kB3Passes; ++pass) {
            const int shift = 32 - kB3Bits * (pass + 1);
            if (pass > 0) {
                for (int t = tid; t < K * kB3Bins; t += kB3Threads) S.hist[t] = 0;
                __syncthreads();
                b3_pass<D>(S, fr, shift, false);
                __syncthreads();
            }
            uint32_t npre = 0; int nres = 0;
            if (tid < K) {
                const int row = pass == 0 ? 0 : lower_bound_i32(S.pre, K, S.pre[tid]);
                int res = S.resid[tid], dg = 0;
                for (; dg < kB3Bins - 1; ++dg) {
                    const int c = (int)S.hist[row * kB3Bins + dg];
                    if (res < c) break;
                    res -= c;
                }
                npre = (S.pre[tid] << kB3Bits) | (uint32_t)dg;
                nres = res;
            }
            __syncthreads();
            if (tid < K) { S.pre[tid] = npre; S.resid[tid] = nres; }
            __syncthreads();
        }
        // ---- resample (S[r0] * (1 - fy) + S[r1] * fy, weights not reset at the clamp) and filter
        if (tid < kB3Out) {
            float v;
            if (M == kB3Out) {
                v = float_unkey(S.pre[tid]);
            } else {
                int sy;
                const float fy = b3_fy(tid, scale, &sy);
                const int last = (int)M - 1;
                const float s0 = float_unkey(S.pre[lower_bound_i32(S.rank, K, min(max(sy, 0), last))]);
                const float s1 = float_unkey(S.pre[lower_bound_i32(S.rank, K, min(max(sy + 1, 0), last))]);
                v = __fadd_rn(__fmul_rn(s0, __fsub_rn(1.f, fy)), __fmul_rn(s1, fy));
            }
            S.p[tid] = v;
        }
        __syncthreads();
        if (tid < kB3Out) {   // correlation, BORDER_REFLECT_101, zero taps skipped, s = 0; s += k[t] * x in tap order
            float s = 0.f;
            for (int t = 0; t < kB3Taps; ++t) {
                const float k = p.dog[t];
                if (k == 0.f) continue;
                int j = tid + t - kB3Taps / 2;
                if (j < 0) j = -j;
                if (j >= kB3Out) j = 2 * (kB3Out - 1) - j;
                s = __fadd_rn(s, __fmul_rn(k, S.p[j]));
            }
            S.d[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {   // from the median out; a NaN compares false and the walk goes on through it
            const int mid = kB3Out / 2;
            int dmax = mid, dmin = mid;
            for (int m = mid; m < kB3Out; ++m) { if ((double)fabsf(S.d[m]) > 0.035) break; dmax = m; }
            for (int m = mid; m >= 0; --m) { if ((double)fabsf(S.d[m]) > 0.035) break; dmin = m; }
            // Rect3d(tl, br) with bb = boundingBox(), the unclipped hull (Candidate.hpp:105-111), in member order
            long long x, y, w, h;
            record_hull64(r, np, x, y, w, h);
            const double z0 = (double)S.p[dmin], z1 = (double)S.p[dmax];
            out[0] = (double)(int)x; out[1] = (double)(int)y; out[2] = z0;
            out[3] = (double)(int)h; out[4] = (double)(int)w; out[5] = __dsub_rn(z1, z0);
        }
        __syncthreads();
    }
}

}  // namespace

void launch_boxes3d(const Boxes3dParams &p, int grid, hipStream_t s)
{
    grid = std::max(std::min(grid, kB3MaxGrid), 1);
    switch (p.depth) {
    case kDepth8U: PBD_LAUNCH(k_boxes3d<kDepth8U>, dim3(grid), dim3(kB3Threads), 0, s, p); break;
    case kDepth16U: PBD_LAUNCH(k_boxes3d<kDepth16U>, dim3(grid), dim3(kB3Threads), 0, s, p); break;
    case kDepth32F: PBD_LAUNCH(k_boxes3d<kDepth32F>, dim3(grid), dim3(kB3Threads), 0, s, p); break;
    default: PBD_LAUNCH(k_boxes3d<kDepth64F>, dim3(grid), dim3(kB3Threads), 0, s, p); break;
    }
}

}  // namespace pbd
