// pbd_kernels_kmeans.hip -- the part types of a flexible-mixtures model (pbd_cluster_parts*): clusterparts.m + k_means.m of the
// reference's Matlab training code (matlab/learning), and the anchors of buildmodel.m:68-70.  include/pbd.h states the contract
// and every summation order, DESIGN.md section 6n the decisions and the cost.
//
//   k_km_trials   one workgroup of 1024 lanes per (part, trial), pairs taken in a stride loop under a capped grid: the whole
//                 k-means run of the pair.  The offsets X are read from global memory (all trials of a part share them: L2);
//                 the centroids, the counts and the change flag are in LDS; the pair's labels are one byte per point in the
//                 workspace.  Point n is always lane n mod 1024's, so a label is read and written by one thread only.
//   k_km_pick     one workgroup per part: the first trial with the smallest sum of distances, its labels, centres and counts,
//                 the anchors and the info record.
//
// All arithmetic is double.  Every sum over the points is R(.) of include/pbd.h (reduce1 of pbd_device.h): lane l adds the values
// of points l, l + 1024, ... from +0.0 (a point that is not a member adds nothing), then the two halving trees.  The 2 K sums of
// an iteration's centroids go through the trees together, behind one barrier.
#include "pbd_device.h"

namespace pbd {
namespace {

constexpr int kLanes = kRLanes;
constexpr int kWaves = kRWaves;
constexpr uint8_t kNoLabel = 0xff;   // a point before its first iteration (Matlab's g0 = ones against gIdx = zeros: all differ)

// X[n] of the part: def[a][n] - def[b][n] per coordinate
__device__ __forceinline__ void offset_of(const double *A, const double *B, int n, double &x, double &y)
{
    x = A[2 * (size_t)n] - B[2 * (size_t)n];
    y = A[2 * (size_t)n + 1] - B[2 * (size_t)n + 1];
}

// KM: the centroids the lane sums are held for (the largest K of the call, rounded up)
template <int KM>
__global__ __launch_bounds__(kLanes) void k_km_trials(KmParams p)
{
    __shared__ double cx[kMaxMix], cy[kMaxMix];
    __shared__ double red[2 * kMaxMix * kWaves];   // [quantity 2 t + coordinate][wavefront]
    __shared__ double red1[kWaves + 1];
    __shared__ int cnt[kMaxMix];
    __shared__ int sh_changed;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long pairs = (long long)p.nparts * p.trials;
    for (long long pr = blockIdx.x; pr < pairs; pr += gridDim.x) {
        const KmPart kp = p.parts[pr / p.trials];
        const int K = min(max(kp.K, 1), KM);
        const double *A = p.def + 2 * (size_t)kp.a * p.npos, *B = p.def + 2 * (size_t)kp.b * p.npos;
        uint8_t *lab = p.lab + (size_t)pr * p.npos;
        __syncthreads();   // the previous pair's centroids and counts have been written out
        if (t < kMaxMix) {
            double x = qnan_d(), y = qnan_d();
            if (t < K) offset_of(A, B, min(max(p.start[pr * kMaxMix + t], 0), p.npos - 1), x, y);
            cx[t] = x; cy[t] = y;
        }
        for (int n = t; n < p.npos; n += kLanes) lab[n] = kNoLabel;
        int it = 0;
        double zacc = 0.0;
        for (;;) {   // every condition that leaves the loop is uniform over the workgroup; at most max_iter rounds
            ++it;
            if (t < kMaxMix) cnt[t] = 0;
            if (t == 0) sh_changed = 0;
            __syncthreads();
            double sx[KM], sy[KM];
#pragma unroll
            for (int q = 0; q < KM; ++q) sx[q] = sy[q] = 0.0;
            zacc = 0.0;
            int changed = 0;
            for (int n0 = 0; n0 < p.npos; n0 += kLanes) {   // whole waves walk the loop (wave_add_by_key)
                const int n = n0 + t;
                const bool on = n < p.npos;
                int label = 0;
                if (on) {
                    double x, y;
                    offset_of(A, B, n, x, y);
                    // Matlab's min over the row: NaN is skipped, the first minimum wins; a row of NaN gives NaN at index 1
                    label = -1;
                    double z = qnan_d();
                    for (int q = 0; q < K; ++q) {
                        const double dx = x - cx[q], dy = y - cy[q];
                        const double D = (0.0 + dx * dx) + dy * dy;
                        if (D == D && (label < 0 || D < z)) { label = q; z = D; }
                    }
                    if (label < 0) label = 0;
                    if (lab[n] != (uint8_t)label) { changed = 1; lab[n] = (uint8_t)label; }
#pragma unroll
                    for (int q = 0; q < KM; ++q)
                        if (q == label) { sx[q] = sx[q] + x; sy[q] = sy[q] + y; }
                    zacc = zacc + z;
                }
                wave_add_by_key(cnt, label, on);
            }
#pragma unroll
            for (int q = 0; q < KM; ++q) {
                if (q < K) {   // uniform
                    double u = sx[q], v = sy[q];
                    for (int h = 32; h >= 1; h >>= 1) { u = u + __shfl_down(u, h, 64); v = v + __shfl_down(v, h, 64); }
                    if (lane == 0) { red[(2 * q) * kWaves + wave] = u; red[(2 * q + 1) * kWaves + wave] = v; }
                }
            }
            if (changed) sh_changed = 1;
            __syncthreads();
            const int ch = sh_changed;
            {   // the tree over the 16 wavefront sums of quantity t / 16, in the 16 lanes t % 16 (every lane shuffles)
                const bool mine = t < 2 * K * kWaves;
                double s = mine ? red[t] : 0.0;
                for (int h = kWaves / 2; h >= 1; h >>= 1) s = s + __shfl_down(s, h, kWaves);
                if (mine && (t & (kWaves - 1)) == 0) {
                    const int q = t / kWaves, c = cnt[q >> 1];
                    const double m = c > 0 ? s / (double)c : qnan_d();   // an empty cluster never wins a point again
                    if (q & 1) cy[q >> 1] = m; else cx[q >> 1] = m;
                }
            }
            __syncthreads();
            if (!ch || it >= p.max_iter) break;
        }
        const double sd = reduce1(zacc, red1);
        if (t < kMaxMix) {
            p.cen[(pr * kMaxMix + t) * 2] = cx[t];
            p.cen[(pr * kMaxMix + t) * 2 + 1] = cy[t];
            p.cnt[pr * kMaxMix + t] = t < K ? cnt[t] : 0;
        }
        if (t == 0) { p.sumdist[pr] = sd; p.iters[pr] = it; }
    }
}

// buildmodel.m:70 and zeroIndex: Matlab's round (halves away from zero) of centre + 1, minus 1; NaN 0; saturating
__device__ int32_t anchor_of(double c)
{
    if (c != c) return 0;
    const double v = c + 1.0;
    double r = trunc(v);
    if (fabs(v - r) >= 0.5) r = r + (v > 0.0 ? 1.0 : -1.0);
    r = r - 1.0;
    return r <= -2147483648.0 ? INT32_MIN : r >= 2147483647.0 ? INT32_MAX : (int32_t)r;
}

__global__ __launch_bounds__(256) void k_km_pick(KmParams p)
{
    __shared__ int sh_best;
    const int part = blockIdx.x, t = threadIdx.x;
    const long long pr0 = (long long)part * p.trials;
    if (t == 0) {   // clusterparts.m:25-26: min skips NaN and takes the first minimum; all NaN: index 1
        int best = -1;
        double bv = 0.0;
        for (int r = 0; r < p.trials; ++r) {
            const double v = p.sumdist[pr0 + r];
            if (v == v && (best < 0 || v < bv)) { best = r; bv = v; }
        }
        if (best < 0) best = 0;
        sh_best = best;
        pbd_cluster_info o;
        o.best_trial = best; o.iterations = p.iters[pr0 + best]; o.sumdist = p.sumdist[pr0 + best];
        p.info[part] = o;
    }
    __syncthreads();
    const long long pr = pr0 + sh_best;
    const uint8_t *lab = p.lab + (size_t)pr * p.npos;
    int32_t *idx = p.idx + (size_t)part * p.npos;
    for (int n = t; n < p.npos; n += 256) idx[n] = lab[n];
    if (t < kMaxMix) {
        const double x = p.cen[(pr * kMaxMix + t) * 2], y = p.cen[(pr * kMaxMix + t) * 2 + 1];
        const size_t o = (size_t)part * kMaxMix + t;
        p.centres[2 * o] = x; p.centres[2 * o + 1] = y;
        p.counts[o] = p.cnt[pr * kMaxMix + t];
        const bool root = p.parts[part].root != 0;
        p.anchors[2 * o] = root ? 0 : anchor_of(x);
        p.anchors[2 * o + 1] = root ? 0 : anchor_of(y);
    }
}

}  // namespace

void launch_km_trials(const KmParams &p, int maxK, hipStream_t s)
{
    const long long pairs = (long long)p.nparts * p.trials;
    const dim3 grid((unsigned)std::min<long long>(pairs, kKmMaxGrid));
    if (maxK <= 8) PBD_LAUNCH(k_km_trials<8>, grid, dim3(kLanes), 0, s, p);
    else PBD_LAUNCH(k_km_trials<kMaxMix>, grid, dim3(kLanes), 0, s, p);
}

void launch_km_pick(const KmParams &p, hipStream_t s) { PBD_LAUNCH(k_km_pick, dim3(p.nparts), dim3(256), 0, s, p); }

}  // namespace pbd
