// pbd_kernels_planes.hip -- opt-in plane removal from organized clouds (pbd_remove_planes): the callers'
// PointCloudClusterer::organizedMultiplaneSegmentation (include/PointCloudClusterer.hpp:294-336; cells/detect.cpp:263-273,
// ros/Node.cpp:218-229).  include/pbd.h states the contract.
//
// Every cloud of a call is one slice of a concatenation of all their points; a point's cloud is found by a binary search of the
// cloud table.  One fixed sequence of launches, each a grid-stride loop (no host loop, nothing read back):
//   normals    k_pl_load (the points, union-find roots), k_pl_rowsums (per pixel: the row window's gradient sums, left to right,
//              and whether the row window holds a depth edge), k_pl_normals (the 2s+1 row sums top to bottom, the normal, d)
//   segments   k_pl_hook: union-find over the left / upper comparator edges (uf_unite, pbd_device.h, as k_cl_hook), k_pl_size:
//              component sizes, one atomic per distinct root of a wave; k_pl_cand: final roots and the flags of the segments
//              above min_inliers; an exclusive scan (launch_scan, pbd_device.h); k_pl_cand_list: the candidates in point order
//   planes     k_pl_moments: one workgroup per candidate, one wave per image row: the row's nine double moments, left to right
//              (ballot, then an ordered walk of the matching lanes through readlane), the row partials top to bottom, then the
//              Jacobi eigenpair (jacobi3, pbd_jacobi.h);
//              k_pl_planes (one thread per cloud): plane numbers in candidate order; k_pl_label: the working label image
//   refine     k_pl_refine, once per pass: one workgroup per cloud, one thread per row, one anti-diagonal per step (the
//              recurrence of include/pbd.h); a row's label and z at the previous step go through LDS (clouds taller than
//              kPlRefLds rows: a global slice)
//   output     k_pl_final (output labels, inlier counts, kept flags), an exclusive scan, k_pl_kept (the kept points and their
//              indices in order, then the NaN fill), k_pl_out (counts, plane records, status)
// Every float / double operation whose bits are compared is an explicitly rounded intrinsic, so none of them is contracted.
#include "pbd_device.h"
#include "pbd_jacobi.h"

#include <math.h>

#include <algorithm>

namespace pbd {
namespace {

constexpr int kPlThreads = 256;
static_assert(kPlThreads == kScanThreads, "the scans of the flags run at the stage's workgroup size");
constexpr int kPlMaxGrid = 4096;
constexpr int kMoThreads = 1024;                 // k_pl_moments: 16 waves, one image row each at a time
constexpr int kMoWaves = kMoThreads / 64;
constexpr int kMoRows = 128;                     // row partials staged in LDS per round
constexpr int kRefThreads = 1024;                // k_pl_refine: one workgroup per cloud

__device__ inline bool pl_finite(float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// the cloud of a point of the concatenation (clouds[nclouds].base = npts)
__device__ inline int pl_cloud(const PlaneParams &p, long long e)
{
    int lo = 0, hi = p.nclouds - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.clouds[mid].base <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline float pl_dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// the depth-dependent threshold t * (z * z)
__device__ inline float pl_thr(float t, float z) { return __fmul_rn(t, __fmul_rn(z, z)); }

// a lane's double, read by the whole wave (the lane index is wave-uniform)
__device__ inline double pl_readlane(double v, int lane)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(kPlThreads) void k_pl_load(PlaneParams p)
{
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads) {
        const PlaneCloud c = p.clouds[pl_cloud(p, e)];
        const long long j = e - c.base;
        const int r = (int)(j / c.cols), cc = (int)(j - (long long)r * c.cols);
        const float *pt = reinterpret_cast<const float *>(c.data + r * c.row_stride + cc * c.point_stride);
        p.xyz[e] = make_float4(pt[0], pt[1], pt[2], 0.f);
        p.parent[e] = (int)e;
        p.csize[e] = 0;
    }
}

// depth edge: not finite, or a 4-neighbour not finite or |z(q) - z(p)| > depth_change * z(p) (all four neighbours exist: the
// callers only ask for pixels off the image border)
__device__ inline bool pl_edge(const PlaneParams &p, const float4 *P, int W, int r, int c)
{
    const float4 v = P[(long long)r * W + c];
    if (!pl_finite(v)) return true;
    const float t = __fmul_rn(p.depth_change, v.z);
    const long long i = (long long)r * W + c;
    const float4 q[4] = {P[i - 1], P[i + 1], P[i - W], P[i + W]};
    for (int k = 0; k < 4; ++k)
        if (!pl_finite(q[k]) || fabsf(__fsub_rn(q[k].z, v.z)) > t) return true;
    return false;
}

// per pixel with 1 <= r <= rows-2 and s+1 <= c <= cols-s-2: the sums of dx and dy over columns c-s .. c+s, left to right, and the
// depth-edge flag of the row window; every other pixel is marked as an edge (its row sum is never part of a valid window)
__global__ __launch_bounds__(kPlThreads) void k_pl_rowsums(PlaneParams p)
{
    const int s = p.half;
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads) {
        const PlaneCloud c = p.clouds[pl_cloud(p, e)];
        const long long j = e - c.base;
        const int W = c.cols, H = c.rows;
        const int r = (int)(j / W), cc = (int)(j - (long long)r * W);
        const float4 *P = p.xyz + c.base;
        if (r < 1 || r > H - 2 || cc < s + 1 || cc > W - s - 2) {
            p.rsx[e] = make_float4(0.f, 0.f, 0.f, 1.f);
            p.rsy[e] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        float sx = 0.f, sy = 0.f, sz = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
        bool edge = false;
        for (int k = cc - s; k <= cc + s; ++k) {
            const long long i = (long long)r * W + k;
            const float4 a = P[i + 1], b = P[i - 1], u = P[i + W], d = P[i - W];
            sx = __fadd_rn(sx, __fsub_rn(a.x, b.x)); sy = __fadd_rn(sy, __fsub_rn(a.y, b.y)); sz = __fadd_rn(sz, __fsub_rn(a.z, b.z));
            tx = __fadd_rn(tx, __fsub_rn(u.x, d.x)); ty = __fadd_rn(ty, __fsub_rn(u.y, d.y)); tz = __fadd_rn(tz, __fsub_rn(u.z, d.z));
            edge = edge || pl_edge(p, P, W, r, k);
        }
        p.rsx[e] = make_float4(sx, sy, sz, edge ? 1.f : 0.f);
        p.rsy[e] = make_float4(tx, ty, tz, 0.f);
    }
}

__global__ __launch_bounds__(kPlThreads) void k_pl_normals(PlaneParams p)
{
    const int s = p.half;
    const float area = (float)((2 * s + 1) * (2 * s + 1));
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads) {
        const PlaneCloud c = p.clouds[pl_cloud(p, e)];
        const long long j = e - c.base;
        const int W = c.cols, H = c.rows;
        const int r = (int)(j / W), cc = (int)(j - (long long)r * W);
        const float4 v = p.xyz[e];
        float4 out = make_float4(qnan_f(), qnan_f(), qnan_f(), qnan_f());
        if (r >= s + 1 && r <= H - s - 2 && cc >= s + 1 && cc <= W - s - 2) {
            float sx = 0.f, sy = 0.f, sz = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
            bool edge = false;
            for (int k = r - s; k <= r + s; ++k) {
                const long long i = c.base + (long long)k * W + cc;
                const float4 a = p.rsx[i], b = p.rsy[i];
                sx = __fadd_rn(sx, a.x); sy = __fadd_rn(sy, a.y); sz = __fadd_rn(sz, a.z);
                tx = __fadd_rn(tx, b.x); ty = __fadd_rn(ty, b.y); tz = __fadd_rn(tz, b.z);
                edge = edge || a.w != 0.f;
            }
            if (!edge) {
                const float mxx = __fdiv_rn(sx, area), mxy = __fdiv_rn(sy, area), mxz = __fdiv_rn(sz, area);
                const float myx = __fdiv_rn(tx, area), myy = __fdiv_rn(ty, area), myz = __fdiv_rn(tz, area);
                // n = cross(mean dy, mean dx)
                float nx = __fsub_rn(__fmul_rn(myy, mxz), __fmul_rn(myz, mxy));
                float ny = __fsub_rn(__fmul_rn(myz, mxx), __fmul_rn(myx, mxz));
                float nz = __fsub_rn(__fmul_rn(myx, mxy), __fmul_rn(myy, mxx));
                // sqrtf is the correctly rounded root; __fsqrt_rn is the native one here (an ulp off on some inputs), and
                // an ulp in a normal decides a join whose dot product sits at cos_thr (tests/cloud_hard_scenes.py, joins)
                const float len = sqrtf(pl_dot3(nx, ny, nz, nx, ny, nz));
                nx = __fdiv_rn(nx, len); ny = __fdiv_rn(ny, len); nz = __fdiv_rn(nz, len);
                if (pl_dot3(nx, ny, nz, v.x, v.y, v.z) > 0.f) { nx = -nx; ny = -ny; nz = -nz; }
                out = make_float4(nx, ny, nz, pl_dot3(nx, ny, nz, v.x, v.y, v.z));
            }
        }
        p.nrm[e] = out;
    }
}

// PlaneCoefficientComparator, depth dependent, z of the current point p; a NaN normal fails both tests
__device__ inline bool pl_join(const PlaneParams &p, float4 vp, float4 np_, float4 vq, float4 nq)
{
    if (!pl_finite(vq)) return false;
    const bool near = fabsf(__fsub_rn(np_.w, nq.w)) < pl_thr(p.dist_thr, vp.z);
    return near && pl_dot3(np_.x, np_.y, np_.z, nq.x, nq.y, nq.z) > p.cos_thr;
}

__global__ __launch_bounds__(kPlThreads) void k_pl_hook(PlaneParams p)
{
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads) {
        const float4 v = p.xyz[e];
        if (!pl_finite(v)) continue;
        const PlaneCloud c = p.clouds[pl_cloud(p, e)];
        const long long j = e - c.base;
        const int W = c.cols;
        const int r = (int)(j / W), cc = (int)(j - (long long)r * W);
        const float4 n = p.nrm[e];
        if (cc >= 1 && pl_join(p, v, n, p.xyz[e - 1], p.nrm[e - 1])) uf_unite(p.parent, (int)e, (int)(e - 1));
        if (r >= 1 && pl_join(p, v, n, p.xyz[e - W], p.nrm[e - W])) uf_unite(p.parent, (int)e, (int)(e - W));
    }
}

__global__ __launch_bounds__(kPlThreads) void k_pl_size(PlaneParams p)
{
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads)
        wave_add_by_key(p.csize, uf_find(p.parent, (int)e), true);
}

// every point's final root; flag = a root of a finite segment with more than min_inliers points
__global__ __launch_bounds__(kPlThreads) void k_pl_cand(PlaneParams p)
{
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads) {
        const int root = uf_root(p.parent, (int)e);
        p.parent[e] = root;
        p.flag[e] = (root == e && pl_finite(p.xyz[e]) && p.csize[e] > p.min_inliers) ? 1 : 0;
    }
}

__global__ __launch_bounds__(kPlThreads) void k_pl_cand_list(PlaneParams p)
{
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads) {
        const int g = p.flag[e];
        if (p.flag[e + 1] > g && g < p.cand_cap) p.cand_root[g] = (int)e;
    }
}

// cyclic Jacobi on the symmetric 3x3 A (double, + - * / sqrt only); V accumulates the rotations from the identity
// one workgroup per candidate: the nine moments {x, y, z, xx, xy, xz, yy, yz, zz} in double, each row left to right, the row
// partials top to bottom; mean, covariance, the smallest eigenpair, curvature and the plane
__global__ __launch_bounds__(kMoThreads) void k_pl_moments(PlaneParams p)
{
    __shared__ double rowp[kMoRows][9];
    __shared__ double tot[9];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ncand = min(p.flag[p.npts], p.cand_cap);
    for (int g = blockIdx.x; g < ncand; g += gridDim.x) {
        const int root = p.cand_root[g];
        const PlaneCloud c = p.clouds[pl_cloud(p, root)];
        const int W = c.cols, H = c.rows;
        double acc = 0.0;                                   // thread k < 9: moment k over the rows so far
        for (int r0 = 0; r0 < H; r0 += kMoRows) {
            const int nr = min(kMoRows, H - r0);
            for (int rr = wv; rr < nr; rr += kMoWaves) {
                const long long row = c.base + (long long)(r0 + rr) * W;
                double s[9];
                for (int k = 0; k < 9; ++k) s[k] = 0.0;
                for (int c0 = 0; c0 < W; c0 += 64) {
                    const int cc = c0 + lane;
                    const bool m = cc < W && p.parent[row + cc] == root;
                    const unsigned long long mask0 = __ballot(m);
                    if (!mask0) continue;
                    const float4 v = m ? p.xyz[row + cc] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const double x = v.x, y = v.y, z = v.z;
                    const double q[9] = {x, y, z, __dmul_rn(x, x), __dmul_rn(x, y), __dmul_rn(x, z), __dmul_rn(y, y),
                                         __dmul_rn(y, z), __dmul_rn(z, z)};
                    unsigned long long mask = mask0;
                    while (mask) {
                        const int src = __ffsll((long long)mask) - 1;
                        mask &= mask - 1;
                        for (int k = 0; k < 9; ++k) s[k] = __dadd_rn(s[k], pl_readlane(q[k], src));
                    }
                }
                if (lane == 0)
                    for (int k = 0; k < 9; ++k) rowp[rr][k] = s[k];
            }
            __syncthreads();
            if (threadIdx.x < 9)
                for (int rr = 0; rr < nr; ++rr) acc = __dadd_rn(acc, rowp[rr][threadIdx.x]);
            __syncthreads();
        }
        if (threadIdx.x < 9) tot[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double n = (double)p.csize[root];
            double m[9];
            for (int k = 0; k < 9; ++k) m[k] = __ddiv_rn(tot[k], n);
            const double xx = __dsub_rn(m[3], __dmul_rn(m[0], m[0])), xy = __dsub_rn(m[4], __dmul_rn(m[0], m[1]));
            const double xz = __dsub_rn(m[5], __dmul_rn(m[0], m[2])), yy = __dsub_rn(m[6], __dmul_rn(m[1], m[1]));
            const double yz = __dsub_rn(m[7], __dmul_rn(m[1], m[2])), zz = __dsub_rn(m[8], __dmul_rn(m[2], m[2]));
            double A[3][3] = {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}}, V[3][3];
            jacobi3(A, V);
            int k = 0;
            if (A[1][1] < A[k][k]) k = 1;
            if (A[2][2] < A[k][k]) k = 2;
            const double curv = __ddiv_rn(A[k][k], __dadd_rn(__dadd_rn(xx, yy), zz));
            double a = V[0][k], b = V[1][k], cz = V[2][k];
            double d = -__dadd_rn(__dadd_rn(__dmul_rn(a, m[0]), __dmul_rn(b, m[1])), __dmul_rn(cz, m[2]));
            const double cosv = __dadd_rn(__dadd_rn(__dmul_rn(-m[0], a), __dmul_rn(-m[1], b)), __dmul_rn(-m[2], cz));
            if (cosv < 0.0) { a = -a; b = -b; cz = -cz; d = -d; }
            p.cand_coef[g] = make_float4((float)a, (float)b, (float)cz, (float)d);
            p.cand_plane[g] = curv < p.max_curv ? 1 : 0;
        }
        __syncthreads();
    }
}

// one thread per cloud: plane numbers in candidate order, the planes' records in the workspace
__global__ __launch_bounds__(kPlThreads) void k_pl_planes(PlaneParams p)
{
    for (int i = blockIdx.x * kPlThreads + threadIdx.x; i < p.nclouds; i += gridDim.x * kPlThreads) {
        const int g0 = p.flag[p.clouds[i].base], g1 = p.flag[p.clouds[i + 1].base];
        int k = 0;
        for (int g = g0; g < g1 && g < p.cand_cap; ++g) {
            if (p.cand_plane[g]) {
                p.plane_coef[g0 + k] = p.cand_coef[g];
                p.plane_cnt[g0 + k] = 0;
                p.cand_plane[g] = k++;
            } else {
                p.cand_plane[g] = -1;
            }
        }
        p.cbase[i] = g0;
        p.np[i] = k;
        if (i == p.nclouds - 1) p.cbase[p.nclouds] = g1;
    }
}

__global__ __launch_bounds__(kPlThreads) void k_pl_label(PlaneParams p)
{
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads) {
        int l = -1;
        if (pl_finite(p.xyz[e])) {
            const int root = p.parent[e];
            const int g = p.flag[root];
            l = (p.flag[root + 1] > g && g < p.cand_cap && p.cand_plane[g] >= 0) ? p.cand_plane[g] : -2;
        }
        p.lab[e] = l;
    }
}

// |((a x + b y) + c z) + d| < dist_thr * (z_cur * z_cur), on the neighbour's point
__device__ inline bool pl_absorb(const PlaneParams &p, float4 pl, float4 v, float zcur)
{
    const float dd = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(pl.x, v.x), __fmul_rn(pl.y, v.y)), __fmul_rn(pl.z, v.z)), pl.w);
    return fabsf(dd) < pl_thr(p.dist_thr, zcur);
}

// One refinement pass (dir 0 forward, 1 backward = the forward pass on the image turned by 180 degrees), one workgroup per
// cloud.  In the pass's own coordinates, with o the label at the pass's start:
//   M(r,c) = F(r-1,c)  if r >= 1, c <= W-2, F(r-1,c) is a plane, (r-1,c+1) is finite, o(r,c) == -2 and absorb(F(r-1,c), P(r,c))
//            o(r,c)    otherwise
//   F(r,c) = F(r,c-1)  if c >= 1, r <= H-2, F(r,c-1) is a plane, M(r,c) == -2 and absorb(F(r,c-1), P(r,c))
//            M(r,c)    otherwise
// Cell (r, c) is computed at step r + c by the thread of row r.
__global__ __launch_bounds__(kRefThreads) void k_pl_refine(PlaneParams p, int dir)
{
    __shared__ int2 xl[2 * kPlRefLds];
    for (int i = blockIdx.x; i < p.nclouds; i += gridDim.x) {
        const PlaneCloud c = p.clouds[i];
        const int H = c.rows, W = c.cols;
        int2 *xb = H <= kPlRefLds ? xl : p.xch + 2 * c.rbase;
        int32_t *lab = p.lab + c.base;
        const float4 *P = p.xyz + c.base;
        const float4 *pl = p.plane_coef + p.cbase[i];
        if (p.np[i] == 0) continue;                         // uniform over the workgroup
        for (int t = 0; t <= H + W - 2; ++t) {
            int2 *cur = xb + (t & 1) * H, *prev = xb + ((t + 1) & 1) * H;
            for (int r = threadIdx.x; r < H; r += kRefThreads) {
                const int cc = t - r;
                if (cc < 0 || cc >= W) continue;
                const long long ar = dir ? H - 1 - r : r, ac = dir ? W - 1 - cc : cc;
                const long long idx = ar * W + ac;
                const float4 v = P[idx];
                const int o = lab[idx];
                int m = o;
                if (r >= 1 && cc <= W - 2 && o == -2) {
                    const int2 u = prev[r - 1];
                    const long long iur = dir ? idx + W - 1 : idx - W + 1;      // (r-1, c+1) of the pass
                    if (u.x >= 0 && pl_finite(P[iur]) && pl_absorb(p, pl[u.x], v, __int_as_float(u.y))) m = u.x;
                }
                int f = m;
                if (cc >= 1 && r <= H - 2 && m == -2) {
                    const int2 l = prev[r];
                    if (l.x >= 0 && pl_absorb(p, pl[l.x], v, __int_as_float(l.y))) f = l.x;
                }
                if (f != o) lab[idx] = f;
                cur[r] = make_int2(f, __float_as_int(v.z));
            }
            __syncthreads();
        }
    }
}

// output labels, inlier counts, kept flags (not a plane)
__global__ __launch_bounds__(kPlThreads) void k_pl_final(PlaneParams p)
{
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads) {
        const int l = p.lab[e];
        wave_add_by_key(p.plane_cnt, l >= 0 ? p.cbase[pl_cloud(p, e)] + l : 0, l >= 0);
        p.labels[e] = l >= 0 ? l : -1;
        p.flag[e] = l < 0 ? 1 : 0;
    }
}

__global__ __launch_bounds__(kPlThreads) void k_pl_kept(PlaneParams p)
{
    for (long long e = blockIdx.x * (long long)kPlThreads + threadIdx.x; e < p.npts; e += (long long)gridDim.x * kPlThreads) {
        const int i = pl_cloud(p, e);
        const long long b0 = p.clouds[i].base, b1 = p.clouds[i + 1].base;
        const int k0 = p.flag[b0];
        const long long j = e - b0, nk = p.flag[b1] - k0;
        if (p.flag[e + 1] > p.flag[e]) {
            const long long o = b0 + (p.flag[e] - k0);
            const float4 v = p.xyz[e];
            p.kept[o] = (int)j;
            p.points[3 * o] = v.x; p.points[3 * o + 1] = v.y; p.points[3 * o + 2] = v.z;
        }
        if (j >= nk) {
            p.kept[e] = -1;
            p.points[3 * e] = p.points[3 * e + 1] = p.points[3 * e + 2] = qnan_f();
        }
    }
}

// one workgroup: per cloud the counts and the first plane_cap planes; status = {kept points, most planes of one cloud}
__global__ __launch_bounds__(kPlThreads) void k_pl_out(PlaneParams p)
{
    for (int i = threadIdx.x; i < p.nclouds; i += kPlThreads) {
        const int nk = p.flag[p.clouds[i + 1].base] - p.flag[p.clouds[i].base];
        const int np = p.np[i], g0 = p.cbase[i];
        p.nkept[i] = nk;
        p.nplanes[i] = np;
        for (int k = 0; k < min(np, p.plane_cap); ++k) {
            const float4 q = p.plane_coef[g0 + k];
            float *o = p.planes + 4 * ((size_t)i * p.plane_cap + k);
            o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
            p.inliers[(size_t)i * p.plane_cap + k] = p.plane_cnt[g0 + k];
        }
    }
    if (threadIdx.x == 0) {
        long long most = 0;
        for (int i = 0; i < p.nclouds; ++i) most = max(most, (long long)p.np[i]);
        p.status[0] = p.flag[p.npts];
        p.status[1] = most;
    }
}

int pl_grid(long long work, int per_block = kPlThreads)
{
    return (int)std::max<long long>(std::min<long long>((work + per_block - 1) / per_block, kPlMaxGrid), 1);
}

}  // namespace

void launch_planes_step(const PlaneParams &p, int step, hipStream_t s)
{
    const dim3 blk(kPlThreads);
    const int g = pl_grid(p.npts);
    switch (step) {
    case kPlStepLoad: PBD_LAUNCH(k_pl_load, dim3(g), blk, 0, s, p); break;
    case kPlStepRowSums: PBD_LAUNCH(k_pl_rowsums, dim3(g), blk, 0, s, p); break;
    case kPlStepNormals: PBD_LAUNCH(k_pl_normals, dim3(g), blk, 0, s, p); break;
    case kPlStepHook: PBD_LAUNCH(k_pl_hook, dim3(g), blk, 0, s, p); break;
    case kPlStepSize: PBD_LAUNCH(k_pl_size, dim3(g), blk, 0, s, p); break;
    case kPlStepCand: PBD_LAUNCH(k_pl_cand, dim3(g), blk, 0, s, p); break;
    case kPlStepCandScan:
    case kPlStepKeptScan:
        // flag[0 .. npts) in place, flag[npts] = the total
        launch_scan<int>(p.flag, (int32_t *)nullptr, p.npts, (const long long *)nullptr, p.part, pl_grid(p.npts, kScanTile),
                         ScanNoTop{}, s);
        break;
    case kPlStepCandList: PBD_LAUNCH(k_pl_cand_list, dim3(g), blk, 0, s, p); break;
    case kPlStepMoments: PBD_LAUNCH(k_pl_moments, dim3(std::max(std::min(p.cand_cap, kPlMaxGrid), 1)), dim3(kMoThreads), 0, s, p); break;
    case kPlStepPlanes: PBD_LAUNCH(k_pl_planes, dim3(pl_grid(p.nclouds)), blk, 0, s, p); break;
    case kPlStepLabel: PBD_LAUNCH(k_pl_label, dim3(g), blk, 0, s, p); break;
    case kPlStepRefine:
        PBD_LAUNCH(k_pl_refine, dim3(std::min(p.nclouds, kPlMaxGrid)), dim3(kRefThreads), 0, s, p, 0);
        PBD_LAUNCH(k_pl_refine, dim3(std::min(p.nclouds, kPlMaxGrid)), dim3(kRefThreads), 0, s, p, 1);
        break;
    case kPlStepFinal: PBD_LAUNCH(k_pl_final, dim3(g), blk, 0, s, p); break;
    case kPlStepKept: PBD_LAUNCH(k_pl_kept, dim3(g), blk, 0, s, p); break;
    default: PBD_LAUNCH(k_pl_out, dim3(1), blk, 0, s, p); break;
    }
}

}  // namespace pbd
