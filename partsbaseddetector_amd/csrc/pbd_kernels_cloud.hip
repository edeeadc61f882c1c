// pbd_kernels_cloud.hip -- opt-in camera boxes, part centres and object clusters (pbd_boxes3d_camera, pbd_cluster_objects): the
// rest of the callers' PointCloudClusterer after Candidate::boundingBox3D (include/PointCloudClusterer.hpp:53-293;
// cells/detect.cpp:224-300, ros/Node.cpp:183-230).  include/pbd.h states the contract.
//
// k_camera_boxes, one wave per record, lanes over its parts: the camera box of k_boxes3d's cube through the pinhole model, and
// one camera-space centre per part from a sequential double sum of its depth samples (the order is the contract's).
//
// The clustering of every box is one fixed sequence of launches (no host loop, nothing read back), each a grid-stride loop:
//   crop     k_cl_crop_count: cropped points of every (box, chunk of 1024 points of the box's cloud); an exclusive scan of those
//            counts (launch_scan, pbd_device.h, as is the grid's scan); k_cl_crop_scatter: the cropped points in ascending
//            point order, box after box (index, box, xyz)
//   grid     a hashed uniform grid of 2 cm cells: k_cl_grid_count (bucket of every cropped point, counts), a scan,
//            k_cl_grid_scatter (points in bucket order).  2 cm is twice the radius, so two points within the radius lie in
//            neighbouring cells whatever the rounding of x * 50; the grid only prunes, the exact predicate decides every edge
//   cc       k_cl_hook: union-find over the 27 neighbouring cells (uf_unite, pbd_device.h: lock-free hooking of the larger root
//            under the smaller, ECL-CC style, agent-scope atomics); k_cl_label: every point's root, component sizes.  A root
//            is the smallest cropped position of its component, so labels do not depend on the order of the atomics
//   select   k_cl_best: per box the largest component (ties: the smallest root = the smallest point index), one 64-bit atomicMax;
//            k_cl_select: output counts and offsets (one workgroup); k_cl_out: one workgroup per box, the crop list filtered to
//            the winner in order, and the centroid as three sequential fp32 sums over points staged in LDS
// Every float / double operation whose bits are compared is an explicitly rounded intrinsic, so none of them is contracted.
#include "pbd_device.h"

#include <math.h>

#include <algorithm>

namespace pbd {
namespace {

constexpr int kClThreads = 256;
constexpr int kClWaves = kClThreads / 64;
static_assert(kClThreads == kScanThreads && kClChunk == kScanTile, "a crop chunk is one scan tile of points");
constexpr float kClCellInv = 50.f;              // 1 / (2 cm cell edge)

// PinholeCameraModel::projectPixelTo3dRay without its z = 1
__device__ inline void cam_ray(const Pinhole &c, double u, double v, double &rx, double &ry)
{
    rx = __ddiv_rn(__dsub_rn(__dsub_rn(u, c.cx), c.tx), c.fx);
    ry = __ddiv_rn(__dsub_rn(__dsub_rn(v, c.cy), c.ty), c.fy);
}

__global__ __launch_bounds__(kClThreads) void k_camera_boxes(CameraParams p)
{
    const int lane = threadIdx.x & 63;
    const int n = payload_count(p.in, p.in_cap);
    for (int i = blockIdx.x * kClWaves + (threadIdx.x >> 6); i < n; i += gridDim.x * kClWaves) {
        const int32_t *r = p.in + 1 + (size_t)i * p.stride;
        const long long f = (long long)r[kRecFrame] - p.frame_offset;
        const int np = r[kRecNparts];
        const double *cube = p.cube + 6 * (size_t)i;
        double *box = p.box + 6 * (size_t)i;
        bool skip = f < 0 || f >= p.nframes || np < 1 || np > p.max_parts;
        for (int k = 0; k < 6 && !skip; ++k) skip = isnan(cube[k]);
        if (skip) {                                     // the reference's `continue`: both outputs keep their initial values
            if (lane < 6) box[lane] = 0.0;
            if (lane == 0) { p.ncentres[i] = 0; p.dense[i] = 1; }
            continue;
        }
        const Pinhole c = p.cams[(int)f];
        const Box3dFrame fr = p.frames[(int)f];
        if (lane == 0) {                                // tl = ray(tl) * z, br = ray(br) * (z + depth), Rect3d(tl, br)
            double tx, ty, bx, by;
            cam_ray(c, cube[0], cube[1], tx, ty);
            cam_ray(c, __dadd_rn(cube[0], cube[4]), __dadd_rn(cube[1], cube[3]), bx, by);
            const double z0 = cube[2], z1 = __dadd_rn(cube[2], cube[5]);
            const double tlx = __dmul_rn(tx, z0), tly = __dmul_rn(ty, z0), tlz = __dmul_rn(1.0, z0);
            const double brx = __dmul_rn(bx, z1), bry = __dmul_rn(by, z1), brz = __dmul_rn(1.0, z1);
            box[0] = tlx; box[1] = tly; box[2] = tlz;
            box[3] = __dsub_rn(bry, tly); box[4] = __dsub_rn(brx, tlx); box[5] = __dsub_rn(brz, tlz);
        }
        int dense = 1;
        for (int j = lane; j < np; j += 64) {
            const int32_t *q = record_part(r, j);
            long long x = q[0], y = q[1], w = q[2], h = q[3];
            rect_and64(x, y, w, h, 0, 0, fr.im_cols, fr.im_rows);
            const double u = (double)(x + w / 2), v = (double)(y + h / 2);
            // literal: rows x .. x+h-1, columns y .. y+w-1 (PointCloudClusterer.hpp:111-120); XY: rows y.., columns x..
            const long long r0 = p.mode == kPartsLiteral ? x : y, c0 = p.mode == kPartsLiteral ? y : x;
            float o[3];
            if (w * h != 0 && (r0 + h > fr.rows || c0 + w > fr.cols)) {
                o[0] = o[1] = o[2] = qnan_f();          // the reference reads outside the depth image: a project decision
            } else {
                double s = 0.0;
                for (long long rr = r0; rr < r0 + h; ++rr) {
                    const float *row = reinterpret_cast<const float *>(fr.data + rr * fr.pitch);
                    for (long long cc = c0; cc < c0 + w; ++cc) s = __dadd_rn(s, (double)row[cc]);
                }
                if (w * h != 0) s = __ddiv_rn(s, (double)(int)(w * h));
                double rx, ry;
                cam_ray(c, u, v, rx, ry);
                o[0] = (float)__dmul_rn(rx, s); o[1] = (float)__dmul_rn(ry, s); o[2] = (float)__dmul_rn(1.0, s);
            }
            float *out = p.centres + ((size_t)i * p.max_parts + j) * 3;
            out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
            if (isnan(o[0]) || isnan(o[1]) || isnan(o[2])) dense = 0;
        }
        dense = __all(dense);
        if (lane == 0) { p.ncentres[i] = np; p.dense[i] = dense; }
    }
}

// ---- clustering ---------------------------------------------------------------------------------------------------------------
__device__ inline int cl_nbox(const ClusterParams &p) { return payload_count(p.in, p.in_cap); }
__device__ inline bool cl_overflow(const ClusterParams &p) { return p.ntab[0] > p.crop_cap; }

// the box's cloud, or -1 (not a box of this call)
__device__ inline int cl_frame(const ClusterParams &p, int b)
{
    const long long f = (long long)p.in[1 + (size_t)b * p.rec_stride + kRecFrame] - p.frame_offset;
    return (f < 0 || f >= p.nclouds) ? -1 : (int)f;
}

// the crop gate and bounds of a camera box (PointCloudClusterer.hpp:190-206): false = the box has no points
__device__ inline bool cl_gate(const double *bx, float *mn, float *mx)
{
    double x = bx[0], y = bx[1], z = bx[2];
    double h = bx[3], w = bx[4], d = bx[5];
    const double vol = __dmul_rn(__dmul_rn(w, h), d);
    if (!(vol >= 1e-6)) return false;
    x = __dsub_rn(x, __dmul_rn(w, 0.1)); y = __dsub_rn(y, __dmul_rn(h, 0.1)); z = __dsub_rn(z, __dmul_rn(d, 0.1));
    w = __dmul_rn(w, 1.2); h = __dmul_rn(h, 1.2); d = __dmul_rn(d, 1.2);
    mn[0] = (float)x; mn[1] = (float)y; mn[2] = (float)z;
    mx[0] = (float)__dadd_rn(x, w); mx[1] = (float)__dadd_rn(y, h); mx[2] = (float)__dadd_rn(z, d);
    return true;
}

__device__ inline float3 cl_load(const CloudFrame &c, int idx)
{
    const int r = idx / c.cols, cc = idx - r * c.cols;
    const float *pt = reinterpret_cast<const float *>(c.data + r * c.row_stride + cc * c.point_stride);
    return make_float3(pt[0], pt[1], pt[2]);
}

__device__ inline bool cl_inside(float3 v, const float *mn, const float *mx)
{
    return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && v.x >= mn[0] && v.x <= mx[0] && v.y >= mn[1] && v.y <= mx[1] &&
           v.z >= mn[2] && v.z <= mx[2];
}

__global__ __launch_bounds__(kClThreads) void k_cl_crop_count(ClusterParams p)
{
    __shared__ long long lds[kClWaves];
    const int n = cl_nbox(p);
    const long long units = (long long)n * p.nchunks;  // the boxes of the payload only: the scans read ntab[2]
    if (blockIdx.x == 0 && threadIdx.x == 0) p.ntab[2] = units;
    for (long long t = blockIdx.x; t < units; t += gridDim.x) {
        const int b = (int)(t / p.nchunks), ch = (int)(t % p.nchunks);
        const int f = cl_frame(p, b);
        float mn[3], mx[3];
        int cnt = 0;
        if (f >= 0 && cl_gate(p.boxes + 6 * (size_t)b, mn, mx)) {
            const CloudFrame c = p.clouds[f];
            const int npts = c.rows * c.cols;
            for (int k = 0; k < 4; ++k) {
                const long long idx = (long long)ch * kClChunk + k * kClThreads + threadIdx.x;
                if (idx < npts && cl_inside(cl_load(c, (int)idx), mn, mx)) ++cnt;
            }
        }
        long long total;
        block_scan<long long, kClWaves>(cnt, lds, total);
        if (threadIdx.x == 0) p.chunk_off[t] = total;
    }
}

__global__ __launch_bounds__(kClThreads) void k_cl_crop_scatter(ClusterParams p)
{
    __shared__ int lds[kClWaves];
    const long long units = (long long)cl_nbox(p) * p.nchunks;
    for (long long t = blockIdx.x; t < units; t += gridDim.x) {
        const int b = (int)(t / p.nchunks), ch = (int)(t % p.nchunks);
        const int f = cl_frame(p, b);
        float mn[3], mx[3];
        if (f < 0 || !cl_gate(p.boxes + 6 * (size_t)b, mn, mx)) continue;   // uniform over the workgroup
        const CloudFrame c = p.clouds[f];
        const int npts = c.rows * c.cols;
        long long pos = p.chunk_off[t];
        for (int k = 0; k < 4; ++k) {
            const long long idx = (long long)ch * kClChunk + k * kClThreads + threadIdx.x;
            float3 v = make_float3(0.f, 0.f, 0.f);
            const bool in = idx < npts && cl_inside(v = cl_load(c, (int)idx), mn, mx);
            int tot;
            const int rk = block_rank<kClWaves>(in, lds, tot);
            if (in && pos + rk < p.crop_cap) {
                p.crop_idx[pos + rk] = (int)idx;
                p.crop_box[pos + rk] = b;
                p.crop_xyz[pos + rk] = make_float4(v.x, v.y, v.z, 0.f);
            }
            pos += tot;
        }
    }
}

// thread 0 of the crop scan's top kernel: the total is the cropped point count (ntab[0], status[0]) and sets the bucket count
// ntab[1]
struct ClCropTotal {
    long long *ntab, *status;
    long long crop_cap;
    int tcap;
    __device__ void operator()(long long total) const
    {
        ntab[0] = total;
        status[0] = total;
        long long T = 1;
        while (T < 2 * total) T <<= 1;
        ntab[1] = total > crop_cap ? 0 : min(T, (long long)tcap);
    }
};

__device__ inline int cl_cell(float v)
{
    return (int)fminf(fmaxf(floorf(__fmul_rn(v, kClCellInv)), -1e9f), 1e9f);
}
__device__ inline uint32_t cl_hash(int b, int ix, int iy, int iz)
{
    uint32_t h = ((uint32_t)ix * 73856093u) ^ ((uint32_t)iy * 19349663u) ^ ((uint32_t)iz * 83492791u) ^ ((uint32_t)b * 2654435761u);
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// zero the bucket counters and the per-box maxima
__global__ __launch_bounds__(kClThreads) void k_cl_clear(ClusterParams p)
{
    const long long nb = p.ntab[1];
    for (long long e = blockIdx.x * (long long)kClThreads + threadIdx.x; e <= max(nb, (long long)p.in_cap);
         e += (long long)gridDim.x * kClThreads) {
        if (e <= nb) p.bstart[e] = 0;
        if (e < p.in_cap) p.best[e] = 0;
    }
}

__global__ __launch_bounds__(kClThreads) void k_cl_grid_count(ClusterParams p)
{
    if (cl_overflow(p)) return;
    const long long m = p.ntab[0];
    const uint32_t mask = (uint32_t)p.ntab[1] - 1u;
    for (long long e = blockIdx.x * (long long)kClThreads + threadIdx.x; e < m; e += (long long)gridDim.x * kClThreads) {
        const float4 v = p.crop_xyz[e];
        const int bk = (int)(cl_hash(p.crop_box[e], cl_cell(v.x), cl_cell(v.y), cl_cell(v.z)) & mask);
        p.bucket[e] = bk;
        p.parent[e] = (int)e;
        p.csize[e] = 0;
        atomicAdd(&p.bstart[bk], 1);
    }
}

__global__ __launch_bounds__(kClThreads) void k_cl_grid_scatter(ClusterParams p)
{
    if (cl_overflow(p)) return;
    const long long m = p.ntab[0];
    for (long long e = blockIdx.x * (long long)kClThreads + threadIdx.x; e < m; e += (long long)gridDim.x * kClThreads)
        p.sorted[atomicAdd(&p.bcur[p.bucket[e]], 1)] = (int)e;
}

// the edge predicate: ((dx*dx + dy*dy) + dz*dz) in fp32, every operation rounded, <= 0.01f^2 in double
__device__ inline bool cl_edge(float4 a, float4 b)
{
    const float dx = __fsub_rn(a.x, b.x), dy = __fsub_rn(a.y, b.y), dz = __fsub_rn(a.z, b.z);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return (double)d2 <= (double)0.01f * (double)0.01f;
}

__global__ __launch_bounds__(kClThreads) void k_cl_hook(ClusterParams p)
{
    if (cl_overflow(p)) return;
    const long long m = p.ntab[0];
    const uint32_t mask = (uint32_t)p.ntab[1] - 1u;
    for (long long e = blockIdx.x * (long long)kClThreads + threadIdx.x; e < m; e += (long long)gridDim.x * kClThreads) {
        const float4 v = p.crop_xyz[e];
        const int b = p.crop_box[e];
        const int ix = cl_cell(v.x), iy = cl_cell(v.y), iz = cl_cell(v.z);
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int bk = (int)(cl_hash(b, ix + dx, iy + dy, iz + dz) & mask);
                    const int s1 = p.bstart[bk + 1];
                    for (int s = p.bstart[bk]; s < s1; ++s) {
                        const int q = p.sorted[s];
                        if (q >= e || p.crop_box[q] != b) continue;
                        if (cl_edge(v, p.crop_xyz[q])) uf_unite(p.parent, (int)e, q);
                    }
                }
    }
}

__global__ __launch_bounds__(kClThreads) void k_cl_label(ClusterParams p)
{
    if (cl_overflow(p)) return;
    const long long m = p.ntab[0];
    for (long long e = blockIdx.x * (long long)kClThreads + threadIdx.x; e < m; e += (long long)gridDim.x * kClThreads) {
        const int root = uf_find(p.parent, (int)e);
        atomicAdd(&p.csize[root], 1);
    }
}

__global__ __launch_bounds__(kClThreads) void k_cl_best(ClusterParams p)
{
    if (cl_overflow(p)) return;
    const long long m = p.ntab[0];
    for (long long e = blockIdx.x * (long long)kClThreads + threadIdx.x; e < m; e += (long long)gridDim.x * kClThreads) {
        const int root = uf_root(p.parent, (int)e);
        p.parent[e] = root;                             // every label final for k_cl_out
        if (root == e)
            atomicMax(&p.best[p.crop_box[e]], ((unsigned long long)(uint32_t)p.csize[e] << 32) | (0xffffffffu - (uint32_t)e));
    }
}

// per box: the kept cluster's size, its first output index, and the needed total (one workgroup)
__global__ __launch_bounds__(kClThreads) void k_cl_select(ClusterParams p)
{
    __shared__ long long lds[kClWaves];
    const int n = cl_nbox(p);
    const bool ovf = cl_overflow(p);
    long long carry = 0;
    for (int b0 = 0; b0 < n; b0 += kClThreads) {
        const int b = b0 + threadIdx.x;
        const long long cnt = (b < n && !ovf) ? (long long)(p.best[b] >> 32) : 0;
        long long total;
        const long long ex = block_scan<long long, kClWaves>(cnt, lds, total);
        if (b < n) {
            p.obase[b] = carry + ex;
            p.counts[b] = (int32_t)cnt;
        }
        carry += total;
    }
    if (threadIdx.x == 0) p.status[1] = ovf ? -1 : carry;
}

// one workgroup per box: the winner's indices in crop order, and its centroid
__global__ __launch_bounds__(kClThreads) void k_cl_out(ClusterParams p)
{
    __shared__ int lds[kClWaves];
    __shared__ float4 stage[kClThreads];
    __shared__ float acc[3];
    const int n = cl_nbox(p);
    const bool ovf = cl_overflow(p);
    const long long need = p.status[1];
    const bool write = need >= 0 && need <= p.index_cap;
    for (int b = blockIdx.x; b < n; b += gridDim.x) {
        const long long cnt = ovf ? 0 : (long long)(p.best[b] >> 32);
        float *cen = p.centres + 3 * (size_t)b;
        if (cnt == 0) {
            if (threadIdx.x < 3) cen[threadIdx.x] = qnan_f();
            continue;
        }
        const int winner = (int)(0xffffffffu - (uint32_t)p.best[b]);
        const long long e1 = p.chunk_off[(long long)(b + 1) * p.nchunks];
        long long o = p.obase[b];
        if (threadIdx.x == 0) acc[0] = acc[1] = acc[2] = 0.f;
        for (long long s = winner; s < e1; s += kClThreads) {   // the root is the cluster's first point
            const long long e = s + threadIdx.x;
            const bool in = e < e1 && p.parent[e] == winner;
            int tot;
            const int rk = block_rank<kClWaves>(in, lds, tot);
            if (in) {
                if (write) p.indices[o + rk] = p.crop_idx[e];
                stage[rk] = p.crop_xyz[e];
            }
            __syncthreads();
            if (threadIdx.x == 0) {                     // the ordered fp32 sums of compute3DCentroid
                float sx = acc[0], sy = acc[1], sz = acc[2];
                for (int k = 0; k < tot; ++k) {
                    const float4 v = stage[k];
                    sx = __fadd_rn(sx, v.x); sy = __fadd_rn(sy, v.y); sz = __fadd_rn(sz, v.z);
                }
                acc[0] = sx; acc[1] = sy; acc[2] = sz;
            }
            __syncthreads();
            o += tot;
        }
        if (threadIdx.x < 3) cen[threadIdx.x] = __fdiv_rn(acc[threadIdx.x], (float)cnt);
        __syncthreads();
    }
}

int cl_grid(long long work, int per_block = kClThreads)
{
    return (int)std::max<long long>(std::min<long long>((work + per_block - 1) / per_block, kClMaxGrid), 1);
}

}  // namespace

void launch_camera_boxes(const CameraParams &p, hipStream_t s)
{
    PBD_LAUNCH(k_camera_boxes, dim3(cl_grid(p.in_cap, kClWaves)), dim3(kClThreads), 0, s, p);
}

void launch_cluster_step(const ClusterParams &p, int step, hipStream_t s)
{
    const long long units = (long long)p.in_cap * p.nchunks;
    const dim3 blk(kClThreads);
    switch (step) {
    case kClStepCropCount: PBD_LAUNCH(k_cl_crop_count, dim3(cl_grid(units, 1)), blk, 0, s, p); break;
    case kClStepCropScan:
        launch_scan<long long>(p.chunk_off, (long long *)nullptr, 0LL, (const long long *)(p.ntab + 2), p.part,
                               cl_grid(units, kScanTile), ClCropTotal{p.ntab, p.status, p.crop_cap, p.tcap}, s);
        break;
    case kClStepCropScatter: PBD_LAUNCH(k_cl_crop_scatter, dim3(cl_grid(units, 1)), blk, 0, s, p); break;
    case kClStepClear: PBD_LAUNCH(k_cl_clear, dim3(cl_grid(std::max<long long>(p.tcap, p.in_cap) + 1)), blk, 0, s, p); break;
    case kClStepGridCount: PBD_LAUNCH(k_cl_grid_count, dim3(cl_grid(p.crop_cap)), blk, 0, s, p); break;
    case kClStepGridScan:
        launch_scan<long long>(p.bstart, p.bcur, 0LL, (const long long *)(p.ntab + 1), p.part, cl_grid(p.tcap, kScanTile),
                               ScanNoTop{}, s);
        break;
    case kClStepGridScatter: PBD_LAUNCH(k_cl_grid_scatter, dim3(cl_grid(p.crop_cap)), blk, 0, s, p); break;
    case kClStepHook: PBD_LAUNCH(k_cl_hook, dim3(cl_grid(p.crop_cap)), blk, 0, s, p); break;
    case kClStepLabel: PBD_LAUNCH(k_cl_label, dim3(cl_grid(p.crop_cap)), blk, 0, s, p); break;
    case kClStepBest: PBD_LAUNCH(k_cl_best, dim3(cl_grid(p.crop_cap)), blk, 0, s, p); break;
    case kClStepSelect: PBD_LAUNCH(k_cl_select, dim3(1), blk, 0, s, p); break;
    default: PBD_LAUNCH(k_cl_out, dim3(cl_grid(p.in_cap, 1)), blk, 0, s, p); break;
    }
}

}  // namespace pbd
