// pbd_kernels_publish.hip -- the ROS node's two remaining products on the device: the candidate mask (pbd_candidate_mask*:
// Candidate::mask, include/Candidate.hpp:306-331, and `rgb & (mask != 0)`, ros/Messages.cpp:157-174) and the part-centre poses
// (pbd_part_poses*: messagePoses, ros/Messages.cpp:187-234).  include/pbd.h states both contracts.
//
// Mask, three launches over every frame of a call:
//   k_mk_init   the per-frame record ranges to (0, 0) and the bad-list flag to 0
//   k_mk_hull   one thread per record: the checks of a device list (count, frame range, grouping, nparts), the part hull
//               (cv::Rect operator|) clipped to the frame, and each frame's [first, end) record range
//   k_mk_tile   one workgroup per kMkTileW x kMkTileH pixel tile, one thread per kMkPix consecutive pixels of a row.  The frame's
//               records are read in rank order, kMkThreads at a time: each chunk's records that overlap the tile are compacted in
//               order into LDS, and every thread walks that list for its own still-unlabelled pixels.  The scan stops as soon as
//               every pixel of the tile is labelled, so a tile inside a box costs one chunk; the work is
//               sum over tiles of (records scanned until the tile is covered + the overlapping records walked), never
//               pixels x records.  The labels, then the masked colour bytes, are written in the same pass.
// Poses: k_part_poses, one thread per record (records number in the hundreds).
// Every float / double operation whose bits are compared is an explicitly rounded intrinsic, so none of them is contracted.
#include "pbd_device.h"
#include "pbd_jacobi.h"

#include <math.h>

namespace pbd {
namespace {

constexpr int kMkThreads = 256;
constexpr int kMkPix = 4;                               // consecutive pixels of one row per thread
constexpr int kMkTileW = 128;                           // kMkTileW / kMkPix threads per tile row
constexpr int kMkTileH = kMkThreads * kMkPix / kMkTileW;
constexpr int kMkMaxGrid = 4096;
constexpr int kPoseThreads = 64;

__global__ __launch_bounds__(kMkThreads) void k_mk_init(MaskParams p)
{
    for (int f = blockIdx.x * kMkThreads + threadIdx.x; f < p.nframes; f += gridDim.x * kMkThreads) {
        p.range[2 * f] = 0;
        p.range[2 * f + 1] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) p.bad[0] = 0;
}

// the record's frame index, or -1 when it is out of range
__device__ inline long long mk_frame(const MaskParams &p, const int32_t *r)
{
    const long long f = (long long)r[kRecFrame] - p.frame_offset;
    return f >= 0 && f < p.nframes ? f : -1;
}

__global__ __launch_bounds__(kMkThreads) void k_mk_hull(MaskParams p)
{
    const int n = p.in[0];
    if (n < 0 || n > p.in_cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(p.bad, 1);
        return;
    }
    for (int i = blockIdx.x * kMkThreads + threadIdx.x; i < n; i += gridDim.x * kMkThreads) {
        const int32_t *r = p.in + 1 + (size_t)i * p.stride;
        const long long f = mk_frame(p, r);
        const int np = r[kRecNparts];
        const long long fprev = i > 0 ? (long long)p.in[1 + (size_t)(i - 1) * p.stride + kRecFrame] - p.frame_offset : -1;
        const long long fnext = i + 1 < n ? (long long)p.in[1 + (size_t)(i + 1) * p.stride + kRecFrame] - p.frame_offset : -1;
        if (f < 0 || np < 1 || np > p.max_parts || (i > 0 && f < fprev)) {
            atomicOr(p.bad, 1);
            continue;
        }
        // boundingBox() & Rect(0, 0, cols, rows), as corners; an empty intersection is (0, 0, 0, 0) and paints nothing
        long long x, y, w, h;
        record_hull64(r, np, x, y, w, h);
        const MaskFrame &fr = p.frames[f];
        rect_and64(x, y, w, h, 0, 0, fr.cols, fr.rows);
        p.hull[i] = make_int4((int)x, (int)y, (int)(x + w), (int)(y + h));
        if (i == 0 || fprev != f) p.range[2 * f] = i;
        if (i + 1 == n || fnext != f) p.range[2 * f + 1] = i + 1;
    }
}

// byte k of the 4 * cn bytes of four consecutive pixels belongs to pixel k / cn
__device__ inline uint32_t mk_word_mask(const int lab[kMkPix], int cn, int w)
{
    uint32_t m = 0;
    for (int b = 0; b < 4; ++b)
        if (lab[(4 * w + b) / cn]) m |= 0xffu << (8 * b);
    return m;
}

__global__ __launch_bounds__(kMkThreads) void k_mk_tile(MaskParams p)
{
    __shared__ int4 lh[kMkThreads];
    __shared__ int lr[kMkThreads];
    __shared__ int wcount[kMkThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (p.bad[0]) {                                      // a bad list: the status word only
        if (blockIdx.x == 0 && t == 0 && p.status) p.status[0] = -1;
        return;
    }
    if (blockIdx.x == 0 && t == 0 && p.status) p.status[0] = p.in[0];
    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        int lo = 0, hi = p.nframes - 1;                  // the frame: the last one whose tile0 <= tile
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.frames[mid].tile0 <= tile) lo = mid;
            else hi = mid - 1;
        }
        const MaskFrame fr = p.frames[lo];
        const int tl = tile - fr.tile0, tiles_x = (fr.cols + kMkTileW - 1) / kMkTileW;
        const int X0 = (tl % tiles_x) * kMkTileW, Y0 = (tl / tiles_x) * kMkTileH;
        const int X1 = min(X0 + kMkTileW, fr.cols), Y1 = min(Y0 + kMkTileH, fr.rows);
        const int y = Y0 + t / (kMkTileW / kMkPix), x = X0 + (t % (kMkTileW / kMkPix)) * kMkPix;
        int lab[kMkPix];
        int todo = 0;                                    // bit k: pixel k is in the frame and still unlabelled
        for (int k = 0; k < kMkPix; ++k) {
            lab[k] = 0;
            if (y < fr.rows && x + k < fr.cols) todo |= 1 << k;
        }
        const int first = p.range[2 * lo], end = p.range[2 * lo + 1];
        for (int base = first; base < end; base += kMkThreads) {
            if (!__syncthreads_or(todo)) break;          // every pixel of the tile is labelled
            const int i = base + t;
            bool hit = false;
            int4 hb = make_int4(0, 0, 0, 0);
            if (i < end) {
                hb = p.hull[i];
                hit = hb.x < X1 && hb.z > X0 && hb.y < Y1 && hb.w > Y0;
            }
            const unsigned long long m = __ballot(hit);
            if (lane == 0) wcount[wv] = __popcll(m);
            __syncthreads();
            int off = 0, total = 0;
            for (int k = 0; k < kMkThreads / 64; ++k) {
                if (k < wv) off += wcount[k];
                total += wcount[k];
            }
            if (hit) {
                const int at = off + lane_rank(m);
                lh[at] = hb;
                lr[at] = i - first;
            }
            __syncthreads();
            for (int k = 0; k < total && todo; ++k) {
                const int4 b = lh[k];
                if (y < b.y || y >= b.w) continue;
                const int v = min(lr[k] + 1, 255);       // setTo(n+1, mask == 0) with saturate_cast<uchar>
                for (int q = 0; q < kMkPix; ++q)
                    if ((todo >> q & 1) && x + q >= b.x && x + q < b.z) {
                        lab[q] = v;
                        todo &= ~(1 << q);
                    }
            }
        }
        __syncthreads();                                 // the LDS list is rewritten by the next tile
        if (y >= fr.rows) continue;
        const int nv = min(kMkPix, fr.cols - x);
        if (nv <= 0) continue;
        if (fr.labels) {
            uint8_t *L = fr.labels + (size_t)y * fr.label_pitch + x;
            if (nv == kMkPix && !(reinterpret_cast<uintptr_t>(L) & 3)) {
                *reinterpret_cast<uint32_t *>(L) = (uint32_t)lab[0] | (uint32_t)lab[1] << 8 | (uint32_t)lab[2] << 16 |
                                                   (uint32_t)lab[3] << 24;
            } else {
                for (int k = 0; k < nv; ++k) L[k] = (uint8_t)lab[k];
            }
        }
        if (fr.masked) {
            const int cn = p.channels;
            const uint8_t *S = fr.colour + (size_t)y * fr.colour_pitch + (size_t)x * cn;
            uint8_t *D = fr.masked + (size_t)y * fr.masked_pitch + (size_t)x * cn;
            if (nv == kMkPix && cn == 4 && !((reinterpret_cast<uintptr_t>(S) | reinterpret_cast<uintptr_t>(D)) & 15)) {
                uint4 v = *reinterpret_cast<const uint4 *>(S);
                v.x &= mk_word_mask(lab, 4, 0); v.y &= mk_word_mask(lab, 4, 1);
                v.z &= mk_word_mask(lab, 4, 2); v.w &= mk_word_mask(lab, 4, 3);
                *reinterpret_cast<uint4 *>(D) = v;
            } else if (nv == kMkPix && !((reinterpret_cast<uintptr_t>(S) | reinterpret_cast<uintptr_t>(D)) & 3)) {
                uint32_t v[4];
                for (int w = 0; w < cn; ++w) v[w] = reinterpret_cast<const uint32_t *>(S)[w];
                for (int w = 0; w < cn; ++w) reinterpret_cast<uint32_t *>(D)[w] = v[w] & mk_word_mask(lab, cn, w);
            } else {
                for (int b = 0; b < nv * cn; ++b) D[b] = lab[b / cn] ? S[b] : 0;
            }
        }
    }
}

// messagePoses for one record: computeMeanAndCovarianceMatrix, covMat /= count, eigen33, Quaternion(evecs).normalize()
__global__ __launch_bounds__(kPoseThreads) void k_part_poses(PoseParams p)
{
    const int n = payload_count(p.count_word, p.cap);
    for (int i = blockIdx.x * kPoseThreads + threadIdx.x; i < n; i += gridDim.x * kPoseThreads) {
        int nc = p.ncentres[i];
        if (nc < 0 || nc > p.max_parts) nc = 0;
        const bool dense = p.dense[i] != 0;
        const float *P = p.centres + (size_t)i * p.max_parts * 3;
        float a[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};    // xx, xy, xz, yy, yz, zz, x, y, z
        int cnt = 0;
        for (int j = 0; j < nc; ++j) {
            const float x = P[3 * j], y = P[3 * j + 1], z = P[3 * j + 2];
            if (!dense && !(isfinite(x) && isfinite(y) && isfinite(z))) continue;
            a[0] = __fadd_rn(a[0], __fmul_rn(x, x));
            a[1] = __fadd_rn(a[1], __fmul_rn(x, y));
            a[2] = __fadd_rn(a[2], __fmul_rn(x, z));
            a[3] = __fadd_rn(a[3], __fmul_rn(y, y));
            a[4] = __fadd_rn(a[4], __fmul_rn(y, z));
            a[5] = __fadd_rn(a[5], __fmul_rn(z, z));
            a[6] = __fadd_rn(a[6], x);
            a[7] = __fadd_rn(a[7], y);
            a[8] = __fadd_rn(a[8], z);
            ++cnt;
        }
        p.count[i] = cnt;
        float *pos = p.position + 3 * (size_t)i, *quat = p.orientation + 4 * (size_t)i, *ev = p.eigenvalues + 3 * (size_t)i;
        const float qn = qnan_f();
        if (cnt == 0) {                                  // "Centroid not found": the node's `continue`
            for (int k = 0; k < 3; ++k) { pos[k] = qn; ev[k] = qn; }
            for (int k = 0; k < 4; ++k) quat[k] = qn;
            continue;
        }
        const float fc = (float)cnt;
        float m[9];
        for (int k = 0; k < 9; ++k) m[k] = __fdiv_rn(a[k], fc);
        float c[6] = {__fsub_rn(m[0], __fmul_rn(m[6], m[6])), __fsub_rn(m[1], __fmul_rn(m[6], m[7])),
                      __fsub_rn(m[2], __fmul_rn(m[6], m[8])), __fsub_rn(m[3], __fmul_rn(m[7], m[7])),
                      __fsub_rn(m[4], __fmul_rn(m[7], m[8])), __fsub_rn(m[5], __fmul_rn(m[8], m[8]))};
        bool finite = true;
        for (int k = 0; k < 6; ++k) {
            c[k] = __fdiv_rn(c[k], fc);                  // the node's second division (ros/Messages.cpp:212)
            finite = finite && isfinite(c[k]);
        }
        pos[0] = m[6]; pos[1] = m[7]; pos[2] = m[8];
        if (!finite) {
            for (int k = 0; k < 3; ++k) ev[k] = qn;
            for (int k = 0; k < 4; ++k) quat[k] = qn;
            continue;
        }
        double A[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}}, V[3][3];
        jacobi3(A, V);
        int o[3] = {0, 1, 2};                            // ascending eigenvalues, ties in index order (a stable insertion sort)
        for (int k = 1; k < 3; ++k)
            for (int j = k; j > 0 && A[o[j]][o[j]] < A[o[j - 1]][o[j - 1]]; --j) {
                const int s = o[j]; o[j] = o[j - 1]; o[j - 1] = s;
            }
        double M[3][3];                                  // columns: the eigenvectors of the two smallest, then their cross product
        for (int col = 0; col < 2; ++col) {
            double v[3] = {V[0][o[col]], V[1][o[col]], V[2][o[col]]};
            int big = 0;
            for (int k = 1; k < 3; ++k)
                if (fabs(v[k]) > fabs(v[big])) big = k;
            const bool neg = v[big] < 0.0;
            for (int k = 0; k < 3; ++k) M[k][col] = neg ? -v[k] : v[k];
        }
        M[0][2] = __dsub_rn(__dmul_rn(M[1][0], M[2][1]), __dmul_rn(M[2][0], M[1][1]));
        M[1][2] = __dsub_rn(__dmul_rn(M[2][0], M[0][1]), __dmul_rn(M[0][0], M[2][1]));
        M[2][2] = __dsub_rn(__dmul_rn(M[0][0], M[1][1]), __dmul_rn(M[1][0], M[0][1]));
        for (int k = 0; k < 3; ++k) ev[k] = (float)A[o[k]][o[k]];
        double q[4];                                     // x, y, z, w (Eigen's coefficient order)
        const double tr = __dadd_rn(__dadd_rn(M[0][0], M[1][1]), M[2][2]);
        if (tr > 0.0) {
            double s = __dsqrt_rn(__dadd_rn(tr, 1.0));
            q[3] = __dmul_rn(0.5, s);
            s = __ddiv_rn(0.5, s);
            q[0] = __dmul_rn(__dsub_rn(M[2][1], M[1][2]), s);
            q[1] = __dmul_rn(__dsub_rn(M[0][2], M[2][0]), s);
            q[2] = __dmul_rn(__dsub_rn(M[1][0], M[0][1]), s);
        } else {
            int ii = 0;
            if (M[1][1] > M[0][0]) ii = 1;
            if (M[2][2] > M[ii][ii]) ii = 2;
            const int jj = (ii + 1) % 3, kk = (jj + 1) % 3;
            double s = __dsqrt_rn(__dadd_rn(__dsub_rn(__dsub_rn(M[ii][ii], M[jj][jj]), M[kk][kk]), 1.0));
            q[ii] = __dmul_rn(0.5, s);
            s = __ddiv_rn(0.5, s);
            q[3] = __dmul_rn(__dsub_rn(M[kk][jj], M[jj][kk]), s);
            q[jj] = __dmul_rn(__dadd_rn(M[jj][ii], M[ii][jj]), s);
            q[kk] = __dmul_rn(__dadd_rn(M[kk][ii], M[ii][kk]), s);
        }
        const double nrm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(q[0], q[0]), __dmul_rn(q[1], q[1])),
                                                          __dmul_rn(q[2], q[2])), __dmul_rn(q[3], q[3])));
        for (int k = 0; k < 4; ++k) quat[k] = (float)__ddiv_rn(q[k], nrm);
    }
}

}  // namespace

void launch_mask(const MaskParams &p, int step, hipStream_t s)
{
    if (step == kMkStepHull) {
        PBD_LAUNCH(k_mk_init, dim3(std::max(1, std::min((p.nframes + kMkThreads - 1) / kMkThreads, kMkMaxGrid))), dim3(kMkThreads),
                   0, s, p);
        PBD_LAUNCH(k_mk_hull, dim3(std::max(1, std::min((p.in_cap + kMkThreads - 1) / kMkThreads, kMkMaxGrid))), dim3(kMkThreads), 0,
                   s, p);
    } else {
        PBD_LAUNCH(k_mk_tile, dim3(std::max(1, std::min(p.ntiles, 1 << 20))), dim3(kMkThreads), 0, s, p);
    }
}

long long mask_tiles(int rows, int cols)
{
    return (long long)((cols + kMkTileW - 1) / kMkTileW) * ((rows + kMkTileH - 1) / kMkTileH);
}

void launch_part_poses(const PoseParams &p, hipStream_t s)
{
    PBD_LAUNCH(k_part_poses, dim3(std::max(1, std::min((p.cap + kPoseThreads - 1) / kPoseThreads, kMkMaxGrid))), dim3(kPoseThreads), 0,
               s, p);
}

}  // namespace pbd
