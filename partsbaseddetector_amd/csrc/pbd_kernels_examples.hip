// pbd_kernels_examples.hip -- training examples of records (pbd_examples*): the block-sparse feature vector the reference's
// Matlab training code writes for a detection (matlab/detection/detect.m backtrack + qp_write).  include/pbd.h states the
// contract, DESIGN.md section 6h the cost.
//
// Two launches over the records of a payload (word 0 = count, read on the device):
//   k_ex_walk    one thread per record: the checks of the record against the resident result, the walk through the resident
//                back-pointer maps (walk_child, as the candidates' walk), the header, the bias and deformation values, and one
//                ExPart per (record, part) for the gather
//   k_ex_gather  one wavefront per (record, part): the k x k x flen feature window, read as 16-byte chunks (a cell is 32 values,
//                so a chunk never straddles two cells and every source chunk is 16-byte aligned) and written as 16-byte chunks at
//                the block's place in the value row (dword aligned: the blocks before it have odd lengths).  A chunk outside the
//                feature map is filled with the convolution's border values without a read.
#include "pbd_dp.h"

namespace pbd {
namespace {

constexpr int kExFlen = 32;                 // channels per cell (build_model refuses any other flen)
constexpr int kExWalkThreads = 128;
constexpr int kExGatherWaves = 4;
constexpr int kExMaxGrid = 8192;

template <typename R> struct RealMax;
template <> struct RealMax<float> { static __device__ __forceinline__ float v() { return 3.402823466e38f; } };
template <> struct RealMax<double> { static __device__ __forceinline__ double v() { return 1.7976931348623157e308; } };

template <typename R, typename PT>
__global__ __launch_bounds__(kExWalkThreads) void k_ex_walk(ExampleParams p)
{
    const int n = min(max(p.in[0], 0), p.in_cap);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int32_t *rec = p.in + 1 + (size_t)i * p.stride;
        const long long f = (long long)rec[0] - p.frame_offset;
        const int c = rec[1], l = rec[2], rx = rec[3], ry = rec[4];
        int32_t *hdr = p.hdr + (size_t)i * p.hdr_words;
        ExPart *parts = p.parts + (size_t)i * p.max_parts;
        // (frame, level) of the record -> (frame of the buffers, level of the plan); mixed plans: frame 0, the virtual level
        const RecordLevel rl = record_level(f, l, p.nframes, p.nlevels, p.frame_lv0);
        const int bf = rl.bf, vl = rl.vl;
        bool ok = vl >= 0 && c >= 0 && c < p.NC;
        LevelDesc d{};
        if (ok) {
            d = p.lv[vl];
            ok = rx >= 0 && rx < d.cols && ry >= 0 && ry < d.rows;   // a level of another rank of a sharded handle is 0 x 0
        }
        hdr[0] = i;
        hdr[1] = c;
        if (!ok) {
            hdr[2] = -1;
            for (int w = 3; w < p.hdr_words; ++w) hdr[w] = 0;
            for (int q = 0; q < p.max_parts; ++q) parts[q].k = 0;
            continue;
        }
        const LevelPlanes<ExampleParams> pl(p, d, bf);
        const PartWalk *walk = p.walk + p.walk_off[c];
        const int nparts = p.walk_off[c + 1] - p.walk_off[c];
        R *vals = static_cast<R *>(p.values) + (size_t)i * p.vstride;
        int nb = 0;
        long long nv = 0;
        for (int pidx = 0; pidx < nparts; ++pidx) {
            const PartWalk w = walk[pidx];
            int x, y, m, pm = 0, px = 0, py = 0;
            if (pidx == 0) {
                x = rx; y = ry;
                m = *pl.rooti((size_t)c * pl.HW + (size_t)ry * d.cols + rx);
            } else {
                const ExPart &par = parts[w.parent];
                px = par.x; py = par.y; pm = par.m;
                const WalkPos ch = walk_child<PT>(pl, w, px, py, pm, p.walk_mode == PBD_WALK_ARGMAX);
                x = ch.x; y = ch.y; m = ch.m;
            }
            const ExGm g = p.gm[w.mix0 + m];
            // bias: the root's is that of mixture 0 for every root mixture (src/DynamicProgram.cpp:163-170); a child's is
            // bias(mm)[pm] = biasw[biasid[mm] + pm] (include/Parts.hpp:172-175)
            hdr[4 + 2 * nb] = pidx == 0 ? p.gm[w.mix0].biasid : g.biasid + pm;
            hdr[5 + 2 * nb] = 1;
            ++nb;
            vals[nv++] = (R)1;
            if (pidx > 0) {
                // the row pass charged a(os - v)^2 + b(os - v), os = px + anchor x, v = x, with a = -w0, b = -w1 (columns likewise)
                const int dx = px + p.anchors[2 * g.defid] - x, dy = py + p.anchors[2 * g.defid + 1] - y;
                hdr[4 + 2 * nb] = p.nbias + 4 * g.defid;
                hdr[5 + 2 * nb] = 4;
                ++nb;
                vals[nv++] = (R)(-(dx * dx));
                vals[nv++] = (R)(-dx);
                vals[nv++] = (R)(-(dy * dy));
                vals[nv++] = (R)(-dy);
            }
            const int k = w.ksize[m];
            hdr[4 + 2 * nb] = (int)(p.nbias + 4LL * p.ndefs + p.foff[g.filterid]);
            hdr[5 + 2 * nb] = k * k * kExFlen;
            ++nb;
            ExPart e{};
            e.cell = (long long)pl.cell; e.dst = (long long)i * p.vstride + nv;
            e.x = x; e.y = y; e.m = m; e.k = k; e.W = d.cols; e.H = d.rows;
            parts[pidx] = e;
            nv += (long long)k * k * kExFlen;
        }
        for (int q = nparts; q < p.max_parts; ++q) parts[q].k = 0;
        hdr[2] = nb;
        hdr[3] = (int)nv;
        for (int w = 4 + 2 * nb; w < p.hdr_words; ++w) hdr[w] = 0;
    }
}

template <typename R>
__global__ __launch_bounds__(64 * kExGatherWaves) void k_ex_gather(ExampleParams p)
{
    constexpr int V = 16 / sizeof(R);                 // values per 16-byte chunk
    constexpr int CPC = kExFlen / V;                  // chunks per cell (8 float, 16 double)
    typedef R vload __attribute__((ext_vector_type(V)));                        // 16-byte aligned source chunk
    typedef R vstore __attribute__((ext_vector_type(V), aligned(sizeof(R))));  // dword-aligned destination chunk
    const int n = min(max(p.in[0], 0), p.in_cap);
    const long long npairs = (long long)n * p.max_parts;
    const int lane = threadIdx.x & 63;
    for (long long t = (long long)blockIdx.x * kExGatherWaves + (threadIdx.x >> 6); t < npairs; t += (long long)gridDim.x * kExGatherWaves) {
        const ExPart e = p.parts[t];
        if (e.k <= 0) continue;
        const int rowc = e.k * CPC;                   // chunks per window row
        const int total = e.k * rowc;
        const int x0 = e.x - e.k / 2, y0 = e.y - e.k / 2;   // OpenCV's centred anchor Point(-1, -1)
        const R *feat = static_cast<const R *>(p.feat) + (size_t)e.cell * kExFlen;
        R *dst = static_cast<R *>(p.values) + e.dst;
        int r = lane / rowc, q = lane - r * rowc;     // row and chunk within the row of chunk j, advanced by 64 per step
        for (int j = lane; j < total; j += 64) {
            const int cx = x0 + q / CPC, cy = y0 + r, ch = (q % CPC) * V;
            vload v;
            if (cx >= 0 && cx < e.W && cy >= 0 && cy < e.H) {
                v = *reinterpret_cast<const vload *>(feat + ((size_t)cy * e.W + cx) * kExFlen + ch);
            } else {   // border: 0 on channels 0..flen-2, 1 on channel flen-1 (src/SpatialConvolutionEngine.cpp:146-156)
#pragma unroll
                for (int u = 0; u < V; ++u) v[u] = (ch + u == kExFlen - 1) ? (R)1 : (R)0;
            }
            *reinterpret_cast<vstore *>(dst + (size_t)j * V) = v;
            q += 64;
            while (q >= rowc) { q -= rowc; ++r; }
        }
    }
}

// ---- latent positives (pbd_detect_latent) --------------------------------------------------------------------------------
// one thread per response value of the latent bank: the plane of (part p, mixture m) at (x, y) of level l keeps its value only
// when m is allowed and the part's record rectangle (src/DynamicProgram.cpp:238-241) overlaps the frame's box of part p by more
// than `overlap` (testoverlap: inclusive areas, in double); otherwise it becomes -1e10 (Matlab's -INF, finite), or
// kLatentMaskHalf where the responses are fp16 (RH)
template <typename R, bool RH = false>
__global__ __launch_bounds__(256) void k_latent_mask(LatentParams p)
{
    const long long total = p.cell_per_frame * p.F;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
        const int lo = level_of(p.lv, 0, p.nlevels, o, p.F);
        const LevelDesc d = p.lv[lo];
        const int HW = d.rows * d.cols;
        if (HW == 0) continue;
        const long long rem = o - d.cell_off * p.F;
        const int gm = (int)(rem / HW), local = (int)(rem - (long long)gm * HW);
        const int x = local % d.cols, y = local / d.cols;
        const int4 g = p.gmtab[gm];
        const int f = p.lv_frame[lo];
        bool keep = !p.mix || p.mix[f * p.nparts + g.x] < 0 || p.mix[f * p.nparts + g.x] == g.y;
        if (keep) {
            const PartRect r = part_rect<R>(x, y, g.z, (R)p.scales[lo], d);
            const long long rx1 = r.x1, ry1 = r.y1, rx2 = r.x2, ry2 = r.y2;
            const int4 b = p.boxes[f * p.nparts + g.x];
            const long long iw = max(0LL, min(rx2, (long long)b.z) - max(rx1, (long long)b.x) + 1);
            const long long ih = max(0LL, min(ry2, (long long)b.w) - max(ry1, (long long)b.y) + 1);
            const double inter = (double)iw * (double)ih;
            const double area = (double)(rx2 - rx1 + 1) * (double)(ry2 - ry1 + 1);
            const double barea = (double)((long long)b.z - b.x + 1) * (double)((long long)b.w - b.y + 1);
            keep = inter / (area + barea - inter) > p.overlap;
        }
        if (!keep) {
            if constexpr (RH) static_cast<_Float16 *>(p.resp)[o] = (_Float16)kLatentMaskHalf;
            else static_cast<R *>(p.resp)[o] = (R)-1e10;
        }
    }
}

// one workgroup per frame: the highest root score over the frame's levels, components and positions; on a tie the first in
// (level, component, y, x) order.  Writes the frame's record header as k_argmin_emit does (root_record: virtual frame 0, virtual level)
template <typename R>
__global__ __launch_bounds__(256) void k_latent_best(LatentParams p)
{
    const int f = blockIdx.x;
    const long long b0 = p.lv[p.frame_lv0[f]].cell_off * p.NC;
    const long long b1 = (p.frame_lv0[f + 1] < p.nlevels ? p.lv[p.frame_lv0[f + 1]].cell_off : p.cell_per_frame) * p.NC;
    const R *rv = static_cast<const R *>(p.rootv);
    R best = -RealMax<R>::v();
    long long bi = -1;
    for (long long o = b0 + threadIdx.x; o < b1; o += blockDim.x)
        if (bi < 0 || rv[o] > best) { best = rv[o]; bi = o; }
    __shared__ R sv[256];
    __shared__ long long si[256];
    sv[threadIdx.x] = best; si[threadIdx.x] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const R v2 = sv[threadIdx.x + w];
            const long long i2 = si[threadIdx.x + w];
            if (i2 >= 0 && (si[threadIdx.x] < 0 || v2 > sv[threadIdx.x] || (v2 == sv[threadIdx.x] && i2 < si[threadIdx.x]))) {
                sv[threadIdx.x] = v2; si[threadIdx.x] = i2;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const long long o = si[0];
    root_record(p.payload + 1 + (size_t)f * p.stride, p.lv, p.frame_lv0[f], p.frame_lv0[f + 1], p.NC, 0, o, rv[o], p.rooti[o]);
    if (f == 0) p.payload[0] = p.nframes;
}

}  // namespace

void launch_latent_mask(const LatentParams &p, bool f64, hipStream_t s)
{
    const long long total = p.cell_per_frame * p.F;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((total + 255) / 256, 65536)));
    if (f64) PBD_LAUNCH(k_latent_mask<double>, grid, dim3(256), 0, s, p);
    else if (p.resp_half) PBD_LAUNCH((k_latent_mask<float, true>), grid, dim3(256), 0, s, p);
    else PBD_LAUNCH(k_latent_mask<float>, grid, dim3(256), 0, s, p);
}

void launch_latent_best(const LatentParams &p, bool f64, hipStream_t s)
{
    if (f64) PBD_LAUNCH(k_latent_best<double>, dim3(p.nframes), dim3(256), 0, s, p);
    else PBD_LAUNCH(k_latent_best<float>, dim3(p.nframes), dim3(256), 0, s, p);
}

void launch_examples(const ExampleParams &p, bool f64, int step, hipStream_t s)
{
    if (p.in_cap <= 0) return;
    if (step == 0) {
        const dim3 grid(std::max(1, std::min((p.in_cap + kExWalkThreads - 1) / kExWalkThreads, kExMaxGrid)));
        if (p.ptr8) {
            if (f64) PBD_LAUNCH((k_ex_walk<double, uint8_t>), grid, dim3(kExWalkThreads), 0, s, p);
            else PBD_LAUNCH((k_ex_walk<float, uint8_t>), grid, dim3(kExWalkThreads), 0, s, p);
        } else {
            if (f64) PBD_LAUNCH((k_ex_walk<double, int16_t>), grid, dim3(kExWalkThreads), 0, s, p);
            else PBD_LAUNCH((k_ex_walk<float, int16_t>), grid, dim3(kExWalkThreads), 0, s, p);
        }
        return;
    }
    const long long pairs = (long long)p.in_cap * p.max_parts;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((pairs + kExGatherWaves - 1) / kExGatherWaves, kExMaxGrid)));
    if (f64) PBD_LAUNCH(k_ex_gather<double>, grid, dim3(64 * kExGatherWaves), 0, s, p);
    else PBD_LAUNCH(k_ex_gather<float>, grid, dim3(64 * kExGatherWaves), 0, s, p);
}

}  // namespace pbd
