// pbd_kernels_partscores.hip -- the score of each part of a detection (pbd_part_scores*, pbd_score_placements*): what the dynamic
// program added up for a record, taken apart again at the record's placement.  include/pbd.h states the contract, DESIGN.md
// section 6s the rule and the cost; partsbaseddetector_amd/partscores.py is the rule in numpy.
//
// Two launches over the records of a payload (word 0 = count, read on the device):
//   k_ps_walk   one thread per record: the checks of the record against the resident result and the walk through the resident
//               back-pointer maps (walk_child, as the candidates' walk and k_ex_walk), which leaves status[i] and place[i][p] =
//               {x, y, m}.  With placements given by the caller (place_in) it checks those instead and walks nothing.  It has
//               no real type: nothing it reads or writes is a score.
//   k_ps_score  one wavefront (= one workgroup) per record.  Lanes own parts (lane, lane + 64, ...): each gathers its part's
//               resident response, bias, deformation weights and displacement, so the loads of all parts are in flight at
//               once.  Then one lane runs the accumulation over LDS in the order of the rule -- children in descending index,
//               each message two roundings (quad_val along x, then along y, as the transform's row and column passes), each
//               add in T -- and the lanes write the values out.  A record's values depend on nothing but the record.
// Compiled without contraction, as pbd_kernels_dp.hip is: quad_val of pbd_dp.h is the statement the transform runs.
#include "pbd_dp.h"

#include <algorithm>

namespace pbd {
namespace {

constexpr int kPsWalkThreads = 128;
constexpr int kPsMaxGrid = 16384;

template <typename PT>
__global__ __launch_bounds__(kPsWalkThreads) void k_ps_walk(PartScoreParams p)
{
    const int n = min(max(p.in[0], 0), p.in_cap);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int32_t *rec = p.in + 1 + (size_t)i * p.stride;
        const long long f = (long long)rec[0] - p.frame_offset;
        const int c = rec[1], l = rec[2], rx = rec[3], ry = rec[4];
        const RecordLevel rl = record_level(f, l, p.nframes, p.nlevels, p.frame_lv0);
        bool ok = rl.vl >= 0 && c >= 0 && c < p.NC;
        LevelDesc d{};
        if (ok) {
            d = p.lv[rl.vl];
            // a level of another rank of a sharded handle is 0 x 0; given placements bring their own root cell
            ok = p.place_in ? d.cols > 0 && d.rows > 0 : rx >= 0 && rx < d.cols && ry >= 0 && ry < d.rows;
        }
        if (!ok) { p.status[i] = -1; continue; }
        const PartWalk *walk = p.walk + p.walk_off[c];
        const int nparts = p.walk_off[c + 1] - p.walk_off[c];
        if (p.place_in) {
            const int32_t *src = p.place_in + (size_t)i * p.max_parts * 3;
            const int *nmix = p.part_nmix + p.walk_off[c];
            for (int q = 0; q < nparts; ++q) {
                const int x = src[3 * q], y = src[3 * q + 1], m = src[3 * q + 2];
                ok = ok && x >= 0 && x < d.cols && y >= 0 && y < d.rows && m >= 0 && m < nmix[q];
            }
            p.status[i] = ok ? nparts : -1;
            continue;
        }
        const LevelPlanes<PartScoreParams> pl(p, d, rl.bf);
        int32_t *place = p.place + (size_t)i * p.max_parts * 3;
        place[0] = rx; place[1] = ry;
        place[2] = *pl.rooti((size_t)c * pl.HW + (size_t)ry * d.cols + rx);
        for (int q = 1; q < nparts; ++q) {
            const PartWalk w = walk[q];
            const int32_t *par = place + 3 * w.parent;
            const WalkPos ch = walk_child<PT>(pl, w, par[0], par[1], par[2], p.walk_mode == PBD_WALK_ARGMAX);
            place[3 * q] = ch.x; place[3 * q + 1] = ch.y; place[3 * q + 2] = ch.m;
        }
        p.status[i] = nparts;
    }
}

template <typename R>
__global__ __launch_bounds__(64) void k_ps_score(PartScoreParams p)
{
    __shared__ R s_total[kWalkMaxParts], s_msg[kWalkMaxParts], s_bias[kWalkMaxParts];
    __shared__ float4 s_w[kWalkMaxParts];             // the part's deformation weights w0 .. w3
    __shared__ int s_par[kWalkMaxParts], s_dx[kWalkMaxParts], s_dy[kWalkMaxParts];
    const int n = min(max(p.in[0], 0), p.in_cap);
    const int lane = threadIdx.x;
    const int32_t *places = p.place_in ? p.place_in : p.place;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {           // every branch on i is the whole workgroup's
        const int nparts = min(p.status[i], kWalkMaxParts);
        if (nparts <= 0) continue;
        const int32_t *rec = p.in + 1 + (size_t)i * p.stride;
        const int c = rec[1];
        const RecordLevel rl = record_level((long long)rec[0] - p.frame_offset, rec[2], p.nframes, p.nlevels, p.frame_lv0);
        const LevelDesc d = p.lv[rl.vl];                        // k_ps_walk accepted the record: the level exists
        const LevelPlanes<PartScoreParams> pl(p, d, rl.bf);
        const PartWalk *walk = p.walk + p.walk_off[c];
        const int32_t *place = places + (size_t)i * p.max_parts * 3;
        R *out = static_cast<R *>(p.scores) + (size_t)i * p.max_parts * 4;
        for (int q = lane; q < nparts; q += 64) {
            const PartWalk w = walk[q];
            const int x = place[3 * q], y = place[3 * q + 1], m = place[3 * q + 2];
            const ExGm g = p.gm[w.mix0 + m];
            const R app = pl.template score<R>(false, p.resp_half != 0, g.filterid, (size_t)y * d.cols + x)[0];
            R bias;
            int dx = 0, dy = 0;
            float4 dw = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q == 0) {
                // the root's bias is that of mixture 0 for every root mixture (src/DynamicProgram.cpp:163-170)
                bias = (R)p.biasw[p.gm[w.mix0].biasid];
            } else {
                const int32_t *par = place + 3 * w.parent;
                bias = (R)p.biasw[g.biasid + par[2]];           // bias(mm)[pm] (include/Parts.hpp:172-175)
                // the row pass charged a (os - v)^2 + b (os - v), os = px + anchor x, v = x (columns likewise)
                dx = par[0] + p.anchors[2 * g.defid] - x;
                dy = par[1] + p.anchors[2 * g.defid + 1] - y;
                dw = *reinterpret_cast<const float4 *>(p.defw + 4 * (size_t)g.defid);
            }
            s_total[q] = app; s_bias[q] = bias; s_w[q] = dw;
            s_par[q] = w.parent; s_dx[q] = dx; s_dy[q] = dy;
            out[4 * q] = app;
            out[4 * q + 2] = bias;
        }
        __syncthreads();
        if (lane == 0) {
            for (int q = nparts - 1; q >= 1; --q) {             // the reference's descending child order
                const float4 w = s_w[q];
                const R r = quad_val<R, false>((double)(-w.x), (double)(-w.y), s_dx[q], s_total[q]);
                const R msg = quad_val<R, false>((double)(-w.z), (double)(-w.w), s_dy[q], r);
                s_msg[q] = msg;
                const int par = s_par[q];
                s_total[par] = s_total[par] + (msg + s_bias[q]);
            }
            s_msg[0] = s_total[0] + s_bias[0];
        }
        __syncthreads();
        for (int q = lane; q < nparts; q += 64) {
            out[4 * q + 1] = s_msg[q];
            out[4 * q + 3] = s_total[q];
        }
        __syncthreads();                                        // the next record rewrites the arrays
    }
}

}  // namespace

void launch_part_scores(const PartScoreParams &p, bool f64, int step, hipStream_t s)
{
    if (p.in_cap <= 0) return;
    if (step == 0) {
        const dim3 grid(std::max(1, std::min((p.in_cap + kPsWalkThreads - 1) / kPsWalkThreads, kPsMaxGrid)));
        if (p.ptr8) PBD_LAUNCH(k_ps_walk<uint8_t>, grid, dim3(kPsWalkThreads), 0, s, p);
        else PBD_LAUNCH(k_ps_walk<int16_t>, grid, dim3(kPsWalkThreads), 0, s, p);
        return;
    }
    const dim3 grid(std::max(1, std::min(p.in_cap, kPsMaxGrid)));
    if (f64) PBD_LAUNCH(k_ps_score<double>, grid, dim3(64), 0, s, p);
    else PBD_LAUNCH(k_ps_score<float>, grid, dim3(64), 0, s, p);
}

}  // namespace pbd
