// pbd_kernels_marginals.hip -- the max-marginals of every part and the poses they decode to (pbd_max_marginals,
// pbd_marginal_poses*; gfx950).  include/pbd.h states the contract, DESIGN.md section 6t the rule and the cost;
// partsbaseddetector_amd/marginals.py is the rule in numpy.
//
// The downward half of the dynamic program.  The transforms themselves -- the upward ones re-run for the messages, the mirrored
// ones of the downward pass -- are the detect path's launch_dt_rows / launch_dt_cols on job tables of this call; the kernels here
// are what stands around them, all streaming over the level planes of one frame, a thread = four consecutive cells of a level
// (k_dp_combine's cut of the frame), every plane read and written once per launch with accesses of four elements:
//   k_mm_messages  M_p[mq] of every parent type mq from the transforms D_p[m] of one part (grid.y), the reduction k_dp_combine runs
//   k_mm_context   C_p[mq]: the parent's response plus its other children's messages in descending order plus its down plane
//   k_mm_down      the reduction over the parent's types of one part's mirrored transforms: down, Jk, the composed Jx / Jy, mm;
//                  a part whose transforms do not fit one slice of the scratch resumes from the planes the slice before left
//   k_mm_decode    one thread per seed: the climb to the root through Jk / Jx / Jy, then walk_child for the parts off the path
// Shared rules (reduce_max / pick_max, walk_child, part_rect, level_of) are pbd_dp.h's.  Compiled without contraction.
#include "pbd_dp.h"

#include <algorithm>
#include <type_traits>

namespace pbd {
namespace {

template <typename T> struct Vec4;
#define PBD_VEC4(T, E) template <> struct Vec4<T> { typedef E type __attribute__((ext_vector_type(4), aligned(sizeof(E)))); }
PBD_VEC4(float, float); PBD_VEC4(double, double); PBD_VEC4(int16_t, short); PBD_VEC4(int8_t, signed char);
#undef PBD_VEC4

// n valid cells (1..4) of a plane: one access of four elements while the group is whole
template <typename T> __device__ __forceinline__ void ld4(const T *src, int n, T *dst)
{
    if (n == 4) {
        const typename Vec4<T>::type v = *reinterpret_cast<const typename Vec4<T>::type *>(src);
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[e] = (T)v[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[e] = e < n ? src[e] : (T)0;
    }
}
template <typename T> __device__ __forceinline__ void st4(T *dst, int n, const T *src)
{
    if (n == 4) {
        typename Vec4<T>::type v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = src[e];
        *reinterpret_cast<typename Vec4<T>::type *>(dst) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (e < n) dst[e] = src[e];
    }
}

// the thread's group of four cells: its level, first cell inside the level and valid cells (0: none)
struct Quad { LevelDesc d; int local, n; size_t HW; };
__device__ __forceinline__ Quad quad_of(const MmParams &p)
{
    Quad q{};
    const long long qidx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (qidx >= p.quad_per_frame) return q;
    q.d = p.lv[level_of<&LevelDesc::quad_off>(p.lv, 0, p.nlevels, qidx)];
    const int HWi = q.d.rows * q.d.cols;
    q.HW = (size_t)HWi;
    q.local = (int)(qidx - q.d.quad_off) * 4;
    q.n = q.local < HWi ? min(4, HWi - q.local) : 0;
    return q;
}
// element `local` of plane `plane` of the level's block in a buffer of `planes` planes per cell block
template <typename T> __device__ __forceinline__ T *plane_at(void *base, const Quad &q, long long cell0, int planes, int plane)
{
    return static_cast<T *>(base) + ((size_t)(cell0 + q.d.cell_off) * planes + (size_t)plane * q.HW + q.local);
}
template <typename T> __device__ __forceinline__ const T *plane_at(const void *base, const Quad &q, long long cell0, int planes, int plane)
{
    return static_cast<const T *>(base) + ((size_t)(cell0 + q.d.cell_off) * planes + (size_t)plane * q.HW + q.local);
}

// ---- messages: block.y = one part of an upward depth group ---------------------------------------------------------------------
// MAXM: compile-time bound on the types per part of the model (the register array of running maxima is sized by it)
template <typename R, int MAXM>
__global__ __launch_bounds__(256) void k_mm_messages(MmParams p)
{
    const Quad q = quad_of(p);
    if (q.n == 0) return;
    const MmSlot sl = p.slots[blockIdx.y];
    R best[MAXM][4];
#pragma unroll
    for (int mq = 0; mq < MAXM; ++mq)
#pragma unroll
        for (int e = 0; e < 4; ++e) best[mq][e] = -RealLimits<R>::inf();
    for (int m = 0; m < sl.nmix; ++m) {
        R dv[4];
        ld4<R>(plane_at<R>(p.dt, q, 0, p.JG, sl.job_begin + m), q.n, dv);
#pragma unroll
        for (int mq = 0; mq < MAXM; ++mq) {
            if (mq < sl.npar) {
                const R b = (R)p.biasw[sl.bias_off[m] + mq];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const R wv = dv[e] + b;
                    int bi = 0;
                    if (sl.nmix == 1) best[mq][e] = wv;        // reduce_max: one type copies
                    else pick_max<R>(wv, m, best[mq][e], bi);
                }
            }
        }
    }
#pragma unroll
    for (int mq = 0; mq < MAXM; ++mq)
        if (mq < sl.npar) st4<R>(plane_at<R>(p.msg, q, 0, p.NS, sl.slot + mq), q.n, best[mq]);
}

// ---- context: block.y = one context plane (part, parent type) of the slice -----------------------------------------------------
template <typename R>
__global__ __launch_bounds__(256) void k_mm_context(MmParams p)
{
    const Quad q = quad_of(p);
    if (q.n == 0) return;
    const MmCtx cj = p.ctxs[blockIdx.y];
    R acc[4], v[4];
    ld4<R>(plane_at<R>(p.resp, q, (long long)p.frame * p.cell_per_frame, p.F, cj.filter), q.n, acc);
    for (int s = cj.sib_begin; s < cj.sib_end; ++s) {
        ld4<R>(plane_at<R>(p.msg, q, 0, p.NS, p.sibs[s]), q.n, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] + v[e];
    }
    ld4<R>(plane_at<R>(p.down, q, 0, p.NJ, cj.down), q.n, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = acc[e] + v[e];
    st4<R>(plane_at<R>(p.ctx, q, 0, p.NCTX, cj.out), q.n, acc);
}

// ---- down: block.y = one run (part, parent types [mq0, mq1)) of the slice; a root is a run without a parent --------------------
template <typename R, typename PT>
__global__ __launch_bounds__(256) void k_mm_down(MmParams p)
{
    const Quad q = quad_of(p);
    if (q.n == 0) return;
    const MmRun run = p.runs[blockIdx.y];
    const int cols = q.d.cols, rows = q.d.rows;
    int cx[4], cy[4];                                  // the cells' coordinates: one divide per thread
    cy[0] = q.local / cols; cx[0] = q.local - cy[0] * cols;
#pragma unroll
    for (int e = 1; e < 4; ++e) {
        const bool wrap = cx[e - 1] + 1 == cols;
        cx[e] = wrap ? 0 : cx[e - 1] + 1;
        cy[e] = wrap ? cy[e - 1] + 1 : cy[e - 1];
    }
    const PT *six = static_cast<const PT *>(p.sIx) + (size_t)q.d.cell_off * p.SJ;
    const PT *siy = static_cast<const PT *>(p.sIy) + (size_t)q.d.cell_off * p.SJ;
    for (int m = 0; m < run.nmix; ++m) {
        const int gm = run.gm0 + m;
        R best[4];
        int wjob[4], wk[4];                            // the winner's transform of this slice (-1: an earlier slice's stays) and type
#pragma unroll
        for (int e = 0; e < 4; ++e) { best[e] = -RealLimits<R>::inf(); wjob[e] = -1; wk[e] = 0; }
        if (run.npar == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) best[e] = (R)p.biasw[run.bias_off[0]];
        } else if (run.mq0 > 0) {
            ld4<R>(plane_at<R>(p.down, q, 0, p.NJ, gm), q.n, best);
        }
        for (int mq = run.mq0; mq < run.mq1; ++mq) {
            const int job = run.job0 + (mq - run.mq0) * run.nmix + m;
            const R b = (R)p.biasw[run.bias_off[m] + mq];
            R rv[4];
            ld4<R>(plane_at<R>(p.dt, q, 0, p.JG, job), q.n, rv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const R wv = rv[e] + b;
                // reduce_max over the parent's types: one type copies; else from -inf with pick_max, index 0 until a type wins
                const bool t = run.npar == 1 || wv > best[e];
                best[e] = t ? wv : best[e];
                if (t || mq == 0) { wjob[e] = job; wk[e] = mq; }
            }
        }
        int16_t jx[4], jy[4];
        int8_t jk[4];
        const bool resumed = run.npar > 0 && run.mq0 > 0;
        if (resumed) {
            ld4<int16_t>(plane_at<int16_t>(p.Jx, q, 0, p.NJ, gm), q.n, jx);
            ld4<int16_t>(plane_at<int16_t>(p.Jy, q, 0, p.NJ, gm), q.n, jy);
            ld4<int8_t>(plane_at<int8_t>(p.Jk, q, 0, p.NJ, gm), q.n, jk);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (run.npar == 0) { jx[e] = -1; jy[e] = -1; jk[e] = -1; continue; }
            if (e >= q.n || wjob[e] < 0) continue;
            // the parent's cell in arg-max order: the columns pass's pointer, then the rows pass's at that row (kept transposed)
            const size_t jo = (size_t)wjob[e] * q.HW;
            const int py = (int)siy[jo + (size_t)cy[e] * cols + cx[e]];
            const int px = (int)six[jo + (size_t)cx[e] * rows + py];
            jx[e] = (int16_t)px; jy[e] = (int16_t)py; jk[e] = (int8_t)wk[e];
        }
        st4<R>(plane_at<R>(p.down, q, 0, p.NJ, gm), q.n, best);
        st4<int16_t>(plane_at<int16_t>(p.Jx, q, 0, p.NJ, gm), q.n, jx);
        st4<int16_t>(plane_at<int16_t>(p.Jy, q, 0, p.NJ, gm), q.n, jy);
        st4<int8_t>(plane_at<int8_t>(p.Jk, q, 0, p.NJ, gm), q.n, jk);
        if (run.mq1 == run.npar) {
            R sv[4];
            if (run.s_from_acc) ld4<R>(plane_at<R>(p.acc, q, (long long)p.frame * p.cell_per_frame, p.NM, gm), q.n, sv);
            else ld4<R>(plane_at<R>(p.resp, q, (long long)p.frame * p.cell_per_frame, p.F, run.s_filter[m]), q.n, sv);
#pragma unroll
            for (int e = 0; e < 4; ++e) sv[e] = sv[e] + best[e];
            st4<R>(plane_at<R>(p.mm, q, 0, p.NJ, gm), q.n, sv);
        }
    }
}

// ---- decode: one thread per seed {level, component, part, type or -1, x, y} ---------------------------------------------------
constexpr int kMmDecodeThreads = 64;

template <typename R, typename PT>
__global__ __launch_bounds__(kMmDecodeThreads) void k_mm_decode(MmParams p)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.nseeds; i += gridDim.x * blockDim.x) {
        const int32_t *sd = p.seeds + 6 * (size_t)i;
        const int l = sd[0], c = sd[1], part = sd[2], x0 = sd[4], y0 = sd[5];
        int m = sd[3];
        bool ok = l >= 0 && l < p.nlevels && c >= 0 && c < p.NC;
        LevelDesc d{};
        int nparts = 0;
        if (ok) {
            d = p.lv[l];
            nparts = p.walk_off[c + 1] - p.walk_off[c];
            ok = part >= 0 && part < nparts && x0 >= 0 && x0 < d.cols && y0 >= 0 && y0 < d.rows;
        }
        if (ok) ok = m >= -1 && m < p.part_nmix[p.walk_off[c] + part];
        if (!ok) { p.status[i] = -1; continue; }
        const PartWalk *walk = p.walk + p.walk_off[c];
        const size_t HW = (size_t)(d.rows * d.cols);
        const size_t blk = (size_t)d.cell_off * p.NJ;
        const R *mm = static_cast<const R *>(p.mm) + blk;
        const size_t cell0 = (size_t)y0 * d.cols + x0;
        // type -1: the first type with the largest mm, type 0 where none wins (every mm NaN or -inf).  The score is the mm of the
        // type decoded, not the running maximum: where no type wins that maximum is still the -inf the search started from
        if (m < 0) reduce_max<R>(p.part_nmix[p.walk_off[c] + part], [&](int t) { return mm[(size_t)(walk[part].mix0 + t) * HW + cell0]; }, m);
        const R score = mm[(size_t)(walk[part].mix0 + m) * HW + cell0];
        int32_t *place = p.place + (size_t)i * p.max_parts * 3;
        for (int q = 0; q < nparts; ++q) place[3 * q + 2] = -1;
        // the climb: every part between the seed and the root takes the cell and type the marginal was taken at
        {
            int q = part, x = x0, y = y0, t = m;
            for (;;) {
                place[3 * q] = x; place[3 * q + 1] = y; place[3 * q + 2] = t;
                if (q == 0) break;
                const size_t o = blk + (size_t)(walk[q].mix0 + t) * HW + (size_t)y * d.cols + x;
                x = p.Jx[o]; y = p.Jy[o]; t = p.Jk[o];
                q = walk[q].parent;
            }
        }
        const LevelPlanes<MmParams> pl(p, d, p.frame);
        const R scale = (R)p.scales[l];
        int32_t *rec = p.cand + (size_t)i * p.stride;
        for (int q = 0; q < nparts; ++q) {
            const PartWalk w = walk[q];
            if (place[3 * q + 2] < 0) {
                const int32_t *par = place + 3 * w.parent;
                const WalkPos ch = walk_child<PT>(pl, w, par[0], par[1], par[2], true);
                place[3 * q] = ch.x; place[3 * q + 1] = ch.y; place[3 * q + 2] = ch.m;
            }
            const PartRect r = part_rect<R>(place[3 * q], place[3 * q + 1], w.ksize[place[3 * q + 2]], scale, d);
            rec[8 + 4 * q] = r.x1; rec[8 + 4 * q + 1] = r.y1; rec[8 + 4 * q + 2] = r.x2 - r.x1; rec[8 + 4 * q + 3] = r.y2 - r.y1;
        }
        rec[0] = p.frame + p.frame_offset; rec[1] = c; rec[2] = l;
        rec[3] = place[0]; rec[4] = place[1];
        rec[5] = __float_as_int((float)score);
        rec[6] = nparts;
        rec[7] = place[2];
        p.status[i] = nparts;
    }
}

template <class F> void for_real(bool f64, F &&f) { if (f64) f(double{}); else f(float{}); }
template <class F> void for_ptr(bool ptr8, F &&f) { if (ptr8) f(uint8_t{}); else f(int16_t{}); }
dim3 quad_grid(const MmParams &p, int ny) { return dim3((unsigned)((p.quad_per_frame + 255) / 256), (unsigned)ny); }

}  // namespace

void launch_mm_messages(const MmParams &p, int nslots, bool f64, hipStream_t s)
{
    if (nslots == 0 || p.quad_per_frame == 0) return;
    auto launch = [&](auto m) {
        constexpr int M = decltype(m)::value;
        for_real(f64, [&](auto r) { PBD_LAUNCH((k_mm_messages<decltype(r), M>), quad_grid(p, nslots), dim3(256), 0, s, p); });
    };
    if (p.max_mix <= 2) launch(std::integral_constant<int, 2>{});
    else if (p.max_mix <= 4) launch(std::integral_constant<int, 4>{});
    else if (p.max_mix <= 8) launch(std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 16>{});
}

void launch_mm_context(const MmParams &p, int nctx, bool f64, hipStream_t s)
{
    if (nctx == 0 || p.quad_per_frame == 0) return;
    for_real(f64, [&](auto r) { PBD_LAUNCH(k_mm_context<decltype(r)>, quad_grid(p, nctx), dim3(256), 0, s, p); });
}

void launch_mm_down(const MmParams &p, int nruns, bool f64, hipStream_t s)
{
    if (nruns == 0 || p.quad_per_frame == 0) return;
    for_real(f64, [&](auto r) { for_ptr(p.ptr8 != 0, [&](auto pt) {
        PBD_LAUNCH((k_mm_down<decltype(r), decltype(pt)>), quad_grid(p, nruns), dim3(256), 0, s, p);
    }); });
}

void launch_mm_decode(const MmParams &p, bool f64, hipStream_t s)
{
    if (p.nseeds <= 0) return;
    const int blocks = std::max(std::min((p.nseeds + kMmDecodeThreads - 1) / kMmDecodeThreads, 2048), 1);
    for_real(f64, [&](auto r) { for_ptr(p.ptr8 != 0, [&](auto pt) {
        PBD_LAUNCH((k_mm_decode<decltype(r), decltype(pt)>), dim3(blocks), dim3(kMmDecodeThreads), 0, s, p);
    }); });
}

}  // namespace pbd
