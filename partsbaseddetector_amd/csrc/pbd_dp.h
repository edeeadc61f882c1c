// pbd_dp.h (private) -- the reference rules and buffer addresses the dynamic program's kernels share, one definition each:
// the level of a flat index, the planes of a level's block in every buffer, Math::reduceMax, the back-pointer composition of a
// walk, the value of a deformation's quadratic, a record's level in the resident result, a part's rectangle and a root's record
// header.  pbd_kernels_dp.hip (detection), pbd_kernels_examples.hip (the trainer) and pbd_kernels_partscores.hip (part scores)
// keep only what is their own; two consumers of a rule agree bit for bit because they run the same statement.
#pragma once

#include "pbd_internal.h"

#include <math.h>

namespace pbd {

template <typename R> struct RealLimits;
template <> struct RealLimits<float> { static __device__ __forceinline__ float inf() { return INFINITY; } };
template <> struct RealLimits<double> { static __device__ __forceinline__ double inf() { return (double)INFINITY; } };

// the level of [lo, hi) whose block holds flat index idx of a buffer with `scale` elements per unit of OFF (cells, or groups of
// four cells): the last level whose offset is <= idx (the offsets ascend; an empty level shares its successor's and is skipped)
template <long long LevelDesc::*OFF = &LevelDesc::cell_off>
__device__ __forceinline__ int level_of(const LevelDesc *lv, int lo, int hi, long long idx, long long scale = 1)
{
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (lv[mid].*OFF * scale <= idx) lo = mid; else hi = mid; }
    return lo;
}

// the plane a part's score is read from: R values (responses or accumulated scores) or, h != nullptr, fp16 responses
template <typename R> struct ScoreSrc {
    const R *v;
    const _Float16 *h;
    __device__ __forceinline__ R operator[](size_t i) const { return h ? (R)(float)h[i] : v[i]; }
};

// Level d's block in the buffers of P (DpParams, ArgminParams or ExampleParams; only the members a caller uses are looked up).
// Every buffer is [frame][cell_per_frame * planes] and a level's block [plane][y][x] from its cell offset on.  `frame` indexes
// the batch's buffers, `fl` the chunk's scratch (tmp, dt)
template <class P> struct LevelPlanes {
    const P &p;
    const LevelDesc &d;
    size_t cell, lcell;           // first cell of the block in a batch buffer / in the chunk's scratch
    size_t HW;                    // cells of a plane (an int product: a level has fewer than 2^31 cells, as its int cell indices say)
    __device__ __forceinline__ LevelPlanes(const P &p_, const LevelDesc &d_, int frame, int fl = 0)
        : p(p_), d(d_), cell((size_t)frame * p_.cell_per_frame + d_.cell_off), lcell((size_t)fl * p_.cell_per_frame + d_.cell_off),
          HW((size_t)(d_.rows * d_.cols)) {}
    // element i of the block in each buffer (the offset is summed first: the buffer's base stays a uniform value)
    template <typename T> __device__ __forceinline__ T *resp(size_t i = 0) const { return static_cast<T *>(p.resp) + (cell * p.F + i); }
    template <typename R> __device__ __forceinline__ auto acc(size_t i = 0) const { return static_cast<R *>(p.acc) + (cell * p.NM + i); }
    __device__ __forceinline__ auto Ik(size_t i = 0) const { return p.Ik + (cell * p.NS + i); }
    template <typename PT> __device__ __forceinline__ auto ix(size_t i = 0) const { return cast<PT>(p.IxRaw) + (cell * p.NJ + i); }   // [gm][x][y]
    template <typename PT> __device__ __forceinline__ auto iy(size_t i = 0) const { return cast<PT>(p.IyRaw) + (cell * p.NJ + i); }   // [gm][y][x]
    template <typename R> __device__ __forceinline__ auto rootv(size_t i = 0) const { return cast<R>(p.rootv) + (cell * p.NC + i); }
    __device__ __forceinline__ auto rooti(size_t i = 0) const { return p.rooti + (cell * p.NC + i); }
    template <typename R> __device__ __forceinline__ R *tmp(size_t i = 0) const { return static_cast<R *>(p.tmp) + (lcell * p.JG + i); }
    template <typename R> __device__ __forceinline__ R *dt(size_t i = 0) const { return static_cast<R *>(p.dt) + (lcell * p.JG + i); }
    // element `local` of a part's score plane: the accumulator of a part with children, else its filter's response (rh: fp16)
    template <typename R> __device__ __forceinline__ ScoreSrc<R> score(bool from_acc, bool rh, int plane, size_t local) const
    {
        const size_t o = (size_t)plane * HW;
        if (from_acc) return {acc<R>(local) + o, nullptr};
        if (rh) return {nullptr, resp<const _Float16>(local) + o};
        return {resp<const R>(local) + o, nullptr};
    }

private:
    template <typename T> static __device__ __forceinline__ T *cast(void *q) { return static_cast<T *>(q); }
    template <typename T> static __device__ __forceinline__ const T *cast(const void *q) { return static_cast<const T *>(q); }
};

// ---- Math::reduceMax / reducePickIndex (include/Math.hpp:95-185) --------------------------------------------------------------
// one candidate: strict >, so the first of equal scores wins
template <typename R> __device__ __forceinline__ void pick_max(R wv, int mm, R &best, int &bi)
{
    const bool t = wv > best;
    best = t ? wv : best;
    bi = t ? mm : bi;
}
// the maximum of score(0 .. n - 1) and its index; the search starts at -inf, and K == 1 copies (a NaN or -inf stays what it is).
// k_dp_combine keeps its own unrolled loop over registers around pick_max (mixtures a child lacks are padded with -inf there)
template <typename R, class Score> __device__ __forceinline__ R reduce_max(int n, Score score, int &bi)
{
    bi = 0;
    if (n == 1) return score(0);
    R best = -RealLimits<R>::inf();
    for (int mm = 0; mm < n; ++mm) pick_max<R>(score(mm), mm, best, bi);
    return best;
}

// ---- Quadratic::operator()(x, y) (include/DistanceTransform.hpp:102-104) -------------------------------------------------------
// a x^2 + b x + y: the int square, double arithmetic left to right, one rounding to T.  The transform's passes write it for every
// cell; the part scores (pbd_kernels_partscores.hip) evaluate it at a placement's displacement.
// BZ: the linear coefficient b is exactly -0.0 and a != 0 (see quad_isect of pbd_kernels_dp.hip: the value is the same)
template <typename R, bool BZ>
__device__ __forceinline__ R quad_val(double a, double b, int x, R y)
{
    if (BZ) return (R)(a * (double)__mul24(x, x) + (double)y);
    return (R)((a * (double)__mul24(x, x) + b * (double)x) + (double)y);     // |x| < 2^16
}

// ---- a record's (frame, level) in the resident result ---------------------------------------------------------------------------
// (frame of the buffers, level of the plan) of a record's frame f (its frame field less the call's frame_offset) and level l, or
// {-1, -1} outside the result.  Mixed plans (frame_lv0 != NULL: [nframes + 1] first virtual level of each frame): frame 0, the
// virtual level.  The host states the same in resident_level (pbd_handle.h)
struct RecordLevel { int bf, vl; };
__device__ __forceinline__ RecordLevel record_level(long long f, int l, int nframes, int nlevels, const int *frame_lv0)
{
    if (f >= 0 && f < nframes && l >= 0) {
        if (frame_lv0) {
            if (l < frame_lv0[f + 1] - frame_lv0[f]) return {0, frame_lv0[f] + l};
        } else if (l < nlevels) {
            return {(int)f, l};
        }
    }
    return {-1, -1};
}

// ---- back-tracking (src/DynamicProgram.cpp:218-244) ---------------------------------------------------------------------------
// a child's position and mixture from its parent's: m = Ik[slot + pm][py][px], x = IxRaw[k][py][px], y = IyRaw[k][py][x] with k
// the plane of the winning mixture m -- the reference's composition Iy[y][x] = IyRaw[y][Ix[y][x]]
// (include/DistanceTransform.hpp:233-244), made here for the walked cells only.
// argmax (PBD_WALK_ARGMAX, pbd_set_walk): the placement the score was taken at.  The column pass ran over the row pass's output,
// so its pointer comes first: y = IyRaw[k][py][px], then x = IxRaw[k][y][px] -- the same two loads in the other order.
struct WalkPos { int x, y, m; };
template <typename PT, class P>
__device__ __forceinline__ WalkPos walk_child(const LevelPlanes<P> &pl, const PartWalk &w, int px, int py, int pm, bool argmax = false)
{
    const LevelDesc &d = pl.d;
    const int m = *pl.Ik((size_t)(w.slot + pm) * pl.HW + (size_t)py * d.cols + px);
    const size_t jo = (size_t)(w.mix0 + m) * pl.HW;
    if (argmax) {
        const int y = *pl.template iy<PT>(jo + (size_t)py * d.cols + px);
        const int x = *pl.template ix<PT>(jo + (size_t)px * d.rows + y);
        return {x, y, m};
    }
    const int x = *pl.template ix<PT>(jo + (size_t)px * d.rows + py);      // IxRaw is kept transposed ([x][y])
    const int y = *pl.template iy<PT>(jo + (size_t)py * d.cols + x);
    return {x, y, m};
}

template <typename R> __device__ __forceinline__ int round_mul(int a, R s);
// cv::Point_<int> * T -> saturate_cast<int>(a*s) = cvRound: round half to even
template <> __device__ __forceinline__ int round_mul<float>(int a, float s) { return __float2int_rn((float)a * s); }
template <> __device__ __forceinline__ int round_mul<double>(int a, double s) { return __double2int_rn((double)a * s); }

// a part's rectangle in the frame (src/DynamicProgram.cpp:238-241): Rect(Point(x - 1, y - 1) * scale, that + Point(ks, ks) *
// scale - Point(1, 1)) -- cv::Rect from two points orders them; (x1, y1) .. (x2, y2) are its corners, w = x2 - x1, h = y2 - y1
// (x, y) is a cell of the level's planes; a padded level (LevelDesc::padx / pady, pbd_set_padding) starts padx / pady cells left of
// and above the image, which the rectangle takes off again (detect.m:266-270)
struct PartRect { int x1, y1, x2, y2; };
template <typename R> __device__ __forceinline__ PartRect part_rect(int x, int y, int ks, R scale, const LevelDesc &d)
{
    const int x1 = round_mul<R>(x - d.padx - 1, scale), y1 = round_mul<R>(y - d.pady - 1, scale);
    const int x2 = x1 + round_mul<R>(ks, scale) - 1, y2 = y1 + round_mul<R>(ks, scale) - 1;
    return {min(x1, x2), min(y1, y2), max(x1, x2), max(y1, y2)};
}

// the root cell at index `rem` of a frame's rootv block ([level][component][y][x]; levels [l0, l1))
struct RootCell { int level, comp, x, y; };
__device__ __forceinline__ RootCell root_cell(const LevelDesc *lv, int l0, int l1, int NC, long long rem)
{
    const int l = level_of(lv, l0, l1, rem, NC);
    const LevelDesc d = lv[l];
    const int HW = d.rows * d.cols;
    const int rem2 = (int)(rem - d.cell_off * NC);
    const int comp = rem2 / HW, local = rem2 - comp * HW;
    return {l, comp, local % d.cols, local / d.cols};
}

// the header of a root's record from its index `rem` into the frame's rootv block: frame, component, level, x, y, the score as
// float (Candidate::confidence_ is float for every T, include/Candidate.hpp:72), no parts yet, and the root's mixture for the walk
template <typename R>
__device__ __forceinline__ void root_record(int32_t *rec, const LevelDesc *lv, int l0, int l1, int NC, int frame, long long rem, R score,
                                            int mixture)
{
    const RootCell rc = root_cell(lv, l0, l1, NC, rem);
    rec[0] = frame; rec[1] = rc.comp; rec[2] = rc.level;
    rec[3] = rc.x; rec[4] = rc.y;
    rec[5] = __float_as_int((float)score);
    rec[6] = 0;
    rec[7] = mixture;
}

}  // namespace pbd
