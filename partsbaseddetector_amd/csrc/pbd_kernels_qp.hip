// pbd_kernels_qp.hip -- the training QP (pbd_qp_*): the cache writes, scores, the coordinate pass and the refresh of the
// reference's Matlab training code (matlab/learning/qp_*.m, oct/qp_one_sparse.cc, oct/lincomb.cc).  include/pbd.h states the
// contract and every summation order, DESIGN.md section 6i the cost.
//
//   k_qp_slots    one workgroup: which examples of a call are valid, and the entry each one goes to (a prefix count)
//   k_qp_write    one workgroup per example: block merge, x' = float(C x / wreg), b, d, the entry's header and block map
//   k_qp_score    one workgroup per entry: R(w . x) - b (computeloss) or R(w . x) / Cpos (qp_scorepos)
//   k_qp_pass     ONE persistent workgroup: the sequential coordinate pass of qp_one_sparse; w stays in global memory (L2)
//   k_qp_lincomb  one workgroup per (layout block, 1024 coordinates): refresh's w, each coordinate summed over its entries in
//                 ascending a; then k_qp_norm (one workgroup): the non-negativity clamps and R(w . w)
//   k_qp_gather   one workgroup per kept entry: prune's compaction into scratch (copied back by the host in order)
//   k_qp_hinge    one workgroup: Cl * R(max(0, 1 - y * score)) over a payload's records (the mining bound, detect.m:135)
//
// R(.) (include/pbd.h): lane l of the 1024 adds the products of values l, l + 1024, ... from +0.0, then a halving tree per
// 64 lanes (one wavefront: __shfl_down), then a halving tree over the 16 wavefront sums.  Products are multiplies then adds:
// the library is compiled with -ffp-contract=off.
#include "pbd_device.h"

namespace pbd {
namespace {

constexpr int kLanes = kRLanes;      // reduce1 / reduce2: pbd_device.h
constexpr int kWaves = kRWaves;

__device__ __forceinline__ double dmin(double a, double b) { return a > b ? b : a; }   // MIN / MAX of qp_one_sparse.cc
__device__ __forceinline__ double dmax(double a, double b) { return a < b ? b : a; }

// an entry's header into LDS (3 words per block); the caller synchronises
__device__ __forceinline__ int load_hdr(const QpCache &c, int i, int *tab, int *nv)
{
    const int32_t *h = c.hd + (size_t)i * c.HW;
    const int nb = min(max(h[0], 0), c.MB);
    for (int k = threadIdx.x; k < 3 * nb; k += kLanes) tab[k] = h[2 + k];
    *nv = min(max(h[1], 0), c.V);
    return nb;
}

// this thread's lane-strided partial of w . x over entry i's values (tab: its header in LDS)
__device__ __forceinline__ double dot_w(const QpCache &c, const double *w, int i, int nv, const int *tab)
{
    const float *x = c.x + (size_t)i * c.V;
    const uint8_t *bm = c.bm + (size_t)i * c.V;
    double acc = 0.0;
#pragma unroll 4
    for (int j = threadIdx.x; j < nv; j += kLanes) {
        const int b = bm[j];
        const int k = tab[3 * b] + j - tab[3 * b + 2];
        acc = acc + w[k] * (double)x[j];
    }
    return acc;
}

// w += da * x over entry i's values
__device__ __forceinline__ void axpy(const QpCache &c, double da, int i, int nv, const int *tab)
{
    const float *x = c.x + (size_t)i * c.V;
    const uint8_t *bm = c.bm + (size_t)i * c.V;
#pragma unroll 4
    for (int j = threadIdx.x; j < nv; j += kLanes) {
        const int b = bm[j];
        const int k = tab[3 * b] + j - tab[3 * b + 2];
        c.w[k] = c.w[k] + da * (double)x[j];
    }
}

__device__ __forceinline__ void clamp_noneg(const QpCache &c)
{
    for (int k = threadIdx.x; k < c.nnoneg; k += kLanes) {
        const int q = c.noneg[k];
        const double v = c.w[q];
        c.w[q] = v < 0.0 ? 0.0 : v;
    }
}

// ---- writes ----------------------------------------------------------------------------------------------------------------
// example e of the call: is it valid (header not marked invalid, every block a layout block, values within the strides)?
__device__ bool example_valid(const QpWriteParams &p, int e)
{
    const int32_t *h = p.in_hdr + (size_t)e * p.in_hw;
    const int nb = h[2], nv = h[3];
    if (nb < 0 || nb > (p.in_hw - 4) / 2 || nb > p.c.MB || nv < 0 || nv > p.in_vs || nv > p.c.V) return false;
    long long tot = 0;
    for (int b = 0; b < nb; ++b) {
        const int off = h[4 + 2 * b], len = h[5 + 2 * b];
        if (off < 0 || off >= p.c.L) return false;
        const int s = p.c.slot_of[off];
        if (s < 0 || p.c.slot_len[s] != len) return false;
        tot += len;
    }
    return tot == nv;
}

__global__ __launch_bounds__(kLanes) void k_qp_slots(QpWriteParams p)
{
    __shared__ int wsum[kWaves + 1];
    const int m = p.payload ? payload_count(p.payload, p.m) : p.m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int e0 = 0; e0 < p.m; e0 += kLanes) {
        const int e = e0 + threadIdx.x;
        const int v = (e < m && example_valid(p, e)) ? 1 : 0;
        const int incl = wave_incl_scan(v);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = base;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        int total = base;
        for (int w = 0; w < kWaves; ++w) total += wsum[w];
        if (e < p.m) {
            const long long at = (long long)p.n0 + before + incl - v;
            p.slot[e] = (v && at < p.c.cap) ? (int)at : -1;
        }
        __syncthreads();
        base = total;
    }
    if (threadIdx.x == 0) {
        const int taken = min(base, max(p.c.cap - p.n0, 0));
        p.taken[0] = taken;
        if (p.taken_user) p.taken_user[0] = taken;
    }
}

template <typename T>
__global__ __launch_bounds__(kLanes) void k_qp_write(QpWriteParams p)
{
    __shared__ int ioff[256], ilen[256], ist[256], nxt[256], oidx[256], ost[256];
    __shared__ int sh_nb, sh_nv;
    __shared__ double red[2 * kWaves + 2];
    const int e = blockIdx.x;
    if (e >= p.m) return;
    const int s = p.slot[e];
    if (s < 0 || s >= p.c.cap) return;   // uniform over the workgroup
    const QpCache &c = p.c;
    const int32_t *h = p.in_hdr + (size_t)e * p.in_hw;
    const int nb = h[2];                  // k_qp_slots checked it against MB (<= 256) and the layout
    const int t = threadIdx.x;
    if (t < nb) { ioff[t] = h[4 + 2 * t]; ilen[t] = h[5 + 2 * t]; }
    __syncthreads();
    if (t < nb) {
        int st = 0, lead = 1;
        for (int b = 0; b < t; ++b) { st += ilen[b]; if (ioff[b] == ioff[t]) lead = 0; }
        ist[t] = st;
        int nx = -1;
        for (int b = nb - 1; b > t; --b) if (ioff[b] == ioff[t]) nx = b;
        nxt[t] = nx;
        oidx[t] = lead ? 0 : -1;
    }
    __syncthreads();
    if (t == 0) {   // output index and first value of every leading block, in block order
        int k = 0, pos = 0;
        for (int b = 0; b < nb; ++b)
            if (oidx[b] >= 0) { oidx[b] = k++; ost[b] = pos; pos += ilen[b]; }
        sh_nb = k; sh_nv = pos;
    }
    __syncthreads();
    const int nbo = sh_nb, nvo = sh_nv;
    int32_t *hd = c.hd + (size_t)s * c.HW;
    for (int k = t; k < c.HW; k += kLanes) hd[k] = k == 0 ? nbo : k == 1 ? nvo : 0;
    __syncthreads();   // the zero fill above precedes the block words below (same workgroup)
    if (t < nb && oidx[t] >= 0) {
        hd[2 + 3 * oidx[t]] = ioff[t];
        hd[3 + 3 * oidx[t]] = ilen[t];
        hd[4 + 3 * oidx[t]] = ost[t];
    }
    const int32_t *ids = p.in_ids ? p.in_ids + (size_t)e * 5 : nullptr;
    int id0;
    if (ids) id0 = ids[0];
    else id0 = p.label;
    const bool label = id0 > 0;
    const double Cl = label ? p.Cpos : p.Cneg;
    const T *in = static_cast<const T *>(p.in_values) + (size_t)e * p.in_vs;
    float *x = c.x + (size_t)s * c.V;
    uint8_t *bm = c.bm + (size_t)s * c.V;
    double pw0 = 0.0, pd = 0.0;
    for (int b = 0; b < nb; ++b) {
        if (oidx[b] < 0) continue;   // uniform
        const int len = ilen[b], o0 = ost[b], off = ioff[b];
        int j = o0 + ((t - o0 % kLanes) + kLanes) % kLanes;   // this lane's first value of the block
        for (; j < o0 + len; j += kLanes) {
            const int k = j - o0;
            double v = (double)in[ist[b] + k];
            for (int q = nxt[b]; q >= 0; q = nxt[q]) v = v + (double)in[ist[q] + k];
            if (!label) v = -v;
            const double xp = (double)(float)((Cl * v) / c.wreg[off + k]);
            pw0 = pw0 + c.w0[off + k] * v;
            pd = pd + xp * xp;
            x[j] = (float)xp;
            bm[j] = (uint8_t)oidx[b];
        }
    }
    for (int j = nvo + t; j < c.V; j += kLanes) { x[j] = 0.f; bm[j] = 0; }
    double sw0, sd;
    reduce2(pw0, pd, red, &sw0, &sd);
    if (t == 0) {
        c.b[s] = Cl * (1.0 - sw0);
        c.d[s] = sd;
        c.a[s] = 0.0;
        c.sv[s] = 1;
        int32_t *o = c.ids + (size_t)s * 5;
        if (ids) {
            for (int k = 0; k < 5; ++k) o[k] = ids[k];
        } else {   // detect.m's ex.id of the payload's record e
            const int32_t *r = p.payload + 1 + (size_t)e * p.rec_stride;
            o[0] = p.label; o[1] = p.id_base + r[0]; o[2] = r[2]; o[3] = r[3]; o[4] = r[4];
        }
    }
}

// ---- scores ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLanes) void k_qp_score(QpScoreParams p)
{
    __shared__ int tab[3 * 256];
    __shared__ double red[kWaves + 1];
    const int k = blockIdx.x;
    if (k >= p.count) return;
    const int i = p.list ? p.list[k] : p.first + k;
    if (i < 0 || i >= p.c.cap) return;
    int nv;
    load_hdr(p.c, i, tab, &nv);
    __syncthreads();
    const double wx = reduce1(dot_w(p.c, p.w, i, nv, tab), red);
    if (threadIdx.x == 0) p.out[k] = p.sub_b ? wx - p.c.b[i] : wx / p.scale;
}

__global__ __launch_bounds__(256) void k_qp_wraw(QpCache c, double *out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < c.L) out[k] = c.w[k] + c.w0[k] * c.wreg[k];
}

// ---- the coordinate pass ---------------------------------------------------------------------------------------------------
// Every thread evaluates the branch of qp_one_sparse.cc on identical values; thread 0 stores the scalars.  The scalars a step
// reads are loaded before its first barrier, and thread 0 stores after it, so no thread reads a value of the same step.
__global__ __launch_bounds__(kLanes) void k_qp_pass(QpPassParams p)
{
    __shared__ int tab1[3 * 256], tab2[3 * 256], part[256];
    __shared__ double red[2 * kWaves + 2];
    const QpCache &c = p.c;
    const int t = threadIdx.x;
    for (int step = 0; step < p.nsteps; ++step) {
        const int i = p.order[step], j = p.gidx[step];
        double Ai = c.a[i];
        const double idCj = p.idC[j], bi = c.b[i], di = c.d[i], errj = p.err[j];
        const int i2 = p.idI[j];
        double A2 = 0.0, b2 = 0.0, d2 = 0.0;
        if (i2 >= 0) { A2 = c.a[i2]; b2 = c.b[i2]; d2 = c.d[i2]; }
        int nv1;
        const int nb1 = load_hdr(c, i, tab1, &nv1);
        __syncthreads();
        const double wx = reduce1(dot_w(c, c.w, i, nv1, tab1), red);

        Ai = dmax(dmin(Ai, 1.0), 0.0);
        const double Ci = dmax(dmin(idCj, 1.0), Ai);
        double G = wx - bi;
        double PG = G;
        if ((Ai == 0.0 && G >= 0.0) || (Ci >= 1.0 && G <= 0.0)) PG = 0.0;
        const double err_new = -G > errj ? -G : errj;
        int sv_clear = (Ai == 0.0 && G > 0.0) ? 1 : 0;
        double Ci_new = idCj;
        bool upd_plain = false, upd_pair = false;
        double dA = 0.0, Ai_new = Ai, A2_new = A2;
        int nv2 = 0;
        if (Ci >= 1.0 && G < -1e-12 && Ai < 1.0 && i2 != i && i2 >= 0) {
            const int nb2 = load_hdr(c, i2, tab2, &nv2);
            __syncthreads();
            if (t < nb1) {   // the block of x2 at the same offset (entries hold one block per offset)
                int q = -1;
                for (int b = 0; b < nb2; ++b) if (tab2[3 * b] == tab1[3 * t]) { q = b; break; }
                part[t] = q;
            }
            __syncthreads();
            double pxx = 0.0;
            {
                const float *x1 = c.x + (size_t)i * c.V, *x2 = c.x + (size_t)i2 * c.V;
                const uint8_t *bm1 = c.bm + (size_t)i * c.V;
                for (int v = t; v < nv1; v += kLanes) {
                    const int b = bm1[v], q = part[b];
                    if (q >= 0) pxx = pxx + (double)x1[v] * (double)x2[tab2[3 * q + 2] + v - tab1[3 * b + 2]];
                    else pxx = pxx + 0.0;
                }
            }
            double wx2, xx2;
            reduce2(dot_w(c, c.w, i2, nv2, tab2), pxx, red, &wx2, &xx2);
            G = G - (wx2 - b2);
            if (Ai == 0.0 && G > 0.0) { G = 0.0; sv_clear = 1; }
            if (G > 1e-12 || G < -1e-12) {
                dA = -G / (di + d2 - 2.0 * xx2);
                if (dA > 0.0) dA = dmin(dmin(dA, 1.0 - Ai), A2);
                else dA = dmax(dmax(dA, -Ai), A2 - 1.0);
                Ai_new = Ai + dA;
                A2_new = A2 - dA;
                upd_pair = true;
            }
        } else if (PG > 1e-12 || PG < -1e-12) {
            const double maxA = 1.0 - (Ci - Ai);
            Ai_new = dmin(dmax(Ai - G / di, 0.0), maxA);
            dA = Ai_new - Ai;
            Ci_new = dmin(dmax(Ci + dA, 0.0), 1.0);
            upd_plain = true;
        }
        if (t == 0) {
            c.a[i] = Ai_new;
            if (upd_pair) c.a[i2] = A2_new;
            if (sv_clear) c.sv[i] = 0;
            if (upd_plain) p.idC[j] = Ci_new;
            p.err[j] = err_new;
            if (Ai_new > 0.0) p.idI[j] = i;
        }
        if (upd_plain || upd_pair) {
            axpy(c, dA, i, nv1, tab1);
            if (upd_pair) {
                __syncthreads();
                axpy(c, -dA, i2, nv2, tab2);
            }
            __syncthreads();
            clamp_noneg(c);
        }
        __syncthreads();
    }
    if (t == 0) {
        double s = 0.0;
        for (int g = 0; g < p.ngroups; ++g) s = s + p.err[g];
        p.loss[0] = s;
    }
}

// ---- refresh ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLanes) void k_qp_lincomb(QpLincombParams p)
{
    const QpTask tk = p.tasks[blockIdx.x];
    const int k = threadIdx.x;
    if (k >= tk.n) return;
    const int coord = tk.c0 + k;
    double acc = 0.0;
#pragma unroll 4
    for (int e = tk.begin; e < tk.end; ++e) {
        const int2 en = p.ent[e];
        acc = acc + p.c.a[en.x] * (double)p.c.x[(size_t)en.x * p.c.V + en.y + coord];
    }
    p.c.w[tk.off + coord] = acc;
}

__global__ __launch_bounds__(kLanes) void k_qp_norm(QpLincombParams p)
{
    __shared__ double red[kWaves + 1];
    clamp_noneg(p.c);
    __syncthreads();
    double acc = 0.0;
    for (int k = threadIdx.x; k < p.c.L; k += kLanes) acc = acc + p.c.w[k] * p.c.w[k];
    const double s = reduce1(acc, red);
    if (threadIdx.x == 0) p.ww[0] = s;
}

// ---- prune -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_qp_gather(QpGatherParams p)
{
    const int k = blockIdx.x;
    if (k >= p.count) return;
    const int i = p.src[k];
    if (i < 0 || i >= p.c.cap) return;
    const QpCache &c = p.c;
    const float4 *xs = reinterpret_cast<const float4 *>(c.x + (size_t)i * c.V);   // V is a multiple of 4
    float4 *xd = reinterpret_cast<float4 *>(p.x + (size_t)k * c.V);
    for (int j = threadIdx.x; j < c.V / 4; j += 256) xd[j] = xs[j];
    for (int j = threadIdx.x; j < c.V; j += 256) p.bm[(size_t)k * c.V + j] = c.bm[(size_t)i * c.V + j];
    for (int j = threadIdx.x; j < c.HW; j += 256) p.hd[(size_t)k * c.HW + j] = c.hd[(size_t)i * c.HW + j];
    if (threadIdx.x < 5) p.ids[(size_t)k * 5 + threadIdx.x] = c.ids[(size_t)i * 5 + threadIdx.x];
    if (threadIdx.x == 0) { p.b[k] = c.b[i]; p.d[k] = c.d[i]; p.a[k] = c.a[i]; }
}

// ---- the mining bound ------------------------------------------------------------------------------------------------------
// one workgroup: record j of the payload on lane j mod 1024, each lane adding its hinges in ascending j from +0.0, then R's trees
__global__ __launch_bounds__(kLanes) void k_qp_hinge(QpHingeParams p)
{
    __shared__ double red[kWaves + 1];
    const int m = payload_count(p.payload, p.capacity);
    double acc = 0.0;
    for (int j = threadIdx.x; j < m; j += kLanes) {
        const double score = (double)__int_as_float(p.payload[1 + (size_t)j * p.rec_stride + 5]);
        const double h = 1.0 - p.y * score;
        acc = acc + (h > 0.0 ? h : 0.0);
    }
    const double s = reduce1(acc, red);
    if (threadIdx.x == 0) p.out[0] = p.Cl * s;
}

}  // namespace

void launch_qp_hinge(const QpHingeParams &p, hipStream_t s) { PBD_LAUNCH(k_qp_hinge, dim3(1), dim3(kLanes), 0, s, p); }

void launch_qp_write(const QpWriteParams &p, bool f64, hipStream_t s)
{
    PBD_LAUNCH(k_qp_slots, dim3(1), dim3(kLanes), 0, s, p);
    if (p.m <= 0) return;
    if (f64) PBD_LAUNCH(k_qp_write<double>, dim3(p.m), dim3(kLanes), 0, s, p);
    else PBD_LAUNCH(k_qp_write<float>, dim3(p.m), dim3(kLanes), 0, s, p);
}

void launch_qp_pass(const QpPassParams &p, hipStream_t s) { PBD_LAUNCH(k_qp_pass, dim3(1), dim3(kLanes), 0, s, p); }

void launch_qp_score(const QpScoreParams &p, hipStream_t s)
{
    if (p.count > 0) PBD_LAUNCH(k_qp_score, dim3(p.count), dim3(kLanes), 0, s, p);
}

void launch_qp_lincomb(const QpLincombParams &p, hipStream_t s)
{
    (void)hipMemsetAsync(p.c.w, 0, (size_t)p.c.L * sizeof(double), s);
    if (p.ntasks > 0) PBD_LAUNCH(k_qp_lincomb, dim3(p.ntasks), dim3(kLanes), 0, s, p);
    launch_qp_norm(p, s);
}

void launch_qp_norm(const QpLincombParams &p, hipStream_t s) { PBD_LAUNCH(k_qp_norm, dim3(1), dim3(kLanes), 0, s, p); }

void launch_qp_wraw(const QpCache &c, double *out, hipStream_t s)
{
    PBD_LAUNCH(k_qp_wraw, dim3((c.L + 255) / 256), dim3(256), 0, s, c, out);
}

void launch_qp_gather(const QpGatherParams &p, hipStream_t s)
{
    if (p.count > 0) PBD_LAUNCH(k_qp_gather, dim3(p.count), dim3(256), 0, s, p);
}

}  // namespace pbd
