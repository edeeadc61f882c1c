// pbd_kernels_model.hip -- the in-place model update (pbd_set_model_vector*, pbd_qp_apply): every weight-dependent table that
// build_model and upload_filters_t build on the host at creation, rebuilt on the device from one model vector.
//
// Order on the stream: k_mu_check (is a referenced deformation's quadratic term zero once rounded to float32? -> *refused),
// k_mu_vector (the source, rounded as pbd_create rounds Model.from_vector(w), into the handle's device model vector), then
// the scatter kernels, which read that vector only.  Every kernel after the check returns at once when *refused is set.
// All of them are in gather form: a thread owns one destination element and computes where its value comes from (the layouts'
// one definition: pbd_layout.h), so stores are coalesced, nothing is accumulated across threads, and padding slots (filters
// past nf, the slack of wts3) are never written and stay zero.
#include "pbd_internal.h"

namespace pbd {

namespace {

constexpr int kB = 256;

// value k of the source in double (exact for float / double; the QP's expression is pbd_qp_weights')
template <int CODE> __device__ inline double mu_load(const MuSource &s, int k)
{
    if (CODE == kMuSrcF32) return (double)static_cast<const float *>(s.w)[k];
    if (CODE == kMuSrcF64) return static_cast<const double *>(s.w)[k];
    return static_cast<const double *>(s.w)[k] / s.wreg[k] + s.w0[k];
}

// one thread per (part, mixture): build_model's refusal.  Several threads may store the same 1.
template <int CODE> __global__ __launch_bounds__(kB) void k_mu_check(MuParams p, MuSource s)
{
    const int gm = blockIdx.x * kB + threadIdx.x;
    if (gm >= p.totmix) return;
    const int d = p.gm_def[gm];
    if (d < 0) return;
    const int o = p.nbias + 4 * d;
    if ((float)mu_load<CODE>(s, o) == 0.f || (float)mu_load<CODE>(s, o + 2) == 0.f) *p.refused = 1;
}

// one thread per value: bias and deformation values through float32 (pbd_model holds them so), filters to R
template <int CODE, typename R> __global__ __launch_bounds__(kB) void k_mu_vector(MuParams p, MuSource s)
{
    if (*p.refused) return;
    const int k = blockIdx.x * kB + threadIdx.x;
    if (k >= p.L) return;
    const double v = mu_load<CODE>(s, k);
    R *mvec = static_cast<R *>(p.mvec);
    if (k < p.nbias + 4 * p.ndefs) {
        const float f = (float)v;
        mvec[k] = (R)f;
        if (k < p.nbias) p.st_bias[k] = f; else p.st_def[k - p.nbias] = f;
    } else {
        mvec[k] = (R)v;
    }
}

// d_biasw, the root bias of every RootJob, the quadratics of every DtJob: one thread per element of the three lists
template <typename R> __global__ __launch_bounds__(kB) void k_mu_tables(MuParams p)
{
    if (*p.refused) return;
    const R *mvec = static_cast<const R *>(p.mvec);
    int k = blockIdx.x * kB + threadIdx.x;
    if (k < p.nbias) { p.biasw[k] = (float)mvec[k]; return; }
    k -= p.nbias;
    if (k < p.NC) { p.rjobs[k].bias = (float)mvec[p.root_bias[k]]; return; }
    k -= p.NC;
    if (k >= p.njobs) return;
    const MuJobRef ref = p.jobs[k];
    const R *w = mvec + p.nbias + 4 * ref.def;
    DtJob *j = ref.job;
    j->ax = (double)(-(float)w[0]); j->bx = (double)(-(float)w[1]); j->ay = (double)(-(float)w[2]); j->by = (double)(-(float)w[3]);
}

template <typename R> __device__ inline R mu_weight(const MuClassParams &p, const WeightSrc &s)
{
    const int f = p.fmap ? p.fmap[s.f] : s.f;
    return static_cast<const R *>(p.mvec)[p.foff[f] + weight_at(s)];
}

template <typename R> __global__ __launch_bounds__(kB) void k_mu_bank(MuClassParams p)
{
    if (*p.refused) return;
    const int KK = p.K * p.K;
    const long long i = (long long)blockIdx.x * kB + threadIdx.x;
    if (i >= generic_bank_size(KK, p.Fpad)) return;
    const WeightSrc s = p.group_layout ? group_bank_source(i, KK, p.nf) : generic_bank_source(i, KK, p.Fpad, p.nf);
    if (s.f >= 0) static_cast<R *>(p.wts)[i] = mu_weight<R>(p, s);
}

// grid y: the unit
template <typename R> __global__ __launch_bounds__(kB) void k_mu_units(MuClassParams p)
{
    if (*p.refused) return;
    const int u = blockIdx.y, KK = p.K * p.K, ql = p.unit_ql[u];
    const long long r = (long long)blockIdx.x * kB + threadIdx.x;
    if (r >= unit_size(KK, ql)) return;
    const WeightSrc s = unit_source(r, KK, p.unit_f0[u], ql, p.nf);
    if (s.f >= 0) p.wts3[p.unit_woff[u] + r] = (float)mu_weight<R>(p, s);
}

// one thread per (border case, filter): the out-of-image taps of channel 31 in raster order, zero weights skipped, from +0.0f
template <typename R> __global__ __launch_bounds__(kB) void k_mu_c31(MuClassParams p)
{
    if (*p.refused) return;
    const int k = blockIdx.x * kB + threadIdx.x;
    if (k >= 81 * p.nf) return;
    const int cs = k / p.nf, fl = k % p.nf;
    float sum = 0.0f;
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) {
            if (!c31_tap_outside(cs, i, j)) continue;
            const float w = (float)mu_weight<R>(p, WeightSrc{fl, i * 5 + j, 31});
            if (w != 0.0f) sum = sum + w;
        }
    p.c31tab[(size_t)cs * p.c31stride + fl] = sum;
}

template <typename R> __global__ __launch_bounds__(kB) void k_mu_frag64(MuClassParams p, int mtiles, int passes)
{
    if (*p.refused) return;
    const int KK = p.K * p.K;
    const long long o = (long long)blockIdx.x * kB + threadIdx.x;
    if (o >= f64_frag_size(KK, mtiles)) return;
    const WeightSrc s = f64_frag_source(o, KK, p.qn, mtiles, passes, p.nf);
    if (s.f >= 0) p.wfrag64[o] = (double)mu_weight<R>(p, s);
}

__global__ __launch_bounds__(kB) void k_mu_wrec(MuClassParams p)
{
    if (*p.refused) return;
    const int KK = p.K * p.K, NV = p.wrec_f16 ? 1 : 2;
    const long long i = (long long)blockIdx.x * kB + threadIdx.x;
    if (i >= wrec_size(KK, NV, p.nfilters)) return;
    int part = 0;
    const WeightSrc s = wrec_source(i, KK, NV, p.nfilters, &part);
    if (s.f >= 0) p.wrec[i] = wrec_value(mu_weight<float>(p, s), p.wrec_f16 != 0, part);
}

// the A-fragments of one size class of PBD_CONV_MFMA_ANY / PBD_CONV_MFMA_F16_ANY (pad slots stay zero)
__global__ __launch_bounds__(kB) void k_mu_wfrag16(MuClassParams p)
{
    if (*p.refused) return;
    const int KK = p.K * p.K, NV = p.wrec_f16 ? 1 : 2;
    const long long i = (long long)blockIdx.x * kB + threadIdx.x;
    if (i >= any_frag_size(KK, p.any_cb, NV, p.nf)) return;
    int part = 0;
    const WeightSrc s = any_frag_source(i, KK, p.any_cb, NV, p.nf, &part);
    if (s.f >= 0) p.wfrag16[i] = wrec_value(mu_weight<float>(p, s), p.wrec_f16 != 0, part);
}

inline dim3 blocks(long long n) { return dim3((unsigned)((n + kB - 1) / kB)); }

}  // namespace

void launch_mu_check(const MuParams &p, const MuSource &src, hipStream_t s)
{
    if (p.totmix <= 0) return;
    if (src.code == kMuSrcF32) PBD_LAUNCH(k_mu_check<kMuSrcF32>, blocks(p.totmix), dim3(kB), 0, s, p, src);
    else if (src.code == kMuSrcF64) PBD_LAUNCH(k_mu_check<kMuSrcF64>, blocks(p.totmix), dim3(kB), 0, s, p, src);
    else PBD_LAUNCH(k_mu_check<kMuSrcQp>, blocks(p.totmix), dim3(kB), 0, s, p, src);
}

template <typename R> static void launch_mu_vector_t(const MuParams &p, const MuSource &src, hipStream_t s)
{
    if (src.code == kMuSrcF32) PBD_LAUNCH((k_mu_vector<kMuSrcF32, R>), blocks(p.L), dim3(kB), 0, s, p, src);
    else if (src.code == kMuSrcF64) PBD_LAUNCH((k_mu_vector<kMuSrcF64, R>), blocks(p.L), dim3(kB), 0, s, p, src);
    else PBD_LAUNCH((k_mu_vector<kMuSrcQp, R>), blocks(p.L), dim3(kB), 0, s, p, src);
}

void launch_mu_vector(const MuParams &p, const MuSource &src, bool f64, hipStream_t s)
{
    if (p.L <= 0) return;
    if (f64) launch_mu_vector_t<double>(p, src, s); else launch_mu_vector_t<float>(p, src, s);
}

void launch_mu_tables(const MuParams &p, bool f64, hipStream_t s)
{
    const long long n = (long long)p.nbias + p.NC + p.njobs;
    if (n <= 0) return;
    if (f64) PBD_LAUNCH(k_mu_tables<double>, blocks(n), dim3(kB), 0, s, p);
    else PBD_LAUNCH(k_mu_tables<float>, blocks(n), dim3(kB), 0, s, p);
}

template <typename R> static void launch_mu_class_t(const MuClassParams &p, hipStream_t s)
{
    const int KK = p.K * p.K;
    if (p.nf <= 0) return;
    PBD_LAUNCH(k_mu_bank<R>, blocks(generic_bank_size(KK, p.Fpad)), dim3(kB), 0, s, p);
    if (p.wts3 && p.nunits > 0) {
        dim3 g = blocks(unit_size(KK, 8));
        g.y = (unsigned)p.nunits;
        PBD_LAUNCH(k_mu_units<R>, g, dim3(kB), 0, s, p);
    }
    if (p.c31tab) PBD_LAUNCH(k_mu_c31<R>, blocks(81LL * p.nf), dim3(kB), 0, s, p);
    if (p.wfrag64) {
        const int mtiles = (p.nf + 15) / 16, passes = mfma_passes(mtiles);
        PBD_LAUNCH(k_mu_frag64<R>, blocks(f64_frag_size(KK, mtiles)), dim3(kB), 0, s, p, mtiles, passes);
    }
}

void launch_mu_class(const MuClassParams &p, bool f64, hipStream_t s)
{
    if (f64) launch_mu_class_t<double>(p, s); else launch_mu_class_t<float>(p, s);
    if (p.wfrag16 && !f64 && p.nf > 0)
        PBD_LAUNCH(k_mu_wfrag16, blocks(any_frag_size(p.K * p.K, p.any_cb, p.wrec_f16 ? 1 : 2, p.nf)), dim3(kB), 0, s, p);
    else if (p.wrec && !f64 && p.nfilters > 0)
        PBD_LAUNCH(k_mu_wrec, blocks(wrec_size(p.K * p.K, p.wrec_f16 ? 1 : 2, p.nfilters)), dim3(kB), 0, s, p);
}

}  // namespace pbd
