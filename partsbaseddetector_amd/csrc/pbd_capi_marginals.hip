// pbd_capi_marginals.hip -- the C entry points of the max-marginals (include/pbd.h): pbd_max_marginals,
// pbd_get_marginals, pbd_marginals_device, pbd_marginal_poses*.  The kernels: pbd_kernels_marginals.hip and the detect path's
// distance-transform launches.  The handle and the layer the entry points are written on: pbd_handle.h.
#include "pbd_handle.h"

using namespace pbd;

namespace {

// The job tables of one call, derived from the handle's CURRENT tables (an in-place model update rewrites the groups' quadratics,
// mu_finish): every upward group's message jobs, then for every tree depth from the root's children down the slices of mirrored
// transforms with their context planes and reduction runs.  A slice holds at most JGmax transforms, the dynamic program's own
// scratch (values, envelope stacks); it is cut between (part, parent type) units, so a part with more transforms than a slice
// holds continues in the next one (MmRun::mq0 > 0).
struct MmSlice { int job0, njobs, ctx0, nctx, run0, nruns, bz_x, bz_y; };
struct MmTables {
    std::vector<DtJob> jobs;
    std::vector<MmSlot> slots;
    std::vector<int> group_slot0;     // [groups + 1]
    std::vector<MmCtx> ctxs;
    std::vector<int> sibs;
    std::vector<MmRun> runs;          // the roots' runs first ([0, NC)), then the slices'
    std::vector<MmSlice> slices;      // in launch order: depth 1 first
};

void close_slice(MmTables &t, MmSlice &cur)
{
    if (cur.njobs == 0) return;
    auto neg_zero = [](double v) { return v == 0.0 && std::signbit(v); };   // set_variant_flags' test, on the mirrored jobs
    cur.bz_x = cur.bz_y = 1;
    for (int j = cur.job0; j < cur.job0 + cur.njobs; ++j) {
        if (!(neg_zero(t.jobs[j].bx) && t.jobs[j].ax != 0.0)) cur.bz_x = 0;
        if (!(neg_zero(t.jobs[j].by) && t.jobs[j].ay != 0.0)) cur.bz_y = 0;
    }
    t.slices.push_back(cur);
    cur = MmSlice{(int)t.jobs.size(), 0, (int)t.ctxs.size(), 0, (int)t.runs.size(), 0, 0, 0};
}

void build_tables(const pbd_handle *h, MmTables &t)
{
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c], g0 = h->mix_offset[p0];
        const RootJob &rj = h->rjobs[c];
        MmRun r{};
        r.nmix = rj.nmix; r.gm0 = g0; r.s_from_acc = rj.from_acc ? 1 : 0;   // (not the sequential schedule: all types or none)
        for (int m = 0; m < rj.nmix; ++m) { r.s_filter[m] = h->filterid[g0 + m]; r.bias_off[m] = h->biasid[g0]; }
        t.runs.push_back(r);
    }
    for (const Group &g : h->groups) {
        t.group_slot0.push_back((int)t.slots.size());
        for (const CombineJob &cj : g.cjobs)
            for (int ch = cj.child_begin; ch < cj.child_end; ++ch) {
                const ChildDesc &cd = g.childs[ch];
                MmSlot s{};
                s.job_begin = cd.job_begin; s.nmix = cd.nmix; s.slot = cd.slot; s.npar = cj.npar;
                std::copy(cd.bias_off, cd.bias_off + kMaxMix, s.bias_off);
                t.slots.push_back(s);
            }
    }
    t.group_slot0.push_back((int)t.slots.size());
    const int cap = std::max(h->JGmax, 1);
    for (int gi = (int)h->groups.size() - 1; gi >= 0; --gi) {     // the groups are kept deepest first
        const Group &g = h->groups[gi];
        MmSlice cur{(int)t.jobs.size(), 0, (int)t.ctxs.size(), 0, (int)t.runs.size(), 0, 0, 0};
        for (const CombineJob &cj : g.cjobs)
            for (int ch = cj.child_begin; ch < cj.child_end; ++ch) {
                const ChildDesc &cd = g.childs[ch];
                const DtJob *fj = &g.jobs[cd.job_begin];
                int run = -1;
                for (int mq = 0; mq < cj.npar; ++mq) {
                    if (cur.njobs + cd.nmix > cap) { close_slice(t, cur); run = -1; }
                    MmCtx cx{};
                    cx.filter = cj.filter[mq]; cx.down = cj.acc_plane + mq; cx.out = cur.nctx;
                    cx.sib_begin = (int)t.sibs.size();
                    for (int c2 = cj.child_begin; c2 < cj.child_end; ++c2)
                        if (c2 != ch) t.sibs.push_back(g.childs[c2].slot + mq);
                    cx.sib_end = (int)t.sibs.size();
                    t.ctxs.push_back(cx);
                    if (run < 0) {
                        MmRun r{};
                        r.job0 = cur.njobs; r.nmix = cd.nmix; r.mq0 = mq; r.mq1 = mq; r.npar = cj.npar; r.gm0 = fj[0].gm;
                        r.s_from_acc = fj[0].from_acc;
                        for (int m = 0; m < cd.nmix; ++m) { r.s_filter[m] = fj[m].plane; r.bias_off[m] = cd.bias_off[m]; }
                        run = (int)t.runs.size();
                        t.runs.push_back(r);
                        cur.nruns += 1;
                    }
                    t.runs[run].mq1 = mq + 1;
                    for (int m = 0; m < cd.nmix; ++m) {
                        DtJob j = fj[m];                // the upward quadratic seen from the child: b and the anchor negated
                        j.plane = cur.nctx; j.from_acc = 1; j.gm = cur.njobs;
                        j.bx = -j.bx; j.by = -j.by; j.osx = -j.osx; j.osy = -j.osy;
                        t.jobs.push_back(j);
                        cur.njobs += 1;
                    }
                    cur.nctx += 1;
                }
            }
        close_slice(t, cur);
    }
}

int check_marginals_held(pbd_handle *h)
{
    if (h->res.plan && h->res.plan->padded)
        return fail(h, PBD_ERR_UNSUPPORTED, "max-marginals of a padded result (pbd_set_padding)");
    if (!h->res.plan || !h->res.marginals)
        return fail(h, PBD_ERR_STATE, "no max-marginals are held (pbd_max_marginals computes them; a detect call, pbd_dp_min or a model update drops them)");
    return PBD_OK;
}

// the decode of n seeds on the handle's stream; d_place NULL: the placements stay in the handle's workspace
int enqueue_decode(pbd_handle *h, int n, const int32_t *d_seeds, const float *scales, int frame_offset, int32_t *d_cand, int32_t *d_place,
                   int32_t *d_status)
{
    Plan &P = *h->res.plan;
    const float *d_scales = P.d_scales.p;
    if (scales) {
        HIPCHK(h, h->mm_scales.ensure(sizeof(float) * PBD_MAX_LEVELS));
        HIPCHK(h, hipMemcpyAsync(h->mm_scales.p, scales, sizeof(float) * P.nlevels, hipMemcpyHostToDevice, h->stream));
        d_scales = h->mm_scales.as<float>();
    } else if (!d_scales || P.kind != 0) {
        return fail(h, PBD_ERR_INVALID, "scales is NULL and the resident result has none of its own (pbd_dp_min)");
    }
    if (!h->mm_nmix.p) {
        std::vector<int> nmix;
        for (size_t gp = 0; gp + 1 < h->mix_offset.size(); ++gp) nmix.push_back(h->mix_offset[gp + 1] - h->mix_offset[gp]);
        HIPCHK(h, h->mm_nmix.upload(nmix));
    }
    if (!d_place) {
        HIPCHK(h, h->mm_place.ensure(std::max<size_t>((size_t)n * h->max_parts * 3 * sizeof(int32_t), 16)));
        d_place = h->mm_place.as<int32_t>();
    }
    MmParams p{};
    p.lv = P.d_lv.p; p.nlevels = P.nlevels;
    p.F = h->F; p.NS = h->NS; p.NC = h->NC; p.NM = h->NM; p.NJ = h->totmix;
    p.cell_per_frame = P.cell_per_frame; p.frame = h->res.mm_frame; p.ptr8 = P.ptr8 ? 1 : 0;
    p.Ik = h->Ik.as<uint8_t>(); p.IxRaw = h->IxRaw.p; p.IyRaw = h->IyRaw.p;
    p.mm = h->mm_val.p; p.Jx = h->mm_jx.as<int16_t>(); p.Jy = h->mm_jy.as<int16_t>(); p.Jk = h->mm_jk.as<int8_t>();
    p.walk = h->d_walk.p; p.walk_off = h->d_walk_off.p; p.part_nmix = h->mm_nmix.p;
    p.scales = d_scales;
    p.seeds = d_seeds; p.nseeds = n; p.stride = stride(h); p.max_parts = h->max_parts; p.frame_offset = frame_offset;
    p.cand = d_cand; p.place = d_place; p.status = d_status;
    { ProfScope ps(h, PBD_K_MM_DECODE, h->stream); launch_mm_decode(p, h->f64, h->stream); }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

}  // namespace

extern "C" {

int pbd_max_marginals(pbd_handle *h, int frame)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (int rc = check_bank(h)) return rc;
        if (h->seq_mode)
            return fail(h, PBD_ERR_UNSUPPORTED, "max-marginals of a model on the sequential schedule (a filter id shared inside a component)");
        if (h->resp_half) return fail(h, PBD_ERR_UNSUPPORTED, "max-marginals with fp16-resident responses (convolution modes 3 and 6)");
        if (h->shard_world > 1) return fail(h, PBD_ERR_UNSUPPORTED, "max-marginals on a level-sharded handle");
        Resident &r = h->res;
        if (r.latent) return fail(h, PBD_ERR_STATE, "the resident result is a latent one (pbd_detect_latent)");
        if (!r.plan || !r.resp || !r.dp)
            return fail(h, PBD_ERR_STATE, "no resident dynamic-program result (pbd_detect* or pbd_dp_min computes one; a model update leaves none)");
        if (r.plan->kind == 2) return fail(h, PBD_ERR_UNSUPPORTED, "max-marginals of a mixed-size result (pbd_detect_frames)");
        if (r.plan->padded) return fail(h, PBD_ERR_UNSUPPORTED, "max-marginals of a padded result (pbd_set_padding): the mirrored transforms take no pad");
        if (frame < 0 || frame >= r.frames) return fail(h, PBD_ERR_INVALID, "frame %d outside 0..%d", frame, r.frames - 1);
        Plan &P = *r.plan;
        r.marginals = false;          // the planes of an earlier call are overwritten from here on
        const size_t cpf = (size_t)P.cell_per_frame, rs = h->rs, pes = P.ptr8 ? 1 : 2;
        const int NJ = std::max(h->totmix, 1), NS = std::max(h->NS, 1), JG = std::max(h->JGmax, 1);
        HIPCHK(h, h->mm_val.ensure(std::max<size_t>(cpf * NJ * rs, 16)));
        HIPCHK(h, h->mm_down.ensure(std::max<size_t>(cpf * NJ * rs, 16)));
        HIPCHK(h, h->mm_jx.ensure(std::max<size_t>(cpf * NJ * 2, 16)));
        HIPCHK(h, h->mm_jy.ensure(std::max<size_t>(cpf * NJ * 2, 16)));
        HIPCHK(h, h->mm_jk.ensure(std::max<size_t>(cpf * NJ, 16)));
        HIPCHK(h, h->mm_msg.ensure(std::max<size_t>(cpf * NS * rs, 16)));
        HIPCHK(h, h->mm_ctx.ensure(std::max<size_t>(cpf * JG * rs, 16)));
        HIPCHK(h, h->mm_six.ensure(cpf * std::max(NJ, JG) * pes + 32));
        HIPCHK(h, h->mm_siy.ensure(cpf * std::max(NJ, JG) * pes + 32));

        MmTables t;
        build_tables(h, t);
        size_t off = 0;
        auto piece = [&](size_t bytes) { off = Carve::up(off, 256); const size_t o = off; off += bytes; return o; };
        const size_t o_jobs = piece(t.jobs.size() * sizeof(DtJob)), o_slots = piece(t.slots.size() * sizeof(MmSlot)),
                     o_ctxs = piece(t.ctxs.size() * sizeof(MmCtx)), o_sibs = piece(t.sibs.size() * sizeof(int)),
                     o_runs = piece(t.runs.size() * sizeof(MmRun));
        std::vector<uint8_t> blob(std::max<size_t>(off, 16), 0);
        auto put = [&](size_t o, const void *src, size_t bytes) { if (bytes) memcpy(blob.data() + o, src, bytes); };
        put(o_jobs, t.jobs.data(), t.jobs.size() * sizeof(DtJob));
        put(o_slots, t.slots.data(), t.slots.size() * sizeof(MmSlot));
        put(o_ctxs, t.ctxs.data(), t.ctxs.size() * sizeof(MmCtx));
        put(o_sibs, t.sibs.data(), t.sibs.size() * sizeof(int));
        put(o_runs, t.runs.data(), t.runs.size() * sizeof(MmRun));
        if (int rc = h->mm_tab.stage(h, blob.data(), blob.size())) return rc;
        const uint8_t *tb = h->mm_tab.as<uint8_t>();
        const hipStream_t st = h->stream;

        MmParams mp{};
        mp.lv = P.d_lv.p; mp.nlevels = P.nlevels;
        mp.F = h->F; mp.NS = NS; mp.NC = h->NC; mp.NM = h->NM; mp.NJ = NJ;
        mp.cell_per_frame = P.cell_per_frame; mp.quad_per_frame = P.quad_per_frame;
        mp.frame = frame; mp.ptr8 = P.ptr8 ? 1 : 0; mp.max_mix = h->max_mix;
        mp.resp = h->resp.p; mp.acc = h->acc.p; mp.biasw = h->d_biasw.p;
        mp.dt = h->dt.p; mp.sIx = h->mm_six.p; mp.sIy = h->mm_siy.p; mp.ctx = h->mm_ctx.p;
        mp.msg = h->mm_msg.p; mp.mm = h->mm_val.p; mp.down = h->mm_down.p;
        mp.Jx = h->mm_jx.as<int16_t>(); mp.Jy = h->mm_jy.as<int16_t>(); mp.Jk = h->mm_jk.as<int8_t>();
        mp.slots = reinterpret_cast<const MmSlot *>(tb + o_slots); mp.ctxs = reinterpret_cast<const MmCtx *>(tb + o_ctxs);
        mp.sibs = reinterpret_cast<const int *>(tb + o_sibs);

        // the transforms' parameter block: the detect path's, with the pointer planes in this call's scratch
        DpParams dp{};
        dp.lv = P.d_lv.p; dp.nlevels = P.nlevels; dp.F = h->F; dp.NS = h->NS; dp.NC = h->NC;
        dp.cell_per_frame = P.cell_per_frame; dp.quad_per_frame = P.quad_per_frame; dp.max_mix = h->max_mix;
        dp.ptr8 = P.ptr8 ? 1 : 0;
        dp.tmp = h->tmp.p; dp.dt = h->dt.p; dp.IxRaw = h->mm_six.p; dp.IyRaw = h->mm_siy.p;
        dp.stk = h->stk.p; dp.stk_per_jf = P.stk_per_jf;
        dp.stk_row_off = P.d_stk_row_off.p; dp.stk_col_off = P.d_stk_col_off.p;
        dp.biasw = h->d_biasw.p;
        dp.row2level = P.d_row2level.p; dp.rowoff = P.d_rowoff.p; dp.col2level = P.d_col2level.p; dp.coloff = P.d_coloff.p;
        dp.nrows_flat = P.nrows_flat; dp.ncols_flat = P.ncols_flat; dp.longest = P.longest;
        auto transforms = [&]() {
            { ProfScope ps(h, PBD_K_MM_DT_ROWS, st); launch_dt_rows(dp, h->dt_opt, 1, h->f64, st); }
            { ProfScope ps(h, PBD_K_MM_DT_COLS, st); launch_dt_cols(dp, h->dt_opt, 1, h->f64, st); }
        };

        // the roots: down_0, mm_0 and -1 in their pointer planes
        mp.runs = reinterpret_cast<const MmRun *>(tb + o_runs);
        { ProfScope ps(h, PBD_K_MM_DOWN, st); launch_mm_down(mp, h->NC, h->f64, st); }
        // the upward transforms again (their values were scratch), for the messages of every part
        for (size_t gi = 0; gi < h->groups.size(); ++gi) {
            const Group &g = h->groups[gi];
            dp.frame0 = frame; dp.resp = h->resp.p; dp.resp_half = 0; dp.acc = h->acc.p; dp.NM = h->NM;
            dp.NJ = NJ; dp.JG = (int)g.jobs.size(); dp.jobs = g.d_jobs.p; dp.bz_x = g.bz_x; dp.bz_y = g.bz_y;
            // the passes address their pointer planes by the frame of the batch (LevelPlanes::ix / iy), as the score planes they
            // read; the scratch holds one frame, so its base is given as if `frame` frames lay before it
            const size_t skip = (size_t)frame * cpf * NJ * pes;
            dp.IxRaw = reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(h->mm_six.p) - skip);
            dp.IyRaw = reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(h->mm_siy.p) - skip);
            transforms();
            MmParams m2 = mp;
            m2.JG = dp.JG; m2.slots = mp.slots + t.group_slot0[gi];
            ProfScope ps(h, PBD_K_MM_MESSAGES, st);
            launch_mm_messages(m2, t.group_slot0[gi + 1] - t.group_slot0[gi], h->f64, st);
        }
        // the downward pass, the root's children first
        for (const MmSlice &s : t.slices) {
            MmParams m2 = mp;
            m2.JG = s.njobs; m2.SJ = s.njobs; m2.NCTX = s.nctx;
            m2.ctxs = mp.ctxs + s.ctx0; m2.runs = mp.runs + s.run0;
            { ProfScope ps(h, PBD_K_MM_CONTEXT, st); launch_mm_context(m2, s.nctx, h->f64, st); }
            dp.frame0 = 0; dp.resp = nullptr; dp.resp_half = 0; dp.acc = h->mm_ctx.p; dp.NM = s.nctx;
            dp.IxRaw = h->mm_six.p; dp.IyRaw = h->mm_siy.p;
            dp.NJ = s.njobs; dp.JG = s.njobs; dp.jobs = reinterpret_cast<const DtJob *>(tb + o_jobs) + s.job0;
            dp.bz_x = s.bz_x; dp.bz_y = s.bz_y;
            transforms();
            { ProfScope ps(h, PBD_K_MM_DOWN, st); launch_mm_down(m2, s.nruns, h->f64, st); }
        }
        HIPCHK(h, hipGetLastError());
        r.marginals = true;
        r.mm_frame = frame;
        return PBD_OK;
    });
}

int pbd_get_marginals(pbd_handle *h, int level, int what, void *dst, size_t dst_bytes)
{
    return entry(h, dst, kIdle, [&]() -> int {
        if (int rc = check_marginals_held(h)) return rc;
        const Plan &P = *h->res.plan;
        if (level < 0 || level >= P.nlevels) return fail(h, PBD_ERR_INVALID, "level %d outside 0..%d", level, P.nlevels - 1);
        const LevelDesc &d = P.lv[level];
        const size_t n = (size_t)d.rows * d.cols * h->totmix, o = (size_t)d.cell_off * h->totmix;
        const bool value = what == PBD_MM_VALUES || what == PBD_MM_DOWN;
        if (!value && what != PBD_MM_PARENT_X && what != PBD_MM_PARENT_Y && what != PBD_MM_PARENT_K)
            return fail(h, PBD_ERR_INVALID, "unknown selector %d", what);
        const size_t bytes = n * (value ? h->rs : sizeof(int32_t));
        if (dst_bytes < bytes) return fail(h, PBD_ERR_INVALID, "destination holds %zu bytes, need %zu", dst_bytes, bytes);
        if (!n) return PBD_OK;
        if (value) {
            const DevBuf &src = what == PBD_MM_VALUES ? h->mm_val : h->mm_down;
            HIPCHK(h, hipMemcpyAsync(dst, src.as<char>() + o * h->rs, bytes, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            return PBD_OK;
        }
        int32_t *out = static_cast<int32_t *>(dst);
        if (what == PBD_MM_PARENT_K) {
            std::vector<int8_t> b(n);
            HIPCHK(h, hipMemcpyAsync(b.data(), h->mm_jk.as<int8_t>() + o, n, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (size_t i = 0; i < n; ++i) out[i] = b[i];
        } else {
            std::vector<int16_t> b(n);
            const DevBuf &src = what == PBD_MM_PARENT_X ? h->mm_jx : h->mm_jy;
            HIPCHK(h, hipMemcpyAsync(b.data(), src.as<int16_t>() + o, n * 2, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (size_t i = 0; i < n; ++i) out[i] = b[i];
        }
        return PBD_OK;
    });
}

int pbd_marginals_device(pbd_handle *h, int level, void **d_values)
{
    return entry(h, d_values, kIdle, [&]() -> int {
        if (int rc = check_marginals_held(h)) return rc;
        const Plan &P = *h->res.plan;
        if (level < 0 || level >= P.nlevels) return fail(h, PBD_ERR_INVALID, "level %d outside 0..%d", level, P.nlevels - 1);
        *d_values = h->mm_val.as<char>() + (size_t)P.lv[level].cell_off * h->totmix * h->rs;
        return PBD_OK;
    });
}

int pbd_marginal_poses_device(pbd_handle *h, int n, const int32_t *d_seeds, const float *scales, int frame_offset, int32_t *d_cand,
                              int32_t *d_place, int32_t *d_status)
{
    return entry(h, n <= 0 || (d_seeds && d_cand && d_status), kIdle, [&]() -> int {
        if (n < 0) return fail(h, PBD_ERR_INVALID, "n %d", n);
        if (int rc = check_marginals_held(h)) return rc;
        if (n == 0) return PBD_OK;
        return enqueue_decode(h, n, d_seeds, scales, frame_offset, d_cand, d_place, d_status);
    });
}

int pbd_marginal_poses(pbd_handle *h, int n, const int32_t *seeds, const float *scales, int frame_offset, int32_t *cand, int32_t *place,
                       int32_t *status)
{
    return entry(h, n <= 0 || (seeds && cand && status), kIdle, [&]() -> int {
        if (n < 0) return fail(h, PBD_ERR_INVALID, "n %d", n);
        if (int rc = check_marginals_held(h)) return rc;
        if (n == 0) return PBD_OK;
        const int stride = ::stride(h), mp = h->max_parts;
        const size_t sb = (size_t)n * 6 * sizeof(int32_t), cb = (size_t)n * stride * sizeof(int32_t),
                     pb = (size_t)n * mp * 3 * sizeof(int32_t), tb = (size_t)n * sizeof(int32_t);
        int32_t *d_seeds = nullptr, *d_cand = nullptr, *d_place = nullptr, *d_status = nullptr;
        if (int rc = carve(h, h->mm_in, [&](Carve &c) { d_seeds = c.take<int32_t>(sb); })) return rc;
        if (int rc = carve(h, h->mm_out, [&](Carve &c) {
                d_cand = c.take<int32_t>(cb); d_place = c.take<int32_t>(pb); d_status = c.take<int32_t>(tb);
            }))
            return rc;
        HIPCHK(h, hipMemcpyAsync(d_seeds, seeds, sb, hipMemcpyHostToDevice, h->stream));
        if (int rc = enqueue_decode(h, n, d_seeds, scales, frame_offset, d_cand, d_place, d_status)) return rc;
        std::vector<int32_t> hc(cb / sizeof(int32_t)), hp(place ? pb / sizeof(int32_t) : 0);
        HIPCHK(h, hipMemcpyAsync(status, d_status, tb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(hc.data(), d_cand, cb, hipMemcpyDeviceToHost, h->stream));
        if (place) HIPCHK(h, hipMemcpyAsync(hp.data(), d_place, pb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int i = 0; i < n; ++i) {                 // a bad seed's record and placement keep the caller's bytes
            const int np = std::min(status[i], mp);
            if (np <= 0) continue;
            memcpy(cand + (size_t)i * stride, hc.data() + (size_t)i * stride, (size_t)(8 + 4 * np) * sizeof(int32_t));
            if (place) memcpy(place + (size_t)i * mp * 3, hp.data() + (size_t)i * mp * 3, (size_t)np * 3 * sizeof(int32_t));
        }
        return PBD_OK;
    });
}

}  // extern "C"
