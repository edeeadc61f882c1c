// pbd_capi_train.hip -- the C entry points of training (include/pbd.h): the model vector and its in-place update, training
// examples and part scores of a resident detect result, latent positives, and the QP over a device-resident example cache.
// The handle and the layer they are written on: pbd_handle.h.
#include "pbd_handle.h"

using namespace pbd;

namespace {

// pbd_examples*: the resident result a record can be walked in (PBD_OK or the failure's status code)
int check_examples_state(pbd_handle *h)
{
    const Resident &r = resident_owner(h)->res;
    if (!r.plan || (r.plan->kind != 0 && r.plan->kind != 2) || !r.features || !r.dp)
        return fail(h, PBD_ERR_STATE, "no resident detect result (pbd_detect* computes one; pbd_dp_min and pbd_conv_set_filters leave none)");
    if (!h->bank_matches_model || h->filter_ksize != h->model_ksize)
        return fail(h, PBD_ERR_STATE, "the filter bank's sizes differ from the model's: the model vector no longer describes it");
    return PBD_OK;
}

// the host forms' check of records against the resident result (after check_examples_state): frame, level and component, and
// with `root` the root cell; a failure names the record
int check_resident_records(pbd_handle *h, const int32_t *cand, int ncand, int frame_offset, bool root)
{
    const int stride = ::stride(h);
    const Resident &res = resident_owner(h)->res;
    const Plan &P = *res.plan;
    for (int i = 0; i < ncand; ++i) {
        const int32_t *r = cand + (size_t)i * stride;
        const long long f = (long long)r[0] - frame_offset;
        int bf = 0, bl = 0;
        if (f < INT32_MIN || f > INT32_MAX || !resident_level(res, (int)f, r[2], &bf, &bl))
            return fail(h, PBD_ERR_INVALID, "record %d: frame %d - frame_offset %d / level %d outside the resident result", i, r[0],
                        frame_offset, r[2]);
        const LevelDesc &d = P.lv[bl];
        if (r[1] < 0 || r[1] >= h->NC) return fail(h, PBD_ERR_INVALID, "record %d: component %d (0..%d)", i, r[1], h->NC - 1);
        if (root && (r[3] < 0 || r[3] >= d.cols || r[4] < 0 || r[4] >= d.rows))
            return fail(h, PBD_ERR_INVALID, "record %d: root (%d, %d) outside the %d x %d map of level %d%s", i, r[3], r[4], d.cols,
                        d.rows, r[2], d.rows ? "" : " (a level of another rank)");
    }
    return PBD_OK;
}

// ---- part scores (the kernels: pbd_kernels_partscores.hip) ----------------------------------------------
// pbd_part_scores* / pbd_score_placements*: the state of pbd_examples*, and the responses the appearances are read from
int check_part_scores_state(pbd_handle *h)
{
    if (int rc = check_examples_state(h)) return rc;
    if (!resident_owner(h)->res.resp) return fail(h, PBD_ERR_STATE, "no resident responses");
    return PBD_OK;
}

// The placements (the walk's, or d_place_in's checked) and the four values per part of min(max(word 0, 0), capacity) records of
// d_in, on the handle's stream.  d_place NULL: the walk's placements stay in the handle's workspace
int enqueue_part_scores(pbd_handle *h, const int32_t *d_in, int capacity, int frame_offset, const int32_t *d_place_in,
                        int32_t *d_status, int32_t *d_place, void *d_scores)
{
    pbd_handle *o = resident_owner(h);   // its maps and responses, and the filter ids of its bank (the latent twin's differ)
    Plan &P = *o->res.plan;
    if (!o->sc_gm.p) {
        std::vector<ExGm> gm(o->totmix);
        for (int i = 0; i < o->totmix; ++i) gm[i] = ExGm{o->filterid[i], o->biasid[i], o->defid[i], 0};
        std::vector<int> anc(o->anchors), nmix;
        anc.push_back(0);
        for (size_t gp = 0; gp + 1 < o->mix_offset.size(); ++gp) nmix.push_back(o->mix_offset[gp + 1] - o->mix_offset[gp]);
        HIPCHK(h, o->sc_anchors.upload(anc));
        HIPCHK(h, o->sc_nmix.upload(nmix));
        HIPCHK(h, o->sc_gm.upload(gm));   // last: its presence marks the set complete
    }
    if (P.kind == 2 && !P.d_frame_lv0.p) HIPCHK(h, P.d_frame_lv0.upload(P.frame_lv0));
    if (!d_place && !d_place_in) {
        HIPCHK(h, h->sc_ws.ensure(std::max<size_t>((size_t)capacity * h->max_parts * 3 * sizeof(int32_t), 16)));
        d_place = h->sc_ws.as<int32_t>();
    }
    std::vector<float> defw(o->defw);
    defw.resize(defw.size() + 4, 0.f);
    if (int rc = h->sc_defw.stage(h, defw.data(), defw.size() * sizeof(float))) return rc;
    PartScoreParams pp{};
    pp.in = d_in; pp.in_cap = capacity; pp.stride = stride(h); pp.frame_offset = frame_offset;
    pp.lv = P.d_lv.p; pp.nlevels = P.nlevels;
    pp.nframes = P.kind == 2 ? P.mixed_frames : o->res.frames;
    pp.frame_lv0 = P.kind == 2 ? P.d_frame_lv0.p : nullptr;
    pp.cell_per_frame = P.cell_per_frame;
    pp.NC = o->NC; pp.NS = o->NS; pp.NJ = o->totmix; pp.ptr8 = P.ptr8 ? 1 : 0; pp.max_parts = h->max_parts;
    pp.walk_mode = h->walk_mode;
    pp.F = o->F; pp.NM = o->NM; pp.resp_half = o->resp_half ? 1 : 0;
    pp.resp = o->resp.p; pp.acc = o->acc.p;
    pp.rooti = o->rooti.as<int>(); pp.IxRaw = o->IxRaw.p; pp.IyRaw = o->IyRaw.p; pp.Ik = o->Ik.as<uint8_t>();
    pp.walk = o->d_walk.p; pp.walk_off = o->d_walk_off.p; pp.part_nmix = o->sc_nmix.p;
    pp.gm = o->sc_gm.p; pp.anchors = o->sc_anchors.p; pp.defw = h->sc_defw.as<float>(); pp.biasw = o->d_biasw.p;
    pp.place_in = d_place_in; pp.status = d_status; pp.place = d_place; pp.scores = d_scores;
    launch_part_scores(pp, h->f64, 0, h->stream);
    launch_part_scores(pp, h->f64, 1, h->stream);
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// Both host forms: `place_in` NULL: pbd_part_scores (place may be NULL), else pbd_score_placements.  A record's status always
// comes back; its placement and values only for the parts it has, so what lies past them, or belongs to a refused record, keeps
// the caller's bytes
int part_scores_host(pbd_handle *h, const int32_t *cand, int ncand, int frame_offset, const int32_t *place_in, int32_t *status,
                     int32_t *place, void *scores)
{
    if (ncand < 0) return fail(h, PBD_ERR_INVALID, "ncand %d", ncand);
    if (int rc = check_part_scores_state(h)) return rc;
    if (int rc = check_resident_records(h, cand, ncand, frame_offset, !place_in)) return rc;
    if (ncand == 0) return PBD_OK;
    const int stride = ::stride(h), mp = h->max_parts;
    const size_t rb = ((size_t)ncand * stride + 1) * sizeof(int32_t), pb = (size_t)ncand * mp * 3 * sizeof(int32_t);
    const size_t sb = (size_t)ncand * sizeof(int32_t), vb = (size_t)ncand * mp * 4 * h->rs;
    int32_t *d_rec = nullptr, *d_pin = nullptr, *d_status = nullptr, *d_place = nullptr;
    char *d_val = nullptr;
    if (int rc = carve(h, h->sc_rec, [&](Carve &c) { d_rec = c.take<int32_t>(rb); d_pin = c.take<int32_t>(place_in ? pb : 0); }))
        return rc;
    if (int rc = carve(h, h->sc_out, [&](Carve &c) {
            d_status = c.take<int32_t>(sb); d_place = c.take<int32_t>(place_in ? 0 : pb); d_val = c.take<char>(vb);
        }))
        return rc;
    HIPCHK(h, hipMemcpyAsync(d_rec, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_rec + 1, cand, rb - sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (place_in) HIPCHK(h, hipMemcpyAsync(d_pin, place_in, pb, hipMemcpyHostToDevice, h->stream));
    if (int rc = enqueue_part_scores(h, d_rec, ncand, frame_offset, place_in ? d_pin : nullptr, d_status, place_in ? nullptr : d_place,
                                     d_val))
        return rc;
    std::vector<char> hv(vb);
    std::vector<int32_t> hp(place && !place_in ? pb / sizeof(int32_t) : 0);
    HIPCHK(h, hipMemcpyAsync(status, d_status, sb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(hv.data(), d_val, vb, hipMemcpyDeviceToHost, h->stream));
    if (!hp.empty()) HIPCHK(h, hipMemcpyAsync(hp.data(), d_place, pb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < ncand; ++i) {
        const int np = std::min(status[i], mp);
        if (np <= 0) continue;
        memcpy(static_cast<char *>(scores) + (size_t)i * mp * 4 * h->rs, hv.data() + (size_t)i * mp * 4 * h->rs, (size_t)np * 4 * h->rs);
        if (!hp.empty()) memcpy(place + (size_t)i * mp * 3, hp.data() + (size_t)i * mp * 3, (size_t)np * 3 * sizeof(int32_t));
    }
    return PBD_OK;
}

// the walk and the gather of min(max(word 0, 0), capacity) records of d_in into d_hdr / d_values, on the handle's stream
int enqueue_examples(pbd_handle *h, const int32_t *d_in, int capacity, int frame_offset, int32_t *d_hdr, void *d_values)
{
    pbd_handle *o = resident_owner(h);   // its maps and features; the model tables (filter ids, offsets) stay this handle's
    Plan &P = *o->res.plan;
    if (!h->ex_gm.p) {
        std::vector<ExGm> gm(h->totmix);
        for (int i = 0; i < h->totmix; ++i) gm[i] = ExGm{h->filterid[i], h->biasid[i], h->defid[i], 0};
        HIPCHK(h, h->ex_gm.upload(gm));
        std::vector<int> anc(h->anchors);
        anc.push_back(0);
        HIPCHK(h, h->ex_anchors.upload(anc));
        HIPCHK(h, h->ex_foff.upload(h->model_foff));
    }
    if (P.kind == 2 && !P.d_frame_lv0.p) HIPCHK(h, P.d_frame_lv0.upload(P.frame_lv0));
    HIPCHK(h, h->ex_ws.ensure(std::max<size_t>((size_t)capacity * h->max_parts * sizeof(ExPart), 16)));
    ExampleParams ep{};
    ep.in = d_in; ep.in_cap = capacity; ep.stride = stride(h); ep.frame_offset = frame_offset;
    ep.lv = P.d_lv.p; ep.nlevels = P.nlevels;
    ep.nframes = P.kind == 2 ? P.mixed_frames : o->res.frames;
    ep.frame_lv0 = P.kind == 2 ? P.d_frame_lv0.p : nullptr;
    ep.cell_per_frame = P.cell_per_frame;
    ep.NC = h->NC; ep.NS = h->NS; ep.NJ = h->totmix; ep.ptr8 = P.ptr8 ? 1 : 0; ep.flen = 32; ep.max_parts = h->max_parts;
    ep.walk_mode = h->walk_mode;
    ep.rooti = o->rooti.as<int>(); ep.IxRaw = o->IxRaw.p; ep.IyRaw = o->IyRaw.p; ep.Ik = o->Ik.as<uint8_t>();
    ep.walk = h->d_walk.p; ep.walk_off = h->d_walk_off.p;
    ep.gm = h->ex_gm.p; ep.anchors = h->ex_anchors.p; ep.foff = h->ex_foff.p; ep.nbias = h->nbias; ep.ndefs = h->ndefs;
    ep.feat = o->feat.p;
    ep.parts = h->ex_ws.as<ExPart>();
    ep.hdr = d_hdr; ep.hdr_words = h->ex_hdr_words;
    ep.values = d_values; ep.vstride = h->ex_values;
    { ProfScope ps(h, PBD_K_EX_WALK, h->stream); launch_examples(ep, h->f64, 0, h->stream); }
    { ProfScope ps(h, PBD_K_EX_GATHER, h->stream); launch_examples(ep, h->f64, 1, h->stream); }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}


// ---- in-place model update (the kernels: pbd_kernels_model.hip) ------------------------------------------
// the host copy of the model vector, brought up to date with the device's after an update
int sync_mvec(pbd_handle *h)
{
    if (!h->mvec_stale) return PBD_OK;
    HIPCHK(h, hipMemcpyAsync(h->mvec.data(), h->d_mvec.p, h->mvec.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->mvec_stale = false;
    return PBD_OK;
}

size_t mu_status_bytes(const pbd_handle *h) { return 4 * sizeof(int) + ((size_t)h->nbias + 4 * (size_t)h->ndefs) * sizeof(float); }

// everything an update of h allocates or uploads (index tables on first use), so that nothing can fail once kernels are queued
int mu_prepare(pbd_handle *h)
{
    HIPCHK(h, h->d_mvec.ensure(std::max<size_t>(h->mvec.size(), 16)));
    HIPCHK(h, h->mu_status.ensure(mu_status_bytes(h)));
    HIPCHK(h, h->mu_status_host.ensure(mu_status_bytes(h), mu_status_bytes(h)));
    if (h->mu_foff.p) return PBD_OK;
    std::vector<int> gm_def(h->totmix, -1), root_bias(h->NC, 0);
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c];
        root_bias[c] = h->biasid[h->mix_offset[p0]];
        for (int gp = p0 + 1; gp < h->part_offset[c + 1]; ++gp)
            for (int gm = h->mix_offset[gp]; gm < h->mix_offset[gp + 1]; ++gm) gm_def[gm] = h->defid[gm];
    }
    std::vector<MuJobRef> jobs;
    for (Group &g : h->groups)
        for (size_t j = 0; j < g.jobs.size(); ++j) jobs.push_back(MuJobRef{g.d_jobs.p + j, h->defid[g.jobs[j].gm], 0});
    const long long fbase = (long long)h->nbias + 4LL * h->ndefs;
    std::vector<long long> foff(h->model_foff);
    for (long long &o : foff) o += fbase;
    HIPCHK(h, h->mu_gm_def.upload(gm_def));
    HIPCHK(h, h->mu_root_bias.upload(root_bias));
    HIPCHK(h, h->mu_jobs.upload(jobs));
    HIPCHK(h, h->mu_foff.upload(foff));   // last: its presence marks the set complete
    return PBD_OK;
}

// the update's kernels for handle h on stream st: its tables from `src`, the refusal flag and the status values at `status`
// (h's own block, or the block of the handle whose latent twin h is: the twin follows its owner's check)
void mu_enqueue(pbd_handle *h, const MuSource &src, char *status, bool check, hipStream_t st)
{
    MuParams p{};
    p.refused = reinterpret_cast<int *>(status);
    p.st_bias = reinterpret_cast<float *>(status + 4 * sizeof(int));
    p.st_def = p.st_bias + h->nbias;
    p.L = (int)(h->mvec.size() / h->rs); p.nbias = h->nbias; p.ndefs = h->ndefs; p.totmix = h->totmix; p.NC = h->NC;
    p.njobs = (int)h->mu_jobs.size;
    p.gm_def = h->mu_gm_def.p; p.root_bias = h->mu_root_bias.p;
    p.mvec = h->d_mvec.p; p.biasw = h->d_biasw.p; p.rjobs = h->d_rjobs.p; p.jobs = h->mu_jobs.p; p.foff = h->mu_foff.p;
    if (check) launch_mu_check(p, src, st);
    launch_mu_vector(p, src, h->f64, st);
    launch_mu_tables(p, h->f64, st);
    const bool mfma = conv_is_matrix_f32(h->cfg.conv_mode), f16 = conv_is_f16(h->cfg.conv_mode);
    for (pbd_handle::ConvClass &C : h->conv_classes) {
        MuClassParams cp{};
        cp.refused = p.refused; cp.mvec = p.mvec; cp.foff = p.foff; cp.fmap = C.fmap.p;
        cp.K = C.K; cp.nf = C.nf; cp.Fpad = C.Fpad; cp.group_layout = (!h->f64 && C.K == 5) ? 1 : 0;
        cp.wts = C.wts.p;
        cp.wts3 = C.wts3.as<float>(); cp.unit_f0 = C.unit_f0.p; cp.unit_ql = C.unit_ql.p; cp.unit_woff = C.unit_woff.p;
        cp.nunits = C.nunits;
        cp.c31tab = C.c31tab.p; cp.c31stride = C.c31stride;
        cp.wfrag64 = C.wfrag64.as<double>(); cp.qn = cp.wfrag64 ? conv_mfma_f64_qn(C.K) : 0;
        if (mfma) { cp.wrec = h->d_wrec.as<uint16_t>(); cp.wrec_f16 = f16; cp.nfilters = h->F; }
        if (mfma && C.wfrag16.p) { cp.wfrag16 = C.wfrag16.as<uint16_t>(); cp.any_cb = conv_mfma_any_cb(C.K, f16); }
        launch_mu_class(cp, h->f64, st);
    }
}

// the host's copies after a successful update: bias and deformation values, the root biases, the jobs' quadratics and the
// groups' variant flags by build_model's own predicate; the host model vector is behind until someone asks for it
void mu_finish(pbd_handle *h, const float *bias, const float *def)
{
    h->biasw.assign(bias, bias + h->nbias);
    h->defw.assign(def, def + 4 * (size_t)h->ndefs);
    for (int c = 0; c < h->NC; ++c) h->rjobs[c].bias = h->biasw[h->biasid[h->mix_offset[h->part_offset[c]]]];
    for (Group &g : h->groups) {
        for (DtJob &j : g.jobs) set_quadratics(j, &h->defw[(size_t)h->defid[j.gm] * 4]);
        set_variant_flags(g);
    }
    h->mvec_stale = true;
    h->res.drop_conv();   // the resident responses and maps were the old weights'
}

// the host-side refusals of an update: nothing is staged, queued or allocated before they pass
int check_update_state(pbd_handle *h)
{
    if (h->broken) return fail(h, PBD_ERR_STATE, "an earlier model update failed half way: the handle must be destroyed");
    if (h->nsubmitted != h->nwaited) return fail(h, PBD_ERR_STATE, "a submitted batch has not been waited for");
    if (int rc = check_bank(h)) return rc;
    if (h->filter_ksize != h->model_ksize)
        return fail(h, PBD_ERR_STATE, "the filter bank's sizes differ from the model's: the model vector no longer describes it");
    if (h->lat && h->lat->mvec.size() > h->mvec.size())
        return fail(h, PBD_ERR_STATE, "the latent twin's model vector is longer than the handle's");
    return PBD_OK;
}

// The update of h from `src` (pbd_model_vector_len values on the device, readable in h's stream order).  Every check that
// can refuse comes before the first kernel except the deformation check, which runs first on the device and gates the rest.
int update_model(pbd_handle *h, const MuSource &src)
{
    if (int rc = check_update_state(h)) return rc;
    pbd_handle *t = h->lat.get();
    if (int rc = mu_prepare(h)) return rc;
    if (t)
        if (int rc = mu_prepare(t)) return fail(h, rc, "latent twin: %s", t->err.c_str());
    char *status = h->mu_status.as<char>();
    HIPCHK(h, hipMemsetAsync(status, 0, 4 * sizeof(int), h->stream));
    mu_enqueue(h, src, status, true, h->stream);
    // the twin's filter gm is the block of filterid[gm] (its own offsets say so), bias and deformation values are the handle's
    if (t) mu_enqueue(t, MuSource{h->d_mvec.p, nullptr, nullptr, h->f64 ? kMuSrcF64 : kMuSrcF32}, status, false, h->stream);
    // From here to the read-back a HIP failure leaves device tables that may be new beside host copies that are old: the handle
    // is marked broken, and every later update and every call that needs the model (check_bank) refuses it with PBD_ERR_STATE.
    const char *host = h->mu_status_host.as<char>();
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h->mu_status_host.p, status, mu_status_bytes(h), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->broken = true;
        if (t) t->broken = true;
        return fail(h, PBD_ERR_HIP, "the model update failed on the device (%s): the handle's tables are undefined and it must be destroyed",
                    hipGetErrorString(e));
    }
    if (*reinterpret_cast<const int *>(host))
        return fail(h, PBD_ERR_INVALID, "a deformation's quadratic term (element 0 or 2) is zero in float32");
    const float *bias = reinterpret_cast<const float *>(host + 4 * sizeof(int)), *def = bias + h->nbias;
    mu_finish(h, bias, def);
    if (t) mu_finish(t, bias, def);
    return PBD_OK;
}

// ---- warped positives (the kernels: pbd_kernels_warp.hip) -----------------------------------------------
// Both forms of pbd_warp_positives.  Host form: `kept` set, d_payload NULL, hdr / values host buffers.  Device form: kept NULL,
// hdr / values device buffers.  Every refusal comes before the first copy or kernel.
int warp_positives(pbd_handle *h, int nframes, const pbd_frame *frames, int cn, int depth, int nboxes, const int32_t *boxes, int filter,
                   int bias, int skip_small, bool host, int id_offset, int32_t *d_payload, int capacity, int32_t *hdr, void *values,
                   int32_t *kept)
{
    if (nboxes < 0 || nframes < 0) return fail(h, PBD_ERR_INVALID, "nboxes %d, nframes %d", nboxes, nframes);
    if (!host) {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (nboxes > capacity) return fail(h, PBD_ERR_CAPACITY, "%d boxes, the payload holds %d records", nboxes, capacity);
    }
    if (int rc = check_bank(h)) return rc;
    if (h->filter_ksize != h->model_ksize)
        return fail(h, PBD_ERR_STATE, "the filter bank's sizes differ from the model's: the model vector no longer describes it");
    const int nfilters = (int)h->model_ksize.size();
    if (filter < 0 || filter >= nfilters) return fail(h, PBD_ERR_INVALID, "filter %d outside 0..%d", filter, nfilters - 1);
    if (bias < -1 || bias >= h->nbias) return fail(h, PBD_ERR_INVALID, "bias %d outside -1..%d", bias, h->nbias - 1);
    if (int rc = check_frame_descs(h, frames ? nframes : 0, frames, cn, depth, host)) return rc;   // frames may be NULL without boxes
    const int k = h->model_ksize[filter], s = h->sbin, P = (k + 2) * s;
    if ((bias >= 0 ? 1 : 0) + k * k * 32 > h->ex_values)   // a filter no part uses may be larger than any example
        return fail(h, PBD_ERR_INVALID, "filter %d (%d x %d) does not fit an example of %d values", filter, k, k, h->ex_values);
    constexpr int kCoordMax = 1 << 24;   // the tap positions of the resize are floats
    for (int i = 0; i < nboxes; ++i) {
        const int32_t *b = boxes + 5 * (size_t)i;
        if (b[0] < 0 || b[0] >= nframes) return fail(h, PBD_ERR_INVALID, "box %d: frame %d outside 0..%d", i, b[0], nframes - 1);
        if (b[3] < b[1] || b[4] < b[2]) return fail(h, PBD_ERR_INVALID, "box %d: (%d, %d) .. (%d, %d) is empty", i, b[1], b[2], b[3], b[4]);
        for (int c = 1; c < 5; ++c)
            if (b[c] < -kCoordMax || b[c] > kCoordMax) return fail(h, PBD_ERR_INVALID, "box %d: coordinate %d outside +-2^24", i, b[c]);
    }
    if (nboxes == 0) {
        if (d_payload) HIPCHK(h, hipMemsetAsync(d_payload, 0, sizeof(int32_t), h->stream));
        return PBD_OK;
    }
    // the kept boxes and their windows (warppos.m:21-26 in Matlab's 1-based coordinates; round() rounds halves away from zero)
    std::vector<int> slot(nboxes, -1), box_frame;
    struct Win { int x0, y0, w, h; };   // 0-based first column / row, size
    std::vector<Win> wins;
    const double minsize = ((double)k * s) * ((double)k * s);
    for (int i = 0; i < nboxes; ++i) {
        const int32_t *b = boxes + 5 * (size_t)i;
        const double width = (double)b[3] - b[1] + 1, height = (double)b[4] - b[2] + 1;
        const bool keep = !(skip_small && width * height < minsize);
        if (kept) kept[i] = keep ? 1 : 0;
        if (!keep) continue;
        const double padx = (double)s * width / ((double)k * s), pady = (double)s * height / ((double)k * s);
        const long long X1 = (long long)round(((double)b[1] + 1) - padx), X2 = (long long)round(((double)b[3] + 1) + padx);
        const long long Y1 = (long long)round(((double)b[2] + 1) - pady), Y2 = (long long)round(((double)b[4] + 1) + pady);
        slot[i] = (int)wins.size();
        wins.push_back(Win{(int)(X1 - 1), (int)(Y1 - 1), (int)(X2 - X1 + 1), (int)(Y2 - Y1 + 1)});
        box_frame.push_back(b[0]);
    }
    const int nkept = (int)wins.size();
    if ((long long)nkept * P * P > INT32_MAX) return fail(h, PBD_ERR_INVALID, "%d kept boxes of %d x %d pixels: more than 2^31 pixels in one call", nkept, P, P);

    // From here on the handle's pyramid and HOG workspaces are this call's: the resident detect result is gone.
    h->res.clear();
    std::vector<FrameDesc> fd;
    if (int rc = frame_descs(h, nframes, frames, cn, depth, host, fd)) return rc;
    Plan *W = nullptr;
    if (nkept)
        if (int rc = warp_plan(h, nkept, P, cn, depth, &W)) return rc;

    // one staged block: frames, box -> frame, box -> kept index, column taps, column and row coefficients
    const bool fix = depth == kDepth8U;
    const size_t cxs = fix ? sizeof(ResizeTabX) : sizeof(ResizeTabXf), cys = fix ? sizeof(ResizeTabY) : sizeof(ResizeTabYf);
    size_t off = 0;
    auto piece = [&](size_t bytes) { off = Carve::up(off, 256); const size_t o = off; off += bytes; return o; };
    const size_t o_fd = piece(fd.size() * sizeof(FrameDesc)), o_bf = piece((size_t)nkept * sizeof(int)), o_slot = piece((size_t)nboxes * sizeof(int)),
                 o_tap = piece((size_t)nkept * P * sizeof(WarpTap)), o_cx = piece((size_t)nkept * P * cxs), o_cy = piece((size_t)nkept * P * cys);
    std::vector<uint8_t> blob(off, 0);
    memcpy(blob.data() + o_fd, fd.data(), fd.size() * sizeof(FrameDesc));
    if (nkept) memcpy(blob.data() + o_bf, box_frame.data(), (size_t)nkept * sizeof(int));
    memcpy(blob.data() + o_slot, slot.data(), (size_t)nboxes * sizeof(int));
    std::vector<ResizeTabX> tx; std::vector<ResizeTabXf> txf; std::vector<ResizeTabY> ty; std::vector<ResizeTabYf> tyf;
    for (int j = 0; j < nkept; ++j) {
        const Win &w = wins[j];
        const pbd_frame &fr = frames[box_frame[j]];
        auto cx = [&](long long v) { return (int)std::min<long long>(std::max<long long>(v, 0), fr.cols - 1); };
        auto cy = [&](long long v) { return (int)std::min<long long>(std::max<long long>(v, 0), fr.rows - 1); };
        tx.clear(); txf.clear(); ty.clear(); tyf.clear();
        resize_taps_x(w.w, P, tx, txf);   // source = the window, destination = the patch
        resize_taps_y(w.h, P, ty, tyf);
        WarpTap *tap = reinterpret_cast<WarpTap *>(blob.data() + o_tap) + (size_t)j * P;
        for (int d = 0; d < P; ++d) {
            const int sx = tx[d].sx, sx1 = sx + 1 < w.w ? sx + 1 : sx;   // the second tap; none past the window's last column
            tap[d] = WarpTap{cx((long long)w.x0 + sx), cx((long long)w.x0 + sx1)};
            ty[d].y0 = tyf[d].y0 = cy((long long)w.y0 + ty[d].y0);
            ty[d].y1 = tyf[d].y1 = cy((long long)w.y0 + ty[d].y1);
        }
        if (fix) {
            memcpy(blob.data() + o_cx + (size_t)j * P * cxs, tx.data(), P * cxs);
            memcpy(blob.data() + o_cy + (size_t)j * P * cys, ty.data(), P * cys);
        } else {
            memcpy(blob.data() + o_cx + (size_t)j * P * cxs, txf.data(), P * cxs);
            memcpy(blob.data() + o_cy + (size_t)j * P * cys, tyf.data(), P * cys);
        }
    }
    int32_t *d_hdr = hdr;
    char *d_val = static_cast<char *>(values);
    const size_t hb = (size_t)nboxes * h->ex_hdr_words * sizeof(int32_t), vrow = (size_t)h->ex_values * h->rs;
    if (host)
        if (int rc = carve(h, h->wp_out, [&](Carve &c) { d_hdr = c.take<int32_t>(hb); d_val = c.take<char>(vrow * nboxes); })) return rc;
    if (int rc = h->wp_tab.stage(h, blob.data(), blob.size())) return rc;
    const uint8_t *tb = h->wp_tab.as<uint8_t>();
    WarpParams wp{};
    wp.fd = reinterpret_cast<const FrameDesc *>(tb + o_fd);
    wp.box_frame = reinterpret_cast<const int *>(tb + o_bf);
    wp.slot = reinterpret_cast<const int *>(tb + o_slot);
    wp.tapx = reinterpret_cast<const WarpTap *>(tb + o_tap);
    wp.cx = tb + o_cx; wp.cy = tb + o_cy;
    wp.nkept = nkept; wp.P = P; wp.cn = cn; wp.depth = depth;
    wp.pyr = h->pyr.as<uint8_t>();
    wp.nboxes = nboxes; wp.bias = bias;
    wp.filter_off = (int)((long long)h->nbias + 4LL * h->ndefs + h->model_foff[filter]);
    wp.filter_len = k * k * 32;
    wp.feat = h->feat.p;
    wp.hdr = d_hdr; wp.hdr_words = h->ex_hdr_words;
    wp.values = d_val; wp.vstride = h->ex_values;
    wp.payload = d_payload; wp.rec_stride = stride(h); wp.id_offset = id_offset;
    if (nkept) {
        { ProfScope ps(h, PBD_K_WARP, h->stream); launch_warp(wp, h->stream); }
        warp_hog(h, *W, cn, depth);
    }
    { ProfScope ps(h, PBD_K_WARP_EMIT, h->stream); launch_warp_emit(wp, h->f64, h->stream); }
    HIPCHK(h, hipGetLastError());
    if (!host) return PBD_OK;
    HIPCHK(h, hipMemcpyAsync(hdr, d_hdr, hb, hipMemcpyDeviceToHost, h->stream));
    // the values of every run of kept boxes, nvalues per row: nothing past nvalues and no row of a skipped box is written
    const size_t nvb = (size_t)((bias >= 0 ? 1 : 0) + k * k * 32) * h->rs;
    for (int i = 0; i < nboxes;) {
        if (slot[i] < 0) { ++i; continue; }
        int e = i;
        while (e < nboxes && slot[e] >= 0) ++e;
        HIPCHK(h, hipMemcpy2DAsync(static_cast<char *>(values) + vrow * i, vrow, d_val + vrow * i, vrow, nvb, (size_t)(e - i),
                                   hipMemcpyDeviceToHost, h->stream));
        i = e;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PBD_OK;
}

// ---- augmented positives (the kernel: pbd_kernels_augment.hip) --------------------------------------------
// The geometry of one copy (matlab/learning/map_rotate_points.m:20-35): the coefficients, the half sizes of the source (hA) and
// of the destination (hB), the destination's size.  Every product is rounded and the sums go left to right (this file is
// compiled with -ffp-contract=off), so partsbaseddetector_amd/augment.py computes the same sizes from the same coefficients.
struct AugGeom { int rotate, orows, ocols; double c, s, hAr, hAc, hBr, hBc; };
constexpr int kAugMaxSide = 32000;   // a frame's largest side (check_frame_descs)

bool augment_geom(int rows, int cols, double degrees, AugGeom *g)
{
    if (rows < 1 || cols < 1 || rows > kAugMaxSide || cols > kAugMaxSide || !std::isfinite(degrees)) return false;
    *g = AugGeom{0, rows, cols, 1.0, 0.0, ((double)rows - 1) / 2, ((double)cols - 1) / 2, 0, 0};
    if (degrees == 0) return true;
    g->rotate = 1;
    if (fmod(degrees, 90.0) == 0) {   // exact coefficients for the multiples of a quarter turn
        static const double kC[4] = {1, 0, -1, 0}, kS[4] = {0, 1, 0, -1};
        const int k = (int)((((long long)(fmod(degrees, 360.0) / 90.0)) % 4 + 4) % 4);
        g->c = kC[k]; g->s = kS[k];
    } else {
        const double phi = degrees * M_PI / 180;
        g->c = cos(phi); g->s = sin(phi);
    }
    // tformfwd([-hAr hAc; hAr hAc], [c s; -s c]): (u, v) -> (u c - v s, u s + v c)
    const double u0 = -g->hAr, u1 = g->hAr, v = g->hAc;
    const double mr = std::max(std::fabs(u0 * g->c - v * g->s), std::fabs(u1 * g->c - v * g->s));
    const double mc = std::max(std::fabs(u0 * g->s + v * g->c), std::fabs(u1 * g->s + v * g->c));
    g->hBr = ceil(mr / 2) * 2;
    g->hBc = ceil(mc / 2) * 2;
    g->orows = (int)(2 * g->hBr + 1);
    g->ocols = (int)(2 * g->hBc + 1);
    return true;
}

// the bytes [first, last) a frame's pixels occupy
inline std::pair<uintptr_t, uintptr_t> frame_span(const pbd_frame &f, size_t px)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(f.data);
    return {a, a + (size_t)(f.rows - 1) * f.stride_bytes + (size_t)f.cols * px};
}

// Both forms of pbd_augment_frames.  Every refusal comes before the first copy or kernel.
int augment_frames(pbd_handle *h, int nframes, const pbd_frame *frames, int cn, int depth, int njobs, const pbd_augment *jobs,
                   const pbd_frame *out, bool host)
{
    if (njobs < 0 || nframes < 0) return fail(h, PBD_ERR_INVALID, "njobs %d, nframes %d", njobs, nframes);
    if (int rc = check_frame_descs(h, frames ? nframes : 0, frames, cn, depth, host)) return rc;   // frames may be NULL without jobs
    const size_t es = depth_size(depth), px = es * cn;
    std::vector<AugGeom> geom(njobs);
    long long ntiles = 0;
    for (int i = 0; i < njobs; ++i) {
        const pbd_augment &a = jobs[i];
        if (a.frame < 0 || a.frame >= nframes) return fail(h, PBD_ERR_INVALID, "job %d: frame %d outside 0..%d", i, a.frame, nframes - 1);
        if (!std::isfinite(a.degrees)) return fail(h, PBD_ERR_INVALID, "job %d: degrees is not finite", i);
        const pbd_frame &src = frames[a.frame], &o = out[i];
        if (!augment_geom(src.rows, src.cols, a.degrees, &geom[i])) return fail(h, PBD_ERR_INVALID, "job %d: no plan", i);
        if (!o.data) return fail(h, PBD_ERR_INVALID, "job %d: the destination is a null pointer", i);
        if (o.rows != geom[i].orows || o.cols != geom[i].ocols)
            return fail(h, PBD_ERR_INVALID, "job %d: destination %dx%d, the plan says %dx%d", i, o.rows, o.cols, geom[i].orows, geom[i].ocols);
        if (o.stride_bytes < (size_t)o.cols * px)
            return fail(h, PBD_ERR_INVALID, "job %d: destination stride %zu < row bytes %zu", i, o.stride_bytes, (size_t)o.cols * px);
        if (!host && (reinterpret_cast<uintptr_t>(o.data) % es || o.stride_bytes % es))
            return fail(h, PBD_ERR_INVALID, "job %d: destination pointer %p / stride %zu not a multiple of the %zu-byte element", i, o.data,
                        o.stride_bytes, es);
        const auto d = frame_span(o, px);
        for (int f = 0; f < nframes; ++f) {
            const auto s = frame_span(frames[f], px);
            if (d.first < s.second && s.first < d.second) return fail(h, PBD_ERR_INVALID, "job %d: the destination overlaps frame %d", i, f);
        }
        ntiles += (long long)((o.rows + kAugTileRows - 1) / kAugTileRows) * ((o.cols + kAugTileCols - 1) / kAugTileCols);
    }
    if (ntiles > (1LL << 26)) return fail(h, PBD_ERR_INVALID, "%lld tiles in one call (at most 2^26)", ntiles);
    if (njobs == 0) return PBD_OK;

    // host form: the frames that have a job and every destination packed into the call's own buffer
    std::vector<const uint8_t *> d_src(nframes, nullptr);
    std::vector<long long> spitch(nframes, 0);
    std::vector<uint8_t *> d_dst(njobs, nullptr);
    if (host) {
        std::vector<char> used(nframes, 0);
        for (int i = 0; i < njobs; ++i) used[jobs[i].frame] = 1;
        size_t off = 0;
        std::vector<size_t> so(nframes, 0), dofs(njobs, 0);
        for (int f = 0; f < nframes; ++f)
            if (used[f]) { off = Carve::up(off, 256); so[f] = off; off += (size_t)frames[f].rows * frames[f].cols * px; }
        for (int i = 0; i < njobs; ++i) { off = Carve::up(off, 256); dofs[i] = off; off += (size_t)out[i].rows * out[i].cols * px; }
        HIPCHK(h, h->aug_buf.ensure(off + 16));
        uint8_t *base = h->aug_buf.as<uint8_t>();
        for (int f = 0; f < nframes; ++f) {
            if (!used[f]) continue;
            const size_t rb = (size_t)frames[f].cols * px;
            HIPCHK(h, hipMemcpy2DAsync(base + so[f], rb, frames[f].data, frames[f].stride_bytes, rb, frames[f].rows, hipMemcpyHostToDevice,
                                       h->stream));
            d_src[f] = base + so[f];
            spitch[f] = (long long)rb;
        }
        for (int i = 0; i < njobs; ++i) d_dst[i] = base + dofs[i];
    } else {
        for (int f = 0; f < nframes; ++f) { d_src[f] = static_cast<const uint8_t *>(frames[f].data); spitch[f] = (long long)frames[f].stride_bytes; }
        for (int i = 0; i < njobs; ++i) d_dst[i] = static_cast<uint8_t *>(const_cast<void *>(out[i].data));
    }

    // one staged block: the job table, then the tile table over every destination
    const size_t o_tiles = Carve::up((size_t)njobs * sizeof(AugJob), 256);
    std::vector<uint8_t> blob(o_tiles + (size_t)ntiles * sizeof(AugTile), 0);
    AugJob *J = reinterpret_cast<AugJob *>(blob.data());
    AugTile *T = reinterpret_cast<AugTile *>(blob.data() + o_tiles);
    long long nt = 0;
    for (int i = 0; i < njobs; ++i) {
        const AugGeom &g = geom[i];
        const int f = jobs[i].frame;
        J[i] = AugJob{d_src[f], d_dst[i], spitch[f], host ? (long long)((size_t)out[i].cols * px) : (long long)out[i].stride_bytes,
                      frames[f].rows, frames[f].cols, g.orows, g.ocols, jobs[i].mirror ? 1 : 0, g.rotate, g.c, g.s, g.hAr, g.hAc, g.hBr,
                      g.hBc};
        for (int y = 0; y < g.orows; y += kAugTileRows)
            for (int x = 0; x < g.ocols; x += kAugTileCols) T[nt++] = AugTile{i, y, x};
    }
    if (int rc = h->aug_tab.stage(h, blob.data(), blob.size())) return rc;
    AugParams ap{};
    ap.jobs = h->aug_tab.as<AugJob>();
    ap.tiles = reinterpret_cast<const AugTile *>(h->aug_tab.as<uint8_t>() + o_tiles);
    ap.ntiles = (int)ntiles; ap.cn = cn; ap.depth = depth;
    launch_augment(ap, h->stream);   // (no id in the handle's profile: the probe times the call with events on pbd_stream())
    HIPCHK(h, hipGetLastError());
    if (!host) return PBD_OK;
    for (int i = 0; i < njobs; ++i) {   // the used width of every row only: bytes beyond it are the caller's
        const size_t rb = (size_t)out[i].cols * px;
        HIPCHK(h, hipMemcpy2DAsync(const_cast<void *>(out[i].data), out[i].stride_bytes, d_dst[i], rb, rb, out[i].rows, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PBD_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

// Augmented positives: the plan and the points on the host, the frames on the device.  See include/pbd.h.
int pbd_augment_plan(int rows, int cols, double degrees, int *out_rows, int *out_cols, double coef[2])
{
    return guarded(nullptr, [&]() -> int {
        AugGeom g;
        if (!out_rows || !out_cols || !coef) return fail(nullptr, PBD_ERR_INVALID, "pbd_augment_plan: a null output");
        if (!augment_geom(rows, cols, degrees, &g))
            return fail(nullptr, PBD_ERR_INVALID, "pbd_augment_plan: %dx%d (1..%d) by %g degrees (finite)", rows, cols, kAugMaxSide, degrees);
        *out_rows = g.orows; *out_cols = g.ocols; coef[0] = g.c; coef[1] = g.s;
        return PBD_OK;
    });
}

int pbd_augment_points(int rows, int cols, double degrees, int mirror, int npoints, const double *xy, double *xy_out)
{
    return guarded(nullptr, [&]() -> int {
        AugGeom g;
        if (npoints < 0 || (npoints > 0 && (!xy || !xy_out))) return fail(nullptr, PBD_ERR_INVALID, "pbd_augment_points: npoints %d", npoints);
        if (!augment_geom(rows, cols, degrees, &g))
            return fail(nullptr, PBD_ERR_INVALID, "pbd_augment_points: %dx%d (1..%d) by %g degrees (finite)", rows, cols, kAugMaxSide, degrees);
        for (int i = 0; i < npoints; ++i) {
            double x = xy[2 * i], y = xy[2 * i + 1];
            if (mirror) x = ((double)cols - 1) - x;
            if (g.rotate) {   // map_rotate_points.m:40: tformfwd(p + loA, rotate) - loB with p = [y x]
                const double u = y - g.hAr, v = x - g.hAc;
                y = (u * g.c - v * g.s) + g.hBr;
                x = (u * g.s + v * g.c) + g.hBc;
            }
            xy_out[2 * i] = x; xy_out[2 * i + 1] = y;
        }
        return PBD_OK;
    });
}

int pbd_augment_frames(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, int njobs,
                       const pbd_augment *jobs, const pbd_frame *out)
{
    return entry(h, njobs <= 0 || (frames && jobs && out), kIdle, [&]() -> int {
        return augment_frames(h, nframes, frames, channels, depth_code, njobs, jobs, out, true);
    });
}

int pbd_augment_frames_device(pbd_handle *h, int nframes, const pbd_frame *d_frames, int channels, int depth_code, int njobs,
                              const pbd_augment *jobs, const pbd_frame *d_out)
{
    return entry(h, njobs <= 0 || (d_frames && jobs && d_out), kIdle, [&]() -> int {
        return augment_frames(h, nframes, d_frames, channels, depth_code, njobs, jobs, d_out, false);
    });
}

// Warped positives (matlab/learning/train.m poswarp, warppos.m, qp_poswrite).  See include/pbd.h.
int pbd_warp_positives(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, int nboxes,
                       const int32_t *boxes, int filter, int bias, int skip_small, int32_t *hdr, void *values, int32_t *kept)
{
    return entry(h, nboxes <= 0 || (frames && boxes && hdr && values && kept), kIdle, [&]() -> int {
        return warp_positives(h, nframes, frames, channels, depth_code, nboxes, boxes, filter, bias, skip_small, true, 0, nullptr, 0, hdr,
                              values, kept);
    });
}

int pbd_warp_positives_device(pbd_handle *h, int nframes, const pbd_frame *d_frames, int channels, int depth_code, int nboxes,
                              const int32_t *boxes, int filter, int bias, int skip_small, int id_offset, int32_t *d_payload,
                              int capacity, int32_t *d_hdr, void *d_values)
{
    return entry(h, d_payload && (nboxes <= 0 || (d_frames && boxes && d_hdr && d_values)), kIdle, [&]() -> int {
        return warp_positives(h, nframes, d_frames, channels, depth_code, nboxes, boxes, filter, bias, skip_small, false, id_offset,
                              d_payload, capacity, d_hdr, d_values, nullptr);
    });
}

// Training examples (matlab/detection/detect.m backtrack + qp_write).  See include/pbd.h.
int pbd_model_vector_len(const pbd_handle *h) { return h ? (int)(h->mvec.size() / h->rs) : 0; }

int pbd_model_vector(pbd_handle *h, void *w)
{
    return entry(h, w, kBusyOk, [&]() -> int {
        if (int rc = sync_mvec(h)) return rc;
        memcpy(w, h->mvec.data(), h->mvec.size());
        return PBD_OK;
    });
}

// In-place model update.  See include/pbd.h and DESIGN.md section 6j.
int pbd_set_model_vector_device(pbd_handle *h, const void *d_w, int real_code)
{
    return entry(h, d_w, kIdle, [&]() -> int {
        if (real_code != PBD_REAL_F32 && real_code != PBD_REAL_F64)
            return fail(h, PBD_ERR_INVALID, "real_code %d: PBD_REAL_F32 or PBD_REAL_F64", real_code);
        return update_model(h, MuSource{d_w, nullptr, nullptr, real_code == PBD_REAL_F64 ? kMuSrcF64 : kMuSrcF32});
    });
}

int pbd_set_model_vector(pbd_handle *h, const void *w)
{
    return entry(h, w, kIdle, [&]() -> int {
        if (int rc = check_update_state(h)) return rc;
        HIPCHK(h, h->mu_src.ensure(std::max<size_t>(h->mvec.size(), 16)));
        HIPCHK(h, hipMemcpyAsync(h->mu_src.p, w, h->mvec.size(), hipMemcpyHostToDevice, h->stream));
        const int rc = update_model(h, MuSource{h->mu_src.p, nullptr, nullptr, h->f64 ? kMuSrcF64 : kMuSrcF32});
        if (rc != PBD_OK) (void)hipStreamSynchronize(h->stream);   // w is the caller's again when the call returns
        return rc;
    });
}

int pbd_set_thresh(pbd_handle *h, float thresh)
{
    return entry(h, true, kIdle, [&]() -> int {
        h->thresh = thresh;
        if (h->lat) h->lat->thresh = thresh;
        return PBD_OK;
    });
}

int pbd_example_stride(const pbd_handle *h, int *hdr_words, int *values)
{
    if (!h || !hdr_words || !values) return PBD_ERR_INVALID;
    *hdr_words = h->ex_hdr_words;
    *values = h->ex_values;
    return PBD_OK;
}

int pbd_examples(pbd_handle *h, const int32_t *cand, int ncand, int frame_offset, int32_t *hdr, void *values)
{
    return entry(h, ncand <= 0 || (cand && hdr && values), kIdle, [&]() -> int {
        if (ncand < 0) return fail(h, PBD_ERR_INVALID, "ncand %d", ncand);
        if (int rc = check_examples_state(h)) return rc;
        const int stride = ::stride(h);
        if (int rc = check_resident_records(h, cand, ncand, frame_offset, true)) return rc;
        if (ncand == 0) return PBD_OK;
        const size_t hb = (size_t)ncand * h->ex_hdr_words * sizeof(int32_t), vb = (size_t)ncand * h->ex_values * h->rs;
        int32_t *d_hdr = nullptr;
        char *d_val = nullptr;
        HIPCHK(h, h->ex_rec.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
        if (int rc = carve(h, h->ex_out, [&](Carve &c) { d_hdr = c.take<int32_t>(hb); d_val = c.take<char>(vb); })) return rc;
        HIPCHK(h, hipMemcpyAsync(h->ex_rec.p, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->ex_rec.as<int32_t>() + 1, cand, (size_t)ncand * stride * sizeof(int32_t), hipMemcpyHostToDevice,
                                 h->stream));
        if (int rc = enqueue_examples(h, h->ex_rec.as<int32_t>(), ncand, frame_offset, d_hdr, d_val)) return rc;
        // an example's values come back up to its nvalues: what lies past them in the workspace is an earlier call's, and the
        // caller's bytes there stay ("values past nvalues are not written")
        std::vector<char> hv(vb);
        HIPCHK(h, hipMemcpyAsync(hdr, d_hdr, hb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(hv.data(), d_val, vb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const size_t vrow = (size_t)h->ex_values * h->rs;
        for (int i = 0; i < ncand; ++i) {
            const int nv = std::min(std::max(hdr[(size_t)i * h->ex_hdr_words + 3], 0), h->ex_values);
            memcpy(static_cast<char *>(values) + vrow * i, hv.data() + vrow * i, (size_t)nv * h->rs);
        }
        return PBD_OK;
    });
}

// Latent positives (matlab/detection/detect.m with a bbox: testoverlap masks, bbox.m fixed mixtures).  See include/pbd.h.
// Both forms: `host` says where enqueue_detect_mixed reads the frames (host pointers, or device pointers read in place).
static int detect_latent(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, const int32_t *boxes,
                         const int32_t *mixtures, float overlap, int32_t *cand, int32_t *found, bool host)
{
    return entry(h, frames && boxes && cand && found, kIdle, [&]() -> int {
        if (h->shard_world > 1)
            return fail(h, PBD_ERR_UNSUPPORTED, "latent detection with level sharding (world %d): the best root is over every level",
                        h->shard_world);
        const int nparts = h->part_offset[1] - h->part_offset[0];
        for (int c = 1; c < h->NC; ++c)
            if (h->part_offset[c + 1] - h->part_offset[c] != nparts)
                return fail(h, PBD_ERR_UNSUPPORTED, "latent detection needs one part count in every component (component %d has %d, "
                            "component 0 %d)", c, h->part_offset[c + 1] - h->part_offset[c], nparts);
        // (PBD_CONV_MFMA_F16_ANY masks its fp16 responses with the most negative finite half, kLatentMaskHalf)
        if (h->resp_half && !conv_is_any(h->cfg.conv_mode))
            return fail(h, PBD_ERR_UNSUPPORTED, "latent detection in PBD_CONV_MFMA_F16: -1e10 has no fp16 value");
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        if (int rc = check_bank(h)) return rc;
        if (h->filter_ksize != h->model_ksize) return fail(h, PBD_ERR_STATE, "the filter bank's sizes differ from the model's");
        if (!h->lat) {   // the latent twin: the same model with one filter per (component, part, mixture), on this handle's stream
            const int T = h->totmix;
            std::vector<int> ks(T), fid(T);
            std::vector<int64_t> off(T);
            for (int gm = 0; gm < T; ++gm) {
                fid[gm] = gm;
                ks[gm] = h->model_ksize[h->filterid[gm]];
                off[gm] = h->model_foff[h->filterid[gm]];
            }
            const size_t fbase = (size_t)h->nbias + 4 * (size_t)h->ndefs;
            if (int rc = sync_mvec(h)) return rc;   // after an in-place update the twin starts from the new weights
            pbd_model m{};
            m.ncomponents = h->NC; m.nfilters = T; m.flen = 32; m.filter_ksize = ks.data(); m.filter_offset = off.data();
            if (h->f64) m.filters_f64 = reinterpret_cast<const double *>(h->mvec.data()) + fbase;
            else m.filters_f32 = reinterpret_cast<const float *>(h->mvec.data()) + fbase;
            m.nbias = h->nbias; m.biasw = h->biasw.data(); m.ndefs = h->ndefs; m.defw = h->defw.data(); m.anchors = h->anchors.data();
            m.part_offset = h->part_offset.data(); m.parentid = h->parentid.data(); m.mix_offset = h->mix_offset.data();
            m.filterid = fid.data(); m.biasid = h->biasid.data(); m.defid = h->defid.data();
            m.thresh = h->thresh; m.sbin = h->sbin; m.interval = h->interval; m.norient = h->norient;
            pbd_config cfg = h->cfg;
            cfg.max_candidates = std::max(cfg.max_batch, 1);
            cfg.stream = reinterpret_cast<void *>(h->stream.s);
            pbd_handle *t = nullptr;
            if (int rc = pbd_create(&m, &cfg, &t)) return fail(h, rc, "latent twin: %s", pbd_last_error(nullptr));
            h->lat.reset(t);
            t->walk_mode = h->walk_mode;
            t->padx = h->padx; t->pady = h->pady;
            t->fine_octave = h->fine_octave;
            std::vector<int4> gm(T);
            for (int c = 0; c < h->NC; ++c)
                for (int gp = h->part_offset[c]; gp < h->part_offset[c + 1]; ++gp)
                    for (int g = h->mix_offset[gp]; g < h->mix_offset[gp + 1]; ++g)
                        gm[g] = make_int4(gp - h->part_offset[c], g - h->mix_offset[gp], ks[g], 0);
            HIPCHK(h, h->lat_gm.upload(gm));
        }
        pbd_handle *t = h->lat.get();
        Plan *P = nullptr;
        if (int rc = check_frames_mixed(t, nframes, frames, channels, depth_code, host, &P)) return fail(h, rc, "%s", t->err.c_str());
        const size_t nb = (size_t)nframes * nparts;
        HIPCHK(h, h->lat_in.ensure(nb * sizeof(int4) + nb * sizeof(int) + 64));
        HIPCHK(h, hipMemcpyAsync(h->lat_in.p, boxes, nb * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        int *d_mix = reinterpret_cast<int *>(h->lat_in.as<char>() + nb * sizeof(int4));
        if (mixtures) HIPCHK(h, hipMemcpyAsync(d_mix, mixtures, nb * sizeof(int), hipMemcpyHostToDevice, h->stream));
        if (!P->d_frame_lv0.p) HIPCHK(h, P->d_frame_lv0.upload(P->frame_lv0));
        const int stride = ::stride(h);
        HIPCHK(h, h->lat_pay.ensure(((size_t)nframes * stride + 1) * sizeof(int32_t)));
        h->res = Resident{};
        h->res.latent = true;
        LatentParams lp{};
        lp.gmtab = h->lat_gm.p; lp.boxes = h->lat_in.as<int4>(); lp.mix = mixtures ? d_mix : nullptr; lp.nparts = nparts;
        lp.overlap = (double)overlap;
        if (int rc = enqueue_detect_mixed(t, *P, nframes, frames, channels, depth_code, host, &lp)) return fail(h, rc, "%s", t->err.c_str());
        lp.rootv = t->rootv.p; lp.rooti = t->rooti.as<int>(); lp.lv = P->d_lv.p; lp.nlevels = P->nlevels;
        lp.cell_per_frame = P->cell_per_frame; lp.frame_lv0 = P->d_frame_lv0.p; lp.nframes = nframes; lp.NC = h->NC;
        lp.stride = stride; lp.payload = h->lat_pay.as<int32_t>();
        launch_latent_best(lp, h->f64, h->stream);
        if (int rc = enqueue_argmin(t, *P, 1, P->d_scales.p, 0, lp.payload, nframes, h->stream, true)) return fail(h, rc, "%s", t->err.c_str());
        HIPCHK(h, hipMemcpyAsync(cand, lp.payload + 1, (size_t)nframes * stride * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipGetLastError());
        for (int f = 0; f < nframes; ++f) {
            float sc;
            memcpy(&sc, &cand[(size_t)f * stride + 5], sizeof sc);
            found[f] = sc > (h->resp_half ? kLatentFoundHalf : -5e9f) ? 1 : 0;
        }
        return PBD_OK;
    });
}

int pbd_detect_latent(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, const int32_t *boxes,
                      const int32_t *mixtures, float overlap, int32_t *cand, int32_t *found)
{
    return detect_latent(h, nframes, frames, channels, depth_code, boxes, mixtures, overlap, cand, found, true);
}

int pbd_detect_latent_device(pbd_handle *h, int nframes, const pbd_frame *d_frames, int channels, int depth_code, const int32_t *boxes,
                             const int32_t *mixtures, float overlap, int32_t *cand, int32_t *found)
{
    return detect_latent(h, nframes, d_frames, channels, depth_code, boxes, mixtures, overlap, cand, found, false);
}

int pbd_examples_device(pbd_handle *h, const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_hdr, void *d_values)
{
    return entry(h, d_payload && (capacity <= 0 || (d_hdr && d_values)), kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = check_examples_state(h)) return rc;
        if (capacity == 0) return PBD_OK;
        return enqueue_examples(h, d_payload, capacity, frame_offset, d_hdr, d_values);
    });
}

int pbd_part_scores(pbd_handle *h, const int32_t *cand, int ncand, int frame_offset, int32_t *status, int32_t *place, void *scores)
{
    return entry(h, ncand <= 0 || (cand && status && scores), kIdle, [&]() -> int {
        return part_scores_host(h, cand, ncand, frame_offset, nullptr, status, place, scores);
    });
}

int pbd_part_scores_device(pbd_handle *h, const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_status, int32_t *d_place,
                           void *d_scores)
{
    return entry(h, d_payload && (capacity <= 0 || (d_status && d_scores)), kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = check_part_scores_state(h)) return rc;
        if (capacity == 0) return PBD_OK;
        return enqueue_part_scores(h, d_payload, capacity, frame_offset, nullptr, d_status, d_place, d_scores);
    });
}

int pbd_score_placements(pbd_handle *h, const int32_t *cand, int ncand, int frame_offset, const int32_t *place, int32_t *status,
                         void *scores)
{
    return entry(h, ncand <= 0 || (cand && place && status && scores), kIdle, [&]() -> int {
        return part_scores_host(h, cand, ncand, frame_offset, place, status, nullptr, scores);
    });
}

int pbd_score_placements_device(pbd_handle *h, const int32_t *d_payload, int capacity, int frame_offset, const int32_t *d_place,
                                int32_t *d_status, void *d_scores)
{
    return entry(h, d_payload && (capacity <= 0 || (d_place && d_status && d_scores)), kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = check_part_scores_state(h)) return rc;
        if (capacity == 0) return PBD_OK;
        return enqueue_part_scores(h, d_payload, capacity, frame_offset, d_place, d_status, nullptr, d_scores);
    });
}

}  // extern "C"

// ================================================================================================
// The training QP (matlab/learning/qp_*.m).  See include/pbd.h and DESIGN.md section 6i.  The kernels are in
// pbd_kernels_qp.hip; the host keeps the ids, block tables and b of the entries (for the grouping, the refresh's entry lists
// and l) and orders every call; all per-value work is on the device.
struct pbd_qp : pbd::ErrCtx {
    Stream stream;
    int cap = 0, L = 0, V = 0, HW = 0, MB = 0, in_hw = 0;
    int rec_stride = 0;            // record words of the handle the QP was created from
    hipStream_t src_stream = nullptr;   // that handle's stream, compared only (the handle may be gone)
    uint64_t fp = 0;
    double Cpos = 0, Cneg = 0;
    DevBuf x, bm, hd, ids, b, d, a, sv, w, wraw, misc, stage, work, lc, scratch;
    DevTable<double> wreg, w0;
    DevTable<int> noneg, slot_of, slot_len;
    std::vector<double> wreg_h, w0_h;
    std::vector<int> slot_of_h, slot_len_h, slot_off_h;   // coordinate -> layout block; its length and offset
    std::vector<int32_t> h_ids, h_hd;   // [n * 5], [n * HW]
    std::vector<double> h_b;
    int n = 0, nfix = 0, nnoneg = 0;
    double lb = NAN, ub = NAN, loss = 0, l = 0, ww = 0;
    bool have_lb = false;
    int lb_dropped = 0, passes = 0, converged = 0;
};

namespace {

constexpr size_t kQpPruneChunkBytes = size_t(256) << 20;   // prune's scratch: at most this much (or one entry) ...
constexpr int kQpPruneChunkEntries = 256;                  // ... and at most this many entries per chunk

// the model-vector layout of a handle: every bias, deformation and filter block (offset, length), the example strides, and
// its FNV-1a fingerprint
struct QpLayout {
    int L = 0, V = 0, in_hw = 0;
    std::vector<std::pair<int, int> > blocks;
    uint64_t fp = 0;
};
QpLayout qp_layout(const pbd_handle *h)
{
    QpLayout lay;
    lay.L = (int)(h->mvec.size() / h->rs);
    lay.V = h->ex_values;
    lay.in_hw = h->ex_hdr_words;
    for (int b = 0; b < h->nbias; ++b) lay.blocks.push_back({b, 1});
    for (int d = 0; d < h->ndefs; ++d) lay.blocks.push_back({h->nbias + 4 * d, 4});
    const long long fbase = (long long)h->nbias + 4LL * h->ndefs;
    for (size_t f = 0; f < h->model_foff.size(); ++f)
        lay.blocks.push_back({(int)(fbase + h->model_foff[f]), h->model_ksize[f] * h->model_ksize[f] * 32});
    uint64_t v = 1469598103934665603ULL;
    auto mix = [&](long long x) { for (int k = 0; k < 8; ++k) { v ^= (uint64_t)((x >> (8 * k)) & 0xff); v *= 1099511628211ULL; } };
    mix(lay.L); mix(lay.V); mix(lay.in_hw); mix((long long)lay.blocks.size());
    for (auto &b : lay.blocks) { mix(b.first); mix(b.second); }
    lay.fp = v;
    return lay;
}

QpCache qp_cache(pbd_qp *q)
{
    QpCache c{};
    c.x = q->x.as<float>(); c.bm = q->bm.as<uint8_t>(); c.hd = q->hd.as<int32_t>(); c.ids = q->ids.as<int32_t>();
    c.b = q->b.as<double>(); c.d = q->d.as<double>(); c.a = q->a.as<double>(); c.sv = q->sv.as<uint8_t>();
    c.cap = q->cap; c.V = q->V; c.HW = q->HW; c.MB = q->MB;
    c.w = q->w.as<double>(); c.wreg = q->wreg.p; c.w0 = q->w0.p;
    c.noneg = q->noneg.p; c.nnoneg = q->nnoneg; c.L = q->L;
    c.slot_of = q->slot_of.p; c.slot_len = q->slot_len.p;
    return c;
}

// a header of pbd_examples' format: -1 marked invalid, 0 not a valid example for this layout, 1 valid
int qp_header_ok(const pbd_qp *q, const int32_t *h)
{
    const int nb = h[2], nv = h[3];
    if (nb == -1) return -1;
    if (nb < 0 || nb > (q->in_hw - 4) / 2 || nb > q->MB || nv < 0 || nv > q->V) return 0;
    long long tot = 0;
    for (int b = 0; b < nb; ++b) {
        const int off = h[4 + 2 * b], len = h[5 + 2 * b];
        if (off < 0 || off >= q->L) return 0;
        const int s = q->slot_of_h[off];
        if (s < 0 || q->slot_len_h[s] != len) return 0;
        tot += len;
    }
    return tot == nv ? 1 : 0;
}

// the write of m examples already on the device (p's inputs set), then the host mirror of the new entries
int qp_write(pbd_qp *q, QpWriteParams &p, bool f64, int *taken)
{
    p.c = qp_cache(q);
    p.in_hw = q->in_hw; p.in_vs = q->V; p.n0 = q->n; p.Cpos = q->Cpos; p.Cneg = q->Cneg;
    HIPCHK(q, q->work.ensure((size_t)std::max(p.m, 1) * sizeof(int)));
    p.slot = q->work.as<int>();
    p.taken = q->misc.as<int>();
    launch_qp_write(p, f64, q->stream);
    HIPCHK(q, hipGetLastError());
    int t = 0;
    HIPCHK(q, hipMemcpyAsync(&t, p.taken, sizeof(int), hipMemcpyDeviceToHost, q->stream));
    HIPCHK(q, hipStreamSynchronize(q->stream));
    if (t < 0 || t > q->cap - q->n) return fail(q, PBD_ERR_HIP, "the write reported %d entries", t);
    const int n0 = q->n, n1 = q->n + t;
    q->h_ids.resize((size_t)n1 * 5);
    q->h_hd.resize((size_t)n1 * q->HW);
    q->h_b.resize(n1);
    if (t > 0) {
        HIPCHK(q, hipMemcpyAsync(&q->h_ids[(size_t)n0 * 5], q->ids.as<int32_t>() + (size_t)n0 * 5, (size_t)t * 5 * sizeof(int32_t),
                                hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipMemcpyAsync(&q->h_hd[(size_t)n0 * q->HW], q->hd.as<int32_t>() + (size_t)n0 * q->HW,
                                (size_t)t * q->HW * sizeof(int32_t), hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipMemcpyAsync(&q->h_b[n0], q->b.as<double>() + n0, (size_t)t * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipStreamSynchronize(q->stream));
    }
    q->n = n1;
    if (taken) *taken = t;
    return PBD_OK;
}

// group numbers of the entries list[0..k) (ascending indices): equal ids share a group, groups numbered by first member
std::vector<int> qp_groups(const pbd_qp *q, const std::vector<int> &list, int *ngroups)
{
    std::map<std::array<int32_t, 5>, int> seen;
    std::vector<int> g(list.size());
    for (size_t k = 0; k < list.size(); ++k) {
        std::array<int32_t, 5> id;
        for (int c = 0; c < 5; ++c) id[c] = q->h_ids[(size_t)list[k] * 5 + c];
        auto it = seen.emplace(id, (int)seen.size()).first;
        g[k] = it->second;
    }
    *ngroups = (int)seen.size();
    return g;
}

// qp_refresh: w and l from a (lincomb's order), the clamps, lb
int qp_refresh(pbd_qp *q)
{
    // every QP call works on q->stream (created non-blocking, or the caller's): the duals are read in its order, after all
    // work queued before (prune's compaction in particular)
    std::vector<double> a(q->n);
    if (q->n) HIPCHK(q, hipMemcpyAsync(a.data(), q->a.p, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
    HIPCHK(q, hipStreamSynchronize(q->stream));
    std::vector<int> P;
    for (int i = 0; i < q->n; ++i) if (a[i] > 0) P.push_back(i);
    std::stable_sort(P.begin(), P.end(), [&](int u, int v) { return a[u] < a[v]; });
    double l = 0.0;
    for (int i : P) l = l + q->h_b[i] * a[i];
    // the entries carrying each layout block, in P's order
    const int nslots = (int)q->slot_len_h.size();
    std::vector<std::vector<int2> > per(nslots);
    for (int i : P) {
        const int32_t *h = &q->h_hd[(size_t)i * q->HW];
        for (int b = 0; b < h[0]; ++b) per[q->slot_of_h[h[2 + 3 * b]]].push_back(make_int2(i, h[4 + 3 * b]));
    }
    std::vector<QpTask> tasks;
    std::vector<int2> ent;
    for (int s = 0; s < nslots; ++s) {
        if (per[s].empty()) continue;
        const int begin = (int)ent.size();
        ent.insert(ent.end(), per[s].begin(), per[s].end());
        const int off = q->slot_off_h[s];
        for (int c0 = 0; c0 < q->slot_len_h[s]; c0 += PBD_QP_LANES)
            tasks.push_back(QpTask{off, c0, std::min(PBD_QP_LANES, q->slot_len_h[s] - c0), begin, (int)ent.size(), 0});
    }
    QpTask *d_tasks = nullptr;
    int2 *d_ent = nullptr;
    if (int rc = carve(q, q->lc, [&](Carve &c) {
            d_tasks = c.take<QpTask>(tasks.size() * sizeof(QpTask));
            d_ent = c.take<int2>(ent.size() * sizeof(int2) + 16);
        })) return rc;
    if (!tasks.empty()) {
        HIPCHK(q, hipMemcpyAsync(d_tasks, tasks.data(), tasks.size() * sizeof(QpTask), hipMemcpyHostToDevice, q->stream));
        HIPCHK(q, hipMemcpyAsync(d_ent, ent.data(), ent.size() * sizeof(int2), hipMemcpyHostToDevice, q->stream));
    }
    QpLincombParams lp{};
    lp.c = qp_cache(q);
    lp.tasks = d_tasks; lp.ntasks = (int)tasks.size();
    lp.ent = d_ent;
    lp.ww = q->misc.as<double>() + 1;
    launch_qp_lincomb(lp, q->stream);
    HIPCHK(q, hipGetLastError());
    double ww = 0;
    HIPCHK(q, hipMemcpyAsync(&ww, lp.ww, sizeof(double), hipMemcpyDeviceToHost, q->stream));
    HIPCHK(q, hipStreamSynchronize(q->stream));
    const double lb = l - ww * 0.5;
    if (q->have_lb && !(lb > q->lb - 1e-5)) q->lb_dropped = 1;
    q->l = l; q->ww = ww; q->lb = lb; q->have_lb = true;
    return PBD_OK;
}

// G = R(w . x) - b of every entry, then computeloss over the whole cache
int qp_true_loss(pbd_qp *q, double *loss)
{
    HIPCHK(q, q->work.ensure((size_t)std::max(q->n, 1) * sizeof(double)));
    QpScoreParams sp{};
    sp.c = qp_cache(q); sp.w = q->w.as<double>(); sp.first = 0; sp.count = q->n; sp.sub_b = 1; sp.scale = 1.0;
    sp.out = q->work.as<double>();
    launch_qp_score(sp, q->stream);
    HIPCHK(q, hipGetLastError());
    std::vector<double> G(q->n);
    if (q->n) HIPCHK(q, hipMemcpyAsync(G.data(), sp.out, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
    HIPCHK(q, hipStreamSynchronize(q->stream));
    std::vector<int> all(q->n);
    std::iota(all.begin(), all.end(), 0);
    int ng = 0;
    const std::vector<int> g = qp_groups(q, all, &ng);
    std::vector<double> best(ng, 0.0);   // max(0, max slack) of every group
    for (int i = 0; i < q->n; ++i) {
        const double slack = -G[i];
        if (slack > best[g[i]]) best[g[i]] = slack;
    }
    double s = 0.0;
    for (int k = 0; k < ng; ++k) if (best[k] > 0) s = s + best[k];
    *loss = s;
    return PBD_OK;
}

uint64_t qp_splitmix64(uint64_t seed, uint64_t i)
{
    const uint64_t base = seed * 0x9E3779B97F4A7C15ULL + 0x1234567ULL;
    uint64_t z = base + i * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

int qp_set_sv(pbd_qp *q, int count)
{
    if (count > 0) HIPCHK(q, hipMemsetAsync(q->sv.p, 1, (size_t)count, q->stream));
    return PBD_OK;
}

// qp_one: the pass over the support vectors, refresh, the fixed set's sv, lb and ub
int qp_one(pbd_qp *q, const int32_t *order, int norder, uint64_t seed)
{
    std::vector<double> a(q->n);
    std::vector<uint8_t> sv(q->n);
    if (q->n) {
        HIPCHK(q, hipMemcpyAsync(a.data(), q->a.p, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipMemcpyAsync(sv.data(), q->sv.p, (size_t)q->n, hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipStreamSynchronize(q->stream));
    }
    std::vector<int> S;
    for (int i = 0; i < q->n; ++i) if (sv[i]) S.push_back(i);
    const int nsv = (int)S.size();
    if (nsv == 0) return fail(q, PBD_ERR_STATE, "no support vectors (empty cache)");
    std::vector<int> perm(nsv);
    if (order) {
        if (norder != nsv) return fail(q, PBD_ERR_INVALID, "order of %d indices, %d support vectors", norder, nsv);
        std::vector<char> used(nsv, 0);
        for (int k = 0; k < nsv; ++k) {
            if (order[k] < 0 || order[k] >= nsv || used[order[k]]) return fail(q, PBD_ERR_INVALID, "order is not a permutation of 0..%d", nsv - 1);
            used[order[k]] = 1;
            perm[k] = order[k];
        }
    } else {
        std::vector<uint64_t> z(nsv);
        for (int k = 0; k < nsv; ++k) z[k] = qp_splitmix64(seed, (uint64_t)k + 1);
        std::iota(perm.begin(), perm.end(), 0);
        std::stable_sort(perm.begin(), perm.end(), [&](int u, int v) { return z[u] < z[v]; });
    }
    int ng = 0;
    const std::vector<int> gS = qp_groups(q, S, &ng);
    std::vector<double> idC(ng, 0.0);
    std::vector<int> idI(ng, -1);
    for (int k = 0; k < nsv; ++k) {
        idC[gS[k]] = idC[gS[k]] + a[S[k]];
        if (a[S[k]] > 0) idI[gS[k]] = S[k];
    }
    std::vector<int> ord(nsv), gidx(nsv);
    for (int k = 0; k < nsv; ++k) { ord[k] = S[perm[k]]; gidx[k] = gS[perm[k]]; }
    // work: order, gidx (int), idC, err (double), idI (int)
    const size_t o_ord = 0, o_g = o_ord + (size_t)nsv * 4, o_c = (o_g + (size_t)nsv * 4 + 7) / 8 * 8, o_e = o_c + (size_t)ng * 8,
                 o_i = o_e + (size_t)ng * 8, tot = o_i + (size_t)ng * 4;
    HIPCHK(q, q->work.ensure(tot + 16));
    char *wb = q->work.as<char>();
    HIPCHK(q, hipMemcpyAsync(wb + o_ord, ord.data(), (size_t)nsv * 4, hipMemcpyHostToDevice, q->stream));
    HIPCHK(q, hipMemcpyAsync(wb + o_g, gidx.data(), (size_t)nsv * 4, hipMemcpyHostToDevice, q->stream));
    HIPCHK(q, hipMemcpyAsync(wb + o_c, idC.data(), (size_t)ng * 8, hipMemcpyHostToDevice, q->stream));
    HIPCHK(q, hipMemsetAsync(wb + o_e, 0, (size_t)ng * 8, q->stream));
    HIPCHK(q, hipMemcpyAsync(wb + o_i, idI.data(), (size_t)ng * 4, hipMemcpyHostToDevice, q->stream));
    QpPassParams pp{};
    pp.c = qp_cache(q);
    pp.order = reinterpret_cast<const int *>(wb + o_ord); pp.gidx = reinterpret_cast<const int *>(wb + o_g);
    pp.nsteps = nsv; pp.ngroups = ng;
    pp.idC = reinterpret_cast<double *>(wb + o_c); pp.err = reinterpret_cast<double *>(wb + o_e);
    pp.idI = reinterpret_cast<int *>(wb + o_i);
    pp.loss = q->misc.as<double>() + 2;
    launch_qp_pass(pp, q->stream);
    HIPCHK(q, hipGetLastError());
    double loss = 0;
    HIPCHK(q, hipMemcpyAsync(&loss, pp.loss, sizeof(double), hipMemcpyDeviceToHost, q->stream));
    HIPCHK(q, hipStreamSynchronize(q->stream));
    if (int rc = qp_refresh(q)) return rc;
    if (int rc = qp_set_sv(q, q->nfix)) return rc;
    q->loss = loss;
    q->ub = q->ww * 0.5 + loss;
    return PBD_OK;
}

void qp_fill_state(const pbd_qp *q, pbd_qp_info *st, int nsv)
{
    if (!st) return;
    *st = pbd_qp_info{};
    st->n = q->n; st->nsv = nsv; st->nfix = q->nfix; st->capacity = q->cap; st->len = q->L; st->hdr_words = q->HW; st->values = q->V;
    st->lb = q->lb; st->ub = q->ub; st->loss = q->loss; st->l = q->l;
    st->lb_dropped = q->lb_dropped; st->passes = q->passes; st->converged = q->converged;
}

int qp_count_sv(pbd_qp *q, int *nsv)
{
    std::vector<uint8_t> sv(q->n);
    if (q->n) HIPCHK(q, hipMemcpyAsync(sv.data(), q->sv.p, (size_t)q->n, hipMemcpyDeviceToHost, q->stream));
    HIPCHK(q, hipStreamSynchronize(q->stream));
    int k = 0;
    for (uint8_t v : sv) k += v ? 1 : 0;
    *nsv = k;
    return PBD_OK;
}

}  // namespace

extern "C" {

int pbd_qp_create(const pbd_handle *h, const struct pbd_qp_config *cfg, pbd_qp **out)
{
    return guarded(nullptr, [&]() -> int {
        if (!h || !cfg || !out) return fail(nullptr, PBD_ERR_INVALID, "null argument");
        *out = nullptr;
        if (cfg->capacity <= 0) return fail(nullptr, PBD_ERR_INVALID, "capacity %d (at least 1)", cfg->capacity);
        const double C = cfg->C == 0 ? 0.002 : cfg->C, wpos = cfg->wpos == 0 ? 2.0 : cfg->wpos;
        if (!(C > 0) || !std::isfinite(C) || !(wpos > 0) || !std::isfinite(wpos))
            return fail(nullptr, PBD_ERR_INVALID, "C %g and wpos %g must be finite and positive", cfg->C, cfg->wpos);
        (void)hipSetDevice(h->device);
        std::unique_ptr<pbd_qp> q(new pbd_qp);
        q->device = h->device;
        const QpLayout lay = qp_layout(h);
        q->L = lay.L; q->V = lay.V; q->in_hw = lay.in_hw; q->fp = lay.fp;
        q->MB = (lay.in_hw - 4) / 2;
        q->rec_stride = ::stride(h); q->src_stream = h->stream.s;
        if (q->MB > 256 || q->MB < 1) return fail(nullptr, PBD_ERR_UNSUPPORTED, "examples of %d blocks (at most 256)", q->MB);
        if (q->V % 4) return fail(nullptr, PBD_ERR_INVALID, "example stride %d", q->V);
        q->HW = 2 + 3 * q->MB;
        q->cap = cfg->capacity;
        q->Cpos = C * wpos; q->Cneg = C;
        q->slot_of_h.assign(q->L, -1);
        for (auto &b : lay.blocks) {
            if (b.first < 0 || b.first + (long long)b.second > q->L)
                return fail(nullptr, PBD_ERR_INVALID, "layout block at %d of %d values outside w", b.first, b.second);
            if (q->slot_of_h[b.first] < 0) {
                q->slot_of_h[b.first] = (int)q->slot_len_h.size();
                q->slot_len_h.push_back(b.second);
                q->slot_off_h.push_back(b.first);
            }
        }
        // model2vec's defaults in this vector order
        q->wreg_h.assign(q->L, 1.0);
        q->w0_h.assign(q->L, 0.0);
        std::vector<int> nn;
        if (cfg->wreg) q->wreg_h.assign(cfg->wreg, cfg->wreg + q->L);
        else for (int c = 0; c < h->NC; ++c) q->wreg_h[h->biasid[h->mix_offset[h->part_offset[c]]]] = 0.01;
        if (cfg->w0) q->w0_h.assign(cfg->w0, cfg->w0 + q->L);
        else for (int d = 0; d < h->ndefs; ++d) { q->w0_h[h->nbias + 4 * d] = 0.01; q->w0_h[h->nbias + 4 * d + 2] = 0.01; }
        if (cfg->noneg) {
            if (cfg->nnoneg < 0) return fail(nullptr, PBD_ERR_INVALID, "nnoneg %d", cfg->nnoneg);
            for (int k = 0; k < cfg->nnoneg; ++k) {
                if (cfg->noneg[k] < 0 || cfg->noneg[k] >= q->L) return fail(nullptr, PBD_ERR_INVALID, "noneg index %d", cfg->noneg[k]);
                nn.push_back(cfg->noneg[k]);
            }
        } else {
            for (int d = 0; d < h->ndefs; ++d) { nn.push_back(h->nbias + 4 * d); nn.push_back(h->nbias + 4 * d + 2); }
        }
        for (int k = 0; k < q->L; ++k)
            if (!std::isfinite(q->wreg_h[k]) || q->wreg_h[k] == 0 || !std::isfinite(q->w0_h[k]))
                return fail(nullptr, PBD_ERR_INVALID, "wreg / w0 at %d: %g / %g (finite, wreg nonzero)", k, q->wreg_h[k], q->w0_h[k]);
        q->nnoneg = (int)nn.size();
        if (cfg->stream) q->stream.borrow(reinterpret_cast<hipStream_t>(cfg->stream));
        else HIPCHK(nullptr, q->stream.create());
        const size_t cap = (size_t)q->cap;
        HIPCHK(nullptr, q->x.alloc_exact(cap * q->V * sizeof(float)));
        HIPCHK(nullptr, q->bm.alloc_exact(cap * q->V));
        HIPCHK(nullptr, q->hd.alloc_exact(cap * q->HW * sizeof(int32_t)));
        HIPCHK(nullptr, q->ids.alloc_exact(cap * 5 * sizeof(int32_t)));
        HIPCHK(nullptr, q->b.alloc_exact(cap * sizeof(double)));
        HIPCHK(nullptr, q->d.alloc_exact(cap * sizeof(double)));
        HIPCHK(nullptr, q->a.alloc_exact(cap * sizeof(double)));
        HIPCHK(nullptr, q->sv.alloc_exact(cap));
        HIPCHK(nullptr, q->w.alloc_exact((size_t)q->L * sizeof(double)));
        HIPCHK(nullptr, q->wraw.alloc_exact((size_t)q->L * sizeof(double)));
        HIPCHK(nullptr, q->misc.alloc_exact(4 * sizeof(double)));
        HIPCHK(nullptr, hipMemsetAsync(q->w.p, 0, (size_t)q->L * sizeof(double), q->stream));
        HIPCHK(nullptr, hipMemsetAsync(q->a.p, 0, cap * sizeof(double), q->stream));
        HIPCHK(nullptr, hipMemsetAsync(q->sv.p, 0, cap, q->stream));
        HIPCHK(nullptr, q->wreg.upload(q->wreg_h));
        HIPCHK(nullptr, q->w0.upload(q->w0_h));
        if (!nn.empty()) HIPCHK(nullptr, q->noneg.upload(nn));
        HIPCHK(nullptr, q->slot_of.upload(q->slot_of_h));
        HIPCHK(nullptr, q->slot_len.upload(q->slot_len_h));   // DevTable uploads are blocking copies
        HIPCHK(nullptr, hipStreamSynchronize(q->stream));
        *out = q.release();
        return PBD_OK;
    });
}

void pbd_qp_destroy(pbd_qp *q)
{
    if (!q) return;
    (void)hipSetDevice(q->device);
    (void)hipStreamSynchronize(q->stream);
    delete q;
}

const char *pbd_qp_last_error(const pbd_qp *q) { return q ? q->err.c_str() : g_create_error.c_str(); }

int pbd_qp_add(pbd_qp *q, const pbd_handle *h, int n, const int32_t *hdr, const void *values, const int32_t *ids, int *taken)
{
    return entry(q, h && (n <= 0 || (hdr && values && ids)), [&]() -> int {
        if (n < 0) return fail(q, PBD_ERR_INVALID, "n %d", n);
        if (qp_layout(h).fp != q->fp) return fail(q, PBD_ERR_INVALID, "the handle's model-vector layout differs from the QP's");
        for (int e = 0; e < n; ++e)
            if (qp_header_ok(q, hdr + (size_t)e * q->in_hw) == 0)
                return fail(q, PBD_ERR_INVALID, "example %d: a block that is not a block of the model vector, or bad counts", e);
        if (taken) *taken = 0;
        if (n == 0) return PBD_OK;
        const size_t rs = h->rs;
        const size_t hb = (size_t)n * q->in_hw * 4, vb = (size_t)n * q->V * rs, ib = (size_t)n * 5 * 4;
        int32_t *d_hdr = nullptr, *d_ids = nullptr;
        char *d_values = nullptr;
        if (int rc = carve(q, q->stage, [&](Carve &c) {
                d_hdr = c.take<int32_t>(hb); d_values = c.take<char>(vb); d_ids = c.take<int32_t>(ib);
            })) return rc;
        HIPCHK(q, hipMemcpyAsync(d_hdr, hdr, hb, hipMemcpyHostToDevice, q->stream));
        HIPCHK(q, hipMemcpyAsync(d_values, values, vb, hipMemcpyHostToDevice, q->stream));
        HIPCHK(q, hipMemcpyAsync(d_ids, ids, ib, hipMemcpyHostToDevice, q->stream));
        QpWriteParams p{};
        p.in_hdr = d_hdr; p.in_values = d_values; p.in_ids = d_ids;
        p.m = n;
        return qp_write(q, p, h->f64, taken);
    });
}

int pbd_qp_add_device(pbd_qp *q, pbd_handle *h, const int32_t *d_payload, int capacity, const int32_t *d_hdr, const void *d_values,
                      int label, int id_base, int32_t *d_taken)
{
    return entry(q, h && d_payload && (capacity <= 0 || (d_hdr && d_values)), [&]() -> int {
        if (capacity < 0) return fail(q, PBD_ERR_INVALID, "capacity %d", capacity);
        if (qp_layout(h).fp != q->fp) return fail(q, PBD_ERR_INVALID, "the handle's model-vector layout differs from the QP's");
        (void)hipSetDevice(q->device);
        if (h->stream.s != q->stream.s) {   // the QP's stream waits for the handle's
            Event ev;
            HIPCHK(q, hipEventCreateWithFlags(&ev.p, hipEventDisableTiming));
            HIPCHK(q, hipEventRecord(ev.p, h->stream));
            HIPCHK(q, hipStreamWaitEvent(q->stream, ev.p, 0));
        }
        QpWriteParams p{};
        p.in_hdr = d_hdr; p.in_values = d_values; p.in_ids = nullptr;
        p.payload = d_payload; p.rec_stride = ::stride(h); p.label = label; p.id_base = id_base;
        p.m = capacity;
        p.taken_user = d_taken;
        if (capacity == 0) {
            if (d_taken) HIPCHK(q, hipMemsetAsync(d_taken, 0, sizeof(int32_t), q->stream));
            HIPCHK(q, hipStreamSynchronize(q->stream));
            return PBD_OK;
        }
        return qp_write(q, p, h->f64, nullptr);
    });
}

int pbd_qp_fix(pbd_qp *q)
{
    return entry(q, true, [&]() -> int {
        q->nfix = q->n;
        if (int rc = qp_set_sv(q, q->n)) return rc;
        HIPCHK(q, hipStreamSynchronize(q->stream));
        return PBD_OK;
    });
}

int pbd_qp_clear(pbd_qp *q)
{
    return entry(q, true, [&]() -> int {
        HIPCHK(q, hipMemsetAsync(q->a.p, 0, (size_t)q->cap * sizeof(double), q->stream));
        HIPCHK(q, hipMemsetAsync(q->sv.p, 0, (size_t)q->cap, q->stream));
        HIPCHK(q, hipStreamSynchronize(q->stream));
        q->h_ids.clear(); q->h_hd.clear(); q->h_b.clear();
        q->n = 0; q->nfix = 0;
        q->lb = NAN; q->ub = NAN; q->loss = 0; q->l = 0; q->ww = 0;
        q->have_lb = false;
        q->lb_dropped = 0; q->passes = 0; q->converged = 0;
        return PBD_OK;
    });
}

int pbd_qp_add_loss_device(pbd_qp *q, const int32_t *d_payload, int capacity, int label, double *added)
{
    return entry(q, d_payload != nullptr, [&]() -> int {
        if (capacity < 0) return fail(q, PBD_ERR_INVALID, "capacity %d", capacity);
        if (std::isnan(q->ub)) return fail(q, PBD_ERR_STATE, "no upper bound yet (pbd_qp_opt or pbd_qp_one first)");
        if (q->stream.s != q->src_stream) HIPCHK(q, hipDeviceSynchronize());   // the producer's stream is not known here
        QpHingeParams p{};
        p.payload = d_payload; p.capacity = capacity; p.rec_stride = q->rec_stride;
        p.y = label > 0 ? 1.0 : -1.0; p.Cl = label > 0 ? q->Cpos : q->Cneg;
        p.out = q->misc.as<double>() + 3;
        launch_qp_hinge(p, q->stream);
        HIPCHK(q, hipGetLastError());
        double add = 0;
        HIPCHK(q, hipMemcpyAsync(&add, p.out, sizeof(double), hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipStreamSynchronize(q->stream));
        q->ub = q->ub + add;
        if (added) *added = add;
        return PBD_OK;
    });
}

int pbd_qp_prune(pbd_qp *q, int *n)
{
    return entry(q, true, [&]() -> int {
        q->lb_dropped = 0;
        std::vector<double> a(q->n);
        std::vector<uint8_t> sv(q->n);
        if (q->n) {
            HIPCHK(q, hipMemcpyAsync(a.data(), q->a.p, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
            HIPCHK(q, hipMemcpyAsync(sv.data(), q->sv.p, (size_t)q->n, hipMemcpyDeviceToHost, q->stream));
            HIPCHK(q, hipStreamSynchronize(q->stream));
        }
        bool all = true;
        for (uint8_t v : sv) all = all && v;
        if (all) for (int i = 0; i < q->n; ++i) sv[i] = (a[i] > 0 || i < q->nfix) ? 1 : 0;
        std::vector<int> I;
        for (int i = 0; i < q->n; ++i) if (sv[i]) I.push_back(i);
        const int n1 = (int)I.size();
        if (n1 == 0) return fail(q, PBD_ERR_STATE, "nothing to keep (empty cache)");
        int first = 0;
        while (first < n1 && I[first] == first) ++first;
        // compaction in ascending chunks of at most `chunk` entries through a scratch buffer freed afterwards: a chunk's sources
        // I[k] >= k lie at or past the chunk's own start and past every earlier chunk's destinations, so each chunk reads
        // entries no earlier chunk has overwritten
        const size_t V = q->V, HW = q->HW;
        const size_t entry_bytes = V * 5 + HW * 4 + 20 + 3 * 8;
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)std::max(n1 - first, 1), kQpPruneChunkEntries),
                                                                     kQpPruneChunkBytes / entry_bytes));
        if (first < n1) {
            const size_t c = (size_t)chunk;
            QpGatherParams gp{};   // a chunk's copies in three groups, each starting 256-aligned and packed inside: x bm, hd ids, b d a
            if (int rc = carve(q, q->scratch, [&](Carve &w) {
                    gp.x = w.take<float>(c * V * 4); gp.bm = w.take<uint8_t>(c * V, 1);
                    gp.hd = w.take<int32_t>(c * HW * 4); gp.ids = w.take<int32_t>(c * 20, 1);
                    gp.b = w.take<double>(c * 8); gp.d = w.take<double>(c * 8, 1); gp.a = w.take<double>(c * 8, 1);
                }, true)) return rc;
            HIPCHK(q, q->work.ensure((size_t)(n1 - first) * sizeof(int)));
            HIPCHK(q, hipMemcpyAsync(q->work.p, &I[first], (size_t)(n1 - first) * sizeof(int), hipMemcpyHostToDevice, q->stream));
            for (int k0 = first; k0 < n1; k0 += chunk) {
                const size_t cnt = (size_t)std::min(chunk, n1 - k0), k = (size_t)k0;
                gp.c = qp_cache(q); gp.src = q->work.as<int>() + (k0 - first); gp.count = (int)cnt; gp.dst0 = k0;
                launch_qp_gather(gp, q->stream);
                HIPCHK(q, hipGetLastError());
                auto back = [&](void *dst, const void *src, size_t bytes) {
                    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, q->stream);
                };
                HIPCHK(q, back(q->x.as<float>() + k * V, gp.x, cnt * V * 4));
                HIPCHK(q, back(q->bm.as<uint8_t>() + k * V, gp.bm, cnt * V));
                HIPCHK(q, back(q->hd.as<int32_t>() + k * HW, gp.hd, cnt * HW * 4));
                HIPCHK(q, back(q->ids.as<int32_t>() + k * 5, gp.ids, cnt * 20));
                HIPCHK(q, back(q->b.as<double>() + k, gp.b, cnt * 8));
                HIPCHK(q, back(q->d.as<double>() + k, gp.d, cnt * 8));
                HIPCHK(q, back(q->a.as<double>() + k, gp.a, cnt * 8));
            }
            HIPCHK(q, hipStreamSynchronize(q->stream));
            q->scratch = DevBuf{};
        }
        int nfix = 0;
        for (int k = 0; k < n1; ++k) {
            const int i = I[k];
            if (i < q->nfix) ++nfix;
            if (k != i) {
                std::copy_n(&q->h_ids[(size_t)i * 5], 5, &q->h_ids[(size_t)k * 5]);
                std::copy_n(&q->h_hd[(size_t)i * q->HW], q->HW, &q->h_hd[(size_t)k * q->HW]);
                q->h_b[k] = q->h_b[i];
            }
        }
        q->h_ids.resize((size_t)n1 * 5); q->h_hd.resize((size_t)n1 * q->HW); q->h_b.resize(n1);
        q->n = n1; q->nfix = nfix;
        if (q->cap > n1) HIPCHK(q, hipMemsetAsync(q->sv.as<uint8_t>() + n1, 0, (size_t)(q->cap - n1), q->stream));
        if (int rc = qp_set_sv(q, n1)) return rc;
        if (int rc = qp_refresh(q)) return rc;
        if (n) *n = n1;
        return PBD_OK;
    });
}

int pbd_qp_one(pbd_qp *q, const int32_t *order, int norder, uint64_t seed, struct pbd_qp_info *state)
{
    return entry(q, true, [&]() -> int {
        q->lb_dropped = 0;
        if (int rc = qp_one(q, order, norder, seed)) return rc;
        q->passes = 1; q->converged = 0;
        int nsv = 0;
        if (int rc = qp_count_sv(q, &nsv)) return rc;
        qp_fill_state(q, state, nsv);
        return PBD_OK;
    });
}

int pbd_qp_opt(pbd_qp *q, double tol, int iter, uint64_t seed, struct pbd_qp_info *state)
{
    return entry(q, true, [&]() -> int {
        if (std::isnan(tol)) return fail(q, PBD_ERR_INVALID, "tol is NaN");
        if (iter < 0) return fail(q, PBD_ERR_INVALID, "iter %d", iter);
        if (q->n == 0) return fail(q, PBD_ERR_STATE, "empty cache");
        q->lb_dropped = 0; q->passes = 0; q->converged = 0;
        if (int rc = qp_refresh(q)) return rc;
        double loss = 0;
        if (int rc = qp_true_loss(q, &loss)) return rc;
        double ub = q->ww * 0.5 + loss;
        if (int rc = qp_set_sv(q, q->n)) return rc;
        for (int t = 0; t < iter; ++t) {
            if (int rc = qp_one(q, nullptr, 0, seed + (uint64_t)t)) return rc;
            q->passes = t + 1;
            const double lb = q->lb, ub_est = ub < q->ub ? ub : q->ub;
            if (lb > 0 && 1 - lb / ub_est < tol) {
                if (int rc = qp_true_loss(q, &loss)) return rc;
                const double u = q->ww * 0.5 + loss;
                ub = u < ub ? u : ub;
                if (1 - lb / ub < tol) { q->converged = 1; break; }
                if (int rc = qp_set_sv(q, q->n)) return rc;
            }
        }
        q->ub = ub;
        int nsv = 0;
        if (int rc = qp_count_sv(q, &nsv)) return rc;
        qp_fill_state(q, state, nsv);
        return PBD_OK;
    });
}

int pbd_qp_weights(pbd_qp *q, double *w)
{
    return entry(q, w != nullptr, [&]() -> int {
        std::vector<double> v(q->L);
        HIPCHK(q, hipMemcpyAsync(v.data(), q->w.p, (size_t)q->L * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipStreamSynchronize(q->stream));
        for (int k = 0; k < q->L; ++k) w[k] = v[k] / q->wreg_h[k] + q->w0_h[k];
        return PBD_OK;
    });
}

int pbd_qp_apply(pbd_qp *q, pbd_handle *h)
{
    return entry(q, h != nullptr, [&]() -> int {
        if (h->device != q->device) return fail(q, PBD_ERR_INVALID, "the QP lives on device %d, the handle on device %d", q->device, h->device);
        if (qp_layout(h).fp != q->fp) return fail(q, PBD_ERR_INVALID, "the handle's model-vector layout differs from the QP's");
        if (h->stream.s != q->stream.s) {   // the handle's stream waits for the QP's
            Event ev;
            HIPCHK(q, hipEventCreateWithFlags(&ev.p, hipEventDisableTiming));
            HIPCHK(q, hipEventRecord(ev.p, q->stream));
            HIPCHK(q, hipStreamWaitEvent(h->stream, ev.p, 0));
        }
        if (int rc = update_model(h, MuSource{q->w.p, q->wreg.p, q->w0.p, kMuSrcQp})) return fail(q, rc, "%s", h->err.c_str());
        return PBD_OK;
    });
}

int pbd_qp_scores(pbd_qp *q, double *s, int *n)
{
    return entry(q, s && n, [&]() -> int {
        std::vector<int> pos;
        for (int i = 0; i < q->n; ++i) if (q->h_ids[(size_t)i * 5] > 0) pos.push_back(i);
        *n = (int)pos.size();
        if (pos.empty()) return PBD_OK;
        int *d_pos = nullptr;
        double *d_out = nullptr;
        if (int rc = carve(q, q->work, [&](Carve &c) { d_pos = c.take<int>(pos.size() * 4); d_out = c.take<double>(pos.size() * 8); }))
            return rc;
        HIPCHK(q, hipMemcpyAsync(d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, q->stream));
        QpCache c = qp_cache(q);
        launch_qp_wraw(c, q->wraw.as<double>(), q->stream);
        QpScoreParams sp{};
        sp.c = c; sp.w = q->wraw.as<double>(); sp.list = d_pos; sp.count = (int)pos.size(); sp.sub_b = 0; sp.scale = q->Cpos;
        sp.out = d_out;
        launch_qp_score(sp, q->stream);
        HIPCHK(q, hipGetLastError());
        HIPCHK(q, hipMemcpyAsync(s, sp.out, pos.size() * 8, hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipStreamSynchronize(q->stream));
        return PBD_OK;
    });
}

int pbd_qp_state(pbd_qp *q, struct pbd_qp_info *state, double *a, uint8_t *sv, double *w)
{
    return entry(q, true, [&]() -> int {
        if (a && q->n) HIPCHK(q, hipMemcpyAsync(a, q->a.p, (size_t)q->n * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        if (sv && q->n) HIPCHK(q, hipMemcpyAsync(sv, q->sv.p, (size_t)q->n, hipMemcpyDeviceToHost, q->stream));
        if (w) HIPCHK(q, hipMemcpyAsync(w, q->w.p, (size_t)q->L * sizeof(double), hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipStreamSynchronize(q->stream));
        int nsv = 0;
        if (int rc = qp_count_sv(q, &nsv)) return rc;
        qp_fill_state(q, state, nsv);
        return PBD_OK;
    });
}

int pbd_qp_entries(pbd_qp *q, int first, int count, int32_t *hdr, float *values, double *b, double *d, int32_t *ids)
{
    return entry(q, true, [&]() -> int {
        if (first < 0 || count < 0 || (long long)first + count > q->n)
            return fail(q, PBD_ERR_INVALID, "entries %d..%d of %d", first, first + count - 1, q->n);
        const size_t f = first, c = count;
        if (c == 0) return PBD_OK;
        if (hdr) HIPCHK(q, hipMemcpyAsync(hdr, q->hd.as<int32_t>() + f * q->HW, c * q->HW * 4, hipMemcpyDeviceToHost, q->stream));
        if (values) HIPCHK(q, hipMemcpyAsync(values, q->x.as<float>() + f * q->V, c * q->V * 4, hipMemcpyDeviceToHost, q->stream));
        if (b) HIPCHK(q, hipMemcpyAsync(b, q->b.as<double>() + f, c * 8, hipMemcpyDeviceToHost, q->stream));
        if (d) HIPCHK(q, hipMemcpyAsync(d, q->d.as<double>() + f, c * 8, hipMemcpyDeviceToHost, q->stream));
        if (ids) HIPCHK(q, hipMemcpyAsync(ids, q->ids.as<int32_t>() + f * 5, c * 20, hipMemcpyDeviceToHost, q->stream));
        HIPCHK(q, hipStreamSynchronize(q->stream));
        return PBD_OK;
    });
}

}  // extern "C"

// ---- part types by k-means (pbd_cluster_parts*; pbd_kernels_kmeans.hip)
namespace {

constexpr long long kKmMaxPairs = 1LL << 20;

int check_cluster(pbd_handle *h, int nparts, int npos, const int32_t *parent, const int32_t *K, int trials, int max_iter, int *maxK)
{
    if (nparts < 2) return fail(h, PBD_ERR_INVALID, "nparts %d: a tree has a root and at least one child", nparts);
    if (npos < 1 || trials < 1 || max_iter < 1)
        return fail(h, PBD_ERR_INVALID, "npos %d, trials %d, max_iter %d (each at least 1)", npos, trials, max_iter);
    if ((long long)nparts * trials > kKmMaxPairs)
        return fail(h, PBD_ERR_INVALID, "%d parts x %d trials (at most %lld pairs)", nparts, trials, kKmMaxPairs);
    *maxK = 1;
    for (int p = 0; p < nparts; ++p) {
        if (K[p] < 1 || K[p] > kMaxMix) return fail(h, PBD_ERR_INVALID, "part %d: K %d (1..%d)", p, K[p], kMaxMix);
        *maxK = std::max(*maxK, (int)K[p]);
        if (p == 0 ? parent[p] != -1 : (parent[p] < 0 || parent[p] >= p))
            return fail(h, PBD_ERR_INVALID, "part %d: parent %d (part 0 is the root, -1; every other parent is in 0..part-1)", p, parent[p]);
    }
    return PBD_OK;
}

// the tables through the staging buffer, the workspace, the two kernels and the per-trial copies on the handle's stream
int enqueue_cluster(pbd_handle *h, int nparts, int npos, const double *d_def, const int32_t *parent, const int32_t *K, int trials,
                    int max_iter, uint64_t seed, int maxK, int32_t *d_idx, double *d_centres, int32_t *d_counts, int32_t *d_anchors,
                    pbd_cluster_info *d_info, double *d_sumdist_all, int32_t *d_iters_all)
{
    const size_t pairs = (size_t)nparts * trials, nstart = pairs * kMaxMix;
    static_assert(sizeof(KmPart) == 4 * sizeof(int32_t), "the staged block is one int32 array");
    std::vector<int32_t> tab(4 * (size_t)nparts + nstart);
    for (int p = 0; p < nparts; ++p) {   // the root reads its lowest-numbered child's offsets: part 1 (parent[1] is 0)
        const KmPart kp = p == 0 ? KmPart{1, 0, K[p], 1} : KmPart{p, parent[p], K[p], 0};
        memcpy(tab.data() + 4 * (size_t)p, &kp, sizeof kp);
    }
    int32_t *start = tab.data() + 4 * (size_t)nparts;
    for (size_t i = 0; i < nstart; ++i) start[i] = (int32_t)(qp_splitmix64(seed, (uint64_t)i + 1) % (uint64_t)npos);
    if (int rc = h->km_tab.stage(h, tab.data(), tab.size() * sizeof(int32_t))) return rc;
    KmParams p{};
    if (int rc = carve(h, h->km_ws, [&](Carve &c) {
            p.sumdist = c.take<double>(pairs * sizeof(double));
            p.cen = c.take<double>(pairs * kMaxMix * 2 * sizeof(double));
            p.iters = c.take<int32_t>(pairs * sizeof(int32_t));
            p.cnt = c.take<int32_t>(pairs * kMaxMix * sizeof(int32_t));
            p.lab = c.take<uint8_t>(pairs * (size_t)npos);
        })) return rc;
    p.def = d_def;
    p.parts = h->km_tab.as<KmPart>();
    p.start = h->km_tab.as<int32_t>() + 4 * (size_t)nparts;
    p.nparts = nparts; p.npos = npos; p.trials = trials; p.max_iter = max_iter;
    p.idx = d_idx; p.centres = d_centres; p.counts = d_counts; p.anchors = d_anchors; p.info = d_info;
    { ProfScope ps(h, PBD_K_KM_TRIALS, h->stream); launch_km_trials(p, maxK, h->stream); }
    { ProfScope ps(h, PBD_K_KM_PICK, h->stream); launch_km_pick(p, h->stream); }
    HIPCHK(h, hipGetLastError());
    if (d_sumdist_all) HIPCHK(h, hipMemcpyAsync(d_sumdist_all, p.sumdist, pairs * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (d_iters_all) HIPCHK(h, hipMemcpyAsync(d_iters_all, p.iters, pairs * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    return PBD_OK;
}

}  // namespace

extern "C" {

// clusterparts.m + k_means.m, and buildmodel.m's anchors.  See include/pbd.h.
int pbd_cluster_parts(pbd_handle *h, int nparts, int npos, const double *def, const int32_t *parent, const int32_t *K, int trials,
                      int max_iter, uint64_t seed, int32_t *idx, double *centres, int32_t *counts, int32_t *anchors,
                      struct pbd_cluster_info *info, double *sumdist_all, int32_t *iters_all)
{
    return entry(h, def && parent && K && idx && centres && counts && anchors && info, kIdle, [&]() -> int {
        int maxK;
        if (int rc = check_cluster(h, nparts, npos, parent, K, trials, max_iter, &maxK)) return rc;
        const size_t np = (size_t)nparts, pairs = np * trials, def_bytes = np * npos * 2 * sizeof(double);
        HIPCHK(h, h->km_in.ensure(def_bytes));
        int32_t *d_idx, *d_counts, *d_anchors, *d_its;
        double *d_centres, *d_sd;
        pbd_cluster_info *d_info;
        if (int rc = carve(h, h->km_out, [&](Carve &c) {
                d_centres = c.take<double>(np * kMaxMix * 2 * sizeof(double));
                d_sd = c.take<double>(pairs * sizeof(double));
                d_info = c.take<pbd_cluster_info>(np * sizeof(pbd_cluster_info));
                d_idx = c.take<int32_t>(np * npos * sizeof(int32_t));
                d_counts = c.take<int32_t>(np * kMaxMix * sizeof(int32_t));
                d_anchors = c.take<int32_t>(np * kMaxMix * 2 * sizeof(int32_t));
                d_its = c.take<int32_t>(pairs * sizeof(int32_t));
            })) return rc;
        HIPCHK(h, hipMemcpyAsync(h->km_in.p, def, def_bytes, hipMemcpyHostToDevice, h->stream));
        if (int rc = enqueue_cluster(h, nparts, npos, h->km_in.as<double>(), parent, K, trials, max_iter, seed, maxK, d_idx, d_centres,
                                     d_counts, d_anchors, d_info, sumdist_all ? d_sd : nullptr, iters_all ? d_its : nullptr)) return rc;
        HIPCHK(h, hipMemcpyAsync(idx, d_idx, np * npos * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(centres, d_centres, np * kMaxMix * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(counts, d_counts, np * kMaxMix * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(anchors, d_anchors, np * kMaxMix * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(info, d_info, np * sizeof(pbd_cluster_info), hipMemcpyDeviceToHost, h->stream));
        if (sumdist_all) HIPCHK(h, hipMemcpyAsync(sumdist_all, d_sd, pairs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (iters_all) HIPCHK(h, hipMemcpyAsync(iters_all, d_its, pairs * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_cluster_parts_device(pbd_handle *h, int nparts, int npos, const double *d_def, const int32_t *parent, const int32_t *K,
                             int trials, int max_iter, uint64_t seed, int32_t *d_idx, double *d_centres, int32_t *d_counts,
                             int32_t *d_anchors, struct pbd_cluster_info *d_info, double *d_sumdist_all, int32_t *d_iters_all)
{
    return entry(h, d_def && parent && K && d_idx && d_centres && d_counts && d_anchors && d_info, kIdle, [&]() -> int {
        int maxK;
        if (int rc = check_cluster(h, nparts, npos, parent, K, trials, max_iter, &maxK)) return rc;
        return enqueue_cluster(h, nparts, npos, d_def, parent, K, trials, max_iter, seed, maxK, d_idx, d_centres, d_counts, d_anchors,
                               d_info, d_sumdist_all, d_iters_all);
    });
}

}  // extern "C"
