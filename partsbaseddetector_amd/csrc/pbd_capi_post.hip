// pbd_capi_post.hip -- the C entry points that work on a finished candidate list (include/pbd.h): 3-D boxes, depth consistency,
// suppression of a caller's list, camera boxes, candidate masks, part poses, object clusters, plane removal, and testing a model
// (part NMS, best overlap, PCK, APK).
// The handle and the layer they are written on: pbd_handle.h.
#include "pbd_handle.h"

using namespace pbd;

namespace {

// ---- 3-D boxes from a depth image (pbd_boxes3d*; pbd_kernels_depth.hip)
// the derivative-of-Gaussian taps of Candidate::boundingBox3D (include/Candidate.hpp:190-193), once, with the C library's exp:
//   g = getGaussianKernel(35, 4, CV_32F): t_i = exp(scale2X * x_i * x_i), x_i = i - 17, scale2X = -0.5 / 16; cf_i = (float)t_i,
//       sum += cf_i in double, then cf_i = (float)(cf_i * (1. / sum))
//   dog = filter2D(g, -1, [-1 0 1]^T): correlation, BORDER_REFLECT_101, s = 0; s += k * x per non-zero tap, in float
const float *boxes3d_taps()
{
    static const struct Taps {
        float v[kB3Taps];
        Taps()
        {
            float g[kB3Taps];
            const double scale2X = -0.5 / (4.0 * 4.0);
            double sum = 0;
            for (int i = 0; i < kB3Taps; ++i) {
                const double x = i - (kB3Taps - 1) * 0.5;
                g[i] = (float)exp(scale2X * x * x);
                sum += g[i];
            }
            sum = 1. / sum;
            for (int i = 0; i < kB3Taps; ++i) g[i] = (float)(g[i] * sum);
            for (int i = 0; i < kB3Taps; ++i) {
                const int a = i == 0 ? 1 : i - 1, b = i == kB3Taps - 1 ? kB3Taps - 2 : i + 1;
                float s = 0.f;
                s = s + -1.f * g[a];
                s = s + 1.f * g[b];
                v[i] = s;
            }
        }
    } taps;
    return taps.v;
}

// every check of a call's depth images before anything is enqueued (pbd_boxes3d*, pbd_boxes3d_camera*, pbd_depth_consistency*).
// With colour-frame sizes (im_rows / im_cols), the boxes of a record lie inside the depth image and their samples, overlaps
// counted, fit an int; without them, rows * cols does.
int check_depth_frames(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, bool host, const int *im_rows = nullptr,
                       const int *im_cols = nullptr, const float *zfactor = nullptr)
{
    if (nframes < 1) return fail(h, PBD_ERR_INVALID, "nframes %d", nframes);
    if (!depth_size(depth_code))
        return fail(h, PBD_ERR_INVALID, "depth code %d: 0 (8U), 2 (16U), 5 (32F) or 6 (64F)", depth_code);
    if (zfactor && std::isnan(*zfactor)) return fail(h, PBD_ERR_INVALID, "zfactor is NaN");   // pbd_depth_consistency*
    const size_t es = depth_size(depth_code);
    const unsigned long long per_pixel = im_rows ? kB3MaxBoxes : 1;
    for (int f = 0; f < nframes; ++f) {
        const pbd_frame &d = depth[f];
        if (!d.data || d.rows < 1 || d.cols < 1) return fail(h, PBD_ERR_INVALID, "frame %d: depth %dx%d at %p", f, d.rows, d.cols, d.data);
        if (im_rows && (im_rows[f] < 1 || im_cols[f] < 1))
            return fail(h, PBD_ERR_INVALID, "frame %d: colour frame %dx%d", f, im_rows[f], im_cols[f]);
        if (per_pixel * (unsigned long long)d.rows * (unsigned long long)d.cols >= (1ull << 31))
            return fail(h, PBD_ERR_INVALID, "frame %d: depth image %dx%d too large", f, d.rows, d.cols);
        if (d.stride_bytes < (size_t)d.cols * es)
            return fail(h, PBD_ERR_INVALID, "frame %d: stride %zu < row bytes %zu", f, d.stride_bytes, (size_t)d.cols * es);
        if (!host && (reinterpret_cast<uintptr_t>(d.data) % es || d.stride_bytes % es))
            return fail(h, PBD_ERR_INVALID, "frame %d: device pointer %p / stride %zu not a multiple of the %zu-byte element", f, d.data,
                        d.stride_bytes, es);
    }
    return PBD_OK;
}

// the kernels' frame table of depth images already on the device (colour-frame sizes 0 where the stage has none)
std::vector<Box3dFrame> depth_table(int nframes, const pbd_frame *d_depth, const int *im_rows = nullptr, const int *im_cols = nullptr)
{
    std::vector<Box3dFrame> tab(nframes);
    for (int f = 0; f < nframes; ++f)
        tab[f] = Box3dFrame{static_cast<const uint8_t *>(d_depth[f].data), d_depth[f].rows, d_depth[f].cols,
                            (long long)d_depth[f].stride_bytes, im_rows ? im_rows[f] : 0, im_cols ? im_cols[f] : 0};
    return tab;
}

// the frame table to the device (through the pinned staging buffer) and the kernel, on the handle's stream
int enqueue_boxes3d(pbd_handle *h, const std::vector<Box3dFrame> &tab, int depth_code, const int32_t *d_payload, int capacity,
                    int frame_offset, double *d_out)
{
    if (int rc = h->b3_tab.stage(h, tab.data(), tab.size() * sizeof(Box3dFrame))) return rc;
    Boxes3dParams bp{};
    bp.in = d_payload; bp.in_cap = capacity;
    bp.stride = stride(h); bp.max_parts = h->max_parts;
    bp.frames = h->b3_tab.as<Box3dFrame>(); bp.nframes = (int)tab.size(); bp.frame_offset = frame_offset;
    bp.depth = depth_code; bp.out = d_out;
    memcpy(bp.dog, boxes3d_taps(), sizeof bp.dog);
    launch_boxes3d(bp, capacity, h->stream);
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// the host records of a call: the frame index of each inside 0..nframes-1 and its part count in range, plus what `what` asks for
enum RecordRule {
    kRecPlain = 0,
    kRecAscending = 1,    // frames non-decreasing (pbd_suppress, pbd_candidate_mask)
    kRecComponent = 2     // a component of the model, with exactly its part count (pbd_depth_consistency)
};
int check_records(pbd_handle *h, int nframes, const int32_t *cand, int ncand, int frame_offset, RecordRule what)
{
    const int stride = ::stride(h);
    long long prev = 0;
    for (int i = 0; i < ncand; ++i) {
        const int32_t *r = cand + (size_t)i * stride;
        const long long f = (long long)r[0] - frame_offset;
        if (f < 0 || f >= nframes || (what == kRecAscending && f < prev))
            return fail(h, PBD_ERR_INVALID, "record %d: frame %d - frame_offset %d outside 0..%d%s", i, r[0], frame_offset, nframes - 1,
                        what == kRecAscending ? " or below the previous record's" : "");
        prev = f;
        if (what == kRecComponent) {
            if (r[1] < 0 || r[1] >= h->NC) return fail(h, PBD_ERR_INVALID, "record %d: component %d (0..%d)", i, r[1], h->NC - 1);
            const int np = h->part_offset[r[1] + 1] - h->part_offset[r[1]];
            if (r[6] != np) return fail(h, PBD_ERR_INVALID, "record %d: nparts %d (component %d has %d)", i, r[6], r[1], np);
        }
        if (r[6] < 1 || r[6] > h->max_parts) return fail(h, PBD_ERR_INVALID, "record %d: nparts %d (1..%d)", i, r[6], h->max_parts);
    }
    return PBD_OK;
}

// the host forms' depth images into the handle's own buffer, packed with dense rows; tab = their frame table
int upload_depth_host(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, const int *im_rows, const int *im_cols,
                      std::vector<Box3dFrame> &tab)
{
    const size_t es = depth_size(depth_code);
    size_t total = 0;
    for (int f = 0; f < nframes; ++f) total += (size_t)depth[f].rows * depth[f].cols * es;
    HIPCHK(h, h->b3_depth.ensure(total + 8));
    std::vector<pbd_frame> packed(nframes);
    size_t off = 0;
    for (int f = 0; f < nframes; ++f) {
        const size_t row_bytes = (size_t)depth[f].cols * es;
        uint8_t *dst = h->b3_depth.as<uint8_t>() + off;
        HIPCHK(h, hipMemcpy2DAsync(dst, row_bytes, depth[f].data, depth[f].stride_bytes, row_bytes, depth[f].rows,
                                   hipMemcpyHostToDevice, h->stream));
        packed[f] = pbd_frame{dst, depth[f].rows, depth[f].cols, row_bytes};
        off += row_bytes * depth[f].rows;
    }
    tab = depth_table(nframes, packed.data(), im_rows, im_cols);
    return PBD_OK;
}

// the same, and the records as a payload (word 0 = ncand)
int upload_boxes3d_host(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, const int *im_rows, const int *im_cols,
                        const int32_t *cand, int ncand, std::vector<Box3dFrame> &tab)
{
    const int stride = ::stride(h);
    HIPCHK(h, h->b3_rec.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
    if (int rc = upload_depth_host(h, nframes, depth, depth_code, im_rows, im_cols, tab)) return rc;
    HIPCHK(h, hipMemcpyAsync(h->b3_rec.p, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->b3_rec.as<int32_t>() + 1, cand, (size_t)ncand * stride * sizeof(int32_t), hipMemcpyHostToDevice,
                             h->stream));
    return PBD_OK;
}

// ---- depth consistency (pbd_depth_consistency*; pbd_kernels_consistency.hip)
// the model's tables the decision reads, uploaded on first use: part offsets, component-local parents, and per part the norm of
// its mixture-0 anchor, std::sqrt((double)ax*ax + (double)ay*ay) (part.anchor(0): src/SearchSpacePruning.cpp:83)
int dc_model_tables(pbd_handle *h)
{
    if (h->dc_norm.p) return PBD_OK;
    const int totparts = (int)h->parentid.size();
    std::vector<double> norm(std::max(totparts, 1), 0.0);
    for (int c = 0; c < h->NC; ++c)
        for (int gp = h->part_offset[c] + 1; gp < h->part_offset[c + 1]; ++gp) {
            const int d = h->defid[h->mix_offset[gp]];
            if (d < 0 || 2 * (size_t)d + 1 >= h->anchors.size()) continue;
            const double ax = h->anchors[2 * (size_t)d], ay = h->anchors[2 * (size_t)d + 1];
            norm[gp] = std::sqrt(ax * ax + ay * ay);
        }
    HIPCHK(h, h->dc_part_offset.upload(h->part_offset));
    HIPCHK(h, h->dc_parent.upload(h->parentid));
    HIPCHK(h, h->dc_norm.upload(norm));
    return PBD_OK;
}

// the frame table and the filter's kernels on the handle's stream: payload d_in (capacity records) -> d_out (out_cap records)
int enqueue_dc(pbd_handle *h, const std::vector<Box3dFrame> &tab, int depth_code, float zfactor, const int32_t *d_in, int capacity,
               int frame_offset, int32_t *d_out, int out_cap)
{
    if (int rc = dc_model_tables(h)) return rc;
    const int cap = std::max(capacity, 0);
    const long long tasks = std::max<long long>((long long)cap * h->max_parts, 1);
    if (tasks >= (1LL << 30)) return fail(h, PBD_ERR_INVALID, "capacity %d: %lld parts (below 2^30)", capacity, tasks);
    const int blocks = dc_record_blocks(cap);
    DcParams p{};
    if (int rc = carve(h, h->dc_ws, [&](Carve &c) {
            p.med = c.take<double>(tasks * sizeof(double));
            p.queue = c.take<int>(tasks * sizeof(int));
            p.qn = c.take<int>(256);
            p.flag = c.take<int>((size_t)blocks * 256 * sizeof(int));
            p.blk = c.take<int>((size_t)blocks * sizeof(int));
        })) return rc;
    if (int rc = h->dc_tab.stage(h, tab.data(), tab.size() * sizeof(Box3dFrame))) return rc;
    p.in = d_in; p.in_cap = cap; p.stride = stride(h); p.max_parts = h->max_parts;
    p.frames = h->dc_tab.as<Box3dFrame>(); p.nframes = (int)tab.size(); p.frame_offset = frame_offset;
    p.depth = depth_code; p.NC = h->NC;
    p.part_offset = h->dc_part_offset.p; p.parent = h->dc_parent.p; p.norm = h->dc_norm.p; p.zfactor = zfactor;
    p.task_cap = tasks;
    p.out = d_out; p.out_cap = std::max(out_cap, 0);
    HIPCHK(h, hipMemsetAsync(p.qn, 0, 8 * sizeof(int), h->stream));
    static const int ids[kDcSteps] = {PBD_K_DC_CLASSIFY, PBD_K_DC_SELECT, PBD_K_DC_COMPACT};
    for (int step = 0; step < kDcSteps; ++step) {
        ProfScope ps(h, ids[step], h->stream);
        launch_depth_consistency(p, h->f64, step, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- scale-depth pruning of a caller's list (pbd_depth_prune*; pbd_kernels_depthprune.hip)
// the frame table, the decision per record and the depth-consistency filter's compaction on the handle's stream: payload d_in
// (capacity records) -> d_out (out_cap records)
int enqueue_depth_prune(pbd_handle *h, const std::vector<Box3dFrame> &tab, int depth_code, const DepthPruneRule &rule,
                        const int32_t *d_in, int capacity, int frame_offset, int32_t *d_out, int out_cap)
{
    const int cap = std::max(capacity, 0), blocks = dc_record_blocks(cap);
    DcParams p{};
    if (int rc = carve(h, h->dpl_ws, [&](Carve &c) {
            p.flag = c.take<int>((size_t)blocks * 256 * sizeof(int));
            p.blk = c.take<int>((size_t)blocks * sizeof(int));
        })) return rc;
    if (int rc = h->dpl_tab.stage(h, tab.data(), tab.size() * sizeof(Box3dFrame))) return rc;
    p.in = d_in; p.in_cap = cap; p.stride = stride(h); p.max_parts = h->max_parts;
    p.frames = h->dpl_tab.as<Box3dFrame>(); p.nframes = (int)tab.size(); p.frame_offset = frame_offset;
    p.depth = depth_code;
    p.out = d_out; p.out_cap = std::max(out_cap, 0);
    {
        ProfScope ps(h, PBD_K_DEPTH_PRUNE, h->stream);
        launch_depth_prune_records(p, rule, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- grid maxima of a caller's planes (pbd_grid_nms*; pbd_kernels_gridnms.hip)
// every check of a call; *total = the elements of all planes
int check_grid_nms(pbd_handle *h, int nplanes, const int *rows, const int *cols, int real_code, const void *src, const void *dst,
                   int sz, long long *total)
{
    if (nplanes < 0) return fail(h, PBD_ERR_INVALID, "nplanes %d", nplanes);
    if (nplanes > 0 && (!rows || !cols || !src || !dst))
        return fail(h, PBD_ERR_INVALID, "a null pointer: rows %p, cols %p, src %p, dst %p", (const void *)rows, (const void *)cols, src, dst);
    if (sz < 0 || sz > 32767) return fail(h, PBD_ERR_INVALID, "window size %d (0..32767)", sz);
    if (real_code != PBD_REAL_F32 && real_code != PBD_REAL_F64)
        return fail(h, PBD_ERR_INVALID, "real_code %d: PBD_REAL_F32 or PBD_REAL_F64", real_code);
    *total = 0;
    for (int i = 0; i < nplanes; ++i) {
        if (rows[i] < 0 || cols[i] < 0) return fail(h, PBD_ERR_INVALID, "plane %d: size %dx%d", i, rows[i], cols[i]);
        *total += (long long)rows[i] * cols[i];
    }
    return PBD_OK;
}

// the plane table to the device and the kernel, on the handle's stream
int enqueue_grid_nms(pbd_handle *h, int nplanes, const int *rows, const int *cols, int real_code, const void *d_src,
                     const uint8_t *d_mask, int sz, uint8_t *d_dst)
{
    std::vector<GnPlane> tab(nplanes);
    long long off = 0, blocks = 0;
    for (int i = 0; i < nplanes; ++i) {
        tab[i] = grid_nms_plane(off, rows[i], cols[i], sz, &blocks);
        off += (long long)rows[i] * cols[i];
    }
    if (blocks == 0) return PBD_OK;
    if (int rc = h->gn_tab.stage(h, tab.data(), tab.size() * sizeof(GnPlane))) return rc;
    GridNmsParams gp{};
    gp.planes = h->gn_tab.as<GnPlane>(); gp.nplanes = nplanes; gp.nframes = 1;
    gp.frame_stride = off; gp.blocks_per_frame = blocks;
    gp.src = d_src; gp.mask = d_mask; gp.sz = sz; gp.dst = d_dst;
    {
        ProfScope ps(h, PBD_K_GRID_NMS, h->stream);
        launch_grid_nms(gp, real_code == PBD_REAL_F64, grid_nms_lanes(sz, h->gn_lanes), h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- the K best elements of a caller's segments (pbd_top_k_cells*; pbd_kernels_topk.hip)
// every check of a call; *total = the elements of all segments
int check_top_k_cells(pbd_handle *h, int nseg, const long long *len, int real_code, const void *src, const void *dst, int k,
                      long long *total)
{
    if (nseg < 0 || k < 0) return fail(h, PBD_ERR_INVALID, "nseg %d, k %d", nseg, k);
    if (real_code != PBD_REAL_F32 && real_code != PBD_REAL_F64)
        return fail(h, PBD_ERR_INVALID, "real_code %d: PBD_REAL_F32 or PBD_REAL_F64", real_code);
    if (nseg > 0 && !len) return fail(h, PBD_ERR_INVALID, "a null pointer: len");
    *total = 0;
    for (int i = 0; i < nseg; ++i) {
        if (len[i] < 0) return fail(h, PBD_ERR_INVALID, "segment %d: length %lld", i, len[i]);
        *total += len[i];
        if (*total > INT_MAX) return fail(h, PBD_ERR_INVALID, "more than 2^31 - 1 elements up to segment %d", i);
    }
    if (*total > 0 && (!src || !dst)) return fail(h, PBD_ERR_INVALID, "a null pointer: src %p, dst %p", src, dst);
    return PBD_OK;
}

// the segment table to the device and the selection's kernels, on the handle's stream
int enqueue_top_k_cells(pbd_handle *h, int nseg, const long long *len, int real_code, const void *d_src, const uint8_t *d_mask,
                        int k, uint8_t *d_dst)
{
    std::vector<TopKTab> tab(nseg + 1);
    long long off = 0, tiles = 0;
    for (int i = 0; i < nseg; ++i) {
        tab[i] = TopKTab{off, tiles};
        off += len[i]; tiles += top_k_tiles(len[i]);
    }
    tab[nseg] = TopKTab{off, tiles};
    if (int rc = h->tk_tab.stage(h, tab.data(), tab.size() * sizeof(TopKTab))) return rc;
    TopKParams tp{};
    tp.tab = h->tk_tab.as<TopKTab>(); tp.nseg = nseg; tp.k = k; tp.ntiles = tiles;
    tp.src = d_src; tp.mask = d_mask; tp.dst = d_dst;
    if (int rc = top_k_workspace(h, tp, h->stream)) return rc;
    {
        ProfScope ps(h, PBD_K_TOP_K, h->stream);
        launch_top_k(tp, real_code == PBD_REAL_F64, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- the K best records of every frame of a caller's list (pbd_top_k*)
int check_top_k_list(pbd_handle *h, int nframes, int k)
{
    if (nframes < 1) return fail(h, PBD_ERR_INVALID, "nframes %d", nframes);
    if (k < 0) return fail(h, PBD_ERR_INVALID, "k %d", k);
    return PBD_OK;
}

// the rank of every record and the depth-consistency filter's compaction on the handle's stream: payload d_in (capacity records)
// -> d_out (out_cap records)
int enqueue_top_k_list(pbd_handle *h, int nframes, int k, const int32_t *d_in, int capacity, int frame_offset, int32_t *d_out,
                       int out_cap)
{
    const int cap = std::max(capacity, 0), blocks = dc_record_blocks(cap);
    DcParams p{};
    if (int rc = carve(h, h->tkl_ws, [&](Carve &c) {
            p.flag = c.take<int>((size_t)blocks * 256 * sizeof(int));
            p.blk = c.take<int>((size_t)blocks * sizeof(int));
        })) return rc;
    p.in = d_in; p.in_cap = cap; p.stride = stride(h); p.max_parts = h->max_parts;
    p.nframes = nframes; p.frame_offset = frame_offset;
    p.out = d_out; p.out_cap = std::max(out_cap, 0);
    {
        ProfScope ps(h, PBD_K_TOP_K, h->stream);
        launch_top_k_records(p, k, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- scale NMS of a caller's list (pbd_scale_nms*; pbd_kernels_scalenms.hip)
int check_scale_nms_list(pbd_handle *h, int nframes, int dl)
{
    if (nframes < 1) return fail(h, PBD_ERR_INVALID, "nframes %d", nframes);
    if (dl < 0 || dl > 255) return fail(h, PBD_ERR_INVALID, "scale NMS level distance %d (0..255)", dl);
    return PBD_OK;
}

// the kept flag of every record and the depth-consistency filter's compaction on the handle's stream: payload d_in (capacity
// records) -> d_out (out_cap records)
int enqueue_scale_nms_list(pbd_handle *h, int nframes, int dl, const int32_t *d_in, int capacity, int frame_offset, int32_t *d_out,
                           int out_cap)
{
    const int cap = std::max(capacity, 0), blocks = dc_record_blocks(cap);
    DcParams p{};
    if (int rc = carve(h, h->snl_ws, [&](Carve &c) {
            p.flag = c.take<int>((size_t)blocks * 256 * sizeof(int));
            p.blk = c.take<int>((size_t)blocks * sizeof(int));
        })) return rc;
    p.in = d_in; p.in_cap = cap; p.stride = stride(h); p.max_parts = h->max_parts;
    p.nframes = nframes; p.frame_offset = frame_offset;
    p.out = d_out; p.out_cap = std::max(out_cap, 0);
    {
        ProfScope ps(h, PBD_K_SCALE_NMS, h->stream);
        launch_scale_nms_records(p, dl, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- suppression of a caller's list (pbd_suppress*): the canvas tables of its frame sizes, kept for the next call of the
// same sizes
int get_suppress_plan(pbd_handle *h, int nframes, const int *rows, const int *cols, Plan **out)
{
    if (nframes < 1) return fail(h, PBD_ERR_INVALID, "nframes %d", nframes);
    std::vector<int> key;
    for (int f = 0; f < nframes; ++f) {
        if (rows[f] < 1 || cols[f] < 1 || rows[f] > 65536 || cols[f] > 65536)
            return fail(h, PBD_ERR_INVALID, "frame %d: size %dx%d (1..65536)", f, rows[f], cols[f]);
        key.push_back(rows[f]); key.push_back(cols[f]);
    }
    if (h->sup_plan && h->sup_plan->key_dims == key) { *out = h->sup_plan.get(); return PBD_OK; }
    if (h->sup_plan) HIPCHK(h, hipStreamSynchronize(h->stream));   // the previous tables may still be read
    auto M = std::make_unique<Plan>();
    M->kind = 4; M->key_dims = key; M->mixed_frames = nframes;
    for (int f = 0; f < nframes; ++f) M->fdim.push_back(make_int2(rows[f], cols[f]));
    post_canvas_plan(*M);
    h->sup_plan.reset();
    HIPCHK(h, M->d_fdim.upload(M->fdim));
    HIPCHK(h, M->d_fcanvas.upload(M->fcanvas));
    HIPCHK(h, M->d_post_lds.upload(M->post_lds));
    HIPCHK(h, M->d_post_glb.upload(M->post_glb));
    h->sup_plan = std::move(M);
    *out = h->sup_plan.get();
    return PBD_OK;
}

// the host forms: records into a payload of the handle's (word 0 = ncand), then, after `run` enqueued the stage into `dout`,
// the kept count and min(kept, capacity) records back into out
template <class Run>
int host_list_call(pbd_handle *h, DevBuf &din, DevBuf &dout, const int32_t *cand, int ncand, int32_t *out, int capacity, int *nout,
                   Run run)
{
    const size_t stride = (size_t)::stride(h);
    HIPCHK(h, din.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
    HIPCHK(h, dout.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
    HIPCHK(h, hipMemcpyAsync(din.p, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (ncand) HIPCHK(h, hipMemcpyAsync(din.as<int32_t>() + 1, cand, (size_t)ncand * stride * sizeof(int32_t), hipMemcpyHostToDevice,
                                        h->stream));
    if (int rc = run(din.as<int32_t>(), dout.as<int32_t>())) return rc;
    int kept = 0;
    HIPCHK(h, hipMemcpyAsync(&kept, dout.p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    const int nret = std::min(std::max(kept, 0), capacity);
    if (nret > 0)
        HIPCHK(h, hipMemcpy(out, dout.as<int32_t>() + 1, (size_t)nret * stride * sizeof(int32_t), hipMemcpyDeviceToHost));
    *nout = kept;
    if (kept > capacity) return fail(h, PBD_ERR_CAPACITY, "%d records kept, capacity %d", kept, capacity);
    return PBD_OK;
}

// ---- camera boxes and part centres (pbd_boxes3d_camera*; pbd_kernels_cloud.hip)
int check_camera(pbd_handle *h, int nframes, int depth_code, const pbd_pinhole *cams, int parts_mode)
{
    if (depth_code != kDepth32F) return fail(h, PBD_ERR_UNSUPPORTED, "depth code %d: the part centres read 32F depth (5)", depth_code);
    if (parts_mode != PBD_PARTS_LITERAL && parts_mode != PBD_PARTS_XY)
        return fail(h, PBD_ERR_INVALID, "parts mode %d: PBD_PARTS_LITERAL (0) or PBD_PARTS_XY (1)", parts_mode);
    for (int f = 0; f < nframes; ++f)
        if (!std::isfinite(cams[f].fx) || !std::isfinite(cams[f].fy) || cams[f].fx == 0 || cams[f].fy == 0)
            return fail(h, PBD_ERR_INVALID, "frame %d: fx %g, fy %g (finite, non-zero)", f, cams[f].fx, cams[f].fy);
    return PBD_OK;
}

// k_boxes3d into the handle's cube buffer, then the camera kernel, on the handle's stream
int enqueue_camera(pbd_handle *h, const std::vector<Box3dFrame> &tab, int depth_code, const pbd_pinhole *cams, int parts_mode,
                   const int32_t *d_payload, int capacity, int frame_offset, double *d_box, float *d_centres, int32_t *d_ncentres,
                   int32_t *d_dense)
{
    static_assert(sizeof(pbd_pinhole) == sizeof(Pinhole), "pbd_pinhole is the kernels' Pinhole");
    HIPCHK(h, h->cam_cube.ensure((size_t)capacity * 6 * sizeof(double)));
    if (int rc = enqueue_boxes3d(h, tab, depth_code, d_payload, capacity, frame_offset, h->cam_cube.as<double>())) return rc;
    if (int rc = h->cam_tab.stage(h, cams, tab.size() * sizeof(Pinhole))) return rc;
    CameraParams cp{};
    cp.in = d_payload; cp.in_cap = capacity; cp.stride = stride(h); cp.max_parts = h->max_parts;
    cp.frames = h->b3_tab.as<Box3dFrame>(); cp.cams = h->cam_tab.as<Pinhole>();
    cp.nframes = (int)tab.size(); cp.frame_offset = frame_offset; cp.mode = parts_mode;
    cp.cube = h->cam_cube.as<double>();
    cp.box = d_box; cp.centres = d_centres; cp.ncentres = d_ncentres; cp.dense = d_dense;
    {
        ProfScope ps(h, PBD_K_CAMERA_BOXES, h->stream);
        launch_camera_boxes(cp, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- candidate mask (pbd_candidate_mask*; pbd_kernels_publish.hip)
// every check of a call's frames before anything is enqueued
int check_mask_frames(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, uint8_t *const *labels, const size_t *label_pitch,
                      int channels, const uint8_t *const *colour, const size_t *colour_pitch, uint8_t *const *masked,
                      const size_t *masked_pitch)
{
    if (nframes < 1) return fail(h, PBD_ERR_INVALID, "nframes %d", nframes);
    if (masked && channels != 1 && channels != 3 && channels != 4)
        return fail(h, PBD_ERR_INVALID, "channels %d: 1, 3 or 4", channels);
    if ((labels && !label_pitch) || (masked && (!masked_pitch || !colour || !colour_pitch)))
        return fail(h, PBD_ERR_INVALID, "an output without its pitches or colour frames");
    for (int f = 0; f < nframes; ++f) {
        if (im_rows[f] < 1 || im_cols[f] < 1 || im_rows[f] > 65536 || im_cols[f] > 65536)
            return fail(h, PBD_ERR_INVALID, "frame %d: size %dx%d (1..65536)", f, im_rows[f], im_cols[f]);
        const size_t row = (size_t)im_cols[f];
        if (labels && (!labels[f] || label_pitch[f] < row))
            return fail(h, PBD_ERR_INVALID, "frame %d: labels %p, pitch %zu < row bytes %zu", f, (const void *)labels[f], label_pitch[f], row);
        if (masked && (!masked[f] || !colour[f] || colour_pitch[f] < row * channels || masked_pitch[f] < row * channels))
            return fail(h, PBD_ERR_INVALID, "frame %d: colour %p / masked %p, pitches %zu / %zu < row bytes %zu", f,
                        (const void *)colour[f], (const void *)masked[f], colour_pitch[f], masked_pitch[f], row * channels);
    }
    return PBD_OK;
}

// the frame table (tile numbering filled in) to the device, then the hull and the tile kernels, on the handle's stream
int enqueue_mask(pbd_handle *h, std::vector<MaskFrame> &tab, int channels, const int32_t *d_payload, int capacity, int frame_offset,
                 int32_t *d_status)
{
    long long tiles = 0;
    for (MaskFrame &fr : tab) {
        fr.tile0 = (int)tiles;
        tiles += mask_tiles(fr.rows, fr.cols);
        if (tiles > 0x7fffffffll) return fail(h, PBD_ERR_INVALID, "%zu frames: 2^31 or more pixel tiles", tab.size());
    }
    if (int rc = h->mk_tab.stage(h, tab.data(), tab.size() * sizeof(MaskFrame))) return rc;
    MaskParams mp{};
    if (int rc = carve(h, h->mk_ws, [&](Carve &c) {
            mp.hull = c.take<int4>((size_t)capacity * sizeof(int4));
            mp.range = c.take<int32_t>((2 * tab.size() + 1) * sizeof(int32_t));   // the frames' ranges, then the bad flag
        })) return rc;
    mp.in = d_payload; mp.in_cap = capacity; mp.stride = stride(h); mp.max_parts = h->max_parts;
    mp.frames = h->mk_tab.as<MaskFrame>(); mp.nframes = (int)tab.size(); mp.frame_offset = frame_offset;
    mp.ntiles = (int)tiles; mp.channels = channels;
    mp.bad = mp.range + 2 * tab.size();
    mp.status = d_status;
    {
        ProfScope ps(h, PBD_K_MK_HULL, h->stream);
        launch_mask(mp, kMkStepHull, h->stream);
    }
    {
        ProfScope ps(h, PBD_K_MK_TILE, h->stream);
        launch_mask(mp, kMkStepTile, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- part-centre poses (pbd_part_poses*; pbd_kernels_publish.hip)
int enqueue_poses(pbd_handle *h, const int32_t *d_word, int capacity, const float *d_centres, const int32_t *d_ncentres,
                  const int32_t *d_dense, int32_t *d_count, float *d_position, float *d_orientation, float *d_eigenvalues)
{
    PoseParams pp{};
    pp.count_word = d_word; pp.cap = capacity; pp.max_parts = h->max_parts;
    pp.centres = d_centres; pp.ncentres = d_ncentres; pp.dense = d_dense;
    pp.count = d_count; pp.position = d_position; pp.orientation = d_orientation; pp.eigenvalues = d_eigenvalues;
    {
        ProfScope ps(h, PBD_K_PART_POSES, h->stream);
        launch_part_poses(pp, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// ---- object clusters (pbd_cluster_objects*; pbd_kernels_cloud.hip)
int check_clouds(pbd_handle *h, int nclouds, const pbd_cloud *c, bool host)
{
    if (nclouds < 1) return fail(h, PBD_ERR_INVALID, "nclouds %d", nclouds);
    for (int f = 0; f < nclouds; ++f) {
        if (!c[f].data || c[f].rows < 1 || c[f].cols < 1 || (long long)c[f].rows * c[f].cols >= (1LL << 31))
            return fail(h, PBD_ERR_INVALID, "cloud %d: %dx%d at %p", f, c[f].rows, c[f].cols, c[f].data);
        if (c[f].point_stride < 3 * sizeof(float))
            return fail(h, PBD_ERR_INVALID, "cloud %d: point stride %zu < 12", f, c[f].point_stride);
        const size_t row_bytes = (size_t)(c[f].cols - 1) * c[f].point_stride + 3 * sizeof(float);
        if (c[f].rows > 1 && c[f].row_stride < row_bytes)
            return fail(h, PBD_ERR_INVALID, "cloud %d: row stride %zu < row bytes %zu", f, c[f].row_stride, row_bytes);
        if (!host && (reinterpret_cast<uintptr_t>(c[f].data) % 4 || c[f].point_stride % 4 || c[f].row_stride % 4))
            return fail(h, PBD_ERR_INVALID, "cloud %d: device pointer %p / strides %zu, %zu not multiples of 4", f, c[f].data,
                        c[f].point_stride, c[f].row_stride);
    }
    return PBD_OK;
}

// the clustering workspace for `capacity` boxes, clouds of at most maxpts points and crop_cap cropped points: the bucket table
// (tcap buckets, a power of two >= 2 crop_cap), the scan partials, and one 256-byte aligned piece per array (cluster_pieces).
// crop_cap <= kClMaxCrop keeps tcap, every bucket index and every count inside an int.
constexpr long long kClMaxCrop = 1LL << 29;
constexpr int kClPieces = 14;
struct ClusterLayout {
    int capacity, nchunks;
    long long crop_cap, units, tcap, nparts;
};
void cluster_pieces(Carve &c, const ClusterLayout &L, ClusterParams &p)
{
    const size_t n = (size_t)L.crop_cap, t = (size_t)L.tcap + 1, cap = (size_t)L.capacity;
    p.chunk_off = c.take<long long>((size_t)(L.units + 1) * 8); p.part = c.take<long long>((size_t)L.nparts * 8);
    p.crop_idx = c.take<int32_t>(n * 4); p.crop_box = c.take<int32_t>(n * 4); p.crop_xyz = c.take<float4>(n * 16);
    p.bucket = c.take<int32_t>(n * 4); p.parent = c.take<int32_t>(n * 4); p.csize = c.take<int32_t>(n * 4);
    p.sorted = c.take<int32_t>(n * 4);
    p.bstart = c.take<int32_t>(t * 4); p.bcur = c.take<int32_t>(t * 4);
    p.best = c.take<unsigned long long>(cap * 8); p.obase = c.take<long long>(cap * 8); p.ntab = c.take<long long>(4 * 8);
}
int cluster_layout(int capacity, long long maxpts, long long crop_cap, ClusterLayout &L)
{
    if (capacity < 0 || maxpts < 1 || crop_cap < 0 || crop_cap > kClMaxCrop) return PBD_ERR_INVALID;
    L.capacity = capacity; L.crop_cap = crop_cap;
    L.nchunks = (int)((maxpts + kClChunk - 1) / kClChunk);
    L.units = (long long)capacity * L.nchunks;
    L.tcap = 2;
    while (L.tcap < 2 * crop_cap) L.tcap <<= 1;
    L.nparts = std::max(L.units + 1, L.tcap + 1) / (4 * 256) + 2;
    return PBD_OK;
}

// the workspace (cluster_layout), the cloud table, and the fixed sequence of launches
int enqueue_cluster(pbd_handle *h, const std::vector<CloudFrame> &tab, const int32_t *d_payload, int capacity, int rec_stride,
                    int frame_offset, const double *d_boxes, int crop_cap, int index_cap, float *d_centres, int32_t *d_counts,
                    int32_t *d_indices, long long *d_status)
{
    long long maxpts = 1;
    for (const CloudFrame &c : tab) maxpts = std::max(maxpts, (long long)c.rows * c.cols);
    ClusterLayout L;
    if (cluster_layout(capacity, maxpts, crop_cap, L))
        return fail(h, PBD_ERR_INVALID, "crop capacity %d (at most 2^29), capacity %d", crop_cap, capacity);
    ClusterParams p{};
    if (int rc = carve(h, h->cl_ws, [&](Carve &c) { cluster_pieces(c, L, p); })) return rc;
    if (int rc = h->cl_tab.stage(h, tab.data(), tab.size() * sizeof(CloudFrame))) return rc;
    p.in = d_payload; p.in_cap = capacity; p.rec_stride = rec_stride; p.frame_offset = frame_offset;
    p.clouds = h->cl_tab.as<CloudFrame>(); p.nclouds = (int)tab.size(); p.nchunks = L.nchunks;
    p.boxes = d_boxes; p.crop_cap = crop_cap; p.index_cap = index_cap;
    p.tcap = (int)L.tcap;      // <= 2^30 (cluster_layout)
    p.centres = d_centres; p.counts = d_counts; p.indices = d_indices; p.status = d_status;
    static const int ids[kClSteps] = {PBD_K_CL_CROP_COUNT, PBD_K_CL_CROP_SCAN, PBD_K_CL_CROP_SCATTER, PBD_K_CL_CLEAR, PBD_K_CL_GRID_COUNT,
                                      PBD_K_CL_GRID_SCAN, PBD_K_CL_GRID_SCATTER, PBD_K_CL_HOOK, PBD_K_CL_LABEL, PBD_K_CL_BEST,
                                      PBD_K_CL_SELECT, PBD_K_CL_OUT};
    for (int step = 0; step < kClSteps; ++step) {
        ProfScope ps(h, ids[step], h->stream);
        launch_cluster_step(p, step, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// the clouds' x, y, z of a host form, packed densely into `buf`; packed[f] describes cloud f there
int upload_clouds_host(pbd_handle *h, DevBuf &buf, int nclouds, const pbd_cloud *clouds, std::vector<pbd_cloud> &packed, size_t *npoints)
{
    size_t total = 0;
    for (int f = 0; f < nclouds; ++f) total += (size_t)clouds[f].rows * clouds[f].cols;
    std::vector<float> xyz(total * 3);
    packed.resize(nclouds);
    HIPCHK(h, buf.ensure(total * 12 + 16));
    size_t off = 0;
    for (int f = 0; f < nclouds; ++f) {
        const pbd_cloud &c = clouds[f];
        for (int r = 0; r < c.rows; ++r)
            for (int k = 0; k < c.cols; ++k)
                memcpy(&xyz[(off + (size_t)r * c.cols + k) * 3],
                       static_cast<const uint8_t *>(c.data) + r * c.row_stride + k * c.point_stride, 12);
        packed[f] = pbd_cloud{buf.as<uint8_t>() + off * 12, c.rows, c.cols, 12, (size_t)c.cols * 12};
        off += (size_t)c.rows * c.cols;
    }
    HIPCHK(h, hipMemcpyAsync(buf.p, xyz.data(), total * 12, hipMemcpyHostToDevice, h->stream));
    *npoints = total;
    return PBD_OK;
}

// the kernels' cloud table of clouds already on the device
std::vector<CloudFrame> cloud_table(int nclouds, const pbd_cloud *d_clouds)
{
    std::vector<CloudFrame> tab(nclouds);
    for (int f = 0; f < nclouds; ++f)
        tab[f] = CloudFrame{static_cast<const uint8_t *>(d_clouds[f].data), d_clouds[f].rows, d_clouds[f].cols,
                            (long long)d_clouds[f].point_stride, (long long)d_clouds[f].row_stride};
    return tab;
}

// ---- plane removal (pbd_remove_planes*; pbd_kernels_planes.hip)
// the reference's call (include/PointCloudClusterer.hpp:294-336 with PCL's defaults): see include/pbd.h
pbd_plane_params plane_defaults()
{
    pbd_plane_params q;
    q.smoothing_size = 10;
    q.depth_change_factor = 0.02f;
    q.distance_threshold = 0.02f;
    q.angular_threshold = 3.0 * M_PI / 180.0;
    q.max_curvature = 0.001;
    q.min_inliers = 1000;
    q.refine = 1;
    return q;
}

int check_plane_params(pbd_handle *h, const pbd_plane_params &q)
{
    if (q.smoothing_size < 2 || q.smoothing_size > 128 || q.min_inliers < 0 || !std::isfinite(q.depth_change_factor) ||
        !std::isfinite(q.distance_threshold) || !std::isfinite(q.angular_threshold) || !std::isfinite(q.max_curvature) ||
        (q.refine != 0 && q.refine != 1))
        return fail(h, PBD_ERR_INVALID, "plane parameters: smoothing size %d (2..128), min inliers %d (>= 0), refine %d (0 or 1), "
                    "every threshold finite", q.smoothing_size, q.min_inliers, q.refine);
    return PBD_OK;
}

// organized clouds: the pbd_cloud rules, rows >= 2 and cols >= 2, and fewer than 2^31 points in the whole call
int check_organized(pbd_handle *h, int nclouds, const pbd_cloud *c, bool host)
{
    if (int rc = check_clouds(h, nclouds, c, host)) return rc;
    long long total = 0;
    for (int f = 0; f < nclouds; ++f) {
        if (c[f].rows < 2 || c[f].cols < 2)
            return fail(h, PBD_ERR_INVALID, "cloud %d: %dx%d is not organized (rows and cols >= 2)", f, c[f].rows, c[f].cols);
        total += (long long)c[f].rows * c[f].cols;
    }
    if (total >= (1LL << 31)) return fail(h, PBD_ERR_INVALID, "the clouds of one call hold %lld points (below 2^31)", total);
    return PBD_OK;
}

// the plane-removal workspace: one 256-byte aligned piece per array.  cand_cap bounds the segments above min_inliers: at most
// points / (min_inliers + 1) per cloud
void plane_pieces(Carve &w, int nclouds, long long npts, long long nrows, long long cand_cap, PlaneParams &p)
{
    const size_t n = (size_t)npts, c = (size_t)cand_cap + 1, tiles = (n + 1023) / 1024 + 2;
    p.xyz = w.take<float4>(n * 16); p.rsx = w.take<float4>(n * 16); p.rsy = w.take<float4>(n * 16); p.nrm = w.take<float4>(n * 16);
    p.parent = w.take<int32_t>(n * 4); p.csize = w.take<int32_t>(n * 4); p.flag = w.take<int32_t>((n + 1) * 4);
    p.lab = w.take<int32_t>(n * 4);
    p.part = w.take<long long>(tiles * 8);
    p.cand_root = w.take<int32_t>(c * 4); p.cand_plane = w.take<int32_t>(c * 4); p.plane_cnt = w.take<int32_t>(c * 4);
    p.cand_coef = w.take<float4>(c * 16); p.plane_coef = w.take<float4>(c * 16);
    p.cbase = w.take<int32_t>(((size_t)nclouds + 1) * 4); p.np = w.take<int32_t>((size_t)nclouds * 4);
    p.xch = w.take<int2>(2 * (size_t)nrows * 8);
}

// the workspace, the cloud table and the fixed sequence of launches; outputs as pbd_remove_planes_device
int enqueue_planes(pbd_handle *h, const std::vector<PlaneCloud> &tab, const pbd_plane_params &q, float *d_points, int32_t *d_kept,
                   int32_t *d_nkept, int32_t *d_labels, float *d_planes, int32_t *d_inliers, int32_t *d_nplanes, int plane_cap,
                   long long *d_status)
{
    const int nclouds = (int)tab.size() - 1;
    long long cand_cap = 0, nrows = 0;
    for (int i = 0; i < nclouds; ++i) {
        cand_cap += (long long)tab[i].rows * tab[i].cols / ((long long)q.min_inliers + 1);
        nrows += tab[i].rows;
    }
    const long long npts = tab[nclouds].base;
    PlaneParams p{};
    if (int rc = carve(h, h->pl_ws, [&](Carve &w) { plane_pieces(w, nclouds, npts, nrows, cand_cap, p); })) return rc;
    if (int rc = h->pl_tab.stage(h, tab.data(), tab.size() * sizeof(PlaneCloud))) return rc;
    p.clouds = h->pl_tab.as<PlaneCloud>(); p.nclouds = nclouds; p.npts = npts;
    p.half = q.smoothing_size / 2;
    p.depth_change = q.depth_change_factor; p.dist_thr = q.distance_threshold;
    p.cos_thr = (float)cos(q.angular_threshold);
    p.max_curv = q.max_curvature; p.min_inliers = q.min_inliers;
    p.plane_cap = plane_cap; p.cand_cap = (int)std::min<long long>(cand_cap, INT32_MAX);
    p.points = d_points; p.kept = d_kept; p.nkept = d_nkept; p.labels = d_labels; p.planes = d_planes; p.inliers = d_inliers;
    p.nplanes = d_nplanes; p.status = d_status;
    for (int step = 0; step < kPlSteps; ++step)
        if (step != kPlStepRefine || q.refine) launch_planes_step(p, step, h->stream);
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// the cloud table of a call: every cloud's place in the concatenation, one closing entry holding the point total
std::vector<PlaneCloud> plane_table(int nclouds, const pbd_cloud *c)
{
    std::vector<PlaneCloud> tab(nclouds + 1);
    long long base = 0, rbase = 0;
    for (int f = 0; f < nclouds; ++f) {
        tab[f] = PlaneCloud{static_cast<const uint8_t *>(c[f].data), c[f].rows, c[f].cols, (long long)c[f].point_stride,
                            (long long)c[f].row_stride, base, rbase};
        base += (long long)c[f].rows * c[f].cols;
        rbase += c[f].rows;
    }
    tab[nclouds] = PlaneCloud{nullptr, 0, 0, 0, 0, base, rbase};
    return tab;
}


// ---- testing a model (pbd_part_nms*, pbd_best_overlap*, pbd_eval_pck*, pbd_eval_apk*; pbd_kernels_eval.hip)
// the one part count of the model's components (Matlab's box matrix has one width)
int eval_nparts(pbd_handle *h, int *nparts)
{
    const int np = h->part_offset[1] - h->part_offset[0];
    for (int c = 1; c < h->NC; ++c)
        if (h->part_offset[c + 1] - h->part_offset[c] != np)
            return fail(h, PBD_ERR_UNSUPPORTED, "component %d has %d parts, component 0 has %d: the evaluation reads one part count", c,
                        h->part_offset[c + 1] - h->part_offset[c], np);
    *nparts = np;
    return PBD_OK;
}

int check_eval_list(pbd_handle *h, int nframes, int capacity, int nparts)
{
    if (nframes < 1 || nframes > 65535) return fail(h, PBD_ERR_INVALID, "nframes %d (1..65535)", nframes);
    if (capacity < 0 || (long long)capacity * std::max(nparts, 1) >= (1LL << 30))
        return fail(h, PBD_ERR_INVALID, "capacity %d: %d-part records (below 2^30 parts)", capacity, nparts);
    return PBD_OK;
}

// the workspace and the four steps of the part NMS on the handle's stream: payload d_in (capacity records) -> d_out
int enqueue_part_nms(pbd_handle *h, int nframes, float overlap, int max_boxes, const int32_t *d_in, int capacity, int frame_offset,
                     int32_t *d_out, int out_cap)
{
    EvalNmsParams p{};
    if (int rc = eval_nparts(h, &p.nparts)) return rc;
    p.row_words = (max_boxes + 63) / 64;
    const size_t cap = (size_t)std::max(capacity, 1), ranks = (size_t)nframes * max_boxes;
    if (int rc = carve(h, h->ev_ws, [&](Carve &c) {
            p.frame = c.take<int32_t>(cap * 4); p.key = c.take<uint32_t>(cap * 4); p.bad = c.take<int32_t>(256);
            p.order = c.take<int32_t>(ranks * 4); p.hull = c.take<double>(ranks * 4 * 8);
            p.bits = c.take<unsigned long long>(ranks * p.row_words * 8); p.slot = c.take<int32_t>(ranks * 4);
            p.fm = c.take<int32_t>((size_t)nframes * 4); p.fkept = c.take<int32_t>((size_t)nframes * 4);
        })) return rc;
    p.in = d_in; p.in_cap = capacity; p.stride = stride(h); p.nframes = nframes; p.frame_offset = frame_offset;
    p.max_boxes = max_boxes; p.overlap = overlap; p.out = d_out; p.out_cap = std::max(out_cap, 0);
    HIPCHK(h, hipMemsetAsync(p.bad, 0, sizeof(int32_t), h->stream));
    static const int ids[kEvNmsSteps] = {PBD_K_EV_NMS_SELECT, PBD_K_EV_NMS_PAIRS, PBD_K_EV_NMS_GREEDY, PBD_K_EV_NMS_EMIT};
    for (int step = 0; step < kEvNmsSteps; ++step) {
        ProfScope ps(h, ids[step], h->stream);
        launch_eval_nms(p, step, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

int check_part_nms(pbd_handle *h, float overlap, int max_boxes)
{
    if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
    if (max_boxes < 1 || max_boxes > kEvMaxBoxes) return fail(h, PBD_ERR_INVALID, "max_boxes %d (1..%d)", max_boxes, kEvMaxBoxes);
    return PBD_OK;
}

// the ground-truth boxes through the staging buffer, then the two kernels
int enqueue_best_overlap(pbd_handle *h, int nframes, const double *gtbox, float overlap, const int32_t *d_in, int capacity,
                         int frame_offset, int32_t *d_out, int32_t *d_found)
{
    EvalBestParams p{};
    if (int rc = eval_nparts(h, &p.nparts)) return rc;
    if (int rc = carve(h, h->ev_ws, [&](Carve &c) { p.best = c.take<unsigned long long>((size_t)nframes * 8); })) return rc;
    if (int rc = h->ev_tab.stage(h, gtbox, (size_t)nframes * 4 * sizeof(double))) return rc;
    p.in = d_in; p.in_cap = capacity; p.stride = stride(h); p.nframes = nframes; p.frame_offset = frame_offset; p.overlap = overlap;
    p.gtbox = h->ev_tab.as<double>(); p.out = d_out; p.found = d_found;
    HIPCHK(h, hipMemsetAsync(p.best, 0, (size_t)nframes * 8, h->stream));
    {
        ProfScope ps(h, PBD_K_EV_BEST, h->stream);
        launch_eval_best(p, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

int enqueue_pck(pbd_handle *h, int nframes, const int32_t *d_rec, const int32_t *d_found, const double *gt_points, const double *scale,
                double thresh, double *d_pck, double *d_dist)
{
    EvalPckParams p{};
    if (int rc = eval_nparts(h, &p.nparts)) return rc;
    const size_t ngt = (size_t)nframes * p.nparts * 2;
    std::vector<double> tab(ngt + nframes);
    memcpy(tab.data(), gt_points, ngt * sizeof(double));
    memcpy(tab.data() + ngt, scale, (size_t)nframes * sizeof(double));
    if (int rc = h->ev_tab.stage(h, tab.data(), tab.size() * sizeof(double))) return rc;
    p.rec = d_rec; p.found = d_found; p.stride = stride(h); p.nframes = nframes;
    p.gt = h->ev_tab.as<double>(); p.scale = p.gt + ngt; p.thresh = thresh; p.pck = d_pck; p.dist = d_dist;
    {
        ProfScope ps(h, PBD_K_EV_PCK, h->stream);
        launch_eval_pck(p, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

int check_apk_gt(pbd_handle *h, int nframes, const int32_t *gt_offset, int nparts)
{
    if (gt_offset[0] != 0) return fail(h, PBD_ERR_INVALID, "gt_offset[0] %d (0)", gt_offset[0]);
    for (int f = 0; f < nframes; ++f)
        if (gt_offset[f + 1] < gt_offset[f]) return fail(h, PBD_ERR_INVALID, "gt_offset[%d] %d below gt_offset[%d] %d", f + 1, gt_offset[f + 1], f, gt_offset[f]);
    const int G = gt_offset[nframes];
    if (G < 1) return fail(h, PBD_ERR_INVALID, "no ground-truth instance: recall is 0 / 0");
    if ((long long)G * nparts >= (1LL << 30)) return fail(h, PBD_ERR_INVALID, "%d instances of %d parts (below 2^30 points)", G, nparts);
    return PBD_OK;
}

int enqueue_apk(pbd_handle *h, int nframes, const int32_t *gt_offset, const double *gt_points, const double *gt_scale, double thresh,
                const int32_t *d_in, int capacity, int frame_offset, double *d_apk, double *d_prec, double *d_rec, int32_t *d_status)
{
    EvalApkParams p{};
    if (int rc = eval_nparts(h, &p.nparts)) return rc;
    p.G = gt_offset[nframes];
    p.list_cap = std::max(std::min(capacity, p.G), 1);
    const size_t cap = (size_t)std::max(capacity, 1), np = (size_t)p.nparts, ngt = (size_t)p.G * np * 2;
    if (int rc = carve(h, h->ev_ws, [&](Carve &c) {
            p.key = c.take<uint32_t>(cap * 4); p.order = c.take<int32_t>(cap * 4); p.close = c.take<int32_t>(cap * np * 4);
            p.first = c.take<int32_t>((size_t)p.G * np * 4); p.tplist = c.take<int32_t>(np * p.list_cap * 4);
            p.mp = c.take<double>(np * p.list_cap * 8);
        })) return rc;
    // one staged block: the points, the scales, the offsets
    std::vector<double> tab(ngt + p.G + (nframes + 2) / 2);
    memcpy(tab.data(), gt_points, ngt * sizeof(double));
    memcpy(tab.data() + ngt, gt_scale, (size_t)p.G * sizeof(double));
    memcpy(tab.data() + ngt + p.G, gt_offset, ((size_t)nframes + 1) * sizeof(int32_t));
    if (int rc = h->ev_tab.stage(h, tab.data(), tab.size() * sizeof(double))) return rc;
    p.gt = h->ev_tab.as<double>(); p.gscale = p.gt + ngt; p.gt_offset = reinterpret_cast<const int32_t *>(p.gscale + p.G);
    p.in = d_in; p.in_cap = capacity; p.stride = stride(h); p.nframes = nframes; p.frame_offset = frame_offset; p.thresh = thresh;
    p.apk = d_apk; p.prec = d_prec; p.rec = d_rec; p.status = d_status;
    HIPCHK(h, hipMemsetAsync(p.first, 0x7f, (size_t)p.G * np * 4, h->stream));   // 0x7f7f7f7f: above every rank
    static const int ids[kEvApkSteps] = {PBD_K_EV_APK_RANK, PBD_K_EV_APK_CLOSE, PBD_K_EV_APK_AP};
    for (int step = 0; step < kEvApkSteps; ++step) {
        ProfScope ps(h, ids[step], h->stream);
        launch_eval_apk(p, step, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    return PBD_OK;
}

// the host records of a call as a payload in h->ev_in (word 0 = ncand)
int upload_eval_list(pbd_handle *h, const int32_t *cand, int ncand)
{
    const size_t words = (size_t)ncand * stride(h);
    HIPCHK(h, h->ev_in.ensure((words + 1) * sizeof(int32_t)));
    HIPCHK(h, hipMemcpyAsync(h->ev_in.p, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (ncand) HIPCHK(h, hipMemcpyAsync(h->ev_in.as<int32_t>() + 1, cand, words * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    return PBD_OK;
}

}  // namespace

// ================================================================================================
extern "C" {

// the clustering workspace of pbd_cluster_objects* (host-only, no GPU needed): out = {nchunks, units, tcap, nparts, total, the
// 14 piece sizes}; PBD_ERR_INVALID for a crop capacity the calls refuse
int pbd_debug_cluster_layout(int capacity, long long maxpts, long long crop_cap, long long *out)
{
    ClusterLayout L;
    if (int rc = cluster_layout(capacity, maxpts, crop_cap, L)) return rc;
    long long sizes[kClPieces] = {0};
    Carve c;   // the sizing pass, keeping the pieces' sizes
    c.sizes = sizes; c.nsizes = kClPieces;
    ClusterParams p{};
    cluster_pieces(c, L, p);
    out[0] = L.nchunks; out[1] = L.units; out[2] = L.tcap; out[3] = L.nparts; out[4] = (long long)Carve::up(c.off, 256);
    for (int i = 0; i < kClPieces; ++i) out[5 + i] = sizes[i];
    return c.pieces == kClPieces ? PBD_OK : PBD_ERR_STATE;
}
// Candidate::boundingBox3D(im, depth) per record (include/Candidate.hpp:140-216).  See include/pbd.h.
int pbd_boxes3d(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, const int *im_rows, const int *im_cols,
                const int32_t *cand, int ncand, int frame_offset, double *out)
{
    return entry(h, depth && im_rows && im_cols && (ncand <= 0 || (cand && out)), kIdle, [&]() -> int {
        if (ncand < 0) return fail(h, PBD_ERR_INVALID, "ncand %d", ncand);
        if (int rc = check_depth_frames(h, nframes, depth, depth_code, true, im_rows, im_cols)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecPlain)) return rc;
        if (ncand == 0) return PBD_OK;
        HIPCHK(h, h->b3_out.ensure((size_t)ncand * 6 * sizeof(double)));
        std::vector<Box3dFrame> tab;
        if (int rc = upload_boxes3d_host(h, nframes, depth, depth_code, im_rows, im_cols, cand, ncand, tab)) return rc;
        if (int rc = enqueue_boxes3d(h, tab, depth_code, h->b3_rec.as<int32_t>(), ncand, frame_offset, h->b3_out.as<double>())) return rc;
        HIPCHK(h, hipMemcpyAsync(out, h->b3_out.p, (size_t)ncand * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_boxes3d_device(pbd_handle *h, int nframes, const pbd_frame *d_depth, int depth_code, const int *im_rows, const int *im_cols,
                       const int32_t *d_payload, int capacity, int frame_offset, double *d_out)
{
    return entry(h, d_depth && im_rows && im_cols && d_payload && (capacity <= 0 || d_out), kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = check_depth_frames(h, nframes, d_depth, depth_code, false, im_rows, im_cols)) return rc;
        if (capacity == 0) return PBD_OK;
        return enqueue_boxes3d(h, depth_table(nframes, d_depth, im_rows, im_cols), depth_code, d_payload, capacity, frame_offset, d_out);
    });
}

// SearchSpacePruning<T>::filterCandidatesByDepth (src/SearchSpacePruning.cpp:73-95).  See include/pbd.h.
int pbd_depth_consistency(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, float zfactor, const int32_t *cand, int ncand,
                          int frame_offset, int32_t *out, int capacity, int *nout)
{
    return entry(h, depth && nout && (ncand <= 0 || cand) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (ncand < 0 || capacity < 0) return fail(h, PBD_ERR_INVALID, "ncand %d, capacity %d", ncand, capacity);
        if (int rc = check_depth_frames(h, nframes, depth, depth_code, true, nullptr, nullptr, &zfactor)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecComponent)) return rc;
        if (ncand == 0) return PBD_OK;
        std::vector<Box3dFrame> tab;   // the depth images packed with dense rows (the pbd_boxes3d host form's buffer)
        if (int rc = upload_depth_host(h, nframes, depth, depth_code, nullptr, nullptr, tab)) return rc;
        return host_list_call(h, h->dc_rec, h->dc_out, cand, ncand, out, capacity, nout, [&](const int32_t *din, int32_t *dout) {
            return enqueue_dc(h, tab, depth_code, zfactor, din, ncand, frame_offset, dout, ncand);
        });
    });
}

int pbd_depth_consistency_device(pbd_handle *h, int nframes, const pbd_frame *d_depth, int depth_code, float zfactor,
                                 const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out, int out_capacity)
{
    return entry(h, d_depth && d_payload && d_out, kIdle, [&]() -> int {
        if (capacity < 0 || out_capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d, out_capacity %d", capacity, out_capacity);
        if (int rc = check_depth_frames(h, nframes, d_depth, depth_code, false, nullptr, nullptr, &zfactor)) return rc;
        return enqueue_dc(h, depth_table(nframes, d_depth), depth_code, zfactor, d_payload, capacity, frame_offset, d_out, out_capacity);
    });
}

// The depth images of the next detect call (pbd_set_depth_prune).  See include/pbd.h.
int pbd_bind_depth(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code)
{
    return entry(h, nframes == 0 || depth, kBusyOk, [&]() -> int {
        h->dpr_bound = pbd_handle::DepthBind{};
        if (nframes == 0) return PBD_OK;
        if (int rc = check_depth_frames(h, nframes, depth, depth_code, true)) return rc;
        // dense rows in a buffer of the binding's own, behind the work already queued (a batch in flight may still read it)
        const size_t es = depth_size(depth_code);
        size_t total = 0;
        for (int f = 0; f < nframes; ++f) total += (size_t)depth[f].rows * depth[f].cols * es;
        HIPCHK(h, h->dpr_depth.ensure(total + 8));
        std::vector<pbd_frame> packed(nframes);
        size_t off = 0;
        for (int f = 0; f < nframes; ++f) {
            const size_t row_bytes = (size_t)depth[f].cols * es;
            uint8_t *dst = h->dpr_depth.as<uint8_t>() + off;
            HIPCHK(h, hipMemcpy2DAsync(dst, row_bytes, depth[f].data, depth[f].stride_bytes, row_bytes, depth[f].rows,
                                       hipMemcpyHostToDevice, h->stream));
            packed[f] = pbd_frame{dst, depth[f].rows, depth[f].cols, row_bytes};
            off += row_bytes * depth[f].rows;
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));   // "copied now": the caller's images may go when the call returns
        h->dpr_bound.tab = depth_table(nframes, packed.data());
        h->dpr_bound.depth = depth_code;
        return PBD_OK;
    });
}

int pbd_bind_depth_device(pbd_handle *h, int nframes, const pbd_frame *d_depth, int depth_code)
{
    return entry(h, nframes == 0 || d_depth, kBusyOk, [&]() -> int {
        h->dpr_bound = pbd_handle::DepthBind{};
        if (nframes == 0) return PBD_OK;
        if (int rc = check_depth_frames(h, nframes, d_depth, depth_code, false)) return rc;
        h->dpr_bound.tab = depth_table(nframes, d_depth);
        h->dpr_bound.depth = depth_code;
        return PBD_OK;
    });
}

// plausible(rect, depth, fx, width, tol) per record of a caller's list.  See include/pbd.h.
int pbd_depth_prune(pbd_handle *h, const pbd_depth_prune_cfg *cfg, int nframes, const pbd_frame *depth, int depth_code,
                    const int32_t *cand, int ncand, int frame_offset, int32_t *out, int capacity, int *nout)
{
    return entry(h, cfg && depth && nout && (ncand <= 0 || cand) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (ncand < 0 || capacity < 0) return fail(h, PBD_ERR_INVALID, "ncand %d, capacity %d", ncand, capacity);
        DepthPruneRule rule;
        if (int rc = depth_prune_rule(h, *cfg, &rule)) return rc;
        if (int rc = check_depth_frames(h, nframes, depth, depth_code, true)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecPlain)) return rc;
        if (ncand == 0) return PBD_OK;
        std::vector<Box3dFrame> tab;   // the depth images packed with dense rows (the pbd_boxes3d host form's buffer)
        if (int rc = upload_depth_host(h, nframes, depth, depth_code, nullptr, nullptr, tab)) return rc;
        return host_list_call(h, h->dc_rec, h->dc_out, cand, ncand, out, capacity, nout, [&](const int32_t *din, int32_t *dout) {
            return enqueue_depth_prune(h, tab, depth_code, rule, din, ncand, frame_offset, dout, ncand);
        });
    });
}

int pbd_depth_prune_device(pbd_handle *h, const pbd_depth_prune_cfg *cfg, int nframes, const pbd_frame *d_depth, int depth_code,
                           const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out, int out_capacity)
{
    return entry(h, cfg && d_depth && d_payload && d_out, kIdle, [&]() -> int {
        if (capacity < 0 || out_capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d, out_capacity %d", capacity, out_capacity);
        DepthPruneRule rule;
        if (int rc = depth_prune_rule(h, *cfg, &rule)) return rc;
        if (int rc = check_depth_frames(h, nframes, d_depth, depth_code, false)) return rc;
        return enqueue_depth_prune(h, depth_table(nframes, d_depth), depth_code, rule, d_payload, capacity, frame_offset, d_out,
                                   out_capacity);
    });
}

// nonMaximaSuppression(src, sz, dst, mask) (src/nms.cpp:84-129) over a set of planes.  See include/pbd.h.
int pbd_grid_nms(pbd_handle *h, int nplanes, const int *rows, const int *cols, int real_code, const void *src, const uint8_t *mask,
                 int sz, uint8_t *dst)
{
    return entry(h, true, kIdle, [&]() -> int {
        long long total = 0;
        if (int rc = check_grid_nms(h, nplanes, rows, cols, real_code, src, dst, sz, &total)) return rc;
        if (total == 0) return PBD_OK;
        const size_t n = (size_t)total, es = real_code == PBD_REAL_F64 ? sizeof(double) : sizeof(float);
        HIPCHK(h, h->gn_src.ensure(n * es));
        HIPCHK(h, h->gn_dst.ensure(n));
        HIPCHK(h, hipMemcpyAsync(h->gn_src.p, src, n * es, hipMemcpyHostToDevice, h->stream));
        if (mask) {
            HIPCHK(h, h->gn_mask.ensure(n));
            HIPCHK(h, hipMemcpyAsync(h->gn_mask.p, mask, n, hipMemcpyHostToDevice, h->stream));
        }
        if (int rc = enqueue_grid_nms(h, nplanes, rows, cols, real_code, h->gn_src.p, mask ? h->gn_mask.as<uint8_t>() : nullptr, sz,
                                      h->gn_dst.as<uint8_t>())) return rc;
        HIPCHK(h, hipMemcpyAsync(dst, h->gn_dst.p, n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_grid_nms_device(pbd_handle *h, int nplanes, const int *rows, const int *cols, int real_code, const void *d_src,
                        const uint8_t *d_mask, int sz, uint8_t *d_dst)
{
    return entry(h, true, kIdle, [&]() -> int {
        long long total = 0;
        if (int rc = check_grid_nms(h, nplanes, rows, cols, real_code, d_src, d_dst, sz, &total)) return rc;
        const size_t es = real_code == PBD_REAL_F64 ? sizeof(double) : sizeof(float);
        if (reinterpret_cast<uintptr_t>(d_src) % es)
            return fail(h, PBD_ERR_INVALID, "device pointer %p not a multiple of the %zu-byte element", d_src, es);
        if (total == 0) return PBD_OK;
        return enqueue_grid_nms(h, nplanes, rows, cols, real_code, d_src, d_mask, sz, d_dst);
    });
}

// The K best elements of every segment of a packed array.  See include/pbd.h.
int pbd_top_k_cells(pbd_handle *h, int nseg, const long long *len, int real_code, const void *src, const uint8_t *mask, int k,
                    uint8_t *dst)
{
    return entry(h, true, kIdle, [&]() -> int {
        long long total = 0;
        if (int rc = check_top_k_cells(h, nseg, len, real_code, src, dst, k, &total)) return rc;
        if (total == 0) return PBD_OK;
        const size_t n = (size_t)total, es = real_code == PBD_REAL_F64 ? sizeof(double) : sizeof(float);
        HIPCHK(h, h->tk_src.ensure(n * es));
        HIPCHK(h, h->tk_dst.ensure(n));
        HIPCHK(h, hipMemcpyAsync(h->tk_src.p, src, n * es, hipMemcpyHostToDevice, h->stream));
        if (mask) {
            HIPCHK(h, h->tk_mask.ensure(n));
            HIPCHK(h, hipMemcpyAsync(h->tk_mask.p, mask, n, hipMemcpyHostToDevice, h->stream));
        }
        if (int rc = enqueue_top_k_cells(h, nseg, len, real_code, h->tk_src.p, mask ? h->tk_mask.as<uint8_t>() : nullptr, k,
                                         h->tk_dst.as<uint8_t>())) return rc;
        HIPCHK(h, hipMemcpyAsync(dst, h->tk_dst.p, n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_top_k_cells_device(pbd_handle *h, int nseg, const long long *len, int real_code, const void *d_src, const uint8_t *d_mask,
                           int k, uint8_t *d_dst)
{
    return entry(h, true, kIdle, [&]() -> int {
        long long total = 0;
        if (int rc = check_top_k_cells(h, nseg, len, real_code, d_src, d_dst, k, &total)) return rc;
        const size_t es = real_code == PBD_REAL_F64 ? sizeof(double) : sizeof(float);
        if (reinterpret_cast<uintptr_t>(d_src) % es)
            return fail(h, PBD_ERR_INVALID, "device pointer %p not a multiple of the %zu-byte element", d_src, es);
        if (total == 0) return PBD_OK;
        return enqueue_top_k_cells(h, nseg, len, real_code, d_src, d_mask, k, d_dst);
    });
}

// The K best records of every frame of a caller's list.  See include/pbd.h.
int pbd_top_k(pbd_handle *h, int nframes, int k, const int32_t *cand, int ncand, int frame_offset, int32_t *out, int capacity,
              int *nout)
{
    return entry(h, nout && (ncand <= 0 || cand) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (ncand < 0 || capacity < 0) return fail(h, PBD_ERR_INVALID, "ncand %d, capacity %d", ncand, capacity);
        if (int rc = check_top_k_list(h, nframes, k)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecAscending)) return rc;
        if (ncand == 0) return PBD_OK;
        return host_list_call(h, h->tkl_in, h->tkl_out, cand, ncand, out, capacity, nout, [&](const int32_t *din, int32_t *dout) {
            return enqueue_top_k_list(h, nframes, k, din, ncand, frame_offset, dout, ncand);
        });
    });
}

int pbd_top_k_device(pbd_handle *h, int nframes, int k, const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out,
                     int out_capacity)
{
    return entry(h, d_payload && d_out, kIdle, [&]() -> int {
        if (capacity < 0 || out_capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d, out_capacity %d", capacity, out_capacity);
        if (int rc = check_top_k_list(h, nframes, k)) return rc;
        return enqueue_top_k_list(h, nframes, k, d_payload, capacity, frame_offset, d_out, out_capacity);
    });
}

// The scale-space maxima of every frame of a caller's list.  See include/pbd.h.
int pbd_scale_nms(pbd_handle *h, int nframes, int dl, const int32_t *cand, int ncand, int frame_offset, int32_t *out, int capacity,
                  int *nout)
{
    return entry(h, nout && (ncand <= 0 || cand) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (ncand < 0 || capacity < 0) return fail(h, PBD_ERR_INVALID, "ncand %d, capacity %d", ncand, capacity);
        if (int rc = check_scale_nms_list(h, nframes, dl)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecAscending)) return rc;
        if (ncand == 0) return PBD_OK;
        return host_list_call(h, h->snl_in, h->snl_out, cand, ncand, out, capacity, nout, [&](const int32_t *din, int32_t *dout) {
            return enqueue_scale_nms_list(h, nframes, dl, din, ncand, frame_offset, dout, ncand);
        });
    });
}

int pbd_scale_nms_device(pbd_handle *h, int nframes, int dl, const int32_t *d_payload, int capacity, int frame_offset, int32_t *d_out,
                         int out_capacity)
{
    return entry(h, d_payload && d_out, kIdle, [&]() -> int {
        if (capacity < 0 || out_capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d, out_capacity %d", capacity, out_capacity);
        if (int rc = check_scale_nms_list(h, nframes, dl)) return rc;
        return enqueue_scale_nms_list(h, nframes, dl, d_payload, capacity, frame_offset, d_out, out_capacity);
    });
}

// Candidate::sort + Candidate::nonMaximaSuppression of a caller's list (the pbd_set_nms stage).  See include/pbd.h.
int pbd_suppress(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, float overlap, const int32_t *cand, int ncand,
                 int frame_offset, int32_t *out, int capacity, int *nout)
{
    return entry(h, im_rows && im_cols && nout && (ncand <= 0 || cand) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (ncand < 0 || capacity < 0) return fail(h, PBD_ERR_INVALID, "ncand %d, capacity %d", ncand, capacity);
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        Plan *P = nullptr;
        if (int rc = get_suppress_plan(h, nframes, im_rows, im_cols, &P)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecAscending)) return rc;
        if (ncand == 0) return PBD_OK;
        return host_list_call(h, h->sup_in, h->sup_out, cand, ncand, out, capacity, nout, [&](const int32_t *din, int32_t *dout) {
            return enqueue_post(h, nframes, 0, 0, overlap, din, ncand, 0, dout, ncand, h->stream, P, frame_offset);
        });
    });
}

int pbd_suppress_device(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, float overlap, const int32_t *d_payload,
                        int capacity, int frame_offset, int32_t *d_out, int out_capacity)
{
    return entry(h, im_rows && im_cols && d_payload && d_out, kIdle, [&]() -> int {
        if (capacity < 1 || out_capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d (>= 1), out_capacity %d", capacity, out_capacity);
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        Plan *P = nullptr;
        if (int rc = get_suppress_plan(h, nframes, im_rows, im_cols, &P)) return rc;
        HIPCHK(h, h->sup_bad.ensure(sizeof(int)));
        if (int rc = enqueue_post(h, nframes, 0, 0, overlap, d_payload, capacity, 0, d_out, out_capacity, h->stream, P, frame_offset,
                                  h->sup_bad.as<int>())) return rc;
        HIPCHK(h, hipGetLastError());
        return PBD_OK;
    });
}

// PointCloudClusterer::computeBoundingBoxes after boundingBox3D (include/PointCloudClusterer.hpp:53-153).  See include/pbd.h.
int pbd_boxes3d_camera(pbd_handle *h, int nframes, const pbd_frame *depth, int depth_code, const int *im_rows, const int *im_cols,
                       const pbd_pinhole *cams, int parts_mode, const int32_t *cand, int ncand, int frame_offset, double *box,
                       float *centres, int32_t *ncentres, int32_t *dense)
{
    return entry(h, depth && im_rows && im_cols && cams && (ncand <= 0 || (cand && box && centres && ncentres && dense)), kIdle,
                 [&]() -> int {
        if (ncand < 0) return fail(h, PBD_ERR_INVALID, "ncand %d", ncand);
        if (depth_code != kDepth32F) return check_camera(h, nframes, depth_code, cams, parts_mode);
        if (int rc = check_depth_frames(h, nframes, depth, depth_code, true, im_rows, im_cols)) return rc;
        if (int rc = check_camera(h, nframes, depth_code, cams, parts_mode)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecPlain)) return rc;
        if (ncand == 0) return PBD_OK;
        const size_t nb = (size_t)ncand * 6 * sizeof(double), nc = (size_t)ncand * h->max_parts * 3 * sizeof(float),
                     ni = (size_t)ncand * sizeof(int32_t);
        HIPCHK(h, h->cam_out.ensure(nb + nc + 2 * ni));
        uint8_t *o = h->cam_out.as<uint8_t>();
        std::vector<Box3dFrame> tab;
        if (int rc = upload_boxes3d_host(h, nframes, depth, depth_code, im_rows, im_cols, cand, ncand, tab)) return rc;
        HIPCHK(h, hipMemsetAsync(o + nb, 0, nc, h->stream));
        if (int rc = enqueue_camera(h, tab, depth_code, cams, parts_mode, h->b3_rec.as<int32_t>(), ncand, frame_offset, (double *)o,
                                    (float *)(o + nb), (int32_t *)(o + nb + nc), (int32_t *)(o + nb + nc + ni))) return rc;
        HIPCHK(h, hipMemcpyAsync(box, o, nb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(centres, o + nb, nc, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(ncentres, o + nb + nc, ni, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(dense, o + nb + nc + ni, ni, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_boxes3d_camera_device(pbd_handle *h, int nframes, const pbd_frame *d_depth, int depth_code, const int *im_rows,
                              const int *im_cols, const pbd_pinhole *cams, int parts_mode, const int32_t *d_payload, int capacity,
                              int frame_offset, double *d_box, float *d_centres, int32_t *d_ncentres, int32_t *d_dense)
{
    return entry(h, d_depth && im_rows && im_cols && cams && d_payload && (capacity <= 0 || (d_box && d_centres && d_ncentres && d_dense)),
                 kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (depth_code != kDepth32F) return check_camera(h, nframes, depth_code, cams, parts_mode);
        if (int rc = check_depth_frames(h, nframes, d_depth, depth_code, false, im_rows, im_cols)) return rc;
        if (int rc = check_camera(h, nframes, depth_code, cams, parts_mode)) return rc;
        if (capacity == 0) return PBD_OK;
        return enqueue_camera(h, depth_table(nframes, d_depth, im_rows, im_cols), depth_code, cams, parts_mode, d_payload, capacity,
                              frame_offset, d_box, d_centres, d_ncentres, d_dense);
    });
}

// PointCloudClusterer::clusterObjects (include/PointCloudClusterer.hpp:157-293).  See include/pbd.h.
int pbd_cluster_objects(pbd_handle *h, int nclouds, const pbd_cloud *clouds, const double *boxes, const int *frames, int nboxes,
                        float *centres, int32_t *counts, int32_t *indices, int index_capacity, int *needed)
{
    return entry(h, clouds && needed && (nboxes <= 0 || (boxes && frames && centres && counts)) && (index_capacity <= 0 || indices),
                 kIdle, [&]() -> int {
        *needed = 0;
        if (nboxes < 0 || index_capacity < 0) return fail(h, PBD_ERR_INVALID, "nboxes %d, index capacity %d", nboxes, index_capacity);
        if (int rc = check_clouds(h, nclouds, clouds, true)) return rc;
        for (int i = 0; i < nboxes; ++i)
            if (frames[i] < 0 || frames[i] >= nclouds) return fail(h, PBD_ERR_INVALID, "box %d: frame %d outside 0..%d", i, frames[i], nclouds - 1);
        if (nboxes == 0) return PBD_OK;
        std::vector<pbd_cloud> packed;
        size_t total = 0;
        if (int rc = upload_clouds_host(h, h->cl_cloud, nclouds, clouds, packed, &total)) return rc;
        const std::vector<CloudFrame> tab = cloud_table(nclouds, packed.data());
        // the boxes and a payload of stride 1 holding the frames
        const size_t bb = (size_t)nboxes * 6 * sizeof(double), pb = ((size_t)nboxes + 1) * sizeof(int32_t);
        HIPCHK(h, h->cl_in.ensure(bb + pb + 16));
        std::vector<int32_t> pay(nboxes + 1);
        pay[0] = nboxes;
        for (int i = 0; i < nboxes; ++i) pay[i + 1] = frames[i];
        HIPCHK(h, hipMemcpyAsync(h->cl_in.p, boxes, bb, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->cl_in.as<uint8_t>() + bb, pay.data(), pb, hipMemcpyHostToDevice, h->stream));
        const double *d_boxes = h->cl_in.as<double>();
        const int32_t *d_pay = reinterpret_cast<const int32_t *>(h->cl_in.as<uint8_t>() + bb);
        // outputs: centres, counts, status, then the indices (at most the cropped points)
        long long crop_cap = std::max<long long>(h->cl_crop_cap, 1 << 16);
        long long status[2] = {0, 0};
        for (int pass = 0; pass < 2; ++pass) {
            const size_t oc = (size_t)nboxes * 12, on = (size_t)nboxes * 4;
            HIPCHK(h, h->cl_out.ensure(oc + on + 16 + 16 + (size_t)crop_cap * 4));
            uint8_t *o = h->cl_out.as<uint8_t>();
            long long *d_status = reinterpret_cast<long long *>(o + (oc + on + 15) / 16 * 16);
            int32_t *d_idx = reinterpret_cast<int32_t *>(d_status + 2);
            if (int rc = enqueue_cluster(h, tab, d_pay, nboxes, 1, 0, d_boxes, (int)crop_cap, (int)crop_cap, (float *)o,
                                         (int32_t *)(o + oc), d_idx, d_status)) return rc;
            HIPCHK(h, hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (status[0] <= crop_cap) {
                h->cl_crop_cap = std::max(h->cl_crop_cap, crop_cap);
                if (status[1] > index_capacity) {
                    *needed = (int)status[1];
                    return fail(h, PBD_ERR_CAPACITY, "the kept clusters hold %lld indices, capacity %d", status[1], index_capacity);
                }
                *needed = (int)status[1];
                HIPCHK(h, hipMemcpyAsync(centres, o, oc, hipMemcpyDeviceToHost, h->stream));
                HIPCHK(h, hipMemcpyAsync(counts, o + oc, on, hipMemcpyDeviceToHost, h->stream));
                if (status[1] > 0) HIPCHK(h, hipMemcpyAsync(indices, d_idx, (size_t)status[1] * 4, hipMemcpyDeviceToHost, h->stream));
                HIPCHK(h, hipStreamSynchronize(h->stream));
                return PBD_OK;
            }
            if (status[0] > kClMaxCrop) return fail(h, PBD_ERR_INVALID, "%lld cropped points (at most 2^29)", status[0]);
            crop_cap = status[0];                      // the first pass counted them all: the second fits
        }
        return fail(h, PBD_ERR_HIP, "cropped points changed between two passes");
    });
}

int pbd_cluster_objects_device(pbd_handle *h, int nclouds, const pbd_cloud *d_clouds, const int32_t *d_payload, int capacity,
                               int frame_offset, const double *d_boxes, int crop_capacity, int index_capacity, float *d_centres,
                               int32_t *d_counts, int32_t *d_indices, long long *d_status)
{
    return entry(h, d_clouds && d_payload && d_status && (capacity <= 0 || (d_boxes && d_centres && d_counts)) &&
                    (index_capacity <= 0 || d_indices), kIdle, [&]() -> int {
        if (capacity < 0 || crop_capacity < 0 || index_capacity < 0 || crop_capacity > kClMaxCrop)
            return fail(h, PBD_ERR_INVALID, "capacity %d, crop capacity %d (at most 2^29), index capacity %d", capacity, crop_capacity,
                        index_capacity);
        if (int rc = check_clouds(h, nclouds, d_clouds, false)) return rc;
        if (capacity == 0) {
            HIPCHK(h, hipMemsetAsync(d_status, 0, 2 * sizeof(long long), h->stream));
            return PBD_OK;
        }
        return enqueue_cluster(h, cloud_table(nclouds, d_clouds), d_payload, capacity, stride(h), frame_offset, d_boxes, crop_capacity,
                               index_capacity, d_centres, d_counts, d_indices, d_status);
    });
}

// PointCloudClusterer::organizedMultiplaneSegmentation (include/PointCloudClusterer.hpp:294-336).  See include/pbd.h.
int pbd_remove_planes(pbd_handle *h, int nclouds, const pbd_cloud *clouds, const pbd_plane_params *params, float *points, int32_t *kept,
                      int32_t *nkept, int32_t *labels, float *planes, int32_t *inliers, int32_t *nplanes, int plane_capacity, int *needed)
{
    return entry(h, clouds && points && kept && nkept && labels && nplanes && needed && (plane_capacity <= 0 || (planes && inliers)),
                 kIdle, [&]() -> int {
        *needed = 0;
        const pbd_plane_params q = params ? *params : plane_defaults();
        if (plane_capacity < 0) return fail(h, PBD_ERR_INVALID, "plane capacity %d", plane_capacity);
        if (int rc = check_plane_params(h, q)) return rc;
        if (int rc = check_organized(h, nclouds, clouds, true)) return rc;
        std::vector<pbd_cloud> packed;
        size_t total = 0;
        if (int rc = upload_clouds_host(h, h->pl_cloud, nclouds, clouds, packed, &total)) return rc;
        // outputs: status, counts, then points, kept, labels, planes, inliers
        const size_t cap = (size_t)std::max(plane_capacity, 0);
        const size_t o_stat = 0, o_nk = 16, o_np = o_nk + (size_t)nclouds * 4, o_pts = (o_np + (size_t)nclouds * 4 + 15) / 16 * 16,
                     o_kept = o_pts + total * 12, o_lab = o_kept + total * 4, o_pl = (o_lab + total * 4 + 15) / 16 * 16,
                     o_in = o_pl + (size_t)nclouds * cap * 16, o_end = o_in + (size_t)nclouds * cap * 4;
        HIPCHK(h, h->pl_out.ensure(o_end + 16));
        uint8_t *o = h->pl_out.as<uint8_t>();
        if (int rc = enqueue_planes(h, plane_table(nclouds, packed.data()), q, (float *)(o + o_pts), (int32_t *)(o + o_kept),
                                    (int32_t *)(o + o_nk), (int32_t *)(o + o_lab), (float *)(o + o_pl), (int32_t *)(o + o_in),
                                    (int32_t *)(o + o_np), (int)cap, (long long *)(o + o_stat))) return rc;
        long long status[2] = {0, 0};
        HIPCHK(h, hipMemcpyAsync(status, o + o_stat, sizeof status, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        *needed = (int)status[1];
        if (status[1] > plane_capacity)
            return fail(h, PBD_ERR_CAPACITY, "a cloud holds %lld planes, capacity %d", status[1], plane_capacity);
        HIPCHK(h, hipMemcpyAsync(nkept, o + o_nk, (size_t)nclouds * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(nplanes, o + o_np, (size_t)nclouds * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(points, o + o_pts, total * 12, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(kept, o + o_kept, total * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(labels, o + o_lab, total * 4, hipMemcpyDeviceToHost, h->stream));
        if (cap) {
            HIPCHK(h, hipMemcpyAsync(planes, o + o_pl, (size_t)nclouds * cap * 16, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipMemcpyAsync(inliers, o + o_in, (size_t)nclouds * cap * 4, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_remove_planes_device(pbd_handle *h, int nclouds, const pbd_cloud *d_clouds, const pbd_plane_params *params, float *d_points,
                             int32_t *d_kept, int32_t *d_nkept, int32_t *d_labels, float *d_planes, int32_t *d_inliers,
                             int32_t *d_nplanes, int plane_capacity, long long *d_status)
{
    return entry(h, d_clouds && d_points && d_kept && d_nkept && d_labels && d_nplanes && d_status &&
                    (plane_capacity <= 0 || (d_planes && d_inliers)), kIdle, [&]() -> int {
        const pbd_plane_params q = params ? *params : plane_defaults();
        if (plane_capacity < 0) return fail(h, PBD_ERR_INVALID, "plane capacity %d", plane_capacity);
        if (int rc = check_plane_params(h, q)) return rc;
        if (int rc = check_organized(h, nclouds, d_clouds, false)) return rc;
        return enqueue_planes(h, plane_table(nclouds, d_clouds), q, d_points, d_kept, d_nkept, d_labels, d_planes, d_inliers, d_nplanes,
                              plane_capacity, d_status);
    });
}

// Candidate::mask (include/Candidate.hpp:306-331) and rgb & (mask != 0) (ros/Messages.cpp:157-174).  See include/pbd.h.
int pbd_candidate_mask(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, const int32_t *cand, int ncand, int frame_offset,
                       uint8_t *const *labels, const size_t *label_pitch, int channels, const uint8_t *const *colour,
                       const size_t *colour_pitch, uint8_t *const *masked, const size_t *masked_pitch)
{
    return entry(h, im_rows && im_cols && (ncand <= 0 || cand), kIdle, [&]() -> int {
        if (ncand < 0) return fail(h, PBD_ERR_INVALID, "ncand %d", ncand);
        if (int rc = check_mask_frames(h, nframes, im_rows, im_cols, labels, label_pitch, channels, colour, colour_pitch, masked,
                                       masked_pitch)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecAscending)) return rc;
        const int stride = ::stride(h);
        if (!labels && !masked) return PBD_OK;
        const int cn = masked ? channels : 0;
        // the records as a payload, each frame's labels and colour packed with dense rows in the handle's own buffers
        size_t lab_total = 0, img_total = 0;
        for (int f = 0; f < nframes; ++f) {
            lab_total += labels ? (size_t)im_rows[f] * im_cols[f] : 0;
            img_total += (size_t)im_rows[f] * im_cols[f] * cn;
        }
        uint8_t *lab = nullptr, *img = nullptr;
        if (int rc = carve(h, h->mk_img, [&](Carve &c) {
                lab = c.take<uint8_t>(lab_total);
                img = c.take<uint8_t>(img_total + 256);   // with the room the buffer always had behind the last frame
            })) return rc;
        HIPCHK(h, h->mk_rec.ensure(((size_t)ncand * stride + 1) * sizeof(int32_t)));
        HIPCHK(h, hipMemcpyAsync(h->mk_rec.p, &ncand, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        if (ncand) HIPCHK(h, hipMemcpyAsync(h->mk_rec.as<int32_t>() + 1, cand, (size_t)ncand * stride * sizeof(int32_t),
                                            hipMemcpyHostToDevice, h->stream));
        std::vector<MaskFrame> tab(nframes);
        for (int f = 0; f < nframes; ++f) {
            const size_t lrow = (size_t)im_cols[f], crow = lrow * cn;
            MaskFrame &fr = tab[f];
            fr = MaskFrame{};
            fr.rows = im_rows[f]; fr.cols = im_cols[f];
            if (labels) { fr.labels = lab; fr.label_pitch = (long long)lrow; lab += lrow * im_rows[f]; }
            if (masked) {
                HIPCHK(h, hipMemcpy2DAsync(img, crow, colour[f], colour_pitch[f], crow, im_rows[f], hipMemcpyHostToDevice, h->stream));
                fr.colour = img; fr.masked = img; fr.colour_pitch = fr.masked_pitch = (long long)crow;
                img += crow * im_rows[f];
            }
        }
        if (int rc = enqueue_mask(h, tab, cn, h->mk_rec.as<int32_t>(), ncand, frame_offset, nullptr)) return rc;
        for (int f = 0; f < nframes; ++f) {
            if (labels)
                HIPCHK(h, hipMemcpy2DAsync(labels[f], label_pitch[f], tab[f].labels, (size_t)im_cols[f], (size_t)im_cols[f], im_rows[f],
                                           hipMemcpyDeviceToHost, h->stream));
            if (masked) {
                const size_t crow = (size_t)im_cols[f] * cn;
                HIPCHK(h, hipMemcpy2DAsync(masked[f], masked_pitch[f], tab[f].masked, crow, crow, im_rows[f], hipMemcpyDeviceToHost,
                                           h->stream));
            }
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_candidate_mask_device(pbd_handle *h, int nframes, const int *im_rows, const int *im_cols, const int32_t *d_payload, int capacity,
                              int frame_offset, uint8_t *const *d_labels, const size_t *label_pitch, int channels,
                              const uint8_t *const *d_colour, const size_t *colour_pitch, uint8_t *const *d_masked,
                              const size_t *masked_pitch, int32_t *d_status)
{
    return entry(h, im_rows && im_cols && d_payload && d_status, kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = check_mask_frames(h, nframes, im_rows, im_cols, d_labels, label_pitch, channels, d_colour, colour_pitch, d_masked,
                                       masked_pitch)) return rc;
        std::vector<MaskFrame> tab(nframes);
        for (int f = 0; f < nframes; ++f) {
            MaskFrame &fr = tab[f];
            fr = MaskFrame{};
            fr.rows = im_rows[f]; fr.cols = im_cols[f];
            if (d_labels) { fr.labels = d_labels[f]; fr.label_pitch = (long long)label_pitch[f]; }
            if (d_masked) {
                fr.colour = d_colour[f]; fr.masked = d_masked[f];
                fr.colour_pitch = (long long)colour_pitch[f]; fr.masked_pitch = (long long)masked_pitch[f];
            }
        }
        return enqueue_mask(h, tab, d_masked ? channels : 0, d_payload, capacity, frame_offset, d_status);
    });
}

// PartsBasedDetectorNode::messagePoses (ros/Messages.cpp:187-234) per record.  See include/pbd.h.
int pbd_part_poses(pbd_handle *h, int n, const float *centres, const int32_t *ncentres, const int32_t *dense, int32_t *count,
                   float *position, float *orientation, float *eigenvalues)
{
    return entry(h, n <= 0 || (centres && ncentres && dense && count && position && orientation && eigenvalues), kIdle, [&]() -> int {
        if (n < 0) return fail(h, PBD_ERR_INVALID, "n %d", n);
        for (int i = 0; i < n; ++i)
            if (ncentres[i] < 0 || ncentres[i] > h->max_parts)
                return fail(h, PBD_ERR_INVALID, "record %d: ncentres %d (0..%d)", i, ncentres[i], h->max_parts);
        if (n == 0) return PBD_OK;
        const size_t nc = (size_t)n * h->max_parts * 3 * sizeof(float), ni = (size_t)n * sizeof(int32_t), n3 = (size_t)n * 3 * sizeof(float),
                     n4 = (size_t)n * 4 * sizeof(float);
        HIPCHK(h, h->ps_buf.ensure(nc + 3 * ni + 2 * n3 + n4 + 256));
        uint8_t *b = h->ps_buf.as<uint8_t>();
        float *d_cen = (float *)b, *d_pos = (float *)(b + nc), *d_ori = (float *)(b + nc + n3), *d_ev = (float *)(b + nc + n3 + n4);
        int32_t *d_nc = (int32_t *)(b + nc + 2 * n3 + n4), *d_dn = d_nc + n, *d_cnt = d_dn + n, *d_word = d_cnt + n;
        HIPCHK(h, hipMemcpyAsync(d_word, &n, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_cen, centres, nc, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_nc, ncentres, ni, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_dn, dense, ni, hipMemcpyHostToDevice, h->stream));
        if (int rc = enqueue_poses(h, d_word, n, d_cen, d_nc, d_dn, d_cnt, d_pos, d_ori, d_ev)) return rc;
        HIPCHK(h, hipMemcpyAsync(count, d_cnt, ni, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(position, d_pos, n3, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(orientation, d_ori, n4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(eigenvalues, d_ev, n3, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_part_poses_device(pbd_handle *h, const int32_t *d_payload, int capacity, const float *d_centres, const int32_t *d_ncentres,
                          const int32_t *d_dense, int32_t *d_count, float *d_position, float *d_orientation, float *d_eigenvalues)
{
    return entry(h, d_payload && (capacity <= 0 || (d_centres && d_ncentres && d_dense && d_count && d_position && d_orientation &&
                                                    d_eigenvalues)), kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (capacity == 0) return PBD_OK;
        return enqueue_poses(h, d_payload, capacity, d_centres, d_ncentres, d_dense, d_count, d_position, d_orientation, d_eigenvalues);
    });
}

// nms.m per frame (matlab/detection/nms.m).  See include/pbd.h.
int pbd_part_nms(pbd_handle *h, int nframes, float overlap, int max_boxes, const int32_t *cand, int ncand, int frame_offset,
                 int32_t *out, int capacity, int *nout)
{
    return entry(h, nout && (ncand <= 0 || cand) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        if (int rc = check_part_nms(h, overlap, max_boxes)) return rc;
        int np;
        if (int rc = eval_nparts(h, &np)) return rc;
        if (int rc = check_eval_list(h, nframes, ncand, np)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecAscending)) return rc;
        if (ncand == 0) return PBD_OK;
        return host_list_call(h, h->ev_in, h->ev_out, cand, ncand, out, capacity, nout, [&](const int32_t *din, int32_t *dout) {
            return enqueue_part_nms(h, nframes, overlap, max_boxes, din, ncand, frame_offset, dout, ncand);
        });
    });
}

int pbd_part_nms_device(pbd_handle *h, int nframes, float overlap, int max_boxes, const int32_t *d_payload, int capacity,
                        int frame_offset, int32_t *d_out, int out_capacity)
{
    return entry(h, d_payload && d_out, kIdle, [&]() -> int {
        if (out_capacity < 0) return fail(h, PBD_ERR_INVALID, "out_capacity %d", out_capacity);
        if (int rc = check_part_nms(h, overlap, max_boxes)) return rc;
        int np;
        if (int rc = eval_nparts(h, &np)) return rc;
        if (int rc = check_eval_list(h, nframes, capacity, np)) return rc;
        return enqueue_part_nms(h, nframes, overlap, max_boxes, d_payload, capacity, frame_offset, d_out, out_capacity);
    });
}

// bestoverlap.m per frame (matlab/detection/bestoverlap.m).  See include/pbd.h.
int pbd_best_overlap(pbd_handle *h, int nframes, const double *gtbox, float overlap, const int32_t *cand, int ncand, int frame_offset,
                     int32_t *out, int32_t *found)
{
    return entry(h, gtbox && out && found && (ncand <= 0 || cand), kIdle, [&]() -> int {
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        int np;
        if (int rc = eval_nparts(h, &np)) return rc;
        if (int rc = check_eval_list(h, nframes, ncand, np)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecPlain)) return rc;
        const size_t rec_bytes = (size_t)nframes * stride(h) * sizeof(int32_t), fnd_bytes = (size_t)nframes * sizeof(int32_t);
        HIPCHK(h, h->ev_out.ensure(rec_bytes + fnd_bytes));
        int32_t *d_out = h->ev_out.as<int32_t>(), *d_found = d_out + (size_t)nframes * stride(h);
        if (int rc = upload_eval_list(h, cand, ncand)) return rc;
        if (int rc = enqueue_best_overlap(h, nframes, gtbox, overlap, h->ev_in.as<int32_t>(), ncand, frame_offset, d_out, d_found)) return rc;
        HIPCHK(h, hipMemcpyAsync(out, d_out, rec_bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(found, d_found, fnd_bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_best_overlap_device(pbd_handle *h, int nframes, const double *gtbox, float overlap, const int32_t *d_payload, int capacity,
                            int frame_offset, int32_t *d_out, int32_t *d_found)
{
    return entry(h, gtbox && d_payload && d_out && d_found, kIdle, [&]() -> int {
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        int np;
        if (int rc = eval_nparts(h, &np)) return rc;
        if (int rc = check_eval_list(h, nframes, capacity, np)) return rc;
        return enqueue_best_overlap(h, nframes, gtbox, overlap, d_payload, capacity, frame_offset, d_out, d_found);
    });
}

// eval_pck.m (matlab/evaluation/eval_pck.m).  See include/pbd.h.
int pbd_eval_pck(pbd_handle *h, int nframes, const int32_t *rec, const int32_t *found, const double *gt_points, const double *scale,
                 double thresh, double *pck, double *dist)
{
    return entry(h, rec && found && gt_points && scale && pck, kIdle, [&]() -> int {
        int np;
        if (int rc = eval_nparts(h, &np)) return rc;
        if (int rc = check_eval_list(h, nframes, nframes, np)) return rc;
        const size_t rec_bytes = (size_t)nframes * stride(h) * sizeof(int32_t), fnd_bytes = (size_t)nframes * sizeof(int32_t),
                     pck_bytes = (size_t)np * sizeof(double), dist_bytes = (size_t)np * nframes * sizeof(double);
        HIPCHK(h, h->ev_in.ensure(rec_bytes + fnd_bytes));
        HIPCHK(h, h->ev_out.ensure(pck_bytes + dist_bytes));
        int32_t *d_rec = h->ev_in.as<int32_t>(), *d_found = d_rec + (size_t)nframes * stride(h);
        double *d_pck = h->ev_out.as<double>(), *d_dist = d_pck + np;
        HIPCHK(h, hipMemcpyAsync(d_rec, rec, rec_bytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_found, found, fnd_bytes, hipMemcpyHostToDevice, h->stream));
        if (int rc = enqueue_pck(h, nframes, d_rec, d_found, gt_points, scale, thresh, d_pck, dist ? d_dist : nullptr)) return rc;
        HIPCHK(h, hipMemcpyAsync(pck, d_pck, pck_bytes, hipMemcpyDeviceToHost, h->stream));
        if (dist) HIPCHK(h, hipMemcpyAsync(dist, d_dist, dist_bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_eval_pck_device(pbd_handle *h, int nframes, const int32_t *d_rec, const int32_t *d_found, const double *gt_points,
                        const double *scale, double thresh, double *d_pck, double *d_dist)
{
    return entry(h, d_rec && d_found && gt_points && scale && d_pck, kIdle, [&]() -> int {
        int np;
        if (int rc = eval_nparts(h, &np)) return rc;
        if (int rc = check_eval_list(h, nframes, nframes, np)) return rc;
        return enqueue_pck(h, nframes, d_rec, d_found, gt_points, scale, thresh, d_pck, d_dist);
    });
}

// eval_apk.m + VOCap.m (matlab/evaluation).  See include/pbd.h.
int pbd_eval_apk(pbd_handle *h, int nframes, const int32_t *gt_offset, const double *gt_points, const double *gt_scale, double thresh,
                 const int32_t *cand, int ncand, int frame_offset, double *apk, double *prec, double *rec)
{
    return entry(h, gt_offset && gt_points && gt_scale && apk && (ncand <= 0 || cand), kIdle, [&]() -> int {
        int np;
        if (int rc = eval_nparts(h, &np)) return rc;
        if (int rc = check_eval_list(h, nframes, ncand, np)) return rc;
        if (int rc = check_apk_gt(h, nframes, gt_offset, np)) return rc;
        if (int rc = check_records(h, nframes, cand, ncand, frame_offset, kRecPlain)) return rc;
        const size_t apk_bytes = (size_t)np * sizeof(double), pr_bytes = (size_t)np * ncand * sizeof(double);
        HIPCHK(h, h->ev_out.ensure(256 + apk_bytes + 2 * pr_bytes));
        double *d_apk = h->ev_out.as<double>() + 32, *d_prec = d_apk + np, *d_rec = d_prec + (size_t)np * ncand;
        if (int rc = upload_eval_list(h, cand, ncand)) return rc;
        if (int rc = enqueue_apk(h, nframes, gt_offset, gt_points, gt_scale, thresh, h->ev_in.as<int32_t>(), ncand, frame_offset, d_apk,
                                 prec ? d_prec : nullptr, rec ? d_rec : nullptr, h->ev_out.as<int32_t>())) return rc;
        HIPCHK(h, hipMemcpyAsync(apk, d_apk, apk_bytes, hipMemcpyDeviceToHost, h->stream));
        if (prec && ncand) HIPCHK(h, hipMemcpyAsync(prec, d_prec, pr_bytes, hipMemcpyDeviceToHost, h->stream));
        if (rec && ncand) HIPCHK(h, hipMemcpyAsync(rec, d_rec, pr_bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_eval_apk_device(pbd_handle *h, int nframes, const int32_t *gt_offset, const double *gt_points, const double *gt_scale,
                        double thresh, const int32_t *d_payload, int capacity, int frame_offset, double *d_apk, double *d_prec,
                        double *d_rec, int32_t *d_status)
{
    return entry(h, gt_offset && gt_points && gt_scale && d_payload && d_apk && d_status, kIdle, [&]() -> int {
        int np;
        if (int rc = eval_nparts(h, &np)) return rc;
        if (int rc = check_eval_list(h, nframes, capacity, np)) return rc;
        if (int rc = check_apk_gt(h, nframes, gt_offset, np)) return rc;
        return enqueue_apk(h, nframes, gt_offset, gt_points, gt_scale, thresh, d_payload, capacity, frame_offset, d_apk, d_prec, d_rec,
                           d_status);
    });
}

}  // extern "C"
