// pbd_capi.hip -- create / destroy, plans, model tables, the detect stages and their C entry points (include/pbd.h), profiling
// and the debug entry points.  The handle and the layer every entry point is written on: pbd_handle.h; the entry points that
// work on a finished candidate list: pbd_capi_post.hip; training: pbd_capi_train.hip.
//
// Host logic restated from the reference for this path:
//   pyramid geometry            src/HOGFeatures.cpp:95-127, include/HOGFeatures.hpp:74-81
//   engine wiring               src/PartsBasedDetector.cpp:69-127
//   Parts index tables          include/Parts.hpp:172-187
// There is no CPU compute path: every stage runs as a HIP kernel (pbd_kernels_*.hip).
#include "pbd_handle.h"

#include <limits.h>
#include <mutex>

using namespace pbd;

namespace pbd {
thread_local ProfHook *g_prof_hook = nullptr;
thread_local std::string g_create_error;

int fail(ErrCtx *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    try {
        if (h) h->err = buf; else g_create_error = buf;
    } catch (...) {   // the message itself could not be stored: the status code still goes out
    }
    return code;
}
}  // namespace pbd

namespace {

// ---- pyramid geometry (host) -------------------------------------------------------------------
// Overload resolution assumed for the reference's expressions: C++11 <cmath>, i.e. pow(float,float)
// and log(float) are the float versions, pow(float,int) promotes to double.
int plan_pyramid(int rows, int cols, int sbin, int interval, std::vector<int> &lr, std::vector<int> &lc,
                 std::vector<float> &scales)
{
    const float sfactor = powf(2.0f, 1.0f / (float)interval);             // HOGFeatures.hpp:78
    const float h = (float)rows, w = (float)cols;
    const float mn = std::min(h, w);
    const float ns = 1 + floorf(logf(mn / (5.0f * (float)sbin)) / logf(sfactor));   // HOGFeatures.cpp:99
    if (!(ns >= 1)) return 0;
    const int n = (int)ns;
    if (n > PBD_MAX_LEVELS) return -1;
    if (n < interval) return -2;   // the reference writes out of bounds here (HOGFeatures.cpp:114-118)
    lr.assign(n, 0); lc.assign(n, 0); scales.assign(n, 0.f);
    for (int i = 0; i < interval; ++i) {
        const float f = (float)((double)1.0f / pow((double)sfactor, (double)i));     // :116
        lc[i] = (int)lrint((double)(w * f));   // Size_<float> -> Size: cvRound, half to even
        lr[i] = (int)lrint((double)(h * f));
        scales[i] = (float)(pow((double)sfactor, (double)i) * (double)sbin);          // :118
        for (int j = i + interval; j < n; j += interval) {                            // :120-126
            lc[j] = (lc[j - interval] + 1) / 2;
            lr[j] = (lr[j - interval] + 1) / 2;
            scales[j] = 2 * scales[j - interval];
        }
    }
    return n;
}

// ---- plan construction -------------------------------------------------------------------------
// Cover a rows x cols level with 256-cell tiles of shape 32x8, 16x16 or 8x32 (shape k: 32>>k wide, 8<<k
// high) so that the fewest lanes compute cells outside the level: a dynamic program over the columns picks
// the vertical strips, each strip is then cut into tiles of its shape.
static void cover_level(int l, int rows, int cols, std::vector<ConvTile> *shaped)
{
    const long long INF = 1LL << 60;
    std::vector<long long> cost(cols + 1, INF);
    std::vector<int> pick(cols + 1, -1);
    cost[0] = 0;
    for (int w = 1; w <= cols; ++w)
        for (int k = 0; k < 3; ++k) {
            const int tw = kConvTW >> k, th = kConvTH << k;
            const int prev = std::max(w - tw, 0);
            const long long c = cost[prev] + (long long)tw * ((rows + th - 1) / th) * th;
            if (c < cost[w]) { cost[w] = c; pick[w] = k; }
        }
    std::vector<std::pair<int, int>> strips;   // (x0, shape), right to left
    for (int w = cols; w > 0;) {
        const int k = pick[w], tw = kConvTW >> k;
        const int x0 = std::max(w - tw, 0);
        strips.push_back({x0, k});
        w = x0;
    }
    for (auto it = strips.rbegin(); it != strips.rend(); ++it) {
        const int k = it->second, th = kConvTH << k;
        for (int y0 = 0; y0 < rows; y0 += th) shaped[k].push_back({l, y0, it->first});
    }
}

// Tiles of the exact 5 x 5 convolution for a launch of `nb` frames (pbd_kernels_conv.hip): the strips of four rows of every
// level of every frame, left to right, form one sequence of positions; a tile takes 64 consecutive positions, in at most
// kConvMaxSeg runs (a run stays inside one strip) -- when a fourth run would be needed the tile ends early.
void build_seg_tiles(const std::vector<LevelDesc> &lv, int nb, std::vector<ConvSegTile> &out)
{
    out.clear();
    ConvSegTile cur{};
    int lanes = 0;
    auto flush = [&]() { if (cur.nseg) out.push_back(cur); cur = ConvSegTile{}; lanes = 0; };
    for (int f = 0; f < nb; ++f)
        for (int l = 0; l < (int)lv.size(); ++l) {
            const int H = lv[l].rows, W = lv[l].cols;
            if (H <= 0 || W <= 0) continue;
            for (int st = 0; st < (H + 3) / 4; ++st)
                for (int x = 0; x < W;) {
                    if (cur.nseg == kConvMaxSeg || lanes == 64) flush();
                    const int take = std::min(W - x, 64 - lanes);
                    cur.len[cur.nseg] = take;
                    cur.seg[cur.nseg] = ConvSeg{f, l, st, x};
                    cur.nseg += 1;
                    lanes += take;
                    x += take;
                }
        }
    flush();
}

hipError_t finish_plan_tables(Plan &P, int sbin)
{
    // flat row / column lookup and conv tiles over the feature maps
    std::vector<int> row2level, rowoff(P.nlevels + 1, 0), col2level, coloff(P.nlevels + 1, 0);
    std::vector<ConvTile> tiles, shaped[3], htiles;
    P.quad_per_frame = 0;
    P.hgroups.clear();
    P.fine = false;
    std::vector<LevelDesc> lv_img;   // the levels of the model's bin size: every level image once
    for (int l = 0; l < P.nlevels; ++l) {
        P.lv[l].quad_off = P.quad_per_frame;
        P.quad_per_frame += ((long long)P.lv[l].rows * P.lv[l].cols + 3) / 4;
        const LevelDesc &d = P.lv[l];
        // the HOG stage's launches: one per run of levels of one bin size (blk1 / tile1 / lv1 grow with the run)
        if (P.hgroups.empty() || P.hgroups.back().sbin != d.sbin)
            P.hgroups.push_back(HogGroup{d.sbin, l, l, (int)htiles.size(), (int)htiles.size(), d.blk_off, d.blk_off});
        if (d.sbin != sbin) P.fine = true;
        else lv_img.push_back(d);
        for (int by0 = 0; by0 < d.blk_rows && d.blk_cols > 0; by0 += hog_tile_rows(d.sbin))
            for (int bx0 = 0; bx0 < d.blk_cols; bx0 += kHogTBX) htiles.push_back({l, by0, bx0});
        HogGroup &g = P.hgroups.back();
        g.lv1 = l + 1; g.tile1 = (int)htiles.size(); g.blk1 = d.blk_off + (long long)d.blk_rows * d.blk_cols;
        rowoff[l] = (int)row2level.size();
        coloff[l] = (int)col2level.size();
        if (d.rows > 0 && d.cols > 0) {
            for (int y = 0; y < d.rows; ++y) row2level.push_back(l);
            for (int x = 0; x < d.cols; ++x) col2level.push_back(l);
            for (int y0 = 0; y0 < d.rows; y0 += kConvTH)
                for (int x0 = 0; x0 < d.cols; x0 += kConvTW) tiles.push_back({l, y0, x0});
            cover_level(l, d.rows, d.cols, shaped);
        }
    }
    {
        int longest = 0;
        for (const LevelDesc &d : P.lv) longest = std::max(longest, std::max(d.rows, d.cols));
        P.ptr8 = longest <= 256;
        P.longest = longest;
    }
    rowoff[P.nlevels] = (int)row2level.size();
    coloff[P.nlevels] = (int)col2level.size();
    P.nrows_flat = (int)row2level.size();
    P.ncols_flat = (int)col2level.size();
    P.ntiles = (int)tiles.size();
    P.nhtiles = (int)htiles.size();
    // wave-private stack regions: a wave of 64 flat rows (columns) needs 64 x ceil(longest row in the wave / 2)
    // two-entry records; levels are ordered large to small, but take the maximum to be safe
    std::vector<long long> srow, scol;
    long long tot_r = 0, tot_c = 0;
    for (int w0 = 0; w0 < P.nrows_flat; w0 += 64) {
        int mx = 0;
        for (int r = w0; r < std::min(w0 + 64, P.nrows_flat); ++r) mx = std::max(mx, P.lv[row2level[r]].cols);
        srow.push_back(tot_r);
        tot_r += 64LL * ((mx + 1) / 2);
    }
    for (int w0 = 0; w0 < P.ncols_flat; w0 += 64) {
        int mx = 0;
        for (int c = w0; c < std::min(w0 + 64, P.ncols_flat); ++c) mx = std::max(mx, P.lv[col2level[c]].rows);
        scol.push_back(tot_c);
        tot_c += 64LL * ((mx + 1) / 2);
    }
    P.stk_per_jf = std::max(tot_r, tot_c);
    std::vector<ConvTile> all;
    for (int k = 0; k < 3; ++k) { P.nshaped[k] = (int)shaped[k].size(); all.insert(all.end(), shaped[k].begin(), shaped[k].end()); }
    hipError_t e;
    if ((e = P.d_stk_row_off.upload(srow)) != hipSuccess) return e;
    if ((e = P.d_stk_col_off.upload(scol)) != hipSuccess) return e;
    if ((e = P.d_lv.upload(P.lv)) != hipSuccess) return e;
    P.nlv_img = 0;
    if (P.fine) {
        P.nlv_img = (int)lv_img.size();
        if ((e = P.d_lv_img.upload(lv_img)) != hipSuccess) return e;
    }
    if ((e = P.d_tiles.upload(tiles)) != hipSuccess) return e;
    if ((e = P.d_shaped.upload(all)) != hipSuccess) return e;
    if ((e = P.d_htiles.upload(htiles)) != hipSuccess) return e;
    if ((e = P.d_row2level.upload(row2level)) != hipSuccess) return e;
    if ((e = P.d_rowoff.upload(rowoff)) != hipSuccess) return e;
    if ((e = P.d_col2level.upload(col2level)) != hipSuccess) return e;
    if ((e = P.d_coloff.upload(coloff)) != hipSuccess) return e;
    return P.d_scales.upload(P.scales);
}

// A finished plan joins the cache; the cache holds at most 16 plans and never evicts the plan the handle's
// resident result refers to.
void cache_plan(pbd_handle *h, std::unique_ptr<Plan> P)
{
    h->plans.push_back(std::move(P));
    while (h->plans.size() > 16) {
        auto it = h->plans.begin();
        if (it->get() == h->res.plan) ++it;
        h->plans.erase(it);
    }
}

// The host side of an image plan (no device work): level table, scales and resize tables of an unsharded rows x cols frame.
// PBD_OK, or PBD_ERR_INVALID / PBD_ERR_UNSUPPORTED with the reason in `err`.
// padx / pady: the padded pyramid (pbd_set_padding) -- every non-empty feature map grows by the pad on each side, and all
// that is derived from level sizes below and in finish_plan_tables follows.
// fine: the fine octave (pbd_set_fine_octave; fineoctave.py states the rule) -- the first nfine = min(interval, n) reference
// levels come a second time, IN FRONT, at bin size sbin / 2 and half the scale.  A fine level owns no image: it shares the one
// of its base level (img_off), so the pyramid does not grow.  Level nfine + l is the reference's level l, unchanged.
int image_plan_host(int rows, int cols, int sbin, int interval, int padx, int pady, bool fine, Plan &Pr, std::string &err)
{
    Plan *P = &Pr;
    char buf[160];
    std::vector<int> lr, lc;
    std::vector<float> scales;
    const int n = plan_pyramid(rows, cols, sbin, interval, lr, lc, scales);
    if (n <= 0) {
        snprintf(buf, sizeof buf, "frame %dx%d too small for sbin %d / interval %d (nscales %d)", rows, cols, sbin, interval, n);
        err = buf;
        return PBD_ERR_INVALID;
    }
    const int nfine = fine ? std::min(interval, n) : 0;
    if (fine && n + nfine > PBD_MAX_LEVELS) {
        snprintf(buf, sizeof buf, "frame %dx%d: %d levels + %d of the fine octave exceed PBD_MAX_LEVELS (%d)", rows, cols, n, nfine, PBD_MAX_LEVELS);
        err = buf;
        return PBD_ERR_UNSUPPORTED;
    }
    P->kind = 0; P->rows = rows; P->cols = cols;
    P->padded = padx != 0 || pady != 0;
    P->nlevels = n + nfine; P->nfine = nfine; P->interval = interval;
    P->scales.resize(n + nfine);
    P->lv.resize(n + nfine);
    std::vector<ResizeTabX> tabx;
    std::vector<ResizeTabY> taby;
    std::vector<ResizeTabXf> tabxf;
    std::vector<ResizeTabYf> tabyf;
    std::vector<long long> img_off(n + 1, 0);
    for (int l = 0; l < n; ++l) img_off[l + 1] = img_off[l] + (long long)lr[l] * lc[l];
    long long blk = 0, cell = 0;
    for (int L = 0; L < n + nfine; ++L) {
        const int l = L < nfine ? L : L - nfine;        // the reference level whose image this level reads
        const int sb = L < nfine ? sbin / 2 : sbin;
        LevelDesc &d = P->lv[L];
        P->scales[L] = L < nfine ? scales[l] / 2 : scales[l];
        d.img_rows = lr[l]; d.img_cols = lc[l];
        if (d.img_rows < 4 || d.img_cols < 4) {
            snprintf(buf, sizeof buf, "pyramid level %d is %dx%d", l, lr[l], lc[l]);
            err = buf;
            return PBD_ERR_INVALID;
        }
        d.sbin = sb;
        d.blk_cols = (int)roundf((float)lc[l] / (float)sb);   // HOGFeatures.cpp:174
        d.blk_rows = (int)roundf((float)lr[l] / (float)sb);
        d.cols = std::max(d.blk_cols - 2, 0);
        d.rows = std::max(d.blk_rows - 2, 0);
        d.padx = d.pady = 0;
        if (d.rows > 0 && d.cols > 0) {   // an empty level is never padded
            d.padx = padx; d.pady = pady;
            d.cols += 2 * padx; d.rows += 2 * pady;
        }
        d.src_level = L >= nfine && l >= interval ? l - interval : -1;
        d.img_off = img_off[l]; d.blk_off = blk; d.cell_off = cell;
        d.tab_x = d.tab_y = 0;
        blk += (long long)d.blk_rows * d.blk_cols;
        cell += (long long)d.rows * d.cols;
        if (L >= nfine && l < interval) {
            // cv::resize INTER_LINEAR coefficient tables (resize_taps_x / _y, pbd_handle.h)
            d.tab_x = (int)tabx.size();
            d.tab_y = (int)taby.size();
            resize_taps_x(cols, lc[l], tabx, tabxf);
            resize_taps_y(rows, lr[l], taby, tabyf);
        }
    }
    P->pix_per_frame = img_off[n]; P->blk_per_frame = blk; P->cell_per_frame = cell;
    P->npix_resized = img_off[std::min(interval, n)];
    P->htabx = std::move(tabx); P->htaby = std::move(taby); P->htabxf = std::move(tabxf); P->htabyf = std::move(tabyf);
    return PBD_OK;
}

// the HOG coordinate table of bin size `sbin` with `need` entries, to `buf`
int upload_coord(pbd_handle *h, int sbin, int need, DevBuf &buf)
{
    // HOGFeatures.cpp:252-259: yp = ((T)y+0.5)/(T)sbin - 0.5; iyp = floor(yp); vy0 = yp-iyp; vy1 = 1.0-vy0
    if (h->f64) {
        std::vector<HogCoordD> coord(need);
        for (int t = 0; t < need; ++t) {
            const double tp = ((double)t + 0.5) / (double)sbin - 0.5;
            const int ip = (int)floor(tp);
            const double v0 = tp - (double)ip;
            coord[t] = {ip, v0, 1.0 - v0};
        }
        HIPCHK(h, buf.ensure(coord.size() * sizeof(HogCoordD)));
        HIPCHK(h, hipMemcpy(buf.p, coord.data(), coord.size() * sizeof(HogCoordD), hipMemcpyHostToDevice));
    } else {
        std::vector<HogCoord> coord(need);
        for (int t = 0; t < need; ++t) {
            const float tp = (float)(((double)(float)t + 0.5) / (double)(float)sbin - 0.5);
            const int ip = (int)floorf(tp);
            const float v0 = tp - (float)ip;
            const float v1 = (float)(1.0 - (double)v0);
            coord[t] = {ip, v0, v1};
        }
        HIPCHK(h, buf.ensure(coord.size() * sizeof(HogCoord)));
        HIPCHK(h, hipMemcpy(buf.p, coord.data(), coord.size() * sizeof(HogCoord), hipMemcpyHostToDevice));
    }
    return PBD_OK;
}

// the HOG coordinate tables grow with the largest frame seen: the model's bin size and, with the fine octave on, half of it
int grow_coord(pbd_handle *h, int rows, int cols)
{
    const int need = std::max(rows, cols) + 4 * h->sbin + 8;
    if (need > h->coord_n) {
        if (int rc = upload_coord(h, h->sbin, need, h->d_coord)) return rc;
        h->coord_n = need;
    }
    if (h->fine_octave && need > h->coord_fine_n) {
        if (int rc = upload_coord(h, h->sbin / 2, need, h->d_coord_fine)) return rc;
        h->coord_fine_n = need;
    }
    return PBD_OK;
}

int get_image_plan(pbd_handle *h, int rows, int cols, Plan **out)
{
    for (auto &p : h->plans)
        if (p->kind == 0 && p->rows == rows && p->cols == cols) { *out = p.get(); return PBD_OK; }
    auto P = std::make_unique<Plan>();
    {
        std::string err;
        if (int rc = image_plan_host(rows, cols, h->sbin, h->interval, h->padx, h->pady, h->fine_octave, *P, err)) return fail(h, rc, "%s", err.c_str());
    }
    const int n = P->nlevels;
    long long blk = P->blk_per_frame, cell = P->cell_per_frame;
    if (h->shard_world > 1) {
        // Level sharding (secondary partitioning): levels are independent through HOG, convolution and DP, so
        // one frame can be split over GPUs by giving each a subset of the levels.  Longest-processing-time assignment
        // over the cell counts (level 0 alone is 13 % of a VGA frame): levels by decreasing size, each to the rank
        // with the least work so far.  Levels of other ranks keep their pyramid image here (a pyrDown chain may run
        // through them) but get empty block / feature maps, so every later stage skips them.
        std::vector<int> order(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            return (long long)P->lv[a].rows * P->lv[a].cols > (long long)P->lv[b].rows * P->lv[b].cols;
        });
        std::vector<long long> load(h->shard_world, 0);
        std::vector<int> owner(n, 0);
        for (int l : order) {
            const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
            owner[l] = r;
            load[r] += (long long)P->lv[l].rows * P->lv[l].cols;
        }
        blk = 0; cell = 0;
        for (int l = 0; l < n; ++l) {
            LevelDesc &d = P->lv[l];
            if (owner[l] != h->shard_rank) d.blk_rows = d.blk_cols = d.rows = d.cols = d.padx = d.pady = 0;
            d.blk_off = blk; d.cell_off = cell;
            blk += (long long)d.blk_rows * d.blk_cols;
            cell += (long long)d.rows * d.cols;
        }
    }
    P->blk_per_frame = blk; P->cell_per_frame = cell;
    HIPCHK(h, P->d_tabx.upload(P->htabx));
    HIPCHK(h, P->d_taby.upload(P->htaby));
    HIPCHK(h, P->d_tabxf.upload(P->htabxf));
    HIPCHK(h, P->d_tabyf.upload(P->htabyf));
    HIPCHK(h, finish_plan_tables(*P, h->sbin));
    if (int rc = grow_coord(h, rows, cols)) return rc;
    *out = P.get();
    cache_plan(h, std::move(P));
    return PBD_OK;
}

int get_dims_plan(pbd_handle *h, int nlevels, const int *rows, const int *cols, Plan **out)
{
    if (nlevels <= 0 || nlevels > PBD_MAX_LEVELS) return fail(h, PBD_ERR_INVALID, "nlevels %d out of range", nlevels);
    std::vector<int> key;
    for (int l = 0; l < nlevels; ++l) {
        if (rows[l] < 0 || cols[l] < 0 || rows[l] > 32000 || cols[l] > 32000)
            return fail(h, PBD_ERR_INVALID, "level %d size %dx%d out of range", l, rows[l], cols[l]);
        key.push_back(rows[l]); key.push_back(cols[l]);
    }
    for (auto &p : h->plans)
        if (p->kind == 1 && p->key_dims == key) { *out = p.get(); return PBD_OK; }
    auto P = std::make_unique<Plan>();
    P->kind = 1; P->key_dims = key; P->nlevels = nlevels; P->interval = h->interval;
    P->padded = h->padx != 0 || h->pady != 0;
    P->lv.resize(nlevels);
    P->scales.assign(nlevels, 1.f);
    long long cell = 0;
    for (int l = 0; l < nlevels; ++l) {
        LevelDesc &d = P->lv[l];
        memset(&d, 0, sizeof d);
        d.rows = rows[l]; d.cols = cols[l]; d.src_level = -1; d.cell_off = cell; d.sbin = h->sbin;
        d.padx = h->padx; d.pady = h->pady;   // the caller's planes are taken to be padded by the handle's setting (the walk's rectangles)
        cell += (long long)rows[l] * cols[l];
    }
    P->cell_per_frame = cell;
    HIPCHK(h, finish_plan_tables(*P, h->sbin));
    *out = P.get();
    cache_plan(h, std::move(P));
    return PBD_OK;
}

// ---- mixed-size plans ----------------------------------------------------------------------------
// Appends frame Q (an unsharded image plan) to the virtual frame M: its levels, scales and resize tables, with every offset
// shifted past the frames already in M.  Host only.
void mixed_append(Plan &M, const Plan &Q)
{
    const int lv0 = M.nlevels, f = M.mixed_frames;
    const int tx0 = (int)M.htabx.size(), ty0 = (int)M.htaby.size();
    if (M.frame_lv0.empty()) M.frame_lv0.push_back(0);
    for (int l = 0; l < Q.nlevels; ++l) {
        LevelDesc d = Q.lv[l];
        d.img_off += M.pix_per_frame; d.blk_off += M.blk_per_frame; d.cell_off += M.cell_per_frame;
        if (d.src_level >= 0) d.src_level += lv0 + Q.nfine;   // (Q's count from its first reference level; M's, from its level 0)
        else { d.tab_x += tx0; d.tab_y += ty0; }
        M.lv.push_back(d);
        M.scales.push_back(Q.scales[l]);
        M.lv_frame.push_back(f);
        M.lv_local.push_back(l);
    }
    M.htabx.insert(M.htabx.end(), Q.htabx.begin(), Q.htabx.end());
    M.htaby.insert(M.htaby.end(), Q.htaby.begin(), Q.htaby.end());
    M.htabxf.insert(M.htabxf.end(), Q.htabxf.begin(), Q.htabxf.end());
    M.htabyf.insert(M.htabyf.end(), Q.htabyf.begin(), Q.htabyf.end());
    M.nlevels += Q.nlevels;
    M.pix_per_frame += Q.pix_per_frame; M.blk_per_frame += Q.blk_per_frame; M.cell_per_frame += Q.cell_per_frame;
    M.frame_lv0.push_back(M.nlevels);
    M.frame_nfine.push_back(Q.nfine);
    M.fdim.push_back(make_int2(Q.rows, Q.cols));
    M.key_dims.push_back(Q.rows); M.key_dims.push_back(Q.cols);
    M.mixed_frames += 1;
    M.padded = M.padded || Q.padded;
}


// After the last mixed_append: the pyramid launches (every frame's resized levels in one, then one per octave over every frame)
// and the post-processing tables.  Host only.
void mixed_finish(Plan &M, int interval)
{
    M.kind = 2; M.interval = interval;
    M.npix_resized = 0;
    int octaves = 0;
    auto base0 = [&](int f) { return M.frame_lv0[f] + M.frame_nfine[f]; };   // the frame's first reference level: fine levels own no image
    for (int f = 0; f < M.mixed_frames; ++f)
        octaves = std::max(octaves, (M.frame_lv0[f + 1] - base0(f) + interval - 1) / interval);
    for (int k = 0; k < octaves; ++k) {
        M.run_lev0.push_back((int)M.run_lev.size());
        M.run_off0.push_back((long long)M.run_off.size());
        long long pix = 0;
        int n = 0;
        for (int f = 0; f < M.mixed_frames; ++f)
            for (int l = base0(f) + k * interval; l < std::min(base0(f) + (k + 1) * interval, M.frame_lv0[f + 1]); ++l) {
                M.run_lev.push_back(l);
                M.run_off.push_back(pix);
                pix += (long long)M.lv[l].img_rows * M.lv[l].img_cols;
                ++n;
            }
        M.run_off.push_back(pix);
        M.run_n.push_back(n);
        M.run_npix.push_back(pix);
    }
    post_canvas_plan(M);
}

}  // namespace

namespace pbd {

// the suppression stage's per-frame tables of a list of frame sizes (M.fdim, M.mixed_frames): each frame's canvas in LDS or at
// its offset in the global workspace.  Host only.
void post_canvas_plan(Plan &M)
{
    M.fcanvas.assign(M.mixed_frames, 0);
    M.post_lds.clear(); M.post_glb.clear();
    M.post_lds_words = M.post_glb_words = 0;
    for (int f = 0; f < M.mixed_frames; ++f) {
        const int r = M.fdim[f].x, c = M.fdim[f].y;
        if (post_canvas_in_lds(r, c)) {
            M.post_lds.push_back(f);
            M.post_lds_words = std::max(M.post_lds_words, post_canvas_words(r, c));
        } else {
            M.post_glb.push_back(f);
            M.fcanvas[f] = (long long)M.post_glb_words;
            M.post_glb_words += post_canvas_words(r, c);
        }
    }
}

}  // namespace pbd

namespace {

// the mixed plan of one call's frame sizes (rows[f] x cols[f], call order), built from the cached image plans of its sizes
int get_mixed_plan(pbd_handle *h, int nframes, const int *rows, const int *cols, Plan **out)
{
    std::vector<int> key;
    for (int f = 0; f < nframes; ++f) { key.push_back(rows[f]); key.push_back(cols[f]); }
    for (auto &p : h->plans)
        if (p->kind == 2 && p->key_dims == key) { *out = p.get(); return PBD_OK; }
    auto M = std::make_unique<Plan>();
    // every frame's tables: those of a cached image plan of its size, else built on the host only (a mixed call never uses an
    // image plan's device tables, and sizes seen only here do not take the equal-size path's places in the plan cache)
    std::map<std::pair<int, int>, std::unique_ptr<Plan>> built;
    for (int f = 0; f < nframes; ++f) {
        const Plan *Q = nullptr;
        for (auto &p : h->plans)
            if (p->kind == 0 && p->rows == rows[f] && p->cols == cols[f]) { Q = p.get(); break; }
        if (!Q) {
            std::unique_ptr<Plan> &B = built[std::make_pair(rows[f], cols[f])];
            if (!B) {
                B = std::make_unique<Plan>();
                std::string err;
                if (int rc = image_plan_host(rows[f], cols[f], h->sbin, h->interval, h->padx, h->pady, h->fine_octave, *B, err))
                    return fail(h, rc, "frame %d: %s", f, err.c_str());
            }
            Q = B.get();
        }
        mixed_append(*M, *Q);
    }
    for (int f = 0; f < nframes; ++f)
        if (int rc = grow_coord(h, rows[f], cols[f])) return rc;
    mixed_finish(*M, h->interval);
    HIPCHK(h, M->d_tabx.upload(M->htabx));
    HIPCHK(h, M->d_taby.upload(M->htaby));
    HIPCHK(h, M->d_tabxf.upload(M->htabxf));
    HIPCHK(h, M->d_tabyf.upload(M->htabyf));
    HIPCHK(h, M->d_lv_frame.upload(M->lv_frame));
    HIPCHK(h, M->d_lv_local.upload(M->lv_local));
    HIPCHK(h, M->d_run_lev.upload(M->run_lev));
    HIPCHK(h, M->d_run_off.upload(M->run_off));
    HIPCHK(h, M->d_fdim.upload(M->fdim));
    HIPCHK(h, M->d_fcanvas.upload(M->fcanvas));
    HIPCHK(h, M->d_post_lds.upload(M->post_lds));
    HIPCHK(h, M->d_post_glb.upload(M->post_glb));
    HIPCHK(h, finish_plan_tables(*M, h->sbin));
    *out = M.get();
    cache_plan(h, std::move(M));
    return PBD_OK;
}

// IEEE binary16 -> float on the host (host_f2h, the other direction: pbd_layout.h)
float host_h2f(uint16_t hv)
{
    const uint32_t sign = (uint32_t)(hv & 0x8000u) << 16;
    const uint32_t ex = (hv >> 10) & 0x1fu, man = hv & 0x3ffu;
    uint32_t u;
    if (ex == 0x1f) u = sign | 0x7f800000u | (man << 13);
    else if (ex != 0) u = sign | ((ex + 112u) << 23) | (man << 13);
    else if (man == 0) u = sign;
    else {                                                                   // subnormal half: normalise
        int sh = 0;
        uint32_t mm = man;
        while (!(mm & 0x400u)) { mm <<= 1; ++sh; }
        u = sign | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ffu) << 13);
    }
    float f; memcpy(&f, &u, 4);
    return f;
}

// ---- model tables --------------------------------------------------------------------------------
// Work items of k_conv3: the nf filters of a size class cut into units of 8 / 6 (and at most one of 4 or 2) filters so that
// `nw` waves taking units largest-first finish together.  156 filters, 6 waves: 6 x 8 + 18 x 6 -- every wave 8 + 6 + 6 + 6.
void conv_units(int nf, int nw, std::vector<int> &f0, std::vector<int> &ql)
{
    const int P = (nf + 1) / 2;                            // filter pairs (an odd bank ends in a padding lane)
    double best = 1e30;
    int ba = 0, bb = 0, bc = 0;
    for (int a = P / 4; a >= 0; --a)
        for (int c = 0; c <= 2; ++c) {                     // c pairs in one last small unit (0: none)
            const int rest = P - 4 * a - c;
            if (rest < 0 || rest % 3) continue;
            const int b = rest / 3;
            // largest-first hand-out to nw equally fast waves; a unit costs its pairs + a fixed overhead (window reads, stores)
            std::vector<double> load(nw, 0.0);
            auto give = [&](int n, double cost) { for (int i = 0; i < n; ++i) *std::min_element(load.begin(), load.end()) += cost; };
            give(a, 4 + 0.2); give(b, 3 + 0.2); if (c) give(1, c + 0.2);
            const double span = *std::max_element(load.begin(), load.end()) + (c ? 0.01 : 0.0);    // ties: no small unit
            if (span < best - 1e-9) { best = span; ba = a; bb = b; bc = c; }
        }
    f0.clear(); ql.clear();
    int f = 0;
    for (int i = 0; i < ba; ++i) { f0.push_back(f); ql.push_back(8); f += 8; }
    for (int i = 0; i < bb; ++i) { f0.push_back(f); ql.push_back(6); f += 6; }
    if (bc) { f0.push_back(f); ql.push_back(2 * bc); f += 2 * bc; }
}

// The dynamic-LDS limit of every convolution kernel that asks for more than the default (the six k_conv_mfma_any and the three
// k_conv_mfma_f64 variants), raised on the CURRENT device: hipFuncSetAttribute acts on that device's copy of a kernel.  Once per
// device and process, never per launch (handles launch concurrently), and before any launch: upload_filters_t calls it and
// reports a failure as its own.
static hipError_t conv_prepare_device()
{
    constexpr int kMaxDevices = 64;
    static std::once_flag once[kMaxDevices];
    static hipError_t result[kMaxDevices];
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;   // (more devices than the flag table holds)
    std::call_once(once[dev], [dev] {
        const hipError_t e = conv_mfma_any_set_lds_limits();
        result[dev] = e ? e : conv_mfma_f64_set_lds_limits();
    });
    return result[dev];
}

// One packed weight table: n entries, entry i = value(i) (a gather from its layout definition, pbd_layout.h), to `buf`
template <typename V, typename Fn>
hipError_t upload_table(DevBuf &buf, long long n, Fn &&value)
{
    std::vector<V> tab((size_t)n);
    for (size_t i = 0; i < tab.size(); ++i) tab[i] = value((long long)i);
    if (hipError_t e = buf.ensure(tab.size() * sizeof(V))) return e;
    return hipMemcpy(buf.p, tab.data(), tab.size() * sizeof(V), hipMemcpyHostToDevice);
}

template <typename R>
int upload_filters_t(pbd_handle *h, int nfilters, const void *const *filters, const int *ksize)
{
    if (nfilters <= 0) return fail(h, PBD_ERR_INVALID, "no filters");
    for (int f = 0; f < nfilters; ++f)
        if (ksize[f] < 1 || ksize[f] > kConvMaxK) return fail(h, PBD_ERR_UNSUPPORTED, "filter %d: size %d not supported (1..%d)", f, ksize[f], kConvMaxK);
    // size classes in order of first appearance
    std::vector<int> sizes;
    for (int f = 0; f < nfilters; ++f)
        if (std::find(sizes.begin(), sizes.end(), ksize[f]) == sizes.end()) sizes.push_back(ksize[f]);
    const int K = ksize[0];
    const bool fast = (sizeof(R) == 4 && K == 5 && sizes.size() == 1);
    const bool mfma = conv_is_matrix_f32(h->cfg.conv_mode), any = conv_is_any(h->cfg.conv_mode), f16 = conv_is_f16(h->cfg.conv_mode);
    if (mfma && !any && !fast) return fail(h, PBD_ERR_UNSUPPORTED, "PBD_CONV_MFMA / PBD_CONV_MFMA_F16 need 5x5 filters and PBD_REAL_F32");
    const bool frags = any && !fast;     // (float handles only: pbd_create refuses the modes for PBD_REAL_F64) per-class A-fragments of k_conv_mfma_any; an all-5x5 bank keeps the records of modes 2 / 3
    // The new bank is built beside the old one and moved in only when every upload has succeeded: a failed setFilters()
    // (out of memory, an unsupported size) leaves the handle with its previous, complete bank.
    std::vector<pbd_handle::ConvClass> classes(sizes.size());
    DevBuf wrec;
    for (size_t ci = 0; ci < sizes.size(); ++ci) {
        pbd_handle::ConvClass &C = classes[ci];
        C.K = sizes[ci];
        std::vector<int> ids;
        for (int f = 0; f < nfilters; ++f) if (ksize[f] == C.K) ids.push_back(f);
        C.nf = (int)ids.size();
        C.Fpad = (C.nf + kConvQ - 1) / kConvQ * kConvQ;
        // device layout: float 5x5 kernel [group][channel][tap][8] (800 contiguous bytes per (group, channel));
        // generic kernel (other sizes, T=double) [channel][tap][Fpad]
        const bool fast5 = (sizeof(R) == 4 && C.K == 5);
        const int KK = C.K * C.K;
        // (every table below is filled in gather form from its one layout definition, pbd_layout.h: the in-place model update's
        // kernels fill the same tables from the same definitions)
        std::vector<R> w((size_t)generic_bank_size(KK, C.Fpad), (R)0);
        for (size_t i = 0; i < w.size(); ++i) {
            const WeightSrc s = fast5 ? group_bank_source((long long)i, KK, C.nf) : generic_bank_source((long long)i, KK, C.Fpad, C.nf);
            if (s.f >= 0) w[i] = static_cast<const R *>(filters[ids[s.f]])[weight_at(s)];
        }
        HIPCHK(h, C.wts.ensure(w.size() * sizeof(R)));
        HIPCHK(h, hipMemcpy(C.wts.p, w.data(), w.size() * sizeof(R), hipMemcpyHostToDevice));
        if (sizes.size() > 1) HIPCHK(h, C.fmap.upload(ids));
        if (fast5) {
            std::vector<int> uf0, uql;
            conv_units(C.nf, kConv3NW, uf0, uql);
            C.nunits = (int)uf0.size();
            std::vector<int> uoff(C.nunits, 0);
            size_t tot = 0;
            for (int u = 0; u < C.nunits; ++u) { uoff[u] = (int)tot; tot += (size_t)unit_size(KK, uql[u]); }
            std::vector<float> w3(tot + 16, 0.0f);       // (slack: the last tap row is fetched once more past the last channel)
            for (int u = 0; u < C.nunits; ++u)
                for (long long r = 0; r < unit_size(KK, uql[u]); ++r) {
                    const WeightSrc s = unit_source(r, KK, uf0[u], uql[u], C.nf);
                    if (s.f >= 0) w3[uoff[u] + r] = (float)static_cast<const R *>(filters[ids[s.f]])[weight_at(s)];
                }
            HIPCHK(h, C.unit_woff.upload(uoff));
            // channel 31 of a window that leaves the image: the reference's sum over the out-of-image taps (border value 1,
            // src/SpatialConvolutionEngine.cpp:147-156) in its tap order (raster, zero weights skipped: src/filter.cpp:3818-3856,
            // 3916-3922), for every combination of rows / columns outside at the top, bottom, left and right (0..2 each)
            C.c31stride = (C.nf + 15) & ~7;                     // a unit's 8 consecutive entries stay inside the row
            std::vector<float> tab((size_t)81 * C.c31stride, 0.0f);
            for (int cs = 0; cs < 81; ++cs) {
                for (int fl = 0; fl < C.nf; ++fl) {
                    const R *src = static_cast<const R *>(filters[ids[fl]]);
                    float sum = 0.0f;
                    for (int i = 0; i < 5; ++i)
                        for (int j = 0; j < 5; ++j) {
                            if (!c31_tap_outside(cs, i, j)) continue;
                            const float w = (float)src[(size_t)(i * 5 + j) * 32 + 31];
                            if (w != 0.0f) sum = sum + w;
                        }
                    tab[(size_t)cs * C.c31stride + fl] = sum;
                }
            }
            HIPCHK(h, C.c31tab.upload(tab));
            HIPCHK(h, C.wts3.ensure(w3.size() * sizeof(float)));
            HIPCHK(h, hipMemcpy(C.wts3.p, w3.data(), w3.size() * sizeof(float), hipMemcpyHostToDevice));
            HIPCHK(h, C.unit_f0.upload(uf0));
            HIPCHK(h, C.unit_ql.upload(uql));
        }
        if (h->cfg.conv_mode == PBD_CONV_MFMA_F64) {
            // A-fragments in the order k_conv_mfma_f64 reads them (f64_frag_source: lane group g supplies channels g QN ..
            // g QN + QN - 1 of its cell); filters past nf are zero
            const int QN = conv_mfma_f64_qn(C.K);
            const int mtiles = (C.nf + 15) / 16, passes = mfma_passes(mtiles);
            HIPCHK(h, conv_prepare_device());
            HIPCHK(h, upload_table<double>(C.wfrag64, f64_frag_size(KK, mtiles), [&](long long o) {
                const WeightSrc s = f64_frag_source(o, KK, QN, mtiles, passes, C.nf);
                return s.f >= 0 ? (double)static_cast<const R *>(filters[ids[s.f]])[weight_at(s)] : 0.0;
            }));
        }
        if (frags) {
            // 16-bit A-fragments in the order k_conv_mfma_any reads them (any_frag_source), rounded as the records of modes
            // 2 / 3 are (wrec_value); pad taps and filters past nf stay zero
            const int NV = f16 ? 1 : 2, CB = conv_mfma_any_cb(C.K, f16);
            HIPCHK(h, conv_prepare_device());
            HIPCHK(h, upload_table<uint16_t>(C.wfrag16, any_frag_size(KK, CB, NV, C.nf), [&](long long o) {
                int part = 0;
                const WeightSrc s = any_frag_source(o, KK, CB, NV, C.nf, &part);
                if (s.f < 0) return (uint16_t)0;
                return wrec_value((float)static_cast<const R *>(filters[ids[s.f]])[weight_at(s)], f16, part);
            }));
        }
    }
    const int Fpad = (nfilters + kConvQ - 1) / kConvQ * kConvQ;
    if (mfma && !frags) {
        // bf16 mode: x = hi + lo with round-to-nearest-even; fp16 mode: one rounding (wrec_value).  A-operand fragments in the
        // order the kernel consumes them (wrec_source)
        const int NV = f16 ? 1 : 2;
        HIPCHK(h, upload_table<uint16_t>(wrec, wrec_size(K * K, NV, nfilters), [&](long long i) {
            int part = 0;
            const WeightSrc s = wrec_source(i, K * K, NV, nfilters, &part);
            return s.f >= 0 ? wrec_value(reinterpret_cast<const float *>(filters[s.f])[weight_at(s)], f16, part) : (uint16_t)0;
        }));
    }
    // commit
    h->conv_classes = std::move(classes);
    if (mfma) h->d_wrec = std::move(wrec);
    h->F = nfilters; h->Fpad = Fpad; h->ksize = K;
    h->filter_ksize.assign(ksize, ksize + nfilters);
    h->filters_set = true;
    return PBD_OK;
}

int upload_filters(pbd_handle *h, int nfilters, const void *const *filters, const int *ksize)
{
    return h->f64 ? upload_filters_t<double>(h, nfilters, filters, ksize) : upload_filters_t<float>(h, nfilters, filters, ksize);
}

// After pbd_conv_set_filters replaced the bank: the model tables built by build_model index response planes by
// filter id, and the part boxes of argmin use the filter size (include/Parts.hpp:185-187), so both are re-checked /
// rebuilt against the new bank.  A bank that does not cover the model's ids leaves the convolution engine usable on
// its own (IConvolutionEngine::pdf) and makes the model-dependent calls fail with PBD_ERR_STATE.
int revalidate_bank(pbd_handle *h)
{
    h->bank_matches_model = true;
    for (int f : h->filterid)
        if (f < 0 || f >= h->F) { h->bank_matches_model = false; return PBD_OK; }
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
        for (int p = 0; p < np; ++p) {
            PartWalk &w = h->walk[h->walk_off[c] + p];
            const int K = h->mix_offset[p0 + p + 1] - h->mix_offset[p0 + p];
            for (int mm = 0; mm < K; ++mm) w.ksize[mm] = h->filter_ksize[h->filterid[h->mix_offset[p0 + p] + mm]];
        }
    }
    HIPCHK(h, h->d_walk.upload(h->walk));
    return PBD_OK;
}

int build_model(pbd_handle *h, const pbd_model *m)
{
    if (m->flen != 32 || m->norient != 18)
        return fail(h, PBD_ERR_UNSUPPORTED, "flen %d / norient %d: only 32 / 18 are supported", m->flen, m->norient);
    if (m->ncomponents < 1 || m->nfilters < 1 || m->sbin < 2 || m->interval < 1)
        return fail(h, PBD_ERR_INVALID, "bad model header");
    h->NC = m->ncomponents; h->sbin = m->sbin; h->interval = m->interval; h->norient = m->norient;
    h->thresh = m->thresh;
    const int totparts = m->part_offset[m->ncomponents];
    const int totmix = m->mix_offset[totparts];
    h->part_offset.assign(m->part_offset, m->part_offset + m->ncomponents + 1);
    h->parentid.assign(m->parentid, m->parentid + totparts);
    h->mix_offset.assign(m->mix_offset, m->mix_offset + totparts + 1);
    h->filterid.assign(m->filterid, m->filterid + totmix);
    h->biasid.assign(m->biasid, m->biasid + totmix);
    h->defid.assign(m->defid, m->defid + totmix);
    h->biasw.assign(m->biasw, m->biasw + m->nbias);
    h->defw.assign(m->defw, m->defw + (size_t)m->ndefs * 4);
    h->anchors.assign(m->anchors, m->anchors + (size_t)m->ndefs * 2);

    // filters
    {
        if (h->f64 ? !m->filters_f64 : !m->filters_f32) return fail(h, PBD_ERR_INVALID, "model has no filters of the requested real type");
        std::vector<const void *> fp(m->nfilters);
        for (int f = 0; f < m->nfilters; ++f)
            fp[f] = h->f64 ? static_cast<const void *>(m->filters_f64 + m->filter_offset[f])
                           : static_cast<const void *>(m->filters_f32 + m->filter_offset[f]);
        if (int rc = upload_filters(h, m->nfilters, fp.data(), m->filter_ksize)) return rc;
    }

    // validation + pointer slots + depth
    h->ptr_slot.assign(totparts, 0);
    std::vector<int> depth(totparts, 0);
    int NS = 0, maxdepth = 0;
    h->max_parts = 0;
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
        if (np < 1) return fail(h, PBD_ERR_INVALID, "component %d has no parts", c);
        h->max_parts = std::max(h->max_parts, np);
        std::set<int> seen;
        for (int p = 0; p < np; ++p) {
            const int gp = p0 + p, par = h->parentid[gp];
            const int K = h->mix_offset[gp + 1] - h->mix_offset[gp];
            if (K < 1 || K > kMaxMix) return fail(h, PBD_ERR_UNSUPPORTED, "part %d has %d mixtures (1..%d supported)", p, K, kMaxMix);
            h->max_mix = std::max(h->max_mix, K);
            if ((p == 0) != (par < 0) || par >= p) return fail(h, PBD_ERR_INVALID, "part %d: parent %d breaks topological order", p, par);
            for (int mm = 0; mm < K; ++mm) {
                const int f = h->filterid[h->mix_offset[gp] + mm];
                if (f < 0 || f >= h->F) return fail(h, PBD_ERR_INVALID, "filter id %d out of range", f);
                if (!seen.insert(f).second) h->seq_mode = true;   // accumulators keyed by filter id interact: see below
            }
            h->ptr_slot[gp] = NS;
            if (p > 0) {
                const int gpar = p0 + par;
                const int L = h->mix_offset[gpar + 1] - h->mix_offset[gpar];
                NS += L;
                depth[gp] = depth[gpar] + 1;
                maxdepth = std::max(maxdepth, depth[gp]);
                for (int mm = 0; mm < K; ++mm) {
                    const int gm = h->mix_offset[gp] + mm;
                    const int d = h->defid[gm], b = h->biasid[gm];
                    if (d < 0 || d >= m->ndefs) return fail(h, PBD_ERR_INVALID, "defid %d out of range", d);
                    if (b < 0 || b + L > m->nbias) return fail(h, PBD_ERR_INVALID, "biasid %d out of range", b);
                    if (h->defw[(size_t)d * 4 + 0] == 0.f || h->defw[(size_t)d * 4 + 2] == 0.f)
                        return fail(h, PBD_ERR_INVALID, "deformation %d has a zero quadratic term", d);
                }
            } else {
                const int b = h->biasid[h->mix_offset[gp]];
                if (b < 0 || b >= m->nbias) return fail(h, PBD_ERR_INVALID, "root biasid %d out of range", b);
            }
        }
    }
    if (h->max_parts > kWalkMaxParts) return fail(h, PBD_ERR_UNSUPPORTED, "%d parts per component (max %d)", h->max_parts, kWalkMaxParts);
    h->NS = NS;

    // children (descending index) per part
    std::vector<std::vector<int>> children(totparts);
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
        for (int p = np - 1; p > 0; --p) children[p0 + h->parentid[p0 + p]].push_back(p0 + p);
    }

    h->groups.clear();
    h->JGmax = 0;
    h->NM = totmix;
    h->totmix = totmix;
    auto dt_job = [&](int gm, bool from_acc, int plane) {
        DtJob j{};
        j.from_acc = from_acc ? 1 : 0;
        j.plane = plane;
        j.gm = gm;
        const int d = h->defid[gm];
        set_quadratics(j, &h->defw[(size_t)d * 4]);
        j.osx = h->anchors[(size_t)d * 2]; j.osy = h->anchors[(size_t)d * 2 + 1];
        return j;
    };
    std::vector<std::vector<char>> touched(h->NC, std::vector<char>(h->F, 0));   // sequential schedule: accumulator (c, f) exists
    if (h->seq_mode) {
        // The reference's own order (src/DynamicProgram.cpp:95): parts nparts-1 .. 1, one step per part; the
        // accumulated scores live in planes keyed by (component, filter id) as its `ncscores` (:93,115-119,154-156).
        // Step s takes part np-1-s of every component (components are independent).
        h->NM = h->NC * h->F;
        for (int sidx = 0; sidx + 1 < h->max_parts; ++sidx) {
            Group g;
            for (int c = 0; c < h->NC; ++c) {
                const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
                const int p = np - 1 - sidx;
                if (p < 1) continue;
                const int gp = p0 + p, gpar = p0 + h->parentid[gp];
                const int K = h->mix_offset[gp + 1] - h->mix_offset[gp], L = h->mix_offset[gpar + 1] - h->mix_offset[gpar];
                SeqCombineJob sj{};
                sj.job_begin = (int)g.jobs.size(); sj.nmix = K; sj.slot = h->ptr_slot[gp]; sj.npar = L;
                for (int mm = 0; mm < K; ++mm) {
                    const int gm = h->mix_offset[gp] + mm, f = h->filterid[gm];
                    g.jobs.push_back(dt_job(gm, touched[c][f] != 0, touched[c][f] ? c * h->F + f : f));   // score_in, :115-119
                    sj.bias_off[mm] = h->biasid[gm];
                }
                for (int pm = 0; pm < L; ++pm) {
                    const int fp = h->filterid[h->mix_offset[gpar] + pm];
                    sj.target[pm] = c * h->F + fp; sj.filter[pm] = fp;
                    sj.init[pm] = touched[c][fp] ? 0 : 1;
                    touched[c][fp] = 1;
                }
                g.sjobs.push_back(sj);
            }
            h->JGmax = std::max(h->JGmax, (int)g.jobs.size());
            h->groups.push_back(std::move(g));
        }
    }
    // depth groups, deepest first: DT jobs of the parts at depth `dep`, combine jobs of their parents
    for (int dep = h->seq_mode ? 0 : maxdepth; dep >= 1; --dep) {
        Group g;
        std::vector<int> job_begin_of(totparts, -1);
        for (int c = 0; c < h->NC; ++c) {
            const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
            for (int p = 1; p < np; ++p) {
                const int gp = p0 + p;
                if (depth[gp] != dep) continue;
                const int K = h->mix_offset[gp + 1] - h->mix_offset[gp];
                job_begin_of[gp] = (int)g.jobs.size();
                for (int mm = 0; mm < K; ++mm) {
                    const int gm = h->mix_offset[gp] + mm;
                    g.jobs.push_back(dt_job(gm, !children[gp].empty(), children[gp].empty() ? h->filterid[gm] : gm));
                }
            }
            // parents at depth dep-1 whose children (all at depth dep) were just listed
            for (int p = 0; p < np; ++p) {
                const int gpar = p0 + p;
                if (depth[gpar] != dep - 1 || children[gpar].empty()) continue;
                const int L = h->mix_offset[gpar + 1] - h->mix_offset[gpar];
                CombineJob cj{};
                cj.npar = L; cj.acc_plane = h->mix_offset[gpar];
                for (int pm = 0; pm < L; ++pm) cj.filter[pm] = h->filterid[h->mix_offset[gpar] + pm];
                cj.child_begin = (int)g.childs.size();
                for (int ch : children[gpar]) {   // already in descending index order
                    ChildDesc cd{};
                    cd.job_begin = job_begin_of[ch];
                    cd.nmix = h->mix_offset[ch + 1] - h->mix_offset[ch];
                    cd.slot = h->ptr_slot[ch];
                    for (int mm = 0; mm < cd.nmix; ++mm) cd.bias_off[mm] = h->biasid[h->mix_offset[ch] + mm];
                    g.childs.push_back(cd);
                }
                cj.child_end = (int)g.childs.size();
                g.cjobs.push_back(cj);
            }
        }
        h->JGmax = std::max(h->JGmax, (int)g.jobs.size());
        h->groups.push_back(std::move(g));
    }
    for (auto &g : h->groups) {
        HIPCHK(h, g.d_jobs.upload(g.jobs));
        set_variant_flags(g);
        HIPCHK(h, g.d_childs.upload(g.childs));
        HIPCHK(h, g.d_cjobs.upload(g.cjobs));
        HIPCHK(h, g.d_sjobs.upload(g.sjobs));
    }
    h->rjobs.assign(h->NC, RootJob{});
    h->walk.clear(); h->walk_off.assign(h->NC + 1, 0);
    for (int c = 0; c < h->NC; ++c) {
        const int p0 = h->part_offset[c], np = h->part_offset[c + 1] - p0;
        RootJob &r = h->rjobs[c];
        r.nmix = h->mix_offset[p0 + 1] - h->mix_offset[p0];
        r.from_acc = 0;
        for (int mm = 0; mm < r.nmix; ++mm) {
            const int f = h->filterid[h->mix_offset[p0] + mm];
            const bool acc = h->seq_mode ? touched[c][f] != 0 : !children[p0].empty();
            if (acc) r.from_acc |= 1 << mm;
            r.plane[mm] = !acc ? f : h->seq_mode ? c * h->F + f : h->mix_offset[p0] + mm;
        }
        r.bias = h->biasw[h->biasid[h->mix_offset[p0]]];
        h->walk_off[c] = (int)h->walk.size();
        for (int p = 0; p < np; ++p) {
            PartWalk w{};
            w.parent = h->parentid[p0 + p];
            w.slot = h->ptr_slot[p0 + p];
            w.mix0 = h->mix_offset[p0 + p];
            const int K = h->mix_offset[p0 + p + 1] - h->mix_offset[p0 + p];
            for (int mm = 0; mm < K; ++mm) w.ksize[mm] = m->filter_ksize[h->filterid[h->mix_offset[p0 + p] + mm]];
            h->walk.push_back(w);
        }
    }
    h->walk_off[h->NC] = (int)h->walk.size();
    HIPCHK(h, h->d_rjobs.upload(h->rjobs));
    HIPCHK(h, h->d_walk.upload(h->walk));
    HIPCHK(h, h->d_walk_off.upload(h->walk_off));
    HIPCHK(h, h->d_biasw.upload(h->biasw));

    // the model vector (pbd_model_vector) and the strides of an example (pbd_examples*)
    h->nbias = m->nbias; h->ndefs = m->ndefs;
    h->model_ksize.assign(m->filter_ksize, m->filter_ksize + m->nfilters);
    const long long fbase = (long long)m->nbias + 4LL * m->ndefs;
    long long len = fbase;
    h->model_foff.assign(m->nfilters, 0);
    for (int f = 0; f < m->nfilters; ++f) {
        if (m->filter_offset[f] < 0) return fail(h, PBD_ERR_INVALID, "filter %d: negative filter_offset", f);
        h->model_foff[f] = m->filter_offset[f];
        len = std::max(len, fbase + m->filter_offset[f] + (long long)m->filter_ksize[f] * m->filter_ksize[f] * 32);
    }
    if (len > INT32_MAX) return fail(h, PBD_ERR_UNSUPPORTED, "model vector of %lld values (at most 2^31 - 1)", len);
    h->mvec.assign((size_t)len * h->rs, 0);
    auto put = [&](long long o, double v) {
        if (h->f64) reinterpret_cast<double *>(h->mvec.data())[o] = v;
        else reinterpret_cast<float *>(h->mvec.data())[o] = (float)v;
    };
    for (int b = 0; b < m->nbias; ++b) put(b, m->biasw[b]);
    for (long long i = 0; i < 4LL * m->ndefs; ++i) put(m->nbias + i, m->defw[i]);
    for (int f = 0; f < m->nfilters; ++f) {
        const long long n = (long long)m->filter_ksize[f] * m->filter_ksize[f] * 32;
        for (long long i = 0; i < n; ++i)
            put(fbase + m->filter_offset[f] + i, h->f64 ? m->filters_f64[m->filter_offset[f] + i] : (double)m->filters_f32[m->filter_offset[f] + i]);
    }
    h->ex_hdr_words = 4 + 2 * (3 * h->max_parts - 1);
    long long vmax = 0;
    for (int c = 0; c < h->NC; ++c) {
        long long v = 0;
        for (int gp = h->part_offset[c]; gp < h->part_offset[c + 1]; ++gp) {
            int kmax = 0;
            for (int gm = h->mix_offset[gp]; gm < h->mix_offset[gp + 1]; ++gm) kmax = std::max(kmax, m->filter_ksize[h->filterid[gm]]);
            v += 1 + (gp > h->part_offset[c] ? 4 : 0) + (long long)kmax * kmax * 32;
        }
        vmax = std::max(vmax, v);
    }
    if (vmax > INT32_MAX / 2) return fail(h, PBD_ERR_UNSUPPORTED, "an example of %lld values", vmax);
    h->ex_values = (int)((vmax + 3) / 4 * 4);
    return PBD_OK;
}

// ---- stages --------------------------------------------------------------------------------------
// alloc_* size the grow-only workspace for `nframes`; launch_* enqueue the kernels for frames
// [f0, f0+nb) on stream `st` (no allocation, no synchronisation inside).
int alloc_features(pbd_handle *h, Plan &P, int nframes, int cn, int depth)
{
    HIPCHK(h, h->pyr.ensure((size_t)nframes * P.pix_per_frame * cn * depth_size(depth) + 32));   // slack: 8-bit pixels are read with 4- and 16-byte loads
    HIPCHK(h, h->gmag.ensure((size_t)nframes * P.pix_per_frame * h->rs));
    HIPCHK(h, h->gori.ensure((size_t)nframes * P.pix_per_frame + 16));
    HIPCHK(h, h->hist.ensure((size_t)nframes * P.blk_per_frame * 18 * h->rs));
    HIPCHK(h, h->norm.ensure((size_t)nframes * P.blk_per_frame * h->rs));
    HIPCHK(h, h->feat.ensure(std::max<size_t>((size_t)nframes * P.cell_per_frame * 32 * h->rs, 16)));
    return PBD_OK;
}

void launch_hog_stage(pbd_handle *h, Plan &P, int cn, int depth, int f0, int nb, hipStream_t st);

void launch_features(pbd_handle *h, Plan &P, const void *d_frames, int cn, int depth, int f0, int nb, hipStream_t st)
{
    PyrParams pp{};
    // the pyramid kernels see the reference levels alone (LevelDesc::src_level counts from there): fine levels own no image
    const LevelDesc *lvb = P.lv.data() + P.nfine;
    const int nbase = P.nlevels - P.nfine;
    pp.lv = P.d_lv.p + P.nfine; pp.nlevels = nbase; pp.interval = std::min(P.interval, nbase); pp.cn = cn; pp.frame0 = f0;
    pp.pix_per_frame = P.pix_per_frame; pp.pyr = h->pyr.as<uint8_t>(); pp.frames = static_cast<const uint8_t *>(d_frames);
    pp.rows = P.rows; pp.cols = P.cols; pp.tabx = P.d_tabx.p; pp.taby = P.d_taby.p;
    pp.depth = depth; pp.tabxf = P.d_tabxf.p; pp.tabyf = P.d_tabyf.p;
    {
        ProfScope ps(h, PBD_K_RESIZE, st);
        launch_resize(pp, nb, P.npix_resized, st);
    }
    for (int first = P.interval; first < nbase; first += P.interval) {
        const int last = std::min(first + P.interval, nbase);
        const long long base = lvb[first].img_off;
        const long long end = (last < nbase) ? lvb[last].img_off : P.pix_per_frame;
        ProfScope ps(h, PBD_K_PYRDOWN, st);
        launch_pyrdown_range(pp, nb, first, last, base, end - base, st);
    }
    launch_hog_stage(h, P, cn, depth, f0, nb, st);
}

void launch_hog_stage(pbd_handle *h, Plan &P, int cn, int depth, int f0, int nb, hipStream_t st)
{
    HogParams hp{};
    hp.lv = P.d_lv.p; hp.nlevels = P.nlevels; hp.cn = cn; hp.sbin = h->sbin; hp.frame0 = f0;
    hp.pix_per_frame = P.pix_per_frame; hp.blk_per_frame = P.blk_per_frame; hp.cell_per_frame = P.cell_per_frame;
    hp.pyr = h->pyr.as<uint8_t>(); hp.depth = depth; hp.coord = h->d_coord.p;
    hp.gmag = h->gmag.p; hp.gori = h->gori.as<uint8_t>();
    hp.hist = h->hist.p; hp.norm = h->norm.p; hp.feat = h->feat.p;
    {
        // one launch per bin size (Plan::hgroups; one group unless the plan has a fine octave); the groups that do not take the
        // fused kernel share ONE pass 1 over the level images
        ProfScope ps(h, PBD_K_HOG_HIST, st);
        bool grad = false;
        for (const HogGroup &g : P.hgroups) {
            HogParams gp = hp;
            gp.sbin = g.sbin; gp.coord = g.sbin == h->sbin ? h->d_coord.p : h->d_coord_fine.p;
            gp.htiles = P.d_htiles.p + g.tile0; gp.nhtiles = g.tile1 - g.tile0;
            gp.lv0 = g.lv0; gp.lv1 = g.lv1; gp.blk0 = g.blk0; gp.blk1 = g.blk1;
            const bool fused = hog_fused(gp, h->f64) && !h->hog_two_pass;
            if (!fused && !grad) {
                HogParams ip = hp;
                if (P.fine) { ip.lv = P.d_lv_img.p; ip.nlevels = P.nlv_img; }
                launch_hog_grad(ip, nb, h->f64, st);
                grad = true;
            }
            launch_hog_hist(gp, nb, h->f64, fused, P.hgroups.size() > 1, st);
        }
    }
    {
        ProfScope ps(h, PBD_K_HOG_FEAT, st);
        launch_hog_feat(hp, nb, h->f64, P.padded, st);
    }
}

// the pyramid and HOG features of a mixed plan's virtual frame; d_fd = the call's FrameDesc table (device)
void launch_features_mixed(pbd_handle *h, Plan &P, const FrameDesc *d_fd, int cn, int depth, hipStream_t st)
{
    PyrParams pp{};
    pp.lv = P.d_lv.p; pp.nlevels = P.nlevels; pp.interval = P.interval; pp.cn = cn; pp.frame0 = 0;
    pp.pyr = h->pyr.as<uint8_t>();
    pp.tabx = P.d_tabx.p; pp.taby = P.d_taby.p; pp.depth = depth; pp.tabxf = P.d_tabxf.p; pp.tabyf = P.d_tabyf.p;
    pp.fd = d_fd; pp.lv_frame = P.d_lv_frame.p;
    for (size_t k = 0; k < P.run_n.size(); ++k) {
        pp.run_lev = P.d_run_lev.p + P.run_lev0[k];
        pp.run_off = P.d_run_off.p + P.run_off0[k];
        pp.nruns = P.run_n[k];
        pp.pix_per_frame = P.run_npix[k];   // the launch's pixel count
        if (k == 0) { ProfScope ps(h, PBD_K_RESIZE, st); launch_resize_runs(pp, st); }
        else { ProfScope ps(h, PBD_K_PYRDOWN, st); launch_pyrdown_runs(pp, st); }
    }
    launch_hog_stage(h, P, cn, depth, 0, 1, st);
}

int ensure_seg_tiles(pbd_handle *h, Plan &P, int nb)
{
    if (nb < 1 || P.segtiles.count(nb)) return PBD_OK;
    std::vector<ConvSegTile> tiles;
    build_seg_tiles(P.lv, nb, tiles);
    DevTable<ConvSegTile> t;
    HIPCHK(h, t.upload(tiles));
    P.segtiles[nb] = std::move(t);
    return PBD_OK;
}

int alloc_conv(pbd_handle *h, Plan &P, int nframes)
{
    if (!h->filters_set) return fail(h, PBD_ERR_STATE, "pdf() before setFilters()");
    HIPCHK(h, h->resp.ensure(std::max<size_t>((size_t)nframes * P.cell_per_frame * h->F * h->resp_es, 16) + 32));   // + slack: 16-half chunk reads
    return PBD_OK;
}

void launch_conv_stage(pbd_handle *h, Plan &P, int f0, int nb, hipStream_t st)
{
    ConvParams cp{};
    cp.lv = P.d_lv.p; cp.tiles = P.d_tiles.p; cp.ntiles = P.ntiles;
    cp.shaped = P.d_shaped.p;
    for (int k = 0; k < 3; ++k) cp.nshaped[k] = P.nshaped[k];
    cp.segtiles = nullptr; cp.nsegtiles = 0;
    if (!h->f64 && !conv_is_matrix_f32(h->cfg.conv_mode)) {
        const auto it = P.segtiles.find(nb);     // built by ensure_seg_tiles before the first launch of this many frames
        if (it != P.segtiles.end()) { cp.segtiles = it->second.p; cp.nsegtiles = (int)it->second.size; }
    }
    cp.F = h->F; cp.frame0 = f0;
    cp.cell_per_frame = P.cell_per_frame;
    cp.feat = h->feat.p; cp.resp = h->resp.p;
    cp.fma = h->cfg.conv_mode == PBD_CONV_FMA;
    cp.c31_zero = h->res.c31_zero ? 1 : 0;
    ProfScope ps(h, PBD_K_CONV, st);
    for (const pbd_handle::ConvClass &C : h->conv_classes) {     // one launch per filter size (one class in every known model)
        cp.nf = C.nf; cp.Fpad = C.Fpad; cp.ksize = C.K; cp.wts = C.wts.p; cp.fmap = C.fmap.p;
        const int ngroups = C.Fpad / kConvQ;
        // few workgroups (single frame): split the filter groups over more workgroups to fill the chip
        const long long wgs = (long long)P.ntiles * nb;
        cp.groups_per_block = wgs >= 1024 ? ngroups : std::max(1, (int)(ngroups * wgs / 1024));
        {   // Channels of the haloed tile staged in LDS at a time (generic kernel).  All 32 staged once is the least work, but 110 KB
            // (T = double, 5 x 5) leaves ONE workgroup -- one wave per SIMD -- on a CU and the kernel then waits for its own LDS
            // reads: the largest block within 36 KB (four or more workgroups per CU) is taken, restaged per filter group.
            // Measured, one 640x480 frame, T = double: 9.84 ms with 32 channels -> see profiles/README.md.
            const size_t plane = (size_t)(((kConvTH + C.K - 1) * (kConvTW + C.K - 1)) | 1) * h->rs;
            cp.cblock = 32;
            while (cp.cblock > 1 && cp.cblock * plane > kConvLdsBudget) cp.cblock /= 2;
        }
        cp.wts3 = C.wts3.p;
        cp.unit_f0 = C.unit_f0.p; cp.unit_ql = C.unit_ql.p; cp.unit_woff = C.unit_woff.p; cp.nunits = C.nunits;
        cp.c31tab = C.c31tab.p; cp.c31stride = C.c31stride;
        cp.units_per_block = wgs >= 1024 ? std::max(C.nunits, 1) : std::max(1, (int)((long long)C.nunits * wgs / 1024));
        if (conv_is_matrix_f32(h->cfg.conv_mode) && C.wfrag16.p)
            launch_conv_mfma_any(cp, C.wfrag16.p, conv_is_f16(h->cfg.conv_mode), nb, st);
        else if (conv_is_matrix_f32(h->cfg.conv_mode))
            launch_conv_mfma(cp, h->d_wrec.p, conv_is_f16(h->cfg.conv_mode), nb, st);
        else if (h->cfg.conv_mode == PBD_CONV_MFMA_F64) launch_conv_mfma_f64(cp, C.wfrag64.as<double>(), nb, st);
        else launch_conv(cp, nb, h->f64, st);
    }
}

// frames per DP chunk so that the chunk scratch stays within the budget
// DP scratch budget per chunk; a handle's DP_BUDGET_MB debug option lets the tests force several chunks on a small batch
size_t dp_budget(const pbd_handle *h)
{
    return h->dp_budget_mb > 0 ? (size_t)h->dp_budget_mb << 20 : (size_t)8 << 30;
}

// bytes of DP scratch for `cells` cells and `stk` stack records per job (12 B / cell-job + 16 B / two stack entries, float)
size_t dp_scratch_bytes(const pbd_handle *h, long long cells, long long stk)
{
    const size_t JG = (size_t)std::max(h->JGmax, 1);
    return (size_t)cells * JG * (6 + 2 * h->rs) + (size_t)stk * JG * (h->f64 ? kStkPairF64 : kStkPairF32);
}

int dp_chunk_frames(pbd_handle *h, Plan &P, int want)
{
    const size_t per_frame = dp_scratch_bytes(h, P.cell_per_frame, P.stk_per_jf), budget = dp_budget(h);
    int chunk = std::max(want, 1);
    while (chunk > 1 && per_frame * chunk > budget) chunk = (chunk + 1) / 2;
    return chunk;
}

int alloc_dp_scratch(pbd_handle *h, Plan &P, int chunk);

int alloc_dp(pbd_handle *h, Plan &P, int nframes, int chunk)
{
    const size_t cpf = (size_t)P.cell_per_frame;
    const int NSa = std::max(h->NS, 1);
    HIPCHK(h, h->acc.ensure(std::max<size_t>((size_t)nframes * cpf * std::max(h->NM, 1) * h->rs, 16)));
    const size_t pes = P.ptr8 ? 1 : 2;        // bytes per position
    HIPCHK(h, h->Ik.ensure(std::max<size_t>((size_t)nframes * cpf * NSa, 16)));
    HIPCHK(h, h->rootv.ensure(std::max<size_t>((size_t)nframes * cpf * h->NC * h->rs, 16)));
    HIPCHK(h, h->rooti.ensure(std::max<size_t>((size_t)nframes * cpf * h->NC * sizeof(int), 16)));
    // the transform's pointer planes are kept for the whole batch (one plane per (part, mixture)): the walk composes Ix / Iy from them
    HIPCHK(h, h->IxRaw.ensure(std::max<size_t>((size_t)nframes * cpf * std::max(h->totmix, 1) * pes, 16) + 32));
    HIPCHK(h, h->IyRaw.ensure(std::max<size_t>((size_t)nframes * cpf * std::max(h->totmix, 1) * pes, 16) + 32));
    return alloc_dp_scratch(h, P, chunk);
}

// the dynamic program's per-chunk scratch for `chunk` frames of plan P
int alloc_dp_scratch(pbd_handle *h, Plan &P, int chunk)
{
    const size_t cpf = (size_t)P.cell_per_frame;
    const size_t per_frame = cpf * std::max(h->JGmax, 1);
    const size_t stk_per_frame = (size_t)P.stk_per_jf * std::max(h->JGmax, 1);
    HIPCHK(h, h->tmp.ensure(std::max<size_t>(per_frame * chunk * h->rs, 16)));
    HIPCHK(h, h->dt.ensure(std::max<size_t>(per_frame * chunk * h->rs, 16) + 32));            // + slack: the combine step reads whole cell groups
    HIPCHK(h, h->stk.ensure(std::max<size_t>(stk_per_frame * chunk * (h->f64 ? kStkPairF64 : kStkPairF32), 16)));
    return PBD_OK;
}

// dynamic program for frames [f0, f0+nb), nb <= the chunk size given to alloc_dp
// (cell0: a mixed plan's group of whole frames, run as sub-plan P whose cell offsets start at 0 -- the whole-batch buffers are
// addressed from the group's first cell of the virtual frame)
void launch_dp_chunk(pbd_handle *h, Plan &P, int f0, int nb, hipStream_t st, long long cell0 = 0)
{
    DpParams dp{};
    dp.lv = P.d_lv.p; dp.nlevels = P.nlevels; dp.F = h->F; dp.NS = h->NS; dp.NC = h->NC; dp.NM = h->NM;
    dp.cell_per_frame = P.cell_per_frame; dp.quad_per_frame = P.quad_per_frame; dp.max_mix = h->max_mix;
    dp.resp = h->resp.p; dp.resp_half = h->resp_half ? 1 : 0; dp.acc = h->acc.p;
    dp.Ik = h->Ik.as<uint8_t>(); dp.NJ = h->totmix; dp.ptr8 = P.ptr8 ? 1 : 0;
    dp.tmp = h->tmp.p; dp.dt = h->dt.p;
    dp.IxRaw = h->IxRaw.p; dp.IyRaw = h->IyRaw.p;
    dp.stk = h->stk.p; dp.stk_per_jf = P.stk_per_jf;
    dp.stk_row_off = P.d_stk_row_off.p; dp.stk_col_off = P.d_stk_col_off.p;
    dp.biasw = h->d_biasw.p;
    dp.row2level = P.d_row2level.p; dp.rowoff = P.d_rowoff.p; dp.col2level = P.d_col2level.p; dp.coloff = P.d_coloff.p;
    dp.nrows_flat = P.nrows_flat; dp.ncols_flat = P.ncols_flat; dp.longest = P.longest;
    dp.rootv = h->rootv.p; dp.rooti = h->rooti.as<int>(); dp.rjobs = h->d_rjobs.p;
    dp.frame0 = f0;
    if (cell0) {
        const size_t c0 = (size_t)cell0, pes = P.ptr8 ? 1 : 2;
        dp.resp = h->resp.as<char>() + c0 * h->F * h->resp_es;
        dp.acc = h->acc.as<char>() + c0 * h->NM * h->rs;
        dp.Ik = h->Ik.as<uint8_t>() + c0 * h->NS;
        dp.IxRaw = h->IxRaw.as<char>() + c0 * h->totmix * pes;
        dp.IyRaw = h->IyRaw.as<char>() + c0 * h->totmix * pes;
        dp.rootv = h->rootv.as<char>() + c0 * h->NC * h->rs;
        dp.rooti = h->rooti.as<int>() + c0 * h->NC;
    }
    for (auto &g : h->groups) {
        dp.JG = (int)g.jobs.size();
        dp.jobs = g.d_jobs.p; dp.cjobs = g.d_cjobs.p; dp.childs = g.d_childs.p;
        dp.bz_x = g.bz_x; dp.bz_y = g.bz_y;
        { ProfScope ps(h, PBD_K_DT_ROWS, st); launch_dt_rows(dp, h->dt_opt, nb, h->f64, st); }
        { ProfScope ps(h, PBD_K_DT_COLS, st); launch_dt_cols(dp, h->dt_opt, nb, h->f64, st); }
        dp.sjobs = g.d_sjobs.p;
        {
            ProfScope ps(h, PBD_K_DP_COMBINE, st);
            if (h->seq_mode) launch_dp_combine_seq(dp, (int)g.sjobs.size(), nb, h->f64, st);
            else launch_dp_combine(dp, (int)g.cjobs.size(), nb, h->f64, st);
        }
    }
    { ProfScope ps(h, PBD_K_DP_ROOT, st); launch_dp_root(dp, nb, h->f64, st); }
}

// the stages over the whole batch on the handle's stream (the dynamic program in chunks of frames within its scratch budget)
int run_conv(pbd_handle *h, Plan &P, int nframes)
{
    if (int rc = alloc_conv(h, P, nframes)) return rc;
    if (int rc = ensure_seg_tiles(h, P, nframes)) return rc;
    launch_conv_stage(h, P, 0, nframes, h->stream);
    HIPCHK(h, hipGetLastError());
    h->res.resp = true;
    return PBD_OK;
}

int run_dp(pbd_handle *h, Plan &P, int nframes)
{
    const int chunk = dp_chunk_frames(h, P, nframes);
    if (int rc = alloc_dp(h, P, nframes, chunk)) return rc;
    for (int f0 = 0; f0 < nframes; f0 += chunk) launch_dp_chunk(h, P, f0, std::min(chunk, nframes - f0), h->stream);
    HIPCHK(h, hipGetLastError());
    h->res.dp = true;
    return PBD_OK;
}

}  // namespace

namespace pbd {

// ---- argmin: find (ordered compaction) + walk into a device payload, then one D2H ---------------------------------
// enqueues the find and walk kernels for the `nframes` frames of the device-resident DP result; the candidate list is
// written to d_payload = int32[1 + capacity * stride] (see pbd_handle::CandBuf).  No host synchronisation.
// pbd_set_root_nms: the grid maxima of every (frame, level, component) plane of rootv among the cells above the threshold, a
// byte per root cell in h->gn_max.  The planes of one frame are cut into blocks once per plan and sz.
// `root_ok` (pbd_set_depth_prune; NULL: off): only the cells whose byte is set are eligible.
static int enqueue_root_nms(pbd_handle *h, Plan &P, int nframes, int sz, const uint8_t *root_ok, hipStream_t st)
{
    if (P.gn_sz != sz) {
        std::vector<GnPlane> tab;
        long long blocks = 0;
        for (int l = 0; l < P.nlevels; ++l)
            for (int c = 0; c < h->NC; ++c) {
                const LevelDesc &d = P.lv[l];
                const long long HW = (long long)d.rows * d.cols;
                tab.push_back(grid_nms_plane(d.cell_off * h->NC + c * HW, d.rows, d.cols, sz, &blocks));
            }
        if (P.d_gn.p) HIPCHK(h, hipStreamSynchronize(st));   // the previous table may still be read
        HIPCHK(h, P.d_gn.upload(tab));
        P.gn_sz = sz; P.gn_blocks = blocks;
    }
    const long long per_frame = P.cell_per_frame * h->NC;
    HIPCHK(h, h->gn_max.ensure(std::max<size_t>((size_t)nframes * per_frame, 16)));
    GridNmsParams gp{};
    gp.planes = P.d_gn.p; gp.nplanes = (int)P.d_gn.size; gp.nframes = nframes;
    gp.frame_stride = per_frame; gp.blocks_per_frame = P.gn_blocks;
    gp.src = h->rootv.p; gp.use_thresh = 1; gp.thresh = h->thresh; gp.mask = root_ok; gp.sz = sz; gp.dst = h->gn_max.as<uint8_t>();
    ProfScope ps(h, PBD_K_GRID_NMS, st);
    launch_grid_nms(gp, h->f64, grid_nms_lanes(sz, h->gn_lanes), st);
    return PBD_OK;
}

int top_k_workspace(pbd_handle *h, TopKParams &p, hipStream_t st)
{
    if (int rc = carve(h, h->tk_ws, [&](Carve &c) {
            p.hist = c.take<int>((size_t)p.nseg * 256 * sizeof(int));
            p.state = c.take<TopKSeg>((size_t)p.nseg * sizeof(TopKSeg));
            p.tcnt = c.take<int>((size_t)(p.ntiles + 1) * sizeof(int));
            p.part = c.take<long long>((size_t)top_k_scan_parts(p.ntiles) * sizeof(long long));
        })) return rc;
    HIPCHK(h, hipMemsetAsync(p.hist, 0, (size_t)p.nseg * 256 * sizeof(int), st));   // (a grown workspace holds anything)
    return PBD_OK;
}

// pbd_set_top_k: the k best root cells of every frame of the call among those above the threshold whose bytes in `root_ok` and
// `root_max` (NULL: off) are set, a byte per root cell in h->tk_keep.  Equal frames are equal segments; a mixed plan's frames are
// the ranges of their own virtual levels, tabulated once per plan.
static int enqueue_top_k(pbd_handle *h, Plan &P, int nframes, int k, const uint8_t *root_ok, const uint8_t *root_max, hipStream_t st)
{
    const long long per_frame = P.cell_per_frame * h->NC, total = per_frame * nframes;
    if (total > INT_MAX) return fail(h, PBD_ERR_INVALID, "top-K: %lld root cells in the call (at most 2^31 - 1)", total);
    TopKParams tp{};
    if (P.kind == 2) {
        if (!P.d_tk.p) {
            std::vector<TopKTab> tab(P.mixed_frames + 1);
            long long tiles = 0;
            for (int f = 0; f <= P.mixed_frames; ++f) {
                const long long off = f < P.mixed_frames ? P.lv[P.frame_lv0[f]].cell_off * h->NC : per_frame;
                if (f > 0) tiles += top_k_tiles(off - tab[f - 1].off);
                tab[f] = TopKTab{off, tiles};
            }
            HIPCHK(h, P.d_tk.upload(tab));
            P.tk_tiles = tiles;
        }
        tp.tab = P.d_tk.p; tp.nseg = P.mixed_frames; tp.ntiles = P.tk_tiles;
    } else {
        tp.nseg = nframes; tp.ulen = per_frame; tp.utiles = top_k_tiles(per_frame); tp.ntiles = tp.utiles * nframes;
    }
    HIPCHK(h, h->tk_keep.ensure(std::max<size_t>((size_t)total, 16)));
    if (int rc = top_k_workspace(h, tp, st)) return rc;
    tp.k = k; tp.src = h->rootv.p; tp.use_thresh = 1; tp.thresh = h->thresh; tp.mask = root_ok; tp.mask2 = root_max;
    tp.dst = h->tk_keep.as<uint8_t>();
    ProfScope ps(h, PBD_K_TOP_K, st);
    launch_top_k(tp, h->f64, st);
    return PBD_OK;
}

// pbd_set_scale_nms: of the root cells above the threshold whose bytes in ap.root_ok and ap.root_max (NULL: off) are set, those
// no better neighbour within dl levels beats, a byte per root cell in h->sn_keep.  The byte implies the two it was built from.
static int enqueue_scale_nms(pbd_handle *h, const ArgminParams &ap, int dl, hipStream_t st)
{
    HIPCHK(h, h->sn_keep.ensure(std::max<size_t>((size_t)ap.ntotal, 16)));
    const ScaleNmsRoots a{dl, ap.root_ok, ap.root_max, h->sn_keep.as<uint8_t>()};
    ProfScope ps(h, PBD_K_SCALE_NMS, st);
    launch_scale_nms_roots(ap, a, h->f64, st);
    return PBD_OK;
}

int enqueue_argmin(pbd_handle *h, Plan &P, int nframes, const float *d_scales, int frame_offset, int32_t *d_payload,
                   int capacity, hipStream_t st, bool walk_only, RootSel sel)
{
    ArgminParams ap{};
    ap.lv = P.d_lv.p; ap.nlevels = P.nlevels; ap.NS = h->NS; ap.NC = h->NC; ap.nframes = nframes;
    ap.cell_per_frame = P.cell_per_frame;
    ap.rootv = h->rootv.p; ap.rooti = h->rooti.as<int>();
    ap.IxRaw = h->IxRaw.p; ap.IyRaw = h->IyRaw.p; ap.NJ = h->totmix; ap.Ik = h->Ik.as<uint8_t>(); ap.ptr8 = P.ptr8 ? 1 : 0;
    ap.walk_mode = h->walk_mode;
    ap.thresh = h->thresh; ap.scales = d_scales;
    ap.walk = h->d_walk.p; ap.walk_off = h->d_walk_off.p;
    ap.max_parts = h->max_parts; ap.stride = stride(h); ap.capacity = std::max(capacity, 0);
    ap.payload = d_payload; ap.frame_offset = frame_offset;
    if (P.kind == 2) { ap.lv_frame = P.d_lv_frame.p; ap.lv_local = P.d_lv_local.p; }
    ap.ntotal = (long long)nframes * P.cell_per_frame * h->NC;
    ap.nblk = (int)std::max<long long>((ap.ntotal + argmin_find_span() - 1) / argmin_find_span(), 1);
    HIPCHK(h, h->find_blk.ensure((size_t)ap.nblk * sizeof(int)));
    ap.blk = h->find_blk.as<int>();
    if (sel.prune && !walk_only) {   // pbd_set_depth_prune with the depth images claim_depth took for this call
        pbd_handle::DepthBind call;   // used once: the next call binds again
        std::swap(call, h->dpr_call);
        if (int rc = h->dpr_tab.stage(h, call.tab.data(), call.tab.size() * sizeof(Box3dFrame))) return rc;
        HIPCHK(h, h->dpr_ok.ensure(std::max<size_t>((size_t)ap.ntotal, 16)));
        const DepthPruneRoots a{h->dpr_tab.as<Box3dFrame>(), call.depth, h->dprune_rule, h->dpr_ok.as<uint8_t>()};
        ProfScope ps(h, PBD_K_DEPTH_PRUNE, st);
        launch_depth_prune_roots(ap, a, h->f64, st);
        ap.root_ok = a.ok;
    }
    if (sel.nms > 0 && !walk_only) {
        if (int rc = enqueue_root_nms(h, P, nframes, sel.nms, ap.root_ok, st)) return rc;
        ap.root_max = h->gn_max.as<uint8_t>();
    }
    if (sel.scale >= 0 && !walk_only && ap.ntotal > 0) {   // handed on as root_max: k_top_k and the find need no new mask
        if (int rc = enqueue_scale_nms(h, ap, sel.scale, st)) return rc;
        ap.root_max = h->sn_keep.as<uint8_t>();
    }
    if (sel.top > 0 && !walk_only && ap.ntotal > 0) {
        if (int rc = enqueue_top_k(h, P, nframes, sel.top, ap.root_ok, ap.root_max, st)) return rc;
        ap.root_top = h->tk_keep.as<uint8_t>();
    }
    ProfScope ps(h, PBD_K_ARGMIN, st);
    if (!walk_only) launch_argmin_find(ap, h->f64, st);   // walk_only: the payload's records were written by the caller
    launch_argmin_walk(ap, h->f64, st);
    return PBD_OK;
}

// pbd_set_depth_prune / pbd_depth_prune*: the rule's parameters widened, or PBD_ERR_INVALID (include/pbd.h: fx and width finite
// and > 0, tol finite and >= 0)
int depth_prune_rule(pbd_handle *h, const pbd_depth_prune_cfg &cfg, DepthPruneRule *rule)
{
    if (!(std::isfinite(cfg.fx) && cfg.fx > 0 && std::isfinite(cfg.width) && cfg.width > 0 && std::isfinite(cfg.tol) && cfg.tol >= 0))
        return fail(h, PBD_ERR_INVALID, "depth prune: fx %g, width %g (finite, > 0), tol %g (finite, >= 0)", (double)cfg.fx,
                    (double)cfg.width, (double)cfg.tol);
    *rule = DepthPruneRule{(double)cfg.fx, (double)cfg.width, (double)cfg.tol};
    return PBD_OK;
}

// ---- post-processing (pbd_set_nms): per-frame sort + suppression of the payload d_in (capacity in_cap records, frame-local
// `frame` fields, nframes frames of rows x cols) into d_out = int32[1 + out_cap * stride]: word 0 = kept count (-1 when more
// than in_cap candidates were found), then the kept records frame by frame, `frame` + frame_offset.  No host synchronisation.
// pbd_suppress*: `in_offset` is subtracted from the input's `frame` fields and `bad` (zeroed here) turns on the list's check.
int enqueue_post(pbd_handle *h, int nframes, int rows, int cols, float overlap, const int32_t *d_in, int in_cap, int frame_offset,
                 int32_t *d_out, int out_cap, hipStream_t st, const Plan *mixed, int in_offset, int *bad)
{
    PostParams pp{};
    pp.in_offset = in_offset; pp.bad = bad;
    if (bad) HIPCHK(h, hipMemsetAsync(bad, 0, sizeof(int), st));
    pp.in = d_in; pp.in_cap = std::max(in_cap, 1);
    pp.stride = stride(h); pp.max_parts = h->max_parts; pp.nframes = nframes;
    pp.rows = rows; pp.cols = cols; pp.wpr = (cols + 31) / 32; pp.overlap = overlap;
    pp.out = d_out; pp.out_cap = std::max(out_cap, 0); pp.frame_offset = frame_offset;
    // workspace: key, frame, perm, slot [in_cap] | box [in_cap] int4 | fkept [nframes] | global canvases (frames too big for LDS)
    const size_t n = (size_t)pp.in_cap, a4 = (4 * n * sizeof(int) + 15) & ~(size_t)15;
    const size_t fk = ((size_t)nframes * sizeof(int) + 15) & ~(size_t)15;
    const size_t canvas = mixed ? mixed->post_glb_words * sizeof(uint32_t)
                                : post_canvas_in_lds(rows, cols) ? 0 : (size_t)nframes * post_canvas_words(rows, cols) * sizeof(uint32_t);
    HIPCHK(h, h->post_ws.ensure(a4 + n * sizeof(int4) + fk + canvas));
    char *ws = h->post_ws.as<char>();
    pp.key = reinterpret_cast<float *>(ws); pp.frame = reinterpret_cast<int *>(ws) + n;
    pp.perm = reinterpret_cast<int *>(ws) + 2 * n; pp.slot = reinterpret_cast<int *>(ws) + 3 * n;
    pp.box = reinterpret_cast<int4 *>(ws + a4);
    pp.fkept = reinterpret_cast<int *>(ws + a4 + n * sizeof(int4));
    pp.canvas = canvas ? reinterpret_cast<uint32_t *>(ws + a4 + n * sizeof(int4) + fk) : nullptr;
    if (mixed) {   // every frame with its own size and canvas kind
        pp.fdim = mixed->d_fdim.p; pp.fcanvas = mixed->d_fcanvas.p;
        launch_postprocess_mixed(pp, mixed->d_post_lds.p, (int)mixed->post_lds.size(), mixed->post_lds_words, mixed->d_post_glb.p,
                                 (int)mixed->post_glb.size(), st);
        return PBD_OK;
    }
    launch_postprocess(pp, st);
    return PBD_OK;
}

// find + walk into cb.payload (then, with `post`, the sort + suppression into cb.post) and the speculative read-back of
// [count | first records], all on `st`

}  // namespace pbd

namespace {

int enqueue_argmin_readback(pbd_handle *h, Plan &P, int nframes, const float *d_scales, pbd_handle::CandBuf &cb, bool post,
                            RootSel sel, hipStream_t st)
{
    const int stride = ::stride(h), cap = std::max(h->cfg.max_candidates, 1);
    HIPCHK(h, cb.payload.ensure(((size_t)cap * stride + 1) * sizeof(int32_t)));
    if (int rc = enqueue_argmin(h, P, nframes, d_scales, 0, cb.payload.as<int32_t>(), cap, st, false, sel)) return rc;
    cb.nms = post;
    if (post) {
        HIPCHK(h, cb.post.ensure(((size_t)cap * stride + 1) * sizeof(int32_t)));
        if (int rc = enqueue_post(h, P.kind == 2 ? P.mixed_frames : nframes, P.rows, P.cols, h->nms_overlap, cb.payload.as<int32_t>(),
                                  cap, 0, cb.post.as<int32_t>(), cap, st, P.kind == 2 ? &P : nullptr))
            return rc;
    }
    cb.copied = std::min(h->cand_guess, cap);
    const size_t words = 1 + (size_t)cb.copied * stride;
    // the mirror is sized for twice the guess: growing pinned memory synchronises the device
    if (cb.host.size < words * sizeof(int32_t))
        HIPCHK(h, cb.reserve(1 + (size_t)std::min(2 * (long long)cb.copied, (long long)cap) * stride));
    HIPCHK(h, hipMemcpyAsync(cb.words(), cb.out().p, words * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return PBD_OK;
}

// after the read-back has completed: hand the records to the caller (the reference's order is nondeterministic,
// src/DynamicProgram.cpp:246-251; here it is (frame, level, component, y, x), produced on the device)
int argmin_deliver(pbd_handle *h, pbd_handle::CandBuf &cb, hipStream_t st, int32_t *cand, int capacity, int *ncand)
{
    const int stride = ::stride(h), cap = std::max(h->cfg.max_candidates, 1);
    const int found = cb.words()[0];
    if (found < 0) {         // the post-processing stage saw more candidates than the list holds: no suppressed prefix
        *ncand = 0;
        return fail(h, PBD_ERR_CAPACITY, "more than max_candidates (%d) candidates were found before non-maxima suppression: "
                    "raise pbd_config.max_candidates", cap);
    }
    const int n = std::min(found, cap);
    if (n > cb.copied) {     // more candidates than the speculative copy covered: fetch the list again, whole
        const size_t words = 1 + (size_t)n * stride;
        HIPCHK(h, cb.reserve(words));
        HIPCHK(h, hipMemcpyAsync(cb.words(), cb.out().p, words * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        cb.copied = n;
    }
    h->cand_guess = std::min(cap, std::max(n + n / 4 + 256, 1024));
    const int nout = std::min(n, std::max(capacity, 0));
    if (nout > 0) memcpy(cand, cb.words() + 1, (size_t)nout * stride * sizeof(int32_t));
    *ncand = nout;
    if (found > cap || n > capacity)
        return fail(h, PBD_ERR_CAPACITY, "%d candidates found, capacity %d (config max_candidates %d)", found, capacity, cap);
    return PBD_OK;
}

int run_argmin(pbd_handle *h, Plan &P, int nframes, const float *d_scales, bool post, RootSel sel, int32_t *cand, int capacity,
               int *ncand)
{
    if (int rc = enqueue_argmin_readback(h, P, nframes, d_scales, h->cb, post, sel, h->stream)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipGetLastError());
    return argmin_deliver(h, h->cb, h->stream, cand, capacity, ncand);
}

// the device-out form: the list straight into the caller's payload, or -- with the post-processing stage on -- the whole list
// into the handle's own payload (capacity max_candidates: the stage never sees a truncated list), then the kept records into
// the caller's
int enqueue_argmin_out(pbd_handle *h, Plan &P, int nframes, int frame_offset, int32_t *d_payload, int capacity)
{
    if (!h->nms) return enqueue_argmin(h, P, nframes, P.d_scales.p, frame_offset, d_payload, capacity, h->stream, false, root_sel(h));
    const int cap = std::max(h->cfg.max_candidates, 1);
    HIPCHK(h, h->cb.payload.ensure(((size_t)cap * stride(h) + 1) * sizeof(int32_t)));
    if (int rc = enqueue_argmin(h, P, nframes, P.d_scales.p, 0, h->cb.payload.as<int32_t>(), cap, h->stream, false, root_sel(h)))
        return rc;
    return enqueue_post(h, P.kind == 2 ? P.mixed_frames : nframes, P.rows, P.cols, h->nms_overlap, h->cb.payload.as<int32_t>(), cap,
                        frame_offset, d_payload, capacity, h->stream, P.kind == 2 ? &P : nullptr);
}

// The first step of every entry point pbd_bind_depth* lists: the call consumes the binding.  Pruning off: dropped unused; a
// binding whose frame count or sizes differ from the call's (size(f) = {rows, cols} of frame f) is refused and dropped; else
// it becomes h->dpr_call, which the call's enqueue_argmin uses (root_sel).  A call refused later leaves it to the next claim.
template <class Size> int claim_depth(pbd_handle *h, int nframes, Size size)
{
    pbd_handle::DepthBind b;
    std::swap(b, h->dpr_bound);
    h->dpr_call = pbd_handle::DepthBind{};
    if (b.tab.empty() || !h->dprune) return PBD_OK;
    if ((int)b.tab.size() != nframes)
        return fail(h, PBD_ERR_INVALID, "%d depth images are bound, the call has %d frames", (int)b.tab.size(), nframes);
    for (int f = 0; f < nframes; ++f) {
        const std::pair<int, int> s = size(f);
        if (b.tab[f].rows != s.first || b.tab[f].cols != s.second)
            return fail(h, PBD_ERR_INVALID, "frame %d: the bound depth image is %dx%d, the frame %dx%d", f, b.tab[f].rows, b.tab[f].cols,
                        s.first, s.second);
    }
    h->dpr_call = std::move(b);
    return PBD_OK;
}
int claim_depth(pbd_handle *h, int nframes, int rows, int cols)
{
    return claim_depth(h, nframes, [&](int) { return std::make_pair(rows, cols); });
}
int claim_depth(pbd_handle *h, int nframes, const pbd_frame *frames)
{
    return claim_depth(h, nframes, [&](int f) { return std::make_pair(frames[f].rows, frames[f].cols); });
}

// Frames of a call: on the host (`host[i]`, rows `stride` bytes apart; uploaded to h->frames by enqueue_features) or
// already packed on the device (`dev`)
struct FrameSrc {
    const void *const *host;
    size_t stride;
    const void *dev;
};

// image depth and channels; for host frames also the row stride and, for 32F / 64F, that every pixel is finite
int check_frames(pbd_handle *h, int nframes, const FrameSrc &src, int rows, int cols, int cn, int depth)
{
    if (!depth_size(depth))
        return fail(h, PBD_ERR_UNSUPPORTED, "image depth code %d: 0 (8U), 2 (16U), 5 (32F) or 6 (64F), src/HOGFeatures.cpp:136-146", depth);
    if (cn != 1 && cn != 3) return fail(h, PBD_ERR_INVALID, "channels %d (1 or 3, src/HOGFeatures.cpp:171)", cn);
    if (!src.host) return PBD_OK;
    for (int i = 0; i < nframes; ++i)
        if (!src.host[i]) return fail(h, PBD_ERR_INVALID, "frame %d is a null pointer", i);
    const size_t row_bytes = (size_t)cols * cn * depth_size(depth);
    if (src.stride < row_bytes) return fail(h, PBD_ERR_INVALID, "stride %zu < row bytes %zu", src.stride, row_bytes);
    // 32F / 64F images: a NaN or Inf pixel is refused.  The reference computes *something* deterministic from one (NaN
    // gradients, NaN histogram bins, NaN responses whose envelope read-out order then matters); the distance transform here
    // walks the envelope top-down, which equals the reference's bottom-up walk only for strictly increasing finite
    // intersections -- so non-finite input is defined as an error instead of being allowed to differ silently.
    if (depth == kDepth32F || depth == kDepth64F) {
        const size_t n = (size_t)cols * cn;
        for (int i = 0; i < nframes; ++i)
            for (int y = 0; y < rows; ++y) {
                const char *row = static_cast<const char *>(src.host[i]) + (size_t)y * src.stride;
                bool ok = true;
                if (depth == kDepth32F) { const float *p = reinterpret_cast<const float *>(row); for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(p[k]); }
                else { const double *p = reinterpret_cast<const double *>(row); for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(p[k]); }
                if (!ok) return fail(h, PBD_ERR_INVALID, "frame %d, row %d holds a NaN or Inf pixel", i, y);
            }
    }
    return PBD_OK;
}

// every check of a detect call, before anything is enqueued; *plan = the batch's image plan
int check_detect(pbd_handle *h, int nframes, const FrameSrc &src, int rows, int cols, int cn, int depth, Plan **plan)
{
    if (int rc = check_batch(h, nframes)) return rc;
    if (int rc = check_frames(h, nframes, src, rows, cols, cn, depth)) return rc;
    if (int rc = check_bank(h)) return rc;
    return get_image_plan(h, rows, cols, plan);
}

int upload_frames(pbd_handle *h, int nframes, const void *const *imgs, int rows, int cols, int cn, int depth, size_t stride_bytes)
{
    const size_t row_bytes = (size_t)cols * cn * depth_size(depth);
    HIPCHK(h, h->frames.ensure((size_t)nframes * rows * row_bytes + 4));
    for (int i = 0; i < nframes; ++i)
        HIPCHK(h, hipMemcpy2DAsync(h->frames.as<uint8_t>() + (size_t)i * rows * row_bytes, row_bytes, imgs[i], stride_bytes,
                                   row_bytes, rows, hipMemcpyHostToDevice, h->stream));
    return PBD_OK;
}

// The batch's result replaces the resident one here; then its frames are uploaded (host frames) and the pyramid and HOG
// features enqueued.  No host synchronisation.
int enqueue_features(pbd_handle *h, Plan &P, int nframes, const FrameSrc &src, int cn, int depth)
{
    h->res = Resident{&P, nframes, cn, depth};
    const void *d_frames = src.dev;
    if (src.host) {
        if (int rc = upload_frames(h, nframes, src.host, P.rows, P.cols, cn, depth, src.stride)) return rc;
        d_frames = h->frames.p;
    }
    if (int rc = alloc_features(h, P, nframes, cn, depth)) return rc;
    launch_features(h, P, d_frames, cn, depth, 0, nframes, h->stream);
    HIPCHK(h, hipGetLastError());
    h->res.features = true;
    h->res.c31_zero = !P.padded;   // a pad cell holds 1 on channel 31
    return PBD_OK;
}

// pyramid -> HOG -> convolution -> dynamic program for a batch that passed check_detect (no host synchronisation)
int enqueue_detect(pbd_handle *h, Plan &P, int nframes, const FrameSrc &src, int cn, int depth)
{
    if (int rc = enqueue_features(h, P, nframes, src, cn, depth)) return rc;
    if (int rc = run_conv(h, P, nframes)) return rc;
    return run_dp(h, P, nframes);
}

// the synchronous detect entry points: the whole path, then the candidates' read-back
int detect_sync(pbd_handle *h, int nframes, const FrameSrc &src, int rows, int cols, int cn, int depth, int32_t *cand, int capacity,
                int *ncand)
{
    Plan *P = nullptr;
    if (int rc = claim_depth(h, nframes, rows, cols)) return rc;
    if (int rc = check_detect(h, nframes, src, rows, cols, cn, depth, &P)) return rc;
    if (int rc = enqueue_detect(h, *P, nframes, src, cn, depth)) return rc;
    return run_argmin(h, *P, nframes, P->d_scales.p, h->nms, root_sel(h), cand, capacity, ncand);
}

// copies n responses from the device to dst as T; in PBD_CONV_MFMA_F16 mode the device holds fp16, widened to float here
int read_responses(pbd_handle *h, void *dst, const void *src, size_t n)
{
    if (!n) return PBD_OK;
    if (!h->resp_half) {
        HIPCHK(h, hipMemcpyAsync(dst, src, n * h->rs, hipMemcpyDeviceToHost, h->stream));
        return PBD_OK;
    }
    std::vector<uint16_t> halfbuf(n);
    HIPCHK(h, hipMemcpyAsync(halfbuf.data(), src, n * 2, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float *out = static_cast<float *>(dst);
    for (size_t i = 0; i < n; ++i) out[i] = host_h2f(halfbuf[i]);
    return PBD_OK;
}

// ---- mixed-size calls (pbd_detect_frames*) -------------------------------------------------------------------------------
// the dynamic program of a mixed plan: the whole virtual frame in one pass when its scratch fits the budget, else in groups
// of whole frames (sub-plans built once per budget)
int run_dp_mixed(pbd_handle *h, Plan &P)
{
    const size_t budget = dp_budget(h);
    auto scratch = [&](long long cells, long long stk) { return dp_scratch_bytes(h, cells, stk); };
    if (int rc = alloc_dp(h, P, 1, 0)) return rc;   // the whole-batch buffers (scratch below)
    if (scratch(P.cell_per_frame, P.stk_per_jf) <= budget || P.mixed_frames == 1) {
        if (int rc = alloc_dp_scratch(h, P, 1)) return rc;
        launch_dp_chunk(h, P, 0, 1, h->stream);
    } else {
        if (P.chunk_budget != budget) {
            // groups of consecutive frames, greedily, by an estimate (cells, and the stack share of the virtual frame's)
            std::vector<std::unique_ptr<Plan>> plans;
            std::vector<long long> cell0s;
            int f = 0;
            while (f < P.mixed_frames) {
                int g = f + 1;
                auto cells = [&](int a, int b) {
                    const int l0 = P.frame_lv0[a], l1 = P.frame_lv0[b];
                    return (l1 < P.nlevels ? P.lv[l1].cell_off : P.cell_per_frame) - P.lv[l0].cell_off;
                };
                auto est = [&](int a, int b) {
                    const long long c = cells(a, b);
                    return scratch(c, P.cell_per_frame ? (long long)((double)P.stk_per_jf * c / P.cell_per_frame) + 64 : 0);
                };
                while (g < P.mixed_frames && est(f, g + 1) <= budget) ++g;
                auto S = std::make_unique<Plan>();
                const int l0 = P.frame_lv0[f], l1 = P.frame_lv0[g];
                const long long c0 = P.lv[l0].cell_off;
                S->kind = 3; S->interval = P.interval; S->nlevels = l1 - l0;
                S->lv.assign(P.lv.begin() + l0, P.lv.begin() + l1);
                for (LevelDesc &d : S->lv) d.cell_off -= c0;
                S->cell_per_frame = cells(f, g);
                HIPCHK(h, finish_plan_tables(*S, h->sbin));
                S->ptr8 = P.ptr8;        // the pointer planes' element size is the whole call's
                plans.push_back(std::move(S));
                cell0s.push_back(c0);
                f = g;
            }
            P.chunk_plans = std::move(plans);
            P.chunk_cell0 = std::move(cell0s);
            P.chunk_budget = budget;
        }
        for (auto &S : P.chunk_plans)
            if (int rc = alloc_dp_scratch(h, *S, 1)) return rc;
        for (size_t i = 0; i < P.chunk_plans.size(); ++i) launch_dp_chunk(h, *P.chunk_plans[i], 0, 1, h->stream, P.chunk_cell0[i]);
    }
    HIPCHK(h, hipGetLastError());
    h->res.dp = true;
    return PBD_OK;
}

}  // namespace

namespace pbd {

// every check of a mixed-size call before anything is enqueued; *plan = its mixed plan
int check_frames_mixed(pbd_handle *h, int nframes, const pbd_frame *frames, int cn, int depth, bool host, Plan **plan)
{
    if (h->shard_world > 1)
        return fail(h, PBD_ERR_UNSUPPORTED, "mixed-size calls with level sharding (world %d): pbd_set_level_shard(h, 0, 1) first",
                    h->shard_world);
    if (int rc = check_batch(h, nframes)) return rc;
    if (int rc = check_frame_descs(h, nframes, frames, cn, depth, host)) return rc;
    std::vector<int> rows(nframes), cols(nframes);
    for (int f = 0; f < nframes; ++f) { rows[f] = frames[f].rows; cols[f] = frames[f].cols; }
    if (int rc = check_bank(h)) return rc;
    return get_mixed_plan(h, nframes, rows.data(), cols.data(), plan);
}

int check_frame_descs(pbd_handle *h, int nframes, const pbd_frame *frames, int cn, int depth, bool host)
{
    if (!depth_size(depth))
        return fail(h, PBD_ERR_UNSUPPORTED, "image depth code %d: 0 (8U), 2 (16U), 5 (32F) or 6 (64F), src/HOGFeatures.cpp:136-146", depth);
    if (cn != 1 && cn != 3) return fail(h, PBD_ERR_INVALID, "channels %d (1 or 3, src/HOGFeatures.cpp:171)", cn);
    for (int f = 0; f < nframes; ++f) {
        const pbd_frame &fr = frames[f];
        if (!fr.data || fr.rows < 1 || fr.cols < 1 || fr.rows > 32000 || fr.cols > 32000)
            return fail(h, PBD_ERR_INVALID, "frame %d: %dx%d at %p", f, fr.rows, fr.cols, fr.data);
        const size_t row_bytes = (size_t)fr.cols * cn * depth_size(depth);
        if (fr.stride_bytes < row_bytes) return fail(h, PBD_ERR_INVALID, "frame %d: stride %zu < row bytes %zu", f, fr.stride_bytes, row_bytes);
        if (!host && (reinterpret_cast<uintptr_t>(fr.data) % depth_size(depth) || fr.stride_bytes % depth_size(depth)))
            return fail(h, PBD_ERR_INVALID, "frame %d: device pointer %p / stride %zu not a multiple of the %zu-byte element", f, fr.data,
                        fr.stride_bytes, depth_size(depth));
        if (host && (depth == kDepth32F || depth == kDepth64F)) {   // as check_frames: non-finite input is an error
            const size_t n = (size_t)fr.cols * cn;
            for (int y = 0; y < fr.rows; ++y) {
                const char *row = static_cast<const char *>(fr.data) + (size_t)y * fr.stride_bytes;
                bool ok = true;
                if (depth == kDepth32F) { const float *q = reinterpret_cast<const float *>(row); for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(q[k]); }
                else { const double *q = reinterpret_cast<const double *>(row); for (size_t k = 0; k < n; ++k) ok = ok && std::isfinite(q[k]); }
                if (!ok) return fail(h, PBD_ERR_INVALID, "frame %d, row %d holds a NaN or Inf pixel", f, y);
            }
        }
    }
    return PBD_OK;
}

int frame_descs(pbd_handle *h, int nframes, const pbd_frame *frames, int cn, int depth, bool host, std::vector<FrameDesc> &fd)
{
    const size_t es = depth_size(depth);
    fd.resize(nframes);
    if (host) {   // the frames go to the handle's frame buffer, packed, each with its own dense rows
        size_t total = 0;
        for (int f = 0; f < nframes; ++f) total += (size_t)frames[f].rows * frames[f].cols * cn * es;
        HIPCHK(h, h->frames.ensure(total + 4));
        size_t off = 0;
        for (int f = 0; f < nframes; ++f) {
            const size_t row_bytes = (size_t)frames[f].cols * cn * es;
            uint8_t *dst = h->frames.as<uint8_t>() + off;
            HIPCHK(h, hipMemcpy2DAsync(dst, row_bytes, frames[f].data, frames[f].stride_bytes, row_bytes, frames[f].rows,
                                       hipMemcpyHostToDevice, h->stream));
            fd[f] = FrameDesc{dst, frames[f].rows, frames[f].cols, (long long)row_bytes};
            off += row_bytes * frames[f].rows;
        }
    } else {
        for (int f = 0; f < nframes; ++f)
            fd[f] = FrameDesc{static_cast<const uint8_t *>(frames[f].data), frames[f].rows, frames[f].cols, (long long)frames[f].stride_bytes};
    }
    return PBD_OK;
}

// pyramid -> HOG -> convolution -> dynamic program of a mixed-size call that passed check_frames_mixed (no host synchronisation)
int enqueue_detect_mixed(pbd_handle *h, Plan &P, int nframes, const pbd_frame *frames, int cn, int depth, bool host,
                         const LatentParams *mask)
{
    h->res = Resident{&P, 1, cn, depth};
    std::vector<FrameDesc> fd;
    if (int rc = frame_descs(h, nframes, frames, cn, depth, host, fd)) return rc;
    if (int rc = h->fd_tab.stage(h, fd.data(), fd.size() * sizeof(FrameDesc))) return rc;
    if (int rc = alloc_features(h, P, 1, cn, depth)) return rc;
    launch_features_mixed(h, P, h->fd_tab.as<FrameDesc>(), cn, depth, h->stream);
    HIPCHK(h, hipGetLastError());
    h->res.features = true;
    h->res.c31_zero = !P.padded;   // a pad cell holds 1 on channel 31
    if (int rc = run_conv(h, P, 1)) return rc;
    if (mask) {   // pbd_detect_latent: the responses of the latent bank, masked before the dynamic program
        LatentParams lp = *mask;
        lp.resp = h->resp.p; lp.lv = P.d_lv.p; lp.nlevels = P.nlevels; lp.F = h->F; lp.cell_per_frame = P.cell_per_frame;
        lp.lv_frame = P.d_lv_frame.p; lp.scales = P.d_scales.p; lp.resp_half = h->resp_half ? 1 : 0;
        launch_latent_mask(lp, h->f64, h->stream);
        HIPCHK(h, hipGetLastError());
    }
    return run_dp_mixed(h, P);
}

// Warped positives: n kept boxes are the n levels of one virtual frame, each a P x P image that no pyramid kernel writes
// (src_level -1, no resize tables: k_warp fills them), so the HOG stage runs over them as over any plan's levels.
int warp_plan(pbd_handle *h, int n, int P, int cn, int depth, Plan **out)
{
    const std::vector<int> key{n, P};
    if (!h->wp_plan || h->wp_plan->key_dims != key) {
        auto W = std::make_unique<Plan>();
        W->kind = 1; W->key_dims = key; W->nlevels = n; W->interval = h->interval;
        W->lv.resize(n);
        W->scales.assign(n, 1.f);
        const int blk = (int)roundf((float)P / (float)h->sbin);   // HOGFeatures.cpp:174: k + 2 exactly
        for (int l = 0; l < n; ++l) {
            LevelDesc &d = W->lv[l];
            memset(&d, 0, sizeof d);
            d.img_rows = d.img_cols = P;
            d.blk_rows = d.blk_cols = blk;
            d.rows = d.cols = std::max(blk - 2, 0);
            d.src_level = -1;
            d.sbin = h->sbin;             // a patch plan never gets the fine octave
            d.img_off = (long long)l * P * P;
            d.blk_off = (long long)l * blk * blk;
            d.cell_off = (long long)l * d.rows * d.cols;
        }
        W->pix_per_frame = (long long)n * P * P;
        W->npix_resized = W->pix_per_frame;
        W->blk_per_frame = (long long)n * blk * blk;
        W->cell_per_frame = n ? W->lv[n - 1].cell_off + (long long)W->lv[n - 1].rows * W->lv[n - 1].cols : 0;
        HIPCHK(h, finish_plan_tables(*W, h->sbin));
        h->wp_plan = std::move(W);
    }
    if (int rc = grow_coord(h, P, P)) return rc;
    if (int rc = alloc_features(h, *h->wp_plan, 1, cn, depth)) return rc;
    *out = h->wp_plan.get();
    return PBD_OK;
}

void warp_hog(pbd_handle *h, Plan &W, int cn, int depth) { launch_hog_stage(h, W, cn, depth, 0, 1, h->stream); }

}  // namespace pbd

// ================================================================================================
extern "C" {

const char *pbd_version(void) { return "pbd-hip 0.1 (gfx950)"; }

// diagnostics, not part of include/pbd.h
// k_conv_mfma_any at filter side `ksize`: what = 0 resident workgroups per CU, 1 LDS bytes per workgroup, 2 channels per staged block
int pbd_debug_conv_any(int ksize, int f16, int what)
{
    if (ksize < 1 || ksize > kConvMaxK) return -1;
    const int cb = conv_mfma_any_cb(ksize, f16 != 0);
    return what == 0 ? conv_mfma_any_occupancy(ksize, f16 != 0) : what == 1 ? (int)conv_mfma_any_lds(ksize, cb, f16 != 0) : cb;
}
int pbd_debug_conv_occupancy(int nw) { return nw == 5 ? conv_mfma_occupancy(false) : nw == 6 ? conv_mfma_occupancy(true) : conv_occupancy(nw); }
// the convolution's tile cover of one rows x cols level (host-only, no GPU needed): out[i] = {shape, y0, x0}
int pbd_debug_cover_level(int rows, int cols, int *out, int capacity)
{
    return guarded(nullptr, [&]() -> int {
        std::vector<ConvTile> shaped[3];
        cover_level(0, rows, cols, shaped);
        int n = 0;
        for (int k = 0; k < 3; ++k)
            for (const ConvTile &t : shaped[k]) {
                if (n < capacity) { out[3 * n] = k; out[3 * n + 1] = t.y0; out[3 * n + 2] = t.x0; }
                ++n;
            }
        return n;
    });
}

// the exact convolution's strip-sequence tiles for `nb` frames of the given feature-map sizes (host-only, no GPU needed):
// out[i] = {nseg, len0, len1, len2, then per segment frame, level, strip, x0} = 16 ints per tile; returns the tile count
int pbd_debug_seg_tiles(int nlevels, const int *rows, const int *cols, int nb, int *out, int capacity)
{
    return guarded(nullptr, [&]() -> int {
        std::vector<LevelDesc> lv(nlevels);
        for (int l = 0; l < nlevels; ++l) { memset(&lv[l], 0, sizeof lv[l]); lv[l].rows = rows[l]; lv[l].cols = cols[l]; }
        std::vector<ConvSegTile> tiles;
        build_seg_tiles(lv, nb, tiles);
        static_assert(sizeof(ConvSegTile) == 16 * sizeof(int), "a tile record is 16 ints");
        for (size_t i = 0; i < tiles.size() && (int)i < capacity; ++i) memcpy(out + 16 * i, &tiles[i], sizeof(ConvSegTile));
        return (int)tiles.size();
    });
}

// the virtual level table of a mixed-size call (host-only, no GPU needed): frames of rows[f] x cols[f] in call order, for a
// model of `sbin` / `interval`; out[i] = {frame, local level, img_rows, img_cols, rows, cols, cell_off} = 7 ints per level
// (cell_off fits an int for every frame size accepted); returns the level count, or PBD_ERR_INVALID (a frame too small)
int pbd_debug_mixed_plan(int sbin, int interval, int nframes, const int *rows, const int *cols, int *out, int capacity)
{
    return guarded(nullptr, [&]() -> int {
        if (nframes < 1 || sbin < 2 || interval < 1 || !rows || !cols) return PBD_ERR_INVALID;
        Plan M;
        for (int f = 0; f < nframes; ++f) {
            Plan Q;
            std::string err;
            if (rows[f] < 1 || cols[f] < 1 || image_plan_host(rows[f], cols[f], sbin, interval, 0, 0, false, Q, err)) return PBD_ERR_INVALID;
            mixed_append(M, Q);
        }
        mixed_finish(M, interval);
        for (int l = 0; l < M.nlevels && l < capacity; ++l) {
            const LevelDesc &d = M.lv[l];
            int *o = out + 7 * (size_t)l;
            o[0] = M.lv_frame[l]; o[1] = M.lv_local[l]; o[2] = d.img_rows; o[3] = d.img_cols; o[4] = d.rows; o[5] = d.cols;
            o[6] = (int)d.cell_off;
        }
        return M.nlevels;
    });
}

// runs a body that throws inside the ABI guard (host-only): 0 = std::bad_alloc, 1 = std::length_error from an absurd
// std::vector size, 2 = another std::exception; returns the status code the guard produced
int pbd_debug_guard_selftest(int kind)
{
    return guarded(nullptr, [&]() -> int {
        if (kind == 0) throw std::bad_alloc();
        if (kind == 1) { std::vector<int32_t> v; v.resize(v.max_size() + (size_t)1); return (int)v.size(); }
        if (kind == 2) throw std::runtime_error("selftest");
        return PBD_OK;
    });
}

// the post-processing stage of pbd_set_nms on a caller-built record list (tests: exact ties, boxes outside the frame, very
// long lists): records[n] grouped by ascending frame (frames 0..), each with 1..max_parts parts; out receives min(kept,
// capacity) records, *nout = that count; PBD_ERR_CAPACITY when more were kept
int pbd_debug_postprocess(pbd_handle *h, int rows, int cols, const int32_t *records, int n, float overlap, int32_t *out, int capacity,
                          int *nout)
{
    return entry(h, nout && (n <= 0 || records) && (capacity <= 0 || out), kIdle, [&]() -> int {
        *nout = 0;
        if (rows < 1 || cols < 1 || rows > 65536 || cols > 65536 || n < 0 || capacity < 0 || std::isnan(overlap))
            return fail(h, PBD_ERR_INVALID, "rows %d, cols %d, n %d, capacity %d", rows, cols, n, capacity);
        const int stride = ::stride(h);
        int nframes = 1;
        for (int i = 0; i < n; ++i) {
            const int32_t *r = records + (size_t)i * stride;
            if (r[0] < 0 || (i > 0 && r[0] < records[(size_t)(i - 1) * stride]) || r[6] < 1 || r[6] > h->max_parts)
                return fail(h, PBD_ERR_INVALID, "record %d: frame %d, nparts %d (frames ascending from 0, 1..%d parts)", i, r[0], r[6],
                            h->max_parts);
            nframes = r[0] + 1;
        }
        if (nframes > 65536) return fail(h, PBD_ERR_INVALID, "%d frames", nframes);
        const int in_cap = std::max(n, 1);
        HIPCHK(h, h->dbg_in.ensure(((size_t)in_cap * stride + 1) * sizeof(int32_t)));
        HIPCHK(h, h->dbg_out.ensure(((size_t)capacity * stride + 1) * sizeof(int32_t)));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(h->dbg_in.p, &n, sizeof(int32_t), hipMemcpyHostToDevice));
        if (n) HIPCHK(h, hipMemcpy(h->dbg_in.as<int32_t>() + 1, records, (size_t)n * stride * sizeof(int32_t), hipMemcpyHostToDevice));
        if (int rc = enqueue_post(h, nframes, rows, cols, overlap, h->dbg_in.as<int32_t>(), in_cap, 0, h->dbg_out.as<int32_t>(), capacity,
                              h->stream)) return rc;
        HIPCHK(h, hipGetLastError());
        int kept = 0;
        HIPCHK(h, hipMemcpyAsync(&kept, h->dbg_out.p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        const int nret = std::min(kept, capacity);
        if (nret > 0) HIPCHK(h, hipMemcpy(out, h->dbg_out.as<int32_t>() + 1, (size_t)nret * stride * sizeof(int32_t), hipMemcpyDeviceToHost));
        *nout = nret;
        if (kept > capacity) return fail(h, PBD_ERR_CAPACITY, "%d records kept, capacity %d", kept, capacity);
        return PBD_OK;
    });
}

// forces one of the handle's launch choices (tests: every distance-transform variant, DP chunking on small batches, the two-pass HOG);
// each option's default value restores the automatic choice
enum { PBD_DEBUG_DT_LANE_SHIFT = 0, PBD_DEBUG_DT_COOP = 1, PBD_DEBUG_DT_COOP_G = 2, PBD_DEBUG_DP_BUDGET_MB = 3,
       PBD_DEBUG_GRID_NMS_LANES = 4, PBD_DEBUG_HOG_TWO_PASS = 5 };
int pbd_debug_set_option(pbd_handle *h, int option, int value)
{
    return entry(h, true, kIdle, [&]() -> int {
        switch (option) {
        case PBD_DEBUG_DT_LANE_SHIFT:   // 0..6: 64 >> value rows per wave; -1: automatic
            if (value < -1 || value > 6) break;
            h->dt_opt.lane_shift = value;
            return PBD_OK;
        case PBD_DEBUG_DT_COOP:         // 0: never the cooperative kernel; 1: when it fits
            if (value != 0 && value != 1) break;
            h->dt_opt.coop = value != 0;
            return PBD_OK;
        case PBD_DEBUG_DT_COOP_G:       // 4 or 8 rows per wave of the cooperative kernel; 0: automatic
            if (value != 0 && value != 4 && value != 8) break;
            h->dt_opt.coop_g = value;
            return PBD_OK;
        case PBD_DEBUG_DP_BUDGET_MB:    // DP scratch per chunk of frames in MB; 0: 8 GB
            if (value < 0) break;
            h->dp_budget_mb = value;
            return PBD_OK;
        case PBD_DEBUG_GRID_NMS_LANES:  // 1 or 64 lanes per block of k_grid_nms; 0: by the window size
            if (value != 0 && value != 1 && value != 64) break;
            h->gn_lanes = value;
            return PBD_OK;
        case PBD_DEBUG_HOG_TWO_PASS:    // 1: the histogram stage never takes the fused gradient + histogram kernel; 0: where it applies
            if (value != 0 && value != 1) break;
            h->hog_two_pass = value != 0;
            return PBD_OK;
        default:
            return fail(h, PBD_ERR_INVALID, "debug option %d unknown", option);
        }
        return fail(h, PBD_ERR_INVALID, "debug option %d: value %d out of range", option, value);
    });
}

const char *pbd_last_error(const pbd_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int pbd_create(const pbd_model *model, const pbd_config *config, pbd_handle **out)
{
    return guarded(nullptr, [&]() -> int {
        if (!model || !config || !out) return fail(nullptr, PBD_ERR_INVALID, "null argument");
        *out = nullptr;
        if (config->real_type != PBD_REAL_F32 && config->real_type != PBD_REAL_F64)
            return fail(nullptr, PBD_ERR_UNSUPPORTED, "real_type %d: PBD_REAL_F32 or PBD_REAL_F64", config->real_type);
        if (config->conv_mode == PBD_CONV_MFMA_F64 && config->real_type != PBD_REAL_F64)
            return fail(nullptr, PBD_ERR_UNSUPPORTED, "PBD_CONV_MFMA_F64 needs PBD_REAL_F64 (fp64 operands and accumulation)");
        if (conv_is_any(config->conv_mode) && config->real_type != PBD_REAL_F32)
            return fail(nullptr, PBD_ERR_UNSUPPORTED, "PBD_CONV_MFMA_ANY / PBD_CONV_MFMA_F16_ANY need PBD_REAL_F32; PBD_REAL_F64 has PBD_CONV_MFMA_F64");
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev < 1)
            return fail(nullptr, PBD_ERR_HIP, "no HIP device available (%s); this library has no CPU path",
                        e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        if (config->device < 0 || config->device >= ndev) return fail(nullptr, PBD_ERR_INVALID, "device %d of %d", config->device, ndev);
        e = hipSetDevice(config->device);
        if (e != hipSuccess) return fail(nullptr, PBD_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
        std::unique_ptr<pbd_handle, void (*)(pbd_handle *)> h(new pbd_handle, pbd_destroy);   // releases device memory on every exit
        h->cfg = *config;
        h->device = config->device;
        h->f64 = config->real_type == PBD_REAL_F64;
        h->rs = h->f64 ? sizeof(double) : sizeof(float);
        h->resp_half = conv_is_f16(config->conv_mode) && !h->f64;
        h->resp_es = h->resp_half ? 2 : h->rs;
        if (h->cfg.max_batch < 1) h->cfg.max_batch = 1;
        if (h->cfg.max_candidates < 1) h->cfg.max_candidates = 65536;
        if (config->stream) {
            h->stream.borrow(reinterpret_cast<hipStream_t>(config->stream));
        } else {
            e = h->stream.create();
            if (e != hipSuccess) return fail(nullptr, PBD_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        int rc = build_model(h.get(), model);
        if (rc != PBD_OK) {
            g_create_error = h->err;
            return rc;
        }
        *out = h.release();
        return PBD_OK;
    });
}

void pbd_destroy(pbd_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (hipStream_t s : {h->stream.s, h->stream_copy.s, h->stream_d2h.s})   // work in flight ends before its memory is freed
        if (s) (void)hipStreamSynchronize(s);
    try {
        h->prof.flush();
    } catch (...) {
    }
    delete h;   // the members' owners free every device, pinned, event and stream resource
}

int pbd_candidate_stride(const pbd_handle *h) { return h ? stride(h) : 0; }
int pbd_binsize(const pbd_handle *h) { return h ? h->sbin : 0; }
int pbd_num_ptr_slots(const pbd_handle *h) { return h ? h->NS : 0; }
int pbd_ptr_slot(const pbd_handle *h, int component, int part)
{
    if (!h || component < 0 || component >= h->NC) return -1;
    const int p0 = h->part_offset[component];
    if (part < 0 || p0 + part >= h->part_offset[component + 1]) return -1;
    return h->ptr_slot[p0 + part];
}

int pbd_set_level_shard(pbd_handle *h, int rank, int world)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (world < 1 || rank < 0 || rank >= world) return fail(h, PBD_ERR_INVALID, "level shard %d of %d", rank, world);
        if (world > 1 && h->nms)
            return fail(h, PBD_ERR_UNSUPPORTED, "level sharding with non-maxima suppression on: suppression of one rank's levels "
                        "is not suppression of the union (pbd_set_nms(h, 0, ...) first)");
        if (world > 1 && h->scale_nms >= 0)
            return fail(h, PBD_ERR_UNSUPPORTED, "level sharding with scale NMS on: one rank does not hold the neighbouring levels "
                        "(pbd_set_scale_nms(h, 0, 0) first; pbd_scale_nms on the merged list)");
        if (rank == h->shard_rank && world == h->shard_world) return PBD_OK;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->shard_rank = rank; h->shard_world = world;
        // image plans depend on the shard
        h->res.clear();
        for (size_t i = 0; i < h->plans.size();)
            if (h->plans[i]->kind == 0) h->plans.erase(h->plans.begin() + i); else ++i;
        return PBD_OK;
    });
}

int pbd_set_padding(pbd_handle *h, int padx, int pady)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (padx < 0 || padx > kConvMaxK || pady < 0 || pady > kConvMaxK)
            return fail(h, PBD_ERR_INVALID, "padding (%d, %d) outside 0..%d", padx, pady, kConvMaxK);
        if ((padx || pady) && h->dprune)
            return fail(h, PBD_ERR_UNSUPPORTED, "a padded pyramid with depth pruning on (pbd_set_depth_prune(h, NULL) first)");
        if (padx == h->padx && pady == h->pady) return PBD_OK;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->padx = padx; h->pady = pady;
        // every plan carries the pad it was built with (the explicit-size plans too: their walks take it off)
        h->res.clear();
        h->plans.clear();
        if (h->lat) {
            h->lat->padx = padx; h->lat->pady = pady;
            h->lat->res.clear();
            h->lat->plans.clear();
        }
        return PBD_OK;
    });
}

int pbd_set_fine_octave(pbd_handle *h, int enable)
{
    return entry(h, true, kIdle, [&]() -> int {
        const bool on = enable != 0;
        if (on && (h->sbin < 4 || h->sbin % 2))
            return fail(h, PBD_ERR_UNSUPPORTED, "a fine octave at bin size %d: sbin / 2 must be an integer >= 2", h->sbin);
        if (on == h->fine_octave) return PBD_OK;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->fine_octave = on;
        // every image plan carries the levels it was built with
        h->res.clear();
        h->plans.clear();
        if (h->lat) {
            h->lat->fine_octave = on;
            h->lat->res.clear();
            h->lat->plans.clear();
        }
        return PBD_OK;
    });
}

int pbd_set_nms(pbd_handle *h, int enable, float overlap)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (std::isnan(overlap)) return fail(h, PBD_ERR_INVALID, "overlap is NaN");
        if (enable && h->shard_world > 1)
            return fail(h, PBD_ERR_UNSUPPORTED, "non-maxima suppression with level sharding (world %d): suppression of one rank's "
                        "levels is not suppression of the union", h->shard_world);
        h->nms = enable != 0;
        h->nms_overlap = overlap;
        return PBD_OK;
    });
}

int pbd_set_root_nms(pbd_handle *h, int sz)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (sz < 0 || sz > 32767) return fail(h, PBD_ERR_INVALID, "root NMS window %d (0: off, 1..32767)", sz);
        h->root_nms = sz;                 // the resident result stays: the planes do not depend on it
        return PBD_OK;
    });
}

int pbd_set_top_k(pbd_handle *h, int k)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (k < 0 || k > (1 << 30)) return fail(h, PBD_ERR_INVALID, "top-K %d (0: off, 1..2^30)", k);
        h->top_k = k;                     // the resident result stays: the planes do not depend on it
        return PBD_OK;
    });
}

int pbd_set_scale_nms(pbd_handle *h, int enable, int dl)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (dl < 0 || dl > 255) return fail(h, PBD_ERR_INVALID, "scale NMS level distance %d (0..255)", dl);
        if (enable && h->shard_world > 1)
            return fail(h, PBD_ERR_UNSUPPORTED, "scale NMS with level sharding (world %d): one rank does not hold the neighbouring "
                        "levels (pbd_scale_nms on the merged list)", h->shard_world);
        h->scale_nms = enable ? dl : -1;  // the resident result stays: the planes do not depend on it
        return PBD_OK;
    });
}

int pbd_set_depth_prune(pbd_handle *h, const pbd_depth_prune_cfg *cfg)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (!cfg) { h->dprune = false; return PBD_OK; }
        if (h->padx || h->pady)
            return fail(h, PBD_ERR_UNSUPPORTED, "depth pruning on a padded pyramid (pbd_set_padding(h, 0, 0) first)");
        if (int rc = depth_prune_rule(h, *cfg, &h->dprune_rule)) return rc;   // (a refused cfg leaves the setting as it was)
        h->dprune = true;                 // the resident result stays: it does not depend on the setting
        return PBD_OK;
    });
}

int pbd_set_walk(pbd_handle *h, int mode)
{
    return entry(h, true, kIdle, [&]() -> int {
        if (mode != PBD_WALK_REFERENCE && mode != PBD_WALK_ARGMAX) return fail(h, PBD_ERR_INVALID, "walk mode %d", mode);
        h->walk_mode = mode;              // the resident result stays: the planes do not depend on the walk
        if (h->lat) h->lat->walk_mode = mode;
        return PBD_OK;
    });
}

int pbd_pyramid_plan(pbd_handle *h, int rows, int cols, int *nlevels, int *img_rows, int *img_cols, int *feat_rows,
                     int *feat_cols, float *scales)
{
    return entry(h, nlevels, kBusyOk, [&]() -> int {
        Plan *P = nullptr;
        if (int rc = get_image_plan(h, rows, cols, &P)) return rc;
        *nlevels = P->nlevels;
        for (int l = 0; l < P->nlevels; ++l) {
            if (img_rows) img_rows[l] = P->lv[l].img_rows;
            if (img_cols) img_cols[l] = P->lv[l].img_cols;
            if (feat_rows) feat_rows[l] = P->lv[l].rows;
            if (feat_cols) feat_cols[l] = P->lv[l].cols;
            if (scales) scales[l] = P->scales[l];
        }
        return PBD_OK;
    });
}

int pbd_features_pyramid(pbd_handle *h, const void *img, int rows, int cols, int channels, size_t stride_bytes,
                         int depth_code, void *const *feat)
{
    return entry(h, img && feat, kIdle, [&]() -> int {
        const FrameSrc src{&img, stride_bytes, nullptr};
        Plan *P = nullptr;
        if (int rc = check_frames(h, 1, src, rows, cols, channels, depth_code)) return rc;
        if (int rc = get_image_plan(h, rows, cols, &P)) return rc;
        if (int rc = enqueue_features(h, *P, 1, src, channels, depth_code)) return rc;
        for (int l = 0; l < P->nlevels; ++l) {
            const LevelDesc &d = P->lv[l];
            const size_t n = (size_t)d.rows * d.cols * 32;
            if (n && feat[l])
                HIPCHK(h, hipMemcpyAsync(feat[l], h->feat.as<char>() + (size_t)d.cell_off * 32 * h->rs, n * h->rs,
                                         hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_get_pyramid_image(pbd_handle *h, int frame, int level, uint8_t *dst)
{
    return entry(h, dst, kIdle, [&]() -> int {
        const Resident &r = h->res;
        if (!r.plan || (r.plan->kind != 0 && r.plan->kind != 2) || !r.features) return fail(h, PBD_ERR_STATE, "no pyramid has been computed");
        const Plan &P = *r.plan;
        if (!resident_level(r, frame, level, &frame, &level)) return fail(h, PBD_ERR_INVALID, "frame/level out of range");
        const LevelDesc &d = P.lv[level];
        const size_t es = depth_size(r.depth);
        HIPCHK(h, hipMemcpyAsync(dst, h->pyr.as<uint8_t>() + ((size_t)frame * P.pix_per_frame + d.img_off) * r.cn * es,
                                 (size_t)d.img_rows * d.img_cols * r.cn * es, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_conv_set_filters(pbd_handle *h, int nfilters, const void *const *filters, const int *ksize)
{
    return entry(h, filters && ksize, kIdle, [&]() -> int {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (int rc = upload_filters(h, nfilters, filters, ksize)) return rc;
        h->res.drop_conv();   // the resident responses were those of the old bank
        if (h->lat) h->lat->res.drop_conv();   // a latent result lives in the twin: it goes as it does after a model update
        return revalidate_bank(h);
    });
}

int pbd_conv_pdf(pbd_handle *h, int nlevels, const void *const *feat, const int *rows, const int *cols, void *const *resp)
{
    return entry(h, feat && rows && cols && resp, kIdle, [&]() -> int {
        Plan *P = nullptr;
        if (int rc = get_dims_plan(h, nlevels, rows, cols, &P)) return rc;
        h->res = Resident{P, 1};
        HIPCHK(h, h->feat.ensure(std::max<size_t>((size_t)P->cell_per_frame * 32 * h->rs, 16)));
        for (int l = 0; l < nlevels; ++l) {
            const size_t n = (size_t)rows[l] * cols[l] * 32;
            if (n) HIPCHK(h, hipMemcpyAsync(h->feat.as<char>() + (size_t)P->lv[l].cell_off * 32 * h->rs, feat[l], n * h->rs,
                                            hipMemcpyHostToDevice, h->stream));
        }
        h->res.features = true;
        if (int rc = run_conv(h, *P, 1)) return rc;
        for (int l = 0; l < nlevels; ++l) {
            const char *src = h->resp.as<char>() + (size_t)P->lv[l].cell_off * h->F * h->resp_es;
            if (int rc = read_responses(h, resp[l], src, (size_t)rows[l] * cols[l] * h->F)) return rc;
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_dp_min(pbd_handle *h, int nlevels, const int *rows, const int *cols, const void *const *resp, int32_t *const *Ix,
               int32_t *const *Iy, int32_t *const *Ik, void *const *rootv, int32_t *const *rooti)
{
    return entry(h, rows && cols && resp, kIdle, [&]() -> int {
        if (int rc = check_bank(h)) return rc;
        Plan *P = nullptr;
        if (int rc = get_dims_plan(h, nlevels, rows, cols, &P)) return rc;
        h->res = Resident{P, 1};
        HIPCHK(h, h->resp.ensure(std::max<size_t>((size_t)P->cell_per_frame * h->F * h->resp_es, 16) + 32));
        std::vector<uint16_t> halfbuf;
        for (int l = 0; l < nlevels; ++l) {
            const size_t n = (size_t)rows[l] * cols[l] * h->F;
            if (!n) continue;
            char *dst = h->resp.as<char>() + (size_t)P->lv[l].cell_off * h->F * h->resp_es;
            if (h->resp_half) {      // the device side of this mode reads fp16 responses (exact for what pbd_conv_pdf returned)
                halfbuf.resize(n);
                const float *src = static_cast<const float *>(resp[l]);
                for (size_t i = 0; i < n; ++i) halfbuf[i] = host_f2h(src[i]);
                HIPCHK(h, hipMemcpy(dst, halfbuf.data(), n * 2, hipMemcpyHostToDevice));
            } else {
                HIPCHK(h, hipMemcpyAsync(dst, resp[l], n * h->rs, hipMemcpyHostToDevice, h->stream));
            }
        }
        h->res.resp = true;
        if (int rc = run_dp(h, *P, 1)) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<uint8_t> t8;
        for (int l = 0; l < nlevels; ++l) {
            const size_t hw = (size_t)rows[l] * cols[l];
            if (!hw) continue;
            const size_t n = hw * h->NS, off = (size_t)P->lv[l].cell_off * h->NS;
            if (n) {
                t8.resize(n);
                // the device keeps the winning mixture per slot (Ik) and the transform's own pointer planes per (part, mixture);
                // the reference's Ix / Iy of a slot are composed here: Ix = IxRaw[k][y][x], Iy = IyRaw[k][y][Ix], k = Ik
                HIPCHK(h, hipMemcpy(t8.data(), h->Ik.as<uint8_t>() + off, n, hipMemcpyDeviceToHost));
                std::vector<uint8_t> ik(t8.begin(), t8.begin() + n);
                if (Ik && Ik[l]) for (size_t i = 0; i < n; ++i) Ik[l][i] = ik[i];
                if ((Ix && Ix[l]) || (Iy && Iy[l])) {
                    const size_t nj = hw * h->totmix, joff = (size_t)P->lv[l].cell_off * h->totmix;
                    std::vector<int> px(nj), py(nj);
                    auto fetch_planes = [&](const DevBuf &src, std::vector<int> &dst) -> hipError_t {
                        if (P->ptr8) {
                            std::vector<uint8_t> b(nj);
                            hipError_t e = hipMemcpy(b.data(), src.as<uint8_t>() + joff, nj, hipMemcpyDeviceToHost);
                            if (e != hipSuccess) return e;
                            for (size_t i = 0; i < nj; ++i) dst[i] = b[i];
                            return hipSuccess;
                        }
                        std::vector<int16_t> b(nj);
                        hipError_t e = hipMemcpy(b.data(), src.as<int16_t>() + joff, nj * 2, hipMemcpyDeviceToHost);
                        if (e != hipSuccess) return e;
                        for (size_t i = 0; i < nj; ++i) dst[i] = b[i];
                        return hipSuccess;
                    };
                    HIPCHK(h, fetch_planes(h->IxRaw, px));
                    HIPCHK(h, fetch_planes(h->IyRaw, py));
                    const int Wl = cols[l];
                    const int totparts = (int)h->parentid.size();
                    for (int gp = 0; gp < totparts; ++gp) {
                        bool root = false;
                        for (int c = 0; c < h->NC; ++c) root = root || gp == h->part_offset[c];
                        if (root) continue;
                        int c = 0;
                        while (c + 1 < h->NC && h->part_offset[c + 1] <= gp) ++c;
                        const int gpar = h->part_offset[c] + h->parentid[gp];
                        const int L = h->mix_offset[gpar + 1] - h->mix_offset[gpar];
                        for (int pm = 0; pm < L; ++pm) {
                            const size_t so = (size_t)(h->ptr_slot[gp] + pm) * hw;
                            for (size_t cell = 0; cell < hw; ++cell) {
                                const size_t plane = (size_t)(h->mix_offset[gp] + ik[so + cell]) * hw;
                                const int x = px[plane + (cell % Wl) * (size_t)rows[l] + cell / Wl];      // IxRaw is kept transposed
                                if (Ix && Ix[l]) Ix[l][so + cell] = x;
                                if (Iy && Iy[l]) Iy[l][so + cell] = py[plane + (cell / Wl) * Wl + x];
                            }
                        }
                    }
                }
            }
            const size_t roff = (size_t)P->lv[l].cell_off * h->NC;
            if (rootv && rootv[l]) HIPCHK(h, hipMemcpy(rootv[l], h->rootv.as<char>() + roff * h->rs, hw * h->NC * h->rs, hipMemcpyDeviceToHost));
            if (rooti && rooti[l]) HIPCHK(h, hipMemcpy(rooti[l], h->rooti.as<int>() + roff, hw * h->NC * sizeof(int), hipMemcpyDeviceToHost));
        }
        return PBD_OK;
    });
}

int pbd_dp_argmin(pbd_handle *h, const float *scales, int32_t *cand, int capacity, int *ncand)
{
    return entry(h, scales && cand && ncand, kIdle, [&]() -> int {
        if (!h->res.plan || !h->res.dp) return fail(h, PBD_ERR_STATE, "argmin() before min()");
        if (h->res.plan->kind == 2)
            return fail(h, PBD_ERR_STATE, "argmin() after a mixed-size call: DynamicProgram::argmin takes the scales of one image");
        Plan &P = *h->res.plan;
        HIPCHK(h, h->scales_tmp.ensure(sizeof(float) * PBD_MAX_LEVELS));
        HIPCHK(h, hipMemcpyAsync(h->scales_tmp.p, scales, sizeof(float) * P.nlevels, hipMemcpyHostToDevice, h->stream));
        return run_argmin(h, P, h->res.frames, h->scales_tmp.as<float>(), false, RootSel{}, cand, capacity, ncand);   // no suppression, no root NMS (DynamicProgram::argmin)
    });
}

int pbd_detect(pbd_handle *h, const void *img, int rows, int cols, int channels, size_t stride_bytes, int32_t *cand,
               int capacity, int *ncand)
{
    return pbd_detect_batch(h, 1, &img, rows, cols, channels, stride_bytes, cand, capacity, ncand);
}

int pbd_detect_batch(pbd_handle *h, int nframes, const void *const *imgs, int rows, int cols, int channels,
                     size_t stride_bytes, int32_t *cand, int capacity, int *ncand)
{
    return entry(h, imgs && cand && ncand, kIdle, [&]() -> int {
        return detect_sync(h, nframes, FrameSrc{imgs, stride_bytes, nullptr}, rows, cols, channels, kDepth8U, cand, capacity, ncand);
    });
}

int pbd_detect_batch_device(pbd_handle *h, int nframes, const void *d_frames, int rows, int cols, int channels,
                            int32_t *cand, int capacity, int *ncand)
{
    return entry(h, d_frames && cand && ncand, kIdle, [&]() -> int {
        return detect_sync(h, nframes, FrameSrc{nullptr, 0, d_frames}, rows, cols, channels, kDepth8U, cand, capacity, ncand);
    });
}

int pbd_detect_typed(pbd_handle *h, const void *img, int rows, int cols, int channels, size_t stride_bytes, int depth_code,
                     int32_t *cand, int capacity, int *ncand)
{
    return entry(h, img && cand && ncand, kIdle, [&]() -> int {
        return detect_sync(h, 1, FrameSrc{&img, stride_bytes, nullptr}, rows, cols, channels, depth_code, cand, capacity, ncand);
    });
}

// what submit() does once the batch has passed check_detect and its frames are (being) made resident at d_frames: the
// whole path, the candidates' read-back and the slot's completion event, all enqueued on the handle's stream without waiting
static int submit_enqueue(pbd_handle *h, pbd_handle::Slot &S, Plan &P, int nframes, const void *d_frames, int channels)
{
    if (!S.done.p) HIPCHK(h, hipEventCreateWithFlags(&S.done.p, hipEventDisableTiming));
    if (int rc = enqueue_detect(h, P, nframes, FrameSrc{nullptr, 0, d_frames}, channels, kDepth8U)) return rc;
    if (int rc = enqueue_argmin_readback(h, P, nframes, P.d_scales.p, S.cb, h->nms, root_sel(h), h->stream)) return rc;
    HIPCHK(h, hipEventRecord(S.done.p, h->stream));
    HIPCHK(h, hipGetLastError());
    h->nsubmitted += 1;
    return PBD_OK;
}

int pbd_detect_batch_submit(pbd_handle *h, int nframes, const void *const *imgs, int rows, int cols, int channels,
                            size_t stride_bytes)
{
    return entry(h, imgs, kBusyOk, [&]() -> int {
        if (h->nsubmitted - h->nwaited >= 2) return fail(h, PBD_ERR_STATE, "two batches are already in flight: call pbd_detect_batch_wait first");
        Plan *P = nullptr;
        if (int rc = claim_depth(h, nframes, rows, cols)) return rc;
        if (int rc = check_detect(h, nframes, FrameSrc{imgs, stride_bytes, nullptr}, rows, cols, channels, kDepth8U, &P)) return rc;
        const size_t row_bytes = (size_t)cols * channels, frame_bytes = row_bytes * rows, bytes = frame_bytes * nframes;
        pbd_handle::Slot &S = h->slot[h->nsubmitted & 1];
        if (!h->stream_copy.s) HIPCHK(h, h->stream_copy.create());
        if (!S.copied.p) HIPCHK(h, hipEventCreateWithFlags(&S.copied.p, hipEventDisableTiming));
        HIPCHK(h, S.pinned.ensure(bytes, bytes + bytes / 8));
        HIPCHK(h, S.frames.ensure(bytes));
        // host staging (this is what overlaps the kernels of the batch submitted before), then one asynchronous copy
        for (int i = 0; i < nframes; ++i) {
            char *dst = S.pinned.as<char>() + (size_t)i * frame_bytes;
            const char *src = static_cast<const char *>(imgs[i]);
            if (stride_bytes == row_bytes) memcpy(dst, src, frame_bytes);
            else for (int y = 0; y < rows; ++y) memcpy(dst + (size_t)y * row_bytes, src + (size_t)y * stride_bytes, row_bytes);
        }
        HIPCHK(h, hipMemcpyAsync(S.frames.p, S.pinned.p, bytes, hipMemcpyHostToDevice, h->stream_copy));
        HIPCHK(h, hipEventRecord(S.copied.p, h->stream_copy));
        HIPCHK(h, hipStreamWaitEvent(h->stream, S.copied.p, 0));
        return submit_enqueue(h, S, *P, nframes, S.frames.p, channels);
    });
}

int pbd_detect_batch_device_submit(pbd_handle *h, int nframes, const void *d_frames, int rows, int cols, int channels)
{
    return entry(h, d_frames, kBusyOk, [&]() -> int {
        if (h->nsubmitted - h->nwaited >= 2) return fail(h, PBD_ERR_STATE, "two batches are already in flight: call pbd_detect_batch_wait first");
        Plan *P = nullptr;
        if (int rc = claim_depth(h, nframes, rows, cols)) return rc;
        if (int rc = check_detect(h, nframes, FrameSrc{nullptr, 0, d_frames}, rows, cols, channels, kDepth8U, &P)) return rc;
        return submit_enqueue(h, h->slot[h->nsubmitted & 1], *P, nframes, d_frames, channels);
    });
}

int pbd_detect_batch_wait(pbd_handle *h, int32_t *cand, int capacity, int *ncand)
{
    return entry(h, cand && ncand, kBusyOk, [&]() -> int {
        if (h->nsubmitted == h->nwaited) return fail(h, PBD_ERR_STATE, "no batch in flight");
        pbd_handle::Slot &S = h->slot[h->nwaited & 1];
        h->nwaited += 1;                       // the slot is released whatever happens below
        HIPCHK(h, hipEventSynchronize(S.done.p));
        if (!h->stream_d2h.s) HIPCHK(h, h->stream_d2h.create());
        // (a list longer than the speculative copy is fetched on a stream of its own: the compute stream may already hold
        //  the next batch, whose kernels this copy must not queue behind -- and they do not touch this slot's payload)
        return argmin_deliver(h, S.cb, h->stream_d2h, cand, capacity, ncand);
    });
}

// Device-resident output (new surface, for multi-GPU jobs and device pipelines): the whole path with the candidate list
// left ON THE DEVICE in the caller's buffer; asynchronous.  See include/pbd.h.
int pbd_detect_batch_device_out(pbd_handle *h, int nframes, const void *d_frames, int rows, int cols, int channels,
                                int frame_offset, int32_t *d_payload, int capacity)
{
    return entry(h, d_frames && d_payload, kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        const FrameSrc src{nullptr, 0, d_frames};
        Plan *P = nullptr;
        if (int rc = claim_depth(h, nframes, rows, cols)) return rc;
        if (int rc = check_detect(h, nframes, src, rows, cols, channels, kDepth8U, &P)) return rc;
        if (int rc = enqueue_detect(h, *P, nframes, src, channels, kDepth8U)) return rc;
        if (int rc = enqueue_argmin_out(h, *P, nframes, frame_offset, d_payload, capacity)) return rc;
        HIPCHK(h, hipGetLastError());
        return PBD_OK;
    });
}

int pbd_argmin_device_out(pbd_handle *h, int frame_offset, int32_t *d_payload, int capacity)
{
    return entry(h, d_payload, kIdle, [&]() -> int {
        const Resident &r = h->res;
        if (!r.plan || !r.dp || (r.plan->kind != 0 && r.plan->kind != 2)) return fail(h, PBD_ERR_STATE, "no detect result is resident on the device");
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        const Plan &RP = *r.plan;   // the resident frames' sizes: a mixed plan's own, else the plan's for every frame
        if (int rc = RP.kind == 2 ? claim_depth(h, RP.mixed_frames, [&](int f) { return std::make_pair(RP.fdim[f].x, RP.fdim[f].y); })
                                  : claim_depth(h, r.frames, RP.rows, RP.cols)) return rc;
        if (int rc = enqueue_argmin_out(h, *r.plan, r.frames, frame_offset, d_payload, capacity)) return rc;
        HIPCHK(h, hipGetLastError());
        return PBD_OK;
    });
}

// Mixed-size calls (new surface): nframes frames of any sizes, planned as one virtual frame.  See include/pbd.h.
int pbd_detect_frames(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, int32_t *cand, int capacity,
                      int *ncand)
{
    return entry(h, frames && cand && ncand, kIdle, [&]() -> int {
        Plan *P = nullptr;
        if (int rc = claim_depth(h, nframes, frames)) return rc;
        if (int rc = check_frames_mixed(h, nframes, frames, channels, depth_code, true, &P)) return rc;
        if (int rc = enqueue_detect_mixed(h, *P, nframes, frames, channels, depth_code, true)) return rc;
        return run_argmin(h, *P, 1, P->d_scales.p, h->nms, root_sel(h), cand, capacity, ncand);
    });
}

int pbd_detect_frames_device(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, int32_t *cand,
                             int capacity, int *ncand)
{
    return entry(h, frames && cand && ncand, kIdle, [&]() -> int {
        Plan *P = nullptr;
        if (int rc = claim_depth(h, nframes, frames)) return rc;
        if (int rc = check_frames_mixed(h, nframes, frames, channels, depth_code, false, &P)) return rc;
        if (int rc = enqueue_detect_mixed(h, *P, nframes, frames, channels, depth_code, false)) return rc;
        return run_argmin(h, *P, 1, P->d_scales.p, h->nms, root_sel(h), cand, capacity, ncand);
    });
}

int pbd_detect_frames_device_out(pbd_handle *h, int nframes, const pbd_frame *frames, int channels, int depth_code, int frame_offset,
                                 int32_t *d_payload, int capacity)
{
    return entry(h, frames && d_payload, kIdle, [&]() -> int {
        if (capacity < 0) return fail(h, PBD_ERR_INVALID, "capacity %d", capacity);
        Plan *P = nullptr;
        if (int rc = claim_depth(h, nframes, frames)) return rc;
        if (int rc = check_frames_mixed(h, nframes, frames, channels, depth_code, false, &P)) return rc;
        if (int rc = enqueue_detect_mixed(h, *P, nframes, frames, channels, depth_code, false)) return rc;
        if (int rc = enqueue_argmin_out(h, *P, 1, frame_offset, d_payload, capacity)) return rc;
        HIPCHK(h, hipGetLastError());
        return PBD_OK;
    });
}

void *pbd_stream(const pbd_handle *h) { return h ? reinterpret_cast<void *>(h->stream.s) : nullptr; }

int pbd_get_stage(pbd_handle *h, int stage, int frame, int level, void *dst, size_t dst_bytes)
{
    return entry(h, dst, kIdle, [&]() -> int {
        pbd_handle *o = resident_owner(h);   // after pbd_detect_latent the twin: its features, masked responses and root planes
        const Resident &r = o->res;
        // (a model update drops the twin's responses and maps: nothing of a latent result is readable then)
        if (!r.plan || (o != h && !(r.resp && r.dp))) return fail(h, PBD_ERR_STATE, "nothing has been computed");
        const Plan &P = *r.plan;
        if (!resident_level(r, frame, level, &frame, &level)) return fail(h, PBD_ERR_INVALID, "frame/level out of range");
        const LevelDesc &d = P.lv[level];
        const size_t hw = (size_t)d.rows * d.cols, cell = (size_t)frame * P.cell_per_frame + d.cell_off;
        const void *src = nullptr;
        size_t bytes = 0;
        switch (stage) {
        case PBD_STAGE_FEATURES:
            if (!r.features) return fail(h, PBD_ERR_STATE, "features not computed");
            src = o->feat.as<char>() + cell * 32 * h->rs; bytes = hw * 32 * h->rs; break;
        case PBD_STAGE_RESPONSES:
            if (!r.resp) return fail(h, PBD_ERR_STATE, "responses not computed");
            src = o->resp.as<char>() + cell * o->F * o->resp_es; bytes = hw * o->F * h->rs; break;
        case PBD_STAGE_ROOTV:
            if (!r.dp) return fail(h, PBD_ERR_STATE, "dp not computed");
            src = o->rootv.as<char>() + cell * o->NC * h->rs; bytes = hw * o->NC * h->rs; break;
        case PBD_STAGE_ROOTI:
            if (!r.dp) return fail(h, PBD_ERR_STATE, "dp not computed");
            src = o->rooti.as<int>() + cell * o->NC; bytes = hw * o->NC * sizeof(int); break;
        default: return fail(h, PBD_ERR_INVALID, "unknown stage %d", stage);
        }
        if (dst_bytes < bytes) return fail(h, PBD_ERR_INVALID, "destination holds %zu bytes, need %zu", dst_bytes, bytes);
        if (stage == PBD_STAGE_RESPONSES) {
            if (int rc = read_responses(h, dst, src, hw * o->F)) return rc;
        } else if (bytes) {
            HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

int pbd_profile_enable(pbd_handle *h, int on)
{
    return entry(h, true, kBusyOk, [&]() -> int {
        h->prof.flush();
        h->prof.on = on == 2 ? 2 : (on != 0 ? 1 : 0);
        return PBD_OK;
    });
}
int pbd_profile_reset(pbd_handle *h)
{
    return entry(h, true, kBusyOk, [&]() -> int {
        h->prof.flush();
        for (int k = 0; k < PBD_K_COUNT; ++k) { h->prof.total[k] = 0; h->prof.launches[k] = 0; }
        return PBD_OK;
    });
}
int pbd_profile_read(pbd_handle *h, int k, double *total_ms, int *launches)
{
    return entry(h, k >= 0 && k < PBD_K_COUNT, kBusyOk, [&]() -> int {
        h->prof.flush();
        if (total_ms) *total_ms = h->prof.total[k];
        if (launches) *launches = h->prof.launches[k];
        return PBD_OK;
    });
}
const char *pbd_kernel_name(int k)
{
    static const char *names[PBD_K_COUNT] = {"k_resize", "k_pyrdown", "k_hog_hist", "k_hog_feat", "k_conv", "k_dt_rows",
                                             "k_dt_cols", "k_dp_combine", "k_dp_root", "k_argmin", "k_camera_boxes",
                                             "k_cl_crop_count", "k_cl_crop_scan", "k_cl_crop_scatter", "k_cl_clear", "k_cl_grid_count",
                                             "k_cl_grid_scan", "k_cl_grid_scatter", "k_cl_hook", "k_cl_label", "k_cl_best", "k_cl_select",
                                             "k_cl_out", "k_dc_classify", "k_dc_select", "k_dc_compact", "k_mk_hull", "k_mk_tile",
                                             "k_part_poses", "k_ex_walk", "k_ex_gather", "k_qp_write", "k_qp_score",
                                             "k_qp_pass", "k_qp_lincomb", "k_qp_slots", "k_qp_norm", "k_qp_wraw",
                                             "k_qp_gather", "k_warp", "k_warp_emit", "k_ev_nms_select", "k_ev_nms_pairs",
                                             "k_ev_nms_greedy", "k_ev_nms_emit", "k_ev_best", "k_ev_pck", "k_ev_apk_rank",
                                             "k_ev_apk_close", "k_ev_apk_ap", "k_qp_hinge", "k_km_trials", "k_km_pick",
                                             "k_grid_nms", "k_top_k", "k_depth_prune", "k_mm_dt_rows", "k_mm_dt_cols",
                                             "k_mm_messages", "k_mm_context", "k_mm_down", "k_mm_decode", "k_scale_nms"};
    return (k >= 0 && k < PBD_K_COUNT) ? names[k] : "?";
}
int pbd_synchronize(pbd_handle *h)
{
    return entry(h, true, kBusyOk, [&]() -> int {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return PBD_OK;
    });
}

}  // extern "C"
