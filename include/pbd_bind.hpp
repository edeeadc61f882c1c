// pbd_bind.hpp -- the bodies of every C++ binding of the C ABI (pbd.h), written ONCE over a small traits type.
//
// Two hosts instantiate these templates:
//   * include/pbd_host.hpp            Tr = pbdhost::HostTraits<T>   (plain buffers, no OpenCV) -- compiled into
//                                     host/pbd_demo and run on the GPU by tests/test_host_demo.py, T = float and double
//   * include/pbd_opencv_adapters.hpp Tr = pbd_adapters::CvTraits<T> (cv::Mat)                  -- what a maintainer of the
//                                     reference adds; it supplies ONLY the cv::Mat traits and class shells
// so the code that crosses the ABI in the OpenCV adapters is the code the tests ran.  No OpenCV, no Boost, C++03-clean.
//
// What a traits type Tr provides (T = the detector's real type, `PartsBasedDetector<T>`: float as src/demo.cpp:85, double as
// cells/detect.cpp:93 / ros/Node.hpp:121):
//   typedef T Real;  typedef ... Mat;  typedef ... IMat (int32 matrix);  typedef ... Image;  typedef ... Candidate;
//   static void        create(Mat &m, int rows, int cols);        rows x cols values of T, continuous
//   static T          *ptr(Mat &m);                                first element
//   static const T    *cptr(const Mat &m);
//   static int         rows(const Mat &m);   static int cols(const Mat &m);
//   static void        icreate(IMat &m, int rows, int cols);   static int32_t *iptr(IMat &m);
//   static Mat         real_continuous(const Mat &m);              m as continuous T data (the same matrix if it already is)
//   static Mat         rows_view(Mat &m, int r0, int r1);          rows [r0, r1) of m (a view where the host has views)
//   static const void *img_data(const Image &);  img_rows / img_cols / img_channels -> int;  img_step -> size_t (bytes
//                      between rows, cv::Mat::step);  img_depth -> int (cv::Mat::depth(): 0 8U, 2 16U, 5 32F, 6 64F)
//   static void        fail(int status, const std::string &text);  throws the host's exception type; never returns
//   static void        candidate(std::vector<Candidate> &out, const pbd_candidate_hdr &hd, const int32_t *rects);
//                      appends one Candidate: hd.nparts boxes {x, y, w, h}; confidence hd.score for part 0, 0 for the others
//                      (src/DynamicProgram.cpp:241-244)
// and, for FlatModel, over the host's model class (reference: include/Model.hpp:49-122 -- the accessor names are its):
//   typedef ... FilterMat;   static int filter_rows(const FilterMat &);
//   static void        filter_values(const FilterMat &w, std::vector<double> &out);   appends rows x (rows*flen) values
#ifndef PBD_BIND_HPP_
#define PBD_BIND_HPP_

#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "pbd.h"

namespace pbdbind {

template <typename T> struct RealCode;
template <> struct RealCode<float> { enum { value = PBD_REAL_F32 }; };
template <> struct RealCode<double> { enum { value = PBD_REAL_F64 }; };

template <class Tr>
inline void check(pbd_handle *h, int rc)
{   // the C ABI never throws; the host's own error channel does (reference: assert / CV_Error -> cv::Exception)
    if (rc != PBD_OK) Tr::fail(rc, std::string("pbd: ") + pbd_last_error(h));
}

// Model -> pbd_model: the flattened Parts tables (include/Parts.hpp:103-189) + the filter pool converted to T
// (src/PartsBasedDetector.cpp:114-117).  ModelT is the reference's Model or pbdhost::Model.
template <class Tr>
struct FlatModel {
    std::vector<int> ksize, part_offset, parentid, mix_offset, filterid, biasid, defid, anchors;
    std::vector<int64_t> foff;
    std::vector<float> filters32, biasw, defw;
    std::vector<double> filters64;
    pbd_model m;

    template <class ModelT>
    explicit FlatModel(ModelT &model)
    {
        int64_t off = 0;
        for (size_t f = 0; f < model.filters().size(); ++f) {
            const typename Tr::FilterMat &w = model.filters()[f];
            ksize.push_back(Tr::filter_rows(w));
            foff.push_back(off);
            const size_t before = filters64.size();
            Tr::filter_values(w, filters64);
            off += (int64_t)(filters64.size() - before);
        }
        filters32.resize(filters64.size());
        for (size_t i = 0; i < filters64.size(); ++i) filters32[i] = (float)filters64[i];   // convertTo(CV_32F): one rounding
        biasw.assign(model.bias().begin(), model.bias().end());
        for (size_t d = 0; d < model.def().size(); ++d) {
            for (int i = 0; i < 4; ++i) defw.push_back(model.def()[d][i]);
            anchors.push_back(model.anchors()[d].x);
            anchors.push_back(model.anchors()[d].y);
        }
        part_offset.push_back(0);
        mix_offset.push_back(0);
        for (size_t c = 0; c < model.filterid().size(); ++c) {
            for (size_t p = 0; p < model.filterid()[c].size(); ++p) {
                parentid.push_back(model.parentid()[c][p]);
                const std::vector<int> &fid = model.filterid()[c][p], &bid = model.biasid()[c][p], &did = model.defid()[c][p];
                for (size_t mm = 0; mm < fid.size(); ++mm) {
                    filterid.push_back(fid[mm]);
                    biasid.push_back(mm < bid.size() ? bid[mm] : -1);
                    defid.push_back(p > 0 && mm < did.size() ? did[mm] : -1);
                }
                mix_offset.push_back(mix_offset.back() + (int)fid.size());
            }
            part_offset.push_back(part_offset.back() + (int)model.filterid()[c].size());
        }
        m.ncomponents = (int)model.filterid().size();
        m.nfilters = (int)ksize.size();
        m.flen = model.flen();
        m.filter_ksize = ksize.empty() ? NULL : &ksize[0];
        m.filter_offset = foff.empty() ? NULL : &foff[0];
        m.filters_f32 = filters32.empty() ? NULL : &filters32[0];
        m.filters_f64 = filters64.empty() ? NULL : &filters64[0];
        m.nbias = (int)biasw.size();
        m.biasw = biasw.empty() ? NULL : &biasw[0];
        m.ndefs = (int)(defw.size() / 4);
        m.defw = defw.empty() ? NULL : &defw[0];
        m.anchors = anchors.empty() ? NULL : &anchors[0];
        m.part_offset = &part_offset[0];
        m.parentid = parentid.empty() ? NULL : &parentid[0];
        m.mix_offset = &mix_offset[0];
        m.filterid = filterid.empty() ? NULL : &filterid[0];
        m.biasid = biasid.empty() ? NULL : &biasid[0];
        m.defid = defid.empty() ? NULL : &defid[0];
        m.thresh = model.thresh();
        m.sbin = model.binsize();
        m.interval = model.nscales();      // Model::nscales_ is the interval (src/FileStorageModel.cpp:105)
        m.norient = model.norient();
    }
private:
    FlatModel(const FlatModel &);
    FlatModel &operator=(const FlatModel &);
};

// pbd_create / pbd_destroy: what distributeModel owns (src/PartsBasedDetector.cpp:102-127)
template <class Tr, class ModelT>
inline pbd_handle *create(ModelT &model, int device, int conv_mode, int max_batch, int max_candidates)
{
    FlatModel<Tr> fm(model);
    pbd_config cfg = {device, RealCode<typename Tr::Real>::value, conv_mode, max_batch, max_candidates, NULL};
    pbd_handle *h = NULL;
    const int rc = pbd_create(&fm.m, &cfg, &h);
    if (rc != PBD_OK) Tr::fail(rc, std::string("pbd_create: ") + pbd_last_error(NULL));
    return h;
}

// IFeatures::pyramid(im, pyrafeatures) + scales() (include/IFeatures.hpp:49-73, src/HOGFeatures.cpp:95-127)
template <class Tr>
inline void pyramid(pbd_handle *h, const typename Tr::Image &im, std::vector<typename Tr::Mat> &pyrafeatures,
                    std::vector<float> &scales)
{
    int n = 0, fr[PBD_MAX_LEVELS], fc[PBD_MAX_LEVELS];
    float sc[PBD_MAX_LEVELS];
    check<Tr>(h, pbd_pyramid_plan(h, Tr::img_rows(im), Tr::img_cols(im), &n, NULL, NULL, fr, fc, sc));
    const int flen = 32;                                        // Mat(H, W*flen), src/HOGFeatures.cpp:180
    pyrafeatures.resize(n);
    std::vector<void *> ptrs(n);
    for (int l = 0; l < n; ++l) {
        Tr::create(pyrafeatures[l], fr[l], fc[l] * flen);
        ptrs[l] = Tr::ptr(pyrafeatures[l]);
    }
    // the depth codes of the C ABI are cv::Mat::depth() itself: 8U / 16U / 32F / 64F are the four features<IT>
    // instantiations (src/HOGFeatures.cpp:136-146); any other depth -> PBD_ERR_UNSUPPORTED (the reference's default: branch)
    check<Tr>(h, pbd_features_pyramid(h, Tr::img_data(im), Tr::img_rows(im), Tr::img_cols(im), Tr::img_channels(im),
                                      Tr::img_step(im), Tr::img_depth(im), n ? &ptrs[0] : NULL));
    scales.assign(sc, sc + n);
}

// IConvolutionEngine::setFilters (include/IConvolutionEngine.hpp:67, src/SpatialConvolutionEngine.cpp:133-159)
template <class Tr>
inline void set_filters(pbd_handle *h, const std::vector<typename Tr::Mat> &filters)
{
    const size_t F = filters.size();
    std::vector<typename Tr::Mat> real(F);                      // converted to T / made continuous, alive across the call
    std::vector<const void *> ptrs(F);
    std::vector<int> ks(F);
    for (size_t f = 0; f < F; ++f) {
        real[f] = Tr::real_continuous(filters[f]);
        ptrs[f] = Tr::cptr(real[f]);
        ks[f] = Tr::rows(real[f]);
    }
    check<Tr>(h, pbd_conv_set_filters(h, (int)F, F ? &ptrs[0] : NULL, F ? &ks[0] : NULL));
}

// IConvolutionEngine::pdf (include/IConvolutionEngine.hpp:56, src/SpatialConvolutionEngine.cpp:106-124):
// responses[level][filter] = H x W, here views of one packed matrix per level (nfilters*H rows x W)
template <class Tr>
inline void pdf(pbd_handle *h, size_t nfilters, const std::vector<typename Tr::Mat> &features,
                std::vector<std::vector<typename Tr::Mat> > &responses)
{
    const int M = (int)features.size(), flen = 32;
    std::vector<typename Tr::Mat> cont(M), packed(M);
    std::vector<const void *> fp(M);
    std::vector<void *> rp(M);
    std::vector<int> rows(M), cols(M);
    for (int m = 0; m < M; ++m) {
        cont[m] = Tr::real_continuous(features[m]);
        rows[m] = Tr::rows(cont[m]);
        cols[m] = Tr::cols(cont[m]) / flen;
        fp[m] = Tr::cptr(cont[m]);
        Tr::create(packed[m], (int)nfilters * rows[m], cols[m]);
        rp[m] = Tr::ptr(packed[m]);
    }
    check<Tr>(h, pbd_conv_pdf(h, M, M ? &fp[0] : NULL, M ? &rows[0] : NULL, M ? &cols[0] : NULL, M ? &rp[0] : NULL));
    responses.assign(M, std::vector<typename Tr::Mat>(nfilters));
    for (int m = 0; m < M; ++m)
        for (size_t n = 0; n < nfilters; ++n) responses[m][n] = Tr::rows_view(packed[m], (int)n * rows[m], (int)(n + 1) * rows[m]);
}

// DynamicProgram<T>::min (include/DynamicProgram.hpp:74, src/DynamicProgram.cpp:67-173): scores[level][filter] in,
// rootv[level][component] (T) and rooti[level][component] (int32, as a T-independent IMat) out; the back-pointers stay on
// the device for argmin().
template <class Tr>
inline void dp_min(pbd_handle *h, int nfilters, int ncomponents, const std::vector<std::vector<typename Tr::Mat> > &scores,
                   std::vector<std::vector<typename Tr::Mat> > &rootv, std::vector<std::vector<typename Tr::IMat> > &rooti)
{
    typedef typename Tr::Real T;
    const int M = (int)scores.size();
    std::vector<int> rows(M), cols(M);
    std::vector<std::vector<T> > packed(M), rv(M);
    std::vector<std::vector<int32_t> > ri(M);
    std::vector<const void *> sp(M);
    std::vector<void *> rvp(M);
    std::vector<int32_t *> rip(M);
    for (int m = 0; m < M; ++m) {
        rows[m] = Tr::rows(scores[m][0]);
        cols[m] = Tr::cols(scores[m][0]);
        const size_t hw = (size_t)rows[m] * cols[m];
        packed[m].resize(hw * nfilters + 1);
        for (int f = 0; f < nfilters; ++f) {
            const typename Tr::Mat c = Tr::real_continuous(scores[m][f]);
            const T *src = Tr::cptr(c);
            for (size_t i = 0; i < hw; ++i) packed[m][f * hw + i] = src[i];
        }
        rv[m].resize(hw * ncomponents + 1);
        ri[m].resize(hw * ncomponents + 1);
        sp[m] = &packed[m][0]; rvp[m] = &rv[m][0]; rip[m] = &ri[m][0];
    }
    check<Tr>(h, pbd_dp_min(h, M, M ? &rows[0] : NULL, M ? &cols[0] : NULL, M ? &sp[0] : NULL, NULL, NULL, NULL,
                            M ? &rvp[0] : NULL, M ? &rip[0] : NULL));
    rootv.assign(M, std::vector<typename Tr::Mat>(ncomponents));
    rooti.assign(M, std::vector<typename Tr::IMat>(ncomponents));
    for (int m = 0; m < M; ++m)
        for (int c = 0; c < ncomponents; ++c) {
            const size_t hw = (size_t)rows[m] * cols[m];
            Tr::create(rootv[m][c], rows[m], cols[m]);
            Tr::icreate(rooti[m][c], rows[m], cols[m]);
            T *dv = Tr::ptr(rootv[m][c]);
            int32_t *di = Tr::iptr(rooti[m][c]);
            for (size_t i = 0; i < hw; ++i) { dv[i] = rv[m][c * hw + i]; di[i] = ri[m][c * hw + i]; }
        }
}

// pbd_set_nms: the callers' Candidate::sort + Candidate::nonMaximaSuppression(im, candidates, overlap) (cells/detect.cpp:237-238,
// ros/Node.cpp:192-196) run on the device after every detect of this handle; enable = false: off
template <class Tr>
inline void set_nms(pbd_handle *h, bool enable, float overlap)
{
    check<Tr>(h, pbd_set_nms(h, enable ? 1 : 0, overlap));
}

// pbd_set_root_nms: the reference's commented-out ssp_.nonMaxSuppression(rootv, scales) (src/PartsBasedDetector.cpp:86) before
// every later walk of this handle: only the roots that are grid maxima within sz cells are returned; sz = 0: off
template <class Tr>
inline void set_root_nms(pbd_handle *h, int sz)
{
    check<Tr>(h, pbd_set_root_nms(h, sz));
}

// nonMaximaSuppression(src, sz, dst, mask) (src/nms.cpp:84-129) on the device (pbd_grid_nms) for one plane of T: dst receives
// rows x cols bytes of 0 / 255, rows dense; mask: NULL, or rows x cols bytes, rows dense
template <class Tr>
inline void grid_nms(pbd_handle *h, const typename Tr::Mat &src, int sz, const uint8_t *mask, uint8_t *dst)
{
    typedef typename Tr::Real T;
    const typename Tr::Mat s = Tr::real_continuous(src);
    const int rows = Tr::rows(s), cols = Tr::cols(s);
    check<Tr>(h, pbd_grid_nms(h, 1, &rows, &cols, RealCode<T>::value, Tr::cptr(s), mask, sz, dst));
}

// pbd_set_padding: every plan the handle builds afterwards pads its feature levels by (padx, pady) cells of the boundary occlusion
// feature (0 on channels 0 .. 30, 1 on channel 31), so that roots and parts can lie outside the frame; (0, 0): off
template <class Tr>
inline void set_padding(pbd_handle *h, int padx, int pady)
{
    check<Tr>(h, pbd_set_padding(h, padx, pady));
}

// pbd_set_fine_octave: every image plan the handle builds afterwards has the first `interval` levels a second time, in front, at
// bin size sbin / 2 and half the scale (objects of half the template's size); levels then index the longer list
template <class Tr>
inline void set_fine_octave(pbd_handle *h, bool on)
{
    check<Tr>(h, pbd_set_fine_octave(h, on ? 1 : 0));
}

// pbd_set_top_k: at most k candidates per frame from every later walk of this handle -- the k best roots of the frame among those
// the threshold and the other root filters leave; k = 0: off
template <class Tr>
inline void set_top_k(pbd_handle *h, int k)
{
    check<Tr>(h, pbd_set_top_k(h, k));
}

// pbd_top_k_cells for one segment, the elements of `src` in row-major order: dst receives rows x cols bytes of 0 / 255, 255 at the
// k best elements that are not NaN (and whose mask byte is non-zero); mask: NULL, or rows x cols bytes, rows dense
template <class Tr>
inline void top_k_cells(pbd_handle *h, const typename Tr::Mat &src, int k, const uint8_t *mask, uint8_t *dst)
{
    typedef typename Tr::Real T;
    const typename Tr::Mat s = Tr::real_continuous(src);
    const long long len = (long long)Tr::rows(s) * Tr::cols(s);
    check<Tr>(h, pbd_top_k_cells(h, 1, &len, RealCode<T>::value, Tr::cptr(s), mask, k, dst));
}

// pbd_top_k over n records of this handle in `buf`, in place: n becomes the kept count, the kept records stay in order; every
// record is taken as one of this frame (frame field 0)
template <class Tr>
inline void top_k(pbd_handle *h, int k, std::vector<int32_t> &buf, int &n)
{
    int kept = 0;
    check<Tr>(h, pbd_top_k(h, 1, k, n ? &buf[0] : NULL, n, 0, n ? &buf[0] : NULL, n, &kept));
    n = kept;
}

// pbd_set_scale_nms: only the roots no better root within dl pyramid levels beats whose rectangle's centre lies in its own, or the
// other way round, from every later walk of this handle (after depth pruning and root NMS, before top-K); on = false: off
template <class Tr>
inline void set_scale_nms(pbd_handle *h, bool on, int dl)
{
    check<Tr>(h, pbd_set_scale_nms(h, on ? 1 : 0, dl));
}

// pbd_scale_nms over n records of this handle in `buf`, in place: n becomes the kept count, the kept records stay in order; every
// record is taken as one of this frame (frame field 0)
template <class Tr>
inline void scale_nms(pbd_handle *h, int dl, std::vector<int32_t> &buf, int &n)
{
    int kept = 0;
    check<Tr>(h, pbd_scale_nms(h, 1, dl, n ? &buf[0] : NULL, n, 0, n ? &buf[0] : NULL, n, &kept));
    n = kept;
}

// pbd_candidate records -> the host's Candidates (include/Candidate.hpp:56-80)
template <class Tr>
inline void unpack_candidates(pbd_handle *h, const std::vector<int32_t> &buf, int n, std::vector<typename Tr::Candidate> &out)
{
    const int stride = pbd_candidate_stride(h);
    for (int i = 0; i < n; ++i) {
        const int32_t *r = &buf[(size_t)i * stride];
        pbd_candidate_hdr hd;
        for (int w = 0; w < 8; ++w) reinterpret_cast<int32_t *>(&hd)[w] = r[w];
        Tr::candidate(out, hd, r + 8);
    }
}

// DynamicProgram<T>::argmin (include/DynamicProgram.hpp:75, src/DynamicProgram.cpp:190-255) on the device-resident result
template <class Tr>
inline void dp_argmin(pbd_handle *h, const std::vector<float> &scales, std::vector<typename Tr::Candidate> &candidates,
                      int capacity)
{
    std::vector<int32_t> buf((size_t)capacity * pbd_candidate_stride(h) + 1);
    int n = 0;
    check<Tr>(h, pbd_dp_argmin(h, scales.empty() ? NULL : &scales[0], &buf[0], capacity, &n));
    unpack_candidates<Tr>(h, buf, n, candidates);
}

// PartsBasedDetector<T>::detect (include/PartsBasedDetector.hpp:172-173, src/PartsBasedDetector.cpp:69-95): the whole path
// on the GPU, only Candidates come back.  Any accepted image depth (pbd_detect_typed).
template <class Tr>
inline void detect(pbd_handle *h, const typename Tr::Image &im, std::vector<typename Tr::Candidate> &candidates,
                   int capacity)
{
    std::vector<int32_t> buf((size_t)capacity * pbd_candidate_stride(h) + 1);
    int n = 0;
    check<Tr>(h, pbd_detect_typed(h, Tr::img_data(im), Tr::img_rows(im), Tr::img_cols(im), Tr::img_channels(im),
                                  Tr::img_step(im), Tr::img_depth(im), &buf[0], capacity, &n));
    unpack_candidates<Tr>(h, buf, n, candidates);
}

// SearchSpacePruning<T>::filterCandidatesByDepth (src/SearchSpacePruning.cpp:73-95) on the device (pbd_depth_consistency) over
// n records of this handle in `buf`, in place: n becomes the kept count, the kept records stay in order.  `depth` is one channel
// of any accepted depth; every record is taken as one of this frame (frame field 0).
template <class Tr>
inline void depth_consistency(pbd_handle *h, const typename Tr::Image &depth, float zfactor, std::vector<int32_t> &buf, int &n)
{
    if (Tr::img_channels(depth) != 1) Tr::fail(PBD_ERR_INVALID, "pbd: depth_consistency: the depth image has one channel");
    pbd_frame fr;
    fr.data = Tr::img_data(depth); fr.rows = Tr::img_rows(depth); fr.cols = Tr::img_cols(depth); fr.stride_bytes = Tr::img_step(depth);
    int kept = 0;
    check<Tr>(h, pbd_depth_consistency(h, 1, &fr, Tr::img_depth(depth), zfactor, n ? &buf[0] : NULL, n, 0, n ? &buf[0] : NULL, n, &kept));
    n = kept;
}

// pbd_set_depth_prune: the intent of the reference's commented-out ssp_.filterResponseByDepth (src/PartsBasedDetector.cpp:86-93,
// src/SearchSpacePruning.cpp:47-70) before every later walk of this handle that has a depth image bound (bind_depth): only the
// roots whose box width agrees with the depth under it are returned.  fx: focal length in pixels, width: the root footprint's
// physical width in the depth image's units, tol: relative tolerance; on = false: off
template <class Tr>
inline void set_depth_prune(pbd_handle *h, bool on, float fx, float width, float tol)
{
    pbd_depth_prune_cfg cfg;
    cfg.fx = fx; cfg.width = width; cfg.tol = tol;
    check<Tr>(h, pbd_set_depth_prune(h, on ? &cfg : NULL));
}

inline pbd_frame depth_frame(const void *data, int rows, int cols, size_t step)
{
    pbd_frame fr;
    fr.data = data; fr.rows = rows; fr.cols = cols; fr.stride_bytes = step;
    return fr;
}

// pbd_bind_depth: `depth` (one channel of any accepted depth, the frame's rows x cols) for the NEXT detect call of this handle,
// copied now
template <class Tr>
inline void bind_depth(pbd_handle *h, const typename Tr::Image &depth)
{
    if (Tr::img_channels(depth) != 1) Tr::fail(PBD_ERR_INVALID, "pbd: bind_depth: the depth image has one channel");
    const pbd_frame fr = depth_frame(Tr::img_data(depth), Tr::img_rows(depth), Tr::img_cols(depth), Tr::img_step(depth));
    check<Tr>(h, pbd_bind_depth(h, 1, &fr, Tr::img_depth(depth)));
}

// pbd_depth_prune over n records of this handle in `buf`, in place: n becomes the kept count, the kept records stay in order;
// every record is taken as one of this frame (frame field 0)
template <class Tr>
inline void depth_prune(pbd_handle *h, const typename Tr::Image &depth, float fx, float width, float tol, std::vector<int32_t> &buf,
                        int &n)
{
    if (Tr::img_channels(depth) != 1) Tr::fail(PBD_ERR_INVALID, "pbd: depth_prune: the depth image has one channel");
    const pbd_frame fr = depth_frame(Tr::img_data(depth), Tr::img_rows(depth), Tr::img_cols(depth), Tr::img_step(depth));
    pbd_depth_prune_cfg cfg;
    cfg.fx = fx; cfg.width = width; cfg.tol = tol;
    int kept = 0;
    check<Tr>(h, pbd_depth_prune(h, &cfg, 1, &fr, Tr::img_depth(depth), n ? &buf[0] : NULL, n, 0, n ? &buf[0] : NULL, n, &kept));
    n = kept;
}

// Candidate::sort + Candidate::nonMaximaSuppression(im, candidates, overlap) of n records of one rows x cols frame in `buf`, on the
// device (pbd_suppress, the pbd_set_nms stage), in place: n becomes the kept count
template <class Tr>
inline void suppress(pbd_handle *h, int rows, int cols, float overlap, std::vector<int32_t> &buf, int &n)
{
    int kept = 0;
    check<Tr>(h, pbd_suppress(h, 1, &rows, &cols, overlap, n ? &buf[0] : NULL, n, 0, n ? &buf[0] : NULL, n, &kept));
    n = kept;
}

// detect(im, depth) with the depth filter on: the unsuppressed list (the handle's pbd_set_nms must be off), the filter, then --
// overlap >= 0 -- the suppression, in the reference's order (src/PartsBasedDetector.cpp:91-93, then cells/detect.cpp:237-238)
template <class Tr>
inline void detect_depth(pbd_handle *h, const typename Tr::Image &im, const typename Tr::Image &depth, float zfactor, float overlap,
                         std::vector<typename Tr::Candidate> &candidates, int capacity)
{
    std::vector<int32_t> buf((size_t)capacity * pbd_candidate_stride(h) + 1);
    int n = 0;
    check<Tr>(h, pbd_detect_typed(h, Tr::img_data(im), Tr::img_rows(im), Tr::img_cols(im), Tr::img_channels(im),
                                  Tr::img_step(im), Tr::img_depth(im), &buf[0], capacity, &n));
    depth_consistency<Tr>(h, depth, zfactor, buf, n);
    if (overlap >= 0) suppress<Tr>(h, Tr::img_rows(im), Tr::img_cols(im), overlap, buf, n);
    unpack_candidates<Tr>(h, buf, n, candidates);
}

// Candidate::mask(im, candidates, mask) (include/Candidate.hpp:306-331) and the ROS node's `rgb & (mask != 0)` (ros/Messages.cpp:
// 157-174) on the device (pbd_candidate_mask) for n records of one frame of im's size in `buf`: the uint8 labels at `labels`
// (label_pitch bytes a row) and, when `masked` is not NULL, im masked there (im's 8-bit channels, masked_pitch bytes a row;
// masked may be im's own pixels).  Either output may be NULL.
template <class Tr>
inline void candidate_mask(pbd_handle *h, const typename Tr::Image &im, const std::vector<int32_t> &buf, int n, uint8_t *labels,
                           size_t label_pitch, uint8_t *masked, size_t masked_pitch)
{
    if (masked && Tr::img_depth(im) != 0) Tr::fail(PBD_ERR_UNSUPPORTED, "pbd: candidate_mask: the masked frame is 8-bit");
    const int rows = Tr::img_rows(im), cols = Tr::img_cols(im);
    const uint8_t *colour = static_cast<const uint8_t *>(Tr::img_data(im));
    const size_t colour_pitch = Tr::img_step(im);
    check<Tr>(h, pbd_candidate_mask(h, 1, &rows, &cols, n ? &buf[0] : NULL, n, 0, labels ? &labels : NULL, labels ? &label_pitch : NULL,
                                    Tr::img_channels(im), masked ? &colour : NULL, masked ? &colour_pitch : NULL,
                                    masked ? &masked : NULL, masked ? &masked_pitch : NULL));
}

// PartsBasedDetectorNode::messagePoses (ros/Messages.cpp:187-234) on the device (pbd_part_poses) for n records' part centres as
// pbd_boxes3d_camera writes them (record i, part j at centres[3 * (i * max_parts + j)]): count[n], position[3n],
// orientation[4n] (x, y, z, w), eigenvalues[3n] (ascending); count 0 is the node's "Centroid not found"
template <class Tr>
inline void part_poses(pbd_handle *h, int n, const std::vector<float> &centres, const std::vector<int32_t> &ncentres,
                       const std::vector<int32_t> &dense, std::vector<int32_t> &count, std::vector<float> &position,
                       std::vector<float> &orientation, std::vector<float> &eigenvalues)
{
    const size_t mp = (size_t)(pbd_candidate_stride(h) - 8) / 4, un = n > 0 ? (size_t)n : 0;
    if (n < 0 || centres.size() < un * mp * 3 || ncentres.size() < un || dense.size() < un)
        Tr::fail(PBD_ERR_INVALID, "pbd: part_poses: n records need 3 * max_parts centres and one ncentres / dense each");
    count.assign(un + 1, 0);
    position.assign(3 * un + 1, 0.f);
    orientation.assign(4 * un + 1, 0.f);
    eigenvalues.assign(3 * un + 1, 0.f);
    check<Tr>(h, pbd_part_poses(h, n, un ? &centres[0] : NULL, un ? &ncentres[0] : NULL, un ? &dense[0] : NULL, &count[0], &position[0],
                                &orientation[0], &eigenvalues[0]));
    count.resize(un);
    position.resize(3 * un);
    orientation.resize(4 * un);
    eigenvalues.resize(3 * un);
}

// One part of a record's part scores (pbd_part_scores / pbd_score_placements, include/pbd.h): its cell and mixture in the
// level's map and the four values, held as double (exact for both real types)
struct PartScore {
    int x, y, m;
    double appearance, message, bias, total;
    PartScore() : x(0), y(0), m(0), appearance(0), message(0), bias(0), total(0) {}
};

// The part scores of n records of the last detect call in `rec`.  place NULL: pbd_part_scores, at the walk's placements;
// else pbd_score_placements at (*place)[j].x / y / m, the records' parts one after another in record order, nparts[i] entries
// for record i.  status[i] = the record's parts or -1; `out` receives the parts of every record with a status above 0, in
// record order.
template <class Tr>
inline void part_scores(pbd_handle *h, const std::vector<int32_t> &rec, int n, const std::vector<int> &nparts,
                        const std::vector<PartScore> *place, std::vector<int32_t> &status, std::vector<PartScore> &out)
{
    typedef typename Tr::Real Real;
    const size_t mp = (size_t)(pbd_candidate_stride(h) - 8) / 4, un = n > 0 ? (size_t)n : 0;
    std::vector<int32_t> pl(un * mp * 3 + 1, 0);
    std::vector<Real> sc(un * mp * 4 + 1, Real(0));
    status.assign(un + 1, 0);
    if (place) {
        size_t j = 0;
        for (size_t i = 0; i < un; ++i) {
            const size_t np = i < nparts.size() && nparts[i] > 0 ? (size_t)nparts[i] : 0;
            if (np > mp || j + np > place->size()) Tr::fail(PBD_ERR_INVALID, "pbd: part_scores: one placement per part of every record");
            for (size_t p = 0; p < np; ++p, ++j) {
                int32_t *q = &pl[(i * mp + p) * 3];
                q[0] = (*place)[j].x; q[1] = (*place)[j].y; q[2] = (*place)[j].m;
            }
        }
        check<Tr>(h, pbd_score_placements(h, un ? &rec[0] : NULL, n, 0, &pl[0], &status[0], &sc[0]));
    } else {
        check<Tr>(h, pbd_part_scores(h, un ? &rec[0] : NULL, n, 0, &status[0], &pl[0], &sc[0]));
    }
    status.resize(un);
    out.clear();
    for (size_t i = 0; i < un; ++i)
        for (size_t p = 0; status[i] > 0 && p < (size_t)status[i] && p < mp; ++p) {
            PartScore s;
            const int32_t *q = &pl[(i * mp + p) * 3];
            const Real *v = &sc[(i * mp + p) * 4];
            s.x = q[0]; s.y = q[1]; s.m = q[2];
            s.appearance = (double)v[0]; s.message = (double)v[1]; s.bias = (double)v[2]; s.total = (double)v[3];
            out.push_back(s);
        }
}

// One level of the max-marginals (pbd_max_marginals / pbd_get_marginals, include/pbd.h): `planes` planes of rows x cols, plane
// gm = the (part, type) pair's global index, values[gm * rows * cols + y * cols + x] held as double (exact for both real types)
struct MarginalLevel {
    int rows, cols, planes;
    std::vector<double> values;
    MarginalLevel() : rows(0), cols(0), planes(0) {}
};

// The max-marginals of frame `frame` of the last detect call on an im_rows x im_cols image (the levels are those of
// pbd_pyramid_plan for that size); planes = the (part, type) pairs of the handle's model.  They stay on the device for
// marginal_poses until the next detect call.
template <class Tr>
inline void max_marginals(pbd_handle *h, int frame, int im_rows, int im_cols, int planes, std::vector<MarginalLevel> &levels)
{
    typedef typename Tr::Real Real;
    check<Tr>(h, pbd_max_marginals(h, frame));
    int n = 0, ir[PBD_MAX_LEVELS], ic[PBD_MAX_LEVELS], fr[PBD_MAX_LEVELS], fc[PBD_MAX_LEVELS];
    float sc[PBD_MAX_LEVELS];
    check<Tr>(h, pbd_pyramid_plan(h, im_rows, im_cols, &n, ir, ic, fr, fc, sc));
    levels.assign(n > 0 ? (size_t)n : 0, MarginalLevel());
    std::vector<Real> buf;
    for (int l = 0; l < n; ++l) {
        MarginalLevel &L = levels[l];
        L.rows = fr[l]; L.cols = fc[l]; L.planes = planes;
        const size_t cnt = (size_t)planes * (size_t)fr[l] * (size_t)fc[l];
        buf.assign(cnt + 1, Real(0));
        check<Tr>(h, pbd_get_marginals(h, l, PBD_MM_VALUES, &buf[0], cnt * sizeof(Real)));
        L.values.assign(buf.begin(), buf.begin() + cnt);
    }
}

// The poses of n seeds {level, component, part, type or -1, x, y} (6 ints each) decoded from the max-marginals held
// (pbd_marginal_poses), at the detect call's own scales: status[i] = the pose's parts or -1 for a bad seed; `candidates` receives
// the poses of the good seeds in seed order, each with the seed's max-marginal as its score
template <class Tr>
inline void marginal_poses(pbd_handle *h, const std::vector<int32_t> &seeds, std::vector<int32_t> &status,
                           std::vector<typename Tr::Candidate> &candidates)
{
    const size_t n = seeds.size() / 6, stride = (size_t)pbd_candidate_stride(h);
    std::vector<int32_t> rec(n * stride + 1, 0);
    status.assign(n + 1, 0);
    check<Tr>(h, pbd_marginal_poses(h, (int)n, n ? &seeds[0] : NULL, NULL, 0, &rec[0], NULL, &status[0]));
    status.resize(n);
    std::vector<int32_t> one(stride + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        if (status[i] <= 0) continue;
        std::copy(rec.begin() + i * stride, rec.begin() + (i + 1) * stride, one.begin());
        one[7] = 0;
        unpack_candidates<Tr>(h, one, 1, candidates);
    }
}

// Frames of any sizes in one call (new surface: pbd_detect_frames; the reference has no batch API): candidates[i] receives
// what detect(images[i]) gives.  The images share one depth and one channel count; any accepted depth.
template <class Tr>
inline void detect_batch(pbd_handle *h, const std::vector<typename Tr::Image> &images,
                         std::vector<std::vector<typename Tr::Candidate> > &candidates, int capacity)
{
    const size_t nf = images.size();
    candidates.assign(nf, std::vector<typename Tr::Candidate>());
    if (nf == 0) return;
    std::vector<pbd_frame> frames(nf);
    for (size_t i = 0; i < nf; ++i) {
        const typename Tr::Image &im = images[i];
        if (Tr::img_channels(im) != Tr::img_channels(images[0]) || Tr::img_depth(im) != Tr::img_depth(images[0]))
            Tr::fail(PBD_ERR_INVALID, "pbd: detect_batch: every image of one call has the first image's depth and channel count");
        frames[i].data = Tr::img_data(im);
        frames[i].rows = Tr::img_rows(im);
        frames[i].cols = Tr::img_cols(im);
        frames[i].stride_bytes = Tr::img_step(im);
    }
    std::vector<int32_t> buf((size_t)capacity * pbd_candidate_stride(h) + 1);
    int n = 0;
    check<Tr>(h, pbd_detect_frames(h, (int)nf, &frames[0], Tr::img_channels(images[0]), Tr::img_depth(images[0]), &buf[0], capacity,
                                   &n));
    const int stride = pbd_candidate_stride(h);
    for (int i = 0; i < n; ++i) {
        const int32_t *r = &buf[(size_t)i * stride];
        pbd_candidate_hdr hd;
        for (int w = 0; w < 8; ++w) reinterpret_cast<int32_t *>(&hd)[w] = r[w];
        Tr::candidate(candidates[hd.frame], hd, r + 8);
    }
}

// the training QP (pbd_qp_*): a failed call throws through Tr::fail with pbd_qp_last_error's text
template <class Tr>
inline void qp_check(pbd_qp *q, int rc)
{
    if (rc != PBD_OK) Tr::fail(rc, std::string("pbd: ") + pbd_qp_last_error(q));
}

template <class Tr>
inline pbd_qp *qp_create(pbd_handle *h, int capacity, double C, double wpos)
{
    pbd_qp_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.capacity = capacity; cfg.C = C; cfg.wpos = wpos;
    pbd_qp *q = NULL;
    qp_check<Tr>(NULL, pbd_qp_create(h, &cfg, &q));
    return q;
}

// qp_write of host examples (pbd_examples' hdr / values of handle h); ids: 5 int32 per example
template <class Tr, typename T>
inline int qp_add(pbd_qp *q, pbd_handle *h, const std::vector<int32_t> &hdr, const std::vector<T> &values,
                  const std::vector<int32_t> &ids)
{
    int hw = 0, vw = 0;
    check<Tr>(h, pbd_example_stride(h, &hw, &vw));
    const size_t n = ids.size() / 5;
    if (hdr.size() != n * (size_t)hw || values.size() != n * (size_t)vw)
        Tr::fail(PBD_ERR_INVALID, "pbd: QP add: one header, one values row and five id words per example");
    int taken = 0;
    qp_check<Tr>(q, pbd_qp_add(q, h, (int)n, n ? &hdr[0] : NULL, n ? (const void *)&values[0] : NULL, n ? &ids[0] : NULL, &taken));
    return taken;
}

template <class Tr>
inline pbd_qp_info qp_opt(pbd_qp *q, double tol, int iter, uint64_t seed)
{
    pbd_qp_info st;
    memset(&st, 0, sizeof st);
    qp_check<Tr>(q, pbd_qp_opt(q, tol, iter, seed, &st));
    return st;
}

template <class Tr>
inline pbd_qp_info qp_one(pbd_qp *q, const std::vector<int32_t> &order, uint64_t seed)
{
    pbd_qp_info st;
    memset(&st, 0, sizeof st);
    qp_check<Tr>(q, pbd_qp_one(q, order.empty() ? NULL : &order[0], (int)order.size(), seed, &st));
    return st;
}

template <class Tr>
inline pbd_qp_info qp_state(pbd_qp *q)
{
    pbd_qp_info st;
    memset(&st, 0, sizeof st);
    qp_check<Tr>(q, pbd_qp_state(q, &st, NULL, NULL, NULL));
    return st;
}

template <class Tr>
inline std::vector<double> qp_weights(pbd_qp *q)
{
    const pbd_qp_info st = qp_state<Tr>(q);
    std::vector<double> w((size_t)st.len + 1);
    qp_check<Tr>(q, pbd_qp_weights(q, &w[0]));
    w.resize(w.size() - 1);
    return w;
}

// the in-place model update (pbd_set_model_vector, pbd_set_thresh, pbd_qp_apply)
template <class Tr, typename T>
inline void set_model_vector(pbd_handle *h, const std::vector<T> &w)
{
    if (w.size() != (size_t)pbd_model_vector_len(h)) Tr::fail(PBD_ERR_INVALID, "pbd: a model vector of pbd_model_vector_len values");
    check<Tr>(h, pbd_set_model_vector(h, w.empty() ? NULL : (const void *)&w[0]));
}

template <class Tr>
inline void set_thresh(pbd_handle *h, float thresh)
{
    check<Tr>(h, pbd_set_thresh(h, thresh));
}

template <class Tr>
inline void qp_apply(pbd_qp *q, pbd_handle *h)
{
    qp_check<Tr>(q, pbd_qp_apply(q, h));
}

template <class Tr>
inline std::vector<double> qp_scores(pbd_qp *q)
{
    const pbd_qp_info st = qp_state<Tr>(q);
    std::vector<double> s((size_t)st.capacity + 1);
    int n = 0;
    qp_check<Tr>(q, pbd_qp_scores(q, &s[0], &n));
    s.resize((size_t)n);
    return s;
}

}  // namespace pbdbind
#endif  // PBD_BIND_HPP_
