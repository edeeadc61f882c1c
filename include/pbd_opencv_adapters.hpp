// pbd_opencv_adapters.hpp -- header-only adapters that drop the HIP path into the reference's C++ host.
//
// Compiled inside the reference tree (it needs OpenCV and the reference's own headers).  This header supplies ONLY the
// cv::Mat traits and the class shells; every line that crosses the C ABI lives in pbd_bind.hpp, the same templates
// include/pbd_host.hpp instantiates with plain buffers and tests/test_host_demo.py runs on the GPU (T = float and double).
// tests/test_adapters_compile.py compiles this very file (both T) against the declarations in tests/adapter_doubles/.
// See INTEGRATION.md for the two-line change in src/PartsBasedDetector.cpp:108,111 that installs these classes.
//
//   HipHOGFeatures<T>        : IFeatures            (include/IFeatures.hpp:49-73)
//   HipConvolutionEngine<T>  : IConvolutionEngine   (include/IConvolutionEngine.hpp:44-68)
//   hipDetect<T>()           : whole PartsBasedDetector<T>::detect on the GPU (src/PartsBasedDetector.cpp:69-95)
//   T = float (src/demo.cpp:85) or double (cells/detect.cpp:93, ros/Node.hpp:121)
#pragma once

#include <opencv2/core/core.hpp>

#include <cstring>
#include <string>
#include <vector>

#include "Candidate.hpp"
#include "IConvolutionEngine.hpp"
#include "IFeatures.hpp"
#include "Model.hpp"
#include "pbd.h"
#include "pbd_bind.hpp"

namespace pbd_adapters {

template <typename T>
struct CvTraits {
    typedef T Real;
    typedef cv::Mat Mat;
    typedef cv::Mat IMat;
    typedef cv::Mat FilterMat;
    typedef cv::Mat Image;
    typedef ::Candidate Candidate;
    static int type() { return cv::DataType<T>::type; }                     // CV_32F / CV_64F, as the reference's DataType<T>::type
    static void create(Mat &m, int rows, int cols) { m.create(rows, cols, type()); }   // cv::Mat::create is continuous
    static T *ptr(Mat &m) { return m.ptr<T>(0); }
    static const T *cptr(const Mat &m) { return m.ptr<T>(0); }
    static int rows(const Mat &m) { return m.rows; }
    static int cols(const Mat &m) { return m.cols; }
    static void icreate(IMat &m, int rows, int cols) { m.create(rows, cols, CV_32S); }
    static int32_t *iptr(IMat &m) { return m.ptr<int32_t>(0); }
    static Mat real_continuous(const Mat &m)
    {
        Mat r = m;
        if (r.depth() != cv::DataType<T>::depth) m.convertTo(r, type());    // src/PartsBasedDetector.cpp:114-117
        if (!r.isContinuous()) r = r.clone();
        return r;
    }
    static Mat rows_view(Mat &m, int r0, int r1) { return m.rowRange(r0, r1); }        // a view: no copy
    static const void *img_data(const Image &im) { return im.data; }
    static int img_rows(const Image &im) { return im.rows; }
    static int img_cols(const Image &im) { return im.cols; }
    static int img_channels(const Image &im) { return im.channels(); }
    static size_t img_step(const Image &im) { return im.step; }
    static int img_depth(const Image &im) { return im.depth(); }
    static void fail(int /*rc*/, const std::string &text) { CV_Error(CV_StsError, text); }   // the reference's error channel
    static void candidate(std::vector<Candidate> &out, const pbd_candidate_hdr &hd, const int32_t *r)
    {
        Candidate c;
        c.setComponent(hd.component);
        for (int p = 0; p < hd.nparts; ++p)
            c.addPart(cv::Rect(r[4 * p], r[4 * p + 1], r[4 * p + 2], r[4 * p + 3]), p == 0 ? hd.score : 0.0f);
        out.push_back(c);
    }
    static int filter_rows(const FilterMat &w) { return w.rows; }
    static void filter_values(const FilterMat &w, std::vector<double> &out)
    {
        cv::Mat d;
        w.convertTo(d, CV_64F);
        for (int r = 0; r < d.rows; ++r) out.insert(out.end(), d.ptr<double>(r), d.ptr<double>(r) + d.cols);
    }
};

// owns the pbd_handle (member of the detector: boost::scoped_ptr<pbd_adapters::Handle<T> > hip_)
template <typename T>
class Handle {
public:
    pbd_handle *h;
    explicit Handle(Model &model, int device = 0, int conv_mode = PBD_CONV_EXACT, int max_batch = 1)
        : h(pbdbind::create<CvTraits<T> >(model, device, conv_mode, max_batch, 1 << 18)) {}
    ~Handle() { pbd_destroy(h); }
private:
    Handle(const Handle &);
    Handle &operator=(const Handle &);
};

template <typename T>
class HipHOGFeatures : public IFeatures {
    pbd_handle *h_;
    size_t binsize_;
    vectorf scales_;
public:
    explicit HipHOGFeatures(pbd_handle *h) : h_(h), binsize_(pbd_binsize(h)) {}
    size_t binsize(void) const { return binsize_; }
    size_t nscales(void) const { return scales_.size(); }
    vectorf scales(void) const { return scales_; }
    void pyramid(const cv::Mat &im, vectorMat &pyrafeatures) { pbdbind::pyramid<CvTraits<T> >(h_, im, pyrafeatures, scales_); }
};

template <typename T>
class HipConvolutionEngine : public IConvolutionEngine {
    pbd_handle *h_;
    size_t nfilters_;
public:
    explicit HipConvolutionEngine(pbd_handle *h) : h_(h), nfilters_(0) {}
    void setFilters(const vectorMat &filters)
    {
        pbdbind::set_filters<CvTraits<T> >(h_, filters);
        nfilters_ = filters.size();
    }
    void pdf(const vectorMat &features, vector2DMat &responses) { pbdbind::pdf<CvTraits<T> >(h_, nfilters_, features, responses); }
};

// Whole detect() on the GPU: pyramid -> pdf -> min -> argmin, only Candidates come back.
template <typename T>
inline void hipDetect(pbd_handle *h, const cv::Mat &im, vectorCandidate &candidates)
{
    pbdbind::detect<CvTraits<T> >(h, im, candidates, 1 << 16);
}

// detect() of several images of any sizes (one depth, one channel count) in one call: candidates[i] = detect(images[i]).
// The handle takes up to its max_batch images (Handle's constructor).  PartsBasedDetector<T>::detectBatch is this call.
template <typename T>
inline void hipDetectBatch(pbd_handle *h, const vectorMat &images, std::vector<vectorCandidate> &candidates)
{
    pbdbind::detect_batch<CvTraits<T> >(h, images, candidates, 1 << 18);
}

// the records (pbd_candidate_stride words each) of candidates of one frame: component, score, parts (the layout pbd_detect returns).
// A template over the candidate type, so that only the calls below instantiate it.
template <class Cand>
inline void hipRecords(pbd_handle *h, std::vector<Cand> &candidates, std::vector<int32_t> &rec)
{
    const size_t stride = (size_t)pbd_candidate_stride(h);
    rec.assign(candidates.size() * stride + 1, 0);
    for (size_t i = 0; i < candidates.size(); ++i) {
        int32_t *r = &rec[i * stride];
        const std::vector<cv::Rect> &parts = candidates[i].parts();
        const float score = candidates[i].score();
        r[1] = candidates[i].component();
        std::memcpy(&r[5], &score, sizeof score);
        r[6] = (int32_t)parts.size();
        for (size_t k = 0; k < parts.size() && 8 + 4 * k + 3 < stride; ++k) {
            r[8 + 4 * k] = parts[k].x; r[9 + 4 * k] = parts[k].y; r[10 + 4 * k] = parts[k].width; r[11 + 4 * k] = parts[k].height;
        }
    }
}

// SearchSpacePruning<T>::filterCandidatesByDepth(parts_, candidates, depth, zfactor) on the device (pbd_depth_consistency): what
// the commented-out call of PartsBasedDetector<T>::detect would do (src/PartsBasedDetector.cpp:91-93, zfactor 0.03).  The kept
// candidates stay in order; `depth` is one channel of any accepted depth; every candidate is one of this frame.
template <typename T>
inline void hipFilterCandidatesByDepth(pbd_handle *h, std::vector<typename CvTraits<T>::Candidate> &candidates, const cv::Mat &depth,
                                       float zfactor)
{
    std::vector<int32_t> rec;
    hipRecords(h, candidates, rec);
    const std::vector<int32_t> in(rec);
    int n = (int)candidates.size();
    pbdbind::depth_consistency<CvTraits<T> >(h, depth, zfactor, rec, n);
    const size_t stride = (size_t)pbd_candidate_stride(h);
    std::vector<typename CvTraits<T>::Candidate> kept;
    for (size_t i = 0, k = 0; i < candidates.size() && k < (size_t)n; ++i)   // the kept records are the input's, in order
        if (std::memcmp(&in[i * stride], &rec[k * stride], stride * sizeof(int32_t)) == 0) {
            kept.push_back(candidates[i]);
            ++k;
        }
    candidates.swap(kept);
}

// Candidate::sort + Candidate::nonMaximaSuppression(im, candidates, overlap) on the device (pbd_suppress, the pbd_set_nms stage)
// for a list built elsewhere, e.g. after hipFilterCandidatesByDepth; every candidate is one of this frame
template <typename T>
inline void hipSuppress(pbd_handle *h, const cv::Mat &im, std::vector<typename CvTraits<T>::Candidate> &candidates, float overlap)
{
    std::vector<int32_t> rec;
    hipRecords(h, candidates, rec);
    int n = (int)candidates.size();
    pbdbind::suppress<CvTraits<T> >(h, im.rows, im.cols, overlap, rec, n);
    candidates.clear();
    pbdbind::unpack_candidates<CvTraits<T> >(h, rec, n, candidates);
}

// SearchSpacePruning<T>::filterResponseByDepth(pdfs, fsizes, depth, scales, X, fx) (include/SearchSpacePruning.hpp:56,
// src/SearchSpacePruning.cpp:47-70; the call PartsBasedDetector<T>::detect leaves commented out) for the NEXT hipDetect of this
// handle: the stub's own parameters behind the handle.  The responses, their sizes and the scales stay on the device, so pdfs,
// fsizes and scales are not read; `depth` (one channel, the image's size) is bound, and the roots whose box width disagrees with
// fx * X / width-in-pixels by more than tol are not walked (pbd_set_depth_prune + pbd_bind_depth: scores are untouched, records
// are removed).  X in the depth image's units.  hipSetDepthPrune<T>(h, false) turns the setting off again.
template <typename T>
inline void hipSetDepthPrune(pbd_handle *h, bool on, float fx = 0.f, float X = 0.f, float tol = 0.3f)
{
    pbdbind::set_depth_prune<CvTraits<T> >(h, on, fx, X, tol);
}
template <typename T, class Pdfs, class Sizes>      // vector2DMat, std::vector<cv::Size>: templates, so that neither is named here
inline void hipDepthPrune(pbd_handle *h, Pdfs &pdfs, const Sizes &fsizes, const cv::Mat &depth, const vectorf &scales, const float X,
                          const float fx, const float tol = 0.3f)
{
    (void)pdfs; (void)fsizes; (void)scales;
    pbdbind::set_depth_prune<CvTraits<T> >(h, true, fx, X, tol);
    pbdbind::bind_depth<CvTraits<T> >(h, depth);
}

// nonMaximaSuppression(src, sz, dst, mask) (include/nms.hpp, src/nms.cpp:84-129) on the device (pbd_grid_nms): the reference's
// parameters behind the handle.  src: one channel; CV_32F and CV_64F are compared in their own type, every other depth as CV_64F
// (exact for the integer depths).  dst becomes the CV_8U plane of 0 / 255; mask: empty, or CV_8U of src's size.
inline void hipGridNMS(pbd_handle *h, const cv::Mat &src, int sz, cv::Mat &dst, const cv::Mat mask = cv::Mat())
{
    const bool masked = mask.data != NULL && mask.rows > 0 && mask.cols > 0;
    if (src.channels() != 1 || (masked && (mask.rows != src.rows || mask.cols != src.cols || mask.depth() != CV_8U || mask.channels() != 1)))
        CV_Error(CV_StsError, "pbd: hipGridNMS: one channel, and a CV_8U mask of the same size");
    const cv::Mat m = masked && !mask.isContinuous() ? mask.clone() : mask;
    dst.create(src.rows, src.cols, CV_8U);
    const uint8_t *mp = masked ? m.ptr<uint8_t>(0) : NULL;
    uint8_t *dp = src.rows > 0 && src.cols > 0 ? dst.ptr<uint8_t>(0) : NULL;
    if (src.depth() == CV_32F) pbdbind::grid_nms<CvTraits<float> >(h, src, sz, mp, dp);
    else pbdbind::grid_nms<CvTraits<double> >(h, src, sz, mp, dp);
}

// PartsBasedDetector<T>::detect's commented-out ssp_.nonMaxSuppression(rootv, scales) (src/PartsBasedDetector.cpp:86) for every
// later hipDetect / hipDetectBatch of this handle (pbd_set_root_nms): sz = 0 turns it off
template <typename T>
inline void hipSetRootNMS(pbd_handle *h, int sz)
{
    pbdbind::set_root_nms<CvTraits<T> >(h, sz);
}

// The padded pyramid of the Matlab detector (featpyramid.m:36-45) for every later hipDetect / hipDetectBatch of this handle
// (pbd_set_padding): every feature level grows by padx / pady cells of the boundary occlusion feature on each side, and an object
// cut off by the frame edge is found with the parts that are not visible placed in the pad.  (0, 0) turns it off
template <typename T>
inline void hipSetPadding(pbd_handle *h, int padx, int pady)
{
    pbdbind::set_padding<CvTraits<T> >(h, padx, pady);
}

// Search an octave above the frame in every later hipDetect / hipDetectBatch of this handle (pbd_set_fine_octave): the first
// `interval` pyramid levels a second time at bin size sbin / 2, in front of the others, so that an object of half the template's
// size is found; a candidate's level then indexes the longer list.  false turns it off
template <typename T>
inline void hipSetFineOctave(pbd_handle *h, bool on)
{
    pbdbind::set_fine_octave<CvTraits<T> >(h, on);
}

// At most k candidates per frame from every later hipDetect / hipDetectBatch of this handle (pbd_set_top_k): the k best roots of
// the frame among those the threshold and the other root filters leave; k = 0 turns it off
template <typename T>
inline void hipSetTopK(pbd_handle *h, int k)
{
    pbdbind::set_top_k<CvTraits<T> >(h, k);
}

// The k best elements of src on the device (pbd_top_k_cells): a larger value is better, of equal values the one earlier in
// row-major order; NaN and masked-out elements take no part.  src: one channel; CV_32F and CV_64F are compared in their own type,
// every other depth as CV_64F (exact for the integer depths).  dst becomes the CV_8U array of 0 / 255; mask: empty, or CV_8U of
// src's size.
inline void hipTopK(pbd_handle *h, const cv::Mat &src, int k, cv::Mat &dst, const cv::Mat mask = cv::Mat())
{
    const bool masked = mask.data != NULL && mask.rows > 0 && mask.cols > 0;
    if (src.channels() != 1 || (masked && (mask.rows != src.rows || mask.cols != src.cols || mask.depth() != CV_8U || mask.channels() != 1)))
        CV_Error(CV_StsError, "pbd: hipTopK: one channel, and a CV_8U mask of the same size");
    const cv::Mat m = masked && !mask.isContinuous() ? mask.clone() : mask;
    dst.create(src.rows, src.cols, CV_8U);
    const uint8_t *mp = masked ? m.ptr<uint8_t>(0) : NULL;
    uint8_t *dp = src.rows > 0 && src.cols > 0 ? dst.ptr<uint8_t>(0) : NULL;
    if (src.depth() == CV_32F) pbdbind::top_k_cells<CvTraits<float> >(h, src, k, mp, dp);
    else pbdbind::top_k_cells<CvTraits<double> >(h, src, k, mp, dp);
}

// The k best candidates of one frame by score on the device (pbd_top_k), ties to the earlier one, in their input order: for a list
// built elsewhere
template <typename T>
inline void hipTopK(pbd_handle *h, std::vector<typename CvTraits<T>::Candidate> &candidates, int k)
{
    std::vector<int32_t> rec;
    hipRecords(h, candidates, rec);
    const std::vector<int32_t> in(rec);
    int n = (int)candidates.size();
    pbdbind::top_k<CvTraits<T> >(h, k, rec, n);
    const size_t stride = (size_t)pbd_candidate_stride(h);
    std::vector<typename CvTraits<T>::Candidate> kept;
    for (size_t i = 0, j = 0; i < candidates.size() && j < (size_t)n; ++i)   // the kept records are the input's, in order
        if (std::memcmp(&in[i * stride], &rec[j * stride], stride * sizeof(int32_t)) == 0) {
            kept.push_back(candidates[i]);
            ++j;
        }
    candidates.swap(kept);
}

// A root's duplicates on neighbouring pyramid levels and components suppressed in every later hipDetect / hipDetectBatch of this
// handle (pbd_set_scale_nms): only the roots no better root within dl levels beats whose rectangle's centre lies in its own, or the
// other way round, are walked; dl in 0..255; on = false turns it off
template <typename T>
inline void hipSetScaleNMS(pbd_handle *h, bool on, int dl)
{
    pbdbind::set_scale_nms<CvTraits<T> >(h, on, dl);
}

// The candidates of one frame no better neighbouring candidate within dl levels beats, decided on the device (pbd_scale_nms), in
// their input order: for a list built elsewhere, e.g. the merged lists of level-sharded handles
template <typename T>
inline void hipScaleNMS(pbd_handle *h, std::vector<typename CvTraits<T>::Candidate> &candidates, int dl)
{
    std::vector<int32_t> rec;
    hipRecords(h, candidates, rec);
    const std::vector<int32_t> in(rec);
    int n = (int)candidates.size();
    pbdbind::scale_nms<CvTraits<T> >(h, dl, rec, n);
    const size_t stride = (size_t)pbd_candidate_stride(h);
    std::vector<typename CvTraits<T>::Candidate> kept;
    for (size_t i = 0, j = 0; i < candidates.size() && j < (size_t)n; ++i)   // the kept records are the input's, in order
        if (std::memcmp(&in[i * stride], &rec[j * stride], stride * sizeof(int32_t)) == 0) {
            kept.push_back(candidates[i]);
            ++j;
        }
    candidates.swap(kept);
}

// Candidate::mask(im, candidates, mask) (include/Candidate.hpp:306-331) on the device (pbd_candidate_mask): mask becomes the
// im.rows x im.cols CV_8U label image; every candidate is one of this frame
template <typename T>
inline void hipCandidateMask(pbd_handle *h, const cv::Mat &im, std::vector<typename CvTraits<T>::Candidate> &candidates, cv::Mat &mask)
{
    std::vector<int32_t> rec;
    hipRecords(h, candidates, rec);
    mask.create(im.rows, im.cols, CV_8U);
    pbdbind::candidate_mask<CvTraits<T> >(h, im, rec, (int)candidates.size(), mask.ptr<uint8_t>(), mask.step, NULL, 0);
}

// messagePoses (ros/Messages.cpp:187-234) on the device (pbd_part_poses) for n candidates' part centres as pbd_boxes3d_camera
// writes them (centres[3 * (i * max_parts + j)], ncentres, dense): count, position, orientation (x, y, z, w) and eigenvalues of
// each, the node's PoseArray before its "Centroid not found" entries (count 0) are skipped
template <typename T>
inline void hipPartPoses(pbd_handle *h, int n, const std::vector<float> &centres, const std::vector<int32_t> &ncentres,
                         const std::vector<int32_t> &dense, std::vector<int32_t> &count, std::vector<float> &position,
                         std::vector<float> &orientation, std::vector<float> &eigenvalues)
{
    pbdbind::part_poses<CvTraits<T> >(h, n, centres, ncentres, dense, count, position, orientation, eigenvalues);
}

// The score of each part of candidates of the last hipDetect (pbd_part_scores; include/pbd.h "Part scores"): `scores` receives
// every candidate's parts in candidate order -- cell and mixture in the level's map; appearance (the confidence the reference's
// Candidate declares per part and never fills, include/Candidate.hpp:54-72), message, bias, total -- and status[i] candidate i's
// parts
template <typename T>
inline void hipPartScores(pbd_handle *h, std::vector<typename CvTraits<T>::Candidate> &candidates, std::vector<int32_t> &status,
                          std::vector<pbdbind::PartScore> &scores)
{
    std::vector<int32_t> rec;
    hipRecords(h, candidates, rec);
    pbdbind::part_scores<CvTraits<T> >(h, rec, (int)candidates.size(), std::vector<int>(), NULL, status, scores);
}

// The max-marginals of every part on frame `frame` of the last hipDetect of an im_rows x im_cols image (pbd_max_marginals;
// include/pbd.h "Max-marginals"): per level the planes of every (part, type) pair of the model, `planes` of them.  They stay on
// the device for hipMarginalPoses until the next detect call
template <typename T>
inline void hipMaxMarginals(pbd_handle *h, int frame, int im_rows, int im_cols, int planes, std::vector<pbdbind::MarginalLevel> &levels)
{
    pbdbind::max_marginals<CvTraits<T> >(h, frame, im_rows, im_cols, planes, levels);
}

// The poses of seeds {level, component, part, type or -1, x, y} decoded from the max-marginals held (pbd_marginal_poses):
// status[i] = the pose's parts or -1 for a bad seed; `candidates` receives the good seeds' poses in seed order
template <typename T>
inline void hipMarginalPoses(pbd_handle *h, const std::vector<int32_t> &seeds, std::vector<int32_t> &status,
                             std::vector<typename CvTraits<T>::Candidate> &candidates)
{
    pbdbind::marginal_poses<CvTraits<T> >(h, seeds, status, candidates);
}

// A training positive's augmented copy on the device (pbd_augment_frames; include/pbd.h "Augmented positives"): dst becomes
// rotate(mirror(im)), turned counter-clockwise by `degrees` (nearest neighbour, zero outside the source), of im's depth and
// channel count (CV_8U, CV_16U, CV_32F or CV_64F; 1 or 3 channels).  The keypoints follow with pbd_augment_points.
inline void hipAugmentFrames(pbd_handle *h, const cv::Mat &im, bool mirror, double degrees, cv::Mat &dst)
{
    int rows = 0, cols = 0;
    double coef[2];
    pbdbind::check<CvTraits<float> >(NULL, pbd_augment_plan(im.rows, im.cols, degrees, &rows, &cols, coef));
    dst.create(rows, cols, im.depth() + ((im.channels() - 1) << 3));   // CV_MAKETYPE(depth, channels)
    pbd_frame src, out;
    src.data = im.data; src.rows = im.rows; src.cols = im.cols; src.stride_bytes = im.step;
    out.data = dst.data; out.rows = dst.rows; out.cols = dst.cols; out.stride_bytes = dst.step;
    pbd_augment job;
    job.frame = 0; job.mirror = mirror ? 1 : 0; job.degrees = degrees;
    pbdbind::check<CvTraits<float> >(h, pbd_augment_frames(h, 1, &src, im.channels(), im.depth(), 1, &job, &out));
}

}  // namespace pbd_adapters
