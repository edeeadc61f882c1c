// demo.cpp -- command-line harness with the flow of the reference's src/demo.cpp:55-117:
//   model file -> FileStorageModel / MatlabIOModel::deserialize -> PartsBasedDetector<T>::distributeModel -> read image ->
//   detect -> "Number of candidates" -> Candidate::sort [-> nonMaximaSuppression] -> list the best ones.
// The GUI part of the reference's demo (Visualize, highgui) is out of scope.
//
//   pbd_demo model.(yml|xml|mat) image.(ppm|pgm) [--double] [--nms OVERLAP] [--device-nms OVERLAP] [--walk reference|argmax] [--root-nms SZ] [--top-k K] [--scale-nms DL] [--pad X[,Y]] [--fine-octave] [--top N] [--staged]
//            [--stream HANDLES FRAMES] [--conv-mode N] [--also IMAGE ...] [--depth DEPTH.pgm [--camera FX,FY,CX,CY]
//            [--remove-planes] [--depth-consistency ZFACTOR] [--depth-prune FX,WIDTH,TOL] [--poses]] [--mask LABELS.pgm [--masked OUT.ppm]]
//            [--part-scores] [--marginal-pose PART]
//   --device-nms: the sort + suppression run on the device (pbd_set_nms) instead of on the host; --nms keeps its host meaning
//   --walk argmax: part boxes at the placement the score was taken at (pbd_set_walk) instead of the reference's composed pointers
//   --root-nms SZ: only the roots that are grid maxima of their score plane within SZ cells are walked and listed
//           (pbd_set_root_nms: the reference's commented-out ssp_.nonMaxSuppression(rootv, scales)); not with --staged
//   --top-k K: at most K candidates per image: only the K best roots among those the threshold (and --root-nms, --depth-prune) leave
//           are walked and listed (pbd_set_top_k); not with --staged
//   --scale-nms DL: a root's duplicates within DL pyramid levels (0..255) and on other components are suppressed before the walk
//           and before --top-k (pbd_set_scale_nms); not with --staged
//   --pad X[,Y]: the padded pyramid of the Matlab detector (pbd_set_padding): every feature level grows by X (Y; Y = X when not
//           given) cells of the boundary occlusion feature on each side, so that roots and parts can lie outside the image; the
//           root cell a candidate line prints is then a cell of the padded plane.  Not with --depth-prune or --marginal-pose
//   --fine-octave: search an octave above the frame (pbd_set_fine_octave): the first `interval` levels a second time at bin size
//           sbin / 2, in front of the others (objects of half the template's size); the level a candidate line prints then
//           indexes the longer list
//   --conv-mode: the handles' convolution mode, a PBD_CONV_* value (include/pbd.h); default PBD_CONV_EXACT.  0 exact, 1 fma,
//           2 / 3 matrix cores bf16 / fp16 (5x5 banks), 4 fp64 matrix cores (--double), 5 / 6 matrix cores bf16 / fp16 for
//           every filter size and mixed banks (PBD_CONV_MFMA_ANY / PBD_CONV_MFMA_F16_ANY; not with --double)
//   --also: one more image (repeatable; same channel count as the first): the first image and every --also image are detected
//           in ONE detectBatch call, and each image's candidates are printed, in order, as a single run prints them
//   --depth: a depth map (PGM, 8- or 16-bit, or grey PFM, float; any size): after the candidate lines, one line "box3d x y z height width depth"
//           per listed candidate, Candidate::boundingBox3D(im, depth) (PartsBasedDetector::boundingBoxes3D, on the device)
//   --camera FX,FY,CX,CY: with --depth, the rest of PointCloudClusterer on the device.  The depth map's values become float
//           unscaled (as cv_bridge's TYPE_32FC1 conversion; a grey PFM map is float already), the cloud is back-projected from
//           it (NaN where the depth is 0 or not finite);
//           then per listed candidate: "box3d_cam x y z height width depth", "centres N x y z ..." (the part centres), and
//           "object SIZE x y z" (the kept cluster's size and centroid)
//   --remove-planes: with --camera, organizedMultiplaneSegmentation before the clustering (the callers' remove_planes option):
//           "plane K a b c d INLIERS" per plane, "kept N" (the reduced cloud's points), then the lines above on the reduced cloud
//   --depth-consistency ZFACTOR: with --depth, one line "depth_consistency zfactor Z: kept K dropped D" (filterCandidatesByDepth
//           on the unsuppressed list, on the device), then the candidates of detect(im, depth) with setDepthConsistency on
//   --mask: Candidate::mask of the listed candidates (after --top), on the device, written as a binary PGM; one line "mask K"
//           (the labelled pixels); --masked: the image & (mask != 0) (the ROS node's mask topic), a binary PPM (PGM for grey)
//   --depth-prune FX,WIDTH,TOL: with --depth (a map of the image's size), only the roots whose box width agrees with the depth under
//           it are walked and listed (pbd_set_depth_prune + pbd_bind_depth: FX in pixels, WIDTH of the root footprint in the map's
//           units, relative tolerance TOL); with --depth-consistency the chain is prune -> filter -> suppression; with --stream
//           every submitted frame carries the map; not with --staged
//   --poses: with --camera, one line per listed candidate after its "object" line: "pose COUNT x y z qx qy qz qw" (messagePoses
//           on the part centres, on the device; COUNT 0 is the node's "Centroid not found")
//   --part-scores: after the candidate lines, one line per listed candidate and part, "part_score CANDIDATE PART x y m appearance
//           message bias total" (pbd_part_scores, DESIGN.md section 6s: the part's cell and mixture in its level's map and the
//           four values, floats as %a so that every bit shows); not with --staged, --stream or --also
//   --marginal-pose PART: after the candidate lines, the pose decoded from the best cell of part PART (of component 0) over all
//           levels of its max-marginals (pbd_max_marginals / pbd_marginal_poses): one line "marginal_pose
//           PART LEVEL X Y SCORE" (the part's level and cell, the score as %a) and the pose as a candidate line; not with --staged,
//           --stream or --also
//   --augment DEG[,mirror] OUT.ppm: no detection; the image's augmented copy rotate(mirror(image)) -- turned counter-clockwise by
//           DEG degrees, nearest neighbour, zero outside (pbd_augment_frames) -- written as a binary PPM
//           (PGM for grey) and one line "augment ROWS COLS"
//   pbd_demo model.(yml|xml|mat) --dump-model  (no GPU needed: prints what the model reader read)
// The model reader follows the extension, as the reference's demo chooses it (src/demo.cpp:63-77): .mat -> MatlabIOModel
// (include/pbd_matlabio.hpp), any other -> FileStorageModel.
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "pbd_host.hpp"
#include "pbd_matlabio.hpp"

using namespace pbdhost;

// what a run prints for one image's candidates (the reference's demo: count, sort, optional NMS, the best ones)
static int g_walk = PBD_WALK_REFERENCE;   // --walk
static int g_root_nms = 0;                // --root-nms
static int g_top_k = 0;                   // --top-k
static int g_scale_nms = -1;              // --scale-nms: the level distance, -1 off
static int g_padx = 0, g_pady = 0;        // --pad
static bool g_fine = false;               // --fine-octave
static bool g_part_scores = false;        // --part-scores
static int g_marginal_part = -1;          // --marginal-pose
static bool g_prune = false;              // --depth-prune fx,width,tol
static float g_prune_fx = 0.f, g_prune_width = 0.f, g_prune_tol = 0.f;

static void report(std::vector<Candidate> &candidates, const Image &im, bool staged, float nms, float dnms, int top)
{
    std::printf("Number of candidates: %zu\n", candidates.size());
    if (dnms >= 0 && !staged) std::printf("After device NMS: %zu\n", candidates.size());   // already sorted (stably) and suppressed
    else Candidate::sort(candidates);
    if (nms >= 0) {
        Candidate::nonMaximaSuppression(im.rows, im.cols, candidates, nms);
        std::printf("After NMS: %zu\n", candidates.size());
    }
    for (size_t i = 0; i < candidates.size() && (int)i < top; ++i) {
        const Candidate &c = candidates[i];
        std::printf("cand %d %d %d %d %.9g", c.level, c.component(), c.root_y, c.root_x, (double)c.score());
        for (size_t p = 0; p < c.parts().size(); ++p)
            std::printf(" %d,%d,%d,%d", c.parts()[p].x, c.parts()[p].y, c.parts()[p].width, c.parts()[p].height);
        std::printf("\n");
    }
}

// the first image and the --also images through one detectBatch call; one report per image, in order
template <typename T>
static int run_batch(Model &model, const std::vector<Image> &ims, float nms, float dnms, int top, int conv_mode)
{
    PartsBasedDetector<T> pbd(0, conv_mode, (int)ims.size());
    if (dnms >= 0) pbd.setNonMaximaSuppression(dnms);
    pbd.setWalk(g_walk);
    pbd.setRootNMS(g_root_nms);
    pbd.setTopK(g_top_k);
    pbd.setScaleNMS(g_scale_nms >= 0, g_scale_nms >= 0 ? g_scale_nms : 0);
    pbd.setPadding(g_padx, g_pady);
    pbd.setFineOctave(g_fine);
    pbd.distributeModel(model);
    std::vector<std::vector<Candidate> > candidates;
    pbd.detectBatch(ims, candidates);
    for (size_t i = 0; i < ims.size(); ++i) report(candidates[i], ims[i], false, nms, dnms, top);
    return 0;
}

// the depth map as float, unscaled; the organized cloud back-projected from it (x = ray(c, r) * d, rounded to float; NaN where
// d is 0 or not finite); camera boxes, part centres and one kept cluster per listed candidate
template <typename T>
static void camera_lines(PartsBasedDetector<T> &pbd, const Image &im, const Image &depth, const pbd_pinhole &cam,
                         const std::vector<Candidate> &listed, bool remove_planes, bool poses)
{
    std::vector<float> df((size_t)depth.rows * depth.cols), cloud(df.size() * 3);
    for (int r = 0; r < depth.rows; ++r)
        for (int c = 0; c < depth.cols; ++c) {
            const uint8_t *row = static_cast<const uint8_t *>(depth.data) + r * depth.step;
            const float d = depth.depth == 5 ? reinterpret_cast<const float *>(row)[c]
                            : depth.depth == 2 ? (float)reinterpret_cast<const uint16_t *>(row)[c] : (float)row[c];
            df[(size_t)r * depth.cols + c] = d;
            float *p = &cloud[((size_t)r * depth.cols + c) * 3];
            if (d == 0 || !std::isfinite(d)) {
                p[0] = p[1] = p[2] = std::numeric_limits<float>::quiet_NaN();
                continue;
            }
            const double rx = (((double)c - cam.cx) - cam.tx) / cam.fx, ry = (((double)r - cam.cy) - cam.ty) / cam.fy;
            p[0] = (float)(rx * (double)d); p[1] = (float)(ry * (double)d); p[2] = d;
        }
    Image dimg;
    dimg.data = df.data(); dimg.rows = depth.rows; dimg.cols = depth.cols; dimg.channels = 1;
    dimg.step = (size_t)depth.cols * sizeof(float); dimg.depth = 5;
    std::vector<Rect3d> boxes;
    std::vector<std::vector<Point3f> > centres;
    std::vector<bool> dense;
    pbd.computeBoundingBoxes(im, dimg, cam, listed, boxes, centres, &dense);
    std::vector<int32_t> pcount;
    std::vector<float> ppos, pquat, pev;
    if (poses) pbd.partPoses(centres, dense, pcount, ppos, pquat, pev);
    pbd_cloud pc;
    pc.data = cloud.data(); pc.rows = depth.rows; pc.cols = depth.cols; pc.point_stride = 12; pc.row_stride = (size_t)depth.cols * 12;
    std::vector<std::vector<int> > clusters;
    std::vector<Point3f> objects;
    std::vector<float> reduced;
    if (remove_planes) {                 // organizedMultiplaneSegmentation first, as the callers with remove_planes set
        std::vector<int> kept, labels, inliers;
        std::vector<std::array<float, 4> > planes;
        pbd.organizedMultiplaneSegmentation(pc, reduced, kept, labels, planes, inliers);
        for (size_t k = 0; k < planes.size(); ++k)
            std::printf("plane %zu %.9g %.9g %.9g %.9g %d\n", k, planes[k][0], planes[k][1], planes[k][2], planes[k][3], inliers[k]);
        std::printf("kept %zu\n", kept.size());
        pc = PartsBasedDetector<T>::reducedCloud(reduced);
    }
    pbd.clusterObjects(pc, boxes, clusters, objects);
    for (size_t i = 0; i < boxes.size(); ++i) {
        std::printf("box3d_cam %.17g %.17g %.17g %.17g %.17g %.17g\n", boxes[i].x, boxes[i].y, boxes[i].z, boxes[i].height, boxes[i].width,
                    boxes[i].depth);
        std::printf("centres %zu", centres[i].size());
        for (size_t j = 0; j < centres[i].size(); ++j) std::printf(" %.9g %.9g %.9g", centres[i][j].x, centres[i][j].y, centres[i][j].z);
        std::printf("\nobject %zu %.9g %.9g %.9g\n", clusters[i].size(), objects[i].x, objects[i].y, objects[i].z);
        if (poses)
            std::printf("pose %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", pcount[i], ppos[3 * i], ppos[3 * i + 1], ppos[3 * i + 2], pquat[4 * i],
                        pquat[4 * i + 1], pquat[4 * i + 2], pquat[4 * i + 3]);
    }
}

// a binary PGM (channels 1) or PPM (channels 3: BGR pixels, written as the RGB a PPM stores) of rows x cols interleaved bytes
static bool writePNM(const char *path, const uint8_t *data, int rows, int cols, int channels)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    std::fprintf(f, "P%d\n%d %d\n255\n", channels == 3 ? 6 : 5, cols, rows);
    std::vector<uint8_t> out(data, data + (size_t)rows * cols * channels);
    if (channels == 3)
        for (size_t i = 0; i < out.size(); i += 3) std::swap(out[i], out[i + 2]);
    const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    return std::fclose(f) == 0 && ok;
}

template <typename T>
static int run(Model &model, const Image &im, bool staged, float nms, float dnms, int top, int stream_k, int stream_n,
               int conv_mode, const Image *depth, const pbd_pinhole *camera, bool remove_planes, float dcz, const char *mask_path,
               const char *masked_path, bool poses)
{
    PartsBasedDetector<T> pbd(0, conv_mode);
    if (dnms >= 0) pbd.setNonMaximaSuppression(dnms);
    pbd.setWalk(g_walk);
    pbd.setRootNMS(g_root_nms);
    pbd.setTopK(g_top_k);
    pbd.setScaleNMS(g_scale_nms >= 0, g_scale_nms >= 0 ? g_scale_nms : 0);
    pbd.setPadding(g_padx, g_pady);
    pbd.setFineOctave(g_fine);
    if (g_prune) pbd.setDepthPrune(true, g_prune_fx, g_prune_width, g_prune_tol);
    std::vector<Candidate> candidates;
    if (stream_k > 0) {
        // the image stream_n times through a FrameStream of stream_k handles: every result must be the first one's
        FrameStream<T> fs(model, stream_k, 0, 1 << 16, conv_mode);
        if (dnms >= 0) fs.setNonMaximaSuppression(dnms);
        fs.setRootNMS(g_root_nms);
        fs.setTopK(g_top_k);
        fs.setScaleNMS(g_scale_nms >= 0, g_scale_nms >= 0 ? g_scale_nms : 0);
        fs.setPadding(g_padx, g_pady);
        fs.setFineOctave(g_fine);
        if (g_prune) fs.setDepthPrune(true, g_prune_fx, g_prune_width, g_prune_tol);
        std::vector<Candidate> first, cur;
        size_t got = 0;
        bool same = true;
        auto cmp = [&](const std::vector<Candidate> &a, const std::vector<Candidate> &b) {
            if (a.size() != b.size()) return false;
            for (size_t i = 0; i < a.size(); ++i) {
                if (a[i].level != b[i].level || a[i].root_x != b[i].root_x || a[i].root_y != b[i].root_y || a[i].score() != b[i].score() ||
                    a[i].parts().size() != b[i].parts().size()) return false;
                for (size_t p = 0; p < a[i].parts().size(); ++p)
                    if (a[i].parts()[p].x != b[i].parts()[p].x || a[i].parts()[p].y != b[i].parts()[p].y ||
                        a[i].parts()[p].width != b[i].parts()[p].width || a[i].parts()[p].height != b[i].parts()[p].height) return false;
            }
            return true;
        };
        auto collect = [&]() {
            fs.next(cur);
            if (got++ == 0) first = cur; else same = same && cmp(first, cur);
        };
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < stream_n; ++i) {
            while (fs.full()) collect();
            if (g_prune && depth) fs.submit(im, *depth); else fs.submit(im);
        }
        while (fs.pending()) collect();
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("stream: %d frames over %d handles, %.1f frames/s, results %s\n", stream_n, stream_k, stream_n / sec, same ? "identical" : "DIFFER");
        if (!same) return -3;
        candidates = first;
    } else if (staged) {
        pbd.distributeModel(model);
        // the four calls of PartsBasedDetector<T>::detect (src/PartsBasedDetector.cpp:73-89) through the engine mirrors
        HOGFeatures<T> features(pbd.handle());
        SpatialConvolutionEngine<T> conv(pbd.handle(), model.filtersw_.size());
        DynamicProgram<T> dp(pbd.handle(), (int)model.filtersw_.size());
        std::vector<MatT<T> > pyramid;
        features.pyramid(im, pyramid);
        std::vector<std::vector<MatT<T> > > pdf, rootv;
        std::vector<std::vector<MatT<int32_t> > > rooti;
        conv.pdf(pyramid, pdf);
        dp.min(pdf, rootv, rooti, model.ncomponents());
        dp.argmin(features.scales(), candidates);
    } else if (depth && dcz >= 0) {
        // filterCandidatesByDepth on the unsuppressed list (its counts), then the chain detect(im, depth) runs with the setting on
        PartsBasedDetector<T> raw(0, conv_mode);
        raw.setPadding(g_padx, g_pady);
        raw.setFineOctave(g_fine);
        raw.distributeModel(model);
        std::vector<Candidate> all, kept;
        raw.detect(im, all);
        kept = all;
        raw.filterCandidatesByDepth(*depth, kept, dcz);
        std::printf("depth_consistency zfactor %g: kept %zu dropped %zu\n", dcz, kept.size(), all.size() - kept.size());
        pbd.distributeModel(model);
        pbd.setDepthConsistency(true, dcz);
        pbd.detect(im, *depth, candidates);
    } else {
        pbd.distributeModel(model);
        if (g_prune && depth) pbd.detect(im, *depth, candidates);   // binds the map for this call
        else pbd.detect(im, candidates);
    }
    report(candidates, im, staged, nms, dnms, top);
    if (depth) {
        if (!pbd.handle()) pbd.distributeModel(model);
        const std::vector<Candidate> listed(candidates.begin(), candidates.begin() + std::min<size_t>(candidates.size(), (size_t)top));
        std::vector<Rect3d> boxes;
        pbd.boundingBoxes3D(im, *depth, listed, boxes);
        for (size_t i = 0; i < boxes.size(); ++i)
            std::printf("box3d %.17g %.17g %.17g %.17g %.17g %.17g\n", boxes[i].x, boxes[i].y, boxes[i].z, boxes[i].height, boxes[i].width,
                        boxes[i].depth);
        if (camera) camera_lines(pbd, im, *depth, *camera, listed, remove_planes, poses);
    }
    if (g_part_scores) {                 // the listed candidates' part scores; floats as %a: every bit
        std::vector<Candidate> listed(candidates.begin(), candidates.begin() + std::min<size_t>(candidates.size(), (size_t)top));
        std::vector<PartScore> scores;
        pbd.partScores(listed, scores);
        size_t j = 0;
        for (size_t i = 0; i < listed.size(); ++i)
            for (size_t p = 0; p < listed[i].confidence().size(); ++p, ++j)
                std::printf("part_score %zu %zu %d %d %d %a %a %a %a\n", i, p, scores[j].x, scores[j].y, scores[j].m, scores[j].appearance,
                            scores[j].message, scores[j].bias, scores[j].total);
    }
    if (g_marginal_part >= 0) {          // the pose with part PART at the best cell of its max-marginals
        std::vector<MarginalLevel> levels;
        pbd.maxMarginals(im, levels);
        // the part's planes: component 0's parts come first, so its first plane is the types of the parts before it
        int g0 = 0, K = 0;
        const std::vector<std::vector<int> > &fid = model.filterid()[0];
        if ((size_t)g_marginal_part >= fid.size()) {
            std::fprintf(stderr, "--marginal-pose %d: component 0 has %zu parts\n", g_marginal_part, fid.size());
            return -1;
        }
        for (int p = 0; p < g_marginal_part; ++p) g0 += (int)fid[p].size();
        K = (int)fid[g_marginal_part].size();
        double best = 0;
        std::vector<int32_t> seed;
        for (size_t l = 0; l < levels.size(); ++l) {
            const MarginalLevel &L = levels[l];
            const size_t hw = (size_t)L.rows * L.cols;
            for (int m = 0; m < K; ++m)
                for (size_t i = 0; i < hw; ++i) {
                    const double v = L.values[(size_t)(g0 + m) * hw + i];
                    if (seed.empty() || v > best) {
                        best = v;
                        const int32_t sd[6] = {(int32_t)l, 0, g_marginal_part, m, (int32_t)(i % L.cols), (int32_t)(i / L.cols)};
                        seed.assign(sd, sd + 6);
                    }
                }
        }
        std::vector<int32_t> status;
        std::vector<Candidate> pose;
        if (!seed.empty()) pbd.marginalPoses(seed, status, pose);
        if (pose.empty()) {
            std::printf("marginal_pose %d none\n", g_marginal_part);
        } else {
            std::printf("marginal_pose %d %d %d %d %a\n", g_marginal_part, seed[0], seed[4], seed[5], (double)pose[0].score());
            report(pose, im, false, -1.f, -1.f, 1);
        }
    }
    if (mask_path) {                     // Candidate::mask and the masked image of the listed candidates
        if (!pbd.handle()) pbd.distributeModel(model);
        const std::vector<Candidate> listed(candidates.begin(), candidates.begin() + std::min<size_t>(candidates.size(), (size_t)top));
        std::vector<uint8_t> labels, masked;
        pbd.mask(im, listed, labels, masked_path ? &masked : NULL);
        size_t on = 0;
        for (size_t i = 0; i < labels.size(); ++i) on += labels[i] != 0;
        std::printf("mask %zu\n", on);
        if (!writePNM(mask_path, labels.data(), im.rows, im.cols, 1) ||
            (masked_path && !writePNM(masked_path, masked.data(), im.rows, im.cols, im.channels))) {
            std::fprintf(stderr, "cannot write the mask\n");
            return -1;
        }
    }
    return 0;
}

// every field the model readers fill, as text (doubles with 17 significant digits: exact round trip)
static int dump_model(const Model &m)
{
    std::printf("name %s\ninterval %d\nthresh %.9g\nsbin %d\nnorient %d\nflen %d\n", m.name().c_str(), m.nscales(), (double)m.thresh(),
                m.binsize(), m.norient(), m.flen());
    for (size_t f = 0; f < m.filtersw_.size(); ++f) {
        std::printf("filter %zu %d %d", f, m.filtersw_[f].rows, m.filtersw_[f].cols);
        for (size_t i = 0; i < m.filtersw_[f].data.size(); ++i) std::printf(" %.17g", m.filtersw_[f].data[i]);
        std::printf("\n");
    }
    std::printf("biasw");
    for (size_t i = 0; i < m.biasw_.size(); ++i) std::printf(" %.9g", (double)m.biasw_[i]);
    std::printf("\nanchors");
    for (size_t i = 0; i < m.anchors_.size(); ++i) std::printf(" %d,%d", m.anchors_[i].x, m.anchors_[i].y);
    std::printf("\n");
    for (size_t d = 0; d < m.defw_.size(); ++d) {
        std::printf("def %zu", d);
        for (size_t i = 0; i < m.defw_[d].size(); ++i) std::printf(" %.9g", (double)m.defw_[d][i]);
        std::printf("\n");
    }
    for (size_t c = 0; c < m.filterid_.size(); ++c)
        for (size_t p = 0; p < m.filterid_[c].size(); ++p) {
            std::printf("part %zu %zu parent %d filterid", c, p, m.parentid_[c][p]);
            for (size_t i = 0; i < m.filterid_[c][p].size(); ++i) std::printf(" %d", m.filterid_[c][p][i]);
            std::printf(" biasid");
            for (size_t i = 0; i < m.biasid_[c][p].size(); ++i) std::printf(" %d", m.biasid_[c][p][i]);
            std::printf(" defid");
            for (size_t i = 0; i < m.defid_[c][p].size(); ++i) std::printf(" %d", m.defid_[c][p][i]);
            std::printf("\n");
        }
    return 0;
}

// --augment: the image's augmented copy, written as a PNM
static int run_augment(Model &model, const Image &im, double degrees, bool mirror, const char *out_path)
{
    PartsBasedDetector<float> pbd(0, PBD_CONV_EXACT);
    pbd.distributeModel(model);
    pbd_augment job;
    job.frame = 0; job.mirror = mirror ? 1 : 0; job.degrees = degrees;
    std::vector<std::vector<unsigned char> > pixels;
    std::vector<Image> out;
    pbd.augmentFrames(std::vector<Image>(1, im), std::vector<pbd_augment>(1, job), pixels, out);
    std::printf("augment %d %d\n", out[0].rows, out[0].cols);
    if (!writePNM(out_path, pixels[0].data(), out[0].rows, out[0].cols, out[0].channels)) {
        std::fprintf(stderr, "cannot write the augmented image\n");
        return -1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "Usage: pbd_demo model_file image_file [--double] [--nms overlap] [--device-nms overlap] [--walk reference|argmax] [--root-nms sz] [--top-k k] [--scale-nms dl] [--pad x[,y]] [--fine-octave] [--top n] [--staged] [--stream handles frames] [--conv-mode 0..6 (5|6: matrix cores, any filter size, float only)] [--also image]... [--depth depth.pgm [--camera fx,fy,cx,cy] [--remove-planes] [--depth-consistency zfactor] [--depth-prune fx,width,tol] [--poses]] [--mask labels.pgm [--masked out.ppm]] [--part-scores] [--marginal-pose part] [--augment deg[,mirror] out.ppm]\n");
        return -1;
    }
    const char *augment_path = NULL;
    double augment_deg = 0;
    bool augment_mirror = false;
    bool dbl = false, staged = false;
    float nms = -1.f, dnms = -1.f;
    int top = 1 << 30, stream_k = 0, stream_n = 0, conv_mode = PBD_CONV_EXACT;
    std::vector<const char *> also;
    const char *depth_path = NULL;
    float dcz = -1.f;
    const char *mask_path = NULL, *masked_path = NULL;
    bool have_camera = false, remove_planes = false, poses = false;
    pbd_pinhole camera = {0, 0, 0, 0, 0, 0};
    for (int i = 3; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--double")) dbl = true;
        else if (!std::strcmp(argv[i], "--staged")) staged = true;
        else if (!std::strcmp(argv[i], "--remove-planes")) remove_planes = true;
        else if (!std::strcmp(argv[i], "--poses")) poses = true;
        else if (!std::strcmp(argv[i], "--part-scores")) g_part_scores = true;
        else if (!std::strcmp(argv[i], "--marginal-pose") && i + 1 < argc) g_marginal_part = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--mask") && i + 1 < argc) mask_path = argv[++i];
        else if (!std::strcmp(argv[i], "--masked") && i + 1 < argc) masked_path = argv[++i];
        else if (!std::strcmp(argv[i], "--nms") && i + 1 < argc) nms = (float)std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--device-nms") && i + 1 < argc) dnms = (float)std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--walk") && i + 1 < argc) {
            ++i;
            if (!std::strcmp(argv[i], "argmax")) g_walk = PBD_WALK_ARGMAX;
            else if (!std::strcmp(argv[i], "reference")) g_walk = PBD_WALK_REFERENCE;
            else { std::fprintf(stderr, "--walk takes reference or argmax\n"); return -1; }
        }
        else if (!std::strcmp(argv[i], "--root-nms") && i + 1 < argc) g_root_nms = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--top-k") && i + 1 < argc) {
            char tail = 0;
            if (std::sscanf(argv[++i], "%d%c", &g_top_k, &tail) != 1 || g_top_k < 0 || g_top_k > (1 << 30)) {
                std::fprintf(stderr, "--top-k takes a count, 0 (off) or 1..1073741824\n");
                return -1;
            }
        }
        else if (!std::strcmp(argv[i], "--scale-nms") && i + 1 < argc) {
            char tail = 0;
            if (std::sscanf(argv[++i], "%d%c", &g_scale_nms, &tail) != 1 || g_scale_nms < 0 || g_scale_nms > 255) {
                std::fprintf(stderr, "--scale-nms takes a level distance, 0..255\n");
                return -1;
            }
        }
        else if (!std::strcmp(argv[i], "--pad") && i + 1 < argc) {
            char tail = 0;
            const int got = std::sscanf(argv[++i], "%d,%d%c", &g_padx, &g_pady, &tail);
            if (got == 1) g_pady = g_padx;
            if (got < 1 || got > 2 || g_padx < 0 || g_padx > 31 || g_pady < 0 || g_pady > 31) {
                std::fprintf(stderr, "--pad takes x[,y], each 0..31 cells\n");
                return -1;
            }
        }
        else if (!std::strcmp(argv[i], "--fine-octave")) g_fine = true;
        else if (!std::strcmp(argv[i], "--top") && i + 1 < argc) top = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--conv-mode") && i + 1 < argc) conv_mode = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--stream") && i + 2 < argc) { stream_k = std::atoi(argv[++i]); stream_n = std::atoi(argv[++i]); }
        else if (!std::strcmp(argv[i], "--also") && i + 1 < argc) also.push_back(argv[++i]);
        else if (!std::strcmp(argv[i], "--depth") && i + 1 < argc) depth_path = argv[++i];
        else if (!std::strcmp(argv[i], "--depth-consistency") && i + 1 < argc) dcz = (float)std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--depth-prune") && i + 1 < argc) {
            char tail = 0;
            g_prune = std::sscanf(argv[++i], "%f,%f,%f%c", &g_prune_fx, &g_prune_width, &g_prune_tol, &tail) == 3;
            if (!g_prune) { std::fprintf(stderr, "--depth-prune takes fx,width,tol\n"); return -1; }
        }
        else if (!std::strcmp(argv[i], "--augment") && i + 2 < argc) {
            char word[8] = "", tail = 0;
            const int got = std::sscanf(argv[++i], "%lf,%7[a-z]%c", &augment_deg, word, &tail);
            augment_mirror = got == 2 && !std::strcmp(word, "mirror");
            if (got < 1 || got > 2 || (got == 2 && !augment_mirror)) { std::fprintf(stderr, "--augment takes deg[,mirror] out.ppm\n"); return -1; }
            augment_path = argv[++i];
        }
        else if (!std::strcmp(argv[i], "--camera") && i + 1 < argc) {
            have_camera = std::sscanf(argv[++i], "%lf,%lf,%lf,%lf", &camera.fx, &camera.fy, &camera.cx, &camera.cy) == 4;
            if (!have_camera) { std::fprintf(stderr, "--camera takes fx,fy,cx,cy\n"); return -1; }
        }
    }
    if (!also.empty() && (staged || stream_k > 0)) {
        std::fprintf(stderr, "--also runs one detectBatch call: not with --staged or --stream\n");
        return -1;
    }
    if (remove_planes && !have_camera) {
        std::fprintf(stderr, "--remove-planes needs --depth and --camera\n");
        return -1;
    }
    if (poses && !have_camera) {
        std::fprintf(stderr, "--poses needs --depth and --camera\n");
        return -1;
    }
    if (masked_path && !mask_path) {
        std::fprintf(stderr, "--masked needs --mask\n");
        return -1;
    }
    if (mask_path && !also.empty()) {
        std::fprintf(stderr, "--mask takes the one image of a single run: not with --also\n");
        return -1;
    }
    if (dcz >= 0 && (!depth_path || staged || stream_k > 0)) {
        std::fprintf(stderr, "--depth-consistency needs --depth, not with --staged or --stream\n");
        return -1;
    }
    if (g_prune && (!depth_path || staged)) {
        std::fprintf(stderr, "--depth-prune needs --depth, not with --staged\n");
        return -1;
    }
    if ((g_padx || g_pady) && (g_prune || g_marginal_part >= 0)) {
        std::fprintf(stderr, "--pad: depth pruning and max-marginals take no padded pyramid: not with --depth-prune or --marginal-pose\n");
        return -1;
    }
    if (g_top_k && staged) {
        std::fprintf(stderr, "--top-k is not applied by the staged run: not with --staged\n");
        return -1;
    }
    if (g_scale_nms >= 0 && staged) {
        std::fprintf(stderr, "--scale-nms is not applied by the staged run: not with --staged\n");
        return -1;
    }
    if (g_part_scores && (staged || stream_k > 0 || !also.empty())) {
        std::fprintf(stderr, "--part-scores reads the resident result of a single detect call: not with --staged, --stream or --also\n");
        return -1;
    }
    if (g_marginal_part >= 0 && (staged || stream_k > 0 || !also.empty())) {
        std::fprintf(stderr, "--marginal-pose reads the resident result of a single detect call: not with --staged, --stream or --also\n");
        return -1;
    }
    if (have_camera && !depth_path) {
        std::fprintf(stderr, "--camera needs --depth\n");
        return -1;
    }
    if (!also.empty() && depth_path) {
        std::fprintf(stderr, "--depth takes the one image of a single run: not with --also\n");
        return -1;
    }
    try {
        const std::string mpath = argv[1];
        const bool mat = mpath.size() >= 4 && mpath.compare(mpath.size() - 4, 4, ".mat") == 0;
        FileStorageModel fs_model;
        MatlabIOModel mat_model;
        Model &model = mat ? static_cast<Model &>(mat_model) : static_cast<Model &>(fs_model);
        if (!(mat ? mat_model.deserialize(mpath) : fs_model.deserialize(mpath))) { std::fprintf(stderr, "Error deserializing file\n"); return -1; }
        if (!std::strcmp(argv[2], "--dump-model")) return dump_model(model);
        std::vector<uint8_t> pix;
        Image im;
        if (!readPNM(argv[2], pix, im)) { std::fprintf(stderr, "Image not found, or invalid image format\n"); return -1; }
        if (augment_path) return run_augment(model, im, augment_deg, augment_mirror, augment_path);
        if (!also.empty()) {
            std::vector<std::vector<uint8_t> > pixels(also.size() + 1);
            std::vector<Image> ims(also.size() + 1);
            pixels[0].swap(pix);
            ims[0] = im;
            for (size_t k = 0; k < also.size(); ++k)
                if (!readPNM(also[k], pixels[k + 1], ims[k + 1])) { std::fprintf(stderr, "Image not found, or invalid image format\n"); return -1; }
            return dbl ? run_batch<double>(model, ims, nms, dnms, top, conv_mode) : run_batch<float>(model, ims, nms, dnms, top, conv_mode);
        }
        std::vector<uint8_t> dpix;
        Image depth;
        if (depth_path && !readPFM(depth_path, dpix, depth) && (!readPNM(depth_path, dpix, depth) || depth.channels != 1)) {
            std::fprintf(stderr, "Depth map not found, or not a PGM or grey PFM\n");
            return -1;
        }
        const Image *dp = depth_path ? &depth : NULL;
        const pbd_pinhole *cp = have_camera ? &camera : NULL;
        return dbl ? run<double>(model, im, staged, nms, dnms, top, stream_k, stream_n, conv_mode, dp, cp, remove_planes, dcz, mask_path,
                                 masked_path, poses)
                   : run<float>(model, im, staged, nms, dnms, top, stream_k, stream_n, conv_mode, dp, cp, remove_planes, dcz, mask_path,
                                masked_path, poses);
    } catch (const Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return -2;
    }
}
