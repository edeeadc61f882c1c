// pbd_host.hpp -- C++ host-side mirror of the reference's operator interface for the detection hot
// path, over the C ABI (pbd.h).  Header-only, no OpenCV, no Boost.  Class and method names follow the
// reference so that host code reads the same:
//
//   Model / FileStorageModel     include/Model.hpp:49-122, src/FileStorageModel.cpp:42-159 (YAML flavour)
//   HOGFeatures                  include/IFeatures.hpp:49-73 (binsize, nscales, scales, pyramid)
//   SpatialConvolutionEngine     include/IConvolutionEngine.hpp:44-68 (setFilters, pdf)
//   DynamicProgram               include/DynamicProgram.hpp:74-75 (min, argmin)
//   PartsBasedDetector           include/PartsBasedDetector.hpp:152-175 (distributeModel, detect, name)
//   Candidate                    include/Candidate.hpp:56-111,277-304 (score, sort, boundingBox, nonMaximaSuppression)
//
// Errors: the reference uses assert / CV_Error -> cv::Exception; here every failure of the C ABI is
// thrown as pbdhost::Error (a std::runtime_error) carrying pbd_last_error().
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <array>
#include <vector>

#include "pbd.h"
#include "pbd_bind.hpp"   // the ABI-calling bodies, shared with the OpenCV adapters (pbd_opencv_adapters.hpp)

namespace pbdhost {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

typedef pbdbind::PartScore PartScore;   // one part of a candidate's part scores (partScores, scorePlacements)
typedef pbdbind::MarginalLevel MarginalLevel;   // one level of the max-marginals (maxMarginals)

// ---------------------------------------------------------------------------------------------- basics
struct Rect {
    int x, y, width, height;
    Rect() : x(0), y(0), width(0), height(0) {}
    Rect(int x_, int y_, int w_, int h_) : x(x_), y(y_), width(w_), height(h_) {}
    int area() const { return width * height; }
    bool empty() const { return width <= 0 || height <= 0; }
    Rect operator|(const Rect &b) const
    {   // cv::Rect union
        if (empty()) return b;
        if (b.empty()) return *this;
        const int x1 = std::min(x, b.x), y1 = std::min(y, b.y);
        return Rect(x1, y1, std::max(x + width, b.x + b.width) - x1, std::max(y + height, b.y + b.height) - y1);
    }
    Rect operator&(const Rect &b) const
    {   // cv::Rect intersection
        const int x1 = std::max(x, b.x), y1 = std::max(y, b.y);
        const int w = std::min(x + width, b.x + b.width) - x1, h = std::min(y + height, b.y + b.height) - y1;
        return (w <= 0 || h <= 0) ? Rect() : Rect(x1, y1, w, h);
    }
};

template <typename T>
struct MatT {   // dense row-major matrix (the role cv::Mat_<T> plays at the reference's seams)
    int rows, cols;
    std::vector<T> data;
    MatT() : rows(0), cols(0) {}
    MatT(int r, int c) : rows(r), cols(c), data((size_t)r * c) {}
    T *ptr(int r = 0) { return data.data() + (size_t)r * cols; }
    const T *ptr(int r = 0) const { return data.data() + (size_t)r * cols; }
};

struct Point {   // cv::Point at the reference's seams (Model::anchors, include/Model.hpp:66)
    int x, y;
    Point() : x(0), y(0) {}
    Point(int x_, int y_) : x(x_), y(y_) {}
};

struct Image {   // image view: rows x cols x channels, BGR interleaved when channels == 3
    const void *data;
    int rows, cols, channels;
    size_t step;   // bytes between rows (cv::Mat::step)
    int depth;     // cv::Mat::depth(): 0 = 8U, 2 = 16U, 5 = 32F, 6 = 64F (src/HOGFeatures.cpp:136-146)
    Image() : data(NULL), rows(0), cols(0), channels(0), step(0), depth(0) {}
};

// include/Rect3.hpp:53-64: a 3-D box in the reference's member order (x, y, z, height, width, depth)
struct Rect3d {
    double x, y, z, height, width, depth;
    Rect3d() : x(0), y(0), z(0), height(0), width(0), depth(0) {}
};

// pcl::PointXYZ's coordinates
struct Point3f {
    float x, y, z;
    Point3f() : x(0), y(0), z(0) {}
};

class Candidate {
public:
    std::vector<Rect> parts_;
    std::vector<float> confidence_;
    int component_;
    int frame, level, root_x, root_y;   // where the candidate was back-tracked from
    Candidate() : component_(0), frame(0), level(0), root_x(0), root_y(0) {}
    const std::vector<Rect> &parts() const { return parts_; }
    const std::vector<float> &confidence() const { return confidence_; }
    void addPart(Rect r, float confidence) { parts_.push_back(r); confidence_.push_back(confidence); }
    float score() const { return confidence_.size() ? confidence_[0] : -std::numeric_limits<float>::infinity(); }
    int component() const { return component_; }
    static bool descending(const Candidate &a, const Candidate &b) { return a.score() > b.score(); }
    static void sort(std::vector<Candidate> &c) { std::sort(c.begin(), c.end(), descending); }
    Rect boundingBox() const
    {
        Rect hull = parts_[0];
        for (size_t n = 0; n < parts_.size(); ++n) hull = hull | parts_[n];
        return hull;
    }
    // greedy paint-the-canvas suppression, include/Candidate.hpp:277-304
    static void nonMaximaSuppression(int rows, int cols, std::vector<Candidate> &candidates, float overlap = 0.0f)
    {
        const Rect bounds(0, 0, cols, rows);
        std::vector<uint8_t> scratch((size_t)rows * cols, 0);
        size_t keep = 0;
        for (size_t n = 0; n < candidates.size(); ++n) {
            const Rect box = candidates[n].boundingBox() & bounds;
            double boxsum = 0;
            for (int y = box.y; y < box.y + box.height; ++y)
                for (int x = box.x; x < box.x + box.width; ++x) boxsum += scratch[(size_t)y * cols + x];
            if (boxsum / box.area() > overlap) continue;   // 0/0 = NaN compares false: an empty box is kept
            for (int y = box.y; y < box.y + box.height; ++y)
                for (int x = box.x; x < box.x + box.width; ++x) scratch[(size_t)y * cols + x] = 1;
            candidates[keep++] = candidates[n];
        }
        candidates.resize(keep);
    }
};

// ---------------------------------------------------------------------------------------------- model
class Model {
public:
    std::string name_;
    int nscales_ = 10;   // the interval (src/FileStorageModel.cpp:105)
    float thresh_ = 0;
    int binsize_ = 4, flen_ = 32, norient_ = 18;
    std::vector<MatT<double> > filtersw_;
    std::vector<float> biasw_;
    std::vector<Point> anchors_;
    std::vector<std::vector<float> > defw_;
    std::vector<std::vector<std::vector<int> > > biasid_, filterid_, defid_;
    std::vector<std::vector<int> > parentid_;

    // accessors named as the reference's (include/Model.hpp:99-121)
    std::vector<MatT<double> > &filters() { return filtersw_; }
    std::vector<float> &bias() { return biasw_; }
    std::vector<std::vector<float> > &def() { return defw_; }
    std::vector<Point> &anchors() { return anchors_; }
    std::vector<std::vector<std::vector<int> > > &filterid() { return filterid_; }
    std::vector<std::vector<std::vector<int> > > &biasid() { return biasid_; }
    std::vector<std::vector<std::vector<int> > > &defid() { return defid_; }
    std::vector<std::vector<int> > &parentid() { return parentid_; }
    std::string name() const { return name_; }
    float thresh() const { return thresh_; }
    int binsize() const { return binsize_; }
    int nscales() const { return nscales_; }
    int flen() const { return flen_; }
    int norient() const { return norient_; }
    int ncomponents() const { return (int)filterid_.size(); }
    virtual ~Model() {}
};

// YAML flavour of cv::FileStorage as FileStorageModel writes it (subset: block mappings/sequences, flow
// sequences, !!opencv-matrix).  See partsbaseddetector_amd/filestorage.py for the Python twin (+ XML).
class FileStorageModel : public Model {
    struct Node {
        std::string scalar;
        std::vector<Node> seq;
        std::vector<std::pair<std::string, Node> > map;
        bool is_seq = false, is_map = false;
        const Node &operator[](const std::string &k) const
        {
            for (size_t i = 0; i < map.size(); ++i)
                if (map[i].first == k) return map[i].second;
            throw Error(PBD_ERR_INVALID, "model file: missing key '" + k + "'");
        }
        bool has(const std::string &k) const
        {
            for (size_t i = 0; i < map.size(); ++i)
                if (map[i].first == k) return true;
            return false;
        }
        double num() const { return parse_num(scalar); }
        std::vector<double> nums() const
        {
            std::vector<double> v;
            if (is_seq) for (size_t i = 0; i < seq.size(); ++i) { if (seq[i].is_seq) { std::vector<double> s = seq[i].nums(); v.insert(v.end(), s.begin(), s.end()); } else v.push_back(seq[i].num()); }
            else if (!scalar.empty()) v.push_back(num());
            return v;
        }
    };
    static double parse_num(const std::string &t)
    {
        if (t == ".Inf" || t == ".inf" || t == "+.Inf") return std::numeric_limits<double>::infinity();
        if (t == "-.Inf" || t == "-.inf") return -std::numeric_limits<double>::infinity();
        if (t == ".Nan" || t == ".nan" || t == ".NaN") return std::numeric_limits<double>::quiet_NaN();
        return std::strtod(t.c_str(), NULL);
    }
    static std::string trim(const std::string &s)
    {
        size_t a = s.find_first_not_of(" \t\r"), b = s.find_last_not_of(" \t\r");
        return a == std::string::npos ? "" : s.substr(a, b - a + 1);
    }
    static int indent_of(const std::string &s) { return (int)s.find_first_not_of(' '); }
    static Node flow(const std::string &t, size_t &pos)
    {
        Node n; n.is_seq = true;
        ++pos;   // '['
        std::string tok;
        for (;;) {
            const char ch = t[pos];
            if (ch == '[') { n.seq.push_back(flow(t, pos)); tok.clear(); }
            else if (ch == ',' || ch == ']') {
                if (!trim(tok).empty()) { Node s; s.scalar = trim(tok); n.seq.push_back(s); }
                tok.clear();
                ++pos;
                if (ch == ']') return n;
            } else { tok += ch; ++pos; }
        }
    }
    static Node value(const std::string &rest)
    {
        if (!rest.empty() && rest[0] == '[') { size_t p = 0; return flow(rest, p); }
        Node s;
        s.scalar = rest;
        if (s.scalar.size() >= 2 && s.scalar[0] == '"') s.scalar = s.scalar.substr(1, s.scalar.size() - 2);
        return s;
    }
    static Node block(const std::vector<std::string> &L, size_t &i, int indent)
    {
        Node n;
        const bool seq = trim(L[i])[0] == '-';
        n.is_seq = seq; n.is_map = !seq;
        while (i < L.size()) {
            const int cur = indent_of(L[i]);
            if (cur < indent) break;
            const std::string body = trim(L[i]);
            if (seq) {
                std::string item = trim(body.substr(1));
                if (item.compare(0, 15, "!!opencv-matrix") == 0) { ++i; n.seq.push_back(block(L, i, cur + 2)); continue; }
                if (item.empty()) { ++i; n.seq.push_back(block(L, i, cur + 1)); continue; }
                n.seq.push_back(value(item));
                ++i;
            } else {
                const size_t c = body.find(':');
                const std::string key = body.substr(0, c), rest = trim(body.substr(c + 1));
                if (rest.compare(0, 15, "!!opencv-matrix") == 0) { ++i; n.map.push_back(std::make_pair(key, block(L, i, cur + 1))); continue; }
                if (rest.empty()) {
                    if (i + 1 < L.size() && indent_of(L[i + 1]) > cur) {
                        const int nxt = indent_of(L[i + 1]);
                        ++i;
                        n.map.push_back(std::make_pair(key, block(L, i, nxt)));
                        continue;
                    }
                    Node e; e.is_seq = true;
                    n.map.push_back(std::make_pair(key, e));
                } else {
                    n.map.push_back(std::make_pair(key, value(rest)));
                }
                ++i;
            }
        }
        return n;
    }
    static std::vector<int> ints(const Node &n)
    {
        std::vector<double> v = n.nums();
        return std::vector<int>(v.begin(), v.end());
    }

    // ---- the <opencv_storage> XML flavour (what the reference's configs name: conf/config_person.by_parts:30,
    // conf/config_face.by_parts:31).  Elements with children become maps (sequences when every child is <_>),
    // leaves become scalars or, with several whitespace-separated tokens, sequences; attributes are not needed
    // (an opencv-matrix is recognised by its rows / cols / data children).
    static void xml_skip(const std::string &t, size_t &p)
    {   // whitespace, comments, processing instructions
        for (;;) {
            while (p < t.size() && (t[p] == ' ' || t[p] == '\n' || t[p] == '\r' || t[p] == '\t')) ++p;
            if (t.compare(p, 4, "<!--") == 0) { const size_t e = t.find("-->", p); p = e == std::string::npos ? t.size() : e + 3; continue; }
            if (t.compare(p, 2, "<?") == 0) { const size_t e = t.find("?>", p); p = e == std::string::npos ? t.size() : e + 2; continue; }
            return;
        }
    }
    static Node xml_leaf(const std::string &text)
    {
        const std::string body = trim_ws(text);
        Node n;
        if (body.empty()) return n;
        if (body[0] == '"') { n.scalar = body.substr(1, body.rfind('"') - 1); return n; }
        std::vector<std::string> toks;
        std::istringstream is(body);
        for (std::string tk; is >> tk;) toks.push_back(tk);
        if (toks.size() == 1) { n.scalar = toks[0]; return n; }
        n.is_seq = true;
        for (size_t i = 0; i < toks.size(); ++i) { Node e; e.scalar = toks[i]; n.seq.push_back(e); }
        return n;
    }
    static std::string trim_ws(const std::string &s)
    {
        size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
        return a == std::string::npos ? "" : s.substr(a, b - a + 1);
    }
    // parses the element starting at t[p] == '<'; returns its tag and value
    static Node xml_element(const std::string &t, size_t &p, std::string &tag)
    {
        if (p >= t.size() || t[p] != '<') throw Error(PBD_ERR_INVALID, "model file: malformed XML");
        const size_t gt = t.find('>', p);
        if (gt == std::string::npos) throw Error(PBD_ERR_INVALID, "model file: unterminated XML tag");
        std::string head = t.substr(p + 1, gt - p - 1);
        const bool self_closed = !head.empty() && head[head.size() - 1] == '/';
        if (self_closed) head.erase(head.size() - 1);
        tag = head.substr(0, head.find_first_of(" \t\r\n"));
        p = gt + 1;
        Node n;
        if (self_closed) return n;
        std::string text;
        std::vector<std::pair<std::string, Node> > kids;
        for (;;) {
            const size_t lt = t.find('<', p);
            if (lt == std::string::npos) throw Error(PBD_ERR_INVALID, "model file: unterminated XML element <" + tag + ">");
            text += t.substr(p, lt - p);
            p = lt;
            if (t.compare(p, 4, "<!--") == 0) { xml_skip(t, p); continue; }
            if (t.compare(p, 2, "<?") == 0) { xml_skip(t, p); continue; }
            if (t.compare(p, 2, "</") == 0) {
                const size_t close = t.find('>', p);
                if (close == std::string::npos) throw Error(PBD_ERR_INVALID, "model file: unterminated closing tag of <" + tag + ">");
                if (trim_ws(t.substr(p + 2, close - p - 2)) != tag)
                    throw Error(PBD_ERR_INVALID, "model file: <" + tag + "> closed by </" + trim_ws(t.substr(p + 2, close - p - 2)) + ">");
                p = close + 1;
                break;
            }
            std::string ktag;
            Node kid = xml_element(t, p, ktag);
            kids.push_back(std::make_pair(ktag, kid));
        }
        if (kids.empty()) return xml_leaf(text);
        bool all_items = true;
        for (size_t i = 0; i < kids.size(); ++i) all_items = all_items && kids[i].first == "_";
        if (all_items) { n.is_seq = true; for (size_t i = 0; i < kids.size(); ++i) n.seq.push_back(kids[i].second); }
        else { n.is_map = true; n.map = kids; }
        return n;
    }
    static Node xml_document(const std::string &t)
    {
        size_t p = 0;
        xml_skip(t, p);
        std::string tag;
        Node root = xml_element(t, p, tag);
        if (tag != "opencv_storage") throw Error(PBD_ERR_INVALID, "model file: root element <" + tag + "> is not <opencv_storage>");
        return root;
    }

public:
    bool deserialize(const std::string &filename)
    {   // src/FileStorageModel.cpp:96-159
        std::ifstream in(filename.c_str());
        if (!in) return false;
        std::stringstream whole;
        whole << in.rdbuf();
        const std::string text = whole.str();
        const size_t first = text.find_first_not_of(" \t\r\n");
        const bool is_xml = first != std::string::npos && text[first] == '<';
        Node doc;
        if (is_xml) {
            doc = xml_document(text);
        } else {
            std::vector<std::string> raw, L;
            std::istringstream lines(text);
            for (std::string ln; std::getline(lines, ln);) {
                if (!ln.empty() && ln[0] == '%') continue;
                if (trim(ln).empty() || trim(ln) == "---") continue;
                raw.push_back(ln);
            }
            int depth = 0;   // join flow sequences wrapped over several lines
            for (size_t i = 0; i < raw.size(); ++i) {
                if (depth == 0) L.push_back(raw[i]); else L.back() += " " + trim(raw[i]);
                for (size_t k = 0; k < raw[i].size(); ++k) depth += (raw[i][k] == '[') - (raw[i][k] == ']');
            }
            size_t i = 0;
            doc = block(L, i, 0);
        }
        name_ = doc.has("name") ? doc["name"].scalar : "";
        nscales_ = (int)doc["interval"].num();
        thresh_ = (float)doc["thresh"].num();
        binsize_ = (int)doc["sbin"].num();
        norient_ = (int)doc["norient"].num();
        flen_ = (int)doc["flen"].num();
        filtersw_.clear();
        const Node &fw = doc["filtersw"];
        for (size_t f = 0; f < fw.seq.size(); ++f) {
            const Node &m = fw.seq[f];
            MatT<double> w((int)m["rows"].num(), (int)m["cols"].num());
            const std::vector<double> d = m["data"].nums();
            if (d.size() != w.data.size()) throw Error(PBD_ERR_INVALID, "model file: filter size mismatch");
            w.data = d;
            filtersw_.push_back(w);
        }
        biasw_.clear();
        { std::vector<double> b = doc["biasw"].nums(); biasw_.assign(b.begin(), b.end()); }
        anchors_.clear();
        { std::vector<double> a = doc["anchors"].nums(); for (size_t k = 0; k + 1 < a.size(); k += 2) anchors_.push_back(Point((int)a[k], (int)a[k + 1])); }
        defw_.clear();
        const Node &defs = doc["defs"];
        for (size_t d = 0; d < defs.seq.size(); ++d) { std::vector<double> w = defs.seq[d].nums(); defw_.push_back(std::vector<float>(w.begin(), w.end())); }
        const Node &comps = doc["indexers"];
        const size_t nc = comps.map.size();
        parentid_.assign(nc, std::vector<int>());
        filterid_.assign(nc, std::vector<std::vector<int> >());
        biasid_ = filterid_; defid_ = filterid_;
        for (size_t c = 0; c < nc; ++c) {
            std::ostringstream cs; cs << "component-" << c;
            const Node &parts = comps[cs.str()];
            for (size_t p = 0; p < parts.map.size(); ++p) {
                std::ostringstream ps; ps << "part-" << p;
                const Node &part = parts[ps.str()];
                parentid_[c].push_back((int)part["parentid"].num());
                filterid_[c].push_back(ints(part["filterid"]));
                biasid_[c].push_back(ints(part["biasid"]));
                // what the writer wrote (scalar, sequence or empty), not the fork's isInt() shortcut
                // that collapses multi-mixture defids to [0] (src/FileStorageModel.cpp:148-152)
                defid_[c].push_back(part.has("defid") ? ints(part["defid"]) : std::vector<int>());
            }
        }
        return true;
    }
};

// ---------------------------------------------------------------------------------------------- engines
// The traits pbd_bind.hpp's templates are instantiated with here (the OpenCV adapters supply the cv::Mat twin).
template <typename T>
struct HostTraits {
    typedef T Real;
    typedef MatT<T> Mat;
    typedef MatT<int32_t> IMat;
    typedef MatT<double> FilterMat;
    typedef pbdhost::Image Image;
    typedef pbdhost::Candidate Candidate;
    static void create(Mat &m, int rows, int cols) { m = Mat(rows, cols); }
    static T *ptr(Mat &m) { return m.ptr(); }
    static const T *cptr(const Mat &m) { return m.ptr(); }
    static int rows(const Mat &m) { return m.rows; }
    static int cols(const Mat &m) { return m.cols; }
    static void icreate(IMat &m, int rows, int cols) { m = IMat(rows, cols); }
    static int32_t *iptr(IMat &m) { return m.ptr(); }
    static Mat real_continuous(const Mat &m) { return m; }                 // MatT is always continuous T data
    static Mat rows_view(Mat &m, int r0, int r1)
    {   // MatT has no views: a copy
        Mat r(r1 - r0, m.cols);
        std::copy(m.ptr(r0), m.ptr(r0) + r.data.size(), r.data.begin());
        return r;
    }
    static const void *img_data(const Image &im) { return im.data; }
    static int img_rows(const Image &im) { return im.rows; }
    static int img_cols(const Image &im) { return im.cols; }
    static int img_channels(const Image &im) { return im.channels; }
    static size_t img_step(const Image &im) { return im.step; }
    static int img_depth(const Image &im) { return im.depth; }
    static void fail(int rc, const std::string &text) { throw Error(rc, text); }
    static void candidate(std::vector<Candidate> &out, const pbd_candidate_hdr &hd, const int32_t *r)
    {
        Candidate c;
        c.component_ = hd.component; c.frame = hd.frame; c.level = hd.level; c.root_x = hd.root_x; c.root_y = hd.root_y;
        for (int p = 0; p < hd.nparts; ++p) c.addPart(Rect(r[4 * p], r[4 * p + 1], r[4 * p + 2], r[4 * p + 3]), p == 0 ? hd.score : 0.0f);
        out.push_back(c);
    }
    static int filter_rows(const FilterMat &w) { return w.rows; }
    static void filter_values(const FilterMat &w, std::vector<double> &out) { out.insert(out.end(), w.data.begin(), w.data.end()); }
};

template <typename T>
class HOGFeatures {   // IFeatures
    pbd_handle *h_;
    std::vector<float> scales_;
public:
    explicit HOGFeatures(pbd_handle *h) : h_(h) {}
    size_t binsize() const { return (size_t)pbd_binsize(h_); }
    size_t nscales() const { return scales_.size(); }
    std::vector<float> scales() const { return scales_; }
    void pyramid(const Image &im, std::vector<MatT<T> > &pyrafeatures) { pbdbind::pyramid<HostTraits<T> >(h_, im, pyrafeatures, scales_); }
};

template <typename T>
class SpatialConvolutionEngine {   // IConvolutionEngine
    pbd_handle *h_;
    size_t nfilters_;
public:
    SpatialConvolutionEngine(pbd_handle *h, size_t nfilters) : h_(h), nfilters_(nfilters) {}
    void setFilters(const std::vector<MatT<T> > &filters)
    {
        pbdbind::set_filters<HostTraits<T> >(h_, filters);
        nfilters_ = filters.size();
    }
    // responses[level][filter] = H x W
    void pdf(const std::vector<MatT<T> > &features, std::vector<std::vector<MatT<T> > > &responses)
    {
        pbdbind::pdf<HostTraits<T> >(h_, nfilters_, features, responses);
    }
};

template <typename T>
class DynamicProgram {
    pbd_handle *h_;
    int nfilters_;
public:
    DynamicProgram(pbd_handle *h, int nfilters) : h_(h), nfilters_(nfilters) {}
    // scores[level][filter]; rootv/rooti[level][component]; the back-pointers stay on the device for argmin()
    void min(const std::vector<std::vector<MatT<T> > > &scores, std::vector<std::vector<MatT<T> > > &rootv,
             std::vector<std::vector<MatT<int32_t> > > &rooti, int ncomponents)
    {
        pbdbind::dp_min<HostTraits<T> >(h_, nfilters_, ncomponents, scores, rootv, rooti);
    }
    void argmin(const std::vector<float> &scales, std::vector<Candidate> &candidates, int capacity = 1 << 16)
    {
        pbdbind::dp_argmin<HostTraits<T> >(h_, scales, candidates, capacity);
    }
};

// The training QP (include/pbd.h pbd_qp_*, matlab/learning/qp_*.m) over a device-resident example cache: created by
// PartsBasedDetector::qp and independent of the detector afterwards (RAII; movable, not copyable).  Every call is synchronous.
class QP {
public:
    explicit QP(pbd_qp *q = NULL) : q_(q) {}
    ~QP() { if (q_) pbd_qp_destroy(q_); }
    QP(QP &&o) : q_(o.q_) { o.q_ = NULL; }
    QP &operator=(QP &&o) { std::swap(q_, o.q_); return *this; }
    QP(const QP &) = delete;
    QP &operator=(const QP &) = delete;
    pbd_qp *get() const { return q_; }
    // qp_write of examples of handle h (PartsBasedDetector::examples, handle()); ids: 5 words per example
    // ({label, frame, level, root x, root y} is detect.m's); the number written
    template <typename T>
    int add(pbd_handle *h, const std::vector<int32_t> &hdr, const std::vector<T> &values, const std::vector<int32_t> &ids)
    {
        return pbdbind::qp_add<HostTraits<T> >(q_, h, hdr, values, ids);
    }
    void fix() { pbdbind::qp_check<HostTraits<float> >(q_, pbd_qp_fix(q_)); }
    // train.m:75's qp.n = 0: an empty cache again, the bounds NaN as after create (pbd_qp_clear)
    void clear() { pbdbind::qp_check<HostTraits<float> >(q_, pbd_qp_clear(q_)); }
    // detect.m:135: ub += Cl * R(max(0, 1 - y * score)) over the records present in a device payload of the detector the QP
    // was created from (pbd_qp_add_loss_device); the addend
    double addLoss(const int32_t *d_payload, int capacity, int label = -1)
    {
        double added = 0;
        pbdbind::qp_check<HostTraits<float> >(q_, pbd_qp_add_loss_device(q_, d_payload, capacity, label, &added));
        return added;
    }
    int prune()
    {
        int n = 0;
        pbdbind::qp_check<HostTraits<float> >(q_, pbd_qp_prune(q_, &n));
        return n;
    }
    // one pass; order: indices into the support-vector set (empty: the seeded order of include/pbd.h)
    pbd_qp_info one(const std::vector<int32_t> &order = std::vector<int32_t>(), uint64_t seed = 0)
    {
        return pbdbind::qp_one<HostTraits<float> >(q_, order, seed);
    }
    pbd_qp_info opt(double tol = 0.05, int iter = 1000, uint64_t seed = 0) { return pbdbind::qp_opt<HostTraits<float> >(q_, tol, iter, seed); }
    std::vector<double> weights() { return pbdbind::qp_weights<HostTraits<float> >(q_); }   // qp_w: the model vector
    std::vector<double> scores() { return pbdbind::qp_scores<HostTraits<float> >(q_); }     // qp_scorepos
    // model = vec2model(qp_w, model) in place: handle h (PartsBasedDetector::handle()) takes weights(), on the device
    void apply(pbd_handle *h) { pbdbind::qp_apply<HostTraits<float> >(q_, h); }
    pbd_qp_info state() { return pbdbind::qp_state<HostTraits<float> >(q_); }

private:
    pbd_qp *q_;
};

// what PartsBasedDetector::clusterParts returns (pbd_cluster_parts): rows of 16 types per part, unused or empty types NaN / 0
struct PartClusters {
    std::vector<int32_t> idx;                  // [part][positive] 0-based type
    std::vector<double> centres;               // [part][16][2]
    std::vector<int32_t> counts, anchors;      // [part][16], [part][16][2]
    std::vector<pbd_cluster_info> info;        // [part] the picked trial
    std::vector<double> sumdist_all;           // [part][trial]
    std::vector<int32_t> iters_all;            // [part][trial]
};

template <typename T>
class PartsBasedDetector {
    std::string name_;
    pbd_handle *h_;
    int device_;
    int conv_mode_;
    int max_batch_;
    bool nms_;
    float overlap_;
    int walk_;
    int root_nms_;
    int top_k_;
    bool scale_nms_on_;
    int scale_nms_dl_;
    int padx_, pady_;
    bool fine_;
    bool depth_on_;
    float zfactor_;
    bool prune_on_;
    float prune_fx_, prune_width_, prune_tol_;
    int planes_;                         // the (part, type) pairs of the distributed model: planes of a max-marginal level
    PartsBasedDetector(const PartsBasedDetector &);
    PartsBasedDetector &operator=(const PartsBasedDetector &);
public:
    // conv_mode: the convolution of every handle distributeModel() creates (PBD_CONV_*, include/pbd.h); new surface, the
    // reference has only its exact convolution.  T = float: every mode but PBD_CONV_MFMA_F64 (PBD_CONV_MFMA / _F16 for all-5x5
    // models, PBD_CONV_MFMA_ANY / _F16_ANY for any filter sizes); T = double: PBD_CONV_EXACT, PBD_CONV_FMA, PBD_CONV_MFMA_F64
    // max_batch: the most images one detectBatch() call takes
    explicit PartsBasedDetector(int device = 0, int conv_mode = PBD_CONV_EXACT, int max_batch = 64)
        : h_(NULL), device_(device), conv_mode_(conv_mode), max_batch_(max_batch), nms_(false), overlap_(0.f), walk_(PBD_WALK_REFERENCE),
          root_nms_(0), top_k_(0), scale_nms_on_(false), scale_nms_dl_(0), padx_(0), pady_(0), fine_(false), depth_on_(false), zfactor_(0.03f), prune_on_(false), prune_fx_(0.f), prune_width_(0.f), prune_tol_(0.3f),
          planes_(0) {}
    ~PartsBasedDetector() { pbd_destroy(h_); }
    const std::string &name() const { return name_; }
    pbd_handle *handle() const { return h_; }
    void distributeModel(Model &model)
    {   // src/PartsBasedDetector.cpp:102-127
        pbd_destroy(h_);
        h_ = NULL;
        h_ = pbdbind::create<HostTraits<T> >(model, device_, conv_mode_, max_batch_, 1 << 18);
        if (nms_) pbdbind::set_nms<HostTraits<T> >(h_, true, overlap_);
        if (walk_ != PBD_WALK_REFERENCE) pbdbind::check<HostTraits<T> >(h_, pbd_set_walk(h_, walk_));
        if (root_nms_) pbdbind::set_root_nms<HostTraits<T> >(h_, root_nms_);
        if (top_k_) pbdbind::set_top_k<HostTraits<T> >(h_, top_k_);
        if (scale_nms_on_) pbdbind::set_scale_nms<HostTraits<T> >(h_, true, scale_nms_dl_);
        if (padx_ || pady_) pbdbind::set_padding<HostTraits<T> >(h_, padx_, pady_);
        if (fine_) pbdbind::set_fine_octave<HostTraits<T> >(h_, true);
        if (prune_on_) pbdbind::set_depth_prune<HostTraits<T> >(h_, true, prune_fx_, prune_width_, prune_tol_);
        name_ = model.name();
        planes_ = 0;
        for (size_t c = 0; c < model.filterid().size(); ++c)
            for (size_t p = 0; p < model.filterid()[c].size(); ++p) planes_ += (int)model.filterid()[c][p].size();
    }
    // new surface: detect() returns Candidate::sort + Candidate::nonMaximaSuppression(im, candidates, overlap) of what it
    // found, computed on the device (pbd_set_nms) -- the callers' post-step, cells/detect.cpp:237-238.  Kept across
    // distributeModel(); a negative overlap turns it off.
    void setNonMaximaSuppression(float overlap)
    {
        if (h_) pbdbind::set_nms<HostTraits<T> >(h_, overlap >= 0, overlap);
        nms_ = overlap >= 0;
        overlap_ = overlap;
    }
    // new surface: how a root is walked to its parts from now on (pbd_set_walk): PBD_WALK_REFERENCE, the reference's composed
    // back-pointers (the default), or PBD_WALK_ARGMAX, the placement the score was taken at -- part boxes, examples() and
    // detectLatent() follow it.  Kept across distributeModel().
    void setWalk(int mode)
    {
        if (mode != PBD_WALK_REFERENCE && mode != PBD_WALK_ARGMAX) throw Error(PBD_ERR_INVALID, "walk mode");
        if (h_) pbdbind::check<HostTraits<T> >(h_, pbd_set_walk(h_, mode));
        walk_ = mode;
    }
    // new surface: the reference's commented-out ssp_.nonMaxSuppression(rootv, scales) (src/PartsBasedDetector.cpp:86) from now on
    // (pbd_set_root_nms): only the roots that are grid maxima of their rootv plane within sz cells are walked and returned;
    // sz = 0 turns it off (the default).  Kept across distributeModel().
    void setRootNMS(int sz)
    {
        if (sz < 0 || sz > 32767) throw Error(PBD_ERR_INVALID, "root NMS window: 0 (off) or 1..32767");
        if (h_) pbdbind::set_root_nms<HostTraits<T> >(h_, sz);
        root_nms_ = sz;
    }
    // nonMaximaSuppression(src, sz, dst, mask) (src/nms.cpp:84-129) on the device (pbd_grid_nms): dst becomes src.rows x src.cols
    // bytes of 0 / 255; mask: empty, or that many bytes
    void gridNMS(const MatT<T> &src, int sz, std::vector<uint8_t> &dst, const std::vector<uint8_t> &mask = std::vector<uint8_t>())
    {
        if (!h_) throw Error(PBD_ERR_STATE, "gridNMS() before distributeModel()");
        const size_t n = (size_t)src.rows * src.cols;
        if (!mask.empty() && mask.size() != n) throw Error(PBD_ERR_INVALID, "gridNMS: the mask has the plane's size");
        dst.assign(n, 0);
        pbdbind::grid_nms<HostTraits<T> >(h_, src, sz, mask.empty() ? NULL : &mask[0], n ? &dst[0] : NULL);
    }
    // new surface: the padded pyramid of the Matlab detector from now on (pbd_set_padding): every feature level grows by padx / pady
    // cells of the boundary occlusion feature on each side, so that roots and parts can lie outside the frame; (0, 0) turns it off
    // (the default).  A Candidate's root is then a cell of the padded plane; its part boxes are frame coordinates as always.  Kept
    // across distributeModel().  Not with setDepthPrune; maxMarginals / marginalPoses refuse a padded result.
    void setPadding(int padx, int pady)
    {
        if (padx < 0 || padx > 31 || pady < 0 || pady > 31) throw Error(PBD_ERR_INVALID, "padding: 0..31 cells");
        if (h_) pbdbind::set_padding<HostTraits<T> >(h_, padx, pady);
        padx_ = padx;
        pady_ = pady;
    }
    // new surface: search an octave above the frame from now on (pbd_set_fine_octave): the first `interval` pyramid levels are
    // computed a second time at bin size sbin / 2 on the same level images, so that an object of half the template's size is found.
    // These levels come first: a Candidate's level then indexes the longer list.  Needs an even sbin >= 4.  Kept across
    // distributeModel(); off by default.
    void setFineOctave(bool on)
    {
        if (h_) pbdbind::set_fine_octave<HostTraits<T> >(h_, on);
        fine_ = on;
    }
    // new surface: at most k candidates per frame from now on (pbd_set_top_k): only the k best roots of each frame -- by score, ties
    // to the earlier cell -- among those the threshold, depth pruning and root NMS leave are walked and returned; k = 0 turns it
    // off (the default).  Kept across distributeModel().
    void setTopK(int k)
    {
        if (k < 0 || k > (1 << 30)) throw Error(PBD_ERR_INVALID, "top-K: 0 (off) or 1..2^30");
        if (h_) pbdbind::set_top_k<HostTraits<T> >(h_, k);
        top_k_ = k;
    }
    // the k best elements of src that are not NaN (and not masked out), ties to the smaller row-major index, selected on the device
    // (pbd_top_k_cells): dst becomes src.rows x src.cols bytes of 0 / 255; mask: empty, or that many bytes
    void topKCells(const MatT<T> &src, int k, std::vector<uint8_t> &dst, const std::vector<uint8_t> &mask = std::vector<uint8_t>())
    {
        if (!h_) throw Error(PBD_ERR_STATE, "topKCells() before distributeModel()");
        const size_t n = (size_t)src.rows * src.cols;
        if (!mask.empty() && mask.size() != n) throw Error(PBD_ERR_INVALID, "topKCells: the mask has the array's size");
        dst.assign(n, 0);
        pbdbind::top_k_cells<HostTraits<T> >(h_, src, k, mask.empty() ? NULL : &mask[0], n ? &dst[0] : NULL);
    }
    // the k best candidates by score, ties to the earlier one, in their input order, decided on the device (pbd_top_k): for a list
    // built elsewhere; every candidate is taken as one of this frame
    void topK(std::vector<Candidate> &candidates, int k)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "topK() before distributeModel()");
        std::vector<int32_t> rec = records(candidates);
        const std::vector<int32_t> in = rec;
        int n = (int)candidates.size();
        pbdbind::top_k<HostTraits<T> >(h_, k, rec, n);
        const size_t stride = (size_t)pbd_candidate_stride(h_);
        std::vector<Candidate> kept;
        for (size_t i = 0, j = 0; i < candidates.size() && j < (size_t)n; ++i)   // the kept records are the input's, in order
            if (std::memcmp(&in[i * stride], &rec[j * stride], stride * sizeof(int32_t)) == 0) {
                kept.push_back(candidates[i]);
                ++j;
            }
        candidates.swap(kept);
    }
    // new surface: a root's duplicates on neighbouring pyramid levels and components suppressed from now on (pbd_set_scale_nms):
    // of the roots the threshold, depth pruning and root NMS leave, only those are walked and returned that no better root within
    // dl levels of the same frame beats -- two roots being neighbours when the centre of one's rectangle lies inside the other's;
    // top-K is then taken among them.  dl in 0..255; on = false turns it off (the default).  Kept across distributeModel().
    void setScaleNMS(bool on, int dl = 1)
    {
        if (dl < 0 || dl > 255) throw Error(PBD_ERR_INVALID, "scale NMS: a level distance of 0..255");
        if (h_) pbdbind::set_scale_nms<HostTraits<T> >(h_, on, dl);
        scale_nms_on_ = on;
        scale_nms_dl_ = dl;
    }
    // the candidates no better neighbouring candidate within dl levels beats, in their input order, decided on the device
    // (pbd_scale_nms): for a list built elsewhere, e.g. the merged lists of level-sharded detectors; every candidate is taken as one
    // of this frame
    void scaleNMS(std::vector<Candidate> &candidates, int dl)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "scaleNMS() before distributeModel()");
        std::vector<int32_t> rec = records(candidates);
        const std::vector<int32_t> in = rec;
        int n = (int)candidates.size();
        pbdbind::scale_nms<HostTraits<T> >(h_, dl, rec, n);
        const size_t stride = (size_t)pbd_candidate_stride(h_);
        std::vector<Candidate> kept;
        for (size_t i = 0, j = 0; i < candidates.size() && j < (size_t)n; ++i)   // the kept records are the input's, in order
            if (std::memcmp(&in[i * stride], &rec[j * stride], stride * sizeof(int32_t)) == 0) {
                kept.push_back(candidates[i]);
                ++j;
            }
        candidates.swap(kept);
    }
    // new surface: detect(im, depth, candidates) runs filterCandidatesByDepth(depth, ., zfactor) on the unsuppressed list, before
    // the suppression -- the reference's commented-out call (src/PartsBasedDetector.cpp:91-93).  Off by default (depth ignored, as
    // in the reference); kept across distributeModel().
    void setDepthConsistency(bool on, float zfactor = 0.03f)
    {
        if (on && zfactor != zfactor) throw Error(PBD_ERR_INVALID, "zfactor is NaN");
        depth_on_ = on;
        zfactor_ = zfactor;
    }
    // new surface: the intent of the reference's commented-out ssp_.filterResponseByDepth (src/PartsBasedDetector.cpp:86-93) from
    // now on (pbd_set_depth_prune): detect(im, depth, candidates) walks and returns only the roots whose box width agrees with the
    // depth under it -- fx in pixels, width of the root footprint in depth units, relative tolerance tol.  Off by default; kept
    // across distributeModel().  With setDepthConsistency as well: prune at the roots, then the consistency filter, then the
    // suppression.
    void setDepthPrune(bool on, float fx = 0.f, float width = 0.f, float tol = 0.3f)
    {
        if (on && !(fx > 0 && fx <= FLT_MAX && width > 0 && width <= FLT_MAX && tol >= 0 && tol <= FLT_MAX))
            throw Error(PBD_ERR_INVALID, "depth prune: fx and width finite and > 0, tol finite and >= 0");
        if (h_) pbdbind::set_depth_prune<HostTraits<T> >(h_, on, fx, width, tol);
        prune_on_ = on; prune_fx_ = fx; prune_width_ = width; prune_tol_ = tol;
    }
    // pbd_bind_depth: the depth image (im's rows x cols) of the NEXT detect / detectBatch call of one frame; detect(im, depth, .)
    // calls it when setDepthPrune is on
    void bindDepth(const Image &depth)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "bindDepth() before distributeModel()");
        pbdbind::bind_depth<HostTraits<T> >(h_, depth);
    }
    // the candidates whose root box agrees with the depth under it, in order, decided on the device (pbd_depth_prune): for a list
    // built elsewhere; every candidate is taken as one of this frame
    void depthPrune(const Image &depth, std::vector<Candidate> &candidates, float fx, float width, float tol = 0.3f)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "depthPrune() before distributeModel()");
        std::vector<int32_t> rec = records(candidates);
        const std::vector<int32_t> in = rec;
        int n = (int)candidates.size();
        pbdbind::depth_prune<HostTraits<T> >(h_, depth, fx, width, tol, rec, n);
        const size_t stride = (size_t)pbd_candidate_stride(h_);
        std::vector<Candidate> kept;
        for (size_t i = 0, k = 0; i < candidates.size() && k < (size_t)n; ++i)   // the kept records are the input's, in order
            if (std::memcmp(&in[i * stride], &rec[k * stride], stride * sizeof(int32_t)) == 0) {
                kept.push_back(candidates[i]);
                ++k;
            }
        candidates.swap(kept);
    }
    void detect(const Image &im, std::vector<Candidate> &candidates) { detect(im, Image(), candidates); }
    // `depth` is ignored, as by the reference (src/PartsBasedDetector.cpp:91-93), unless it is not empty (the reference's `if
    // (!depth.empty())`) and setDepthPrune(true) and / or setDepthConsistency(true) ask for it
    void detect(const Image &im, const Image &depth, std::vector<Candidate> &candidates)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "detect() before distributeModel()");
        const bool has_depth = depth.data && depth.rows >= 1 && depth.cols >= 1;
        if (prune_on_ && has_depth) pbdbind::bind_depth<HostTraits<T> >(h_, depth);
        if (!depth_on_ || !has_depth) {
            pbdbind::detect<HostTraits<T> >(h_, im, candidates, 1 << 16);
            return;
        }
        if (nms_) pbdbind::set_nms<HostTraits<T> >(h_, false, overlap_);   // the filter reads the unsuppressed list
        try {
            pbdbind::detect_depth<HostTraits<T> >(h_, im, depth, zfactor_, nms_ ? overlap_ : -1.f, candidates, 1 << 18);
        } catch (...) {
            if (nms_) pbdbind::set_nms<HostTraits<T> >(h_, true, overlap_);
            throw;
        }
        if (nms_) pbdbind::set_nms<HostTraits<T> >(h_, true, overlap_);
    }
    // SearchSpacePruning<T>::filterCandidatesByDepth(parts, candidates, depth, zfactor) (src/SearchSpacePruning.cpp:73-95) on the
    // device (pbd_depth_consistency): the candidates whose parts agree in depth, in order.  `depth` is one channel of any accepted
    // depth, read in its own coordinates; every candidate is taken as one of this frame.
    void filterCandidatesByDepth(const Image &depth, std::vector<Candidate> &candidates, float zfactor = 0.03f)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "filterCandidatesByDepth() before distributeModel()");
        std::vector<int32_t> rec = records(candidates);
        const std::vector<int32_t> in = rec;
        int n = (int)candidates.size();
        pbdbind::depth_consistency<HostTraits<T> >(h_, depth, zfactor, rec, n);
        const size_t stride = (size_t)pbd_candidate_stride(h_);
        std::vector<Candidate> kept;
        for (size_t i = 0, k = 0; i < candidates.size() && k < (size_t)n; ++i)   // the kept records are the input's, in order
            if (std::memcmp(&in[i * stride], &rec[k * stride], stride * sizeof(int32_t)) == 0) {
                kept.push_back(candidates[i]);
                ++k;
            }
        candidates.swap(kept);
    }
    // Candidate::sort + Candidate::nonMaximaSuppression(im, candidates, overlap) on the device (pbd_suppress), for a list built
    // elsewhere (e.g. after filterCandidatesByDepth); every candidate is taken as one of this rows x cols frame
    void suppress(const Image &im, std::vector<Candidate> &candidates, float overlap)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "suppress() before distributeModel()");
        std::vector<int32_t> rec = records(candidates);
        int n = (int)candidates.size();
        pbdbind::suppress<HostTraits<T> >(h_, im.rows, im.cols, overlap, rec, n);
        candidates.clear();
        pbdbind::unpack_candidates<HostTraits<T> >(h_, rec, n, candidates);
    }
    // this handle's records of frame 0 for the candidates (the layout pbd_detect returns)
    std::vector<int32_t> records(const std::vector<Candidate> &candidates) const
    {
        const int stride = pbd_candidate_stride(h_);
        std::vector<int32_t> rec(candidates.size() * (size_t)stride + 1, 0);
        for (size_t i = 0; i < candidates.size(); ++i) {
            int32_t *r = &rec[i * stride];
            const Candidate &c = candidates[i];
            const float score = c.score();
            r[1] = c.component_; r[2] = c.level; r[3] = c.root_x; r[4] = c.root_y;
            std::memcpy(&r[5], &score, sizeof score);
            r[6] = (int32_t)c.parts_.size();
            for (size_t k = 0; k < c.parts_.size() && 8 + 4 * k + 3 < (size_t)stride; ++k) {
                r[8 + 4 * k] = c.parts_[k].x; r[9 + 4 * k] = c.parts_[k].y;
                r[10 + 4 * k] = c.parts_[k].width; r[11 + 4 * k] = c.parts_[k].height;
            }
        }
        return rec;
    }
    static Rect3d rect3d(const double *o)
    {
        Rect3d b;
        b.x = o[0]; b.y = o[1]; b.z = o[2]; b.height = o[3]; b.width = o[4]; b.depth = o[5];
        return b;
    }
    // Candidate::boundingBox3D(im, depth) of every candidate (include/Candidate.hpp:140-216), on the device (pbd_boxes3d): the
    // callers' next step after detect + suppression (cells/detect.cpp:224-255).  `im` gives the colour frame's size, `depth` is
    // one channel of any accepted depth and any size; every candidate is taken as one of this frame.
    void boundingBoxes3D(const Image &im, const Image &depth, const std::vector<Candidate> &candidates, std::vector<Rect3d> &boxes)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "boundingBoxes3D() before distributeModel()");
        if (depth.channels != 1) throw Error(PBD_ERR_INVALID, "the depth image has one channel");
        const std::vector<int32_t> rec = records(candidates);
        pbd_frame fr;
        fr.data = depth.data; fr.rows = depth.rows; fr.cols = depth.cols; fr.stride_bytes = depth.step;
        std::vector<double> out(candidates.size() * 6 + 1);
        pbdbind::check<HostTraits<T> >(h_, pbd_boxes3d(h_, 1, &fr, depth.depth, &im.rows, &im.cols, rec.data(), (int)candidates.size(), 0, out.data()));
        boxes.resize(candidates.size());
        for (size_t i = 0; i < candidates.size(); ++i) boxes[i] = rect3d(&out[6 * i]);
    }
    // PointCloudClusterer::computeBoundingBoxes(candidates, rgb, depth, projecter, ...) (include/PointCloudClusterer.hpp:53-153)
    // on the device (pbd_boxes3d_camera): every candidate's camera box and part centres.  `depth` is one 32F channel (the
    // reference reads depth.ptr<float>); parts_mode PBD_PARTS_LITERAL is the reference's sample loop.  A candidate whose cube holds
    // a NaN gets the zero box and no part centres, as the reference's `continue` leaves them; `dense` (optional) is each list's
    // is_dense.
    void computeBoundingBoxes(const Image &im, const Image &depth, const pbd_pinhole &camera, const std::vector<Candidate> &candidates,
                              std::vector<Rect3d> &boxes, std::vector<std::vector<Point3f> > &part_centres,
                              std::vector<bool> *dense = NULL, int parts_mode = PBD_PARTS_LITERAL)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "computeBoundingBoxes() before distributeModel()");
        if (depth.channels != 1) throw Error(PBD_ERR_INVALID, "the depth image has one channel");
        const std::vector<int32_t> rec = records(candidates);
        const size_t n = candidates.size();
        const int mp = (pbd_candidate_stride(h_) - 8) / 4;
        pbd_frame fr;
        fr.data = depth.data; fr.rows = depth.rows; fr.cols = depth.cols; fr.stride_bytes = depth.step;
        std::vector<double> box(n * 6 + 1);
        std::vector<float> cen(n * mp * 3 + 1);
        std::vector<int32_t> nc(n + 1), dn(n + 1);
        pbdbind::check<HostTraits<T> >(h_, pbd_boxes3d_camera(h_, 1, &fr, depth.depth, &im.rows, &im.cols, &camera, parts_mode, rec.data(),
                                                              (int)n, 0, box.data(), cen.data(), nc.data(), dn.data()));
        boxes.resize(n);
        part_centres.assign(n, std::vector<Point3f>());
        if (dense) dense->assign(n, true);
        for (size_t i = 0; i < n; ++i) {
            boxes[i] = rect3d(&box[6 * i]);
            for (int j = 0; j < nc[i]; ++j) {
                Point3f q;
                const float *c = &cen[(i * mp + j) * 3];
                q.x = c[0]; q.y = c[1]; q.z = c[2];
                part_centres[i].push_back(q);
            }
            if (dense) (*dense)[i] = dn[i] != 0;
        }
    }
    // Candidate::mask(im, candidates, mask) (include/Candidate.hpp:306-331) on the device (pbd_candidate_mask): mask receives
    // im.rows x im.cols uint8 labels (n+1 on the pixels of candidate n's boundingBox() no earlier candidate claimed, 255 from
    // n = 254 on); with `masked`, also the ROS node's rgb & (mask != 0) (ros/Messages.cpp:157-174) of the 8-bit im, interleaved
    // like im with dense rows
    void mask(const Image &im, const std::vector<Candidate> &candidates, std::vector<uint8_t> &mask, std::vector<uint8_t> *masked = NULL)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "mask() before distributeModel()");
        const std::vector<int32_t> rec = records(candidates);
        const size_t npix = (size_t)(im.rows > 0 ? im.rows : 0) * (size_t)(im.cols > 0 ? im.cols : 0);
        mask.assign(npix + 1, 0);
        if (masked) masked->assign(npix * (size_t)(im.channels > 0 ? im.channels : 0) + 1, 0);
        pbdbind::candidate_mask<HostTraits<T> >(h_, im, rec, (int)candidates.size(), &mask[0], (size_t)im.cols,
                                                masked ? &(*masked)[0] : NULL, (size_t)im.cols * im.channels);
        mask.resize(npix);
        if (masked) masked->resize(masked->size() - 1);
    }
    // messagePoses (ros/Messages.cpp:187-234) on the device (pbd_part_poses) for the part centres computeBoundingBoxes returns:
    // per candidate count (0: "Centroid not found", the node's `continue`), position (the centroid), orientation (x, y, z, w:
    // the eigen-frame of the centres' spread) and eigenvalues (ascending)
    void partPoses(const std::vector<std::vector<Point3f> > &part_centres, const std::vector<bool> &dense, std::vector<int32_t> &count,
                   std::vector<float> &position, std::vector<float> &orientation, std::vector<float> &eigenvalues)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "partPoses() before distributeModel()");
        const size_t n = part_centres.size(), mp = (size_t)(pbd_candidate_stride(h_) - 8) / 4;
        if (dense.size() != n) throw Error(PBD_ERR_INVALID, "one dense flag per candidate");
        std::vector<float> cen(n * mp * 3, 0.f);
        std::vector<int32_t> nc(n), dn(n);
        for (size_t i = 0; i < n; ++i) {
            if (part_centres[i].size() > mp) throw Error(PBD_ERR_INVALID, "more part centres than the model's parts");
            nc[i] = (int32_t)part_centres[i].size();
            dn[i] = dense[i] ? 1 : 0;
            for (size_t j = 0; j < part_centres[i].size(); ++j) {
                float *c = &cen[(i * mp + j) * 3];
                c[0] = part_centres[i][j].x; c[1] = part_centres[i][j].y; c[2] = part_centres[i][j].z;
            }
        }
        pbdbind::part_poses<HostTraits<T> >(h_, (int)n, cen, nc, dn, count, position, orientation, eigenvalues);
    }
    // the model vector w = [biasw | defw | filters] in T (pbd_model_vector): the parameter order of examples()
    std::vector<T> modelVector()
    {
        if (!h_) throw Error(PBD_ERR_STATE, "modelVector() before distributeModel()");
        std::vector<T> w((size_t)pbd_model_vector_len(h_) + 1);
        pbdbind::check<HostTraits<T> >(h_, pbd_model_vector(h_, &w[0]));
        w.resize(w.size() - 1);
        return w;
    }
    // the in-place model update (pbd_set_model_vector): the detector's parameters become w (modelVector()'s order); afterwards
    // it equals a detector given distributeModel() of the model with those parameters
    void setModelVector(const std::vector<T> &w)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "setModelVector() before distributeModel()");
        pbdbind::set_model_vector<HostTraits<T> >(h_, w);
    }
    // model.thresh for every later detect() (pbd_set_thresh)
    void setThreshold(float thresh)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "setThreshold() before distributeModel()");
        pbdbind::set_thresh<HostTraits<T> >(h_, thresh);
    }
    // training examples of candidates of the last detect() (pbd_examples, include/pbd.h): hdr receives hdr_words int32 per
    // candidate {index, component, nblocks, nvalues, (offset in modelVector(), length) x nblocks}, values `values` T per candidate
    // (the blocks' values in order); w . x is the candidate's score when its parts sit at the transform's arg-max
    void examples(const std::vector<Candidate> &candidates, std::vector<int32_t> &hdr, std::vector<T> &values, int &hdr_words,
                  int &nvalues)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "examples() before distributeModel()");
        pbdbind::check<HostTraits<T> >(h_, pbd_example_stride(h_, &hdr_words, &nvalues));
        const std::vector<int32_t> rec = records(candidates);
        const size_t n = candidates.size();
        hdr.assign(n * (size_t)hdr_words + 1, 0);
        values.assign(n * (size_t)nvalues + 1, T(0));
        pbdbind::check<HostTraits<T> >(h_, pbd_examples(h_, n ? &rec[0] : NULL, (int)n, 0, &hdr[0], &values[0]));
        hdr.resize(hdr.size() - 1);
        values.resize(values.size() - 1);
    }
    // the score of each part of candidates of the last detect() (pbd_part_scores, include/pbd.h): `scores`
    // receives every candidate's parts in candidate order (cell and mixture in the level's map; appearance, message, bias,
    // total), and every candidate what the reference's record declares and never fills (include/Candidate.hpp:54-72):
    // confidence_[p >= 1] = part p's appearance; confidence_[0] stays the score
    void partScores(std::vector<Candidate> &candidates, std::vector<PartScore> &scores)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "partScores() before distributeModel()");
        const std::vector<int32_t> rec = records(candidates);
        std::vector<int32_t> status;
        pbdbind::part_scores<HostTraits<T> >(h_, rec, (int)candidates.size(), std::vector<int>(), NULL, status, scores);
        size_t j = 0;
        for (size_t i = 0; i < candidates.size(); ++i) {
            const size_t np = status[i] > 0 ? (size_t)status[i] : 0;
            const float score = candidates[i].score();
            candidates[i].confidence_.assign(np, 0.f);
            for (size_t p = 0; p < np; ++p, ++j) candidates[i].confidence_[p] = p ? (float)scores[j].appearance : score;
        }
    }
    // the same four values at placements the caller gives (pbd_score_placements): place holds x, y, m of every candidate's parts
    // in candidate order (parts_.size() each, the root first), in the candidate's frame, level and component.  status[i] = the
    // candidate's parts, or -1 for a placement outside the level's map or a part's mixtures; `scores` receives the parts of the
    // candidates that have a status above 0
    void scorePlacements(const std::vector<Candidate> &candidates, const std::vector<PartScore> &place, std::vector<int32_t> &status,
                         std::vector<PartScore> &scores)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "scorePlacements() before distributeModel()");
        const std::vector<int32_t> rec = records(candidates);
        std::vector<int> nparts(candidates.size());
        for (size_t i = 0; i < candidates.size(); ++i) nparts[i] = (int)candidates[i].parts_.size();
        pbdbind::part_scores<HostTraits<T> >(h_, rec, (int)candidates.size(), nparts, &place, status, scores);
    }
    // the max-marginals of every part on frame `frame` of the last detect() / detectBatch() of images of im's size
    // (pbd_max_marginals, include/pbd.h): per level the planes of every (part, type) pair,
    // values[gm][y][x] = the score of the best configuration with that part of that type at (x, y).  They stay on the device for
    // marginalPoses() until the next detect call or model update
    void maxMarginals(const Image &im, std::vector<MarginalLevel> &levels, int frame = 0)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "maxMarginals() before distributeModel()");
        pbdbind::max_marginals<HostTraits<T> >(h_, frame, im.rows, im.cols, planes_, levels);
    }
    // the poses decoded from the max-marginals held (pbd_marginal_poses): seeds holds {level, component, part, type or -1 for the
    // best at the cell, x, y} per seed; status[i] = the pose's parts or -1 for a bad seed, `candidates` the good seeds' poses in
    // seed order, each scored with its seed's max-marginal
    void marginalPoses(const std::vector<int32_t> &seeds, std::vector<int32_t> &status, std::vector<Candidate> &candidates)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "marginalPoses() before distributeModel()");
        pbdbind::marginal_poses<HostTraits<T> >(h_, seeds, status, candidates);
    }
    // a training QP of `capacity` examples of this detector's model layout (pbd_qp_create; Cpos = C * wpos, Cneg = C)
    QP qp(int capacity, double C = 0.002, double wpos = 2.0)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "qp() before distributeModel()");
        return QP(pbdbind::qp_create<HostTraits<T> >(h_, capacity, C, wpos));
    }
    // PointCloudClusterer::clusterObjects(cloud, bounding_boxes, object_clusters, object_centers) (:157-293) on the device
    // (pbd_cluster_objects): clusters[i] = the point indices of box i's kept cluster, ascending (gather the points from the
    // cloud as ExtractIndices does); centres[i] its centroid, NaN without one.  `cloud`: x, y, z the first three floats of a point.
    void clusterObjects(const pbd_cloud &cloud, const std::vector<Rect3d> &boxes, std::vector<std::vector<int> > &clusters,
                        std::vector<Point3f> &centres)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "clusterObjects() before distributeModel()");
        const size_t n = boxes.size();
        std::vector<double> bx(n * 6 + 1);
        for (size_t i = 0; i < n; ++i) {
            double *o = &bx[6 * i];
            o[0] = boxes[i].x; o[1] = boxes[i].y; o[2] = boxes[i].z; o[3] = boxes[i].height; o[4] = boxes[i].width; o[5] = boxes[i].depth;
        }
        std::vector<int> frames(n + 1, 0);
        std::vector<float> cen(n * 3 + 1);
        std::vector<int32_t> cnt(n + 1);
        std::vector<int32_t> idx(1 << 16);
        int needed = 0;
        int rc = pbd_cluster_objects(h_, 1, &cloud, bx.data(), frames.data(), (int)n, cen.data(), cnt.data(), idx.data(), (int)idx.size(), &needed);
        if (rc == PBD_ERR_CAPACITY) {
            idx.resize((size_t)needed);
            rc = pbd_cluster_objects(h_, 1, &cloud, bx.data(), frames.data(), (int)n, cen.data(), cnt.data(), idx.data(), (int)idx.size(), &needed);
        }
        pbdbind::check<HostTraits<T> >(h_, rc);
        clusters.assign(n, std::vector<int>());
        centres.resize(n);
        size_t off = 0;
        for (size_t i = 0; i < n; ++i) {
            clusters[i].assign(idx.begin() + off, idx.begin() + off + cnt[i]);
            off += cnt[i];
            centres[i].x = cen[3 * i]; centres[i].y = cen[3 * i + 1]; centres[i].z = cen[3 * i + 2];
        }
    }
    // PointCloudClusterer::organizedMultiplaneSegmentation(cloud, cloud_no_plane) (:294-336) on the device (pbd_remove_planes):
    // cloud_no_plane = every point of no plane, NaN points included, as xyz triples in ascending index order (pass
    // reducedCloud(cloud_no_plane) to clusterObjects); kept[i] = its original index; labels = the plane index of every point or
    // -1; planes = {a, b, c, d} per plane; inliers = each plane's points.  `params` NULL: the reference's call.
    void organizedMultiplaneSegmentation(const pbd_cloud &cloud, std::vector<float> &cloud_no_plane, std::vector<int> &kept,
                                         std::vector<int> &labels, std::vector<std::array<float, 4> > &planes, std::vector<int> &inliers,
                                         const pbd_plane_params *params = NULL)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "organizedMultiplaneSegmentation() before distributeModel()");
        const size_t n = (size_t)std::max(cloud.rows, 0) * (size_t)std::max(cloud.cols, 0);
        std::vector<float> pts(n * 3 + 3);
        std::vector<int32_t> kp(n + 1), lab(n + 1);
        int32_t nkept = 0, nplanes = 0;
        int cap = 16, needed = 0;
        std::vector<float> pl;
        std::vector<int32_t> in;
        int rc = PBD_ERR_CAPACITY;
        for (int pass = 0; pass < 2 && rc == PBD_ERR_CAPACITY; ++pass) {
            if (pass) cap = needed;
            pl.assign((size_t)cap * 4 + 4, 0.f);
            in.assign((size_t)cap + 1, 0);
            rc = pbd_remove_planes(h_, 1, &cloud, params, pts.data(), kp.data(), &nkept, lab.data(), pl.data(), in.data(), &nplanes, cap,
                                   &needed);
        }
        pbdbind::check<HostTraits<T> >(h_, rc);
        cloud_no_plane.assign(pts.begin(), pts.begin() + (size_t)nkept * 3);
        kept.assign(kp.begin(), kp.begin() + nkept);
        labels.assign(lab.begin(), lab.begin() + n);
        planes.resize(nplanes);
        inliers.assign(in.begin(), in.begin() + nplanes);
        for (int k = 0; k < nplanes; ++k)
            for (int j = 0; j < 4; ++j) planes[k][j] = pl[4 * k + j];
    }
    // the unorganized pbd_cloud of organizedMultiplaneSegmentation's output
    static pbd_cloud reducedCloud(const std::vector<float> &cloud_no_plane)
    {
        pbd_cloud c;
        c.data = cloud_no_plane.data(); c.rows = 1; c.cols = (int)(cloud_no_plane.size() / 3);
        c.point_stride = 12; c.row_stride = cloud_no_plane.size() * sizeof(float);
        return c;
    }
    // new surface: images of any sizes (one depth, one channel count) in one call; candidates[i] = detect(images[i])
    // both forms of detectLatent
    void latent(bool device, const std::vector<pbd_frame> &frames, int channels, int depth, const std::vector<std::vector<int32_t> > &boxes,
                float overlap, const std::vector<std::vector<int32_t> > &mixtures, std::vector<Candidate> &candidates,
                std::vector<bool> &found)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "detectLatent() before distributeModel()");
        const size_t n = frames.size();
        if (n == 0 || boxes.size() != n || (!mixtures.empty() && mixtures.size() != n))
            throw Error(PBD_ERR_INVALID, "detectLatent: one box list (and mixture list) per image");
        const size_t np = boxes[0].size() / 4;
        std::vector<int32_t> bx, mx;
        for (size_t i = 0; i < n; ++i) {
            if (boxes[i].size() != 4 * np || (!mixtures.empty() && mixtures[i].size() != np))
                throw Error(PBD_ERR_INVALID, "detectLatent: four box values and one mixture per part");
            bx.insert(bx.end(), boxes[i].begin(), boxes[i].end());
            if (!mixtures.empty()) mx.insert(mx.end(), mixtures[i].begin(), mixtures[i].end());
        }
        const int stride = pbd_candidate_stride(h_);
        std::vector<int32_t> rec(n * (size_t)stride), fnd(n);
        bx.push_back(0);
        pbdbind::check<HostTraits<T> >(h_, (device ? pbd_detect_latent_device : pbd_detect_latent)(
                                               h_, (int)n, &frames[0], channels, depth, &bx[0], mx.empty() ? NULL : &mx[0], overlap,
                                               &rec[0], &fnd[0]));
        candidates.clear();
        pbdbind::unpack_candidates<HostTraits<T> >(h_, rec, (int)n, candidates);
        found.assign(n, false);
        for (size_t i = 0; i < n; ++i) found[i] = fnd[i] != 0;
    }
    void detectBatch(const std::vector<Image> &images, std::vector<std::vector<Candidate> > &candidates)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "detectBatch() before distributeModel()");
        pbdbind::detect_batch<HostTraits<T> >(h_, images, candidates, 1 << 18);
    }
    // latent positives (matlab/detection/detect.m with a bbox) on the device (pbd_detect_latent): per image the best candidate
    // whose part p overlaps boxes[i][p] = {x1, y1, x2, y2} (inclusive) by more than `overlap`; mixtures[i][p] >= 0 fixes part p's
    // mixture (empty: all free).  One candidate per image; found[i] = false when no placement passes.  One depth per call.
    void detectLatent(const std::vector<Image> &images, const std::vector<std::vector<int32_t> > &boxes, float overlap,
                      const std::vector<std::vector<int32_t> > &mixtures, std::vector<Candidate> &candidates, std::vector<bool> &found)
    {
        std::vector<pbd_frame> fr(images.size());
        for (size_t i = 0; i < images.size(); ++i) {
            fr[i].data = images[i].data; fr[i].rows = images[i].rows; fr[i].cols = images[i].cols; fr[i].stride_bytes = images[i].step;
        }
        latent(false, fr, images.empty() ? 3 : images[0].channels, images.empty() ? 0 : images[0].depth, boxes, overlap, mixtures,
               candidates, found);
    }
    // the same on frames already on the device (pbd_detect_latent_device): d_frames hold device pointers, regions of larger device
    // images included (read in place through their pitch); boxes, mixtures and the result stay on the host; synchronous
    void detectLatentDevice(const std::vector<pbd_frame> &d_frames, int channels, int depth,
                            const std::vector<std::vector<int32_t> > &boxes, float overlap,
                            const std::vector<std::vector<int32_t> > &mixtures, std::vector<Candidate> &candidates,
                            std::vector<bool> &found)
    {
        latent(true, d_frames, channels, depth, boxes, overlap, mixtures, candidates, found);
    }
    // ---- augmented positives (include/pbd.h "Augmented positives"): rotated and mirrored copies.
    // the size of the copy of a rows x cols frame turned by `degrees`, and the coefficients {cos, sin} the kernel uses
    static void augmentPlan(int rows, int cols, double degrees, int &out_rows, int &out_cols, double coef[2])
    {
        const int rc = pbd_augment_plan(rows, cols, degrees, &out_rows, &out_cols, coef);
        if (rc != PBD_OK) throw Error(rc, pbd_last_error(NULL));
    }
    // points {x, y, x, y ...} (0-based, real) of a rows x cols frame mapped into its copy (map_rotate_points.m 'ori2new' after the
    // mirror).  In a mirrored copy the caller gives part p the mapped point of part perm[p].
    static std::vector<double> augmentPoints(int rows, int cols, double degrees, bool mirror, const std::vector<double> &xy)
    {
        if (xy.size() % 2) throw Error(PBD_ERR_INVALID, "augmentPoints: two values per point {x, y}");
        std::vector<double> in(xy), out(xy.size() + 1, 0.0);
        in.push_back(0.0);
        const int rc = pbd_augment_points(rows, cols, degrees, mirror ? 1 : 0, (int)(xy.size() / 2), &in[0], &out[0]);
        if (rc != PBD_OK) throw Error(rc, pbd_last_error(NULL));
        out.resize(xy.size());
        return out;
    }
    // copy i = rotate(mirror(images[jobs[i].frame])) by jobs[i].degrees (counter-clockwise, nearest neighbour, zero outside), all
    // in one launch (pbd_augment_frames): out[i] views pixels[i], dense rows.  One depth and one channel count per call.
    void augmentFrames(const std::vector<Image> &images, const std::vector<pbd_augment> &jobs,
                       std::vector<std::vector<unsigned char> > &pixels, std::vector<Image> &out)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "augmentFrames() before distributeModel()");
        const size_t n = jobs.size(), nf = images.size();
        const int cn = nf ? images[0].channels : 3, depth = nf ? images[0].depth : 0;
        const size_t es = depth == 0 ? 1 : depth == 2 ? 2 : depth == 5 ? 4 : 8;
        std::vector<pbd_frame> fr(nf + 1), dst(n + 1);
        for (size_t i = 0; i < nf; ++i) {
            fr[i].data = images[i].data; fr[i].rows = images[i].rows; fr[i].cols = images[i].cols; fr[i].stride_bytes = images[i].step;
        }
        pixels.assign(n, std::vector<unsigned char>());
        out.assign(n, Image());
        for (size_t i = 0; i < n; ++i) {
            if (jobs[i].frame < 0 || (size_t)jobs[i].frame >= nf) throw Error(PBD_ERR_INVALID, "augmentFrames: a job names no image");
            double coef[2];
            augmentPlan(images[jobs[i].frame].rows, images[jobs[i].frame].cols, jobs[i].degrees, out[i].rows, out[i].cols, coef);
            out[i].channels = cn; out[i].depth = depth; out[i].step = (size_t)out[i].cols * cn * es;
            pixels[i].assign(out[i].step * out[i].rows, 0);
            out[i].data = &pixels[i][0];
            dst[i].data = out[i].data; dst[i].rows = out[i].rows; dst[i].cols = out[i].cols; dst[i].stride_bytes = out[i].step;
        }
        std::vector<pbd_augment> jb(jobs);
        jb.push_back(pbd_augment());
        pbdbind::check<HostTraits<T> >(h_, pbd_augment_frames(h_, (int)nf, &fr[0], cn, depth, (int)n, &jb[0], &dst[0]));
    }
    // ---- testing a model on the device (include/pbd.h "Testing a model"): matlab/detection/nms.m, bestoverlap.m and
    // matlab/evaluation/eval_pck.m, eval_apk.m + VOCap.m.  Candidates carry their frame in `frame` (0 .. nframes-1).
    // records() with every candidate's own frame
    std::vector<int32_t> frameRecords(const std::vector<Candidate> &candidates) const
    {
        std::vector<int32_t> rec = records(candidates);
        const size_t stride = (size_t)pbd_candidate_stride(h_);
        for (size_t i = 0; i < candidates.size(); ++i) rec[i * stride] = candidates[i].frame;
        return rec;
    }
    // nms.m per frame (pbd_part_nms): candidates grouped by ascending frame; the kept ones, frame by frame, in pick order
    std::vector<Candidate> partNMS(const std::vector<Candidate> &candidates, int nframes, float overlap = 0.3f, int max_boxes = 1000)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "partNMS() before distributeModel()");
        std::vector<int32_t> rec = frameRecords(candidates);
        int n = 0;
        pbdbind::check<HostTraits<T> >(h_, pbd_part_nms(h_, nframes, overlap, max_boxes, &rec[0], (int)candidates.size(), 0, &rec[0],
                                                        (int)candidates.size(), &n));
        std::vector<Candidate> kept;
        pbdbind::unpack_candidates<HostTraits<T> >(h_, rec, n, kept);
        return kept;
    }
    // bestoverlap.m per frame (pbd_best_overlap): gtboxes holds {x1, y1, x2, y2} per frame (a NaN: no ground truth); best[f] is
    // frame f's highest-scoring candidate whose part-centre hull covers more than `overlap` of the box, where found[f]
    void bestOverlap(const std::vector<Candidate> &candidates, const std::vector<double> &gtboxes, float overlap,
                     std::vector<Candidate> &best, std::vector<bool> &found)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "bestOverlap() before distributeModel()");
        const size_t n = gtboxes.size() / 4;
        if (n == 0 || gtboxes.size() != 4 * n) throw Error(PBD_ERR_INVALID, "bestOverlap: four ground-truth values per frame");
        std::vector<int32_t> rec = frameRecords(candidates);
        std::vector<int32_t> out(n * (size_t)pbd_candidate_stride(h_)), fnd(n);
        pbdbind::check<HostTraits<T> >(h_, pbd_best_overlap(h_, (int)n, &gtboxes[0], overlap, &rec[0], (int)candidates.size(), 0, &out[0],
                                                            &fnd[0]));
        best.clear();
        pbdbind::unpack_candidates<HostTraits<T> >(h_, out, (int)n, best);
        found.assign(n, false);
        for (size_t i = 0; i < n; ++i) found[i] = fnd[i] != 0;
    }
    // eval_pck.m (pbd_eval_pck) on bestOverlap's output: gt_points = [frame][part][2], scale = [frame]; pck per part and, when
    // asked for, dist = [part][frame]
    std::vector<double> evalPCK(const std::vector<Candidate> &best, const std::vector<bool> &found, const std::vector<double> &gt_points,
                                const std::vector<double> &scale, double thresh = 0.5, std::vector<double> *dist = NULL)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "evalPCK() before distributeModel()");
        const size_t n = best.size(), np = (size_t)(pbd_candidate_stride(h_) - 8) / 4;
        if (n == 0 || found.size() != n || scale.size() != n || gt_points.size() != n * np * 2)
            throw Error(PBD_ERR_INVALID, "evalPCK: one candidate, flag and scale per frame, two values per part of a frame");
        std::vector<int32_t> rec = frameRecords(best), fnd(n);
        for (size_t i = 0; i < n; ++i) fnd[i] = found[i] ? 1 : 0;
        std::vector<double> pck(np);
        if (dist) dist->assign(np * n, 0.0);
        pbdbind::check<HostTraits<T> >(h_, pbd_eval_pck(h_, (int)n, &rec[0], &fnd[0], &gt_points[0], &scale[0], thresh, &pck[0],
                                                        dist ? &(*dist)[0] : NULL));
        return pck;
    }
    // eval_apk.m + VOCap.m (pbd_eval_apk) for every part: frame f's instances are gt_offset[f] .. gt_offset[f + 1] - 1 of
    // gt_points = [instance][part][2] and gt_scale = [instance]; apk per part and, when asked for, prec / rec = [part][candidate]
    std::vector<double> evalAPK(const std::vector<Candidate> &candidates, const std::vector<int32_t> &gt_offset,
                                const std::vector<double> &gt_points, const std::vector<double> &gt_scale, double thresh = 0.5,
                                std::vector<double> *prec = NULL, std::vector<double> *rec = NULL)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "evalAPK() before distributeModel()");
        const size_t n = candidates.size(), np = (size_t)(pbd_candidate_stride(h_) - 8) / 4;
        if (gt_offset.size() < 2 || gt_offset.back() < 0 || gt_scale.size() != (size_t)gt_offset.back() ||
            gt_points.size() != gt_scale.size() * np * 2)
            throw Error(PBD_ERR_INVALID, "evalAPK: gt_offset has nframes + 1 entries, the last one counts the instances");
        std::vector<int32_t> records_ = frameRecords(candidates);
        std::vector<double> apk(np), none(1);
        if (prec) prec->assign(np * n + 1, 0.0);
        if (rec) rec->assign(np * n + 1, 0.0);
        pbdbind::check<HostTraits<T> >(h_, pbd_eval_apk(h_, (int)gt_offset.size() - 1, &gt_offset[0], gt_points.empty() ? &none[0] : &gt_points[0],
                                                        gt_scale.empty() ? &none[0] : &gt_scale[0], thresh, &records_[0], (int)n, 0, &apk[0],
                                                        prec ? &(*prec)[0] : NULL, rec ? &(*rec)[0] : NULL));
        if (prec) prec->resize(np * n);
        if (rec) rec->resize(np * n);
        return apk;
    }
    // new surface: clusterparts.m + k_means.m and buildmodel.m's anchors on the device (pbd_cluster_parts): the part types of a
    // flexible-mixtures model by `trials` k-means restarts per part.  def = [part][positive][2] (data_def.m), parent = 0-based
    // parents (root -1, parent < child), K = types per part (1..16).  The detector's model is not read.  trainmodel.m's pipeline
    // around it is Python's (partsbaseddetector_amd/trainmodel.py), as train.m's is.
    PartClusters clusterParts(const std::vector<double> &def, const std::vector<int32_t> &parent, const std::vector<int32_t> &K,
                              int trials = 100, int max_iter = 1000, uint64_t seed = 0)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "clusterParts() before distributeModel()");
        const size_t np = parent.size();
        if (np < 2 || K.size() != np || def.empty() || def.size() % (2 * np) || trials < 1)
            throw Error(PBD_ERR_INVALID, "clusterParts: def holds two values per part and positive, parent and K one per part");
        const size_t n = def.size() / (2 * np);
        PartClusters out;
        out.idx.assign(np * n, 0); out.centres.assign(np * 32, 0.0); out.counts.assign(np * 16, 0); out.anchors.assign(np * 32, 0);
        out.info.resize(np); out.sumdist_all.assign(np * (size_t)trials, 0.0); out.iters_all.assign(np * (size_t)trials, 0);
        pbdbind::check<HostTraits<T> >(h_, pbd_cluster_parts(h_, (int)np, (int)n, &def[0], &parent[0], &K[0], trials, max_iter, seed,
                                                             &out.idx[0], &out.centres[0], &out.counts[0], &out.anchors[0],
                                                             &out.info[0], &out.sumdist_all[0], &out.iters_all[0]));
        return out;
    }
    // warped positives (matlab/learning/train.m poswarp, warppos.m, qp_poswrite) on the device (pbd_warp_positives): boxes holds
    // five values per box, {image, x1, y1, x2, y2} (0-based, inclusive); each box is padded by one cell, cropped with edge
    // replication, resized to (k + 2) * sbin pixels and its HOG written as the example [bias = 1 | filter block] of filter
    // `filter` (bias -1: the filter block alone) in examples()' format.  kept[i] = false: skipped as smaller than the filter's
    // pixels (skipSmall), its header marked invalid (hdr[2] = -1).  One depth and one channel count per call.
    void warpPositives(const std::vector<Image> &images, const std::vector<int32_t> &boxes, int filter, int bias, bool skipSmall,
                       std::vector<int32_t> &hdr, std::vector<T> &values, std::vector<bool> &kept, int &hdr_words, int &nvalues)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "warpPositives() before distributeModel()");
        if (boxes.size() % 5) throw Error(PBD_ERR_INVALID, "warpPositives: five values per box {image, x1, y1, x2, y2}");
        pbdbind::check<HostTraits<T> >(h_, pbd_example_stride(h_, &hdr_words, &nvalues));
        const size_t n = boxes.size() / 5, nf = images.size();
        std::vector<pbd_frame> fr(nf + 1);
        for (size_t i = 0; i < nf; ++i) {
            fr[i].data = images[i].data; fr[i].rows = images[i].rows; fr[i].cols = images[i].cols; fr[i].stride_bytes = images[i].step;
        }
        hdr.assign(n * (size_t)hdr_words + 1, 0);
        values.assign(n * (size_t)nvalues + 1, T(0));
        std::vector<int32_t> kp(n + 1, 0), bx(boxes);
        bx.push_back(0);
        pbdbind::check<HostTraits<T> >(h_, pbd_warp_positives(h_, (int)nf, &fr[0], nf ? images[0].channels : 3, nf ? images[0].depth : 0,
                                                              (int)n, &bx[0], filter, bias, skipSmall ? 1 : 0, &hdr[0], &values[0], &kp[0]));
        hdr.resize(hdr.size() - 1);
        values.resize(values.size() - 1);
        kept.assign(n, false);
        for (size_t i = 0; i < n; ++i) kept[i] = kp[i] != 0;
    }
    // the device form (pbd_warp_positives_device): d_frames are device frames (a region of a larger image is read in place
    // through its pitch), the examples and the payload (word 0 = boxes, record i = {idOffset + i, 0 ...}) stay on the device for
    // QP::addDevice / pbd_qp_add_device; asynchronous on the detector's stream
    void warpPositivesDevice(const std::vector<pbd_frame> &d_frames, int channels, int depth, const std::vector<int32_t> &boxes,
                             int filter, int bias, bool skipSmall, int idOffset, int32_t *d_payload, int capacity, int32_t *d_hdr,
                             T *d_values)
    {
        if (!h_) throw Error(PBD_ERR_STATE, "warpPositivesDevice() before distributeModel()");
        if (boxes.size() % 5) throw Error(PBD_ERR_INVALID, "warpPositivesDevice: five values per box {frame, x1, y1, x2, y2}");
        std::vector<pbd_frame> fr(d_frames);
        fr.push_back(pbd_frame());
        std::vector<int32_t> bx(boxes);
        bx.push_back(0);
        pbdbind::check<HostTraits<T> >(h_, pbd_warp_positives_device(h_, (int)d_frames.size(), &fr[0], channels, depth,
                                                                     (int)(boxes.size() / 5), &bx[0], filter, bias, skipSmall ? 1 : 0,
                                                                     idOffset, d_payload, capacity, d_hdr, d_values));
    }
};

// A stream of single frames over K handles (K HIP streams + workspaces) of one GPU, fed round-robin -- new surface: the
// reference's callers run detect(im) one frame at a time (cells/detect.cpp:213, ros/Node.cpp:144), and one frame's kernels do
// not fill an MI355X; frames on different handles overlap at kernel granularity (one 640x480 frame: 423 -> 525 frames/s with
// four handles, measured by bench.py through the same scheme in Python, detector.DetectorPool; `pbd_demo --stream` prints this
// class's own rate).  Results come back in submission order and are those of detect() on one handle.
//     FrameStream<float> fs(model, 4);
//     for (;;) { while (fs.full()) { fs.next(cands); use(cands); }   fs.submit(frame); }
//     while (fs.pending()) { fs.next(cands); use(cands); }
// Frames are 8-bit (pbd_detect_batch_submit); a submitted frame's pixels are copied before submit() returns.
// A next() that throws (PBD_ERR_CAPACITY: the frame held more candidates than `capacity`) has consumed its frame: `candidates`
// is left empty, and the following next() returns the following frame's list, from the next handle.  Only the "nothing
// submitted" refusal consumes nothing.
template <typename T>
class FrameStream {
    std::vector<pbd_handle *> h_;
    size_t submitted_, collected_;
    int capacity_;
    std::vector<int32_t> buf_;       // next()'s record buffer, kept between calls
    FrameStream(const FrameStream &);
    FrameStream &operator=(const FrameStream &);
public:
    // conv_mode: the convolution of every handle (PBD_CONV_*, include/pbd.h)
    FrameStream(Model &model, int nhandles = 4, int device = 0, int capacity = 1 << 16, int conv_mode = PBD_CONV_EXACT)
        : submitted_(0), collected_(0), capacity_(capacity)
    {
        if (nhandles < 1) throw Error(PBD_ERR_INVALID, "FrameStream needs at least one handle");
        try {
            for (int i = 0; i < nhandles; ++i) h_.push_back(pbdbind::create<HostTraits<T> >(model, device, conv_mode, 1, capacity));
        } catch (...) {      // a later handle failed (out of memory): the earlier ones must not leak
            for (size_t i = 0; i < h_.size(); ++i) pbd_destroy(h_[i]);
            throw;
        }
    }
    ~FrameStream() { for (size_t i = 0; i < h_.size(); ++i) pbd_destroy(h_[i]); }
    // every handle returns sorted, suppressed lists (PartsBasedDetector::setNonMaximaSuppression); nothing may be pending
    void setNonMaximaSuppression(float overlap)
    {
        for (size_t i = 0; i < h_.size(); ++i) pbdbind::set_nms<HostTraits<T> >(h_[i], overlap >= 0, overlap);
    }
    // every handle keeps only the grid maxima of its root scores (PartsBasedDetector::setRootNMS); nothing may be pending
    void setRootNMS(int sz)
    {
        for (size_t i = 0; i < h_.size(); ++i) pbdbind::set_root_nms<HostTraits<T> >(h_[i], sz);
    }
    // every handle detects on the padded pyramid (PartsBasedDetector::setPadding); nothing may be pending
    void setPadding(int padx, int pady)
    {
        for (size_t i = 0; i < h_.size(); ++i) pbdbind::set_padding<HostTraits<T> >(h_[i], padx, pady);
    }
    // every handle searches the fine octave (PartsBasedDetector::setFineOctave); nothing may be pending
    void setFineOctave(bool on)
    {
        for (size_t i = 0; i < h_.size(); ++i) pbdbind::set_fine_octave<HostTraits<T> >(h_[i], on);
    }
    // every handle keeps at most k candidates per frame (PartsBasedDetector::setTopK); nothing may be pending
    void setTopK(int k)
    {
        for (size_t i = 0; i < h_.size(); ++i) pbdbind::set_top_k<HostTraits<T> >(h_[i], k);
    }
    // every handle suppresses a root's duplicates on neighbouring levels (PartsBasedDetector::setScaleNMS); nothing may be pending
    void setScaleNMS(bool on, int dl = 1)
    {
        for (size_t i = 0; i < h_.size(); ++i) pbdbind::set_scale_nms<HostTraits<T> >(h_[i], on, dl);
    }
    // every handle prunes the roots of a frame submitted with its depth image (PartsBasedDetector::setDepthPrune); nothing may be
    // pending
    void setDepthPrune(bool on, float fx = 0.f, float width = 0.f, float tol = 0.3f)
    {
        for (size_t i = 0; i < h_.size(); ++i) pbdbind::set_depth_prune<HostTraits<T> >(h_[i], on, fx, width, tol);
    }
    size_t pending() const { return submitted_ - collected_; }
    bool full() const { return pending() >= h_.size(); }        // the handle the next frame would go to still holds a result
    // the frame with its depth image (one channel, the frame's size; copied before submit() returns), for setDepthPrune
    void submit(const Image &im, const Image &depth)
    {
        if (full()) throw Error(PBD_ERR_STATE, "FrameStream::submit(): every handle holds an uncollected frame; call next() first");
        if (depth.data && depth.rows >= 1 && depth.cols >= 1) pbdbind::bind_depth<HostTraits<T> >(h_[submitted_ % h_.size()], depth);
        submit(im);
    }
    void submit(const Image &im)
    {
        if (full()) throw Error(PBD_ERR_STATE, "FrameStream::submit(): every handle holds an uncollected frame; call next() first");
        if (im.depth != 0) throw Error(PBD_ERR_UNSUPPORTED, "FrameStream takes 8-bit frames");
        pbd_handle *h = h_[submitted_ % h_.size()];
        const void *img = im.data;
        pbdbind::check<HostTraits<T> >(h, pbd_detect_batch_submit(h, 1, &img, im.rows, im.cols, im.channels, im.step));
        ++submitted_;
    }
    void next(std::vector<Candidate> &candidates)
    {   // the oldest submitted frame's candidates
        if (!pending()) throw Error(PBD_ERR_STATE, "FrameStream::next(): nothing submitted");
        pbd_handle *h = h_[collected_ % h_.size()];
        buf_.resize((size_t)capacity_ * pbd_candidate_stride(h) + 1);      // sized once: every handle has the model's stride
        int n = 0;
        const int rc = pbd_detect_batch_wait(h, &buf_[0], capacity_, &n);
        ++collected_;        // the wait has released the handle's slot, failed or not: the next call takes the next handle
        candidates.clear();
        pbdbind::check<HostTraits<T> >(h, rc);
        pbdbind::unpack_candidates<HostTraits<T> >(h, buf_, n, candidates);
    }
};

// grey PFM ("Pf", a float depth map): rows stored bottom to top, little-endian for a negative scale; returned as 32F (depth 5),
// top row first, in native byte order
inline bool readPFM(const std::string &path, std::vector<uint8_t> &pix, Image &im)
{
    std::ifstream in(path.c_str(), std::ios::binary);
    std::string magic;
    int w = 0, h = 0;
    double scale = 0;
    if (!(in >> magic >> w >> h >> scale) || magic != "Pf" || w < 1 || h < 1 || scale == 0) return false;
    in.get();
    const size_t row = (size_t)w * 4;
    std::vector<uint8_t> raw(row * h);
    in.read(reinterpret_cast<char *>(raw.data()), (std::streamsize)raw.size());
    if (!in) return false;
    pix.resize(raw.size());
    const uint16_t one = 1;
    const bool little = *reinterpret_cast<const uint8_t *>(&one) == 1;
    for (int r = 0; r < h; ++r)
        for (size_t k = 0; k < row; k += 4)
            for (int b = 0; b < 4; ++b)
                pix[r * row + k + b] = raw[(size_t)(h - 1 - r) * row + k + ((scale < 0) == little ? b : 3 - b)];
    im.data = pix.data(); im.rows = h; im.cols = w; im.channels = 1; im.step = row; im.depth = 5;
    return true;
}

// binary PGM (P5) / PPM (P6, stored RGB -> returned BGR as cv::imread does); a PGM of maxval 65535 (big-endian samples, a
// depth map) is returned as 16U (depth 2) in native byte order
inline bool readPNM(const std::string &path, std::vector<uint8_t> &pix, Image &im)
{
    std::ifstream in(path.c_str(), std::ios::binary);
    std::string magic;
    int w = 0, h = 0, maxv = 0;
    if (!(in >> magic >> w >> h >> maxv) || (magic != "P5" && magic != "P6")) return false;
    const bool wide = magic == "P5" && maxv == 65535;
    if (maxv != 255 && !wide) return false;
    in.get();
    const int cn = magic == "P6" ? 3 : 1;
    const size_t es = wide ? 2 : 1;
    pix.resize((size_t)w * h * cn * es);
    in.read(reinterpret_cast<char *>(pix.data()), (std::streamsize)pix.size());
    if (!in) return false;
    if (cn == 3) for (size_t i = 0; i < pix.size(); i += 3) std::swap(pix[i], pix[i + 2]);
    if (wide)
        for (size_t i = 0; i < pix.size(); i += 2) {
            const uint16_t v = (uint16_t)(pix[i] << 8 | pix[i + 1]);
            std::memcpy(&pix[i], &v, 2);
        }
    im.data = pix.data(); im.rows = h; im.cols = w; im.channels = cn; im.step = (size_t)w * cn * es; im.depth = wide ? 2 : 0;
    return true;
}

}  // namespace pbdhost
