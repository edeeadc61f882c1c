// Test double (declarations only) of the members of the reference's Candidate (include/Candidate.hpp:56-80) that
// include/pbd_opencv_adapters.hpp calls, the accessors its depth-consistency and suppression wrappers read included.
// tests/test_adapters_depth_compile.py puts this directory before tests/adapter_doubles.
#ifndef PBD_TEST_DOUBLE_CANDIDATE_HPP_
#define PBD_TEST_DOUBLE_CANDIDATE_HPP_
#include <vector>
#include <opencv2/core/core.hpp>
class Candidate {
public:
    Candidate();
    virtual ~Candidate();
    void addPart(cv::Rect r, float confidence);
    void setComponent(int c);
    const std::vector<cv::Rect> &parts(void) const;
    float score(void) const;
    int component(void);
};
#endif
