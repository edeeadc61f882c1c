// Test program of tests/test_host_stream.py: PPM frames through pbdhost::FrameStream<float> in the loop of the class comment
// (include/pbd_host.hpp), one report per frame in submission order.
//   host_stream_check model.yml HANDLES CAPACITY frame0.ppm [frame1.ppm ...]
// Per frame i:  "frame i" followed by its candidates after Candidate::sort, one per line in pbd_demo's format
//   cand LEVEL COMPONENT ROOT_Y ROOT_X SCORE X,Y,W,H ...
// or, when next() threw a pbdhost::Error, "frame i" followed by "error CODE".  Every frame is read into the SAME pixel buffer,
// which the next frame overwrites: submit() has to have copied the pixels.  Exit status 0 when every frame was reported.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pbd_host.hpp"

using namespace pbdhost;

static size_t g_reported = 0, g_frames = 0;

static void report_next(FrameStream<float> &fs)
{
    std::vector<Candidate> candidates;
    // a stream that does not move on after a failed next() would be asked for ever: every frame is reported once
    if (g_reported >= g_frames) throw Error(PBD_ERR_STATE, "the stream still reports pending frames after every frame was collected");
    std::printf("frame %zu\n", g_reported++);
    try {
        fs.next(candidates);
    } catch (const Error &e) {
        std::printf("error %d\n", e.code);
        return;
    }
    Candidate::sort(candidates);
    for (size_t i = 0; i < candidates.size(); ++i) {
        const Candidate &c = candidates[i];
        std::printf("cand %d %d %d %d %.9g", c.level, c.component(), c.root_y, c.root_x, (double)c.score());
        for (size_t p = 0; p < c.parts().size(); ++p)
            std::printf(" %d,%d,%d,%d", c.parts()[p].x, c.parts()[p].y, c.parts()[p].width, c.parts()[p].height);
        std::printf("\n");
    }
}

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "Usage: host_stream_check model_file handles capacity frame.ppm...\n");
        return 1;
    }
    g_frames = (size_t)(argc - 4);
    try {
        FileStorageModel model;
        if (!model.deserialize(argv[1])) { std::fprintf(stderr, "Error deserializing file\n"); return 1; }
        const int handles = std::atoi(argv[2]), capacity = std::atoi(argv[3]);
        FrameStream<float> fs(model, handles, 0, capacity);
        std::vector<uint8_t> pix;
        for (int i = 4; i < argc; ++i) {
            while (fs.full()) report_next(fs);
            Image im;
            if (!readPNM(argv[i], pix, im)) { std::fprintf(stderr, "Image not found, or invalid image format: %s\n", argv[i]); return 1; }
            fs.submit(im);
        }
        while (fs.pending()) report_next(fs);
    } catch (const Error &e) {
        std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
        return 2;
    }
    return g_reported == (size_t)(argc - 4) ? 0 : 3;
}
