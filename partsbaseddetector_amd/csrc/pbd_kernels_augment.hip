// pbd_kernels_augment.hip -- augmented positives (pbd_augment_frames*): rotated and mirrored copies of training frames, the step
// the reference's training pipeline assumes (matlab/globals.m:18-23 imrotate/ and imflip/ caches, matlab/learning/
// map_rotate_points.m, train.m:130,165).  include/pbd.h states the contract, DESIGN.md section 6r the rule and the design; the
// numpy yardstick is partsbaseddetector_amd/augment.py (rotate_ref), matched byte for byte.  Compiled with -ffp-contract=off, as
// every file that resamples.
//
//   k_augment    one workgroup per tile of kAugTileCols x kAugTileRows destination pixels of one job, one thread per destination
//                column of the tile: consecutive lanes write consecutive pixels of a destination row.  The pixel's source
//                position is the inverse map of map_rotate_points.m:42 in double, every product rounded (__dmul_rn) and the sums
//                taken left to right (__dadd_rn), the index floor(x + 0.5); the products of the column coordinate are the same in
//                every row of the tile and computed once.  A pixel is moved as cn elements of the depth's size, as unsigned
//                integers: no byte of it is interpreted.  Outside the source every byte of the pixel is 0.
// No atomics, no LDS, and no kernel reads what another workgroup of the same launch writes (a destination that overlaps a source
// is refused by the entry layer).
#include "pbd_internal.h"

namespace pbd {
namespace {

template <typename PT>
__global__ __launch_bounds__(kAugTileCols) void k_augment(AugParams p)
{
    const AugTile t = p.tiles[blockIdx.x];
    const AugJob j = p.jobs[t.job];
    const int Q = t.x0 + (int)threadIdx.x;
    if (Q >= j.dcols) return;
    const int cn = p.cn;
    const int y1 = t.y0 + kAugTileRows < j.drows ? t.y0 + kAugTileRows : j.drows;
    double vs = 0, vc = 0;
    if (j.rotate) {
        const double v = (double)Q - j.hBc;
        vs = __dmul_rn(v, j.s);
        vc = __dmul_rn(v, j.c);
    }
    for (int R = t.y0; R < y1; ++R) {
        int r = R, q = Q;
        bool inside = true;
        if (j.rotate) {
            const double u = (double)R - j.hBr;
            const double fr = floor(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(u, j.c), vs), j.hAr), 0.5));
            const double fq = floor(__dadd_rn(__dadd_rn(__dadd_rn(-__dmul_rn(u, j.s), vc), j.hAc), 0.5));
            inside = fr >= 0 && fr < (double)j.srows && fq >= 0 && fq < (double)j.scols;
            r = inside ? (int)fr : 0;
            q = inside ? (int)fq : 0;
        }
        PT *d = reinterpret_cast<PT *>(j.dst + (size_t)R * j.dpitch) + (size_t)Q * cn;
        if (inside) {
            if (j.mirror) q = j.scols - 1 - q;
            const PT *s = reinterpret_cast<const PT *>(j.src + (size_t)r * j.spitch) + (size_t)q * cn;
            for (int c = 0; c < cn; ++c) d[c] = s[c];
        } else {
            for (int c = 0; c < cn; ++c) d[c] = (PT)0;
        }
    }
}

}  // namespace

void launch_augment(const AugParams &p, hipStream_t s)
{
    if (p.ntiles == 0) return;
    const dim3 grid((unsigned)p.ntiles), block(kAugTileCols);
    switch (depth_size(p.depth)) {
    case 1: PBD_LAUNCH(k_augment<uint8_t>, grid, block, 0, s, p); break;
    case 2: PBD_LAUNCH(k_augment<uint16_t>, grid, block, 0, s, p); break;
    case 4: PBD_LAUNCH(k_augment<uint32_t>, grid, block, 0, s, p); break;
    default: PBD_LAUNCH(k_augment<uint64_t>, grid, block, 0, s, p); break;
    }
}

}  // namespace pbd
