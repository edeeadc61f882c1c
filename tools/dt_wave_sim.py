#!/usr/bin/env python3
"""CPU replay of the distance transform's ring service for a whole wave (the kernel's lock step of 64 adjacent lines): how often
the WAVE runs the spill and reload paths per element under a service policy.  tools/dt_ring_sim.py counts one lane; here the
64 lanes share every pass through a path (tests/dt_wave_replay.py is the replay, and checks every line against computeRow).

Inputs, as for tools/dt_ring_sim.py: the oracle's raw responses of the synthetic person model at levels 0, 3 and 6 of a 640x480
frame (rows pass, then the columns pass on its output), and the accumulated scores of the parts whose children are all leaves
(response + the children's transformed scores, best mixture each, biases left out: they shift whole planes).

    python tools/dt_wave_sim.py [--filters 4]        -> the table of profiles/dt_ring_service/README.md"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import dt_wave_replay as W                                   # noqa: E402
from oracle import oracle                                    # noqa: E402
from partsbaseddetector_amd import model as M, synth         # noqa: E402

POLICIES = [("lane by lane (spill when full, reload in pop)", W.LANE_BY_LANE),
            ("whole wave 6 / 2 / 6 (shipped)", dict(high=6, low=2, low_ro=6)),
            ("whole wave 6 / 2 / 2 (read-out as forward)", dict(high=6, low=2, low_ro=2)),
            ("whole wave 7 / 2 / 6", dict(high=7, low=2, low_ro=6)),
            ("whole wave 5 / 2 / 6", dict(high=5, low=2, low_ro=6)),
            ("whole wave 4 / 2 / 6 (thrashes)", dict(high=4, low=2, low_ro=6)),
            ("whole wave 6 / 4 / 6", dict(high=6, low=4, low_ro=6)),
            ("spill service only 6 / - / -", dict(high=6, low=-1, low_ro=-1)),
            ("reload service only 9 / 2 / 6", dict(high=9, low=2, low_ro=6))]


def jobs_of(flat, resp):
    """(label, plane, ax, bx, ay, by, osx, osy): leaf parts' raw planes and one-level accumulated planes of their parents."""
    c = 0
    p0, p1 = int(flat.part_offset[c]), int(flat.part_offset[c + 1])
    children = {g: [h for h in range(p0 + 1, p1) if p0 + int(flat.parentid[h]) == g] for g in range(p0, p1)}

    def quad(gm):
        w = flat.defw[int(flat.defid[gm])]
        an = flat.anchors[int(flat.defid[gm])]
        return float(-w[0]), float(-w[1]), float(-w[2]), float(-w[3]), int(an[0]), int(an[1])

    out = []
    for g in range(p0 + 1, p1):
        mixes = range(int(flat.mix_offset[g]), int(flat.mix_offset[g + 1]))
        if not children[g]:
            out += [("leaf", resp[int(flat.filterid[gm])]) + quad(gm) for gm in mixes]
        elif all(not children[h] for h in children[g]):
            for gm in mixes:
                acc = resp[int(flat.filterid[gm])].copy()
                for h in sorted(children[g], reverse=True):
                    best = None
                    for hm in range(int(flat.mix_offset[h]), int(flat.mix_offset[h + 1])):
                        d = oracle.dt(resp[int(flat.filterid[hm])], *quad(hm))[0]
                        best = d if best is None else np.maximum(best, d)
                    acc = acc + best
                out.append(("inner", acc) + quad(gm))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=4, help="jobs of each kind sampled per level")
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 3, 6])
    args = ap.parse_args()
    oracle.build()
    flat = M.synthetic_person_model().flatten()
    feats = oracle.features_pyramid(flat, synth.synthetic_frame(1, 480, 640, 3))
    feats = feats if isinstance(feats, list) else feats[0]
    rng = np.random.default_rng(0)
    work = []
    for lv in args.levels:
        jobs = jobs_of(flat, oracle.responses(flat, feats[lv]))
        for kind in ("leaf", "inner"):
            mine = [j for j in jobs if j[0] == kind]
            work += [mine[i] for i in rng.choice(len(mine), min(args.filters, len(mine)), replace=False)]
    print(f"{len(work)} transforms ({sum(j[0] == 'inner' for j in work)} of accumulated scores), levels {args.levels}, ring {W.T_RING}")
    print("per wave-element; reload = whole-wave passes + passes through pop()'s own reload")
    print(f"{'policy':48s} {'kind':5s} {'fwd pops':>8s} {'spill':>6s} {'reload':>6s} {'(in pop)':>8s} {'r-o pops':>8s} {'spilled/lane-el':>15s}")
    for name, pol in POLICIES:
        for kind in ("leaf", "inner"):
            c = W.new_counts()
            for k, plane, ax, bx, ay, by, osx, osy in work:
                if k != kind:
                    continue
                tmp, _ = W.replay_levels([plane], ax, bx, osx, np.float32, counts=c, **pol)
                W.replay_levels([tmp[0].T.copy()], ay, by, osy, np.float32, counts=c, **pol)
            el = c["fwd_steps"]
            fb = c["fallback_fwd"] + c["fallback_ro"]
            print(f"{name:48s} {kind:5s} {c['fwd_pop_iters'] / el:8.3f} {c['spill_paths'] / el:6.3f} "
                  f"{(c['service_fwd'] + c['service_ro'] + fb) / el:6.3f} {fb / el:8.3f} {c['ro_pop_iters'] / el:8.3f} "
                  f"{c['spilled_entries'] / c['fwd_lane_elements']:15.3f}")


if __name__ == "__main__":
    main()
