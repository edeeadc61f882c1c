"""Models and score planes that drive the selection half of the dynamic program -- k_dp_combine, k_dp_combine_seq, k_dp_root, the
k_argmin_count / _scan / _emit compaction and k_argmin_walk in pbd_kernels_dp.hip -- into what ordinary data never reaches:
parts that differ in their number of mixtures, exact ties between mixtures (Math::reduceMax / reducePickIndex keep the FIRST
maximum: a strict `>`), root scores equal to the threshold, rectangles on exact halves (cvRound rounds half to even).

Everything sits on a power-of-two grid -- planes multiples of 2^-3 with magnitude <= 8, biases multiples of 2^-4 with magnitude
<= 2, deformations of dt_hard_planes' pow2 family -- so that every sum the program forms is exact in fp16 planes, fp32 and fp64
alike, a float64 brute force over the tree equals the oracle bit for bit, and a tie is a tie in every arithmetic.

Shared by tests/test_dp_select_cpu.py (the oracle against the brute force, and counts of what the inputs reach) and
tests/test_gpu_dp_select.py (the kernels against the oracle)."""
import numpy as np

from partsbaseddetector_amd import model as M

import dt_hard_planes as H

# biases: multiples of 2^-4, magnitude <= 2, repeated values, both signs of zero
BIAS_GRID = np.array([-2.0, -1.0625, -0.5, -0.0625, -0.0, 0.0, 0.0, 0.0625, 0.5, 0.5, 1.0, 2.0])
BIAS_STEPS = np.array([-1.0, -0.5, -0.125, 0.0, 0.0, 0.125, 0.5, 1.0])
GROUP = 3       # mixtures mm with equal mm // GROUP share one deformation and one anchor: equal planes give equal transforms


def mixed_model(mix, pa, ncomponents=1, ksize=3, seed=0, thresh=0.0, interval=5, name="mixed"):
    """A Model whose part p has mix[p] mixtures (mix: one list, or one list per component; pa: 1-based parents, 0 for the root,
    one list or one per component).  Every (part, mixture) has its own ksize x ksize filter (small seeded values: the staged entry
    points never read them), the bias tables have synthetic_model's child-major L x K layout, and
    - the deformation and the anchor of mixture mm are those of its group mm // GROUP (dt_hard_planes' pow2 family): mixtures of
      one group transform equal planes into equal planes;
    - bias(mm)[pm] of the first mixture of a group is drawn from BIAS_GRID; the group's other mixtures differ from it by a
      multiple of 2^-3 (BIAS_STEPS: a plane of the 2^-3 grid can make up for the difference), by nothing under parent mixture 0
      (equal planes tie there); the column of the second parent mixture of a group repeats the column of the first (a part's
      mixtures 0 and 1, 3 and 4, ... receive equal messages)."""
    rng = np.random.default_rng(seed)
    frng = np.random.default_rng(seed + 100003)     # the filters' own stream: models that differ in ksize alone are otherwise equal
    per_c = isinstance(mix[0], (list, tuple))
    flen = 32
    m = M.Model(name=name, interval=interval, thresh=thresh, sbin=4, norient=18, flen=flen)
    for c in range(ncomponents):
        mix_c = list(mix[c] if per_c else mix)
        pa_c = list(pa[c] if isinstance(pa[0], (list, tuple)) else pa)
        assert len(mix_c) == len(pa_c)
        fid_c, bid_c, did_c, par_c = [], [], [], []
        for p, K in enumerate(mix_c):
            parent = pa_c[p] - 1
            par_c.append(parent)
            fid = []
            for _ in range(K):
                fid.append(len(m.filtersw))
                m.filtersw.append(frng.integers(-8, 9, (ksize, ksize * flen)) / 128.0)
            fid_c.append(fid)
            if parent < 0:
                bid_c.append([len(m.biasw)])
                m.biasw.append(float(rng.choice(BIAS_GRID)))
                did_c.append([])
                continue
            L = len(fid_c[parent])
            base = len(m.biasw)
            table = rng.choice(BIAS_GRID, size=(K, L))              # table[mm][pm] = bias(mm)[pm]
            table[0, 0] = -0.0 if p % 2 else 0.0                    # both signs of zero in every model
            for mm in range(K):                                     # within a group the rows differ by multiples of 2^-3
                if mm % GROUP:
                    step = rng.choice(BIAS_STEPS, size=L)
                    first = table[mm - mm % GROUP]
                    table[mm] = np.where(np.abs(first + step) <= 2.0, first + step, first - step)
                    table[mm, 0] = first[0]
            for pm in range(1, L, GROUP):
                table[:, pm] = table[:, pm - 1]
            m.biasw.extend(float(v) for v in table.ravel())
            bid_c.append([base + mm * L + l for l in range(L) for mm in range(K)])
            dids = []
            ngroups = (K + GROUP - 1) // GROUP
            ax, ay = rng.integers(-2, 3, ngroups), rng.integers(-2, 3, ngroups)
            for mm in range(K):
                g = mm // GROUP
                dids.append(len(m.defw))
                m.defw.append([float(v) for v in H.DEFORMATIONS["pow2"](g)])
                m.anchors.append((int(ax[g]), int(ay[g])))
            did_c.append(dids)
        m.filterid.append(fid_c)
        m.biasid.append(bid_c)
        m.defid.append(did_c)
        m.parentid.append(par_c)
    m.validate()
    return m


def table_model(K, ksize=3):
    """The model of row K of the combine / root table: tree pa = [0, 1, 1, 2, 2] with mixtures [K, 1, K, max(K-1, 1), min(K, 2)]
    -- a one-mixture child under a K-mixture root, children below the kernel's MAXM, parents (parts 3 and 4 hang below the
    one-mixture part 1) with fewer mixtures than their children -- and, for K = 2 and K = 8, a second component of three parts in
    a chain with mixtures [max(K-1, 1), K, 1]."""
    mix, pa = [K, 1, K, max(K - 1, 1), min(K, 2)], [0, 1, 1, 2, 2]
    if K in (2, 8):
        return mixed_model([mix, [max(K - 1, 1), K, 1]], [pa, [0, 1, 2]], ncomponents=2, ksize=ksize, seed=700 + K, name=f"table{K}")
    return mixed_model(mix, pa, ksize=ksize, seed=700 + K, name=f"table{K}")


TABLE_K = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16)      # both edges of every MAXM bucket of k_dp_combine: 2 | 4 | 6 | 8 | 16

# (rows, cols).  u8: no side above 256 (uint8 position planes); cell counts 1, 2, 3 and every HW % 4; (13, 11) = 143 cells is
# odd (fp64's two-cell threads) and leaves a tail of 3, so the wide load of the last plane's last cells reads the buffer's slack
SETS = {
    "u8": [(1, 1), (1, 2), (1, 3), (2, 2), (3, 5), (7, 9), (5, 13), (4, 16), (1, 256), (13, 11)],
    "i16": [(1, 1), (1, 2), (1, 3), (2, 2), (3, 5), (7, 9), (5, 13), (4, 16), (1, 257), (258, 1), (13, 11)],
}
HALF_SCALES = (0.5, 1.5, 2.5, 1.0, 0.75)       # (x - 1) * scale is an exact half for every odd x - 1 under the first three


def half_scales(nlevels):
    return np.array([HALF_SCALES[l % len(HALF_SCALES)] for l in range(nlevels)], np.float32)


def quantised_scores(model, dims, seed, dtype=np.float32):
    """One (nfilters, h, w) array per level: multiples of 2^-3 with magnitude <= 8.  The planes of the mixtures of one group
    (m0, m0 + 1, m0 + 2) of a part follow the variant (level + part) % 4:
      0  all equal: they tie wherever their biases are equal (bias(.)[0] is, within a group);
      1  plane(m0 + 1) = plane(m0) + bias(m0)[pm] - bias(m0 + 1)[pm] for pm = level % L: a tie reached through the bias;
         plane(m0 + 2) half a unit below;
      2  plane(m0) six units below; plane(m0 + 2) = plane(m0 + 1) + the bias difference: the tied pair is not the first mixture of
         its group and the lower-indexed mixture loses;
      3  independent planes over the whole range.
    A root has no bias per mixture: its differences are zero, and variant 1 is variant 0 with the third plane lowered."""
    rng = np.random.default_rng(seed)
    F = len(model.filtersw)
    bw = np.asarray(model.biasw, np.float32).astype(np.float64)
    out = []
    for l, (h, w) in enumerate(dims):
        s = rng.integers(-64, 65, (F, h, w)) / 8.0
        for c in range(model.ncomponents()):
            for p in range(model.nparts(c)):
                fid, par = model.filterid[c][p], model.parentid[c][p]
                L = len(model.filterid[c][par]) if par >= 0 else 1
                pm = l % L
                variant = (l + p) % 4
                if variant == 3:
                    continue

                def diff(ma, mb):       # bias(ma)[pm] - bias(mb)[pm]: what plane(mb) must exceed plane(ma) by to tie with it
                    return float(bw[model.biasid[c][p][ma] + pm] - bw[model.biasid[c][p][mb] + pm]) if par >= 0 else 0.0
                for m0 in range(0, len(fid), GROUP):
                    grp = list(range(m0, min(m0 + GROUP, len(fid))))
                    base = rng.integers(-16, 17, (h, w)) / 8.0 + (0.25 if m0 else 0.0)
                    if variant == 0:
                        for mm in grp:
                            s[fid[mm]] = base
                    elif variant == 1:
                        s[fid[m0]] = base
                        if len(grp) > 1:
                            s[fid[m0 + 1]] = base + diff(m0, m0 + 1)
                        if len(grp) > 2:
                            s[fid[m0 + 2]] = base - 0.5
                    else:
                        s[fid[m0]] = base - 6.0
                        if len(grp) > 1:
                            s[fid[m0 + 1]] = base
                        if len(grp) > 2:
                            s[fid[m0 + 2]] = base + diff(m0 + 1, m0 + 2)
        assert np.abs(s).max() <= 8.0 and np.array_equal(s * 8, np.rint(s * 8))
        out.append(np.ascontiguousarray(s, dtype))
    return out


# ---- float64 brute force over the tree ------------------------------------------------------------------------------------------
def _transform(sc, w, anchor):
    """out[y, x] = max over (y', x') of sc[y', x'] - w0 dx^2 - w1 dx - w2 dy^2 - w3 dy, dx = ax + x - x', dy = ay + y - y': every
    source cell tried for every cell (the two axes separate exactly: all terms are exact)."""
    h, wd = sc.shape
    dx = (anchor[0] + np.arange(wd)[:, None] - np.arange(wd)[None, :]).astype(np.float64)      # [x, x']
    dy = (anchor[1] + np.arange(h)[:, None] - np.arange(h)[None, :]).astype(np.float64)        # [y, y']
    tmp = (sc[:, None, :] - (w[0] * dx * dx + w[1] * dx)[None, :, :]).max(axis=2)             # [y', x]
    return (tmp.T[:, None, :] - (w[2] * dy * dy + w[3] * dy)[None, :, :]).max(axis=2).T        # [y, x]


def _first_max(values):
    """reduceMax / reducePickIndex over a list of planes: the first maximum wins.  Returns the maximum, its index, and per cell
    whether a second mixture reaches it."""
    best = np.full(values[0].shape, -np.inf)
    bi = np.zeros(values[0].shape, np.int32)
    for mm, v in enumerate(values):
        t = v > best
        best = np.where(t, v, best)
        bi = np.where(t, mm, bi)
    tied = sum((v == best).astype(np.int32) for v in values) > 1
    return best, bi, tied


def brute_force(flat, c, resp):
    """Max-sum over the tree of component c in float64 on resp (nfilters, H, W), parts with any number of mixtures, every filter
    used by one (part, mixture) only.  Returns rootv (H, W) float64, rooti, Ik (nslots, H, W) under the first-wins rule, and the
    counts of what the selection met: cells * parent mixtures whose maximum is shared by two child mixtures with the winner at
    index 0 ("tie_first") or above ("tie_later"), cells * parent mixtures of a one-mixture child under a parent with more
    ("k1_under_many"), and root cells whose maximum two root mixtures share ("root_tie", "root_tie_later")."""
    model = flat.model
    resp = np.asarray(resp, np.float64)
    _, Hh, Ww = resp.shape
    n = model.nparts(c)
    p0 = int(flat.part_offset[c])
    acc = [[resp[f].copy() for f in model.filterid[c][p]] for p in range(n)]
    Ik = np.zeros((max(flat.nslots, 1), Hh, Ww), np.int32)
    bw = np.asarray(model.biasw, np.float32).astype(np.float64)
    reach = {"tie_first": 0, "tie_later": 0, "k1_under_many": 0, "root_tie": 0, "root_tie_later": 0}
    for p in range(n - 1, 0, -1):       # children carry higher indices than their parents: acc[p] is complete here
        par = model.parentid[c][p]
        K, L = len(model.filterid[c][p]), len(model.filterid[c][par])
        msgs = []
        for mm in range(K):
            d = model.defid[c][p][mm]
            msgs.append(_transform(acc[p][mm], np.float32(model.defw[d]).astype(np.float64), model.anchors[d]))
        for pm in range(L):
            best, bi, tied = _first_max([msgs[mm] + bw[model.biasid[c][p][mm] + pm] for mm in range(K)])
            Ik[int(flat.ptr_slot[p0 + p]) + pm] = bi
            acc[par][pm] = acc[par][pm] + best
            reach["tie_first"] += int((tied & (bi == 0)).sum())
            reach["tie_later"] += int((tied & (bi > 0)).sum())
            if K == 1 and L > 1:
                reach["k1_under_many"] += Hh * Ww
    rb = bw[model.biasid[c][0][0]]
    rootv, rooti, tied = _first_max([a + rb for a in acc[0]])
    reach["root_tie"] += int(tied.sum())
    reach["root_tie_later"] += int((tied & (rooti > 0)).sum())
    return rootv, rooti, Ik, reach


# ---- numpy find + walk -----------------------------------------------------------------------------------------------------------
def round_mul(a, scale, R):
    """cv::Point_<int> * T: cvRound(a * scale) with the product in R -- round half to even"""
    return np.rint(np.asarray(a).astype(R) * R(scale)).astype(np.int64)


def find_walk(flat, c, scale, Ix, Iy, Ik, rootv, rooti, thresh, R=np.float32):
    """DynamicProgram::argmin for one (level, component) given min()'s planes: the roots rootv > R(float32(thresh)) in raster
    order, the positions and mixtures of every part walked down from them, and the parts' rectangles.  Returns roots (n, 2) as
    (x, y), scores (n,) float32, rects (n, nparts, 4), and counts of the rectangle corners (x - 1) * scale and (y - 1) * scale that
    are an exact half: below an even floor, below an odd floor, and -0.5 itself."""
    Hh, Ww = rootv.shape
    hit = rootv > R(np.float32(thresh))
    ys, xs = np.nonzero(hit)            # raster order
    p0 = int(flat.part_offset[c])
    n = int(flat.part_offset[c + 1]) - p0
    X = np.zeros((n, len(xs)), np.int64)
    Y = np.zeros((n, len(xs)), np.int64)
    Mx = np.zeros((n, len(xs)), np.int64)
    rects = np.zeros((len(xs), n, 4), np.int64)
    halves = {"even": 0, "odd": 0, "minus_half": 0}
    for p in range(n):
        gp = p0 + p
        if p == 0:
            X[0], Y[0], Mx[0] = xs, ys, rooti[ys, xs]
        else:
            par = int(flat.parentid[gp])
            sl = int(flat.ptr_slot[gp]) + Mx[par]
            X[p], Y[p], Mx[p] = Ix[sl, Y[par], X[par]], Iy[sl, Y[par], X[par]], Ik[sl, Y[par], X[par]]
        ks = flat.filter_ksize[flat.filterid[int(flat.mix_offset[gp]) + Mx[p]]].astype(np.int64)
        x1, y1 = round_mul(X[p] - 1, scale, R), round_mul(Y[p] - 1, scale, R)
        k = round_mul(ks, scale, R)
        x2, y2 = x1 + k - 1, y1 + k - 1
        rx, ry = np.minimum(x1, x2), np.minimum(y1, y2)
        rects[:, p] = np.stack([rx, ry, np.maximum(x1, x2) - rx, np.maximum(y1, y2) - ry], axis=1)
        for v in (X[p] - 1, Y[p] - 1):
            prod = v.astype(np.float64) * float(np.float32(scale))
            fl = np.floor(prod)
            half = prod - fl == 0.5
            halves["even"] += int((half & (fl % 2 == 0)).sum())
            halves["odd"] += int((half & (fl % 2 != 0)).sum())
            halves["minus_half"] += int((prod == -0.5).sum())
    return np.stack([xs, ys], axis=1), rootv[ys, xs].astype(np.float32), rects, halves


def same_candidates(roots, scores, rects, want):
    """the find + walk arrays against oracle.dp_argmin's list"""
    if len(want) != len(roots):
        return False
    for i, wc in enumerate(want):
        if (wc["root_x"], wc["root_y"]) != (int(roots[i][0]), int(roots[i][1])):
            return False
        if np.float32(wc["score"]).view(np.uint32) != scores[i].view(np.uint32):
            return False
        if not np.array_equal(wc["parts"], rects[i]):
            return False
    return True


# ---- the other models of the two test modules -------------------------------------------------------------------------------------
RAGGED_THRESH = 13.484375  # a value of the grid that root scores of ragged_model reach exactly (test_dp_select_cpu.py counts them)


RAGGED_SEED = 77        # of ragged_model's quantised_scores in both test modules


def ragged_model(ksize=3, thresh=RAGGED_THRESH, interval=5):
    """Two components whose parts have between 1 and 9 mixtures: the walk's Ik slot (w.slot + parent mixture) and plane
    (w.mix0 + mixture) differ from part to part."""
    return mixed_model([[3, 1, 9, 2, 5, 1, 7, 4], [2, 4, 1, 6]], [[0, 1, 1, 2, 2, 3, 3, 4], [0, 1, 2, 2]], ncomponents=2, ksize=ksize,
                       seed=911, thresh=thresh, interval=interval, name="ragged")


def chain_model(n, ksize=3):
    """n parts in one chain, one mixture each"""
    return mixed_model([1] * n, list(range(n)), ksize=ksize, seed=160, thresh=-1e6, name=f"chain{n}")


def tree_model(n, ksize=3):
    """n parts in a binary tree, two mixtures each"""
    return mixed_model([2] * n, [0] + [(i + 1) // 2 for i in range(1, n)], ksize=ksize, seed=161, thresh=-1e6, name=f"tree{n}")


WALK_SETS = {"u8": [(10, 10), (7, 15), (9, 11), (4, 25), (1, 100)], "i16": [(1, 257), (10, 10), (9, 11), (2, 50), (5, 21)]}


def shared_model(case, ksize=3):
    """The three shared-filter cases of test_filter_shared_inside_a_component (the sequential schedule, k_dp_combine_seq) with
    parts of two and three mixtures."""
    model = mixed_model([2, 3, 3, 2, 2, 2], [0, 1, 1, 2, 2, 3], ksize=ksize, seed=230 + case, name=f"shared{case}")
    fid = model.filterid[0]
    if case == 0:
        fid[2] = list(fid[1])                      # siblings 1 and 2 (children of the root) share their three filters
    elif case == 1:
        fid[3][0] = fid[1][1]                      # part 3 shares a filter with its parent (part 1) ...
        fid[5] = [fid[2][0], fid[2][0]]            # ... and part 5 uses its parent's (part 2) filter for both mixtures
    else:
        fid[0][1] = fid[0][0]                      # both root mixtures on one filter
        fid[4] = list(fid[3])                      # siblings 3 and 4 share
        fid[5][1] = fid[1][0]                      # a grandchild's filter = its grandparent's
    model.validate()
    return model


def root_only_model(K, ksize=3):
    """one part: the root kernel reads raw responses (from_acc == 0)"""
    return mixed_model([K], [0], ksize=ksize, seed=40 + K, name=f"root{K}")
