"""CPU replay of one wave of the streamed distance transform (dt_stream / DtRing in pbd_kernels_dp.hip): up to 64 lines in lock
step, each lane with its envelope's top in registers, a ring of T entries below it and a stack of spilled pairs, under the
whole-wave ring service: a spill pass takes every lane with at least `high` entries once one lane is over its ring, a reload pass
at an element boundary takes every lane with spilled pairs and at most `low` (read-out: `low_ro`) entries once one lane's ring is
drained over spilled pairs (no entry left; in the forward scan, whose elements end with a push, one), and pop() keeps its own reload for the lane that pops below its ring inside one element.

The replay MOVES the entries (ring slots are poisoned when an entry leaves them, the stack has exactly the kernel's records), so
a service that overwrote a live slot, reloaded into a full ring or lost a pair would show in the results; every service also
checks the invariants it relies on.  plain_rows is computeRow (include/DistanceTransform.hpp:152-182) with nothing else; its
read-out is stated as the entry every kernel variant takes, max{k : z[k] < os + q} (computeRow's own wherever z[] holds no NaN).
Shared by tests/test_dt_ring_service_cpu.py, tests/test_gpu_dt_ring_service.py and tools/dt_wave_sim.py."""
import numpy as np

import dt_hard_planes as H

T_RING, HIGH, LOW, LOW_RO, CHUNK = 8, 6, 2, 6, 16      # PBD_DT_RING, PBD_DT_HIGH, PBD_DT_LOW, PBD_DT_LOW_RO, PBD_DT_CH(C)
LANE_BY_LANE = dict(high=T_RING + 1, low=-1, low_ro=-1)  # every lane for itself: the service before the whole-wave one


def _isect(a, b, x0, x1, y0, y1, R):
    """quad_isect: Quadratic::operator()(x0, x1, y0, y1) in double, rounded once to R."""
    d = (x1 - x0).astype(np.float64)
    sq = ((x1 - x0) * (x1 + x0)).astype(np.float64)
    with np.errstate(all="ignore"):
        return ((((y1 - y0) - b * d) + a * sq) / ((2 * a) * d)).astype(R)


def plain_rows(src, a, b, os0, R=np.float32):
    """computeRow's forward scan on every row of src (M, N) and the read-out every kernel variant shares.  Returns the finished
    envelope v (M, N), z (M, N), its top index (M,), and the read-out's values (M, N) R and pointers (M, N)."""
    src = np.ascontiguousarray(src, R)
    Mr, N = src.shape
    rows = np.arange(Mr)
    s64 = src.astype(np.float64)
    v = np.zeros((Mr, N), np.int64)
    z = np.full((Mr, N + 1), np.inf, R)
    z[:, 0] = -np.inf
    k = np.zeros(Mr, np.int64)
    for q in range(1, N):
        qq = np.full(Mr, q, np.int64)
        s = _isect(a, b, v[rows, k], qq, s64[rows, v[rows, k]], s64[:, q], R)
        while True:
            m = (s <= z[rows, k]) & (k > 0)
            if not m.any():
                break
            k[m] -= 1
            s[m] = _isect(a, b, v[m, k[m]], qq[m], s64[m, v[m, k[m]]], s64[m, q], R)
        k += 1
        v[rows, k] = q
        z[rows, k] = s
    ktop = k.copy()
    out = np.empty((Mr, N), R)
    ptr = np.empty((Mr, N), np.int64)
    entry = np.arange(N + 1)
    for q in range(N):
        # the read-out of dt_stream (and of k_dt_coop): entry max{k : z[k] < os + q}, a comparison with NaN being false
        # (include/pbd.h, pbd_dp_min); where z[1..top] is increasing it is the entry computeRow's walk up from 0 stops at
        with np.errstate(invalid="ignore"):
            below = (z < R(os0 + q)) & (entry[None, :] <= ktop[:, None])      # entries above the top are stale
        k = N - np.argmax(below[:, ::-1], axis=1)
        vk = v[rows, k]
        x = np.float64(os0 + q) - vk
        with np.errstate(invalid="ignore"):
            out[:, q] = ((a * (x * x) + b * x) + s64[rows, vk]).astype(R)
        ptr[:, q] = vk
    return v, z[:, :N], ktop, out, ptr


def new_counts():
    return {"fwd_steps": 0, "fwd_lane_elements": 0, "fwd_pop_iters": 0, "ro_steps": 0, "ro_pop_iters": 0, "spill_paths": 0,
            "spilled_entries": 0, "service_fwd": 0, "service_ro": 0, "service_lanes": 0, "fallback_fwd": 0, "fallback_ro": 0,
            # the events the tests ask the inputs to reach
            "a_high_joins_high_minus_1_stays": 0, "b_lo0_bystander": 0, "c_fwd_service_joined": 0, "d_ro_service_joined": 0}


class Wave:
    """The lanes' state and the three ring operations, as DtRing has them."""

    def __init__(self, lines, a, b, os0, R, T, high, low, low_ro, counts):
        self.L = len(lines)
        assert 1 <= self.L <= 64
        self.a, self.b, self.os0, self.R, self.T = float(a), float(b), int(os0), R, T
        self.high, self.low, self.low_ro, self.c = high, low, low_ro, counts
        assert 3 <= high <= T + 1 and low <= T - 2 and low_ro <= T - 2
        self.N = np.array([len(x) for x in lines], np.int64)
        nmax = int(self.N.max())
        self.src = np.zeros((self.L, nmax), np.float64)
        for i, x in enumerate(lines):
            self.src[i, :len(x)] = np.asarray(x, R)
        self.rz = np.full((self.L, T), np.nan, R)          # ring: z, s (kept in double, R-valued), v; NaN / -1 = no entry
        self.rs = np.full((self.L, T), np.nan, np.float64)
        self.rv = np.full((self.L, T), -1, np.int64)
        npairs = (nmax + 1) // 2                             # the records the host gives a wave: ceil(longest line / 2) per lane
        self.ks = np.full((self.L, npairs, 3), np.nan, np.float64)   # sa, sb, za
        self.kv = np.full((self.L, npairs, 2), -1, np.int64)
        self.lo = np.zeros(self.L, np.int64)
        self.k = np.zeros(self.L, np.int64)
        self.vk = np.zeros(self.L, np.int64)
        self.zk = np.full(self.L, -np.inf, R)
        self.sk = self.src[:, 0].copy()

    def isect(self, m, x0, x1, y0, y1):
        return _isect(self.a, self.b, x0, x1, y0, y1, self.R)

    def push_below(self, act):
        n = self.k - self.lo + 1
        if (act & (n > self.T)).any():
            sp = act & (n >= self.high)
            assert (sp | ~(act & (n > self.T))).all()                     # a lane over its ring always spills
            assert (self.k[sp] - self.lo[sp] >= 2).all() and (self.lo[sp] % 2 == 0).all()
            joined = sp & (n <= self.T)
            if (joined & (n == self.high)).any() and (act & ~sp & (n == self.high - 1)).any():
                self.c["a_high_joins_high_minus_1_stays"] += 1
            i = np.flatnonzero(sp)
            sl = self.lo[i] % self.T
            rec = self.lo[i] >> 1
            assert (self.rv[i, sl] >= 0).all() and (self.rv[i, sl + 1] >= 0).all()
            self.ks[i, rec, 0], self.ks[i, rec, 1], self.ks[i, rec, 2] = self.rs[i, sl], self.rs[i, sl + 1], self.rz[i, sl]
            self.kv[i, rec, 0], self.kv[i, rec, 1] = self.rv[i, sl], self.rv[i, sl + 1]
            for d in (0, 1):
                self.rz[i, sl + d] = np.nan; self.rs[i, sl + d] = np.nan; self.rv[i, sl + d] = -1
            self.lo[i] += 2
            self.c["spill_paths"] += 1
            self.c["spilled_entries"] += 2 * len(i)
        i = np.flatnonzero(act)
        sl = self.k[i] % self.T
        assert (self.rv[i, sl] < 0).all(), "push onto a live ring slot"
        self.rz[i, sl], self.rs[i, sl], self.rv[i, sl] = self.zk[i], self.sk[i], self.vk[i]

    def _take_pair(self, i):
        """Lanes i take the record of their pair (lo-2, lo-1) off the stack: (sa, sb, za, va, vb, z of the upper entry)."""
        assert (self.lo[i] >= 2).all() and (self.lo[i] % 2 == 0).all()
        rec = (self.lo[i] - 2) >> 1
        sa, sb, za = self.ks[i, rec, 0].copy(), self.ks[i, rec, 1].copy(), self.ks[i, rec, 2].astype(self.R)
        va, vb = self.kv[i, rec, 0].copy(), self.kv[i, rec, 1].copy()
        assert (va >= 0).all() and (vb > va).all(), "reload of a record that was never spilled"
        self.ks[i, rec] = np.nan; self.kv[i, rec] = -1
        return sa, sb, za, va, vb, self.isect(i, va, vb, sa, sb)

    def service_reload(self, act, low, readout):
        n = self.k - self.lo
        trig = act & (n <= (0 if readout else 1)) & (self.lo > 0)     # a drained ring: the forward scan's holds the last push
        if not trig.any():
            return
        rl = act & (n <= low) & (self.lo > 0)
        self.c["b_lo0_bystander"] += int((act & (n <= low) & (self.lo == 0)).any())
        i = np.flatnonzero(rl)
        if len(i) == 0:
            return
        assert (n[i] <= self.T - 2).all(), "reload into a ring without room for two entries"
        sa, sb, za, va, vb, zb = self._take_pair(i)
        sl = (self.lo[i] - 2) % self.T
        assert (self.rv[i, sl] < 0).all() and (self.rv[i, sl + 1] < 0).all(), "reload onto a live ring slot"
        self.rz[i, sl], self.rs[i, sl], self.rv[i, sl] = za, sa, va
        self.rz[i, sl + 1], self.rs[i, sl + 1], self.rv[i, sl + 1] = zb, sb, vb
        self.lo[i] -= 2
        self.c["service_ro" if readout else "service_fwd"] += 1
        self.c["service_lanes"] += len(i)
        if (rl & ~trig).any():
            self.c["d_ro_service_joined" if readout else "c_fwd_service_joined"] += 1

    def pop(self, m, readout):
        """Lanes m (k already decremented): entry k becomes the top."""
        i = np.flatnonzero(m)
        sl = self.k[i] % self.T
        self.zk[i], self.sk[i], self.vk[i] = self.rz[i, sl], self.rs[i, sl], self.rv[i, sl]
        self.rz[i, sl] = np.nan; self.rs[i, sl] = np.nan; self.rv[i, sl] = -1
        under = m & (self.k < self.lo)
        if under.any():
            j = np.flatnonzero(under)
            assert (self.k[j] == self.lo[j] - 1).all()
            sa, sb, za, va, vb, zb = self._take_pair(j)
            sl = (self.lo[j] - 2) % self.T
            self.rz[j, sl], self.rs[j, sl], self.rv[j, sl] = za, sa, va
            self.sk[j], self.vk[j], self.zk[j] = sb, vb, zb
            self.lo[j] -= 2
            self.c["fallback_ro" if readout else "fallback_fwd"] += 1
        assert (self.vk[i] >= 0).all(), "pop of a ring slot that holds no entry"

    def envelope(self, lane):
        """The lane's whole envelope (v, z), gathered from the stack, the ring and the top."""
        v, z = [], []
        for p in range(int(self.lo[lane]) >> 1):
            sa, sb, za = self.ks[lane, p]
            va, vb = self.kv[lane, p]
            v += [va, vb]
            z += [self.R(za), _isect(self.a, self.b, np.array([va]), np.array([vb]), np.array([sa]), np.array([sb]), self.R)[0]]
        for e in range(int(self.lo[lane]), int(self.k[lane])):
            v.append(self.rv[lane, e % self.T]); z.append(self.rz[lane, e % self.T])
        v.append(self.vk[lane]); z.append(self.zk[lane])
        return np.array(v, np.int64), np.array(z, self.R)


def replay_wave(lines, a, b, os0, R=np.float32, T=T_RING, high=HIGH, low=LOW, low_ro=LOW_RO, CH=CHUNK, counts=None):
    """dt_stream on up to 64 lines (1-D arrays, any lengths) in lock step.  Returns per line the finished envelope (v, z), the
    read-out's values and pointers, and the counts (new_counts) with this wave's added."""
    c = counts if counts is not None else new_counts()
    w = Wave(lines, a, b, os0, R, T, high, low, low_ro, c)
    lanes = np.arange(w.L)
    for q in range(1, int(w.N.max())):
        act = q < w.N
        c["fwd_steps"] += 1
        c["fwd_lane_elements"] += int(act.sum())
        w.service_reload(act, low, False)
        qq = np.full(w.L, q, np.int64)
        sq = w.src[:, q]
        s = w.isect(lanes, w.vk, qq, w.sk, sq)
        while True:
            with np.errstate(invalid="ignore"):
                m = act & (s <= w.zk) & (w.k > 0)
            if not m.any():
                break
            c["fwd_pop_iters"] += 1
            w.k[m] -= 1
            w.pop(m, False)
            s[m] = w.isect(m, w.vk[m], qq[m], w.sk[m], sq[m])
        w.push_below(act)
        w.k[act] += 1
        w.vk[act] = q; w.zk[act] = s[act]; w.sk[act] = sq[act]
    env = [w.envelope(i) for i in range(w.L)]
    nch = (w.N + CH - 1) // CH
    out = [np.zeros(n, R) for n in w.N]
    ptr = [np.zeros(n, np.int64) for n in w.N]
    for it in range(int(nch.max())):
        q0 = (nch - 1 - it) * CH
        for i in range(CH - 1, -1, -1):
            q = q0 + i
            act = (it < nch) & (q < w.N)
            if not act.any():
                continue
            c["ro_steps"] += 1
            w.service_reload(act, low_ro, True)
            osf = (w.os0 + q).astype(R)
            while True:
                m = act & ~(w.zk < osf)
                if not m.any():
                    break
                c["ro_pop_iters"] += 1
                w.k[m] -= 1
                assert (w.k[m] >= 0).all()
                w.pop(m, True)
            x = (w.os0 + q - w.vk).astype(np.float64)
            val = ((w.a * (x * x) + w.b * x) + w.sk).astype(R)
            for lane in np.flatnonzero(act):
                out[lane][q[lane]] = val[lane]
                ptr[lane][q[lane]] = w.vk[lane]
    return env, out, ptr, c


def replay_levels(planes, a, b, os0, R=np.float32, **policy):
    """One pass over a pyramid the way the launch lays it out: the rows of all planes, in order, form flat lines and every 64 of
    them a wave.  Each wave's envelopes and read-out are compared with plain_rows, line for line and bit for bit; returns the
    read-out values per plane (the next pass's input) and the counts."""
    bits = np.uint64 if R == np.float64 else np.uint32
    counts = policy.pop("counts", None) or new_counts()
    plain = [plain_rows(p, a, b, os0, R) for p in planes]
    flat = [(l, r) for l, p in enumerate(planes) for r in range(p.shape[0])]
    for w0 in range(0, len(flat), 64):
        group = flat[w0:w0 + 64]
        env, out, ptr, _ = replay_wave([np.asarray(planes[l][r], R) for l, r in group], a, b, os0, R, counts=counts, **policy)
        for (l, r), (ev, ez), o, p in zip(group, env, out, ptr):
            pv, pz, ktop, pout, pptr = plain[l]
            kt = int(ktop[r])
            assert len(ev) == kt + 1 and np.array_equal(ev, pv[r, :kt + 1]), ("envelope v", l, r)
            assert np.array_equal(ez.view(bits), pz[r, :kt + 1].view(bits)), ("envelope z", l, r)
            assert np.array_equal(o.view(bits), pout[r].view(bits)), ("read-out value", l, r)
            assert np.array_equal(p, pptr[r]), ("read-out pointer", l, r)
    return [pl[3] for pl in plain], counts


# ---- planes whose neighbouring lines sit at different depths -----------------------------------------------------------------
# (rows, cols); "u8": no side above 256 (uint8 position planes), "i16": int16 planes for the whole launch.  Each size also runs
# transposed, so that the columns of a level cycle through the kinds as its rows do.
SIZES = {"u8": [(64, 9), (64, 10), (65, 11), (63, 12), (2, 13), (64, 17), (130, 40), (64, 255)], "i16": [(5, 300), (64, 17), (130, 40)]}
ROW_KINDS = ("constant", "ramp", "spikes", "quantised", "normal", "stairs0", "stairs1", "stairs2", "stairs3", "dip10", "dip11")
def _row(kind, rng, n, r):
    if kind == "ramp":          # steep and convex upwards: every element pops the whole envelope
        q = np.arange(n, dtype=np.float64)
        return 4.0 * q * q + float(r % 3)
    if kind.startswith("stairs"):
        # stairs<s>: steps of 7 + s equal values (the first one longer by one: no riser has left an entry under it yet) at the
        # levels 4096 j^2 -- each riser pops its whole step and the riser before it, so the envelope is 8 + s entries deep at the
        # end of every step
        w = 7 + int(kind[-1])
        j = np.maximum(np.arange(n) - 1, 0) // w
        return 4096.0 * j * j
    if kind.startswith("dip"):
        # a plateau with a spike every 32 elements that pops the 10 (dip10) or 11 (dip11) entries it dominates (d (d + 1) <= h / |a|
        # for the entry d cells back; one fewer at |a| = 0.012) and no more: a pop run that ends deep inside the envelope, on an
        # entry of the other parity in the neighbouring row -- one lane drains its ring, the next keeps one entry more
        out = np.full(n, 0.5)
        out[30::32] += 1.25 if kind == "dip10" else 1.5
        return out
    return H.plane(kind, rng, 1, n)[0]


def service_plane(rng, h, w, first):
    """(h, w) float64 plane, every value exact in float32: row r is of kind ROW_KINDS[(first + r) % 11]."""
    return np.stack([_row(ROW_KINDS[(first + r) % len(ROW_KINDS)], rng, w, r) for r in range(h)])


def service_levels(nfilters, set_name, seed, dtype=np.float32):
    """The score planes of a set: [level] -> (nfilters, rows, cols); every size of SIZES[set_name], then every size transposed."""
    rng = np.random.default_rng(seed)
    sizes = SIZES[set_name]
    out = [np.stack([service_plane(rng, h, w, f + l) for f in range(nfilters)]) for l, (h, w) in enumerate(sizes)]
    out += [np.stack([service_plane(rng, h, w, f + l + 4).T for f in range(nfilters)]) for l, (h, w) in enumerate(sizes)]
    return [np.ascontiguousarray(o.astype(np.float32).astype(dtype)) for o in out]
