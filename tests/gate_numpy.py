"""The rules of the traffic gates (include/copo_hip.h) restated: a python loop over records, scenes and slots, the
side and extent tests in numpy.float32 with the operations in the order the rules give them, one rounding each.  Equality with the
kernel is by construction: there is no ambiguity band and no tolerance; every comparison is on raw integers."""
import numpy as np

ST_EMPTY, ST_ALIVE, ST_WRECK = 0, 1, 2
RAW = ("count", "speed_q", "series", "headway", "sec_count", "sec_sum", "sec_hist", "scene_records", "alive")
f32 = np.float32


def speed_q(v):
    """rint(min(max(v, 0), 255) x 256) in float32, half to even (the field maps' quantisation)"""
    v = f32(v)
    v = f32(0.0) if not v >= f32(0.0) else v          # (fmaxf(NaN, 0) = 0)
    v = min(v, f32(255.0))
    return int(np.rint(f32(v * f32(256.0))))


def crossings(gates, px, py, cx, cy):
    """int [L]: +1 forward, -1 backward, 0 none, of the motion prev (px, py) -> cur (cx, cy) across every gate {ax, ay, bx, by} of `gates`
    [L, 4].  float32 throughout; numpy rounds every array operation by itself, so each line below is one rounding per element."""
    g = np.asarray(gates, np.float32).reshape(-1, 4)
    ax, ay, bx, by = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    px, py, cx, cy = f32(px), f32(py), f32(cx), f32(cy)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = bx - ax, by - ay
        sp = dx * (py - ay) - dy * (px - ax)
        sc = dx * (cy - ay) - dy * (cx - ax)
        mx, my = f32(cx - px), f32(cy - py)
        a = mx * (ay - py) - my * (ax - px)
        b = mx * (by - py) - my * (bx - px)
        within = ((a <= 0) & (b >= 0)) | ((a >= 0) & (b <= 0))
        fwd, bwd = within & (sp < 0) & (sc >= 0), within & (sp >= 0) & (sc < 0)
    assert sp.dtype == np.float32 and a.dtype == np.float32
    return fwd.astype(np.int64) - bwd.astype(np.int64)


def crossing(gate, px, py, cx, cy):
    return int(crossings(np.asarray(gate, np.float32).reshape(1, 4), px, py, cx, cy)[0])


class Recorder:
    def __init__(self, gates, sections, E, N, groups=1, bins=(1, 1), headway_bins=32, tt_bins=(32, 10)):
        self.gates = np.asarray(gates, np.float32).reshape(-1, 4)
        self.sections = [(int(a), int(b)) for a, b in sections]
        self.E, self.N, self.G, self.L, self.S = E, N, int(groups), len(self.gates), len(self.sections)
        (self.T, self.bin_records), self.HB, (self.TB, self.tt_bin) = bins, headway_bins, tt_bins
        self.group = np.zeros(E, np.int64)
        self.reset()

    def set_groups(self, group):
        self.group = np.asarray(group, np.int64).reshape(self.E).copy()

    def forget(self):
        E, N = self.E, self.N
        self.valid = np.zeros((E, N), bool)
        self.mem_x, self.mem_y = np.zeros((E, N), np.float32), np.zeros((E, N), np.float32)
        self.mem_aid, self.mem_ep = np.zeros((E, N), np.int64), np.zeros(E, np.int64)
        self.last_fwd = np.full((E, self.L), -1, np.int64)
        self.entry = np.full((E, N, self.S), -1, np.int64)

    def reset(self):
        G, L, S = self.G, self.L, self.S
        self.forget()
        self.r = 0
        self.count, self.speed_q = np.zeros((G, L, 2), np.int64), np.zeros((G, L, 2), np.int64)
        self.series, self.headway = np.zeros((G, L, 2, self.T), np.int64), np.zeros((G, L, self.HB), np.int64)
        self.sec_count, self.sec_sum = np.zeros((G, S), np.int64), np.zeros((G, S), np.int64)
        self.sec_hist = np.zeros((G, S, self.TB), np.int64)
        self.scene_records, self.alive = np.zeros(G, np.int64), np.zeros(G, np.int64)
        self.max_crossings_of_a_gate_in_a_scene_record = 0      # (a premise of the tests, not an accumulator)
        self.first_crossings = 0                                # forward crossings that found last_fwd = -1 (all groups, routed scenes)

    def raw(self):
        return {k: getattr(self, k) for k in RAW}

    def record(self, state, env):
        """state [16][E][N] float32 words, env [E][4] int32 of the simulator after a step / reset / set_state"""
        st = np.ascontiguousarray(state, np.float32)
        si = st.view(np.int32)
        r, tbin = self.r, min(self.r // self.bin_records, self.T - 1)
        for e in range(self.E):
            g = int(self.group[e])
            routed = 0 <= g < self.G
            ep = int(env[e, 1])
            alive_now = (si[13, e] & 0xFF) == ST_ALIVE
            fwd = [[] for _ in range(self.L)]                   # per gate: the slots that crossed forward, ascending
            for n in range(self.N):
                followed = bool(alive_now[n]) and bool(self.valid[e, n]) and int(si[14, e, n]) == int(self.mem_aid[e, n]) and ep == int(self.mem_ep[e])
                if not followed:
                    self.entry[e, n, :] = -1
                    continue
                cs = crossings(self.gates, self.mem_x[e, n], self.mem_y[e, n], st[0, e, n], st[1, e, n])
                for l in np.nonzero(cs)[0]:
                    c, q = int(cs[l]), speed_q(st[3, e, n])
                    d = 0 if c > 0 else 1
                    if c > 0:
                        fwd[l].append(n)
                    if routed:
                        self.count[g, l, d] += 1
                        self.speed_q[g, l, d] += q
                        self.series[g, l, d, tbin] += 1
            for l in range(self.L):
                self.max_crossings_of_a_gate_in_a_scene_record = max(self.max_crossings_of_a_gate_in_a_scene_record, len(fwd[l]))
                for k, n in enumerate(fwd[l]):
                    if k == 0:
                        if self.last_fwd[e, l] >= 0:
                            if routed:
                                self.headway[g, l, min(r - int(self.last_fwd[e, l]), self.HB - 1)] += 1
                        elif routed:
                            self.first_crossings += 1
                    elif routed:
                        self.headway[g, l, 0] += 1              # (h = 0: bin min(0, HB - 1))
                    self.last_fwd[e, l] = r
            # sections: every entry of this record first, then the exits
            for s, (gi, go) in enumerate(self.sections):
                for n in fwd[gi]:
                    self.entry[e, n, s] = r
            for s, (gi, go) in enumerate(self.sections):
                for n in fwd[go]:
                    if self.entry[e, n, s] >= 0:
                        tt = r - int(self.entry[e, n, s])
                        if routed:
                            self.sec_count[g, s] += 1
                            self.sec_sum[g, s] += tt
                            self.sec_hist[g, s, min(tt // self.tt_bin, self.TB - 1)] += 1
                        self.entry[e, n, s] = -1
            if routed:
                self.scene_records[g] += 1
                self.alive[g] += int(alive_now.sum())
            self.valid[e] = alive_now
            self.mem_x[e], self.mem_y[e] = st[0, e], st[1, e]
            self.mem_aid[e], self.mem_ep[e] = si[14, e], ep
        self.r += 1


def compare(got, ref):
    """every accumulator of `got` (dict of int64 arrays) equals the restatement's"""
    for k in RAW:
        a, b = np.asarray(got[k]), getattr(ref, k)
        assert a.shape == b.shape and np.array_equal(a, b), (k, np.argwhere(a != b)[:8].tolist() if a.shape == b.shape else (a.shape, b.shape))
