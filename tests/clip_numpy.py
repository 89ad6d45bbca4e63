"""Restatement of the event-clip rules (csrc/clip_kernels.hip) in plain numpy, scene by scene and record by record:
the per-scene ring is a python list of every snapshot ever taken (so no ring arithmetic is shared with the kernels), the state machine
and the ordered commit are loops.  Everything is copies, integer logic and float32 `<`, so the comparison with the device is bit for bit."""
import numpy as np

WORDS, HEADER = 6, 8
KIND_FLAG, KIND_TTC, KIND_GAP = 1, 2, 4
H_SCENE, H_FIRST_REC, H_LENGTH, H_TRIG_REC, H_TRIG_SLOT, H_KIND, H_TRIG_AID, H_N_EVENTS = range(8)


def snapshot(st, env):
    """(words uint32 [E][6][N], env words int32 [E][2]) of a state block [16][E][N] (any 32-bit dtype) and env block [E][4]"""
    su = np.ascontiguousarray(st).view(np.uint32)
    w = np.stack([su[0], su[1], su[2], su[3], su[13] & np.uint32(0xFF), su[14]], 1)
    return w.astype(np.uint32), np.asarray(env)[:, :2].astype(np.int32)


class ClipTracker:
    def __init__(self, E, N, pre, post, max_clips, flag_mask=0, ttc_below=0.0, gap_below=0.0):
        self.E, self.N, self.pre, self.post, self.max_clips = E, N, pre, post, max_clips
        self.cap = pre + post + 1
        self.flag_mask, self.ttc_below, self.gap_below = int(flag_mask), np.float32(ttc_below), np.float32(gap_below)
        self.reset()

    def reset(self):
        self.r = 0
        self.history = []                              # every snapshot so far: (words [E][6][N], env [E][2])
        self.armed = [None] * self.E                   # per scene None (idle) or dict(trig_rec, slot, kind, aid, n_events, countdown)
        self.lo = [0] * self.E
        self.n_clips = self.dropped = 0
        self.header = np.zeros((self.max_clips, HEADER), np.int32)
        self.snaps = np.zeros((self.max_clips, self.cap, WORDS, self.N), np.uint32)
        self.envw = np.zeros((self.max_clips, self.cap, 2), np.int32)
        self.ready_log = []                            # per record: the scenes that committed in it (tests look at these)

    def _fires(self, flags, ttc, gap):
        """per scene: (bool [N] any trigger, kind)"""
        E, N = self.E, self.N
        f = np.zeros((E, N), bool)
        t = np.zeros((E, N), bool)
        g = np.zeros((E, N), bool)
        if flags is not None:
            f = (np.asarray(flags, np.uint8).reshape(E, N).astype(np.int64) & self.flag_mask) != 0
        with np.errstate(invalid="ignore"):
            if ttc is not None and self.ttc_below > 0:
                t = np.asarray(ttc, np.float32).reshape(E, N) < self.ttc_below
            if gap is not None and self.gap_below > 0:
                g = np.asarray(gap, np.float32).reshape(E, N) < self.gap_below
        kind = KIND_FLAG * f.any(1) + KIND_TTC * t.any(1) + KIND_GAP * g.any(1)
        return f | t | g, kind

    def _commit(self, scenes, last):
        for e in scenes:                               # ascending scene order
            a = self.armed[e]
            first = max(a["trig_rec"] - self.pre, self.lo[e])
            length = last - first + 1
            assert 1 <= length <= self.cap
            if self.n_clips < self.max_clips:
                c = self.n_clips
                self.header[c] = [e, first, length, a["trig_rec"], a["slot"], a["kind"], a["aid"], a["n_events"]]
                for k in range(length):
                    w, v = self.history[first + k]
                    self.snaps[c, k], self.envw[c, k] = w[e], v[e]
                self.n_clips += 1
            else:
                self.dropped += 1
            self.armed[e] = None
            self.lo[e] = last + 1

    def record(self, st, env, flags=None, ttc=None, gap=None):
        w, v = snapshot(st, env)
        self.history.append((w, v))
        fire, kind = self._fires(flags, ttc, gap)
        ready = []
        for e in range(self.E):
            a = self.armed[e]
            if a is not None:
                if fire[e].any():
                    a["n_events"] += 1
            elif fire[e].any():
                slot = int(np.argmax(fire[e]))
                a = self.armed[e] = dict(trig_rec=self.r, slot=slot, kind=int(kind[e]), aid=int(w[e, 5, slot].view(np.int32)), n_events=1,
                                         countdown=self.post)
            if a is not None:
                if a["countdown"] == 0:
                    ready.append(e)
                else:
                    a["countdown"] -= 1
        self.ready_log.append(list(ready))
        self._commit(ready, self.r)
        self.r += 1

    def flush(self):
        self._commit([e for e in range(self.E) if self.armed[e] is not None], self.r - 1)
