"""Restatement of the scene-rewind rules (csrc/rewind_kernels.hip) in plain numpy on `get_state()` arrays: the ring of
a scene is a python list of (record, state words [16][N], env words [4]) from which the oldest entry is dropped -- no ring arithmetic is
shared with the kernels --, the fork selection walks that list, the tally is a loop over the scenes.  Everything is copies, integer
logic and one float32 clamp, so the comparison with the device is bit for bit."""
import numpy as np

ST_EMPTY, ST_ALIVE, ST_WRECK = 0, 1, 2
F_ACTED, F_DONE, F_ARRIVE, F_CRASH, F_OUT, F_MAXSTEP, F_SPAWNED, F_ENV_RESET = (1 << i for i in range(8))
TALLY_INIT = (0, 0, 0, 0, 0, 0, 0, -1)
T_STEPS, T_ACTED, T_ARRIVE, T_CRASH, T_OUT, T_MAXSTEP, T_WATCH_FLAGS, T_WATCH_STEP = range(8)


class RewindRing:
    """The last `depth` stored records of each of E scenes; record r is stored iff r % stride == 0."""

    def __init__(self, E, N, depth, stride):
        self.E, self.N, self.depth, self.stride = E, N, depth, stride
        self.reset()

    def reset(self):
        self.r = 0
        self.rings = [[] for _ in range(self.E)]       # per scene: [(record, words uint32 [16][N], env int32 [4])], oldest first

    def record(self, st, env):
        su = np.ascontiguousarray(st).view(np.uint32)
        env = np.asarray(env, np.int32)
        if self.r % self.stride == 0:
            for e in range(self.E):
                self.rings[e].append((self.r, su[:, e].copy(), env[e].copy()))
                if len(self.rings[e]) > self.depth:
                    self.rings[e].pop(0)
        self.r += 1

    def span(self):
        return (self.rings[0][0][0], self.rings[0][-1][0]) if self.r else None

    def lookup(self, scene, rec):
        """(record, words, env) of the newest stored record <= rec of `scene`, or None for an invalid request"""
        if self.r == 0 or rec < 0 or not 0 <= scene < self.E:
            return None
        best = None
        stored = 0
        while stored + self.stride <= min(rec, self.r - 1):      # the newest stored record <= rec, whether the ring still has it or not
            stored += self.stride
        for entry in self.rings[scene]:
            if entry[0] == stored:
                best = entry
        return best

    def fork(self, t_st, t_env, first, scenes, records, copies=1, lcf=None, watch_slots=None):
        """Applies the fork to a target state block [16][TE][N] / env block [TE][4] (in place, any 32-bit dtype); lcf / watch_slots:
        None or one value per TARGET scene.  Returns (status [T], watch_aid [T]) with T = len(scenes) * copies."""
        tu, tv = t_st.view(np.uint32), t_env
        sc, rc = np.repeat(np.asarray(scenes), copies), np.repeat(np.asarray(records), copies)
        T = len(sc)
        status, aid = np.full(T, -1, np.int32), np.full(T, -1, np.int32)
        for j in range(T):
            hit = self.lookup(int(sc[j]), int(rc[j]))
            if hit is None:
                tu[:, first + j] = 0
                tu[13, first + j] = ST_EMPTY
                tv[first + j] = [0, 0, 0, 1]
                continue
            r, words, envw = hit
            words = words.copy()
            alive = (words[13] & 0xFF) == ST_ALIVE
            if lcf is not None and not np.isnan(np.float32(lcf[j])):
                v = np.minimum(np.maximum(np.float32(lcf[j]), np.float32(-1.0)), np.float32(1.0))
                words[10, alive] = np.float32(v).view(np.uint32)
            tu[:, first + j] = words
            tv[first + j] = envw
            status[j] = r
            if watch_slots is not None and 0 <= watch_slots[j] < self.N and alive[watch_slots[j]]:
                aid[j] = words[14, watch_slots[j]].view(np.int32)
        return status, aid


def tally_init(B):
    return np.tile(np.asarray(TALLY_INIT, np.int32), (B, 1))


def tally(flags, watch_slots, rows):
    """one step's flags uint8 [B][N] into the rows int32 [B][8] (in place); watch_slots [B] or None"""
    flags = np.asarray(flags, np.uint8)
    B, N = flags.shape
    for b in range(B):
        f = flags[b].astype(np.int64)
        done = (f & F_DONE) != 0
        steps_before = int(rows[b, T_STEPS])
        rows[b, T_STEPS] += 1
        rows[b, T_ACTED] += int(((f & F_ACTED) != 0).sum())
        for col, bit in ((T_ARRIVE, F_ARRIVE), (T_CRASH, F_CRASH), (T_OUT, F_OUT), (T_MAXSTEP, F_MAXSTEP)):
            rows[b, col] += int((done & ((f & bit) != 0)).sum())
        w = -1 if watch_slots is None else int(watch_slots[b])
        if rows[b, T_WATCH_FLAGS] == 0 and 0 <= w < N and done[w]:
            rows[b, T_WATCH_FLAGS] = int(f[w])
            rows[b, T_WATCH_STEP] = steps_before
    return rows


def hand_tally_case():
    """(flags of three steps, uint8 [3][5] each; watch_slots [3]; the rows they must give, worked out by hand).  Scene 0 watches slot 2,
    whose agent crashes in step 0; the slot's next occupant arrives in step 2 and must not overwrite the first end.  Scene 1 watches
    nothing (-1) and has a CRASH bit without DONE, which is not counted.  Scene 2 watches slot 4, which leaves the road in step 1, and
    is reset in step 2 (ENV_RESET on every slot, one agent at its horizon)."""
    A, D = F_ACTED, F_DONE
    steps = [np.zeros((3, 5), np.uint8) for _ in range(3)]
    steps[0][0, 1], steps[0][0, 2] = A, A | D | F_CRASH
    steps[0][1, 0] = A | D | F_ARRIVE
    steps[0][2, 4] = A
    steps[1][0, 2] = F_SPAWNED
    steps[1][2, 4] = A | D | F_OUT
    steps[2][0, 2] = A | D | F_ARRIVE
    steps[2][1, 3] = A | F_CRASH
    steps[2][2, :] = F_SPAWNED | F_ENV_RESET
    steps[2][2, 0] = A | D | F_MAXSTEP | F_ENV_RESET
    watch = np.array([2, -1, 4], np.int32)
    want = np.array([[3, 3, 1, 1, 0, 0, A | D | F_CRASH, 0],
                     [3, 2, 1, 0, 0, 0, 0, -1],
                     [3, 3, 0, 0, 1, 1, A | D | F_OUT, 1]], np.int32)
    return steps, watch, want


def random_actions(rng, E, N):
    """random actions [E][N][2] under which agents crash within a short horizon: any steering, and a throttle around +0.8 in the odd
    slots and around -0.6 (braking) in the even ones, so that followers run into standing leaders"""
    act = np.zeros((E, N, 2), np.float32)
    act[..., 0] = rng.uniform(-1.0, 1.0, (E, N))
    act[..., 1] = np.where(np.arange(N) % 2 == 1, 0.8, -0.6)[None, :] + rng.uniform(-0.2, 0.2, (E, N))
    return act
