"""Hand-made distance tables for tests/influence_numpy.py, shared by test_influence_cpu.py and test_gpu_influence.py.  No GPU and no
native library is touched at import."""
import numpy as np

RNG = 40.0
F = np.float32
DELTAS = (0.05, 0.05)
POISON = 0x7FC0BEEF              # a NaN with a payload: what an entry nobody wrote still holds


def table():
    """Four egos, five vehicles (slot = index; an ego's own column is RNG), six beams.
    ego 0 (slot 0): vehicles 1 and 2 tie on beam 0 (the lower slot owns it, min2 = min1); vehicle 3 is behind 1 on beam 1 (occluded
        there) and alone on beam 2; a box ties vehicle 4 on beam 3 (nobody owns it) and is nearer than vehicle 2 on beam 4.
    ego 1 (slot 1): four owners at distinct distances -- order by distance, truncation at M < 4; two of them tie in their smallest
        distance (the lower slot first).
    ego 2 (slot 2): nobody in range (no candidates).
    ego 3 (slot 3): one vehicle on every beam, a value above the range among them."""
    d = np.full((4, 5, 6), RNG, F)
    s = np.full((4, 6), RNG, F)
    d[0, 1, 0], d[0, 2, 0] = 7.5, 7.5
    d[0, 1, 1], d[0, 3, 1] = 9.0, 12.0
    d[0, 3, 2] = 15.0
    d[0, 4, 3], s[0, 3] = 20.0, 20.0
    d[0, 2, 4], s[0, 4] = 11.0, 6.0
    d[1, 0, 0], d[1, 2, 1], d[1, 3, 2], d[1, 4, 3] = 30.0, 5.0, 5.0, 12.5
    d[1, 0, 4], d[1, 4, 4] = 2.0, 3.0
    d[3, 0, :] = (4.0, 4.5, 5.0, 41.0, 39.5, 0.0)
    return d, s


# (E, N, K, G, M) of the stand-alone fold: one scene of one member; rounds of exactly 64; three rounds, the last of two lanes, and every
# lane of the first a different member; a last workgroup of two scenes.  The scenes named in TALLY_BAD_GROUPS are outside [0, G).
TALLY_SHAPES = ((1, 7, 1, 1, 1), (3, 64, 3, 5, 4), (3, 130, 64, 1, 8), (1030, 7, 3, 5, 2))
TALLY_BAD_GROUPS = {(3, 64, 3, 5, 4): {2: -1}, (3, 130, 64, 1, 8): {2: 1}, (1030, 7, 3, 5, 2): {5: -1, 6: 5}}
F_ACTED = 0x01


def tally_tables(shape, seed=0):
    """Random inputs of copo_influence_tally at `shape`, as a dict of numpy arrays: flags uint8 [E N] (explicit: about a third of the rows
    lack ACTED), dist [E N][4], verdict_cf [E N M][K][4], who int32 [E N][M] (-1 holes), ncand int32 [E N] (kept | truncated << 16), hit
    [E N][M], seat int32 [E][N] (-1: nobody), group int32 [E] (-1 and G among them where E >= 3).  Scene 1 has a single member; with K >=
    64 the first 64 slots of scene 0 all act and are 64 different members.  Among the counted pairs up to two verdict means are 2000 (beyond the clamp
    of 1024) and up to two NaN."""
    E, N, K, G, M = shape
    rng = np.random.RandomState(seed + E + N)
    group = rng.randint(0, G, E).astype(np.int32)
    for e, g in TALLY_BAD_GROUPS.get(shape, {}).items():
        group[e] = g
    seat = rng.randint(-1, K, (E, N)).astype(np.int32)
    flags = ((rng.randint(0, 256, E * N) & ~F_ACTED) | (rng.uniform(size=E * N) < 0.67)).astype(np.uint8)
    if K >= 64:
        seat[0, :64] = rng.permutation(K)[:64]
        flags[:64] |= F_ACTED
    if E >= 3:
        seat[1] = np.where(rng.uniform(size=N) < 0.2, -1, K - 1)
    who = np.where(rng.uniform(size=(E * N, M)) < 0.3, -1, rng.randint(0, N, (E * N, M))).astype(np.int32)
    trunc = np.where(rng.uniform(size=E * N) < 0.5, 0, rng.randint(1, 6, E * N))
    ncand = ((who >= 0).sum(1) | (trunc << 16)).astype(np.int32)
    dist = np.concatenate([rng.normal(0.0, 0.3, (E * N, 2)), rng.normal(-0.5, 0.2, (E * N, 2))], 1).astype(F)
    shift = np.concatenate([rng.normal(0.0, 0.05, (E * N * M, K, 2)), rng.normal(0.0, 0.1, (E * N * M, K, 2))], 2)
    verdict_cf = (np.repeat(dist, M, 0)[:, None, :] + shift).astype(F)
    ok = (group >= 0) & (group < G)
    counted = (ok[:, None] & (seat >= 0)).reshape(-1) & ((flags & F_ACTED) != 0)
    rows, cands = np.nonzero(counted[:, None] & (who >= 0))
    for i, value in zip(rng.choice(len(rows), min(4, len(rows)), replace=False), (2000.0, np.nan, 2000.0, np.nan)):
        verdict_cf[rows[i] * M + cands[i], seat.reshape(-1)[rows[i]], i % 2] = value
    return dict(flags=flags, dist=dist, verdict_cf=verdict_cf, who=who, ncand=ncand, hit=rng.uniform(0.0, 1.0, (E * N, M)).astype(F), seat=seat,
                group=group)


WANT_OWNER =np.array([[1, 1, 3, -1, -1, -1], [0, 2, 3, 4, 0, -1], [-1] * 6, [0, 0, 0, -1, 0, 0]])
WANT_MIN2 = {(0, 0): 7.5, (0, 1): 12.0, (0, 2): RNG, (1, 4): 3.0, (1, 0): RNG, (3, 4): RNG}
WANT_WHO4 = np.array([[1, 3, -1, -1], [0, 2, 3, 4], [-1] * 4, [0, -1, -1, -1]])
WANT_WHO2 = np.array([[1, 3], [0, 2], [-1, -1], [0, -1]])
WANT_TRUNC2 = np.array([0, 2, 0, 0])
