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


WANT_OWNER = np.array([[1, 1, 3, -1, -1, -1], [0, 2, 3, 4, 0, -1], [-1] * 6, [0, 0, 0, -1, 0, 0]])
WANT_MIN2 = {(0, 0): 7.5, (0, 1): 12.0, (0, 2): RNG, (1, 4): 3.0, (1, 0): RNG, (3, 4): RNG}
WANT_WHO4 = np.array([[1, 3, -1, -1], [0, 2, 3, 4], [-1] * 4, [0, -1, -1, -1]])
WANT_WHO2 = np.array([[1, 3], [0, 2], [-1, -1], [0, -1]])
WANT_TRUNC2 = np.array([0, 2, 0, 0])
