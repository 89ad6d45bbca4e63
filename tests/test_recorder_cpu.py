"""The rules of the device evaluation recorder without a GPU: their restatement (tests/recorder_numpy.py) against what the REFERENCE's
RecorderEnv returned for the scripted episodes of tests/golden/recorder.npz -- the SVO estimate included -- and against `VecRecorder` on
the 25 columns the two share; the column names of `copo_amd.eval.device_recorder`; the argument checks of `copo_recorder_create`."""
import ctypes as C

import numpy as np

import recorder_cases as rc
import recorder_numpy as rn


def test_columns_are_the_vectorised_recorders_plus_the_svo_estimate():
    from copo_amd import _capi
    from copo_amd.eval import device_recorder as dr, vec_recorder as vr
    assert dr.COLUMNS == vr.COLUMNS + dr.SVO_COLUMNS == rn.COLUMNS and dr.SVO_COLUMNS == rc.SVO
    assert dr.NCOL == rn.NCOL == _capi.RECORDER_NCOL == 31


def test_restatement_equals_the_reference_recorder(golden_dir):
    """Every column, the four SVO columns among them, at the tolerance of test_vectorised_recorder_equals_the_reference_recorder: the
    reference's statistics in float64 on the same numbers rounded to float32.  Every agent of the fixture terminates, so the estimate
    over the terminated agents is the reference's over all agents."""
    cases = rc.golden_cases(golden_dir)
    assert len(cases) == 3
    for c, (stream, ref) in enumerate(cases):
        T, _, N = stream["flags"].shape
        rows = rc.restate([stream], 1, N).rows
        assert rows.shape == (1, rn.NCOL) and rows[0, -2] == 0 and rows[0, -1] == 0
        row = dict(zip(rn.COLUMNS, rows[0]))
        assert row["env_episode_steps"] == T and row["num_agents_total"] == ref["num_agents_total"]
        for col in rn.COLUMNS:
            if col in rc.SVO:
                print("case %d %s: %.3e from the reference" % (c, col, abs(row[col] - ref[col])))
            if col != "env_episode_steps":
                np.testing.assert_allclose(row[col], ref[col], rtol=2e-6, atol=2e-6, err_msg="case %d: %s" % (c, col))


STREAM = dict(E=3, N=9, T=40, resets={0: [13, 30], 1: [21], 2: [0, 17, 39]}, seed=3, lonely=((1, 4),))


def test_restatement_equals_the_vectorised_recorder():
    """The 25 shared columns on a scripted stream of three scenes cut into fragments of 8 (episodes end inside and across fragments,
    one with no terminated agent): float64 both, they differ by the order of the sums over at most 9 slots."""
    import torch
    from copo_amd.eval.vec_recorder import COLUMNS, VecRecorder
    frags = rc.cut(rc.scripted(**STREAM), 8)
    rows = rc.restate(frags, STREAM["E"], STREAM["N"]).rows
    rec = VecRecorder(STREAM["E"], "cpu")
    for b in frags:
        rec.add({k: torch.from_numpy(v) for k, v in b.items()})
    assert len(rec.rows) == len(rows) == 5                  # (scene 2's first episode ends at step 0 with nobody terminated)
    for e in range(STREAM["E"]):
        mine, theirs = rows[rows[:, -2] == e], [r for r in rec.rows if r["scene"] == e]
        assert len(mine) == len(theirs) > 0
        for a, b in zip(mine, theirs):
            np.testing.assert_allclose(a[:25], [b[c] for c in COLUMNS], rtol=1e-9, atol=1e-9)
    assert rows[rows[:, -2] == 2][:, -1].tolist() == [1, 2]    # the episode without a row still counts


def test_recorder_create_rejects_bad_arguments_without_a_gpu():
    """The checks come before any HIP call and leave the error string."""
    from copo_amd import _capi
    h = C.c_void_p()
    assert _capi.lib.copo_recorder_create(4, 8, 16, 0, None) == -1
    for E, N, max_rows, limit, word in ((0, 8, 16, 0, b"E=0"), (4, 0, 16, 0, b"N=0"), (4, _capi.RECORDER_MAX_SLOTS + 1, 16, 0, b"N=257"),
                                        (4, 8, 0, 0, b"max_rows=0"), (4, 8, 16, -1, b"limit=-1")):
        assert _capi.lib.copo_recorder_create(E, N, max_rows, limit, C.byref(h)) == -2 and not h.value
        assert word in _capi.lib.copo_last_error()
    assert _capi.lib.copo_recorder_add(None, None, None, None, None, None, 1, None) == -1
    assert _capi.lib.copo_recorder_destroy(None) == -1
