"""CPU: the `.npz` files of a `TripTable` and a `ConflictTable` written before the two shared `copo_amd/_rowlog.py`
(tests/golden/rowlog_*.npz: the hand sequences' rows at 7 slots, the trips after the flush and the conflicts before the `clear`) load
with the same raw rows, `meta` and decoded columns, and a file written now reads back the same."""
import os

import numpy as np

import conflict_cases as cc
import trip_cases as tc
from copo_amd import conflicts, trips
from copo_amd.sim import SimConfig


def test_npz_files_of_both_tables_keep_their_format(golden_dir, tmp_path):
    cfg = SimConfig(map="roundabout", num_envs=4, num_agents=7)
    want = dict(trips=trips.TripTable(tc.hand_expected(7)[1], trips.trip_meta(cfg, 7, 100, tc.STOP_SPEED, dropped=3, n_records=8)),
                conflicts=conflicts.ConflictTable(cc.hand_expected(7)[0], conflicts.conflict_meta(cfg, 7, 100, cc.RADIUS, cc.LEAVE, dropped=3, n_records=4)))
    for name, t in want.items():
        old = type(t).load(os.path.join(golden_dir, "rowlog_%s.npz" % name))
        back = type(t).load(t.save(str(tmp_path / (name + ".npz"))))
        for got in (old, back):
            assert len(got) == len(t) > 0 and got.raw.dtype == np.uint32 and np.array_equal(got.raw, t.raw) and got.meta == t.meta
            assert list(got.columns) == list(t.columns)
            for k, v in t.columns.items():
                assert got[k].dtype == v.dtype and np.array_equal(got[k], v, equal_nan=v.dtype.kind == "f"), (name, k)
