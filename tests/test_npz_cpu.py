"""CPU: the `.npz` files of the field maps, the traffic gates and the encroachment log's aggregates written before the three shared one
implementation of the format (`copo_amd/_npz.py`; tests/golden/npz_*.npz, hand-made integer arrays of a few cells) load with the same
arrays, derived arrays and `meta`, hold the same keys and dtypes as a file written now, and a file written now reads back the same."""
import os

import numpy as np

from copo_amd import encroach, fields, gates

META = dict(dt=0.1, num_agents=7, n_records=12, note="hand-made", nested=dict(a=[1, 2.5, None], b=True))


def _fields():
    G, H, W = 2, 3, 4
    maps = (np.arange(G * len(fields.LAYERS) * H * W, dtype=np.int64).reshape(G, len(fields.LAYERS), H, W) * 7) % 23
    maps[:, 4] -= 11                                         # (vx_q is signed)
    maps[1, 2, 0, 0] = 0                                     # a cell nobody visited
    data = fields.derive(maps, np.array([12, 0], np.int64), META["dt"])
    data["meta"] = dict(META, x0=-1.5, y0=2.0, cell=0.5, W=W, H=H, groups=G)
    return dict(maps=maps, scene_records=data["scene_records"]), data


def _gates():
    dims = G, L, S, T, HB, TB = 2, 3, 2, 4, 5, 3
    words = sum(int(np.prod(s)) for s in gates.shapes(*dims).values())
    raw = gates.split((np.arange(words, dtype=np.int64) * 5) % 17, *dims)
    raw["scene_records"][1] = 0
    raw["count"][0, 1] = 0
    raw["sec_count"][1, 0] = 0
    data = gates.derive(raw, META["dt"])
    data["meta"] = dict(META, gates=[[0.0, 1.0, 2.0, 3.0]] * L, sections=[[0, 1], [1, 2]], groups=G, bins=[T, 10], headway_bins=HB,
                        tt_bins=[TB, 10], route_section=None)
    return {k: data[k] for k in gates.RAW}, data


def _encroach():
    G, H, W, window = 2, 3, 4, 6
    hist = (np.arange(G * 3 * window, dtype=np.int64).reshape(G, 3, window) * 3) % 5
    hist[1, 2] = 0                                           # a type without encounters
    critical = (np.arange(G * H * W, dtype=np.int64).reshape(G, H, W) * 2) % 3
    data = encroach.aggregates_dict(hist, critical, dict(META, x0=0.0, y0=0.0, cell=1.0, W=W, H=H, window=window, critical_records=2, groups=G))
    return dict(hist=hist, critical=critical), data


CASES = dict(fields=(fields, _fields), gates=(gates, _gates), encroach=(encroach, _encroach))


def _same(got, want, name):
    assert list(got) == list(want), (name, list(got), list(want))
    for k, v in want.items():
        if k == "meta":
            assert got[k] == v, (name, got[k], v)
        else:
            assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v, equal_nan=v.dtype.kind == "f"), (name, k)


def _stored(path):
    with np.load(path, allow_pickle=False) as f:
        return {k: (f[k].dtype.kind, f[k].shape) if k == "meta" else (f[k].dtype.str, f[k].shape) for k in sorted(f.files)}


def test_npz_files_of_the_three_observers_keep_their_format(golden_dir, tmp_path):
    for name, (mod, make) in CASES.items():
        stored, want = make()
        old_path = os.path.join(golden_dir, "npz_%s.npz" % name)
        new_path = mod.save(str(tmp_path / (name + ".npz")), want)
        _same(mod.load(old_path), want, name)
        _same(mod.load(new_path), want, name)
        assert _stored(old_path) == _stored(new_path) == dict(meta=("U", ()), **{k: ("<i8", v.shape) for k, v in stored.items()}), name
        with np.load(old_path, allow_pickle=False) as f:
            for k, v in stored.items():
                assert np.array_equal(f[k], v), (name, k)
    # the derived arrays are what the hand-made integers give
    f, g, p = (make()[1] for _, make in CASES.values())
    assert f["mean_speed"][0, 0, 0] == f["speed_q"][0, 0, 0] / 256.0 / f["visits"][0, 0, 0] and np.isnan(f["mean_speed"][1, 0, 0])
    assert np.isnan(f["occupancy_frac"][1]).all() and f["occupancy_s"][0, 1, 1] == f["occupancy"][0, 1, 1] * 0.1
    assert np.isnan(g["flow_per_hour"][1]).all() and np.isnan(g["mean_speed"][0, 1]).all() and np.isnan(g["mean_travel_s"][1, 0])
    assert np.isnan(p["critical_frac"][1, 2]) and p["critical_frac"][0, 0] == p["hist"][0, 0, :2].sum() / p["hist"][0, 0].sum()
