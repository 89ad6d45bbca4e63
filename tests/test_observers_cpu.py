"""The env's observer list without a GPU (copo_amd/observers.py): `ObserverList` over a stub simulator with the table pointed at fake
classes that log their calls, and every real observer's `env_record` against a stub of its own methods."""
import sys
import types

import pytest

from copo_amd import observers as ob

KEYS = ("interaction_metrics", "event_clips", "rewind", "field_maps", "traffic_gates", "trip_log")
ALL_ON = dict(interaction_metrics=True, event_clips=dict(pre=1), rewind=dict(depth=2), field_maps=dict(cell=2.0), traffic_gates={}, trip_log={})


def test_table_and_defaults():
    from copo_amd.torch_copo.utils.env_wrappers import MultiAgentIntersectionEnv
    assert tuple(r.key for r in ob.ENV_OBSERVERS) == KEYS
    assert [r.default for r in ob.ENV_OBSERVERS] == [False, None, None, None, None, None]
    cfg = MultiAgentIntersectionEnv.default_config()
    assert [cfg[k] for k in KEYS] == [False, None, None, None, None, None]
    assert "torch" not in vars(ob)


@pytest.fixture
def fakes(monkeypatch):
    """The table with one fake class per key; `log` takes (name, call, argument) of everything the list does to them."""
    log = []
    mod = types.ModuleType("fake_observers")

    def make(key):
        class Fake:
            name = key
            gap, ttc = "gap of " + key, "ttc of " + key
            n_records = 0

            @classmethod
            def from_env(cls, sim, value):
                log.append((key, "from_env", (sim, value)))
                return cls()

            def env_record(self, feed):
                self.n_records += 1
                log.append((self.name, "env_record", feed))

            def close(self):
                log.append((self.name, "close", None))
        return Fake
    rows = []
    for row in ob.ENV_OBSERVERS:
        setattr(mod, row.cls, make(row.key))
        rows.append(ob.Row(row.key, row.default, "fake_observers", row.cls))
    monkeypatch.setitem(sys.modules, "fake_observers", mod)
    monkeypatch.setattr(ob, "ENV_OBSERVERS", tuple(rows))
    return log, make


def test_build_record_close_in_table_order(fakes):
    log, make = fakes
    lst = ob.ObserverList("sim", dict(ALL_ON))
    assert [(n, c) for n, c, _ in log] == [(k, "from_env") for k in KEYS]
    assert [a for _, _, a in log] == [("sim", ALL_ON[k]) for k in KEYS]
    assert all(lst.get(k).name == k for k in KEYS) and lst.get("renderer") is None
    del log[:]
    lst.after_reset()
    assert [(n, c) for n, c, _ in log] == [(k, "env_record") for k in KEYS]
    feed = log[0][2]
    assert all(f is feed for _, _, f in log)                       # one Feed for every member
    assert feed.after_reset and feed.flags is None and feed.rew is None and feed.records == 0
    assert (feed.gap, feed.ttc) == ("gap of interaction_metrics", "ttc of interaction_metrics")
    del log[:]
    lst.after_step(dict(flags="F", rew="R", obs="O"))
    feed = log[-1][2]
    assert not feed.after_reset and (feed.flags, feed.rew, feed.records) == ("F", "R", 1) and feed.gap == "gap of interaction_metrics"
    # the renderer, made late, goes first; another one of that name replaces it and closes it
    r1, r2 = make("renderer")(), make("renderer")()
    lst.add_first("renderer", r1)
    del log[:]
    lst.after_reset()
    assert [n for n, _, _ in log] == ["renderer"] + list(KEYS)
    assert log[0][2].after_reset and log[0][2].records == 2 and log[0][2].flags is None      # the count goes on over a reset
    del log[:]
    lst.add_first("renderer", r2)
    assert log == [("renderer", "close", None)] and lst.get("renderer") is r2
    lst.after_step(dict(flags="F", rew="R"))
    assert [n for n, _, _ in log[1:]] == ["renderer"] + list(KEYS) and lst.records == 4
    del log[:]
    lst.close()
    assert sorted(log) == sorted((k, "close", None) for k in KEYS + ("renderer",))           # each member once
    assert all(lst.get(k) is None for k in KEYS + ("renderer",))
    lst.close()
    assert len(log) == len(KEYS) + 1                               # the second close does nothing


def test_keys_that_are_off(fakes):
    log, _ = fakes
    lst = ob.ObserverList("sim", dict(interaction_metrics=False, event_clips=None, trip_log={}))      # (an empty dict is on)
    assert [(n, c) for n, c, _ in log] == [("trip_log", "from_env")]
    assert lst.get("interaction_metrics") is None and lst.get("rewind") is None and lst.get("trip_log") is not None
    lst.after_reset()
    lst.after_step(dict(flags="F", rew="R"))
    feeds = [f for _, c, f in log if c == "env_record"]
    assert [(f.gap, f.ttc, f.records) for f in feeds] == [(None, None, 0), (None, None, 1)]
    empty = ob.ObserverList("sim", {})
    empty.after_reset()
    empty.after_step(dict(flags="F", rew="R"))
    empty.close()
    assert len(log) == 3


def test_clips_and_rewind_count_the_same_records(fakes):
    lst = ob.ObserverList("sim", dict(event_clips={}, rewind={}))
    lst.after_reset()
    lst.after_step(dict(flags="F", rew="R"))
    lst.get("rewind").n_records += 1                               # a record behind the list's back
    with pytest.raises(AssertionError):
        lst.after_step(dict(flags="F", rew="R"))


@pytest.mark.parametrize("cfg, text", [
    (dict(event_clips=dict(ttc_below=1.0)), "event_clips with ttc_below / gap_below reads the interaction meter: set interaction_metrics=True"),
    (dict(event_clips=dict(gap_below=0.5)), "event_clips with ttc_below / gap_below reads the interaction meter: set interaction_metrics=True"),
    (dict(field_maps=dict(ttc_below=1.5)), "field_maps with ttc_below reads the interaction meter: set interaction_metrics=True"),
])
def test_validate(fakes, monkeypatch, cfg, text):
    log, _ = fakes
    with pytest.raises(ValueError) as e:
        ob.ObserverList.validate(cfg)
    assert str(e.value) == text
    ob.ObserverList.validate(dict(cfg, interaction_metrics=True))
    ob.ObserverList.validate(dict(event_clips=dict(pre=2), field_maps={}, rewind=None))
    # the env raises it before it creates anything
    from copo_amd.torch_copo.utils import env_wrappers as W

    def no_sim(*a, **k):
        raise AssertionError("the simulator was created")
    monkeypatch.setattr(W, "VecSim", no_sim)
    with pytest.raises(ValueError) as e:
        W.MultiAgentIntersectionEnv(cfg)
    assert str(e.value) == text and log == []


# ---- every real observer's reset rule, against a stub of its own methods ----
def _stub(log, **attrs):
    s = types.SimpleNamespace(**attrs)
    for name in ("record", "reset", "clear", "flush", "invalidate", "forget"):
        setattr(s, name, lambda *a, _n=name, **k: log.append((_n, a, k)))
    return s


def _calls(cls, feed, **attrs):
    log = []
    cls.env_record(_stub(log, **attrs), feed)
    return log


RESET0, RESET5 = ob.Feed(after_reset=True, records=0, gap="G", ttc="T"), ob.Feed(after_reset=True, records=5, gap="G", ttc="T")
STEP = ob.Feed(flags="F", rew="R", gap="G", ttc="T", records=3)


def test_env_record_of_the_meter_and_the_renderer():
    from copo_amd.interact import InteractionMeter
    from copo_amd.render import TopDownRenderer
    assert [c[0] for c in _calls(InteractionMeter, RESET0)] == ["reset", "record"]
    assert [c[0] for c in _calls(InteractionMeter, STEP)] == ["record"]
    assert [c[0] for c in _calls(TopDownRenderer, RESET5)] == ["clear", "record"]
    assert [c[0] for c in _calls(TopDownRenderer, STEP)] == ["record"]


def test_env_record_of_the_clips():
    from copo_amd.clips import ClipRecorder
    on, off = dict(ttc_below=1.0, gap_below=0.5), dict(ttc_below=0.0, gap_below=0.0)
    assert _calls(ClipRecorder, RESET0, **on) == [("record", (), dict(flags=None, ttc="T", gap="G"))]      # nothing to flush yet
    assert _calls(ClipRecorder, RESET5, **off) == [("flush", (), {}), ("record", (), dict(flags=None, ttc=None, gap=None))]
    assert _calls(ClipRecorder, STEP, ttc_below=1.0, gap_below=0.0) == [("record", (), dict(flags="F", ttc="T", gap=None))]


def test_env_record_of_the_rewind():
    from copo_amd.rewind import RewindBuffer
    assert [c[0] for c in _calls(RewindBuffer, RESET5, n_records=0)] == ["record"]       # its own count decides, not the list's
    assert [c[0] for c in _calls(RewindBuffer, RESET0, n_records=4)] == ["invalidate", "record"]
    assert [c[0] for c in _calls(RewindBuffer, STEP, n_records=4)] == ["record"]


def test_env_record_of_fields_gates_trips():
    from copo_amd.fields import FieldMaps
    from copo_amd.gates import TrafficGates
    from copo_amd.trips import TripLog
    assert _calls(FieldMaps, RESET5, ttc_below=1.5) == [("record", (), dict(flags=None, ttc="T"))]
    assert _calls(FieldMaps, STEP, ttc_below=0.0) == [("record", (), dict(flags="F", ttc=None))]
    assert _calls(TrafficGates, RESET0) == [("forget", (), {}), ("record", (), {})]
    assert _calls(TrafficGates, STEP) == [("record", (), {})]
    assert _calls(TripLog, ob.Feed(after_reset=True)) == [("record", (), dict(flags=None, rew=None, gap=None, ttc=None))]
    assert _calls(TripLog, STEP) == [("record", (), dict(flags="F", rew="R", gap="G", ttc="T"))]


def test_from_env_rules():
    from copo_amd.fields import FieldMaps
    from copo_amd.gates import TrafficGates
    from copo_amd.interact import InteractionMeter
    from copo_amd.trips import TripLog

    def spy(base):
        class Spy(base):
            def __init__(self, *a, **k):
                self.made = ("init", a, k)

            @classmethod
            def for_map(cls, *a, **k):
                self = cls()
                self.made = ("for_map", a, k)
                return self

            def close(self):
                pass
        return Spy
    assert spy(FieldMaps).from_env("sim", dict(cell=2.0)).made == ("for_map", ("sim",), dict(cell=2.0))
    assert spy(FieldMaps).from_env("sim", dict(x0=0.0, y0=0.0, W=4, H=4)).made == ("init", ("sim",), dict(x0=0.0, y0=0.0, W=4, H=4))
    assert spy(FieldMaps).from_env("sim", dict(x0=0.0, y0=0.0, W=4)).made[0] == "for_map"
    assert spy(TrafficGates).from_env("sim", dict(inset=30.0)).made == ("for_map", ("sim",), dict(inset=30.0))
    assert spy(TrafficGates).from_env("sim", dict(gates=[[0, 0, 1, 1]])).made == ("init", ("sim",), dict(gates=[[0, 0, 1, 1]]))
    assert spy(TripLog).from_env("sim", dict(max_rows=8)).made == ("init", ("sim",), dict(max_rows=8))
    assert spy(InteractionMeter).from_env("sim", True).made == ("init", ("sim",), {})
