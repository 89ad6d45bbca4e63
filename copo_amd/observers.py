"""The env's observers of its simulator: one table of config keys, one protocol, one list that drives them.

An observer is a `Handle` over a `VecSim` that takes one record of the state after every reset and every step.  Its module holds two
methods for the env: `from_env(sim, value)` builds it from the value of its config key, and `env_record(feed)` makes that one record
from a `Feed`, with whatever a reset by hand means to it.  `ENV_OBSERVERS` names the keys in record order; a new observer is one row
here and those two methods there.
"""
import importlib
from collections import namedtuple

Row = namedtuple("Row", "key default module cls")

# in record order: the meter first, because the observers after it read its arrays of the same state
ENV_OBSERVERS = (
    Row("interaction_metrics", False, "copo_amd.interact", "InteractionMeter"),   # gaps, time to collision, near misses of every step
    Row("event_clips", None, "copo_amd.clips", "ClipRecorder"),                   # clips of the records around a crash / near miss
    Row("rewind", None, "copo_amd.rewind", "RewindBuffer"),                       # ring of full snapshots per scene to fork past records from
    Row("field_maps", None, "copo_amd.fields", "FieldMaps"),                      # occupancy, speed, flow and event grids over scenes and steps
    Row("traffic_gates", None, "copo_amd.gates", "TrafficGates"),                 # line-crossing counts, headways and travel times per gate
    Row("trip_log", None, "copo_amd.trips", "TripLog"),                           # one device-written row per finished agent
)
METER, CLIPS, REWIND = "interaction_metrics", "event_clips", "rewind"


def _on(row, cfg):
    v = cfg.get(row.key, row.default)
    return bool(v) if row.default is False else v is not None


class Feed:
    """What one record is made from: `flags` / `rew`, the step's tensors (None after a reset); `gap` / `ttc`, the meter's tensors of
    this state (None without a meter); `after_reset`; `records`, the records the list has made so far, this one not included."""
    __slots__ = ("flags", "rew", "gap", "ttc", "after_reset", "records")

    def __init__(self, flags=None, rew=None, gap=None, ttc=None, after_reset=False, records=0):
        self.flags, self.rew, self.gap, self.ttc, self.after_reset, self.records = flags, rew, gap, ttc, after_reset, records


class ObserverList:
    """The observers that the env config `cfg` switches on over `sim`, built and recorded in `ENV_OBSERVERS` order."""

    @classmethod
    def validate(cls, cfg):
        """The config errors that can be told before the simulator exists."""
        if cfg.get(METER, False):
            return
        clips, fields = dict(cfg.get(CLIPS) or {}), dict(cfg.get("field_maps") or {})
        if clips.get("ttc_below", 0.0) > 0.0 or clips.get("gap_below", 0.0) > 0.0:
            raise ValueError("event_clips with ttc_below / gap_below reads the interaction meter: set interaction_metrics=True")
        if fields.get("ttc_below", 0.0) > 0.0:
            raise ValueError("field_maps with ttc_below reads the interaction meter: set interaction_metrics=True")

    def __init__(self, sim, cfg):
        self._members = []             # (name, observer) in record order
        self.records = 0
        for row in ENV_OBSERVERS:
            if _on(row, cfg):
                cls = getattr(importlib.import_module(row.module), row.cls)
                self._members.append((row.key, cls.from_env(sim, cfg[row.key])))

    def names(self):
        """The members' names in record order."""
        return [name for name, _ in self._members]

    def get(self, key):
        """The observer of `key`, None when it is off."""
        for name, o in self._members:
            if name == key:
                return o
        return None

    def add_first(self, name, observer):
        """`observer` records ahead of the rest from now on; one of that name already in the list is closed and replaced."""
        old = self.get(name)
        if old is not None:
            old.close()
        self._members = [(name, observer)] + [m for m in self._members if m[0] != name]

    def add(self, name, observer):
        """`observer` records after the rest from now on; one of that name already in the list is closed and replaced."""
        old = self.get(name)
        if old is not None:
            old.close()
        self._members = [m for m in self._members if m[0] != name] + [(name, observer)]

    def after_reset(self):
        self._record(Feed(after_reset=True, records=self.records))

    def after_step(self, out):
        self._record(Feed(flags=out["flags"], rew=out["rew"], records=self.records))

    def _record(self, feed):
        meter = self.get(METER)
        if meter is not None:          # the tensors are the meter's own, written by its record ahead of every observer that reads them
            feed.gap, feed.ttc = meter.gap, meter.ttc
        for _, o in self._members:
            o.env_record(feed)
        self.records += 1
        rewind = self.get(REWIND)
        if rewind is not None and self.get(CLIPS) is not None:
            # a clip header's first_rec / trig_rec name rewind records: both count the list's records
            assert rewind.n_records == self.records, (rewind.n_records, self.records)

    def close(self):
        members, self._members = self._members, []
        for _, o in members:
            o.close()
