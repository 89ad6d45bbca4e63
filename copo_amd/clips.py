"""Event clips: a flight recorder over the simulator's scenes and its playback (host side of `copo_clip_*`).

`ClipRecorder` owns one `copo_clip` handle over a `VecSim`.  `record()` snapshots, on the GPU, what the renderer and the interaction
meter read of every scene into that scene's ring of the last `pre + post + 1` records; when a chosen flag, a small time to collision or
a small gap fires in a scene, the lead-up, the event and `post` records after it are committed as one clip into a pool of `max_clips`
-- in scene order, without host synchronisation.  `clips()` reads the pool out as a `ClipSet` (numpy only; `save` / `load` one
`.npz`), and `ClipPlayer` plays a clip set back into a simulator handle of its own that is never stepped: `TopDownRenderer` and
`InteractionMeter` work on it unchanged and give the bits they gave live.  The rules are DESIGN.md section 8c; `tests/clip_numpy.py`
restates them.
"""
import ctypes as C
import dataclasses

import numpy as np

from ._abi import CLIP_HEADER as HEADER, CLIP_MAX_CAP as MAX_CAP, CLIP_WORDS as WORDS
from . import _npz
from ._handle import Handle

HEADER_KEYS = ("scene", "first_rec", "length", "trig_rec", "trig_slot", "kind", "trig_aid", "n_events")
KIND_FLAG, KIND_TTC, KIND_GAP = 1, 2, 4
KINDS = dict(flag=KIND_FLAG, ttc=KIND_TTC, gap=KIND_GAP)
# trigger flags by name: the COPO_F_* bits of the step's `flags` output
FLAG_BITS = dict(acted=0x01, done=0x02, arrive=0x04, crash=0x08, out=0x10, maxstep=0x20, spawned=0x40, env_reset=0x80)


def flag_mask(flags):
    """Bit mask of flag names (`FLAG_BITS`) or of an int."""
    if isinstance(flags, (int, np.integer)):
        mask = int(flags)
    else:
        unknown = [f for f in flags if f not in FLAG_BITS]
        if unknown:
            raise ValueError("unknown trigger flags %r (known: %s)" % (unknown, ", ".join(FLAG_BITS)))
        mask = 0
        for f in flags:
            mask |= FLAG_BITS[f]
    if not 0 <= mask <= 0xFF:
        raise ValueError("flag mask 0x%x outside the COPO_F_* bits" % mask)
    return mask


class ClipSet:
    """Clips as numpy arrays: `header` int32 [C, 8] (columns `HEADER_KEYS`), `snaps` uint32 [C, cap, 6, N] (x, y, heading, speed as
    raw float bits, status byte, agent id; frames beyond a clip's length are 0), `envw` int32 [C, cap, 2] (t_env, episode) and
    `meta`: `pre`, `post`, `dt`, `hl`, `hw`, `num_agents` and `sim_config`, the `SimConfig` fields that rebuild the map."""

    def __init__(self, header, snaps, envw, meta):
        self.header = np.ascontiguousarray(header, np.int32).reshape(-1, HEADER)
        self.snaps = np.ascontiguousarray(snaps, np.uint32)
        self.envw = np.ascontiguousarray(envw, np.int32)
        self.meta = dict(meta)
        C_ = len(self.header)
        assert self.snaps.ndim == 4 and self.snaps.shape[0] == C_ and self.snaps.shape[2] == WORDS, self.snaps.shape
        assert self.envw.shape == (C_, self.snaps.shape[1], 2), self.envw.shape
        assert self.cap == self.meta["pre"] + self.meta["post"] + 1

    def __len__(self):
        return len(self.header)

    cap = property(lambda self: self.snaps.shape[1])
    N = property(lambda self: self.snaps.shape[3])
    # float views of the first four words [C, cap, N], and the integer ones
    x = property(lambda self: self.snaps[:, :, 0].view(np.float32))
    y = property(lambda self: self.snaps[:, :, 1].view(np.float32))
    heading = property(lambda self: self.snaps[:, :, 2].view(np.float32))
    speed = property(lambda self: self.snaps[:, :, 3].view(np.float32))
    status = property(lambda self: self.snaps[:, :, 4])
    agent_id = property(lambda self: self.snaps[:, :, 5].view(np.int32))

    def column(self, key):
        return self.header[:, HEADER_KEYS.index(key)]

    def info(self, c):
        """Header of clip `c` as a dict."""
        return {k: int(v) for k, v in zip(HEADER_KEYS, self.header[c])}

    def select(self, kind=None, scene=None):
        """The clips whose trigger kind has any of `kind` ("flag" / "ttc" / "gap", a list of those, or the bits) and whose scene is
        (in) `scene`, as a new `ClipSet`."""
        keep = np.ones(len(self), bool)
        if kind is not None:
            names = [kind] if isinstance(kind, (str, int, np.integer)) else list(kind)
            mask = 0
            for k in names:
                mask |= KINDS[k] if isinstance(k, str) else int(k)
            keep &= (self.column("kind") & mask) != 0
        if scene is not None:
            keep &= np.isin(self.column("scene"), np.asarray(scene, np.int64).reshape(-1))
        return ClipSet(self.header[keep], self.snaps[keep], self.envw[keep], self.meta)

    def save(self, path):
        """One `.npz` without pickled objects (`np.load(path, allow_pickle=False)` reads it)."""
        return _npz.save(path, self.meta, header=self.header, snaps=self.snaps, envw=self.envw)

    @classmethod
    def load(cls, path):
        return cls(*_npz.load(path, "header", "snaps", "envw"))

    def sim_config(self, num_envs=1):
        """`SimConfig` of the recorded map with `num_envs` scenes."""
        from .sim import SimConfig
        kw = dict(self.meta["sim_config"])
        kw.update(num_envs=int(num_envs), num_agents=int(self.meta["num_agents"]))
        return SimConfig(**kw)


def clip_meta(cfg, N, pre, post):
    """`ClipSet.meta` of a recorder over a simulator of `SimConfig` `cfg` with `N` slots."""
    return dict(pre=int(pre), post=int(post), dt=float(cfg.dt), hl=float(cfg.veh_half_len), hw=float(cfg.veh_half_wid), num_agents=int(N),
                sim_config=dataclasses.asdict(cfg))


class ClipRecorder(Handle):
    """Flight recorder of a `VecSim`: clips of `pre` records before and `post` after the record in which a scene fires -- a slot whose
    step flags contain one of `flags` (names of `FLAG_BITS`, or the bits), whose TTC is below `ttc_below` seconds or whose gap is
    below `gap_below` metres (0: off) --, at most `max_clips` of them (later ones are counted as dropped).  `close()` it when done
    (before or after its simulator; no other call once the simulator is closed); every call is asynchronous on torch's current stream
    except `count()` / `clips()`."""

    _prefix = "copo_clip_"

    def __init__(self, sim, pre=24, post=8, max_clips=256, flags=("crash",), ttc_below=0.0, gap_below=0.0):
        self._attach(sim)
        self.pre, self.post, self.max_clips = int(pre), int(post), int(max_clips)
        self.flag_mask, self.ttc_below, self.gap_below = flag_mask(flags), float(ttc_below), float(gap_below)
        cfg = self._capi.ClipCfg(self.pre, self.post, self.max_clips, self.flag_mask, self.ttc_below, self.gap_below)
        self._create(self._capi.lib.copo_clip_create, sim._h, C.byref(cfg))
        self.cap = self.pre + self.post + 1

    @classmethod
    def from_env(cls, sim, value):
        """The env's recorder (config key `event_clips`: None, or the arguments of `ClipRecorder`)."""
        return cls(sim, **dict(value))

    def env_record(self, feed):
        """One record of the state after reset and after every step, fed with the step's flags and, for the ttc / gap triggers, the
        meter's arrays of that state.  Clips are kept over resets; a clip still waiting for its `post` records when the scenes are
        reset by hand is committed with what it has."""
        if feed.after_reset and feed.records > 0:
            self.flush()
        self.record(flags=feed.flags, ttc=feed.ttc if self.ttc_below > 0.0 else None, gap=feed.gap if self.gap_below > 0.0 else None)

    def record(self, flags=None, ttc=None, gap=None):
        """Snapshot the current state of every scene; `flags` (uint8 [E, N], the step's output) and `ttc` / `gap` (float32 [E, N],
        `InteractionMeter.record()`'s) feed the triggers of this record, None switches one off for the call."""
        torch = self.sim._torch
        self._capi.check(self._capi.lib.copo_clip_record(self._h, self._en_arg(flags, torch.uint8, "flags"), self._en_arg(ttc, torch.float32, "ttc"),
                                                         self._en_arg(gap, torch.float32, "gap"), self._stream()))

    def flush(self):
        """Commit the clips of the scenes that are still waiting for their `post` records, with what they have."""
        self._call("flush")

    def count(self):
        """(clips stored, clips dropped); waits for the stream."""
        n, d = C.c_int32(), C.c_int32()
        self._call("count", C.byref(n), C.byref(d))
        return n.value, d.value

    def clips(self):
        """The stored clips as a `ClipSet`."""
        torch = self.sim._torch
        n, _ = self.count()
        dev, N = self.sim.device, self.sim.N
        header = torch.empty(n, HEADER, dtype=torch.int32, device=dev)
        snaps = torch.empty(n, self.cap, WORDS, N, dtype=torch.int32, device=dev)
        envw = torch.empty(n, self.cap, 2, dtype=torch.int32, device=dev)
        if n:
            self._call("read", 0, n, header.data_ptr(), snaps.data_ptr(), envw.data_ptr())
        return ClipSet(header.cpu().numpy(), snaps.cpu().numpy().view(np.uint32), envw.cpu().numpy(),
                       clip_meta(self.sim.cfg, N, self.pre, self.post))

    def reset(self):
        """Forget every clip, counter and waiting scene; records count from 0 again."""
        self._call("reset")


class ClipPlayer:
    """Playback of a `ClipSet` on GPU `device`: a `VecSim` on the clip set's map (`num_envs` scenes) that is never stepped, into which
    `seek` writes frames of clips; `render` and `interaction` run the renderer and the interaction meter on it.  `close()` when done."""

    def __init__(self, clipset, device=0, num_envs=1):
        import torch
        from .sim import VecSim
        self.clips, self._torch = clipset, torch
        self.sim = VecSim(clipset.sim_config(num_envs), device=device, with_info=False)
        assert self.sim.N == clipset.N
        self._snaps = torch.from_numpy(clipset.snaps.view(np.int32)).to(self.sim.device)
        self._envw = torch.from_numpy(clipset.envw).to(self.sim.device)
        self._renderer = self._meter = None

    def seek(self, clip_ids, frame):
        """Frame `frame` (one for all, or one per clip; -1: an all-EMPTY scene) of clip `clip_ids[j]` becomes scene j of the player's
        simulator."""
        capi, torch = self.sim._capi, self._torch
        ids = np.asarray(clip_ids, np.int64).reshape(-1)
        frames = np.broadcast_to(np.asarray(frame, np.int64), ids.shape)
        if ids.size < 1 or ids.size > self.sim.E:
            raise ValueError("1..%d clips at a time (the player's num_envs), not %d" % (self.sim.E, ids.size))
        if ((ids < 0) | (ids >= len(self.clips))).any():
            raise ValueError("clip ids outside 0..%d" % (len(self.clips) - 1))
        if ((frames < -1) | (frames >= self.clips.column("length")[ids])).any():
            raise ValueError("frame outside its clip (lengths %s)" % self.clips.column("length")[ids].tolist())
        ci = torch.from_numpy(ids.astype(np.int32)).to(self.sim.device)
        fi = torch.from_numpy(np.ascontiguousarray(frames, np.int32)).to(self.sim.device)
        capi.check(capi.lib.copo_clip_scatter(self.sim._h, self._snaps.data_ptr(), self._envw.data_ptr(), self.clips.cap, self.clips.N,
                                              ci.data_ptr(), fi.data_ptr(), int(ids.size), self.sim._stream()))

    def render(self, clip, trail=25, film_size=(512, 512), view="map", m_per_px=None, follow_slot=None):
        """numpy uint8 [length, H, W, 4] RGBA frames of clip `clip` (`film_size` = (width, height)): the whole map, or centred on slot
        `follow_slot` (default: the slot that triggered).  Per frame: seek, `TopDownRenderer.record()`, `frames()` with the last
        `trail` recorded poses (at most 32) as the trail -- a clip's first frames have fewer."""
        from .render import MAX_TRAIL, TopDownRenderer
        W, H = int(film_size[0]), int(film_size[1])
        r = self._renderer
        if r is None or (r.W, r.H) != (W, H):
            if r is not None:
                r.close()
            self._renderer = r = TopDownRenderer(self.sim, W, H, trail=MAX_TRAIL)
        r.clear()
        info = self.clips.info(clip)
        slot = info["trig_slot"] if follow_slot is None else int(follow_slot)
        out = np.empty((info["length"], H, W, 4), np.uint8)
        for k in range(info["length"]):
            self.seek([clip], k)
            r.record()
            out[k] = r.frames(scenes=[0], view=view, m_per_px=m_per_px, follow_slot=slot, trail=max(0, min(int(trail), MAX_TRAIL))).cpu().numpy()[0]
        return out

    def interaction(self, clip, **meter_kwargs):
        """dict(gap, ttc): float32 [length, N] per frame of clip `clip`, measured by an `InteractionMeter(**meter_kwargs)` on the
        player's simulator."""
        from .interact import InteractionMeter
        if self._meter is None or self._meter_kwargs != meter_kwargs:
            if self._meter is not None:
                self._meter.close()
            self._meter, self._meter_kwargs = InteractionMeter(self.sim, **meter_kwargs), dict(meter_kwargs)
        self._meter.reset()
        length = self.clips.info(clip)["length"]
        gap, ttc = np.empty((length, self.clips.N), np.float32), np.empty((length, self.clips.N), np.float32)
        for k in range(length):
            self.seek([clip], k)
            g, t = self._meter.record()
            gap[k], ttc[k] = g[0].cpu().numpy(), t[0].cpu().numpy()
        return dict(gap=gap, ttc=ttc)

    def close(self):
        for name in ("_renderer", "_meter"):
            if getattr(self, name, None) is not None:
                getattr(self, name).close()
                setattr(self, name, None)
        if getattr(self, "sim", None) is not None:
            self.sim.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
