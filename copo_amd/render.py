"""Top-down rendering of the simulator's scenes (host side of `copo_render_*`).

`TopDownRenderer` owns one `copo_render` handle over a `VecSim`: `record()` pushes the current poses into a ring of the last
`trail` snapshots, `frames()` rasterises a batch of scenes on the GPU into a `uint8 [S, H, W, 4]` RGBA tensor.  The render rules
(paint order, colours, trail weights) are DESIGN.md section 8; `tests/render_numpy.py` restates them.  This is the reference's
`env.render(mode="top_down", num_stack=25)` (copo/vis.py); MetaDrive's own renderer is not copied pixel for pixel.
"""
import os

import numpy as np

from . import maps as _maps
from ._handle import Handle

# vehicle colours by agent id % 12 (the only copy: handed to the library at create)
PALETTE = np.array([
    (31, 119, 180), (255, 127, 14), (44, 160, 44), (148, 103, 189), (140, 86, 75), (227, 119, 194),
    (23, 190, 207), (188, 189, 34), (57, 59, 121), (0, 128, 128), (214, 156, 0), (99, 99, 255),
], np.uint8)
BACKGROUND, ROAD, LINE = (235, 235, 235), (90, 90, 90), (255, 255, 255)
BOX_SEEN, BOX_HIDDEN, WRECK = (120, 80, 50), (190, 150, 110), (220, 40, 40)
MAX_TRAIL, MAX_SIZE = 32, 4096


def map_view(tables, width, height, margin=1.05):
    """(cx, cy, metres per pixel) that fits the map's bounding box into a width x height frame."""
    x0, x1, y0, y1 = _maps.bounding_box(tables)
    m = max((x1 - x0) / width, (y1 - y0) / height) * margin
    return 0.5 * (x0 + x1), 0.5 * (y0 + y1), m


class TopDownRenderer(Handle):
    """Frames of a `VecSim`'s scenes, `width` x `height` pixels, with a trail ring of `trail` snapshots (0..32).  `close()` it
    when done (before or after its simulator; no other call once the simulator is closed); every call is asynchronous on torch's
    current stream."""

    _prefix = "copo_render_"

    def __init__(self, sim, width=512, height=512, trail=0):
        self._attach(sim)
        self.W, self.H, self.trail = int(width), int(height), int(trail)
        self._pal = np.ascontiguousarray(PALETTE)
        self._create(self._capi.lib.copo_render_create, sim._h, self.W, self.H, self.trail, self._pal.ctypes.data)
        self.recorded = 0

    def env_record(self, feed):
        """One snapshot after reset and after every step; a reset empties the trail first."""
        if feed.after_reset:
            self.clear()
        self.record()

    def record(self):
        """Push every slot's current pose / status / agent id and each scene's episode counter into the trail ring."""
        self._capi.check(self._capi.lib.copo_render_record(self._h, self._stream()))
        self.recorded = min(self.recorded + 1, self.trail)

    def clear(self):
        """Empty the trail ring (after a manual reset or set_state)."""
        self._call("clear")
        self.recorded = 0

    def views(self, scenes, view="map", m_per_px=None, follow_slot=0):
        """[S, 3] float32 (cx, cy, m) per scene: the whole map (`m_per_px` overrides the fitted scale) or centred on slot
        `follow_slot` (an int, or one per scene) at `m_per_px` (default 0.2 m per pixel)."""
        S = len(scenes)
        if view == "map":
            cx, cy, m = map_view(self.sim.tables, self.W, self.H)
            v = np.tile(np.array([cx, cy, m if m_per_px is None else m_per_px], np.float64), (S, 1))
        elif view == "follow":
            st, _ = self.sim.get_state()
            xy = st[0:2].cpu().numpy()                       # [2][E][N]
            slots = np.broadcast_to(np.asarray(follow_slot, np.int64), (S,))
            if ((slots < 0) | (slots >= self.sim.N)).any():
                raise ValueError("follow_slot outside 0..%d" % (self.sim.N - 1))
            m = 0.2 if m_per_px is None else float(m_per_px)
            v = np.stack([xy[0, scenes, slots], xy[1, scenes, slots], np.full(S, m)], 1)
        else:
            raise ValueError("view must be 'map' or 'follow', not %r" % (view,))
        return v.astype(np.float32)

    def frames(self, scenes=None, view="map", m_per_px=None, follow_slot=0, trail=None, views=None):
        """uint8 [S, H, W, 4] RGBA frames of `scenes` (default: all, in order) on the simulator's device.  `trail` = snapshots
        drawn (default: the capacity); `views` ([S, 3] cx, cy, m) overrides `view`."""
        torch = self.sim._torch
        scenes = np.arange(self.sim.E) if scenes is None else np.asarray(scenes, np.int64).reshape(-1)
        if scenes.size < 1 or scenes.size > self.sim.E or ((scenes < 0) | (scenes >= self.sim.E)).any():
            raise ValueError("scenes must be 1..%d indices in 0..%d" % (self.sim.E, self.sim.E - 1))
        trail = self.trail if trail is None else int(trail)
        v = self.views(scenes, view, m_per_px, follow_slot) if views is None else np.asarray(views, np.float32).reshape(-1, 3)
        assert v.shape == (scenes.size, 3)
        dev = self.sim.device
        sc = torch.from_numpy(scenes.astype(np.int32)).to(dev)
        vt = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
        out = torch.empty(scenes.size, self.H, self.W, dtype=torch.int32, device=dev)
        self._call("frames", sc.data_ptr(), int(scenes.size), vt.data_ptr(), trail, out.data_ptr())
        return out.view(torch.uint8).view(scenes.size, self.H, self.W, 4)


def to_numpy_rgb(frames):
    """uint8 [..., H, W, 4] RGBA (torch or numpy) -> numpy uint8 [..., H, W, 3]."""
    if hasattr(frames, "cpu"):
        frames = frames.cpu().numpy()
    return np.ascontiguousarray(np.asarray(frames)[..., :3])


def write_ppm(frames, out_dir, prefix="frame", start=0):
    """Binary PPM (P6) files `<prefix>_<start>.ppm`, ... (5 digits) of RGB(A) frames [S, H, W, 3|4] (or one [H, W, 3|4]); returns
    the paths."""
    rgb = to_numpy_rgb(frames)
    if rgb.ndim == 3:
        rgb = rgb[None]
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for k, f in enumerate(rgb):
        p = os.path.join(out_dir, "%s_%05d.ppm" % (prefix, start + k))
        with open(p, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (f.shape[1], f.shape[0]))
            fh.write(f.tobytes())
        paths.append(p)
    return paths


def read_ppm(path):
    """numpy uint8 [H, W, 3] of a binary PPM written by `write_ppm`."""
    with open(path, "rb") as fh:
        data = fh.read()
    toks, pos = [], 0
    while len(toks) < 4:             # magic, width, height, maxval; then ONE whitespace byte before the pixels
        while data[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while end < len(data) and not data[end:end + 1].isspace():
            end += 1
        toks.append(data[pos:end])
        pos = end
    if toks[0] != b"P6" or int(toks[3]) != 255:
        raise ValueError("%s is not an 8-bit binary PPM" % path)
    w, h = int(toks[1]), int(toks[2])
    return np.frombuffer(data, np.uint8, count=w * h * 3, offset=pos + 1).reshape(h, w, 3)


def write_gif(frames, path, fps=10):
    """Animated GIF of RGB(A) frames [S, H, W, 3|4]; needs PIL (Pillow), which is optional."""
    try:
        from PIL import Image
    except ImportError as err:
        raise RuntimeError("write_gif needs Pillow (PIL), which is not installed; write_ppm needs no library") from err
    rgb = to_numpy_rgb(frames)
    if rgb.ndim == 3:
        rgb = rgb[None]
    imgs = [Image.fromarray(f) for f in rgb]
    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=max(1, int(round(1000.0 / fps))), loop=0)
    return path
