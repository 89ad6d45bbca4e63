"""The grid of cells per scene of `FieldMaps` and `EncroachmentLog` on the host (the device side is `csrc/grid_common.h`).  DESIGN.md 8e."""
import numpy as np


class SceneGrid:
    """Mixin of a handle whose `__init__(sim, x0, y0, W, H, cell=..., ...)` hands a grid of `W` x `H` cells of `cell` metres to `_set_grid`."""

    def _set_grid(self, x0, y0, W, H, cell):        # (the origin and the cell size as the library gets them: rounded to float32)
        self.x0, self.y0, self.cell = float(np.float32(x0)), float(np.float32(y0)), float(np.float32(cell))
        self.W, self.H = int(W), int(H)

    grid = property(lambda self: (self.x0, self.y0, self.cell))

    @classmethod
    def for_map(cls, sim, cell=1.0, margin=5.0, **kwargs):
        """Grid over the bounding box of the simulator's road tables plus `margin` metres."""
        from .fields import grid_for_map
        x0, y0, W, H = grid_for_map(sim.tables, cell, margin)
        return cls(sim, x0, y0, W, H, cell=cell, **kwargs)

    @classmethod
    def from_env(cls, sim, value):
        """The env's handle from the arguments of the class: with x0, y0, W, H an explicit grid, else `for_map`."""
        kwargs = dict(value or {})
        explicit = all(k in kwargs for k in ("x0", "y0", "W", "H"))
        return cls(sim, **kwargs) if explicit else cls.for_map(sim, **kwargs)

    def heat_overlay(self, frame_rgb, layer2d, view, lo=None, hi=None, alpha=160):
        from .fields import heat_overlay
        return heat_overlay(frame_rgb, layer2d, view, lo, hi, alpha, grid=self.grid)
