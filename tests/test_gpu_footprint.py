"""One footprint under the field maps and the encroachment log (csrc/grid_common.h): over the same simulator state and the same grid, the
cells the encroachment log stamps in a record are the cells the field maps count a driving body over, scene by scene, and both are the
cells of tests/field_numpy.py's footprint.  3 scenes x 7 slots and 5 x 64, random poses, a 32 x 32 grid of 1 m cells that cuts bodies
off at its edges, one scene group per scene on the field maps.  Every comparison is on sets of cells: exact.

`field_numpy.footprint` is float64 and names the cells whose centre lies within 1e-3 m of a body's edge apart (fp32 cannot decide them
the same way: an ulp of the coordinates is 1e-5 m): the device's cells hold every sure cell and nothing but sure and ambiguous ones; among
the ambiguous ones `pet_numpy.cells`, the fp32 rule operation for operation on those candidates, decides, and the device equals it."""
import numpy as np
import pytest

import field_numpy as fn
import interact_cases as ic
import pet_numpy as pn
from rowlog_gpu import _np_state, _set_state, _sim64

pytestmark = pytest.mark.gpu

W = H = 32


@pytest.mark.parametrize("E,N,x0,y0", [(3, 7, 60.0, -40.0), (5, 64, 84.0, -16.0)])
def test_stamped_cells_are_the_occupied_cells(E, N, x0, y0):
    import torch
    from copo_amd.encroach import EncroachmentLog
    from copo_amd.fields import FieldMaps
    sim = _sim64(E, N)
    maps = log = None
    try:
        sim.reset()
        st0, env0 = _np_state(sim)
        st = ic.random_state(st0, seed=5)
        _set_state(sim, st, env0)
        hl, hw = sim.cfg.veh_half_len, sim.cfg.veh_half_wid
        maps = FieldMaps(sim, x0, y0, W, H, cell=1.0, groups=E)
        maps.set_groups(np.arange(E))
        log = EncroachmentLog(sim, x0, y0, W, H, cell=1.0, max_rows=64)
        assert maps.grid == log.grid == (x0, y0, 1.0)
        maps.record()
        log.record()
        occupancy = maps.maps()[0][:, 0].cpu().numpy()                        # [G = E, H, W]
        stamps = log.memory()[0]                                              # [E, H, W]
        torch.cuda.synchronize()
        assert ((stamps >> np.uint64(32)) <= 1).all()                         # record 0 writes record field 1; nothing else is there
        grid = fn.Grid(x0, y0, W, H, 1.0)
        status = st.view(np.int32)[13] & 0xFF
        clipped = covered = 0
        for e in range(E):
            sure, maybe, exact = set(), set(), set()
            for n in np.nonzero(status[e] == fn.ST_ALIVE)[0]:
                pose = (st[0, e, n], st[1, e, n], st[2, e, n])
                s, a = fn.footprint(*pose, grid, hl, hw)
                s, a = set((s[0] * W + s[1]).tolist()), set((a[0] * W + a[1]).tolist())
                c = set(pn.cells(*pose, grid, hl, hw).tolist())
                assert s <= c <= s | a, (e, n)
                sure |= s
                maybe |= s | a
                exact |= c
                inside = (x0 + hl + hw < pose[0] < x0 + W - hl - hw) and (y0 + hl + hw < pose[1] < y0 + H - hl - hw)
                clipped += bool(c) and not inside
            stamped = set(np.nonzero(stamps[e].reshape(-1))[0].tolist())
            occupied = set(np.nonzero(occupancy[e].reshape(-1) > 0)[0].tolist())
            assert stamped == occupied, (e, sorted(stamped ^ occupied))
            assert sure <= stamped <= maybe and stamped == exact, (e, sorted(stamped ^ exact))
            covered += len(stamped)
        assert covered >= 8 * E and clipped >= 1, (covered, clipped)        # the premises: bodies on the grid, one cut off by its edge
    finally:
        for h in (maps, log):
            if h is not None:
                h.close()
        sim.close()
