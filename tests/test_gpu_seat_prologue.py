"""The tile prologue the four seat passes share (csrc/learn_seat.inc), on the one path where it alone decides the result: a row list
whose last tile is partial and holds an index outside [0, n_out).  The case is the smallest of tests/adversary_cases.py -- hidden 64,
observation width 91, 48 rows, member 2's seventeen listed rows -- with the seventeenth index set to n_out.  That slot is no row: its
tile (the slot alone) writes nothing.  Two comparisons per pass:

* against the numpy model of the pass (adversary_numpy, pgd_numpy, certify_numpy, linbound_numpy) run on the SAME list, bad index
  included: the rows it writes, and their values as the pass's own test file compares them -- the PGD pass bit for bit (the model
  follows the signs of the kernel's trace), the one-step pass's `obs_seen` bit for bit from the kernel's own gradient and that gradient
  within the case's tau of the float64 model, the two bound passes within their case's tau of the float64 model (tau = 4 x the
  deviation of torch fp32 from float64: tests/adversary_cases.py, certify_cases.py, linbound_cases.py);
* against a second launch of the same kernel on the sixteen valid rows alone, bit for bit on every output, one guard row behind n_out
  included.  This reference is the kernel itself, not an independent one: it shows that the slot changes nothing else."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adversary_cases as ac
import adversary_numpy as an
import certify_cases as cc
import certify_numpy as cz
import linbound_cases as lc
import linbound_numpy as lz
import pgd_cases as pc
import pgd_numpy as pn

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

POISON = 0x7FC0DEAD      # a NaN with a payload: what a kernel did not write
HIDDEN, IN_DIM, N_OUT = 64, 91, ac.E * ac.N
PASSES = ("adversary", "pgd", "interval", "linear")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(*tail):
    """A poisoned output of n_out rows with one more row behind it: (what the launch gets, the whole buffer)."""
    whole = torch.full((N_OUT + 1,) + tail, POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    return whole[:N_OUT], whole


def _launch(which, bank, rows, counts):
    """One launch of pass `which` over the lists; its two output buffers (guard rows included) as float32 numpy."""
    pb = SimpleNamespace(K=ac.K, G=ac.G, N=ac.N, E=ac.E, cap=ac.CAP, n_out=N_OUT, rows=_dev(rows), counts=_dev(counts),
                         group=_dev(ac.GROUP if which == "adversary" else pc.GROUP))
    lv = lambda level_of, words: SimpleNamespace(K=ac.K, G=ac.G, L=len(words), level_of=_dev(level_of), levels=_dev(words), max_iters=pc.MAX_ITERS)  # noqa: E731
    obs = _dev(ac.observations(IN_DIM))
    if which == "adversary":
        (a, wa), (b, wb) = _guarded(IN_DIM), _guarded(IN_DIM)
        bank.perturb_seats(pb, lv(ac.LEVEL_OF["A"], ac.LEVELS), obs, a, ac.COL_LO, ac.COL_HI, grad=b)
    elif which == "pgd":
        (a, wa), wb = _guarded(IN_DIM), torch.full((pc.MAX_ITERS, N_OUT, IN_DIM), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        bank.pgd_seats(pb, lv(pc.LEVEL_OF, pc.words()), obs, a, pc.COL_LO, pc.COL_HI, pc.SEED, None, wb, pc.MAX_ITERS)
    elif which == "interval":
        (a, wa), wb = _guarded(8), torch.zeros(1, device="cuda")
        bank.certify_seats(pb, lv(cc.LEVEL_OF["main"], cc.LEVELS), obs, a, cc.COL_LO, cc.COL_HI)
    else:
        (a, wa), (b, wb) = _guarded(8), _guarded(8)
        bank.certify_seats(pb, lv(lc.LEVEL_OF["main"], lc.LEVELS), obs, a, lc.COL_LO, lc.COL_HI, 0.0, "linear", b)
    torch.cuda.synchronize()
    return wa.cpu().numpy(), wb.cpu().numpy()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rel(x, x64):
    return float((np.abs(np.asarray(x, np.float64) - x64) / np.maximum(1.0, np.abs(x64))).max())


@pytest.fixture(scope="module")
def bank():
    from copo_amd.eval.bank import PolicyBank
    b = PolicyBank(_policy("ippo", IN_DIM, HIDDEN, False), ac.members(IN_DIM, HIDDEN))
    b.sync_mirror()
    return b


def _against_the_model(which, main, second, bad, counts):
    """The launch on the list with the bad index against the pass's numpy model on the same list -> the rows the model writes."""
    c = pc.inputs(HIDDEN, IN_DIM)
    nets, obs = c["nets"], c["obs"]
    if which == "adversary":
        seen64, grad64, written, perturbed = an.adversary(nets, obs, ac.N, bad, counts, ac.GROUP, ac.LEVEL_OF["A"], ac.LEVELS[:, :3], ac.COL_LO, ac.COL_HI)
        tau, n = ac.reference(HIDDEN, IN_DIM, "A")["tau"], 0
        for r in np.flatnonzero(written):
            if not perturbed[r]:          # table A has no eps == 0 level with a direction: every other listed row is a copy
                assert np.array_equal(_u32(main[r]), _u32(obs[r])) and (_u32(second[r]) == 0).all(), r
                continue
            assert np.abs(second[r].astype(np.float64) - grad64[r]).max() / np.abs(grad64[r]).max() <= tau, r
            lv = an.level_index(int(r), ac.N, 1 if r in ac.ROWS_1 else 2, ac.GROUP, ac.LEVEL_OF["A"], len(ac.LEVELS))
            want = obs[r].copy()
            want[ac.COL_LO:ac.COL_HI] = np.clip(obs[r][ac.COL_LO:ac.COL_HI] + ac.LEVELS[lv][0] * np.sign(second[r][ac.COL_LO:ac.COL_HI]).astype(np.float32),
                                                np.float32(0.0), np.float32(1.0))
            assert want.dtype == np.float32 and np.array_equal(_u32(main[r]), _u32(want)), r
            n += 1
        assert n == 11          # member 1's row, member 2's five rows of group 0 and five of group 1; its rows of group 2 are at index -1
        return written
    if which == "pgd":
        m = pn.pgd(nets, obs, pc.N, bad, counts, pc.GROUP, pc.LEVEL_OF, pc.LEVELS, pc.COL_LO, pc.COL_HI, pc.SEED, None, pc.MAX_ITERS, second)
        listed = m["its"] >= 0
        assert np.array_equal(_u32(main[:N_OUT][listed]), _u32(m["seen"][listed])) and m["its"].max() == pc.MAX_ITERS
        for r in np.flatnonzero(listed):          # the trace is zero past a row's own count
            assert (_u32(second[int(m["its"][r]):, r]) == 0).all(), r
        return listed
    if which == "interval":
        bounds, index = cz.certify(nets, obs, cc.N, bad, counts, cc.GROUP, cc.LEVEL_OF["main"], cc.LEVELS[:, :3], cc.COL_LO, cc.COL_HI)
        tau, valid = cc.reference(HIDDEN, IN_DIM)["tau"], np.flatnonzero(index >= 0)
        assert len(valid) == 15 and max(_rel(main[r][:6], bounds[r][:6]) for r in valid) <= tau
    else:
        bounds, parts, index = lz.certify(nets, obs, lc.N, bad, counts, lc.GROUP, lc.LEVEL_OF["main"], lc.LEVELS[:, :3], lc.COL_LO, lc.COL_HI)
        tau, valid = lc.reference(HIDDEN, IN_DIM)["tau"], np.flatnonzero(index >= 0)
        assert len(valid) == 15 and max(_rel(lc.numbers(main[r], second[r]), lc.numbers(bounds[r], parts[r])) for r in valid) <= tau
        assert all((_u32(second[r]) == 0).all() for r in np.flatnonzero(index == -1))
    levels = cc.LEVELS if which == "interval" else lc.LEVELS
    for r in valid:
        assert main[r][6] == 1.0 and _u32(main[r][7]) == _u32(levels[index[r]][0]), r
    assert all((_u32(main[r]) == 0).all() for r in np.flatnonzero(index == -1))          # a listed row of a group out of range: eight zeros
    return index != -2


@pytest.mark.parametrize("which", PASSES)
def test_an_index_outside_the_rows_in_a_partial_last_tile_is_no_row(bank, which):
    rows, counts = ac.lists()
    assert counts[2] == 17 and rows[2, 16] == 42
    bad = rows.copy()
    bad[2, 16] = N_OUT                      # seventeen listed rows, the last tile holds this index alone
    valid = counts.copy()
    valid[2] = 16                           # the sixteen valid rows: one full tile
    main, second = _launch(which, bank, bad, counts)
    written = _against_the_model(which, main, second, bad, counts)
    listed = np.zeros(N_OUT + 1, bool)
    listed[ac.ROWS_1 + ac.ROWS_2[:16]] = True
    assert np.array_equal(written, listed[:N_OUT])
    bits = _u32(main)
    assert ((bits != POISON).all(axis=1) == listed).all() and ((bits == POISON).all(axis=1) == ~listed).all()
    assert (bits[42] == POISON).all() and (bits[N_OUT] == POISON).all()
    if which == "pgd":
        assert ((_u32(second) != POISON).all(axis=2) == listed[:N_OUT]).all()          # the trace: listed rows, every iteration
    elif which != "interval":
        assert ((_u32(second) != POISON).all(axis=1) == listed).all()
    for g, w in zip((main, second), _launch(which, bank, rows, valid)):                # the same kernel on the valid rows alone
        assert np.array_equal(_u32(g), _u32(w))
