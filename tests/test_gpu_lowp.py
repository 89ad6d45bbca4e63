"""The low-precision policy forward on the GPU (copo_lowp_pack, copo_lowp_forward_seats, copo_amd/eval/precision.py, DESIGN.md section
8t).  (1) an exact case compared in BITS with the fp32 seat forward, (2) the list rules, (3) a trained net's weights against the float64
model of tests/lowp_numpy.py with a yardstick that is not the kernel, (4) a mixed plan, (5) the sampler.  References are computed once
per case and shared."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adversary_cases as ac
import bank_cases as bc
import lowp_cases as lc
import lowp_numpy as ln

pytestmark = pytest.mark.gpu

from test_gpu_policy_bank import _policy  # noqa: E402

POISON = lc.POISON
F = np.float32
KEYS = ("dist_inputs", "action", "logp", "clipped")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def _poison(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _outputs(n):
    return dict(dist_inputs=_poison(n, 4), action=_poison(n, 2), logp=_poison(n), clipped=_poison(n, 2))


def _lists(rows, counts, n_out):
    return SimpleNamespace(K=rows.shape[0], cap=rows.shape[1], n_out=n_out, rows=_dev(rows), counts=_dev(counts))


def _launch(bank, lists, obs, eps):
    """The four outputs (uint32 bits, host) of `bank.act_seats` -- a `PolicyBank` or a `LowpBank` -- on poisoned arrays."""
    out = _outputs(lists.n_out)
    bank.act_seats(lists, obs, eps, out["action"], out["logp"], out["dist_inputs"], out["clipped"])
    torch.cuda.synchronize()
    return {k: _u32(v) for k, v in out.items()}


def _f32(bits):
    return bits.view(F)


# ---- (1) the exact case --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact(hidden, in_dim):
    from copo_amd.eval.bank import PolicyBank
    c = lc.exact_case(hidden, in_dim)
    bank = PolicyBank(_policy("ippo", in_dim, hidden, False), [lc.as_weights(n) for n in c["nets"]])
    bank.sync_mirror()
    lists, obs, eps = _lists(c["rows"], c["counts"], lc.EXACT_ROWS), _dev(c["obs"]), _dev(c["eps"])
    return dict(c=c, bank=bank, lists=lists, obs=obs, eps=eps, ref=_launch(bank, lists, obs, eps))


@pytest.mark.parametrize("fmt", ln.FORMATS)
@pytest.mark.parametrize("in_dim", lc.EXACT_IN_DIMS)
@pytest.mark.parametrize("hidden", lc.EXACT_HIDDENS)
def test_exact_case_has_the_fp32_kernels_bits(hidden, in_dim, fmt):
    """Premise first: the fp32 seat forward's dist_inputs ARE the float64 value of W3 sgn(W2 sgn(W1 o + b1) + b2) + b3 (tanh_fast
    saturates to exactly +-1 and gives 0 at 0).  Then the low-precision launch has that launch's bits in all four outputs, the poison of
    the unlisted rows included; and the packed image is tests/lowp_numpy.py's, byte for byte."""
    from copo_amd.eval.precision import LowpBank
    e = _exact(hidden, in_dim)
    c, ref = e["c"], e["ref"]
    for k, rows in enumerate(lc.EXACT_LISTS):
        want = ln.sign_net64(c["nets"][k], c["obs"][rows])
        assert np.array_equal(_f32(ref["dist_inputs"])[rows].astype(np.float64), want), "premise: the fp32 kernel is not exact here"
        assert np.abs(want).max() > 1.0 and len(np.unique(want)) > 8
    unlisted = sorted(set(range(lc.EXACT_ROWS)) - set(sum(lc.EXACT_LISTS, [])))
    assert unlisted and (ref["dist_inputs"][unlisted] == POISON).all()
    lb = LowpBank(e["bank"], fmt)
    torch.cuda.synchronize()
    img = lb.packed.cpu().numpy()
    for k in range(2):
        want = ln.pack_image(fmt, c["nets"][k])
        assert lb.image_bytes == want.size == ln.image_bytes(fmt, hidden, in_dim)
        assert np.array_equal(img[k, :want.size], want), "member %d: packed image" % k
    got = _launch(lb, e["lists"], e["obs"], e["eps"])
    for key in KEYS:
        bad = np.nonzero((got[key] != ref[key]).reshape(lc.EXACT_ROWS, -1).any(1))[0]
        assert bad.size == 0, "%s differs in rows %s" % (key, bad[:8])


# ---- (2) lists ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_bank(hidden, in_dim=92):
    from copo_amd.eval.bank import PolicyBank
    ws = ac.members(in_dim, hidden)
    bank = PolicyBank(_policy("copo" if in_dim == 92 else "ippo", in_dim, hidden, False), ws)
    bank.sync_mirror()
    return bank, ws


@functools.lru_cache(maxsize=None)
def _single_rows(fmt):
    """Every row of the list case launched ALONE (a one-entry list of member 0, cap 1): the bits a row must have in any list."""
    from copo_amd.eval.precision import LowpBank
    bank, _ = _random_bank(64)
    lb = LowpBank(bank, fmt)
    rng = np.random.RandomState(7300)
    obs, eps = _dev(rng.rand(lc.LIST_N_OUT, 92).astype(F)), _dev(rng.randn(lc.LIST_N_OUT, 2).astype(F))
    out = _outputs(lc.LIST_N_OUT)
    counts = _dev(np.array([1, 0, 0], np.int32))
    for r in range(lc.LIST_N_OUT):
        lists = SimpleNamespace(K=3, cap=1, n_out=lc.LIST_N_OUT, rows=torch.full((3, 1), r, dtype=torch.int64, device="cuda"), counts=counts)
        lb.act_seats(lists, obs, eps, out["action"], out["logp"], out["dist_inputs"], out["clipped"])
    torch.cuda.synchronize()
    return lb, obs, eps, {k: _u32(v) for k, v in out.items()}


@pytest.mark.parametrize("fmt", ln.FORMATS)
@pytest.mark.parametrize("count", lc.LIST_COUNTS)
def test_lists(count, fmt):
    """Counts of 0, 1, 15, 16, 17, 33 under a capacity of 40 and a count above it; -1 and n_out inside the list.  Rows in no list keep
    the poison, every listed row has the bits of its single-row launch: the tile's neighbours and the masks do not matter."""
    lb, obs, eps, alone = _single_rows(fmt)
    rows, counts, listed = lc.list_case(count)
    rows3, counts3 = np.concatenate([rows, np.zeros((2, lc.LIST_CAP), np.int64)]), np.array([counts[0], 0, 0], np.int32)
    got = _launch(lb, _lists(rows3, counts3, lc.LIST_N_OUT), obs, eps)
    assert len(listed) == max(min(count, lc.LIST_CAP) - (2 if count >= 3 else 0), 0)
    mask = np.zeros(lc.LIST_N_OUT, bool)
    mask[listed] = True
    for key in KEYS:
        assert (alone[key] != POISON).all()
        assert np.array_equal(got[key][mask], alone[key][mask]), key
        assert (got[key][~mask] == POISON).all(), key


# ---- (3) a trained net's weights against the float64 model -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(golden_dir, hidden):
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.checkpoint_io import policy_state_dict
    w = bc.members(golden_dir, "copo_inter", 92, hidden, 1)[0]
    net = ac.net_of({k: v.numpy() for k, v in policy_state_dict(w).items()}, F)          # (the golden file has the reference's key layout)
    obs = ac.observations(92)
    n = obs.shape[0]
    bank = PolicyBank(_policy("copo", 92, hidden, False), [w])
    bank.sync_mirror()
    bank16 = PolicyBank(_policy("copo", 92, hidden, True), [w])          # the learner's bfloat16 operand mode, the existing seat forward
    bank16.sync_mirror()
    lists = _lists(np.arange(n, dtype=np.int64)[None], np.array([n], np.int32), n)
    old = _f32(_launch(bank16, lists, _dev(obs), _dev(np.zeros((n, 2), F)))["dist_inputs"]).astype(np.float64)
    return dict(net=net, obs=obs, bank=bank, old16=old)


@pytest.mark.parametrize("fmt", ln.FORMATS)
@pytest.mark.parametrize("hidden", (64, 256))
def test_random_case_against_the_float64_model(golden_dir, hidden, fmt):
    """The yardstick is the largest deviation, per output, between two evaluations of the spec that differ in fp32 summation order only
    (the float64 model and a float32 model that sums in chunks of 32); the kernel gets twice that.  bfloat16: the existing operand_dtype =
    1 seat forward's deviation from the same model on the same rows is reported, and the new kernel may not exceed twice it.

    Measured on an MI355X.  bfloat16: yardstick 0, kernel 0 at hidden 64 and 256 (the existing mode: 8.3e-7 in one output at 64, 0 at
    256).  float8_e4m3: hidden 64 yardstick [0, 0, 1.9e-9, 0], kernel the same; hidden 256 yardstick [1.5e-7, 2.0e-7, 3.2e-7, 2.1e-7],
    kernel [2.0e-7, 1.6e-7, 2.4e-7, 1.5e-7].  (With the fp8 instruction's full operands the kernel missed this bound by three to five
    orders of magnitude: DESIGN.md section 8t.)"""
    from copo_amd.eval.precision import lowp_forward
    c = _random_case(golden_dir, hidden)
    m64 = ln.forward64(fmt, c["net"], c["obs"])
    m32 = ln.forward32_chunked(fmt, c["net"], c["obs"]).astype(np.float64)
    yard = np.abs(m32 - m64).max(axis=0)
    got = lowp_forward(c["bank"], fmt, _dev(c["obs"])).cpu().numpy().astype(np.float64)
    dev = np.abs(got - m64).max(axis=0)
    print("hidden %d %s: model-to-model deviation per output %s, the kernel's %s" % (hidden, fmt, yard, dev))
    if fmt == "bfloat16":
        old = np.abs(c["old16"] - m64).max(axis=0)
        print("hidden %d bfloat16: the operand_dtype = 1 seat forward's deviation from the model %s" % (hidden, old))
        assert (dev <= 2.0 * old).all(), (dev, old)
    assert (dev <= 2.0 * yard).all(), (dev, yard)


# ---- (4) a mixed plan ------------------------------------------------------------------------------------------------------------------
def test_mixed_plan():
    """2 checkpoints x 3 precisions, twins in one scene: the fp32 members' rows are `PolicyBank.act_seats` on their lists alone, bit for
    bit; the low-precision members' rows are their own format's launch; two launches agree; a graph replay equals the eager launch."""
    from copo_amd.eval.bank import PolicyBank
    from copo_amd.eval.crossplay import PlanBuffers
    from copo_amd.eval.precision import PRECISIONS, LowpBank, MixedBank, PrecisionPlan
    _, ws = _random_bank(64)
    seats, plan = PrecisionPlan.sweep(2, PRECISIONS, 1, 12, share=0.75)
    bank = PolicyBank(_policy("copo", 92, 64, False), plan.members(ws[:2]))
    bank.sync_mirror()
    mixed = MixedBank(bank, plan.precisions, plan.member_precision)
    pb = PlanBuffers(seats, "cuda")
    n = seats.E * seats.N
    rng = np.random.RandomState(7400)
    obs, eps = _dev(rng.rand(n, 92).astype(F)), _dev(rng.randn(n, 2).astype(F))
    got = _launch(mixed, pb, obs, eps)
    again = _launch(mixed, pb, obs, eps)
    parts = {"float32": bank, "bfloat16": LowpBank(bank, "bfloat16"), "float8_e4m3": LowpBank(bank, "float8_e4m3")}
    seen = np.zeros(n, bool)
    for p, b in parts.items():
        alone = _launch(b, _lists(seats.rows, plan.counts[p], n), obs, eps)
        mine = np.isin(seats.seat.reshape(-1), np.nonzero(plan.member_precision == plan.precisions.index(p))[0])
        assert mine.any() and not (seen & mine).any()
        seen |= mine
        for key in KEYS:
            assert (alone[key][~mine] == POISON).all() and (alone[key][mine] != POISON).all(), (p, key)
            assert np.array_equal(got[key][mine], alone[key][mine]), (p, key)
    assert seen.all()
    for key in KEYS:
        assert np.array_equal(got[key], again[key]), key
    assert not np.array_equal(got["dist_inputs"][seats.seat.reshape(-1) == 2], got["dist_inputs"][seats.seat.reshape(-1) == 4])
    out = _outputs(n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mixed.act_seats(pb, obs, eps, out["action"], out["logp"], out["dist_inputs"], out["clipped"])          # (warm: the images and masks exist)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mixed.act_seats(pb, obs, eps, out["action"], out["logp"], out["dist_inputs"], out["clipped"])
    for v in out.values():
        v.view(torch.int32).fill_(POISON)
    graph.replay()
    torch.cuda.synchronize()
    for key in KEYS:
        assert np.array_equal(_u32(out[key]), got[key]), key


# ---- (5) the sampler -------------------------------------------------------------------------------------------------------------------
E2E = (2, 2, 12, 8, 3)          # checkpoints, scenes per cell, slots, T, fragments


def _fragments(smp, n_frag, seed=3):
    torch.manual_seed(seed)
    smp.reset()
    smp.obs[smp.T].copy_(smp.obs[0])
    for _ in range(n_frag):
        smp.sample()
    torch.cuda.synchronize()
    return smp


def test_sampler(golden_dir):
    """2 checkpoints x 3 precisions, 2 scenes per cell, 12 slots, T = 8, 3 fragments, share = 1."""
    from copo_amd.eval.bank import PolicyBank, draw_cell_noise
    from copo_amd.eval.crossplay import SeatSampler
    from copo_amd.eval.evaluate import make_eval_trainer
    from copo_amd.eval.precision import PRECISIONS, PrecisionPlan, PrecisionSeatSampler, precision_frame
    Cn, S, N, T, n_frag = E2E
    w = bc.golden_population(golden_dir, "copo_inter")
    ws = [w, bc.perturbed(w, 1, 0.05)]
    seats, plan = PrecisionPlan.sweep(Cn, PRECISIONS, S, N, share=1.0)
    t = make_eval_trainer("copo", "inter", seats.E, N, 0)
    try:
        bank = PolicyBank(t.policy, plan.members(ws))
        smp = _fragments(PrecisionSeatSampler(t.env, t.policy, bank, seats, plan, T, use_graph=True), n_frag)
        tally, jt = smp.tally.cpu().numpy(), smp.jury_tally.cpu().numpy()

        class Plain(SeatSampler):          # the same cells, every member in fp32, the same shared noise
            def _draw_noise(self):
                draw_cell_noise(self.eps, S)

        plain = _fragments(Plain(t.env, t.policy, bank, seats, T, use_graph=False), n_frag).tally.cpu().numpy()
    finally:
        t.stop()
    P = len(PRECISIONS)
    for c in range(Cn):
        g32 = c * P
        assert tally[g32, c, 0] > 0 and np.array_equal(tally[g32], plain[g32])          # the fp32 cells: a plain SeatSampler's words
        assert jt[g32, c, c, 0] == tally[g32, c, 0] and not jt[g32, c, c, 1:].any()      # ... and no drift from themselves
        for p in range(1, P):
            g, m = c * P + p, p * Cn + c
            assert jt[g, m, c, 0] == tally[g, m, 0] > 0          # every acted seat-step of the twin was judged, once
            assert jt[g, m, c, 7] > 0
    df = precision_frame(tally, jt, seats, plan, labels=["a", "b"], deltas=(0.05, 0.05))
    assert [(r.checkpoint, r.precision) for r in df.itertuples()] == [(c, p) for c in range(Cn) for p in PRECISIONS]
    print(df[["checkpoint", "precision", "acted", "success", "reward_per_step", "drift_steer", "drift_throttle", "drift_kl", "drift_max", "disagree_rate"]].to_string())
    for c in range(Cn):
        rows = df[df.checkpoint == c].set_index("precision")
        assert rows.loc["float32", "drift_max"] == 0.0 and rows.loc["float32", "drift_pairs"] == rows.loc["float32", "acted"]
        assert rows.loc["float8_e4m3", "drift_max"] >= rows.loc["bfloat16", "drift_max"] > 0.0
