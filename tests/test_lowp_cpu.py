"""CPU: the low-precision policy forward (copo_amd/eval/precision.py, copo_lowp_pack, copo_lowp_forward_seats) --
the two roundings against the framework's casts (the numpy restatement AND the C++ the kernels run, through copo_debug_lowp_round), the
row scales, the packed image, the plan of a sweep, the exact case's premise on the float64 model, and what is exported."""
import ctypes as C

import numpy as np
import pytest
import torch

import lowp_cases as lc
import lowp_numpy as ln

F = np.float32


def _native_round(fmt, x):
    from copo_amd import _capi
    x = np.ascontiguousarray(x, F)
    out = np.empty_like(x)
    assert _capi.lib.copo_debug_lowp_round({"bfloat16": 1, "float8_e4m3": 2}[fmt], x.ctypes.data, x.size, out.ctypes.data) == 0
    return out


def _same(a, b):
    a, b = np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32)
    return np.array_equal(a, b)


def _probes():
    """All 2^16 bfloat16-representable inputs inside [-448, 448]; every e4m3 tie and its float32 neighbours; the e4m3 subnormal range; random."""
    every = (np.arange(65536, dtype=np.uint32) << 16).view(F)
    every = every[np.isfinite(every) & (np.abs(every) <= 448.0)]
    grid = np.unique(np.abs(torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).numpy()))
    grid = grid[np.isfinite(grid)]
    ties = ((grid[:-1].astype(np.float64) + grid[1:]) / 2).astype(F)          # (exact: one more mantissa bit)
    ties = np.concatenate([ties, np.nextafter(ties, F(0)), np.nextafter(ties, F(1000))])
    sub = np.linspace(0, 2.0 ** -6, 4097).astype(F)
    rng = np.random.RandomState(0)
    rand = (rng.randn(100000) * np.exp(rng.randn(100000) * 3)).astype(F)
    rand = rand[np.abs(rand) <= 448.0]
    return np.concatenate([every, ties, -ties, sub, -sub, rand, np.array([1e-30, -1e-30, 1e-45, 448.0, -448.0], F)])


def test_rnd_bf16_is_the_frameworks_cast():
    x = np.concatenate([_probes(), np.array([3.0e38, -3.0e38, 65280.0, 1.00390625, 1.01171875], F)])
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert _same(ln.rnd_bf16(x), want) and _same(_native_round("bfloat16", x), want)


def test_rnd_e4m3_is_the_frameworks_cast_inside_the_range_and_clamps_outside():
    x = _probes()
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).to(torch.float32).numpy()
    assert _same(ln.rnd_e4m3(x), want) and _same(_native_round("float8_e4m3", x), want)
    assert len(np.unique(want)) == 253          # every finite code but -0 is hit: 2 x 126 + 1
    out = np.array([448.5, 449.0, 464.0, 480.0, 1e9, np.inf], F)          # outside the range the clamp is ours: the definition
    for sgn in (1.0, -1.0):
        assert _same(ln.rnd_e4m3(sgn * out), np.full(out.size, sgn * 448.0, F)) and _same(_native_round("float8_e4m3", sgn * out), np.full(out.size, sgn * 448.0, F))


def test_row_scales():
    from copo_amd import _capi
    rng = np.random.RandomState(1)
    amax = np.concatenate([np.exp(rng.randn(2000) * 6), [448.0, 448.0001, 224.0, 224.0001, 1.75, 1.7500001, 2.0 ** -20, 1.0]]).astype(F)
    W = np.zeros((amax.size + 1, 5), F)
    W[:-1, 2] = amax * rng.choice([-1.0, 1.0], amax.size)
    W[:-1, 4] = amax * 0.3
    s = ln.row_scales("float8_e4m3", W)
    assert s[-1] == 1.0          # a zero row
    m, e = np.frexp(s.astype(np.float64))
    assert (m == 0.5).all()          # powers of two
    top = amax.astype(np.float64) / s[:-1]
    assert ((top > 224.0) & (top <= 448.0)).all()
    native = np.empty(amax.size + 1, F)
    a = np.concatenate([amax, [0.0]]).astype(F)
    assert _capi.lib.copo_debug_lowp_scale(a.ctypes.data, a.size, native.ctypes.data) == 0 and _same(native, s)
    assert (ln.row_scales("bfloat16", W) == 1.0).all()


@pytest.mark.parametrize("fmt", ln.FORMATS)
def test_pack_layout_round_trip_and_padding(fmt):
    rng = np.random.RandomState(2)
    H, K1 = 64, 92
    net = (rng.randn(H, K1).astype(F), rng.randn(H).astype(F), (rng.randn(H, H) * 20).astype(F), rng.randn(H).astype(F),
           (rng.randn(4, H) * 1e-3).astype(F), rng.randn(4).astype(F))
    net[2][5] = 0.0
    img = ln.pack_image(fmt, net)
    assert img.dtype == np.uint8 and img.size == ln.image_bytes(fmt, H, K1)
    from copo_amd.eval.precision import packed_bytes
    assert packed_bytes(H, K1, fmt) == img.size
    got, q = ln.unpack_image(fmt, img, H, K1), ln.quantise(fmt, net)
    assert got["q1"].shape == (H, 96) and not got["q1"][:, K1:].any() and _same(got["q1"][:, :K1], q["q1"])
    for k in ("q2", "q3", "s1", "s2", "s3", "b1", "b2", "b3"):
        assert _same(got[k], q[k]), k
    assert _same(ln.decode(fmt, ln.encode(fmt, q["q2"])), q["q2"])
    if fmt == "float8_e4m3":
        assert q["s2"][5] == 1.0 and np.abs(q["q1"]).max() <= 448.0 and ((np.abs(net[2]).max(axis=1) / q["s2"])[np.arange(H) != 5] > 224.0).all()
        assert _same(q["b1"], net[1])          # biases stay fp32
        # dequantised weights are within half an e4m3 step (2^-4 relative) of the originals
        assert np.abs(q["q1"] * q["s1"][:, None] - net[0]).max() <= 2.0 ** -4 * np.abs(net[0]).max(axis=1).max() * 1.0001
    else:
        assert _same(q["q1"], ln.rnd_bf16(net[0])) and _same(q["b1"], ln.rnd_bf16(net[1]))


@pytest.mark.parametrize("hidden,in_dim", [(64, 92), (512, 96)])
def test_exact_case_premise_on_the_model(hidden, in_dim):
    """On the float64 model of both formats the exact case IS the sign network: quantisation loses nothing, every pre-activation is 0 or
    at least 32 in magnitude, and the float32 chunked model agrees to the bit."""
    c = lc.exact_case(hidden, in_dim)
    for net in c["nets"]:
        want = ln.sign_net64(net, c["obs"])
        z1 = c["obs"].astype(np.float64) @ net[0].astype(np.float64).T + net[1]
        z2 = np.sign(z1) @ net[2].astype(np.float64).T + net[3]
        for z in (z1, z2):
            assert ((z == 0) | (np.abs(z) >= 32)).all() and (z == 0).any() and (z != 0).any()
        assert np.tanh(32.0).astype(F) == 1.0
        for fmt in ln.FORMATS:
            q = ln.quantise(fmt, net)
            for l in (1, 2, 3):
                assert _same(q["q%d" % l] * q["s%d" % l][:, None], net[2 * l - 2]) and _same(q["b%d" % l], net[2 * l - 1])
            assert np.array_equal(ln.forward64(fmt, net, c["obs"]), want)
            assert np.array_equal(ln.forward32_chunked(fmt, net, c["obs"]).astype(np.float64), want)


def test_precision_plan():
    from copo_amd.eval.precision import PRECISIONS, PrecisionPlan
    seats, plan = PrecisionPlan.sweep(2, PRECISIONS, 3, 10, share=1.0)
    assert (seats.E, seats.N, seats.K, seats.n_groups, seats.replica_scenes) == (18, 10, 6, 6, 3)
    assert list(plan.member_precision) == [0, 0, 1, 1, 2, 2] and list(plan.member_checkpoint) == [0, 1, 0, 1, 0, 1]
    for g in range(6):
        c, p = g // 3, g % 3
        assert (plan.checkpoint[g], plan.precision[g]) == (c, p) and (seats.group[3 * g:3 * g + 3] == g).all()
        assert (seats.seat[3 * g:3 * g + 3] == p * 2 + c).all()
        assert list(np.nonzero(plan.jury.judges[g])[0]) == [c]          # the only judge: the fp32 twin
    assert list(seats.counts) == [30] * 6
    assert list(plan.counts["float32"]) == [30, 30, 0, 0, 0, 0] and list(plan.counts["bfloat16"]) == [0, 0, 30, 30, 0, 0]
    assert list(plan.counts["float8_e4m3"]) == [0, 0, 0, 0, 30, 30] and sum(plan.counts.values()).tolist() == seats.counts.tolist()
    assert list(plan.jury.counts) == [90, 90, 0, 0, 0, 0] and plan.jury.kind == "panel"
    assert plan.members(["a", "b"]) == ["a", "b"] * 3
    # share < 1: the twins sit in one scene
    seats, plan = PrecisionPlan.sweep(2, ("float32", "float8_e4m3"), 1, 10, share=0.3)
    assert seats.K == 4 and plan.n_lowp == 3
    assert list(seats.seat[1]) == [2, 2, 2, 0, 0, 0, 0, 0, 0, 0] and list(seats.seat[3]) == [3, 3, 3, 1, 1, 1, 1, 1, 1, 1]
    assert (seats.seat[0] == 0).all() and (seats.seat[2] == 1).all()
    assert list(plan.counts["float32"]) == [17, 17, 0, 0] and list(plan.counts["float8_e4m3"]) == [0, 0, 3, 3]
    assert list(plan.jury.counts) == [20, 20, 0, 0]
    for bad in (dict(precisions=("bfloat16",)), dict(precisions=("float32", "float16")), dict(precisions=("float32", "float32")), dict(precisions=()),
                dict(precisions=("bfloat16", "float32")), dict(n_checkpoints=0), dict(scenes_per_cell=0), dict(N=0), dict(share=1.5), dict(share=-0.1)):
        with pytest.raises(ValueError, match="PrecisionPlan.sweep"):
            PrecisionPlan.sweep(**dict(dict(n_checkpoints=2, precisions=PRECISIONS, scenes_per_cell=1, N=4), **bad))
    with pytest.raises(ValueError, match="populations"):
        plan.members(["a"])
    other, _ = PrecisionPlan.sweep(3, PRECISIONS, 1, 4)
    with pytest.raises(ValueError, match="PrecisionPlan"):
        plan.check(other)


def test_exports_and_refusals():
    """The two entry points, their ctypes signatures, and what they refuse without touching a device."""
    from copo_amd import _abi, _capi
    assert {"copo_lowp_pack", "copo_lowp_forward_seats"} <= set(_capi.EXPORTED_SYMBOLS) and _capi.lib.copo_version() == 8 == _abi.ABI_VERSION
    assert _capi.lib.copo_lowp_pack.argtypes == [C.POINTER(_capi.PpoCfg), C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    assert _capi.lib.copo_lowp_forward_seats.argtypes == [C.POINTER(_capi.PpoCfg), C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                         C.c_int64, C.c_int64] + [C.c_void_p] * 7
    assert (_capi.LOWP_BF16, _capi.LOWP_E4M3) == (1, 2)
    cfg = _capi.PpoCfg()
    cfg.mb, cfg.hidden, cfg.act_dim, cfg.n_params = 64, 64, 2, 64 * 92 + 64 * 64 + 4 * 64 + 132
    cfg.pol.in_dim, cfg.pol.out_dim = 92, 4
    need = ln.image_bytes("bfloat16", 64, 92)
    fake = 4096          # an aligned non-NULL address: every call below is refused before anything is launched
    pack = dict(cfg=C.byref(cfg), theta=fake, member_stride=cfg.n_params, n_members=1, fmt=1, packed=fake, packed_stride=(need + 15) // 16 * 16, stream=None)
    fwd = dict(cfg=C.byref(cfg), packed=fake, packed_stride=(need + 15) // 16 * 16, fmt=1, n_members=1, rows=fake, counts=fake, cap=4, n_out=8, obs_src=fake,
               dist_inputs=fake, eps=None, action=None, logp=None, clipped=None, stream=None)
    call = lambda fn, good, **kw: getattr(_capi.lib, fn)(*dict(good, **kw).values())  # noqa: E731
    for fn, good in (("copo_lowp_pack", pack), ("copo_lowp_forward_seats", fwd)):
        for bad, rc in ((dict(cfg=None), -1), (dict(packed=None), -1), (dict(fmt=0), -2), (dict(fmt=3), -2), (dict(n_members=0), -2), (dict(n_members=65536), -2),
                        (dict(packed_stride=need - 16), -2), (dict(packed_stride=need + 1), -2), (dict(packed=fake + 4), -2)):
            assert call(fn, good, **bad) == rc and fn.encode() in _capi.lib.copo_last_error(), (fn, bad)
        cfg.hidden = 96
        assert call(fn, good) == -2
        cfg.hidden = 64
    assert call("copo_lowp_pack", pack, theta=None) == -1 and call("copo_lowp_pack", pack, member_stride=10) == -2
    for bad, rc in ((dict(rows=None), -1), (dict(counts=None), -1), (dict(obs_src=None), -1), (dict(dist_inputs=None), -1), (dict(eps=fake), -1),
                    (dict(cap=0), -2), (dict(n_out=0), -2), (dict(dist_inputs=fake + 4), -2)):
        assert call("copo_lowp_forward_seats", fwd, **bad) == rc, bad
    with pytest.raises(ValueError, match="LowpBank"):
        from copo_amd.eval.precision import LowpBank
        LowpBank(None, "float16")
