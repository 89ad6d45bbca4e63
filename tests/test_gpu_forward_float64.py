"""The forward-only kernel on the GPU (mlp_fwd_kernel, csrc/learn_rowpass.inc; FusedLearner.act / values, PolicyBank.act) against the
float64 model of tests/forward_numpy.py, on the cases of tests/forward_cases.py; tests/test_forward_cpu.py checks their premises on the
model alone.  Every output kind of every case stays within the case's tau = 4 dev of the torch-fp32-CPU yardstick; the worst ratio
err / tau per output kind is printed, and a ratio above 1 fails.  Bit comparisons: two launches, the clip, rows past a launch (poison),
row lists, a misaligned source, the two-tile variant's fall-back and the dense bank against the single-member launch.  tanh_fast
(csrc/learn_gemm.inc) is probed as a function through two nets whose sums are exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import forward_cases as fc
import forward_numpy as fn
import jury_cases as jc

pytestmark = pytest.mark.gpu

from test_gpu_fused_learner import _make  # noqa: E402
from test_learner_plan_cpu import FORWARD, MIRROR_ALIGNED, query  # noqa: E402

POISON = jc.POISON
TAIL = 16
KINDS = ("dist_inputs", "action", "logp", "clipped")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _same(a, b):
    return np.array_equal(_u32(a), _u32(b))


def _poison(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _poisoned(t):
    return bool((_u32(t) == POISON).all())


@functools.lru_cache(maxsize=None)
def _policy(pclass, fuse, width, hidden):
    pol = _make(pclass, fuse, width, fused=True, hiddens=(hidden, hidden))
    assert pol.fused is not None and pol.fused.can_forward
    return pol


def _linears(model):
    """[[l1, l2, l3] of the policy net, of every value net]: the order of fused.model_layouts."""
    from copo_amd.fused import _mlp_layers
    nets = [_mlp_layers(model._hidden_layers) + [model._logits._model[0]],
            _mlp_layers(model._value_branch_separate) + [model._value_branch._model[0]]]
    for name in ("nei_value_network", "global_value_network"):
        if getattr(model, name, None) is not None:
            nets.append(_mlp_layers(getattr(model, name)))
    return nets


def _load(pol, nets):
    """The parameter sets of a variant into the policy's model (net g of `nets` into net g of the model), and the mirror."""
    with torch.no_grad():
        for lins, w in zip(_linears(pol.model), nets):
            for lin, name in zip(lins, fc.bc.TORCH_LAYERS):
                assert tuple(lin.weight.shape) == w[name + ".weight"].shape, (name, tuple(lin.weight.shape), w[name + ".weight"].shape)
                lin.weight.copy_(torch.from_numpy(w[name + ".weight"]))
                lin.bias.copy_(torch.from_numpy(w[name + ".bias"]))
    pol.fused.invalidate_mirror()
    pol.fused.sync_mirror()
    return pol.fused


def _launched(fz, rows, first_net=0, n_nets=1, n_members=0):
    rc, _geo, launches = query(fz.cfg, FORWARD, n=rows, facts=MIRROR_ALIGNED, first_net=first_net, n_nets=n_nets, n_members=n_members)
    return rc, (launches[0][0] if rc == 0 else None)


def _act(fz, obs, eps, sample=True):
    """One launch on obs.shape[0] rows into buffers TAIL rows longer, poisoned: ({kind: tensor of the launch's rows}, tails intact)."""
    n = obs.shape[0]
    out = dict(dist_inputs=_poison(n + TAIL, 4), action=_poison(n + TAIL, 2), logp=_poison(n + TAIL), clipped=_poison(n + TAIL, 2))
    if sample:
        fz.act(obs, eps, out["action"], out["logp"], out["dist_inputs"], out["clipped"])
    else:
        from copo_amd import _capi
        _capi.check(_capi.lib.copo_mlp_forward_f32(C.byref(fz.cfg), fz.flat.flat.data_ptr(), fz.flat_t.data_ptr(), obs.data_ptr(), None, n, 0, 1, None,
                                                   out["dist_inputs"].data_ptr(), None, out["action"].data_ptr(), out["logp"].data_ptr(),
                                                   out["clipped"].data_ptr(), _capi.current_stream()))
    torch.cuda.synchronize()
    return {k: v[:n] for k, v in out.items()}, all(_poisoned(v[n:]) for v in out.values())


def _values(fz, obs, cc, rows=None):
    """[nv][n] of one launch into a buffer TAIL floats longer (poisoned tail; zeros under a row list): (values, tail intact)."""
    n, nv = obs.shape[0], int(fz.cfg.n_value_heads)
    buf = _poison(nv * n + TAIL)
    if rows is not None:
        buf[:nv * n] = 0.0
    got = fz.values(obs, cc, out=buf[:nv * n].view(nv, n), rows=rows)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    return got, _poisoned(buf[nv * n:])


def _ratio(got, x64, tau):
    err = np.abs(got.astype(np.float64) - x64) / np.maximum(1.0, np.abs(x64))
    return float(err.max()) / tau if err.size else 0.0


def _check_outputs(where, out, v, eps, rows=None):
    """Every output kind of a launch within the variant's tau of the float64 model (tiled to the launch's rows); the clip in bits.
    -> {kind: worst err / tau}"""
    got = {k: t.cpu().numpy() for k, t in out.items()}
    n = len(got["logp"])
    ratios = {k: _ratio(got[k], fc.tiled(v["x64"][k], n) if rows is None else v["x64"][k][rows], v["tau"][k]) for k in KINDS}
    assert _same(out["clipped"], out["action"].clamp(-1.0, 1.0)), where
    assert all(np.isfinite(g).all() for g in got.values()), where
    print("%s: err / tau %s" % (where, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= 1.0, (where, ratios)
    return ratios


def _check_epilogue(where, fz, obs_rows, n=fc.EPILOGUE_ROWS):
    """The sampling epilogue alone: sample64 on the kernel's OWN dist_inputs (as float64), within 4 dev of the sampling yardstick on
    those same inputs, on `n` rows (`obs_rows` again and again) under independent draws of eps (forward_cases: why not on the case's rows)."""
    eps = fc.epilogue_eps(n)
    out, tail_ok = _act(fz, _dev(fc.tiled(obs_rows, n)), _dev(eps))
    assert tail_ok, where
    got = {k: t.cpu().numpy() for k, t in out.items()}
    a64, lp64 = fn.sample64(got["dist_inputs"], eps)
    a32, lp32 = fn.sample32(got["dist_inputs"], eps)
    ratios = {}
    for k, g, x64, x32 in (("action", got["action"], a64, a32), ("logp", got["logp"], lp64, lp32)):
        tau = 4.0 * fn.deviation(x32, x64)
        assert tau > 0.0, (where, k)
        ratios[k] = _ratio(g, x64, tau)
    assert _same(out["clipped"], out["action"].clamp(-1.0, 1.0)), where
    print("%s: epilogue alone on %d rows, err / tau %s" % (where, n, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    assert max(ratios.values()) <= 1.0, (where, ratios)


@pytest.mark.parametrize("hidden,width", fc.POLICY_CASES)
def test_every_policy_case_against_float64(hidden, width):
    c = fc.policy_case(hidden, width)
    pol = _policy(c["pclass"], c["fuse"], width, hidden)
    for name, v in c["variants"].items():
        obs, eps = _dev(c["obs"][v["rows"]]), _dev(c["eps"][v["rows"]])
        fz = _load(pol, v["nets"])
        rc, kernel = _launched(fz, len(obs))
        if c["name"] in fc.REFUSED:          # (none today: the table names what plan_forward refuses for LDS)
            from copo_amd import _capi
            assert rc == -2
            with pytest.raises(_capi.CopoError, match="COPO_ERR_DIM"):
                _act(fz, obs, eps)
            continue
        assert (rc, kernel) == (0, fc.fwd_name(hidden)), (rc, kernel)
        out, tail_ok = _act(fz, obs, eps)
        assert tail_ok, "written past the launch"
        _check_outputs("%s %s" % (c["name"], name), out, v, c["eps"][v["rows"]])
        _check_epilogue("%s %s" % (c["name"], name), fz, c["obs"][v["rows"]])
        again, _ = _act(fz, obs, eps)
        for k in KINDS:
            assert _same(out[k], again[k]), (name, k)
        assert _same(obs, _dev(c["obs"][v["rows"]])) and _same(eps, _dev(c["eps"][v["rows"]]))


@pytest.mark.parametrize("name", sorted(fc.CRITICS))
def test_every_critic_case_against_float64(name):
    c = fc.critic_case(name)
    pol = _policy(c["pclass"], c["fuse"], c["width"], c["hidden"])
    assert int(pol.model.value_input_dim()) == c["val_dims"][0] and int(pol.fused.cfg.n_value_heads) == len(c["val_dims"])
    for vname, v in c["variants"].items():
        obs, eps, cc = _dev(c["obs"][v["rows"]]), _dev(c["eps"][v["rows"]]), None if c["cc"] is None else _dev(c["cc"][v["rows"]])
        fz = _load(pol, v["nets"])
        assert _launched(fz, len(obs), 1, len(c["val_dims"])) == (0, fc.fwd_name(c["hidden"]))
        got, tail_ok = _values(fz, obs, cc)
        assert tail_ok and got.shape == v["x64"]["values"].shape
        ratio = _ratio(got.cpu().numpy(), v["x64"]["values"], v["tau"]["values"])
        print("%s %s: values err / tau %.3f" % (name, vname, ratio))
        assert np.isfinite(got.cpu().numpy()).all() and ratio <= 1.0
        again, _ = _values(fz, obs, cc)
        assert _same(got, again)
        out, tail_ok = _act(fz, obs, eps)          # the policy net of the same layout, next to its critics in the flat buffer
        assert tail_ok
        _check_outputs("%s %s policy" % (name, vname), out, v, c["eps"][v["rows"]])
        _check_epilogue("%s %s policy" % (name, vname), fz, c["obs"][v["rows"]])


@pytest.mark.parametrize("which", ["policy_h64_k91", "policy_h256_k92", "ccppo_mf_91", "copo_92"])
def test_row_counts_tails_and_poison(which):
    """Launches of 1, 15, 16, 17 and 49 rows: the rows of a launch are the bits of the same rows in the 49-row launch (a row's outputs
    do not depend on the rows that share its tile), nothing is written past the launch, a launch without `eps` leaves action,
    log-probability and clipped action alone; `values` with an unsorted row list and a one-row list."""
    c = fc.critic_case(which) if which in fc.CRITICS else fc.policy_case(*[int(s[1:]) for s in which.split("_")[1:]])
    pol = _policy(c["pclass"], c["fuse"], c["width"], c["hidden"])
    v = c["variants"]["plain"]
    fz = _load(pol, v["nets"])
    obs, eps, cc = _dev(c["obs"]), _dev(c["eps"]), None if c["cc"] is None else _dev(c["cc"])
    full, _ = _act(fz, obs, eps)
    vfull = _values(fz, obs, cc)[0] if c["val_dims"] else None
    for n in fc.ROW_COUNTS:
        out, tail_ok = _act(fz, obs[:n].contiguous(), eps[:n].contiguous())
        assert tail_ok, n
        for k in KINDS:
            assert not (_u32(out[k]) == POISON).any() and _same(out[k], full[k][:n]), (n, k)
        dry, tail_ok = _act(fz, obs[:n].contiguous(), None, sample=False)
        assert tail_ok and _same(dry["dist_inputs"], full["dist_inputs"][:n]), n
        assert all(_poisoned(dry[k]) for k in ("action", "logp", "clipped")), n
        if vfull is not None:
            got, tail_ok = _values(fz, obs[:n].contiguous(), None if cc is None else cc[:n].contiguous())
            assert tail_ok and _same(got, vfull[:, :n]), n
    if vfull is not None:
        perm = np.random.RandomState(7).permutation(fc.ROWS)[:33].astype(np.int64)
        assert (np.diff(perm) < 0).any()
        for rows in (perm, np.array([17], np.int64)):
            got, tail_ok = _values(fz, obs, cc, rows=_dev(rows))
            listed, rest = _dev(rows), _dev(np.setdiff1d(np.arange(fc.ROWS), rows))
            assert tail_ok and _same(got[:, listed], vfull[:, listed]) and not _u32(got[:, rest]).any(), rows


@pytest.mark.parametrize("which", ["policy_h256_k92", "policy_h256_k256", "policy_h64_k92", "ccppo_mf_91"])
def test_misaligned_source(which):
    """A source one float into its storage (4-byte aligned only) takes the scalar gather at a width that is a multiple of 4: the same
    bits as the aligned launch -- the gather differs, the order of the sums does not.  ccppo_mf_91: the critic source (184 wide)."""
    c = fc.critic_case(which) if which in fc.CRITICS else fc.policy_case(*[int(s[1:]) for s in which.split("_")[1:]])
    pol = _policy(c["pclass"], c["fuse"], c["width"], c["hidden"])
    fz = _load(pol, c["variants"]["plain"]["nets"])

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device="cuda")
        view = buf[1:].view(*a.shape)
        view.copy_(_dev(a))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    obs, eps = _dev(c["obs"]), _dev(c["eps"])
    if c["val_dims"]:
        assert c["val_dims"][0] % 4 == 0 and c["cc"] is not None
        want, _ = _values(fz, obs, _dev(c["cc"]))
        got, tail_ok = _values(fz, obs, shifted(c["cc"]))
        assert tail_ok and _same(got, want)
    else:
        assert c["width"] % 4 == 0
        want, _ = _act(fz, obs, eps)
        got, tail_ok = _act(fz, shifted(c["obs"]), eps)
        assert tail_ok
        for k in KINDS:
            assert _same(got[k], want[k]), k


@pytest.mark.parametrize("width", fc.TWO_TILE_WIDTHS)
def test_two_tile_variant(width):
    """Hidden 256 on 16 401 rows (the case's 49 rows again and again): two 16-row tiles per workgroup up to width 256, where the input
    tile fills the dead h2 tile exactly; at 257 the launcher falls back to the one-tile kernel, whose rows are the 49-row launch's bits.
    Width 92 also runs the three critics of CoPO; width 256 the dense bank of two members, each the bits of its own launch."""
    R = fc.TWO_TILE_ROWS
    c = fc.policy_case(256, width)
    v = c["variants"]["plain"]
    pol = _policy("ippo", "none", width, 256)
    fz = _load(pol, v["nets"])
    want_kernel = fc.fwd_name(256, two_tile=width <= 256)
    assert _launched(fz, R) == (0, want_kernel)
    obs, eps = _dev(fc.tiled(c["obs"], R)), _dev(fc.tiled(c["eps"], R))
    out, tail_ok = _act(fz, obs, eps)
    assert tail_ok
    _check_outputs("two-tile %s (%s)" % (c["name"], want_kernel), out, v, fc.tiled(c["eps"], R))
    _check_epilogue("two-tile %s" % c["name"], fz, c["obs"], R)
    small, _ = _act(fz, obs[:fc.ROWS].contiguous(), eps[:fc.ROWS].contiguous())
    if width > 256:
        for k in KINDS:
            assert _same(out[k][:fc.ROWS], small[k]), k
    for k in KINDS:          # the same rows in another workgroup: the same bits
        assert _same(out[k][fc.ROWS * 32:fc.ROWS * 64], out[k][:fc.ROWS * 32]), k
    if width == 92:
        cc = fc.critic_case("copo_92")
        cv = cc["variants"]["plain"]
        cpol = _policy(cc["pclass"], cc["fuse"], 92, 256)
        cfz = _load(cpol, cv["nets"])
        assert _launched(cfz, R, 1, 3) == (0, fc.fwd_name(256, two_tile=True))
        got, tail_ok = _values(cfz, _dev(fc.tiled(cc["obs"], R)), None)
        ratio = _ratio(got.cpu().numpy(), fc.tiled(cv["x64"]["values"].T, R).T, cv["tau"]["values"])
        print("two-tile copo_92 values: err / tau %.3f" % ratio)
        assert tail_ok and ratio <= 1.0
    if width == 256:
        from copo_amd.eval.bank import PolicyBank
        members = [v["nets"][0], fc.bc.perturbed(v["nets"][0], 1)]
        bank = PolicyBank(pol, members)
        bank.sync_mirror()
        assert _launched(fz, R, n_members=2) == (0, fc.fwd_name(256, two_tile=True, bank=True))
        both = dict(dist_inputs=_poison(2 * R + TAIL, 4), action=_poison(2 * R + TAIL, 2), logp=_poison(2 * R + TAIL), clipped=_poison(2 * R + TAIL, 2))
        bank.act(obs.repeat(2, 1), eps.repeat(2, 1), both["action"], both["logp"], both["dist_inputs"], both["clipped"])
        torch.cuda.synchronize()
        for m, w in enumerate(members):
            alone, _ = _act(_load(pol, [w]), obs, eps)
            for k in KINDS:
                assert _same(both[k][m * R:(m + 1) * R], alone[k]), (m, k)
        assert all(_poisoned(t[2 * R:]) for t in both.values())
        assert not _same(both["dist_inputs"][:R], both["dist_inputs"][R:2 * R])


@pytest.mark.parametrize("hidden", [64, 128, 256, 512])
def test_dense_bank_holds_the_single_launch_bits_at_every_shape(hidden):
    """The four one-tile BANK instantiations on two members of 49 rows each."""
    from copo_amd.eval.bank import PolicyBank
    c = fc.policy_case(hidden, 92)
    pol = _policy("ippo", "none", 92, hidden)
    plain = c["variants"]["plain"]["nets"][0]
    members = [plain, fc.bc.perturbed(plain, 1)]
    bank = PolicyBank(pol, members)
    bank.sync_mirror()
    R = fc.ROWS
    obs, eps = _dev(c["obs"]), _dev(c["eps"])
    both = dict(dist_inputs=_poison(2 * R + TAIL, 4), action=_poison(2 * R + TAIL, 2), logp=_poison(2 * R + TAIL), clipped=_poison(2 * R + TAIL, 2))
    bank.act(obs.repeat(2, 1), eps.repeat(2, 1), both["action"], both["logp"], both["dist_inputs"], both["clipped"])
    torch.cuda.synchronize()
    assert all(_poisoned(t[2 * R:]) for t in both.values())
    for m, w in enumerate(members):
        fz = _load(pol, [w])
        assert _launched(fz, R, n_members=2) == (0, fc.fwd_name(hidden, bank=True))
        alone, _ = _act(fz, obs, eps)
        for k in KINDS:
            assert _same(both[k][m * R:(m + 1) * R], alone[k]), (m, k)
    _check_outputs("bank h%d member 0" % hidden, {k: t[:R] for k, t in both.items()}, c["variants"]["plain"], c["eps"])


def test_a_refused_layout_answers_err_dim_and_writes_nothing():
    """A critic input too wide for the workgroup's LDS at hidden 512 (forward_cases.BEYOND): COPO_ERR_DIM, the output keeps its poison;
    the policy net of the same layout is launched."""
    from copo_amd import _capi
    pclass, fuse, hidden, width, val_dims = fc.BEYOND
    pol = _policy(pclass, fuse, width, hidden)
    fz = pol.fused
    fz.sync_mirror()
    assert int(pol.model.value_input_dim()) == val_dims[0]
    assert _launched(fz, fc.ROWS, 1, 1) == (-2, None) and _launched(fz, fc.ROWS) == (0, fc.fwd_name(hidden))
    obs, cc = torch.zeros(fc.ROWS, width, device="cuda"), torch.zeros(fc.ROWS, val_dims[0], device="cuda")
    out = _poison(1, fc.ROWS)
    with pytest.raises(_capi.CopoError, match="COPO_ERR_DIM"):
        fz.values(obs, cc, out=out)
    with pytest.raises(_capi.CopoError, match="COPO_ERR_DIM"):
        fz.values(obs, cc, out=out, rows=_dev(np.array([3, 1], np.int64)))
    torch.cuda.synchronize()
    assert _poisoned(out)
    got, tail_ok = _act(fz, obs, torch.zeros(fc.ROWS, 2, device="cuda"))
    assert tail_ok and not (_u32(got["dist_inputs"]) == POISON).any()


@pytest.mark.parametrize("layer", [1, 2])
def test_tanh_fast_probe(layer):
    """tanh_fast as a function, through a net whose every sum has one non-zero term (forward_cases.probe_net): the absolute error
    against np.tanh in float64 within 4 times the formula's own maximum with exact exp and division (test_forward_cpu.py recomputes
    it; the margin is for __expf and __frcp_rn, 1 to 2 ulp each), |y| <= 1, exactly +-1 from |argument| = 10 on, finite at the ends,
    y(0) == 0."""
    pol = _policy("ippo", "none", fc.PROBE_WIDTH, fc.PROBE_HIDDEN)
    fz = _load(pol, [fc.probe_net(layer)])
    x = fc.probe_points(layer)
    out, tail_ok = _act(fz, _dev(fc.probe_obs(layer)), None, sample=False)
    d = out["dist_inputs"].cpu().numpy()
    assert tail_ok and np.isfinite(d).all() and not d[:, 1:].any()
    o = d[:, 0]
    arg = fc.probe_argument64(layer)
    err = np.abs(fc.probe_undo64(layer, o) - np.tanh(arg))
    unit = fc.formula_error()[0]
    rel = np.where(arg != 0.0, err / np.where(arg != 0.0, np.abs(np.tanh(arg)), 1.0), 0.0)
    print("tanh_fast in layer %d: max abs error %.3g at argument %.6g (%.2f of the formula's own %.3g; bound 4), max rel error %.3g at %.6g" % (
        layer, err.max(), arg[err.argmax()], err.max() / unit, unit, rel.max(), arg[rel.argmax()]))
    assert err.max() <= 4.0 * unit
    # saturation: layer 1 shows y through the second call, whose output for y == 1 exactly is known in bits
    top = fc.probe_saturated_output() if layer == 1 else np.float32(1.0)
    sat = np.abs(arg) >= fc.SATURATED_FROM
    assert sat.sum() > 600 and (np.abs(o) <= top).all()
    assert np.array_equal(o[sat], np.where(arg[sat] > 0, top, -top).astype(np.float32))
    assert (o[x == 0.0] == 0.0).all() and np.array_equal(o[x > 0], np.abs(o[x > 0])) and np.array_equal(o[x < 0], -np.abs(o[x < 0]))
