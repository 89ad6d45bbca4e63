"""CPU: the premises of tests/test_gpu_forward_float64.py, on the float64 model and its fp32 yardstick alone (tests/forward_numpy.py,
tests/forward_cases.py).  What the GPU tests rely on for exactly their inputs is measured here: the model is jury_cases' model, every
case is well enough conditioned to referee anything, the value regimes are where the case table says they are, the launch plan sends
the table's launches to every fp32 instantiation of the forward kernel, and the tanh formula's own error is known."""
import numpy as np
import pytest

import adversary_cases as ac
import forward_cases as fc
import forward_numpy as fn
import jury_cases as jc
from test_learner_plan_cpu import kernel

ALL_CASES = [("policy", key) for key in fc.POLICY_CASES] + [("critic", name) for name in sorted(fc.CRITICS)]


def _get(kind, key):
    return fc.policy_case(*key) if kind == "policy" else fc.critic_case(key)


def test_the_float64_model_is_the_jurys():
    for hidden, in_dim in ((64, 91), (256, 92)):
        ws, obs = ac.members(in_dim, hidden), ac.observations(in_dim)
        for w in ws:
            assert np.array_equal(fn.forward64(w, obs), jc.forward64(w, obs))
    d = fn.forward64(ws[0], obs)
    eps = np.random.RandomState(0).standard_normal((len(obs), 2))
    a, lp = fn.sample64(d, eps)
    assert np.array_equal(a, d[:, :2] + np.exp(d[:, 2:]) * eps)
    # TorchDiagGaussian.logp in float64
    import torch
    from copo_amd.engine import TorchDiagGaussian
    want = TorchDiagGaussian(torch.from_numpy(d)).logp(torch.from_numpy(a)).numpy()
    assert want.dtype == np.float64 and np.abs(lp - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(fn.clip64([[-3.0, 0.5], [1.0, 7.0]]), [[-1.0, 0.5], [1.0, 1.0]])
    a32, lp32 = fn.sample32(d, eps)
    assert a32.dtype == lp32.dtype == np.float32 and fn.deviation(a32, a) < 1e-5 and fn.deviation(lp32, lp) < 1e-4


@pytest.mark.parametrize("kind,key", ALL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_every_case_is_conditioned_and_its_regimes_are_where_the_table_says(kind, key):
    c = _get(kind, key)
    assert c["obs"].shape == (fc.ROWS, c["width"]) and c["obs"].dtype == np.float32 and c["eps"].shape == (fc.ROWS, 2)
    assert np.array_equal(c["eps"][:len(fc.EPS_FIXED)], np.asarray(fc.EPS_FIXED, np.float32)) and np.abs(c["eps"]).max() == 6.0
    assert np.abs(c["obs"][fc.BLOCKS["uniform"]]).max() <= 1.0 and not c["obs"][fc.BLOCKS["zero"]].any()
    for name, v in c["variants"].items():
        for k, cap in fc.DEV_CAP.items():          # a condition on the reference alone
            assert v["dev"][k] <= cap, (c["name"], name, k, v["dev"][k])
        for k in ("dist_inputs", "action", "logp", "clipped") + (("values",) if c["val_dims"] else ()):
            assert np.isfinite(v["x64"][k]).all() and v["tau"][k] == 4.0 * v["dev"][k] and v["dev"][k] > 0.0, (c["name"], name, k)
        if name != "trained":
            assert np.array_equal(v["nets"][0][fc.bc.TORCH_LAYERS[2] + ".bias"][2:], np.full(2, c["logstd_bias"], np.float32))
        print("%s %s: dev %s" % (c["name"], name, " ".join("%s %.3g" % kv for kv in sorted(v["dev"].items()))))
    # the regimes: layer-1 pre-activations of the nets that read the rows
    plain, small = c["variants"]["plain"]["nets"], c["variants"]["small"]["nets"]
    readers = [(plain[0], c["obs"])] + [(w, c["obs"] if c["cc"] is None else c["cc"]) for w in plain[1:]]
    for w, x in readers:
        z = np.abs(fc.pre_activations(w, x))
        for blk, passed in fc.Z_PASSED.items():
            assert (z[fc.BLOCKS[blk]].max(axis=1) > passed).all(), (c["name"], blk)
        assert z[fc.BLOCKS["uniform"]].max() < 20.0 and z.max() < 1e3
    for w, x in [(small[0], c["obs"])] + [(w, c["obs"] if c["cc"] is None else c["cc"]) for w in small[1:]]:
        W1, b1, W2, b2 = ac.net_of(w)[:4]
        u = fc.SMALL_ROWS                              # the uniform rows and the zero row: both layers in the polynomial branch
        assert u == slice(0, fc.BLOCKS["zero"].stop) == c["variants"]["small"]["rows"] and c["variants"]["plain"]["rows"] == slice(0, fc.ROWS)
        z1 = fc.pre_activations(w, x)[u]
        assert np.abs(z1).max() < 0.3 and np.abs(np.tanh(z1) @ W2.T + b2).max() < 0.3
    # the small variant's outputs are of the plain variant's magnitude, not buried under the head bias
    s, p = c["variants"]["small"]["x64"]["dist_inputs"][:32, :2], c["variants"]["plain"]["x64"]["dist_inputs"][:32, :2]
    assert 0.1 < np.abs(s).mean() / np.abs(p).mean() < 10.0
    if c["cc"] is not None:
        assert c["cc"].shape == (fc.ROWS, c["val_dims"][0]) and np.array_equal(c["cc"][:32, :c["width"]], c["obs"][:32])


def test_the_matrix_is_the_issues_and_nothing_is_refused_but_what_the_table_names():
    assert len(fc.POLICY_CASES) == len(set(fc.POLICY_CASES)) == 2 * 14 + 2 * 3 and fc.MIN_WIDTH < 15
    assert {k for _h, k in fc.POLICY_CASES if _h in (64, 256)} == {fc.MIN_WIDTH, 15, 16, 17, 91, 92, 127, 128, 129, 156, 255, 256, 257, 260}
    assert sorted((v[3], v[4]) for v in fc.CRITICS.values()) == [(91, (184,)), (91, (463,)), (92, (92, 92, 92)), (156, (314,)), (260, (260, 260, 260)),
                                                                 (260, (522,))]
    refused = []
    for h, k in fc.POLICY_CASES:
        rc, _ = fc.launch_name(h, k, (), fc.ROWS)
        if rc != 0:
            assert rc == -2
            refused.append("policy_h%d_k%d" % (h, k))
    for name, (_p, _f, h, k, vd) in sorted(fc.CRITICS.items()):
        rc, _ = fc.launch_name(h, k, vd, fc.ROWS, first_net=1, n_nets=len(vd))
        if rc != 0:
            assert rc == -2
            refused.append(name)
    assert tuple(refused) == fc.REFUSED and len(refused) <= 2
    _p, _f, h, k, vd = fc.BEYOND
    assert fc.launch_name(h, k, vd, fc.ROWS, first_net=1, n_nets=1) == (-2, None)
    assert fc.launch_name(h, k, vd, fc.ROWS)[0] == 0          # its policy net alone is launched


def test_the_tables_launches_reach_every_fp32_instantiation_of_the_forward_kernel():
    names, i = [], 0
    while kernel(i)[0] is not None:
        names.append(kernel(i)[0])
        i += 1
    fp32 = {n for n in names if n.startswith("mlp_fwd_kernel<") and n[len("mlp_fwd_kernel<"):-1].split(", ")[2] == "false"}
    assert len(fp32) == 10          # FWD and FWD_BANK at four shapes, FWD_RT2, FWD_BANK_RT2
    seen = set()
    for what, h, k, vd, rows, first, n_nets, members, want in fc.launches():
        rc, name = fc.launch_name(h, k, vd, rows, first, n_nets, members)
        assert rc == 0 and name == want, (what, h, k, rows, name, want)
        seen.add(name)
    assert seen == fp32, seen ^ fp32
    assert fc.TWO_TILE_ROWS == 16401 and fc.launch_name(256, 92, (), 2 * 32 * 256 - 1)[1] == fc.fwd_name(256)


def test_tanh_formula_against_float64():
    """The formula's own error with exact exp and division, over the probe's sweep: recomputed here, used by the GPU probe as its unit.
    (Printed, not hard-coded; numpy gives 1.76e-7 absolute at x = -3.19 and 4.0e-7 relative just beyond -0.3 on this sweep.)"""
    x = fc.probe_points(1)
    assert x.dtype == np.float32 and len(x) == 4097 + 2049 + 6 + 9 and len(fc.probe_points(2)) == len(x)
    for v in (0.3, -0.3):
        below, at, above = fc._neighbours(v)
        assert below < at < above and at == np.float32(v) and {below, at, above} <= set(x.tolist())
    for v in (0.0, 44.0, -44.0, 45.0, -45.0, 89.0, -89.0, np.float32(1e-20), -np.float32(1e-20)):
        assert v in x
    abs_err, abs_at, rel_err, rel_at = fc.formula_error()
    print("tanh_fast_formula32 vs np.tanh (float64): max abs %.3g at x = %.6g, max rel %.3g at x = %.6g" % (abs_err, abs_at, rel_err, rel_at))
    assert 0.0 < abs_err < 4 * 2.0 ** -23 and 0.0 < rel_err < 8 * 2.0 ** -23          # a handful of fp32 roundings of values of at most 2
    y = fn.tanh_fast_formula32(x)
    assert np.isfinite(y).all() and np.abs(y).max() == 1.0 and y[x == 0.0][0] == 0.0
    assert (y[x >= fc.SATURATED_FROM] == 1.0).all() and (y[x <= -fc.SATURATED_FROM] == -1.0).all()
    assert fn.tanh_fast_formula32(np.float32(89.0)) == 1.0 and fn.tanh_fast_formula32(np.float32(-89.0)) == -1.0
    # the probe nets on the float64 model: what the GPU probe decodes is the probed call's value
    for layer in (1, 2):
        out = fn.forward64(fc.probe_net(layer), fc.probe_obs(layer))
        assert not out[:, 1:].any()
        arg = fc.probe_argument64(layer)
        assert np.abs(fc.probe_undo64(layer, out[:, 0]) - np.tanh(arg)).max() < 1e-12
    assert np.abs(fc.probe_argument64(2)).max() > 63.9 and (np.abs(fc.probe_points(2)) <= 1.0).all()
    # layer 1 saturated: the second call sees exactly 2^-10 and the head gives 2^10 p(2^-10), the largest output the probe can show
    assert fc.probe_saturated_output() == np.float32(1.0) - 5 * np.float32(2.0 ** -24)
