"""Shared by tests/test_forward_cpu.py and tests/test_gpu_forward_float64.py: the case table of the forward kernel's float64 referee
(mlp_fwd_kernel, csrc/learn_rowpass.inc, launched through plan_forward, csrc/learn_plan.inc), the float64 model's outputs, the fp32
yardstick's deviation and tau of every case, and the tanh_fast probe nets.  No GPU is touched; the native library is loaded only by
`launch_name`, which asks its launch plan (no device call) which instantiation a case takes.

A case is one net layout with its inputs: `policy_case(hidden, width)` of the shape matrix, `critic_case(name)` of CRITICS.  Its rows
are the BLOCKS below, one after the other, 49 in all: three full 16-row tiles and a one-row masked tile.  Its `variants` are the
parameter sets the same rows run against:
  plain    the random nets of the existing helpers (adversary_cases.members: tanh layers of unit gain, a head of gain 0.1);
  small    W1, b1 and W2 of `plain` times 2^-8, b2 times 2^-16 and W3 times 2^16 (exact): every pre-activation of both layers sits
           in tanh_fast's polynomial branch (layer 1 near 2^-8, layer 2 near 2^-16), and the head brings the outputs back to the
           magnitude of `plain`'s, so that an error of the branch is not hidden under the head bias.  Its rows are the uniform rows and
           the zero row (SMALL_ROWS): the scaled blocks are built against `plain`'s layer 1 and pass nothing here -- against these
           weights they are a linear net on inputs of magnitude 50, which is no regime of the table;
  trained  hidden 256 at widths 91 / 92 only: the populations of tests/golden/eval_policy_function.npz (bank_cases.members).
The two log-std head biases of `plain` and `small` are LOGSTD_BIAS[case number % 3] (`trained` keeps its own); `eps` holds EPS_FIXED
and random normals.

The sampling epilogue alone is judged on EPILOGUE_ROWS rows (the case's rows again and again under independent `eps` draws,
`epilogue_eps`), not on the case's 33 or 49: its yardstick is a sample maximum of per-row rounding errors whose scale differs from row to
row (the log-probability is a sum of terms of magnitude 3 that may cancel to 0.06), so on a few dozen rows one row's draw decides it --
two fp32 evaluations of about six roundings each then differ by a factor above 4 in a few per cent of the cases, and with some 75 variants
a false alarm is expected (one was seen: 1.36 at hidden 128, width 260, `small`; the kernel's second-largest error there equalled the
yardstick's largest).  On 4096 rows both maxima sit near their worst cases and the rule tau = 4 dev compares those.

tau: per case, variant and output kind, `dev` = max |x32 - x64| / max(1, |x64|) of the torch-fp32-CPU yardstick (forward_numpy) and
tau = 4 dev: the convention of certify_cases, adversary_cases and pgd_cases.  No case's dev may pass DEV_CAP (test_forward_cpu.py)."""
import functools
import os

import numpy as np

import adversary_cases as ac
import bank_cases as bc
import forward_numpy as fn

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the shape matrix -----------------------------------------------------------------------------------------------------------------------
MIN_WIDTH = 1                                   # the smallest observation the policy constructor accepts
WIDTHS_FULL = (MIN_WIDTH, 15, 16, 17, 91, 92, 127, 128, 129, 156, 255, 256, 257, 260)
WIDTHS_FEW = (91, 92, 260)
POLICY_CASES = [(h, k) for h in (64, 256) for k in WIDTHS_FULL] + [(h, k) for h in (128, 512) for k in WIDTHS_FEW]
# name: (policy class, fuse mode, hidden, observation width, critic input widths)
CRITICS = {
    "ccppo_mf_91": ("ccppo", "mf", 256, 91, (184,)),
    "ccppo_mf_156": ("ccppo", "mf", 64, 156, (314,)),
    "ccppo_mf_260": ("ccppo", "mf", 512, 260, (522,)),
    "ccppo_concat_91": ("ccppo", "concat", 128, 91, (463,)),
    "copo_92": ("copo", "none", 256, 92, (92, 92, 92)),
    "copo_260": ("copo", "none", 64, 260, (260, 260, 260)),
}
# the combinations above that plan_forward refuses for LDS (COPO_ERR_DIM, outputs keep their poison): none -- the widest layer 1, 522
# columns padded to 640 at hidden 512, takes 115 456 of the 153 600 bytes a workgroup may have.  test_forward_cpu.py holds the plan to
# this list; BEYOND is a layout outside the matrix that IS refused (CCPPO concat on the 260-wide observation, a 1308-wide critic at
# hidden 512: 164 608 bytes), so that the refusal itself is exercised
REFUSED = ()
BEYOND = ("ccppo", "concat", 512, 260, (1308,))
ROW_COUNTS = (1, 15, 16, 17, 49)
TWO_TILE_ROWS = 16384 + 17                      # hidden 256: the two-tile variant from 2 * 32 * 256 rows on
TWO_TILE_WIDTHS = (92, 256, 257)                # 256: XP == HP, the tightest the launcher admits; 257: back to the one-tile kernel
LOGSTD_BIAS = (-3.0, 0.0, 1.0)
EPS_FIXED = ((0.0, 0.0), (1.0, -1.0), (-1.0, 1.0), (6.0, -6.0), (-6.0, 6.0), (0.0, 6.0), (-1.0, 0.0))
DEV_CAP = dict(dist_inputs=1e-5, values=1e-5, logp=1e-3)
OBS_SEED, CC_SEED, EPS_SEED = 4500, 4600, 4700
EPILOGUE_ROWS = 4096

# rows of a case: uniform [-1, 1]; one all-zero row; rows scaled until the largest layer-1 pre-activation of the row is 25 (some pass
# |z| = 20: 1 - tanh is below an fp32 ulp) and 50 (some pass |z| = 45: __expf(2 z) overflows to infinity or underflows to zero)
BLOCKS = dict(uniform=slice(0, 32), zero=slice(32, 33), z20=slice(33, 41), z45=slice(41, 49))
ROWS = 49
SMALL_ROWS = slice(0, 33)                       # the rows of the `small` variant: two full tiles and a one-row masked tile
Z_TARGET = dict(z20=25.0, z45=50.0)
Z_PASSED = dict(z20=20.0, z45=45.0)


def _value_net(in_dim, hidden, seed):
    """A critic net in the policy nets' key layout: bank_cases.random_population with the first head row alone."""
    w = bc.random_population(in_dim, hidden, seed)
    head = bc.TORCH_LAYERS[2]
    w[head + ".weight"], w[head + ".bias"] = w[head + ".weight"][:1].copy(), w[head + ".bias"][:1].copy()
    return w


def _with_logstd(w, bias):
    w = {k: v.copy() for k, v in w.items()}
    w[bc.TORCH_LAYERS[2] + ".bias"][2:] = bias
    return w


def small_copy(w):
    """W1, b1, W2 times 2^-8, b2 times 2^-16, W3 times 2^16, b3 as it is: exact in fp32."""
    l1, l2, l3 = bc.TORCH_LAYERS
    out = {k: v.copy() for k, v in w.items()}
    for key, scale in ((l1 + ".weight", -8), (l1 + ".bias", -8), (l2 + ".weight", -8), (l2 + ".bias", -16), (l3 + ".weight", 16)):
        out[key] *= F(2.0 ** scale)
    return out


def pre_activations(w, x):
    """[n][hidden] float64: W1 x + b1."""
    W1, b1 = ac.net_of(w)[:2]
    return np.asarray(x, np.float64) @ W1.T + b1


def _rows(nets, width, seed):
    """[ROWS][width] float32, the blocks of BLOCKS against the layer 1 of every net of `nets` (they read the same rows): a scaled row's
    largest |W1 x| reaches the block's target in each of them."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1.0, 1.0, (ROWS, width)).astype(F)
    x[BLOCKS["zero"]] = 0.0
    for name, target in Z_TARGET.items():
        blk = x[BLOCKS[name]]
        top = np.min([np.abs(blk.astype(np.float64) @ ac.net_of(w)[0].T).max(axis=1) for w in nets], axis=0)
        blk *= (target / top).astype(F)[:, None]
    return x


def _eps(seed):
    rng = np.random.RandomState(seed)
    eps = rng.standard_normal((ROWS, 2)).astype(F)
    eps[:len(EPS_FIXED)] = EPS_FIXED
    eps[BLOCKS["z45"].start] = (6.0, 6.0)
    return eps


def epilogue_eps(rows=EPILOGUE_ROWS, seed=EPS_SEED):
    """[rows][2] float32 of the epilogue check: EPS_FIXED, then independent standard normals."""
    eps = np.random.RandomState(seed + rows).standard_normal((rows, 2)).astype(F)
    eps[:len(EPS_FIXED)] = EPS_FIXED
    return eps


def _kinds(nets, obs, cc, eps, rows):
    """The float64 model and the yardstick of one variant on its rows, per output kind, and dev / tau."""
    obs, eps, cc = obs[rows], eps[rows], None if cc is None else cc[rows]
    x64, x32 = {}, {}
    x64["dist_inputs"], x32["dist_inputs"] = fn.forward64(nets[0], obs), fn.forward32(nets[0], obs)
    x64["action"], x64["logp"] = fn.sample64(x64["dist_inputs"], eps)
    x32["action"], x32["logp"] = fn.sample32(x32["dist_inputs"], eps)
    x64["clipped"], x32["clipped"] = fn.clip64(x64["action"]), fn.clip32(x32["action"])
    src = obs if cc is None else cc
    x64["values"] = np.stack([fn.forward64(w, src)[:, 0] for w in nets[1:]]) if len(nets) > 1 else np.zeros((0, len(obs)))
    x32["values"] = np.stack([fn.forward32(w, src)[:, 0] for w in nets[1:]]) if len(nets) > 1 else np.zeros((0, len(obs)), F)
    dev = {k: fn.deviation(x32[k], x64[k]) for k in x64}
    return dict(nets=nets, rows=rows, x64=x64, dev=dev, tau={k: 4.0 * v for k, v in dev.items()})


def _case(number, name, pclass, fuse, hidden, width, val_dims, trained_key=None):
    pol = ac.members(width, hidden)[0]
    vals = [_value_net(k, hidden, 4400 + 10 * k + g) for g, k in enumerate(val_dims)]
    bias = LOGSTD_BIAS[number % 3]
    variants = dict(plain=[_with_logstd(pol, bias)] + vals)
    variants["small"] = [small_copy(w) for w in variants["plain"]]
    if trained_key is not None:
        from copo_amd.eval.checkpoint_io import policy_state_dict
        variants["trained"] = [{k: v.numpy() for k, v in policy_state_dict(bc.members(GOLDEN, trained_key, width, hidden, 1)[0]).items()}]
    shared = bool(val_dims) and val_dims[0] == width        # CoPO: the critics read the observation itself
    obs = _rows([pol] + (vals if shared else []), width, OBS_SEED + width)
    cc = None
    if val_dims and not shared:                # the critic input: the observation, then what the fusion appends; its zero and scaled
        rng = np.random.RandomState(CC_SEED + val_dims[0])      # blocks are built against the critic's own layer 1
        cc = np.concatenate([obs, (rng.standard_normal((ROWS, val_dims[0] - width)) * 0.5).astype(F)], axis=1)
        scaled = _rows(vals, val_dims[0], CC_SEED + val_dims[0])
        for blk in ("zero", "z20", "z45"):
            cc[BLOCKS[blk]] = scaled[BLOCKS[blk]]
        cc = np.ascontiguousarray(cc)
    eps = _eps(EPS_SEED + width)
    return dict(name=name, number=number, pclass=pclass, fuse=fuse, hidden=hidden, width=width, val_dims=tuple(val_dims), logstd_bias=bias,
                obs=obs, cc=cc, eps=eps, variants={v: _kinds(nets, obs, cc, eps, SMALL_ROWS if v == "small" else slice(0, ROWS)) for v, nets in variants.items()})


@functools.lru_cache(maxsize=None)
def policy_case(hidden, width):
    """One cell of the shape matrix: an IPPO policy (the policy nets of all three algorithms have one shape)."""
    trained = {91: "ippo_inter", 92: "copo_inter"}.get(width) if hidden == 256 else None
    return _case(POLICY_CASES.index((hidden, width)), "policy_h%d_k%d" % (hidden, width), "ippo", "none", hidden, width, (), trained)


@functools.lru_cache(maxsize=None)
def critic_case(name):
    pclass, fuse, hidden, width, val_dims = CRITICS[name]
    return _case(len(POLICY_CASES) + sorted(CRITICS).index(name), name, pclass, fuse, hidden, width, val_dims)


def tiled(a, rows):
    """`rows` rows: the rows of `a` again and again (axis 0 is the row)."""
    a = np.asarray(a)
    reps = -(-rows // len(a))
    return np.concatenate([a] * reps, axis=0)[:rows]


# ---- which instantiation a launch takes -------------------------------------------------------------------------------------------------------
def launch_name(hidden, width, val_dims, rows, first_net=0, n_nets=1, n_members=0):
    """(return code, kernel name or None) of plan_forward for nets laid out as FusedLearner lays them out; no device is touched."""
    from test_learner_plan_cpu import FORWARD, make_cfg, query
    rc, _geo, launches = query(make_cfg(hidden=hidden, in_pol=width, in_val=tuple(val_dims) or (width,)), FORWARD, n=rows, first_net=first_net,
                               n_nets=n_nets, n_members=n_members)
    return rc, (launches[0][0] if rc == 0 else None)


def fwd_name(hidden, two_tile=False, bank=False):
    nt_w = {64: "1, 4", 128: "2, 4", 256: "2, 8", 512: "4, 8"}[hidden]
    tail = ", 2, true" if two_tile and bank else ", 2" if two_tile else ", 1, true" if bank else ""
    return "mlp_fwd_kernel<%s, false%s>" % (nt_w, tail)


def launches():
    """[(what, hidden, width, critic widths, rows, first net, nets, members, expected kernel)]: every launch shape of the GPU tests."""
    out = []
    for h, k in POLICY_CASES:
        out.append(("act", h, k, (), ROWS, 0, 1, 0, fwd_name(h)))
    for name, (_p, _f, h, k, vd) in sorted(CRITICS.items()):
        out.append(("values " + name, h, k, vd, ROWS, 1, len(vd), 0, fwd_name(h)))
    for k in TWO_TILE_WIDTHS:
        out.append(("two-tile act", 256, k, (), TWO_TILE_ROWS, 0, 1, 0, fwd_name(256, two_tile=k <= 256)))
    out.append(("two-tile values", 256, 92, (92, 92, 92), TWO_TILE_ROWS, 1, 3, 0, fwd_name(256, two_tile=True)))
    out.append(("two-tile bank", 256, 256, (), TWO_TILE_ROWS, 0, 1, 2, fwd_name(256, two_tile=True, bank=True)))
    for h in (64, 128, 256, 512):
        out.append(("bank", h, 92, (), ROWS, 0, 1, 2, fwd_name(h, bank=True)))
    return out


# ---- tanh_fast probes (hidden 64, width 16) ---------------------------------------------------------------------------------------------------
PROBE_HIDDEN, PROBE_WIDTH = 64, 16
# layer: (W1[0][0], W2[0][0], W3[0][0]); every other weight and every bias is zero, so dist_inputs[0] = w3 tanh_fast(w2 tanh_fast(w1 x))
# and every sum is exact (its other terms are zeros)
PROBE_WEIGHTS = {1: (1.0, 2.0 ** -10, 2.0 ** 10), 2: (2.0 ** -10, 2.0 ** 16, 1.0)}
SATURATED_FROM = 10.0                            # 2 / (exp(20) + 1) = 4.1e-9 is below half an ulp of 1: the formula gives exactly 1


def probe_net(layer):
    l1, l2, l3 = bc.TORCH_LAYERS
    H, K = PROBE_HIDDEN, PROBE_WIDTH
    w = {l1 + ".weight": np.zeros((H, K), F), l1 + ".bias": np.zeros(H, F), l2 + ".weight": np.zeros((H, H), F), l2 + ".bias": np.zeros(H, F),
         l3 + ".weight": np.zeros((4, H), F), l3 + ".bias": np.zeros(4, F)}
    for name, v in zip((l1, l2, l3), PROBE_WEIGHTS[layer]):
        w[name + ".weight"][0, 0] = v
    return w


def _neighbours(v):
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


@functools.lru_cache(maxsize=None)
def probe_points(layer):
    """float32 x of the sweep.  Layer 1: tanh_fast sees x itself.  Layer 2: it sees 2^16 tanh_fast(2^-10 x), about 64 x, |x| <= 1."""
    pts = [np.linspace(-12.0, 12.0, 4097), np.linspace(-0.31, 0.31, 2049), _neighbours(0.3), _neighbours(-0.3),
           [44.0, -44.0, 45.0, -45.0, 89.0, -89.0, 1e-20, -1e-20, 0.0]]
    x = np.concatenate([np.asarray(p, np.float64) for p in pts])
    if layer == 2:
        x = np.where(np.abs(x) == 89.0, np.sign(x) * 64.0, x) / 64.0          # (+-89 is out of its reach: the ends of the range instead)
    return x.astype(F)


def probe_obs(layer):
    obs = np.zeros((len(probe_points(layer)), PROBE_WIDTH), F)
    obs[:, 0] = probe_points(layer)
    return obs


def probe_argument64(layer):
    """float64: what the probed tanh_fast call is given (layer 2: up to the first call's error, about one ulp of the argument)."""
    x = probe_points(layer).astype(np.float64)
    return x if layer == 1 else 2.0 ** 16 * np.tanh(2.0 ** -10 * x)


def probe_undo64(layer, out):
    """float64 y of the probed call from dist_inputs[:, 0]: layer 1 inverts the exact scaling and the second call's tanh."""
    out = np.asarray(out, np.float64)
    return 2.0 ** 10 * np.arctanh(out * 2.0 ** -10) if layer == 1 else out


def probe_saturated_output():
    """float32: dist_inputs[0] of the layer-1 probe where the first call returns exactly 1: 2^10 p(2^-10), p the polynomial branch.  In
    p(t) = t (1 + t^2 (-1/3 + ...)) the bracket is 1 - 5.33 x 2^-24, which rounds to 1 - 5 x 2^-24 with or without a fused multiply-add,
    and the two products by powers of two are exact: the emulation and the kernel give the same bits.  One ulp less from the first
    call moves this output by 2^-24, so `exactly 1` can be read off it."""
    return F(2.0 ** 10) * fn.tanh_fast_formula32(F(2.0 ** -10))


@functools.lru_cache(maxsize=None)
def formula_error():
    """tanh_fast_formula32 against np.tanh in float64 over the layer-1 sweep: (max absolute error, where, max relative error, where)."""
    x = probe_points(1)
    want = np.tanh(x.astype(np.float64))
    err = np.abs(fn.tanh_fast_formula32(x).astype(np.float64) - want)
    rel = np.where(want != 0.0, err / np.where(want != 0.0, np.abs(want), 1.0), 0.0)
    return float(err.max()), float(x[err.argmax()]), float(rel.max()), float(x[rel.argmax()])
