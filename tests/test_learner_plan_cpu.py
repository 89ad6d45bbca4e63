"""CPU: the launch plan of the fused learner (copo_debug_learner_plan, csrc/learn_fused.hip) -- which kernel instantiation a
configuration launches, with which grid, workgroup size and dynamic LDS.  The expected plans are written out by hand from the
dispatcher this plan replaced (its `launch_fused_step` / `mlp_forward`); the size queries of the C ABI must agree with the plan's
geometry, every kernel a plan names must be in the kernel table with room for the plan's LDS, and refused configurations keep
their error codes.  No device is touched."""
import ctypes as C
import itertools

import pytest

from copo_amd import _capi

PPO_STEP, PPO_GRADS, DP_STEP, META_PAIR, META_PAIR_TAIL, META_BATCH, ROW_STORE, ROW_WGRADS, FORWARD = range(9)
ALIGNED, MIRROR, MIRROR_ALIGNED, STORE_OK = 1, 2, 4, 8
ALL = ALIGNED | MIRROR | MIRROR_ALIGNED | STORE_OK
GEMM_LDS = lambda mb: (2 * ((mb + 3) & ~3) + 2 * 4352) * 4      # noqa: E731  two row tables + two 64 x 68 operand slabs
WGRAD_LDS = 8 * 32 * 33 * 4


def make_cfg(mb=512, hidden=256, in_pol=92, in_val=(92, 92, 92), bf16=False):
    """Nets one after the other in the flat buffer, every tensor padded to 16 bytes (as FlatParams lays them out)."""
    c = _capi.PpoCfg()
    c.mb, c.hidden, c.act_dim, c.n_value_heads = mb, hidden, 2, len(in_val)
    c.operand_dtype = _capi.OPERAND_BF16 if bf16 else _capi.OPERAND_F32
    off = 0
    for g, (k, out) in enumerate([(in_pol, 4)] + [(k, 1) for k in in_val]):
        L = _capi.NetLayout()
        for name, n in (("w1", hidden * k), ("b1", hidden), ("w2", hidden * hidden), ("b2", hidden), ("w3", out * hidden), ("b3", out)):
            setattr(L, name, off)
            off += (n + 3) // 4 * 4
        L.in_dim, L.out_dim = k, out
        if g == 0:
            c.pol = L
        else:
            c.val[g - 1] = L
    c.n_params = off
    return c


def kernel(i):
    block, cap = C.c_int32(), C.c_int32()
    name = _capi.lib.copo_debug_learner_kernel(i, C.byref(block), C.byref(cap))
    return (name.decode() if name else None), block.value, cap.value


def query(cfg, mode, n=0, facts=ALL, head=_capi.HEAD_PPO, world=1, first_net=0, n_nets=1, n_members=0):
    """(rc, geometry dict, [(kernel name, (gx, gy, gz), block, lds)]); the table's view of every launch is checked on the way."""
    out = (C.c_int32 * 64)()
    rc = _capi.lib.copo_debug_learner_plan(C.byref(cfg), mode, head, n, world, facts, first_net, n_nets, n_members, out, 64)
    if rc != 0:
        return rc, None, None
    geo = dict(fold_blocks=out[1], n_fold=out[2], lo=(out[3] & 0xffffffff) | (out[4] << 32), refresh=out[5], ksplit=out[6], wgrad_tiles=out[7])
    launches = []
    for i in range(out[0]):
        kid, gx, gy, gz, block, lds = out[8 + 6 * i:14 + 6 * i]
        name, kblock, cap = kernel(kid)
        assert name is not None and block == kblock and 0 <= lds <= cap, (kid, name, block, kblock, lds, cap)
        launches.append((name, (gx, gy, gz), block, lds))
    return rc, geo, launches


def plan(cfg, mode, **kw):
    rc, _geo, launches = query(cfg, mode, **kw)
    assert rc == 0
    return launches


def wgrad(name, hidden, kmax, groups):
    nty, wx2, wx1 = -(-hidden // 32), -(-(hidden + 1) // 32), -(-(kmax + 1) // 32)
    return ("wgrad_adam_kernel<%s>" % name, ((wx2 + wx1) * nty + wx2, groups, 1), 512, WGRAD_LDS)


def test_production_copo_step():
    want = [("rowpass8_kernel<4>", (64, 4, 1), 1024, 66432), ("wgrad_adam_kernel<1, false, true>", (105, 4, 1), 512, 33792)]
    for mode in (PPO_STEP, PPO_GRADS, DP_STEP):
        assert plan(make_cfg(), mode) == want
    assert plan(make_cfg(), DP_STEP, world=8) == want
    # sources that are not 16-byte aligned: the mirror path still takes the row pass
    assert plan(make_cfg(), PPO_STEP, facts=MIRROR | MIRROR_ALIGNED) == want
    # the legacy two-call meta step: the policy net alone
    assert plan(make_cfg(), PPO_GRADS, head=_capi.HEAD_META_NEW) == [("rowpass8_kernel<4>", (64, 1, 1), 1024, 66432),
                                                                      wgrad("1, false, true", 256, 92, 1)]


@pytest.mark.parametrize("bf16", [False, True])
def test_ippo_and_ccppo_steps(bf16):
    """Input 91: no vector rows, the transposed mirror carries the row pass; bfloat16 operands take the BF instantiations."""
    rp, wg = ("rowpass8_kernel<4, true>", "1, true, true") if bf16 else ("rowpass8_kernel<4>", "1, false, true")
    assert plan(make_cfg(in_pol=91, in_val=(91,), bf16=bf16), PPO_STEP) == [(rp, (64, 2, 1), 1024, 66432), wgrad(wg, 256, 91, 2)]
    # CCPPO mean-field critic, 184 wide: layer 1 of the 8-row kernel is padded to 256
    assert plan(make_cfg(in_pol=91, in_val=(184,), bf16=bf16), PPO_STEP) == [(rp, (64, 2, 1), 1024, 70528), wgrad(wg, 256, 184, 2)]
    assert wgrad(wg, 256, 184, 2)[1] == (129, 2, 1)


@pytest.mark.parametrize("hidden,nt_w,block,lds,bf16", [
    (64, "1, 4", 256, 23296, False), (128, "2, 4", 256, 36608, False), (512, "4, 8", 512, 116480, False),
    (64, "1, 4", 256, 23296, True), (128, "2, 4", 256, 36608, True), (512, "4, 8", 512, 116480, True)])
def test_other_row_pass_shapes(hidden, nt_w, block, lds, bf16):
    rp = "rowpass_kernel<%s, true%s>" % (nt_w, ", true" if bf16 else "")
    wg = "1, true, true" if bf16 else "1, false, true"
    assert plan(make_cfg(hidden=hidden, in_pol=91, in_val=(91,), bf16=bf16), PPO_STEP) == [(rp, (32, 2, 1), block, lds), wgrad(wg, hidden, 91, 2)]
    if not bf16:      # without the mirror (vector rows): the instantiation that reads W1 / W2 as stored
        assert plan(make_cfg(hidden=hidden), PPO_STEP, facts=ALIGNED)[0] == ("rowpass_kernel<%s, false>" % nt_w, (32, 4, 1), block, lds)


def test_hidden_256_beyond_the_8_row_tiles():
    """More than 160 workgroups of 16 rows: 16-row tiles; the hand-over variant while every input is at most 128 wide."""
    assert plan(make_cfg(mb=1024), PPO_STEP) == [("rowpass_kernel<2, 8, true, false, true>", (64, 4, 1), 512, 63232), wgrad("1", 256, 92, 4)]
    assert plan(make_cfg(mb=1024, in_pol=260, in_val=(260, 260, 260)), PPO_STEP) == [
        ("rowpass_kernel<2, 8, true>", (64, 4, 1), 512, (16 * 388 + 48 * 260 + 1024 + 64 + 128) * 4), wgrad("1", 256, 260, 4)]
    assert plan(make_cfg(mb=1024), PPO_STEP, facts=ALIGNED)[0][0] == "rowpass_kernel<2, 8, false>"


def test_hidden_without_a_row_pass_instantiation():
    """Hidden 96: forward, head and backward-input tile GEMMs; the PPO step then ends in the weight-gradient kernel like every
    PPO step of the shipped library, the meta pair in gemm_bw + the fold."""
    c = make_cfg(hidden=96)
    chain = lambda v, g: [("gemm_kernel<FwdOpT<1>, %s>" % v, (2, 8, g), 256, 38912), ("gemm_kernel<FwdOpT<2>, %s>" % v, (2, 8, g), 256, 38912),  # noqa: E731
                          ("head_kernel", (32, g, 1), 256, (16 * 97 + 4 * 96 + 64 + 32) * 4), ("gemm_kernel<BxOp, %s>" % v, (2, 8, g), 256, 38912)]
    assert plan(c, PPO_STEP) == chain("true", 4) + [wgrad("1, false, true", 96, 92, 4)]
    # operands that are not 16-byte aligned, or an input width that is no multiple of 4: the scalar instantiations
    assert plan(c, PPO_STEP, facts=MIRROR) == chain("false", 4) + [wgrad("1, false, true", 96, 92, 4)]
    assert plan(make_cfg(hidden=96, in_pol=91, in_val=(91,)), PPO_STEP)[0][0] == "gemm_kernel<FwdOpT<1>, false>"
    # hidden 96 does not fill whole 64-wide tiles: 2 + 1 column tiles of layers 2 / 3 and 2 of layer 1, 2 row tiles, 4 row splits
    for mode in (META_PAIR, META_PAIR_TAIL):
        rc, geo, launches = query(c, mode)
        assert launches == chain("true", 2) + [("gemm_bw_kernel<true>", ((2 + 2) * 2 + 2, 2 * 4, 1), 256, 38912),
                                               ("reduce_adam_kernel", (geo["fold_blocks"], 1, 1), 256, 0)]
        assert geo["n_fold"] == 96 * 92 + 96 + 96 * 96 + 96 + 4 * 96 + 4 and geo["fold_blocks"] == -(-geo["n_fold"] // 1024) and geo["lo"] == 0
        assert geo["ksplit"] == 4 and not geo["refresh"]
    # misaligned operands keep a row-pass shape off the row pass too
    assert [k for k, *_ in plan(make_cfg(), PPO_STEP, facts=MIRROR)] == [
        "gemm_kernel<FwdOpT<1>, false>", "gemm_kernel<FwdOpT<2>, false>", "head_kernel", "gemm_kernel<BxOp, false>", "wgrad_adam_kernel<1, false, true>"]


N_FOLD = 256 * 92 + 256 + 256 * 256 + 256 + 4 * 256 + 4      # the policy net of make_cfg()


def test_meta_pair():
    """The step-by-step pair: both policies as two groups of the row pass that reads the weights as stored (no mirror of the target)."""
    for mode in (META_PAIR, META_PAIR_TAIL):
        rc, geo, launches = query(make_cfg(), mode)
        assert launches == [("rowpass_kernel<2, 8, false>", (32, 2, 1), 512, 63232), ("gemm_bw_kernel<true>", ((4 + 2) * 4 + 4, 2 * 4, 1), 256, 38912),
                            ("reduce_adam_kernel", (89, 1, 1), 256, 0)]
        assert (geo["n_fold"], geo["fold_blocks"], geo["lo"]) == (N_FOLD, 89, 0)


@pytest.mark.parametrize("nb", [1, 3, 8, 32])
def test_batched_meta_modes(nb):
    c, g = make_cfg(), 2 * nb
    rows = [("gemm_kernel<FwdOpT<1>, true>", (4, 8, g), 256, 38912), ("gemm_kernel<FwdOpT<2>, true>", (4, 8, g), 256, 38912),
            ("head_kernel", (32, g, 1), 256, (16 * 257 + 1024 + 64 + 32) * 4), ("gemm_kernel<BxOp, true>", (4, 8, g), 256, 38912)]
    fold = ("meta_batch_fold_kernel", (89, nb, 1), 256, 0)
    assert plan(c, ROW_STORE, n=nb) == rows
    assert plan(c, META_BATCH, n=nb) == rows + [("gemm_bw_kernel<true>", (28, g, 1), 256, 38912), fold]
    # from the row store: the head layer's tiles are one workgroup on the vector path
    assert plan(c, ROW_WGRADS, n=nb) == [("gemm_bw_kernel<true, true>", (25, g, 1), 256, 38912), fold]
    assert plan(c, ROW_WGRADS, n=nb, facts=ALIGNED | MIRROR) == [("gemm_bw_kernel<false, true>", (28, g, 1), 256, 38912), fold]
    rc, geo, _ = query(c, META_BATCH, n=nb)
    assert (geo["n_fold"], geo["fold_blocks"], geo["lo"], geo["ksplit"]) == (N_FOLD, 89, 0, 1)


def test_forward_pass():
    c = make_cfg()
    one, two = (16 * 132 + 32 * 260 + 1024) * 4, (4 * 16 * 260 + 1024) * 4
    assert plan(c, FORWARD, n=2 * 32 * 256 - 1, n_nets=4) == [("mlp_fwd_kernel<2, 8, false>", (1024, 4, 1), 512, one)]
    assert plan(c, FORWARD, n=2 * 32 * 256, n_nets=4) == [("mlp_fwd_kernel<2, 8, false, 2>", (512, 4, 1), 512, two)]
    assert plan(c, FORWARD, n=1007, first_net=1, n_nets=3) == [("mlp_fwd_kernel<2, 8, false>", (63, 3, 1), 512, one)]
    assert plan(make_cfg(bf16=True), FORWARD, n=2 * 32 * 256) == [("mlp_fwd_kernel<2, 8, true, 2>", (512, 1, 1), 512, two)]
    assert plan(make_cfg(hidden=64, in_pol=91, in_val=(184,)), FORWARD, n=40000, n_nets=2) == [
        ("mlp_fwd_kernel<1, 4, false>", (2500, 2, 1), 256, (16 * 260 + 32 * 68 + 256) * 4)]
    # an input wider than the hidden layers keeps one tile per workgroup (the two-tile form shares the input rows' LDS with layer 2)
    assert plan(make_cfg(in_pol=283, in_val=(283,)), FORWARD, n=40000)[0][0] == "mlp_fwd_kernel<2, 8, false>"
    # the bank: the variant of ONE member's rows, the member as the grid's second dimension
    assert plan(c, FORWARD, n=1000, n_members=5) == [("mlp_fwd_kernel<2, 8, false, 1, true>", (63, 5, 1), 512, one)]
    assert plan(c, FORWARD, n=16384, n_members=3) == [("mlp_fwd_kernel<2, 8, false, 2, true>", (512, 3, 1), 512, two)]
    assert plan(make_cfg(hidden=128, bf16=True), FORWARD, n=16384, n_members=3)[0][0] == "mlp_fwd_kernel<2, 4, true, 1, true>"


CFGS = [make_cfg(), make_cfg(in_pol=91, in_val=(91,)), make_cfg(in_pol=91, in_val=(184,), bf16=True), make_cfg(hidden=64), make_cfg(hidden=128, mb=200),
        make_cfg(hidden=512, mb=1000), make_cfg(hidden=96), make_cfg(hidden=48, mb=72, in_pol=91, in_val=(184,))]


@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "h%d_mb%d_k%d_%d" % (c.hidden, c.mb, c.pol.in_dim, c.n_value_heads))
def test_size_queries_agree_with_the_plan(cfg):
    ws_total = lambda gcap, nreg: (4 * gcap * cfg.mb * cfg.hidden + gcap * cfg.mb * 4 + nreg * (1 if gcap > 4 else 4) * cfg.n_params  # noqa: E731
                                   + gcap * ((cfg.mb + 7) // 8) * 8 + 12)
    rc, geo, launches = query(cfg, PPO_STEP, facts=ALIGNED)     # (the grid does not depend on the pointers; bf16 needs the mirror: refused)
    if rc != 0:
        rc, geo, launches = query(cfg, PPO_STEP)
    tiles = launches[-1][1][0] * launches[-1][1][1]
    assert launches[-1][0].startswith("wgrad_adam_kernel") and tiles == geo["wgrad_tiles"]
    for world in (1, 2, 8):
        n_own = -(-tiles // world)
        words = (((n_own * world + tiles) * 1024 + n_own * world + tiles + 3) & ~3) + 8
        assert _capi.lib.copo_dp_workspace_bytes(C.byref(cfg), world) == 4 * words
    if cfg.operand_dtype == _capi.OPERAND_F32:
        for nb in (1, 3, 8, 32):
            rc, geo, _ = query(cfg, META_BATCH, n=nb)
            assert rc == 0 and _capi.lib.copo_meta_fold_len(C.byref(cfg)) == geo["n_fold"]
            gcap = 2 * nb if 2 * nb > 4 else 8
            assert _capi.lib.copo_meta_batch_workspace_floats(C.byref(cfg), nb) == ((ws_total(gcap, gcap) + 1) & ~1) + 2 * nb * geo["fold_blocks"]
    assert _capi.lib.copo_ppo_workspace_floats(C.byref(cfg)) == ws_total(4, 2)


def test_every_plan_names_table_entries_with_room_for_its_lds():
    """query() asserts, for every launch, that the id is in the table, that the workgroup size is the entry's and that the LDS
    bytes fit the entry's ceiling; every kernel of the table is reached by some configuration of the sweep or of the shipped
    profiling switches (wgrad_adam_kernel<2>, the RT8 row passes of rowpass_kernel and reduce_adam's mirror refresh are not)."""
    names, i = [], 0
    while kernel(i)[0] is not None:
        names.append(kernel(i)[0])
        i += 1
    assert len(names) == len(set(names)) == 55 and kernel(-1)[0] is None
    seen = set()
    for mb, hidden, k, bf16 in itertools.product((64, 128, 256, 512, 1024), (64, 96, 128, 256, 512), (91, 92, 156, 283), (False, True)):
        for in_val in ((k,), (k, k, k), (2 * k + 2,)):
            cfg = make_cfg(mb, hidden, k, in_val, bf16)
            for mode, facts, n in [(m, f, 0) for m in (PPO_STEP, PPO_GRADS, DP_STEP, META_PAIR, META_PAIR_TAIL) for f in (0, ALIGNED, MIRROR | MIRROR_ALIGNED, ALL)] + \
                                  [(m, f, nb) for m in (META_BATCH, ROW_STORE, ROW_WGRADS) for f in (0, ALIGNED, ALL) for nb in (1, 32)]:
                rc, _geo, launches = query(cfg, mode, n=n, facts=facts)
                assert rc in (0, -3) and (rc == 0 or bf16)
                seen.update(name for name, *_ in launches or [])
            for n, members in ((1000, 0), (16384, 0), (1000, 4), (16384, 4)):
                rc, _geo, launches = query(cfg, FORWARD, n=n, n_nets=1 + len(in_val) if not members else 1, n_members=members)
                assert rc == (0 if hidden != 96 else -2)
                seen.update(name for name, *_ in launches or [])
    never = {"wgrad_adam_kernel<2>", "rowpass_kernel<2, 8, true, false, true, 8>", "rowpass_kernel<2, 8, true, false, false, 8>"}
    assert set(names) - seen == never, (set(names) - seen) ^ never


def test_refused_configurations_keep_their_codes():
    dev, dim = -3, -2      # COPO_ERR_DEVICE: what the entry points answer for a plan they refuse; COPO_ERR_DIM: a forward shape
    assert query(make_cfg(hidden=96, bf16=True), PPO_STEP)[0] == dev             # bfloat16 without the row pass
    assert query(make_cfg(bf16=True), PPO_STEP, facts=ALIGNED)[0] == dev          # ... without the mirror
    assert query(make_cfg(bf16=True), PPO_GRADS, head=_capi.HEAD_META_NEW)[0] == dev
    assert query(make_cfg(bf16=True), META_BATCH, n=3)[0] == dev
    assert query(make_cfg(bf16=True), PPO_STEP)[0] == 0
    for mode in (META_PAIR, META_PAIR_TAIL, META_BATCH, ROW_WGRADS, PPO_GRADS):    # data-parallel: the PPO step with Adam only
        assert query(make_cfg(), mode, n=3, world=2)[0] == dev
    assert query(make_cfg(), PPO_STEP, world=2)[0] == 0
    big = make_cfg(hidden=1024, in_pol=8000, in_val=())      # a policy net of more than COPO_META_DOT_PARTIALS fold workgroups
    assert big.pol.b3 + 4 > 8192 * 1024
    assert query(big, META_PAIR)[0] == dev and query(big, META_BATCH, n=1)[0] == dev
    assert query(make_cfg(hidden=96), FORWARD, n=100)[0] == dim
    assert query(make_cfg(), FORWARD, n=100, facts=MIRROR)[0] == dim              # mirror not 16-byte aligned
    assert query(make_cfg(), FORWARD, n=100, first_net=3, n_nets=2)[0] == dim
    assert query(make_cfg(), FORWARD, n=0)[0] == dim
    assert query(make_cfg(mb=2048), PPO_STEP)[0] == dim and query(make_cfg(), 9)[0] == dim and query(make_cfg(), META_BATCH, n=0)[0] == dim
    assert _capi.lib.copo_debug_learner_plan(None, 0, 0, 0, 1, 0, 0, 1, 0, None, 0) == -1
    out = (C.c_int32 * 8)()
    assert _capi.lib.copo_debug_learner_plan(C.byref(make_cfg()), 0, 0, 0, 1, ALL, 0, 1, 0, out, 8) == dim      # buffer too small
