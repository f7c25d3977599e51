"""The w4 weight format (trace_amd/w4.py), the probes of its decode GEMV (tests/w4_probes.py) and the host-side entry points — no GPU."""
import ctypes as C
import functools

import pytest
import torch

import w4_probes as P
from trace_amd import w4

BF = torch.bfloat16
SHAPES = ((16, 256), (48, 512), (16384, 256), (64, 14336), (4112, 4352))       # one per plan class of the GEMV (see test_plan_classes)


def _row(vals, scale=1.0):
    """a [1, 32] bf16 block from a short list of values (rest zero)"""
    r = torch.zeros(32)
    r[:len(vals)] = torch.tensor(vals, dtype=torch.float32) * scale
    return r.to(BF)[None, :]


def test_every_code_and_every_tie_on_a_hand_written_table():
    # the block's amax is 6 (e = 0), so codes are read off |v| directly; ties go to the even code
    table = [(0.0, 0), (0.2, 0), (0.25, 0), (0.26, 1), (0.5, 1), (0.74, 1), (0.75, 2), (1.0, 2), (1.25, 2), (1.26, 3), (1.5, 3), (1.74, 3), (1.75, 4),
             (2.0, 4), (2.5, 4), (2.51, 5), (3.0, 5), (3.49, 5), (3.5, 6), (4.0, 6), (5.0, 6), (5.03, 7), (6.0, 7)]
    for sign in (1.0, -1.0):
        vals = [6.0] + [sign * v for v, _ in table]
        codes, exps = w4.quant(_row(vals))
        got = w4.unpack_codes(codes)[0, 1:1 + len(table)].tolist()
        want = [(m | 8) if (sign < 0 and m) else m for _, m in table]          # no negative zero
        assert got == want, (sign, got, want)
        assert exps[0, 0].item() == 127
    assert w4.unpack_codes(w4.quant(_row([6.0]))[0])[0, 0].item() == 7


@pytest.mark.parametrize("e", (-20, -1, 0, 3, 40))
def test_scale_rule_just_below_at_and_above_six(e):
    s = 2.0 ** e
    below, at, above = 5.96875, 6.0, 6.03125                                    # bf16 neighbours of 6
    for amax, want_e in ((below, e), (at, e), (above, e + 1)):
        W = _row([amax, -1.0, 0.5], s)
        assert W[0, 0].float().item() == amax * s
        codes, exps = w4.quant(W)
        assert exps[0, 0].item() == want_e + 127, (amax, exps[0, 0].item())
        Wt = w4.dequant(codes, exps, torch.float32)
        assert Wt.abs().max().item() <= 6 * 2.0 ** want_e                        # nothing saturates
        assert Wt[0, 0].item() == 6 * s                                          # (6.03 under the doubled scale: 3.0156 -> code 3.0 -> 6)


def test_zero_blocks_and_tiny_values():
    W = torch.zeros((2, 64), dtype=BF)
    W[0, 40] = -0.0
    W[1, 3] = 2.0 ** -130                                                       # a bf16 denormal: e is kept at -120, the value rounds to code 0
    codes, exps = w4.quant(W)
    assert exps.tolist() == [[0, 0], [7, 0]]
    assert int(codes.sum()) == 0
    assert torch.equal(w4.dequant(codes, exps), torch.zeros((2, 64), dtype=BF))
    assert not torch.signbit(w4.dequant(codes, exps).float()).any()


def _gauss(N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn((N, K), generator=g) * 0.02).to(BF)
    W[0, :32] = 0                                                               # a zero block
    W[1, 32:64] = torch.tensor([0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, 0.25] * 4).to(BF) * 2.0 ** -7     # exact ties under amax 6 * 2^-7
    return W


def test_format_is_idempotent_exact_in_bf16_and_never_saturates():
    W = _gauss(48, 512)
    codes, exps = w4.quant(W)
    Wt64 = w4.dequant(codes, exps, torch.float64)
    Wt = w4.dequant(codes, exps)
    assert Wt.dtype == BF and torch.equal(Wt.double(), Wt64)                    # every W~ value survives .to(bfloat16)
    c2, e2 = w4.quant(Wt)
    assert torch.equal(w4.dequant(c2, e2), Wt)                                  # dequant(quant(W~)) == W~ (a block whose largest code fell to 3 or below
    assert (e2 <= exps).all()                                                   #  re-quantises under a smaller scale, to the same values)
    err = (Wt.float() - W.float()).abs().view(48, 16, 32)
    unit = torch.where(exps == 0, torch.zeros(1), torch.pow(torch.tensor(2.0), exps.float() - 127))[..., None]
    assert (err <= unit).all()                                                  # half the widest gap between neighbouring codes (4 and 6)
    # the ties of row 1 went to the even codes
    assert w4.unpack_codes(codes)[1, 32:40].tolist() == [2, 2, 4, 4, 6, 6, 7, 0]


def test_packer_round_trip_and_index_map():
    W = _gauss(32, 512, seed=3)
    codes, exps = w4.quant(W)
    tc, te = w4.tile_pack(codes, exps)
    assert tc.shape == (2, 2, 64, 32) and te.shape == (2, 2, 64, 2)
    c2, e2 = w4.tile_unpack(tc, te)
    assert torch.equal(c2, codes) and torch.equal(e2, exps)
    cc = w4.unpack_codes(codes)
    for n, k in ((0, 0), (17, 1), (5, 255), (31, 256 + 64 * 3 + 33), (16, 511)):
        (t, u, lane, byte, nib), (t2, u2, lane2, half) = w4.tile_index(n, k, 512)
        assert (int(tc[t, u, lane, byte]) >> (4 * nib)) & 15 == int(cc[n, k])
        assert int(te[t2, u2, lane2, half]) == int(exps[n, k // 32])
    assert w4.weight_bytes(4096, 4096) == 4096 * 4096 * 17 // 32


def test_twin_items_replace_exactly_the_projections():
    W = _gauss(16, 256, seed=5)
    items = [("model.layers.0.self_attn.q_proj.weight", W), ("model.layers.1.mlp.down_proj.weight", W), ("model.layers.0.input_layernorm.weight", W),
             ("lm_head.weight", W), ("model.vision_tower.vision_tower.vision_model.encoder.layers.0.self_attn.q_proj.weight", W)]
    out = dict(w4.twin_items(items))
    for name, _ in items:
        assert torch.equal(out[name], w4.roundtrip(W) if name.startswith("model.layers.") and "layernorm" not in name else W), name


# ---- the probes' own condition, and the named faults ----
@functools.lru_cache(maxsize=None)
def _plan(N, K, B):
    from trace_amd import build
    from trace_amd.engine import ops
    build.build()
    return ops.skinny_w4_plan(N, K, B)


@pytest.mark.parametrize("N,K", SHAPES + ((32, 4096),))               # the five shapes the GPU tests run, and the longest K with activations up to 8
@pytest.mark.parametrize("name", P.PROBES)
def test_probe_answers_do_not_depend_on_the_summation_order(name, N, K):
    codes, exps, X = P.build(name, N, K, 3)
    assert X.float().abs().max().item() <= (1 if K > 4096 else 8)
    assert int(exps.max()) - int(exps.min()) <= 3
    assert P.order_free(codes, exps, X)


@pytest.mark.parametrize("N,K,B", ((16, 256, 1), (48, 512, 3), (64, 14336, 17), (4112, 4352, 3)))
@pytest.mark.parametrize("name", P.PROBES)
def test_fault_free_emulation_is_accepted(name, N, K, B):
    codes, exps, X = P.build(name, N, K, B)
    tc, te = w4.tile_pack(codes, exps)
    got, clean = P.result(P.emulate(tc, te, X, N, K, B, _plan(N, K, B)), B)
    assert clean and torch.equal(got, P.expected(codes, exps, X))


@pytest.mark.parametrize("fault", P.FAULTS)
def test_every_fault_is_rejected_by_its_named_probe(fault):
    N, K, B = 64, 14336, 3                                                      # KS > 1 here, so the chunk faults have an edge to lose
    plan = _plan(N, K, B)
    assert plan["KS"] > 1 and 16 * plan["NB"] > B
    codes, exps, X = P.build(P.REJECTS[fault], N, K, B)
    tc, te = w4.tile_pack(codes, exps)
    got, clean = P.result(P.emulate(tc, te, X, N, K, B, plan, fault), B)
    assert not (clean and torch.equal(got, P.expected(codes, exps, X))), fault


# ---- host-side entry points ----
NEW_SYMBOLS = ("trace_op_quant_rows_w4", "trace_op_tile_pack_w4", "trace_op_dequant_w4", "trace_op_skinny_w4", "trace_op_skinny_w4_plan",
               "trace_op_decode_route_w4", "trace_ctx_llm_weights_type")


def test_both_libraries_export_the_w4_entry_points():
    from trace_amd import build, _lib
    build.build()
    for element in ("bf16", "f16"):
        lib = _lib.load(element)
        for name in NEW_SYMBOLS:
            assert name in _lib.SIGNATURES and hasattr(lib, name), (element, name)
    from trace_amd.engine import ops
    for name in ("quant_rows_w4", "tile_pack_w4", "dequant_w4", "skinny_w4", "skinny_w4_plan", "decode_route_w4"):
        assert callable(getattr(ops, name))


def test_plan_classes():
    """the five shapes of the GPU tests are five different plans: the minimum, several tiles, NT = 2, KS > 1 with WPT > 1, ragged tiles"""
    p = {s: _plan(s[0], s[1], 1) for s in SHAPES}
    assert (p[(16, 256)]["KS"], p[(16, 256)]["chunk_units"], p[(16, 256)]["ntiles"], p[(16, 256)]["WPT"]) == (1, 1, 1, 1)
    assert p[(48, 512)]["ntiles"] == 3 and p[(48, 512)]["NT"] == 1
    assert p[(16384, 256)]["NT"] == 2
    assert p[(64, 14336)]["KS"] > 1 and p[(64, 14336)]["WPT"] > 1
    q = p[(4112, 4352)]
    assert q["ntiles"] == 257 and (q["ntiles"] % q["T"] != 0 or q["T"] == 1)


@pytest.mark.parametrize("N,K", SHAPES + ((4096, 4096), (6144, 4096), (28672, 4096), (4096, 14336)))
def test_plan_invariants(N, K):
    """as tests/test_decode_plan_cpu.py states them for the other kinds: one workspace figure per shape, LDS within budget, grid >= 1"""
    figs = set()
    for B in (1, 16, 17, 32, 33, 64):
        p = _plan(N, K, B)
        figs.add(p["partial_floats"])
        assert p["NB"] == (1 if B <= 16 else 2 if B <= 32 else 4)
        assert p["KS"] >= 1 and p["grid"] >= 1 and p["KS"] * p["chunk_units"] >= K // 256
        assert (p["KS"] - 1) * p["chunk_units"] < K // 256                      # no empty chunk
        assert p["KS"] * 256 * N <= p["partial_floats"]
        assert p["lds_bytes"] <= 160 * 1024
        assert p["lds_bytes"] >= p["chunk_units"] * 8 * p["NB"] * 1024          # eight 1 KB activation images per unit and row group
        assert p["threads"] % 64 == 0 and 64 <= p["threads"] <= 512
        assert p["grid"] == p["KS"] * -(-p["ntiles"] // p["T"])
    assert len(figs) == 1


def test_plan_and_route_refuse_what_the_kernel_does_not_take():
    from trace_amd import _lib
    from trace_amd.engine import ops
    _plan(16, 256, 1)
    for N, K, B in ((16, 128, 1), (16, 384, 1), (24, 256, 1), (16, 256, 65), (16, 256, 0), (8, 256, 1)):
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_skinny_w4_plan"):
            ops.skinny_w4_plan(N, K, B)
    # the older entry points keep refusing kind / scheme 3
    with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_skinny_plan"):
        ops.skinny_plan(3, 4096, 4096, 4, 1)
    with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_decode_route"):
        ops.decode_route(1, 3, 4096, 14336, 6144)
    for B in (1, 3, 16, 33, 64):
        r = ops.decode_route_w4(B, 4096, 14336, 6144)
        assert r["step"] == 1 and r["kind"] == 3
        assert (r["ks_q"], r["ks_o"], r["ks_g"], r["ks_d"]) == tuple(ops.skinny_w4_plan(N, K, B)["KS"] for N, K in ((6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)))
    for bad in ((65, 4096, 14336, 6144), (0, 4096, 14336, 6144), (1, 4096 + 128, 14336, 6144), (1, 4096, 14336 + 128, 6144)):
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_decode_route_w4"):
            ops.decode_route_w4(*bad)


def test_create_opts_refuses_bad_w4_combinations_before_any_device_call():
    from trace_amd import build, _lib
    build.build()
    assert C.sizeof(_lib.TraceCtxOptsC) == 8 and C.sizeof(_lib.TraceCtxOptsW4C) == 12

    def create(lib, c, o):
        h = C.c_void_p()
        try:
            lib.trace_ctx_create_opts(C.byref(c), 0, C.cast(C.byref(o), C.POINTER(_lib.TraceCtxOptsC)), C.byref(h))
        finally:
            assert not h.value
    lib = _lib.load("bf16")
    c = _lib.TraceConfigC()
    c.hidden_size, c.intermediate_size = 4096, 256
    with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: llm_weights_w4 must be 0 or 1"):
        create(lib, c, _lib.TraceCtxOptsW4C(12, 0, 2))
    with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: llm_weights_w4 with kv_cache_fp8"):
        create(lib, c, _lib.TraceCtxOptsW4C(12, 1, 1))
    c.llm_weights_fp8 = 2
    with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: llm_weights_w4 with llm_weights_fp8"):
        create(lib, c, _lib.TraceCtxOptsW4C(12, 0, 1))
    c.llm_weights_fp8 = 0
    c.intermediate_size = 384
    with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: w4 weight path needs hidden / intermediate"):
        create(lib, c, _lib.TraceCtxOptsW4C(12, 0, 1))
    c.intermediate_size = 256
    with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: trace_ctx_opts::size"):
        create(lib, c, _lib.TraceCtxOptsW4C(4, 0, 1))
    with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: llm_weights_w4 needs the bf16 library"):
        create(_lib.load("f16"), c, _lib.TraceCtxOptsW4C(12, 0, 1))
    # the w4 kernels' hooks in the fp16 library answer before any device call as well
    with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_op_quant_rows_w4: the w4 kernels need the bf16 library"):
        _lib.load("f16").trace_op_quant_rows_w4(None, None, None, 16, 256, None)


def test_engine_argument_checks_come_before_any_device_work():
    from trace_amd import config as tcfg
    from trace_amd.engine import TraceEngine
    for bad in ("yes", 1.5, "w4", 2):
        with pytest.raises(ValueError, match="llm_w4 must be False or True"):
            TraceEngine(tcfg.tiny(), llm_w4=bad)
    with pytest.raises(ValueError, match="llm_w4 with llm_fp8"):
        TraceEngine(tcfg.tiny(), llm_w4=True, llm_fp8="weight_only")
    with pytest.raises(ValueError, match="llm_w4 with kv_cache='fp8'"):
        TraceEngine(tcfg.tiny(), llm_w4=True, kv_cache="fp8")
    with pytest.raises(ValueError, match="w4 weight path exists in the bf16 library only"):
        TraceEngine(tcfg.tiny(), llm_w4=True, dtype=torch.float16)
    cfg = tcfg.tiny()
    cfg.intermediate_size = 384
    with pytest.raises(ValueError, match="multiples of 256"):
        TraceEngine(cfg, llm_w4=True)


def test_load_4bit_reaches_the_device(tmp_path):
    """load_4bit=True no longer raises NotImplementedError: without a device it gets as far as the engine's "no HIP device", with one it loads"""
    from trace_amd import _lib, config as tcfg
    from trace_amd.model import builder
    path = builder.save_synthetic_checkpoint(str(tmp_path / "ck"), tcfg.tiny())
    if torch.cuda.is_available():
        _, model, _, _ = builder.load_pretrained_model(path, None, "trace-tiny", load_4bit=True, max_new_tokens=8)
        assert model.engine.llm_w4 and model.engine.lib.trace_ctx_llm_weights_type(model.engine.h) == 3
        model.engine.close()
    else:
        with pytest.raises(_lib.TraceHipError, match="no HIP device"):
            builder.load_pretrained_model(path, None, "trace-tiny", load_4bit=True)
    with pytest.raises(NotImplementedError, match=r'kv_cache="fp8".*llm_fp8'):
        builder.load_pretrained_model(path, None, "trace-tiny", load_8bit=True)
