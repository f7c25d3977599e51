"""The decode-row probes judged on the CPU (tests/decode_row_probes.py): the float64 references agree with the oracle's RMSNorm and SwiGLU, the
e4m3 rounder is torch.float8_e4m3fn's on the code table, the fault-free torch emulations of the four kernels pass the judge at every shape
tests/test_gpu_decode_row_probes.py runs, every listed fault is rejected by a named probe, and a table states which of those faults the Gaussian
checks of tests/test_gpu_kernels.py (test_skinny_gemm's x within 2^-6 of the row maximum and check(.., 2e-2, 1e-2) on y, check(.., 3e-2, 1e-2) on
the SwiGLU rows; test_skinny_gemv_with_fused_add_rmsnorm's check(.., 2e-2, 1e-2) on the product) accept — the reason this file exists."""
from types import SimpleNamespace

import pytest
import torch

import decode_row_probes as DP
import encode_probes as EP
from oracle import trace_oracle as O

BF, HF = torch.bfloat16, torch.float16
DTYPES = [BF, HF]
IDS = ["bf16", "f16"]
INF = float("inf")


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- references against the oracle, the rounder against torch ------------------------------------------------------------------------------------
def test_references_are_the_oracles():
    x, w = _randn(5, 252, seed=1) * 2, 1 + 0.1 * _randn(252, seed=2)
    for eps in (1e-5, 1e-6):
        ora = O.Oracle._rms(SimpleNamespace(cfg=SimpleNamespace(rms_norm_eps=eps)), x, w)
        R = EP.norm_reference(x, w, None, eps, BF, rms=True)
        assert torch.allclose(ora.double(), R.ref, rtol=1e-5, atol=1e-6)
    pr = DP.swiglu_probe("gaussian", 3, 64, 5, BF)
    pre, _ = DP.swiglu_reference(pr)
    g, u = pr.G.float(), pr.U.float()
    assert torch.allclose((torch.nn.functional.silu(g) * u).double(), pre, rtol=1e-5, atol=1e-6)        # the oracle's expression (llm_forward)
    pr = DP.swiglu_probe("chunk-pointer", 3, 64, 5, BF)
    gg, uu = EP.GP.swiglu_split(DP.lay_part(pr.vals)[:5, :3].double().sum(0))
    assert torch.equal(gg, pr.G) and torch.equal(uu, pr.U), "interleave() is gemm_probes.swiglu_split's inverse"


def test_e4m3_rounder_is_torchs_on_the_code_table():
    codes = torch.arange(256, dtype=torch.uint8)
    v = codes.view(torch.float8_e4m3fn).double()
    fin = ~torch.isnan(v)
    assert int(fin.sum()) == 254
    assert torch.equal(DP.e4m3_decode(codes)[fin], v[fin]) and torch.equal(DP.e4m3_round(v[fin]), codes[fin])
    t = DP.e4m3_values()
    assert t.numel() == 127 and float(t[1]) == 2.0 ** -9 and float(t[8]) == 2.0 ** -6 and float(t[-1]) == 448.0
    mid = (t[1:] + t[:-1]) / 2
    pts = torch.cat([mid, -mid, torch.zeros(1)])                                                        # 253 midpoints; across zero: 0 itself
    want = pts.float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(DP.e4m3_round(pts)[:-1], want[:-1])
    for dtype in DTYPES:                                                                                # and the whole table of the code-table probe
        tv = DP.code_table_values(dtype)
        assert torch.equal(DP.e4m3_round(tv), tv.float().to(torch.float8_e4m3fn).view(torch.uint8))
        assert bool((tv.to(dtype).double() == tv).all())
    assert torch.equal(DP.e4m3_round(torch.tensor([1e9, -1e9, 449.0], dtype=torch.float64)), torch.tensor([0x7E, 0xFE, 0x7E], dtype=torch.uint8))
    even = (DP.e4m3_round(mid).to(torch.int64) & 1) == 0
    assert bool(even.all()), "ties go to the even code"
    assert int((DP.e4m3_round(mid, "ties_away") != DP.e4m3_round(mid)).sum()) == 63 and int((DP.e4m3_round(mid, "truncate") != DP.e4m3_round(mid)).sum()) == 63


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_probe_properties(dtype):
    p = DP.P_BITS[dtype]
    pr = DP.add_probe("ties", 5, 1024, 9, dtype)
    s = pr.vals.sum(0)
    assert bool((s.abs() % 2 == 1).all()) and bool((s.abs() >= 2 ** p).all()) and bool((s.abs() < 2 ** (p + 1)).all()), "every sum is a 16-bit tie"
    r = DP.round16(s, dtype).double()
    assert 0.3 < float((r.abs() > s.abs()).double().mean()) < 0.7, "both parities: the even neighbour is above for some, below for others"
    second = (r + pr.R.double()).abs()
    assert float(((second % 2 == 1) & (second < 2 ** (p + 1))).double().mean()) > 0.9, "el(sum) + R is a tie again"
    pr = DP.add_probe("double-rounding", 5, 1024, 9, dtype)
    s = pr.vals.sum(0)
    x, _ = DP.x_reference(pr)
    assert bool((x.double() != DP.round16(s + pr.R.double(), dtype, exact=False).double()).all()), "the inner rounding shows on every element"
    pr = DP.add_probe("chunk-pointer", 3, 252, 7, dtype)
    assert bool(((pr.vals != 0).sum(0) == 1).all()), "one chunk per column"
    x = DP.quant_probe("code-table", 256, dtype)
    v, _ = DP.quant_reference(x)
    have = set(v.abs().flatten().tolist())
    t = DP.e4m3_values()
    assert set(t.tolist()) <= have and set(((t[1:] + t[:-1]) / 2).tolist()) <= have, "every value and every midpoint, after the exact scaling"
    assert len(DP.add_cases()) == 48
    for ax, i in ((DP.ADD_N, 0), (DP.ADD_B, 1), (DP.ADD_KS, 2)):
        for val in ax:                                                                                   # every value with the extremes of the others
            others = {tuple(c[j] for j in range(3) if j != i) for c in DP.add_cases() if c[i] == val}
            assert len(others) >= 4
    assert set(p_ for c in DP.add_cases() for p_ in c[3]) == set(DP.ADD_PROBES)


# ---- add_rmsnorm ---------------------------------------------------------------------------------------------------------------------------------------
def emulated_add(dtype, fault=None):
    def fn(pr, part, L, fp8):
        return DP.emulate_add_rmsnorm(part, pr.KS, L.Rb, L.ldr, L.xb, L.ldx, pr.w, L.yb, L.ldy, pr.B, pr.N, pr.eps, dtype, fp8, fault)
    return fn


def add_verdict(name, B, N, KS, dtype, fault=None, form="pad", fp8=True):
    ratios, intact = DP.run_add(DP.add_probe(name, B, N, KS, dtype), emulated_add(dtype, fault), form, fp8)
    return intact and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_rmsnorm_emulation_passes_at_the_gpu_shapes(dtype):
    worst = {}
    for i, (N, B, KS, probes) in enumerate(DP.add_cases()):
        for name in probes:
            if name == "tiny-row" and dtype != BF:
                continue
            form = ("pad", "inplace")[i % 2]
            ok, ratios = add_verdict(name, B, N, KS, dtype, None, form)
            assert ok, (name, B, N, KS, form, ratios)
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print({k: round(v, 3) for k, v in worst.items()})


# fault -> (probe, B, N, KS, form) that rejects it
ADD_REJECTED_BY = {
    "chunk_tail_dropped": ("chunk-pointer", 3, 252, 9, "pad"),
    "chunk_stride_is_B": ("chunk-pointer", 3, 252, 9, "pad"),
    "inner_rounding_skipped": ("double-rounding", 3, 252, 9, "pad"),
    "stats_from_unrounded_x": ("ties-up", 3, 1024, 9, "pad"),
    "mean_over_4096": ("ramp/R", 3, 252, 1, "pad"),
    "eps_dropped": ("eps/split", 3, 1024, 7, "pad"),
    "idle_threads_counted": ("onehot/R", 3, 252, 1, "pad"),
    "ldr_ignored": ("chunk-pointer", 3, 252, 9, "pad"),
    "ldx_ignored": ("chunk-pointer", 3, 252, 9, "pad"),
    "ldy_ignored": ("ramp/split", 3, 252, 9, "pad"),
    "amax_from_unrounded_y": ("massive", 65, 1024, 8, "inplace"),
    "zero_row_scale_0": ("zero-row", 3, 252, 9, "inplace"),
    "reciprocal_unguarded": ("tiny-row", 3, 252, 1, "inplace"),
}


@pytest.mark.parametrize("fault", sorted(ADD_REJECTED_BY))
def test_add_rmsnorm_fault_is_rejected(fault):
    name, B, N, KS, form = ADD_REJECTED_BY[fault]
    for dtype in DTYPES if name != "tiny-row" else [BF]:
        ok, ratios = add_verdict(name, B, N, KS, dtype, fault, form)
        assert not ok, (fault, name, ratios)
        assert add_verdict(name, B, N, KS, dtype, None, form)[0]


def test_every_add_fault_has_a_probe():
    assert set(DP.ADD_FAULTS) | {"reciprocal_unguarded"} == set(ADD_REJECTED_BY)


def test_ties_alone_do_not_pin_the_inner_rounding_order_but_double_rounding_does():
    """el(s) + R vs s + R: on `ties` the two differ as well (odd + odd is even and exact); `double-rounding` is the probe built for it"""
    assert not add_verdict("ties", 3, 252, 9, BF, "inner_rounding_skipped")[0]


# ---- quantiser ---------------------------------------------------------------------------------------------------------------------------------------------
def quant_verdict(name, K, dtype, fault=None):
    x = DP.quant_probe(name, K, dtype)
    codes, sy = DP.emulate_quant(x, fault)
    ratios = DP.judge_quant_probe(name, x, codes, sy)
    return max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_quantiser_emulation_passes_at_the_gpu_shapes(dtype):
    for K in (256, 4096, 14336):
        for name in DP.QUANT_PROBES:
            ok, ratios = quant_verdict(name, K, dtype)
            assert ok, (name, K, ratios)


QUANT_REJECTED_BY = {"truncate": "code-table", "ties_away": "code-table", "subnormals_flushed": "code-table", "amax_without_abs": "zero-row",
                     "scale_of_unclamped": "last-ulp", "reciprocal_unguarded": "tiny-row"}


@pytest.mark.parametrize("fault", DP.QUANT_FAULTS)
def test_quantiser_fault_is_rejected(fault):
    for dtype in DTYPES if fault != "reciprocal_unguarded" else [BF]:
        ok, ratios = quant_verdict(QUANT_REJECTED_BY[fault], 256, dtype, fault)
        assert not ok, (fault, ratios)


def test_unguarded_reciprocal_is_what_the_issue_says():
    """0 < amax < 448 / FLT_MAX: 448 / amax is inf in fp32, a zero element becomes NaN and leaves fminf(fmaxf(., -448), 448) as -448 (code 0xFE)"""
    x = DP.quant_probe("tiny-row", 256, BF)
    codes, sy = DP.emulate_quant(x, "reciprocal_unguarded")
    assert bool((codes[1][x[1] == 0] == 0xFE).all()) and float(sy[1]) == float(torch.tensor(2.0 ** -121) / 448)
    codes, sy = DP.emulate_quant(x)
    assert bool((codes[1][x[1] == 0] == 0).all()) and float(sy[1]) == float(torch.tensor(2.0 ** -121) / 448)
    big = DP.quant_probe("zero-row", 256, BF)                   # the guard leaves every other row's bits alone
    a, b = DP.emulate_quant(big), DP.emulate_quant(big, "reciprocal_unguarded")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- swiglu ---------------------------------------------------------------------------------------------------------------------------------------------------
SWIGLU_N2, SWIGLU_B, SWIGLU_KS = (32, 1024, 28672), (1, 4, 64, 256), (1, 3, 4, 5, 8)


def swiglu_verdict(name, B, N2, KS, dtype, fault=None):
    pr = DP.swiglu_probe(name, B, N2, KS, dtype)
    got = DP.emulate_swiglu(DP.lay_part(pr.vals), KS, B, N2, dtype, fault)
    r = DP.swiglu_ratio(got, pr)
    return r <= 1.0, r


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_swiglu_emulation_passes_at_the_gpu_shapes(dtype):
    for N2 in SWIGLU_N2:
        for B in SWIGLU_B:
            for KS in SWIGLU_KS:
                big = N2 == 28672 and B >= 64                        # (hundreds of MB in float64 on the CPU: one probe, the ends of the unroll)
                if big and KS not in (1, 5, 8):
                    continue
                for name in (("chunk-pointer",) if big else ("chunk-pointer", "gaussian")):
                    ok, r = swiglu_verdict(name, B, N2, KS, dtype)
                    assert ok, (name, B, N2, KS, r)
    for N, K, B in ((64, 64, 1), (1024, 1024, 4), (4096, 14336, 4)):     # the SwiGLU prologue's shapes (the same emulation: it restates the kernel)
        for KS in (1, 3, 4, 5):
            for name in ("chunk-pointer", "gaussian"):
                ok, r = swiglu_verdict(name, B, 2 * K, KS, dtype)
                assert ok, (name, B, K, KS, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gate_range_on_the_emulation(dtype):
    """g / (1 + exp(-g)) in fp32: exp(89) is inf and the plain quotient is -0 where float64 has -89 e^-89 = -2.0e-37.  fp16 cannot hold that (the
    floor of one smallest normal covers it); bf16 can — 17 smallest normals — so the unguarded formula is OUTSIDE the judge in bf16 at gate -89, up
    +-1, and nowhere else.  The kernels' guarded form (e^g as e^(g + 64) e^-64) is inside at every gate."""
    for KS in (1, 5):
        pr = DP.swiglu_probe("gate-range", 4, 2048, KS, dtype)
        assert {float(v) for v in pr.G.flatten()} == set(DP.GATES) and {float(v) for v in pr.U.flatten()} == {-1.0, 0.0, 1.0}
        part = DP.lay_part(pr.vals)
        assert DP.swiglu_ratio(DP.emulate_swiglu(part, KS, 4, 2048, dtype), pr) <= 1.0
        bad = DP.swiglu_ratio_map(DP.emulate_swiglu(part, KS, 4, 2048, dtype, "exp_overflow_unguarded"), pr) > 1
        if dtype == HF:
            assert not bool(bad.any())
        else:
            assert bool(bad.any()) and bool((pr.G[bad] == -89.0).all()) and bool((pr.U[bad] != 0).all())


SWIGLU_REJECTED_BY = {"gate_up_swapped": ("chunk-pointer", 4, 1024, 5), "interleave_8_not_16": ("chunk-pointer", 4, 1024, 5),
                      "chunk_tail_dropped": ("chunk-pointer", 4, 1024, 5), "silu_of_rounded_gate": ("chunk-pointer", 4, 1024, 5),
                      "chunk_stride_is_B": ("chunk-pointer", 4, 1024, 5), "exp_overflow_unguarded": ("gate-range", 4, 2048, 5)}


@pytest.mark.parametrize("fault", DP.SWIGLU_FAULTS)
def test_swiglu_fault_is_rejected(fault):
    name, B, N2, KS = SWIGLU_REJECTED_BY[fault]
    for dtype in DTYPES if fault != "exp_overflow_unguarded" else [BF]:          # (fp16 cannot hold silu(-89): nothing to reject there)
        ok, r = swiglu_verdict(name, B, N2, KS, dtype, fault)
        assert not ok and swiglu_verdict(name, B, N2, KS, dtype)[0], (fault, r)


# ---- fused-norm prologue -----------------------------------------------------------------------------------------------------------------------------------
def fused_verdict(name, B, K, ks_in, dtype, fault=None, KS_out=2, chunk_units=None):
    cu = chunk_units or -(-(K // 64) // KS_out)
    pr = DP.add_probe(name, B, K, max(ks_in, 1), dtype)
    part = DP.lay_part(pr.vals)
    if ks_in == 0:
        pr.vals = pr.vals * 0
    xout, parked = DP.emulate_fused_norm(part, ks_in, pr.R, pr.w, pr.eps, dtype, KS_out, cu, fault)
    rx = DP.x_ratio(xout, pr)
    ry = DP.y_ratio(parked, xout, pr) if rx <= 1 else INF
    return max(rx, ry) <= 1.0, {"x": rx, "y": ry}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_norm_emulation_passes(dtype):
    for K in (64, 1024, 4096):
        for B in (1, 4):
            for ks_in in (0, 1, 7, 8):
                for name in ("chunk-pointer", "ramp/split", "massive", "ties"):
                    ok, r = fused_verdict(name, B, K, ks_in, dtype, KS_out=1 if K == 64 else 3)
                    assert ok, (name, B, K, ks_in, r)


FUSED_REJECTED_BY = {"stats_over_own_chunk": ("massive", 7), "half_swapped": ("ramp/split", 7), "unit_shifted": ("ramp/split", 7),
                     "xout_from_every_row_group_with_stale_R": ("chunk-pointer", 7), "xout_missing_last_chunk": ("chunk-pointer", 7)}


@pytest.mark.parametrize("fault", DP.FUSED_NORM_FAULTS)
def test_fused_norm_fault_is_rejected(fault):
    name, ks_in = FUSED_REJECTED_BY[fault]
    for dtype in DTYPES:
        ok, r = fused_verdict(name, 3, 1024, ks_in, dtype, fault, KS_out=3)
        assert not ok and fused_verdict(name, 3, 1024, ks_in, dtype, None, KS_out=3)[0], (fault, r)


def test_selection_matrix_reads_the_parked_row_back():
    """on the CPU: out[c] = parked[:, chunk c] . W[:, chunk c]^T for a selection matrix returns every parked value exactly, in one chunk"""
    for N, K, cu, KS in ((1024, 1024, 6, 3), (256, 1024, 16, 1)):
        for off in DP.offsets_covering(N, K):
            W = DP.selection_matrix(N, K, BF, off)
            assert bool(((W != 0).sum(1) == 1).all())
            parked = (_randn(3, K, seed=K + off)).to(BF)
            out = torch.zeros((KS, DP.SK_ROWS, N))
            for c in range(KS):
                k0, k1 = c * cu * 64, min(K, (c + 1) * cu * 64)
                out[c, :3] = parked[:, k0:k1].float() @ W[:, k0:k1].float().t()
            got, looked, zeros_ok = DP.read_parked(out, 3, N, K, cu, off)
            assert zeros_ok and int(looked.sum()) == N and torch.equal(got[:, looked], parked.float()[:, looked])
        seen = torch.zeros(K, dtype=torch.bool)
        for off in DP.offsets_covering(N, K):
            seen[DP.sel_of(N, K, off)] = True
        assert bool(seen.all())


# ---- what the Gaussian checks accept ---------------------------------------------------------------------------------------------------------------------------
def old_check(got, ref, atol, rtol):
    got, ref = got.float(), ref.float()
    return bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())


def old_add_check_accepts(fault, B=2, N=512, KS=9):
    """test_skinny_gemm's judgement of add_rmsnorm, on Gaussian rows: contiguous buffers, zeros where nothing was written (so the stride faults
    cannot show at all: that test has no strides)"""
    part = torch.zeros((KS, DP.SK_ROWS, N))
    part[:, :B] = _randn(KS, B, N, seed=3) * 0.5
    R, w = _randn(B, N, seed=4).to(BF), _randn(N, seed=9).to(BF)
    xb, yb = torch.zeros((B, N), dtype=BF), torch.zeros((B, N), dtype=BF)
    DP.emulate_add_rmsnorm(part, KS, R, N, xb, N, w, yb, N, B, N, 1e-5, BF, False, fault)
    xr = (part[:, :B].sum(0).to(BF).float() + R.float()).to(BF)
    ok_x = bool(((xb.float() - xr.float()).abs().max() <= 2 ** -6 * xr.float().abs().max()))
    xf = xb.float()
    return ok_x and old_check(yb, xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-5) * w.float(), 2e-2, 1e-2)


def old_swiglu_check_accepts(fault, B=2, N2=512, KS=5):
    pr = DP.swiglu_probe("gaussian", B, N2, KS, BF)
    part = torch.zeros((KS, DP.SK_ROWS, N2))
    part[:, :B] = pr.vals.float()
    got = DP.emulate_swiglu(part, KS, B, N2, BF, fault)
    return old_check(got, torch.nn.functional.silu(pr.G.float()) * pr.U.float(), 3e-2, 1e-2)


def old_fused_check_accepts(fault, B=4, N=512, K=4096, ks_in=2):
    """test_skinny_gemv_with_fused_add_rmsnorm at its (4, 512, 4096, 2) case, cut as the library's own plan cuts it: xout bit equal to add_rmsnorm's,
    the product against the unfused pair's at 2e-2 / 1e-2"""
    import ctypes as C
    from trace_amd import _lib
    plan = (C.c_int64 * 11)()
    _lib.check(_lib.load().trace_op_skinny_plan(0, N, K, 4, B, plan))
    KS_out, cu = int(plan[0]), int(plan[1])
    part = torch.zeros((ks_in, DP.SK_ROWS, K))
    part[:, :B] = _randn(ks_in, B, K, seed=5) * 0.3
    R, w, W = _randn(B, K, seed=1).to(BF), (1 + 0.2 * _randn(K, seed=2)).to(BF), (_randn(N, K, seed=3) * 0.05).to(BF)
    xout, parked = DP.emulate_fused_norm(part, ks_in, R, w, 1e-5, BF, KS_out, cu, fault)
    xr, yr = torch.zeros_like(R), torch.zeros_like(R)
    DP.emulate_add_rmsnorm(part, ks_in, R, K, xr, K, w, yr, K, B, K, 1e-5, BF)
    return torch.equal(xout, xr) and old_check(parked.float() @ W.float().t(), yr.float() @ W.float().t(), 2e-2, 1e-2)


ACCEPTED_BY_THE_GAUSSIAN_CHECKS = {
    "add_rmsnorm": {"inner_rounding_skipped", "stats_from_unrounded_x", "eps_dropped", "ldr_ignored", "ldx_ignored", "ldy_ignored",
                    "amax_from_unrounded_y", "zero_row_scale_0"},
    "swiglu": {"silu_of_rounded_gate", "exp_overflow_unguarded"},
    # none: a Gaussian row's K-chunks differ in energy by a percent or two, which the product tolerance does notice at K = 4096, and the Gaussian
    # weights are not smooth, so exchanged groups show too — by margin, not by construction (the probes above reject each of them outright)
    "fused norm": set(),
}


def test_what_the_gaussian_checks_accept():
    got = {"add_rmsnorm": {f for f in DP.ADD_FAULTS if old_add_check_accepts(f)},
           "swiglu": {f for f in DP.SWIGLU_FAULTS if old_swiglu_check_accepts(f)},
           "fused norm": {f for f in DP.FUSED_NORM_FAULTS if old_fused_check_accepts(f)}}
    print(got)
    assert old_add_check_accepts(None) and old_swiglu_check_accepts(None) and old_fused_check_accepts(None)
    assert got == ACCEPTED_BY_THE_GAUSSIAN_CHECKS
