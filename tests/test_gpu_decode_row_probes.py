"""The decode step's row kernels against float64 (tests/decode_row_probes.py; tests/test_decode_row_probes_cpu.py shows on the CPU which faults these
probes reject and which of them the Gaussian checks of test_gpu_kernels.py let through): add_rmsnorm_kernel through trace_op_add_rmsnorm_ex — out of
place with padded strides and in place as the engine calls it, with and without its e4m3 tail — swiglu_combine_kernel, quant_rows_fp8_kernel, and the
two fused prologues of skinny_lds_kernel read back through a selection matrix.

One judge (decode_row_probes): x bit equal (gaussian: two half ulps + the fp32 sum's E), y by encode_probes.bound, SwiGLU by gemm_probes.act_bound,
e4m3 codes nearest-even up to 2^-22 of a tie, scales to one fp32 ulp.  The largest error / bound per kernel and probe is printed and appended to the
file the environment variable TRACE_DECODE_ROW_PROBE_MARGINS names (profiles/decode_row_probe_margins.txt is made from it).  Both libraries run every
entry the fp16 library accepts; it refuses the e4m3 tail of add_rmsnorm (it has no fp8 weight path).

Two defects these probes exposed are fixed with them: zeros of a row with 0 < amax < 448 / FLT_MAX were quantised to -448 (tiny-row), and
the two SwiGLU row kernels flushed silu(g) u to 0 below the fp32 overflow of exp(-g) at g = -88.7, where bf16 still holds it (gate-range, bf16
library: error / bound 15.9 at gate -89 before the fix)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import decode_row_probes as DP  # noqa: E402
from trace_amd import _lib  # noqa: E402
from trace_amd.engine import ops  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
MARGINS = {}                      # (library, kernel, probe) -> [max err / bound, cases]


@pytest.fixture(scope="module", autouse=True)
def margins_record():
    yield
    lines = [f"{lib:<5} {k:<24} {p:<18} max err/bound {m[0]:.4f}  cases {m[1]}" for (lib, k, p), m in sorted(MARGINS.items())]
    print("\n".join(lines))
    path = os.environ.get("TRACE_DECODE_ROW_PROBE_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(params=["bf16", "f16"])
def el(request):
    ops.use(request.param)
    yield request.param
    ops.use("bf16")


def record(el, kernel, probe, ratio):
    m = MARGINS.setdefault((el, kernel, probe), [0.0, 0])
    m[0], m[1] = max(m[0], ratio), m[1] + 1


def judge(el, kernel, probe, ratios, what):
    """ratios: {quantity: error / bound}; each goes to the margins under `kernel quantity`, then all must be <= 1"""
    for q, r in ratios.items():
        record(el, f"{kernel} {q}", probe, r)
    assert max(ratios.values()) <= 1.0, f"{kernel} {probe} {what}: error / bound {ratios}"


# ---- add_rmsnorm_ex -------------------------------------------------------------------------------------------------------------------------------------
def device_add(pr, part, L, fp8):
    r = ops.add_rmsnorm_ex(part, L.Rv, pr.w, pr.eps, KS=pr.KS, xout=L.xv, y=L.yv, fp8=fp8)
    return (r[2], r[3]) if fp8 else (None, None)


@pytest.mark.parametrize("N,B,KS,probes", DP.add_cases(), ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_add_rmsnorm(el, N, B, KS, probes):
    dtype = DTYPES[el]
    assert ops.sk_rows() == DP.SK_ROWS
    fp8_lib = el == "bf16"
    for name in probes:
        if name == "tiny-row" and not fp8_lib:
            continue
        pr = DP.add_probe(name, B, N, KS, dtype, DEV)
        for form, fp8 in ((("pad", False), ("pad", True), ("inplace", True)) if fp8_lib else (("pad", False), ("inplace", False))):
            ratios, intact = DP.run_add(pr, device_add, form, fp8)
            judge(el, "add_rmsnorm", name, ratios, f"B {B} N {N} KS {KS} {form} fp8 {fp8}")
            assert intact, f"add_rmsnorm {name} B {B} N {N} KS {KS} {form}: a store outside the output rows, or the residual rows changed"
        if fp8_lib and N % 8 == 0:                                         # "exactly as quant_rows_fp8 would": the same bytes and scales
            x, y, y8, sy = ops.add_rmsnorm_ex(DP.lay_part(pr.vals), pr.R, pr.w, pr.eps, KS=KS, fp8=True)
            q, sq = ops.quant_rows_fp8(y)
            assert torch.equal(y8, q) and torch.equal(sy, sq), f"add_rmsnorm {name} B {B} N {N} KS {KS}: y8 / sy differ from quant_rows_fp8(y)"


def test_add_rmsnorm_refusals(el):
    dtype = DTYPES[el]
    SK = ops.sk_rows()

    def call(B=2, N=64, KS=2, pr=0, px=0, py=0, fp8=False, ks_arg=None):
        part = torch.zeros((max(KS, 1), SK, N), dtype=torch.float32, device=DEV)
        bufs = [torch.zeros((B, N + p), dtype=dtype, device=DEV)[:, :N] for p in (pr, px, py)]
        return ops.add_rmsnorm_ex(part, bufs[0], torch.ones(N, dtype=dtype, device=DEV), 1e-5, KS=KS if ks_arg is None else ks_arg, xout=bufs[1],
                                  y=bufs[2], fp8=fp8)

    call()
    call(pr=4, px=8, py=12)
    for kw in (dict(N=62), dict(N=4100), dict(B=SK + 1), dict(ks_arg=0), dict(ks_arg=-1), dict(pr=2), dict(px=2), dict(py=2), dict(pr=1), dict(py=3)):
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_add_rmsnorm_ex"):
            call(**kw)
    if el == "f16":                                                       # no fp8 weight path in the fp16 library: the e4m3 tail is refused
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_add_rmsnorm_ex: y8 / sy need the bf16 library"):
            call(fp8=True)
    else:
        call(fp8=True)
    lib = _lib.load(el)
    z = torch.zeros((2, 64), dtype=dtype, device=DEV)
    part = torch.zeros((1, SK, 64), dtype=torch.float32, device=DEV)
    y8 = torch.zeros((2, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.TraceHipError, match="y8 and sy go together"):
        _lib.check(lib.trace_op_add_rmsnorm_ex(part.data_ptr(), 1, z.data_ptr(), 64, z.data_ptr(), 64, z.data_ptr(), z.data_ptr(), 64, y8.data_ptr(), None,
                                               2, 64, 1e-5, None))


# ---- swiglu_combine ---------------------------------------------------------------------------------------------------------------------------------------
SWIGLU_KS = (1, 3, 4, 5, 8)


@pytest.mark.parametrize("B", [1, 4, 64, 256])
@pytest.mark.parametrize("N2", [32, 1024, 28672])
def test_swiglu_combine(el, N2, B):
    dtype = DTYPES[el]
    for KS in SWIGLU_KS:
        for name in ("chunk-pointer", "gaussian"):
            pr = DP.swiglu_probe(name, B, N2, KS, dtype, DEV)
            part = DP.lay_part(pr.vals)
            got = ops.swiglu_combine(part[:KS], B)                         # KS from the tensor's shape; the NaN chunks lie right behind it
            judge(el, "swiglu_combine", name, {"out": DP.swiglu_ratio(got, pr)}, f"B {B} N2 {N2} KS {KS}")


def gate_range_report(got, pr):
    m = DP.swiglu_ratio_map(got, pr)
    bad = m > 1
    gates = sorted(set(pr.G[bad].tolist()))
    return float(m.max()), int(bad.sum()), gates


@pytest.mark.parametrize("KS", [1, 5])
def test_swiglu_gate_range(el, KS):
    """gates 0, +-2^-20, +-1, +-16, +-87, +-89, +-128 against ups +-1 and 0, through swiglu_combine and through the SwiGLU prologue (bit equal to
    it).  At gate -89 exp(-g) is inf in fp32 while bf16 still holds silu(-89) = -2.0e-37: the kernels' guarded form is what keeps that inside."""
    dtype = DTYPES[el]
    B, K = 4, 1024
    pr = DP.swiglu_probe("gate-range", B, 2 * K, KS, dtype, DEV)
    part = DP.lay_part(pr.vals)
    got = ops.swiglu_combine(part[:KS], B)
    worst, n, gates = gate_range_report(got, pr)
    print(f"{el} swiglu_combine gate-range KS {KS}: worst error / bound {worst:.3f}, {n} elements outside, at gates {gates}")
    out = ops.skinny_fused_swiglu(part, selection(K, K, dtype), B, KS=KS)
    parked, looked, ok = DP.read_parked(out, B, K, K, ops.skinny_plan(0, K, K, 4, B)["chunk_units"])
    assert ok and bool(looked.all()) and bool((parked == got.float()).all()), "the SwiGLU prologue differs from swiglu_combine"
    judge(el, "swiglu_combine", "gate-range", {"out": worst}, f"B {B} N2 {2 * K} KS {KS}: {n} elements outside, at gates {gates}")


# ---- the fused-norm GEMV ------------------------------------------------------------------------------------------------------------------------------------
FUSED_PROBES = ("chunk-pointer", "ties", "ramp/split", "onehot/R", "massive", "zero-row", "gaussian")
_SEL = {}


def selection(N, K, dtype, off=0):
    if (N, K, dtype, off) not in _SEL:
        if len(_SEL) > 8:
            _SEL.clear()
        _SEL[(N, K, dtype, off)] = DP.selection_matrix(N, K, dtype, off, DEV)
    return _SEL[(N, K, dtype, off)]


def fused_norm_case(el, B, N, K, ks_in, name):
    dtype = DTYPES[el]
    pr = DP.add_probe(name, B, K, max(ks_in, 1), dtype, DEV)
    part = DP.lay_part(pr.vals)
    if ks_in == 0:
        pr.vals = pr.vals * 0
    plan = ops.skinny_plan(0, N, K, 4, B)
    xout, out = ops.skinny_fused_norm(part, pr.R, pr.w, pr.eps, selection(N, K, dtype), KS=ks_in)
    parked, looked, ok = DP.read_parked(out, B, N, K, plan["chunk_units"])
    what = f"B {B} N {N} K {K} ks_in {ks_in} (out chunks {plan['KS']})"
    assert ok and bool(looked.all()), f"fused norm {name} {what}: a chunk that does not own a column is not zero there"
    y = parked.to(dtype)
    assert bool((y.float() == parked).all()), f"fused norm {name} {what}: the parked row is not a 16-bit row"
    judge(el, "fused_norm", name, {"x": DP.x_ratio(xout, pr), "y": DP.y_ratio(y, xout, pr)}, what)
    x2, y2 = ops.add_rmsnorm_ex(part, pr.R, pr.w, pr.eps, KS=ks_in) if ks_in else (pr.R, ops.rmsnorm_ex(pr.R, pr.w, pr.eps))
    assert torch.equal(xout.view(torch.int16), x2.view(torch.int16)), f"fused norm {name} {what}: xout differs from add_rmsnorm's"
    apart = DP.ulps16_apart(y, y2)
    record(el, "fused_norm y vs add", name, apart)
    assert apart <= 1, f"fused norm {name} {what}: {apart} 16-bit ulps from add_rmsnorm's y"


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("K", [64, 1024, 4096])
def test_skinny_fused_norm(el, K, B):
    for ks_in in (0, 1, 7, 8):
        for name in FUSED_PROBES:
            fused_norm_case(el, B, K, K, ks_in, name)


@pytest.mark.parametrize("N", [6144, 28672])
def test_skinny_fused_norm_real_widths(el, N):
    """the qkv and gate|up widths of the 7 B decoder, the selection matrix cut to N columns (every k is read by one or more of them)"""
    for ks_in, name in ((0, "ramp/R"), (8, "chunk-pointer"), (7, "massive")):
        fused_norm_case(el, 1, N, 4096, ks_in, name)


# ---- the fused-SwiGLU GEMV ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("N,K", [(64, 64), (1024, 1024), (4096, 14336)])
def test_skinny_fused_swiglu(el, N, K, B):
    dtype = DTYPES[el]
    cu = ops.skinny_plan(0, N, K, 4, B)["chunk_units"]
    Ws = [selection(N, K, dtype, off) for off in DP.offsets_covering(N, K)]
    for ks_gu in (1, 3, 4, 5):
        for name in DP.SWIGLU_PROBES:
            pr = DP.swiglu_probe(name, B, 2 * K, ks_gu, dtype, DEV)
            part = DP.lay_part(pr.vals)
            parked = torch.full((B, K), float("nan"), dtype=torch.float32, device=DEV)
            for W, off in zip(Ws, DP.offsets_covering(N, K)):
                pk, looked, ok = DP.read_parked(ops.skinny_fused_swiglu(part, W, B, KS=ks_gu), B, N, K, cu, off)
                assert ok, f"fused swiglu {name} B {B} N {N} K {K} ks {ks_gu}: a chunk that does not own a column is not zero there"
                parked[:, looked] = pk[:, looked]
            ref = ops.swiglu_combine(part[:ks_gu], B)
            assert bool((parked == ref.float()).all()), f"fused swiglu {name} B {B} N {N} K {K} ks {ks_gu}: differs from swiglu_combine"
            if name != "gate-range":                                       # (judged in test_swiglu_gate_range; here: the bit equality)
                judge(el, "fused_swiglu", name, {"out": DP.swiglu_ratio(parked.to(dtype), pr)}, f"B {B} N {N} K {K} ks {ks_gu}")


def test_skinny_fused_swiglu_refusals(el):
    dtype = DTYPES[el]
    SK = ops.sk_rows()

    def call(B=2, N=64, K=64, ks=2, ks_arg=None):
        part = torch.zeros((max(ks, 1), SK, 2 * K), dtype=torch.float32, device=DEV)
        return ops.skinny_fused_swiglu(part, torch.zeros((N, K), dtype=dtype, device=DEV), B, KS=ks if ks_arg is None else ks_arg)

    assert float(call()[:, :2].abs().max()) == 0.0                         # (rows past B of the partial rows are never written: whatever the scratch held)
    for kw in (dict(B=5), dict(B=0), dict(K=96), dict(K=32), dict(N=72), dict(N=8), dict(ks_arg=0)):
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_skinny_fused_swiglu"):
            call(**kw)
    lib = _lib.load(el)
    with pytest.raises(_lib.TraceHipError, match="null argument"):
        _lib.check(lib.trace_op_skinny_fused_swiglu(None, 1, None, None, 1, 64, 64, None))


# ---- quant_rows_fp8 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 4096, 14336])
def test_quant_rows_fp8(el, K):
    """code-table: the convert instruction is round-to-nearest-even on every e4m3 value, midpoint and midpoint +- a 16-bit ulp, subnormals included;
    tiny-row: zeros of a row with 0 < amax < 448 / FLT_MAX stay zeros, sy stays amax / 448; zero-row; last-ulp (the clamp's case)"""
    dtype = DTYPES[el]
    for name in DP.QUANT_PROBES:
        x = DP.quant_probe(name, K, dtype, DEV)
        codes, sy = ops.quant_rows_fp8(x)
        judge(el, "quant_rows_fp8", name, DP.judge_quant_probe(name, x, codes, sy), f"K {K}")
