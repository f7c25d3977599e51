"""The GEMM / GEMV family against exact answers (tests/gemm_probes.py; tests/test_gemm_probes_cpu.py shows on the CPU that these probes reject a lost,
doubled or permuted product, a stale K-tile, a 16-bit accumulator, a truncating store, a residual added before the rounding, and every stride and
guard mistake, and which of them the Gaussian checks of test_gpu_kernels.py let through).

Every operand is a small integer times a power of two: the product is exact in fp32 in any order, so `none` and `residual` outputs, fp32 partial rows and
fp32 GEMV outputs are compared BIT FOR BIT with the float64 reference, for every kernel variant, and the variant a case really ran on is asserted through
trace_op_gemm_route (a forced variant that falls back to the 128^2 kernel is counted as the 128^2 kernel).  `quickgelu` / `swiglu` outputs are held to
one output rounding (half an ulp of the float64 value) + 2^-15 |ref| for the fp32 exp2 / rcp chain: gemm_probes.act_bound.  The flat form
(2^-(p+1) + 2^-15) |ref| is the lower end of what one rounding costs — the correctly rounded reference itself exceeds it by up to 1.97 x — so it is
recorded next to the margins (profiles/gemm_probe_margins.txt, column "flat"), not asserted.

References are built on the device in float64, once per (probe, shape, epilogue class), and shared by all kernel variants."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import gemm_probes as P  # noqa: E402
from gemm_probes import EPI_NONE, EPI_RESIDUAL, EPI_QUICKGELU, EPI_SWIGLU  # noqa: E402
from trace_amd import engine as E  # noqa: E402
from trace_amd.engine import ops  # noqa: E402

DEV = torch.device("cuda", 0)
BF, HF = torch.bfloat16, torch.float16
EPIS = (EPI_NONE, EPI_RESIDUAL, EPI_QUICKGELU, EPI_SWIGLU)
GK128, GK256, GKLDR, GKPERS, GKW4 = 0, 1, 2, 3, 4                # trace_op_gemm_route's kernel codes

# name -> (gemm.kernel, gemm.pers.walk, gemm.w4.opt)
KERNELS = {"auto": (0, 0, 0), "tile128": (2, 0, 0), "tile256": (3, 0, 0), "ldr": (4, 0, 0), "pers": (5, 0, 0), "pers-walk1": (5, 1, 0),
           "pers-static": (6, 0, 0), "pers-one": (7, 0, 0), "w4": (8, 0, 0), "w4-walk1": (8, 1, 0), "w4-opt2": (8, 0, 2)}
MARGINS = {}                      # (kernel, epilogue) -> [max err / bound, max err / flat bound, cases]
RAN = {}                          # (kernel name, epilogue or "strided") -> the route codes its cases ran on


def tuned(kernel):
    k, walk, opt = KERNELS[kernel]
    return ops.tuned(gemm__kernel=k, gemm__pers__walk=walk, gemm__w4__opt=opt)


def expected_route(kernel, M, N, K):
    """csrc/gemm.hip gemm_route restated for M < 1024 (auto then takes the 128^2 kernel): the kernel code | walk << 8"""
    k, walk, _ = KERNELS[kernel]
    n256 = N % 256 == 0
    if k == 8 and n256 and K >= 192:
        return GKW4 | (walk << 8)
    if 5 <= k <= 7 and n256 and K >= 128:
        return GKPERS | ((1 if k == 5 and walk == 1 else k - 5) << 8)
    if k == 4 and n256:
        return GKLDR
    return GK256 if k == 3 and n256 else GK128


def own_kernel(kernel):
    """the route code a KERNELS entry is there for (auto: every shape here has M < 1024, which auto sends to the 128^2 kernel)"""
    return {"auto": GK128, "tile128": GK128, "tile256": GK256, "ldr": GKLDR, "w4": GKW4, "w4-walk1": GKW4, "w4-opt2": GKW4}.get(kernel, GKPERS)


def route(M, N, K, lda, ldw, ldc, ldr, epi, fp8=0):
    return E._lib.load(ops.element).trace_op_gemm_route(M, N, K, lda, ldw, ldc, ldr, epi, fp8)


@pytest.fixture(scope="module", autouse=True)
def margins_record():
    """the measured activation-epilogue margins (per kernel and epilogue: the largest error / bound, the same against the flat bound, cases) are printed,
    and appended to the file that the environment variable TRACE_GEMM_PROBE_MARGINS names, if it is set: the record profiles/gemm_probe_margins.txt
    is made from"""
    yield
    lines = [f"{k:<22} {e:<10} max err/bound {m[0]:.3f}  flat {m[1]:.3f}  cases {m[2]}" for (k, e), m in sorted(MARGINS.items())]
    print("\n".join(lines))
    path = os.environ.get("TRACE_GEMM_PROBE_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


_CASES = {}


def case(name, M, N, K, epi, dtype=BF, fp8=False):
    """(probe, reference, float64 pre-rounding value) on the device, built once"""
    scaled = epi in (EPI_QUICKGELU, EPI_SWIGLU)
    key = (name, M, N, K, scaled, dtype, fp8)
    if key not in _CASES:
        _CASES[key] = (P.build(name, M, N, K, dtype, DEV, fp8=fp8, epi=epi), {})
    pr, refs = _CASES[key]
    if epi not in refs:
        sa, sw = fp8_scales(pr)
        refs[epi] = P.probe_reference(pr, epi, sa, sw)
    return pr, refs[epi][0], refs[epi][1]


def fp8_scales(pr):
    return (P.pow2_scales(pr.M, -3, 0, 3, DEV), P.pow2_scales(pr.N, -2, 2, 3, DEV)) if pr.fp8 else (None, None)


def judge(kernel, epi, got, ref, pre, what, dtype=BF):
    if epi in (EPI_NONE, EPI_RESIDUAL):
        if not torch.equal(got.view(torch.int16), ref.view(torch.int16)):
            bad = torch.nonzero(got.view(torch.int16) != ref.view(torch.int16))
            i = tuple(bad[0].tolist())
            pytest.fail(f"{kernel} {P.EPI_NAMES[epi]} {what}: {bad.shape[0]} of {ref.numel()} outputs differ; first {i}: got {float(got[i])} ref {float(ref[i])}; "
                        f"rows {torch.unique(bad[:, 0])[:12].tolist()} cols {torch.unique(bad[:, 1])[:12].tolist()}")
        return
    assert bool(torch.isfinite(got).all()), (kernel, what)
    ratio, flat = P.act_error_ratio(got, pre, dtype), P.act_error_ratio(got, pre, dtype, literal=True)
    m = MARGINS.setdefault((kernel, P.EPI_NAMES[epi]), [0.0, 0.0, 0])
    m[0], m[1], m[2] = max(m[0], ratio), max(m[1], flat), m[2] + 1
    assert ratio <= 1.0, f"{kernel} {P.EPI_NAMES[epi]} {what}: error / bound {ratio:.3f}"


def launch(pr, epi, **kw):
    return ops.gemm(pr.A, pr.W, bias=None if epi == EPI_SWIGLU else pr.bias, R=pr.R if epi == EPI_RESIDUAL else None, epilogue=epi, **kw)


# ---- trace_op_gemm, every kernel --------------------------------------------------------------------------------------------------------
MS, NS, KS = (1, 127, 129, 255, 257, 300), (128, 256, 384, 512), (64, 128, 192, 256, 320, 1024)


@pytest.mark.parametrize("epi", EPIS, ids=[P.EPI_NAMES[e] for e in EPIS])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gemm_every_kernel_every_probe(kernel, epi):
    """M x N x K over row counts around the 128- and 256-row tiles, column counts that are and are not multiples of 256, K from one K-tile through the
    lower bounds of the persistent kernel (128) and of gemm_w4 (192) to an odd number of K-tiles (320) and 1024; all five probes"""
    ran = RAN.setdefault((kernel, epi), set())
    with tuned(kernel):
        for M in MS:
            for N in NS:
                for K in KS:
                    No = N // 2 if epi == EPI_SWIGLU else N
                    r = route(M, N, K, K, K, No, No, epi)
                    assert r == expected_route(kernel, M, N, K), (kernel, M, N, K, hex(r))
                    ran.add(r & 0xFF)
                    for name in P.PROBES:
                        pr, ref, pre = case(name, M, N, K, epi)
                        judge(kernel, epi, launch(pr, epi), ref, pre, f"{name} {M}x{N}x{K}")
    assert own_kernel(kernel) in ran, f"{kernel} never ran its own kernel"


# ---- several tiles per workgroup at a small shape ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [192, 320, 1024])
def test_gemm_persistent_several_tiles_per_workgroup(K):
    """gemm.pers.grid_cap = 3: the 12 tiles of 1300 x 512 go to three workgroups, four each — the ticket walk (kernels 5, 8), the static deal (6), the
    carry from one tile's epilogue into the next tile's prologue and the counters' re-arming (three launches back to back, kernels 8 and 5 alternating
    on one stream) are judged against float64, not against another kernel."""
    M, N = 1300, 512
    with ops.tuned(gemm__pers__grid_cap=3):
        for epi in EPIS:
            No = N // 2 if epi == EPI_SWIGLU else N
            for name in ("hadamard", "pointer-A"):
                pr, ref, pre = case(name, M, N, K, epi)
                for kernel in ("pers", "pers-static", "w4", "pers-walk1", "w4-walk1"):
                    with tuned(kernel):
                        assert route(M, N, K, K, K, No, No, epi) == expected_route(kernel, M, N, K)
                        outs = [launch(pr, epi) for _ in range(3)]
                    for rep, got in enumerate(outs):
                        judge(kernel + " cap3", epi, got, ref, pre, f"{name} K={K} launch {rep}")
                outs = []
                for rep in range(3):
                    for kernel in ("w4", "pers"):
                        with tuned(kernel):
                            outs.append((kernel, launch(pr, epi)))
                for kernel, got in outs:
                    judge(kernel + " cap3 alternating", epi, got, ref, pre, f"{name} K={K}")


# ---- strides, base offsets, poison, guards ----------------------------------------------------------------------------------------------
def run_laid(kernel, pr, epi, cls, in_place=False, dtype=BF):
    L = P.lay_probe(pr, epi, cls, in_place=in_place)
    ref, pre = P.probe_reference(pr, epi)
    lda, ldw, ldr = L.A.stride(0), L.W.stride(0), 0 if L.R is None else L.R.stride(0)
    r = route(pr.M, pr.N, pr.K, lda, ldw, L.ldc, ldr, epi)
    assert r == expected_route(kernel, pr.M, pr.N, pr.K), (kernel, hex(r))
    RAN.setdefault((kernel, "strided"), set()).add(r & 0xFF)
    got = ops.gemm(L.A, L.W, bias=None if epi == EPI_SWIGLU else pr.bias, R=L.R, epilogue=epi, out=L.Cb, ldc=L.ldc, out_offset=L.coff)
    what = f"{pr.name} {cls}{' in place' if in_place else ''} {pr.M}x{pr.N}x{pr.K}"
    judge(kernel + (" f16" if dtype == HF else "") + " strided", epi, got, ref, pre, what, dtype)
    assert P.outside_window_intact(L.Cb, L.coff, L.ldc, pr.M, L.No), f"{kernel} {P.EPI_NAMES[epi]} {what}: bytes outside the M x N window were written"
    for before, after in zip(L.snap, (L.Ab, L.Wb, L.Rb)):
        assert torch.equal(before.view(torch.uint8), after.view(torch.uint8)), f"{kernel} {what}: an input changed"


@pytest.mark.parametrize("cls", ["engine", "api"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gemm_strides_offsets_and_guards(kernel, cls):
    """lda > K, ldw > K, ldc > N, ldr > N (engine: different from ldc), base offsets, +-2^14 in every pad column of A and W, in the rows past M and in
    the guard rows, C pre-filled with a sentinel: the window equals the reference, every other word of C is still the sentinel (a row >= M stored,
    a store that ignores ldc), the inputs are unchanged.  api = leading dimension dim + 8, base offset 8 elements: rows aligned to 16 bytes only, which
    is all that the kernels' 16-byte LDS-DMA pieces, 16-byte residual loads, 8-byte bias loads and 16-byte stores need (read from gemm.hip,
    gemm_ldr.hip, gemm_pers.hip, gemm_w4.hip: every address is base + row * ld + a multiple of 8 elements)."""
    with tuned(kernel):
        for M in (129, 300):
            for epi in EPIS:
                for name in ("ties", "hadamard", "pointer-A"):
                    run_laid(kernel, P.build(name, M, 256, 256, BF, DEV, epi=epi), epi, cls)
            run_laid(kernel, P.build("ties", M, 256, 256, BF, DEV), EPI_RESIDUAL, cls, in_place=True)
    assert own_kernel(kernel) in RAN[(kernel, "strided")], f"{kernel} never ran its own kernel"


def sentinel_like(t):
    return torch.full(t.shape, P.SENTINEL, dtype=torch.int16, device=t.device).view(t.dtype)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gemm_engine_column_slice_form(kernel):
    """the K/V projection of the engine in miniature: C = buf + 256 with ldc = 768 and N = 256, W (and the bias) 256 rows into a 768-row matrix"""
    M, N, K = 300, 256, 256
    with tuned(kernel):
        for name in ("ties", "hadamard"):
            pr = P.build(name, M, N, K, BF, DEV)
            ref, _ = P.probe_reference(pr, EPI_NONE)
            Wbig = (P.poison_fill(DEV)(3 * N * K)).to(BF).view(3 * N, K)
            Wbig[N:2 * N] = pr.W
            bbig = torch.full((3 * N,), P.POISON, dtype=BF, device=DEV)
            bbig[N:2 * N] = pr.bias
            snap = Wbig.clone()
            buf = sentinel_like(torch.empty((M + 8) * 3 * N, dtype=BF, device=DEV))
            assert route(M, N, K, K, K, 3 * N, 0, EPI_NONE) == expected_route(kernel, M, N, K)
            got = ops.gemm(pr.A, Wbig[N:2 * N], bias=bbig[N:2 * N], out=buf, ldc=3 * N, out_offset=N)
            judge(kernel + " column slice", EPI_NONE, got, ref, None, name)
            assert P.outside_window_intact(buf, N, 3 * N, M, N) and torch.equal(snap, Wbig)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gemm_engine_last_rows_form(kernel):
    """the last layer's "last rows only" products in miniature: M = 3 rows taken every 5 K elements of A, stored every 5 N elements with the residual in
    place (ldr = ldc = 5 N); the rows between them are full of sentinel (C / R) and poison (A) and stay so"""
    M, N, K = 3, 256, 256
    with tuned(kernel):
        for name in ("ties", "hadamard"):
            pr = P.build(name, M, N, K, BF, DEV)
            ref, _ = P.probe_reference(pr, EPI_RESIDUAL)
            Abig = P.poison_fill(DEV)(5 * M * K).to(BF).view(5 * M, K)
            Abig[::5] = pr.A
            snap = Abig.clone()
            buf = sentinel_like(torch.empty(5 * M * N, dtype=BF, device=DEV))
            win = buf.as_strided((M, N), (5 * N, 1), 0)
            win.copy_(pr.R)
            assert route(M, N, K, 5 * K, K, 5 * N, 5 * N, EPI_RESIDUAL) == expected_route(kernel, M, N, K)
            got = ops.gemm(Abig.as_strided((M, K), (5 * K, 1), 0), pr.W, bias=pr.bias, R=win, epilogue=EPI_RESIDUAL, out=win)
            judge(kernel + " last rows", EPI_RESIDUAL, got, ref, None, name)
            assert P.outside_window_intact(buf, 0, 5 * N, M, N) and torch.equal(snap, Abig)


# ---- the split-K partial-row GEMM and the tiled SwiGLU GEMM of the wide decode step ------------------------------------------------------
def chunk_sums(pr, ks):
    """float64 sums of the ks contiguous k-chunks: [ks, M, N]"""
    A, W = pr.A.double().view(pr.M, ks, -1), pr.W.double().view(pr.N, ks, -1)
    return torch.einsum("mck,nck->cmn", A, W)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("K", [256, 1024, 4096])
def test_gemm_partial_rows_exact(cfg, K):
    """trace_op_gemm_partial, row-major and tiled 1 / 5 weights, every decode.partial_cfg: each k-chunk's partial rows of the rows < M are the chunk's
    exact integer sums, bit for bit (row-major and tiled weights cut K into the same contiguous chunks); rows >= M stay zero"""
    with ops.tuned(decode__partial_cfg=cfg):
        for M in (65, 128, 129, 200):
            for N in (256, 512):
                for name in ("pointer-A", "hadamard", "count"):
                    pr, _, _ = case(name, M, N, K, EPI_NONE)
                    Wt = ops.tile_pack(pr.W)
                    for tiled, W in ((0, pr.W), (1, Wt), (5, Wt)):
                        part = ops.gemm_partial(pr.A, W, tiled=tiled)
                        ref = chunk_sums(pr, part.shape[0]).float()
                        assert torch.equal(part[:, :M], ref), (cfg, name, M, N, K, tiled, int((part[:, :M] != ref).sum()))
                        assert part.shape[1] == ops.sk_rows() and not bool(part[:, M:].any()), (cfg, name, M, N, K, tiled, "rows >= M written")


@pytest.mark.parametrize("K", [256, 1024, 4096])
def test_gemm_swiglu_tiled_probes(K):
    for M in (65, 128, 129, 200):
        for N in (256, 512):
            for name in ("pointer-A", "hadamard", "count"):
                pr, ref, pre = case(name, M, N, K, EPI_SWIGLU)
                Wt = ops.tile_pack(pr.W)
                for ring in (True, False):
                    judge(f"swiglu_tiled ring={int(ring)}", EPI_SWIGLU, ops.gemm_swiglu_tiled(pr.A, Wt, ring=ring), ref, pre, f"{name} {M}x{N}x{K}")


# ---- the decode GEMVs ---------------------------------------------------------------------------------------------------------------------
BS = (1, 3, 4, 5, 16, 17, 33, 64)


@pytest.mark.parametrize("K", [128, 1024, 4096])
@pytest.mark.parametrize("N", [128, 512])
def test_skinny_gemm_probes(N, K):
    """trace_op_skinny_gemm, row-major and tiled weights: 16-bit outputs (none, residual) bit equal to the reference, the fp32 partial rows sum to the
    float64 product exactly, add_rmsnorm's new residual rows equal round16(round16(sum) + R), SwiGLU (fused and partial rows + swiglu_combine) within
    one output rounding"""
    for B in BS:
        for name in ("pointer-W", "hadamard", "count"):
            pr, _, _ = case(name, B, N, K, EPI_NONE)
            ref, lin = P.reference(pr.A, pr.W, None, None, EPI_NONE, BF)             # (the GEMVs take no bias)
            ref_r, _ = P.reference(pr.A, pr.W, None, pr.R, EPI_RESIDUAL, BF)
            Wt = ops.tile_pack(pr.W)
            what = f"{name} B={B} N={N} K={K}"
            for tiled, W in ((False, pr.W), (True, Wt)):
                judge(f"skinny tiled={int(tiled)}", EPI_NONE, ops.skinny_gemm(pr.A, W, tiled=tiled), ref, None, what)
                judge(f"skinny tiled={int(tiled)}", EPI_RESIDUAL, ops.skinny_gemm(pr.A, W, R=pr.R, epilogue=EPI_RESIDUAL, tiled=tiled), ref_r, None, what)
                part = ops.skinny_gemm(pr.A, W, epilogue=E.EPI_PARTIAL, tiled=tiled)
                assert torch.equal(part.double().sum(0)[:B], lin), (what, tiled, "partial rows")     # (rows >= B: the hook copies its whole scratch, stale rows included)
            w = torch.ones(N, dtype=BF, device=DEV)
            x, _ = ops.add_rmsnorm(part, pr.R, w, 1e-5)
            judge("add_rmsnorm xout", EPI_RESIDUAL, x, ref_r, None, what)
            ps, ref_s, pre_s = case(name, B, N, K, EPI_SWIGLU)
            Wts = ops.tile_pack(ps.W)
            for tiled, W in ((False, ps.W), (True, Wts)):
                judge(f"skinny tiled={int(tiled)}", EPI_SWIGLU, ops.skinny_gemm(ps.A, W, epilogue=EPI_SWIGLU, tiled=tiled), ref_s, pre_s, what)
            pg = ops.skinny_gemm(ps.A, Wts, epilogue=E.EPI_PARTIAL, tiled=True)
            judge("swiglu_combine", EPI_SWIGLU, ops.swiglu_combine(pg, B), ref_s, pre_s, what)


@pytest.mark.parametrize("K", [128, 1024, 4096])
@pytest.mark.parametrize("N", [128, 512])
def test_skinny_fp8_and_w8_probes(N, K):
    """trace_op_skinny_fp8 (e4m3 activations and weights) and trace_op_skinny_w8 (e4m3 weights widened, 16-bit activations): fp32 outputs bit equal to
    the float64 product times the power-of-two scales"""
    for B in BS:
        for name in ("pointer-W", "hadamard", "count"):
            pr, _, _ = case(name, B, N, K, EPI_NONE, fp8=True)
            sx, sw = fp8_scales(pr)
            ref = P.linear64(pr.A, pr.W, True, sx, sw).float()
            got = ops.skinny_fp8(pr.A, sx, pr.W, sw)
            assert torch.equal(got, ref), ("skinny_fp8", name, B, N, K, int((got != ref).sum()))
            X = P.widen(pr.A, True).to(BF)                                          # the same integers as 16-bit activations
            ref = (P.widen(pr.A, True) @ P.widen(pr.W, True).t() * sw.double()[None, :]).float()
            got = ops.skinny_w8(X, pr.W, sw)
            assert torch.equal(got, ref), ("skinny_w8", name, B, N, K, int((got != ref).sum()))


# ---- the fp8 GEMM ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["tile128", "tile256"])
@pytest.mark.parametrize("K", [128, 256, 1024])
def test_gemm_fp8_probes(kernel, K):
    """trace_op_gemm_fp8 on e4m3 bytes and power-of-two scales built directly (no quantiser): C = (A8 . W8^T) sa[m] sw[n] is exact.  The path has no
    bias, so the ties probe (an integer bias) does not exist for it; its residual order is pinned by the small-integer residual of the other probes
    on sums that the scales move off the 16-bit grid."""
    with tuned(kernel):
        for M in (129, 300):
            for N in (256, 512):
                for epi in (EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU):
                    No = N // 2 if epi == EPI_SWIGLU else N
                    assert route(M, N, K, K, K, No, No, epi, 1) == (GK256 if kernel == "tile256" else GK128)
                    for name in ("pointer-A", "pointer-W", "hadamard", "count"):
                        pr, ref, pre = case(name, M, N, K, epi, fp8=True)
                        sa, sw = fp8_scales(pr)
                        got = ops.gemm_fp8(pr.A, sa, pr.W, sw, R=pr.R if epi == EPI_RESIDUAL else None, epilogue=epi)
                        judge("fp8 " + kernel, epi, got, ref, pre, f"{name} {M}x{N}x{K}")


# ---- the fp16 library -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def f16_ops():
    ops.use("f16")
    yield ops
    ops.use("bf16")


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_gemm_f16_library(f16_ops, kernel):
    """the same kernels compiled for IEEE half (p = 11): ties (bias in [2048, 4096)), count (63 K / 64 = 4032 at K = 4096 needs 6 bits, its partial sums
    up to 12) and the strided / guarded form"""
    with tuned(kernel):
        for epi in (EPI_NONE, EPI_RESIDUAL):
            pr, ref, pre = case("ties", 300, 256, 256, epi, HF)
            judge(kernel + " f16", epi, launch(pr, epi), ref, pre, "ties 300x256x256", HF)
            pr, ref, pre = case("count", 129, 256, 4096, epi, HF)
            judge(kernel + " f16", epi, launch(pr, epi), ref, pre, "count 129x256x4096", HF)
        for epi in EPIS:
            for cls in ("engine", "api"):
                run_laid(kernel, P.build("ties", 300, 256, 256, HF, DEV, epi=epi), epi, cls, dtype=HF)
