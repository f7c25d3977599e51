"""The evidence that the GEMM probes (tests/gemm_probes.py) are tight, on the CPU: a torch emulation of a tiled, K-looped GEMM over flat buffers
with leading dimensions (fp32 accumulators, the epilogues as csrc/gemm.hip documents them) and a `fault=` switch.

  * fault-free, the emulation equals gemm_probes.reference bit for bit on every probe (bf16, fp16 and the fp8 form), packed and strided;
  * the probes have the properties they state (exact partial sums, at most p significant bits, at least 85 % of the outputs +-1-visible);
  * every fault of FAULTS is rejected by at least one probe, at a small shape and at a real width (K = 4096);
  * the present Gaussian checks (tests/test_gpu_kernels.py: same rnd(), same tolerances; tests/test_gpu_fp8.py for the fp8 scales) are run against
    every fault: which ones they accept is printed (DESIGN.md section 2 holds the table) and the always-accepted ones are asserted."""
import pytest
import torch

import gemm_probes as P
from gemm_probes import EPI_NONE, EPI_RESIDUAL, EPI_QUICKGELU, EPI_SWIGLU

BF, HF = torch.bfloat16, torch.float16

# fault -> (epilogue it needs, stride class it needs (None: packed operands), fp8 form)
FAULTS = {
    "lost product: last k of the last K-tile, one column tile": (EPI_NONE, None, False),
    "lost product: first k of a middle K-tile, one column tile": (EPI_NONE, None, False),
    "one product counted twice": (EPI_NONE, None, False),
    "a K-tile skipped for one (row tile, column tile)": (EPI_NONE, None, False),
    "K-tile t read as t - 1 (ring slot reused early)": (EPI_NONE, None, False),
    "two k-slots swapped in W only (tile_pack mismatch)": (EPI_NONE, None, False),
    "accumulator rounded to 16 bits between K-tiles": (EPI_NONE, None, False),
    "truncating store": (EPI_NONE, None, False),
    "residual added before the rounding": (EPI_RESIDUAL, None, False),
    "bias taken four columns off": (EPI_NONE, None, False),
    "gate and up swapped": (EPI_SWIGLU, None, False),
    "interleave group of 8 instead of 16": (EPI_SWIGLU, None, False),
    "a row >= M stored": (EPI_NONE, "api", False),
    "ldc ignored (packed store)": (EPI_NONE, "engine", False),
    "lda ignored": (EPI_NONE, "engine", False),
    "ldr taken as ldc": (EPI_RESIDUAL, "engine", False),
    "K loop runs into the pad columns": (EPI_NONE, "engine", False),
    "fp8 row scale taken from row m + 1": (EPI_NONE, None, True),
    "fp8 column scale shifted by four": (EPI_NONE, None, True),
}
FAULT_KEYS = list(FAULTS)
LOST_LAST, LOST_MID, DOUBLED, SKIP, STALE, SWAPK, ACC16, TRUNC, RES_FIRST, BIAS4, GU_SWAP, IL8, ROW_M, LDC, LDA, LDR, KPAD, SA1, SW4 = FAULT_KEYS


def emulate(A, lda, W, ldw, C, ldc, bias, R, ldr, M, N, K, epi, dtype, fault=None, BM=128, BN=128, fp8=False, sa=None, sw=None):
    """A, W, C, R: (flat buffer, offset of element [0, 0]).  K-tiles of 64, all row and column tiles of a K-tile at once (the order of exact sums is
    free); rows of the last row tile beyond M read row M - 1 (the kernels' clamp) and are not stored.  Stores into C's buffer."""
    Ab, aoff = A
    Wb, woff = W
    Cb, coff = C
    Mp = -(-M // BM) * BM
    rows = torch.arange(Mp).clamp(max=M - 1)
    ftn, ftm = N // BN - 1, Mp // BM - 1                          # the column / row tile a one-tile fault sits in
    fc, fr = slice(ftn * BN, (ftn + 1) * BN), slice(ftm * BM, (ftm + 1) * BM)
    nk = K // 64
    mid = nk // 2
    lda_e = K if fault == LDA else lda

    def tile(buf, off, ld, idx, kt):
        flat = off + idx[:, None] * ld + kt * 64 + torch.arange(64)[None, :]
        t = buf[flat]
        return (t.view(P.FP8) if fp8 else t).float()

    acc = torch.zeros((Mp, N), dtype=torch.float32)
    for kt in range(nk + (1 if fault == KPAD else 0)):
        src = kt - 1 if fault == STALE and kt == max(mid, 1) else kt
        At, Wt = tile(Ab, aoff, lda_e, rows, src), tile(Wb, woff, ldw, torch.arange(N), src)
        if fault == SWAPK:
            Wt = Wt.clone()
            Wt[:, [3, 40]] = Wt[:, [40, 3]]
        part = At @ Wt.t()
        if fault == LOST_LAST and kt == nk - 1:
            part[:, fc] -= At[:, 63:64] * Wt[fc, 63][None, :]
        if fault == LOST_MID and kt == mid:
            part[:, fc] -= At[:, 0:1] * Wt[fc, 0][None, :]
        if fault == DOUBLED and kt == mid:
            part[:, fc] += At[:, 17:18] * Wt[fc, 17][None, :]
        if fault == SKIP and kt == mid:
            part[fr, fc] = 0
        acc += part
        if fault == ACC16:
            acc = acc.to(dtype).float()
    n = torch.arange(N)
    x = acc
    if fp8:
        s_row = sa[(rows + 1).clamp(max=M - 1)] if fault == SA1 else sa[rows]
        s_col = sw[(n + 4) % N] if fault == SW4 else sw
        x = x * (s_row[:, None] * s_col[None, :])
    elif bias is not None and epi != EPI_SWIGLU:
        x = x + bias.float()[(n + 4) % N if fault == BIAS4 else n][None, :]
    if epi == EPI_QUICKGELU:
        x = x * (1.0 / (1.0 + torch.exp2(-2.4554669595930157 * x)))
    if epi == EPI_SWIGLU:
        grp = 8 if fault == IL8 else 16
        v = x.reshape(Mp, -1, 2, grp)
        g, u = v[:, :, 0].reshape(Mp, -1), v[:, :, 1].reshape(Mp, -1)
        if fault == GU_SWAP:
            g, u = u, g
        x = g * (1.0 / (1.0 + torch.exp2(-1.4426950408889634 * g))) * u
    No = x.shape[1]
    if epi == EPI_RESIDUAL:
        Rb, roff = R
        r = Rb[(roff + rows[:, None] * (ldc if fault == LDR else ldr) + n[None, :]).clamp(max=Rb.numel() - 1)].float()      # (clamp: the faulty stride leaves the buffer)
        x = (x + r) if fault == RES_FIRST else x.to(dtype).float() + r
    out = P.truncate16(x.double(), dtype) if fault == TRUNC else x.to(dtype)
    stored = Mp if fault == ROW_M else M
    m_idx = torch.arange(stored)
    Cb[coff + m_idx[:, None] * (No if fault == LDC else ldc) + torch.arange(No)[None, :]] = out[:stored]


def scales(pr):
    return (P.pow2_scales(pr.M, -3, 0, 3), P.pow2_scales(pr.N, -2, 2, 3)) if pr.fp8 else (None, None)


def run_probe(pr, epi, cls, fault=None, in_place=False):
    """the emulation on one probe, packed (cls None) or strided; returns the list of what a GPU test would flag (empty = accepted)"""
    sa, sw = scales(pr)
    ref, pre = P.probe_reference(pr, epi, sa, sw)
    if cls is None:
        No = ref.shape[1]
        pad = lambda t: torch.cat([t.reshape(-1), t.reshape(-1)[:256]])            # (the K-into-pad fault reads past a packed operand's end)
        Cb = torch.full(((pr.M + 256) * No,), P.SENTINEL, dtype=torch.int16).view(pr.dtype)
        R = (pr.R.reshape(-1), 0) if epi == EPI_RESIDUAL else None
        emulate((pad(pr.A), 0), pr.K, (pad(pr.W), 0), pr.K, (Cb, 0), No, pr.bias, R, pr.N, pr.M, pr.N, pr.K, epi, pr.dtype, fault, fp8=pr.fp8, sa=sa, sw=sw)
        got, intact, inputs_ok = Cb[: pr.M * No].view(pr.M, No), bool((Cb.view(torch.int16)[pr.M * No:] == P.SENTINEL).all()), True
    else:
        L = P.lay_probe(pr, epi, cls, tile_rows=128, in_place=in_place)
        R = None if L.Rb is None else (L.Rb, L.R.storage_offset())
        emulate((L.Ab, L.A.storage_offset()), L.A.stride(0), (L.Wb, L.W.storage_offset()), L.W.stride(0), (L.Cb, L.coff), L.ldc, pr.bias, R,
                0 if L.R is None else L.R.stride(0), pr.M, pr.N, pr.K, epi, pr.dtype, fault, fp8=pr.fp8, sa=sa, sw=sw)
        got, intact = L.C, P.outside_window_intact(L.Cb, L.coff, L.ldc, pr.M, L.No)
        inputs_ok = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(L.snap, (L.Ab, L.Wb, L.Rb)))
    flagged = []
    if epi in (EPI_NONE, EPI_RESIDUAL):
        if not torch.equal(got.view(torch.int16), ref.view(torch.int16)):
            flagged.append(f"{int((got.view(torch.int16) != ref.view(torch.int16)).sum())} of {ref.numel()} outputs differ")
    elif P.act_error_ratio(got, pre, pr.dtype) > 1.0:
        flagged.append(f"activation error / bound {P.act_error_ratio(got, pre, pr.dtype):.3g}")
    if not intact:
        flagged.append("bytes outside the window written")
    if not inputs_ok:
        flagged.append("inputs changed")
    return flagged


# ---- the probes' stated properties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
def test_tables_have_distinct_rows_and_columns(dtype):
    for amp, N, K in ((128, 512, 4096), (128, 1300, 1024), (128, 64, 4096), (15, 512, 1024), (15, 64, 4096), (128, 4, 64)):
        T = P.table(N, K, amp)
        assert float(T.abs().max()) <= amp and bool((T == T.round()).all())
        assert torch.unique(T, dim=0).shape[0] == N and torch.unique(T, dim=1).shape[1] == K
        assert 0.4 < float((T % 2).mean()) < 0.6                                   # odd about half of the time (the ties probe)
        assert bool((T.to(dtype).double() == T).all())


@pytest.mark.parametrize("M,K", [(1, 64), (127, 256), (129, 128), (300, 192), (300, 1024), (1300, 320), (64, 4096), (3, 128)])
def test_pointer_hot_columns_cover_every_k(M, K):
    ks = P.k_of(M, K)
    hot = ks[ks >= 0]
    assert set(hot.tolist()) == set(range(K))
    if M <= K:
        assert hot.numel() == K                                                     # each k exactly once
    pr = P.pointer_a(M, 128, K, BF)
    lin = P.linear64(pr.A, pr.W)
    m = min(M - 1, 5)
    assert torch.equal(lin[m], pr.T[:, ks[m][ks[m] >= 0]].sum(1))                   # C[m, n] = sum of T[n][k] over the hot k of row m
    if M >= K:
        assert torch.equal(lin, pr.T[:, ks[:, 0]].t())                              # one-hot rows: C[m, n] = T[n][k(m)]
    pw = P.pointer_w(16, 128, K, BF)
    kw = P.k_of(128, K)
    assert torch.equal(P.linear64(pw.A, pw.W)[:, 7], pw.T[:, kw[7][kw[7] >= 0]].sum(1))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
@pytest.mark.parametrize("K", [64, 192, 256, 320, 1024, 4096, 14336])
def test_hadamard_properties(dtype, K):
    M, N = 300, 256
    pr = P.hadamard(M, N, K, dtype)
    A, W = pr.A.double(), pr.W.double()
    assert bool((A.abs() == 1).all()) and bool((W.abs() == 1).all())                # all K products are non-zero
    tiles = torch.einsum("mtk,ntk->tmn", A.view(M, -1, 64), W.view(N, -1, 64))
    assert bool(((tiles == 0) | (tiles.abs() == 64)).all())                         # every tile contributes 0 or +-64
    partial = tiles.cumsum(0)
    assert float(partial.abs().max()) < 2 ** 24                                     # partial sums (any order: multiples of 64 below 2^24) exact in fp32
    lin = P.linear64(pr.A, pr.W)
    assert torch.equal(lin, partial[-1])
    assert int(P.significant_bits(lin).max()) <= P.P_BITS[dtype]                    # the sum itself needs no rounding
    assert P.pm1_visible(lin, dtype) >= 0.85
    assert float((lin == 0).double().mean()) > 0.5                                  # most outputs are exactly 0
    if K in (256, 1024) and dtype == BF:                                            # one lost product changes every stored output
        lost = lin - A[:, K - 1:K] * W[:, K - 1][None, :]
        assert bool((P.round16(lost, dtype) != P.round16(lin, dtype)).all())


@pytest.mark.parametrize("K", [64, 384, 1024, 4096])
def test_count_with_holes_properties(K):
    pr = P.count_holes(130, 256, K, BF)
    lin = P.linear64(pr.A, pr.W)
    assert bool((lin == 63 * K // 64).all())
    assert bool((pr.W.view(256, -1, 64).double().sum(2) == 63).all())               # one zero per 64-k tile
    holes = (pr.W.view(256, -1, 64) == 0).double().argmax(2)
    assert torch.unique(holes[:, 0]).numel() == 64 and (K == 64 or torch.unique(holes[0]).numel() > 1)    # its place depends on n and on the tile
    if K >= 384:                                                                    # a 16-bit accumulator goes wrong (315 = 63 * 5 needs 9 bits: one more tile shows it)
        a16 = torch.zeros(())
        for t in range(K // 64):
            a16 = (a16 + 63).to(BF).float()
        assert float(a16) != float(P.round16(lin[0, 0], BF))


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
def test_ties_probe_lands_on_ties(dtype):
    """300 x 256 x 192, the shape the issue measured (bf16: a truncating store differs on 18 % of the elements, a residual added before the rounding on 21 %)"""
    pr = P.ties(300, 256, 192, dtype)
    p = P.P_BITS[dtype]
    b = pr.bias.double()
    assert bool((b % 2 == 0).all()) and float(b.min()) >= 2 ** p and float(b.max()) < 2 ** (p + 1)
    lin = P.linear64(pr.A, pr.W) + b[None, :]
    ref = P.round16(lin, dtype)
    tie = (ref.double() - lin).abs() == 1                                           # spacing 2 there: an odd sum is half way
    assert float(tie.double().mean()) > 0.15
    trunc = float((P.truncate16(lin, dtype) != ref).double().mean())
    res_first = float((P.round16(lin + pr.R.double(), dtype) != P.round16(ref.double() + pr.R.double(), dtype)).double().mean())
    print(f"ties {dtype}: ties {float(tie.double().mean()):.3f}, truncating store differs on {trunc:.3f}, residual before rounding on {res_first:.3f}")
    assert trunc > 0.10 and res_first > 0.10


def test_round16_is_round_to_nearest_even_and_truncate16_is_not():
    x = torch.tensor([257.0, 259.0, 258.0, -257.0, -259.0, 255.0, 1036.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)
    assert P.round16(x, BF).double().tolist() == [256.0, 260.0, 258.0, -256.0, -260.0, 255.0, 1040.0, 1.0, 1.0 + 2.0 ** -6]
    assert P.truncate16(x, BF).double().tolist() == [256.0, 258.0, 258.0, -256.0, -258.0, 255.0, 1032.0, 1.0, 1.0 + 2.0 ** -7]
    y = torch.tensor([2049.0, 2051.0, -2049.0, -2051.0, 2050.0], dtype=torch.float64)
    assert P.round16(y, HF).double().tolist() == [2048.0, 2052.0, -2048.0, -2052.0, 2050.0]
    assert P.truncate16(y, HF).double().tolist() == [2048.0, 2050.0, -2048.0, -2050.0, 2050.0]
    with pytest.raises(AssertionError):
        P.round16(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), BF)


@pytest.mark.parametrize("dtype", [BF, HF], ids=["bf16", "f16"])
def test_activation_bound_is_one_output_rounding(dtype):
    """half an ulp + slack: the correctly rounded float64 value always meets it, a value two steps away never does (one step away can, next to a tie); the flat 2^-(p+1) |ref| form would
    reject the correctly rounded value wherever ref sits in the lower half of a binade"""
    g = torch.Generator().manual_seed(5)
    pre = (torch.rand(20000, generator=g, dtype=torch.float64) - 0.5) * 40
    pre[:4] = torch.tensor([1.0 + 2.0 ** -(P.P_BITS[dtype]), -2.0 - 2.0 ** -(P.P_BITS[dtype] - 1), 2.0 ** -130, 0.0], dtype=torch.float64)
    ref = P.round16(pre, dtype, exact=False)
    assert P.act_error_ratio(ref, pre, dtype) <= 1.0
    up = (ref.view(torch.int16) + 2).view(dtype)
    off = (up.double() - pre).abs() / P.act_bound(pre, dtype)
    assert float(off[4:].min()) > 1.0
    assert 1.5 < P.act_error_ratio(ref, pre, dtype, literal=True) < 2.0


# ---- the emulation equals the reference, fault-free ----------------------------------------------------------------------------------------
SMALL = (450, 256, 448)            # M >= K: one-hot pointer rows; K = 448: seven K-tiles (an odd count); from the sixth on a 16-bit accumulator is off (63 * 5 = 315 needs 9 bits)
WIDE = (300, 256, 4096)


@pytest.mark.parametrize("form", ["bf16", "f16", "fp8"])
@pytest.mark.parametrize("M,N,K", [SMALL, (129, 384, 256), (1, 128, 64), WIDE])
def test_emulation_equals_reference_fault_free(form, M, N, K):
    dtype, fp8 = (HF if form == "f16" else BF), form == "fp8"
    if fp8 and K % 128:
        K += 64
    for name in P.PROBES:
        if fp8 and name == "ties":
            continue
        for epi in (EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU) + (() if fp8 else (EPI_QUICKGELU,)):
            pr = P.build(name, M, N, K, dtype, fp8=fp8, epi=epi)
            for cls in (None,) if fp8 or (M, N, K) == WIDE else (None, "engine", "api"):
                assert run_probe(pr, epi, cls) == [], (form, name, P.EPI_NAMES[epi], cls)
    if not fp8:
        pr = P.build("ties", M, N, K, dtype)
        assert run_probe(pr, EPI_RESIDUAL, "engine", in_place=True) == []


# ---- every fault is rejected by some probe -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, WIDE], ids=["small", "K4096"])
@pytest.mark.parametrize("fault", FAULT_KEYS)
def test_every_fault_is_rejected_by_a_probe(fault, shape):
    epi, cls, fp8 = FAULTS[fault]
    M, N, K = shape
    if fp8 and K % 128:
        K += 64
    rejecting = []
    for name in P.PROBES:
        if fp8 and name == "ties":
            continue
        pr = P.build(name, M, N, K, BF, fp8=fp8, epi=epi)
        if run_probe(pr, epi, cls, fault):
            rejecting.append(name)
    print(f"{fault} @ {M}x{N}x{K}: rejected by {rejecting}")
    assert rejecting, f"no probe notices: {fault}"


def test_the_faults_each_probe_family_is_there_for():
    """the pairs the probes were designed around (a probe that stops noticing its own fault has lost its point)"""
    M, N, K = SMALL
    for fault, name in ((ACC16, "count"), (TRUNC, "ties"), (RES_FIRST, "ties"), (LOST_LAST, "hadamard"), (LOST_MID, "pointer-A"), (STALE, "hadamard"),
                        (SWAPK, "pointer-A"), (SWAPK, "pointer-W"), (DOUBLED, "count"), (BIAS4, "ties")):
        epi, cls, fp8 = FAULTS[fault]
        assert run_probe(P.build(name, M, N, K, BF, epi=epi), epi, cls, fault), (fault, name)
    assert run_probe(P.build("count", M, N, 4096, HF), EPI_NONE, None, ACC16)       # fp16 holds 11 bits: 63 * 33 = 2079 is the first sum that does not fit
    for fault in (ROW_M, LDC, LDA, LDR, KPAD):                                      # the stride / guard faults, in both classes where the class can tell
        epi, _, _ = FAULTS[fault]
        for cls in ("engine", "api"):
            flagged = run_probe(P.build("pointer-A", M, N, K, BF), epi, cls, fault)
            if fault == LDR and cls == "api":
                assert flagged == []            # api: ldr == ldc (both N + 8) — why the engine class gives the residual a leading dimension of its own
            elif fault == KPAD and cls == "api":
                assert flagged                  # (8 pad columns: the extra K-tile reads them and the next row)
            else:
                assert flagged, (fault, cls)
    assert run_probe(P.build("ties", M, N, K, BF), EPI_RESIDUAL, "engine", LDR, in_place=False)


# ---- what the present Gaussian checks accept -----------------------------------------------------------------------------------------------
def rnd(*shape, scale=1.0, seed=0):
    """tests/test_gpu_kernels.py rnd(), on the CPU"""
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def gaussian_flagged(M, N, K, fault, epi=EPI_NONE, fp8=False):
    """elements the check of test_gemm_plain_bias / test_gemm_epilogues (or, for the fp8 form, of test_gemm_fp8_vs_exact_restatement) flags when
    the GEMM has this fault; the epilogue is the one the fault lives in (fault None: the epilogue / form asked for)"""
    if fault is not None:
        epi, _, fp8 = FAULTS[fault]
    spare = 256
    if fp8:
        torch.manual_seed(M + N)
        a, w = torch.randn(M, K).to(BF), (torch.randn(N, K) * 0.02).to(BF)

        def quant(x):
            amax = x.float().abs().amax(dim=1)
            return (x.float() * (448.0 / amax)[:, None]).clamp(-448.0, 448.0).to(P.FP8).view(torch.uint8), amax / 448.0
        (a8, sa), (w8, sw) = quant(a), quant(w)
        Cb = torch.zeros((M + spare) * N, dtype=BF)
        emulate((a8.reshape(-1), 0), K, (w8.reshape(-1), 0), K, (Cb, 0), N, None, None, 0, M, N, K, epi, BF, fault, fp8=True, sa=sa, sw=sw)
        ref = (a8.view(P.FP8).float() @ w8.view(P.FP8).float().t()) * sa[:, None] * sw[None, :]
        err = (Cb[: M * N].view(M, N).float() - ref).abs()
        return int((err >= 2e-2 * float(ref.abs().max()) + 1e-3).sum())
    A, W, b, R = rnd(M, K), rnd(N, K, scale=0.05), rnd(N, scale=0.5), rnd(M, N)
    pad = lambda t: torch.cat([t.reshape(-1), t.reshape(-1)[:256]])
    if epi == EPI_SWIGLU:
        Wg, Wu = rnd(N // 2, K, scale=0.05, seed=1), rnd(N // 2, K, scale=0.05, seed=2)
        W = torch.stack([Wg.view(-1, 16, K), Wu.view(-1, 16, K)], dim=1).reshape(N, K).contiguous()
        ref, atol = torch.nn.functional.silu(A.float() @ Wg.float().t()) * (A.float() @ Wu.float().t()), 2e-2
    else:
        lin = A.float() @ W.float().t() + b.float()
        ref, atol = (lin.to(BF).float() + R.float(), 3e-2) if epi == EPI_RESIDUAL else (lin * torch.sigmoid(1.702 * lin) if epi == EPI_QUICKGELU else lin, 2e-2)
    No = ref.shape[1]
    Cb = torch.zeros((M + spare) * No, dtype=BF)
    emulate((pad(A), 0), K, (pad(W), 0), K, (Cb, 0), No, b, (R.reshape(-1), 0), N, M, N, K, epi, BF, fault)
    got = Cb[: M * No].view(M, No).float()
    return int((((got - ref).abs() > atol + 1e-2 * ref.abs()) | ~torch.isfinite(got)).sum())


GAUSSIAN_SHAPES = [(64, 128, 4096), (577, 384, 1024), (300, 256, 256)]              # shapes of the present tests


def test_what_the_gaussian_checks_accept():
    """The table of DESIGN.md section 2: flagged elements per fault and shape (0 = the fault goes through).  Fault-free the checks pass; a truncating
    store and a residual added before the rounding are never seen; the stride and guard faults are invisible to packed operands by construction."""
    for M, N, K in GAUSSIAN_SHAPES:
        for epi in (EPI_NONE, EPI_RESIDUAL, EPI_QUICKGELU, EPI_SWIGLU):
            assert gaussian_flagged(M, N, K, None, epi) == 0, (M, N, K, epi)
        assert gaussian_flagged(M, N, K, None, EPI_NONE, fp8=True) == 0
    lines = []
    for fault in FAULT_KEYS:
        counts = [gaussian_flagged(M, N, K, fault) for M, N, K in GAUSSIAN_SHAPES]
        lines.append(f"{fault:<62} " + " ".join(f"{c:>13}" for c in counts))
        if fault in (TRUNC, RES_FIRST, ROW_M, LDC, LDA, LDR):
            assert counts == [0, 0, 0], (fault, counts)
    print("\n" + f"{'fault':<62} " + " ".join(f"{'x'.join(map(str, s)):>13}" for s in GAUSSIAN_SHAPES) + "\n" + "\n".join(lines))


# ---- the shape check, through trace_op_gemm_route (host code: no GPU) ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from trace_amd import build, _lib
    build.build()
    lib = _lib.load()
    lib.trace_op_tuning_reset()
    yield lib
    lib.trace_op_tuning_reset()


def test_shape_check_admits_rows_aligned_to_16_bytes_and_nothing_weaker(lib):
    """The `api` stride class (leading dimension = dim + 8 elements) is the weakest gemm_shape_ok admits, for every kernel: their LDS-DMA pieces,
    residual loads and stores are 16 bytes at base + row * ld + a multiple of 8 elements.  A leading dimension that is not a multiple of 8 is rejected
    before any launch (fp8: 16)."""
    from trace_amd import _lib
    M, N, K = 300, 256, 256
    for k in (0, 2, 3, 4, 5, 6, 7, 8):
        lib.trace_op_tuning_set(b"gemm.kernel", k)
        for epi in (EPI_NONE, EPI_RESIDUAL, EPI_QUICKGELU, EPI_SWIGLU):
            No = N // 2 if epi == EPI_SWIGLU else N
            assert lib.trace_op_gemm_route(M, N, K, K + 8, K + 8, No + 8, No + 8, epi, 0) >= 0
            for bad in ((K + 4, K, No, No), (K, K + 4, No, No), (K, K, No + 4, No), (K + 2, K + 8, No + 8, No + 8)):
                with pytest.raises(_lib.TraceHipError):
                    lib.trace_op_gemm_route(M, N, K, *bad, epi, 0)
        with pytest.raises(_lib.TraceHipError):
            lib.trace_op_gemm_route(M, N, K, K, K, N, N + 4, EPI_RESIDUAL, 0)
        assert lib.trace_op_gemm_route(M, N, K, K, K, N, N + 4, EPI_NONE, 0) >= 0          # (ldr counts only where a residual is read)
    lib.trace_op_tuning_set(b"gemm.kernel", 0)
    assert lib.trace_op_gemm_route(M, N, K, K + 16, K + 16, N + 8, N + 8, EPI_NONE, 1) >= 0
    with pytest.raises(_lib.TraceHipError):
        lib.trace_op_gemm_route(M, N, K, K + 8, K + 8, N + 8, N + 8, EPI_NONE, 1)


def test_ops_gemm_checks_its_out_argument(lib):
    """ops.gemm's out= / ldc= / out_offset= are checked before anything is launched"""
    from trace_amd.engine import ops
    A, W = torch.zeros((4, 64), dtype=BF), torch.zeros((128, 64), dtype=BF)
    for kw in (dict(ldc=128), dict(out=torch.zeros((4, 64), dtype=BF)), dict(out=torch.zeros((4, 128), dtype=HF)), dict(out=torch.zeros(4 * 128, dtype=BF)),
               dict(out=torch.zeros(4 * 128, dtype=BF), ldc=64), dict(out=torch.zeros(4 * 128, dtype=BF), ldc=128, out_offset=8),
               dict(out=torch.zeros((4, 128, 1), dtype=BF))):
        with pytest.raises(ValueError):
            ops.gemm(A, W, **kw)
    with pytest.raises(ValueError):
        ops.gemm(A.t(), W)
