"""The table of named tuning values (csrc/tuning.h, csrc/engine.hip TUNE_ROWS), the numeric codes of trace_op_set_gemm_variant that write the same
fields, and the 256^2 GEMM routing rule (csrc/gemm.hip gemm_route) — all host code: checked on the built library without a GPU.

The defaults, the code ranges and the routing rule below are restated from the commit before the table existed (the `int g_...` initialisers, the
`if` chain of trace_op_set_gemm_variant, the body of launch_gemm_bf16), not read from the library."""
import ctypes as C
import os
import random

import pytest

# name -> default: the initialisers of the former globals (gemm.w4 was -1 = "TRACE_GEMM_W4, else on"; decode.partial_wgs 0 = "TRACE_PARTIAL_WGS, else 192")
DEFAULTS = {
    "gemm.kernel": 0, "gemm.w4": 1, "gemm.resid_pers": 0, "gemm.pers.walk": 0, "gemm.pers.opt": 0, "gemm.pers.grid_cap": 0, "gemm.ldr.opt": 0,
    "gemm.w4.opt": 0, "decode.wide_min_rows": 32, "decode.wide_fuse_qkv": 0, "decode.gemm_tiled": 21, "decode.fuse_norm_rows": 1,
    "decode.fuse_swiglu": 1, "decode.unfused_qkv": 0, "decode.partial_cfg": 0, "decode.partial_wgs": 192, "attn.decode.debug": 0,
    "attn.decode.waves": -1, "attn.decode.nt": 0, "attn.decode.lds_pad_kb": 0, "attn.decode.nsplit": 0, "attn.prefill.debug": 0, "attn.vit.big": 2,
    "skinny.debug": 0, "prefill.last_rows": 1, "vit.patch_fused": 1,
}

# (first code, last code, field, value stored for a code): the `if` chain of the former trace_op_set_gemm_variant, in its order
LEGACY = [
    (1000, 2024, "gemm.pers.grid_cap", lambda c: c - 1000),
    (100, 109, "attn.decode.debug", lambda c: c - 100),
    (110, 119, "attn.prefill.debug", lambda c: c - 110),
    (120, 122, "decode.unfused_qkv", lambda c: c - 120),
    (130, 137, "decode.gemm_tiled", lambda c: c - 130),
    (760, 764, "attn.decode.waves", lambda c: -1 if c == 762 else c - 760),
    (780, 799, "attn.decode.lds_pad_kb", lambda c: (c - 780) * 8),
    (770, 771, "attn.decode.nt", lambda c: c - 770),
    (750, 751, "prefill.last_rows", lambda c: c - 750),
    (740, 743, "decode.partial_cfg", lambda c: c - 740),
    (800, 832, "decode.partial_wgs", lambda c: (c - 800) * 32),
    (700, 731, "decode.gemm_tiled", lambda c: c - 700),
    (160, 161, "vit.patch_fused", lambda c: c - 160),
    (170, 174, "decode.fuse_norm_rows", lambda c: c - 170),
    (180, 181, "decode.fuse_swiglu", lambda c: c - 180),
    (190, 192, "attn.vit.big", lambda c: c - 190),
    (850, 866, "attn.decode.nsplit", lambda c: c - 850),
    (144, 145, "decode.wide_fuse_qkv", lambda c: c - 144),
    (140, 143, "decode.wide_min_rows", lambda c: {140: 65, 141: 33, 142: 17, 143: 32}[c]),
    (200, 209, "skinny.debug", lambda c: c - 200),
    (300, 363, "gemm.pers.opt", lambda c: c - 300),
    (500, 501, "gemm.pers.walk", lambda c: c - 500),
    (520, 521, "gemm.resid_pers", lambda c: c - 520),
    (530, 531, "gemm.w4", lambda c: c - 530),
    (540, 547, "gemm.w4.opt", lambda c: c - 540),
    (400, 403, "gemm.ldr.opt", lambda c: c - 400),
    (0, 8, "gemm.kernel", lambda c: c),
]
REJECTED = [-1, -1000, 9, 10, 99, 123, 129, 138, 139, 146, 159, 162, 175, 193, 210, 299, 364, 404, 499, 502, 522, 532, 548, 699, 732, 744, 752, 765,
            772, 779, 833, 849, 867, 999, 2025, 2100, 1 << 30]


@pytest.fixture(scope="module")
def lib():
    from trace_amd import build, _lib
    assert "TRACE_GEMM_W4" not in os.environ and "TRACE_PARTIAL_WGS" not in os.environ, "these set the initial values this file checks"
    build.build()
    return _lib.load()


@pytest.fixture(autouse=True)
def fresh(lib):
    lib.trace_op_tuning_reset()
    yield
    lib.trace_op_tuning_reset()


def names(lib):
    out = []
    while (n := lib.trace_op_tuning_name(len(out))) is not None:
        out.append(n.decode())
    return out


def get(lib, name):
    v = C.c_int(-12345)
    lib.trace_op_tuning_get(name.encode(), C.byref(v))
    return v.value


def snapshot(lib):
    return {n: get(lib, n) for n in names(lib)}


def test_every_field_is_named_once_with_its_default(lib):
    ns = names(lib)
    assert len(ns) == len(set(ns)) and set(ns) == set(DEFAULTS), set(ns) ^ set(DEFAULTS)
    assert lib.trace_op_tuning_name(-1) is None and lib.trace_op_tuning_name(len(ns)) is None
    assert snapshot(lib) == DEFAULTS


def test_legacy_codes_store_what_they_stored(lib):
    assert len(LEGACY) == 27
    for lo, hi, field, value in LEGACY:
        codes = range(lo, hi + 1) if hi - lo < 8 else (lo, (lo + hi) // 2, hi)       # both ends and the inside; short ranges whole
        for code in codes:
            lib.trace_op_tuning_reset()
            assert lib.trace_op_set_gemm_variant(code) == 0
            want = dict(DEFAULTS)
            want[field] = value(code)
            assert snapshot(lib) == want, code


def test_legacy_special_cases(lib):
    for code, field, want in [(140, "decode.wide_min_rows", 65), (141, "decode.wide_min_rows", 33), (142, "decode.wide_min_rows", 17),
                              (143, "decode.wide_min_rows", 32), (762, "attn.decode.waves", -1), (761, "attn.decode.waves", 1),
                              (764, "attn.decode.waves", 4), (783, "attn.decode.lds_pad_kb", 24), (799, "attn.decode.lds_pad_kb", 152),
                              (806, "decode.partial_wgs", 192), (832, "decode.partial_wgs", 1024), (800, "decode.partial_wgs", 0),
                              (135, "decode.gemm_tiled", 5), (705, "decode.gemm_tiled", 5), (721, "decode.gemm_tiled", 21), (116, "attn.prefill.debug", 6)]:
        lib.trace_op_set_gemm_variant(code)
        assert get(lib, field) == want, code


def test_rejected_codes(lib):
    from trace_amd._lib import TraceHipError
    lib.trace_op_tuning_set(b"gemm.kernel", 5)
    before = snapshot(lib)
    for code in REJECTED:
        with pytest.raises(TraceHipError, match=r"error -1 in trace_op_set_gemm_variant: variant must be 0\.\.8$"):
            lib.trace_op_set_gemm_variant(code)
        assert lib.trace_last_error() == b"variant must be 0..8"
        assert snapshot(lib) == before, code


def test_set_checks_names_and_ranges_and_reset_restores(lib):
    from trace_amd._lib import TraceHipError
    for name, value in [("gemm.kernel", 9), ("gemm.kernel", -1), ("gemm.w4", 2), ("decode.gemm_tiled", 32), ("attn.decode.waves", -2),
                        ("attn.decode.waves", 5), ("decode.wide_min_rows", 0), ("decode.wide_min_rows", 66), ("gemm.pers.grid_cap", 1025),
                        ("attn.decode.lds_pad_kb", 153), ("decode.partial_wgs", 1025), ("no.such.value", 0), ("gemm", 0), ("", 0), ("gemm.kernel ", 0)]:
        with pytest.raises(TraceHipError, match="error -1 in trace_op_tuning_set"):
            lib.trace_op_tuning_set(name.encode(), value)
    with pytest.raises(TraceHipError, match="error -1 in trace_op_tuning_get"):
        lib.trace_op_tuning_get(b"no.such.value", C.byref(C.c_int(0)))
    assert snapshot(lib) == DEFAULTS                                   # a rejected set writes nothing
    for n in names(lib):                                                # every field away from its default, inside its range
        lib.trace_op_tuning_set(n.encode(), {"decode.wide_min_rows": 17, "attn.decode.waves": 3, "decode.partial_wgs": 64}.get(n, 1 - DEFAULTS[n] if DEFAULTS[n] in (0, 1) else 1))
    moved = snapshot(lib)
    assert all(moved[n] != DEFAULTS[n] for n in DEFAULTS), moved
    assert lib.trace_op_tuning_reset() == 0
    assert snapshot(lib) == DEFAULTS


def test_tuned_restores_the_values_it_found(lib):
    from trace_amd.engine import ops
    assert ops.tuning_names() == names(lib)
    ops.tune("gemm.w4.opt", 4)
    with ops.tuned(gemm__kernel=8, gemm__w4__opt=1):
        assert (get(lib, "gemm.kernel"), get(lib, "gemm.w4.opt")) == (8, 1)
        with pytest.raises(ZeroDivisionError):
            with ops.tuned(gemm__kernel=5, attn__decode__waves=1):
                assert (get(lib, "gemm.kernel"), get(lib, "attn.decode.waves")) == (5, 1)
                1 / 0
        assert (get(lib, "gemm.kernel"), get(lib, "gemm.w4.opt"), get(lib, "attn.decode.waves")) == (8, 1, -1)
    assert (get(lib, "gemm.kernel"), get(lib, "gemm.w4.opt")) == (0, 4)
    with pytest.raises(Exception):
        with ops.tuned(gemm__kernel=4, no__such__value=1):
            pass
    assert get(lib, "gemm.kernel") == 0                               # a failing entry restores what it had set


# ---- routing -----------------------------------------------------------------------------------------------------------------------------
EPI_NONE, EPI_RESIDUAL, EPI_QUICKGELU, EPI_SWIGLU = 0, 1, 2, 3
GLDS128, GLDS256, LDR, PERS, W4 = range(5)


def shape_ok(M, N, K, lda, ldw, ldc, ldr, epi, fp8):
    """what launch_gemm_bf16 takes at all (128 x 128 x 64 tiles; fp8: 128-byte K-tiles, 16-byte rows, no QuickGELU)"""
    if M <= 0 or N % 128 or K % 64 or K < 64:
        return False
    if fp8 and (K % 128 or lda % 16 or ldw % 16 or epi == EPI_QUICKGELU):
        return False
    if lda % 8 or ldw % 8 or ldc % 8:
        return False
    return not (epi == EPI_RESIDUAL and ldr % 8)


def route(M, N, K, lda, ldw, ldc, ldr, epi, fp8, k, w4, resid_pers):
    blocks256 = -(-M // 256) * (N // 256)
    rounds = -(-blocks256 // 256)
    big = N % 256 == 0 and M >= 1024 and blocks256 * 10 >= rounds * 256 * 7
    pers_ok = N % 256 == 0 and not fp8 and K >= 128 and M * ldc < 2 ** 30 and (epi != EPI_RESIDUAL or M * ldr < 2 ** 30)
    w4_ok = pers_ok and K >= 192 and M * lda < 2 ** 31 and N * ldw < 2 ** 31
    if k == 8 and w4_ok:
        return W4, 0
    if 5 <= k <= 7 and pers_ok:
        return PERS, k - 5
    if (k == 4 or (k == 0 and big)) and N % 256 == 0:
        if k == 0 and pers_ok and (epi != EPI_RESIDUAL or resid_pers):
            return (W4, 0) if w4 and epi != EPI_RESIDUAL and w4_ok else (PERS, 0)
        return LDR, 0
    if k == 3 and N % 256 == 0:
        return GLDS256, 0
    return GLDS128, 0


def engine_shapes():
    """(M, N, K, lda, ldw, ldc, ldr, epi, fp8) of the GEMMs the full-size engine launches"""
    out = []
    Mv, vh, vi = 128 * 577, 1024, 4096                                      # ViT-L/14 at 336 px, 128 frames a call
    out += [(Mv, 3 * vh, vh, vh, vh, 3 * vh, 0, EPI_NONE, 0), (Mv, vh, vh, vh, vh, vh, vh, EPI_RESIDUAL, 0),
            (Mv, vi, vh, vh, vh, vi, 0, EPI_QUICKGELU, 0), (Mv, vh, vi, vi, vi, vh, vh, EPI_RESIDUAL, 0)]
    H, I, QKV, QW = 4096, 14336, 6144, 4096                                  # the 7B decoder
    for L, nb in [(1967, 1), (1967, 2), (1967, 4), (1086, 7)]:
        M = L * nb
        out += [(M, QKV, H, H, H, QKV, 0, EPI_NONE, 0), (M, H, H, H, H, H, H, EPI_RESIDUAL, 0), (M, 2 * I, H, H, H, I, 0, EPI_SWIGLU, 0),
                (M, H, I, I, I, H, H, EPI_RESIDUAL, 0)]
        # the last layer: k | v for every row, the rest for each prompt's last row (row stride L x width)
        out += [(M, QKV - QW, H, H, H, QKV, 0, EPI_NONE, 0), (nb, QW, H, L * H, H, L * QKV, 0, EPI_NONE, 0),
                (nb, H, H, L * H, H, L * H, L * H, EPI_RESIDUAL, 0), (nb, 2 * I, H, L * H, H, L * I, 0, EPI_SWIGLU, 0),
                (nb, H, I, L * I, I, L * H, L * H, EPI_RESIDUAL, 0)]
        # the same four on the fp8 weight path (byte strides)
        out += [(M, QKV, H, H, H, QKV, 0, EPI_NONE, 1), (M, H, H, H, H, H, H, EPI_RESIDUAL, 1), (M, 2 * I, H, H, H, I, 0, EPI_SWIGLU, 1),
                (M, H, I, I, I, H, H, EPI_RESIDUAL, 1)]
    return out


def random_shapes(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        M = rng.choice([rng.randint(1, 300), rng.randint(1, 5000), rng.randint(1000, 80000), rng.randint(200000, 600000), 0, -3, 1024, 1023])
        N = rng.choice([128, 256, 384, 512, 1024, 3072, 4096, 6144, 28672, 100, 192]) * rng.choice([1, 1, 1, 2])
        K = rng.choice([64, 128, 192, 256, 320, 1024, 4096, 14336, 32, 96, 0])
        epi = rng.choice([EPI_NONE, EPI_RESIDUAL, EPI_QUICKGELU, EPI_SWIGLU])
        fp8 = rng.random() < 0.2
        pad = lambda x: x + rng.choice([0, 0, 0, 8, 16, 4, 4096 * rng.randint(1, 4)])        # (4: a stride the launcher rejects)
        lda, ldw = pad(max(K, 8)), pad(max(K, 8))
        ldc = pad(N // 2 if epi == EPI_SWIGLU else N)
        ldr = pad(N) if epi == EPI_RESIDUAL or rng.random() < 0.1 else 0
        if rng.random() < 0.15:                                              # rows a long way apart: the 32-bit offset limits of the persistent kernels
            which = rng.randrange(4)
            far = rng.choice([1 << 13, 1 << 15, 1 << 18, 1 << 20])
            lda, ldw, ldc, ldr = (lda * far if which == 0 else lda), (ldw * far if which == 1 else ldw), (ldc * far if which == 2 else ldc), (ldr * far if which == 3 else ldr)
        if max(lda, ldw, ldc, ldr) < 2 ** 31:
            out.append((M, N, K, lda, ldw, ldc, ldr, epi, int(fp8)))
    return out


def test_gemm_route_is_the_stated_rule(lib):
    from trace_amd._lib import TraceHipError
    shapes = engine_shapes() + random_shapes(2400, 20251017)
    assert len(shapes) >= 2000 + len(engine_shapes())
    reached, rejected = set(), 0
    for k in (0, 2, 3, 4, 5, 6, 7, 8):
        for w4 in (0, 1):
            for rp in (0, 1):
                lib.trace_op_tuning_set(b"gemm.kernel", k)
                lib.trace_op_tuning_set(b"gemm.w4", w4)
                lib.trace_op_tuning_set(b"gemm.resid_pers", rp)
                for sh in shapes:
                    if not shape_ok(*sh):
                        with pytest.raises(TraceHipError, match="error -1 in trace_op_gemm_route"):
                            lib.trace_op_gemm_route(*sh)
                        rejected += 1
                        continue
                    got = lib.trace_op_gemm_route(*sh)
                    want = route(*sh, k, w4, rp)
                    assert (got & 255, got >> 8) == want, (sh, k, w4, rp, got)
                    reached.add(want)
    assert {r[0] for r in reached} == {GLDS128, GLDS256, LDR, PERS, W4}
    assert {(PERS, 0), (PERS, 1), (PERS, 2), (W4, 0)} <= reached and rejected > 0
    # what the engine's own shapes run on as shipped: the ViT and prefill projections on the persistent kernels, residual ones on the loader-wave kernel
    lib.trace_op_tuning_reset()
    Mv = 128 * 577
    assert lib.trace_op_gemm_route(Mv, 3072, 1024, 1024, 1024, 3072, 0, EPI_NONE, 0) == W4
    assert lib.trace_op_gemm_route(Mv, 1024, 1024, 1024, 1024, 1024, 1024, EPI_RESIDUAL, 0) == LDR
    assert lib.trace_op_gemm_route(1, 4096, 4096, 1967 * 4096, 4096, 1967 * 6144, 0, EPI_NONE, 0) == GLDS128


def test_static_walk_is_forced_on_every_persistent_route(lib):
    sh = (40000, 1024, 512, 512, 512, 1024, 0, EPI_NONE, 0)              # 628 tiles of 256^2: auto routing takes them
    lib.trace_op_tuning_set(b"gemm.pers.walk", 1)
    for k, want in [(0, W4 | 1 << 8), (5, PERS | 1 << 8), (6, PERS | 1 << 8), (7, PERS | 2 << 8), (8, W4 | 1 << 8), (4, LDR), (2, GLDS128)]:
        lib.trace_op_tuning_set(b"gemm.kernel", k)
        assert lib.trace_op_gemm_route(*sh) == want, k
