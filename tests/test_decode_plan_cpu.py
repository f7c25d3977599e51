"""The host rules of the decode step — how a decode GEMV is cut into workgroups (csrc/decode.hip skinny_plan), how many partial-row floats a projection
needs at any batch (skinny_partial_floats) and what a step of B sequences does (csrc/engine.hip decode_route) — checked on the built library without a GPU.

The rules below are restated from the commit before they were unified (decode.hip's skinny_plan / skinny_lds_launch, fp8.hip's fp8_plan / fp8_launch,
gemm.hip's gemm_partial_ks, the `if` chain of engine.hip's decode_step and its decode_nsplit), not read from the library.  With no device the library
plans for 256 CUs, which is the MI355X's own count: the table checked here is the table the GPU runs."""
import ctypes as C
import itertools
import os

import pytest

EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU, EPI_PARTIAL = 0, 1, 3, 4
BF16, W8A8, W8A16 = 0, 1, 2
SK_ROWS, SKINNY_ROWS, NCU = 256, 64, 256
GEOMETRIES = [(4096, 14336, 6144), (4096, 16384, 6144), (2048, 8192, 3072), (1024, 2816, 1536), (256, 512, 384), (128, 256, 192)]      # H, I, QKV
TINY, LLM7B = (4096, 256, 6144), (4096, 14336, 6144)
PLAN_FIELDS = ("KS", "chunk_units", "T", "WPT", "ntiles", "grid", "threads", "NT", "NB", "lds_bytes")


def projections(H, I, QKV):
    """(N, K) of qkv, o, gate|up, down"""
    return [(QKV, H), (H, H), (2 * I, H), (H, I)]


def epilogues(kind, N):
    return [EPI_PARTIAL] if kind != BF16 else [EPI_NONE, EPI_RESIDUAL, EPI_PARTIAL] + ([EPI_SWIGLU] if N % 32 == 0 else [])


def plan(kind, N, K, epi, B):
    """one statement of skinny_plan (bf16: 64-k units, 64 of them in LDS) and fp8_plan (128-k units; 64 as e4m3 images, 32 as bf16 rows), with the
    launchers' LDS bytes: 2 KB per unit and 16-row group (4 KB for bf16 rows beside e4m3 weights) + 1 KB of reduction scratch per wave, tile and group"""
    unit, units_in_lds, kb_per_unit = {BF16: (64, 64, 2), W8A8: (128, 64, 2), W8A16: (128, 32, 4)}[kind]
    NT = 2 if epi == EPI_SWIGLU or (epi == EPI_PARTIAL and N >= 16384 and N % 32 == 0) else 1
    NB = 4 if B > 32 else 2 if B > 16 else 1
    U = K // unit
    cap = units_in_lds // NB
    ks_min = -(-U // cap)
    ks_max = min(U, ks_min + 4) if epi == EPI_PARTIAL else ks_min
    ntiles = N // (16 * NT)
    best = None
    for ks in range(ks_min, ks_max + 1):
        chunk = -(-U // ks)
        for T in range(1, 17):
            grid = ks * -(-ntiles // T)
            rounds = -(-grid // NCU)
            cost = rounds * T * chunk * 64 + rounds * 8 + ks
            if best is None or cost < best[0]:
                best = (cost, ks, chunk, T, grid)
    _, KS, chunk, T, grid = best
    WPT = 1
    while WPT * 2 * T <= 8 and WPT * 2 * T * NT * NB <= 28 and WPT * 2 <= chunk:
        WPT *= 2
    lds = chunk * kb_per_unit * NB * 1024 + (T * WPT * NT * NB * 1024 if WPT > 1 else 0)
    return dict(KS=KS, chunk_units=chunk, T=T, WPT=WPT, ntiles=ntiles, grid=grid, threads=min(T, 8) * WPT * 64, NT=NT, NB=NB, lds_bytes=lds)


@pytest.fixture(scope="module")
def lib():
    from trace_amd import build, _lib
    assert "TRACE_SK_CAP" not in os.environ and "TRACE_PARTIAL_WGS" not in os.environ, "these change the rules this file checks"
    build.build()
    return _lib.load()


@pytest.fixture(autouse=True)
def fresh(lib):
    lib.trace_op_tuning_reset()
    yield
    lib.trace_op_tuning_reset()


def lib_plan(lib, kind, N, K, epi, B):
    out = (C.c_int64 * 11)()
    lib.trace_op_skinny_plan(kind, N, K, epi, B, out)
    return dict(zip(PLAN_FIELDS, out)), out[10]


def test_skinny_plan_is_the_stated_partition(lib):
    cases = 0
    for (H, I, QKV), kind in itertools.product(GEOMETRIES, (BF16, W8A8, W8A16)):
        for N, K in projections(H, I, QKV):
            for epi in epilogues(kind, N):
                for B in range(1, SKINNY_ROWS + 1):
                    got, _ = lib_plan(lib, kind, N, K, epi, B)
                    assert got == plan(kind, N, K, epi, B), (kind, N, K, epi, B)
                    assert got["lds_bytes"] <= 160 * 1024                # the CU's LDS
                    if kind == BF16:
                        assert lib.trace_op_skinny_ks(N, K, epi, B) == got["KS"]
                    cases += 1
    assert cases == 9216


def test_skinny_plan_rejects_what_the_launchers_reject(lib):
    from trace_amd._lib import TraceHipError
    out = (C.c_int64 * 11)()
    for kind, N, K, epi, B in [(BF16, 4096, 4096, EPI_PARTIAL, 0), (BF16, 4096, 4096, EPI_PARTIAL, 65), (BF16, 4096, 4096 + 32, EPI_PARTIAL, 1),
                               (BF16, 4096 + 8, 4096, EPI_NONE, 1), (BF16, 4096 + 16, 4096, EPI_SWIGLU, 1), (BF16, 4096, 4096, 2, 1), (BF16, 4096, 4096, 5, 1),
                               (W8A8, 4096, 4096 + 64, EPI_PARTIAL, 1), (W8A16, 4096, 4096 + 64, EPI_PARTIAL, 1), (W8A8, 4096, 4096, EPI_NONE, 1),
                               (W8A16, 4096, 4096, EPI_SWIGLU, 1), (W8A8, 4096 + 8, 4096, EPI_PARTIAL, 1), (W8A16, 4096, 4096, EPI_PARTIAL, 65),
                               (3, 4096, 4096, EPI_PARTIAL, 1), (-1, 4096, 4096, EPI_PARTIAL, 1), (BF16, 4096, 0, EPI_PARTIAL, 1)]:
        with pytest.raises(TraceHipError, match="error -1 in trace_op_skinny_plan"):
            lib.trace_op_skinny_plan(kind, N, K, epi, B, out)
    lib.trace_op_skinny_plan(BF16, 4096 + 16, 4096 + 64, EPI_RESIDUAL, 64, out)      # 16-row and 64-k granules: accepted
    lib.trace_op_skinny_plan(W8A16, 4096 + 16, 4096 + 128, EPI_PARTIAL, 64, out)


def test_partial_floats_hold_every_batch(lib):
    """a condition, not a tolerance: the workspace sized from the three batch classes holds the partial rows of every B, and is no larger than the
    largest of them"""
    for (H, I, QKV), kind in itertools.product(GEOMETRIES, (BF16, W8A8, W8A16)):
        for N, K in projections(H, I, QKV):
            needs, sizes = [], set()
            for B in range(1, SKINNY_ROWS + 1):
                got, floats = lib_plan(lib, kind, N, K, EPI_PARTIAL, B)
                needs.append(got["KS"] * SK_ROWS * N)
                sizes.add(floats)
            assert len(sizes) == 1, (kind, N, K, sizes)                # one figure per kind and shape, whatever B asks
            assert max(needs) == sizes.pop(), (kind, N, K)              # >= every B's need, == at least one


# ---- the step route ------------------------------------------------------------------------------------------------------------------------
def gemm_partial_ks(N, K, partial_wgs):
    """gemm.hip: chunks of whole 64-k tiles, at least 4 tiles a chunk, until (N / 128 column tiles) x ks reaches the workgroup target (0 = 192)"""
    target = partial_wgs if partial_wgs > 0 else 192
    tiles, nk, ks = N // 128, K // 64, 1
    while tiles * ks < target and nk % (ks * 2) == 0 and nk // (ks * 2) >= 4:
        ks *= 2
    return ks


def fused_norm_ok(N, K, B):
    return 1 <= B <= 4 and K % 64 == 0 and K <= 16384 and N % 16 == 0 and (K >> 3) <= 2 * plan(BF16, N, K, EPI_PARTIAL, B)["threads"]


class Routes:
    """decode_step's conditions for one geometry; the chunk counts tabulated once per batch class / workgroup target"""

    def __init__(self, H, I, QKV):
        self.shapes = projections(H, I, QKV)
        self.sk = {(kind, B): [plan(kind, N, K, EPI_PARTIAL, B)["KS"] for N, K in self.shapes] for kind in (BF16, W8A8, W8A16) for B in (16, 32, 64)}
        self.wide = {w: [gemm_partial_ks(N, K, w) for N, K in self.shapes] for w in (0, 64, 192, 256)}
        self.fusable = {B: fused_norm_ok(QKV, H, B) and fused_norm_ok(2 * I, H, B) for B in range(1, 5)}

    def route(self, B, scheme, wide_min_rows, fuse_norm_rows, unfused_qkv, wide_fuse_qkv, nsplit, partial_wgs):
        fp8 = scheme != 0
        kind = (BF16, W8A8, W8A16)[scheme]
        ns = nsplit if nsplit > 0 else max(1, min(16, (40 + B // 2) // B))
        if B > SKINNY_ROWS or (B >= wide_min_rows and not fp8):
            q, o, _, d = self.wide[partial_wgs]
            return (3, kind, int(not wide_fuse_qkv), q, o, 0, d, ns)
        q, o, g, d = self.sk[kind, 16 if B <= 16 else 32 if B <= 32 else 64]
        if B <= fuse_norm_rows and not fp8 and self.fusable[B]:
            return (2, kind, 0, q, o, g, d, ns)
        return (1, kind, int(unfused_qkv == 1 or (unfused_qkv == 0 and B >= 32)), q, o, g, d, ns)


def tune(lib, **kw):
    for k, v in kw.items():
        lib.trace_op_tuning_set(k.replace("__", ".").encode(), v)


@pytest.mark.parametrize("wide_min_rows", [17, 32, 33, 65])
@pytest.mark.parametrize("geometry", [TINY, LLM7B], ids=["tiny", "7b"])
def test_decode_route_is_the_stated_rule(lib, geometry, wide_min_rows):
    R = Routes(*geometry)
    out = (C.c_int32 * 8)()
    steps = set()
    tune(lib, decode__wide_min_rows=wide_min_rows)
    for fuse_norm_rows, unfused_qkv, wide_fuse_qkv, nsplit, partial_wgs in itertools.product(range(5), range(3), range(2), (0, 1, 16), (0, 64, 192, 256)):
        tune(lib, decode__fuse_norm_rows=fuse_norm_rows, decode__unfused_qkv=unfused_qkv, decode__wide_fuse_qkv=wide_fuse_qkv,
             attn__decode__nsplit=nsplit, decode__partial_wgs=partial_wgs)
        for scheme in (0, 1, 2):
            for B in range(1, (SKINNY_ROWS if scheme else SK_ROWS) + 1):
                lib.trace_op_decode_route(B, scheme, *geometry, out)
                want = R.route(B, scheme, wide_min_rows, fuse_norm_rows, unfused_qkv, wide_fuse_qkv, nsplit, partial_wgs)
                assert tuple(out) == want, (B, scheme, fuse_norm_rows, unfused_qkv, wide_fuse_qkv, nsplit, partial_wgs)
                steps.add((scheme, want[0]))
    assert steps == {(0, 1), (0, 2), (0, 3), (1, 1), (2, 1)}


def test_decode_route_rejects_what_decode_begin_rejects(lib):
    """B outside 1..256, and more than 64 sequences on fp8 weights: refused before any tuning value is read, so under two settings"""
    from trace_amd._lib import TraceHipError
    out = (C.c_int32 * 8)()
    for setting in ({}, dict(decode__wide_min_rows=65, decode__fuse_norm_rows=4, decode__wide_fuse_qkv=1)):
        tune(lib, **setting)
        for B, scheme in [(0, 0), (-1, 0), (SK_ROWS + 1, 0), (1, 3), (1, -1)] + [(B, s) for B in range(SKINNY_ROWS + 1, SK_ROWS + 1) for s in (1, 2)]:
            with pytest.raises(TraceHipError, match="error -1 in trace_op_decode_route"):
                lib.trace_op_decode_route(B, scheme, *TINY, out)


def test_the_probes_split_count_is_the_routes(lib):
    import attn_probes as P
    from trace_amd.engine import ops
    for B in range(1, SK_ROWS + 1):
        assert P.decode_nsplit(B) == ops.decode_route(B, 0, *LLM7B)["nsplit"], B
    assert ops.skinny_plan(BF16, 4096, 4096, EPI_PARTIAL, 1)["KS"] == ops.skinny_ks(4096, 4096, EPI_PARTIAL, 1)
