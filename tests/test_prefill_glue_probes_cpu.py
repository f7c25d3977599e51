"""The prefill cache-write probes judged on the CPU (tests/prefill_glue_probes.py): the fault-free torch emulations of rope_kv, transpose_v and
gather_rows pass every probe tests/test_gpu_prefill_glue_probes.py runs, every listed fault is rejected by a NAMED probe, the Gaussian RoPE judge's bound
holds an fp32 restatement in both operation orders with and without contraction, and a table states which faults leave a full prefill and a
prefix + append of the same prompt with EQUAL caches — the comparison tests/test_gpu_prefix_reuse.py makes, and the reason this file exists."""
import pytest
import torch

import encode_probes as EP
import prefill_glue_probes as PG

BF, HF = torch.bfloat16, torch.float16
DTYPES = [BF, HF]
IDS = ["bf16", "f16"]
ROPE_THETA = 1000000.0


@pytest.fixture(scope="module")
def tables():
    return EP.rope_tables(4096, 128, ROPE_THETA)


# ---- what the probes promise about their own inputs --------------------------------------------------------------------------------------------------
def test_probe_inputs():
    x = PG.hashed_rows(9, 48, 128)
    assert float(x.abs().max()) <= 63 and bool((x == x.round()).all())
    assert bool((x[..., :64] != x[..., 64:]).all()), "d and its partner d + hd/2"
    assert bool((x[..., 0::2] != x[..., 1::2]).all()), "d and d ^ 1 (what interleaved pairs would take)"
    assert bool((x[:, 1:] != x[:, :-1]).all()) and bool((x[1:] != x[:-1]).all()) and bool((x[:, :8] != x[:, 32:40]).all()), "neighbouring heads, rows, q head j and k head j"
    for name in PG.ROPE_EXACT:
        c, s = PG.exact_tables(name, 4096, 64)
        assert set(torch.cat([c, s]).unique().tolist()) <= {0.0, 1.0, -1.0, 0.5, -0.5}
    c, s = PG.exact_tables("per-position", 4096, 64)
    rows = torch.cat([c, s], 1)
    assert rows.unique(dim=0).shape[0] == 4096, "every position has its own table row"
    assert bool(((rows[1:] != rows[:-1]).sum(1) >= 16).all()), "neighbouring positions differ in a quarter of the row at least"
    c, s = PG.exact_tables("quarter-turn", 64, 64)
    assert 0.3 < float((s > 0).float().mean()) < 0.7, "both signs of the sine"
    for dtype in DTYPES:                                        # every product and sum of the exact probes is a 16-bit number
        for name in PG.ROPE_EXACT:
            pr = PG.rope_probe(name, "multi-3xL7", dtype)
            o = PG.rope_reference(pr).o
            assert bool((o.to(dtype).double() == o).all()), name
    cz = PG.codes(70000, 1)
    assert bool((cz != PG.SENTINEL).all()) and bool((cz != 0).all()) and bool((cz[1:] != cz[:-1]).all())
    assert PG.GATHER_ROWS == (5, 3, 7, 2, 1, 4) and len(set(PG.GATHER_ROWS)) == 6
    pr = PG.gather_probe(256, 77, BF)
    seen = {(int(k), int(r)) for k, r in zip(pr.kind, pr.row)}
    for k, n in enumerate(PG.GATHER_ROWS):
        assert (k, 0) in seen and (k, n - 1) in seen, "first and last row of every table"
    assert len(seen) < pr.L, "repeated rows"
    assert 2051 * 4096 // 8 > PG.GRID_THREADS and 2760 * 48 * 8 > PG.GRID_THREADS > 2730 * 48 * 8, "the grid-stride cases pass the launchers' grid cap"
    assert max(c["R"] for c in PG.ROPE_CASES.values()) >= 2731 and {c["R"] for c in PG.ROPE_CASES.values()} >= {1, 7, 64}


def test_gaussian_tables_are_the_engines(tables):
    """trace_ctx_finalize: inv = 1 / float(pow(theta, float(2 j) / float(d))), angle = float(t) * inv in fp32, cos / sin of it in double, stored fp32"""
    import math
    import numpy as np
    cos_t, sin_t = tables
    for t, j in ((0, 0), (1, 0), (1, 63), (4095, 1), (4095, 63), (2047, 17)):
        inv = np.float32(1.0) / np.float32(math.pow(ROPE_THETA, float(np.float32(2 * j) / np.float32(128))))
        ang = float(np.float32(t) * inv)
        assert float(cos_t[t, j]) == float(np.float32(math.cos(ang))) and float(sin_t[t, j]) == float(np.float32(math.sin(ang)))


# ---- the fault-free emulations pass every probe ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unfaulted_rope_passes(dtype, tables):
    for case in PG.ROPE_CASES:
        for name in PG.ROPE_EXACT:
            if case == "grid-stride" and name != "per-position":
                continue
            pr = PG.rope_probe(name, case, dtype)
            assert PG.rope_judge(pr, PG.emulate_rope(pr)) == (0.0, True), (name, case)
    for c in PG.GAUSSIAN_CASES:
        pr = PG.gaussian_rope_probe(c, dtype, tables)
        ratio, intact = PG.rope_judge(pr, PG.emulate_rope(pr))
        assert ratio <= 1.0 and intact, (c["label"], ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gaussian_bound_holds_an_fp32_restatement(dtype, tables):
    """float64 reference against fp32 arithmetic: products then sum in either order, the second product contracted into the sum or not"""
    for c in PG.GAUSSIAN_CASES:
        pr = PG.gaussian_rope_probe(c, dtype, tables, seed=3)
        ref = PG.rope_reference(pr)
        for fma in (False, True):
            for swap in (False, True):
                ratio, intact = PG.rope_judge(pr, PG.emulate_rope(pr, fma=fma, swap_order=swap), ref)
                assert ratio <= 1.0 and intact, (c["label"], fma, swap, ratio)
    # and the bound is not slack: E is a 2^-15 part of the half ulp except where the two products cancel, so one 16-bit ulp off in a row is outside it
    pr = PG.gaussian_rope_probe(PG.GAUSSIAN_CASES[0], dtype, tables)
    ref = PG.rope_reference(pr)
    assert float((ref.bound / EP.half_ulp(ref.o, dtype)).median()) < 1.001
    qkv, kc, vc = PG.emulate_rope(pr)
    PG.bits(kc)[int(ref.idx[3, 0, 5])] += 1
    assert PG.rope_judge(pr, (qkv, kc, vc), ref)[0] > 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unfaulted_transpose_and_gather_pass(dtype):
    for hd in (64, 128):
        for label, kw in PG.transpose_cases(hd):
            pr = PG.transpose_probe(dtype=dtype, **kw)
            assert PG.transpose_judge(pr, PG.emulate_transpose(pr)), (hd, label)
    for label, H, L in PG.GATHER_CASES:
        pr = PG.gather_probe(H, L, dtype)
        assert PG.gather_judge(pr, PG.emulate_gather(pr)), label


def test_transpose_cases_cover_the_edges():
    for hd in (64, 128):
        cases = [kw for _, kw in PG.transpose_cases(hd)]
        plain = {(kw["p0"], kw["n"]) for kw in cases if not kw.get("perm")}
        assert plain >= {(p0, n) for p0 in (0, 1, 7, 8, 9, 63, 64, 65, 100) for n in (1, 2, 7, 8, 55, 64, 65, 130)}
        assert {kw["n"] for kw in cases if kw.get("perm")} >= {128, 130} and all(kw["p0"] == 0 for kw in cases if kw.get("perm"))
        tight = [PG.transpose_probe(dtype=BF, **kw) for kw in cases if kw.get("tight")]
        assert any(pr.p0 + pr.n == pr.dst_rs for pr in tight)
        pr = PG.transpose_probe(dtype=BF, **cases[0])
        assert pr.heads == 2 and pr.batch == 2 and pr.src_rs > pr.heads * pr.hd and pr.dst_hs > pr.hd * pr.dst_rs and pr.dst_bs > pr.heads * pr.dst_hs


def test_transpose_reference_states_the_contract():
    """the reference against the contract spelled out element by element (a small case, python loops)"""
    for perm, p0, n in ((0, 9, 7), (1, 0, 21)):
        pr = PG.transpose_probe(64, p0, n, BF, perm=perm)
        ref, src, before = PG.transpose_reference(pr), PG.bits(pr.src), PG.bits(pr.dst)
        end = PG.round_up(p0 + n, 64)
        for b in range(2):
            for h in range(2):
                for d in (0, 1, 63):
                    for q in range(pr.dst_rs):
                        at = b * pr.dst_bs + h * pr.dst_hs + d * pr.dst_rs + q
                        key = (q // 16) * 16 + PG.PERM16[q % 16] if perm else q - p0
                        if q < p0 or q >= end:
                            want = int(before[at])
                        elif key < n:
                            want = int(src[b * pr.src_bs + h * pr.src_hs + key * pr.src_rs + d])
                        else:
                            want = 0
                        assert int(ref[at]) == want, (perm, b, h, d, q)
        assert PG.PERM16 == (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


# ---- every fault is rejected, and by which probe ---------------------------------------------------------------------------------------------------------
ROPE_REJECTED_BY = {            # fault -> (probe, case)
    "interleaved_pairs": ("quarter-turn", "single-R7"),
    "sin_sign": ("quarter-turn", "single-R1"),
    "second_half_from_rotated_first": ("half", "single-R7"),
    "q_not_rotated": ("quarter-turn", "single-R7"),
    "k_not_rotated": ("quarter-turn", "single-R7"),
    "pos_ignores_past": ("per-position", "past-R64"),
    "pos_not_reset_per_sequence": ("per-position", "multi-3xL7"),
    "pos_off_by_one": ("per-position", "single-R7"),
    "slot_not_advanced": ("identity", "multi-3xL7"),
    "k_head_from_q_index": ("heads", "multi-3xL7"),
    "table_stride_hd": ("per-position", "past-R64"),
    "rows_past_grid_dropped": ("per-position", "grid-stride"),
    "padding_columns_written": ("identity", "ld-padded"),
    "products_rounded_to_16": ("gaussian", "pos0"),
}
TRANSPOSE_REJECTED_BY = {       # fault -> (hd, case, the part of the contract it breaks)
    "p0_chunk_clobbered": (128, "p0=9-n=55", "before-p0"),
    "no_zero_fill": (128, "p0=0-n=55", "zero-fill"),
    "zero_fill_past_block": (64, "p0=0-n=64", "past-block"),
    "rows_past_n_read": (128, "p0=1-n=7", "zero-fill"),
    "perm_ignored": (64, "perm-n=128", "rows"),
    "perm_when_zero": (64, "p0=0-n=64", "rows"),
    "p0_mod_64_ignored": (128, "p0=65-n=130", "before-p0"),
    "batch_head_strides_swapped": (128, "p0=0-n=1", "rows"),
}
GATHER_REJECTED_BY = {"kind_ignored": "H256-L77", "last_chunk_dropped": "H8-L1", "gather_rows_past_grid_dropped": "H4096-grid-stride"}


def test_fault_tables_are_complete():
    assert set(ROPE_REJECTED_BY) == set(PG.ROPE_FAULTS) and set(TRANSPOSE_REJECTED_BY) == set(PG.TRANSPOSE_FAULTS) and set(GATHER_REJECTED_BY) == set(PG.GATHER_FAULTS)


@pytest.mark.parametrize("fault", PG.ROPE_FAULTS)
def test_rope_fault_is_rejected(fault, tables):
    name, case = ROPE_REJECTED_BY[fault]
    for dtype in DTYPES:
        if name == "gaussian":
            pr = PG.gaussian_rope_probe(next(c for c in PG.GAUSSIAN_CASES if c["label"] == case), dtype, tables)
        else:
            pr = PG.rope_probe(name, case, dtype)
        ratio, intact = PG.rope_judge(pr, PG.emulate_rope(pr, fault))
        assert ratio > 1.0 or not intact, f"{fault} passes {name} @ {case}"
        if fault == "padding_columns_written":
            assert ratio == 0.0 and not intact, "only the sentinel in the padding columns shows it"
        if fault == "products_rounded_to_16":                  # exact products: no exact probe can see it, the Gaussian one must
            e = PG.rope_probe("half", "single-R7", dtype)
            assert PG.rope_judge(e, PG.emulate_rope(e, fault)) == (0.0, True)


@pytest.mark.parametrize("fault", PG.TRANSPOSE_FAULTS)
def test_transpose_fault_is_rejected(fault):
    hd, case, region = TRANSPOSE_REJECTED_BY[fault]
    kw = dict(PG.transpose_cases(hd))[case]
    for dtype in DTYPES:
        pr = PG.transpose_probe(dtype=dtype, **kw)
        got = PG.emulate_transpose(pr, fault)
        assert not PG.transpose_judge(pr, got), f"{fault} passes hd {hd} {case}"
        assert region in PG.transpose_region_report(pr, got), (fault, PG.transpose_region_report(pr, got))


@pytest.mark.parametrize("fault", PG.GATHER_FAULTS)
def test_gather_fault_is_rejected(fault):
    label, H, L = next(c for c in PG.GATHER_CASES if c[0] == GATHER_REJECTED_BY[fault])
    for dtype in DTYPES:
        pr = PG.gather_probe(H, L, dtype)
        assert not PG.gather_judge(pr, PG.emulate_gather(pr, fault)), f"{fault} passes {label}"


# ---- what a prefill-against-prefill comparison cannot see ------------------------------------------------------------------------------------------------
# The same fault in a full prefill of 79 rows and in a prefill of 66 rows continued by 13 at past = 66 (the cut of tests/test_gpu_prefix_reuse.py): the two
# K caches and the two V^T caches come out EQUAL over the prompt's positions for every fault listed here, so that comparison passes with the fault in.
INVISIBLE_TO_PREFIX_REUSE = (
    "interleaved_pairs", "sin_sign", "second_half_from_rotated_first", "q_not_rotated", "k_not_rotated", "pos_not_reset_per_sequence", "pos_off_by_one",
    "slot_not_advanced", "k_head_from_q_index", "table_stride_hd", "rows_past_grid_dropped", "padding_columns_written", "products_rounded_to_16",
    "no_zero_fill", "zero_fill_past_block", "rows_past_n_read", "perm_ignored", "perm_when_zero", "batch_head_strides_swapped")
VISIBLE_TO_PREFIX_REUSE = ("pos_ignores_past", "p0_chunk_clobbered", "p0_mod_64_ignored")


def test_faults_a_prefill_against_prefill_comparison_cannot_see():
    assert set(INVISIBLE_TO_PREFIX_REUSE) | set(VISIBLE_TO_PREFIX_REUSE) == set(PG.ROPE_FAULTS) | set(PG.TRANSPOSE_FAULTS)
    for dtype in DTYPES:
        (k0, v0), (k1, v1) = PG.emulate_prefill_writes(79, 66, dtype, nq=8, nkv=2)
        assert torch.equal(k0, k1) and torch.equal(v0, v1), "fault free: the identity the prefix-reuse tests rely on"
        for fault in PG.ROPE_FAULTS + PG.TRANSPOSE_FAULTS:
            kw = dict(rope_fault=fault) if fault in PG.ROPE_FAULTS else dict(transpose_fault=fault)
            (a, b), (c, d) = PG.emulate_prefill_writes(79, 66, dtype, nq=8, nkv=2, **kw)
            same = torch.equal(a, c) and torch.equal(b, d)
            assert same == (fault in INVISIBLE_TO_PREFIX_REUSE), f"{fault}: full and prefix + append caches {'equal' if same else 'differ'}"
            if same and fault not in ("rows_past_grid_dropped", "padding_columns_written", "slot_not_advanced", "pos_not_reset_per_sequence", "zero_fill_past_block",
                             "no_zero_fill", "rows_past_n_read", "perm_ignored", "q_not_rotated", "products_rounded_to_16"):   # (no effect on ONE short exact prompt's positions)
                assert not (torch.equal(a, k0) and torch.equal(b, v0)), f"{fault} leaves this prompt's caches right: it proves nothing here"
