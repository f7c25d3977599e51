"""The identity-layer decoder of tests/token_select_probes.py, checked without a device: every named case has the property it claims, the plain
restatement of the selection rules equals the oracle on the crafted weights, and the batches the device tests run tell the rules from ten near
misses (a restatement with one rule broken on purpose must give other ids on them)."""
import os

import numpy as np
import pytest
import torch

import token_select_probes as P
from oracle.trace_oracle import Oracle
from trace_amd import synth


@pytest.fixture(scope="module", params=list(P.GEOMETRIES))
def geom(request):
    cfg = P.GEOMETRIES[request.param]()
    T, plan = P.build_table(cfg)
    return request.param, cfg, T, plan


def test_named_cases_hold(geom):
    name, cfg, T, plan = geom
    V, Tv, Sv, NV, NVpad = P.dims(cfg)
    assert T.shape == (NV, NVpad) and T.min() >= -64 and T.max() <= 64 and (T[:, NV:] == 0).all()
    for c in plan.cases:
        P.check_case(T, cfg, c)
        assert P.column(cfg, c.token) is not None and P.select(T[c.token], *P.head_range(cfg, c.head)) == c.expect
    kinds = {h: {c.kind for c in plan.by_head(h)} for h in range(3)}
    for h in range(3):
        assert {"unique_lo", "unique_hi_1", "decoys", "all_negative", "flat", "tie_same_tile", "tie3"} <= kinds[h], (name, h, kinds[h])
    assert {"tile_first", "tile_last", "tie_same_wave"} <= kinds[0]
    assert "shared_tile" in kinds[1]
    if name == "big":
        assert NV == 4526 and NVpad // 16 == 283 and V % 16
        assert {"shared_tile", "tie_other_wave", "tie_wave_order", "tie_same_thread"} <= kinds[0]
        assert any(c.kind == "tie3" and {"same_thread", "other_wave"} <= {P.pair_relation(a, b) for a in c.ties for b in c.ties if a < b} for c in plan.cases)
    # tokens without a column (big: text ids from 3000) have zero rows and no case feeds them
    fed = {c.token for c in plan.cases} | {t for t, _ in plan.chain} | {plan.eos_emitter} | set(plan.fillers)
    assert all(P.column(cfg, t) is not None for t in fed)


def test_host_argmax_is_the_selection_rule(geom):
    """sampling.argmax_rows, the greedy pick of the host-driven loop (TraceEngine.decode_stepwise), on every named case under every head - ties in
    one tile, one wave, across waves, flat heads, larger decoys outside the range, all-negative ranges: P.select, the lowest id among equal maxima
    of the head's range.  Rows of -inf give the range's first id; numpy rows and torch rows give the same ids."""
    from trace_amd.sampling import argmax_rows
    name, cfg, T, plan = geom
    V, Tv, Sv, NV, _ = P.dims(cfg)
    toks = [c.token for c in plan.cases] + [t for t, _ in plan.chain]
    rows = T[toks, :NV].astype(np.float32) * np.float32(3.921875)
    for head in range(3):
        lo, hi = P.head_range(cfg, head)
        want = [P.select(T[t], lo, hi) for t in toks]
        assert argmax_rows(rows, [head] * len(toks), V, Tv, Sv) == want, (name, head)
        assert argmax_rows(torch.from_numpy(rows), [head] * len(toks), V, Tv, Sv) == want
    heads = [c.head for c in plan.cases]
    assert argmax_rows(rows[:len(heads)], heads, V, Tv, Sv) == [c.expect for c in plan.cases]         # a batch whose rows differ in head
    assert sum(len(c.ties) > 1 for c in plan.cases) >= 9
    assert argmax_rows(np.full((3, NV), -np.inf, np.float32), [0, 1, 2], V, Tv, Sv) == [P.head_range(cfg, h)[0] for h in range(3)]


def test_ordinary_rows_have_unique_maxima_that_differ_between_neighbours(geom):
    _, cfg, T, plan = geom
    V, Tv, Sv, NV, _ = P.dims(cfg)
    special = {c.token for c in plan.cases} | {t for t, _ in plan.chain} | {plan.eos_emitter}
    toks = [int(t) for t in P.tokens_with_columns(cfg)]
    for h in range(3):
        lo, hi = P.head_range(cfg, h)
        am = {}
        for t in toks:
            if t in special:
                continue
            row = T[t, lo:hi]
            assert (row == row.max()).sum() == 1, (t, h)
            am[t] = lo + int(row.argmax())
        pairs = [(t, t + 1) for t in am if t + 1 in am]
        same = [p for p in pairs if am[p[0]] == am[p[1]]]
        assert len(same) <= 2, same[:5]                        # (the one row moved off the EOS id may meet its neighbour)
    # the chain: free-running from any of its points passes sync, time, score and text in turn
    for i, (t, h) in enumerate(plan.chain):
        nxt = plan.chain[(i + 1) % len(plan.chain)][0]
        assert P.select(T[t], *P.head_range(cfg, h)) == nxt
    ids, n, head = P.restate(T, cfg, plan.chain[0][0], 0, [-1] * 23, -1, 23)
    assert n == 23 and {V, V + 1, V + Tv + 1} <= set(ids) and ids[:11] == ids[11:22]


def test_crafted_weights(geom):
    _, cfg, T, plan = geom
    V, Tv, Sv, NV, _ = P.dims(cfg)
    sd = P.crafted_weights(cfg, T)
    ref = synth.weight_specs(cfg)
    assert set(sd) == {n for n, _, _ in ref} and all(tuple(sd[n].shape) == s for n, s, _ in ref)
    emb = torch.cat([sd["model.embed_tokens.weight"], sd["model.sync_tower.embed_tokens.weight"], sd["model.time_tower.embed_tokens.weight"],
                     sd["model.score_tower.embed_tokens.weight"]]).float()
    W = torch.cat([sd["lm_head.weight"], sd["sync_head.weight"], sd["time_head.weight"], sd["score_head.weight"]]).float()
    toks = torch.from_numpy(P.tokens_with_columns(cfg))
    assert emb.sum() == len(toks) and (emb[toks].sum(-1) == 1).all() and (emb.sum(0) <= 1).all()         # one-hot, no column shared
    assert torch.equal((emb[toks] @ W.t()) * 16, torch.from_numpy(T[toks.numpy(), :NV].astype(np.float32)))
    for t in (0, V - 1, V, V + 1, V + Tv, NV - 1):
        assert torch.equal(P.embedding_row(cfg, t).float(), emb[t])
    assert all(not sd[f"model.layers.{l}.{k}.weight"].any() for l in range(cfg.num_hidden_layers) for k in ("self_attn.o_proj", "mlp.down_proj"))
    assert P.logit_scale(cfg) == 3.921875


# ---- restate == the oracle on the crafted weights (V = 320) ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_small(golden_dir):
    cfg = P.small()
    T, plan = P.build_table(cfg)
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    orc = Oracle(cfg, P.crafted_weights(cfg, T), emulate_bf16=True)
    frames = synth.synth_frames(cfg, 0)
    # the video rows and the prompt's KV do not depend on the row: encode once
    feats = orc.encode_video(frames, E["timestamps"].tolist())
    orc.encode_video = lambda *_: feats
    return cfg, T, plan, E, orc, frames


def _oracle_run(o, start, head, forced, eos, max_new):
    cfg, T, plan, E, orc, frames = o
    ids = torch.from_numpy(E["input_ids"]).clone()
    ids[-1] = start                                               # the prompt's last id (<sync>) replaced by a text id
    return orc.generate(ids, frames, E["timestamps"].tolist(), head=head, max_new_tokens=max_new, eos_token_id=None if eos < 0 else eos,
                        forced_ids=None if forced is None else forced, return_logits=True)


def _check_oracle_logits(o, lg, trace):
    cfg, T = o[0], o[1]
    V, Tv, Sv, NV, _ = P.dims(cfg)
    scale = P.logit_scale(cfg)
    for s in range(lg.shape[0]):
        state, head, _ = trace[s]
        lo, hi = P.head_range(cfg, head)
        want = torch.full((NV,), float("-inf"))
        want[lo:hi] = torch.from_numpy(T[state, lo:hi].astype(np.float32)) * scale
        assert torch.equal(lg[s], want), (s, state, head)


def test_restate_equals_oracle_forced_through_all_heads(oracle_small):
    cfg, T, plan = oracle_small[:3]
    max_new = P.max_new_for(cfg, plan)
    for r in (0, 1):
        start, head, forced = P.batch_rows(cfg, plan, 2, max_new)[r]
        assert start < cfg.vocab_size
        trace = []
        ids, n, final = P.restate(T, cfg, start, head, forced, -1, max_new, trace=trace)
        assert {h for _, h, _ in trace} == {0, 1, 2} and trace[-1][1] == head and n == max_new
        got, lg = _oracle_run(oracle_small, start, head, forced, -1, max_new)
        assert got == ids
        _check_oracle_logits(oracle_small, lg, trace)


def test_restate_equals_oracle_free_running(oracle_small):
    cfg, T, plan = oracle_small[:3]
    trace = []
    ids, n, final = P.restate(T, cfg, plan.chain[1][0], 0, [-1] * 24, -1, 24, trace=trace)
    got, lg = _oracle_run(oracle_small, plan.chain[1][0], 0, None, -1, 24)
    assert got == ids and {h for _, h, _ in trace} == {0, 1, 2}
    _check_oracle_logits(oracle_small, lg, trace)


def test_restate_equals_oracle_row_that_ends_on_eos(oracle_small):
    cfg, T, plan = oracle_small[:3]
    rows, fin = P.eos_rows(cfg, plan, 5, 12)
    for (start, head, forced), at in zip(rows, fin):
        ids, n, _ = P.restate(T, cfg, start, head, forced, plan.eos, 12)
        got, _ = _oracle_run(oracle_small, start, head, forced, plan.eos, 12)
        assert got == ids and n == len(ids) == (12 if at is None else at + 1)
        assert (ids[-1] == plan.eos) == (at is not None) and plan.eos not in ids[:-1]


# ---- the device tests' batches against the mutants --------------------------------------------------------------------------------------------------
def _device_case_lists():
    for name, make in P.GEOMETRIES.items():
        cfg = make()
        T, plan = P.build_table(cfg)
        max_new = P.max_new_for(cfg, plan)
        for B in P.BATCHES[name]:
            yield name, B, cfg, T, P.batch_rows(cfg, plan, B, max_new), -1, max_new
        rows, _ = P.eos_rows(cfg, plan, P.EOS_BATCH, max_new)
        yield name, "eos", cfg, T, rows, plan.eos, max_new


@pytest.fixture(scope="module")
def case_lists():
    return [(name, B, cfg, T, rows, eos, mn, P.restate_batch(T, cfg, rows, eos, mn)) for name, B, cfg, T, rows, eos, mn in _device_case_lists()]


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_the_batches_reject_a_wrong_selector(case_lists, mutant):
    """a selector with one rule broken must give other ids, lengths or heads on the batches tests/test_gpu_token_select.py runs: a mutant that
    no batch catches is a missing case"""
    caught = [(name, B) for name, B, cfg, T, rows, eos, mn, right in case_lists if P.restate_batch(T, cfg, rows, eos, mn, mutant) != right]
    assert caught, mutant
    if mutant not in ("done_keeps_recording", "tiles_from_256_ignored", "first_wave_only"):
        # the rules that do not depend on the geometry or on EOS: every batch of both geometries catches them, the single row included
        assert len(caught) == len(case_lists), (mutant, sorted(set((n, b) for n, b, *_ in case_lists) - set(caught)))
    if mutant in ("tiles_from_256_ignored", "first_wave_only"):
        assert {("big", B) for B in P.BATCHES["big"]} <= set(caught)
    if mutant == "done_keeps_recording":
        assert {("small", "eos"), ("big", "eos")} <= set(caught)


def test_every_step_has_a_row_in_every_head_and_the_edge_rows_pass_every_case(case_lists):
    for name, B, cfg, T, rows, eos, mn, _ in case_lists:
        if B == "eos" or B < 16:
            continue
        plan = P.build_table(cfg)[1]
        traces = []
        for t, h, f in rows:
            tr = []
            P.restate(T, cfg, t, h, f, eos, mn, trace=tr)
            traces.append(tr)
        for s in range(mn):
            assert {tr[s][1] for tr in traces} == {0, 1, 2}, (name, B, s)
        assert len({h for _, h, _ in rows}) == 3
        for r in set(P.SPECIAL_ROWS + (B - 1,)):
            if r < B:
                seen = {(state, head) for state, head, _ in traces[r]}
                assert all((c.token, c.head) in seen for c in plan.cases), (name, B, r)
        free = [r for r, (_, _, f) in enumerate(rows) if f[0] < 0]
        assert free and all({h for _, h, _ in traces[r]} == {0, 1, 2} for r in free)


def test_eos_rows_finish_where_planned(geom):
    _, cfg, T, plan = geom
    mn = P.max_new_for(cfg, plan)
    rows, fin = P.eos_rows(cfg, plan, P.EOS_BATCH, mn)
    ids, lens, heads = P.restate_batch(T, cfg, rows, plan.eos, mn)
    assert fin == [0, 1, mn // 2, mn - 1, None]
    for r, at in enumerate(fin):
        assert lens[r] == (mn if at is None else at + 1) and (ids[r][-1] == plan.eos) == (at is not None)
    assert heads[1] == 1                                          # fed <sync> after it finished: the head still switches
    assert all(n == mn for n in lens[len(fin):])                  # rows that stay alive have length max_new
    free_ids, free_lens, free_heads = P.restate_batch(T, cfg, rows, -1, mn)
    assert free_heads == heads and all(a == b[:len(a)] for a, b in zip(ids, free_ids))
