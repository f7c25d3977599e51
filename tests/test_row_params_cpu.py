"""Per-row generation parameters, on the CPU: the restatement the GPU tests compare against (tests/row_params_probes.py) is anchored to
admit_probes.restate_origins, every scenario tells the near misses it names, and the host side — RowParams.check, the request shapes of
generate_queue(per_request=), the trace_row_params struct, the queue's schedule with a bound per row, the schedule models against decode_loop — is checked without the library's GPU half."""
import os
import re

import numpy as np
import pytest

import admit_probes as AP
import constraint_probes as CP
import row_params_probes as RP
import token_select_probes as P
from trace_amd.sampling import LogitsParams, RowParams, SamplingParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4


@pytest.fixture(scope="module")
def world():
    cfg = P.small()
    T, plan, soft = RP.soft_table(cfg)
    return cfg, T, plan, soft, P.max_new_for(cfg, plan), P.logit_scale(cfg)


@pytest.fixture(scope="module")
def cworld():
    cfg = CP.GEOMETRIES["small"]()
    T, cplan = CP.build_table(cfg)
    return cfg, T, cplan, CP.MAX_NEW, P.logit_scale(cfg)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_soft_states_are_neither_flat_nor_one_hot(world):
    cfg, T, plan, soft, mn, scale = world
    T0, _ = P.build_table(cfg)
    changed = np.nonzero((T != T0).any(1))[0].tolist()
    assert sorted(changed) == sorted(soft)                      # every state the retire / admit tests run is P's own
    for h, t in enumerate(soft):
        lo, hi = P.head_range(cfg, h)
        x = T[t, lo:hi].astype(np.float32) * np.float32(scale)
        p = np.exp(x - x.max())
        p /= p.sum()
        top = np.sort(p)[::-1]
        assert (T[t, lo:hi] == 8).sum() == RP.SOFT[0] and 0.2 < top[0] < 0.5 and top[RP.SOFT[0]] > 1e-3, (h, top[:5])


def test_uniform_params_equal_restate_origins(world, cworld):
    """with the same params in every row the generalisation is admit_probes.restate_origins, on its own scenarios"""
    cfg, T, plan, soft, mn, scale = world
    sc = AP.plain_scenario(cfg, plan, mn)
    want = AP.restate_origins(T, cfg, sc["rows"], AP.ORIGINS, sc["eos"], mn, scale)
    got = RP.restate_rows(T, cfg, sc["rows"], AP.ORIGINS, sc["eos"], mn, scale, [None] * 4)
    assert got[:3] == want
    sc = AP.sampled_scenario(cfg, plan, mn)
    want = AP.restate_origins(T, cfg, sc["rows"], AP.ORIGINS, sc["eos"], mn, scale, sampling=sc["sampling"], row_ids=sc["row_ids"])
    t, k, p, seed = sc["sampling"]
    got = RP.restate_rows(T, cfg, sc["rows"], AP.ORIGINS, sc["eos"], mn, scale, [RowParams(SamplingParams(t, k, p, seed=seed))] * 4, row_ids=sc["row_ids"])
    assert got[:3] == want
    ccfg, CT, cplan, cmn, cscale = cworld
    for sc in AP.processor_scenarios(ccfg, cplan):
        want = AP.restate_origins(CT, ccfg, sc["rows"], AP.ORIGINS, sc["eos"], cmn, cscale, sc["params"], sc["cons"])
        got = RP.restate_rows(CT, ccfg, sc["rows"], AP.ORIGINS, sc["eos"], cmn, cscale, [RowParams(logits=sc["params"])] * 4, sc["cons"])
        assert got[:3] == want, sc["name"]


def _scenarios(world, cworld):
    cfg, T, plan, soft, mn, scale = world
    ccfg, CT, cplan, cmn, cscale = cworld
    out = {f.__name__: (T, cfg, f(cfg, plan, soft, mn), mn, scale)
           for f in (RP.mixed_scenario, RP.sampled_first_scenario, RP.max_new_scenario, RP.retire_scenario, RP.admit_scenario)}
    out["processor_scenario"] = (CT, ccfg, RP.processor_scenario(ccfg, cplan), cmn, cscale)
    return out


def test_every_near_miss_is_told_by_the_scenario_that_names_it(world, cworld):
    named = set()
    for name, (T, cfg, sc, mn, scale) in _scenarios(world, cworld).items():
        right = RP.run(T, cfg, sc, mn, scale)
        for miss in RP.MISSES:
            wrong = RP.run(T, cfg, sc, mn, scale, miss=miss)
            if miss in sc["tells"]:
                assert wrong[0] != right[0], f"{name} does not tell {miss}"
                named.add(miss)
    assert named == set(RP.MISSES)


def test_scenarios_hold_what_they_claim(world):
    cfg, T, plan, soft, mn, scale = world
    sc = RP.mixed_scenario(cfg, plan, soft, mn)
    ids, lens, heads, _ = RP.run(T, cfg, sc, mn, scale)
    assert lens[7] == 7 and ids[7][-1] == plan.eos and lens[:7] == [mn] * 7
    assert len(set(ids[1])) > 6 and heads[1] is not None                                         # the free-running row tours the chain
    for r in (2, 3, 4):
        assert 1 < len(set(ids[r])) <= sum(RP.SOFT), (r, sorted(set(ids[r])))                     # a sampled row draws several ids, all of its soft state
    sc = RP.max_new_scenario(cfg, plan, soft, mn)
    ids, lens, _, lps = RP.run(T, cfg, sc, mn, scale, logprobs=True)
    assert lens == [1, 2, 5, mn] * 2
    assert all((lps[r, lens[r]:] == 0).all() and (lps[r, :lens[r]] <= 0).all() for r in range(8)) and (lps[4:, 0] < 0).all()
    every = dict(sc, params=[RowParams(p.sampling) for p in sc["params"]])
    full = RP.run(T, cfg, every, mn, scale)
    assert all(ids[r] == full[0][r][:lens[r]] for r in range(8))                                  # a short row is a prefix of the row at the batch's bound
    sc = RP.retire_scenario(cfg, plan, soft, mn, CHUNK)
    ids, lens, _, _ = RP.run(T, cfg, sc, mn, scale)
    whole = RP.run(T, cfg, dict(sc, retire=None), mn, scale)
    assert [ids[r] for r in (1, 3, 4)] == [whole[0][r] for r in (1, 3, 4)] and lens[4] == 17
    assert [lens[r] for r in (0, 2, 5)] == [3, 1, 4]                                              # the rows that leave have ended by then
    sc = RP.admit_scenario(cfg, plan, soft, mn, CHUNK)
    ids, lens, _, _ = RP.run(T, cfg, sc, mn, scale)
    for r in range(6):
        assert ids[r] == RP.alone(T, cfg, sc["rows"][r], sc["eos"], mn, scale, sc["params"][r], row_id=sc["row_ids"][r])[0], r
    assert lens == [mn, mn, mn, mn, mn, 9]


# ---------------------------------------------------------------------------------------------------------------- host checks
def test_row_params_check():
    assert RowParams().check(41) is not None
    RowParams(SamplingParams(0.7, 50, 0.9, seed=3), LogitsParams(1.2, 2, 1), 7).check(41)
    RowParams(SamplingParams(0.0, 5000, 1.0)).check()                                              # greedy: the rest is not read
    with pytest.raises(ValueError, match="device sampler"):
        RowParams(SamplingParams(1.0, 2000, 1.0)).check()
    with pytest.raises(ValueError, match="device sampler"):
        RowParams(SamplingParams(1.0, 0, 0.9)).check()
    for bad in (0, -3, True, 2.5):
        with pytest.raises(ValueError, match="max_new_tokens"):
            RowParams(max_new_tokens=bad).check()
    with pytest.raises(ValueError, match="at most the batch's"):
        RowParams(max_new_tokens=42).check(41)
    with pytest.raises(ValueError, match="SamplingParams"):
        RowParams(sampling=(0.7, 3, 0.9)).check()
    with pytest.raises(ValueError, match="LogitsParams"):
        RowParams(logits=1.2).check()
    with pytest.raises(ValueError):
        LogitsParams(no_repeat_ngram_size=65)
    full = RowParams(max_new_tokens=5).over(SamplingParams(0.5, 4, 1.0, seed=1), LogitsParams(1.1), 41)
    assert full.sampling.top_k == 4 and full.logits.repetition_penalty == 1.1 and full.max_new_tokens == 5 and full.armed
    assert RowParams().over(None, None, 41) == RowParams(None, None, 41) and not RowParams().armed


def _queue(requests, **kw):
    """the request checks of generate_queue / decode_queue (max_new_tokens 41, a vocabulary of 400) on requests of which one is bad: a list or a tuple
    has to fail at the call itself, before anything is pulled; an iterator passes the call and fails when the bad request is pulled"""
    from trace_amd.decode_loop import checked_requests
    pulled = checked_requests(requests, 41, 400, kw.pop("sampling", None), kw.pop("logits", None), None, **kw)
    assert not isinstance(requests, (list, tuple)), "a list with a bad request passed the call"
    return list(pulled)


def test_per_request_request_shapes():
    six = (None, None, [1], 0, None, RowParams(max_new_tokens=3))
    with pytest.raises(ValueError, match="per_request=True"):
        _queue([six])                                                           # a list: before any work
    with pytest.raises(ValueError, match="per_request=True"):
        _queue(iter([six]))                                                     # an iterator: when pulled (the first request here)
    with pytest.raises(ValueError, match="a request is"):
        _queue([six + (1,)], per_request=True)
    with pytest.raises(ValueError, match="at most the batch's"):
        _queue([six[:5] + (RowParams(max_new_tokens=42),)], per_request=True)
    with pytest.raises(ValueError, match="device sampler"):
        _queue([six[:5] + (RowParams(SamplingParams(1.0, 0, 0.5)),)], per_request=True)
    with pytest.raises(ValueError, match="forced"):                            # forced ids on a row whose own processors are armed
        _queue([(None, None, [1], 0, [5] * 41, RowParams(logits=LogitsParams(1.3)))], per_request=True)
    with pytest.raises(ValueError, match="forced"):                            # ... or armed through the call's fallback
        _queue([(None, None, [1], 0, [5] * 41, RowParams())], per_request=True, logits=LogitsParams(1.3))


def test_a_list_is_checked_whole_before_any_work_and_an_iterator_as_it_is_pulled():
    from trace_amd.decode_loop import checked_requests
    good, bad = (None, None, [1], 0), (None, None, [1], 0, None, RowParams(max_new_tokens=3))
    for seq in ([good, good, bad], (good, good, bad)):
        with pytest.raises(ValueError, match="per_request=True"):
            checked_requests(seq, 41, 400)                                      # the bad request is the last one; nothing has been pulled
    pulled = checked_requests(iter([good, good, bad]), 41, 400)                # an iterator: the call itself looks at nothing
    assert next(pulled) == good + (None, None) and next(pulled) == good + (None, None)
    with pytest.raises(ValueError, match="per_request=True"):
        next(pulled)
    assert list(checked_requests([good, good], 41, 400)) == [good + (None, None)] * 2


def test_row_params_struct_matches_header():
    import ctypes as C
    from trace_amd._lib import SIGNATURES, TraceRowParamsC, TraceSamplingC
    hdr = open(os.path.join(ROOT, "include", "trace_hip.h")).read()
    body = hdr[hdr.index("typedef struct trace_row_params {"):hdr.index("} trace_row_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"(?:int32_t|float|trace_sampling)\s+([^;]+);", body):
        names += [n.strip() for n in decl.split(",")]
    assert names == [f[0] for f in TraceRowParamsC._fields_]
    assert dict(TraceRowParamsC._fields_)["sampling"] is TraceSamplingC
    assert C.sizeof(TraceRowParamsC) == 64 and TraceRowParamsC.sampling.offset == 8 and TraceRowParamsC.max_new.offset == 60
    assert len(SIGNATURES["trace_decode_admit_ex"][1]) == len(SIGNATURES["trace_decode_admit"][1]) + 1
    assert "#define TRACE_ABI_VERSION 4" in hdr


def test_queue_schedule_with_a_bound_per_row(world):
    cfg, T, plan, soft, mn, scale = world
    ends = AP.QUEUE_ENDS
    uniform = [mn if e is None else e + 1 for e in ends]
    assert RP.queue_schedule(uniform, [mn] * 24, 8, CHUNK) == AP.queue_schedule(uniform, mn, 8, CHUNK)      # one bound: the schedule the parent has
    bounds = [RP.queue_params(i, mn).max_new_tokens for i in range(24)]
    assert set(bounds) == {3, 12, 41} and len({(i % RP.QUEUE_SETS, b) for i, b in enumerate(bounds)}) == 12
    lengths = [min(b, mn if e is None else e + 1) for e, b in zip(ends, bounds)]
    row_steps, sizes, admits, retires, begun = RP.queue_schedule(lengths, bounds, 8, CHUNK)
    assert row_steps < AP.queue_schedule(uniform, mn, 8, CHUNK)[0] and max(sizes) <= 8 and admits >= 2 and retires >= 2 and begun >= 1
    # every request gets the steps it needs: rows x steps covers the ids recorded after every row's token 0
    assert row_steps >= sum(n - 1 for n in lengths)


def test_the_schedule_models_are_the_loop_that_ships(world):
    """the schedules the GPU tests take as oracles (restated from lengths alone) against decode_loop itself on the scripted device"""
    from decode_loop_probes import run, script_with_ends
    from trace_amd.decode_loop import DECODE, QUEUE
    mn, ends = world[4], AP.QUEUE_ENDS
    script = script_with_ends(ends, mn)
    shape = lambda book, dev: (dev.row_steps, dev.sizes, dev.admits, dev.retires, dev.begun)
    uniform = [mn if e is None else e + 1 for e in ends]
    book, dev = run(script, mn, CHUNK, 8, QUEUE, logprobs=False)
    assert shape(book, dev) == AP.queue_schedule(uniform, mn, 8, CHUNK) and (book.admits, book.retires) == (dev.admits, dev.retires)
    bounds = [RP.queue_params(i, mn).max_new_tokens for i in range(24)]
    lengths = [min(b, n) for b, n in zip(bounds, uniform)]
    book, dev = run(script, mn, CHUNK, 8, QUEUE, logprobs=False, bounds=bounds)
    assert shape(book, dev) == RP.queue_schedule(lengths, bounds, 8, CHUNK)
    assert [len(o[0]) for o in book.results()] == lengths
    fixed = sum(run(script[i:i + 8], mn, CHUNK, 8, DECODE, logprobs=False)[1].row_steps for i in range(0, 24, 8))
    assert fixed == AP.fixed_schedule(uniform, [e is not None for e in ends], mn, 8, CHUNK)
