"""Per-row generation parameters: the tail of the decode step restated with every row's own (sampling, logits processors, max_new), on the exact
decoders of tests/token_select_probes.py and tests/constraint_probes.py — admit_probes.restate_origins generalised, and equal to it under uniform
params (tests/test_row_params_cpu.py holds the two together on the admission scenarios).

The three per-row arrays of the device sit beside row_id / step0: entry i belongs to the row at POSITION i of the batch.  A retire moves the entries
with the rows, an admission writes the new rows' entries at [B, B + n).  MISSES names the near misses of that bookkeeping and of the per-row
selection; `miss=` makes the restatement commit one, and every scenario names the misses it must tell (`tells`): the CPU test asserts that it does.

The P table has flat heads and heads with one dominant id, nothing between; soft_table adds states whose head holds a few ids a unit or two apart (one
unit = logit_scale = 3.92 in the logits), so that temperature, top_k, top_p and the seed all decide what a sampled row draws.

Nothing here imports the HIP library; everything runs on the CPU."""
import dataclasses
from typing import Optional, Sequence

import numpy as np

import constraint_probes as CP
import token_select_probes as P
from trace_amd.sampling import Constraints, LogitsParams, RowParams, SamplingParams, philox_uniform, process_row_ref, sample_row_ref, token_logprob_ref

MISSES = ("row0_sample", "row0_seed", "row0_processors", "batch_max_new", "greedy_sampled", "sampled_greedy", "stale_after_retire", "admit_entry_i",
          "highest_id_tie")
SOFT = (3, 4, 6)                      # ids per level of a soft state: 3 at the top value, 4 one unit below, 6 two units below


# ---- the table: P's, plus soft states ---------------------------------------------------------------------------------------------------------
def soft_table(cfg):
    """(T, plan, soft): P.build_table's table with three more states, soft[h] read under head h, whose head range holds SOFT[0] ids at 8, SOFT[1]
    at 7, SOFT[2] at 6 and -40 elsewhere; outside the range the row keeps what it had (the decoys of a neighbour head stay out of reach of the mask)."""
    T, plan = P.build_table(cfg)
    T = T.copy()
    V = cfg.vocab_size
    used = {c.token for c in plan.cases} | {t for t, _ in plan.chain} | {plan.eos, plan.eos_emitter} | set(plan.fillers)
    free = [t for t in range(200, V) if t not in used]
    soft = []
    for h in range(3):
        t = free[7 * h + 1]
        lo, hi = P.head_range(cfg, h)
        n = hi - lo
        T[t, lo:hi] = -40
        ids, k = [], 0
        for level, count in zip((8, 7, 6), SOFT):
            for _ in range(count):
                i = lo + (5 + 11 * k) % n                     # spread over the range, not neighbours
                while i in ids:
                    i = lo + (i - lo + 1) % n
                ids.append(i)
                T[t, i] = level
                k += 1
        assert plan.eos not in ids, "a soft state must not emit EOS (the rows held in one are fed the state itself, so a switch token it emits switches nothing)"
        soft.append(t)
    return T, plan, soft


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def resolved(p: Optional[RowParams], max_new) -> RowParams:
    return (p or RowParams()).over(None, None, max_new)


def _draw(row, lo, hi, sp: SamplingParams, step, row_id):
    u = philox_uniform(sp.seed, step, row_id)
    return lo + sample_row_ref(row[lo:hi], sp.temperature, sp.top_k, sp.top_p, u, None, *sp.warpers)


def restate_rows(table, cfg, rows, origins, eos, max_new, scale, params: Sequence[Optional[RowParams]], cons: Optional[Constraints] = None,
                 row_ids: Optional[Sequence[int]] = None, miss: Optional[str] = None, retire=None, extra_steps: int = 3, logprobs: bool = False):
    """([ids], [length], [head after the row's last own step], [logprobs float32 [max_new]]) of rows [(start token, head, forced[max_new] or None)]
    listed in batch order (origins non-decreasing: the rows of the begin, then every admission's), row b under params[b] (None fields: greedy, no
    processors, max_new).  max_new is the batch's: the stride, and the bound of every row's own.  retire = (g, keep): before shared step g the
    batch shrinks to the rows keep (indices into `rows`, increasing); the others stop there.  A row is stepped like the batch it sits in: past
    its own bound it records nothing.  miss: one of MISSES."""
    V, Tv, Sv, NV, _ = P.dims(cfg)
    assert miss is None or miss in MISSES
    assert list(origins) == sorted(origins)
    cons = cons or Constraints()
    no_begin = Constraints(cons.stop_sequences, cons.bad_words_ids, cons.suppress_tokens, ())
    only_begin = Constraints((), (), (), cons.begin_suppress_tokens)
    B = len(rows)
    params = [resolved(p, max_new) for p in params]
    row_ids = list(range(B)) if row_ids is None else list(row_ids)
    where = list(range(B))                      # position of row b in the batch's arrays (None: retired)
    entry = list(range(B))                      # entry[position] = whose RowParams the per-row arrays hold there
    state = [int(t) for t, _, _ in rows]
    head = [int(h) for _, h, _ in rows]
    forced = [list(f) if f is not None else [-1] * max_new for _, _, f in rows]
    done, out_len = [False] * B, [0] * B
    out_ids = [[0] * max_new for _ in range(B)]
    lps = np.zeros((B, max_new), np.float32)
    head_at = [None] * B

    def own_params(b):
        pos = where[b]
        if miss == "admit_entry_i" and origins[b] > 0:
            pos = [x for x in range(B) if origins[x] == origins[b]].index(b)           # entry i of the admission's list, not B + i
        p = params[entry[pos]]
        first = params[entry[0]]
        sp, lp, mx = p.sampling, p.logits, p.max_new_tokens
        greedy = sp is None or sp.greedy
        if miss == "row0_sample":
            f = first.sampling
            sp = None if f is None or f.greedy else dataclasses.replace(f, seed=0 if greedy else sp.seed)
        elif miss == "row0_seed" and not greedy:
            f = first.sampling
            sp = dataclasses.replace(sp, seed=0 if f is None or f.greedy else f.seed)
        elif miss == "greedy_sampled" and greedy:
            sp = SamplingParams(1.0, 0, 1.0, seed=0)
        elif miss == "sampled_greedy":
            sp = None
        if miss == "row0_processors":
            lp = first.logits
        if miss == "batch_max_new":
            mx = max_new
        return sp, lp or LogitsParams(), mx

    last = max(o + resolved(p, max_new).max_new_tokens for o, p in zip(origins, params))
    for g in range(last + extra_steps):
        if retire is not None and g == retire[0]:
            keep = list(retire[1])
            assert keep == sorted(keep) and all(where[b] is not None for b in keep)
            if miss != "stale_after_retire":
                entry = [entry[where[b]] for b in keep] + entry[len(keep):]
            where = [keep.index(b) if b in keep else None for b in range(B)]
        for b in range(B):
            if origins[b] > g or where[b] is None:
                continue
            local = g - origins[b]
            sp, lp, own = own_params(b)
            lo, hi = P.head_range(cfg, head[b])
            raw = (table[state[b], :NV].astype(np.float32) * np.float32(scale)).astype(np.float32)
            hist = out_ids[b][:max(0, min(out_len[b], max_new))]
            row = process_row_ref(raw, hist, lo, hi, lp, local, eos)
            row = CP.constrain_row(row, hist, lo, hi, no_begin, local, lp.min_new_tokens)
            row = CP.constrain_row(row, hist, lo, hi, only_begin, local, 0)
            if sp is None or sp.greedy:
                tok = P.select(row, lo, hi, "highest_id_wins_tie" if miss == "highest_id_tie" else None)
            else:
                tok = _draw(row, lo, hi, sp, local, row_ids[b])
            feed = tok
            if local < own and forced[b][local] >= 0:
                feed = forced[b][local]
            s_len = 0
            if not done[b] and local < own:
                out_ids[b][local] = tok
                out_len[b] = local + 1
                if eos >= 0 and tok == eos:
                    done[b] = True
                s_len = local + 1
                if logprobs:
                    masked = np.full(NV, -np.inf, np.float32)
                    masked[lo:hi] = raw[lo:hi]
                    lps[b, local] = token_logprob_ref(masked[lo:hi], tok - lo) if lo <= tok < hi else -np.inf
            head[b] = {V: 1, V + 1: 2, V + Tv + 1: 0}.get(feed, head[b])
            state[b] = feed
            if s_len > 0 and CP.stop_match(out_ids[b][:s_len], cons):
                done[b] = True
            if local == own - 1:
                head_at[b] = head[b]
    return [out_ids[b][:out_len[b]] for b in range(B)], list(out_len), head_at, lps


def alone(table, cfg, row, eos, max_new, scale, params: Optional[RowParams], cons=None, row_id=0, logprobs=False):
    """one row decoded alone from the counter's zero under its own params: (ids, length, head, logprobs [max_new])"""
    o = restate_rows(table, cfg, [row], [0], eos, max_new, scale, [params], cons, [row_id], extra_steps=0, logprobs=logprobs)
    return o[0][0], o[1][0], o[2][0], o[3][0]


# ---- the params ---------------------------------------------------------------------------------------------------------------------------------------
def S(temperature, top_k, top_p, seed, **kw):
    return SamplingParams(temperature, top_k, top_p, seed=seed, **kw)


SEED = 20261021
COOL = dict(temperature=0.7, top_k=3, top_p=0.9)                          # the issue's two sampled settings and one with all four warpers armed
WARM = dict(temperature=1.3, top_k=0, top_p=1.0)
WARPED = dict(temperature=1.0, top_k=8, top_p=0.95, min_p=0.01, typical_p=0.9, epsilon_cutoff=0.003, eta_cutoff=0.004)


def stay(token, max_new):
    """forced ids that keep a row in one state"""
    return [token] * max_new


def ending_row(plan, r, at, max_new):
    """a teacher-forced row under head 0 that emits EOS at its own step `at` (test_gpu_retire.ending_row)"""
    st = [plan.fillers[(3 * r + i) % len(plan.fillers)] for i in range(max_new + 1)]
    if at is not None:
        st[at] = plan.eos_emitter
    return (st[0], 0, st[1:])


# ---- the scenarios the GPU tests run: dict(rows, origins, eos, params, row_ids, retire, tells) ---------------------------------------------------
def mixed_scenario(cfg, plan, soft, max_new):
    """eight rows begun together, each with params of its own: a greedy teacher-forced tour over the tie / decoy states, a greedy free-running row
    across the head switches, three sampled rows held in soft states (one under the time head), two greedy tour rows that start under the time and
    the score head, a row that emits EOS at step 6"""
    tour = [r for r in P.batch_rows(cfg, plan, 32, max_new) if r[2][0] >= 0]                   # the teacher-forced ones
    timed, scored = next(r for r in tour if r[1] == 1), next(r for r in tour if r[1] == 2)
    rows = [tour[0], (plan.chain[0][0], plan.chain[0][1], None), (soft[0], 0, stay(soft[0], max_new)), (soft[1], 1, stay(soft[1], max_new)),
            (soft[0], 0, stay(soft[0], max_new)), timed, scored, ending_row(plan, 7, 6, max_new)]
    params = [RowParams(), RowParams(), RowParams(S(seed=SEED + 2, **COOL)), RowParams(S(seed=SEED + 3, **WARM)), RowParams(S(seed=SEED + 4, **WARPED)),
              RowParams(), RowParams(), RowParams()]
    return dict(rows=rows, origins=[0] * 8, eos=plan.eos, params=params, row_ids=None, retire=None,
                tells=("greedy_sampled", "sampled_greedy", "highest_id_tie"))


def sampled_first_scenario(cfg, plan, soft, max_new):
    """four rows in one soft state: row 0 sampled COOL, row 1 WARM, row 2 COOL under another seed, row 3 greedy — what differs from row 0 is the
    params (row 1), the seed alone (row 2), sampling at all (row 3)"""
    rows = [(soft[0], 0, stay(soft[0], max_new))] * 4
    params = [RowParams(S(seed=SEED, **COOL)), RowParams(S(seed=SEED, **WARM)), RowParams(S(seed=SEED + 9, **COOL)), RowParams()]
    return dict(rows=rows, origins=[0] * 4, eos=-1, params=params, row_ids=None, retire=None, tells=("row0_sample", "row0_seed", "greedy_sampled"))


MAX_NEWS = (1, 2, 5, 41)


def max_new_scenario(cfg, plan, soft, max_new):
    """per-row max_new 1, 2, 5 and the batch's in one batch, twice: free-running chain rows (greedy) and soft-state rows (sampled)"""
    rows, params = [], []
    for i, m in enumerate(MAX_NEWS):
        t, h = plan.chain[(3 * i) % len(plan.chain)]
        rows.append((t, h, None))
        params.append(RowParams(max_new_tokens=min(m, max_new)))
    for i, m in enumerate(MAX_NEWS):
        rows.append((soft[0], 0, stay(soft[0], max_new)))
        params.append(RowParams(S(seed=SEED + 20 + i, **WARM), max_new_tokens=min(m, max_new)))
    return dict(rows=rows, origins=[0] * 8, eos=-1, params=params, row_ids=None, retire=None, tells=("batch_max_new",))


def retire_scenario(cfg, plan, soft, max_new, chunk=4):
    """six rows with distinct params; after one chunk the batch shrinks to rows 1, 3, 4: every kept row lands on a position whose old entry differs"""
    rows = [ending_row(plan, 0, 2, max_new), (soft[0], 0, stay(soft[0], max_new)), ending_row(plan, 2, 0, max_new), (soft[0], 0, stay(soft[0], max_new)),
            (plan.chain[0][0], plan.chain[0][1], None), ending_row(plan, 5, 3, max_new)]
    params = [RowParams(), RowParams(S(seed=SEED + 31, **COOL)), RowParams(S(seed=SEED + 32, **WARM)), RowParams(S(seed=SEED + 33, **WARM)),
              RowParams(max_new_tokens=17), RowParams(S(seed=SEED + 35, **WARPED))]
    return dict(rows=rows, origins=[0] * 6, eos=plan.eos, params=params, row_ids=None, retire=(1 + chunk, [1, 3, 4]), tells=("stale_after_retire",))


def admit_scenario(cfg, plan, soft, max_new, chunk=4):
    """three rows begun, three admitted after one chunk with other params and Philox row indices 6, 2, 9"""
    rows = [(soft[0], 0, stay(soft[0], max_new)), (plan.chain[0][0], plan.chain[0][1], None), (soft[0], 0, stay(soft[0], max_new)),
            (soft[0], 0, stay(soft[0], max_new)), (soft[0], 0, stay(soft[0], max_new)), (plan.chain[4][0], plan.chain[4][1], None)]
    params = [RowParams(S(seed=SEED + 41, **COOL)), RowParams(), RowParams(S(seed=SEED + 43, **WARM)),
              RowParams(), RowParams(S(seed=SEED + 45, **WARPED)), RowParams(S(seed=SEED + 46, **WARM), max_new_tokens=9)]
    return dict(rows=rows, origins=[0, 0, 0, chunk, chunk, chunk], eos=-1, params=params, row_ids=[0, 1, 2, 6, 2, 9], retire=None,
                tells=("admit_entry_i",))


def processor_scenario(cfg, cplan):
    """the CP table, free-running rows (admit_probes.processor_scenarios' states) whose processors differ by row, under a batch-wide stop sequence"""
    b = cplan.base
    c0, c1, c2 = b.cycle
    rows = [(c0, 0, None), (c0, 0, None), (c2, 0, None), (b.eos_emitter, 0, None), (b.eos_back, 0, None), (b.tour[0][0], 0, None)]
    params = [RowParams(), RowParams(logits=LogitsParams(no_repeat_ngram_size=2)), RowParams(logits=LogitsParams(repetition_penalty=1.5)),
              RowParams(logits=LogitsParams(min_new_tokens=3)), RowParams(logits=LogitsParams(min_new_tokens=1)),
              RowParams(logits=LogitsParams(repetition_penalty=2.0, no_repeat_ngram_size=3))]
    return dict(rows=rows, origins=[0] * 6, eos=b.eos, params=params, row_ids=None, retire=None, cons=Constraints(stop_sequences=[[c1, c2, c0]]),
                tells=("row0_processors",))


def run(table, cfg, sc, max_new, scale, miss=None, logprobs=False):
    return restate_rows(table, cfg, sc["rows"], sc["origins"], sc["eos"], max_new, scale, sc["params"], sc.get("cons"), sc["row_ids"], miss, sc["retire"],
                        logprobs=logprobs)


# ---- the queue -------------------------------------------------------------------------------------------------------------------------------------------
QUEUE_SETS = 4
QUEUE_MAX_NEWS = (3, 12, 41)


def queue_params(i, max_new):
    """request i's RowParams: the sampling cycles through four sets (greedy, COOL, WARM, WARPED; a seed per request), max_new_tokens through 3, 12, 41"""
    sp = [None, S(seed=SEED + 100 + i, **COOL), S(seed=SEED + 100 + i, **WARM), S(seed=SEED + 100 + i, **WARPED)][i % QUEUE_SETS]
    return RowParams(sp, None, min(QUEUE_MAX_NEWS[i % len(QUEUE_MAX_NEWS)], max_new))


def queue_row(plan, soft, r, at, max_new):
    """request r's row: a greedy request is ending_row; a sampled one is held in the soft state of head 0 and fed the EOS emitter at its own step
    `at` (whose head holds one dominant id: the draw is EOS under every setting here)"""
    if r % QUEUE_SETS == 0:
        return ending_row(plan, r, at, max_new)
    st = [soft[0]] * (max_new + 1)
    if at is not None:
        st[at] = plan.eos_emitter
    return (st[0], 0, st[1:])


def queue_schedule(lengths, bounds, cap, chunk, retire_fraction=8, admit_fraction=8):
    """admit_probes.queue_schedule with a bound per request: request r is finished once it has recorded lengths[r] ids (its EOS, or bounds[r] of them),
    and the chunk is as long as the largest remainder of a row: (rows x steps, [batch size of every chunk stepped], admits, retires, batches begun)"""
    from trace_amd.admit import admit_plan
    from trace_amd.retire import retire_plan
    todo = list(range(len(lengths)))
    row_steps, sizes, admits, retires, begun = 0, [], 0, 0, 0
    while todo:
        rows, todo = todo[:cap], todo[cap:]
        own = [1] * len(rows)
        begun += 1
        while True:
            while True:
                fin = [o >= lengths[r] for r, o in zip(rows, own)]
                live = fin.count(False)
                if live == 0:
                    break
                if retire_plan(len(rows), live, retire_fraction):
                    rows, own = [r for r, f in zip(rows, fin) if not f], [o for o, f in zip(own, fin) if not f]
                    retires += 1
                k = admit_plan(len(rows), cap, len(todo), cap - len(rows), admit_fraction)
                if not k:
                    break
                rows, own, todo = rows + todo[:k], own + [1] * k, todo[k:]
                admits += 1
            if live == 0:
                break
            n = min(chunk, max(bounds[r] - o for r, o in zip(rows, own)))
            row_steps += n * len(rows)
            sizes.append(len(rows))
            own = [o + n for o in own]
    return row_steps, sizes, admits, retires, begun
