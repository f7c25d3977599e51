"""Admission probes: the tail of the decode step restated over a SHARED step counter with a per-row origin, as the kernels have it
(select_next_kernel, logits_process_kernel, the log-probability launch: trace_amd/csrc/select.h, logits.hip, sample.hip), on the exact decoders of
tests/token_select_probes.py and tests/constraint_probes.py.

Row b joins the batch when the shared counter is origins[b]; from then on every step of the batch is a step of the row, and everything that belongs
to the row counts local = shared - origins[b].  USES names the places where a kernel takes a step number for something of the row's; `shared=` makes
the restatement take the shared counter there instead: the near misses that tests/test_admit_host.py holds the scenarios of the GPU tests up against.

Nothing here imports the HIP library; everything runs on the CPU."""
from typing import Optional, Sequence

import numpy as np

import constraint_probes as CP
import token_select_probes as P
from trace_amd.sampling import Constraints, LogitsParams, philox_uniform, process_row_ref, sample_row_ref

USES = ("index", "out_len", "guard", "philox", "min_new", "begin_suppress", "stop_len")
ORIGINS = (0, 0, 5, 9)


def restate_origins(table, cfg, rows, origins, eos, max_new, scale, params: Optional[LogitsParams] = None, cons: Optional[Constraints] = None,
                    sampling=None, row_ids: Optional[Sequence[int]] = None, shared: Sequence[str] = (), extra_steps: int = 3):
    """([ids], [length], [head after the row's own step max_new - 1]) of rows [(start token, head, forced[max_new] or None)].  The shared counter runs
    until the last row has had max_new steps of its own and extra_steps more: rows that joined earlier are stepped past their max_new, as a running
    batch steps them.  sampling: (temperature, top_k, top_p, seed); row_ids: the Philox row index of each row (default: its position)."""
    V, Tv, Sv, NV, _ = P.dims(cfg)
    assert all(u in USES for u in shared)
    params = params or LogitsParams()
    cons = cons or Constraints()
    no_begin = Constraints(cons.stop_sequences, cons.bad_words_ids, cons.suppress_tokens, ())
    only_begin = Constraints((), (), (), cons.begin_suppress_tokens)
    B = len(rows)
    row_ids = list(range(B)) if row_ids is None else list(row_ids)
    state = [int(t) for t, _, _ in rows]
    head = [int(h) for _, h, _ in rows]
    forced = [list(f) if f is not None else [-1] * max_new for _, _, f in rows]
    done, out_len = [False] * B, [0] * B
    out_ids = [[0] * max_new for _ in range(B)]
    head_at = [None] * B
    for g in range(max(origins) + max_new + extra_steps):
        for b in range(B):
            if origins[b] > g:
                continue
            local = g - origins[b]
            step = lambda use: g if use in shared else local
            lo, hi = P.head_range(cfg, head[b])
            raw = (table[state[b], :NV].astype(np.float32) * np.float32(scale)).astype(np.float32)
            hist = out_ids[b][:max(0, min(out_len[b], max_new))]
            row = process_row_ref(raw, hist, lo, hi, params, step("min_new"), eos)
            row = CP.constrain_row(row, hist, lo, hi, no_begin, step("min_new"), params.min_new_tokens)
            row = CP.constrain_row(row, hist, lo, hi, only_begin, step("begin_suppress"), 0)
            if sampling is None:
                tok = P.select(row, lo, hi)
            else:
                tok = lo + sample_row_ref(row[lo:hi], sampling[0], sampling[1], sampling[2], philox_uniform(sampling[3], step("philox"), row_ids[b]))
            feed = tok
            if step("guard") < max_new:
                i = step("index")
                if 0 <= i < max_new and forced[b][i] >= 0:
                    feed = forced[b][i]
            s_len = 0
            if not done[b] and step("guard") < max_new:
                i = step("index")
                if i < max_new:                               # (past the row of the array: the model drops the write)
                    out_ids[b][i] = tok
                out_len[b] = step("out_len") + 1
                if eos >= 0 and tok == eos:
                    done[b] = True
                s_len = step("stop_len") + 1
            head[b] = {V: 1, V + 1: 2, V + Tv + 1: 0}.get(feed, head[b])
            state[b] = feed
            if s_len > 0 and CP.stop_match(out_ids[b][:min(s_len, max_new)], cons):
                done[b] = True
            if local == max_new - 1:
                head_at[b] = head[b]
    return [out_ids[b][:min(out_len[b], max_new)] for b in range(B)], list(out_len), head_at


def alone(table, cfg, row, eos, max_new, scale, params=None, cons=None, sampling=None, row_id=0):
    """one row decoded alone from the counter's zero: (ids, length, head)"""
    o = restate_origins(table, cfg, [row], [0], eos, max_new, scale, params, cons, sampling, [row_id], extra_steps=0)
    return o[0][0], o[1][0], o[2][0]


# ---- the scenarios: four rows at ORIGINS; rows 2 and 3 join a running batch.  Each names the uses whose near miss it must tell. --------------------
def plain_scenario(cfg, plan, max_new):
    """the P table, greedy: two rows of eos_rows that run from the start (one ends at step 1), an admitted row that starts under the time head, an
    admitted teacher-forced row that emits EOS at its own step 6"""
    rows, _ = P.eos_rows(cfg, plan, P.EOS_BATCH, max_new)
    tour = P.batch_rows(cfg, plan, 8, max_new)
    timed = next(r for r in tour if r[1] == 1)
    st = [plan.fillers[(5 + i) % len(plan.fillers)] for i in range(max_new + 1)]
    st[6] = plan.eos_emitter
    return dict(rows=[rows[1], rows[4], timed, (st[0], 0, st[1:])], eos=plan.eos, tells=("index", "out_len", "guard"))


def sampled_scenario(cfg, plan, max_new, seed=20261020):
    """the P table, flat heads (the draw depends on the Philox counter alone): every row is forced to stay in its flat state"""
    case = {c.name: c for c in plan.cases}
    f0, f1 = case["flat@0"].token, case["flat@1"].token
    rows = [(f0, 0, [f0] * max_new), (f1, 1, [f1] * max_new), (f1, 1, [f1] * max_new), (f0, 0, [f0] * max_new)]
    return dict(rows=rows, eos=-1, sampling=(1.0, 0, 1.0, seed), row_ids=[0, 1, 6, 2], tells=("philox",))


def processor_scenarios(cfg, cplan):
    """the CP table, free-running rows: (name, rows, eos, params, constraints, tells)"""
    b = cplan.base
    c0, c1, c2 = b.cycle
    b0, m, _, _ = cplan.begin
    C = Constraints
    fill = [(c0, 0, None), (b.tour[0][0], 0, None)]
    return [
        dict(name="min_new", rows=fill + [(b.eos_emitter, 0, None), (b.eos_back, 0, None)], eos=b.eos, params=LogitsParams(min_new_tokens=3),
             cons=C(), tells=("min_new",)),
        dict(name="begin_suppress", rows=fill + [(b0, 0, None), (b0, 0, None)], eos=-1, params=None, cons=C(begin_suppress_tokens=[m]),
             tells=("begin_suppress",)),
        dict(name="stop", rows=fill + [(c0, 0, None), (c1, 0, None)], eos=-1, params=None, cons=C(stop_sequences=[[c1, c2, c0]]),
             tells=("stop_len",)),
        dict(name="ngram", rows=fill + [(c0, 0, None), (c2, 0, None)], eos=-1, params=LogitsParams(no_repeat_ngram_size=2), cons=C(), tells=()),
    ]


# ---- the schedules, from the lengths alone ------------------------------------------------------------------------------------------------------
def queue_schedule(lengths, max_new, cap, chunk, retire_fraction=8, admit_fraction=8):
    """TraceEngine.generate_queue's schedule for requests whose restated lengths are `lengths` (a row is finished once it has recorded that many ids:
    its EOS, or max_new of them): (rows x steps, [batch size of every chunk stepped], admits, retires, batches begun)"""
    from trace_amd.admit import admit_plan
    from trace_amd.retire import retire_plan
    todo = list(range(len(lengths)))
    row_steps, sizes, admits, retires, begun = 0, [], 0, 0, 0
    while todo:
        rows, todo = todo[:cap], todo[cap:]
        own = [1] * len(rows)                             # ids recorded
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
            n = min(chunk, max_new - min(own))
            row_steps += n * len(rows)
            sizes.append(len(rows))
            own = [o + n for o in own]
    return row_steps, sizes, admits, retires, begun


def fixed_schedule(lengths, ends_in_eos, max_new, batch, chunk, retire_fraction=8):
    """rows x steps of TraceEngine.decode(retire_finished=True) over fixed batches of `batch` requests: a row is finished once it has recorded its EOS
    (ends_in_eos[r]); a row that runs to max_new ids is never retired"""
    from trace_amd.retire import retire_plan
    total = 0
    for i in range(0, len(lengths), batch):
        rows, done = list(range(i, min(i + batch, len(lengths)))), 0
        while done < max_new - 1:
            n = min(chunk, max_new - 1 - done)
            total += n * len(rows)
            done += n
            fin = [ends_in_eos[r] and done + 1 >= lengths[r] for r in rows]
            if all(fin):
                break
            if done < max_new - 1 and retire_plan(len(rows), fin.count(False), retire_fraction):
                rows = [r for r, f in zip(rows, fin) if not f]
    return total


# EOS position (own step, None = never) of the 24 requests of the end-to-end test: per eight, two that end with their token 0, two that never end
QUEUE_ENDS = [0, None, 5, 2, 0, 17, None, 9,   1, 0, None, 30, 3, 0, 12, None,   None, 0, 7, 22, 0, 1, None, 4]
