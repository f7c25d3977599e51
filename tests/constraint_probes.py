"""Constraint probes: the table of tests/logits_probes.py with a few more designed states, on which bad words, suppressed ids, begin-suppress, stop
sequences and min_new_tokens over several EOS ids each have one right answer per step; a restatement of the decode loop with the rules in it; the
mutants; the case list.

The decoder's logits after feeding token t are exactly logit_scale * T[t] (token_select_probes.py), and every row of T has, per head, one maximum,
one runner-up 4 units below it and nothing else within 8 units of the runner-up (logits_probes.build_table): a ban on the maximum hands the step to
the runner-up.  States used here (text head unless said otherwise):

  * cycle  c0 -> c1 -> c2 -> c0, runner-ups q0, q1, q2 outside the cycle (logits_probes).
  * tour   d0 -> d1 -> <sync> -> time id tm+5 -> first time id tm -> score id sc+4 -> first score id sc -> d0: all three heads (logits_probes).
  * EOS    e -> eos, runner-up r; r -> x -> e (logits_probes).  Added: g -> eos2 (a second EOS id), runner-up r.
  * begin  b0 -> m, runner-up y0; y0 -> y1 -> b0: from b0, m is the maximum at step 0 and again at step 3.

Nothing here imports the HIP library; everything runs on the CPU."""
import dataclasses
from typing import List, Optional, Tuple

import numpy as np

import logits_probes as LP
import token_select_probes as P
from trace_amd.sampling import Constraints, LogitsParams, philox_uniform, process_row_ref, sample_row_ref

MAX_NEW = 40                                     # a stop sequence of 32 ids fires at step 31
GEOMETRIES = P.GEOMETRIES
MUTANTS = ("badword_prefix_one_short", "badword_prefix_one_long", "badword_len1_ignored", "badword_wraps_short_history",
           "ban_outside_head_hits_other_head", "suppress_only_first_step", "begin_suppress_every_step", "stop_matches_anywhere",
           "stop_wraps_short_history", "stop_drops_stop_ids", "stop_records_after_done", "stop_reads_row_zero", "prompt_in_history",
           "min_new_ignores_extra_eos")


@dataclasses.dataclass
class Plan:
    base: LP.Plan
    eos2: int
    eos2_emitter: int                # g
    begin: Tuple[int, int, int, int]  # b0, m, y0, y1
    alias: int                       # a text id x with (V + 1) + (x - (V + 1)) mod Tv == tm + 5: what a ban without a range check would hit under head 1


def build_table(cfg, seed=1):
    """(T int16 [NV, NVpad], Plan): logits_probes.build_table plus the states above, set by the same recipe (20 / 16 / at most 8)"""
    V, Tv, Sv, NV, NVpad = P.dims(cfg)
    T, base = LP.build_table(cfg, seed)
    T = T.copy()
    eos2, g, b0, m, y0, y1 = 310, 311, 312, 313, 314, 315
    taken = {base.eos, base.eos_emitter, base.eos_runner, base.eos_back, *base.cycle, *base.cycle_runner, *(t for t, _ in base.tour), *base.fillers}
    assert not taken & {eos2, g, b0, m, y0, y1}

    def set_pair(t, top, runner):
        lo, hi = P.head_range(cfg, 0)
        T[t, lo:hi] = np.minimum(T[t, lo:hi], LP.T_REST)
        T[t, top], T[t, runner] = LP.T_MAX, LP.T_RUNNER

    set_pair(g, eos2, base.eos_runner)
    set_pair(b0, m, y0)
    set_pair(y0, y1, 290)
    set_pair(y1, b0, 291)
    lo1, _ = P.head_range(cfg, 1)
    alias = next(x for x in range(P.text_cols(cfg) - 1, 0, -1)
                 if (x - lo1) % Tv == 5 and x not in taken and x not in (eos2, g, b0, m, y0, y1, 290, 291))
    LP.check_table(T, cfg)
    return T, Plan(base, eos2, g, (b0, m, y0, y1), alias)


# ---- the rules, restated with one broken on purpose -----------------------------------------------------------------------------------------
def constrain_row(row, hist, lo, hi, cons: Constraints, step, min_new, mutant=None):
    """sampling.constrain_row_ref written out rule by rule (mutant None: the same values — tests/test_constraints_cpu.py holds the two together),
    with the near misses of MUTANTS that live inside one row"""
    x = np.asarray(row, np.float32)
    out = np.full(len(x), -np.inf, np.float32)
    out[lo:hi] = x[lo:hi]
    h, L, n = [int(t) for t in hist], len(hist), hi - lo

    def ban(t):
        if lo <= t < hi:
            out[t] = -np.inf
        elif mutant == "ban_outside_head_hits_other_head":
            out[lo + (t - lo) % n] = -np.inf               # the offset without its range check, folded into the head

    for w in cons.bad_words_ids:
        k = len(w)
        if k == 1:
            if mutant != "badword_len1_ignored":
                ban(w[0])
            continue
        pre = list(w[:-1])
        if mutant == "badword_prefix_one_short":
            pre = pre[1:]                                   # one id fewer compared
        need = len(pre) + (1 if mutant == "badword_prefix_one_long" else 0)       # one id more of history asked for
        if mutant == "badword_wraps_short_history" and L < len(pre):
            pre = pre[len(pre) - L:]                        # the ids the history does not have are not compared
            need = L
        if L >= need and (h[L - len(pre):] if pre else []) == pre:
            ban(w[-1])
    if not (mutant == "suppress_only_first_step" and step > 0):
        for t in cons.suppress_tokens:
            ban(t)
    if step == 0 or mutant == "begin_suppress_every_step":
        for t in cons.begin_suppress_tokens:
            ban(t)
    if step < min_new and mutant != "min_new_ignores_extra_eos":
        for w in cons.stop_sequences:
            if len(w) == 1:
                ban(w[0])
    return out


def stop_match(hist, cons: Constraints, mutant=None):
    """sampling.stop_match_ref with the near misses; returns the length of the sequence that fired, 0 for none"""
    h, L = [int(t) for t in hist], len(hist)
    for w in cons.stop_sequences:
        w, k = list(w), len(w)
        if L >= k and h[L - k:] == w:
            return k
        if mutant == "stop_wraps_short_history" and 0 < L < k and h == w[k - L:]:
            return k
        if mutant == "stop_matches_anywhere" and k > 1 and L >= k and h[-1] == w[-1] and any(h[i:i + k - 1] == w[:-1] for i in range(L - k + 1)):
            return k
    return 0


def restate(table, cfg, start_token, head, params: Optional[LogitsParams], cons: Constraints, eos, max_new, scale, mutant=None, row_zero=None,
            sampling=None, row_index=0, trace=None):
    """(ids, length, final_head) of one free-running row: logits_probes.restate_processed with the ban rules behind the processors and the stop rule
    behind the recording.  row_zero: the per-step histories of row 0 (the mutant that matches every row against row 0's ids).  trace receives
    (state, head, raw row, processed row, tok) per step."""
    V, Tv, Sv, NV, _ = P.dims(cfg)
    assert mutant is None or mutant in MUTANTS
    params = params or LogitsParams()
    state, ids, length, done = int(start_token), [], 0, False
    for s in range(max_new):
        lo, hi = P.head_range(cfg, head)
        raw = (table[state, :NV].astype(np.float32) * np.float32(scale)).astype(np.float32)
        hist = ([int(start_token)] if mutant == "prompt_in_history" else []) + list(ids)
        row = process_row_ref(raw, hist, lo, hi, params, s, eos)
        row = constrain_row(row, hist, lo, hi, cons, s, params.min_new_tokens, mutant)
        if sampling is None:
            tok = P.select(row, lo, hi)
        else:
            tok = lo + sample_row_ref(row[lo:hi], sampling[0], sampling[1], sampling[2], philox_uniform(sampling[3], s, row_index))
        if trace is not None:
            raw[:lo] = -np.inf
            raw[hi:] = -np.inf
            trace.append((state, head, raw, row, tok))
        if not done or mutant == "stop_records_after_done":
            ids.append(tok)
            length = len(ids)
            if eos >= 0 and tok == eos:
                done = True
            match_hist = ([int(start_token)] if mutant == "prompt_in_history" else []) + ids
            if mutant == "stop_reads_row_zero" and row_zero is not None:
                match_hist = row_zero[s]
            k = 0 if done else stop_match(match_hist, cons, mutant)
            if k:
                done = True
                if mutant == "stop_drops_stop_ids":
                    ids = ids[:max(len(ids) - k, 0)]
                    length = len(ids)
        head = {V: 1, V + 1: 2, V + Tv + 1: 0}.get(tok, head)
        state = tok
    return ids, length, head


def restate_batch(table, cfg, rows, params, cons, eos, max_new, scale, mutant=None, sampling=None):
    """([ids], [length], [final head]); rows: [(start token, start head)]"""
    out, zero = [], None
    for b, (t, h) in enumerate(rows):
        o = restate(table, cfg, t, h, params, cons, eos, max_new, scale, mutant, zero if b else None, sampling, b)
        if b == 0:
            zero = [o[0][:s + 1] for s in range(max_new)]          # row 0's recorded ids after each step
        out.append(o)
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


# ---- the decode cases (the GPU test runs them; the CPU test holds the same list up against the mutants) ---------------------------------------
@dataclasses.dataclass
class DecodeCase:
    name: str
    cons: Constraints
    rows: List[Tuple[int, int]]
    eos: int = -1
    params: Optional[LogitsParams] = None
    stops: bool = False              # a stop case: some row must end before MAX_NEW
    rejects: Tuple[str, ...] = ()    # the mutants this case is there to tell from the rules


def decode_cases(cfg, plan: Plan):
    V, Tv, Sv, NV, _ = P.dims(cfg)
    b = plan.base
    c0, c1, c2 = b.cycle
    d0, d1 = b.tour[0][0], b.tour[1][0]
    tm = V + 1
    b0, m, y0, y1 = plan.begin
    C = Constraints
    cyc, tour = [(c0, 0)], [(d0, 0)]
    period = [c1, c2, c0]
    return [
        DecodeCase("badword_len1", C(bad_words_ids=[[c2]]), cyc, rejects=("badword_len1_ignored",)),
        # the prefix (c1, c2) is there at step 2, when the history is exactly as long as it
        DecodeCase("badword3_once", C(bad_words_ids=[[c1, c2, c0]]), cyc, rejects=("badword_prefix_one_long",)),
        # the prefix (c0, c1) is complete at step 4 only; at step 1 the history is its second id alone, and the prompt's last id is c0
        DecodeCase("badword3_short_history", C(bad_words_ids=[[c0, c1, c2]]), cyc, rejects=("badword_wraps_short_history", "prompt_in_history")),
        DecodeCase("badword_cross_heads", C(bad_words_ids=[[d1, V, tm + 5]]), tour),
        # (d0, <sync>) never ends the history, (<sync>) alone does at step 2; the second word fires at step 3
        DecodeCase("badword_near_miss", C(bad_words_ids=[[d0, V, tm + 5], [V, tm + 5, tm]]), tour, rejects=("badword_prefix_one_short",)),
        # the first word's last id is a text id while the time head is active: nothing may happen at step 2; the second fires at step 3
        DecodeCase("badword_other_head", C(bad_words_ids=[[d1, V, plan.alias], [tm]]), tour, rejects=("ban_outside_head_hits_other_head",)),
        DecodeCase("suppress", C(suppress_tokens=[m, V + 3]), [(b0, 0)], rejects=("suppress_only_first_step",)),
        DecodeCase("begin_suppress", C(begin_suppress_tokens=[m]), [(b0, 0)], rejects=("begin_suppress_every_step",)),
        DecodeCase("stop_second_eos", C(stop_sequences=[[plan.eos2]]), [(plan.eos2_emitter, 0), (b.eos_emitter, 0)], eos=b.eos, stops=True,
                   rejects=("stop_drops_stop_ids", "stop_records_after_done")),
        DecodeCase("stop3_at_step2", C(stop_sequences=[period]), cyc, stops=True, rejects=("stop_records_after_done",)),
        DecodeCase("stop32", C(stop_sequences=[(period * 11)[:32]]), cyc, stops=True, rejects=("stop_wraps_short_history",)),
        # (c1, c2) opens the history and c1 comes round again at step 3, but (c1, c2, c1) is never its tail; the second sequence fires at step 5
        DecodeCase("stop_prefix_earlier", C(stop_sequences=[[c1, c2, c1], [c0, c1, c2, c0]]), cyc, stops=True, rejects=("stop_matches_anywhere",)),
        # at step 1 the history (c1, c2) is the sequence's last two ids; it fires at step 4
        DecodeCase("stop_longer_than_history", C(stop_sequences=[[c2, c0, c1, c2]]), cyc, stops=True, rejects=("stop_wraps_short_history",)),
        # row 0 tours the heads and never holds the sequence; rows 1 and 2 do, at steps 2 and 4
        DecodeCase("stop_other_row", C(stop_sequences=[period]), [(d0, 0), (c0, 0), (c1, 0)], stops=True, rejects=("stop_reads_row_zero",)),
        DecodeCase("stop_cross_heads", C(stop_sequences=[[V, tm + 5, tm]]), tour, stops=True),
        # the prompt ends in c0: (c0, c1) is in the generated ids at step 3, not at step 0
        DecodeCase("stop_not_in_prompt", C(stop_sequences=[[c0, c1]]), cyc, stops=True, rejects=("prompt_in_history",)),
        DecodeCase("min_new3_two_eos", C(stop_sequences=[[plan.eos2]]), [(plan.eos2_emitter, 0), (b.eos_emitter, 0), (b.eos_back, 0)], eos=b.eos,
                   params=LogitsParams(min_new_tokens=3), stops=True, rejects=("min_new_ignores_extra_eos",)),
        DecodeCase("all_rules", C([[plan.eos2], period], [[c1, c2, c0], [d1, V, tm + 5]], [m], [c1]),
                   [(c0, 0), (d0, 0), (b0, 0), (plan.eos2_emitter, 0)], eos=b.eos, params=LogitsParams(1.5, 0, 2), stops=True),
    ]


def wide_rows(plan: Plan, B):
    """B rows that carry different histories: the designed start states in turn"""
    b = plan.base
    pool = [(c, 0) for c in b.cycle] + list(b.tour) + [(plan.begin[0], 0), (plan.eos2_emitter, 0), (b.eos_emitter, 0), (b.eos_back, 0)]
    pool += [(t, 0) for t in b.fillers]
    return [pool[i % len(pool)] for i in range(B)]


# ---- loose rows: what the loose-row ops and HF's processors are held against ------------------------------------------------------------------
@dataclasses.dataclass
class RowCase:
    row: np.ndarray                  # float32 [NV], -inf outside the head
    head: int
    hist: List[int]
    cons: Constraints
    step: int
    min_new: int


def row_cases(cfg, seed=7) -> List[RowCase]:
    """random rows per head; bad words of 1, 2, 3 and 32 ids whose prefixes end the history, end it one id early, are longer than it or are absent;
    last ids inside the head, at its two ends, just outside them and in other heads; suppress lists with the same spread; steps 0 and 2; histories
    of length 0, 1, k - 2, k - 1, k and 40"""
    V, Tv, Sv, NV, _ = P.dims(cfg)
    rng = np.random.default_rng(seed)
    cases = []
    for head in range(3):
        lo, hi = P.head_range(cfg, head)
        spread = [t for t in (lo, hi - 1, lo - 1, hi, 0, V, V + 1, V + 1 + Tv, NV - 1) if 0 <= t < NV] + [int(t) for t in rng.integers(lo, hi, size=4)]
        for L in (0, 1, 2, 3, 31, 40):
            for step in (0, 2):
                row = np.full(NV, -np.inf, np.float32)
                row[lo:hi] = (rng.standard_normal(hi - lo) * 4).astype(np.float32)
                hist = [int(t) for t in rng.integers(0, NV, size=L)]
                bad = [[t] for t in spread[:3]]
                for k in (2, 3, 32):
                    last = [int(spread[int(i)]) for i in rng.integers(0, len(spread), size=4)]
                    if L >= k - 1:
                        bad.append(hist[L - (k - 1):] + [last[0]])                             # the prefix ends the history
                    if L >= k:
                        bad.append(hist[L - k:L - 1] + [last[1]])                              # ... ends it one id early
                    bad.append([int(t) for t in rng.integers(0, NV, size=k - 1)] + [last[2]])   # absent (or longer than the history)
                    if L >= 1:
                        bad.append([NV - 1] * (k - 1 - min(L, k - 2)) + hist[L - min(L, k - 2):] + [last[3]])   # only its last ids end the history
                stops = [[spread[0]], [spread[3], spread[1]], [int(t) for t in rng.integers(lo, hi, size=1)]]
                cons = Constraints(stops, bad[:64], spread[3:9], spread[::2])
                for min_new in (0, 3):
                    cases.append(RowCase(row, head, hist, cons, step, min_new))
    return cases


def history_cases(cfg, seed=9):
    """[(histories, Constraints)] for the stop matcher: sequences of 1, 2, 3 and 32 ids against histories shorter than, as long as and longer than
    them, ending in them, holding them earlier but not at the tail, ending in all but their first id"""
    V, Tv, Sv, NV, _ = P.dims(cfg)
    rng = np.random.default_rng(seed)
    out = []
    for k in (1, 2, 3, 32):
        w = [int(t) for t in rng.integers(0, NV, size=k)]
        other = [int(t) for t in rng.integers(0, NV, size=40)]
        hists = [[], w, w[1:], w[:-1], other[:5] + w, w + other[:5], other + w, w + w, other[:3] + w[1:], (other + w)[-k:], [w[-1]], other]
        out.append((hists, Constraints(stop_sequences=[w, [NV - 1, 0, NV - 1]])))
    many = [[int(t) for t in rng.integers(0, NV, size=int(n))] for n in rng.integers(1, 33, size=64)]
    out.append(([many[5], many[63] + [1], [2] + many[63], many[0][:-1], other[:7] + many[40]], Constraints(stop_sequences=many)))
    return out
