"""Logits-processor probes: a table for the identity-layer decoder of tests/token_select_probes.py on which repetition penalty, no-repeat n-grams
and min_new_tokens each have one right answer per step, a restatement of the decode loop with the processors in it, the mutants, and the case lists.

The decoder's logits after feeding token t are exactly logit_scale * T[t] (token_select_probes.py).  Here every row of T has, in each head, one
maximum (20), one known runner-up (16: 4 units below) and nothing else above 8 (8 units below the runner-up), so a processor that takes the
maximum away hands the step to the runner-up, and 20 / 1.5 < 16 while 20 / 1.2 > 16 > 20 / 1.2^2.  The designed states:

  * cycle  c0 -> c1 -> c2 -> c0 (text head, free running).  c0 and c2 have a positive maximum; c1 has a NEGATIVE one (-10, runner-up -14,
    everything else <= -18): -10 * 1.5 < -14 < -10 / 1.5, so the penalty has to multiply there.  Runner-ups q0, q1, q2 lie outside the cycle.
  * tour   d0 -> d1 -> <sync> -> time id -> first time id -> score id -> first score id -> d0: a cycle through all three heads, whose history
    holds ids of other heads than the active one.
  * EOS    e -> eos, runner-up r; r -> x -> e: from e with min_new_tokens = 3 the row emits r, x, e, eos: EOS at exactly step 3, length 4.
  * last   (score id sc + 9, head 2) -> the last id of the vocabulary: what a min_new_tokens rule that forgets `eos >= 0` bans at eos = -1.

Nothing here imports the HIP library; everything runs on the CPU."""
import dataclasses
from typing import List, Optional, Sequence, Tuple

import numpy as np

import token_select_probes as P
from trace_amd.sampling import LogitsParams, philox_uniform, process_row_ref, sample_row_ref

T_MAX, T_RUNNER, T_REST = 20, 16, 8
N_MAX, N_RUNNER, N_REST = -10, -14, -18          # the negative state
MUTANTS = ("penalty_per_occurrence", "penalty_divides_negative", "penalty_multiplies_positive", "prompt_in_history", "ngram_window_one_short",
           "ngram_window_one_long", "ngram_bans_suffix_start", "min_new_off_by_one", "min_new_ignores_eos_off", "history_of_row_zero_for_all")
MAX_NEW = 24                                     # every case below: long enough for two rounds of the longer cycle and n = 3 (7 + 3 - 1 < 24)
GEOMETRIES = P.GEOMETRIES


@dataclasses.dataclass
class Plan:
    cycle: List[int]                 # c0, c1, c2 (text ids, head 0); c1 is the negative state
    cycle_runner: List[int]          # q0, q1, q2
    tour: List[Tuple[int, int]]      # (state, head it is read under), cyclic
    eos: int
    eos_emitter: int
    eos_runner: int                  # r
    eos_back: int                    # x: r -> x -> e
    last_state: Tuple[int, int]      # (sc + 9, 2) -> NV - 1
    fillers: List[int]               # ordinary text tokens


def build_table(cfg, seed=1):
    """(T int16 [NV, NVpad], Plan) on the recipe of token_select_probes.build_table: row t = the logits after feeding t in units of logit_scale.
    Ordinary rows: per head one 20 at m_h(t), one 16 at r_h(t), the rest in [-40, 8]; m_0 and r_0 stay inside the text ids that own a column, so a
    free-running row leaves the text head only through a designed state."""
    V, Tv, Sv, NV, NVpad = P.dims(cfg)
    rng = np.random.default_rng(seed)
    T = np.zeros((NV, NVpad), np.int16)
    toks = P.tokens_with_columns(cfg)
    ncol = P.text_cols(cfg)
    T[toks, :NV] = rng.integers(-40, T_REST + 1, size=(len(toks), NV))
    eos, e, r, x = 300, 305, 306, 307
    cyc, cq = [250, 255, 260], [251, 256, 261]
    d0, d1 = 265, 266
    tm, sc = V + 1, V + 1 + Tv
    tour = [(d0, 0), (d1, 0), (V, 1), (tm + 5, 1), (tm, 2), (sc + 4, 2), (sc, 0)]
    designed_text = {eos, e, r, x, d0, d1, *cyc, *cq}

    def avoid(n):                                # ordinary rows never point at a designed text state
        while n in designed_text:
            n = (n + 1) % ncol
        return n

    def set_pair(t, h, top, runner, vals=(T_MAX, T_RUNNER, T_REST)):
        lo, hi = P.head_range(cfg, h)
        T[t, lo:hi] = np.minimum(T[t, lo:hi], vals[2])
        T[t, top], T[t, runner] = vals[0], vals[1]

    for t in toks:
        t = int(t)
        m0 = avoid((7 * t + 3) % ncol)
        r0 = avoid((11 * t + 5) % ncol)
        if r0 == m0:
            r0 = avoid((r0 + 1) % ncol)
        set_pair(t, 0, m0, r0)
        m1, r1 = tm + (5 * t + 2) % (Tv - 1) + 1, tm + (3 * t + 1) % (Tv - 1) + 1            # never the first time id (the switch to the score head)
        set_pair(t, 1, m1, r1 if r1 != m1 else tm + (r1 - tm) % (Tv - 1) + 1)
        m2, r2 = sc + (5 * t + 4) % (Sv - 1) + 1, sc + (3 * t + 2) % (Sv - 1) + 1            # never the first score id (the switch to the text head)
        set_pair(t, 2, m2, r2 if r2 != m2 else sc + (r2 - sc) % (Sv - 1) + 1)
    # the designed states
    for i, c in enumerate(cyc):
        set_pair(c, 0, cyc[(i + 1) % 3], cq[i], (N_MAX, N_RUNNER, N_REST) if i == 1 else (T_MAX, T_RUNNER, T_REST))
    for i, (t, h) in enumerate(tour):
        lo, hi = P.head_range(cfg, h)
        nxt = tour[(i + 1) % len(tour)][0]
        runner = next(n for n in range(lo + 2, hi) if n != nxt and n not in designed_text and n not in (tm, sc, V))
        set_pair(t, h, nxt, runner)
    set_pair(e, 0, eos, r)
    set_pair(r, 0, x, avoid(270))
    set_pair(x, 0, e, avoid(271))
    set_pair(sc + 9, 2, NV - 1, sc + 3)
    assert T.min() >= -64 and T.max() <= 64 and (T[:, NV:] == 0).all()
    fillers = [t for t in range(272, 290) if t not in designed_text]
    return T, Plan(cyc, cq, tour, eos, e, r, x, (sc + 9, 2), fillers)


def check_table(T, cfg):
    """every row that owns a column: per head one maximum, one runner-up >= 4 units below it, everything else >= 4 units below the runner-up"""
    for t in P.tokens_with_columns(cfg):
        for h in range(3):
            lo, hi = P.head_range(cfg, h)
            v = np.sort(T[int(t), lo:hi].astype(np.int64))[::-1]
            assert v[0] - v[1] >= 4 and v[1] - v[2] >= 4, (int(t), h, v[:3])


def runner_up(T, cfg, state, head):
    lo, hi = P.head_range(cfg, head)
    return lo + int(np.argsort(-T[state, lo:hi].astype(np.int64), kind="stable")[1])


# ---- the rules, restated with one broken on purpose -----------------------------------------------------------------------------------------
def process_row(row, hist, lo, hi, params, step, eos, mutant=None):
    """sampling.process_row_ref written out id by id (mutant None: the same bits — tests/test_logits_processors_cpu.py holds them together), with
    the near misses of MUTANTS that live inside one row"""
    x = np.asarray(row, np.float32)
    out = np.full(len(x), -np.inf, np.float32)
    out[lo:hi] = x[lo:hi]
    p = np.float32(params.repetition_penalty)
    h = [int(t) for t in hist]
    if p != np.float32(1.0):
        seen = set()
        for t in h:
            if not lo <= t < hi or (t in seen and mutant != "penalty_per_occurrence"):
                continue
            seen.add(t)
            v = out[t] if mutant == "penalty_per_occurrence" else x[t]
            neg = v < 0
            if mutant == "penalty_divides_negative":
                neg = False
            elif mutant == "penalty_multiplies_positive":
                neg = True
            out[t] = v * p if neg else v / p
    n, L = int(params.no_repeat_ngram_size), len(h)
    if n >= 1:
        w = n - 1 + {"ngram_window_one_short": -1, "ngram_window_one_long": 1}.get(mutant, 0)         # ids compared
        w = max(w, 0)
        if L >= w:
            suffix = h[L - w:] if w else []
            for i in range(0, L - w):
                if h[i:i + w] == suffix:
                    t = h[i + w - 1] if mutant == "ngram_bans_suffix_start" and w else h[i + w]
                    if lo <= t < hi:
                        out[t] = -np.inf
    m = int(params.min_new_tokens) - (1 if mutant == "min_new_off_by_one" else 0)
    if step < m:
        if mutant == "min_new_ignores_eos_off" and eos < 0:
            out[len(x) + eos] = -np.inf                       # the unguarded store lands on the row's last id
        elif lo <= eos < hi:
            out[eos] = -np.inf
    return out


def restate_processed(table, cfg, start_token, head, params, eos, max_new, scale, mutant=None, other_hist=None, sampling=None, row_index=0,
                      trace=None):
    """(ids, length, final_head) of one free-running row: token_select_probes.restate with the processors applied to logit_scale * T[state]
    before the selection.  params: LogitsParams.  other_hist: the ids of row 0 (the mutant that hands every row row 0's history).  sampling:
    (temperature, top_k, top_p, seed) draws with sampling.sample_row_ref from the processed row, Philox counter (step, row_index).
    trace: receives (state, head, raw row, tok) per step."""
    V, Tv, Sv, NV, _ = P.dims(cfg)
    assert mutant is None or mutant in MUTANTS
    state, ids, length, done = int(start_token), [], 0, False
    for s in range(max_new):
        lo, hi = P.head_range(cfg, head)
        raw = (table[state, :NV].astype(np.float32) * np.float32(scale)).astype(np.float32)
        hist = list(ids)
        if mutant == "prompt_in_history":
            hist = [int(start_token)] + hist
        elif mutant == "history_of_row_zero_for_all" and other_hist is not None:
            hist = list(other_hist[:s])
        row = process_row(raw, hist, lo, hi, params, s, eos, mutant) if mutant else process_row_ref(raw, hist, lo, hi, params, s, eos)
        if sampling is None:
            tok = P.select(row, lo, hi)
        else:
            tok = lo + sample_row_ref(row[lo:hi], sampling[0], sampling[1], sampling[2], philox_uniform(sampling[3], s, row_index))
        if trace is not None:
            raw[:lo] = -np.inf
            raw[hi:] = -np.inf
            trace.append((state, head, raw, tok))
        if not done:
            ids.append(tok)
            length = s + 1
        if eos >= 0 and tok == eos:
            done = True
        head = {V: 1, V + 1: 2, V + Tv + 1: 0}.get(tok, head)
        state = tok
    return ids, length, head


def restate_batch(table, cfg, rows, params, eos, max_new, scale, mutant=None, sampling=None):
    """([ids], [length], [final head]); rows: [(start token, start head)]"""
    out = []
    for b, (t, h) in enumerate(rows):
        other = out[0][0] if b and mutant == "history_of_row_zero_for_all" else None
        out.append(restate_processed(table, cfg, t, h, params, eos, max_new, scale, mutant, other, sampling, b))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


# ---- the decode cases (the GPU test runs them; the CPU test holds the same lists up against the mutants) --------------------------------------
def start_rows(cfg, plan, B):
    """[(start token, start head)] of a batch: the three cycle states first (so B = 3 starts in three different states, the negative one among
    them), then the tour's states, the EOS states, the last-id state and fillers"""
    pool = [(c, 0) for c in plan.cycle] + list(plan.tour) + [(plan.eos_emitter, 0), (plan.eos_back, 0), plan.last_state]
    pool += [(t, 0) for t in plan.fillers]
    return pool[:B]


@dataclasses.dataclass
class DecodeCase:
    name: str
    params: LogitsParams
    eos: int                         # -1, or "plan" resolved by decode_cases
    rows: List[Tuple[int, int]]


def decode_cases(cfg, plan):
    rows3, rows17 = start_rows(cfg, plan, 3), start_rows(cfg, plan, 17)
    c0 = [(plan.cycle[0], 0)]
    cs = [DecodeCase("ngram2", LogitsParams(no_repeat_ngram_size=2), -1, rows3),
          DecodeCase("ngram3", LogitsParams(no_repeat_ngram_size=3), -1, rows3),
          DecodeCase("ngram2_b1", LogitsParams(no_repeat_ngram_size=2), -1, c0),
          DecodeCase("ngram1_b17", LogitsParams(no_repeat_ngram_size=1), -1, rows17),
          DecodeCase("penalty1.5", LogitsParams(repetition_penalty=1.5), -1, rows3),
          DecodeCase("penalty1.5_b17", LogitsParams(repetition_penalty=1.5), -1, rows17),
          DecodeCase("penalty1.2", LogitsParams(repetition_penalty=1.2), -1, rows3),
          DecodeCase("min_new3", LogitsParams(min_new_tokens=3), plan.eos, [(plan.eos_emitter, 0), (plan.eos_back, 0), (plan.cycle[0], 0)]),
          DecodeCase("min_new2", LogitsParams(min_new_tokens=2), plan.eos, [(plan.eos_back, 0)]),
          DecodeCase("min_new2_no_eos", LogitsParams(min_new_tokens=2), -1, [plan.last_state, (plan.eos_emitter, 0)]),
          DecodeCase("all_three", LogitsParams(1.5, 3, 3), plan.eos, rows3),
          DecodeCase("all_three_b17", LogitsParams(1.2, 2, 3), plan.eos, rows17)]
    return cs


# ---- loose rows: what the loose-row op and HF's processors are held against (the CPU and the GPU test share the list) ---------------------------
@dataclasses.dataclass
class RowCase:
    row: np.ndarray                  # float32 [NV], -inf outside the head
    head: int
    hist: List[int]
    params: LogitsParams
    step: int
    eos: int


def _rich_row(rng, lo, hi, NV):
    """a masked row whose head range holds two zeros, two -inf, a positive and a negative value at `inside` (six distinct ids) among Gaussians"""
    row = np.full(NV, -np.inf, np.float32)
    row[lo:hi] = (rng.standard_normal(hi - lo) * 4).astype(np.float32)
    inside = lo + rng.choice(hi - lo, size=6, replace=False)
    row[inside[:2]] = 0.0
    row[inside[2:4]] = -np.inf
    row[inside[4]], row[inside[5]] = 1.5, -1.5
    return row, inside


def row_cases(cfg, seed=5) -> List[RowCase]:
    """rows with -inf masks inside the head, zeros and both signs; histories with duplicate ids, ids of other heads and the ids at and just outside
    the head's ends; lengths 0, 1, n - 2, n - 1, n, 40; n in {1, 2, 3, 5}; p in {1.0, 0.7, 1.3}; m in {0, 1, 3} with eos inside and outside the head"""
    V, Tv, Sv, NV, _ = P.dims(cfg)
    rng = np.random.default_rng(seed)
    cases = []
    for head in range(3):
        lo, hi = P.head_range(cfg, head)
        edge = [t for t in (lo, hi - 1, lo - 1, hi) if 0 <= t < NV]
        other = [t for t in (0, V, V + 1, V + 1 + Tv, NV - 1) if not lo <= t < hi]
        for n in (1, 2, 3, 5):
            for L in sorted({0, 1, max(n - 2, 0), n - 1, n, 40}):
                for p, m in ((1.0, 0), (0.7, 1), (1.3, 3)):
                    row, inside = _rich_row(rng, lo, hi, NV)
                    # a short alphabet: repeated ids and repeated n-grams; then the edges, other heads' ids, a zero and a masked id
                    alpha = list(rng.integers(lo, hi, size=3)) + [int(inside[0]), int(inside[2])] + edge + other[:2]
                    hist = [int(alpha[j]) for j in rng.integers(0, len(alpha), size=L)]
                    if L >= 2 * n and n > 1:                                  # make sure the suffix has occurred before
                        hist[-(n - 1):] = hist[:n - 1]
                    eos_in = int(rng.integers(lo, hi))
                    for eos in (eos_in, other[0], -1):
                        for step in ((0, m) if m else (0,)):
                            cases.append(RowCase(row, head, hist, LogitsParams(p, n, m), step, eos))
    # 48 equal ids: the penalty applies once, 48 threads claim one bit
    lo, hi = P.head_range(cfg, 0)
    row, inside = _rich_row(rng, lo, hi, NV)
    for t in (int(inside[4]), int(inside[5])):                       # a positive and a negative value
        cases.append(RowCase(row, 0, [t] * 48, LogitsParams(1.3, 0, 0), 5, -1))
    # ids just outside the head only: the row stays untouched
    for head in range(3):
        lo, hi = P.head_range(cfg, head)
        out_ids = [t for t in (lo - 1, hi) if 0 <= t < NV]
        cases.append(RowCase(_rich_row(rng, lo, hi, NV)[0], head, out_ids * 3, LogitsParams(1.3, 1, 0), 2, -1))
    return cases
