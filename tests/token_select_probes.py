"""Token-selection probes: an identity-layer decoder whose logits are known exactly, a plain restatement of the selection rules, and the case lists.

The stage under test turns the final-norm hidden row into a token: head_logits_kernel (active-head GEMV, head mask, per-tile arg-max partials),
select_next_kernel (arg-max over the tile partials with lowest-id tie-break, forced ids, EOS / done / out_len, the head switch, the gather of the
next embedding from the text, sync, time and score tables) and trace_llm_head_logits.  On random weights an exact tie, a larger logit just outside
the head's range or a flat head never occur.  Here they are built:

  * every self_attn.o_proj / mlp.down_proj weight is zero and model.norm.weight is one: every layer runs all of its kernels, the residual stream
    stays the embedding of the last fed token, bit for bit;
  * the embedding of token t is one-hot (value 1) at column col(t), in all four tables;
  * the head rows lm | sync | time | score hold W[n, col(t)] = T[t][n] / 16 with T an integer table in [-64, 64].

The logit of id n after feeding t is then one fp32 product s * T[t][n] / 16 plus exact zeros, s = the 16-bit rounding of rsqrt(1 / 4096 + eps) — the
same for every n.  Equal table entries give bit-equal logits and the order of the logits is the order of T: every emitted id has one right answer.

Columns: the hidden size is 4096, so at most 4096 tokens can own a column.  Where the vocabulary is larger (BIG) only the first 3000 text ids, sync,
time and score own one; the other text ids embed to zero, their T rows are zero, and no test feeds them.

Nothing here imports the HIP library; everything runs on the CPU."""
import dataclasses
from typing import List, Tuple

import numpy as np
import torch

from trace_amd import config as tcfg, synth

HIDDEN = 4096
BIG_TEXT_COLS = 3000
T_TIE, T_DECOY, T_BASE_HI = 20, 50, 8            # in-range maxima, out-of-range decoys, the largest ordinary in-range value
MUTANTS = ("highest_id_wins_tie", "lo_one_low", "hi_one_high", "no_mask", "switch_dropped", "switch_on_tok", "time_row_off_by_one",
           "done_keeps_recording", "tiles_from_256_ignored", "first_wave_only")


# ---- geometries ---------------------------------------------------------------------------------------------------------------------------
def small():
    """V = 320: 22 tiles of 16 ids, the time head inside one tile, all three heads inside tile 20"""
    return tcfg.tiny(num_frames=4)


def big():
    """V = 4499 (no multiple of 16: every head boundary falls mid-tile), NV = 4526: 283 tiles, so select_next_kernel's strided loop, its
    shuffle over all 64 lanes and its cross-wave merge all run"""
    return dataclasses.replace(tcfg.tiny(num_frames=4), vocab_size=4499)


def dims(cfg):
    V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
    NV = V + 1 + Tv + Sv
    return V, Tv, Sv, NV, (NV + 15) // 16 * 16


def head_range(cfg, head):
    V, Tv, Sv, _, _ = dims(cfg)
    return [(0, V + 1), (V + 1, V + 1 + Tv), (V + 1 + Tv, V + 1 + Tv + Sv)][head]


def switch_token(cfg, head):
    """the fed token that switches a row to `head`"""
    V, Tv, _, _, _ = dims(cfg)
    return [V + Tv + 1, V, V + 1][head]


def text_cols(cfg):
    V, _, _, NV, _ = dims(cfg)
    return V if NV <= HIDDEN else BIG_TEXT_COLS


def column(cfg, t):
    """the hidden column that token t's embedding is one-hot at, None for a text id without one"""
    V = cfg.vocab_size
    n = text_cols(cfg)
    if t < V:
        return t if t < n else None
    return n + (t - V)


def tokens_with_columns(cfg):
    V, _, _, NV, _ = dims(cfg)
    return np.concatenate([np.arange(text_cols(cfg)), np.arange(V, NV)])


def tile_of(n):
    return n // 16


def thread_of(n):
    """the thread of select_next_kernel that reads id n's tile partial (256 threads, tiles t, t + 256, ...)"""
    return tile_of(n) % 256


def wave_of(n):
    return thread_of(n) // 64


def pair_relation(a, b):
    """how select_next_kernel meets the tile partials of two ids: in one partial, in one thread's loop, in one wave's shuffle, or across waves"""
    if tile_of(a) == tile_of(b):
        return "same_tile"
    if thread_of(a) == thread_of(b):
        return "same_thread"
    return "same_wave" if wave_of(a) == wave_of(b) else "other_wave"


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    head: int
    token: int                       # feeding this token under `head` is the case
    ties: Tuple[int, ...]            # the ids that hold the in-range maximum; the lowest must be emitted
    kind: str                        # what the case claims (checked in integers by check_case)
    decoys: Tuple[int, ...] = ()     # out-of-range ids that hold more than the in-range maximum

    @property
    def expect(self):
        return min(self.ties)


@dataclasses.dataclass
class Plan:
    """what build_table designed besides the named cases"""
    cases: List[Case]
    chain: List[Tuple[int, int]]     # (state token, head it is read under), cyclic: free-running from chain[i] visits chain[i + 1], ...
    eos: int                         # a text id that only `eos_emitter` emits under head 0
    eos_emitter: int
    fillers: List[int]               # ordinary text tokens that emit neither eos nor a switch token under head 0

    def by_head(self, head):
        return [c for c in self.cases if c.head == head]


def _case_specs(cfg):
    """(name, head, ties, kind) for every named case the geometry has room for"""
    V, Tv, Sv, NV, _ = dims(cfg)
    specs = []
    for h in range(3):
        lo, hi = head_range(cfg, h)
        first_tile, last_tile = tile_of(lo), tile_of(hi - 1)
        add = lambda name, ties, kind=None: specs.append((f"{name}@{h}", h, tuple(sorted(ties)), kind or name))
        mid_tile = (first_tile + last_tile + 1) // 2 if h else min(100, last_tile // 2)
        mid = min(max(mid_tile * 16 + 6, lo + 1), hi - 2)
        add("unique_lo", [lo])
        add("unique_hi_1", [hi - 1])
        ft = (lo + 15) // 16 * 16                                      # the first id of a tile, inside the range and not lo itself
        if ft == lo:
            ft += 16
        if h == 0:
            ft = mid_tile * 16
        if lo < ft < hi:
            add("tile_first", [ft])
        lt = lo // 16 * 16 + 15 if h else mid_tile * 16 + 15           # the last id of a tile
        if lo < lt < hi - 1:
            add("tile_last", [lt])
        shared = [n for n in range(V // 16 * 16, V // 16 * 16 + 16) if lo < n < hi - 1]       # the tile that holds V: three heads share it
        if shared:
            add("shared_tile", [shared[len(shared) // 2]])
        add("decoys", [mid])
        add("all_negative", [mid + 1 if mid + 1 < hi - 1 else mid])
        add("flat", range(lo, hi))
        # two equal maxima in one tile: the tile that holds the most ids of the range, the two away from its ends where it has room
        t0 = mid_tile if h == 0 else max(range(first_tile, last_tile + 1), key=lambda t: min(hi, t * 16 + 16) - max(lo, t * 16))
        inside = [n for n in range(t0 * 16, t0 * 16 + 16) if lo <= n < hi]
        add("tie_same_tile", [inside[1], inside[-2]] if len(inside) > 3 else [inside[0], inside[-1]])
        # two tiles of one wave
        if last_tile > first_tile:
            i = first_tile if h else 3
            j = i + 1 if h else min(40, last_tile - 1)
            if wave_of(i * 16) == wave_of(j * 16):
                add("tie_same_wave", [max(lo, i * 16 + 9), min(hi - 1, j * 16 + 2)])
        if h == 0 and last_tile >= 130:
            add("tie_other_wave", [5 * 16 + 3, 130 * 16 + 12])                        # waves 0 and 2
            add("tie_wave_order", [100 * 16 + 7, 270 * 16 + 1])                       # the lower id sits in wave 1, the higher in wave 0's second pass
        if h == 0 and last_tile >= 256 + 20:
            add("tie_same_thread", [9 * 16 + 15, (9 + 256) * 16])                     # tiles i and i + 256: one thread reads both
            add("tie3_thread_wave", [20 * 16 + 4, 200 * 16 + 4, (20 + 256) * 16 + 4], "tie3")
        if last_tile > first_tile:
            i = first_tile if h else 7
            add("tie3_tile_wave", [max(lo, i * 16 + 8), max(lo, i * 16 + 8) + 2, min(hi - 1, (i + 1) * 16 + 5)], "tie3")
        else:
            add("tie3_tile", [lo + 2, lo + 5, lo + 9], "tie3")
    return specs


def build_table(cfg, seed=0):
    """(T int16 [NV, NVpad], Plan).  Row t is what feeding token t leaves in the logits, in units of s / 16; the pad columns NV .. NVpad - 1 are
    zero as the engine's padded head rows are, and so are the rows of text ids that own no column.

    Ordinary rows: values in [-40, 8] and one 20 per head, at (7 t + 3) mod (V + 1), lo + (5 t + 2) mod Tv, lo + (5 t + 4) mod Sv: neighbouring
    tokens differ in every head, so a gather from the wrong table row shows as the wrong id."""
    V, Tv, Sv, NV, NVpad = dims(cfg)
    rng = np.random.default_rng(seed)
    T = np.zeros((NV, NVpad), np.int16)
    toks = tokens_with_columns(cfg)
    T[toks, :NV] = rng.integers(-40, T_BASE_HI + 1, size=(len(toks), NV))
    T[toks, (7 * toks + 3) % (V + 1)] = T_TIE
    T[toks, V + 1 + (5 * toks + 2) % Tv] = T_TIE
    T[toks, V + 1 + Tv + (5 * toks + 4) % Sv] = T_TIE

    def set_unique_max(t, h, target):
        lo, hi = head_range(cfg, h)
        T[t, lo:hi] = np.minimum(T[t, lo:hi], T_BASE_HI)
        T[t, target] = T_TIE

    # reserved text tokens (below 320: both geometries have them)
    chain_text = [250, 255, 260, 265]
    eos, eos_emitter = 300, 305
    fillers = [t for t in range(270, 290) if (7 * t + 3) % (V + 1) not in (eos, V)]
    reserved = set(chain_text) | {eos, eos_emitter} | set(fillers)
    # the free-running chain: text, text, text, <sync>, time, time, first time id, score, score, first score id, text, and round again
    c0, c1, c2, c3 = chain_text
    tm, sc = V + 1, V + 1 + Tv
    chain = [(c0, 0), (c1, 0), (c2, 0), (V, 1), (tm + 5, 1), (tm + 7, 1), (tm, 2), (sc + 4, 2), (sc + 9, 2), (sc, 0), (c3, 0)]
    for i, (t, h) in enumerate(chain):
        set_unique_max(t, h, chain[(i + 1) % len(chain)][0])
    set_unique_max(eos_emitter, 0, eos)
    for t in toks:                                   # nothing but the emitter emits eos under head 0
        if t != eos_emitter and T[t, eos] == T_TIE:
            set_unique_max(int(t), 0, (eos + 1))

    specs = _case_specs(cfg)
    pool = [t for t in range(3, text_cols(cfg)) if t not in reserved]
    stride = len(pool) // (len(specs) + 1)
    cases = []
    for i, (name, h, ties, kind) in enumerate(specs):
        t = pool[(i + 1) * stride]
        lo, hi = head_range(cfg, h)
        row = np.zeros(NVpad, np.int16)
        row[:NV] = rng.integers(-40, T_BASE_HI + 1, size=NV)
        top = T_TIE
        if kind == "all_negative":
            row[:NV] = rng.integers(1, 41, size=NV)
            row[lo:hi] = rng.integers(-40, -4, size=hi - lo)
            top = -1
        elif kind == "flat":
            top = 7
        row[list(ties)] = top
        # decoys larger than every in-range value: just outside the range and inside every other head
        decoys = [n for n in (lo - 1, hi) if 0 <= n < NV]
        for g in range(3):
            if g != h:
                glo, ghi = head_range(cfg, g)
                decoys += [glo, ghi - 1, int(rng.integers(glo, ghi))]
        decoys = tuple(sorted(set(decoys)))
        row[list(decoys)] = T_DECOY
        T[t] = row
        cases.append(Case(name, h, t, ties, kind, decoys))
    assert T.min() >= -64 and T.max() <= 64
    return T, Plan(cases, chain, eos, eos_emitter, fillers)


def check_case(T, cfg, case):
    """the property a named case claims, in integers; raises AssertionError with the case's name"""
    V, Tv, Sv, NV, NVpad = dims(cfg)
    lo, hi = head_range(cfg, case.head)
    row = T[case.token].astype(np.int64)
    ties = np.array(case.ties)
    name = case.name
    assert ((ties >= lo) & (ties < hi)).all(), name
    m = row[lo:hi].max()
    assert sorted(lo + np.nonzero(row[lo:hi] == m)[0]) == sorted(case.ties), f"{name}: the in-range maximum is not held by exactly the ids named"
    assert (row[NV:] == 0).all(), f"{name}: pad columns"
    assert len(case.decoys) >= 3 and all((n < lo or n >= hi) and row[n] > m for n in case.decoys), f"{name}: decoys"
    if lo > 0:
        assert lo - 1 in case.decoys, name
    if hi < NV:
        assert hi in case.decoys, name
    for g in range(3):
        if g != case.head:
            glo, ghi = head_range(cfg, g)
            assert any(glo <= n < ghi for n in case.decoys), f"{name}: no decoy in head {g}"
    k = case.kind
    t = [tile_of(n) for n in case.ties]
    if k == "unique_lo":
        assert case.ties == (lo,)
    elif k == "unique_hi_1":
        assert case.ties == (hi - 1,)
    elif k == "tile_first":
        assert len(ties) == 1 and ties[0] % 16 == 0 and ties[0] != lo
    elif k == "tile_last":
        assert len(ties) == 1 and ties[0] % 16 == 15 and ties[0] != hi - 1
    elif k == "shared_tile":
        assert len(ties) == 1 and tile_of(ties[0]) == tile_of(V)
    elif k == "decoys":
        assert len(ties) == 1
    elif k == "all_negative":
        out = np.concatenate([row[:lo], row[hi:NV]])
        assert m < 0 and (out > 0).all() and len(ties) == 1, name
        if hi == NV and NVpad > NV:
            assert (row[NV:] > m).all(), name                       # head 2: the zero pad rows beat every in-range value
    elif k == "flat":
        assert case.ties == tuple(range(lo, hi))
    elif k == "tie_same_tile":
        assert len(ties) == 2 and t[0] == t[1]
    elif k == "tie_same_wave":
        assert len(ties) == 2 and t[0] != t[1] and wave_of(ties[0]) == wave_of(ties[1]) and thread_of(ties[0]) != thread_of(ties[1])
    elif k == "tie_other_wave":
        assert len(ties) == 2 and wave_of(ties[0]) != wave_of(ties[1]) and t[0] < 256 and t[1] < 256
    elif k == "tie_wave_order":
        assert len(ties) == 2 and wave_of(min(ties)) > wave_of(max(ties)), name
    elif k == "tie_same_thread":
        assert len(ties) == 2 and t[1] == t[0] + 256
    elif k == "tie3":
        assert len(ties) == 3
        rel = {pair_relation(a, b) for i, a in enumerate(case.ties) for b in case.ties[i + 1:]}
        assert len(rel) >= 2 or hi - lo <= 16, f"{name}: a three-way tie has to mix two relations, has {rel}"
    else:
        raise AssertionError(f"{name}: unknown kind {k}")


# ---- the weights ----------------------------------------------------------------------------------------------------------------------------
def crafted_weights(cfg, table, dtype=torch.bfloat16):
    """ordinary synthetic weights with zero o_proj / down_proj, a unit final norm, one-hot embeddings and head rows T / 16"""
    V, Tv, Sv, NV, _ = dims(cfg)
    assert cfg.hidden_size == HIDDEN and text_cols(cfg) + 1 + Tv + Sv <= HIDDEN
    sd = synth.state_dict(cfg, dtype)
    for k in sd:
        if k.endswith("self_attn.o_proj.weight") or k.endswith("mlp.down_proj.weight"):
            sd[k] = torch.zeros_like(sd[k])
    sd["model.norm.weight"] = torch.ones(HIDDEN, dtype=dtype)
    toks = tokens_with_columns(cfg)
    cols = np.array([column(cfg, int(t)) for t in toks])
    emb = torch.zeros((NV, HIDDEN), dtype=dtype)
    emb[torch.from_numpy(toks), torch.from_numpy(cols)] = 1
    W = torch.zeros((NV, HIDDEN), dtype=torch.float32)
    W[:, torch.from_numpy(cols)] = torch.from_numpy(table[toks, :NV].astype(np.float32).T.copy()) / 16.0
    W = W.to(dtype)
    sd["model.embed_tokens.weight"], sd["lm_head.weight"] = emb[:V].clone(), W[:V].clone()
    sd["model.sync_tower.embed_tokens.weight"], sd["sync_head.weight"] = emb[V:V + 1].clone(), W[V:V + 1].clone()
    sd["model.time_tower.embed_tokens.weight"], sd["time_head.weight"] = emb[V + 1:V + 1 + Tv].clone(), W[V + 1:V + 1 + Tv].clone()
    sd["model.score_tower.embed_tokens.weight"], sd["score_head.weight"] = emb[V + 1 + Tv:].clone(), W[V + 1 + Tv:].clone()
    return sd


def embedding_row(cfg, token, dtype=torch.bfloat16):
    """the crafted embedding of one token: what the last prompt row holds once the prompt's last id is replaced by `token`"""
    e = torch.zeros(HIDDEN, dtype=dtype)
    c = column(cfg, int(token))
    if c is not None:
        e[c] = 1
    return e


def logit_scale(cfg, dtype=torch.bfloat16):
    """the logits are exactly logit_scale * T: the 16-bit rounding of rsqrt(1 / 4096 + eps), over 16 (3.921875 in bf16)"""
    s = torch.rsqrt(torch.tensor(1.0 / HIDDEN + cfg.rms_norm_eps, dtype=torch.float32)).to(dtype).float()
    return float(s) / 16.0


# ---- the rules, restated ----------------------------------------------------------------------------------------------------------------------
def select(row, lo, hi, mutant=None):
    """lowest-id arg-max of row over [lo, hi)"""
    n = np.arange(lo, hi)
    if mutant == "tiles_from_256_ignored":
        n = n[n // 16 < 256]
    elif mutant == "first_wave_only":
        n = n[(n // 16) % 256 < 64]
    if len(n) == 0:
        return -1
    v = row[n]
    best = n[v == v.max()]
    return int(best[-1] if mutant == "highest_id_wins_tie" else best[0])


def restate(table, cfg, start_token, head, forced, eos, max_new, mutant=None, trace=None):
    """(ids, length, final_head) of one row, by the rules of select_next_kernel and trace_mistral.py:86-88.  forced: max_new ints, -1 = not forced.
    mutant: one rule broken on purpose (MUTANTS) — the CPU tests use it to show that the case lists tell the rules from their near misses.
    trace: a list that receives (state, head, tok) per step."""
    V, Tv, Sv, NV, NVpad = dims(cfg)
    assert mutant is None or mutant in MUTANTS
    state, ids, length, done = int(start_token), [], 0, False
    for s in range(max_new):
        r = state
        if mutant == "time_row_off_by_one" and V < state < V + 1 + Tv:
            r = min(state + 1, V + Tv)
        lo, hi = head_range(cfg, head)
        if mutant == "lo_one_low":
            lo = max(lo - 1, 0)
        elif mutant == "hi_one_high":
            hi = min(hi + 1, NVpad)
        elif mutant == "no_mask":
            lo, hi = 0, NV
        tok = select(table[r], lo, hi, mutant)
        if trace is not None:
            trace.append((state, head, tok))
        feed = int(forced[s]) if forced[s] >= 0 else tok
        if not done or mutant == "done_keeps_recording":
            ids.append(tok)
            length = s + 1
        if eos >= 0 and tok == eos:
            done = True
        sw = tok if mutant == "switch_on_tok" else feed
        if mutant != "switch_dropped":
            head = {V: 1, V + 1: 2, V + Tv + 1: 0}.get(sw, head)
        state = feed
    return ids, length, head


# ---- the rows of a batch ------------------------------------------------------------------------------------------------------------------------
SPECIAL_ROWS = (0, 15, 16, 31, 32)            # with B - 1: the first and last row of head_logits_kernel's two 16-row halves and of its second launch


def tour_states(cfg, plan, r):
    """[(state, head it is read under)] a teacher-forced row visits, cyclic: from head r % 3 on, per head every named case (rotated by r), then
    time and score ids (table rows other than the first, the last ones included), then the token that switches to the next head"""
    V, Tv, Sv, NV, _ = dims(cfg)
    out = []
    for k in range(3):
        h = (r + k) % 3
        cs = plan.by_head(h)
        rot = r % len(cs)
        seg = [c.token for c in cs[rot:] + cs[:rot]]
        if h == 1:
            seg += [V + 1 + 3, V + Tv, V + 1 + 8]
        elif h == 2:
            seg += [V + 1 + Tv + 2, NV - 1, V + 1 + Tv + 11]
        else:
            seg += [plan.fillers[r % len(plan.fillers)]]
        if k:
            seg = [switch_token(cfg, h)] + seg               # (the row reads the switch token's own table row under the new head)
        out += [(t, h) for t in seg]
    return out + [(switch_token(cfg, r % 3), r % 3)]


def tour_length(cfg, plan):
    return len(tour_states(cfg, plan, 0))


def batch_rows(cfg, plan, B, max_new):
    """[(start token, start head, forced[max_new])] for a batch of B rows.  Rows 0, 15, 16, 31, 32 and B - 1 and two of every four others are
    teacher-forced along tour_states, each from another point of its tour (a tour is cyclic and max_new covers all of it, so every such row
    passes every named case); the others run free (forced = -1) along the chain, each from another point of it."""
    rows = []
    for r in range(B):
        if r in SPECIAL_ROWS or r == B - 1 or r % 4 < 2:
            st = tour_states(cfg, plan, r)
            off = (r * 5) % len(st)
            st = [st[(off + i) % len(st)] for i in range(max_new + 1)]
            rows.append((st[0][0], st[0][1], [t for t, _ in st[1:]]))
        else:
            t, h = plan.chain[(r * 3) % len(plan.chain)]
            rows.append((t, h, [-1] * max_new))
    return rows


def eos_rows(cfg, plan, B, max_new):
    """rows for the EOS test (eos = plan.eos, all under head 0 at first): row r of the first five emits EOS at step 0, 1, max_new // 2, max_new - 1
    and never; it is fed on afterwards, switch tokens included (the head of a finished row keeps switching).  Further rows: batch_rows."""
    V = cfg.vocab_size
    fin = [0, 1, max_new // 2, max_new - 1, None]
    rows = []
    for r, at in enumerate(fin[:B]):
        st = [plan.fillers[(r + i) % len(plan.fillers)] for i in range(max_new + 1)]
        if at is not None:
            st[at] = plan.eos_emitter
        for i in (3, max_new // 2 + 2, max_new - 2):          # a switch to the time head and straight back: the row stays under head 0 where it counts
            if 0 < i < max_new - 1 and plan.eos_emitter not in st[i - 1:i + 3]:
                st[i], st[i + 1] = V, switch_token(cfg, 0)
        if r == 1:
            st[max_new] = V                                      # the last feed of a finished row switches its head
        rows.append((st[0], 0, st[1:]))
    rows += batch_rows(cfg, plan, B, max_new)[len(rows):]
    return rows, fin[:B]


def restate_batch(table, cfg, rows, eos, max_new, mutant=None):
    """([ids], [length], [final head]) of batch_rows / eos_rows"""
    out = [restate(table, cfg, t, h, f, eos, max_new, mutant) for t, h, f in rows]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


# ---- the batches the device tests run (the CPU tests hold the same lists up against the mutants) ------------------------------------------------
BATCHES = {"small": (1, 16, 17, 32, 33, 100, 256), "big": (1, 33, 100)}
GEOMETRIES = {"small": small, "big": big}
EOS_BATCH = 9


def max_new_for(cfg, plan):
    """long enough for a teacher-forced row to pass every named case of all three heads and to come back to its first head"""
    return tour_length(cfg, plan) + 2
