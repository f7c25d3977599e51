"""Host helpers for scoring GIVEN continuations (TraceEngine.score_continuations, TraceMistralForCausalLM.score; the semantics are stated in
include/trace_hip.h at trace_llm_score_append).  Nothing here touches the device.

A continuation is a list of global vocabulary ids over [text | <sync> | time | score] and the head active for its first id.  Position i is
predicted by the hidden row that precedes it: the last prompt row for i = 0, the row fed with the embedding of c[i - 1] otherwise, under the head
the decode step would be in after the FED ids c[0 .. i) — `head_chain`.  `embed_placeholders` maps ids to what trace_embed_rows takes, which is
the decode branch's embedding rule (the oracle's decode_embed)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

SYNC_PLACEHOLDER, TIME_PLACEHOLDER, SCORE_PLACEHOLDER = -205, -203, -204      # trace_amd.constants / trace_splice_embeds
IGNORE = -1                                                                  # target id of a padding row: its log-probability is 0.0


def swap(cfg, token: int, head: int) -> int:
    """the head after feeding `token` under `head` (select_next_kernel's switch, trace_mistral.py:86-88)"""
    V, Tv = cfg.vocab_size, cfg.time_vocab_size
    token = int(token)
    return 1 if token == V else 2 if token == V + 1 else 0 if token == V + Tv + 1 else int(head)


def head_chain(cfg, ids: Sequence[int], head: int = 1) -> List[int]:
    """head[i] = the head that c[i] is drawn from: head[0] = `head`, head[i + 1] = swap(c[i], head[i])"""
    out, h = [], int(head)
    for t in ids:
        out.append(h)
        h = swap(cfg, t, h)
    return out


def check_continuation(cfg, ids: Sequence[int], head: int) -> List[int]:
    ids = [int(t) for t in ids]
    if int(head) not in (0, 1, 2):
        raise ValueError(f"head must be 0 (text), 1 (time) or 2 (score), got {head}")
    if not ids:
        raise ValueError("an empty continuation has nothing to score")
    nv = cfg.vocab_size + 1 + cfg.time_vocab_size + cfg.score_vocab_size
    bad = [t for t in ids if not 0 <= t < nv]
    if bad:
        raise ValueError(f"continuation ids must be global vocabulary ids in [0, {nv}), got {bad[:4]}")
    return ids


def embed_placeholders(cfg, ids: Sequence[int]) -> Tuple[List[int], List[int], List[int]]:
    """global ids -> (ids with placeholders, time tower rows, score tower rows) for TraceEngine.embed_rows: text ids stay, <sync> becomes its
    placeholder, a time / score id its placeholder plus the tower row it names — the embedding the decode step gathers for a fed id"""
    V, Tv = cfg.vocab_size, cfg.time_vocab_size
    out, tr, sr = [], [], []
    for t in ids:
        t = int(t)
        if t < V:
            out.append(t)
        elif t == V:
            out.append(SYNC_PLACEHOLDER)
        elif t < V + 1 + Tv:
            out.append(TIME_PLACEHOLDER)
            tr.append(t - V - 1)
        else:
            out.append(SCORE_PLACEHOLDER)
            sr.append(t - V - 1 - Tv)
    return out, tr, sr


def fed_ids(ids: Sequence[int], L: int, pad_id: int = 0) -> List[int]:
    """the ids whose embeddings follow the last prompt row in a continuation's L appended rows: c[0 .. n - 1) and padding (any text id: the
    padding comes after the real rows, so causality keeps it from touching them)"""
    ids = list(ids)
    return ids[:-1] + [int(pad_id)] * (L - len(ids))


def targets(ids: Sequence[int], heads: Sequence[int], L: int) -> Tuple[List[int], List[int]]:
    """(target ids, heads) of the L appended rows: the continuation, then IGNORE under the text head"""
    ids, heads = list(ids), list(heads)
    return ids + [IGNORE] * (L - len(ids)), heads + [0] * (L - len(ids))


def groups_of(lengths: Sequence[int], rows_cap: int, group_max: int = 8) -> List[List[int]]:
    """continuation indices in runs of at most group_max, in order, each run's padded size (run length x its longest member) within rows_cap"""
    out, cur, longest = [], [], 0
    for i, n in enumerate(lengths):
        if n > rows_cap:
            raise ValueError(f"a continuation of {n} tokens exceeds the prefill workspace ({rows_cap} rows)")
        if cur and (len(cur) == group_max or (len(cur) + 1) * max(longest, n) > rows_cap):
            out.append(cur)
            cur, longest = [], 0
        cur.append(i)
        longest = max(longest, n)
    if cur:
        out.append(cur)
    return out


@dataclass
class ScoreResult:
    """logprobs[b]: float32 per token of continuation b; heads[b]: the head each token was scored under; scores[b]: the float64 sum;
    order: continuation indices by descending score, ties to the lower index"""
    logprobs: List[np.ndarray]
    heads: List[List[int]]
    scores: np.ndarray
    order: List[int]
