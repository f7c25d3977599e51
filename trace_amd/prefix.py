"""Host-side bookkeeping of prompt-prefix reuse (no torch, no device): where a prompt is cut, which prompts share a prefix, and how the
suffixes are grouped for trace_llm_prefill_append.  The reference's per-question drivers (trace/eval/videomme/evaluate.py:349-386) call
generate once per question with one video and prompts identical through `<video>`; the engine prefills those rows once."""
from __future__ import annotations

from typing import List, Sequence, Tuple

from .constants import MMODAL_TOKEN_INDEX

VIDEO_IDS = (MMODAL_TOKEN_INDEX["VIDEO"], MMODAL_TOKEN_INDEX["IMAGE"])      # both expand to the encoded rows (trace_splice_embeds)
APPEND_GROUP_MAX = 8                                                        # slots one trace_llm_prefill_append call takes


def split_prompt(ids: Sequence[int]) -> Tuple[List[int], List[int]]:
    """(prefix, suffix): the ids through the single video placeholder, and the ids after it (possibly none).
    ValueError unless the prompt holds exactly one placeholder — the rule of trace_splice_embeds (trace_arch.py:411)."""
    ids = [int(x) for x in ids]
    at = [i for i, x in enumerate(ids) if x in VIDEO_IDS]
    if len(at) != 1:
        raise ValueError(f"a prompt must hold exactly one video placeholder, found {len(at)}")
    return ids[: at[0] + 1], ids[at[0] + 1:]


def split_questions(prompts: Sequence[Sequence[int]]) -> Tuple[List[int], List[List[int]]]:
    """(the common prefix, one suffix per prompt) of prompts that agree up to and including their video placeholder.
    ValueError when a prompt has no / several placeholders or two prompts disagree inside the prefix."""
    if not prompts:
        raise ValueError("no prompts")
    parts = [split_prompt(p) for p in prompts]
    prefix = parts[0][0]
    for q, (p, _) in enumerate(parts):
        if p != prefix:
            raise ValueError(f"prompt {q} differs from prompt 0 before or at the video placeholder: no common prefix to share")
    return prefix, [s for _, s in parts]


def group_by_length(lengths: Sequence[int], max_group: int = APPEND_GROUP_MAX) -> List[Tuple[int, List[int]]]:
    """[(length, [prompt indices])]: the prompts grouped by suffix length, at most `max_group` per group, lengths in order of first
    appearance and indices ascending inside a group (one trace_llm_prefill_append call per group, over consecutive slots)."""
    if max_group < 1:
        raise ValueError("max_group must be at least 1")
    by_len = {}
    for i, n in enumerate(lengths):
        by_len.setdefault(int(n), []).append(i)
    out = []
    for n, idx in by_len.items():
        for o in range(0, len(idx), max_group):
            out.append((n, idx[o:o + max_group]))
    return out
