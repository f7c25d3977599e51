"""Host-side bookkeeping of prompt-prefix reuse (no torch, no device): where a prompt is cut, which prompts share a prefix, and how the
suffixes are grouped for trace_llm_prefill_append.  The reference's per-question drivers (trace/eval/videomme/evaluate.py:349-386) call
generate once per question with one video and prompts identical through `<video>`; the engine prefills those rows once."""
from __future__ import annotations

from typing import List, Sequence, Tuple

from .constants import MMODAL_TOKEN_INDEX

VIDEO_IDS = (MMODAL_TOKEN_INDEX["VIDEO"], MMODAL_TOKEN_INDEX["IMAGE"])      # both expand to the encoded rows (trace_splice_embeds)
APPEND_GROUP_MAX = 8                                                        # slots one trace_llm_prefill_append call takes
# Smallest batch whose common prompt rows are prefilled once and shared (TraceEngine.share_prefix_min_batch).  Sharing P rows saves (B - 1) x P prefill
# rows (about 0.9 ms per video at P = 150 on the 7B decoder) for one P-row prefill on its own (about 15 ms, a launch-bound pass) and one copy of the rows
# into every slot: break-even near 16 - 20 videos.
SHARE_PREFIX_MIN_BATCH = 32


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


def shared_prefix_len(prompts: Sequence[Sequence[int]]) -> int:
    """Rows a batch shares before the video: P, the number of ids in front of the first prompt's video placeholder, if EVERY prompt has those
    same P ids followed by its placeholder (one question put to every video — the evaluation loops); otherwise 0, the batch shares nothing.
    Those ids are plain embedding rows, the same in every prompt, and the decoder is causal: their K / V rows are the same bits for every
    sequence.  What follows the placeholder may differ.  0 as well for an empty batch, a prompt without a placeholder, or a placeholder in
    front; a single prompt "shares" its own P rows (the caller decides whether one prompt is a batch)."""
    prompts = [[int(x) for x in p] for p in prompts]
    if not prompts:
        return 0
    first = prompts[0]
    at = next((i for i, x in enumerate(first) if x in VIDEO_IDS), None)
    if at is None or any(p[: at + 1] != first[: at + 1] for p in prompts):
        return 0
    return at
