"""Host-side bookkeeping of retiring finished rows from a running decode batch (no torch, no device): when a retire is worth its gather, which rows
stay, where the results of the rows that left are kept, and how the batch's result is put back in its original order.  TraceEngine._decode drives it
with the ids it reads back at every chunk boundary; tests/test_retire_host.py drives it with scripted read-backs."""
from __future__ import annotations

from typing import List, Optional, Sequence

# Retire when at least 1 / RETIRE_FRACTION of the rows of the running batch have finished since the last retire (at least one row).  A retire costs
# one gather and, the first time a process meets a batch size, one graph capture; it saves the finished rows' share of every later step.  Measured
# (profiles/retire_ab.txt, synthetic 7B, context 1968, batch 128): a retire 0.09 ms, a capture about 1 ms, against about 1 ms per step that sixteen rows
# fewer save at that width, so a retire at this threshold is repaid within two steps; the profile whose rows all end in the last chunk runs within the
# run-to-run spread of the flag off (-1.7 ms in a 4.8 ms spread on a 2.8 s call).  The starting value stays: a smaller denominator gives up savings
# between retires, a larger one captures more batch sizes for less gain each.
RETIRE_FRACTION = 8


def retire_plan(B_now: int, live: int, fraction: int = RETIRE_FRACTION) -> bool:
    """Retire now?  B_now rows run, `live` of them are unfinished.  Never when nothing has finished; always allowed when nothing is left.
    fraction: the denominator of the rule (TraceEngine.retire_fraction; a value above B_now retires as soon as one row has finished)."""
    finished = int(B_now) - int(live)
    if finished <= 0:
        return False
    return live <= 0 or finished >= max(1, int(B_now) // max(1, int(fraction)))


class RetireBook:
    """The rows of one decode batch across its retires.  rows: the original index of every live row, in batch order (position i of the running batch
    is original row rows[i]).  history: rows after begin and after every retire.  Results of retired rows wait in a stash until result()."""

    def __init__(self, B: int, logprobs: bool = False):
        self.B0 = int(B)
        self.rows: List[int] = list(range(self.B0))
        self.history: List[List[int]] = [list(self.rows)]
        self.logprobs = bool(logprobs)
        self._ids: List[Optional[list]] = [None] * self.B0
        self._heads: List[Optional[int]] = [None] * self.B0
        self._lps: List[Optional[object]] = [None] * self.B0

    @property
    def retires(self) -> int:
        return len(self.history) - 1

    def keep_list(self, finished: Sequence[bool]) -> List[int]:
        """positions (in the running batch) of the rows that are not finished: strictly increasing"""
        if len(finished) != len(self.rows):
            raise ValueError(f"{len(finished)} flags for {len(self.rows)} live rows")
        return [i for i, f in enumerate(finished) if not f]

    def retire(self, keep: Sequence[int], ids: Sequence[Sequence[int]], heads: Sequence[int], lps: Optional[Sequence] = None) -> None:
        """the running batch shrinks to positions `keep`; ids / heads / lps (one entry per live row, as read back) of the others are stashed"""
        keep = [int(k) for k in keep]
        n = len(self.rows)
        if len(ids) != n or len(heads) != n or (self.logprobs and (lps is None or len(lps) != n)):
            raise ValueError("one read-back entry per live row")
        if not keep or any(k < 0 or k >= n for k in keep) or any(b <= a for a, b in zip(keep, keep[1:])):
            raise ValueError("keep must be a non-empty, strictly increasing list of live positions")
        kept = set(keep)
        for i in range(n):
            if i not in kept:
                self._put(self.rows[i], ids[i], heads[i], lps[i] if self.logprobs else None)
        self.rows = [self.rows[k] for k in keep]
        self.history.append(list(self.rows))

    def _put(self, r, ids, head, lp):
        self._ids[r], self._heads[r], self._lps[r] = list(ids), int(head), lp

    def result(self, ids: Sequence[Sequence[int]], heads: Sequence[int], lps: Optional[Sequence] = None):
        """the final read-back of the live rows joins the stash: (ids, heads[, lps]) of all B0 rows in their original order"""
        n = len(self.rows)
        if len(ids) != n or len(heads) != n or (self.logprobs and (lps is None or len(lps) != n)):
            raise ValueError("one read-back entry per live row")
        for i, r in enumerate(self.rows):
            self._put(r, ids[i], heads[i], lps[i] if self.logprobs else None)
        assert all(x is not None for x in self._ids)
        return (self._ids, self._heads, self._lps) if self.logprobs else (self._ids, self._heads)
