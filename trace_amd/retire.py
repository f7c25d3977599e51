"""When retiring finished rows from a running decode batch is worth its gather (no torch, no device).  decode_loop.decode_loop asks retire_plan at
every chunk boundary, with the ids it has read back; RowBook, below, keeps which rows stay, the results of the rows that left, and the order in
which everything comes back.  tests/test_retire_host.py runs that loop on a scripted device."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

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


class RowBook:
    """The rows of a decode batch that requests enter and leave.  rows: the request index of every live row, in batch order (position i of the
    running batch decodes request rows[i]); slots: the KV slot of every live row; free: the KV slots no live row holds, lowest first.  history: rows
    after every begin, retire and admit.  Results of rows that left wait in a stash until results() / columns()."""

    def __init__(self, slots: Sequence[int], logprobs: bool = False):
        slots = [int(s) for s in slots]
        if not slots or len(set(slots)) != len(slots) or min(slots) < 0:
            raise ValueError("slots must be a non-empty list of distinct KV slots")
        self.free: List[int] = sorted(slots)
        self.rows: List[int] = []
        self.slots: List[int] = []
        self.history: List[List[int]] = []
        self.logprobs = bool(logprobs)
        self.requests = 0                              # requests that entered so far: the next one's index
        self.retires = 0
        self.admits = 0
        self._out: Dict[int, tuple] = {}

    def admit(self, n: int) -> List[int]:
        """the next n requests (indices self.requests ..) enter behind the live rows, each into the lowest free KV slot: returns their slots, in
        order.  On an empty batch this is the begin of a batch."""
        n = int(n)
        if n < 1 or n > len(self.free):
            raise ValueError(f"{n} requests for {len(self.free)} free KV slots")
        took, self.free = self.free[:n], self.free[n:]
        if self.rows:
            self.admits += 1
        self.rows += list(range(self.requests, self.requests + n))
        self.slots += took
        self.requests += n
        self.history.append(list(self.rows))
        return took

    def _leave(self, gone, ids, heads, lps):
        if len(ids) != len(self.rows) or len(heads) != len(self.rows) or (self.logprobs and (lps is None or len(lps) != len(self.rows))):
            raise ValueError("one read-back entry per live row")
        for i in gone:
            self._out[self.rows[i]] = (list(ids[i]), int(heads[i]), lps[i] if self.logprobs else None)
            self.free.append(self.slots[i])
        self.free.sort()

    def keep_list(self, finished: Sequence[bool]) -> List[int]:
        """positions (in the running batch) of the rows that are not finished: strictly increasing"""
        if len(finished) != len(self.rows):
            raise ValueError(f"{len(finished)} flags for {len(self.rows)} live rows")
        return [i for i, f in enumerate(finished) if not f]

    def retire(self, keep: Sequence[int], ids: Sequence[Sequence[int]], heads: Sequence[int], lps: Optional[Sequence] = None) -> None:
        """the running batch shrinks to positions `keep` (non-empty: the device keeps one row at least); ids / heads / lps (one entry per live row,
        as read back) of the others are stashed and their KV slots become free"""
        keep = [int(k) for k in keep]
        n = len(self.rows)
        if not keep or any(k < 0 or k >= n for k in keep) or any(b <= a for a, b in zip(keep, keep[1:])):
            raise ValueError("keep must be a non-empty, strictly increasing list of live positions")
        self._leave(sorted(set(range(n)) - set(keep)), ids, heads, lps)
        self.rows = [self.rows[k] for k in keep]
        self.slots = [self.slots[k] for k in keep]
        self.retires += 1
        self.history.append(list(self.rows))

    def finish(self, ids: Sequence[Sequence[int]], heads: Sequence[int], lps: Optional[Sequence] = None) -> None:
        """every live row leaves (the batch ended): its results join the stash and every KV slot is free again"""
        self._leave(range(len(self.rows)), ids, heads, lps)
        self.rows, self.slots = [], []

    def results(self):
        """one (ids, head[, logprobs]) per request that entered, in request order; every row must have left (finish)"""
        if self.rows or len(self._out) != self.requests:
            raise ValueError(f"{len(self.rows)} rows are still live" if self.rows else "a request has no result")
        out = [self._out[r] for r in range(self.requests)]
        return [o if self.logprobs else o[:2] for o in out]

    def columns(self):
        """results() by column: (ids, heads[, logprobs]) of all rows in their original order, as a batch's read-back has them"""
        return tuple(list(c) for c in zip(*self.results()))


# Not a second class: the name under which tests/test_retire_host.py of the commit before this class imports it at module level.  Without
# it that module cannot be imported at all and its tests of the plan rule and the header go down with the ones that used the old book.
RetireBook = RowBook
