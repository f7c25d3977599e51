"""Host-side bookkeeping of continuous batching (no torch, no device): when the room that retired rows left in a running decode batch is worth
admitting waiting requests into, which request sits at which position of the batch and in which KV slot, where the results of the rows that
left are kept, and how everything comes back in request order.  TraceEngine.generate_queue drives it with the ids it reads back at every chunk
boundary; tests/test_admit_host.py drives it with scripted read-backs.  It extends retire.RetireBook's idea: there the batch only shrinks, here
positions are appended behind the live ones (trace_decode_admit) and KV slots are recycled."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

from .retire import RETIRE_FRACTION

# Admit once the room in the batch (rows below the cap for which a KV slot is free) is at least cap // ADMIT_FRACTION rows, or as soon as the batch
# would otherwise be empty.  An admission costs the encode and prefill of the new rows (which a fixed batch pays too), one admit call and, the first
# time a process meets the new batch size, one graph capture; it saves the steps that a later batch would have run for those rows beside a thin
# batch's weight stream.  The starting value is the retire rule's denominator: retire and admit then trigger at the same boundaries of a full batch
# (a retire of cap // 8 rows makes exactly the room an admission waits for), so a batch moves between two sizes per exchange instead of capturing one
# graph per row that left.  Measured (profiles/admit_ab.txt, synthetic 7B, context 1968, 256 requests through 128 rows, chunk 32): an admission of 16 rows
# 0.22 ms and at most one capture of about 1 ms, against about 1 ms per step that sixteen rows change at that width; denominators 4, 8 and 32 gave the
# same schedule (10 retires, 3 admits) and the same 0.78 x against two fixed batches, because with answers of mean length 56 the room after a chunk
# is far above any of them.  The threshold matters only for a batch that loses a few rows per chunk; the starting value stays.
ADMIT_FRACTION = RETIRE_FRACTION


def admit_plan(B_now: int, cap: int, waiting: int, free_slots: int, fraction: int = ADMIT_FRACTION) -> int:
    """How many waiting requests to admit at this chunk boundary.  B_now rows run (after this boundary's retire), the batch may hold `cap`, `waiting`
    requests wait and `free_slots` KV slots are free.  0 when nothing waits, no slot is free or the cap is reached; 0 while the room is below
    max(1, cap // fraction) rows, unless the batch is empty (B_now == 0): then whatever fits is admitted.  Otherwise min(room, waiting)."""
    B_now, cap, waiting, free_slots = int(B_now), int(cap), int(waiting), int(free_slots)
    room = min(cap - B_now, free_slots)
    if waiting <= 0 or room <= 0:
        return 0
    if B_now > 0 and room < max(1, cap // max(1, int(fraction))):
        return 0
    return min(room, waiting)


class QueueBook:
    """The rows of a decode batch that requests enter and leave.  rows: the request index of every live row, in batch order (position i of the
    running batch decodes request rows[i]); slots: the KV slot of every live row; free: the KV slots no live row holds, lowest first.  history: rows
    after every begin, retire and admit.  Results of rows that left wait in a stash until results()."""

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

    def _check(self, ids, heads, lps):
        n = len(self.rows)
        if len(ids) != n or len(heads) != n or (self.logprobs and (lps is None or len(lps) != n)):
            raise ValueError("one read-back entry per live row")

    def _put(self, i, ids, heads, lps):
        self._out[self.rows[i]] = (list(ids[i]), int(heads[i]), lps[i] if self.logprobs else None)
        self.free.append(self.slots[i])

    def keep_list(self, finished: Sequence[bool]) -> List[int]:
        """positions (in the running batch) of the rows that are not finished: strictly increasing"""
        if len(finished) != len(self.rows):
            raise ValueError(f"{len(finished)} flags for {len(self.rows)} live rows")
        return [i for i, f in enumerate(finished) if not f]

    def retire(self, keep: Sequence[int], ids: Sequence[Sequence[int]], heads: Sequence[int], lps: Optional[Sequence] = None) -> None:
        """the running batch shrinks to positions `keep` (non-empty: the device keeps one row at least); results of the others are stashed and their
        KV slots become free"""
        keep = [int(k) for k in keep]
        self._check(ids, heads, lps)
        n = len(self.rows)
        if not keep or any(k < 0 or k >= n for k in keep) or any(b <= a for a, b in zip(keep, keep[1:])):
            raise ValueError("keep must be a non-empty, strictly increasing list of live positions")
        kept = set(keep)
        for i in range(n):
            if i not in kept:
                self._put(i, ids, heads, lps)
        self.free.sort()
        self.rows = [self.rows[k] for k in keep]
        self.slots = [self.slots[k] for k in keep]
        self.retires += 1
        self.history.append(list(self.rows))

    def finish(self, ids: Sequence[Sequence[int]], heads: Sequence[int], lps: Optional[Sequence] = None) -> None:
        """every live row leaves (the batch ended): its results join the stash and every KV slot is free again"""
        self._check(ids, heads, lps)
        for i in range(len(self.rows)):
            self._put(i, ids, heads, lps)
        self.free.sort()
        self.rows, self.slots = [], []

    def results(self):
        """one (ids, head[, logprobs]) per request that entered, in request order; every row must have left (finish)"""
        if self.rows or len(self._out) != self.requests:
            raise ValueError(f"{len(self.rows)} rows are still live" if self.rows else "a request has no result")
        out = [self._out[r] for r in range(self.requests)]
        return [o if self.logprobs else o[:2] for o in out]
