"""When the room that retired rows left in a running decode batch is worth admitting waiting requests into (continuous batching; no torch, no
device).  decode_loop.decode_loop asks admit_plan at every chunk boundary, after that boundary's retire; retire.RowBook keeps which request
sits at which position of the batch and in which KV slot, recycles the slots, and returns everything in request order.  tests/test_admit_host.py
runs that loop on a scripted device."""
from __future__ import annotations

from .retire import RETIRE_FRACTION, RowBook

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


# Not a second class: the name under which tests/test_admit_host.py of the commit before this class imports it at module level.  Without
# it that module cannot be imported at all and its tests of the plan rule and the header go down with the ones that used the old book.
QueueBook = RowBook
