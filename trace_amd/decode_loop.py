"""The one host loop that steps a running decode batch (no torch, no device), the book of its rows, and the checks of the requests that enter it.

The device is six primitives (Device; TraceEngine binds its decode_begin, _admit, decode_steps, retire_rows, decode_read and decode_read_logprobs,
tests/decode_loop_probes.py scripts them on lists).  decode_loop() has one boundary: read the recorded ids, decide which rows are finished, retire by
retire.retire_plan (the rows that leave go into retire.RowBook), admit by admit.admit_plan, look again at what an admission brought; then it chooses the stride and steps.  When every row of the
batch has ended, whatever waits begins the next batch.  Everything else is data: the bound of every row, the chunk, whether retiring is on, the
waiting requests (none beyond the batch for TraceEngine.decode), the `place` callback that prefills a request into its KV slot, and Rules.

Rules holds the edges at which the three loops this one replaced differed (DESIGN.md 4k lists them as standing differences).  They change results
— a row's returned head keeps changing while it rides steps after it has finished — so each entry point keeps its own: DECODE, DECODE_ROWS, QUEUE."""
from __future__ import annotations

from typing import Callable, Iterable, Iterator, List, NamedTuple, Optional, Sequence

from .admit import ADMIT_FRACTION, admit_plan
from .retire import RETIRE_FRACTION, RowBook, retire_plan
from .sampling import Constraints, LogitsParams, RowParams, SamplingParams, check_constraints, ends_stopped


class Device(NamedTuple):
    """what the loop asks of a device"""
    begin: Callable          # (slots, heads, forced, row_params): a batch of these KV slots; token 0 of every row is recorded
    admit: Callable          # (slots, heads, row_ids, forced, row_params): rows behind the live ones; row_ids: their Philox row indices
    steps: Callable          # (n): n decode steps of every row of the batch
    retire: Callable         # (keep): the batch shrinks to these positions
    read: Callable           # () -> (ids per row, heads)
    read_logprobs: Callable  # (lengths) -> one array per row, cut to that row's length


class Rules(NamedTuple):
    """the edges of the loop that an entry point chooses"""
    first_boundary: str      # the boundary before the first chunk: "skip" (no read-back: the batch rides a chunk whatever token 0 was), "look" (reads,
    #                          may end the batch, never retires) or "full" (reads, may end, retires, admits)
    stride_finished: bool    # the stride is the largest remainder of every row of the batch, finished ones still riding included (else: unfinished only)
    idle_chunk: Optional[int]  # the chunk while retiring is off (None: the retire chunk)
    one_launch: bool         # when nothing can end a row early (eos < 0, no stop sequences): one stride of the whole remainder, no read-back between
    bound_finishes: bool     # a row that has recorded its bound is finished (else: EOS / stop only, and the batch ends when no step is left)


DECODE = Rules("skip", True, 32, True, False)             # TraceEngine.decode
DECODE_ROWS = Rules("look", False, 32, False, True)       # TraceEngine.decode(row_params=...)
QUEUE = Rules("full", True, None, False, True)            # TraceEngine.generate_queue / decode_queue


def checked_requests(requests: Iterable, max_new_tokens: int, total_vocab: int, sampling: Optional[SamplingParams] = None,
                     logits: Optional[LogitsParams] = None, constraints: Optional[Constraints] = None, per_request: bool = False) -> Iterator[tuple]:
    """The requests of generate_queue / decode_queue, each checked and widened to (video, timestamps, input_ids, head, forced ids or None, the
    row's own RowParams or None) as it is pulled.  ValueError, here and now, for sampling parameters outside the device sampler's domain, for
    constraints outside the vocabulary, and, when `requests` is a list or a tuple, for any bad request in it: every request is looked at before any
    work.  An iterator is looked at as it is pulled, so there the error comes when the bad request is reached."""
    armed = logits is not None and not logits.off
    bound = constraints is not None and not constraints.off
    if sampling is not None and not sampling.greedy and not sampling.on_device:
        raise ValueError("generate_queue needs the device decode loop: these sampling parameters lie outside the device sampler's domain")
    if bound:
        check_constraints(constraints.stop_sequences, constraints.bad_words_ids, constraints.suppress_tokens, constraints.begin_suppress_tokens,
                          total_vocab)
    mn = int(max_new_tokens)

    def checked(req):
        req = tuple(req)
        if len(req) == 6 and not per_request:
            raise ValueError("a request with a sixth element (RowParams) needs per_request=True")
        if len(req) not in ((4, 5, 6) if per_request else (4, 5)):
            raise ValueError("a request is (video, timestamps, input_ids, head[, forced ids[, RowParams]])" if per_request else
                             "a request is (video, timestamps, input_ids, head[, forced ids])")
        req = req + (None,) * (6 - len(req))
        own = None
        if per_request:                               # the row's own params, every None field from the call's; checked here, before any work on it
            own = (req[5] if req[5] is not None else RowParams()).over(sampling, logits, mn).check(mn)
        if ((own.armed if per_request else armed) or bound) and req[4] is not None:
            raise ValueError("logits processors and constraints act on the ids a row has recorded; under forced ids those are not the fed ones "
                             "(a forced request with logits= / constraints=)")
        return req[:5] + (own,)

    if isinstance(requests, (list, tuple)):
        for r in requests:                            # every request is looked at before any work; the generator checks again as it is pulled
            checked(r)
    return (checked(r) for r in requests)


def forced_of(reqs: Sequence[tuple], max_new: int):
    """the forced rows of a begin or an admission: None when no request carries any, else one row per request (-1 throughout: nothing forced)"""
    if all(r[4] is None for r in reqs):
        return None
    return [list(r[4]) if r[4] is not None else [-1] * max_new for r in reqs]


def flat_forced(forced: Optional[Sequence[Sequence[int]]], max_new: int) -> Optional[List[int]]:
    """forced rows cut or zero-padded to max_new ids each, flattened row after row (what trace_decode_begin / trace_decode_admit take); None stays"""
    if forced is None:
        return None
    flat = []
    for row in forced:
        row = list(row)[:max_new]
        flat += row + [0] * (max_new - len(row))
    return flat


def decode_loop(dev, requests: Iterator[tuple], place: Callable, book: RowBook, rules: Rules, *, cap: int, max_new: int, eos: int = -1,
                constraints: Optional[Constraints] = None, chunk: int = 32, retiring: bool = True, retire_fraction: int = RETIRE_FRACTION,
                admit_fraction: int = ADMIT_FRACTION) -> RowBook:
    """Decode every request of `requests` (checked_requests' tuples; a request with RowParams has its own bound) through running batches of at most
    `cap` rows on `dev`; afterwards `book` (a fresh RowBook over the KV slots it may hand out) holds every result.  place(slots the book hands
    out, requests) -> the KV slots the rows decode from, prefilled.  chunk: steps between two boundaries while retiring.  RuntimeError when a
    row that is not finished has no step left."""
    mn, buf = int(max_new), []
    read_lps = lambda ids: dev.read_logprobs([len(x) for x in ids]) if book.logprobs else None
    params_of = lambda reqs: [r[5] for r in reqs] if reqs[0][5] is not None else None
    limits_of = lambda reqs: [mn if r[5] is None else int(r[5].max_new_tokens) for r in reqs]      # every row's own bound
    if not retiring and rules.idle_chunk is not None:
        chunk = rules.idle_chunk
    if rules.one_launch and eos < 0 and not (constraints is not None and constraints.stop_sequences):
        chunk = mn                                     # (no row can finish: nothing to look at between the steps, nothing to retire)
    chunk = max(1, int(chunk))

    def waiting(want: int) -> int:
        """requests in hand, after pulling until `want` are (or the source is dry)"""
        while len(buf) < want:
            try:
                buf.append(next(requests))
            except StopIteration:
                break
        return len(buf)

    def stride(count=None) -> int:
        """steps to the next boundary: the chunk, or the largest remainder of the rows that count (default: every row of the batch)"""
        left = [m - 1 - s for m, s in zip(lim, own)]
        return min(chunk, max([x for x, c in zip(left, count or [True] * len(left)) if c] + [0]))

    while waiting(cap):
        reqs = [buf.pop(0) for _ in range(min(cap, len(buf)))]
        base = book.requests                           # the batch's first request: Philox row indices count from it, as the device's begin counts
        dev.begin(place(book.admit(len(reqs)), reqs), [int(r[3]) for r in reqs], forced_of(reqs, mn), params_of(reqs))
        own = [0] * len(reqs)                          # steps of its own every live row has taken
        lim = limits_of(reqs)                          # ids it may record
        n = stride() if rules.first_boundary == "skip" else 0      # the steps taken before the boundary below: 0 = it is the batch's first
        while True:
            if n > 0:
                dev.steps(n)
                own = [s + n for s in own]
            # a boundary: look at the recorded ids, retire, admit — and look again at what an admission brought (a row whose token 0 ends it
            # leaves before it has ridden a chunk), until nothing more is admitted
            while True:
                ids, hd = dev.read()
                finished = [(rules.bound_finishes and len(x) >= m) or ends_stopped(x, eos, constraints) for x, m in zip(ids, lim)]
                live = finished.count(False)
                ended = live == 0 or (not rules.bound_finishes and stride() <= 0)
                if ended:
                    break
                if retiring and (rules.first_boundary == "full" or n > 0) and retire_plan(len(ids), live, retire_fraction):
                    keep = book.keep_list(finished)
                    book.retire(keep, ids, hd, read_lps(ids))
                    dev.retire(keep)
                    own, lim, finished = [own[k] for k in keep], [lim[k] for k in keep], [False] * len(keep)
                room = min(cap - len(own), len(book.free))
                k = admit_plan(len(own), cap, waiting(room), len(book.free), admit_fraction) if room > 0 else 0
                if not k:
                    break
                reqs = [buf.pop(0) for _ in range(k)]
                first = book.requests
                dev.admit(place(book.admit(k), reqs), [int(r[3]) for r in reqs], list(range(first - base, first - base + k)), forced_of(reqs, mn),
                          params_of(reqs))
                own += [0] * k
                lim += limits_of(reqs)
            if ended:                                 # the batch ended: whatever waits begins the next one
                book.finish(ids, hd, read_lps(ids))
                break
            n = stride(None if rules.stride_finished else [not f for f in finished])      # the largest remainder of a row
            if n <= 0:
                raise RuntimeError("decode loop: a row has taken every step its bound allows and is not finished")
    return book
