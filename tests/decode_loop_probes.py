"""A scripted device for the host decode loop (trace_amd/decode_loop.py): what the engine's device side does to the recorded ids, on lists.  It
implements the loop's protocol (begin, admit, steps, retire, read, read_logprobs), so the host tests run the loop that ships, and the call-trace test
puts it behind a TraceEngine whose device primitives are overridden.  Nothing here imports the HIP library; everything runs on the CPU."""
import numpy as np

EOS = 7


def script_with_ends(ends, max_new, eos=EOS):
    """request r records ids 10 + r until position ends[r], where it records EOS (None: never)"""
    return [[eos if s == e else 10 + r for s in range(max_new)] for r, e in enumerate(ends)]


def expected(script, eos=EOS):
    return [row[: row.index(eos) + 1 if eos in row else len(row)] for row in script]


def run(script, max_new, chunk, cap, rules, logprobs=True, retiring=True, bounds=None, eos=EOS):
    """trace_amd.decode_loop.decode_loop under `rules` on the scripted device: request r is script[r] (head r names it; bounds[r]: its own
    max_new_tokens), at most `cap` rows run together in the KV slots the book hands out -> (the book, the device)"""
    from trace_amd.decode_loop import RowBook, decode_loop
    from trace_amd.sampling import RowParams
    book = RowBook(range(cap), logprobs)
    dev = ScriptedDevice(script, max_new, eos, book=book)
    reqs = [(None, None, None, r, None, None if bounds is None else RowParams(None, None, bounds[r])) for r in range(len(script))]
    decode_loop(dev, iter(reqs), lambda slots, _: slots, book, rules, cap=cap, max_new=max_new, eos=eos, chunk=chunk, retiring=retiring)
    return book, dev


class ScriptedDevice:
    """Request r records script[r] from its own step 0 until EOS, a stop sequence or its bound (max_new, or its RowParams' max_new_tokens); positions
    hold requests; begin / admit append, retire keeps positions.  The head a row is begun or admitted with names its request.  Every KV slot
    remembers the request prefilled into it (`place`: what the loop's place callback reports, or the slot itself when nothing was placed).
    head_of(request, steps ridden): the head read back; a row rides steps, and its head goes on changing, after it has finished.
    book: the loop's RowBook, when the test wants the invariants checked from this side after every begin, admit, retire and before every step."""

    def __init__(self, script, max_new, eos=EOS, stops=(), head_of=None, book=None):
        self.script, self.max_new, self.eos, self.stops = script, max_new, eos, [list(s) for s in stops]
        self.head_of = head_of or (lambda r, steps: 100 + r)
        self.book, self.all_slots = book, sorted(book.free) if book is not None else None      # (a fresh book: every KV slot is free)
        self.rows, self.own, self.slot_of, self.bound = [], [], [], []
        self.prefilled = {}
        self.row_steps = 0
        self.sizes = []                                   # the batch size of every steps() call
        self.begun = self.admits = self.retires = 0

    def _check(self):
        if self.book is not None:
            b = self.book
            assert b.rows == self.rows and b.slots == self.slot_of and sorted(b.free + b.slots) == self.all_slots

    def _enter(self, slots, heads, row_params):
        for r, s in zip(heads, slots):
            assert s not in self.slot_of, "a live row's KV slot was handed out again"
            self.prefilled[s] = r
        self.rows += [int(h) for h in heads]
        self.own += [1] * len(heads)                      # begin / admit record id 0
        self.slot_of += [int(s) for s in slots]
        self.bound += [self.max_new if p is None else int(p.max_new_tokens) for p in (row_params or [None] * len(heads))]
        self._check()

    def begin(self, slots, heads, forced=None, row_params=None):
        self.rows, self.own, self.slot_of, self.bound = [], [], [], []
        self.begun += 1
        self._enter(slots, heads, row_params)

    def admit(self, slots, heads, row_ids=None, forced=None, row_params=None):
        assert self.rows, "admit into a batch that was never begun"
        self.admits += 1
        self._enter(slots, heads, row_params)

    def steps(self, n):
        assert n > 0
        self._check()
        self.own = [s + n for s in self.own]
        self.row_steps += n * len(self.rows)
        self.sizes.append(len(self.rows))

    def _ids(self, r, own, bound):
        out = []
        for t in self.script[r][: min(own, bound)]:
            out.append(t)
            if (self.eos >= 0 and t == self.eos) or any(len(out) >= len(s) and out[len(out) - len(s):] == s for s in self.stops):
                break
        return out

    def read(self):
        for r, slot in zip(self.rows, self.slot_of):
            assert self.prefilled[slot] == r, "the row attends another request's KV slot"
        ids = [self._ids(r, s, b) for r, s, b in zip(self.rows, self.own, self.bound)]
        return ids, [self.head_of(r, s - 1) for r, s in zip(self.rows, self.own)]

    def read_logprobs(self, lengths):
        assert len(lengths) == len(self.rows)
        return [np.array([-(r + 1) - 0.001 * s for s in range(int(n))], np.float32) for r, n in zip(self.rows, lengths)]

    def retire(self, keep):
        assert list(keep) == sorted(set(keep)) and 0 <= keep[0] and keep[-1] < len(self.rows)
        if len(keep) != len(self.rows):
            self.retires += 1
        self.rows, self.own, self.slot_of, self.bound = ([a[k] for k in keep] for a in (self.rows, self.own, self.slot_of, self.bound))
        self._check()
