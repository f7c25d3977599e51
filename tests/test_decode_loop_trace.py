"""The host decode loop's call traces: every public entry point that steps a running batch (decode, decode_queue, generate_queue) is driven on a
TraceEngine whose device primitives are overridden by a scripted device (tests/decode_loop_probes.py), and the calls it issues, in order and with
their arguments, and the results it returns are compared with tests/golden/decode_loop_traces.json.  The fixture was recorded by this file
(PYTHONPATH=. python tests/test_decode_loop_trace.py) on the engine as it stood before the three host loops became one: it pins the order and arguments of
begin / admit / retire / steps, every arm and disarm call, and the ids, heads and log-probability lengths of every result.  A row's scripted head is
1000 * request + the steps it has ridden, so a chunk ridden too many or too few shows in the result.  One normalisation, on both sides: read-backs
that follow one another with no other call between them count as one.  No device."""
import json
import os
from types import SimpleNamespace

import pytest

import admit_probes as AP
import row_params_probes as RP
from decode_loop_probes import ScriptedDevice, script_with_ends
from trace_amd.engine import TraceEngine
from trace_amd.sampling import Constraints, LogitsParams, RowParams, SamplingParams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_loop_traces.json")
EOS = 7


def _ints(x):
    return None if x is None else [int(v) for v in x]


def _rows(x):
    return None if x is None else [_ints(r) for r in x]


class StubEngine(TraceEngine):
    """TraceEngine without __init__: the device primitives run a ScriptedDevice and log themselves; everything else is the engine's own code"""
    decode_batch_max = 9

    def __init__(self, script, max_batch=9, chunk=4):
        self.script, self.max_batch, self.retire_chunk = script, max_batch, chunk
        self.cfg = SimpleNamespace(total_vocab=400)
        self.stats = {"decode_row_steps": 0}
        self.retires = self.admits = 0
        self.calls, self.dev, self.stops = [], None, ()

    # ---- the four modes
    def set_sampling(self, sampling):
        self.calls.append(["set_sampling", repr(sampling)])

    def set_logprobs(self, on):
        self.calls.append(["set_logprobs", bool(on)])

    def set_logits_params(self, logits):
        self.calls.append(["set_logits_params", repr(logits)])

    def set_constraints(self, constraints):
        self.calls.append(["set_constraints", repr(constraints)])
        self.stops = constraints.stop_sequences if constraints is not None else ()

    # ---- the device
    def encode_prefill(self, videos, timestamps, input_ids, slot0=0, **kw):
        self.calls.append(["prefill", int(slot0), _rows(input_ids), {k: kw[k] for k in sorted(kw)}])

    def decode_begin(self, slots, heads, max_new, eos=-1, forced=None, want_logits=False, shared_prefix=None, row_params=None):
        self.calls.append(["begin", _ints(slots), _ints(heads), int(max_new), int(eos), _rows(forced), shared_prefix,
                           None if row_params is None else [repr(p) for p in row_params]])
        if self.dev is None:
            self.dev = ScriptedDevice(self.script, max_new, eos, self.stops, head_of=lambda r, steps: 1000 * r + steps)
        self.dev.stops = [list(s) for s in self.stops]
        self._B, self._max_new = len(slots), max_new
        self._rows = list(range(self._B))
        self._rows_history = [list(self._rows)]
        self.dev.begin(list(slots), list(heads), forced, row_params)

    def _admit(self, slots, heads, row_ids, forced, row_params):
        self.calls.append(["admit", _ints(slots), _ints(heads), _ints(row_ids), _rows(forced), None if row_params is None else [repr(p) for p in row_params]])
        nxt = 1 + max([max(h) for h in self._rows_history if h] + [-1])
        self._rows = self._rows + list(range(nxt, nxt + len(slots)))
        self._B += len(slots)
        self.admits += 1
        self._rows_history.append(list(self._rows))
        self.dev.admit(list(slots), list(heads), row_ids, forced, row_params)

    def decode_steps(self, n, use_graph=True, want_logits=False):
        self.calls.append(["steps", int(n), bool(use_graph)])
        self.stats["decode_row_steps"] += self._B * n
        self.dev.steps(n)

    def retire_rows(self, keep):
        self.calls.append(["retire", _ints(keep)])
        if len(keep) != self._B:
            self.retires += 1
            self._rows_history.append([self._rows[k] for k in keep])
        self._rows = [self._rows[k] for k in keep]
        self._B = len(keep)
        self.dev.retire(list(keep))

    def decode_read(self):
        self.calls.append(["read"])
        return self.dev.read()

    def decode_read_logprobs(self, lengths=None):
        self.calls.append(["read_logprobs", _ints(lengths)])
        return self.dev.read_logprobs(lengths)


def _result(out):
    """ids, heads and the lengths of the log-probabilities: of decode()'s columns, or of the queue's one tuple per request"""
    if isinstance(out, tuple):
        return [_rows(out[0]), _ints(out[1])] + ([[len(x) for x in out[2]]] if len(out) > 2 else [])
    return [[_ints(o[0]), int(o[1])] + ([len(o[2])] if len(o) > 2 else []) for o in out]


def _trace(eng, call):
    try:
        out = {"result": _result(call())}
    except (ValueError, RuntimeError) as e:
        out = {"error": f"{type(e).__name__}: {e}"}
    out.update(calls=eng.calls, rows_history=eng._rows_history, retires=eng.retires, admits=eng.admits, row_steps=eng.stats["decode_row_steps"])
    return json.loads(json.dumps(out))


# ---- the cases: the smallest at which each edge of the three former loops shows -----------------------------------------------------------------------
SAMPLED = SamplingParams(0.7, 50, 0.9, seed=3)
DECODE = {   # name: (ends, max_new, eos, stop sequences)
    "chunks": ([0, 17, 3, None, 9, 5, 20, 1, 13], 21, EOS, None),          # rows ending in different chunks
    "token0": ([0] * 5, 21, EOS, None),                                    # every row ends with its token 0: decode() still rides one chunk
    "never": ([None] * 6, 21, EOS, None),                                  # eos >= 0, no row ever ends: chunks with read-backs to the bound
    "endless": ([None] * 4, 21, -1, None),                                 # nothing can end early: one steps(max_new - 1), one read-back
    "stop": ([None, 6, None], 21, -1, [[11, EOS]]),                        # eos = -1, but row 1 records 11 .. 11, 7: a stop sequence ends it
    "one": ([0, None, None], 1, EOS, None),                                # max_new = 1: no step at all
    "threshold": ([None if r not in (5, 9, 20, 21, 30) else {5: 1, 9: 6, 20: 10, 21: 11, 30: 30}[r] for r in range(32)], 41, EOS, None),
}
ROW_BOUNDS = [3, 12, 21, 3, 12, 21, 21, 12, 3]
ROW_ENDS = [None, 5, 17, 1, None, None, 9, 11, 0]                          # row 8 ends with its token 0: not retired before the first chunk
SMALL_QUEUES = {   # the scripts of tests/test_admit_host.py: (ends, max_new, cap)
    "interleaved": ([0, None, 3, 9, 6, 1, None, 2], 13, 4),
    "ends_at_once": ([1, 2, 1, 3, None, 1], 9, 4),
    "token0_rides_no_chunk": ([1, 2, 0, 3, None, 1], 9, 4),
    "nothing_ends": ([None] * 5, 9, 2),
}


def decode_case(name, retire, logprobs):
    ends, mn, eos, stops = DECODE[name]
    eng = StubEngine(script_with_ends(ends, mn))
    cons = Constraints(stop_sequences=stops) if stops else None
    return _trace(eng, lambda: eng.decode(range(len(ends)), range(len(ends)), mn, eos, logprobs=logprobs, constraints=cons, retire_finished=retire,
                                          sampling=SAMPLED if name == "chunks" else None, logits=LogitsParams(1.2) if name == "never" else None))


def rows_case(retire, logprobs):
    eng = StubEngine(script_with_ends(ROW_ENDS, 21))
    params = [RowParams(SAMPLED if r % 2 else None, None, b) for r, b in enumerate(ROW_BOUNDS)]
    return _trace(eng, lambda: eng.decode(range(10, 19), range(9), 21, EOS, logprobs=logprobs, retire_finished=retire, row_params=params))


def requests(ends, generate, forced=None, params=None):
    """request r: its head and (generate_queue) its input ids name it; its KV slot in decode_queue is 20 + r"""
    out = []
    for r in range(len(ends)):
        req = (None, None, [r] if generate else 20 + r, r)
        if forced is not None or params is not None:
            req += (None if forced is None else forced[r],)
        if params is not None:
            req += (params[r],)
        out.append(req)
    return out


def queue_case(ends, mn, cap, generate, logprobs=False, forced=None, params=None, source=list, fraction=None, max_batch=9, **kw):
    eng = StubEngine(script_with_ends(ends, mn), max_batch=max_batch)
    if fraction:
        eng.retire_fraction = fraction
    reqs = requests(ends, generate, forced, params)
    if generate:
        return _trace(eng, lambda: eng.generate_queue(source(reqs), mn, EOS, max_rows=cap, logprobs=logprobs, per_request=params is not None, **kw))
    return _trace(eng, lambda: eng.decode_queue([r[2] for r in reqs], [r[3] for r in reqs], mn, EOS, max_rows=cap, logprobs=logprobs, forced=forced,
                                                row_params=params, **kw))


def bad_fifth(reqs):
    """an iterator whose fifth request is malformed"""
    for r, req in enumerate(reqs):
        yield req + (None, None, None) if r == 4 else req


# The stride edge: cap 5, retire_fraction 2 (a retire needs two finished rows of four or five).  Requests 0 and 1 end in the first chunk and retire;
# request 5 is admitted beside 2, 3, 4 (bound 12, four steps ridden) and ends with its token 0: one finished row of four stays in the batch.  At the
# next boundary but one the live rows have ridden 8 of their 11 steps and need 3; the finished row has ridden 4 of its bound's 20, and the stride is
# taken over every row of the batch: the third "steps" call of the trace is steps(4), not steps(3), and the heads returned for 2, 3, 4 end in 12.
STRIDE_ENDS = [2, 2, None, None, None, 0]
STRIDE_PARAMS = [RowParams(None, None, b) for b in (21, 21, 12, 12, 12, 21)]

CASES = {}
for _name in DECODE:
    for _retire in (False, True):
        for _lp in (False, True):
            CASES[f"decode/{_name}/retire={int(_retire)}/logprobs={int(_lp)}"] = lambda n=_name, r=_retire, l=_lp: decode_case(n, r, l)
for _retire in (False, True):
    CASES[f"decode_rows/retire={int(_retire)}"] = lambda r=_retire: rows_case(r, r)
for _gen in (False, True):
    _api = "generate_queue" if _gen else "decode_queue"
    CASES[f"{_api}/queue_ends"] = lambda g=_gen: queue_case(AP.QUEUE_ENDS, 41, 8, g, logprobs=g)
    for _name, (_ends, _mn, _cap) in SMALL_QUEUES.items():
        CASES[f"{_api}/{_name}"] = lambda g=_gen, e=_ends, m=_mn, c=_cap: queue_case(e, m, c, g, logprobs=not g)
    CASES[f"{_api}/per_request"] = lambda g=_gen: queue_case(AP.QUEUE_ENDS, 41, 8, g, params=[RP.queue_params(i, 41) for i in range(24)],
                                                             sampling=SAMPLED, logits=LogitsParams(1.2))
    CASES[f"{_api}/forced"] = lambda g=_gen: queue_case(SMALL_QUEUES["interleaved"][0], 13, 4, g,
                                                        forced=[None if r % 3 else [-1, 50 + r, -1] for r in range(8)], sampling=SAMPLED)
CASES["generate_queue/bad_fifth_request"] = lambda: queue_case(SMALL_QUEUES["interleaved"][0], 13, 4, True, logprobs=True, source=bad_fifth,
                                                               sampling=SAMPLED, logits=LogitsParams(1.2),
                                                               constraints=Constraints(stop_sequences=[[300, 301]]))
CASES["decode_queue/stride_over_a_finished_row"] = lambda: queue_case(STRIDE_ENDS, 21, 5, False, params=STRIDE_PARAMS, fraction=2)


def normalised(trace):
    """consecutive read-backs count as one"""
    calls = []
    for c in trace["calls"]:
        if not (c == ["read"] and calls and calls[-1] == ["read"]):
            calls.append(c)
    return dict(trace, calls=calls)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_and_results_are_the_recorded_ones(golden, name):
    got, want = normalised(CASES[name]()), normalised(golden[name])
    assert got["calls"] == want["calls"]
    assert got == want


def test_read_backs_never_appear(golden):
    """the normalisation lets read-backs disappear, never appear"""
    for name in CASES:
        assert sum(c == ["read"] for c in CASES[name]()["calls"]) <= sum(c == ["read"] for c in golden[name]["calls"]), name


def test_the_benchmark_path_is_one_begin_one_launch_one_read_back(golden):
    calls = CASES["decode/endless/retire=0/logprobs=0"]()["calls"]
    assert [c[0] for c in calls] == ["begin", "steps", "read"] and calls[1] == ["steps", 20, True]


def test_the_stride_case_reaches_the_state_it_names(golden):
    t = golden["decode_queue/stride_over_a_finished_row"]
    steps = [c for c in t["calls"] if c[0] == "steps"]
    assert steps == [["steps", 4, True]] * 3 and t["rows_history"][-1] == [2, 3, 4, 5] and [o[1] for o in t["result"]][2:5] == [2012, 3012, 4012]


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(CASES[k](), sort_keys=True)}" for k in sorted(CASES)) + "\n}\n")
    print(f"{len(CASES)} traces -> {GOLDEN}")
