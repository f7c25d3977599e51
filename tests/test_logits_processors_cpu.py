"""Logits processors without a GPU: the float32 restatement (trace_amd/sampling.py process_row_ref) against HF's own processors, the probe
table's claims, the mutants against the case lists the GPU test runs (tests/logits_probes.py), the argument mapping of generate() on a fake
engine, and the C ABI's two new entries."""
import json
import os
import re

import numpy as np
import pytest

import logits_probes as LP
import token_select_probes as P
from trace_amd.sampling import LogitsParams, check_logits_params, process_row_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- 1: the restatement vs HF
def test_restatement_equals_hf_processors():
    """torch.equal against RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> MinNewTokensLengthLogitsProcessor on every loose row
    of the list the GPU op is held against: -inf masks, zeros, both signs, duplicate ids, ids of other heads, every history length around n"""
    torch = pytest.importorskip("torch")
    tf = pytest.importorskip("transformers")
    cfg = P.small()
    cases = LP.row_cases(cfg)
    seen = {"lens": set(), "n": set(), "p": set(), "m": set(), "eos_in": set()}
    for c in cases:
        lo, hi = P.head_range(cfg, c.head)
        got = torch.from_numpy(process_row_ref(c.row, c.hist, lo, hi, c.params, c.step, c.eos))
        ids = torch.tensor([c.hist], dtype=torch.long).reshape(1, len(c.hist))
        want = torch.from_numpy(c.row.copy())[None]
        if c.params.repetition_penalty != 1.0:
            want = tf.RepetitionPenaltyLogitsProcessor(float(c.params.repetition_penalty))(ids, want)
        if c.params.no_repeat_ngram_size:
            want = tf.NoRepeatNGramLogitsProcessor(c.params.no_repeat_ngram_size)(ids, want)
        if c.params.min_new_tokens and c.eos >= 0:
            # HF counts the new tokens as input_ids.shape[-1] - prompt_length_to_skip and reads nothing else of input_ids: the device step is that number
            want = tf.MinNewTokensLengthLogitsProcessor(0, c.params.min_new_tokens, c.eos, device="cpu")(torch.zeros((1, c.step), dtype=torch.long), want)
        assert torch.equal(got, want[0]), (c.head, c.hist, c.params, c.step, c.eos)
        seen["lens"].add(len(c.hist)); seen["n"].add(c.params.no_repeat_ngram_size); seen["p"].add(c.params.repetition_penalty)
        seen["m"].add(c.params.min_new_tokens); seen["eos_in"].add(c.eos >= 0 and lo <= c.eos < hi)
        assert bool(np.isneginf(c.row[lo:hi]).any()) and (c.row[lo:hi] == 0).any() and (c.row[lo:hi] > 0).any() and (c.row[lo:hi] < 0).any()
    assert {0, 1, 2, 3, 4, 5, 40} <= seen["lens"] and {1, 2, 3, 5} <= seen["n"] and {1.0, 0.7, 1.3} <= seen["p"] and {0, 1, 3} <= seen["m"]
    assert seen["eos_in"] == {True, False}
    assert any(len(set(c.hist)) < len(c.hist) for c in cases)                                             # duplicate ids
    assert any(any(not P.head_range(cfg, c.head)[0] <= t < P.head_range(cfg, c.head)[1] for t in c.hist) for c in cases)      # ids of another head


def test_off_is_the_identity_bitwise():
    cfg = P.small()
    assert LogitsParams().off and not LogitsParams(1.2).off and not LogitsParams(1.0, 2).off and not LogitsParams(1.0, 0, 1).off
    for c in LP.row_cases(cfg)[::7]:
        lo, hi = P.head_range(cfg, c.head)
        got = process_row_ref(c.row, c.hist, lo, hi, LogitsParams(), c.step, c.eos)
        assert got.tobytes() == c.row.tobytes()                          # (the case rows are -inf outside the head already)


def test_probe_restatement_without_a_mutant_is_the_restatement():
    cfg = P.small()
    for c in LP.row_cases(cfg)[::3]:
        lo, hi = P.head_range(cfg, c.head)
        a = LP.process_row(c.row, c.hist, lo, hi, c.params, c.step, c.eos)
        assert a.tobytes() == process_row_ref(c.row, c.hist, lo, hi, c.params, c.step, c.eos).tobytes(), (c.hist, c.params)


def test_check_logits_params():
    check_logits_params(1.0, 0, 0)
    check_logits_params(0.5, 64, 7)
    for bad in ((0.0, 0, 0), (-1.0, 0, 0), (float("nan"), 0, 0), (float("inf"), 0, 0), (1.0, -1, 0), (1.0, 65, 0), (1.0, 0, -1), (1.0, 1.5, 0)):
        with pytest.raises(ValueError):
            check_logits_params(*bad)
        with pytest.raises(ValueError):
            LogitsParams(*bad)


# ---------------------------------------------------------------------------------------------------------------- 3: the table and the mutants
@pytest.fixture(scope="module", params=list(LP.GEOMETRIES))
def probe(request):
    cfg = LP.GEOMETRIES[request.param]()
    T, plan = LP.build_table(cfg)
    return cfg, T, plan, P.logit_scale(cfg)


def test_table_has_a_maximum_and_a_runner_up_everywhere(probe):
    cfg, T, plan, _ = probe
    LP.check_table(T, cfg)
    c0, c1, c2 = plan.cycle
    assert T[c0, :cfg.vocab_size + 1].max() > 0 > T[c1, :cfg.vocab_size + 1].max()            # a positive and a negative state on the cycle
    assert LP.runner_up(T, cfg, c0, 0) == plan.cycle_runner[0] and LP.runner_up(T, cfg, c1, 0) == plan.cycle_runner[1]
    assert LP.runner_up(T, cfg, plan.eos_emitter, 0) == plan.eos_runner
    P.crafted_weights(cfg, T)                                                                 # the probes' recipe takes the table


def test_unprocessed_rows_cycle_and_processed_rows_break_where_predicted(probe):
    cfg, T, plan, scale = probe
    c0, c1, c2 = plan.cycle
    q0, q1, q2 = plan.cycle_runner
    mn = LP.MAX_NEW
    run = lambda start, head, params, eos=-1: LP.restate_processed(T, cfg, start, head, params, eos, mn, scale)
    ids, length, _ = run(c0, 0, LogitsParams())
    assert ids == [(c1, c2, c0)[i % 3] for i in range(mn)] and length == mn                     # the free-running cycle
    tour_ids = [t for t, _ in plan.tour]
    ids, _, _ = run(plan.tour[0][0], 0, LogitsParams())
    assert ids == [tour_ids[(i + 1) % len(tour_ids)] for i in range(mn)]                        # and the one through all three heads
    # no-repeat n-grams: a cycle of C ids repeats its first n-gram at step C + n - 1, on the state whose successor closes it
    for n in (2, 3):
        ids, _, _ = run(c0, 0, LogitsParams(no_repeat_ngram_size=n))
        at = 3 + n - 1
        assert ids[:at] == [(c1, c2, c0)[i % 3] for i in range(at)]
        state = ids[at - 1]
        assert ids[at] == LP.runner_up(T, cfg, state, 0) == {c0: q0, c1: q1, c2: q2}[state], (n, ids[:at + 1])
        ids, _, _ = run(plan.tour[0][0], 0, LogitsParams(no_repeat_ngram_size=n))
        at = len(tour_ids) + n - 1
        assert ids[:at] == [tour_ids[(i + 1) % len(tour_ids)] for i in range(at)] and ids[at] != tour_ids[(at + 1) % len(tour_ids)]
    # the penalty at 1.5: from c0 the positive state c0 meets its maximum c1 again at step 3: 20 / 1.5 < 16, the runner-up q0 wins
    ids, _, _ = run(c0, 0, LogitsParams(repetition_penalty=1.5))
    assert ids[:4] == [c1, c2, c0, q0]
    # from c1 the NEGATIVE state c1 meets its maximum c2 again at step 3: -10 * 1.5 < -14, the runner-up q1 wins
    ids, _, _ = run(c1, 0, LogitsParams(repetition_penalty=1.5))
    assert ids[:4] == [c2, c0, c1, q1]
    # at 1.2 one occurrence is not enough (20 / 1.2 > 16, -10 * 1.2 > -14): the cycle goes round again
    ids, _, _ = run(c0, 0, LogitsParams(repetition_penalty=1.2))
    assert ids[:9] == [c1, c2, c0] * 3
    # min_new_tokens = 3 from the EOS emitter: EOS at exactly step 3, length 4; without it: EOS at step 0
    ids, length, _ = run(plan.eos_emitter, 0, LogitsParams(min_new_tokens=3), plan.eos)
    assert ids == [plan.eos_runner, plan.eos_back, plan.eos_emitter, plan.eos] and length == 4
    assert run(plan.eos_emitter, 0, LogitsParams(), plan.eos)[:2] == ([plan.eos], 1)
    for m in (1, 2, 5):
        ids, length, _ = run(plan.eos_emitter, 0, LogitsParams(min_new_tokens=m), plan.eos)
        assert length >= m + 1 and plan.eos not in ids[:m]


@pytest.mark.parametrize("mutant", LP.MUTANTS)
def test_the_decode_cases_reject_a_wrong_processor(probe, mutant):
    """every mutant changes at least one emitted id or one length on the case lists the GPU test runs"""
    cfg, T, plan, scale = probe
    hit = []
    for c in LP.decode_cases(cfg, plan):
        good = LP.restate_batch(T, cfg, c.rows, c.params, c.eos, LP.MAX_NEW, scale)
        bad = LP.restate_batch(T, cfg, c.rows, c.params, c.eos, LP.MAX_NEW, scale, mutant)
        if (good[0], good[1]) != (bad[0], bad[1]):
            hit.append(c.name)
    assert hit, f"{mutant}: no decode case tells it from the rules"


def test_decode_cases_cover_the_batches_and_all_heads(probe):
    cfg, T, plan, scale = probe
    cases = LP.decode_cases(cfg, plan)
    assert {len(c.rows) for c in cases} >= {1, 3, 17} and LP.MAX_NEW <= 48
    assert all(len(set(c.rows)) == len(c.rows) for c in cases)                                  # different start states per row
    heads = set()
    for c in cases:
        if len(c.rows) == 17:
            for b, (t, h) in enumerate(c.rows):
                tr = []
                LP.restate_processed(T, cfg, t, h, c.params, c.eos, LP.MAX_NEW, scale, trace=tr)
                heads |= {hd for _, hd, _, _ in tr}
    assert heads == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------- 4: generate()'s arguments
class _FakeEngine:
    device, dtype = "cpu", None
    max_batch, decode_batch_max = 8, 8

    def __init__(self):
        self.calls = []

    def host_mode(self, on):
        pass

    def generate(self, vids, ts, ids, heads, max_new, eos=-1, sampling=None, logprobs=False, **kw):
        self.calls.append(("generate", sampling, kw))
        return [[5, 6, 7] for _ in vids], [0] * len(vids)

    def generate_samples(self, video, ts, prompt_ids, head, n, max_new, eos=-1, sampling=None, use_graph=True, **kw):
        self.calls.append(("generate_samples", sampling, kw))
        return [[10 + r] * 2 for r in range(n)], [0] * n, [np.array([-1.0, -0.5 * r], np.float32) for r in range(n)]


def _model():
    from trace_amd.config import tiny
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    eng = _FakeEngine()
    return TraceMistralForCausalLM(tiny(num_frames=4), eng), eng


def _kw(torch):
    return dict(images_or_videos=[torch.zeros(4, 3, 8, 8)], video_timestamps=[[[0.0]] * 4], heads=[0], max_new_tokens=4, eos_token_id=-1)


def test_generate_hands_the_three_arguments_to_the_engine():
    torch = pytest.importorskip("torch")
    m, eng = _model()
    ids = torch.tensor([[1, 2]])
    m.generate(ids, **_kw(torch))
    assert eng.calls[-1] == ("generate", None, {})                                              # all off: the engine is called as before
    m.generate(ids, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, **_kw(torch))
    assert eng.calls[-1] == ("generate", None, {})
    m.generate(ids, repetition_penalty=1.2, no_repeat_ngram_size=3, **_kw(torch))
    assert eng.calls[-1][2] == {"logits": LogitsParams(1.2, 3, 0)}
    # precedence: explicit argument > generation_config > the model's defaults
    m.generate(ids, generation_config={"repetition_penalty": 1.3, "min_new_tokens": 2}, **_kw(torch))
    assert eng.calls[-1][2] == {"logits": LogitsParams(1.3, 0, 2)}
    m.generate(ids, repetition_penalty=1.1, generation_config={"repetition_penalty": 1.3, "min_new_tokens": 2}, **_kw(torch))
    assert eng.calls[-1][2] == {"logits": LogitsParams(1.1, 0, 2)}
    m.generation_config.no_repeat_ngram_size = 4
    m.generate(ids, **_kw(torch))
    assert eng.calls[-1][2] == {"logits": LogitsParams(1.0, 4, 0)}
    m.generate(ids, no_repeat_ngram_size=0, **_kw(torch))                                       # an explicit "off" wins over the model's default
    assert eng.calls[-1] == ("generate", None, {})
    m.generate(ids, generation_config={"no_repeat_ngram_size": 2}, do_sample=True, temperature=0.7, **_kw(torch))
    assert eng.calls[-1][1] is not None and eng.calls[-1][2] == {"logits": LogitsParams(1.0, 2, 0)}
    # generate_samples takes the same names
    m.generation_config.no_repeat_ngram_size = 0
    m.generate_samples(ids, n=2, temperature=0.7, repetition_penalty=1.2, **_kw(torch))
    assert eng.calls[-1][0] == "generate_samples" and eng.calls[-1][2] == {"logits": LogitsParams(1.2, 0, 0)}
    m.generate_samples(ids, n=2, temperature=0.7, **_kw(torch))
    assert eng.calls[-1][2] == {}


def test_generate_rejects_what_hf_rejects_and_what_stays_refused():
    torch = pytest.importorskip("torch")
    m, eng = _model()
    ids = torch.tensor([[1, 2]])
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=65),
                dict(min_new_tokens=-1)):
        with pytest.raises(ValueError):
            m.generate(ids, **bad, **_kw(torch))
    for refused in (dict(num_beams=2), dict(num_return_sequences=2), dict(typical_p=0.9), dict(min_p=0.1)):
        with pytest.raises(NotImplementedError):
            m.generate(ids, repetition_penalty=1.2, **refused, **_kw(torch))
    assert not eng.calls
    # called directly, _sampling_params refuses the name as it always did
    with pytest.raises(NotImplementedError):
        m._sampling_params(True, 1.0, None, None, None, {"repetition_penalty": 1.2})
    assert m._sampling_params(True, 1.0, None, None, None, {"repetition_penalty": 1.0}) is not None


def test_generation_config_json_is_picked_up(tmp_path):
    torch = pytest.importorskip("torch")
    from trace_amd.model.builder import apply_generation_config
    m, eng = _model()
    (tmp_path / "generation_config.json").write_text(json.dumps({"repetition_penalty": 1.15, "no_repeat_ngram_size": 3, "min_new_tokens": 1,
                                                                  "top_k": 20}))
    apply_generation_config(m, str(tmp_path))
    assert m._logits_params(None, None, None, None) == LogitsParams(1.15, 3, 1)
    m.generate(torch.tensor([[1, 2]]), **_kw(torch))
    assert eng.calls[-1][2] == {"logits": LogitsParams(1.15, 3, 1)}
    assert m._logits_params(1.0, 0, 0, None) is None                                           # explicit arguments win


# ---------------------------------------------------------------------------------------------------------------- 5: the C ABI
def test_header_and_signatures_name_the_two_entries():
    """no GPU, no library: the header declares both entries with the argument lists the ctypes table gives them"""
    import ctypes as C
    from trace_amd._lib import SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "trace_hip.h")).read()
    for name, nargs in (("trace_decode_set_logits_params", 4), ("trace_op_logits_process", 17)):
        assert name in SIGNATURES, f"missing symbol {name}"
        mm = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert mm, f"{name} is not declared in include/trace_hip.h"
        assert len(mm.group(1).split(",")) == nargs == len(SIGNATURES[name][1]), name
    assert SIGNATURES["trace_decode_set_logits_params"][1][1:] == [C.c_float, C.c_int, C.c_int]
    assert re.search(r"int\s+trace_abi_version", hdr)


def test_both_libraries_export_the_entries_under_abi_4():
    from trace_amd import build, _lib
    build.build()
    for element in ("bf16", "f16"):
        lib = _lib.load(element)
        assert lib.trace_abi_version() == 4
        assert hasattr(lib, "trace_decode_set_logits_params") and hasattr(lib, "trace_op_logits_process")
    # argument checks that come before any HIP call
    lib = _lib.load()
    with pytest.raises(_lib.TraceHipError, match="null pointer"):
        lib.trace_op_logits_process(None, 0, 1, None, 1, 1, 1, None, 0, None, None, -1, 1.0, 0, 0, None, None)


def test_new_kernels_have_no_scratch(tmp_path):
    """logits.hip holds logits_process_kernel, select.hip the three forms of select_next_kernel (the third one is the arg-max over a processed row),
    all without scratch, in the bf16 and the fp16 build"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "trace_amd", "csrc")
    for f16 in (False, True):
        found, cur = {}, None
        for name in ("logits", "select"):
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(csrc, name + ".hip"), "-I", csrc,
                   "-o", str(tmp_path / (name + ".o")), "-Rpass-analysis=kernel-resource-usage"] + (["-DTRACE_F16"] if f16 else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            for line in r.stderr.splitlines():
                mm = re.search(r"Function Name: (\S+)", line)
                if mm:
                    cur = mm.group(1)
                mm = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
                if mm and cur:
                    found[cur] = int(mm.group(1))
        assert sum("logits_process_kernel" in k for k in found) == 1 and sum("select_next_kernel" in k for k in found) == 3, sorted(found)
        assert all(v == 0 for v in found.values()), found
