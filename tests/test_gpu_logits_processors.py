"""Logits processors on the device (trace_amd/csrc/logits.h): repetition penalty, no-repeat n-grams and min_new_tokens inside the decode step.

The loose-row op is held against the float32 restatement bit for bit (sampling.process_row_ref, which tests/test_logits_processors_cpu.py holds
against HF's own processors).  The decode step runs on the identity-layer decoder of tests/token_select_probes.py with the table of
tests/logits_probes.py, where every processor rule has one right answer per step: ids, lengths and final heads are compared for exact equality with
LP.restate_processed, eager and graph-replayed, greedy and sampled; the log-probabilities stay those of the RAW row.  model.generate() takes the
three HF arguments on the tiny model, in the device loop and in the stepwise (stopping-criteria) loop alike."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import logits_probes as LP  # noqa: E402
import token_select_probes as P  # noqa: E402
from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402
from trace_amd.sampling import LogitsParams, SamplingParams, process_row_ref, token_logprob_ref  # noqa: E402

SLOTS = 17


class Rig:
    def __init__(self, geom, E):
        self.cfg = LP.GEOMETRIES[geom]()
        self.T, self.plan = LP.build_table(self.cfg)
        self.max_new = LP.MAX_NEW
        self.eng = TraceEngine(self.cfg, max_batch=SLOTS, max_ctx=160, max_frames=4, max_new_tokens=self.max_new)
        self.eng.load_weights(P.crafted_weights(self.cfg, self.T).items())
        self.eng.encode_video(synth.synth_frames(self.cfg, 0).to(torch.bfloat16), E["timestamps"].tolist())
        self.L, emb = self.eng.splice(E["input_ids"].tolist(), want_output=True)
        self.emb = emb.clone()
        self.start = {}
        self.scale = P.logit_scale(self.cfg)
        self.cases = {c.name: c for c in LP.decode_cases(self.cfg, self.plan)}

    def place(self, rows):
        """slot b <- the prompt whose last row is row b's start token (kept from earlier batches where it is the same)"""
        for b, (start, _) in enumerate(rows):
            if self.start.get(b) != start:
                self.emb[-1] = P.embedding_row(self.cfg, start).to(self.emb.device)
                self.eng.prefill(b, self.L, embeds=self.emb)
                self.start[b] = start

    def run(self, rows, params, eos, graph, sampling=None):
        """(ids, lengths, heads): decode_begin and max_new - 1 steps, replayed from the captured graph or eager one at a time"""
        self.place(rows)
        eng, mn = self.eng, self.max_new
        eng.set_logits_params(params)
        eng.set_sampling(sampling)
        try:
            eng.decode_begin(list(range(len(rows))), [h for _, h in rows], mn, eos=eos)
            if graph:
                eng.decode_steps(mn - 1, use_graph=True)
            else:
                for _ in range(mn - 1):
                    eng.decode_steps(1, use_graph=False)
            ids, heads = eng.decode_read()
        finally:
            eng.set_logits_params(None)
            eng.set_sampling(None)
        return ids, [len(x) for x in ids], heads

    def want(self, rows, params, eos, sampling=None):
        sp = None if sampling is None else (sampling.temperature, sampling.top_k, sampling.top_p, sampling.seed)
        return LP.restate_batch(self.T, self.cfg, rows, params, eos, self.max_new, self.scale, sampling=sp)

    def check(self, rows, params, eos, graph, tag, sampling=None):
        want, got = self.want(rows, params, eos, sampling), self.run(rows, params, eos, graph, sampling)
        if got != want:
            bad = [b for b in range(len(rows)) if (got[0][b], got[1][b], got[2][b]) != (want[0][b], want[1][b], want[2][b])]
            b = bad[0]
            raise AssertionError(f"{tag}: {len(bad)} of {len(rows)} rows differ; row {b} (start {rows[b]}): got {got[0][b]} head {got[2][b]}, "
                                 f"want {want[0][b]} head {want[2][b]}")


_rigs = {}


@pytest.fixture(scope="module")
def rigs(golden_dir):
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))

    def get(geom):
        if geom not in _rigs:
            _rigs[geom] = Rig(geom, E)
        return _rigs[geom]
    yield get
    for r in _rigs.values():
        r.eng.close()
    _rigs.clear()


# ---------------------------------------------------------------------------------------------------------------- 1: the loose-row op
@pytest.mark.parametrize("geom", list(LP.GEOMETRIES))
def test_loose_op_equals_restatement_bitwise(geom):
    """every row of LP.row_cases (the list the restatement is held against HF on), grouped by parameters and run in batches of 17, 3 and 1 rows with
    a different history per row; torch.equal on the whole output row: the processed head range AND -inf everywhere else.  The list holds histories
    with lo, hi - 1, lo - 1 and hi (the last two touch nothing) and 48 equal ids (the penalty applies once)."""
    cfg = LP.GEOMETRIES[geom]()
    V, Tv, Sv, NV, _ = P.dims(cfg)
    groups = {}
    for c in LP.row_cases(cfg):
        groups.setdefault((c.params, c.eos), []).append(c)
    sizes, rows_run = [17, 3, 1], 0
    for gi, ((params, eos), cs) in enumerate(groups.items()):
        o = 0
        while o < len(cs):
            B = min(sizes[(gi + o) % 3], len(cs) - o)
            part = cs[o:o + B]
            o += B
            lg = torch.from_numpy(np.stack([c.row for c in part])).cuda()
            got = ops.logits_process(lg, [c.head for c in part], [c.hist for c in part], params, [c.step for c in part], eos, V, Tv, Sv).cpu()
            for b, c in enumerate(part):
                lo, hi = P.head_range(cfg, c.head)
                want = torch.from_numpy(process_row_ref(c.row, c.hist, lo, hi, params, c.step, eos))
                assert torch.equal(got[b], want), (geom, b, B, c.head, c.hist, params, c.step, eos,
                                                   torch.nonzero(~((got[b] == want) | (got[b].isnan() & want.isnan())))[:8, 0].tolist())
                assert bool((got[b, :lo] == float("-inf")).all()) and bool((got[b, hi:] == float("-inf")).all())
            rows_run += B
    assert rows_run == len(LP.row_cases(cfg))


def test_loose_op_masks_an_unmasked_row_and_leaves_the_input_alone():
    """the input row is finite everywhere: the output is -inf outside the head all the same, and the input is not edited; inputs at every
    alignment; the fp16 library runs the same code"""
    cfg = P.small()
    V, Tv, Sv, NV, _ = P.dims(cfg)
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((3, NV)) * 3).astype(np.float32)
    hist = [[5, 5, V + 3], [V + 2, V + 2, V + 1], [V + 1 + Tv + 1, 0]]
    params = LogitsParams(1.3, 1, 1)
    for element, shift in (("bf16", 0), ("bf16", 1), ("bf16", 2), ("bf16", 3), ("f16", 0)):
        # shift: the input starts that many floats past a 16-byte boundary while the output does not - the copy then stores float by float
        buf = torch.zeros(3 * NV + 4, device="cuda")
        lg = buf[shift:shift + 3 * NV].view(3, NV)
        lg.copy_(torch.from_numpy(x))
        got = ops.logits_process(lg, [0, 1, 2], hist, params, [0, 0, 0], V + 4, V, Tv, Sv, element=element).cpu().numpy()
        assert np.array_equal(lg.cpu().numpy(), x)
        for b in range(3):
            lo, hi = P.head_range(cfg, b)
            assert got[b].tobytes() == process_row_ref(x[b], hist[b], lo, hi, params, 0, V + 4).tobytes(), (element, shift, b)


# ---------------------------------------------------------------------------------------------------------------- 2: the decode step, greedy
CASES = ("ngram2", "ngram3", "ngram2_b1", "ngram1_b17", "penalty1.5", "penalty1.5_b17", "penalty1.2", "min_new3", "min_new2", "min_new2_no_eos",
         "all_three", "all_three_b17")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("geom", list(LP.GEOMETRIES))
def test_decode_equals_restatement(rigs, geom, case, graph):
    """ids, lengths and final heads of every row, exactly: the n-gram rule breaks the cycle at the predicted step onto the runner-up, the penalty
    at 1.5 takes the positive state's maximum by division and the negative state's by multiplication, min_new_tokens = 3 holds EOS back until
    exactly step 3; B = 1, 3 (three different start states) and 17; eager and graph replay"""
    rig = rigs(geom)
    assert set(CASES) == set(rig.cases)
    c = rig.cases[case]
    rig.check(c.rows, c.params, c.eos, graph, f"{geom} {case}")


def test_decode_claims_hold_on_the_device(rigs):
    """the claims themselves, read off the device's ids: the cycle breaks at step 3 + n - 1 onto the runner-up; EOS at exactly step 3, length 4"""
    rig = rigs("small")
    plan = rig.plan
    c0, c1, c2 = plan.cycle
    for n in (2, 3):
        ids, _, _ = rig.run([(c0, 0)], LogitsParams(no_repeat_ngram_size=n), -1, True)
        at = 3 + n - 1
        assert ids[0][:at] == [(c1, c2, c0)[i % 3] for i in range(at)] and ids[0][at] == LP.runner_up(rig.T, rig.cfg, ids[0][at - 1], 0)
    ids, lens, _ = rig.run([(plan.eos_emitter, 0)], LogitsParams(min_new_tokens=3), plan.eos, True)
    assert ids[0] == [plan.eos_runner, plan.eos_back, plan.eos_emitter, plan.eos] and lens == [4]
    ids, _, _ = rig.run([(c0, 0), (c1, 0)], LogitsParams(repetition_penalty=1.5), -1, True)
    assert ids[0][:4] == [c1, c2, c0, plan.cycle_runner[0]] and ids[1][:4] == [c2, c0, c1, plan.cycle_runner[1]]


def test_parameters_change_between_batches_without_recapture(rigs):
    """the captured step reads the parameters from device memory: three batches of one size replay one graph, each under its own parameters"""
    rig = rigs("small")
    a, b, c = rig.cases["ngram2"], rig.cases["penalty1.5"], rig.cases["all_three"]
    assert len(a.rows) == len(b.rows) == len(c.rows)
    for k in (a, b, c, a):
        rig.check(k.rows, k.params, k.eos, True, f"replay {k.name}")


# ---------------------------------------------------------------------------------------------------------------- 3: sampling, log-probabilities
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("geom", list(LP.GEOMETRIES))
def test_sampling_draws_from_the_processed_row(rigs, geom, graph):
    """temperature 0.7, top_k 5, top_p 0.9, a fixed seed: every id is sample_row_ref of the processed row under the step's Philox counter"""
    rig = rigs(geom)
    sp = SamplingParams(0.7, 5, 0.9, seed=0x1234ABCD5678)
    rows = LP.start_rows(rig.cfg, rig.plan, 17)
    for params in (LogitsParams(1.5, 2, 0), LogitsParams(1.2, 3, 2)):
        rig.check(rows, params, rig.plan.eos, graph, f"{geom} sampled {params}", sampling=sp)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_logprobs_describe_the_raw_row(rigs, sampled):
    """processors on: logprob[b][s] is token_logprob_ref of the RAW row at the emitted id, bit for bit - not of the processed row"""
    rig = rigs("small")
    cfg, mn = rig.cfg, rig.max_new
    rows = LP.start_rows(cfg, rig.plan, 3)
    params = LogitsParams(1.5, 2, 0)
    sp = SamplingParams(0.7, 5, 0.9, seed=77) if sampled else None
    rig.place(rows)
    ids, heads, lps = rig.eng.decode(list(range(3)), [h for _, h in rows], mn, eos=-1, sampling=sp, logprobs=True, logits=params)
    want = rig.want(rows, params, -1, sp)
    assert (ids, heads) == (want[0], want[2])
    differs = 0
    for b, (t, h) in enumerate(rows):
        tr = []
        LP.restate_processed(rig.T, cfg, t, h, params, -1, mn, rig.scale, sampling=None if sp is None else (0.7, 5, 0.9, 77), row_index=b, trace=tr)
        for s, (state, head, raw, tok) in enumerate(tr):
            lo, hi = P.head_range(cfg, head)
            ref = token_logprob_ref(raw[lo:hi], tok - lo)
            assert np.float32(lps[b][s]).tobytes() == np.float32(ref).tobytes(), (b, s, lps[b][s], ref)
            proc = process_row_ref(raw, ids[b][:s], lo, hi, params, s, -1)
            differs += token_logprob_ref(proc[lo:hi], tok - lo) != ref
    assert differs > 0                           # the processed row would have given other values: the test can tell the two apart


# ---------------------------------------------------------------------------------------------------------------- 4: disarmed, errors
def test_disarmed_after_an_armed_batch_is_a_context_that_never_armed(rigs, golden_dir):
    rig = rigs("small")
    rows = LP.start_rows(rig.cfg, rig.plan, 3)
    rig.run(rows, LogitsParams(1.5, 2, 3), rig.plan.eos, True)
    got = [rig.run(rows, LogitsParams(), rig.plan.eos, g) for g in (True, False)]
    fresh = Rig("small", np.load(os.path.join(golden_dir, "tiny_e2e.npz")))
    try:
        fresh.place(rows)
        fresh.eng.decode_begin([0, 1, 2], [h for _, h in rows], fresh.max_new, eos=rig.plan.eos)
        fresh.eng.decode_steps(fresh.max_new - 1, use_graph=True)
        ids, heads = fresh.eng.decode_read()
    finally:
        fresh.eng.close()
    assert got[0] == got[1] == (ids, [len(x) for x in ids], heads)
    assert got[0] == rig.want(rows, LogitsParams(), rig.plan.eos)


def test_argument_errors(rigs):
    rig = rigs("small")
    eng = rig.eng
    rows = LP.start_rows(rig.cfg, rig.plan, 1)
    rig.place(rows)
    err_arg = r"error -1 in "                     # TRACE_ERR_ARG
    for bad in ((1.0, 65, 0), (0.0, 0, 0), (float("inf"), 0, 0), (1.0, -1, 0), (1.0, 0, -1)):
        with pytest.raises(_lib.TraceHipError, match=err_arg + "trace_decode_set_logits_params"):
            eng.lib.trace_decode_set_logits_params(eng.h, *bad)
    eng.set_logits_params(LogitsParams(1.2, 0, 0))
    try:
        with pytest.raises(_lib.TraceHipError, match=err_arg + "trace_decode_begin"):
            eng.decode_begin([0], [0], rig.max_new, eos=-1, forced=[[1] * rig.max_new])
    finally:
        eng.set_logits_params(None)
    eng.decode_begin([0], [0], rig.max_new, eos=-1, forced=[[1] * rig.max_new])           # disarmed: forced ids are welcome again
    with pytest.raises(ValueError, match="forced"):
        eng.decode([0], [0], rig.max_new, forced=[[1] * rig.max_new], logits=LogitsParams(1.2))
    lg = torch.zeros((1, P.dims(rig.cfg)[3]), device="cuda")
    z = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.TraceHipError, match="alias"):                                  # out may not be the input
        eng.lib.trace_op_logits_process(lg.data_ptr(), lg.shape[1], 1, z.data_ptr(), rig.cfg.vocab_size, rig.cfg.time_vocab_size, rig.cfg.score_vocab_size,
                                        z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), -1, 1.2, 0, 0, lg.data_ptr(), None)


# ---------------------------------------------------------------------------------------------------------------- 5: model.generate
def test_model_generate_takes_the_three_arguments_in_both_loops(tmp_path_factory):
    """generate(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2) on the tiny model: the device loop, and the same call with a
    stopping criterion that never fires (the stepwise loop through the loose-row op) - identical ids; the processors change the greedy ids, no id
    pair repeats, and EOS is not among the first two tokens"""
    from trace_amd.mm_utils import get_model_name_from_path
    from trace_amd.model.builder import load_pretrained_model, save_synthetic_checkpoint
    path = str(tmp_path_factory.mktemp("ckpt") / "trace-tiny")
    cfg = tcfg.tiny(num_frames=4)
    save_synthetic_checkpoint(path, cfg)
    tok, model, proc, _ = load_pretrained_model(path, None, get_model_name_from_path(path), max_batch=2, max_new_tokens=32)
    try:
        frames = synth.synth_frames(cfg, 0).to(torch.bfloat16).cuda()
        ts = [[i * 2.5] for i in range(4)]
        ids = synth.synth_prompt_ids(cfg, n_text=24, video_pos=10).unsqueeze(0)
        kw = dict(images_or_videos=[frames], modal_list=["video"], video_timestamps=[ts], max_new_tokens=24, eos_token_id=cfg.eos_token_id)
        for head in (0, 1):
            plain = model.generate(ids, heads=[head], **kw)[0].tolist()
            a = model.generate(ids, heads=[head], repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2, **kw)[0].tolist()
            b = model.generate(ids, heads=[head], repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2,
                               stopping_criteria=[lambda i, s: False], **kw)[0].tolist()
            assert a == b, (head, a, b)
            gen = a[:a.index(cfg.eos_token_id) + 1] if cfg.eos_token_id in a else a
            pairs = list(zip(gen, gen[1:]))
            assert len(set(pairs)) == len(pairs), (head, gen)
            assert cfg.eos_token_id not in gen[:2]
            print(f"head {head}: plain {plain}\n         processed {a}")
        c = model.generate(ids, heads=[0], generation_config={"no_repeat_ngram_size": 1}, **kw)[0].tolist()
        gen = c[:c.index(cfg.eos_token_id) + 1] if cfg.eos_token_id in c else c
        assert len(set(gen)) == len(gen), gen                          # n = 1: no id twice
    finally:
        model.engine.close()
