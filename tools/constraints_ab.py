"""Cost of the constraints (bad words, suppressed ids, stop sequences: trace_amd/csrc/constrain.h) per decode step, and the host loop against the
device, synthetic TRACE-7B.

Step cost: interleaved rounds of ms per step (trace_get_profile[0], graph replay) at each batch size for greedy and sampled (temperature 0.2,
top_k 50), each unarmed and armed with 8 stop sequences of 1-4 ids, 16 bad words and 64 suppressed ids.  --tree DIR imports trace_amd from another
checkout (the parent commit built beside this one): a tree without the feature runs the unarmed arms only.  Run the trees as separate processes,
alternated, two runs each, and hold the unarmed arms together.

Host loop against the device (--host-loop, this tree only): one B = 1 model.generate() call of 256 new tokens with
stopping_criteria=[KeywordsStoppingCriteria(["</s>"], ...)] — one eager step, a logits read-back, a host pick, a feed and a read per token —
against the same call with stop_sequences=stop_sequences_from_keywords(criterion): the captured decode step.  Wall ms of each call after a warm-up
call, the ids compared, and the wall of a 1-token call (the encode and prefill both calls share).
python tools/constraints_ab.py [--tree DIR] [--batch 1 128] [--ctx 1968] [--host-loop]"""
import argparse
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--batch", type=int, nargs="+", default=[1, 128])
ap.add_argument("--ctx", type=int, default=1968)
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--host-loop", action="store_true")
ap.add_argument("--new-tokens", type=int, default=256)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from trace_amd import config as tcfg, sampling, synth  # noqa: E402
from trace_amd.engine import SamplingParams, TraceEngine  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("constraints_ab.py measures on an MI355X: no HIP device visible")
cfg = tcfg.trace_7b()
HAVE = hasattr(sampling, "Constraints")
SP = SamplingParams(0.2, 50, 1.0, 20261019)
CONS = None
if HAVE:
    g = torch.Generator().manual_seed(11)
    ids = lambda n: torch.randint(3, cfg.total_vocab, (n,), generator=g).tolist()
    CONS = sampling.Constraints(stop_sequences=[ids(1 + i % 4) for i in range(8)], bad_words_ids=[ids(1 + i % 3) for i in range(16)],
                                suppress_tokens=ids(64))
max_new = 2 + a.steps + 8
ARMS = [("greedy", None, None), ("sampled", SP, None)] + ([("greedy+cons", None, CONS), ("sampled+cons", SP, CONS)] if HAVE else [])
print(f"tree {'with' if HAVE else 'without'} constraints; synthetic TRACE-7B, ctx {a.ctx}, {a.steps} steps per round, {a.rounds} interleaved rounds "
      f"(median of rounds 2..); armed = 8 stop sequences of 1-4 ids, 16 bad words of 1-3 ids, 64 suppressed ids", flush=True)


def graph_round(e, B, sp, cons):
    e.set_sampling(sp)
    if HAVE:
        e.set_constraints(cons)
    try:
        e.decode_begin(list(range(B)), [1] * B, max_new, eos=-1)
        e.decode_steps(2, use_graph=True)            # captures on first use (a graph per batch size and form)
        e.decode_steps(a.steps, use_graph=True)
        prof = e.get_profile()[0]
        out, _ = e.decode_read()
    finally:
        if HAVE:
            e.set_constraints(None)
        e.set_sampling(None)
    return prof, out


def host_loop(e):
    from trace_amd.mm_utils import KeywordsStoppingCriteria, stop_sequences_from_keywords
    from trace_amd.model.builder import ByteTokenizer
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    model, tok = TraceMistralForCausalLM(cfg, e, None), ByteTokenizer(cfg.vocab_size)
    frames = synth.synth_frames(cfg, 0, device="cuda").to(torch.bfloat16)
    ts = [[i * 2.0] for i in range(cfg.num_frames)]
    prompt = synth.synth_prompt_ids(cfg).unsqueeze(0)
    crit = KeywordsStoppingCriteria(["</s>"], tok, prompt)
    kw = dict(images_or_videos=[frames], modal_list=["video"], video_timestamps=[ts], heads=[0], eos_token_id=-1)

    def timed(n, **extra):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(prompt, max_new_tokens=n, **kw, **extra)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out[0].tolist()
    seqs = stop_sequences_from_keywords(crit)
    res = {}
    for name, extra in (("stopping_criteria (host loop)", {"stopping_criteria": [crit]}), ("stop_sequences (device)", {"stop_sequences": seqs})):
        timed(a.new_tokens, **extra)                   # warm-up: graph capture, allocations
        runs = [timed(a.new_tokens, **extra) for _ in range(3)]
        one = [timed(1, **extra)[0] for _ in range(2)]
        res[name] = (statistics.median(r[0] for r in runs), runs[0][1], min(one))
        print(f"B=1 {a.new_tokens} new tokens  {name:30s} {res[name][0]:9.1f} wall ms per call (runs: {' '.join('%.1f' % r[0] for r in runs)}); "
              f"1-token call {min(one):.1f} ms; {len(runs[0][1])} ids returned", flush=True)
    (h, hid, h1), (d, did, d1) = res.values()
    print(f"B=1 host loop / device = {h / d:.2f} x whole call, {(h - h1) / (d - d1):.2f} x behind the shared encode + prefill "
          f"({(h - h1) / (a.new_tokens - 1):.3f} vs {(d - d1) / (a.new_tokens - 1):.3f} ms per token); keyword ids {seqs}; same ids: {hid == did}", flush=True)


for B in a.batch:
    torch.manual_seed(0)
    mn = max(max_new, a.new_tokens + 8) if a.host_loop and B == 1 else max_new
    e = TraceEngine(cfg, max_batch=B, max_ctx=a.ctx + mn + 32, max_frames=128, max_new_tokens=mn)
    e.load_weights(synth.iter_weights(cfg, device="cuda"))
    for s in range(B):
        e.prefill(s, a.ctx, embeds=(torch.randn(a.ctx, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16))
    e.set_profile(1)
    res = {k: [] for k, _, _ in ARMS}
    ids_of = {}
    for rnd in range(a.rounds):
        for k, sp, cons in ARMS:
            p, out = graph_round(e, B, sp, cons)
            res[k].append(p)
            assert ids_of.setdefault(k, out) == out, f"{k}: ids differ between rounds"
    med = {k: statistics.median(v[1:] if len(v) > 1 else v) for k, v in res.items()}
    for k, v in res.items():
        print(f"B={B:4d} {k:13s} {med[k]:8.3f} device ms/step (graph)   rounds: {' '.join('%.3f' % x for x in v)}", flush=True)
    if HAVE:
        print(f"B={B:4d} greedy+cons - greedy = +{(med['greedy+cons'] - med['greedy']) * 1e3:.1f} us per step (x{med['greedy+cons'] / med['greedy']:.4f})   "
              f"sampled+cons - sampled = +{(med['sampled+cons'] - med['sampled']) * 1e3:.1f} us (x{med['sampled+cons'] / med['sampled']:.4f})   "
              f"rows ended by a stop sequence: {sum(len(r) < a.steps + 3 for r in ids_of['greedy+cons'])} of {B}", flush=True)
    if a.host_loop and B == 1 and HAVE:
        e.set_profile(0)
        host_loop(e)
    e.close()
    del e
    torch.cuda.empty_cache()
