"""Cost of the logits processors per decode step, synthetic TRACE-7B: interleaved rounds of ms per step (trace_get_profile[0], graph replay) for
four arms — greedy, greedy + processors, sampled (temperature 0.2, top_k 50), sampled + processors — at each batch size.  The processors' arm is
(repetition_penalty 1.2, no_repeat_ngram_size 3, min_new_tokens 0) unless --params says otherwise; the disarmed arms issue the launches of a tree
without the feature (hold them against the parent commit's tools/logprob_ab.py --no-nbest, run as a process of its own beside this one).
python tools/logits_ab.py [--batch 1 128] [--ctx 1968] [--params 1.2 3 0]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trace_amd import config as tcfg, synth  # noqa: E402
from trace_amd.engine import SamplingParams, TraceEngine  # noqa: E402
from trace_amd.sampling import LogitsParams  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[1, 128])
ap.add_argument("--ctx", type=int, default=1968)
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--params", type=float, nargs=3, default=[1.2, 3, 0])
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("logits_ab.py measures on an MI355X: no HIP device visible")
cfg = tcfg.trace_7b()
SP = SamplingParams(0.2, 50, 1.0, 20261016)
LG = LogitsParams(a.params[0], int(a.params[1]), int(a.params[2]))
max_new = 2 + a.steps + 8
ARMS = [("greedy", None, None), ("greedy+proc", None, LG), ("sampled", SP, None), ("sampled+proc", SP, LG)]
print(f"synthetic TRACE-7B, ctx {a.ctx}, {a.steps} steps per round, {a.rounds} interleaved rounds (median of rounds 2..), processors {LG}")


def graph_round(e, B, sampling, lg):
    e.set_sampling(sampling)
    e.set_logits_params(lg)
    try:
        e.decode_begin(list(range(B)), [1] * B, max_new, eos=-1)
        e.decode_steps(2, use_graph=True)            # captures on first use (a graph per batch size and form)
        e.decode_steps(a.steps, use_graph=True)
        prof = e.get_profile()[0]
        ids, _ = e.decode_read()
    finally:
        e.set_logits_params(None)
        e.set_sampling(None)
    return prof, ids


for B in a.batch:
    torch.manual_seed(0)
    e = TraceEngine(cfg, max_batch=B, max_ctx=a.ctx + max_new + 32, max_frames=128, max_new_tokens=max_new)
    e.load_weights(synth.iter_weights(cfg, device="cuda"))
    for s in range(B):
        e.prefill(s, a.ctx, embeds=(torch.randn(a.ctx, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16))
    e.set_profile(1)
    res = {k: [] for k, _, _ in ARMS}
    ids_of = {}
    for rnd in range(a.rounds):
        for k, sp, lg in ARMS:
            p, ids = graph_round(e, B, sp, lg)
            res[k].append(p)
            assert ids_of.setdefault(k, ids) == ids, f"{k}: ids differ between rounds"
    med = {k: statistics.median(v[1:] if len(v) > 1 else v) for k, v in res.items()}
    for k, v in res.items():
        print(f"B={B:4d} {k:13s} {med[k]:8.3f} device ms/step (graph)   rounds: {' '.join('%.3f' % x for x in v)}")
    rep = lambda ids: sum(1 for r in ids for i in range(2, len(r)) if tuple(r[i - 2:i + 1]) in {tuple(r[j - 2:j + 1]) for j in range(2, i)})
    print(f"B={B:4d} greedy+proc / greedy = {med['greedy+proc'] / med['greedy']:.4f}   sampled+proc / sampled = {med['sampled+proc'] / med['sampled']:.4f}"
          f"   (+{(med['greedy+proc'] - med['greedy']) * 1e3:.1f} / +{(med['sampled+proc'] - med['sampled']) * 1e3:.1f} us per step; repeated 3-grams in the "
          f"greedy rows: {rep(ids_of['greedy'])} without, {rep(ids_of['greedy+proc'])} with)")
    e.close()
    del e
    torch.cuda.empty_cache()
