"""Cost of sampling per decode step, synthetic TRACE-7B: interleaved A/B of ms per step (trace_get_profile[0], graph replay) for greedy vs device
sampling (temperature 0.2, top_k 50), beside the host-driven stepwise loop the sampled generate() used before (eager step, the [B, NV] logits
to torch, softmax + multinomial, trace_decode_feed; wall ms per step).   python tools/sample_ab.py [--batch 1 128] [--ctx 1968]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trace_amd import config as tcfg, synth  # noqa: E402
from trace_amd.engine import SamplingParams, TraceEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[1, 128])
ap.add_argument("--ctx", type=int, default=1968)
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
cfg = tcfg.trace_7b()
SP = SamplingParams(0.2, 50, 1.0, 20261016)
max_new = 2 + a.steps + 8
print(f"synthetic TRACE-7B, ctx {a.ctx}, {a.steps} steps per round, {a.rounds} interleaved rounds (median of rounds 2..)")


def graph_round(e, B, sampling):
    e.set_sampling(sampling)
    e.decode_begin(list(range(B)), [1] * B, max_new, eos=-1)
    e.decode_steps(2, use_graph=True)            # captures on first use (a graph per batch size and form)
    e.decode_steps(a.steps, use_graph=True)
    prof = e.get_profile()[0]
    ids, _ = e.decode_read()
    e.set_sampling(None)
    return prof, ids


def stepwise_round(e, B):
    e.host_mode(True)
    try:
        lg = e.decode_begin(list(range(B)), [1] * B, max_new, eos=-1, want_logits=True)
        e.feed(torch.multinomial(torch.softmax(lg / 0.2, -1), 1).view(-1).tolist())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            lg = e.decode_steps(1, use_graph=False, want_logits=True)
            e.feed(torch.multinomial(torch.softmax(lg / 0.2, -1), 1).view(-1).tolist())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3
    finally:
        e.host_mode(False)


for B in a.batch:
    torch.manual_seed(0)
    e = TraceEngine(cfg, max_batch=B, max_ctx=a.ctx + max_new + 32, max_frames=128, max_new_tokens=max_new)
    e.load_weights(synth.iter_weights(cfg, device="cuda"))
    for s in range(B):
        e.prefill(s, a.ctx, embeds=(torch.randn(a.ctx, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16))
    e.set_profile(1)
    res = {"greedy": [], "sampled": [], "stepwise": []}
    ids_s = None
    for rnd in range(a.rounds):
        res["greedy"].append(graph_round(e, B, None)[0])
        p, ids = graph_round(e, B, SP)
        res["sampled"].append(p)
        assert ids_s is None or ids == ids_s, "sampled ids differ between rounds"
        ids_s = ids
        res["stepwise"].append(stepwise_round(e, B))
    med = {k: statistics.median(v[1:] if len(v) > 1 else v) for k, v in res.items()}
    for k, v in res.items():
        unit = "device ms/step (graph)" if k != "stepwise" else "wall ms/step (eager + host)"
        print(f"B={B:4d} {k:9s} {med[k]:8.3f} {unit}   rounds: {' '.join('%.3f' % x for x in v)}")
    print(f"B={B:4d} sampled / greedy = {med['sampled'] / med['greedy']:.4f}   stepwise / greedy = {med['stepwise'] / med['greedy']:.2f}x"
          f"   (sampled ids identical in every round: True)")
    e.close()
    del e
    torch.cuda.empty_cache()
