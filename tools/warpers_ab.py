"""Cost of min_p / typical_p / epsilon_cutoff / eta_cutoff per decode step (trace_amd/csrc/sample.h sample_warp), synthetic TRACE-7B.

Interleaved rounds of ms per step (trace_get_profile[0], graph replay) at each batch size for device sampling with temperature 0.7, top_k 50,
top_p 1: the four off, each of the four armed alone, all four armed.  Every row starts on the text head (the 32 001-wide one, where the sampler
costs the most) and stays there unless it draws <sync>: the arms draw different ids, and a row that wandered onto a 13-wide head would make its arm
look cheaper, so each line also says how many of its ids came from the text head.  --tree DIR imports trace_amd from another checkout (the parent commit built
beside this one): a tree without the warpers runs the off arm only.  Run the trees as separate processes, alternated, two runs each, and hold the
off arms together: the off arm of this tree has to sit inside the run-to-run spread of the parent's.  Per arm: the warm median over the rounds
after the first, with min / max beside it.  --out FILE appends what is printed to FILE (profiles/warpers_ab.txt).
python tools/warpers_ab.py [--tree DIR] [--batch 1 128] [--ctx 1968] [--out FILE]"""
import argparse
import dataclasses
import os
import statistics
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--batch", type=int, nargs="+", default=[1, 128])
ap.add_argument("--ctx", type=int, default=1968)
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from trace_amd import config as tcfg, synth  # noqa: E402
from trace_amd.engine import SamplingParams, TraceEngine  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("warpers_ab.py measures on an MI355X: no HIP device visible")


def say(line):
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


cfg = tcfg.trace_7b()
HAVE = "min_p" in {f.name for f in dataclasses.fields(SamplingParams)}
OFF = SamplingParams(0.7, 50, 1.0, 20261020)
ARMED = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)
ARMS = [("off", OFF)]
if HAVE:
    ARMS += [(name, dataclasses.replace(OFF, **{name: v})) for name, v in ARMED.items()] + [("all", dataclasses.replace(OFF, **ARMED))]
max_new = 2 + a.steps + 8
say(f"tree {'with' if HAVE else 'without'} the warpers; synthetic TRACE-7B, ctx {a.ctx}, {a.steps} steps per "
    f"round, {a.rounds} interleaved rounds (median of rounds 2.., min / max beside it); T 0.7, top_k 50, top_p 1; armed = {ARMED}")


def graph_round(e, B, sp):
    e.set_sampling(sp)
    try:
        e.decode_begin(list(range(B)), [0] * B, max_new, eos=-1)
        e.decode_steps(2, use_graph=True)            # captures on first use (a graph per batch size and form)
        e.decode_steps(a.steps, use_graph=True)
        prof = e.get_profile()[0]
        out, _ = e.decode_read()
    finally:
        e.set_sampling(None)
    return prof, out


for B in a.batch:
    torch.manual_seed(0)
    e = TraceEngine(cfg, max_batch=B, max_ctx=a.ctx + max_new + 32, max_frames=128, max_new_tokens=max_new)
    e.load_weights(synth.iter_weights(cfg, device="cuda"))
    for s in range(B):
        e.prefill(s, a.ctx, embeds=(torch.randn(a.ctx, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16))
    e.set_profile(1)
    res = {k: [] for k, _ in ARMS}
    ids_of = {}
    for rnd in range(a.rounds):
        for k, sp in ARMS:
            p, out = graph_round(e, B, sp)
            res[k].append(p)
            assert ids_of.setdefault(k, out) == out, f"{k}: ids differ between rounds"
    warm = {k: (v[1:] if len(v) > 1 else v) for k, v in res.items()}
    med = {k: statistics.median(v) for k, v in warm.items()}
    for k, v in res.items():
        extra = "" if k == "off" else f"   - off = {(med[k] - med['off']) * 1e3:+.1f} us per step (x{med[k] / med['off']:.4f})"
        text = sum(t <= cfg.vocab_size for r in ids_of[k] for t in r)
        say(f"B={B:4d} {k:15s} {med[k]:8.3f} device ms/step (graph)  min {min(warm[k]):.3f} max {max(warm[k]):.3f}   rounds: "
            f"{' '.join('%.3f' % x for x in v)}   text-head ids {text} of {sum(len(r) for r in ids_of[k])}{extra}")
    e.close()
    del e
    torch.cuda.empty_cache()
