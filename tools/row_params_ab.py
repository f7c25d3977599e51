"""Cost of per-row generation parameters per decode step (select_next_kernel<SELECT_PER_ROW>, trace_amd/csrc/select.h), synthetic TRACE-7B.

Interleaved rounds of ms per step (trace_get_profile[0], graph replay) at each batch size, every row on the text head (the 32 001-wide one):
  off-greedy / off-sampled     the batch-wide settings (greedy; T 0.7, top_k 50, top_p 1) — the arms a tree without per-row params also runs;
  rows-greedy / rows-sampled   the same params as one RowParams in every row (armed, uniform);
  rows-mixed                   half the rows greedy, half sampled, a seed per row (armed, mixed; batch 1 has no halves and skips it);
  queue                        (--queue, batch >= 2) decode_queue over 2 B prefilled slots through B rows, half max_new_tokens 32 and half 256:
                               rows x steps and wall time with per-row bounds in one queue, against two queues of one bound each (what a tree
                               without per-row params has to do).
--tree DIR imports trace_amd from another checkout (the parent commit built beside this one): a tree without per-row params runs the off arms and
the two-queue side only.  Run the trees as separate processes, alternated, two runs each, and hold the off arms together: this tree's have to sit
inside the parent's own round-to-round and run-to-run spread.  Per arm: the warm median over the rounds after the first, with min / max beside it.
--out FILE appends what is printed to FILE (profiles/row_params_ab.txt).
python tools/row_params_ab.py [--tree DIR] [--batch 1 128] [--ctx 1968] [--queue] [--out FILE]"""
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
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--queue", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))
from trace_amd import config as tcfg, sampling as tsamp, synth  # noqa: E402
from trace_amd.engine import SamplingParams, TraceEngine  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("row_params_ab.py measures on an MI355X: no HIP device visible")


def say(line):
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


cfg = tcfg.trace_7b()
HAVE = hasattr(tsamp, "RowParams")
RowParams = getattr(tsamp, "RowParams", None)
SP = SamplingParams(0.7, 50, 1.0, 20261021)
QUEUE_NEW = (32, 256)
max_new = max(2 + a.steps + 8, QUEUE_NEW[1] if a.queue else 0)
say(f"tree {'with' if HAVE else 'without'} per-row params; synthetic TRACE-7B, ctx {a.ctx}, {a.steps} steps per round, {a.rounds} interleaved "
    f"rounds (median of rounds 2.., min / max beside it); sampled = T 0.7, top_k 50, top_p 1")


def arms_for(B):
    arms = [("off-greedy", dict(sampling=None)), ("off-sampled", dict(sampling=SP))]
    if HAVE:
        seeded = lambda b: SamplingParams(0.7, 50, 1.0, 20261021 + b)
        arms += [("rows-greedy", dict(rows=[RowParams()] * B)), ("rows-sampled", dict(rows=[RowParams(SP)] * B))]
        if B > 1:
            arms.append(("rows-mixed", dict(rows=[RowParams(seeded(b)) if b % 2 else RowParams() for b in range(B)])))
    return arms


def graph_round(e, B, sampling=None, rows=None):
    e.set_sampling(sampling)
    try:
        kw = dict(row_params=rows) if rows is not None else {}
        e.decode_begin(list(range(B)), [0] * B, max_new, eos=-1, **kw)
        e.decode_steps(2, use_graph=True)            # captures on first use (a graph per batch size and form)
        e.decode_steps(a.steps, use_graph=True)
        prof = e.get_profile()[0]
        out, _ = e.decode_read()
    finally:
        e.set_sampling(None)
    return prof, out


def queue_round(e, B):
    """2 B prefilled slots through B rows, half at each bound: (rows x steps, wall ms) of one queue with per-row bounds and of two queues of one bound"""
    slots = list(range(2 * B))
    short = [s for s in slots if s % 2 == 0]
    longs = [s for s in slots if s % 2]
    res = {}
    if HAVE:
        s0, t0 = e.stats["decode_row_steps"], time.perf_counter()
        e.decode_queue(slots, [0] * len(slots), QUEUE_NEW[1], -1, max_rows=B, row_params=[RowParams(max_new_tokens=QUEUE_NEW[s % 2]) for s in slots])
        torch.cuda.synchronize()
        res["one queue, per-row bounds"] = (e.stats["decode_row_steps"] - s0, (time.perf_counter() - t0) * 1e3)
    s0, t0 = e.stats["decode_row_steps"], time.perf_counter()
    e.decode_queue(short, [0] * len(short), QUEUE_NEW[0], -1, max_rows=B)
    e.decode_queue(longs, [0] * len(longs), QUEUE_NEW[1], -1, max_rows=B)
    torch.cuda.synchronize()
    res["two queues, one bound each"] = (e.stats["decode_row_steps"] - s0, (time.perf_counter() - t0) * 1e3)
    return res


for B in a.batch:
    torch.manual_seed(0)
    nslots = 2 * B if a.queue and B > 1 else B
    e = TraceEngine(cfg, max_batch=nslots, max_ctx=a.ctx + max_new + 32, max_frames=128, max_new_tokens=max_new)
    e.load_weights(synth.iter_weights(cfg, device="cuda"))
    for s in range(nslots):
        e.prefill(s, a.ctx, embeds=(torch.randn(a.ctx, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16))
    e.set_profile(1)
    arms = arms_for(B)
    res = {k: [] for k, _ in arms}
    ids_of = {}
    for rnd in range(a.rounds):
        for k, kw in arms:
            p, out = graph_round(e, B, **kw)
            res[k].append(p)
            assert ids_of.setdefault(k, out) == out, f"{k}: ids differ between rounds"
    if HAVE:
        assert ids_of["rows-greedy"] == ids_of["off-greedy"] and ids_of["rows-sampled"] == ids_of["off-sampled"], "uniform row params draw other ids"
    warm = {k: (v[1:] if len(v) > 1 else v) for k, v in res.items()}
    med = {k: statistics.median(v) for k, v in warm.items()}
    for k, v in res.items():
        base = "off-sampled" if k == "rows-sampled" else "off-greedy"
        extra = "" if k.startswith("off") else f"   - {base} = {(med[k] - med[base]) * 1e3:+.1f} us per step (x{med[k] / med[base]:.4f})"
        say(f"B={B:4d} {k:13s} {med[k]:8.3f} device ms/step (graph)  min {min(warm[k]):.3f} max {max(warm[k]):.3f}   rounds: "
            f"{' '.join('%.3f' % x for x in v)}{extra}")
    if a.queue and B > 1:
        e.set_profile(0)
        queue_round(e, B)                                # captures every batch size the schedule visits
        for name, (steps, ms) in queue_round(e, B).items():
            say(f"B={B:4d} queue, {2 * B} requests, max_new_tokens {QUEUE_NEW[0]} / {QUEUE_NEW[1]} by halves: {name}: {steps} rows x steps, {ms:.1f} ms wall")
    e.close()
    del e
    torch.cuda.empty_cache()
