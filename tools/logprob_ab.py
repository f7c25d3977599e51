"""Cost of per-token log-probabilities per decode step, synthetic TRACE-7B: interleaved rounds of ms per step (trace_get_profile[0], graph replay)
for four arms — greedy, greedy + logprobs, sampled (temperature 0.2, top_k 50), sampled + logprobs — at each batch size; and one n-best line at
the C2 shape (128 frames, L = 1967): wall ms of generate_samples(n = 8) against generate() of the prompt repeated eight times (eight towers and
prefills), same SamplingParams, the results compared.   python tools/logprob_ab.py [--batch 1 128] [--ctx 1968] [--nbest-new 32] [--no-nbest]"""
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
ap.add_argument("--nbest-new", type=int, default=32)
ap.add_argument("--nbest-rounds", type=int, default=3)
ap.add_argument("--no-nbest", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("logprob_ab.py measures on an MI355X: no HIP device visible")
cfg = tcfg.trace_7b()
SP = SamplingParams(0.2, 50, 1.0, 20261016)
max_new = 2 + a.steps + 8
ARMS = [("greedy", None, False), ("greedy+lp", None, True), ("sampled", SP, False), ("sampled+lp", SP, True)]
print(f"synthetic TRACE-7B, ctx {a.ctx}, {a.steps} steps per round, {a.rounds} interleaved rounds (median of rounds 2..)")


def graph_round(e, B, sampling, lp):
    e.set_sampling(sampling)
    e.set_logprobs(lp)
    try:
        e.decode_begin(list(range(B)), [1] * B, max_new, eos=-1)
        e.decode_steps(2, use_graph=True)            # captures on first use (a graph per batch size and form)
        e.decode_steps(a.steps, use_graph=True)
        prof = e.get_profile()[0]
        ids, _ = e.decode_read()
        vals = e.decode_read_logprobs([len(x) for x in ids]) if lp else None
    finally:
        e.set_logprobs(False)
        e.set_sampling(None)
    return prof, ids, vals


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
        for k, sp, lp in ARMS:
            p, ids, vals = graph_round(e, B, sp, lp)
            res[k].append(p)
            key = "sampled" if sp is not None else "greedy"
            assert ids_of.setdefault(key, ids) == ids, f"{k}: ids differ from the {key} arm's"      # logprobs on changes no id
            if vals is not None:
                assert all(len(v) == len(x) and bool((v <= 0).all()) for v, x in zip(vals, ids))
    med = {k: statistics.median(v[1:] if len(v) > 1 else v) for k, v in res.items()}
    for k, v in res.items():
        print(f"B={B:4d} {k:11s} {med[k]:8.3f} device ms/step (graph)   rounds: {' '.join('%.3f' % x for x in v)}")
    print(f"B={B:4d} greedy+lp / greedy = {med['greedy+lp'] / med['greedy']:.4f}   sampled+lp / sampled = {med['sampled+lp'] / med['sampled']:.4f}"
          f"   sampled / greedy = {med['sampled'] / med['greedy']:.4f}   (ids identical with the setting on and off: True)")
    e.close()
    del e
    torch.cuda.empty_cache()

if not a.no_nbest:
    cfg = tcfg.trace_7b(128)
    L, n_new, N = 1967, a.nbest_new, 8
    e = TraceEngine(cfg, max_batch=N, max_ctx=(L + n_new + 63) // 64 * 64, max_frames=128, max_new_tokens=n_new)
    e.load_weights(synth.iter_weights(cfg, device="cuda:0"))
    frames = synth.synth_frames(cfg, 0, num_frames=128, device="cuda").to(torch.bfloat16)
    ts = [[i * 2.0] for i in range(128)]
    prompt = synth.synth_prompt_ids(cfg, n_text=176, video_pos=150).tolist()
    sp = SamplingParams(1.0, 50, 1.0, 20261016)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    rep = lambda: e.generate([frames] * N, [ts] * N, [prompt] * N, [1] * N, n_new, sampling=sp, logprobs=True)
    nb = lambda: e.generate_samples(frames, ts, prompt, 1, N, n_new, sampling=sp)
    rep(); nb()                                                                # warm: graphs captured, workspaces sized
    t_rep, t_nb, same = [], [], True
    for _ in range(a.nbest_rounds):
        t, r1 = timed(rep)
        t_rep.append(t)
        t, r2 = timed(nb)
        t_nb.append(t)
        same = same and r1[0] == r2[0] and all((x.view("uint32") == y.view("uint32")).all() for x, y in zip(r1[2], r2[2]))
    m_rep, m_nb = statistics.median(t_rep), statistics.median(t_nb)
    print(f"n-best, C2 shape (128 frames, L = {L}, {n_new} new tokens, n = {N}): generate() of the prompt repeated {N} times {m_rep:9.1f} wall ms "
          f"[{' '.join('%.1f' % x for x in t_rep)}]   generate_samples(n = {N}) {m_nb:9.1f} wall ms [{' '.join('%.1f' % x for x in t_nb)}]   "
          f"ratio {m_nb / m_rep:.3f}   (ids and log-probability bits identical: {same}; distinct rows: {len({tuple(x) for x in r2[0]})})")
    e.close()
