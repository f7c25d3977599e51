"""The e4m3 KV cache against the 16-bit cache: synthetic TRACE-7B, one process, both engines alive (built once, for the largest batch), rounds
interleaved.  Per batch size, from context --ctx on: device ms per decode step (trace_get_profile[0], graph replay; warm median of the rounds after the
first, with min / max), and from eager steps with one HIP-event bracket per step (trace_set_profile(2) with trace_set_profile_brackets 4 / 8) the us of
the layer-0 decode attention launch and of the layer-0 append launch.  The 16-bit engine appends inside its attention launch up to 64 rows (no append
launch of its own: its attention figure includes the append); kv8 always appends with qkv_finish_kv8.  Beside the attention launch: its achieved bytes/s
over the algorithmic K + V bytes (512 per position and kv head, or 264) as a fraction of the HBM peak (tools/roofline_hbm's figure for the 16-bit
kernel at B = 128 is 0.71).  Last: the device bytes of both contexts and the largest max_batch that fits a card at --fit-ctx.
python tools/kv8_ab.py [--batch 128 16 1] [--ctx 1968] [--steps 253] [--rounds 5] [--out profiles/kv8_decode_ab.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trace_amd import _lib, config as tcfg, kv8, synth  # noqa: E402
from trace_amd.engine import TraceEngine  # noqa: E402

HBM_PEAK = 8.0e12                 # bytes/s, MI355X

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[128, 16, 1])
ap.add_argument("--ctx", type=int, default=1968)
ap.add_argument("--steps", type=int, default=253)                    # 2 + 253 steps: contexts 1968 -> 2223, the C2 decode shape
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--fit-ctx", type=int, default=2304)
ap.add_argument("--card-gb", type=float, default=288.0)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("kv8_ab.py measures on an MI355X: no HIP device visible")
cfg = tcfg.trace_7b()
max_new = 2 + a.steps + 8
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


say(f"synthetic TRACE-7B ({cfg.num_hidden_layers} layers), decode from context {a.ctx}, {a.steps} graph-replayed steps per round, {a.rounds} interleaved "
    f"rounds (median of rounds 2.., min / max of those)")


def graph_round(e, B):
    e.decode_begin(list(range(B)), [1] * B, max_new, eos=-1)
    e.decode_steps(2, use_graph=True)                # captures on first use
    e.decode_steps(a.steps, use_graph=True)
    return e.get_profile()[0]


def bracket_round(e, B, bit, steps=6):
    """eager steps with one per-launch bracket (bit 4: the layer-0 decode attention, 8: the layer-0 append launch):
    (mean ms of the bracketed launch, its algorithmic bytes, samples)"""
    _lib.check(e.lib.trace_set_profile_brackets(e.h, bit))
    e.set_profile(2)
    e.decode_begin(list(range(B)), [1] * B, max_new, eos=-1)
    e.decode_steps(steps, use_graph=False)
    p = e.get_profile()
    e.set_profile(1)
    _lib.check(e.lib.trace_set_profile_brackets(e.h, 3))
    return p[2], p[4], int(p[3])


def launch_us(engs, B, bit):
    """{engine: (median us over 5 interleaved bracket rounds after a warm one, min, max, bytes)}; None where the step has no such launch"""
    got = {k: [] for k in engs}
    for rnd in range(6):
        for k, e in engs.items():
            got[k].append(bracket_round(e, B, bit))
    out = {}
    for k, v in got.items():
        v = [x for x in v[1:] if x[2] > 0]
        us = [x[0] * 1e3 for x in v]
        out[k] = (statistics.median(us), min(us), max(us), v[0][1]) if v else None
    return out


Bmax = max(a.batch)
torch.manual_seed(0)
engs, bytes_of = {}, {}
for name, kv in (("16-bit", None), ("kv8", "fp8")):
    e = TraceEngine(cfg, max_batch=Bmax, max_ctx=a.ctx + max_new + 32, max_frames=128, max_new_tokens=max_new, kv_cache=kv)
    e.load_weights(synth.iter_weights(cfg, device="cuda"))
    engs[name] = e
    bytes_of[name] = (e.device_bytes(), e.max_ctx)
emb = (torch.randn(a.ctx, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16)
for e in engs.values():
    e.prefill(0, a.ctx, embeds=emb)
    if Bmax > 1:
        e.kv_copy(0, list(range(1, Bmax)), a.ctx)       # every row the same prompt: the step's time does not depend on what the rows hold
    e.set_profile(1)
for B in a.batch:
    res = {k: [] for k in engs}
    for rnd in range(a.rounds):
        for k, e in engs.items():
            res[k].append(graph_round(e, B))
    use = {k: (v[1:] if len(v) > 1 else v) for k, v in res.items()}
    med = {k: statistics.median(v) for k, v in use.items()}
    for k in engs:
        say(f"B={B:4d} {k:7s} {med[k]:8.3f} ms/step (min {min(use[k]):.3f} max {max(use[k]):.3f})   rounds: {' '.join('%.3f' % x for x in res[k])}")
    say(f"B={B:4d} kv8 / 16-bit = {med['kv8'] / med['16-bit']:.4f}  ({(med['kv8'] - med['16-bit']) * 1e3:+.0f} us per step, "
        f"{(med['kv8'] - med['16-bit']) * 1e3 / cfg.num_hidden_layers:+.1f} us per layer)")
    att, app = launch_us(engs, B, 4), launch_us(engs, B, 8)
    for k in engs:
        us, lo, hi, by = att[k]
        say(f"B={B:4d} {k:7s} layer-0 decode attention launch {us:7.1f} us (min {lo:.1f} max {hi:.1f}), {by / 1e6:.2f} MB of K + V -> "
            f"{by / (us * 1e-6) / 1e12:.2f} TB/s = {by / (us * 1e-6) / HBM_PEAK:.2f} of the HBM peak")
        if app[k]:
            say(f"B={B:4d} {k:7s} layer-0 append launch           {app[k][0]:7.1f} us (min {app[k][1]:.1f} max {app[k][2]:.1f})")
        else:
            say(f"B={B:4d} {k:7s} no append launch: this step appends inside the attention launch")
for e in engs.values():
    e.close()
del engs, e
torch.cuda.empty_cache()

# capacity: the context's bytes are (everything but the cache) + slots x (cache bytes per slot); the first term from a measured context
NL, NKV = cfg.num_hidden_layers, cfg.num_key_value_heads
ctx_pad = (a.fit_ctx + 63) // 64 * 64
say(f"capacity at max_ctx {a.fit_ctx} on a {a.card_gb:.0f} GB card (device bytes of the measured contexts minus their caches, plus slots x cache per slot):")
for name, fp8 in (("16-bit", False), ("kv8", True)):
    B0 = Bmax
    total, mc = bytes_of[name]
    per_slot_meas = NL * ((mc + 63) // 64 * 64) * kv8.cache_bytes_per_position(NKV, fp8)
    fixed = total - B0 * per_slot_meas
    per_slot = NL * ctx_pad * kv8.cache_bytes_per_position(NKV, fp8)
    fit = int((a.card_gb * 1e9 - fixed) // per_slot)
    say(f"  {name:7s} context of {B0} slots x {mc}: {total / 1e9:.2f} GB ({fixed / 1e9:.2f} GB besides the cache); {per_slot / 1e6:.1f} MB per slot at "
        f"{a.fit_ctx} -> largest max_batch {min(fit, 512)}{' (the library caps the slots at 512)' if fit > 512 else ''}  [{fit} by bytes]")
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
