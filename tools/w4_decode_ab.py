"""Decoder weights as bf16, as e4m3 weight-only (llm_fp8="weight_only", W8A16 decode GEMVs) and as w4 (llm_w4=True): synthetic TRACE-7B, a FRESH CHILD
PROCESS per configuration and round, the rounds interleaved (bf16, w8a16, w4, bf16, ...), so that neither clocks nor allocator state favour one.  A child
builds its engine, prefills context --ctx, and reports: device ms per decode step (trace_get_profile[0], graph replay) at every --batch size; the wall
ms of one 256-token B = 1 call (decode_begin + 255 graph-replayed steps + decode_read); the ms of a prefill of one (--ctx - 1)-row prompt and of seven
such prompts in one pass (HIP events, second of two runs) — the w4 engine dequantises each layer's projections once per pass, so the pair shows the
dequantiser's share; trace_ctx_device_bytes.  The parent prints, per figure, the warm median over the rounds after the first with min / max.
python tools/w4_decode_ab.py [--batch 1 16 64] [--ctx 1968] [--steps 253] [--rounds 4] [--out profiles/w4_decode_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = ("bf16", "w8a16", "w4")

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[1, 16, 64])
ap.add_argument("--ctx", type=int, default=1968)
ap.add_argument("--steps", type=int, default=253)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--out", default=None)
ap.add_argument("--child", choices=CONFIGS, default=None)
a = ap.parse_args()


def child(name):
    import torch
    from trace_amd import config as tcfg, synth
    from trace_amd.engine import TraceEngine
    cfg = tcfg.trace_7b()
    cfg.num_hidden_layers = a.layers
    max_new = 2 + a.steps + 8
    Bmax, Lp = max(a.batch), a.ctx - 1
    max_ctx = max(a.ctx + max_new + 32, (7 * Lp + 3) // 4 + 1)          # the prefill workspaces hold 4 x max_ctx rows: room for seven prompts in one pass
    torch.manual_seed(0)
    e = TraceEngine(cfg, max_batch=max(Bmax, 7), max_ctx=max_ctx, max_frames=128, max_new_tokens=max_new,
                    llm_fp8="weight_only" if name == "w8a16" else False, llm_w4=name == "w4")
    e.load_weights(synth.iter_weights(cfg, device="cuda"))
    out = {"config": name, "device_bytes": e.device_bytes(), "max_ctx": max_ctx}
    emb = (torch.randn(a.ctx, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])
    one = emb[:Lp].contiguous()
    out["prefill_1"] = timed(lambda: e.prefill(0, Lp, embeds=one))
    out["prefill_7"] = timed(lambda: e.prefill_multi(0, [one] * 7))
    e.prefill(0, a.ctx, embeds=emb)
    if Bmax > 1:
        e.kv_copy(0, list(range(1, Bmax)), a.ctx)
    e.set_profile(1)
    for B in a.batch:
        ms = []
        for _ in range(2):
            e.decode_begin(list(range(B)), [1] * B, max_new, eos=-1)
            e.decode_steps(2, use_graph=True)
            e.decode_steps(a.steps, use_graph=True)
            ms.append(e.get_profile()[0])
        out[f"step_B{B}"] = ms[1]
    e.set_profile(0)
    wall = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.decode_begin([0], [1], 256, eos=-1)
        e.decode_steps(255, use_graph=True)
        e.decode_read()
        wall.append((time.perf_counter() - t0) * 1e3)
    out["call_256"] = wall[1]
    e.close()
    print("W4AB " + json.dumps(out), flush=True)


def parent():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"synthetic TRACE-7B ({a.layers} layers), decode from context {a.ctx}, {a.steps} graph-replayed steps; a fresh process per configuration and round, "
        f"{a.rounds} interleaved rounds (median of rounds 2.., min / max of those)")
    res = {c: [] for c in CONFIGS}
    for rnd in range(a.rounds):
        for c in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", c, "--ctx", str(a.ctx), "--steps", str(a.steps), "--layers", str(a.layers),
                   "--batch", *[str(b) for b in a.batch]]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            got = [ln[5:] for ln in r.stdout.splitlines() if ln.startswith("W4AB ")]
            if r.returncode != 0 or not got:
                sys.exit(f"child {c} round {rnd} failed (rc {r.returncode}):\n{r.stderr[-2000:]}")
            res[c].append(json.loads(got[0]))
            print(f"  round {rnd} {c}: {got[0]}", flush=True)
    keys = [f"step_B{b}" for b in a.batch] + ["call_256", "prefill_1", "prefill_7"]
    label = {"call_256": "one 256-token B = 1 call, wall ms", "prefill_1": f"prefill, one {a.ctx - 1}-row prompt, ms", "prefill_7": f"prefill, seven {a.ctx - 1}-row prompts in one pass, ms"}
    med, spread = {}, {}
    for k in keys:
        for c in CONFIGS:
            v = [x[k] for x in res[c]]
            use = v[1:] if len(v) > 1 else v
            med[k, c], spread[k, c] = statistics.median(use), max(use) - min(use)
            say(f"{label.get(k, 'decode ms / step, B = ' + k[6:]):58s} {c:6s} {med[k, c]:9.3f} (min {min(use):.3f} max {max(use):.3f})   rounds: {' '.join('%.3f' % x for x in v)}")
        say(f"{'':58s} w4 / w8a16 = {med[k, 'w4'] / med[k, 'w8a16']:.4f}, w4 / bf16 = {med[k, 'w4'] / med[k, 'bf16']:.4f}")
    k = f"step_B{a.batch[0]}"
    gain, noise = med[k, "w8a16"] - med[k, "w4"], spread[k, "w8a16"] + spread[k, "w4"]
    say(f"B = {a.batch[0]} step: w8a16 - w4 = {gain * 1e3:+.0f} us against a combined min-max spread of {noise * 1e3:.0f} us -> "
        f"{'w4 is faster by more than the spread' if gain > noise else 'w4 is NOT faster by more than the spread'}")
    say(f"dequantiser share of a prefill: w4 - bf16 = {med['prefill_1', 'w4'] - med['prefill_1', 'bf16']:+.2f} ms for one prompt, "
        f"{med['prefill_7', 'w4'] - med['prefill_7', 'bf16']:+.2f} ms for seven in one pass")
    for c in CONFIGS:
        say(f"trace_ctx_device_bytes {c:6s} {res[c][0]['device_bytes'] / 1e9:8.2f} GB (max_batch {max(max(a.batch), 7)}, max_ctx {res[c][0]['max_ctx']})")
    say(f"  bf16 - w4 = {(res['bf16'][0]['device_bytes'] - res['w4'][0]['device_bytes']) / 1e9:.2f} GB, w8a16 - w4 = "
        f"{(res['w8a16'][0]['device_bytes'] - res['w4'][0]['device_bytes']) / 1e9:.2f} GB")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if a.child:
    child(a.child)
else:
    import torch
    if not torch.cuda.is_available():
        sys.exit("w4_decode_ab.py measures on an MI355X: no HIP device visible")
    parent()
