"""Continuous batching against the path as it stands, decode side only: synthetic TRACE-7B, context --ctx, --requests requests prefilled beforehand into
as many KV slots, 256 tokens, the answer-length profiles of tools/retire_ab.py ('tail': mean 54, tail to 255; 'last': every answer ends in the last
chunk, where a queue can win nothing).
  arm A  decode(retire_finished=True) over the slots in calls of --rows slots each: what a driver does today;
  arm B  one decode_queue(max_rows=--rows) over all of them: rows that ended leave, waiting slots are admitted (trace_decode_admit).
One process: the weights are loaded and the slots prefilled once, both arms run once unmeasured (that run captures the step graphs of the batch sizes
each arm meets and is timed as 'first'), then the arms alternate A B A B ... for --runs measured runs each; median with min / max.  Forced ids end
the rows as in tools/retire_ab.py (identity-layer weights; a calibrated token whose successor pick is EOS); both arms must record the drawn lengths.
Also: the wall time of one admit_rows of --rows // 8 rows into a batch of --rows - --rows // 8 (host checks, copies, the head and selection of the
new rows, synchronisation), and first - warm per arm (the captures).
python tools/admit_ab.py [--requests 256] [--rows 128] [--ctx 1968] [--runs 3] [--fraction 8] [--out FILE]
profiles/admit_ab.txt holds what --out writes as its first block, marked as such, with hand-written notes below it: write a rerun to another file."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROFILES = ("tail", "last")
MAX_NEW = 256

ap = argparse.ArgumentParser()
ap.add_argument("--requests", type=int, default=256)
ap.add_argument("--rows", type=int, default=128)
ap.add_argument("--ctx", type=int, default=1968)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--seed", type=int, default=20261019)
ap.add_argument("--fraction", type=int, default=None, help="the denominator of the admit rule (TraceEngine.admit_fraction) for this run")
ap.add_argument("--out", default=None)
a = ap.parse_args()


def lengths(profile, n):
    import numpy as np
    rng = np.random.default_rng(a.seed + PROFILES.index(profile))
    if profile == "tail":
        return np.clip(np.rint(np.exp(rng.normal(np.log(40.0), 0.8, n))), 8, MAX_NEW - 1).astype(int).tolist()
    return rng.integers(MAX_NEW - 30, MAX_NEW + 1, n).tolist()


def main():
    import torch
    if not torch.cuda.is_available():
        sys.exit("admit_ab.py measures on an MI355X: no HIP device visible")
    from trace_amd import config as tcfg, synth
    from trace_amd.engine import TraceEngine
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cfg = tcfg.trace_7b()
    cfg.num_hidden_layers = a.layers
    N, R = a.requests, a.rows
    torch.manual_seed(0)
    e = TraceEngine(cfg, max_batch=N, max_ctx=a.ctx + MAX_NEW + 32, max_frames=128, max_new_tokens=MAX_NEW)

    def identity_layers(items):
        for k, t in items:
            if k.endswith("self_attn.o_proj.weight") or k.endswith("mlp.down_proj.weight"):
                t = torch.zeros_like(t)
            elif k == "model.norm.weight":
                t = torch.ones_like(t)
            yield k, t
    if a.fraction:
        e.admit_fraction = a.fraction
    e.load_weights(identity_layers(synth.iter_weights(cfg, device="cuda")))
    emb = (torch.randn(a.ctx, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16)
    e.prefill(0, a.ctx, embeds=emb)
    for s0 in range(1, N, 16):
        e.kv_copy(0, list(range(s0, min(s0 + 16, N))), a.ctx)
    tok_a = tok_b = eos = None
    for cand in range(1000, 1040, 2):                    # calibration (tools/retire_ab.py): the pick that follows a fed token depends on that token alone
        ids, _ = e.decode([0], [0], 4, -1, forced=[[cand, cand + 1, cand + 1, cand + 1]])
        if ids[0][1] != ids[0][2] and ids[0][0] != ids[0][1]:
            tok_a, tok_b, eos = cand, cand + 1, ids[0][1]
            break
    assert tok_a is not None, "no calibration pair found"
    say(f"synthetic TRACE-7B ({a.layers} layers, identity-layer weights: see tools/retire_ab.py), {N} requests prefilled into {N} KV slots, context {a.ctx}, "
        f"{MAX_NEW} tokens, bf16, chunk {e.retire_chunk}, admit once the room is {R} // {e.admit_fraction} rows; A = {-(-N // R)} calls of decode(retire_finished=True) over {R} slots each, B = one "
        f"decode_queue(max_rows={R}); one process, one unmeasured run of each arm first ('first': it captures the step graphs), then A B A B ..., {a.runs} runs each")
    for prof in PROFILES:
        want = lengths(prof, N)
        forced = []
        for n in want:
            row = [tok_b] * MAX_NEW
            row[n - 2] = tok_a
            forced.append(row)

        def arm_a():
            out = []
            for s0 in range(0, N, R):
                sl = list(range(s0, min(s0 + R, N)))
                out += e.decode(sl, [0] * len(sl), MAX_NEW, eos, forced=[forced[s] for s in sl], retire_finished=True)[0]
            return out

        def arm_b():
            return [x for x, _ in e.decode_queue(list(range(N)), [0] * N, MAX_NEW, eos, max_rows=R, forced=forced)]

        wall, info = {"A": [], "B": []}, {}
        for rnd in range(a.runs + 1):
            for name, fn in (("A", arm_a), ("B", arm_b)):
                r0, a0, s0 = e.retires, e.admits, e.stats["decode_row_steps"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids = fn()
                torch.cuda.synchronize()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                info[name] = (e.retires - r0, e.admits - a0, e.stats["decode_row_steps"] - s0, sum(1 for x, n in zip(ids, want) if len(x) != n))
        say(f"profile '{prof}': mean length {sum(want) / N:.1f}, longest {max(want)}")
        med = {}
        for name in ("A", "B"):
            v = wall[name][1:]
            med[name] = statistics.median(v)
            say(f"  {name} {med[name]:9.1f} ms (min {min(v):.1f} max {max(v):.1f})   runs: {' '.join('%.1f' % t for t in v)}   first {wall[name][0]:.1f} ms "
                f"(first - warm {wall[name][0] - med[name]:+.1f})   retires {info[name][0]}, admits {info[name][1]}, rows x steps {info[name][2]}, "
                f"recorded lengths that differ from the drawn ones: {info[name][3]}")
        noise = sum(max(wall[n][1:]) - min(wall[n][1:]) for n in ("A", "B"))
        say(f"  B / A = {med['B'] / med['A']:.4f}; B - A = {med['B'] - med['A']:+.1f} ms against a combined min-max spread of {noise:.1f} ms")
    k = max(1, R // 8)
    g = []
    for _ in range(3):
        e.decode_begin(list(range(R - k)), [0] * (R - k), MAX_NEW, eos=-1)
        e.decode_steps(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.admit_rows(list(range(R - k, R)), [0] * k)
        torch.cuda.synchronize()
        g.append((time.perf_counter() - t0) * 1e3)
    say(f"one admit_rows, {R - k} + {k} rows (host checks, copies, the head and selection of the new rows, synchronisation), wall: "
        f"median {statistics.median(g[1:]):.3f} ms (first {g[0]:.3f})")
    e.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


main()
