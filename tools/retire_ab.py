"""decode(..., retire_finished=True) against the default on a batch whose rows end at different lengths: synthetic TRACE-7B, context --ctx, batch --batch,
256 tokens, a FRESH CHILD PROCESS per configuration (off, on) and round, the rounds interleaved (off, on, off, ...).  Forced ids end the rows at lengths
drawn once from a fixed seed, in two profiles:
  tail   short answers with a long tail: round(exp(N(ln 40, 0.8))) clipped to [8, 255] - a moment-retrieval batch with a few dense captions in it;
  last   every row ends inside the last chunk of 32 steps (226 .. 256 ids): nothing can be retired, the worst case for the flag.
A forced id is fed, not recorded, so a forced EOS ends nothing by itself: the child loads the synthetic weights with o_proj / down_proj zeroed and a
unit final norm (every kernel of every layer runs on the same shapes and bytes; the residual stream stays the embedding of the fed token), finds by a
three-step calibration run a token `a` whose successor pick is taken as EOS and a filler `b` whose pick is another id, and feeds `a` where a row is
to end.  The child checks that the recorded lengths are the drawn ones.
Per profile a child reports the wall ms of the first decode() call (with the flag on it captures one step graph per batch size it meets) and of the
second (warm: what a process that has seen these sizes pays), the retires, rows x steps, and the wall ms of one trace_decode_retire of 128 -> 112 rows
(host check, copy of the keep list, the two gather launches, stream synchronisation).  The parent prints the warm median over the rounds after the first
with min / max, the on / off ratio against the run-to-run spread, and the capture cost per new batch size.
python tools/retire_ab.py [--batch 128] [--ctx 1968] [--rounds 3] [--out profiles/retire_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = ("off", "on")
PROFILES = ("tail", "last")
MAX_NEW = 256

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--ctx", type=int, default=1968)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--seed", type=int, default=20261019)
ap.add_argument("--out", default=None)
ap.add_argument("--child", choices=CONFIGS, default=None)
a = ap.parse_args()


def lengths(profile, B):
    import numpy as np
    rng = np.random.default_rng(a.seed + PROFILES.index(profile))
    if profile == "tail":
        return np.clip(np.rint(np.exp(rng.normal(np.log(40.0), 0.8, B))), 8, MAX_NEW - 1).astype(int).tolist()
    return rng.integers(MAX_NEW - 30, MAX_NEW + 1, B).tolist()


def child(name):
    import torch
    from trace_amd import config as tcfg, synth
    from trace_amd.engine import TraceEngine
    cfg = tcfg.trace_7b()
    cfg.num_hidden_layers = a.layers
    B = a.batch
    torch.manual_seed(0)
    e = TraceEngine(cfg, max_batch=B, max_ctx=a.ctx + MAX_NEW + 32, max_frames=128, max_new_tokens=MAX_NEW)

    def identity_layers(items):
        for k, t in items:
            if k.endswith("self_attn.o_proj.weight") or k.endswith("mlp.down_proj.weight"):
                t = torch.zeros_like(t)
            elif k == "model.norm.weight":
                t = torch.ones_like(t)
            yield k, t
    e.load_weights(identity_layers(synth.iter_weights(cfg, device="cuda")))
    emb = (torch.randn(a.ctx, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16)
    e.prefill(0, a.ctx, embeds=emb)
    if B > 1:
        e.kv_copy(0, list(range(1, B)), a.ctx)
    # calibration: the pick that follows a fed token depends on that token alone
    tok_a, tok_b, eos = None, None, None
    for cand in range(1000, 1040, 2):
        ids, _ = e.decode([0], [0], 4, -1, forced=[[cand, cand + 1, cand + 1, cand + 1]])
        if ids[0][1] != ids[0][2] and ids[0][0] != ids[0][1]:
            tok_a, tok_b, eos = cand, cand + 1, ids[0][1]
            break
    assert tok_a is not None, "no calibration pair found"
    out = {"config": name, "eos": eos}
    flag = name == "on"
    for prof in PROFILES:
        want = lengths(prof, B)
        forced = []
        for n in want:
            row = [tok_b] * MAX_NEW
            row[n - 2] = tok_a                     # fed after step n - 2: the state of step n - 1, whose pick (the n-th id) is EOS
            forced.append(row)
        wall, rs = [], []
        for _ in range(2):
            r0, s0 = e.retires, e.stats["decode_row_steps"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids, _ = e.decode(list(range(B)), [0] * B, MAX_NEW, eos, forced=forced, retire_finished=flag)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            rs.append((e.retires - r0, e.stats["decode_row_steps"] - s0, [len(h) for h in e._rows_history]))
        bad = sum(1 for x, n in zip(ids, want) if len(x) != n)
        out[prof] = {"first": wall[0], "warm": wall[1], "retires": rs[1][0], "row_steps": rs[1][1], "sizes": rs[1][2], "length_mismatches": bad,
                     "mean_len": sum(want) / B, "max_len": max(want)}
    g = []
    keep = [i for i in range(B) if i % 8 != 7] if B >= 8 else list(range(B - 1))
    for _ in range(2):
        e.decode_begin(list(range(B)), [0] * B, MAX_NEW, eos=-1)
        e.decode_steps(2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.retire_rows(keep)
        g.append((time.perf_counter() - t0) * 1e3)
    out["gather_ms"], out["gather_rows"] = g[1], [B, len(keep)]
    e.close()
    print("RETAB " + json.dumps(out), flush=True)


def parent():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"synthetic TRACE-7B ({a.layers} layers, identity-layer weights: see tools/retire_ab.py), batch {a.batch}, context {a.ctx}, {MAX_NEW} tokens, bf16; "
        f"decode(retire_finished=False / True), chunk 32; a fresh process per configuration and round, {a.rounds} interleaved rounds; 'warm' = the second "
        f"call of a process, median of rounds 2.. (min / max of those); 'first' = the first call of a process (with the flag on it captures a step graph "
        f"per batch size)")
    res = {c: [] for c in CONFIGS}
    for rnd in range(a.rounds):
        for c in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", c, "--ctx", str(a.ctx), "--batch", str(a.batch), "--layers", str(a.layers),
                   "--seed", str(a.seed)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            got = [ln[6:] for ln in r.stdout.splitlines() if ln.startswith("RETAB ")]
            if r.returncode != 0 or not got:
                sys.exit(f"child {c} round {rnd} failed (rc {r.returncode}):\n{r.stderr[-2000:]}")
            res[c].append(json.loads(got[0]))
            print(f"  round {rnd} {c}: {got[0]}", flush=True)
    for prof in PROFILES:
        p0 = res["on"][0][prof]
        say(f"profile '{prof}': mean length {p0['mean_len']:.1f}, longest {p0['max_len']}; recorded lengths that differ from the drawn ones: "
            f"{sum(x[prof]['length_mismatches'] for c in CONFIGS for x in res[c])}")
        med, spread = {}, {}
        for c in CONFIGS:
            v = [x[prof]["warm"] for x in res[c]]
            use = v[1:] if len(v) > 1 else v
            med[c], spread[c] = statistics.median(use), max(use) - min(use)
            x = res[c][-1][prof]
            say(f"  {c:3s} warm call {med[c]:9.1f} ms (min {min(use):.1f} max {max(use):.1f})   rounds: {' '.join('%.1f' % t for t in v)}   "
                f"rows x steps {x['row_steps']}, retires {x['retires']}, batch sizes {x['sizes']}")
        noise = spread["off"] + spread["on"]
        say(f"  on / off = {med['on'] / med['off']:.4f}; on - off = {med['on'] - med['off']:+.1f} ms against a combined min-max spread of {noise:.1f} ms")
        if prof == "last":
            say("  -> " + ("the flag costs no more than the run-to-run spread where nothing can be retired" if med["on"] - med["off"] <= noise
                           else "the flag is SLOWER than off by more than the spread where nothing can be retired"))
        first = [x[prof]["first"] - x[prof]["warm"] for x in res["on"]]
        first_off = [x[prof]["first"] - x[prof]["warm"] for x in res["off"]]
        new = len(set(p0["sizes"][1:]))
        say(f"  first call - warm call: on {statistics.median(first):+.1f} ms, off {statistics.median(first_off):+.1f} ms; " +
            (f"{new} batch sizes beyond the first -> {(statistics.median(first) - statistics.median(first_off)) / new:.1f} ms of capture per new batch size"
             if new else "no batch size beyond the first"))
    gms = [x["gather_ms"] for c in CONFIGS for x in res[c]]
    say(f"one trace_decode_retire, {res['on'][0]['gather_rows'][0]} -> {res['on'][0]['gather_rows'][1]} rows (host checks, keep list copy, two gather launches, "
        f"synchronisation), wall: median {statistics.median(gms):.3f} ms (min {min(gms):.3f} max {max(gms):.3f})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if a.child:
    child(a.child)
else:
    import torch
    if not torch.cuda.is_available():
        sys.exit("retire_ab.py measures on an MI355X: no HIP device visible")
    parent()
