"""What scoring given continuations costs, synthetic TRACE-7B (32 layers, hidden 4096, V = 32000), prompt of 1967 rows, one process, warmed, arms
alternated round by round; medians with [min .. max]:

  head     the head stage alone over R = 256, 2048, 8192 text rows, device ms (events): the fused kernels (trace_llm_score_rows: score_head_kernel +
           score_merge_kernel, no logits stored) against the only composition there was before them — trace_llm_head_logits (the decode step's
           VALU GEMV, 32 rows per workgroup pass: it re-streams the 262 MB head matrix once per 32 rows) writing [R, 32028] fp32 logits, then
           trace_op_token_logprob over them.  Also the fused stage's achieved fraction of the bf16 MFMA peak (2 R (V + 1) hidden flop).
  call     the whole call: score of 1 and of 8 continuations of 128 and 256 tokens behind the cached prompt (TraceEngine.score_continuations: kv_copy,
           one trace_llm_score_append) against a host-mode forced decode of the same tokens (one eager decode step per token with the masked logits
           brought out, trace_op_token_logprob on them, the id fed back), wall ms around each (both end in a device synchronise), and the largest
           difference between the two arms' log-probabilities.

  python tools/score_ab.py [--rounds 5] [--only head call] [--layers 32] > profiles/score_ab.txt
"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only", nargs="+", default=["head", "call"])
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--rows", type=int, nargs="+", default=[256, 2048, 8192])
ap.add_argument("--tokens", type=int, nargs="+", default=[128, 256])
a = ap.parse_args()


import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine, _ptr, _stream  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("score_ab.py measures on an MI355X: no HIP device visible")

MFMA_PEAK = 2.5e15                  # dense bf16 flop/s of the MI355X (the rate gemm.hip's knock-out runs measure against)
cfg = tcfg.trace_7b(128)
if a.layers != cfg.num_hidden_layers:
    cfg = dataclasses.replace(cfg, num_hidden_layers=a.layers)
P, H = 1967, cfg.hidden_size
V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
NV = V + 1 + Tv + Sv
max_new = max(a.tokens)
eng = TraceEngine(cfg, max_batch=8, max_ctx=(P + max_new + 63) // 64 * 64, max_frames=128, max_new_tokens=max_new)
eng.load_weights(synth.iter_weights(cfg, device="cuda:0"))
print(f"synthetic TRACE-7B, {cfg.num_hidden_layers} layers, prompt {P} rows; {a.rounds} alternated rounds after one warm-up round; median [min .. max]")


def fmt(v):
    return f"{statistics.median(v):9.3f} [{min(v):8.3f} .. {max(v):8.3f}]"


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


g = torch.Generator(device="cuda").manual_seed(1)
if "head" in a.only:
    print(f"-- head stage alone, text rows x {V + 1} columns, device ms")
    for R in a.rows:
        if R > eng.prefill_rows:
            print(f"   R = {R}: above the prefill workspace ({eng.prefill_rows} rows), skipped")
            continue
        hid = (torch.randn(R, H, device="cuda", generator=g) * 1.0).to(torch.bfloat16)
        heads = torch.zeros(R, dtype=torch.int32, device="cuda")
        ids = torch.randint(0, V + 1, (R,), dtype=torch.int32, device="cuda", generator=g)
        out_f = torch.empty(R, dtype=torch.float32, device="cuda")
        out_c = torch.empty(R, dtype=torch.float32, device="cuda")
        logits = torch.empty((R, NV), dtype=torch.float32, device="cuda")

        def fused():
            _lib.check(eng.lib.trace_llm_score_rows(eng.h, _ptr(hid), R, _ptr(heads), _ptr(ids), _ptr(out_f), _stream()))

        def composed():
            _lib.check(eng.lib.trace_llm_head_logits(eng.h, _ptr(hid), R, 0, _ptr(logits), _stream()))
            _lib.check(eng.lib.trace_op_token_logprob(_ptr(logits), NV, R, _ptr(heads), V, Tv, Sv, _ptr(ids), _ptr(out_c), _stream()))

        tf, tc = [], []
        for rnd in range(a.rounds + 1):
            x, y = event_ms(fused), event_ms(composed)
            if rnd:
                tf.append(x)
                tc.append(y)
        diff = float((out_f - out_c).abs().max())
        mf, mc = statistics.median(tf), statistics.median(tc)
        flop = 2.0 * R * (V + 1) * H
        print(f"   R = {R:5d}: fused {fmt(tf)}   head_logits + token_logprob {fmt(tc)}   composed / fused = {mc / mf:6.2f}   "
              f"fused: {flop / (mf * 1e-3) / 1e12:7.1f} TFLOP/s = {100 * flop / (mf * 1e-3) / MFMA_PEAK:4.1f} % of the bf16 MFMA peak   "
              f"max |fused - composed| = {diff:.2e}   logits the composition stores: {R * NV * 4 / 1e6:.0f} MB")
        del logits

if "call" in a.only:
    emb = (torch.randn(P, H, device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    eng.prefill(0, P - 1, embeds=emb[: P - 1])
    rng = np.random.RandomState(4)
    print("-- the whole call behind the cached prompt, wall ms: score_continuations against a host-mode forced decode + trace_op_token_logprob")
    for ntok in a.tokens:
        for n in (1, 8):
            conts = [[int(t) for t in rng.randint(3, V, ntok)] for _ in range(n)]          # text continuations under the text head

            def score():
                return eng.score_continuations(0, P, emb[P - 1], conts, head=0)[0]

            def forced_decode():
                if n > 1:
                    eng.kv_copy(0, list(range(1, n)), P)
                eng.host_mode(True)
                try:
                    lp = np.zeros((n, ntok), np.float32)
                    lg = eng.decode_begin(list(range(n)), [0] * n, ntok, eos=-1, want_logits=True)
                    for s in range(ntok):
                        tok = [c[s] for c in conts]
                        lp[:, s] = eng.token_logprob(lg, [0] * n, tok)
                        eng.feed(tok)
                        if s + 1 < ntok:
                            lg = eng.decode_steps(1, use_graph=False, want_logits=True)
                    return lp
                finally:
                    eng.host_mode(False)

            ts, td = [], []
            for rnd in range(a.rounds + 1):
                x, rs = wall_ms(score)
                eng.prefill_append(0, P - 1, emb[P - 1:P])       # untimed: slot 0 holds the whole prompt again (the score arm rewrote its rows >= P - 1)
                y, rd = wall_ms(forced_decode)
                if rnd:
                    ts.append(x)
                    td.append(y)
            diff = max(float(np.abs(np.asarray(rs[b]) - rd[b]).max()) for b in range(n))
            ms, md = statistics.median(ts), statistics.median(td)
            print(f"   {n} x {ntok:3d} tokens: score {fmt(ts)}   forced decode {fmt(td)}   decode / score = {md / ms:6.1f}   "
                  f"{ms / (n * ntok) * 1e3:7.1f} us per scored token   max |score - decode| = {diff:.3f}")
eng.close()
