"""What the w4 weight format costs in accuracy — reported, not asserted (tests/test_gpu_w4.py holds the w4 engine to its twin instead: the same
quantised matrix through 16-bit kernels, where the answer is exact).  (1) The relative rms of W~ - W over the four projections of layer 0 of the
synthetic TRACE-7B weights.  (2) A w4 engine against the reference's teacher-forced fp32 logits of tests/golden/deep_llm.npz (8 real-width layers) and
full_depth_llm.npz (32): max / rms logit error and the 13-way (time / score head) arg-max decisions that flip, with the lines
profiles/r06_parity_measured.txt holds for the bf16 and fp8 engines on the same fixtures quoted beside them.
Writes sections 1 and 2 of profiles/w4_parity_measured.txt and keeps its section 3 (the w4 engine against its twin), which
`python -m pytest -m gpu tests/test_gpu_w4.py` rewrites: the two commands together reproduce the file.
python tools/w4_parity.py [--fixtures deep_llm.npz:8 full_depth_llm.npz:32] [--out profiles/w4_parity_measured.txt]"""
import argparse
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trace_amd import config as tcfg, synth, w4  # noqa: E402
from trace_amd.engine import TraceEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fixtures", nargs="+", default=["deep_llm.npz:8", "full_depth_llm.npz:32"])
ap.add_argument("--schemes", nargs="+", default=["w4"], choices=["bf16", "weight_only", "w4"])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w4_parity_measured.txt"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("w4_parity.py measures on an MI355X: no HIP device visible")
lines = ["w4 decoder weights (TraceEngine(llm_w4=True)): what quantisation costs (sections 1 and 2: python tools/w4_parity.py; reported, not asserted) and how",
         "closely the w4 engine follows the same matrix on 16-bit kernels (section 3: python -m pytest -m gpu tests/test_gpu_w4.py; asserted).  MI355X.", "",
         "-- 1. the format's rounding error on the synthetic weights (Gaussian: no outliers for a block scale to exploit) --"]
MARK = "-- 3. the w4 engine against its twin"          # tests/test_gpu_w4.py writes from this line on


def say(s):
    print(s, flush=True)
    lines.append(s)


def flip_stats(lg, M):
    """tests/test_gpu_fp8.py _flip_stats: 13-way teacher-forced steps whose arg-max differs from the reference's, and the logit error"""
    ref = torch.from_numpy(M["tf_logits"])
    fin = torch.isfinite(ref)
    steps13 = [i for i in range(ref.shape[0]) if int(fin[i].sum()) <= 13]
    neg = torch.full_like(ref, -1e30)
    ra, ea = torch.where(fin, ref, neg).argmax(-1), torch.where(fin, lg, neg).argmax(-1)
    srt = torch.sort(torch.where(fin, ref, neg), dim=-1, descending=True).values
    margin = srt[:, 0] - srt[:, 1]
    clear = [i for i in steps13 if float(margin[i]) > 0.5]
    d = lg[fin] - ref[fin]
    return dict(steps=len(steps13), flips=sum(int(ra[i] != ea[i]) for i in steps13), clear=len(clear), flips_clear=sum(int(ra[i] != ea[i]) for i in clear),
                max=d.abs().max().item(), rms=d.pow(2).mean().sqrt().item())


cfg1 = dataclasses.replace(tcfg.tiny(num_frames=4), intermediate_size=14336, num_hidden_layers=1)
for name, t in synth.iter_weights(cfg1):
    if w4.is_projection(name):
        W = t.detach().to("cpu", torch.bfloat16)
        d = w4.roundtrip(W).double() - W.double()
        say(f"synthetic weights, {name.split('.', 3)[3]} {tuple(W.shape)}: rms(W~ - W) / rms(W) = {(d.pow(2).mean().sqrt() / W.double().pow(2).mean().sqrt()).item():.4f}")

say("(e4m3 with a scale per row: 0.036 per element, tests/test_gpu_fp8.py's E8)")
say("")
say("-- 2. against the reference's teacher-forced fp32 logits, beside the lines of profiles/r06_parity_measured.txt for the same depth --")
r06 = open(os.path.join(ROOT, "profiles", "r06_parity_measured.txt")).read().splitlines()
for spec in a.fixtures:
    fixture, layers = spec.split(":")
    cfg = dataclasses.replace(tcfg.tiny(num_frames=4), intermediate_size=14336, num_hidden_layers=int(layers))
    M = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    ts, ids, forced = M["timestamps"].tolist(), M["input_ids"].tolist(), M["forced_ids"].tolist()
    n = len(forced) + 1
    for scheme in a.schemes:
        eng = TraceEngine(cfg, max_batch=2, max_ctx=192, max_frames=4, max_new_tokens=64, llm_fp8="weight_only" if scheme == "weight_only" else False,
                          llm_w4=scheme == "w4")
        eng.load_weights(synth.iter_weights(cfg))
        eng.encode_video(frames, ts)
        L, emb = eng.splice(ids, want_output=True)
        eng.prefill(0, L, embeds=emb)
        lgs = [eng.decode_begin([0], [1], n, eos=-1, forced=[forced], want_logits=True).float().cpu()]
        for _ in range(n - 1):
            lgs.append(eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu())
        eng.close()
        st = flip_stats(torch.cat(lgs), M)
        say(f"{fixture}, {layers} real-width layers, {scheme}: max |dlogit| = {st['max']:.4f}, rms = {st['rms']:.4f}; 13-way steps {st['steps']}: arg-max flips vs "
            f"reference {st['flips']} ({st['flips_clear']} of the {st['clear']} with reference margin > 0.5)")
    for ln in r06:
        if ln.startswith(f"fp8 schemes, {layers} real-width layers, scheme") or (layers == "32" and ln.startswith("full depth (32 layers), bf16 anchor")):
            say("  (r06) " + ln)
say("Random Gaussian weights have no outlier structure for block scales to exploit and no trained margins to protect; a trained checkpoint is not measured here.")
say("")
if a.out:
    tail = ""
    if os.path.exists(a.out) and MARK in open(a.out).read():
        tail = MARK + open(a.out).read().split(MARK, 1)[1]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n" + tail)
