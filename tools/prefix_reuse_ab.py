"""What reusing a prompt prefix is worth, synthetic TRACE-7B at the C2 shape (32 layers, 128 frames, L = 1967: 150 rows before <video>, 1792 video
rows, 25 after), one process, warmed, arms alternated:

  questions  wall ms (host clock around generate(), which ends in a device synchronise) of the 2nd and 3rd question on one video, prefix cache
             off against on, at --new tokens each, B = 1; and three questions as ONE B = 3 call (cache on: TraceEngine.generate_questions)
             against the same B = 3 call with the cache off and against three B = 1 calls
  append     device ms (events) of trace_embed_rows + trace_llm_prefill_append of 25 rows on 1942 cached rows, beside the full 1967-row prefill
  copy       device ms of trace_kv_copy of 1942 rows to 1, 2 and 7 slots and the achieved bytes/s (one read + n writes of the rows' K and V^T
             bytes) against the 8 TB/s HBM3E spec

  batch      (--batch-shared B, a run of its own) B different videos with ONE prompt through generate(), the batch's 150 rows before <video>
             prefilled once and read from one slot by the decode attention (share_prefix_min_batch = 2) against every video on its own (off), in one
             process with interleaved rounds: wall ms per call, the prefill stage's device ms, rows prefilled, ids identical

  python tools/prefix_reuse_ab.py [--rounds 5] [--new 8 128] [--only questions append copy]
  python tools/prefix_reuse_ab.py --batch-shared 32 [--rounds 3] [--new 64]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/prefix_reuse_ab.py --only append --append-reps 20
  python tools/prefix_reuse_ab.py --summarize DIR      # kernel time of the traced run by (kernel, grid): the append's attention launches are the
                                                       # 8-workgroup ones (grid 2048), the prefix prefill's the large ones
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--new", type=int, nargs="+", default=[8, 128])
ap.add_argument("--only", nargs="+", default=["questions", "append", "copy"])
ap.add_argument("--append-reps", type=int, default=10)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--summarize", default=None)
ap.add_argument("--batch-shared", type=int, default=0, metavar="B", help="the batch arm alone: B videos, one prompt, sharing on against off")
a = ap.parse_args()


def summarize(root):
    files = sorted(glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"no *kernel_trace.csv under {root}")
    agg = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            grid = next((int(r[k]) for k in ("Grid_Size_X", "Grid_Size", "grid_size_x") if k in r and r[k]), 0)
            key = (r.get("Kernel_Name", r.get("Name", "?")), grid)
            d = agg.setdefault(key, [0, 0.0])
            d[0] += 1
            d[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    tot = sum(v[1] for v in agg.values())
    print(f"{len(files)} trace file(s), {tot / 1e3:.1f} ms of kernel time; by (kernel, grid size x in work-items):")
    for (name, grid), (calls, us) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:24]:
        print(f"{name[:90]:90s} grid {grid:9d} calls {calls:6d} avg {us / calls:9.1f} us  tot {us / 1e3:9.2f} ms {100 * us / tot:5.1f}%")


if a.summarize:
    summarize(a.summarize)
    sys.exit(0)

import dataclasses  # noqa: E402

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trace_amd import config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine  # noqa: E402
from trace_amd.model.trace_mistral import TraceMistralForCausalLM  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("prefix_reuse_ab.py measures on an MI355X: no HIP device visible")

cfg = tcfg.trace_7b(128)
if a.layers != cfg.num_hidden_layers:
    cfg = dataclasses.replace(cfg, num_hidden_layers=a.layers)


def batch_shared(B):
    L, n_new = 1967, a.new[0]
    eng = TraceEngine(cfg, max_batch=B, max_ctx=(L + n_new + 63) // 64 * 64, max_frames=128, max_new_tokens=n_new)
    eng.load_weights(synth.iter_weights(cfg, device="cuda:0"))
    vids = [synth.synth_frames(cfg, b, num_frames=128, device="cuda").to(torch.bfloat16) for b in range(B)]
    ts = [[[i * 2.0] for i in range(128)]] * B
    ids = [synth.synth_prompt_ids(cfg, n_text=176, video_pos=150).tolist()] * B
    res = {arm: {"wall": [], "prefill": [], "rows": []} for arm in ("off", "on")}
    first = None
    for rnd in range(a.rounds + 1):                          # round 0 warms both arms (graphs of both (slot, rows) pairs) and is dropped
        for arm in ("off", "on"):
            eng.share_prefix_min_batch = 2 if arm == "on" else B + 1
            eng.stage_timing(True)
            rows0 = eng.stats["prefill_rows"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.generate(vids, ts, ids, [1] * B, n_new)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            st = eng.stage_times()
            eng.stage_timing(False)
            first = first or out
            assert out == first, "ids / heads differ between the arms or rounds"
            if rnd:
                res[arm]["wall"].append(wall); res[arm]["prefill"].append(st["prefill_ms"]); res[arm]["rows"].append(eng.stats["prefill_rows"] - rows0)
    print(f"synthetic TRACE-7B, {cfg.num_hidden_layers} layers, {B} videos x 128 frames, one prompt (150 rows before <video>, L = {L}), {n_new} new tokens; "
          f"{a.rounds} interleaved rounds after a warm-up round; median [min .. max]; ids and heads identical in both arms and every round: True")
    for arm, r in res.items():
        print(f"   sharing {arm:3s}: generate() wall ms {fmt(r['wall'])}   prefill stage device ms {fmt(r['prefill'])}   rows prefilled {r['rows'][0]}")
    m = lambda k: statistics.median(res["on"][k]) / statistics.median(res["off"][k])
    print(f"   on / off: wall {m('wall'):.4f}   prefill stage {m('prefill'):.4f}")
    eng.close()


def fmt(v):
    return f"{statistics.median(v):9.2f} [{min(v):8.2f} .. {max(v):8.2f}]"


if a.batch_shared:
    batch_shared(a.batch_shared)
    sys.exit(0)

L, P = 1967, 1942
max_new = max(a.new)
eng = TraceEngine(cfg, max_batch=8, max_ctx=(L + max_new + 63) // 64 * 64, max_frames=128, max_new_tokens=max_new)
eng.load_weights(synth.iter_weights(cfg, device="cuda:0"))
model = TraceMistralForCausalLM(cfg, eng)
frames = synth.synth_frames(cfg, 0, num_frames=128, device="cuda").to(torch.bfloat16)
ts = [[i * 2.0] for i in range(128)]
base = synth.synth_prompt_ids(cfg, n_text=176, video_pos=150)
cut = base.tolist().index(-201) + 1
prompts = []
for q in range(3):
    p = base.clone()
    p[cut:-1] = (p[cut:-1] + 101 * q) % (cfg.vocab_size - 3) + 3
    prompts.append(p)
assert cut + 1792 - 1 == P and len(base) - cut == L - P
print(f"synthetic TRACE-7B, {cfg.num_hidden_layers} layers, 128 frames, L = {L} = {P} rows through <video> + {L - P}; {a.rounds} alternated rounds; "
      f"median [min .. max]")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def gen(ps, n_new):
    B = len(ps)
    return model.generate(torch.stack(ps), images_or_videos=[frames] * B, modal_list=["video"] * B, video_timestamps=[ts] * B, heads=[1] * B,
                          max_new_tokens=n_new, eos_token_id=-1).tolist()


def events(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


if "questions" in a.only:
    for n_new in a.new:
        res = {k: [] for k in ("off q1", "off q2+q3", "on q1 (miss)", "on q2+q3", "off 3 x B=1", "off B=3", "on B=3")}
        ids = {}
        for rnd in range(a.rounds + 1):                      # round 0 warms every shape (graphs, code objects) and is dropped
            for arm in ("off", "on"):
                model.enable_prefix_cache(arm == "on")       # (also drops the entry: q1 of every round is a miss)
                t1, o1 = timed(lambda: gen([prompts[0]], n_new))
                t2, o2 = timed(lambda: gen([prompts[1]], n_new))
                t3, o3 = timed(lambda: gen([prompts[2]], n_new))
                model.enable_prefix_cache(arm == "on")
                tb, ob = timed(lambda: gen(prompts, n_new))
                got = (o1, o2, o3, ob)
                assert ids.setdefault("all", got) == got, "ids differ between the arms / rounds"
                if rnd == 0:
                    continue
                res["off q1" if arm == "off" else "on q1 (miss)"].append(t1)
                res[arm + " q2+q3"].append((t2 + t3) / 2)
                res[arm + " B=3"].append(tb)
                if arm == "off":
                    res["off 3 x B=1"].append(t1 + t2 + t3)
        model.enable_prefix_cache(False)
        print(f"-- {n_new} new tokens per question, wall ms per generate() call (ids identical in both arms and every round: True)")
        for k, v in res.items():
            print(f"   {k:14s} {fmt(v)}")
        m = {k: statistics.median(v) for k, v in res.items()}
        print(f"   2nd / 3rd question: on / off = {m['on q2+q3'] / m['off q2+q3']:.3f}   first question (two-pass prefill): on / off = "
              f"{m['on q1 (miss)'] / m['off q1']:.3f}   three questions: B=3 on / B=3 off = {m['on B=3'] / m['off B=3']:.3f}, "
              f"B=3 on / 3 x B=1 off = {m['on B=3'] / m['off 3 x B=1']:.3f}")

emb = (torch.randn(L, cfg.hidden_size, device="cuda") * 0.02).to(torch.bfloat16)

if "append" in a.only:
    suffix_ids = prompts[1][cut:].tolist()
    eng.prefill(0, P, embeds=emb[:P])

    def append():
        eng.embed_rows(suffix_ids)
        eng.prefill_append(0, P, None, L=L - P)
    events(append, 3)
    t_app = events(append, a.append_reps)
    print(f"-- append alone: embed_rows + prefill_append of {L - P} rows on {P} cached rows, device ms: {fmt(t_app)}")
    if a.only != ["append"]:                                  # (a traced run keeps to the append: one kernel name, two grid sizes)
        t_full = events(lambda: eng.prefill(0, L, embeds=emb), max(3, a.append_reps // 2))
        t_pre = events(lambda: eng.prefill(0, P, embeds=emb[:P]), max(3, a.append_reps // 2))
        print(f"   full prefill of {L} rows: {fmt(t_full)}   prefix prefill of {P} rows: {fmt(t_pre)}")

if "copy" in a.only:
    eng.prefill(0, P, embeds=emb[:P])
    per_slot = cfg.num_hidden_layers * cfg.num_key_value_heads * (P * 128 + 128 * ((P + 7) // 8 * 8)) * 2
    print(f"-- trace_kv_copy of {P} rows ({per_slot / 1e6:.1f} MB of K + V^T per slot), device ms and achieved bytes/s (one read + n writes) of 8 TB/s:")
    for n in (1, 2, 7):
        dsts = list(range(1, 1 + n))
        events(lambda: eng.kv_copy(0, dsts, P), 3)
        t = events(lambda: eng.kv_copy(0, dsts, P), max(10, a.append_reps))
        med = statistics.median(t)
        bw = (1 + n) * per_slot / (med * 1e-3)
        print(f"   to {n} slot(s): {fmt(t)}   {bw / 1e12:.2f} TB/s = {100 * bw / 8e12:.0f} % of spec")
eng.close()
