"""The prefill's cache-write kernels on the device, each alone (tests/prefill_glue_probes.py; tests/test_prefill_glue_probes_cpu.py shows on the CPU which
faults these probes reject and which of them a prefill-against-prefill comparison cannot see): rope_kv_kernel through trace_op_rope_kv in every launch
form (pos0 = 0, pos0 = past, seq_len with three sequences, slot_arr / pos_arr, a row-major V cache, a padded ld, 4/1 and 32/8 heads, R = 1 .. 2760 — the
last past the launcher's grid cap), transpose_v_kernel<64|128> through trace_op_transpose_v at every p0 x n of the probe module with and without perm,
gather_rows_kernel through trace_op_gather_rows over six tables up to the 4096 x 256-chunk grid cap.  Both libraries.

Exact probes are bit equal; the Gaussian RoPE probe is judged by half a 16-bit ulp + E (prefill_glue_probes.rope_judge) and its error / bound goes to
the file the environment variable TRACE_PREFILL_GLUE_PROBE_MARGINS names (profiles/prefill_glue_probe_margins.txt is made from it).  The hooks' refusals
are checked: an error return, never a launch.  Three "the engine is the op" tests then pin the call sites: layer 0's K and V^T after prefill,
prefill_multi, prefill_append and the one-layer last-rows shortcut equal the hooks applied to op_gemm(op_rmsnorm(embeds)) with the restated RoPE table,
bit for bit, over EVERY word of the layer's caches; splice / embed_rows equal trace_op_gather_rows on the same index lists."""
import ctypes as C
import dataclasses
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import encode_probes as EP  # noqa: E402
import prefill_glue_probes as PG  # noqa: E402
from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
MARGINS = {}                      # (library, kernel, probe) -> [max err / bound, cases]


@pytest.fixture(scope="module", autouse=True)
def margins_record():
    yield
    lines = [f"{lib:<5} {k:<12} {p:<24} max err/bound {m[0]:.6f}  cases {m[1]}" for (lib, k, p), m in sorted(MARGINS.items())]
    print("\n".join(lines))
    path = os.environ.get("TRACE_PREFILL_GLUE_PROBE_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(params=["bf16", "f16"])
def el(request):
    ops.use(request.param)
    yield request.param
    ops.use("bf16")


def record(el, kernel, probe, ratio):
    m = MARGINS.setdefault((el, kernel, probe), [0.0, 0])
    m[0], m[1] = max(m[0], ratio), m[1] + 1


# ---- rope_kv --------------------------------------------------------------------------------------------------------------------------------------------
def device_rope(pr, **over):
    qkv, kc = pr.qkv.clone(), pr.kcache.clone()
    vc = None if pr.vcache is None else pr.vcache.clone()
    kw = dict(slot0=pr.slot0, pos0=pr.pos0, seq_len=pr.seq_len, slot_arr=pr.slot_arr, pos_arr=pr.pos_arr, vcache=vc)
    kw.update(over)
    ops.rope_kv(qkv, pr.ld, kc, pr.slot_stride, pr.kv_head_stride, pr.R, pr.nq, pr.nkv, pr.hd, pr.cos_t, pr.sin_t, **kw)
    return qkv, kc, vc


@pytest.mark.parametrize("case", list(PG.ROPE_CASES))
def test_rope_exact(el, case):
    dtype = DTYPES[el]
    for name in PG.ROPE_EXACT:
        if case == "grid-stride" and name != "per-position":          # one 34 MB launch: the probe whose table row names the position
            continue
        pr = PG.rope_probe(name, case, dtype, DEV)
        ratio, intact = PG.rope_judge(pr, device_rope(pr))
        print(f"{el} rope {name} @ {case}: bit equal {ratio == 0.0}, outside intact {intact}")
        assert ratio == 0.0, f"rope_kv {name} @ {case}: rotated q / cached k differ from the float64 reference rounded once"
        assert intact, f"rope_kv {name} @ {case}: a word outside the q heads and the cache rows changed (or the V rows are not the copy)"
    if case == "grid-stride":                                          # the last rows are the grid-stride loop's: name them
        slot, pos = PG.rope_rows(pr)
        assert int(slot[-1]) == pr.slot0 + 2 and int(pos[-1]) == pr.pos0 + 919 and pr.R * (pr.nq + 2 * pr.nkv) * 8 > PG.GRID_THREADS


def test_rope_gaussian(el):
    dtype = DTYPES[el]
    tables = EP.rope_tables(4096, 128, tcfg.tiny().rope_theta, DEV)
    for c in PG.GAUSSIAN_CASES:
        pr = PG.gaussian_rope_probe(c, dtype, tables, DEV)
        ratio, intact = PG.rope_judge(pr, device_rope(pr))
        print(f"{el} rope gaussian @ {c['label']}: error / bound {ratio:.6f}, outside intact {intact}")
        record(el, "rope_kv", f"gaussian {c['label']}", ratio)
        assert ratio <= 1.0, f"rope_kv gaussian @ {c['label']}: error / bound {ratio}"
        assert intact, f"rope_kv gaussian @ {c['label']}: a word outside the q heads and the cache rows changed"


def test_rope_refusals(el):
    dtype = DTYPES[el]
    pr = PG.rope_probe("identity", "multi-3xL7", dtype, DEV)           # 3 sequences of 7 at pos0 = 5 into slots 1..3 of 5, 16 positions a head
    device_rope(pr)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    bad = [dict(pos0=10), dict(pos0=-1), dict(slot0=3), dict(slot0=-1), dict(seq_len=-1),
           dict(slot_arr=i32([0] * 21), pos_arr=i32([0] * 21)),                         # two rows to one cache row
           dict(slot_arr=i32(list(range(21))), pos_arr=i32([0] * 21)),                  # slots past the cache
           dict(seq_len=0, slot_arr=i32([0] * 21), pos_arr=i32(list(range(15)) + [16] * 6)),   # positions past the table
           dict(seq_len=0, slot_arr=i32([0] * 21), pos_arr=i32([-1] + list(range(1, 16)) + [0] * 5)),
           dict(seq_len=0, slot_arr=i32([-1] + [0] * 20), pos_arr=i32(list(range(16)) + [0] * 5)),
           dict(slot_arr=i32([0] * 20))]                                                  # fewer entries than rows
    for kw in bad:
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_rope_kv"):
            device_rope(pr, **kw)

    def raw(qkv=pr.qkv, ld=pr.ld, kc=pr.kcache, R=pr.R, hd=pr.hd, cos_t=pr.cos_t, table_rows=None, ss=pr.slot_stride, khs=pr.kv_head_stride, vcache=None):
        ops.rope_kv(qkv.clone(), ld, kc.clone(), ss, khs, R, pr.nq, pr.nkv, hd, cos_t, pr.sin_t, slot0=1, pos0=5, seq_len=7, table_rows=table_rows, vcache=vcache)
    raw()
    for kw in (dict(ld=pr.ld + 4), dict(ld=pr.ld - 8), dict(hd=24), dict(hd=0), dict(R=0), dict(R=22), dict(qkv=pr.qkv[:-8]), dict(table_rows=11),
               dict(kc=pr.kcache[:3 * pr.slot_stride + 8]), dict(ss=pr.slot_stride + 4), dict(khs=8 * 128),
               dict(qkv=pr.qkv[4:]), dict(vcache=pr.kcache[:3 * pr.slot_stride].clone())):
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_rope_kv"):
            raw(**kw)
    lib = _lib.load(el)
    with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_rope_kv: null argument"):
        lib.trace_op_rope_kv(None, 0, 64, None, 0, None, 0, 0, 0, None, None, 0, 0, 0, 1, 1, 1, 16, None, None, 1, 0, None)


# ---- transpose_v ----------------------------------------------------------------------------------------------------------------------------------------
def device_transpose(pr, **over):
    dst = pr.dst.clone()
    kw = dict(src_bs=pr.src_bs, src_hs=pr.src_hs, src_rs=pr.src_rs, dst_bs=pr.dst_bs, dst_hs=pr.dst_hs, dst_rs=pr.dst_rs, n=pr.n, hd=pr.hd, heads=pr.heads,
              batch=pr.batch, perm=pr.perm, p0=pr.p0, src=pr.src, dst=dst)
    kw.update(over)
    ops.transpose_v(kw.pop("src"), kw.pop("src_bs"), kw.pop("src_hs"), kw.pop("src_rs"), kw.pop("dst"), kw.pop("dst_bs"), kw.pop("dst_hs"), kw.pop("dst_rs"),
                    kw.pop("n"), kw.pop("hd"), kw.pop("heads"), kw.pop("batch"), **kw)
    return dst


@pytest.mark.parametrize("hd", [64, 128])
def test_transpose(el, hd):
    dtype = DTYPES[el]
    wrong = []
    for label, kw in PG.transpose_cases(hd):
        pr = PG.transpose_probe(dtype=dtype, device=DEV, **kw)
        got = device_transpose(pr)
        if not PG.transpose_judge(pr, got):
            wrong.append((label, PG.transpose_region_report(pr, got)))
    print(f"{el} transpose_v<{hd}>: {len(PG.transpose_cases(hd))} cases, wrong {wrong}")
    assert not wrong, f"transpose_v<{hd}>: cases whose destination differs from the contract, with the part of it they break: {wrong}"


def test_transpose_refusals(el):
    dtype = DTYPES[el]
    pr = PG.transpose_probe(128, 9, 55, dtype, device=DEV)             # dst_rs = 128
    device_transpose(pr)
    for kw in (dict(p0=74), dict(n=120), dict(perm=1), dict(perm=2), dict(perm=-1), dict(hd=32), dict(hd=96), dict(hd=256), dict(dst_rs=96), dict(dst_rs=0),
               dict(n=0), dict(p0=-1), dict(heads=0), dict(batch=0), dict(batch=3), dict(heads=3), dict(src_rs=120), dict(src_rs=pr.src_rs + 4),
               dict(src_hs=pr.src_hs + 4), dict(dst_hs=pr.dst_hs + 4), dict(dst_bs=pr.dst_bs + 4), dict(dst_bs=pr.dst_bs + 120),
               dict(src=pr.src[:pr.src_bs + pr.src_hs + 54 * pr.src_rs + 120]), dict(dst=pr.dst[:-120].clone()), dict(src=pr.src[4:]), dict(src_bs=-8)):
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_transpose_v"):
            device_transpose(pr, **kw)
    tight = PG.transpose_probe(128, 64, 64, dtype, tight=True, device=DEV)
    assert tight.p0 + tight.n == tight.dst_rs
    device_transpose(tight)
    with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_transpose_v"):
        device_transpose(tight, n=65)


# ---- gather_rows ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,H,L", PG.GATHER_CASES, ids=[c[0] for c in PG.GATHER_CASES])
def test_gather(el, label, H, L):
    pr = PG.gather_probe(H, L, DTYPES[el], DEV)
    out = pr.out.clone()
    ops.gather_rows(pr.tabs, pr.kind, pr.row, out, L, H)
    ref = PG.gather_reference(pr)
    got = PG.bits(out)
    rows_ok = bool((got.view(-1, H)[:L] == ref.view(-1, H)[:L]).all())
    tail_ok = bool((got.view(-1, H)[L:] == PG.SENTINEL).all())
    print(f"{el} gather_rows {label}: rows equal {rows_ok}, sentinel past row L {tail_ok}")
    assert rows_ok, f"gather_rows {label}: first wrong row {int(torch.nonzero((got.view(-1, H)[:L] != ref.view(-1, H)[:L]).any(1))[0])}"
    assert tail_ok, f"gather_rows {label}: a store past row L"


def test_gather_refusals(el):
    dtype = DTYPES[el]
    pr = PG.gather_probe(256, 24, dtype, DEV)

    def call(kind=pr.kind, row=pr.row, L=24, H=256, out=None, tabs=pr.tabs, tab_rows=None):
        ops.gather_rows(tabs, kind, row, pr.out.clone() if out is None else out, L, H, tab_rows=tab_rows)

    def at(t, i, v):
        t = t.clone()
        t[i] = v
        return t
    call()
    first = lambda k: int(torch.nonzero(pr.kind == k)[0])
    for kw in (dict(kind=at(pr.kind, 23, 6)), dict(kind=at(pr.kind, 0, -1)), dict(row=at(pr.row, first(2), 7)), dict(row=at(pr.row, first(4), 1)),
               dict(row=at(pr.row, 5, -1)), dict(tabs=[None if k == 3 else t for k, t in enumerate(pr.tabs)]), dict(tab_rows=[5, 3, 6, 2, 1, 4]),
               dict(H=252), dict(H=0), dict(L=0), dict(L=25), dict(kind=pr.kind[:23]), dict(row=pr.row[:23]), dict(out=pr.out[:24 * 256 - 8].clone()),
               dict(out=pr.out[4:])):
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_gather_rows"):
            call(**kw)
    call(tabs=[None if k == 3 else t for k, t in enumerate(pr.tabs)], kind=torch.where(pr.kind == 3, 0, pr.kind).to(torch.int32),
         row=torch.where(pr.kind == 3, 0, pr.row).to(torch.int32))    # an unused table may be NULL


# ---- the engine is the op ---------------------------------------------------------------------------------------------------------------------------------
class _Dev:                       # a [n] int16 view of device memory for torch
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i2", "data": (ptr, False), "version": 3}


NSLOTS, MAX_CTX = 4, 256
_sd = {}


def state(cfg):
    if "sd" not in _sd:
        _sd["sd"] = synth.state_dict(tcfg.tiny(num_frames=4))
    return {k: v for k, v in _sd["sd"].items() if not k.startswith("model.layers.") or int(k.split(".")[2]) < cfg.num_hidden_layers}


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(el, layers):
        if (el, layers) not in made:
            cfg = dataclasses.replace(tcfg.tiny(num_frames=4), num_hidden_layers=layers)
            eng = TraceEngine(cfg, max_batch=NSLOTS, max_ctx=MAX_CTX, max_frames=4, max_new_tokens=8, dtype=DTYPES[el])
            sd = state(cfg)
            eng.load_weights(sd.items())
            kc, vc, xl = C.c_void_p(), C.c_void_p(), C.c_void_p()
            st = (C.c_int64 * 8)()
            _lib.check(eng.lib.trace_debug_buffers(eng.h, C.byref(kc), C.byref(vc), C.byref(xl), st))
            layer_stride, slot_stride, head_stride, ctx_pad, NL, NKV, HD, H = [int(x) for x in st]
            assert NL == layers and layer_stride == NSLOTS * slot_stride
            K0 = torch.as_tensor(_Dev(kc.value, layer_stride), device="cuda").view(DTYPES[el])          # layer 0, every slot
            VT0 = torch.as_tensor(_Dev(vc.value, layer_stride), device="cuda").view(DTYPES[el])
            g = lambda n: sd[n].to(DTYPES[el]).to(DEV).contiguous()
            p = "model.layers.0."
            W = torch.cat([g(p + "self_attn.q_proj.weight"), g(p + "self_attn.k_proj.weight"), g(p + "self_attn.v_proj.weight")]).contiguous()
            tabs = EP.rope_tables(MAX_CTX, HD, cfg.rope_theta, DEV)
            made[(el, layers)] = dict(cfg=cfg, eng=eng, K0=K0, VT0=VT0, W=W, rms1=g(p + "input_layernorm.weight"), tabs=tabs, slot_stride=slot_stride,
                                      head_stride=head_stride, ctx_pad=ctx_pad, NKV=NKV, HD=HD, H=H, sd=sd, g=g)
        return made[(el, layers)]
    yield get
    for v in made.values():
        v["eng"].close()


def rows_of(L, H, seed, dtype):
    return (0.05 * torch.randn((L, H), generator=torch.Generator().manual_seed(seed))).to(dtype).to(DEV)


def restated_layer0(e, embeds, slot0, past, shortcut):
    """layer 0's caches as the hooks leave them, starting from what the engine's caches hold now: the engine's own route (rmsnorm over all rows, the qkv
    GEMM at lda = ldw = H, ldc = QKV — under the last-rows shortcut its k | v columns only), trace_op_rope_kv at seq_len = L into slots slot0 ..,
    trace_op_transpose_v at p0 = past"""
    cfg, HD, NKV = e["cfg"], e["HD"], e["NKV"]
    NQ = cfg.num_attention_heads
    QKV = (NQ + 2 * NKV) * HD
    nb, L = len(embeds), embeds[0].shape[0]
    x = torch.cat(embeds).contiguous()
    h = ops.rmsnorm(x, e["rms1"], cfg.rms_norm_eps)
    if shortcut:
        qkv = torch.zeros((nb * L, QKV), dtype=x.dtype, device=DEV)
        ops.gemm(h, e["W"][NQ * HD:], out=qkv[:, NQ * HD:])
    else:
        qkv = ops.gemm(h, e["W"])
    assert qkv.stride(0) == QKV
    kc, vt = e["K0"].clone(), e["VT0"].clone()
    flat = qkv.view(-1)
    ops.rope_kv(flat, QKV, kc, e["slot_stride"], e["head_stride"], nb * L, NQ, NKV, HD, e["tabs"][0], e["tabs"][1], slot0=slot0, pos0=past, seq_len=L)
    ops.transpose_v(flat[(NQ + NKV) * HD:], L * QKV, HD, QKV, vt[slot0 * e["slot_stride"]:], e["slot_stride"], e["head_stride"], e["ctx_pad"], L, HD, NKV, nb,
                    perm=0, p0=past)
    return kc, vt


def same_bits(got, want, what):
    a, b = PG.bits(got), PG.bits(want)
    if not torch.equal(a, b):
        ne = torch.nonzero(a != b).reshape(-1)
        raise AssertionError(f"{what}: {ne.numel()} of {a.numel()} words differ, first at element {int(ne[0])}, last at {int(ne[-1])}")


def check_call(e, call, embeds, slot0, past, shortcut, what):
    want_k, want_vt = restated_layer0(e, embeds, slot0, past, shortcut)            # from the caches as they are BEFORE the call
    assert not torch.equal(PG.bits(want_k), PG.bits(e["K0"])) and not torch.equal(PG.bits(want_vt), PG.bits(e["VT0"])), what + ": the call under test writes nothing new"
    call()
    torch.cuda.synchronize()
    same_bits(e["K0"], want_k, what + ": layer 0 K cache")
    same_bits(e["VT0"], want_vt, what + ": layer 0 V^T cache")


def stale(e, L=200):
    """every slot holds L rows of something else first: the rows past a new end are stale data, not zeros"""
    H, dtype = e["H"], e["eng"].dtype
    for s in range(0, NSLOTS, 2):
        e["eng"].prefill_multi(s, [rows_of(L, H, 100 + s, dtype), rows_of(L, H, 101 + s, dtype)])


def test_engine_prefill_is_the_ops(el, engines):
    e = engines(el, 2)
    eng, H, dtype = e["eng"], e["H"], DTYPES[el]
    stale(e)
    for L in (79, 1, 64):
        emb = rows_of(L, H, L, dtype)
        check_call(e, lambda: eng.prefill(1, L, embeds=emb), [emb], 1, 0, False, f"{el} prefill of {L} rows into slot 1")
    assert float(e["K0"].float().abs().max()) > 0.01, "the cache holds keys, not zeros"


def test_engine_multi_and_append_are_the_ops(el, engines):
    e = engines(el, 2)
    eng, H, dtype = e["eng"], e["H"], DTYPES[el]
    stale(e)
    three = [rows_of(37, H, 7 + i, dtype) for i in range(3)]
    check_call(e, lambda: eng.prefill_multi(1, three), three, 1, 0, False, f"{el} prefill_multi of 3 x 37 rows into slots 1..3")
    for past in (5, 66):
        stale(e)                                                               # something longer first: stale rows past the new end
        pre = [rows_of(past, H, 20 + i, dtype) for i in range(3)]
        eng.prefill_multi(0, pre)
        new = [rows_of(13, H, 30 + i, dtype) for i in range(3)]
        check_call(e, lambda: eng.prefill_append(0, past, new), new, 0, past, False, f"{el} prefill_append of 3 x 13 rows at past = {past}")
        one = rows_of(9, H, 40, dtype)
        check_call(e, lambda: eng.prefill_append(2, past, one), [one], 2, past, False, f"{el} prefill_append of 9 rows at past = {past} into slot 2")


def test_engine_last_layer_shortcut_is_the_ops(el, engines):
    """one decoder layer: layer 0 is the last layer and prefill (no hidden rows asked for) takes the prefill_last_rows shortcut — rope_kv over rows whose q
    columns are stale, the k | v columns from a GEMM of their own"""
    e = engines(el, 1)
    eng, H, dtype = e["eng"], e["H"], DTYPES[el]
    stale(e)
    emb = rows_of(79, H, 1, dtype)
    check_call(e, lambda: eng.prefill(1, 79, embeds=emb), [emb], 1, 0, True, f"{el} one-layer prefill of 79 rows (last-rows shortcut)")
    three = [rows_of(37, H, 7 + i, dtype) for i in range(3)]
    check_call(e, lambda: eng.prefill_multi(0, three), three, 0, 0, True, f"{el} one-layer prefill_multi of 3 x 37 rows")
    new = [rows_of(13, H, 30 + i, dtype) for i in range(3)]
    check_call(e, lambda: eng.prefill_append(0, 37, new), new, 0, 37, True, f"{el} one-layer prefill_append of 3 x 13 rows at past = 37")
    k_short = e["K0"].clone()
    stale(e)
    eng.prefill_multi(0, three)
    hid = eng.prefill_append(1, 37, new[1], want_hidden=True)                  # hidden rows asked for: the full layer, no shortcut
    assert hid.shape[0] == 13
    ss = e["slot_stride"]
    same_bits(e["K0"][ss:2 * ss].view(e["NKV"], -1)[:, :50 * e["HD"]], k_short[ss:2 * ss].view(e["NKV"], -1)[:, :50 * e["HD"]], f"{el} shortcut against the full layer: K rows of slot 1")


def test_engine_splice_is_gather_rows(el, engines):
    e = engines(el, 2)
    eng, cfg, g, dtype = e["eng"], e["cfg"], e["g"], DTYPES[el]
    H, V = cfg.hidden_size, cfg.vocab_size
    tabs = [g("model.embed_tokens.weight"), None, g("model.time_tower.embed_tokens.weight"), g("model.score_tower.embed_tokens.weight"),
            g("model.sync_tower.embed_tokens.weight").reshape(1, H).contiguous(), None]
    ids = [1, 0, V - 1, -203, 17, -204, -205, -203, V - 1, -1, -204, 5, 5, -205]
    time_rows, score_rows = [0, cfg.time_vocab_size - 1], [cfg.score_vocab_size - 1, 0]

    def lists(ids, video_rows=0):
        kind, row, ti, si = [], [], 0, 0
        for i in ids:
            if i in (-200, -201):
                kind += [1] * video_rows
                row += list(range(video_rows))
            elif i == -205:
                kind, row = kind + [4], row + [0]
            elif i == -203:
                kind, row, ti = kind + [2], row + [time_rows[ti]], ti + 1
            elif i == -204:
                kind, row, si = kind + [3], row + [score_rows[si]], si + 1
            else:
                kind, row = kind + [0], row + [max(i, 0)]
        return torch.tensor(kind, dtype=torch.int32, device=DEV), torch.tensor(row, dtype=torch.int32, device=DEV)

    got = eng.embed_rows(ids, time_rows, score_rows, want_output=True)
    kind, row = lists(ids)
    out = PG.sentinel_buf((len(ids) + 2) * H, dtype, DEV)
    ops.gather_rows(tabs, kind, row, out, len(ids), H)
    same_bits(got.reshape(-1), out[:len(ids) * H], f"{el} embed_rows against gather_rows")
    assert bool((PG.bits(out[len(ids) * H:]) == PG.SENTINEL).all())
    ts = [[float(i)] for i in range(4)]
    video = eng.encode_video(synth.synth_frames(cfg, 0).to(dtype), ts, want_output=True).clone()
    ids2 = ids[:4] + [-201] + ids[4:]
    L, got2 = eng.splice(ids2, time_rows, score_rows, want_output=True)
    kind, row = lists(ids2, video.shape[0])
    assert L == len(ids2) - 1 + video.shape[0] == kind.numel()
    out = PG.sentinel_buf(L * H, dtype, DEV)
    ops.gather_rows(tabs[:1] + [video.contiguous()] + tabs[2:], kind, row, out, L, H)
    same_bits(got2.reshape(-1), out, f"{el} splice against gather_rows")
