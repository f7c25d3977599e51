"""The six calls that prefill share one layer body (engine.hip prefill_impl) and one checked entry path (prefill_entry).

The routes are one body: prefill, prefill_multi of one and prefill_append at past = 0 leave the same bits in EVERY word of every layer's K and V^T caches and of
the xlast rows, compared after a common stale fill so that a store outside the prompt's rows shows too; so do prefill_pair and prefill_multi of two, and a
prompt from the engine's own embedding buffer (embeds=None after embed_rows) and the same rows handed in.  On a one-layer engine the calls take the last-rows
shortcut, and the full layer (want_hidden) leaves the shortcut's bits.  L = 1 is the L > 1 edge of the shortcut, 37 and 79 are multiples of no tile.

The old three refuse as before: every bad argument of trace_llm_prefill, trace_llm_prefill_pair and trace_llm_prefill_multi answers the status their own
checks gave before they went through append_check (TRACE_ERR_ARG for each, read off those checks), before any launch: the caches keep their bits and the
slots their lengths."""
import ctypes as C
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import prefill_glue_probes as PG  # noqa: E402
from test_gpu_prefill_glue_probes import DEV, DTYPES, MAX_CTX, NSLOTS, _Dev, el, engines, rows_of, same_bits, state  # noqa: E402,F401
from trace_amd import _lib, config as tcfg  # noqa: E402
from trace_amd.engine import TraceEngine  # noqa: E402

ERR_ARG = -1                       # TRACE_ERR_ARG (csrc/common.h)


def views(eng, dtype, slots):
    """every layer's K and V^T caches and the slots' xlast rows, as flat tensors over the engine's own memory (trace_debug_buffers)"""
    kc, vc, xl = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 8)()
    _lib.check(eng.lib.trace_debug_buffers(eng.h, C.byref(kc), C.byref(vc), C.byref(xl), st))
    layer_stride, slot_stride, NL, H = int(st[0]), int(st[1]), int(st[4]), int(st[7])
    assert layer_stride == slots * slot_stride
    at = lambda p, n: torch.as_tensor(_Dev(p.value, n), device="cuda").view(dtype)
    return {"K": at(kc, NL * layer_stride), "V^T": at(vc, NL * layer_stride), "xlast": at(xl, slots * H)}


def stale_fill(v, dtype):
    """the same finite words everywhere before each call under comparison"""
    for i, t in enumerate(v.values()):
        t.copy_((0.05 * torch.randn(t.numel(), generator=torch.Generator().manual_seed(900 + i))).to(dtype).to(DEV))


def after(v, dtype, call):
    stale_fill(v, dtype)
    call()
    torch.cuda.synchronize()
    return {k: t.clone() for k, t in v.items()}


def same_state(got, want, what):
    for k in want:
        same_bits(got[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("layers", [2, 1])
def test_routes_are_one_body(el, engines, layers):
    e = engines(el, layers)
    eng, H, dtype = e["eng"], e["H"], DTYPES[el]
    v = views(eng, dtype, NSLOTS)
    for L in (1, 37, 79):
        emb = rows_of(L, H, L, dtype)
        want = after(v, dtype, lambda: eng.prefill(1, L, embeds=emb))
        filled = after(v, dtype, lambda: None)
        assert not torch.equal(PG.bits(want["K"]), PG.bits(filled["K"])) and not torch.equal(PG.bits(want["xlast"]), PG.bits(filled["xlast"]))
        same_state(after(v, dtype, lambda: eng.prefill_multi(1, [emb])), want, f"{el} {layers} layers, L = {L}: prefill_multi of one against prefill")
        same_state(after(v, dtype, lambda: eng.prefill_append(1, 0, emb)), want, f"{el} {layers} layers, L = {L}: prefill_append at past = 0 against prefill")
        if layers == 1:                # the calls above took the last-rows shortcut (L > 1); hidden rows asked for: the full layer
            hid = []
            full = after(v, dtype, lambda: hid.append(eng.prefill_append(1, 0, emb, want_hidden=True)))
            assert hid[0].shape == (L, H)
            same_state(full, want, f"{el} one layer, L = {L}: the full layer against the shortcut")
        two = [rows_of(L, H, 50 + L + i, dtype) for i in range(2)]
        want = after(v, dtype, lambda: eng.prefill_multi(2, two))
        same_state(after(v, dtype, lambda: eng.prefill_pair(2, two[0], two[1])), want, f"{el} {layers} layers, L = {L}: prefill_pair against prefill_multi of two")


@pytest.mark.parametrize("layers", [2, 1])
def test_internal_buffer_is_the_rows_handed_in(el, engines, layers):
    e = engines(el, layers)
    eng, dtype = e["eng"], DTYPES[el]
    v = views(eng, dtype, NSLOTS)
    ids = [1, 5, 17, 3, 9, 2, 11]
    rows = eng.embed_rows(ids, want_output=True).clone()

    def from_buffer():
        eng.embed_rows(ids)
        eng.prefill(3, len(ids))
    want = after(v, dtype, lambda: eng.prefill(3, len(ids), embeds=rows))
    same_state(after(v, dtype, from_buffer), want, f"{el} {layers} layers: prefill(embeds=None) after embed_rows against the rows as a tensor")


def bad_calls(lib, h, max_batch, max_ctx, embs):
    """(what, call): every argument the old three refuse, at a context of max_batch slots; embs: 2 device tensors of one shape [L, hidden]"""
    L = embs[0].shape[0]
    p = [C.c_void_p(t.data_ptr()) for t in embs]
    arr = lambda *ps: (C.c_void_p * len(ps))(*ps)
    one, pair, multi = lib.trace_llm_prefill, lib.trace_llm_prefill_pair, lib.trace_llm_prefill_multi
    out = []
    for what, slot, n_L in (("slot -1", -1, L), ("slot = max_batch", max_batch, L), ("L = 0", 0, 0), ("L = max_ctx + 1", 0, max_ctx + 1)):
        out.append((f"prefill, {what}", lambda slot=slot, n_L=n_L: one(h, slot, p[0], n_L, None, None)))
        out.append((f"prefill_pair, {what}", lambda slot=slot, n_L=n_L: pair(h, slot, p[0], p[1], n_L, None)))
        out.append((f"prefill_multi, {what}", lambda slot=slot, n_L=n_L: multi(h, slot, arr(p[0], p[1]), 2, n_L, None)))
    out.append(("prefill_pair, slot0 + 2 > max_batch", lambda: pair(h, max_batch - 1, p[0], p[1], L, None)))
    out.append(("prefill_multi, slot0 + n > max_batch", lambda: multi(h, max_batch - 2, arr(p[0], p[1], p[0]), 3, L, None)))
    out.append(("prefill_multi, n = 0", lambda: multi(h, 0, arr(p[0]), 0, L, None)))
    out.append(("prefill_multi, n = 9", lambda: multi(h, 0, arr(*[p[0]] * 9), 9, L, None)))
    out.append(("prefill_multi, a null entry", lambda: multi(h, 0, arr(p[0], None), 2, L, None)))
    out.append(("prefill_multi, a null first entry", lambda: multi(h, 0, arr(None, p[1]), 2, L, None)))
    out.append(("prefill_multi, embeds NULL, n = 1", lambda: multi(h, 0, None, 1, L, None)))
    out.append(("prefill_multi, embeds NULL, n = 2", lambda: multi(h, 0, None, 2, L, None)))
    out.append(("prefill_pair, embeds0 NULL", lambda: pair(h, 0, None, p[1], L, None)))
    out.append(("prefill_pair, embeds1 NULL", lambda: pair(h, 0, p[0], None, L, None)))
    return out


def refused(call, what):
    with pytest.raises(_lib.TraceHipError, match=rf"error {ERR_ARG} in trace_llm_prefill") as ei:
        call()
    print(f"{what}: {ei.value}")


def test_old_three_refuse_as_before(el, engines):
    e = engines(el, 2)
    eng, H, dtype = e["eng"], e["H"], DTYPES[el]
    v = views(eng, dtype, NSLOTS)
    r1, r2 = [rows_of(1, H, 60 + i, dtype) for i in range(NSLOTS)], [rows_of(1, H, 70 + i, dtype) for i in range(NSLOTS)]

    def settle():                      # every slot holds 21 rows; row 21 of K is r2's, V^T is zero from position 21 to the end of its block
        eng.prefill_append(0, 20, r1)
        torch.cuda.synchronize()
        return {k: t.clone() for k, t in v.items()}
    eng.prefill_multi(0, [rows_of(20, H, 80 + i, dtype) for i in range(NSLOTS)])
    eng.prefill_append(0, 20, r1)
    eng.prefill_append(0, 21, r2)
    held = settle()
    embs = [rows_of(13, H, 90 + i, dtype) for i in range(2)]
    for what, call in bad_calls(eng.lib, eng.h, NSLOTS, MAX_CTX, embs):
        refused(call, f"{el} {what}")
        torch.cuda.synchronize()
        same_state(v, held, f"{el} {what}: refused, yet written")
        eng.prefill_append(0, 21, r2)              # accepted only while every slot still holds its 21 rows
        same_state(settle(), held, f"{el} {what}: the slots after the refusal")


def test_workspace_rows_refused(el):
    """n x L above the prefill workspace: five max_ctx-long prompts where the workspace is 4 max_ctx rows (max_ctx = 2048: max(8192, min(8192, 16384)))"""
    dtype = DTYPES[el]
    cfg = dataclasses.replace(tcfg.tiny(num_frames=4), num_hidden_layers=1)
    big = TraceEngine(cfg, max_batch=8, max_ctx=2048, max_frames=4, max_new_tokens=8, dtype=dtype)
    try:
        big.load_weights(state(cfg).items())
        assert big.prefill_rows == 4 * 2048
        H = cfg.hidden_size
        v = views(big, dtype, 8)
        pre = [rows_of(10, H, 40 + i, dtype) for i in range(5)]
        big.prefill_multi(0, pre)
        torch.cuda.synchronize()
        held = {k: t.clone() for k, t in v.items()}
        long_embs = [rows_of(2048, H, 30 + i, dtype) for i in range(5)]
        ptrs = (C.c_void_p * 5)(*[t.data_ptr() for t in long_embs])
        refused(lambda: big.lib.trace_llm_prefill_multi(big.h, 0, ptrs, 5, 2048, None), f"{el} prefill_multi, 5 x 2048 rows over 8192")
        torch.cuda.synchronize()
        same_state(v, held, f"{el} 5 x 2048 rows: refused, yet written")
        big.prefill_append(0, 10, [rows_of(1, H, 50 + i, dtype) for i in range(5)])       # the five slots still hold their 10 rows
    finally:
        big.close()
