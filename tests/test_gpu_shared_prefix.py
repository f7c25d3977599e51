"""A batch's shared prompt prefix on the device: the decode attention reading the shared positions from one slot
(trace_op_attn_decode_shared, trace_decode_set_shared_prefix) and the prefill of the shared rows once per batch (trace_llm_prefill_shared,
TraceEngine.encode_prefill).

Both halves claim an identity, not a tolerance: the shared rows are the same bits in every slot, so reading them from one place, or
computing them once and copying them, changes no output bit.  "Equal" below is torch.equal on attention outputs and fp32 logits, and == on
ids and heads.  The tests that poison cache rows prove where the kernel reads: private rows the shared run must not read hold other finite
values, and the outputs still match a run in which they held the right ones.

Tiny geometry (config.tiny, 4 frames = 56 video rows); prompts of P text rows, <video>, 13 more rows."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import attn_probes as P  # noqa: E402
from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd._lib import TraceHipError  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402

DEV = "cuda"
NQ, NKV, HD = 8, 2, 128
SCALE = HD ** -0.5


# ---------------------------------------------------------------------------------------------------- the kernel, exact
def _caches(B, max_ctx, seed):
    """q [B, NQ * HD]; K [B + 1, NKV, max_ctx, HD] and V^T [B + 1, NKV, HD, max_ctx] with slot B as the shared one; `other`: a second set of
    values for rows the shared run must not read"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).to(DEV)
    return r(B, NQ * HD), r(B + 1, NKV, max_ctx, HD), r(B + 1, NKV, HD, max_ctx), r(B + 1, NKV, max_ctx, HD), r(B + 1, NKV, HD, max_ctx)


def _shared_vs_private(poss, max_ctx, rows, nsplit, seed=0):
    """(unshared output over private slots that hold the shared values, shared output over private slots that hold other values there)"""
    B = len(poss)
    q, k, vt, k2, vt2 = _caches(B, max_ctx, seed)
    pos = torch.tensor(poss, dtype=torch.int32, device=DEV)
    kp, vp = k.clone(), vt.clone()                     # the unshared run: every private slot holds slot B's rows below `rows`
    kp[:B, :, :rows] = k[B, :, :rows]
    vp[:B, :, :, :rows] = vt[B, :, :, :rows]
    want = ops.attn_decode(q, kp[:B].contiguous(), None, pos, nsplit, SCALE, vtcache=vp[:B].contiguous())
    ks, vs = k.clone(), vt.clone()                     # the shared run: the private rows below `rows` hold something else
    ks[:B, :, :rows] = k2[:B, :, :rows]
    vs[:B, :, :, :rows] = vt2[:B, :, :, :rows]
    got = ops.attn_decode_shared(q, ks, vs, pos, nsplit, SCALE, B, rows)
    if rows:
        assert not torch.equal(ops.attn_decode_shared(q, ks, vs, pos, nsplit, SCALE, -1, 0), want), "the poisoned rows do not show: the test proves nothing"
    return want, got


@pytest.mark.parametrize("nsplit", [P.decode_nsplit(3), 2])
@pytest.mark.parametrize("rows", [0, 32, 64])
def test_shared_rows_come_from_the_shared_slot_and_nothing_else_changes(rows, nsplit):
    """B = 3, max_ctx 128, the default split count and a two-way split.  Positions 33 / 64 / 97; under 64 shared rows the first sequence would be
    shorter than the prefix (refused: next test), so that case runs 64 / 97 / 127."""
    poss = [33, 64, 97] if rows <= 32 else [64, 97, 127]
    want, got = _shared_vs_private(poss, 128, rows, nsplit)
    assert torch.equal(got, want)


@pytest.mark.parametrize("waves", [-1, 1])
@pytest.mark.parametrize("rows,nsplit", [(160, 1), (96, 1), (256, 2)])
def test_shared_boundary_inside_a_wave_s_block_loop(rows, nsplit, waves):
    """Contexts long enough for a wave's steady loop (more blocks per split than waves): the block a wave requests ahead lies on the other side of
    the boundary than the one it computes on.  4-wave and 3-wave workgroups."""
    with ops.tuned(attn__decode__waves=waves):
        want, got = _shared_vs_private([479, 300, 256, 511], 512, rows, nsplit, seed=3)
    assert torch.equal(got, want)


def test_a_sequence_shorter_than_the_shared_rows_is_refused_before_any_launch():
    q, k, vt, _, _ = _caches(3, 128, 1)
    pos = torch.tensor([33, 64, 97], dtype=torch.int32, device=DEV)
    with pytest.raises(TraceHipError, match="error -1 in trace_op_attn_decode_shared: a sequence is shorter than the shared prefix"):      # TRACE_ERR_ARG
        ops.attn_decode_shared(q, k, vt, pos, 2, SCALE, 3, 64)
    with pytest.raises(TraceHipError, match="shared slot out of range"):
        ops.attn_decode_shared(q, k, vt, pos, 2, SCALE, 4, 32)
    assert torch.equal(ops.attn_decode_shared(q, k, vt, pos, 2, SCALE, 3, 63),           # floored to whole blocks: 32
                       ops.attn_decode_shared(q, k, vt, pos, 2, SCALE, 3, 32))


# ---------------------------------------------------------------------------------------------------- the engine, tiny geometry
NEW = 10


def _prompt(cfg, P_, seed=7):
    return synth.synth_prompt_ids(cfg, n_text=P_ + 14, video_pos=P_, seed=seed).tolist()


def _videos(cfg, n, base=0):
    vids = [synth.synth_frames(cfg, base + b).to(torch.bfloat16).cuda() for b in range(n)]
    ts = [[[float(i) * 2.5 + b] for i in range(4)] for b in range(n)]
    return vids, ts


@pytest.fixture(scope="module")
def eng():
    cfg = tcfg.tiny(num_frames=4)
    e = TraceEngine(cfg, max_batch=8, max_ctx=192, max_frames=4, max_new_tokens=32)
    e.load_weights(synth.state_dict(cfg).items())
    yield cfg, e
    e.close()


def _prefill(e, vids, ts, ids, min_batch, slot0=0):
    """encode_prefill under a threshold -> (what it returned, rows it prefilled)"""
    before = e.stats["prefill_rows"]
    e.share_prefix_min_batch = min_batch
    try:
        shared = e.encode_prefill(vids, ts, ids, slot0)
    finally:
        del e.share_prefix_min_batch                    # back to the class default
    return shared, e.stats["prefill_rows"] - before


def _logits(e, slots, shared, steps=3):
    lg = [e.decode_begin(list(slots), [1] * len(slots), NEW, want_logits=True, shared_prefix=shared).clone()]
    for _ in range(steps):
        lg.append(e.decode_steps(1, use_graph=False, want_logits=True).clone())
    return torch.stack(lg)


def _generate(e, vids, ts, ids, min_batch, **kw):
    e.share_prefix_min_batch = min_batch
    try:
        return e.generate(vids, ts, ids, [1] * len(vids), NEW, **kw)
    finally:
        del e.share_prefix_min_batch


@pytest.fixture(scope="module")
def unshared(eng):
    """four videos, one prompt of P = 64 rows before <video>, prefilled and decoded without sharing: (inputs, rows, logits, ids, heads)"""
    cfg, e = eng
    vids, ts = _videos(cfg, 4)
    ids = [_prompt(cfg, 64)] * 4
    shared, rows = _prefill(e, vids, ts, ids, 99)
    assert shared is None
    lg = _logits(e, range(4), None)
    out = _generate(e, vids, ts, ids, 99)
    return (vids, ts, ids), rows, lg, out


def test_default_threshold_leaves_small_batches_alone(eng, unshared):
    cfg, e = eng
    (vids, ts, ids), rows, _, _ = unshared
    assert TraceEngine.share_prefix_min_batch == 32 and "share_prefix_min_batch" not in vars(e)
    before = e.stats["prefill_rows"]
    assert e.encode_prefill(vids, ts, ids, 0) is None
    assert e.stats["prefill_rows"] - before == rows == 4 * (64 + 56 + 13)


def test_shared_batch_same_logits_fewer_rows(eng, unshared):
    cfg, e = eng
    (vids, ts, ids), rows, lg, _ = unshared
    shared, rows_s = _prefill(e, vids, ts, ids, 2)
    assert shared == (0, 64)
    assert rows - rows_s == 3 * 64
    got = _logits(e, range(4), shared)
    assert torch.equal(got[0], lg[0]), "step-0 logits"
    assert torch.equal(got, lg)
    assert torch.equal(_logits(e, range(4), None), lg)          # the same slots decoded unshared: the prefill half alone


@pytest.mark.parametrize("use_graph", [True, False])
def test_shared_generate_equals_unshared(eng, unshared, use_graph):
    cfg, e = eng
    (vids, ts, ids), _, _, want = unshared
    got = _generate(e, vids, ts, ids, 2, use_graph=use_graph)
    assert got[0] == want[0] and got[1] == want[1]
    with ops.tuned(attn__decode__nsplit=2):
        got2 = _generate(e, vids, ts, ids, 2, use_graph=False)
    assert got2[0] == want[0] and got2[1] == want[1]


def _cache_views(e, nslots):
    kc, vc, xl = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 8)()
    _lib.check(e.lib.trace_debug_buffers(e.h, C.byref(kc), C.byref(vc), C.byref(xl), st))
    layer_stride, slot_stride, head_stride, ctx_pad, NL, NKV_, HD_, H = [int(x) for x in st]
    assert layer_stride == nslots * slot_stride

    class _Dev:
        def __init__(self, ptr, n):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i2", "data": (ptr, False), "version": 3}
    K = torch.as_tensor(_Dev(kc.value, layer_stride * NL), device="cuda").view(NL, nslots, NKV_, ctx_pad, HD_)
    VT = torch.as_tensor(_Dev(vc.value, layer_stride * NL), device="cuda").view(NL, nslots, NKV_, HD_, ctx_pad)
    return K, VT


def test_prefix_of_40_rows_shares_40_in_prefill_and_32_in_decode(eng):
    """P = 40 is no multiple of the attention's 32-position block: the prefill shares all 40 rows, the decode attention the first 32.  Shown on the
    cache: with the other slots' rows [0, 32) overwritten by other finite values the shared decode still gives the unshared logits (it reads them from
    slot 0), and with slot 0's rows [32, 40) overwritten as well the OTHER sequences still do (they read those rows from their own slots)."""
    cfg, e = eng
    vids, ts = _videos(cfg, 4, base=20)
    ids = [_prompt(cfg, 40, seed=11)] * 4
    _, rows = _prefill(e, vids, ts, ids, 99)
    want = _logits(e, range(4), None)
    shared, rows_s = _prefill(e, vids, ts, ids, 2)
    assert shared == (0, 40) and rows - rows_s == 3 * 40
    K, VT = _cache_views(e, 8)
    K[:, 1:4, :, :32] = K[:, 1:4, :, 40:72].clone()
    VT[:, 1:4, :, :, :32] = VT[:, 1:4, :, :, 40:72].clone()
    assert torch.equal(_logits(e, range(4), shared), want)
    shared, _ = _prefill(e, vids, ts, ids, 2)
    K[:, 0, :, 32:40] = K[:, 0, :, 48:56].clone()
    VT[:, 0, :, :, 32:40] = VT[:, 0, :, :, 48:56].clone()
    got = _logits(e, range(4), shared)
    assert torch.equal(got[:, 1:], want[:, 1:])
    assert not torch.equal(got[1:, 0], want[1:, 0]), "sequence 0 attends its own rows 32 .. 39: overwriting them must show"


def test_prompts_that_differ_before_the_video_do_not_share(eng):
    cfg, e = eng
    vids, ts = _videos(cfg, 4, base=30)
    ids = [_prompt(cfg, 64)] * 3 + [_prompt(cfg, 64, seed=8)]
    assert ids[3][0] == ids[0][0] and ids[3][:64] != ids[0][:64]
    shared, rows = _prefill(e, vids, ts, ids, 2)
    assert shared is None and rows == 4 * (64 + 56 + 13)
    assert _generate(e, vids, ts, ids, 2) == _generate(e, vids, ts, ids, 99)


def test_batch_below_the_threshold_does_not_share(eng, unshared):
    cfg, e = eng
    (vids, ts, ids), rows, _, want = unshared
    shared, rows_s = _prefill(e, vids, ts, ids, 5)
    assert shared is None and rows_s == rows
    got = _generate(e, vids, ts, ids, 5)
    assert got[0] == want[0] and got[1] == want[1]


def test_kv8_engine_does_not_share(unshared):
    """under the e4m3 KV cache a continuation attends quantised rows and is not bit-identical: the engine prefills whole prompts whatever the threshold"""
    (vids, ts, ids), rows, _, _ = unshared
    cfg = tcfg.tiny(num_frames=4)
    e = TraceEngine(cfg, max_batch=4, max_ctx=192, max_frames=4, max_new_tokens=32, kv_cache="fp8")
    try:
        e.load_weights(synth.state_dict(cfg).items())
        shared, rows_s = _prefill(e, vids, ts, ids, 2)
        assert shared is None and rows_s == rows
        assert _generate(e, vids, ts, ids, 2) == _generate(e, vids, ts, ids, 99)
        with pytest.raises(TraceHipError, match="trace_decode_set_shared_prefix"):
            e.decode_begin(range(4), [1] * 4, NEW, shared_prefix=(0, 64))
    finally:
        e.close()


def test_two_pipelined_batches_equal_two_generate_calls(eng):
    """generate_stream: each bank of KV slots has its own shared slot (0 and 4 here), and the captured steps of the two are cached apart"""
    cfg, e = eng
    batches = []
    for k in range(2):
        vids, ts = _videos(cfg, 4, base=40 + 10 * k)
        batches.append((vids, ts, [_prompt(cfg, 64, seed=5 + k)] * 4, [1] * 4, None))
    want = [_generate(e, v, t, i, 99) for v, t, i, _, _ in batches]
    e.share_prefix_min_batch = 2
    try:
        before = e.stats["prefill_rows"]
        got = list(e.generate_stream(batches, NEW))
        assert e.stats["prefill_rows"] - before == 2 * (4 * (64 + 56 + 13) - 3 * 64)
        again = list(e.generate_stream(batches[::-1], NEW))          # banks swapped: every (slot, rows) pair replays its own graph
    finally:
        del e.share_prefix_min_batch
    assert [g[0] for g in got] == [w[0] for w in want] and [g[1] for g in got] == [w[1] for w in want]
    assert [g[0] for g in again] == [w[0] for w in want[::-1]]


def test_begin_refuses_a_sequence_shorter_than_the_shared_rows(eng, unshared):
    cfg, e = eng
    (vids, ts, ids), _, _, _ = unshared
    _prefill(e, vids, ts, ids, 99)
    e.embed_rows(ids[0][:40])
    e.prefill(4, 40)                                                     # slot 4: 40 rows only
    with pytest.raises(TraceHipError, match="a sequence is shorter than the shared prefix"):
        e.decode_begin([0, 1, 4], [1] * 3, NEW, shared_prefix=(0, 64))
    lg = e.decode_begin([0, 1], [1] * 2, NEW, want_logits=True)          # the refused request is gone: this batch decodes unshared
    assert lg.shape[0] == 2
