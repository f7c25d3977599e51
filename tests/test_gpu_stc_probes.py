"""The STC connector's row kernels against float64 (tests/stc_probes.py; tests/test_stc_probes_cpu.py shows on the CPU which faults these probes
reject): dwconv3x3_kernel, avgpool_kernel, bias_act_kernel, scale_rows_kernel, im2col3d_kernel and permute_conv3d_w_kernel through their trace_op_*
entries, at odd and even extents, ragged pixel counts, one and several workgroups and the shapes whose launches take a second grid-stride trip; the
Conv3d sampler and the squeeze-excite gate chained as the engine chains them; the engine's own trace_stc_connector against the same chain run
through `ops` from the same state dict, bit for bit; and every op's refusals.

The largest error / bound per (library, kernel, probe) is printed and appended to the file the environment variable TRACE_STC_PROBE_MARGINS names
(profiles/stc_probe_margins.txt is made from it); 0.000 stands for an equality check that held.  Both libraries (bf16 and fp16 elements) run
everything."""
import dataclasses
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import stc_probes as SP  # noqa: E402
from gemm_probes import round16  # noqa: E402
from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
MARGINS = {}                      # (library, kernel, probe) -> [max err / bound, cases]


@pytest.fixture(scope="module", autouse=True)
def margins_record():
    yield
    lines = [f"{lib:<5} {k:<18} {p:<22} max err/bound {m[0]:.3f}  cases {m[1]}" for (lib, k, p), m in sorted(MARGINS.items())]
    print("\n".join(lines))
    path = os.environ.get("TRACE_STC_PROBE_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(params=["bf16", "f16"])
def el(request):
    ops.use(request.param)
    yield request.param
    ops.use("bf16")


def judge(el, kernel, probe, verdict, what):
    ratio, bad = verdict
    m = MARGINS.setdefault((el, kernel, probe), [0.0, 0])
    m[0], m[1] = max(m[0], ratio), m[1] + 1
    assert ratio <= 1.0 and not bad, f"{kernel} {probe} {what}: error / bound {ratio:.3f}; " + "; ".join(bad)


# ---- the six kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SP.DWCONV_SHAPES + [SP.DWCONV_TWO_TRIPS], ids=lambda s: "x".join(map(str, s)))
def test_dwconv3x3(el, shape):
    """1 x 1, single rows and columns (every tap but the centre outside), odd and even grids, C of 1, 2, 3, 8, 9, 32 and 512 chunks, the 13 x 13 grid
    of the real sampler output, and 9 x 24 x 24 x 4096: 2 654 208 items, a second trip for the last 557 056"""
    N, H, W, C = shape
    if shape == SP.DWCONV_TWO_TRIPS:
        assert SP.trips_of(N * H * W * C // 8) == 2
    for name in SP.DWCONV_PROBES:
        judge(el, "dwconv3x3", name, SP.dwconv_case(name, N, H, W, C, DTYPES[el], DEV, lambda x, w, y: ops.dwconv3x3(x, w, out=y)), f"shape {shape}")


@pytest.mark.parametrize("C", SP.AVGPOOL_C)
def test_avgpool(el, C):
    """HW of 1, 7 and 31 (idle pixel lanes), 32, 33 and 36 (one full round and a ragged tail), 169 and 576 (the real grids); one, three and 64 slabs"""
    for N, HW, Cc in SP.AVGPOOL_SHAPES:
        if Cc != C:
            continue
        for name in SP.AVGPOOL_PROBES:
            for shift in (SP.onehot_shifts(HW, C) if name == "onehot" else (0,)):
                judge(el, "avgpool", name + ("=" if SP.avgpool_is_exact(name, HW) else ""),
                      SP.avgpool_case(name, N, HW, C, DTYPES[el], DEV, lambda x, y: ops.avgpool(x, out=y), shift), f"N {N} HW {HW} C {C} shift {shift}")


@pytest.mark.parametrize("C", SP.BIAS_ACT_C)
def test_bias_act(el, C):
    for rows in SP.BIAS_ACT_ROWS:
        for act, aname in SP.ACT_NAMES.items():
            for with_bias in (False, True):
                for name in SP.BIAS_ACT_PROBES:
                    judge(el, "bias_act", f"{name} {aname}{' +bias' if with_bias else ''}",
                          SP.bias_act_case(name, rows, C, act, with_bias, DTYPES[el], DEV, lambda x, b, a: ops.bias_act(x, b, a)), f"rows {rows} C {C}")


def test_bias_act_second_trip(el):
    rows, C = SP.BIAS_ACT_TWO_TRIPS
    assert SP.trips_of(rows * C // 8) == 2
    for act, with_bias, name in ((SP.ACT_SILU, True, "grid"), (SP.ACT_GELU, False, "grid"), (SP.ACT_SIGMOID, True, "gauss")):
        judge(el, "bias_act", f"{name} {SP.ACT_NAMES[act]}{' +bias' if with_bias else ''}",
              SP.bias_act_case(name, rows, C, act, with_bias, DTYPES[el], DEV, lambda x, b, a: ops.bias_act(x, b, a)), f"rows {rows} C {C}")


@pytest.mark.parametrize("shape", SP.SCALE_SHAPES + [SP.SCALE_TWO_TRIPS], ids=lambda s: "x".join(map(str, s)))
def test_scale_rows(el, shape):
    N, HW, C = shape
    if shape == SP.SCALE_TWO_TRIPS:
        assert SP.trips_of(N * HW * C // 8) == 2
    for name in SP.SCALE_PROBES:
        judge(el, "scale_rows", name, SP.scale_case(name, N, HW, C, DTYPES[el], DEV, lambda x, g: ops.scale_rows(x, g)), f"shape {shape}")


@pytest.mark.parametrize("shape", SP.IM2COL_SHAPES + [SP.IM2COL_TWO_TRIPS], ids=lambda s: "x".join(map(str, s)))
def test_im2col3d(el, shape):
    """odd extents (the trailing tap is a real pixel) and even ones (it is a zero that must be WRITTEN: the matrix is sentinel-filled), T = 1"""
    T, H, W, C = shape
    if shape == SP.IM2COL_TWO_TRIPS:
        assert SP.trips_of((T // 2 + 1) * (H // 2 + 1) * (W // 2 + 1) * C) == 2
    judge(el, "im2col3d", "ident", SP.im2col_case(T, H, W, C, DTYPES[el], DEV, lambda x, A: ops.im2col3d(x, out=A)), f"shape {shape}")


@pytest.mark.parametrize("shape", SP.PERMUTE_SHAPES + [SP.PERMUTE_TRIPS], ids=lambda s: "x".join(map(str, s)))
def test_permute_conv3d_w(el, shape):
    Co, Ci = shape
    judge(el, "permute_conv3d_w", "ident", SP.permute_case(Co, Ci, DTYPES[el], DEV, lambda w, o: ops.permute_conv3d_w(w, out=o)), f"shape {shape}")


# ---- the chains ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H,W", [(3, 5, 5), (4, 6, 6)])
def test_conv3d_as_the_engine_computes_it(el, T, H, W):
    """im2col3d -> the permuted weight -> trace_op_gemm with bias -> bias_act(SiLU), at the smallest widths the GEMM takes (K = 8 C = 64, N = 128):
    on integer data the pre-activation equals F.conv3d(stride 2, padding 1) in float64 exactly — the gather's and the permute's tap orders agree"""
    dtype, C, Co = DTYPES[el], 8, 128
    x, w, b = SP.conv3d_probe(T, H, W, C, Co, dtype, DEV)
    col = ops.im2col3d(x)
    wp = ops.permute_conv3d_w(w)
    pre = ops.gemm(col, wp, bias=b)
    ref = SP.conv3d_reference(x, w, b)
    assert pre.shape == ref.shape == ((T // 2 + 1) * (H // 2 + 1) * (W // 2 + 1), Co)
    judge(el, "conv3d chain", "pre-activation=", (SP.ratio_exact(pre, ref, dtype), []), f"T {T} H {H} W {W}")
    pre16 = pre.clone()
    ops.bias_act(pre, None, SP.ACT_SILU)
    r64, t64 = SP.bias_act_reference(pre16, None, SP.ACT_SILU)
    judge(el, "conv3d chain", "silu", (SP.ratio_bound(pre, r64, SP.bias_act_bound(r64, t64, SP.ACT_SILU, dtype), dtype), []), f"T {T} H {H} W {W}")


@pytest.mark.parametrize("C,rd,HW", [(256, 64, 36), (1024, 256, 49)])
def test_squeeze_excite_as_the_engine_computes_it(el, C, rd, HW):
    """avgpool -> skinny_gemm -> bias_act(SiLU) -> skinny_gemm -> bias_act(sigmoid) -> scale_rows: every stage by its own bound against float64 of
    the previous stage's 16-bit output (the GEMVs: a K-term fp32 dot product in any order, stc_probes.linear_bound)"""
    dtype = DTYPES[el]
    for N in (1, 3, 17, 32):
        pr = SP.se_probe(N, HW, C, rd, dtype, DEV)
        what = f"C {C} rd {rd} N {N}"
        pool = ops.avgpool(pr.z)
        ref, ma = SP.avgpool_reference(pr.z)
        judge(el, "se chain", "avgpool", (SP.ratio_bound(pool, ref, SP.avgpool_bound(ref, ma, HW, dtype), dtype), []), what)
        g1 = ops.skinny_gemm(pool, pr.fc1w)
        ref = pool.double() @ pr.fc1w.double().t()
        judge(el, "se chain", "fc1", (SP.ratio_bound(g1, ref, SP.linear_bound(pool, pr.fc1w, ref, dtype), dtype), []), what)
        g1_16 = g1.clone()
        ops.bias_act(g1, pr.fc1b, SP.ACT_SILU)
        ref, t = SP.bias_act_reference(g1_16, pr.fc1b, SP.ACT_SILU)
        judge(el, "se chain", "silu", (SP.ratio_bound(g1, ref, SP.bias_act_bound(ref, t, SP.ACT_SILU, dtype), dtype), []), what)
        g2 = ops.skinny_gemm(g1, pr.fc2w)
        ref = g1.double() @ pr.fc2w.double().t()
        judge(el, "se chain", "fc2", (SP.ratio_bound(g2, ref, SP.linear_bound(g1, pr.fc2w, ref, dtype), dtype), []), what)
        g2_16 = g2.clone()
        ops.bias_act(g2, pr.fc2b, SP.ACT_SIGMOID)
        ref, t = SP.bias_act_reference(g2_16, pr.fc2b, SP.ACT_SIGMOID)
        judge(el, "se chain", "sigmoid", (SP.ratio_bound(g2, ref, SP.bias_act_bound(ref, t, SP.ACT_SIGMOID, dtype), dtype), []), what)
        z = pr.z.clone()
        ops.scale_rows(z, g2)
        want = round16(pr.z.double() * g2.double()[:, None, :], dtype, exact=False)
        # (a gate near 0 may carry the product into the subnormal range, where the fp32 product is still exact: equal values)
        judge(el, "se chain", "scale_rows=", (0.0 if bool((z.double() == want.double()).all()) else SP.INF, []), what)


# ---- the engine's own call -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[("bf16", 84), ("f16", 84), ("bf16", 98), ("f16", 98)], ids=lambda p: f"{p[0]}-grid{p[1] // 14}")
def stc_engine(request):
    """the tiny STC engine of test_gpu_stc.py (patch grid 6) and one on an odd grid (7); weights drawn per tensor name, so every block's differ"""
    element, image = request.param
    dtype = DTYPES[element]
    cfg = dataclasses.replace(tcfg.tiny(num_frames=4), mm_projector_type="stc_connector", vision_image_size=image, vision_hidden_size=256,
                              vision_num_heads=4, mm_hidden_size=256)
    sd = {k: v.to(dtype) for k, v in synth.iter_weights(cfg, device="cuda")}
    eng = TraceEngine(cfg, device=0, max_batch=1, max_ctx=256, max_frames=4, max_new_tokens=8, dtype=dtype)
    eng.load_weights(sd.items())
    stc = {k[len("model.mm_projector."):]: v for k, v in sd.items() if k.startswith("model.mm_projector.")}
    del sd
    yield SimpleNamespace(eng=eng, cfg=cfg, w=stc, el=element, dtype=dtype, G=image // 14)
    ops.use("bf16")
    eng.close()


def _block(w, q, x, N, hh, ww, H):
    """stc_block through ops: x [N hh ww, cin] -> [N hh ww, H]"""
    g = lambda k: w[q + k]
    HW, cin = hh * ww, x.shape[1]
    y = ops.gemm(x, g("conv1.conv.weight").reshape(H, cin))
    ops.layernorm_ex(y, g("conv1.bn.weight"), g("conv1.bn.bias"), 1e-6, out=y, silu=True)
    z = ops.dwconv3x3(y.view(N, hh, ww, H), g("conv2.conv.weight").reshape(H, 9)).view(N * HW, H)
    ops.layernorm_ex(z, g("conv2.bn.weight"), g("conv2.bn.bias"), 1e-6, out=z, silu=True)
    pool = ops.avgpool(z.view(N, HW, H))
    rd = g("se.fc1.weight").shape[0]
    g1 = ops.skinny_gemm(pool, g("se.fc1.weight").reshape(rd, H))
    ops.bias_act(g1, g("se.fc1.bias"), SP.ACT_SILU)
    g2 = ops.skinny_gemm(g1, g("se.fc2.weight").reshape(H, rd))
    ops.bias_act(g2, g("se.fc2.bias"), SP.ACT_SIGMOID)
    ops.scale_rows(z.view(N, HW, H), g2)
    y = ops.gemm(z, g("conv3.conv.weight").reshape(H, H))
    shortcut = x
    if q + "downsample.conv.weight" in w:                 # stage 1's block 0: the shortcut is a 1 x 1 convolution + LayerNorm, read at pitch cin
        shortcut = ops.gemm(x, g("downsample.conv.weight").reshape(H, cin))
        ops.layernorm_ex(shortcut, g("downsample.bn.weight"), g("downsample.bn.bias"), 1e-6, out=shortcut)
    return ops.layernorm_ex(y, g("conv3.bn.weight"), g("conv3.bn.bias"), 1e-6, out=shortcut, silu=True, res=shortcut)


def stc_through_ops(w, feats, T, G, H):
    """trace_stc_connector restated with `ops`: feats [T, G G, vh] -> [(T // 2 + 1)(G // 2 + 1)^2, H]"""
    x = feats.reshape(T * G * G, -1)
    for b in range(1, 5):
        x = _block(w, f"s1.b{b}.", x.clone() if b == 1 else x, T, G, G, H)
    col = ops.im2col3d(x.view(T, G, G, H))
    x = ops.gemm(col, ops.permute_conv3d_w(w["sampler.0.weight"]), bias=w["sampler.0.bias"])
    ops.bias_act(x, None, SP.ACT_SILU)
    To, Go = T // 2 + 1, G // 2 + 1
    for b in range(1, 5):
        x = _block(w, f"s2.b{b}.", x, To, Go, Go, H)
    y = ops.gemm(x, w["readout.0.weight"], bias=w["readout.0.bias"])
    ops.bias_act(y, None, SP.ACT_GELU)                    # nn.GELU(): the exact-erf form
    return ops.gemm(y, w["readout.2.weight"], bias=w["readout.2.bias"])


@pytest.mark.parametrize("T", [1, 3, 4])
def test_engine_stc_connector_is_the_ops(stc_engine, T):
    """eng.stc_connector(feats, T) == the same chain through `ops`, bit for bit: stage 1 (block 0 with the downsample shortcut and the pitch
    vh -> H), the Conv3d sampler at odd and even T and grid, stage 2, the GELU readout; (T // 2 + 1)(G // 2 + 1)^2 rows; a second call repeats the
    first exactly"""
    e = stc_engine
    ops.use(e.el)
    G, H, vh = e.G, e.cfg.hidden_size, e.cfg.vision_hidden_size
    assert e.cfg.vision_grid == G
    g = torch.Generator().manual_seed(17 + T + G)
    feats = torch.randn(T, G * G, vh, generator=g).to(e.dtype).to(DEV)
    got = e.eng.stc_connector(feats, T)
    again = e.eng.stc_connector(feats, T)
    assert got.shape == ((T // 2 + 1) * (G // 2 + 1) ** 2, H)
    assert bool(torch.isfinite(got).all()) and float(got.float().abs().max()) > 0
    assert torch.equal(got, again), "a second call differs from the first"
    want = stc_through_ops(e.w, feats, T, G, H)
    diff = int((got.view(torch.int16) != want.view(torch.int16)).sum())
    m = MARGINS.setdefault((e.el, "engine", f"grid {G} == ops"), [0.0, 0])
    m[1] += 1
    assert diff == 0, f"T {T} grid {G}: {diff} of {got.numel()} words differ from the chain through ops (max {float((got.float() - want.float()).abs().max()):.4g})"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffers_untouched(el):
    """every op answers TRACE_ERR_ARG (-1) for what its kernel cannot take — non-positive extents, C % 8 (C % 64 for the pool), an act outside 0..3,
    null tensors — before it launches anything"""
    dtype = DTYPES[el]
    bufs = [SP.sentinel_out((4096,), dtype, DEV)[0] for _ in range(3)]
    a, b, c = bufs

    def refused(name, call):
        with pytest.raises(_lib.TraceHipError, match=rf"error -1 in trace_op_{name}"):
            call()
        torch.cuda.synchronize()
        assert all(SP.sentinel_words(t) == t.numel() for t in bufs), f"trace_op_{name}: a refused call wrote"

    for dims in ((0, 2, 2, 8), (1, 0, 2, 8), (1, 2, 0, 8), (1, 2, 2, 12), (1, 2, 2, 0), (-1, 2, 2, 8)):
        refused("dwconv3x3", lambda: ops.dwconv3x3(a, b, out=c, dims=dims))
    for args in ((None, b), (a, None)):
        refused("dwconv3x3", lambda: ops.dwconv3x3(args[0], args[1], out=c, dims=(1, 2, 2, 8)))
    for dims in ((0, 4, 64), (1, 0, 64), (1, 4, 32), (1, 4, 96), (1, 4, 0), (65536, 1, 64)):
        refused("avgpool", lambda: ops.avgpool(a, out=c, dims=dims))
    refused("avgpool", lambda: ops.avgpool(None, out=c, dims=(1, 4, 64)))
    for dims, act in (((0, 8), 1), ((2, 12), 1), ((2, 0), 1), ((2, 8), -1), ((2, 8), 4)):
        refused("bias_act", lambda: ops.bias_act(a, b, act, dims=dims))
    refused("bias_act", lambda: ops.bias_act(None, b, 1, dims=(2, 8)))
    for dims in ((0, 4, 8), (2, 0, 8), (2, 4, 4), (2, 4, 0)):
        refused("scale_rows", lambda: ops.scale_rows(a, b, dims=dims))
    refused("scale_rows", lambda: ops.scale_rows(a, None, dims=(2, 4, 8)))
    for dims in ((0, 2, 2, 8), (2, 0, 2, 8), (2, 2, 0, 8), (2, 2, 2, 12), (2, 2, 2, 0)):
        refused("im2col3d", lambda: ops.im2col3d(a, out=c, dims=dims))
    refused("im2col3d", lambda: ops.im2col3d(None, out=c, dims=(2, 2, 2, 8)))
    for dims in ((0, 8), (8, 0), (-2, 8)):
        refused("permute_conv3d_w", lambda: ops.permute_conv3d_w(a, out=c, dims=dims))
    refused("permute_conv3d_w", lambda: ops.permute_conv3d_w(None, out=c, dims=(2, 8)))
