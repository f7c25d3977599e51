"""The STC row-kernel probes judged on the CPU (tests/stc_probes.py): the float64 references agree with torch's own operators, the arithmetic facts
the bounds rest on hold in both element types, the fault-free torch emulations of the six kernels pass every probe at every shape
tests/test_gpu_stc_probes.py runs (the shapes that take a second grid trip on the device are stood in for by small shapes under a lowered cap), and
every listed fault is rejected by the probe NAMED in the tables below."""
import pytest
import torch
import torch.nn.functional as F

import stc_probes as SP
from gemm_probes import P_BITS

BF, HF = torch.bfloat16, torch.float16
DTYPES = [BF, HF]
IDS = ["bf16", "f16"]


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---- the references against torch's operators -------------------------------------------------------------------------------------------------
def test_dwconv_reference_is_conv2d():
    for N, H, W, C in ((2, 3, 5, 24), (1, 1, 1, 8), (2, 7, 7, 72)):
        x, w = _randn(N, H, W, C, seed=1), _randn(C, 9, seed=2)
        ref, mag = SP.dwconv_reference(x, w)
        want = F.conv2d(x.permute(0, 3, 1, 2), w.view(C, 1, 3, 3), padding=1, groups=C).permute(0, 2, 3, 1)
        assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
        assert bool((mag >= ref.abs() - 1e-12).all())


@pytest.mark.parametrize("T,H,W", [(3, 5, 5), (4, 6, 6), (1, 1, 1), (2, 7, 4), (1, 2, 3)])
def test_im2col_and_permute_references_make_conv3d(T, H, W):
    """im2col_reference(x) @ permute_reference(w)^T + b == F.conv3d(stride 2, padding 1) exactly on integer data: the two references agree on the
    tap order, for odd and even extents"""
    C, Co = 8, 16
    x, w, b = SP.conv3d_probe(T, H, W, C, Co, BF)
    A, Wp = SP.im2col_reference(x), SP.permute_reference(w)
    got = A.double() @ Wp.double().t() + b.double()
    want = SP.conv3d_reference(x, w, b)
    assert got.shape == want.shape == ((T // 2 + 1) * (H // 2 + 1) * (W // 2 + 1), Co)
    assert torch.equal(got, want)
    assert float(want.abs().max()) < 2 ** 24


def test_activation_references():
    t = torch.cat([_randn(4096, seed=3) * 4, torch.tensor([0.0, 88.0, -88.0, 20.0, -20.0], dtype=torch.float64)])
    assert torch.allclose(SP.act64(t, SP.ACT_SILU), F.silu(t), rtol=1e-14, atol=0)
    assert torch.allclose(SP.act64(t, SP.ACT_SIGMOID), torch.sigmoid(t), rtol=1e-14, atol=0)
    g = SP.act64(t, SP.ACT_GELU)                # torch's own form cancels for negative t: 1 + erf is known to 2^-53 absolute there
    assert bool(((g - F.gelu(t)).abs() <= 1e-13 * g.abs() + 2.0 ** -52 * t.abs()).all())
    assert torch.equal(SP.act64(t, SP.ACT_NONE), t)
    assert float(SP.act64(torch.tensor([-20.0], dtype=torch.float64), SP.ACT_GELU)) < 0      # erfc keeps what 1 + erf loses
    x = _randn(3, 36, 64, seed=4)
    ref, ma = SP.avgpool_reference(x)
    assert torch.allclose(ref, x.mean(1)) and torch.allclose(ma, x.abs().mean(1))


# ---- the arithmetic facts the bounds rest on -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_products_of_16_bit_values_are_exact_in_fp32(dtype):
    """two p-bit significands: the product has at most 2 p <= 22 bits — fp32 holds it (dwconv's taps, scale_rows)"""
    a = (_randn(1 << 16, seed=5) * 3).to(dtype)
    b = (_randn(1 << 16, seed=6) * 3).to(dtype)
    full = torch.tensor([2.0 - 2.0 ** -(P_BITS[dtype] - 1)], dtype=torch.float64).to(dtype)       # every significand bit set
    a, b = torch.cat([a, full, full]), torch.cat([b, full, -full])
    pr = a.double() * b.double()
    assert torch.equal(pr.float().double(), pr)
    assert torch.equal((a.float() * b.float()).double(), pr)
    x, g = SP.scale_probe("ramp", 3, 7, 64, dtype)
    SP.scale_reference(x, g, dtype)                    # (asserts exactness itself)
    lo, hi = float((x.double() * g.double()[:, None]).abs().min()), float((x.double() * g.double()[:, None]).abs().max())
    assert 2.0 ** -6 <= lo and hi <= 2.0 ** 6, "scale_rows products stay clear of the 16-bit subnormal range"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_integer_probes_have_exact_sums(dtype):
    """every partial sum of the integer probes, in any order, is a multiple of 2^-8 whose count stays below 2^24"""
    for name in SP.DWCONV_EXACT:
        for shape in ((2, 7, 7, 72), (2, 13, 13, 256)):
            x, w = SP.dwconv_probe(name, *shape, dtype)
            ref, mag = SP.dwconv_reference(x, w)
            t = x.double()[..., None] * w.double()
            assert torch.equal(t * 256, (t * 256).round()) and float(mag.max()) * 256 < 2 ** 24
    for name in ("count", "cancel"):
        for HW in (1, 32, 576):
            x = SP.avgpool_probe(name, 3, HW, 64, dtype).double()
            assert torch.equal(x * 2, (x * 2).round()) and float(x.abs().sum(1).max()) * 2 < 2 ** 24
    assert SP.avgpool_is_exact("count", 32) and SP.avgpool_is_exact("cancel", 1) and not SP.avgpool_is_exact("count", 36) \
        and not SP.avgpool_is_exact("gauss", 32)
    for T, H, W in ((3, 5, 5), (4, 6, 6)):
        x, w, b = SP.conv3d_probe(T, H, W, 8, 128, dtype)
        assert float(x.abs().max()) * float(w.abs().max()) * 8 * 8 + float(b.abs().max()) < 2 ** 24, "the Conv3d chain's sums are exact integers"
        pre = SP.conv3d_reference(x, w, b)
        assert 20 < float(pre.abs().max()) <= 88, "inside the range the SiLU behind the sampler is judged on"
        assert float((w != 0).double().mean()) > 0.5 and bool((x != 0).all())


def test_probe_properties():
    for dtype in DTYPES:
        x = SP.dwconv_probe("delta", 3, 24, 24, 16, dtype)[0].double()
        assert bool((x != 0).all()) and float(x.abs().max()) <= 254
        flat = x[:, :, :, 0].reshape(-1)
        assert all(len(set(flat[i:i + 508].tolist())) == 508 for i in (0, 300, 1220)), "508 consecutive positions are distinct"
        w = SP.ident_words((5000,), dtype, "cpu")
        assert bool(torch.isfinite(w.float()).all()) and bool((w.float() > 0).all()) and len(set(w[:4093].view(torch.int16).tolist())) == 4093
        assert SP.sentinel_words(w) == 0
        b = SP.act_bias(1024, dtype).double()
        assert len(set(b.tolist())) == 1024 and float(b.abs().max()) < 4
    for HW in SP.AVGPOOL_HW:                      # the one-hot probe visits every pixel of every frame, the last one of a ragged tail included
        for C in (64, 192):
            hit = set()
            for s in SP.onehot_shifts(HW, C):
                hit |= {(c + s) % HW for c in range(C)}
            assert hit == set(range(HW))
    # the launches that take later trips on the device, and their stand-ins under a lowered cap
    N, H, W, C = SP.DWCONV_TWO_TRIPS
    assert SP.trips_of(N * H * W * C // 8) == 2 and SP.trips_of(2 * 13 * 13 * 4096 // 8) == 1
    assert SP.trips_of(SP.BIAS_ACT_TWO_TRIPS[0] * SP.BIAS_ACT_TWO_TRIPS[1] // 8) == 2
    N, HW, C = SP.SCALE_TWO_TRIPS
    assert SP.trips_of(N * HW * C // 8) == 2
    T, H, W, C = SP.IM2COL_TWO_TRIPS
    assert SP.trips_of((T // 2 + 1) * (H // 2 + 1) * (W // 2 + 1) * C) == 2
    assert SP.trips_of(SP.PERMUTE_TRIPS[0] * SP.PERMUTE_TRIPS[1] * 8) == 4
    assert SP.trips_of(16 * 24 * 24 * 4096 // 8) == 3, "16 frames: the row kernels take three trips"


# ---- the runners: an emulation behind the signature the GPU test gives the op -----------------------------------------------------------------
def dwconv_verdict(name, shape, dtype, fault=None, cap=SP.CAP):
    N, H, W, C = shape
    r, bad = SP.dwconv_case(name, N, H, W, C, dtype, "cpu",
                            lambda x, w, y: SP.emulate_dwconv(SP.with_guard(x), w, SP.with_guard(y), N, H, W, C, dtype, fault, cap))
    return r <= 1 and not bad, r


def avgpool_verdict(name, shape, dtype, fault=None, shift=0):
    N, HW, C = shape
    r, bad = SP.avgpool_case(name, N, HW, C, dtype, "cpu",
                             lambda x, y: SP.emulate_avgpool(SP.with_guard(x), SP.with_guard(y), N, HW, C, dtype, fault), shift)
    return r <= 1 and not bad, r


def bias_act_verdict(name, shape, act, with_bias, dtype, fault=None, cap=SP.CAP):
    rows, C = shape
    r, bad = SP.bias_act_case(name, rows, C, act, with_bias, dtype, "cpu",
                              lambda x, b, a: SP.emulate_bias_act(SP.with_guard(x), b, rows, C, a, dtype, fault, cap))
    return r <= 1 and not bad, r


def scale_verdict(name, shape, dtype, fault=None, cap=SP.CAP):
    N, HW, C = shape
    r, bad = SP.scale_case(name, N, HW, C, dtype, "cpu", lambda x, g: SP.emulate_scale_rows(SP.with_guard(x), g, N, HW, C, dtype, fault, cap))
    return r <= 1 and not bad, r


def im2col_verdict(shape, dtype, fault=None, cap=SP.CAP):
    T, H, W, C = shape
    r, bad = SP.im2col_case(T, H, W, C, dtype, "cpu", lambda x, A: SP.emulate_im2col3d(SP.with_guard(x), A, T, H, W, C, dtype, fault, cap))
    return r <= 1 and not bad, r


def permute_verdict(shape, dtype, fault=None, cap=SP.CAP):
    Co, Ci = shape
    r, bad = SP.permute_case(Co, Ci, dtype, "cpu", lambda w, o: SP.emulate_permute(SP.with_guard(w), SP.with_guard(o), Co, Ci, dtype, fault, cap))
    return r <= 1 and not bad, r


# ---- the fault-free emulations pass, at the GPU tests' shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dwconv_emulation_passes(dtype):
    for shape in SP.DWCONV_SHAPES + [(3, 4, 4, 256)]:
        for name in SP.DWCONV_PROBES:
            ok, r = dwconv_verdict(name, shape, dtype, cap=1 if shape == (3, 4, 4, 256) else SP.CAP)
            assert ok, (name, shape, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_avgpool_emulation_passes(dtype):
    for shape in SP.AVGPOOL_SHAPES:
        for name in SP.AVGPOOL_PROBES:
            for shift in (SP.onehot_shifts(shape[1], shape[2]) if name == "onehot" else (0,)):
                ok, r = avgpool_verdict(name, shape, dtype, shift=shift)
                assert ok, (name, shape, shift, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bias_act_emulation_passes(dtype):
    for rows in SP.BIAS_ACT_ROWS + (40,):
        for C in SP.BIAS_ACT_C:
            for act in SP.ACT_NAMES:
                for with_bias in (False, True):
                    for name in SP.BIAS_ACT_PROBES:
                        ok, r = bias_act_verdict(name, (rows, C), act, with_bias, dtype, cap=1 if rows == 40 else SP.CAP)
                        assert ok, (name, rows, C, SP.ACT_NAMES[act], with_bias, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_movers_and_scale_emulations_pass(dtype):
    for shape in SP.SCALE_SHAPES:
        for name in SP.SCALE_PROBES:
            ok, r = scale_verdict(name, shape, dtype, cap=1 if shape == (2, 36, 256) else SP.CAP)
            assert ok, (name, shape, r)
    for shape in SP.IM2COL_SHAPES:
        ok, r = im2col_verdict(shape, dtype, cap=1 if shape == (3, 7, 7, 64) else SP.CAP)
        assert ok, (shape, r)
    for shape in SP.PERMUTE_SHAPES:
        ok, r = permute_verdict(shape, dtype, cap=1)
        assert ok, (shape, r)


# ---- every fault is rejected by a named probe -----------------------------------------------------------------------------------------------
# fault -> (probe, shape[, extras]): the probe NAMED here must reject it.  cap = 1: a launch of one workgroup, so 256 items per trip.
DWCONV_REJECTS = {
    "taps_transposed": ("delta", (2, 7, 7, 72)),
    "taps_flipped": ("delta", (2, 7, 7, 72)),
    "wrap_row": ("delta", (2, 7, 7, 72)),
    "wrap_frame": ("delta", (2, 7, 7, 72)),
    "lost_tap": ("delta", (2, 7, 7, 72)),
    "weight_layout": ("delta", (2, 7, 7, 72)),
    "weight_chunk0": ("delta", (2, 7, 7, 72)),
    "second_trip_lost": ("count", (3, 4, 4, 256)),
}
AVGPOOL_REJECTS = {
    "ragged_pixels_lost": ("onehot", (3, 33, 64)),
    "divide_by_padded": ("onehot", (3, 33, 64)),
    "slab_shift": ("onehot", (32, 36, 192)),
    "frame_mix": ("onehot", (3, 36, 64)),
}
BIAS_ACT_REJECTS = {
    "act_swapped": ("grid", (17, 64), SP.ACT_SILU),
    "bias_skipped": ("grid", (17, 64), SP.ACT_SILU),
    "bias_chunk0": ("grid", (17, 64), SP.ACT_SIGMOID),
    "act_before_bias": ("grid", (17, 64), SP.ACT_SILU),
    "second_trip_lost": ("grid", (17, 256), SP.ACT_SILU),
}
SCALE_REJECTS = {
    "gate_frame0": ("ramp", (3, 7, 8)),
    "gate_frame_pow2": ("ramp", (3, 7, 8)),
    "second_trip_lost": ("ramp", (2, 36, 256)),
}
IM2COL_REJECTS = {
    "no_leading_pad": ("ident", (3, 5, 4, 8)),
    "tap_order": ("ident", (3, 5, 4, 8)),
    "trailing_clamped": ("ident", (2, 2, 2, 16)),
    "zeros_not_written": ("ident", (3, 5, 4, 8)),
    "second_trip_lost": ("ident", (3, 7, 7, 64)),
}
PERMUTE_REJECTS = {
    "co_ci_swapped": ("ident", (16, 8)),
    "tap_minor": ("ident", (16, 8)),
    "second_trip_lost": ("ident", (16, 8)),
}


def test_fault_lists_are_complete():
    assert set(DWCONV_REJECTS) == set(SP.DWCONV_FAULTS) and set(AVGPOOL_REJECTS) == set(SP.AVGPOOL_FAULTS)
    assert set(BIAS_ACT_REJECTS) == set(SP.BIAS_ACT_FAULTS) and set(SCALE_REJECTS) == set(SP.SCALE_FAULTS)
    assert set(IM2COL_REJECTS) == set(SP.IM2COL_FAULTS) and set(PERMUTE_REJECTS) == set(SP.PERMUTE_FAULTS)
    gpu = SP.DWCONV_SHAPES + SP.AVGPOOL_SHAPES + [(r, c) for r in SP.BIAS_ACT_ROWS for c in SP.BIAS_ACT_C] + SP.SCALE_SHAPES + SP.IM2COL_SHAPES \
        + SP.PERMUTE_SHAPES
    for table in (DWCONV_REJECTS, AVGPOOL_REJECTS, BIAS_ACT_REJECTS, SCALE_REJECTS, IM2COL_REJECTS, PERMUTE_REJECTS):
        for fault, row in table.items():
            assert row[1] in gpu, f"{fault}: the rejecting shape is one the GPU test runs"


def _show(fault, probe, r0, r):
    print(f"{fault:<22} {probe:<8} fault-free {r0:.3f}  with the fault {r:.3g}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", SP.DWCONV_FAULTS)
def test_dwconv_fault_is_rejected(dtype, fault):
    probe, shape = DWCONV_REJECTS[fault]
    ok0, r0 = dwconv_verdict(probe, shape, dtype, None, 1)
    ok, r = dwconv_verdict(probe, shape, dtype, fault, 1)
    _show(fault, probe, r0, r)
    assert ok0 and not ok


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", SP.AVGPOOL_FAULTS)
def test_avgpool_fault_is_rejected(dtype, fault):
    probe, shape = AVGPOOL_REJECTS[fault]
    shifts = SP.onehot_shifts(shape[1], shape[2])
    v0 = [avgpool_verdict(probe, shape, dtype, None, s) for s in shifts]
    v = [avgpool_verdict(probe, shape, dtype, fault, s) for s in shifts]
    _show(fault, probe, max(r for _, r in v0), max(r for _, r in v))
    assert all(ok for ok, _ in v0) and not all(ok for ok, _ in v)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", SP.BIAS_ACT_FAULTS)
def test_bias_act_fault_is_rejected(dtype, fault):
    probe, shape, act = BIAS_ACT_REJECTS[fault]
    ok0, r0 = bias_act_verdict(probe, shape, act, True, dtype, None, 1)
    ok, r = bias_act_verdict(probe, shape, act, True, dtype, fault, 1)
    _show(fault, probe, r0, r)
    assert ok0 and not ok


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", SP.SCALE_FAULTS)
def test_scale_rows_fault_is_rejected(dtype, fault):
    probe, shape = SCALE_REJECTS[fault]
    ok0, r0 = scale_verdict(probe, shape, dtype, None, 1)
    ok, r = scale_verdict(probe, shape, dtype, fault, 1)
    _show(fault, probe, r0, r)
    assert ok0 and not ok


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", SP.IM2COL_FAULTS)
def test_im2col3d_fault_is_rejected(dtype, fault):
    probe, shape = IM2COL_REJECTS[fault]
    ok0, r0 = im2col_verdict(shape, dtype, None, 1)
    ok, r = im2col_verdict(shape, dtype, fault, 1)
    _show(fault, probe, r0, r)
    assert ok0 and not ok


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", SP.PERMUTE_FAULTS)
def test_permute_fault_is_rejected(dtype, fault):
    probe, shape = PERMUTE_REJECTS[fault]
    ok0, r0 = permute_verdict(shape, dtype, None, 1)
    ok, r = permute_verdict(shape, dtype, fault, 1)
    _show(fault, probe, r0, r)
    assert ok0 and not ok


@pytest.mark.parametrize("element", IDS)
def test_ops_refuse_before_any_launch(element):
    """the six trace_op_* entries answer TRACE_ERR_ARG from their argument checks alone — no HIP call is reached, so this runs without a device (the
    pointers are host words that a refused call must not touch)"""
    import ctypes as C
    from trace_amd import _lib, build
    build.build()
    lib = _lib.load(element)
    words = (C.c_uint16 * 64)(*([SP.SENTINEL] * 64))
    p = C.c_void_p(C.addressof(words))
    calls = [("dwconv3x3", lambda d: lib.trace_op_dwconv3x3(p, p, p, *d, None), [(0, 2, 2, 8), (1, 0, 2, 8), (1, 2, 0, 8), (1, 2, 2, 12), (1, 2, 2, 0)]),
             ("avgpool", lambda d: lib.trace_op_avgpool(p, p, *d, None), [(0, 4, 64), (1, 0, 64), (1, 4, 32), (1, 4, 96), (1, 4, 0), (65536, 4, 64)]),
             ("bias_act", lambda d: lib.trace_op_bias_act(p, p, *d, None), [(0, 8, 1), (2, 12, 1), (2, 0, 1), (2, 8, -1), (2, 8, 4)]),
             ("scale_rows", lambda d: lib.trace_op_scale_rows(p, p, *d, None), [(0, 4, 8), (2, 0, 8), (2, 4, 4), (2, 4, 0)]),
             ("im2col3d", lambda d: lib.trace_op_im2col3d(p, p, *d, None), [(0, 2, 2, 8), (2, 0, 2, 8), (2, 2, 0, 8), (2, 2, 2, 12)]),
             ("permute_conv3d_w", lambda d: lib.trace_op_permute_conv3d_w(p, p, *d, None), [(0, 8), (8, 0)])]
    for name, call, cases in calls:
        for d in cases:
            with pytest.raises(_lib.TraceHipError, match=rf"error -1 in trace_op_{name}"):
                call(d)
    for name, call in (("dwconv3x3", lambda: lib.trace_op_dwconv3x3(p, None, p, 1, 2, 2, 8, None)), ("avgpool", lambda: lib.trace_op_avgpool(None, p, 1, 4, 64, None)),
                       ("bias_act", lambda: lib.trace_op_bias_act(None, p, 2, 8, 1, None)), ("scale_rows", lambda: lib.trace_op_scale_rows(p, None, 2, 4, 8, None)),
                       ("im2col3d", lambda: lib.trace_op_im2col3d(p, None, 2, 2, 2, 8, None)),
                       ("permute_conv3d_w", lambda: lib.trace_op_permute_conv3d_w(None, p, 2, 8, None))):
        with pytest.raises(_lib.TraceHipError, match=rf"error -1 in trace_op_{name}: null argument"):
            call()
    assert all(w == SP.SENTINEL for w in words)


def test_a_lost_tap_pixel_or_zero_fails_the_other_probes_too():
    """what the issue's last criterion names — one tap, one ragged pixel, one trailing zero, the second trip — against the probes beside the named one"""
    for dtype in DTYPES:
        assert not dwconv_verdict("count", (2, 7, 7, 72), dtype, "lost_tap")[0]
        assert not dwconv_verdict("cancel", (2, 7, 7, 72), dtype, "lost_tap")[0]
        assert not dwconv_verdict("gauss", (2, 7, 7, 72), dtype, "lost_tap")[0]
        assert not avgpool_verdict("count", (3, 33, 64), dtype, "ragged_pixels_lost")[0]
        assert not avgpool_verdict("gauss", (3, 33, 64), dtype, "ragged_pixels_lost")[0]
        assert not im2col_verdict((4, 6, 6, 256), dtype, "trailing_clamped")[0]
        assert im2col_verdict((3, 7, 7, 64), dtype, "trailing_clamped")[0], "odd extents have no trailing zero to lose"
