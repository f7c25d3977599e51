"""The encode-side probes judged on the CPU (tests/encode_probes.py): the float64 references agree with the oracle, the fault-free torch emulations of
the three kernels pass the judge on every probe and shape tests/test_gpu_encode_probes.py runs, every listed fault is rejected by a named probe,
and a table states which of those faults the present Gaussian checks accept (test_gpu_kernels.py::test_norms' check(.., 2e-2, 1e-2) and
test_gpu_parity.report at 3e-2 with its 0.2 % allowance)."""
import pytest
import torch

import encode_probes as EP
from gemm_probes import small_residual
from oracle import trace_oracle as O
from trace_amd import config as tcfg, synth

BF, HF = torch.bfloat16, torch.float16
DTYPES = [BF, HF]
IDS = ["bf16", "f16"]


# ---- the references against the oracle --------------------------------------------------------------------------------------------------------
def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_ln_reference_is_the_oracles():
    x, w, b = _randn(7, 520, seed=1) * 2, 1 + 0.1 * _randn(520, seed=2), 0.1 * _randn(520, seed=3)
    for eps in (1e-5, 1e-6):
        ln, mag = EP._ln64(x.double(), w.double(), b.double(), eps)
        assert torch.allclose(O.Oracle._ln(x, w, b, eps).double(), ln, rtol=1e-5, atol=1e-5)
        assert bool((mag >= ln.abs() - 1e-12).all())
    sc, _ = EP._ln64(x.double(), w.double(), None, 1e-5, rms=True)
    assert torch.allclose((x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * w).double(), sc, rtol=1e-5, atol=1e-5)


def _tiny_cfg():
    cfg = tcfg.tiny(num_frames=3)
    cfg.vision_num_layers = 1                     # hidden_states[-2] is the front end's output: no encoder layer runs
    assert cfg.vision_layers_used == 0
    return cfg


def test_slot_reference_is_the_oracles_slot_pool():
    """Oracle.slot_pool with readout = [I; 0] returns `res` in its first v_hidden columns; the reference without the logit rounding is the same
    module in float64, with the engine's tables"""
    cfg = _tiny_cfg()
    sd = dict(synth.state_dict(cfg))
    vh, H, n = cfg.vision_hidden_size, cfg.hidden_size, cfg.vision_patches
    ro = torch.zeros((H, vh))
    ro[:vh] = torch.eye(vh)
    sd["model.mm_projector.readout.weight"] = ro
    feats = _randn(3, n, vh, seed=5)
    got = O.Oracle(cfg, sd).slot_pool(feats)[:, :, :vh]
    cos_t, sin_t = EP.rope_tables(n, vh, cfg.slot_rope_base)
    R = EP.slot_reference(feats, sd["model.mm_projector.ln_vision.weight"], sd["model.mm_projector.ln_vision.bias"], sd["model.mm_projector.slots"],
                          cos_t, sin_t, cfg.slot_ln_eps, BF, logit_rounding=False)
    assert torch.allclose(got.double(), R.ref, rtol=1e-4, atol=1e-5), float((got.double() - R.ref).abs().max())
    assert torch.allclose(R.p.sum(1), torch.ones(3, 8, dtype=torch.float64))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_frontend_reference_is_the_oracles_front_end(dtype):
    """Oracle.vit_forward with no encoder layer, rounding where the engine stores: the same rounding points in fp32.  A value of the oracle's that sits
    within fp32 noise of a 16-bit tie may round the other way, so: all but 0.1 % of the elements inside the judge's bound, and every one within what one
    flipped intermediate moves a row by (2 ulps of the row's largest scaled value)."""
    cfg = _tiny_cfg()
    sd = dict(synth.state_dict(cfg))
    frames = synth.synth_frames(cfg, 0).to(dtype)
    got = O.Oracle(cfg, sd, emulate_bf16=True if dtype == BF else dtype).vit_forward(frames.float())
    g = lambda k: sd[synth.VIS + k].to(dtype)
    vh, P = cfg.vision_hidden_size, cfg.vision_patch_size
    R = EP.frontend_reference(frames, g("embeddings.patch_embedding.weight").reshape(vh, -1), g("embeddings.class_embedding"),
                              g("embeddings.position_embedding.weight"), g("pre_layrnorm.weight"), g("pre_layrnorm.bias"), P,
                              cfg.vision_layer_norm_eps, dtype)
    ref = R.ref[:, 1:]
    r = ((got.double() - ref).abs() / R.bounds[0][:, 1:])
    assert float((r > 1).double().mean()) < 1e-3
    _, mag = EP._ln64(R.pre, g("pre_layrnorm.weight").double(), g("pre_layrnorm.bias").double(), cfg.vision_layer_norm_eps)
    assert bool(((got.double() - ref).abs() <= 2.0 ** -(EP.P_BITS[dtype] - 2) * mag[:, 1:].amax(-1, keepdim=True)).all())


# ---- the probes' own properties -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_probe_properties(dtype):
    for D in (8, 520, 1024):
        for ratio in EP.OFFSET_RATIOS:
            x, real = EP.offset_rows(5, D, dtype, ratio)
            xd = x.double()
            if ratio:
                assert bool((xd.sum(-1) == D * EP.OFFSET_M).all()), "the row sum is D m exactly"
                got = float(EP.OFFSET_M / xd.std(-1, unbiased=False)[0])
                assert abs(got / real - 1) < 1e-9 and 0.8 < real / ratio < 1.25, (ratio, real, got)
        w, b = EP.ramp_weights(D, dtype)
        assert len({(float(a), float(c)) for a, c in zip(w, b)}) == D
    # the one place the judge accepts an interval instead of a point: SiLU / residual references whose LN output cancels so far that the 2^-15
    # slack spans more than two neighbouring 16-bit values.  How many elements take it, per probe; each of them has |LN| < (|scaled| + |bias|) / 8
    for name in EP.NORM_PROBES:
        for ratio in (EP.OFFSET_RATIOS if name == "offset" else (0,)):
            cnt = tot = 0
            for D in (8, 128, 520, 1024, 4096):
                x = EP.norm_rows(name, 5, D, dtype, ratio=ratio)
                w, b = EP.ramp_weights(D, dtype)
                ln, mag = EP._ln64(x.double(), w.double(), b.double(), 1e-6)
                for res in (None, small_residual(5, D).to(dtype), EP.cancel_residual(x, w, b, 1e-6, dtype)):
                    R = EP.norm_reference(x, w, b, 1e-6, dtype, False, True, res)
                    assert bool((ln.abs()[R.wide] < mag[R.wide] / 8).all())
                    cnt, tot = cnt + int(R.wide.sum()), tot + R.wide.numel()
            print(f"wide references, {name}{'/' + str(ratio) if name == 'offset' else ''}: {cnt} of {tot} elements ({cnt / tot:.2%})")
            assert cnt / tot < (0.08 if dtype == HF else 0.01), (name, ratio, cnt, tot)
    assert EP.slot_targets(576)[:3] == [0, 71, 67] and 575 in EP.slot_targets(576) and EP.slot_targets(1) == [0]
    for P, D in ((14, 128), (16, 128), (14, 1024)):
        K = 3 * P * P
        ks = {(n + s) % K for s in EP.pointer_shifts(D, P) for n in range(D)}
        assert ks == set(range(K)), "the pointer shifts cover every k"
    pr = EP.frontend_probe("pointer", 2, 56, 14, 128, dtype)
    R = EP.frontend_probe_reference(pr)
    assert bool((R.pre == R.pre.round()).all()) and float(R.pre.abs().max()) <= 16, "integer rows before the LN"


# ---- fault-free emulations pass, at the GPU tests' shapes -------------------------------------------------------------------------------------
def norm_verdict(name, rows, D, dtype, fault=None, ratio=0, rms=False, eps=1e-5, form="plain", pads=(64, 8)):
    """(passes, error / bound): one norm probe through the emulation.  form: plain | inplace | silu | res | res_silu | cancel | cancel_silu (res: y == res)"""
    x = EP.norm_rows(name, rows, D, dtype, ratio=ratio)
    w, b = EP.ramp_weights(D, dtype)
    silu = form.endswith("silu")
    res = None
    if form.startswith("res"):
        res = small_residual(rows, D).to(dtype)
    elif form.startswith("cancel"):
        res = EP.cancel_residual(x, w, b, eps, dtype)
    R = EP.norm_reference(x, w, b, eps, dtype, rms, silu, res)
    xb, xv, ldx = EP.lay_rows(x, pads[0], dtype, EP.POISON)
    if form == "inplace":
        yb, yv, ldy = xb, xv, ldx
    elif res is not None:
        yb, yv, ldy = EP.lay_rows(res, pads[1], dtype, "sentinel")
    else:
        yb, yv, ldy = EP.lay_rows(torch.zeros_like(x), pads[1], dtype, "sentinel")
    snap = yb.clone()
    EP.emulate_norm(xb, ldx, yb, ldy, w, b, rows, D, eps, dtype, rms, silu, yb if res is not None else None, ldy, fault)
    r = EP.error_ratio(yv, R)
    return r <= 1.0 and EP.outside_unchanged(yb, snap, ldy, rows, D), r


NORM_FORMS = ("plain", "inplace", "silu", "res", "res_silu", "cancel", "cancel_silu")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [8, 128, 520, 1024, 4096])
def test_norm_emulation_passes(dtype, D):
    for rows in (1, 3, 4, 5):
        for name in EP.NORM_PROBES:
            for ratio in (EP.OFFSET_RATIOS if name == "offset" else (0,)):
                for rms in (False, True):
                    for eps in (1e-5, 1e-6):
                        for form in (("plain", "inplace") if rms or rows in (1, 4) else NORM_FORMS):
                            ok, r = norm_verdict(name, rows, D, dtype, None, ratio, rms, eps, form)
                            assert ok, (name, ratio, rows, D, rms, eps, form, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("rows", [4095, 4096, 4097, 4111])
def test_norm_emulation_passes_at_the_1024_switch(dtype, rows):
    for name, ratio in (("onehot", 0), ("ramp", 0), ("eps", 0), ("offset", 256)):
        for rms in (False, True):
            for eps in ((1e-5, 1e-6) if name == "eps" else (1e-5,)):
                for form in (NORM_FORMS if name == "ramp" and not rms else ("plain", "inplace")):
                    ok, r = norm_verdict(name, rows, 1024, dtype, None, ratio, rms, 1e-6 if form not in ("plain", "inplace") else eps, form)
                    assert ok, (name, rows, rms, eps, form, r)


SLOT_CASES = [("uniform", 0, None), ("pointer", 0, None), ("pointer", 0, "padded"), ("ramp", 0, None), ("rope", 0, None), ("eps", 0, None),
              ("frames", 0, None), ("offset", 0, None), ("offset", 4, None), ("offset", 32, None)]


def slot_verdict(name, T, n, D, dtype, fault=None, ratio=0, layout=None):
    pr = EP.slot_probe(name, T, n, D, dtype, ratio=ratio, layout=layout)
    r = EP.error_ratio(EP.emulate_slot_pool(pr, fault), EP.slot_probe_reference(pr))
    return r <= 1.0, r


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("D", [16, 128, 1024])
def test_slot_pool_emulation_passes(dtype, D):
    for n in (1, 7, 8, 9, 16, 37, 576, 577, 729):
        for T in (1, 3):
            for name, ratio, layout in SLOT_CASES:
                ok, r = slot_verdict(name, T, n, D, dtype, None, ratio, layout)
                assert ok, (name, ratio, layout, T, n, D, r)


def frontend_verdict(name, T, S, P, D, dtype, fault=None, shift=0, fp32=False):
    pr = EP.frontend_probe(name, T, S, P, D, dtype, shift=shift)
    if fp32 and name != "round":
        pr.frames = pr.frames.float()
    R = EP.frontend_probe_reference(pr)
    X = EP.emulate_frontend(pr, fault)
    NT = pr.G * pr.G + 1
    got = X[:T * NT].view(T, NT, D)
    r = EP.frontend_ratio(got, R, pr)
    intact = bool((X[T * NT:].view(torch.int16) == EP.SENTINEL).all())
    return r <= 1.0 and intact and EP.nan_rows_ok(got, pr), r


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,S", [(14, 14), (14, 56), (14, 112), (14, 126), (14, 336), (16, 16), (16, 144), (16, 336)])
def test_frontend_emulation_passes(dtype, P, S):
    for D in (128, 1024) + ((256,) if (P, S) == (14, 126) else ()) + ((512,) if (P, S) == (16, 144) else ()):
        for T in (1, 3):
            for name in EP.FRONTEND_PROBES:
                for shift in (EP.pointer_shifts(D, P) if name == "pointer" else (0,)):
                    for fp32 in ((True,) if name == "round" else (False, True)):
                        ok, r = frontend_verdict(name, T, S, P, D, dtype, None, shift, fp32)
                        assert ok, (name, T, S, P, D, shift, fp32, r)


# ---- every fault is rejected by a named probe -----------------------------------------------------------------------------------------------
# fault -> (probe, kwargs of norm_verdict): the probe NAMED here must reject it
NORM_REJECTS = {
    "eps_dropped": ("eps", dict(rows=3, D=128, eps=1e-6)),
    "mean_count": ("onehot", dict(rows=3, D=520)),
    "tail_rows_written": ("ramp", dict(rows=4097, D=1024)),
    "tail_neighbour_stats": ("balanced", dict(rows=4111, D=1024)),
    "chunk_shift64": ("ramp", dict(rows=3, D=1024)),
    "ldx_ignored": ("onehot", dict(rows=3, D=128)),
    "ldy_ignored": ("ramp", dict(rows=3, D=128)),
    "silu_before_round": ("ramp", dict(rows=5, D=520, form="silu", eps=1e-6)),
    "res_before_round": ("ramp", dict(rows=5, D=520, form="cancel", eps=1e-6)),
    "res_after_store": ("onehot", dict(rows=3, D=128, form="res", eps=1e-6)),
}
SLOT_REJECTS = {
    "part_drops_last_row": ("uniform", dict(T=1, n=37, D=128)),
    "clamped_row_counted": ("uniform", dict(T=1, n=37, D=128)),
    "empty_part_contributes": ("uniform", dict(T=1, n=9, D=128)),
    "merge_no_rescale": ("ramp", dict(T=1, n=37, D=128)),
    "merge_other_den": ("ramp", dict(T=1, n=37, D=128)),
    "softmax_over_slots": ("pointer", dict(T=1, n=37, D=128)),
    "rope_adjacent_pairs": ("rope", dict(T=1, n=37, D=128)),
    "sin_sign": ("rope", dict(T=1, n=37, D=128)),
    "position_off_by_one": ("rope", dict(T=1, n=37, D=128)),
    "eps_dropped": ("eps", dict(T=1, n=16, D=128)),
    "eps_1e-5": ("eps", dict(T=1, n=16, D=128)),
    "idle_lanes_contribute": ("offset", dict(T=1, n=16, D=128, ratio=4)),
    "row_stride_ignored": ("pointer", dict(T=1, n=16, D=128, layout="padded")),
    "frame_stride_ignored": ("frames", dict(T=3, n=16, D=128)),
    "ln_second_half_from_first": ("uniform", dict(T=1, n=16, D=128)),
}
FRONTEND_REJECTS = {
    "pad_as_pixel": ("count", dict(T=1, S=56, P=14, D=128)),
    "pad_pixel_not_zeroed": ("poison", dict(T=3, S=56, P=14, D=128)),
    "window_not_shifted": ("pointer", dict(T=1, S=56, P=14, D=128, shift=0)),
    "ky_j_swapped": ("pointer", dict(T=1, S=56, P=14, D=128, shift=0)),
    "channel_stride": ("pointer", dict(T=1, S=56, P=14, D=128, shift=256)),
    "last_wg_stores_all_rows": ("pos", dict(T=3, S=126, P=14, D=128)),
    "duplicate_row_stored": ("pos", dict(T=3, S=126, P=14, D=128)),
    "pos_row0_for_patch0": ("pos", dict(T=1, S=56, P=14, D=128)),
    "cls_no_ln": ("pos", dict(T=1, S=56, P=14, D=128)),
    "fp32_truncates": ("round", dict(T=1, S=56, P=14, D=128)),
}


def test_fault_lists_are_complete():
    assert set(NORM_REJECTS) == set(EP.NORM_FAULTS) and set(SLOT_REJECTS) == set(EP.SLOT_FAULTS) and set(FRONTEND_REJECTS) == set(EP.FRONTEND_FAULTS)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", EP.NORM_FAULTS)
def test_norm_fault_is_rejected(dtype, fault):
    probe, kw = NORM_REJECTS[fault]
    kw = dict(kw)
    rows, D = kw.pop("rows"), kw.pop("D")
    ok0, r0 = norm_verdict(probe, rows, D, dtype, None, **kw)
    ok, r = norm_verdict(probe, rows, D, dtype, fault, **kw)
    print(f"{fault:<24} {probe:<9} fault-free {r0:.3f}  with the fault {r:.3g}")
    assert ok0 and not ok


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", EP.SLOT_FAULTS)
def test_slot_pool_fault_is_rejected(dtype, fault):
    probe, kw = SLOT_REJECTS[fault]
    ok0, r0 = slot_verdict(probe, dtype=dtype, fault=None, **kw)
    ok, r = slot_verdict(probe, dtype=dtype, fault=fault, **kw)
    print(f"{fault:<26} {probe:<8} fault-free {r0:.3f}  with the fault {r:.3g}")
    assert ok0 and not ok


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault", EP.FRONTEND_FAULTS)
def test_frontend_fault_is_rejected(dtype, fault):
    probe, kw = FRONTEND_REJECTS[fault]
    ok0, r0 = frontend_verdict(probe, dtype=dtype, fault=None, **kw)
    ok, r = frontend_verdict(probe, dtype=dtype, fault=fault, **kw)
    print(f"{fault:<26} {probe:<8} fault-free {r0:.3f}  with the fault {r:.3g}")
    assert ok0 and not ok


# ---- what the present Gaussian checks accept --------------------------------------------------------------------------------------------------
def gaussian_check(got, ref, atol, rtol):
    """test_gpu_kernels.check"""
    got, ref = got.float(), ref.float()
    return bool(((got - ref).abs() <= atol + rtol * ref.abs()).all()) and bool(torch.isfinite(got).all())


def gaussian_report(got, ref, atol=3e-2, rtol=3e-2):
    """test_gpu_parity.report: 0.2 % of the elements may be off, none by more than 20 x the tolerance at the largest reference value"""
    got, ref = got.float(), ref.float()
    err = (got - ref).abs()
    frac = float((err > atol + rtol * ref.abs()).float().mean())
    return bool(torch.isfinite(got).all()) and frac < 2e-3 and float(err.max()) < 20 * (atol + rtol * float(ref.abs().max()))


def norms_gaussian_accepts(fault):
    """test_norms as it stands: N(0, 4) rows, contiguous, eps 1e-5, no SiLU, no residual, the output tensor exactly rows x D"""
    for rows, D in ((5, 128), (577, 1024), (33, 4096), (4618, 1024)):
        x, w, b = (_randn(rows, D, seed=rows) * 2).to(BF), (1 + 0.1 * _randn(D, seed=D)).to(BF), (0.1 * _randn(D, seed=D + 1)).to(BF)
        for rms in (False, True):
            xb, _, _ = EP.lay_rows(x, 0, BF, 0.0)
            yb, yv, _ = EP.lay_rows(torch.zeros_like(x), 0, BF, 0.0)
            EP.emulate_norm(xb, D, yb, D, w, b, rows, D, 1e-5, BF, rms, fault=fault)
            xf = x.float()
            ref = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5) * w.float()) if rms else \
                torch.nn.functional.layer_norm(xf, (D,), w.float(), b.float(), 1e-5)
            if not gaussian_check(yv, ref, 2e-2, 1e-2):
                return False
    return True


def slot_gaussian_accepts(fault):
    """test_gpu_parity.test_slot_pool as it stands: the tiny geometry (16 patches, D = 128, 4 frames), Gaussian features, contiguous"""
    T, n, D = 4, 16, 128
    x = _randn(T, n, D, seed=9).to(BF)
    w, b, sl = (1 + 0.1 * _randn(D, seed=10)).to(BF), (0.02 * _randn(D, seed=11)).to(BF), _randn(D, 8, seed=12).to(BF)
    cos_t, sin_t = EP.rope_tables(n, D)
    buf, v = EP.lay_feats(x, "plain", BF)
    pr = EP.SimpleNamespace(feats=v, buf=buf, ln_w=w, ln_b=b, slots=sl, cos_t=cos_t, sin_t=sin_t, eps=1e-6, dtype=BF, T=T, n=n, D=D)
    ref = EP.slot_reference(v, w, b, sl, cos_t, sin_t, 1e-6, BF).ref
    return gaussian_report(EP.emulate_slot_pool(pr, fault), ref)


def frontend_gaussian_accepts(fault):
    """the front end is only ever seen through an encoder layer; read in its favour, report() is applied to the front end's own output here: the tiny
    geometry (4 x 4 patches of 14, D = 128), Gaussian pixels and N(0, 0.02^2) weights, 16-bit frames (fp32 frames for the fp32 fault)"""
    T, S, P, D = 4, 56, 14, 128
    f = _randn(T, 3, S, S, seed=20)
    pr = EP.SimpleNamespace(frames=f if fault == "fp32_truncates" else f.to(BF), W=(0.02 * _randn(D, 3 * P * P, seed=21)).to(BF),
                            cls=(0.02 * _randn(D, seed=22)).to(BF), pos=(0.02 * _randn(17, D, seed=23)).to(BF), lw=(1 + 0.1 * _randn(D, seed=24)).to(BF),
                            lb=(0.02 * _randn(D, seed=25)).to(BF), eps=1e-5, P=P, T=T, S=S, D=D, G=4, dtype=BF)
    ref = EP.frontend_reference(pr.frames, pr.W, pr.cls, pr.pos, pr.lw, pr.lb, P, 1e-5, BF).ref
    X = EP.emulate_frontend(pr, fault)
    return gaussian_report(X[:T * 17].view(T, 17, D), ref)


# the faults the Gaussian checks let through (the probes above reject every one of them)
GAUSSIAN_ACCEPTS = {
    "norms": {"eps_dropped", "tail_rows_written", "ldx_ignored", "ldy_ignored", "silu_before_round", "res_before_round", "res_after_store"},
    "slot pool": {"clamped_row_counted", "empty_part_contributes", "eps_dropped", "eps_1e-5", "row_stride_ignored", "frame_stride_ignored"},
    "front end": {"pad_pixel_not_zeroed", "fp32_truncates"},
}


def test_what_the_gaussian_checks_accept():
    table = {"norms": {f for f in EP.NORM_FAULTS if norms_gaussian_accepts(f)},
             "slot pool": {f for f in EP.SLOT_FAULTS if slot_gaussian_accepts(f)},
             "front end": {f for f in EP.FRONTEND_FAULTS if frontend_gaussian_accepts(f)}}
    assert norms_gaussian_accepts(None) and slot_gaussian_accepts(None) and frontend_gaussian_accepts(None)
    for k, faults in (("norms", EP.NORM_FAULTS), ("slot pool", EP.SLOT_FAULTS), ("front end", EP.FRONTEND_FAULTS)):
        for f in faults:
            print(f"{k:<10} {f:<28} {'ACCEPTED' if f in table[k] else 'rejected'} by the Gaussian check")
    assert table == GAUSSIAN_ACCEPTS, table
