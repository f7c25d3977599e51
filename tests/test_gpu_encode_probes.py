"""The encode-side kernels against float64 (tests/encode_probes.py; tests/test_encode_probes_cpu.py shows on the CPU which faults these probes reject
and which of them the Gaussian checks of test_gpu_kernels.py / test_gpu_parity.py let through): norm_kernel / norm1024_kernel with every stride,
in-place, SiLU and residual form the engine uses; slot_pool_part_kernel / slot_pool_merge_kernel at patch counts that leave empty, one-row and
ragged parts; patch_pack_kernel / cls_row_kernel / patch_embed_kernel at both patch sizes with one, several and a ragged last workgroup per frame;
and the engine's own calls of them (one tiny engine with crafted weights).

One judge (encode_probes.bound): half a 16-bit ulp of the float64 value + 2^-15 (|scaled term| + |bias|) [+ 2 E for the slot pool].  The largest
error / bound per kernel and probe is printed and appended to the file the environment variable TRACE_ENCODE_PROBE_MARGINS names
(profiles/encode_probe_margins.txt is made from it).  Both libraries (bf16 and fp16 elements) run everything."""
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import encode_probes as EP  # noqa: E402
from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402

DEV = torch.device("cuda", 0)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
MARGINS = {}                      # (library, kernel, probe) -> [max err / bound, cases]
RECORDED = {}                     # the same for what is measured and not asserted (slot pool, offset at ratio 256)
EPS_SET = (1e-5, 1e-6)            # CLIP; slot pool / STC; (the config's RMS eps is 1e-5 as well)


@pytest.fixture(scope="module", autouse=True)
def margins_record():
    yield
    lines = [f"{lib:<5} {k:<12} {p:<30} max err/bound {m[0]:.3f}  cases {m[1]}" for (lib, k, p), m in sorted(MARGINS.items())]
    lines += [f"{lib:<5} {k:<12} {p:<30} max err/bound {m[0]:.3f}  cases {m[1]}  (recorded, not asserted)" for (lib, k, p), m in sorted(RECORDED.items())]
    print("\n".join(lines))
    path = os.environ.get("TRACE_ENCODE_PROBE_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(params=["bf16", "f16"])
def el(request):
    ops.use(request.param)
    yield request.param
    ops.use("bf16")


def judge(el, kernel, probe, ratio, what, table=MARGINS, detail=None):
    m = table.setdefault((el, kernel, probe), [0.0, 0])
    m[0], m[1] = max(m[0], ratio), m[1] + 1
    if table is MARGINS:
        assert ratio <= 1.0, f"{kernel} {probe} {what}: error / bound {ratio:.3f}" + (f"\n{detail()}" if detail else "")


# ---- norms ----------------------------------------------------------------------------------------------------------------------------------
def norm_case(el, name, rows, D, dtype, ratio=0, kinds=(False, True), eps_set=EPS_SET, forms=True):
    """one probe through LayerNorm and RMSNorm: contiguous and padded (poison between the input rows, sentinel between the output rows), and for
    the LayerNorm in place (y == x), SiLU, residual with y == res, residual + SiLU"""
    x = EP.norm_rows(name, rows, D, dtype, DEV, ratio)
    w, b = EP.ramp_weights(D, dtype, DEV)
    tag = f"{name}{'/' + str(ratio) if name == 'offset' else ''}"
    what = f"rows {rows} D {D}"
    for rms in kinds:
        kern = "rmsnorm" if rms else "layernorm"
        run = (lambda xv, out, eps: ops.rmsnorm_ex(xv, w, eps, out=out)) if rms else (lambda xv, out, eps: ops.layernorm_ex(xv, w, b, eps, out=out))
        for eps in eps_set:
            R = EP.norm_reference(x, w, b, eps, dtype, rms)
            for padx, pady in ((0, 0), (64, 8)):
                xb, xv, _ = EP.lay_rows(x, padx, dtype, EP.POISON)
                yb, yv, ldy = EP.lay_rows(torch.zeros_like(x), pady, dtype, "sentinel")
                snap_x, snap_y = xb.clone(), yb.clone()
                run(xv, yv, eps)
                judge(el, kern, tag, EP.error_ratio(yv, R), f"{what} eps {eps} pad {padx}/{pady}", detail=lambda: EP.describe(kern, yv, R))
                assert torch.equal(xb, snap_x), f"{kern} {tag} {what}: the input buffer changed"
                assert EP.outside_unchanged(yb, snap_y, ldy, rows, D), f"{kern} {tag} {what}: a store outside the output rows"
            # in place, strided: the engine's last-row prefill form (ldx = ldy > D)
            xb, xv, ld = EP.lay_rows(x, 64, dtype, EP.POISON)
            snap = xb.clone()
            run(xv, xv, eps)
            judge(el, kern, tag, EP.error_ratio(xv, R), f"{what} eps {eps} in place", detail=lambda: EP.describe(kern, xv, R))
            assert EP.outside_unchanged(xb, snap, ld, rows, D), f"{kern} {tag} {what}: in place, a store outside the rows"
    if not forms:
        return
    eps = 1e-6                                                      # the STC connector's call sites
    res_small = small_residual(rows, D, dtype)
    for silu in (True, False):
        for res_name, res in (("none", None), ("small", res_small), ("cancel", EP.cancel_residual(x, w, b, eps, dtype))):
            if res is None and not silu:
                continue
            R = EP.norm_reference(x, w, b, eps, dtype, False, silu, res)
            form = f"{'silu' if silu else 'id'}+res:{res_name}"
            xb, xv, _ = EP.lay_rows(x, 8, dtype, EP.POISON)
            if res is None:
                yb, yv, ldy = EP.lay_rows(torch.zeros_like(x), 8, dtype, "sentinel")
                snap = yb.clone()
                ops.layernorm_ex(xv, w, b, eps, out=yv, silu=silu)
            else:                                                   # y == res, as the RegNet block tail calls it
                yb, yv, ldy = EP.lay_rows(res, 16, dtype, "sentinel")
                snap = yb.clone()
                ops.layernorm_ex(xv, w, b, eps, out=yv, silu=silu, res=yv)
            judge(el, "layernorm", f"{tag} {form}", EP.error_ratio(yv, R), what, detail=lambda: EP.describe(form, yv, R))
            assert EP.outside_unchanged(yb, snap, ldy, rows, D), f"layernorm {tag} {form} {what}: a store outside the output rows"


def small_residual(rows, D, dtype):
    return EP.GP.small_residual(rows, D, DEV).to(dtype)


@pytest.mark.parametrize("D", [8, 128, 520, 1024, 4096])
def test_norms(el, D):
    dtype = DTYPES[el]
    for rows in (1, 3, 4, 5):
        for name in EP.NORM_PROBES:
            for ratio in (EP.OFFSET_RATIOS if name == "offset" else (0,)):
                norm_case(el, name, rows, D, dtype, ratio, forms=(rows in (3, 5)))


@pytest.mark.parametrize("rows", [4095, 4096, 4097, 4111])
def test_norm1024_switch(el, rows):
    """D = 1024 on either side of the 4096-row switch to norm1024_kernel (4 rows per wave: rows % 16 in {15, 0, 1, 15} leave 1 .. 3 clamped tail rows)"""
    dtype = DTYPES[el]
    for name, ratio in (("onehot", 0), ("ramp", 0), ("eps", 0), ("offset", 256)):
        norm_case(el, name, rows, 1024, dtype, ratio, eps_set=(1e-5,) if name != "eps" else EPS_SET, forms=(name == "ramp"))


# ---- slot pool ------------------------------------------------------------------------------------------------------------------------------
def slot_run(pr):
    return ops.slot_pool(pr.feats, pr.ln_w, pr.ln_b, pr.slots, pr.cos_t, pr.sin_t, pr.eps)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 16, 37, 576, 577, 729])
@pytest.mark.parametrize("D", [16, 128, 1024])
def test_slot_pool(el, D, n):
    """8 parts of ceil(n / 8) rows: n = 1, 7 leave empty parts, 8 one row each, 9 and 37 a ragged last part and empty ones, 576 the real shape,
    577 a last part of one row, 729 parts of 92 rows"""
    dtype = DTYPES[el]
    for T in (1, 3):
        cases = [("uniform", 0, None), ("pointer", 0, None), ("pointer", 0, "padded"), ("ramp", 0, None), ("rope", 0, None), ("eps", 0, None),
                 ("frames", 0, None), ("offset", 0, None), ("offset", 4, None), ("offset", 32, None), ("offset", 256, None)]
        for name, ratio, layout in cases:
            pr = EP.slot_probe(name, T, n, D, dtype, DEV, ratio, layout)
            R = EP.slot_probe_reference(pr)
            snap = pr.buf.clone()
            got = slot_run(pr)
            assert torch.equal(pr.buf, snap)
            tag = name + (f"/{ratio}" if name == "offset" else "") + (f" {layout}" if layout else "")
            judge(el, "slot_pool", tag, EP.error_ratio(got, R), f"T {T} n {n} D {D}", table=RECORDED if (name, ratio) == ("offset", 256) else MARGINS,
                  detail=lambda: EP.describe(tag, got, R))


# ---- front end ------------------------------------------------------------------------------------------------------------------------------
def frontend_run(pr, guard=True):
    """-> (X [T, G G + 1, D], the guard rows after it are intact)"""
    NT = pr.G * pr.G + 1
    buf = torch.zeros((pr.T * NT + EP.FRONTEND_GUARD_ROWS) * pr.D, dtype=pr.dtype, device=DEV)
    buf.view(torch.int16).fill_(EP.SENTINEL)
    X = ops.patch_embed(pr.frames, pr.W, pr.cls, pr.pos, pr.lw, pr.lb, pr.P, pr.eps, out=buf)
    return X, bool((buf[pr.T * NT * pr.D:].view(torch.int16) == EP.SENTINEL).all())


FRONTEND_SHAPES = [(14, S, D) for S in (14, 56, 112, 126, 336) for D in (128, 1024)] + [(16, S, D) for S in (16, 144, 336) for D in (128, 1024)] \
    + [(14, 126, 256), (16, 144, 512)]


@pytest.mark.parametrize("P,S,D", FRONTEND_SHAPES, ids=[f"P{p}-S{s}-D{d}" for p, s, d in FRONTEND_SHAPES])
def test_frontend(el, P, S, D):
    """grids of 1, 16, 64, 81 = 64 + 17 and 576 patches at P = 14 (pad columns, the shifted window at the last patch column); 1, 81 and
    441 = 6 x 64 + 57 at P = 16 (no pad columns)"""
    dtype = DTYPES[el]
    for T in (1, 3):
        for name in EP.FRONTEND_PROBES:
            for shift in (EP.pointer_shifts(D, P) if name == "pointer" else (0,)):
                for fp32 in ((True,) if name == "round" else (False, True)):
                    pr = EP.frontend_probe(name, T, S, P, D, dtype, DEV, shift)
                    if fp32 and name != "round":
                        pr.frames = pr.frames.float()
                    R = EP.frontend_probe_reference(pr)
                    X, intact = frontend_run(pr)
                    what = f"P {P} S {S} D {D} T {T} shift {shift} {'fp32' if fp32 else el} frames"
                    judge(el, "patch_embed", name, EP.frontend_ratio(X, R, pr), what, detail=lambda: EP.describe(name, torch.nan_to_num(X.float()), R))
                    assert intact, f"patch_embed {name} {what}: a store past the last frame's rows"
                    assert EP.nan_rows_ok(X, pr), f"patch_embed {name} {what}: a NaN pixel's own row is finite, or its left neighbour's row is not"
                    if fp32 and name == "pointer":                  # 16-bit-representable fp32 pixels: the same bits as the 16-bit frames
                        pr.frames = pr.frames.to(dtype)
                        assert torch.equal(frontend_run(pr)[0], X), f"patch_embed {what}: fp32 frames differ from the 16-bit frames"


def test_frontend_refused_geometries(el):
    """P = 12, S % P != 0 and D = 384 are the three-pass path's: the op answers TRACE_ERR_ARG (-1) before it touches anything"""
    dtype = DTYPES[el]
    for P, S, D in ((12, 48, 128), (14, 60, 128), (14, 56, 384)):
        G = S // P
        z = lambda *shape: torch.zeros(shape, dtype=dtype, device=DEV)
        with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_op_patch_embed"):
            ops.patch_embed(z(1, 3, S, S), z(D, 3 * P * P), z(D), z(G * G + 1, D), z(D), z(D), P, 1e-5)


# ---- wiring: the engine's own calls --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["bf16", "f16"])
def wired(request):
    """a tiny engine whose ViT runs no encoder layer (vision_num_layers = 1: hidden_states[-2] is the front end's output), with the front end's
    weights taken from the `pointer` probe and the slot pool's readout = [I; 0]: eng.slot_pool returns `res` in its first v_hidden columns"""
    element = request.param
    dtype = DTYPES[element]
    cfg = tcfg.tiny(num_frames=3)
    cfg.vision_num_layers = 1
    assert cfg.vision_layers_used == 0
    pr = EP.frontend_probe("pointer", 3, cfg.vision_image_size, cfg.vision_patch_size, cfg.vision_hidden_size, dtype, DEV)
    sd = dict(synth.state_dict(cfg))
    vh, H = cfg.vision_hidden_size, cfg.hidden_size
    sd[synth.VIS + "embeddings.patch_embedding.weight"] = pr.W.reshape(vh, 3, pr.P, pr.P).float().cpu()
    sd[synth.VIS + "embeddings.class_embedding"] = pr.cls.float().cpu()
    sd[synth.VIS + "embeddings.position_embedding.weight"] = pr.pos.float().cpu()
    sd[synth.VIS + "pre_layrnorm.weight"] = pr.lw.float().cpu()
    sd[synth.VIS + "pre_layrnorm.bias"] = pr.lb.float().cpu()
    ro = torch.zeros((H, vh))
    ro[:vh] = torch.eye(vh)
    sd["model.mm_projector.readout.weight"] = ro
    eng = TraceEngine(cfg, device=0, max_batch=1, max_ctx=128, max_frames=3, max_new_tokens=8, dtype=dtype)
    eng.load_weights(sd.items())
    yield SimpleNamespace(eng=eng, cfg=cfg, pr=pr, sd=sd, el=element, dtype=dtype)
    ops.use("bf16")
    eng.close()


def test_engine_front_end_is_the_op(wired):
    """eng.vit_forward (no encoder layer) == trace_op_patch_embed bit for bit, for 16-bit and fp32 frames; and within the judge's bound"""
    ops.use(wired.el)
    pr = wired.pr
    R = EP.frontend_probe_reference(pr)
    X, _ = frontend_run(pr)
    for frames in (pr.frames, pr.frames.float()):
        f = wired.eng.vit_forward(frames)
        assert torch.equal(f, X[:, 1:]), "the engine's front end differs from the op"
    judge(wired.el, "patch_embed", "engine", EP.frontend_ratio(X, R, pr), "tiny engine")


def test_engine_three_pass_front_end(wired):
    """vit.patch_fused = 0: im2col -> GEMM -> assemble passes the same judge (its rows before the LN are the same exact integers)"""
    ops.use(wired.el)
    pr = wired.pr
    R = EP.frontend_probe_reference(pr)
    with ops.tuned(vit__patch_fused=0):
        f = wired.eng.vit_forward(pr.frames)
    Rp = SimpleNamespace(cands=[c[:, 1:] for c in R.cands], bounds=[b[:, 1:] for b in R.bounds], ref=R.ref[:, 1:])
    judge(wired.el, "vit 3-pass", "pointer", EP.error_ratio(f, Rp), "tiny engine", detail=lambda: EP.describe("three-pass", f, Rp))


def test_engine_slot_pool_is_the_op(wired):
    """eng.slot_pool(None, T) (internal feats: frame stride (n + 1) D, CLS skipped) and eng.slot_pool(feats, T) == trace_op_slot_pool with the engine's
    own tables, bit for bit; the op's result within the judge's bound"""
    ops.use(wired.el)
    cfg, eng, dtype = wired.cfg, wired.eng, wired.dtype
    vh, n, T = cfg.vision_hidden_size, cfg.vision_patches, 3
    frames = synth.synth_frames(cfg, 0)[:T].to(dtype).to(DEV)
    feats = eng.vit_forward(frames)
    own = eng.slot_pool(None, T)
    given = eng.slot_pool(feats, T)
    g = lambda k: wired.sd[k].to(dtype).to(DEV)
    cos_t, sin_t = EP.rope_tables(n, vh, cfg.slot_rope_base, DEV)
    lw, lb, sl = g("model.mm_projector.ln_vision.weight"), g("model.mm_projector.ln_vision.bias"), g("model.mm_projector.slots")
    res = ops.slot_pool(feats, lw, lb, sl, cos_t, sin_t, cfg.slot_ln_eps)
    assert torch.equal(own[:, :, :vh], res) and torch.equal(given[:, :, :vh], res), "the engine's slot pool differs from the op"
    assert not bool(own[:, :, vh:].any()) and not bool(given[:, :, vh:].any())
    R = EP.slot_reference(feats, lw, lb, sl, cos_t, sin_t, cfg.slot_ln_eps, dtype)
    judge(wired.el, "slot_pool", "engine", EP.error_ratio(res, R), "tiny engine", detail=lambda: EP.describe("slot pool", res, R))
