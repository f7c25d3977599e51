"""Which of the three decode-step bodies a batch runs (csrc/engine.hip decode_step): the body that takes profiling mode 2's bracket (get_profile()[8]: 1 the
GEMV step, 2 the fused-norm GEMV step, 3 the wide GEMM step) is the one ops.decode_route announces, at every batch size where the route changes and under
the tuning values that move those edges.

The geometry is the tiny one (hidden 4096, intermediate 256, 2 layers): the smallest that reaches all three bodies — its qkv (6144 x 4096) and gate|up
(512 x 4096) shapes take the fused-norm GEMV up to 4 rows.  `want` restates decode_step's conditions for it (tests/test_decode_plan_cpu.py checks the
route against them over every batch size without a GPU)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from trace_amd import config as tcfg, synth  # noqa: E402
from trace_amd._lib import TraceHipError  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402

ROWS = 8                      # prefilled rows per slot
SCHEMES = {None: 0, "w8a8": 1, "weight_only": 2}
WIDE65, FUSE0, FUSE4 = dict(decode__wide_min_rows=65), dict(decode__fuse_norm_rows=0), dict(decode__fuse_norm_rows=4)
# (fp8 scheme, B, tuning values, step body)
CASES = [(None, 1, {}, 2), (None, 2, {}, 1), (None, 31, {}, 1), (None, 32, {}, 3), (None, 64, {}, 3), (None, 65, {}, 3), (None, 129, {}, 3),
         (None, 32, WIDE65, 1), (None, 65, WIDE65, 3), (None, 1, FUSE0, 1), (None, 4, FUSE4, 2)]
CASES += [(s, B, {}, 1) for s in ("w8a8", "weight_only") for B in (1, 33, 64)]


@pytest.fixture(scope="module")
def engines():
    """get(scheme) -> engine whose KV slots all hold the same ROWS prefilled rows; made on first use"""
    cfg = tcfg.tiny(num_frames=4)
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers) == (4096, 256, 2)
    sd = synth.state_dict(cfg)
    made = {}

    def get(scheme):
        if scheme not in made:
            nslots = 130 if scheme is None else 66
            eng = TraceEngine(cfg, max_batch=nslots, max_ctx=64, max_frames=4, max_new_tokens=4, llm_fp8=scheme or False)
            eng.load_weights(sd.items())
            emb = torch.randn((ROWS, cfg.hidden_size), generator=torch.Generator().manual_seed(7)).to(torch.bfloat16).cuda()
            eng.prefill(0, ROWS, embeds=emb)
            eng.kv_copy(0, list(range(1, nslots)), ROWS)
            made[scheme] = eng
        return made[scheme]
    yield cfg, get
    for eng in made.values():
        eng.close()


@pytest.mark.parametrize("scheme,B,tuning,want", CASES, ids=[f"{s or 'bf16'}-{B}" + "".join(f"-{k.split('__')[-1]}{v}" for k, v in t.items()) for s, B, t, _ in CASES])
def test_the_announced_step_body_runs(engines, scheme, B, tuning, want):
    cfg, get = engines
    eng = get(scheme)
    qkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * (cfg.hidden_size // cfg.num_attention_heads)
    with ops.tuned(**tuning):
        route = ops.decode_route(B, SCHEMES[scheme], cfg.hidden_size, cfg.intermediate_size, qkv)
        eng.set_profile(2)
        eng.decode_begin(list(range(B)), [1] * B, 4)
        eng.decode_steps(1, use_graph=False)
        ran = eng.get_profile()[8]
        eng.set_profile(0)
    assert route["step"] == want and route["kind"] == SCHEMES[scheme]
    assert ran == want


@pytest.mark.parametrize("scheme", ["w8a8", "weight_only"])
def test_fp8_weights_decode_at_most_64_sequences(engines, scheme):
    _, get = engines
    with pytest.raises(TraceHipError, match="bad batch"):
        get(scheme).decode_begin(list(range(65)), [1] * 65, 4)
