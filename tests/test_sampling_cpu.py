"""Sampling without a GPU: the Philox known-answer check against rocRAND's own header, the float32 restatement of the device sampler
(trace_amd/sampling.py) against transformers' warpers, the generate() argument mapping, and the sampling kernel's register budget."""
import json
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from trace_amd.sampling import SamplingParams, philox_uniform, philox_x, sample_row_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

_KAT = r"""
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_philox4x32_10.h>
#include <stdio.h>
#include "philox.h"
int main() {
    unsigned long long s = 88172645463325252ull;
    for (int i = 0; i < 12000; ++i) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const unsigned long long seed = i % 3 ? s : (unsigned long long)i;
        const unsigned step = (unsigned)(s >> 20) % 100000, b = (unsigned)(s >> 44) % 512;
        rocrand_state_philox4x32_10 st;
        rocrand_init(seed, b, 4ull * step, &st);
        printf("%llu %u %u %u %u\n", seed, step, b, rocrand(&st), philox4x32_10_x(seed, step, 0u, b, 0u));
    }
    return 0;
}
"""


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_philox_equals_rocrand(tmp_path):
    src = tmp_path / "kat.cpp"
    src.write_text(_KAT)
    exe = str(tmp_path / "kat")
    r = subprocess.run([HIPCC, "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    d = np.array([int(x) for x in out], dtype=object).reshape(-1, 5)
    seed = np.array(d[:, 0].tolist(), np.uint64)
    step, b, want, mine = (np.array(d[:, i].tolist(), np.uint64) for i in (1, 2, 3, 4))
    assert len(seed) >= 10000
    assert (mine == want).all()                                                   # the project's header
    assert (philox_x(seed, step, 0, b, 0) == want.astype(np.uint32)).all()        # the numpy restatement
    u = philox_uniform(seed, step, b)
    assert (u == ((want >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24))).all() and u.max() < 1


def _hf_kept(row, T, k, p):
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    s = torch.from_numpy(row.copy()).view(1, -1)
    s = lp.TemperatureLogitsWarper(T)(None, s)
    if k:
        s = lp.TopKLogitsWarper(k)(None, s)
    if p < 1:
        s = lp.TopPLogitsWarper(p)(None, s)
    return torch.isfinite(s).view(-1).numpy()


@pytest.mark.parametrize("n", [32001, 13, 320])
@pytest.mark.parametrize("kind", ["distinct", "ties"])
def test_restatement_keeps_what_hf_keeps(n, kind):
    rng = np.random.RandomState(n + len(kind))
    checked = 0
    for trial in range(6):
        row = (rng.randn(n) * 2.5).astype(np.float32)
        if kind == "ties":
            row = (np.round(row * 2) / 2).astype(np.float32)
        for T, k, p in [(0.2, 50, 1.0), (1.0, 5, 0.8), (1.7, 1024, 0.1), (1.0, 1, 1.0), (0.7, 0, 0.9), (1.0, 50, 0.95)]:
            info = {}
            pick = sample_row_ref(row, T, k, p, np.float32(rng.rand()), info)
            kept = np.zeros(n, bool)
            kept[info["kept"]] = True
            assert kept[pick]
            hf = _hf_kept(row, T, k, p)
            x = row / np.float32(T)
            if kind == "distinct" or p >= 1:
                # HF's top-p order among EQUAL values is torch.sort's, not id order: with ties only the count and the value set must agree
                if kind == "distinct":
                    mass = np.sort(np.exp(x[hf].astype(np.float64) - x.max()))[::-1].cumsum() / np.exp(x[hf] - x.max()).sum()
                    if p < 1 and np.abs(mass - p).min() < 1e-5:
                        continue                                            # a boundary case of float rounding
                assert (kept == hf).all(), (T, k, p, kept.sum(), hf.sum())
            else:
                assert kept.sum() == hf.sum() and set(x[kept]) == set(x[hf]), (T, k, p)
            checked += 1
    assert checked >= 30


def test_restatement_draw_walks_the_kept_order():
    row = np.array([0.0, 3.0, 1.0, 3.0, 2.0], np.float32)
    # T = 1, k = 3: kept = 1, 3 (tie at the top, id order), 4; weights 1, 1, e^-1
    w = np.array([1.0, 1.0, np.exp(-1.0)])
    cum = np.cumsum(w) / w.sum()
    for u, want in [(0.0, 1), (cum[0] - 1e-4, 1), (cum[0] + 1e-4, 3), (cum[1] + 1e-4, 4), (0.99999, 4)]:
        assert sample_row_ref(row, 1.0, 3, 1.0, np.float32(u)) == want
    # top_p 0.5: the mass above token 3 is 1 / (2 + e^-1) < 0.5 -> both top tokens stay, token 4 goes
    info = {}
    sample_row_ref(row, 1.0, 3, 0.5, np.float32(0.5), info)
    assert sorted(info["kept"].tolist()) == [1, 3]
    # top_k 0 / top_p 1: the whole row in id order
    assert sample_row_ref(row, 1.0, 0, 1.0, np.float32(0.0)) == 0


def test_sampling_params_validation():
    assert SamplingParams().top_k == 50 and SamplingParams().top_p == 1.0
    for bad in (dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    assert SamplingParams(1.0, 1024, 0.3).on_device and SamplingParams(1.0, 0, 1.0).on_device
    assert not SamplingParams(1.0, 0, 0.9).on_device and not SamplingParams(1.0, 2048, 1.0).on_device


class _FakeEngine:
    device, dtype = "cpu", None


def _model():
    from trace_amd.config import tiny
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    return TraceMistralForCausalLM(tiny(num_frames=4), _FakeEngine())


def test_generate_argument_mapping():
    torch = pytest.importorskip("torch")
    m = _model()
    sp = m._sampling_params(True, 0.2, None, None, None, {})
    assert (sp.temperature, sp.top_k, sp.top_p) == (0.2, 50, 1.0)                   # HF's defaults
    assert m._sampling_params(None, None, None, None, None, {}) is None             # greedy by default
    assert m._sampling_params(True, 0.0, None, None, None, {}) is None              # temperature 0 = greedy
    sp = m._sampling_params(None, None, None, None, {"do_sample": True, "top_k": 7, "top_p": 0.5}, {})
    assert (sp.temperature, sp.top_k, sp.top_p) == (1.0, 7, 0.5)
    torch.manual_seed(11)
    s1 = m._sampling_params(True, 1.0, 3, 0.9, None, {}).seed
    s2 = m._sampling_params(True, 1.0, 3, 0.9, None, {}).seed
    torch.manual_seed(11)
    assert m._sampling_params(True, 1.0, 3, 0.9, None, {}).seed == s1 != s2
    for bad in (dict(top_p=0.0), dict(top_p=1.01), dict(top_k=-2)):
        with pytest.raises(ValueError):
            m._sampling_params(True, 1.0, bad.get("top_k"), bad.get("top_p"), None, {})
    for kw in (dict(num_beams=2), dict(num_return_sequences=2), dict(typical_p=0.9), dict(min_p=0.1), dict(repetition_penalty=1.2)):
        with pytest.raises(NotImplementedError):
            m._sampling_params(True, 1.0, None, None, None, kw)
    assert m._sampling_params(True, 1.0, None, None, None, dict(num_beams=1, repetition_penalty=1.0)) is not None


def test_generation_config_json_pickup(tmp_path):
    from trace_amd.model.builder import apply_generation_config
    m = _model()
    apply_generation_config(m, str(tmp_path))                                       # no file: HF defaults stay
    assert (m.generation_config.do_sample, m.generation_config.top_k) == (False, 50)
    (tmp_path / "generation_config.json").write_text(json.dumps({"do_sample": True, "temperature": 0.6, "top_k": 20, "top_p": 0.9,
                                                                  "bos_token_id": 1}))
    apply_generation_config(m, str(tmp_path))
    sp = m._sampling_params(None, None, None, None, None, {})
    assert (sp.temperature, sp.top_k, sp.top_p) == (0.6, 20, 0.9)
    assert m._sampling_params(False, None, None, None, None, {}) is None            # an explicit argument wins


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_sampling_kernels_have_no_scratch(tmp_path):
    for name, pat in (("sample", "sample_rows_kernel"), ("select", "select_next_kernel")):
        for f16 in (False, True):
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(CSRC, name + ".hip"), "-I", CSRC,
                   "-o", str(tmp_path / (name + ".o")), "-Rpass-analysis=kernel-resource-usage"] + (["-DTRACE_F16"] if f16 else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            found, cur = 0, None
            for line in r.stderr.splitlines():
                mm = re.search(r"Function Name: (\S+)", line)
                if mm:
                    cur = mm.group(1)
                mm = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
                if mm and cur and pat in cur:
                    found += 1
                    assert int(mm.group(1)) == 0, (cur, line)
            assert found == (1 if name == "sample" else 3), (name, found)       # select.hip: the tile, the sampling and the row form
