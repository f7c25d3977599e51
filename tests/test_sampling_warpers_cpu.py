"""min_p, typical_p, epsilon_cutoff and eta_cutoff without a GPU: the float32 restatement of the device sampler (trace_amd/sampling.py
sample_row_ref) against transformers' own warpers in HF's order, hand-made rows with the answer written out, the four-off path against ids
recorded from the sampler before it had them (tests/golden/sampling_off_ids.json), the argument checks and generate()'s argument mapping."""
import json
import os

import numpy as np
import pytest

from trace_amd.sampling import SamplingParams, check_sampling, sample_row_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)


def _hf_kept(row, T, k, p, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """the ids HF's chain keeps: the warpers as _get_logits_processor orders them, each built only when armed"""
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    s = torch.from_numpy(np.asarray(row, np.float32).copy()).view(1, -1)
    s = lp.TemperatureLogitsWarper(float(T))(None, s)
    if k:
        s = lp.TopKLogitsWarper(int(k))(None, s)
    if p < 1:
        s = lp.TopPLogitsWarper(float(p))(None, s)
    if min_p > 0:
        s = lp.MinPLogitsWarper(float(min_p))(None, s)
    if typical_p < 1:
        s = lp.TypicalLogitsWarper(float(typical_p))(None, s)
    if epsilon_cutoff > 0:
        s = lp.EpsilonLogitsWarper(float(epsilon_cutoff))(None, s)
    if eta_cutoff > 0:
        s = lp.EtaLogitsWarper(float(eta_cutoff))(None, s)
    return torch.isfinite(s).view(-1).numpy()


def _row(rng, n, kind):
    x = (rng.randn(n) * 2.0).astype(np.float32)
    if kind == "ties":
        x[rng.randint(0, n, 3 + n // 64)] = x.max()                    # a tie at the top
        x[rng.randint(0, n, 3 + n // 64)] = np.sort(x)[-5]             # and one further down
    if kind == "flat":
        x[:] = np.float32(rng.randn())
    return x


def _kept_mask(info, n):
    kept = np.zeros(n, bool)
    kept[info["kept"]] = True
    return kept


_BASES = [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.4, 20, 0.9)]              # (T, top_k, top_p) in front of the new warpers
_VALUES = dict(min_p=(0.02, 0.1, 0.3), typical_p=(0.2, 0.6, 0.95), epsilon_cutoff=(1e-3, 0.01, 0.05), eta_cutoff=(1e-3, 0.01, 0.1))


@pytest.mark.parametrize("n", [13, 33, 321])
@pytest.mark.parametrize("kind", ["gauss", "ties", "flat"])
def test_restatement_keeps_what_hf_keeps(n, kind):
    rng = np.random.RandomState(1000 + n + len(kind))
    rows = left_out = 0
    for armed in (["min_p"], ["typical_p"], ["epsilon_cutoff"], ["eta_cutoff"], list(_VALUES)):
        for T, k, p in _BASES:
            for trial in range(20):
                row = _row(rng, n, kind)
                w = dict(OFF, **{name: _VALUES[name][rng.randint(3)] for name in armed})
                info = {}
                pick = sample_row_ref(row, T, k, p, np.float32(rng.rand()), info, **w)
                kept = _kept_mask(info, n)
                assert kept[pick] and kept.sum() >= 1
                assert set(info["stages"]) == {"top_p"} | set(armed)
                rows += 1
                if info["margin"] < 1e-5:                              # a decision within float rounding of its threshold: either side is right
                    left_out += 1
                    continue
                hf = _hf_kept(row, T, k, p, **w)
                if kind == "gauss" or p >= 1:
                    assert (kept == hf).all(), (armed, T, k, p, w, np.nonzero(kept)[0], np.nonzero(hf)[0], info["margins"])
                else:
                    # HF's top-p order among EQUAL values is torch.sort's, not id order: which ids of a cut tie class stay differs, their number and
                    # value do not
                    x = row / np.float32(T)
                    assert sorted(x[kept]) == sorted(x[hf]), (armed, T, k, p, w, info["margins"])
    print(f"n={n} {kind}: {left_out} of {rows} rows left out (margin < 1e-5)")
    assert left_out <= 0.01 * rows


def _kept(row, **kw):
    info = {}
    args = dict(temperature=1.0, top_k=50, top_p=1.0, u=np.float32(0.5), info=info)
    args.update(kw)
    pick = sample_row_ref(np.asarray(row, np.float32), **args)
    assert pick in info["kept"]
    return sorted(int(i) for i in info["kept"]), info


def test_min_p_keeps_exactly_two():
    row = -np.arange(10, dtype=np.float32)                              # p ratios 1, e^-1 = 0.37, e^-2 = 0.135 < 0.2, ...
    for k in (50, 0):
        kept, info = _kept(row, top_k=k, min_p=0.2)
        assert kept == [0, 1]
        assert info["margin"] > 0.3
    assert _hf_kept(row, 1.0, 50, 1.0, min_p=0.2).nonzero()[0].tolist() == [0, 1]


def test_typical_p_drops_the_arg_max():
    # one token at p = 0.3 beside 70 at 0.01: H = 3.585, |-log p - H| = 2.38 for the top one and 1.02 for the others, which come first and reach 0.6
    row = np.log(np.array([0.01] * 30 + [0.3] + [0.01] * 40, np.float64)).astype(np.float32)
    want = [i for i in range(71) if i != 30]
    for k in (1024, 50, 0):
        kept, info = _kept(row, top_k=k, typical_p=0.6)
        assert kept == want, k
        assert info["margin"] > 0.1
        for u in (0.0, 0.3, 0.999):
            assert sample_row_ref(row, 1.0, k, 1.0, np.float32(u), typical_p=0.6) != 30
    assert _hf_kept(row, 1.0, 0, 1.0, typical_p=0.6).nonzero()[0].tolist() == want
    # the same with the 70 all different (an interval of sorted candidates instead of the tie block)
    row2 = row.copy()
    row2[np.arange(71) != 30] += np.linspace(-0.05, 0.05, 70).astype(np.float32)
    kept, _ = _kept(row2, top_k=1024, typical_p=0.6)
    assert 30 not in kept and kept == _hf_kept(row2, 1.0, 0, 1.0, typical_p=0.6).nonzero()[0].tolist()


def test_epsilon_keeps_a_tied_maximum_when_everything_is_below():
    row = np.zeros(300, np.float32)
    row[[17, 200]] = 0.5                                               # every p is about 1 / 300, far below 0.5
    for k in (1024, 0):
        kept, info = _kept(row, top_k=k, epsilon_cutoff=0.5)
        assert kept == [17, 200]
    assert _hf_kept(row, 1.0, 0, 1.0, epsilon_cutoff=0.5).nonzero()[0].tolist() == [17, 200]


def test_eta_takes_both_branches_of_the_min():
    # flat-ish: H = 4.46, sqrt(0.36) exp(-H) = 0.0069 < 0.36: p = 0.0049 goes, 0.015 stays (epsilon itself would leave the top token alone)
    p = np.array([0.02] + [0.015] * 49 + [0.0049] * 50)
    row = np.log(p / p.sum()).astype(np.float32)
    kept, info = _kept(row, top_k=1024, eta_cutoff=0.36)
    assert kept == list(range(50)) and info["margin"] > 0.2
    assert _hf_kept(row, 1.0, 0, 1.0, eta_cutoff=0.36).nonzero()[0].tolist() == kept
    # peaked: H = 0.43, sqrt(0.04) exp(-H) = 0.13 > 0.04: eta = epsilon = 0.04 keeps 0.9 and 0.05 (the other branch would keep 0.9 alone)
    row = np.log(np.array([0.03, 0.9, 0.02, 0.05])).astype(np.float32)
    kept, info = _kept(row, top_k=1024, eta_cutoff=0.04)
    assert kept == [1, 3] and info["margin"] > 0.2
    assert _hf_kept(row, 1.0, 0, 1.0, eta_cutoff=0.04).nonzero()[0].tolist() == kept


def test_four_off_returns_the_recorded_ids():
    """the rows, parameters and u of tests/test_sampling_cpu.py test_restatement_keeps_what_hf_keeps, drawn the same way; the ids are those the
    restatement returned before it knew the four warpers"""
    with open(os.path.join(ROOT, "tests", "golden", "sampling_off_ids.json")) as f:
        golden = json.load(f)
    for n in (32001, 13, 320):
        for kind in ("distinct", "ties"):
            rng = np.random.RandomState(n + len(kind))
            got = []
            for trial in range(6):
                row = (rng.randn(n) * 2.5).astype(np.float32)
                if kind == "ties":
                    row = (np.round(row * 2) / 2).astype(np.float32)
                for T, k, p in [(0.2, 50, 1.0), (1.0, 5, 0.8), (1.7, 1024, 0.1), (1.0, 1, 1.0), (0.7, 0, 0.9), (1.0, 50, 0.95)]:
                    u = np.float32(rng.rand())
                    a = sample_row_ref(row, T, k, p, u)
                    assert a == sample_row_ref(row, T, k, p, u, None, **OFF)
                    got.append(a)
            assert got == golden[f"{n}-{kind}"], (n, kind)


def test_check_sampling_domains_and_device_domain():
    sp = SamplingParams(0.7, 40, 0.9, 123)                               # positional (T, k, p, seed) still builds, the four off
    assert (sp.seed, sp.min_p, sp.typical_p, sp.epsilon_cutoff, sp.eta_cutoff) == (123, 0.0, 1.0, 0.0, 0.0) and not sp.warpers_armed
    for bad, msg in ((dict(min_p=-0.1), "`min_p` has to be a float in the [0, 1] interval"), (dict(min_p=1.5), "`min_p`"),
                     (dict(typical_p=0.0), "`typical_p` has to be a float > 0 and < 1"), (dict(typical_p=1.2), "`typical_p`"),
                     (dict(epsilon_cutoff=1.0), "`epsilon_cutoff` has to be a float > 0 and < 1"), (dict(epsilon_cutoff=-1e-3), "`epsilon_cutoff`"),
                     (dict(eta_cutoff=1.0), "`eta_cutoff` has to be a float > 0 and < 1"), (dict(eta_cutoff=float("nan")), "`eta_cutoff`")):
        with pytest.raises(ValueError, match=msg.replace("[", r"\[").replace("]", r"\]")):
            SamplingParams(**bad)
        with pytest.raises(ValueError):
            check_sampling(1.0, 50, 1.0, **dict(OFF, **bad))
    check_sampling(1.0, 50, 1.0, min_p=1.0, typical_p=0.5, epsilon_cutoff=0.999, eta_cutoff=1e-4)
    for name, v in (("min_p", 0.1), ("typical_p", 0.9), ("epsilon_cutoff", 3e-4), ("eta_cutoff", 3e-4)):
        assert SamplingParams(1.0, 50, 1.0, **{name: v}).on_device and SamplingParams(1.0, 1024, 0.5, **{name: v}).on_device
        assert SamplingParams(1.0, 50, 1.0, **{name: v}).warpers_armed
        assert not SamplingParams(1.0, 0, 1.0, **{name: v}).on_device          # top_k off with a warper armed: the host path
        assert not SamplingParams(1.0, 2000, 1.0, **{name: v}).on_device
    assert SamplingParams(1.0, 0, 1.0).on_device


class _FakeEngine:
    """stands for TraceEngine: what the model asks of it here is the list of warpers its sampler applies"""
    device, dtype = "cpu", None
    sampling_warpers = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def _model(engine=None):
    from trace_amd.config import tiny
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    return TraceMistralForCausalLM(tiny(num_frames=4), engine or _FakeEngine())


def test_generate_argument_mapping_of_the_four():
    """generate() picks min_p / typical_p / epsilon_cutoff / eta_cutoff with HF's precedence.  Before, typical_p and min_p raised
    NotImplementedError and the two cutoffs were read by nothing: a generation_config that set them was sampled without them."""
    pytest.importorskip("torch")
    from trace_amd.engine import TraceEngine
    assert TraceEngine.sampling_warpers == _FakeEngine.sampling_warpers               # the real engine lists all four
    m = _model()
    sp = m._sampling_params(True, 1.0, None, None, None, dict(typical_p=0.9))           # (raised NotImplementedError before)
    assert sp.typical_p == 0.9 and (sp.min_p, sp.epsilon_cutoff, sp.eta_cutoff) == (0.0, 0.0, 0.0)
    sp = m._sampling_params(True, 1.0, None, None, None, dict(min_p=0.1, epsilon_cutoff=3e-4, eta_cutoff=2e-3))
    assert (sp.min_p, sp.typical_p, sp.epsilon_cutoff, sp.eta_cutoff) == (0.1, 1.0, 3e-4, 2e-3)
    gc = {"do_sample": True, "min_p": 0.05, "typical_p": 0.8, "epsilon_cutoff": 1e-3, "eta_cutoff": 5e-3}
    sp = m._sampling_params(None, None, None, None, gc, {})
    assert (sp.min_p, sp.typical_p, sp.epsilon_cutoff, sp.eta_cutoff) == (0.05, 0.8, 1e-3, 5e-3)
    sp = m._sampling_params(None, None, None, None, gc, dict(min_p=0.3, typical_p=None))     # an argument wins; None falls through
    assert (sp.min_p, sp.typical_p) == (0.3, 0.8)
    m.generation_config.min_p, m.generation_config.eta_cutoff = 0.2, 4e-3                  # the model's own defaults come last
    sp = m._sampling_params(True, 1.0, None, None, {"eta_cutoff": 6e-3}, {})
    assert (sp.min_p, sp.eta_cutoff) == (0.2, 6e-3)
    m.generation_config.min_p, m.generation_config.eta_cutoff = None, None
    sp = m._sampling_params(True, 1.0, None, None, None, dict(min_p=None, typical_p=1.0, epsilon_cutoff=None, eta_cutoff=0.0))
    assert not sp.warpers_armed                                                            # None and the off values: nothing armed
    for kw in (dict(typical_p=1.5), dict(min_p=2.0), dict(epsilon_cutoff=1.0), dict(eta_cutoff=-0.5)):
        with pytest.raises(ValueError):
            m._sampling_params(True, 1.0, None, None, None, kw)
    with pytest.raises(NotImplementedError):
        m._sampling_params(True, 1.0, None, None, None, dict(num_beams=2))


def test_an_engine_without_the_warpers_refuses_them():
    """the model maps a warper only for an engine that lists it: anything else is NotImplementedError, never a silent drop"""
    pytest.importorskip("torch")

    class Bare:
        device, dtype = "cpu", None
    m = _model(Bare())
    for kw in (dict(min_p=0.1), dict(typical_p=0.9), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3)):
        with pytest.raises(NotImplementedError):
            m._sampling_params(True, 1.0, None, None, None, kw)
    assert not m._sampling_params(True, 1.0, None, None, None, dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=None)).warpers_armed


def test_sampling_params_take_none_as_off():
    sp = SamplingParams(1.0, 50, 1.0, 0, None, None, None, None)
    assert (sp.min_p, sp.typical_p, sp.epsilon_cutoff, sp.eta_cutoff) == (0.0, 1.0, 0.0, 0.0) and not sp.warpers_armed
    check_sampling(1.0, 50, 1.0, None, None, None, None)
