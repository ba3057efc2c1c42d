"""Named LoRA adapters on the engine: the stacked image of the active set, per-adapter and per-image weights (lx_lora_scale_rows on the
adapter scratch), switching, and the pipeline / generate surface. Tiny model (D = 256), B = 2, the inputs of tests/test_lora_wide_gpu.py;
the adapters are the slices [0:4] ("a") and [4:16] ("b") of its rank-16 set (tests/test_lora_adapters_cpu.py), the oracle the unmodified
oracle.flux_modules.LoraLinear with both adapters active and a scaling each."""
import inspect
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import relerr  # noqa: E402
from tests.test_engine_gpu import TOL  # noqa: E402
from tests.test_lora_adapters_cpu import AB, base_sd, lora_slice, packed_with, split_oracle_out  # noqa: E402
from tests.test_lora_rank_cpu import _cfg  # noqa: E402
from tests.test_lora_wide_gpu import _inputs, condition, forward, make_engine, oracle_out, rank_model  # noqa: E402
from tests.test_precise_gpu import TOL_P  # noqa: E402

DEV = "cuda"
AB4 = [("a", 0, 2), ("b", 2, 4)]             # the 2 + 2 split of the rank-4 set (precise mode: 4 modules x 4 = one 16-column slab)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


def adapter_engine(parts=AB, r=16, precise=False, active=None):
    from loongx_amd.flux.engine import DiTEngine
    eng = DiTEngine(packed_with(r, parts, precise=precise, device=DEV), DEV)
    eng.precise_default = precise
    if active is not None:
        eng.set_adapters(active)
    return eng


_ORACLE = {}


def weighted_oracle(r, parts, scalings, mc):
    key = (r, tuple(parts), tuple(sorted(scalings.items())), tuple(sorted(mc.items())))
    if key not in _ORACLE:
        _ORACLE[key] = split_oracle_out(r, parts, scalings, mc)
    return _ORACLE[key]


_STACKED = {}


def stacked_forward(operands):
    """The forward of the engine packed with the whole rank-16 set, per operand format (computed once)."""
    if operands not in _STACKED:
        eng = make_engine(16)
        condition(eng, {"operands": operands})
        _STACKED[operands] = forward(eng)
    return _STACKED[operands]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_unit_weights_are_the_stacked_model(ops, operands):
    eng = adapter_engine(active=["a", "b"])
    assert eng.cfg.lora_r == 16
    condition(eng, {"operands": operands})
    assert eng.lora_w is None
    eng.use_graph = False
    eager = forward(eng)
    eng.use_graph = True
    captured, replayed = forward(eng), forward(eng)
    want = stacked_forward(operands)
    assert torch.equal(eager, want) and torch.equal(captured, want) and torch.equal(replayed, want)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("operands", ["bf16", "fp16"])
@pytest.mark.parametrize("mc", [{}, {"latent_lora": True}, {"independent_condition": True}, {"attn_fp8": True}])
def test_scalar_weights_against_the_oracle(ops, mc, operands):
    eng = adapter_engine()
    eng.set_adapters(["a", "b"], {"a": 0.5, "b": 2.0})
    condition(eng, dict(mc, operands=operands))
    assert eng.lora_w is not None and eng.lora_w.shape == (2, 16)
    a = forward(eng)
    b = forward(eng)                            # captured / replayed (with independent_condition: the cached condition stream)
    omc = {k: v for k, v in mc.items() if k != "attn_fp8"}
    want = weighted_oracle(16, AB, {"a": 0.5, "b": 2.0}, omc)
    ea, eb = relerr(a, want), relerr(b, want)
    print(f"weights (0.5, 2.0) {mc} {operands}: relerr eager {ea:.3e} replay {eb:.3e}")
    bound = 7e-2 if mc.get("attn_fp8") else TOL
    assert ea < bound and eb < bound, (ea, eb)
    assert relerr(a, oracle_out(16, omc)) > 1e-3              # the weights matter


def test_scalar_weights_in_precise_mode(ops):
    eng = adapter_engine(AB4, r=4, precise=True)
    eng.set_adapters(["a", "b"], {"a": 0.5, "b": 2.0})
    condition(eng, {})
    assert eng.precise and eng.lora_w is not None and eng.lora_w.shape == (2, 4)
    a, b = forward(eng), forward(eng)
    want = weighted_oracle(4, AB4, {"a": 0.5, "b": 2.0}, {})
    ea, eb = relerr(a, want), relerr(b, want)
    print(f"precise, weights (0.5, 2.0): relerr eager {ea:.3e} replay {eb:.3e}")
    assert ea < TOL_P and eb < TOL_P, (ea, eb)
    assert relerr(a, oracle_out(4, {})) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("mc", [{}, {"latent_lora": True}])
def test_per_image_weights(ops, mc):
    eng = adapter_engine()
    eng.set_adapters(["a", "b"], {"a": [1.0, 0.0], "b": torch.tensor([0.0, 1.0])})
    condition(eng, mc)
    got = forward(eng)
    replay = forward(eng)
    only_a, only_b = weighted_oracle(16, AB, {"a": 1.0, "b": 0.0}, mc), weighted_oracle(16, AB, {"a": 0.0, "b": 1.0}, mc)
    for out in (got, replay):
        e0, e1 = relerr(out[0], only_a[0]), relerr(out[1], only_b[1])
        print(f"per-image weights {mc}: image 0 {e0:.3e} image 1 {e1:.3e}")
        assert e0 < TOL and e1 < TOL, (e0, e1)
    eng.set_adapter_weights({"a": 0.5, "b": 0.5})
    assert not eng.cond_ready
    condition(eng, mc)
    assert relerr(got, forward(eng)) > 1e-3


def test_per_image_weights_of_another_length_are_refused(ops):
    eng = adapter_engine(active=["a", "b"])
    condition(eng, {})
    want = forward(eng)
    eng.set_adapter_weights({"a": [1.0, 0.5, 0.25]})
    with pytest.raises(ValueError, match="3 per-image weights for a batch of 2"):
        condition(eng, {})
    assert not eng.cond_ready
    eng.set_adapter_weights({})
    condition(eng, {})
    assert torch.equal(forward(eng), want)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("mc", [{}, {"independent_condition": True}])
@pytest.mark.parametrize("operands", ["bf16", "fp16"])
def test_switching_adapters(ops, operands, mc):
    mc = dict(mc, operands=operands)
    fresh = {}
    for name, lo, hi in AB:
        e = adapter_engine([(name, lo, hi)])
        condition(e, mc)
        fresh[name] = forward(e)
    assert relerr(fresh["a"], fresh["b"]) > 1e-3
    eng = adapter_engine()
    images = None
    for name in ("a", "b", "a"):
        eng.set_adapters(name)
        condition(eng, mc)
        first, second = forward(eng), forward(eng)              # (the second: replayed, with independent_condition from the condition cache)
        assert torch.equal(first, fresh[name]) and torch.equal(second, fresh[name]), f"after switching to {name!r}"
        if operands == "fp16":
            now = {k: v.data_ptr() for k, v in eng.w16.items() if not k.endswith(".down")}
            assert len(now) > 8 and (images is None or now == images), "a switch of adapters rebuilt the fp16 weight images"
            images = now
            assert sorted(k for k in eng.w16 if k.endswith(".down")) == sorted(k + ".down" for k in eng.w.lora)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_the_default_path_launches_nothing_new(ops, monkeypatch):
    from loongx_amd.flux.engine import DiTEngine
    calls = []
    real = ops.lora_scale_rows
    monkeypatch.setattr(ops, "lora_scale_rows", lambda T, *a, **k: (calls.append(tuple(T.shape)), real(T, *a, **k))[1])
    eng = adapter_engine([("a", 0, 4)])
    for mc in ({}, {"latent_lora": True}):
        condition(eng, mc)
        eng.use_graph = False
        forward(eng)
        eng.use_graph = True
        forward(eng), forward(eng)
    assert calls == [] and eng.lora_w is None
    eng = adapter_engine()
    eng.set_adapters(["a", "b"], {"a": 0.5, "b": 2.0})
    condition(eng, {"latent_lora": True})
    n0 = len(calls)
    assert n0 > 0                                                # the conditioning: x_embedder's and the modulations' scratch
    eng.use_graph = False
    forward(eng)
    assert len(calls) > n0
    # no torch arithmetic on the adapter scratch is left beside the kernel
    src = inspect.getsource(DiTEngine)
    assert "mul_(self.lora_scale)" not in src and ".mul_(" not in src


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("mc", [{}, {"latent_lora": True}])
def test_lora_scale_multiplies_on_top_of_the_weights(ops, mc):
    from types import SimpleNamespace
    from loongx_amd.flux.lora_controller import set_lora_scale
    eng = adapter_engine()
    eng.set_adapters(["a", "b"], {"a": 0.5, "b": 0.5})
    condition(eng, mc)
    want = forward(eng)
    eng.set_adapters(["a", "b"], {"a": 1.0, "b": 1.0})
    with set_lora_scale([SimpleNamespace(engine=eng)], 0.5):
        condition(eng, mc)
        assert torch.equal(forward(eng), want)                  # the same table entries
    assert eng.lora_scale == 1.0 and not eng.cond_ready


def test_gemm_fp8_keeps_lora_scale_in_the_e4m3_down_projection(ops):
    """gemm_fp8: lx_lora_down_fp8 takes lora_scale with its descale and the table (without lora_scale) comes on top. 0.5 is a power of
    two, so (x . descale) . 0.5 and x . (0.5 descale) are the same bits: weights (0.5, 0.5) at scale 1 equal weights (1, 1) at scale 0.5."""
    eng = adapter_engine(AB4, r=4)
    mc = {"gemm_fp8": True}
    eng.set_adapters(["a", "b"])
    condition(eng, mc)
    assert eng.gemm_fp8 and eng.lora_w is None and eng.lora_w_ns is None
    unit = forward(eng)
    eng.set_adapters(["a", "b"], {"a": 0.5, "b": 0.5})
    condition(eng, mc)
    assert eng.lora_w is not None and eng.lora_w_ns is not None
    want = forward(eng)
    assert torch.equal(forward(eng), want) and not torch.equal(want, unit)          # (replay; and the weights take effect)
    eng.set_adapters(["a", "b"], {})
    eng.set_lora_scale(0.5)
    condition(eng, mc)
    assert eng.lora_w is not None and eng.lora_w_ns is None
    assert torch.equal(forward(eng), want)


# ---------------------------------------------------------------------------------------------------------------- 7
def _pipe():
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    tr, sd, _ = rank_model(16)
    return LxFluxPipeline(LxFluxTransformer.from_state_dict(base_sd(sd), _cfg(tr), DEV))


def _generate(pipe, ctype, default_lora):
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    kw, cond, _ = _inputs()
    hw = 8
    c = Condition(ctype, latents=cond.to(DEV), latent_hw=(hw, hw), position_delta=[0, -hw])
    return generate(None, pipe, conditions=[c], height=hw * 16, width=hw * 16, num_inference_steps=2, latents=kw["hidden_states"].to(DEV),
                    prompt_embeds=kw["encoder_hidden_states"].to(DEV), pooled_prompt_embeds=kw["pooled_projections"].to(DEV),
                    output_type="latent", model_config={}, default_lora=default_lora, use_brain_condition=False).images.float().cpu()


def test_pipeline_and_generate_select_adapters_by_name(ops, tmp_path):
    from safetensors.torch import save_file
    sd = rank_model(16)[1]
    for name, (lo, hi) in (("subject", (0, 4)), ("canny", (4, 16))):
        (tmp_path / name).mkdir()
        save_file(lora_slice(sd, lo, hi), str(tmp_path / name / "pytorch_lora_weights.safetensors"))
    pipe = _pipe()
    assert pipe.get_list_adapters() == {"transformer": []} and pipe.get_active_adapters() == []
    assert pipe.load_lora_weights(str(tmp_path / "subject"), adapter_name="subject") == 25
    assert pipe.load_lora_weights(str(tmp_path / "canny"), adapter_name="canny") == 25
    assert pipe.get_list_adapters() == {"transformer": ["subject", "canny"]} and pipe.get_active_adapters() == ["subject"]
    pipe.set_adapters("subject")
    want = _generate(pipe, "subject", default_lora=True)
    pipe.set_adapters("canny")
    assert pipe.get_active_adapters() == ["canny"]
    canny = _generate(pipe, "subject", default_lora=True)
    got = _generate(pipe, "subject", default_lora=False)          # selects "subject" itself
    assert pipe.get_active_adapters() == ["subject"]
    assert torch.equal(got, want) and relerr(got, canny) > 1e-3
    with pytest.raises(ValueError, match=r"'coloring'.*\['subject', 'canny'\]"):
        _generate(pipe, "coloring", default_lora=False)
    assert pipe.get_active_adapters() == ["subject"]
    with pytest.raises(ValueError, match=r"'nope'.*\['subject', 'canny'\]"):
        pipe.set_adapters(["subject", "nope"])
    # weights through the pipeline: a float for all, one item per name, per-image items
    pipe.set_adapters(["subject", "canny"], [0.5, [1.0, 0.0]])
    eng = pipe.transformer.engine
    assert eng.adapter_weights == {"subject": 0.5, "canny": (1.0, 0.0)} and eng.cfg.lora_r == 16
    mixed = _generate(pipe, "subject", default_lora=True)
    assert relerr(mixed, want) > 1e-3
    with pytest.raises(ValueError, match="3 adapter weights for 2 adapters"):
        pipe.set_adapters(["subject", "canny"], [1.0, 1.0, 1.0])
    pipe.delete_adapters("canny")
    assert pipe.get_list_adapters() == {"transformer": ["subject"]} and pipe.get_active_adapters() == ["subject"]
    pipe.set_adapters("subject")
    assert torch.equal(_generate(pipe, "subject", default_lora=True), want)


def test_generate_keeps_a_single_unnamed_adapter(ops, tmp_path):
    from safetensors.torch import save_file
    from loongx_amd.flux import generate as gen
    sd = rank_model(16)[1]
    save_file(lora_slice(sd, 0, 4), str(tmp_path / "pytorch_lora_weights.safetensors"))
    pipe = _pipe()
    assert pipe.load_lora_weights(str(tmp_path)) == 25
    assert pipe.get_list_adapters() == {"transformer": ["default"]}
    want = _generate(pipe, "subject", default_lora=True)
    gen._UNNAMED_ADAPTER_WARNED = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = _generate(pipe, "subject", default_lora=False)
        again = _generate(pipe, "subject", default_lora=False)
    assert torch.equal(got, want) and torch.equal(again, want)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning) and "default" in str(w.message)]) == 1
