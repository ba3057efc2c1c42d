"""brain_guidance_scale on the host, without a GPU: the keyword is named (no longer among prepare_params' swallowed kwargs), generate()
refuses a bad scale before it touches the pipeline, scheduler.step refuses a batch that is not three parts, lx_euler_step_cfg3 validates
before any launch -- every refusal of include/lx.h returns LX_ERR_INVALID (-1) and names the entry point in lx_last_error(); the addresses
are fake and aligned, and every call made here is one that must be refused, so none is dereferenced -- and inference.py hands the flag to
generate() only when given."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tests.test_inference_cli_cpu import case  # noqa: F401  (the fixture: the recorder, the stand-in model and the recorded calls)

A, N = 0x100000, 1024           # x at A, [3N] floats = 0x3000 bytes; the other operands 0x10000 apart


def call(x=A, v=A + 0x10000, bf16=0, scale_brain=2.0, scale_text=3.0, x0=None, z=None, m=None, n=N):
    from loongx_amd._lib import lib
    status = lib.lx_euler_step_cfg3(x, v, bf16, ctypes.c_float(-0.1), ctypes.c_float(scale_brain), ctypes.c_float(scale_text), x0, z, m,
                                    ctypes.c_float(0.5), n, None)
    return status, lib.lx_last_error()


def refused(**kw):
    status, msg = call(**kw)
    return status == -1 and b"lx_euler_step_cfg3" in msg


BLEND = dict(x0=A + 0x20000, z=A + 0x30000, m=A + 0x40000)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_under_the_same_abi_version():
    from loongx_amd import _lib
    assert "lx_euler_step_cfg3" in _lib.EXPORTS and hasattr(_lib.lib, "lx_euler_step_cfg3") and _lib.lib.lx_version() == 404


def test_null_operands_and_an_empty_call():
    assert refused(x=None) and refused(v=None) and refused(x=None, v=None)
    assert refused(n=0) and refused(n=0, **BLEND)


@pytest.mark.parametrize("given", [("x0",), ("z",), ("m",), ("x0", "z"), ("x0", "m"), ("z", "m")])
def test_a_partly_null_blend_triple(given):
    assert refused(**{k: BLEND[k] for k in given})


@pytest.mark.parametrize("which", ["x0", "z", "m"])
@pytest.mark.parametrize("delta", [0, 4 * N, 4 * 2 * N, 4 * (3 * N - 1), -4 * (N - 1)],
                         ids=["on_x", "on_the_text_part", "on_the_negative_part", "last_element", "ends_on_x0"])
def test_blend_operands_on_x(which, delta):
    """[n] floats that touch x[0, 3n) anywhere: the same address, the second or third part, x's last element, or ending on x's first"""
    assert refused(**dict(BLEND, **{which: A + delta}))


def test_blend_operands_next_to_x_are_not_what_is_refused():
    """the overlap test is exact: [n] floats that end where x begins, or begin where x[3n) ends, pass it -- shown on a call that is refused
    for another reason (n stays > 0 and no launch is made), by the message naming that reason"""
    for delta in (-4 * N, 4 * 3 * N):
        status, msg = call(scale_brain=float("nan"), **dict(BLEND, x0=A + delta))
        assert status == -1 and b"not finite" in msg


@pytest.mark.parametrize("delta", [0, 4 * (3 * N - 1), -4 * (3 * N - 1)])
def test_fp32_v_on_x(delta):
    assert refused(v=A + delta)


@pytest.mark.parametrize("scale", [float("nan"), float("inf"), float("-inf")])
def test_a_scale_that_is_not_finite(scale):
    assert refused(scale_brain=scale) and refused(scale_text=scale) and refused(scale_brain=scale, **BLEND) and refused(scale_text=scale, **BLEND)


# ---- the keyword ------------------------------------------------------------------------------------------------------------------
def test_prepare_params_names_the_keyword_and_keeps_its_tuple():
    from loongx_amd.flux.generate import prepare_brain_cfg_params, prepare_cfg_params, prepare_params
    kw = dict(prompt="p", brain_guidance_scale=2.5, true_cfg_scale=4.0, height=64, unknown=1)
    assert len(prepare_params(**kw)) == 18 and prepare_params(**kw)[:3] == ("p", None, 64)
    assert prepare_brain_cfg_params(**kw) == 2.5 and prepare_brain_cfg_params(prompt="p") == 1.0
    assert prepare_cfg_params(**kw)[4] == 4.0
    import inspect
    assert "brain_guidance_scale" in inspect.signature(prepare_params).parameters


class Untouchable:
    """a pipeline (and a model) of which a refused call may read or set nothing"""

    def __getattr__(self, name):
        raise AssertionError(f"generate() read .{name} before it refused the call")

    def __setattr__(self, name, value):
        raise AssertionError(f"generate() set .{name} before it refused the call")


@pytest.mark.parametrize("scale", [True, False, "2", None, [2.0], float("nan"), float("inf"), float("-inf"), np.float32("nan"), -0.5, -1],
                         ids=["true", "false", "str", "none", "list", "nan", "inf", "-inf", "np_nan", "-0.5", "-1"])
def test_generate_refuses_a_bad_scale_before_it_touches_the_pipeline(scale):
    from loongx_amd.flux.generate import generate
    kw = dict(height=64, width=64, num_inference_steps=4, prompt_embeds=torch.zeros(2, 8, 32), pooled_prompt_embeds=torch.zeros(2, 32),
              output_type="latent", model_config={}, condition_scale=2.0, additional_condition1=torch.zeros(4, 64))
    with pytest.raises(ValueError, match="brain_guidance_scale"):
        generate(Untouchable(), Untouchable(), brain_guidance_scale=scale, **kw)


def test_the_scale_rule():
    from loongx_amd.flux.generate import _brain_cfg
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _brain_cfg(1.0) is False and _brain_cfg(1) is False
        assert _brain_cfg(2.0) is True and _brain_cfg(np.float32(1.5)) is True and _brain_cfg(3) is True
    for off in (0, 0.0, 0.5, np.float64(0.999)):
        with pytest.warns(RuntimeWarning, match="guidance is off") as rec:
            assert _brain_cfg(off) is False
        assert len(rec) == 1


# ---- scheduler.step ---------------------------------------------------------------------------------------------------------------
def test_scheduler_step_refuses_shapes_that_are_not_the_branches():
    """step(true_cfg_scale=, brain_guidance_scale=): a leading dimension that is no multiple of 3, a model_output of another shape, or
    inpaint operands that are not one part's; step(brain_guidance_scale=) alone: the same with halves; and a scale that is not > 1"""
    from loongx_amd.flux.pipeline import FlowMatchEulerDiscreteScheduler
    sch = FlowMatchEulerDiscreteScheduler()
    sch.set_timesteps(sigmas=np.linspace(1.0, 0.25, 4), device="cpu", mu=0.5)
    x2, x3, x4 = torch.zeros(2, 4, 64), torch.zeros(3, 4, 64), torch.zeros(4, 4, 64)
    part = torch.zeros(1, 4, 64)
    for bad in (dict(model_output=x2, sample=x2), dict(model_output=x4, sample=x4), dict(model_output=x3, sample=torch.zeros(6, 4, 64)),
                dict(model_output=torch.zeros(0, 4, 64), sample=torch.zeros(0, 4, 64)),
                dict(model_output=x3, sample=x3, inpaint=(x3, x3, x3)), dict(model_output=x3, sample=x3, inpaint=(part, part, x3))):
        with pytest.raises(ValueError, match="multiple of 3|latents' shape"):
            sch.step(timestep=None, true_cfg_scale=2.0, brain_guidance_scale=2.0, **bad)
    for bad in (dict(model_output=x3, sample=x3), dict(model_output=x2, sample=x4), dict(model_output=x2, sample=x2, inpaint=(x2, x2, x2))):
        with pytest.raises(ValueError, match="even leading dimension|latents' shape"):
            sch.step(timestep=None, brain_guidance_scale=2.0, **bad)
    for s_b in (1.0, 0.5, float("nan")):                    # (the three-branch launch is never made with s_b <= 1)
        with pytest.raises(ValueError, match="must be > 1"):
            sch.step(x3, None, x3, true_cfg_scale=2.0, brain_guidance_scale=s_b)
    assert sch._step_index == 0


# ---- inference.py -----------------------------------------------------------------------------------------------------------------
def _run(case, tag, **flags):  # noqa: F811
    """batch_inference as the recorded call made it; returns (the recorder's calls, the keyword names generate() received per call)"""
    inf, rec, model, idir, cap, pkl, want, tmp = case
    import src.flux.generate as sg
    inner, names, given = sg.generate, [], []

    def generate(model, pipeline, **kw):
        names.append(set(kw))
        given.append({k: kw[k] for k in ("brain_guidance_scale", "true_cfg_scale", "negative_prompt") if k in kw})
        return inner(model, pipeline, **kw)
    sg.generate = generate                    # (the fixture's monkeypatch puts the module's own back)
    rec.calls = []
    try:
        inf.batch_inference(model, idir, str(tmp / tag), caption_path=cap, condition_type="subject", target_size=256, position_delta=[0, -16],
                            seed=7, brain_data_path=pkl, **flags)
    finally:
        sg.generate = inner
    return list(rec.calls), names, given


def test_the_flag_reaches_generate_only_when_given(case):  # noqa: F811
    want = case[6]["batch"]["calls"]
    plain, plain_names, plain_given = _run(case, "plain")
    assert plain == want and len(plain) == 7
    assert all(g == {} for g in plain_given)
    guided, names, given = _run(case, "brain", brain_guidance_scale=2.5)
    assert guided == want, "the flag changed something else that reaches generate()"
    assert all(g == {"brain_guidance_scale": 2.5} for g in given) and len(given) == 7
    assert [n - p for n, p in zip(names, plain_names)] == [{"brain_guidance_scale"}] * 7
    _, _, both = _run(case, "both", brain_guidance_scale=1.5, true_cfg_scale=2.0, negative_prompt="blurry")
    assert all(g == {"brain_guidance_scale": 1.5, "true_cfg_scale": 2.0, "negative_prompt": "blurry"} for g in both)


def test_cfg_kwargs_and_the_parser(monkeypatch, tmp_path):
    import inference as inf
    assert inf.cfg_kwargs() == {} and inf.cfg_kwargs(None, None, None) == {}
    assert inf.cfg_kwargs(brain_guidance_scale=2.0) == {"brain_guidance_scale": 2.0}
    assert inf.cfg_kwargs(3.0, "n", 2.0) == {"true_cfg_scale": 3.0, "negative_prompt": "n", "brain_guidance_scale": 2.0}
    with pytest.raises(SystemExit):
        inf.main(["--brain_guidance_scale", "much"])
    with pytest.raises(SystemExit):                       # (a synthetic run passes no keywords through)
        inf.main(["--synthetic", "--brain_guidance_scale", "2.0"])
    seen = {}

    def stop(model, input_dir, output_dir, caption_path=None, **kw):
        seen.update(kw)
    monkeypatch.setattr(inf, "load_model", lambda *a, **k: None)
    monkeypatch.setattr(inf, "batch_inference", stop)
    inf.main(["--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"), "--num_gpus", "1", "--brain_guidance_scale", "2.5"])
    assert seen["brain_guidance_scale"] == 2.5 and seen["true_cfg_scale"] is None
    seen.clear()
    inf.main(["--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"), "--num_gpus", "1"])
    assert seen["brain_guidance_scale"] is None
