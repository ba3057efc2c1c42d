"""lx_euler_step_cfg validates on the host, before any launch: every refusal of include/lx.h returns LX_ERR_INVALID (-1) and names the
entry point in lx_last_error(). No GPU: the addresses are fake and aligned, and every call made here is one that must be refused, so none
is dereferenced on a machine that has a device either. The host side of the keywords that reach it
-- prepare_cfg_params and generate()'s refusals -- is here too."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

A, N = 0x100000, 1024           # x at A, [2N] floats = 0x2000 bytes; the other operands 0x10000 apart


def call(x=A, v=A + 0x10000, bf16=0, scale=2.0, x0=None, z=None, m=None, n=N):
    from loongx_amd._lib import lib
    status = lib.lx_euler_step_cfg(x, v, bf16, ctypes.c_float(-0.1), ctypes.c_float(scale), x0, z, m, ctypes.c_float(0.5), n, None)
    return status, lib.lx_last_error()


def refused(**kw):
    status, msg = call(**kw)
    return status == -1 and b"lx_euler_step_cfg" in msg


BLEND = dict(x0=A + 0x20000, z=A + 0x30000, m=A + 0x40000)


def test_the_symbol_is_exported_under_the_same_abi_version():
    from loongx_amd import _lib
    assert "lx_euler_step_cfg" in _lib.EXPORTS and hasattr(_lib.lib, "lx_euler_step_cfg") and _lib.lib.lx_version() == 404


def test_null_operands_and_an_empty_call():
    assert refused(x=None) and refused(v=None) and refused(x=None, v=None)
    assert refused(n=0) and refused(n=0, **BLEND)


@pytest.mark.parametrize("given", [("x0",), ("z",), ("m",), ("x0", "z"), ("x0", "m"), ("z", "m")])
def test_a_partly_null_blend_triple(given):
    assert refused(**{k: BLEND[k] for k in given})


@pytest.mark.parametrize("which", ["x0", "z", "m"])
@pytest.mark.parametrize("delta", [0, 4 * N, 4 * (2 * N - 1), -4 * (N - 1)], ids=["on_x", "on_the_negative_half", "last_element", "ends_on_x0"])
def test_blend_operands_on_x(which, delta):
    """[n] floats that touch x[0, 2n) anywhere: the same address, the negative half, x's last element, or ending on x's first"""
    assert refused(**dict(BLEND, **{which: A + delta}))


@pytest.mark.parametrize("delta", [0, 4 * (2 * N - 1), -4 * (2 * N - 1)])
def test_fp32_v_on_x(delta):
    assert refused(v=A + delta)


@pytest.mark.parametrize("scale", [float("nan"), float("inf"), float("-inf")])
def test_a_scale_that_is_not_finite(scale):
    assert refused(scale=scale) and refused(scale=scale, **BLEND)


def test_prepare_params_names_the_keywords_and_keeps_its_tuple():
    from loongx_amd.flux.generate import prepare_cfg_params, prepare_inpaint_params, prepare_params
    kw = dict(prompt="p", negative_prompt="n", negative_prompt_2="n2", negative_prompt_embeds="e", negative_pooled_prompt_embeds="q",
              true_cfg_scale=4.0, height=64, strength=0.25, unknown=1)
    assert len(prepare_params(**kw)) == 18 and prepare_params(**kw)[:3] == ("p", None, 64)
    assert prepare_cfg_params(**kw) == ("n", "n2", "e", "q", 4.0)
    assert prepare_cfg_params(prompt="p") == (None, None, None, None, 1.0)
    assert prepare_inpaint_params(**kw)[4] == 0.25


_pe, _pooled = torch.zeros(2, 8, 32), torch.zeros(2, 32)
HOST_ERRORS = {
    "scale_nan": dict(true_cfg_scale=float("nan"), negative_prompt_embeds=_pe, negative_pooled_prompt_embeds=_pooled),
    "scale_inf": dict(true_cfg_scale=float("inf"), negative_prompt_embeds=_pe, negative_pooled_prompt_embeds=_pooled),
    "scale_not_a_number": dict(true_cfg_scale="3", negative_prompt_embeds=_pe, negative_pooled_prompt_embeds=_pooled),
    "scale_none": dict(true_cfg_scale=None),
    "prompt_and_embeds": dict(true_cfg_scale=2.0, negative_prompt="n", negative_prompt_embeds=_pe, negative_pooled_prompt_embeds=_pooled),
    "embeds_without_pooled": dict(true_cfg_scale=2.0, negative_prompt_embeds=_pe),
    "pooled_without_embeds": dict(true_cfg_scale=2.0, negative_pooled_prompt_embeds=_pooled),
    "embeds_tokens": dict(true_cfg_scale=2.0, negative_prompt_embeds=torch.zeros(2, 9, 32), negative_pooled_prompt_embeds=_pooled),
    "embeds_width": dict(true_cfg_scale=2.0, negative_prompt_embeds=torch.zeros(2, 8, 16), negative_pooled_prompt_embeds=_pooled),
    "embeds_batch": dict(true_cfg_scale=2.0, negative_prompt_embeds=torch.zeros(3, 8, 32), negative_pooled_prompt_embeds=torch.zeros(3, 32)),
    "pooled_width": dict(true_cfg_scale=2.0, negative_prompt_embeds=_pe, negative_pooled_prompt_embeds=torch.zeros(2, 31)),
    "pooled_batch": dict(true_cfg_scale=2.0, negative_prompt_embeds=_pe, negative_pooled_prompt_embeds=torch.zeros(3, 32)),
    "prompt_list_length": dict(true_cfg_scale=2.0, negative_prompt=["a", "b", "c"]),
    "shape_checked_when_off": dict(true_cfg_scale=1.0, negative_prompt_embeds=torch.zeros(2, 9, 32), negative_pooled_prompt_embeds=_pooled),
}


@pytest.mark.parametrize("case", list(HOST_ERRORS))
def test_generate_refuses_before_it_touches_the_pipeline(case):
    """as tests/test_inpaint_cpu.py does for the inpaint keywords: the stand-in transformer has no c_factor to lose, and the scheduler is
    as new afterwards"""
    from loongx_amd.flux.generate import generate
    from loongx_amd.flux.pipeline import LxFluxPipeline
    pipe = LxFluxPipeline(SimpleNamespace(device="cpu", config=SimpleNamespace(in_channels=64, guidance_embeds=True)))
    kw = dict(height=64, width=64, num_inference_steps=4, prompt_embeds=torch.zeros(2, 8, 32), pooled_prompt_embeds=torch.zeros(2, 32),
              output_type="latent", model_config={}, condition_scale=2.0)
    kw.update(HOST_ERRORS[case])
    with pytest.raises(ValueError):
        generate(None, pipe, **kw)
    assert not hasattr(pipe.transformer, "c_factor") and pipe.scheduler.timesteps is None and pipe.scheduler._step_index is None


def test_a_batch_one_negative_is_accepted_by_the_host_check():
    from loongx_amd.flux.generate import _true_cfg
    assert _true_cfg(None, _pe[:1], _pooled[:1], 2.0, None, _pe, _pooled) is True
    assert _true_cfg(["n"], None, None, 1.5, ["a", "b"], None, None) is True
    assert _true_cfg(None, None, None, 1.0, None, _pe, _pooled) is False
    with pytest.warns(RuntimeWarning, match="without a negative prompt"):
        assert _true_cfg(None, None, None, 3.0, None, _pe, _pooled) is False
    with pytest.warns(RuntimeWarning, match="guidance is off"):
        assert _true_cfg(None, _pe, _pooled, 1.0, None, _pe, _pooled) is False


def test_scheduler_step_refuses_shapes_that_are_not_two_halves():
    """step(true_cfg_scale=...): an odd leading dimension, a model_output of another shape, or inpaint operands that are not one half's"""
    import numpy as np
    from loongx_amd.flux.pipeline import FlowMatchEulerDiscreteScheduler
    sch = FlowMatchEulerDiscreteScheduler()
    sch.set_timesteps(sigmas=np.linspace(1.0, 0.25, 4), device="cpu", mu=0.5)
    x2, x3 = torch.zeros(2, 4, 64), torch.zeros(3, 4, 64)
    half = torch.zeros(1, 4, 64)
    for bad in (dict(model_output=x3, sample=x3), dict(model_output=x2, sample=torch.zeros(4, 4, 64)),
                dict(model_output=x2, sample=x2, inpaint=(x2, x2, x2)), dict(model_output=x2, sample=x2, inpaint=(half, half, x2))):
        with pytest.raises(ValueError):
            sch.step(timestep=None, true_cfg_scale=2.0, **bad)
    assert sch._step_index == 0
