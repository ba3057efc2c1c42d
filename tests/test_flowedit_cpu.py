"""generate(source_prompt=...) on the host, without a GPU: FlowEdit's refusals (each a ValueError before anything of the pipeline is
touched, naming the keyword), its one warning, the default n_max, the coefficient rule, the state, and the scheduler's refusals before a
launch.

The coefficient (include/lx.h, lx_flowedit_step): coef = fp32((s_{i+1} - s_i in fp32) / n_avg), the quotient formed in float64 from the
fp32 difference that scheduler.step() forms, rounded once."""
import inspect
import warnings

import numpy as np
import pytest
import torch

from tests.test_brain_cfg_cpu import Untouchable
from tests.test_solver_cpu import schedule

KEYS = ("source_prompt", "source_prompt_2", "source_prompt_embeds", "source_pooled_prompt_embeds", "source_guidance_scale",
        "flowedit_n_max", "flowedit_n_avg")
PE, POOLED = torch.zeros(2, 8, 32), torch.zeros(2, 32)
SRC = dict(source_prompt_embeds=torch.zeros(1, 8, 32), source_pooled_prompt_embeds=torch.zeros(1, 32))
X = torch.zeros(2, 16, 64)


def refused(match, **kw):
    """generate() with a model and a pipeline that may not be read: a ValueError that names `match`"""
    from loongx_amd.flux.generate import generate
    base = dict(height=64, width=64, num_inference_steps=28, prompt_embeds=PE, pooled_prompt_embeds=POOLED, output_type="latent",
                model_config={}, condition_scale=2.0, additional_condition1=torch.zeros(4, 64))
    base.update(kw)
    with pytest.raises(ValueError, match=match):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # (half a guided request warns before FlowEdit refuses the pair)
            generate(Untouchable(), Untouchable(), **base)


def test_the_keywords_are_named():
    from loongx_amd.flux.generate import prepare_flowedit_params, prepare_params
    assert all(k in inspect.signature(prepare_params).parameters for k in KEYS)
    assert prepare_flowedit_params(prompt="p") == (None, None, None, None, 1.5, None, 1)
    assert prepare_flowedit_params(source_prompt="s", flowedit_n_max=3, flowedit_n_avg=2, source_guidance_scale=2.0, prompt="p") == \
        ("s", None, None, None, 2.0, 3, 2)


@pytest.mark.parametrize("T,want", [(28, 24), (6, 6), (7, 6), (14, 12), (50, 43), (1, 1), (4, 4)])
def test_the_default_n_max(T, want):
    from loongx_amd.flux.generate import _flowedit, flowedit_default_n_max
    assert flowedit_default_n_max(T) == want == T - T // 7
    assert _flowedit("a cat", None, None, 1.5, None, 1, T, None, PE, POOLED) == (want, 1)
    assert _flowedit("a cat", None, None, 1.5, 1, 3, T, None, PE, POOLED) == (1, 3)
    assert _flowedit(None, None, None, 1.5, None, 1, T, None, PE, POOLED) is None          # (no description: off)
    assert _flowedit(None, SRC["source_prompt_embeds"], SRC["source_pooled_prompt_embeds"], 0, T, 1, T, None, PE, POOLED) == (T, 1)


@pytest.mark.parametrize("n_max", [0, 29, -1, 2.0, "4", True, [4], float("nan")], ids=str)
@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
def test_a_bad_n_max(n_max, on):
    refused("flowedit_n_max", flowedit_n_max=n_max, **(dict(SRC, image_latents=X) if on else {}))


@pytest.mark.parametrize("n_avg", [0, -2, 1.0, "1", True, None, [1]], ids=str)
@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
def test_a_bad_n_avg(n_avg, on):
    refused("flowedit_n_avg", flowedit_n_avg=n_avg, **(dict(SRC, image_latents=X) if on else {}))


@pytest.mark.parametrize("scale", [True, "2", None, [2.0], float("nan"), float("inf"), float("-inf"), np.float32("nan"), -0.5, -1], ids=str)
@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
def test_a_bad_source_guidance_scale(scale, on):
    refused("source_guidance_scale", source_guidance_scale=scale, **(dict(SRC, image_latents=X) if on else {}))


def test_the_source_description():
    refused("source_prompt_embeds", source_prompt="a cat", image_latents=X, **SRC)                       # both forms
    refused("source_pooled_prompt_embeds", source_prompt_embeds=SRC["source_prompt_embeds"], image_latents=X)      # half of the pair
    refused("source_pooled_prompt_embeds", source_pooled_prompt_embeds=SRC["source_pooled_prompt_embeds"], image_latents=X)
    refused("source_prompt", source_prompt=3, image_latents=X)
    refused("source_prompt", source_prompt=["a", "b", "c"], image_latents=X)                             # three for a batch of two
    refused("source_prompt_embeds", source_prompt_embeds=torch.zeros(3, 8, 32), source_pooled_prompt_embeds=torch.zeros(3, 32),
            image_latents=X)
    refused("source_prompt_embeds", source_prompt_embeds=torch.zeros(1, 9, 32), source_pooled_prompt_embeds=torch.zeros(1, 32),
            image_latents=X)
    refused("source_pooled_prompt_embeds", source_prompt_embeds=torch.zeros(1, 8, 32), source_pooled_prompt_embeds=torch.zeros(1, 33),
            image_latents=X)


def test_a_description_without_a_source_image_and_a_strength():
    refused("image", **SRC)
    refused("image", source_prompt="a cat")
    refused("image", latent_mask=torch.ones(2, 16, 1), **SRC)
    refused("strength", strength=0.6, image_latents=X, **SRC)
    refused("strength", strength=0.0, image_latents=X, **SRC)


NEG = dict(negative_prompt_embeds=torch.zeros(1, 8, 32), negative_pooled_prompt_embeds=torch.zeros(1, 32))


@pytest.mark.parametrize("kw,match", [
    (dict(true_cfg_scale=2.0, **NEG), "true CFG"),
    (dict(brain_guidance_scale=2.0), "brain_guidance_scale"),
    (dict(apg_eta=0.5), "apg_eta"),
    (dict(apg_norm_threshold=2.0), "apg_norm_threshold"),
    (dict(apg_momentum=-0.5), "apg_momentum"),
    (dict(solver="dpmpp_2m"), "solver"),
    (dict(model_config={"step_cache_thresh": 0.3}), "step_cache_thresh"),
], ids=["true_cfg", "brain_guidance", "apg_eta", "apg_norm_threshold", "apg_momentum", "solver", "step_cache"])
def test_what_flowedit_does_not_combine_with(kw, match):
    refused(match, image_latents=X, **SRC, **kw)
    refused(match, image_latents=X, source_prompt="a cat", **kw)


def test_what_is_off_is_not_refused():
    """true_cfg_scale without a negative prompt, a negative prompt at scale 1, brain_guidance_scale 1, the default apg values, solver
    "euler" and a step cache threshold of 0 are the call without them: FlowEdit's own checks pass (the call then reaches the pipeline)"""
    from loongx_amd.flux.generate import _flowedit_alone
    for args in ((False, 1.0, None, False, {}), (False, 1, None, False, {"step_cache_thresh": 0}), (False, 0.5, None, False, None)):
        _flowedit_alone(*args, None, X, 1.0)
        _flowedit_alone(*args, object(), None, 1)
    with pytest.raises(ValueError, match="image"):
        _flowedit_alone(False, 1.0, None, False, {}, None, None, 1.0)


def test_the_guidance_vector_and_the_one_warning():
    from loongx_amd.flux.generate import _flowedit_guidance
    g = _flowedit_guidance(torch.full((2,), 5.5), 2, 1.5)
    assert g.dtype == torch.float32 and g.tolist() == [5.5, 5.5, 1.5, 1.5]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _flowedit_guidance(None, 2, 1.5) is None                       # (the default: nothing to say)
    with pytest.warns(RuntimeWarning, match="source_guidance_scale") as rec:
        assert _flowedit_guidance(None, 2, 2.0) is None
    assert len(rec) == 1


@pytest.mark.parametrize("steps,tokens", [(28, 1024), (6, 16), (16, 4096)])
@pytest.mark.parametrize("n_avg", [1, 2, 3, 7])
def test_the_coefficient_rule(steps, tokens, n_avg):
    from loongx_amd.flux.pipeline import flowedit_coefficient
    sig = schedule(steps, tokens)
    assert sig.dtype == np.float32
    for i in range(steps):
        ds32 = np.float32(sig[i + 1]) - np.float32(sig[i])
        assert ds32.dtype == np.float32
        c = flowedit_coefficient(sig, i, n_avg)
        assert isinstance(c, float) and c == float(np.float32(np.float64(ds32) / n_avg)) and c < 0.0
        assert float(np.float32(c)) == c                                       # an fp32 value: what the C ABI receives is what was recorded
        if n_avg == 1:                                                         # one forward per step: Euler's own dsigma, bit for bit
            assert c == float(ds32)
        assert abs(c * n_avg - float(ds32)) <= 2.0 ** -24 * n_avg * abs(c)


def test_the_state():
    from loongx_amd.flux.pipeline import FlowEditState
    Xs = torch.arange(2 * 4 * 64, dtype=torch.float64).view(2, 4, 64)
    m = torch.ones(2, 4, 64)
    st = FlowEditState(Xs, m, 3)
    assert st.X.dtype == st.Z.dtype == torch.float32 and st.X.is_contiguous() and st.Z.is_contiguous() and st.Z is not st.X
    assert torch.equal(st.Z, st.X) and st.mask is not None and st.n_avg == 3 and st.pending == 0 and st.taken == []
    assert st.inputs.shape == (3, 4, 4, 64) and st.inputs.dtype == torch.float32
    st.Z.fill_(3.0)
    st.taken.append((0, 1.0, -0.1))
    st.pending = 2
    st.zero()
    assert torch.equal(st.Z, st.X) and st.taken == [] and st.pending == 0
    assert FlowEditState(Xs.float()).mask is None and FlowEditState(Xs.float()).inputs.shape == (1, 4, 4, 64)
    for bad in (dict(n_avg=0), dict(n_avg=1.0), dict(n_avg=True), dict(mask=torch.ones(2, 4, 1)), dict(mask=torch.ones(1, 4, 64))):
        with pytest.raises(ValueError, match="FlowEditState"):
            FlowEditState(Xs, **bad)


def test_the_scheduler_refuses_a_mismatch_before_a_launch():
    """every ValueError comes on the host: the tensors live on the CPU, where a launch could only fail"""
    from loongx_amd.flux.pipeline import FlowEditState, FlowMatchEulerDiscreteScheduler
    sch = FlowMatchEulerDiscreteScheduler()
    st = FlowEditState(torch.zeros(1, 4, 64), None, 2)
    nz = torch.zeros(1, 4, 64)
    with pytest.raises(ValueError, match="set_timesteps"):
        sch.flowedit_inputs(st, [nz, nz])
    sch.set_timesteps(sigmas=np.linspace(1.0, 0.25, 4), device="cpu", mu=0.5)
    for noises in ([nz], [nz, nz, nz], [nz, torch.zeros(2, 4, 64)], [nz, torch.zeros(1, 4, 32)], [nz, None]):
        with pytest.raises(ValueError, match="flowedit_inputs"):
            sch.flowedit_inputs(st, noises)
    with pytest.raises(ValueError, match="flowedit_inputs"):
        sch.flowedit_inputs(object(), [nz, nz])
    v = torch.zeros(2, 4, 64)
    with pytest.raises(ValueError, match="flowedit"):                  # no inputs were formed for this step
        sch.step(v, 0, v, flowedit=st)
    st.pending = 1
    with pytest.raises(ValueError, match="flowedit_inputs"):           # a forward of the previous inputs is still to be applied
        sch.flowedit_inputs(st, [nz, nz])
    for bad in (torch.zeros(1, 4, 64), torch.zeros(2, 4, 32), torch.zeros(4, 4, 64)):
        with pytest.raises(ValueError, match="flowedit"):
            sch.step(bad, 0, bad, flowedit=st)
    for kw in (dict(inpaint=(nz, nz, nz)), dict(true_cfg_scale=2.0), dict(brain_guidance_scale=2.0), dict(multistep=object()), dict(apg=object())):
        with pytest.raises(ValueError, match="flowedit"):
            sch.step(v, 0, v, flowedit=st, **kw)
    with pytest.raises(ValueError, match="flowedit"):
        sch.step(v, 0, v, flowedit=object())
    assert sch._step_index == 0 and st.taken == [] and st.pending == 1 and not bool(st.Z.any())
    sch._step_index = 4
    st.pending = 0
    with pytest.raises(ValueError, match="flowedit_inputs"):           # past the schedule
        sch.flowedit_inputs(st, [nz, nz])


def test_get_timesteps_from():
    from loongx_amd.flux.pipeline import FlowMatchEulerDiscreteScheduler, LxFluxPipeline
    pipe = LxFluxPipeline.__new__(LxFluxPipeline)
    pipe.scheduler = FlowMatchEulerDiscreteScheduler()
    with pytest.raises(ValueError, match="set_timesteps"):
        pipe.get_timesteps_from(0)
    pipe.scheduler.set_timesteps(sigmas=np.linspace(1.0, 1 / 6, 6), device="cpu", mu=0.5)
    ts, n, th = pipe.get_timesteps_from(2)
    assert n == 4 and len(ts) == len(th) == 4 and pipe.scheduler._begin_index == pipe.scheduler._step_index == 2
    assert torch.equal(ts, pipe.scheduler.timesteps[2:]) and np.array_equal(th, pipe.scheduler.timesteps_host[2:])
    assert pipe.get_timesteps_from(0)[1] == 6 and pipe.scheduler._step_index == 0
    for bad in (6, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="get_timesteps_from"):
            pipe.get_timesteps_from(bad)
    # the strength form is the same tail: strength 0.5 of 6 steps begins at step 3
    a = pipe.get_timesteps(6, 0.5)
    b = pipe.get_timesteps_from(3)
    assert a[1] == b[1] == 3 and torch.equal(a[0], b[0]) and np.array_equal(a[2], b[2])
