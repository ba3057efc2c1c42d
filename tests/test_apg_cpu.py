"""apg_eta / apg_norm_threshold / apg_momentum on the host, without a GPU: the keywords are named (no longer among prepare_params' swallowed
kwargs), generate() refuses a bad value -- and warns about an unguided call it can already see -- before it touches the pipeline,
scheduler.step refuses an APG state without a guidance scale, and inference.py hands the flags to generate() only when given."""
import inspect
import warnings

import numpy as np
import pytest
import torch

from tests.test_brain_cfg_cpu import Untouchable
from tests.test_inference_cli_cpu import case  # noqa: F401  (the fixture: the recorder, the stand-in model and the recorded calls)

KEYS = ("apg_eta", "apg_norm_threshold", "apg_momentum")
KW = dict(height=64, width=64, num_inference_steps=4, prompt_embeds=torch.zeros(2, 8, 32), pooled_prompt_embeds=torch.zeros(2, 32),
          output_type="latent", model_config={}, condition_scale=2.0, additional_condition1=torch.zeros(4, 64))


# ---- the keywords -----------------------------------------------------------------------------------------------------------------
def test_prepare_params_names_the_keywords_and_keeps_its_tuple():
    from loongx_amd.flux.generate import prepare_apg_params, prepare_brain_cfg_params, prepare_params
    kw = dict(prompt="p", apg_eta=0.25, apg_norm_threshold=12.5, apg_momentum=-0.5, brain_guidance_scale=2.5, height=64, unknown=1)
    assert len(prepare_params(**kw)) == 18 and prepare_params(**kw)[:3] == ("p", None, 64)
    assert prepare_apg_params(**kw) == (0.25, 12.5, -0.5) and prepare_apg_params(prompt="p") == (1.0, 0.0, 0.0)
    assert prepare_brain_cfg_params(**kw) == 2.5
    assert all(k in inspect.signature(prepare_params).parameters for k in KEYS)


def test_the_rule_for_asking():
    """asked for exactly when one of the three differs from (1, 0, 0); the values come back as Python floats"""
    from loongx_amd.flux.generate import _apg
    assert _apg(1.0, 0.0, 0.0) is None and _apg(1, 0, np.float32(0.0)) is None and _apg(np.float64(1.0), -0.0, 0) is None
    assert _apg(0.0, 0.0, 0.0) == (0.0, 0.0, 0.0) and _apg(1.0, 15, 0.0) == (1.0, 15.0, 0.0) and _apg(1.0, 0.0, -0.5) == (1.0, 0.0, -0.5)
    got = _apg(np.float32(0.5), np.int64(3), np.float64(0.75))
    assert got == (0.5, 3.0, 0.75) and all(type(g) is float for g in got)
    assert _apg(0.0, 0.0, -0.999) is not None and _apg(1.0, 1e-30, 0.999) is not None


BAD = {"bool": True, "false": False, "str": "0.5", "none": None, "list": [0.5], "nan": float("nan"), "inf": float("inf"),
       "-inf": float("-inf"), "np_nan": np.float32("nan"), "complex": 0.5 + 0j}
OUTSIDE = {"apg_eta": (-0.01, 1.01, 2, -1), "apg_norm_threshold": (-1e-9, -1, np.float32(-2.0)), "apg_momentum": (1, -1, 1.0, -1.5, 7)}


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("bad", list(BAD))
def test_generate_refuses_a_bad_value_before_it_touches_the_pipeline(key, bad):
    from loongx_amd.flux.generate import generate
    with pytest.raises(ValueError, match=key):
        generate(Untouchable(), Untouchable(), **{key: BAD[bad]}, **KW)
    with pytest.raises(ValueError, match=key):                 # (guided or not: the value is checked first)
        generate(Untouchable(), Untouchable(), brain_guidance_scale=2.0, **{key: BAD[bad]}, **KW)


@pytest.mark.parametrize("key", KEYS)
def test_generate_refuses_a_value_outside_its_range_before_it_touches_the_pipeline(key):
    from loongx_amd.flux.generate import generate
    for value in OUTSIDE[key]:
        with pytest.raises(ValueError, match=key):
            generate(Untouchable(), Untouchable(), true_cfg_scale=2.0, negative_prompt_embeds=torch.zeros(2, 8, 32),
                     negative_pooled_prompt_embeds=torch.zeros(2, 32), **{key: value}, **KW)


def test_an_unguided_call_that_can_be_seen_early_warns_before_the_pipeline_is_touched():
    """no true_cfg_scale and no brain_guidance_scale: the one RuntimeWarning is out before generate() reads anything of the pipeline (the stub
    then ends the call); with the keywords at their defaults nothing warns"""
    from loongx_amd.flux.generate import generate
    with pytest.warns(RuntimeWarning, match="not guided") as rec:
        with pytest.raises(AssertionError, match="before it refused"):
            generate(Untouchable(), Untouchable(), apg_eta=0.0, apg_momentum=-0.5, **KW)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(AssertionError, match="before it refused"):
            generate(Untouchable(), Untouchable(), apg_eta=1.0, apg_norm_threshold=0, apg_momentum=0.0, **KW)
        with pytest.raises(AssertionError, match="before it refused"):      # (brain guidance asked for: whether it is on is known later)
            generate(Untouchable(), Untouchable(), apg_eta=0.0, brain_guidance_scale=2.0, **KW)


# ---- scheduler.step ---------------------------------------------------------------------------------------------------------------
def test_scheduler_step_refuses_a_state_without_a_guidance_scale():
    from loongx_amd.flux.pipeline import ApgState, FlowMatchEulerDiscreteScheduler
    sch = FlowMatchEulerDiscreteScheduler()
    sch.set_timesteps(sigmas=np.linspace(1.0, 0.25, 4), device="cpu", mu=0.5)
    state = ApgState(0.0, 0.0, -0.5, (1, 4, 64), 4, "cpu")
    assert state.M.shape == (1, 4, 64) and state.M.dtype == torch.float32 and state.sums.shape == (4, 1, 3) and state.sums.dtype == torch.float64
    assert state.workspace.numel() * state.workspace.element_size() >= 24 and state.step == 0
    x2 = torch.zeros(2, 4, 64)
    with pytest.raises(ValueError, match="true_cfg_scale and/or brain_guidance_scale"):
        sch.step(x2, None, x2, apg=state)
    with pytest.raises(ValueError, match="true_cfg_scale and/or brain_guidance_scale"):
        sch.step(x2, None, x2, inpaint=(x2, x2, x2), apg=state)
    other = ApgState(0.0, 0.0, -0.5, (2, 4, 64), 4, "cpu")           # (a state made for another shape, and one that has run out of steps)
    with pytest.raises(ValueError, match="was not made for parts of shape"):
        sch.step(x2, None, x2, true_cfg_scale=2.0, apg=other)
    state.step = 4
    with pytest.raises(ValueError, match="run out of steps"):
        sch.step(x2, None, x2, brain_guidance_scale=2.0, apg=state)
    assert sch._step_index == 0
    state.M.fill_(1.0)
    state.sums.fill_(1.0)
    state.zero()
    assert state.step == 0 and not bool(state.M.any()) and not bool(state.sums.any())


# ---- inference.py -----------------------------------------------------------------------------------------------------------------
def _run(case, tag, **flags):  # noqa: F811
    """batch_inference as the recorded call made it; returns (the recorder's calls, the keyword names generate() received per call, the APG
    and guidance keywords among them)"""
    inf, rec, model, idir, cap, pkl, want, tmp = case
    import src.flux.generate as sg
    inner, names, given = sg.generate, [], []

    def generate(model, pipeline, **kw):
        names.append(set(kw))
        given.append({k: kw[k] for k in KEYS + ("brain_guidance_scale", "true_cfg_scale", "negative_prompt") if k in kw})
        return inner(model, pipeline, **kw)
    sg.generate = generate                    # (the fixture's monkeypatch puts the module's own back)
    rec.calls = []
    try:
        inf.batch_inference(model, idir, str(tmp / tag), caption_path=cap, condition_type="subject", target_size=256, position_delta=[0, -16],
                            seed=7, brain_data_path=pkl, **flags)
    finally:
        sg.generate = inner
    return list(rec.calls), names, given


def test_the_flags_reach_generate_only_when_given(case):  # noqa: F811
    want = case[6]["batch"]["calls"]
    plain, plain_names, plain_given = _run(case, "plain")
    assert plain == want and len(plain) == 7 and all(g == {} for g in plain_given)
    one, names, given = _run(case, "eta", apg_eta=0.0)
    assert one == want, "the flag changed something else that reaches generate()"
    assert all(g == {"apg_eta": 0.0} for g in given) and [n - p for n, p in zip(names, plain_names)] == [{"apg_eta"}] * 7
    _, _, given = _run(case, "all", apg_eta=0.25, apg_norm_threshold=12.5, apg_momentum=-0.5, brain_guidance_scale=4.0)
    assert all(g == {"apg_eta": 0.25, "apg_norm_threshold": 12.5, "apg_momentum": -0.5, "brain_guidance_scale": 4.0} for g in given)
    _, _, given = _run(case, "momentum", apg_momentum=-0.5)
    assert all(g == {"apg_momentum": -0.5} for g in given) and len(given) == 7


def test_cfg_kwargs_and_the_parser(monkeypatch, tmp_path):
    import inference as inf
    assert inf.cfg_kwargs() == {} and inf.cfg_kwargs(3.0, "n", 2.0) == {"true_cfg_scale": 3.0, "negative_prompt": "n", "brain_guidance_scale": 2.0}
    assert inf.cfg_kwargs(apg_norm_threshold=0.0) == {"apg_norm_threshold": 0.0}            # (given is given, the default's value included)
    assert inf.cfg_kwargs(3.0, None, None, 0.0, 2.5, -0.5) == {"true_cfg_scale": 3.0, "apg_eta": 0.0, "apg_norm_threshold": 2.5, "apg_momentum": -0.5}
    for flag in KEYS:
        with pytest.raises(SystemExit):
            inf.main([f"--{flag}", "much"])
        with pytest.raises(SystemExit):                   # (a synthetic run passes no keywords through)
            inf.main(["--synthetic", f"--{flag}", "0.5"])
    seen = {}

    def stop(model, input_dir, output_dir, caption_path=None, **kw):
        seen.update(kw)
    monkeypatch.setattr(inf, "load_model", lambda *a, **k: None)
    monkeypatch.setattr(inf, "batch_inference", stop)
    base = ["--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"), "--num_gpus", "1"]
    inf.main(base + ["--apg_eta", "0", "--apg_momentum", "-0.5", "--brain_guidance_scale", "4"])
    assert (seen["apg_eta"], seen["apg_norm_threshold"], seen["apg_momentum"], seen["brain_guidance_scale"]) == (0.0, None, -0.5, 4.0)
    seen.clear()
    inf.main(base)
    assert all(seen[k] is None for k in KEYS)
