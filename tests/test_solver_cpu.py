"""generate(solver=) on the host, without a GPU: the coefficient of the second-order multistep step (pipeline.multistep_coefficient) against a
float64 restatement written here, the three cases where it is zero, the refusals of generate() and of scheduler.step(), and inference.py's
--solver flag.

The rule (include/lx.h, lx_dpmpp2m_step): DPM-Solver++(2M) on the flow x = (1 - s) x0 + s eps is the Euler step plus c_i (D_i - D_{i-1}),
c_i = (1 - s_{i+1} / s_i) (lam_{i+1} - lam_i) / (2 (lam_i - lam_{i-1})), lam(s) = ln((1 - s) / s); c_i = 0 on the first step of a trajectory,
on the step onto s = 0 and on a step whose previous sigma is >= 1."""
import math

import numpy as np
import pytest
import torch

from tests.test_brain_cfg_cpu import Untouchable
from tests.test_inference_cli_cpu import case  # noqa: F401  (the fixture: the recorder, the stand-in model and the recorded calls)


def schedule(steps, tokens):
    """the fp32 sigmas generate() steps through for `steps` steps at `tokens` image tokens, the final 0 included (the scheduler's own)"""
    from loongx_amd.flux.pipeline import FlowMatchEulerDiscreteScheduler, calculate_shift
    sch = FlowMatchEulerDiscreteScheduler()
    cfg = sch.config
    mu = calculate_shift(tokens, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / steps, steps), device="cpu", mu=mu)
    sig = sch._sig_host
    assert sig.dtype == np.float32 and len(sig) == steps + 1 and sig[0] == 1.0 and sig[-1] == 0.0 and (np.diff(sig) < 0).all()
    return sig


def coefficient64(sig, i, begin):
    """the rule in float64, not rounded; None where it is one of the three zero cases"""
    s_prev, s, s_next = (float(sig[k]) if k >= 0 else None for k in (i - 1, i, i + 1))
    if i == begin or s_next == 0.0 or s_prev >= 1.0:
        return None
    lam = lambda t: math.log1p(-t) - math.log(t)  # noqa: E731
    h, h_prev = lam(s_next) - lam(s), lam(s) - lam(s_prev)
    return (1.0 - s_next / s) * h / (2.0 * h_prev)


@pytest.mark.parametrize("begin", [0, 2])
@pytest.mark.parametrize("steps,tokens", [(8, 1024), (28, 1024), (6, 16)])
def test_coefficient_against_float64(steps, tokens, begin):
    """relative difference <= 2^-23: the one rounding to fp32 (2^-24) and the float64 arithmetic of two differently written logarithms"""
    from loongx_amd.flux.pipeline import multistep_coefficient
    sig = schedule(steps, tokens)
    second_order = 0
    for i in range(begin, steps):
        c = multistep_coefficient(sig, i, begin)
        assert isinstance(c, float) and math.isfinite(c) and c >= 0.0 and float(np.float32(c)) == c, (i, c)
        want = coefficient64(sig, i, begin)
        if want is None:
            assert c == 0.0, (i, c)
        else:
            second_order += 1
            assert c > 0.0 and abs(c - want) <= 2.0 ** -23 * abs(want), (i, c, want)
    # a full trajectory has two Euler steps at its start (no history; sigma_0 = 1) and one at its end; one that begins later has one and one
    assert second_order == steps - begin - (3 if begin == 0 else 2)


def test_the_eight_step_values():
    from loongx_amd.flux.pipeline import multistep_coefficient
    sig = schedule(8, 1024)
    got = [round(multistep_coefficient(sig, i, 0), 4) for i in range(8)]
    assert got == [0.0, 0.0, 0.0373, 0.0604, 0.0940, 0.1573, 0.3248, 0.0], got
    # a trajectory that begins at step 2 (img2img): its first step has no history, the rest are the full trajectory's
    assert [round(multistep_coefficient(sig, i, 2), 4) for i in range(2, 8)] == [0.0] + got[3:]


def test_the_three_zero_cases():
    from loongx_amd.flux.pipeline import multistep_coefficient
    sig = schedule(6, 16)
    assert multistep_coefficient(sig, 0, 0) == 0.0 and multistep_coefficient(sig, 3, 3) == 0.0          # the first step: no history
    assert multistep_coefficient(sig, 5, 0) == 0.0 and sig[6] == 0.0                                    # the step onto sigma 0
    assert multistep_coefficient(sig, 1, 0) == 0.0 and sig[0] >= 1.0                                    # the previous sigma is 1
    assert multistep_coefficient(sig, 2, 0) > 0.0 and multistep_coefficient(sig, 4, 3) > 0.0
    # a schedule that stays at 1 for two steps: still zero, nothing divides by lam(1) = -inf
    flat = np.array([1.0, 1.0, 0.7, 0.4, 0.0], np.float32)
    assert [multistep_coefficient(flat, i, 0) for i in range(4)][:2] == [0.0, 0.0] and multistep_coefficient(flat, 2, 0) == 0.0
    assert multistep_coefficient(flat, 3, 0) == 0.0 and multistep_coefficient(np.array([0.9, 0.7, 0.4, 0.2, 0.0], np.float32), 2, 0) > 0.0


def test_the_state():
    from loongx_amd.flux.pipeline import FlowMatchEulerDiscreteScheduler, MultistepState
    st = MultistepState((2, 4, 64), "cpu")
    assert st.D.shape == (2, 4, 64) and st.D.dtype == torch.float32 and st.have is False and st.coefficients == []
    st.D.fill_(3.0)
    st.have = True
    st.coefficients.append(0.25)
    st.zero()
    assert not bool(st.D.any()) and st.have is False and st.coefficients == []
    assert FlowMatchEulerDiscreteScheduler.order == 1


def test_scheduler_step_refuses_a_state_of_another_shape_or_dtype():
    """before any launch: the ValueError comes on the host"""
    from loongx_amd.flux.pipeline import FlowMatchEulerDiscreteScheduler, MultistepState
    sch = FlowMatchEulerDiscreteScheduler()
    sch.set_timesteps(sigmas=np.linspace(1.0, 0.25, 4), device="cpu", mu=0.5)
    x1, x2 = torch.zeros(1, 4, 64), torch.zeros(2, 4, 64)
    with pytest.raises(ValueError, match="multistep"):
        sch.step(x1, 0, x1, multistep=MultistepState((2, 4, 64), "cpu"))
    with pytest.raises(ValueError, match="multistep"):              # guided: the state has one part's shape, not the batch's
        sch.step(x2, 0, x2, true_cfg_scale=2.0, multistep=MultistepState((2, 4, 64), "cpu"))
    st = MultistepState((1, 4, 64), "cpu")
    st.D = st.D.double()
    with pytest.raises(ValueError, match="multistep"):
        sch.step(x1, 0, x1, multistep=st)
    assert sch._step_index == 0 and st.have is False and st.coefficients == []


@pytest.mark.parametrize("solver", ["heun", 2, None, "", "DPMPP_2M", True, ["euler"]],
                         ids=["heun", "int", "none", "empty", "upper", "bool", "list"])
def test_generate_refuses_an_unknown_solver_before_it_touches_the_pipeline(solver):
    from loongx_amd.flux.generate import generate
    kw = dict(height=64, width=64, num_inference_steps=4, prompt_embeds=torch.zeros(2, 8, 32), pooled_prompt_embeds=torch.zeros(2, 32),
              output_type="latent", model_config={}, condition_scale=2.0, additional_condition1=torch.zeros(4, 64))
    with pytest.raises(ValueError, match="solver"):
        generate(Untouchable(), Untouchable(), solver=solver, **kw)


def test_the_keyword_is_named():
    import inspect
    from loongx_amd.flux.generate import SOLVERS, _solver, prepare_params, prepare_solver_params
    assert "solver" in inspect.signature(prepare_params).parameters
    assert prepare_solver_params(prompt="p") == "euler" and prepare_solver_params(solver="dpmpp_2m", prompt="p") == "dpmpp_2m"
    assert SOLVERS == ("euler", "dpmpp_2m") and _solver("euler") is False and _solver("dpmpp_2m") is True


# ---- inference.py --solver ---------------------------------------------------------------------------------------------------------
def _run(case, tag, **flags):  # noqa: F811
    """batch_inference as the recorded call made it; returns (the recorder's calls, the keyword names generate() received per call, the
    solver keyword of each)"""
    inf, rec, model, idir, cap, pkl, want, tmp = case
    import src.flux.generate as sg
    inner, names, given = sg.generate, [], []

    def generate(model, pipeline, **kw):
        names.append(set(kw))
        given.append({k: kw[k] for k in ("solver",) if k in kw})
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
    assert plain == want and all(g == {} for g in plain_given)
    solved, names, given = _run(case, "solver", solver="dpmpp_2m")
    assert solved == want, "the flag changed something else that reaches generate()"
    assert all(g == {"solver": "dpmpp_2m"} for g in given) and len(given) == len(plain_given) > 0
    assert [n - p for n, p in zip(names, plain_names)] == [{"solver"}] * len(names)


def test_cfg_kwargs_and_the_parser(monkeypatch, tmp_path):
    import inference as inf
    assert inf.cfg_kwargs() == {} and inf.cfg_kwargs(solver="dpmpp_2m") == {"solver": "dpmpp_2m"}
    assert inf.cfg_kwargs(2.0, solver="euler") == {"true_cfg_scale": 2.0, "solver": "euler"}
    with pytest.raises(SystemExit):
        inf.main(["--solver", "heun"])
    seen = {}

    def stop(model, input_dir, output_dir, caption_path=None, **kw):
        seen.update(kw)
    monkeypatch.setattr(inf, "load_model", lambda *a, **k: None)
    monkeypatch.setattr(inf, "batch_inference", stop)
    inf.main(["--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"), "--num_gpus", "1", "--solver", "dpmpp_2m"])
    assert seen["solver"] == "dpmpp_2m"
    seen.clear()
    inf.main(["--input_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"), "--num_gpus", "1"])
    assert seen["solver"] is None
