"""The step cache without a GPU: lx_ln_modulate_delta validates on the host, before any launch (every refusal of include/lx.h returns
LX_ERR_INVALID (-1) and names the entry point; the addresses are fake and aligned, and every call made here is one that must be refused, so
none is dereferenced on a machine that has a device either); the host rule of loongx_amd/flux/step_cache.py against sequences worked out by
hand; and the model_config keys as generate() and a YAML file hand them over."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

A = 0x100000                     # X; the other operands 0x100000 apart: far more than M * ld * 4 bytes
GOOD = dict(X=A, ldx=260, shift=A + 0x100000, scale=A + 0x200000, mod_ld=1544, P=A + 0x300000, ldp=264, M=8, D=256, rpb=4,
            row_sums=A + 0x400000, sums=A + 0x500000)


def call(**over):
    from loongx_amd._lib import lib
    a = dict(GOOD, **over)
    status = lib.lx_ln_modulate_delta(a["X"], a["ldx"], a["shift"], a["scale"], a["mod_ld"], a["P"], a["ldp"], a["M"], a["D"], a["rpb"],
                                      ctypes.c_float(1e-6), a["row_sums"], a["sums"], None)
    return status, lib.lx_last_error()


def refused(**over):
    status, msg = call(**over)
    return status == -1 and b"lx_ln_modulate_delta" in msg


def test_the_symbol_is_exported_under_the_same_abi_version():
    from loongx_amd import _lib
    assert "lx_ln_modulate_delta" in _lib.EXPORTS and hasattr(_lib.lib, "lx_ln_modulate_delta") and _lib.lib.lx_version() == 404


@pytest.mark.parametrize("which", ["X", "shift", "scale", "P", "row_sums", "sums"])
def test_null_pointers(which):
    assert refused(**{which: None})


@pytest.mark.parametrize("over", [dict(M=0), dict(M=-3), dict(D=0), dict(D=-4), dict(rpb=0), dict(rpb=-1)])
def test_counts_that_are_not_positive(over):
    assert refused(**over)


@pytest.mark.parametrize("over", [dict(D=254, ldx=256, ldp=256), dict(D=16388, ldx=16388, ldp=16388, mod_ld=16388), dict(D=16640, ldx=16640, ldp=16640, mod_ld=16640)])
def test_row_widths_the_kernel_does_not_take(over):
    assert refused(**over)


@pytest.mark.parametrize("which", ["ldx", "ldp", "mod_ld"])
@pytest.mark.parametrize("value", [258, 252, 0, -260])
def test_leading_dimensions(which, value):
    """not a multiple of 4, or smaller than D"""
    assert refused(**{which: value})


@pytest.mark.parametrize("delta", [0, 1008, 8288, -8400, 4000])
def test_p_on_x(delta):
    """P [8, 264] floats (8416 bytes) that touch X [8, 260] (8304 bytes) anywhere: the same address, inside row 0, X's last 16 bytes, ending
    16 bytes into X, in between (all 16-byte aligned: the overlap is what is refused)"""
    status, msg = call(P=A + delta)
    assert status == -1 and b"lx_ln_modulate_delta: P may not overlap X" in msg


# ------------------------------------------------------------------------------------------------------------------ the host rule
def run_rule(indices, n, rels, thresh, coefficients):
    from loongx_amd.flux.step_cache import StepCacheState
    st = StepCacheState(thresh, coefficients)
    out = [st.step(i, n, None if i == 0 else r) for i, r in zip(indices, rels)]
    return out, st.report()


def test_first_and_last_step_are_forced():
    out, rep = run_rule(range(5), 5, [None, 0.0, 0.0, 0.0, 0.0], 1.0, (1.0, 0.0))
    assert out == [True, False, False, False, True]
    assert rep["computed"] == [0, 4] and rep["steps"] == 5 and rep["rel"] == [None, 0.0, 0.0, 0.0, 0.0] and rep["acc"] == [0.0] * 5


def test_identity_coefficients_accumulate_and_reset():
    """thresh 0.5, raw distances: 0.2 -> acc 0.2 skip; 0.2 -> 0.4 skip; 0.2 -> 0.6000000000000001 >= 0.5 compute, acc 0; 0.3 skip; 0.1 -> 0.4
    skip; 0.1 -> 0.5 >= 0.5 compute; then the last step"""
    rels = [None, 0.2, 0.2, 0.2, 0.3, 0.1, 0.1, 0.0]
    out, rep = run_rule(range(8), 8, rels, 0.5, (1.0, 0.0))
    assert out == [True, False, False, True, False, False, True, True]
    assert rep["acc"] == [0.0, 0.2, 0.4, 0.0, 0.3, 0.4, 0.0, 0.0] and rep["computed"] == [0, 3, 6, 7]
    assert rep["thresh"] == 0.5 and rep["coefficients"] == (1.0, 0.0)


def test_cubic_coefficients():
    """poly(r) = 8 r^3 - 2 r + 0.5: poly(0.5) = 0.5, poly(0.25) = 0.125, poly(1) = 6.5"""
    c = (8.0, 0.0, -2.0, 0.5)
    assert [float(np.poly1d(c)(r)) for r in (0.5, 0.25, 1.0)] == [0.5, 0.125, 6.5]
    out, rep = run_rule(range(6), 6, [None, 0.5, 0.25, 0.25, 1.0, 0.5], 0.75, c)
    # 0.5 skip; 0.625 skip; 0.75 >= 0.75 compute; 6.5 compute; last
    assert out == [True, False, False, True, True, True]
    assert rep["acc"] == [0.0, 0.5, 0.625, 0.0, 0.0, 0.0]


def test_a_jump_in_the_index_forces_a_compute():
    out, rep = run_rule([0, 1, 2, 4, 5, 3, 4], 9, [None, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], 1.0, (1.0, 0.0))
    assert out == [True, False, False, True, False, True, False]
    assert rep["indices"] == [0, 1, 2, 4, 5, 3, 4] and rep["computed"] == [0, 4, 3]
    # a repeated index is a jump too, and so is a first call that is not step 0
    assert run_rule([0, 1, 1], 9, [None, 0.0, 0.0], 1.0, (1.0, 0.0))[0] == [True, False, True]
    assert run_rule([3, 4], 9, [0.0, 0.0], 1.0, (1.0, 0.0))[0] == [True, False]


def test_decide_is_the_rule_in_one_function():
    from loongx_amd.flux.step_cache import decide
    p = np.poly1d((1.0, 0.0))
    assert decide(0, 4, None, 0.3, None, 1.0, p) == (True, 0.0)
    assert decide(3, 4, 2, 0.0, 0.0, 1.0, p) == (True, 0.0)
    assert decide(2, 4, 0, 0.0, 0.0, 1.0, p) == (True, 0.0)
    assert decide(2, 4, 1, 0.25, 0.5, 1.0, p) == (False, 0.75)
    assert decide(2, 4, 1, 0.5, 0.5, 1.0, p) == (True, 0.0)                   # acc + poly(rel) == thresh computes
    assert decide(2, 4, 1, 0.0, float("inf"), 1.0, p) == (True, 0.0)
    assert decide(2, 4, 1, 0.0, float("nan"), 1.0, p) == (True, 0.0)          # (a distance that is no number never skips)
    assert decide(1, 3, 0, 0.0, 1.0, 1e30, p) == (False, 1.0) and decide(1, 3, 0, 0.0, 0.0, 1e-30, p) == (False, 0.0)


# ------------------------------------------------------------------------------------------------------------------ the keys
def test_config_on_and_off():
    from loongx_amd.flux.step_cache import DEFAULT_COEFFICIENTS, step_cache_config
    assert step_cache_config(None) is None and step_cache_config({}) is None
    assert step_cache_config({"step_cache_thresh": None}) is None and step_cache_config({"step_cache_thresh": 0}) is None
    assert step_cache_config({"step_cache_thresh": 0.0, "step_cache_coefficients": [1, 0]}) is None
    assert step_cache_config({"step_cache_thresh": 0.4}) == (0.4, DEFAULT_COEFFICIENTS)
    assert step_cache_config({"step_cache_thresh": 1, "step_cache_coefficients": (1.0, 0.0)}) == (1.0, (1.0, 0.0))
    assert step_cache_config({"step_cache_thresh": np.float32(0.5), "step_cache_coefficients": np.array([2.0])}) == (0.5, (2.0,))


BAD = {
    "negative": {"step_cache_thresh": -0.1},
    "nan": {"step_cache_thresh": float("nan")},
    "inf": {"step_cache_thresh": float("inf")},
    "string": {"step_cache_thresh": "0.4"},
    "bool": {"step_cache_thresh": True},
    "no_coefficients": {"step_cache_thresh": 0.4, "step_cache_coefficients": []},
    "no_coefficients_off": {"step_cache_coefficients": ()},
    "a_word": {"step_cache_thresh": 0.4, "step_cache_coefficients": [1.0, "x"]},
    "a_string": {"step_cache_thresh": 0.4, "step_cache_coefficients": "1, 0"},
    "a_scalar": {"step_cache_thresh": 0.4, "step_cache_coefficients": 1.0},
    "nan_coefficient": {"step_cache_thresh": 0.4, "step_cache_coefficients": [1.0, float("nan")]},
    "none_coefficient": {"step_cache_thresh": 0.4, "step_cache_coefficients": [1.0, None]},
}


@pytest.mark.parametrize("case", list(BAD))
def test_bad_values(case):
    from loongx_amd.flux.step_cache import normalise_model_config, step_cache_config
    with pytest.raises(ValueError, match="step_cache"):
        step_cache_config(BAD[case])
    with pytest.raises(ValueError, match="step_cache"):
        step_cache_config(normalise_model_config(dict(BAD[case])))


@pytest.mark.parametrize("case", list(BAD))
def test_generate_refuses_before_it_touches_the_pipeline(case):
    """as tests/test_cfg_abi_cpu.py does for the guidance keywords: the stand-in transformer has no c_factor to lose, and the scheduler is as
    new afterwards"""
    from loongx_amd.flux.generate import generate
    from loongx_amd.flux.pipeline import LxFluxPipeline
    pipe = LxFluxPipeline(SimpleNamespace(device="cpu", config=SimpleNamespace(in_channels=64, guidance_embeds=True)))
    with pytest.raises(ValueError, match="step_cache"):
        generate(None, pipe, height=64, width=64, num_inference_steps=4, prompt_embeds=torch.zeros(2, 8, 32), pooled_prompt_embeds=torch.zeros(2, 32),
                 output_type="latent", model_config=dict(BAD[case]), condition_scale=2.0)
    assert not hasattr(pipe.transformer, "c_factor") and pipe.scheduler.timesteps is None and pipe.scheduler._step_index is None


def test_a_yaml_list_is_accepted_and_becomes_a_tuple():
    from loongx_amd.flux.step_cache import normalise_model_config, step_cache_config
    mc = yaml.safe_load("model:\n  union_cond_attn: true\n  step_cache_thresh: 0.25\n  step_cache_coefficients: [2, -1.5, 0.125]\n")["model"]
    assert isinstance(mc["step_cache_coefficients"], list)
    assert step_cache_config(mc) == (0.25, (2.0, -1.5, 0.125))
    mc = normalise_model_config(dict(mc))
    assert mc["step_cache_coefficients"] == (2.0, -1.5, 0.125) and step_cache_config(mc) == (0.25, (2.0, -1.5, 0.125))
    hash(tuple(sorted(mc.items())))                                  # (what the engine's graph key does with it)
    assert math.isclose(float(np.poly1d(mc["step_cache_coefficients"])(2.0)), 5.125)
