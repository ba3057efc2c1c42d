"""Mirror of the reference's src/flux/generate.py: `generate()` (:72-394), `prepare_params` (:25-65), `get_config`
(:16-22), `seed_everything` (:68-71) -- the LoongX denoise driver on MI355X.

Differences from the reference, all deliberate and recorded in DESIGN.md:
  Q1  brain signals reach the CS3 encoders as [B,C,L] (what OminiModel.step does, model.py:659-673), not flatten(1);
  Q2  with fuse_flag=False the reference replaces the text embeddings only when BOTH brain sides exist (generate.py:252-255);
      that literal rule is the default here (`brain_replace="both"`). `brain_replace="per_stream"` is the opt-in extension that
      lets each side replace its own embedding (EEG[+PPG] -> prompt_embeds, fNIRS[+Motion] -> pooled), which is what makes
      EEG-only conditioning (BASELINE configs[1]) take effect; bench.py / inference.py --synthetic ask for it explicitly;
  Q5  signals may carry a batch dimension ([B,C,L]); a [C,L] tensor is treated as batch 1 like the reference.
  Q6  fp16 operand mode (model_config["operands"] = "fp16" / dtype float16): where the reference clips fp16 activations silently
      (block.py:275-276, 336-337) the kernels saturate AND count; generate() reads the counter once per image and applies
      model_config["f16_overflow"]: "raise" (default; F16OverflowError), "warn", or "fallback" (the image is computed again from the
      same start latents with bf16 operands).
  Q7  true classifier-free guidance (negative_prompt[_embeds], true_cfg_scale > 1; diffusers' FluxPipeline, the reference has none): the
      brain signals act on the POSITIVE branch only. The negative embeddings are used as given -- never fused with, gated by or replaced
      by brain embeddings: under brain_replace both branches would otherwise carry the same embedding and guidance would do nothing. Both
      branches run as one forward at batch 2B per step, [positive; negative], and lx_euler_step_cfg steps both halves.
  Q8  step caching (model_config["step_cache_thresh"]; TeaCache, diffusers has none built in): opt-in, the loop below is unchanged -- the
      engine decides per forward whether the blocks run (step_cache.py) and the output carries its report as `lx_step_cache`.
  Q9  guidance along the brain signal (brain_guidance_scale > 1; InstructPix2Pix's second scale with the brain embedding as the
      instruction channel, neither the reference nor diffusers has it): a text-only branch T carries the embeddings as encode_prompt left
      them, the full branch F what the brain section made of them, and the velocity is nested so that each scale alone is what exists:
      v_b = v_T + s_b (v_F - v_T), then g = v_N + s_t (v_b - v_N) under true CFG. On only where the signals changed an embedding (decided by
      tensor identity); otherwise one RuntimeWarning and the call without it. One forward per step at batch k·B·n, [F; T], [F; N] or
      [F; T; N]; lx_euler_step_cfg steps two branches, lx_euler_step_cfg3 three.
  Q10 adaptive projected guidance (apg_eta, apg_norm_threshold, apg_momentum; Sadat, Hilliges and Weber -- PAPERS.md; neither the
      reference nor diffusers' FluxPipeline has it): against the oversaturation of high guidance scales, the TOTAL guidance update of a
      guided call (Q7 and/or Q9) is taken to the space of the denoised prediction, given a momentum, clamped in norm and split along the
      first branch's prediction, whose part is weighted by eta. On only where the call is guided and one of the three differs from its
      default (1, 0, 0); otherwise the call is what it was, bit for bit (unguided: one RuntimeWarning). lx_euler_step_apg then steps in
      place of lx_euler_step_cfg / lx_euler_step_cfg3; the per-step sums stay on the device as the output's `lx_apg`.
  Q11 a second-order multistep sampler (solver="dpmpp_2m"; Lu et al., DPM-Solver++ -- PAPERS.md; diffusers has it as
      DPMSolverMultistepScheduler(use_flow_sigmas=True), the reference steps with Euler only): the same schedule and the same one forward
      per step, and each step is the Euler step plus c_i (D_i - D_{i-1}) on the denoised prediction D = x - sigma g along whatever velocity g
      the step runs (plain, guided by Q7 / Q9, projected by Q10). c_i is formed on the host (pipeline.multistep_coefficient) and is 0 -- the
      Euler step bit for bit -- on the first step of a trajectory, on the step onto sigma 0 and after sigma 1. One fp32 history buffer of one
      part's shape lives for the call; lx_dpmpp2m_step / lx_dpmpp2m_step_apg step in place of the Euler entries. A callback that returns
      latents keeps the history: the next step's difference is then taken against the prediction of the latents it replaced. The default,
      solver="euler", launches what it launched before; the coefficients used are the output's `lx_solver`.
  Q12 editing a source image along a prompt change (source_prompt[_embeds], source_guidance_scale, flowedit_n_max, flowedit_n_avg; Kulikov
      et al., FlowEdit -- PAPERS.md; neither the reference nor diffusers has it): with a description of what `image` / `image_latents`
      shows, the call integrates an ODE from the source latents X straight to the edited ones, without inversion: Z starts as X, and over
      the last n_max steps of the schedule every step draws n_avg noises, forms S = scale_noise(X, sigma_i, N) and R = Z + (S - X)
      (lx_flowedit_inputs), runs ONE forward at batch 2·B·n on [R; S] with the embeddings [target; source] and the per-row guidance
      [guidance_scale; source_guidance_scale], and updates Z += mask (s_{i+1} - s_i) / n_avg (Vt - Vs) (lx_flowedit_step). The target
      branch is what the brain section made of the embeddings (branch F); the source embeddings are used as given, by Q7's rule and for the
      same reason. mask_image / latent_mask become the mask of the update: kept tokens are the source bit for bit. The first noise is
      what prepare_latents returns (the caller's `latents`, or its draw), every later one a fresh draw from the same `generator`; the fp16
      fallback's second pass starts from Z = X at the begin index again and draws ON from the generator (it does not replay the first
      pass's noises). A callback sees, and may replace, Z. Refused together with true CFG, brain guidance, APG, solver != "euler", the step
      cache and strength != 1; the paper's n_min tail (plain sampling of the target over the last steps) does not exist here. What was
      done is the output's `lx_flowedit`; a call without the keywords launches what it launched before.
"""
from __future__ import annotations

import contextlib
import os
import warnings
from typing import Any, Callable, Dict, List, Optional, Union

import numpy as np
import torch
import yaml

from .condition import Condition
from .pipeline import ApgState, FlowEditState, FluxPipelineOutput, MultistepState, calculate_shift, retrieve_timesteps
from .pipeline_tools import encode_images
from .step_cache import step_cache_config
from .transformer import tranformer_forward


F16_OVERFLOW_POLICIES = ("raise", "warn", "fallback")


class F16OverflowError(RuntimeError):
    """An operand of the fp16 operand mode left fp16's range (+-65504) and was saturated: the image is not what the mode promises."""


@contextlib.contextmanager
def vae_f16_overflow(vae, policy: Optional[str]):
    """model_config["f16_overflow"] handed to the VAE for one call: a VAE that has the attribute (LxAutoencoderKL; it matters on fp16
    operands only) runs under `policy` inside the block and gets its own setting back after it. Any other VAE, or no policy: a no-op."""
    if policy is None or not hasattr(vae, "f16_overflow"):
        yield
        return
    if policy not in F16_OVERFLOW_POLICIES:
        raise ValueError(f'model_config["f16_overflow"] = {policy!r}: one of {F16_OVERFLOW_POLICIES}')
    own, vae.f16_overflow = vae.f16_overflow, policy
    try:
        yield
    finally:
        vae.f16_overflow = own


@contextlib.contextmanager
def adapter_weight_tiles(engine, tiles: int):
    """A guided call runs the branches of the same images ([positive; negative], [full; text; negative]) in one batch: inside the block a
    per-image adapter weight table (set_adapters(names, [w per image])) of length B applies to each of the `tiles` parts of a conditioning
    with tiles x B images. Told to the engine for the steps of one call, the way c_factor is; tiles == 1 or no engine: a no-op."""
    if engine is None or tiles == 1:
        yield
        return
    engine.adapter_weight_tiles = tiles
    try:
        yield
    finally:
        engine.adapter_weight_tiles = 1


def get_config(config_path: str = None):
    config_path = config_path or os.environ.get("XFL_CONFIG")
    if not config_path:
        return {}
    with open(config_path, "r") as f:
        return yaml.safe_load(f)


def prepare_params(prompt: Union[str, List[str]] = None, prompt_2=None, height: Optional[int] = 512, width: Optional[int] = 512,
                   num_inference_steps: int = 28, timesteps: List[int] = None, guidance_scale: float = 3.5,
                   num_images_per_prompt: Optional[int] = 1, generator=None, latents: Optional[torch.Tensor] = None,
                   prompt_embeds: Optional[torch.Tensor] = None, pooled_prompt_embeds: Optional[torch.Tensor] = None,
                   output_type: Optional[str] = "pil", return_dict: bool = True,
                   joint_attention_kwargs: Optional[Dict[str, Any]] = None,
                   callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                   callback_on_step_end_tensor_inputs: List[str] = ["latents"], max_sequence_length: int = 512,
                   image=None, image_latents: Optional[torch.Tensor] = None, mask_image=None,
                   latent_mask: Optional[torch.Tensor] = None, strength: float = 1.0,
                   negative_prompt: Union[str, List[str]] = None, negative_prompt_2=None,
                   negative_prompt_embeds: Optional[torch.Tensor] = None, negative_pooled_prompt_embeds: Optional[torch.Tensor] = None,
                   true_cfg_scale: float = 1.0, brain_guidance_scale: float = 1.0, apg_eta: float = 1.0,
                   apg_norm_threshold: float = 0.0, apg_momentum: float = 0.0, solver: str = "euler",
                   source_prompt: Union[str, List[str]] = None, source_prompt_2=None, source_prompt_embeds: Optional[torch.Tensor] = None,
                   source_pooled_prompt_embeds: Optional[torch.Tensor] = None, source_guidance_scale: float = 1.5,
                   flowedit_n_max: Optional[int] = None, flowedit_n_avg: int = 1, **kwargs):
    """The reference's 18-tuple. The img2img / inpaint keywords of diffusers' FluxImg2ImgPipeline / FluxInpaintPipeline, the true-CFG
    keywords of its FluxPipeline and this project's brain_guidance_scale, apg_*, solver and FlowEdit keywords (source_*, flowedit_*) are
    named here (so they are not among the swallowed **kwargs) and returned by prepare_inpaint_params / prepare_cfg_params /
    prepare_brain_cfg_params / prepare_apg_params / prepare_solver_params / prepare_flowedit_params."""
    return (prompt, prompt_2, height, width, num_inference_steps, timesteps, guidance_scale, num_images_per_prompt, generator,
            latents, prompt_embeds, pooled_prompt_embeds, output_type, return_dict, joint_attention_kwargs, callback_on_step_end,
            callback_on_step_end_tensor_inputs, max_sequence_length)


def prepare_inpaint_params(image=None, image_latents: Optional[torch.Tensor] = None, mask_image=None,
                           latent_mask: Optional[torch.Tensor] = None, strength: float = 1.0, **kwargs):
    return image, image_latents, mask_image, latent_mask, strength


def prepare_cfg_params(negative_prompt=None, negative_prompt_2=None, negative_prompt_embeds=None, negative_pooled_prompt_embeds=None,
                       true_cfg_scale: float = 1.0, **kwargs):
    return negative_prompt, negative_prompt_2, negative_prompt_embeds, negative_pooled_prompt_embeds, true_cfg_scale


def prepare_brain_cfg_params(brain_guidance_scale: float = 1.0, **kwargs):
    return brain_guidance_scale


def _finite_number(name, value, at_least=None) -> None:
    """a keyword that takes a number: anything but a finite int or float (a bool is neither), or one below `at_least`, is a ValueError"""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not np.isfinite(value) or \
            (at_least is not None and float(value) < at_least):
        raise ValueError(f"{name} must be a finite number{'' if at_least is None else f' >= {at_least}'}, got {value!r}")


def _n_prompts(prompt, prompt_embeds):
    """how many prompts the call has: from `prompt`, else from the embeddings' batch; None where neither says"""
    return 1 if isinstance(prompt, str) else len(prompt) if isinstance(prompt, list) else \
        prompt_embeds.shape[0] if prompt_embeds is not None else None


def _brain_cfg(brain_guidance_scale) -> bool:
    """generate()'s brain_guidance_scale -> whether guidance along the brain signal is asked for (s_b > 1; whether it is ON is known only
    after the brain section: the signals have to change an embedding). A refusal is a ValueError on the host, before anything of the
    pipeline is touched; a scale in [0, 1) is one RuntimeWarning and the plain call, as true_cfg_scale <= 1 is."""
    s = brain_guidance_scale
    _finite_number("brain_guidance_scale", s, at_least=0)
    if float(s) < 1:
        warnings.warn(f"brain_guidance_scale={s} (< 1): guidance is off, running the plain call", RuntimeWarning, stacklevel=3)
    return float(s) > 1


def prepare_apg_params(apg_eta: float = 1.0, apg_norm_threshold: float = 0.0, apg_momentum: float = 0.0, **kwargs):
    return apg_eta, apg_norm_threshold, apg_momentum


_APG_UNGUIDED = ("apg_eta / apg_norm_threshold / apg_momentum were given but the call is not guided (neither true_cfg_scale nor "
                 "brain_guidance_scale is on): there is no guidance update to project, running the plain call")


def _apg(apg_eta, apg_norm_threshold, apg_momentum):
    """generate()'s apg_eta / apg_norm_threshold / apg_momentum -> (eta, norm_threshold, momentum) as floats where adaptive projected
    guidance is asked for (one of them differs from its default), else None; whether it is ON is known only once the branches are (it needs
    a guided call). A refusal is a ValueError on the host, before anything of the pipeline is touched."""
    for name, value in (("apg_eta", apg_eta), ("apg_norm_threshold", apg_norm_threshold), ("apg_momentum", apg_momentum)):
        _finite_number(name, value)
    eta, norm_threshold, momentum = float(apg_eta), float(apg_norm_threshold), float(apg_momentum)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"apg_eta must lie in [0, 1] (the weight of the update's part along the prediction), got {apg_eta!r}")
    if norm_threshold < 0.0:
        raise ValueError(f"apg_norm_threshold must be >= 0 (0: no clamp), got {apg_norm_threshold!r}")
    if not abs(momentum) < 1.0:
        raise ValueError(f"apg_momentum must lie in (-1, 1), got {apg_momentum!r}")
    return None if (eta, norm_threshold, momentum) == (1.0, 0.0, 0.0) else (eta, norm_threshold, momentum)


SOLVERS = ("euler", "dpmpp_2m")


def prepare_solver_params(solver: str = "euler", **kwargs):
    return solver


def _solver(solver) -> bool:
    """generate()'s solver -> whether the second-order multistep solver is on (Q11). Anything but one of SOLVERS is a ValueError on the
    host, before anything of the pipeline is touched."""
    if not isinstance(solver, str) or solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    return solver == "dpmpp_2m"


def prepare_flowedit_params(source_prompt=None, source_prompt_2=None, source_prompt_embeds=None, source_pooled_prompt_embeds=None,
                            source_guidance_scale: float = 1.5, flowedit_n_max: Optional[int] = None, flowedit_n_avg: int = 1, **kwargs):
    return (source_prompt, source_prompt_2, source_prompt_embeds, source_pooled_prompt_embeds, source_guidance_scale, flowedit_n_max,
            flowedit_n_avg)


def flowedit_default_n_max(num_inference_steps: int) -> int:
    """T - T // 7: the paper's 24 of 28 steps, kept in proportion (at least 1)"""
    return max(int(num_inference_steps) - int(num_inference_steps) // 7, 1)


def _flowedit(source_prompt, source_prompt_embeds, source_pooled_prompt_embeds, source_guidance_scale, flowedit_n_max, flowedit_n_avg,
              num_inference_steps, prompt, prompt_embeds, pooled_prompt_embeds):
    """generate()'s FlowEdit arguments (Q12) -> (n_max, n_avg) where a source description is given, else None. The three numbers are
    checked whether or not it is on. Every refusal is a ValueError on the host, before anything of the pipeline is touched, naming the
    keyword."""
    T = num_inference_steps
    if flowedit_n_max is not None and (isinstance(flowedit_n_max, bool) or not isinstance(flowedit_n_max, (int, np.integer)) or
                                       not isinstance(T, (int, np.integer)) or not 1 <= int(flowedit_n_max) <= int(T)):
        raise ValueError(f"flowedit_n_max must be an int in [1, num_inference_steps = {T}] (None: T - T // 7), got {flowedit_n_max!r}")
    if isinstance(flowedit_n_avg, bool) or not isinstance(flowedit_n_avg, (int, np.integer)) or int(flowedit_n_avg) < 1:
        raise ValueError(f"flowedit_n_avg must be an int >= 1, got {flowedit_n_avg!r}")
    _finite_number("source_guidance_scale", source_guidance_scale, at_least=0)
    if source_prompt is not None and source_prompt_embeds is not None:
        raise ValueError("Cannot forward both `source_prompt` and `source_prompt_embeds`.")
    if (source_prompt_embeds is None) != (source_pooled_prompt_embeds is None):
        raise ValueError("`source_prompt_embeds` and `source_pooled_prompt_embeds` have to be passed together.")
    if source_prompt is not None:
        n_prompts = _n_prompts(prompt, prompt_embeds)
        if not isinstance(source_prompt, (str, list)):
            raise ValueError(f"`source_prompt` has to be of type `str` or `list` but is {type(source_prompt)}")
        if isinstance(source_prompt, list) and n_prompts is not None and len(source_prompt) not in (1, n_prompts):
            raise ValueError(f"`source_prompt` has {len(source_prompt)} entries for a batch of {n_prompts} prompts: one, or one per prompt")
    if source_prompt_embeds is not None and prompt_embeds is not None and pooled_prompt_embeds is not None:
        _fits_positive("source_prompt_embeds", source_prompt_embeds, prompt_embeds)
        _fits_positive("source_pooled_prompt_embeds", source_pooled_prompt_embeds, pooled_prompt_embeds)
    if source_prompt is None and source_prompt_embeds is None:
        return None
    if not isinstance(T, (int, np.integer)) or isinstance(T, bool) or int(T) < 1:
        raise ValueError(f"source_prompt: FlowEdit needs num_inference_steps as an int >= 1, got {T!r}")
    return (flowedit_default_n_max(T) if flowedit_n_max is None else int(flowedit_n_max)), int(flowedit_n_avg)


_FLOWEDIT_WITH = "source_prompt (FlowEdit) does not combine with {}: its velocity is the difference of its own two branches"


def _flowedit_alone(do_true_cfg, brain_guidance_scale, want_apg, multistep, model_config, image, image_latents, strength):
    """what FlowEdit refuses to run with (Q12): ValueErrors on the host, before anything of the pipeline is touched"""
    if do_true_cfg:
        raise ValueError(_FLOWEDIT_WITH.format("an active true CFG (true_cfg_scale > 1 with a negative prompt)"))
    if float(brain_guidance_scale) > 1:
        raise ValueError(_FLOWEDIT_WITH.format(f"brain_guidance_scale={brain_guidance_scale} (> 1)"))
    if want_apg is not None:
        raise ValueError(_FLOWEDIT_WITH.format("apg_eta / apg_norm_threshold / apg_momentum: there is no guidance update to project"))
    if multistep:
        raise ValueError(_FLOWEDIT_WITH.format('solver != "euler": every step starts from fresh noise, there is no history to extrapolate'))
    if step_cache_config(model_config) is not None:
        raise ValueError(_FLOWEDIT_WITH.format('model_config["step_cache_thresh"]: its probe compares consecutive block inputs, which fresh '
                                               "noise makes meaningless"))
    if image is None and image_latents is None:
        raise ValueError("source_prompt (FlowEdit) describes a source image: pass `image` or `image_latents`.")
    if not (isinstance(strength, (int, float)) and float(strength) == 1.0):
        raise ValueError(f"strength={strength} with source_prompt (FlowEdit): flowedit_n_max plays its part, leave strength at 1")


def _flowedit_guidance(guidance, n_images, source_guidance_scale):
    """The per-row distilled-guidance vector of FlowEdit's batch [target; source]: `guidance` ([B·n]: the target branch's value per image)
    followed by source_guidance_scale per image. On a transformer without guidance embeddings (`guidance` is None) there is none, and a
    source_guidance_scale that differs from its default is one RuntimeWarning."""
    if guidance is None:
        if float(source_guidance_scale) != 1.5:
            warnings.warn(f"source_guidance_scale={source_guidance_scale} on a transformer without guidance embeddings: it has no effect",
                          RuntimeWarning, stacklevel=3)
        return None
    return torch.cat([guidance, torch.full((n_images,), float(source_guidance_scale), device=guidance.device, dtype=guidance.dtype)])


def _fits_positive(name, neg, pos):
    """negative embeddings differ from the positive ones in nothing but a batch of 1"""
    if not isinstance(neg, torch.Tensor) or neg.dim() != pos.dim() or neg.shape[1:] != pos.shape[1:] or neg.shape[0] not in (1, pos.shape[0]):
        raise ValueError(f"`{name}` must have the positive embeddings' shape {tuple(pos.shape)} (or a batch of 1), got "
                         f"{tuple(neg.shape) if isinstance(neg, torch.Tensor) else type(neg).__name__}")


def _true_cfg(negative_prompt, negative_prompt_embeds, negative_pooled_prompt_embeds, true_cfg_scale, prompt, prompt_embeds,
              pooled_prompt_embeds) -> bool:
    """generate()'s true-CFG arguments -> whether the call is guided (diffusers' rule: true_cfg_scale > 1 and a negative prompt given). Every
    refusal is a ValueError on the host, before anything of the pipeline is touched; half a request is one RuntimeWarning and the plain call."""
    s = true_cfg_scale
    _finite_number("true_cfg_scale", s)
    if negative_prompt is not None and negative_prompt_embeds is not None:
        raise ValueError("Cannot forward both `negative_prompt` and `negative_prompt_embeds`.")
    if (negative_prompt_embeds is None) != (negative_pooled_prompt_embeds is None):
        raise ValueError("`negative_prompt_embeds` and `negative_pooled_prompt_embeds` have to be passed together.")
    n_prompts = _n_prompts(prompt, prompt_embeds)
    if negative_prompt is not None:
        if not isinstance(negative_prompt, (str, list)):
            raise ValueError(f"`negative_prompt` has to be of type `str` or `list` but is {type(negative_prompt)}")
        if isinstance(negative_prompt, list) and n_prompts is not None and len(negative_prompt) not in (1, n_prompts):
            raise ValueError(f"`negative_prompt` has {len(negative_prompt)} entries for a batch of {n_prompts} prompts: one, or one per prompt")
    if negative_prompt_embeds is not None and prompt_embeds is not None and pooled_prompt_embeds is not None:
        _fits_positive("negative_prompt_embeds", negative_prompt_embeds, prompt_embeds)
        _fits_positive("negative_pooled_prompt_embeds", negative_pooled_prompt_embeds, pooled_prompt_embeds)
    has_negative = negative_prompt is not None or negative_prompt_embeds is not None
    if float(s) > 1 and not has_negative:
        warnings.warn(f"true_cfg_scale={s} without a negative prompt: nothing to guide away from, running the plain call",
                      RuntimeWarning, stacklevel=3)
    elif has_negative and not float(s) > 1:
        warnings.warn(f"a negative prompt with true_cfg_scale={s} (<= 1): guidance is off, running the plain call",
                      RuntimeWarning, stacklevel=3)
    return float(s) > 1 and has_negative


def _inpaint_source(pipeline, image, image_latents, mask_image, latent_mask, strength, num_inference_steps, batch, tokens, height, width,
                    f16_overflow):
    """generate()'s img2img / inpaint arguments -> (image_latents, mask): fp32 contiguous [batch, tokens, 64] on the pipeline's device (None
    where not asked for). Every refusal is a ValueError and comes before the first launch -- the host-side ones first, then the one
    synchronous min / max of a latent_mask -- so that a refused call leaves the pipeline as it was. `batch` is None where the caller's
    arguments do not determine it (check_inputs then refuses the call)."""
    if not (isinstance(strength, (int, float)) and 0.0 <= float(strength) <= 1.0):          # (a NaN fails both comparisons)
        raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
    if image is not None and image_latents is not None:
        raise ValueError("Cannot forward both `image` and `image_latents`.")
    if mask_image is not None and latent_mask is not None:
        raise ValueError("Cannot forward both `mask_image` and `latent_mask`.")
    source, mask = (image if image is not None else image_latents), (mask_image if mask_image is not None else latent_mask)
    if source is None:
        if mask is not None:
            raise ValueError("`mask_image` / `latent_mask` need a source to keep: pass `image` or `image_latents`.")
        if float(strength) != 1.0:
            raise ValueError(f"strength={strength} needs a source to start from: pass `image` or `image_latents`.")
        return None, None
    t_start = int(max(num_inference_steps - min(num_inference_steps * strength, num_inference_steps), 0))      # (get_timesteps' arithmetic)
    if num_inference_steps - t_start < 1:
        raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline steps is "
                         f"{num_inference_steps - t_start} which is < 1 and not appropriate for this pipeline.")

    def fits(name, t, last):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[1] != tokens or t.shape[2] not in last or \
                (batch is not None and t.shape[0] not in (1, batch)):
            raise ValueError(f"`{name}` must be a tensor of shape [1|{batch}, {tokens}, {' | '.join(map(str, last))}] for these latents, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if image_latents is not None:
        fits("image_latents", image_latents, (64,))
    if latent_mask is not None:
        fits("latent_mask", latent_mask, (64, 1))
    if batch is None:
        return None, None
    dev = pipeline.device
    if latent_mask is not None:
        mask = latent_mask.to(device=dev, dtype=torch.float32)
        lo, hi = torch.aminmax(mask)
        lo, hi = float(lo), float(hi)
        if not (0.0 <= lo and hi <= 1.0):                                                    # (a NaN fails both comparisons)
            raise ValueError(f"`latent_mask` must be finite and lie in [0, 1] (1: repaint, 0: keep); its values span [{lo}, {hi}]")
    elif mask_image is not None:
        mask = pipeline.pack_mask(mask_image, batch, height, width).to(dev)
        fits("mask_image (packed)", mask, (64,))
    if image is not None:
        image_latents = encode_images(pipeline, image, f16_overflow)[0].to(torch.float32)
        fits("image (encoded)", image_latents, (64,))
    image_latents = image_latents.to(device=dev, dtype=torch.float32).expand(batch, -1, -1).contiguous()
    if mask is not None:
        mask = mask.expand(batch, tokens, 64).contiguous()
    return image_latents, mask


def seed_everything(seed: int = 42):
    torch.manual_seed(seed)
    np.random.seed(seed)


def _signal(x, device, dtype, fixed_len, model):
    """[C,L] or [B,C,L] array-like -> padded/truncated [B,C,fixed_len] (generate.py:170-211)."""
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        x = torch.tensor(np.asarray(x))
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dim() != 3:
        raise ValueError(f"brain signal must be [C,L] or [B,C,L], got {tuple(x.shape)}")
    return model.spatial_pyramid_pooling(x.to(device).to(dtype), fixed_len)


_UNNAMED_ADAPTER_WARNED = False


def _select_adapter(pipeline, name: str) -> None:
    """generate(default_lora=False): run with the adapter named after the condition type (generate.py:279). One compatibility rule: a
    pipeline whose only adapter is the unnamed "default" (packed with the checkpoint, or loaded without an adapter_name) keeps it,
    with one RuntimeWarning per process; any other unknown name is set_adapters' ValueError."""
    global _UNNAMED_ADAPTER_WARNED
    loaded = pipeline.get_list_adapters()["transformer"]
    if name not in loaded and loaded == ["default"]:
        if not _UNNAMED_ADAPTER_WARNED:
            _UNNAMED_ADAPTER_WARNED = True
            warnings.warn(f'generate(default_lora=False): no adapter named {name!r} is loaded; keeping the only adapter, the unnamed '
                          '"default" (load it with adapter_name=... to select by condition type)', RuntimeWarning, stacklevel=3)
        return
    pipeline.set_adapters(name)


@torch.no_grad()
def generate(model, pipeline, conditions: List[Condition] = None, config_path: str = None,
             model_config: Optional[Dict[str, Any]] = {}, condition_scale: float = 1.0, default_lora: bool = False,
             additional_condition1: Optional[torch.Tensor] = None,   # EEG
             additional_condition2: Optional[torch.Tensor] = None,   # fNIRS
             additional_condition3: Optional[torch.Tensor] = None,   # PPG
             additional_condition4: Optional[torch.Tensor] = None,   # Motion
             use_brain_condition: bool = True, fuse_flag: bool = True, brain_replace: str = "both", **params):
    model_config = model_config or get_config(config_path).get("model", {})
    self = pipeline
    if brain_replace not in ("both", "per_stream"):
        raise ValueError(f"brain_replace must be 'both' (the reference rule) or 'per_stream', got {brain_replace!r}")
    (prompt, prompt_2, height, width, num_inference_steps, timesteps, guidance_scale, num_images_per_prompt, generator, latents,
     prompt_embeds, pooled_prompt_embeds, output_type, return_dict, joint_attention_kwargs, callback_on_step_end,
     callback_on_step_end_tensor_inputs, max_sequence_length) = prepare_params(**params)
    height = height or self.default_sample_size * self.vae_scale_factor
    width = width or self.default_sample_size * self.vae_scale_factor
    # ---- img2img / inpaint arguments (diffusers FluxImg2ImgPipeline / FluxInpaintPipeline): checked, and the source encoded, before
    # anything of the pipeline is touched. The source image is the first draw from the global generator, as in diffusers' prepare_latents.
    image, image_latents, mask_image, latent_mask, strength = prepare_inpaint_params(**params)
    # ---- true classifier-free guidance (diffusers FluxPipeline): its host-side refusals come first, with the inpaint ones
    negative_prompt, negative_prompt_2, negative_prompt_embeds, negative_pooled_prompt_embeds, true_cfg_scale = prepare_cfg_params(**params)
    do_true_cfg = _true_cfg(negative_prompt, negative_prompt_embeds, negative_pooled_prompt_embeds, true_cfg_scale, prompt, prompt_embeds,
                            pooled_prompt_embeds)
    # ---- guidance along the brain signal (Q9): the scale is checked here; whether it is on is known after the brain section
    brain_guidance_scale = prepare_brain_cfg_params(**params)
    want_brain_cfg = _brain_cfg(brain_guidance_scale)
    # ---- adaptive projected guidance (Q10): the three values are checked here; it is on only if the call ends up guided
    want_apg = _apg(*prepare_apg_params(**params))
    if want_apg is not None and not do_true_cfg and not want_brain_cfg:
        warnings.warn(_APG_UNGUIDED, RuntimeWarning, stacklevel=2)
    # ---- the sampler (Q11): the name is checked here
    multistep = _solver(prepare_solver_params(**params))
    step_cache_config(model_config)         # (model_config step_cache_thresh / step_cache_coefficients: a bad value is a ValueError here)
    # ---- FlowEdit (Q12): on where a source description is given; its numbers are checked here, and what it does not combine with
    (source_prompt, source_prompt_2, source_prompt_embeds, source_pooled_prompt_embeds, source_guidance_scale, flowedit_n_max,
     flowedit_n_avg) = prepare_flowedit_params(**params)
    flowedit = _flowedit(source_prompt, source_prompt_embeds, source_pooled_prompt_embeds, source_guidance_scale, flowedit_n_max,
                         flowedit_n_avg, num_inference_steps, prompt, prompt_embeds, pooled_prompt_embeds)
    if flowedit is not None:
        _flowedit_alone(do_true_cfg, brain_guidance_scale, want_apg, multistep, model_config, image, image_latents, strength)
    if any(a is not None for a in (image, image_latents, mask_image, latent_mask)) or strength != 1.0:
        n_prompts = _n_prompts(prompt, prompt_embeds)
        image_latents, inpaint_mask = _inpaint_source(
            pipeline, image, image_latents, mask_image, latent_mask, strength, num_inference_steps,
            latents.shape[0] if latents is not None else None if n_prompts is None else n_prompts * num_images_per_prompt,
            latents.shape[1] if latents is not None else (int(height) // self.vae_scale_factor) * (int(width) // self.vae_scale_factor),
            height, width, (model_config or {}).get("f16_overflow"))
    else:
        image_latents = inpaint_mask = None
    # the step-invariant conditioning cache of the transformer lives for the steps of ONE image: every tensor made below is
    # freed on return and its address may come back with different content on the next call
    if hasattr(pipeline.transformer, "invalidate_conditioning"):
        pipeline.transformer.invalidate_conditioning()
    if condition_scale != 1:
        pipeline.transformer.c_factor = float(condition_scale)
    self.check_inputs(prompt, prompt_2, height, width, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds,
                      callback_on_step_end_tensor_inputs=callback_on_step_end_tensor_inputs, max_sequence_length=max_sequence_length)
    self._guidance_scale, self._joint_attention_kwargs, self._interrupt = guidance_scale, joint_attention_kwargs, False
    batch_size = _n_prompts(prompt, prompt_embeds)
    device = self._execution_device
    lora_scale = self.joint_attention_kwargs.get("scale", None) if self.joint_attention_kwargs is not None else None
    prompt_embeds, pooled_prompt_embeds, text_ids = self.encode_prompt(
        prompt=prompt, prompt_2=prompt_2, prompt_embeds=prompt_embeds, pooled_prompt_embeds=pooled_prompt_embeds, device=device,
        num_images_per_prompt=num_images_per_prompt, max_sequence_length=max_sequence_length, lora_scale=lora_scale)
    if do_true_cfg:
        negative_prompt_embeds, negative_pooled_prompt_embeds, _ = self.encode_prompt(
            prompt=negative_prompt, prompt_2=negative_prompt_2, prompt_embeds=negative_prompt_embeds,
            pooled_prompt_embeds=negative_pooled_prompt_embeds, device=device, num_images_per_prompt=num_images_per_prompt,
            max_sequence_length=max_sequence_length, lora_scale=lora_scale)
    if flowedit is not None:
        source_prompt_embeds, source_pooled_prompt_embeds, _ = self.encode_prompt(
            prompt=source_prompt, prompt_2=source_prompt_2, prompt_embeds=source_prompt_embeds,
            pooled_prompt_embeds=source_pooled_prompt_embeds, device=device, num_images_per_prompt=num_images_per_prompt,
            max_sequence_length=max_sequence_length, lora_scale=lora_scale)
    text_prompt_embeds, text_pooled_prompt_embeds = prompt_embeds, pooled_prompt_embeds      # (branch T of brain guidance: the text alone)

    # ---- CS3 encoders + DGF fusion: once per image, outside the loop (generate.py:168-258) ----------
    brain_ran = use_brain_condition and any(c is not None for c in (additional_condition1, additional_condition2,
                                                                    additional_condition3, additional_condition4))
    if brain_ran:
        f32 = torch.float32
        eeg = _signal(additional_condition1, device, f32, model.eeg_fixed_length, model)
        fnirs = _signal(additional_condition2, device, f32, model.fnirs_fixed_length, model)
        ppg = _signal(additional_condition3, device, f32, model.ppg_fixed_length, model)
        motion = _signal(additional_condition4, device, f32, model.motion_fixed_length, model)
        prompt_embeds_brain = pooled_prompt_embeds_brain = None
        if eeg is not None:
            eeg_features = model.eeg_projection(eeg)
            prompt_embeds_brain = model.fuse_eeg(eeg_features, model.ppg_projection(ppg)) if ppg is not None else eeg_features
        if fnirs is not None:
            fnirs_features = model.fnirs_projection(fnirs)
            pooled_prompt_embeds_brain = (model.fuse_fnirs(fnirs_features, model.motion_projection(motion))
                                          if motion is not None else fnirs_features)
        for name, t, ref in (("prompt", prompt_embeds_brain, prompt_embeds), ("pooled", pooled_prompt_embeds_brain, pooled_prompt_embeds)):
            if t is not None and t.shape[0] != ref.shape[0]:
                if t.shape[0] != 1:
                    raise ValueError(f"brain {name} embeddings have batch {t.shape[0]}, prompt batch is {ref.shape[0]}")
        if fuse_flag and prompt_embeds_brain is not None and pooled_prompt_embeds_brain is not None:
            prompt_embeds = model.duan_norm_prompt(prompt_embeds.float(), prompt_embeds_brain.expand_as(prompt_embeds).contiguous())
            pooled_prompt_embeds = model.duan_norm_pooled(
                pooled_prompt_embeds.float().unsqueeze(1),
                pooled_prompt_embeds_brain.expand_as(pooled_prompt_embeds).contiguous().unsqueeze(1)).squeeze(1)
        elif brain_replace == "per_stream":
            if prompt_embeds_brain is not None:
                prompt_embeds = prompt_embeds_brain.expand(prompt_embeds.shape[0], -1, -1)
            if pooled_prompt_embeds_brain is not None:
                pooled_prompt_embeds = pooled_prompt_embeds_brain.expand(pooled_prompt_embeds.shape[0], -1)
        elif prompt_embeds_brain is not None and pooled_prompt_embeds_brain is not None:
            prompt_embeds, pooled_prompt_embeds = prompt_embeds_brain, pooled_prompt_embeds_brain

    # ---- guidance along the brain signal (Q9): on only where the signals changed an embedding (by identity: the brain section rebinds
    # what it replaces or fuses). Branch T, the text alone, then sits between the full branch and the negative one: [F; T], [F; N] or
    # [F; T; N] in ONE batch of k·B·n. The signals act on branch F only.
    do_brain_cfg = bool(want_brain_cfg and brain_ran and (prompt_embeds is not text_prompt_embeds or
                                                          pooled_prompt_embeds is not text_pooled_prompt_embeds))
    if want_brain_cfg and not do_brain_cfg:
        warnings.warn(f"brain_guidance_scale={brain_guidance_scale} but the brain signals change no embedding (no signals, "
                      "use_brain_condition=False, or brain_replace='both' with one side missing): nothing to guide along, running without "
                      "brain guidance", RuntimeWarning, stacklevel=2)
    if do_brain_cfg:
        for name, full, text in (("prompt_embeds", prompt_embeds, text_prompt_embeds),
                                 ("pooled_prompt_embeds", pooled_prompt_embeds, text_pooled_prompt_embeds)):
            if full.dim() != text.dim() or full.shape[1:] != text.shape[1:] or \
                    (full.shape[0] != text.shape[0] and 1 not in (full.shape[0], text.shape[0])):
                raise ValueError(f"brain_guidance_scale: the brain-conditioned `{name}` {tuple(full.shape)} and the text-only ones "
                                 f"{tuple(text.shape)} must have one shape (or a batch of 1) to run as branches of one batch")
        rows = max(prompt_embeds.shape[0], text_prompt_embeds.shape[0], pooled_prompt_embeds.shape[0], text_pooled_prompt_embeds.shape[0])
        prompt_embeds, text_prompt_embeds = (t if t.shape[0] == rows else t.expand(rows, -1, -1) for t in (prompt_embeds, text_prompt_embeds))
        pooled_prompt_embeds, text_pooled_prompt_embeds = (t if t.shape[0] == rows else t.expand(rows, -1)
                                                           for t in (pooled_prompt_embeds, text_pooled_prompt_embeds))
    # ---- true CFG: the negative branch is the last part of that ONE batch, built here once per image. Its embeddings are used as
    # given -- the brain signals above act on the full branch only (under brain_replace both branches would otherwise carry the same
    # embedding and guidance would do nothing)
    if do_true_cfg:
        if negative_prompt_embeds.shape[0] != prompt_embeds.shape[0]:           # (one negative prompt for the whole batch)
            negative_prompt_embeds = negative_prompt_embeds[:1].expand(prompt_embeds.shape[0], -1, -1)
            negative_pooled_prompt_embeds = negative_pooled_prompt_embeds[:1].expand(pooled_prompt_embeds.shape[0], -1)
        _fits_positive("negative_prompt_embeds", negative_prompt_embeds, prompt_embeds)
        _fits_positive("negative_pooled_prompt_embeds", negative_pooled_prompt_embeds, pooled_prompt_embeds)
    # ---- FlowEdit (Q12): the source branch is the second part of that ONE batch, [target; source]. The target is the embeddings as the
    # brain section left them (branch F); the source embeddings are used as given, for the reason the negative ones are. Both get one row
    # per image, so that the parts are [B·n] each.
    if flowedit is not None:
        rows = batch_size * num_images_per_prompt
        for name, t in (("prompt_embeds", prompt_embeds), ("pooled_prompt_embeds", pooled_prompt_embeds),
                        ("source_prompt_embeds", source_prompt_embeds), ("source_pooled_prompt_embeds", source_pooled_prompt_embeds)):
            if t.shape[0] not in (1, rows):
                raise ValueError(f"source_prompt (FlowEdit): `{name}` has batch {t.shape[0]} for {rows} image(s): one row, or one per image")
        prompt_embeds, source_prompt_embeds = (t if t.shape[0] == rows else t[:1].expand(rows, -1, -1)
                                               for t in (prompt_embeds, source_prompt_embeds))
        pooled_prompt_embeds, source_pooled_prompt_embeds = (t if t.shape[0] == rows else t[:1].expand(rows, -1)
                                                             for t in (pooled_prompt_embeds, source_pooled_prompt_embeds))
        _fits_positive("source_prompt_embeds", source_prompt_embeds, prompt_embeds)
        _fits_positive("source_pooled_prompt_embeds", source_pooled_prompt_embeds, pooled_prompt_embeds)
    n_branches = 1 + do_brain_cfg + do_true_cfg + (flowedit is not None)
    if n_branches > 1:
        others = ([(text_prompt_embeds, text_pooled_prompt_embeds)] if do_brain_cfg else []) + \
                 ([(negative_prompt_embeds, negative_pooled_prompt_embeds)] if do_true_cfg else []) + \
                 ([(source_prompt_embeds, source_pooled_prompt_embeds)] if flowedit is not None else [])
        prompt_embeds = torch.cat([prompt_embeds] + [e.to(prompt_embeds.dtype) for e, _ in others])
        pooled_prompt_embeds = torch.cat([pooled_prompt_embeds] + [p.to(pooled_prompt_embeds.dtype) for _, p in others])

    # ---- latents + condition tokens ----------------------------------------------------------------------
    num_channels_latents = self.transformer.config.in_channels // 4
    latents, latent_image_ids = self.prepare_latents(batch_size * num_images_per_prompt, num_channels_latents, height, width,
                                                     torch.float32, device, generator, latents)
    condition_latents, condition_ids, condition_type_ids = ([] for _ in range(3))
    use_condition = conditions is not None or []
    if use_condition:
        assert len(conditions) <= 1, "Only one condition is supported for now."
        if not default_lora:
            _select_adapter(pipeline, conditions[0].condition_type)
        for condition in conditions:
            with vae_f16_overflow(self.vae, (model_config or {}).get("f16_overflow")):      # (condition images go through encode_images)
                tokens, ids, type_id = condition.encode(self)
            condition_latents.append(tokens)
            condition_ids.append(ids)
            condition_type_ids.append(type_id)
        condition_latents = torch.cat(condition_latents, dim=1)
        condition_ids = torch.cat(condition_ids, dim=0)
        condition_type_ids = torch.cat(condition_type_ids, dim=0)
        if condition_latents.shape[0] == 1 and latents.shape[0] > 1:
            condition_latents = condition_latents.expand(latents.shape[0], -1, -1).contiguous()

    # ---- sigma schedule (generate.py:290-310) ---------------------------------------------------------------
    sigmas = np.linspace(1.0, 1 / num_inference_steps, num_inference_steps)
    cfg = self.scheduler.config
    mu = calculate_shift(latents.shape[1], cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, timesteps, sigmas, mu=mu)
    n_schedule = num_inference_steps
    num_warmup_steps = max(len(timesteps) - num_inference_steps * self.scheduler.order, 0)
    flowedit_state = flowedit_begin = None
    if flowedit is not None:
        # (Q12) the trajectory is the last n_max steps of the schedule, from the source itself: `latents` (the caller's, or the draw) is the
        # first noise, the edit state Z = X is what the loop carries, and the mask belongs to the state (no blend: kept tokens never move)
        flowedit_noise = [latents.contiguous()]
        flowedit_begin = n_schedule - flowedit[0]
        timesteps, num_inference_steps, th_left = self.get_timesteps_from(flowedit_begin, device)
        flowedit_state = FlowEditState(image_latents, inpaint_mask, flowedit[1])
        latents = flowedit_state.Z
        num_warmup_steps = max(len(timesteps) - num_inference_steps * self.scheduler.order, 0)
    elif image_latents is not None:
        # the trajectory starts at sigma[t_start] from the source noised to that level; `latents` (the caller's, or the draw) is the noise
        noise = latents.contiguous()
        timesteps, num_inference_steps, th_left = self.get_timesteps(n_schedule, strength, device)
        latents = self.scheduler.scale_noise(image_latents, n_schedule - num_inference_steps, noise)
        num_warmup_steps = max(len(timesteps) - num_inference_steps * self.scheduler.order, 0)
    step_kwargs = {} if inpaint_mask is None or flowedit is not None else {"inpaint": (image_latents, noise, inpaint_mask)}
    n_images = latents.shape[0]
    apg_state = multistep_state = None
    if multistep:
        # (Q11) one history buffer for the steps of this call, of one part's shape [B·n, ...]: made before the latents are repeated per branch
        multistep_state = MultistepState(tuple(latents.shape), device)
        step_kwargs["multistep"] = multistep_state
    if want_apg is not None and n_branches == 1 and (do_true_cfg or want_brain_cfg):      # (brain guidance was asked for and is off)
        warnings.warn(_APG_UNGUIDED, RuntimeWarning, stacklevel=2)
    if n_branches > 1:
        # the start latents once per branch ([full; text; negative] where all are on; the draw above stays [B·n, ...], so the generator is
        # consumed as in the plain call), the condition tokens and a [B·n] attention mask for every part; image_latents / noise / mask stay
        # [B·n, ...] (lx_euler_step_cfg, lx_euler_step_cfg3)
        if do_true_cfg:
            step_kwargs["true_cfg_scale"] = float(true_cfg_scale)
        if do_brain_cfg:
            step_kwargs["brain_guidance_scale"] = float(brain_guidance_scale)
        if want_apg is not None:
            # (Q10) one state for the steps of this call: M and the sums have one part's shape, [B·n, ...]; lx_euler_step_apg then steps in
            # place of lx_euler_step_cfg / lx_euler_step_cfg3. With all three keywords at their defaults the call is not routed here.
            apg_state = ApgState(*want_apg, tuple(latents.shape), len(timesteps), device)
            step_kwargs["apg"] = apg_state
        if flowedit is None:
            latents = torch.cat([latents] * n_branches)      # (FlowEdit's batch is formed per step, from Z and fresh noise: `latents` stays Z)
        if use_condition:
            condition_latents = condition_latents.repeat(n_branches * n_images // condition_latents.shape[0], 1, 1)
        user_mask = (self.joint_attention_kwargs or {}).get("attention_mask")
        if isinstance(user_mask, torch.Tensor) and user_mask.dim() == 4 and user_mask.shape[0] == n_images and n_images > 1:
            self._joint_attention_kwargs = dict(self.joint_attention_kwargs, attention_mask=torch.cat([user_mask] * n_branches))
    self._num_timesteps = len(timesteps)
    guidance = None
    if self.transformer.config.guidance_embeds:
        guidance = torch.full((latents.shape[0],), float(guidance_scale), device=device, dtype=torch.float32)
    if flowedit is not None:
        guidance = _flowedit_guidance(guidance, n_images, source_guidance_scale)
    prompt_embeds = prompt_embeds.contiguous()
    pooled_prompt_embeds = pooled_prompt_embeds.contiguous()

    # ---- denoise loop (generate.py:313-369) ------------------------------------------------------------------
    # the whole schedule is known here: hand it to the engine so the AdaLN modulation weights stream once per image
    # (host copy of the same fp32 values: a .tolist() on the device tensor would drain the stream here and keep the host from
    #  preparing this image while the GPU is still busy with the previous one)
    th = getattr(self.scheduler, "timesteps_host", None) if image_latents is None else th_left
    if th is not None and latents.dtype == torch.float32 and len(th) == len(timesteps):
        sched_ts = (th / np.float32(1000)).tolist()
    else:
        sched_ts = (timesteps.to(latents.dtype) / 1000).tolist()
    engine = getattr(pipeline.transformer, "engine", None)
    policy = str((model_config or {}).get("f16_overflow", "raise"))
    if policy not in F16_OVERFLOW_POLICIES:
        raise ValueError(f'model_config["f16_overflow"] = {policy!r}: one of {F16_OVERFLOW_POLICIES}')
    start_latents, operands_used, step_cache_report = latents, None, None

    def denoise(latents, prompt_embeds, model_config):
        nonlocal step_cache_report
        if apg_state is not None:
            apg_state.zero()                  # (empty momentum: the fp16 fallback's second pass starts as a fresh call does)
        if multistep_state is not None:
            multistep_state.zero()            # (no history: the same)
        if flowedit_state is not None:
            flowedit_state.zero()             # (Z = X again; the noises are NOT replayed: the second pass draws on from the generator)
            latents = flowedit_state.Z
        with adapter_weight_tiles(engine, n_branches), self.progress_bar(total=num_inference_steps) as progress_bar:
            for i, t in enumerate(timesteps):
                if self.interrupt:
                    continue
                if flowedit_state is not None:
                    # (Q12) n_avg noises, the inputs of all their forwards from the same Z, then per forward one launch that updates Z
                    noises = [flowedit_noise.pop() if flowedit_noise else
                              self.prepare_latents(n_images, num_channels_latents, height, width, torch.float32, device, generator, None)[0]
                              for _ in range(flowedit_state.n_avg)]
                    batches = self.scheduler.flowedit_inputs(flowedit_state, noises)
                    timestep = t.expand(batches.shape[1]).to(batches.dtype)
                    for k in range(flowedit_state.n_avg):
                        noise_pred = tranformer_forward(
                            self.transformer, model_config=model_config,
                            condition_latents=condition_latents if use_condition else None,
                            condition_ids=condition_ids if use_condition else None,
                            condition_type_ids=condition_type_ids if use_condition else None,
                            hidden_states=batches[k], timestep=timestep / 1000, guidance=guidance, pooled_projections=pooled_prompt_embeds,
                            encoder_hidden_states=prompt_embeds, txt_ids=text_ids, img_ids=latent_image_ids,
                            joint_attention_kwargs=self.joint_attention_kwargs, return_dict=False, lx_schedule=(i, sched_ts))[0]
                        latents = self.scheduler.step(noise_pred, t, batches[k], return_dict=False, flowedit=flowedit_state)[0]
                    if callback_on_step_end is not None:
                        scope = dict(locals())
                        callback_outputs = callback_on_step_end(self, i, t, {k: scope[k] for k in callback_on_step_end_tensor_inputs})
                        given = callback_outputs.pop("latents", latents)
                        if given is not latents:                            # (its latents become the edit state)
                            flowedit_state.Z.copy_(given)
                        prompt_embeds = callback_outputs.pop("prompt_embeds", prompt_embeds)
                    progress_bar.update()
                    continue
                timestep = t.expand(latents.shape[0]).to(latents.dtype)
                noise_pred = tranformer_forward(
                    self.transformer, model_config=model_config,
                    condition_latents=condition_latents if use_condition else None,
                    condition_ids=condition_ids if use_condition else None,
                    condition_type_ids=condition_type_ids if use_condition else None,
                    hidden_states=latents, timestep=timestep / 1000, guidance=guidance, pooled_projections=pooled_prompt_embeds,
                    encoder_hidden_states=prompt_embeds, txt_ids=text_ids, img_ids=latent_image_ids,
                    joint_attention_kwargs=self.joint_attention_kwargs, return_dict=False, lx_schedule=(i, sched_ts))[0]
                latents = self.scheduler.step(noise_pred, t, latents, return_dict=False, **step_kwargs)[0]
                if callback_on_step_end is not None:
                    scope = dict(locals())                                  # (a comprehension has its own locals() before 3.12)
                    if n_branches > 1:
                        scope["latents"] = shown = latents[:n_images]       # (the parts are equal: a callback sees the images' own)
                    callback_kwargs = {}
                    for k in callback_on_step_end_tensor_inputs:
                        callback_kwargs[k] = scope[k]
                    callback_outputs = callback_on_step_end(self, i, t, callback_kwargs)
                    if n_branches > 1:
                        given = callback_outputs.pop("latents", shown)
                        if given is not shown:                              # (its latents go to every part: a copy, made only when it returns some)
                            latents = torch.cat([given] * n_branches)
                    else:
                        latents = callback_outputs.pop("latents", latents)
                    prompt_embeds = callback_outputs.pop("prompt_embeds", prompt_embeds)
                if i == len(timesteps) - 1 or ((i + 1) > num_warmup_steps and (i + 1) % self.scheduler.order == 0):
                    progress_bar.update()
        # what the step cache decided for this trajectory (None when off): read here, the conditioning it belongs to ends with the image
        step_cache_report = engine.step_cache_report() if hasattr(engine, "step_cache_report") else None
        return latents[:n_images] if n_branches > 1 else latents

    latents = denoise(start_latents, prompt_embeds, model_config)
    if engine is not None and engine.f16:
        # Q6: the saturation counter of this image's fp16 operand images. "fallback" has to know NOW, and a decode drains the stream anyway:
        # one 4-byte synchronous read. Otherwise (latent output: the host runs ahead of the GPU) the pinned-host asynchronous read of
        # check_status(sync=False) -- an event then surfaces at the next image's check; callers that keep latents end their loop with
        # engine.f16_overflow_poll(sync=True) (inference.py does, per image, before it saves).
        operands_used = "fp16"
        n_sat = engine.f16_overflow_poll(sync=(policy == "fallback" or output_type != "latent"))
        if n_sat:
            what = (f"fp16 operand mode: {n_sat} saturation event(s) (producer waves that clipped an operand to +-65504, or clipped weights: "
                    f"{getattr(engine, 'w16_clipped', 0)})")
            if policy == "raise":
                raise F16OverflowError(what + '; model_config["f16_overflow"] = "fallback" recomputes such images with bf16 operands, "warn" keeps them')
            if policy == "warn":
                warnings.warn(what + "; the image was kept", RuntimeWarning, stacklevel=2)
            else:
                warnings.warn(what + "; recomputing this image with bf16 operands", RuntimeWarning, stacklevel=2)
                pipeline.transformer.invalidate_conditioning()
                timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, n_schedule, device, None, sigmas, mu=mu)      # (step index back to 0)
                if flowedit_state is not None:                # (Q12: the begin index again; denoise puts Z = X and draws on from the generator)
                    timesteps, num_inference_steps, _ = self.get_timesteps_from(flowedit_begin, device)
                elif image_latents is not None:               # (and on to t_start again: the same start latents, the same blend)
                    timesteps, num_inference_steps, _ = self.get_timesteps(n_schedule, strength, device)
                latents = denoise(start_latents, prompt_embeds, dict(model_config or {}, operands="bf16"))
                operands_used = "bf16 (fp16 overflow fallback)"

    if output_type == "latent":
        image = latents
    else:
        if self.vae is None or self.image_processor is None:
            raise NotImplementedError("decoding to pixels needs a VAE (outside the MI355X hot path): use output_type='latent' "
                                      "or construct LxFluxPipeline(vae=..., image_processor=...)")
        if hasattr(pipeline.transformer, "engine"):
            # a split-K pair time-out invalidates this image's latents: find out BEFORE it is decoded and handed back (the decode
            # drains the stream anyway, so the synchronous check costs one 4-byte read)
            pipeline.transformer.engine.check_status(sync=True)
        z = self._unpack_latents(latents, height, width, self.vae_scale_factor)
        z = (z / self.vae.config.scaling_factor) + self.vae.config.shift_factor
        with vae_f16_overflow(self.vae, (model_config or {}).get("f16_overflow")):      # (an fp16-operand VAE applies it to its own counter)
            image = self.vae.decode(z, return_dict=False)[0]
        image = self.image_processor.postprocess(image, output_type=output_type)
    self.maybe_free_model_hooks()
    if condition_scale != 1:
        pipeline.transformer.c_factor = None
    if hasattr(pipeline.transformer, "invalidate_conditioning"):
        pipeline.transformer.invalidate_conditioning()
        if output_type == "latent":
            # latents stay on the device and the host runs ahead: no synchronisation here. A pair time-out surfaces at the next
            # image's check; callers that keep latents must call engine.check_status() once at the end of their loop
            # (inference.py does, per shard)
            pipeline.transformer.engine.check_status(sync=False)
    if not return_dict:
        return (image,)
    return FluxPipelineOutput(images=image, lx_operands=operands_used, lx_step_cache=step_cache_report,
                              lx_apg=None if apg_state is None else apg_state.sums,
                              lx_solver=None if multistep_state is None else {"solver": "dpmpp_2m",
                                                                              "coefficients": list(multistep_state.coefficients)},
                              lx_flowedit=None if flowedit_state is None else {
                                  "n_max": flowedit[0], "n_avg": flowedit[1], "begin_index": flowedit_begin,
                                  "sigmas": [s for _, s, _ in flowedit_state.taken], "coefs": [c for _, _, c in flowedit_state.taken],
                                  "guidance_scale": float(guidance_scale), "source_guidance_scale": float(source_guidance_scale)})
