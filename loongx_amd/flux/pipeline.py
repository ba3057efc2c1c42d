"""`LxFluxPipeline`: the slice of diffusers' FluxPipeline that the reference's generate() touches
(src/flux/generate.py:72-394), for MI355X.  Restated from diffusers==0.31.0 (train/requirements.txt:1): latent packing,
latent image ids, calculate_shift, FlowMatchEulerDiscreteScheduler.  The Euler update runs in HIP (lx_euler_step).
Beyond what the reference calls, from diffusers' FluxImg2ImgPipeline / FluxInpaintPipeline: scale_noise, set_begin_index, get_timesteps,
the packed latent mask (pack_mask) and the per-step blend (lx_scale_noise, lx_euler_step_blend). Beyond diffusers: the guided, projected
and second-order steps, and FlowEdit's two scheduler functions (flowedit_inputs, step(flowedit=); lx_flowedit_inputs, lx_flowedit_step).

Text encoders (T5/CLIP) and the VAE are outside the denoise hot path ("next"): pass `prompt_embeds`,
`pooled_prompt_embeds` and `output_type="latent"`, or plug callables in via `text_encoder=` / `vae=`.
"""
from __future__ import annotations

import math
from contextlib import contextmanager
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from .. import ops


class FluxPipelineOutput(SimpleNamespace):
    pass


def calculate_shift(image_seq_len, base_seq_len: int = 256, max_seq_len: int = 4096, base_shift: float = 0.5,
                    max_shift: float = 1.16):
    m = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    return image_seq_len * m + (base_shift - m * base_seq_len)


class ApgState:
    """What adaptive projected guidance carries through the steps of one guided call (FlowMatchEulerDiscreteScheduler.step(apg=)): the three
    parameters, the momentum buffer M (fp32, one part's shape, in the space of the denoised prediction), the sums every step leaves
    ([steps, images, 3] float64: sum Db^2, sum Db w, sum w^2 per image; on the device, never synchronised), lx_euler_step_apg's workspace and
    the number of steps taken. zero() is the state before the first step."""

    def __init__(self, eta: float, norm_threshold: float, momentum: float, part_shape, steps: int, device):
        images, elems = int(part_shape[0]), int(np.prod(part_shape[1:], dtype=np.int64))
        self.eta, self.norm_threshold, self.momentum = float(eta), float(norm_threshold), float(momentum)
        self.M = torch.zeros(tuple(part_shape), dtype=torch.float32, device=device)
        self.sums = torch.zeros(int(steps), images, 3, dtype=torch.float64, device=device)
        self.workspace = torch.empty(max(ops.apg_workspace_bytes(images, elems), 8) // 8, dtype=torch.float64, device=device)
        self.step = 0

    def zero(self):
        self.M.zero_()
        self.sums.zero_()
        self.step = 0


class MultistepState:
    """What the second-order multistep solver carries through the steps of one call (FlowMatchEulerDiscreteScheduler.step(multistep=);
    generate's solver="dpmpp_2m"): the previous step's denoised prediction D (fp32, one part's shape, on the device), whether one is
    stored (`have`), and the coefficient of every step taken so far (host floats holding fp32 values; the first-order steps' are 0).
    zero() is the state before the first step. The analogue of ApgState."""

    def __init__(self, part_shape, device):
        self.D = torch.zeros(tuple(part_shape), dtype=torch.float32, device=device)
        self.have = False
        self.coefficients: List[float] = []

    def zero(self):
        self.D.zero_()
        self.have = False
        self.coefficients = []


class FlowEditState:
    """What FlowEdit carries through the steps of one call (FlowMatchEulerDiscreteScheduler.flowedit_inputs / step(flowedit=); generate's
    source_prompt): the source latents X and the edit state Z (fp32, contiguous, one part's shape [B·n, ...], on X's device; Z starts as
    X), the mask (X's shape; 1 edit, 0 keep) or None, n_avg, the inputs of a step's n_avg forwards ([n_avg, 2·B·n, ...]: row k is
    [target; source] of the k-th forward), how many of them have been applied (`pending` counts down from n_avg to 0), and the record of
    the steps taken: (step index, sigma, coef) per forward, host floats holding fp32 values. zero() puts Z = X again and empties the
    record. The analogue of MultistepState."""

    def __init__(self, X: torch.Tensor, mask: Optional[torch.Tensor] = None, n_avg: int = 1):
        if not isinstance(X, torch.Tensor) or X.dim() < 1 or X.shape[0] == 0:
            raise ValueError("FlowEditState: X is the packed source latents, a tensor [B, ...]")
        if isinstance(n_avg, bool) or not isinstance(n_avg, (int, np.integer)) or int(n_avg) < 1:
            raise ValueError(f"FlowEditState: n_avg must be an int >= 1, got {n_avg!r}")
        self.X = X.to(torch.float32).contiguous()
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != tuple(self.X.shape) or mask.device != self.X.device:
                raise ValueError(f"FlowEditState: the mask must have X's shape {tuple(self.X.shape)} on its device, got "
                                 f"{tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__}")
            mask = mask.to(torch.float32).contiguous()
        self.mask, self.n_avg = mask, int(n_avg)
        self.Z = self.X.clone()
        self.inputs = torch.empty((self.n_avg, 2 * self.X.shape[0]) + tuple(self.X.shape[1:]), dtype=torch.float32, device=self.X.device)
        self.pending = 0
        self.taken: List[tuple] = []

    def zero(self):
        self.Z.copy_(self.X)
        self.pending = 0
        self.taken = []


def flowedit_coefficient(sig_host, i: int, n_avg: int = 1) -> float:
    """The coefficient of one forward's update of FlowEdit's step i on the schedule `sig_host` (its fp32 sigmas, the final 0 included):
    (s_{i+1} - s_i) / n_avg, the difference formed in fp32 as step() forms it, the quotient in float64 and rounded once to fp32; a Python
    float. Host only."""
    ds32 = np.float32(sig_host[i + 1]) - np.float32(sig_host[i])
    return float(np.float32(np.float64(ds32) / n_avg))


def multistep_coefficient(sig_host, i: int, begin: int = 0) -> float:
    """The coefficient c_i of DPM-Solver++(2M) written as the Euler step plus c_i (D_i - D_{i-1}) (include/lx.h, lx_dpmpp2m_step), for step i
    of the schedule `sig_host` (its fp32 sigmas, the final 0 included) on a trajectory that began at step `begin`:
        c_i = (1 - s_{i+1} / s_i) (lam_{i+1} - lam_i) / (2 (lam_i - lam_{i-1})),   lam(s) = ln((1 - s) / s)
    in float64, rounded once to fp32 and returned as a Python float. 0 where the step is first order: the first step of the trajectory (no
    history), a step onto sigma 0 (diffusers' final_sigmas_type "zero"), and a step whose previous sigma is >= 1 (lam_{i-1} = -inf: the
    history carries no weight). Host only."""
    if i <= begin:
        return 0.0
    s_prev, s, s_next = (float(sig_host[k]) for k in (i - 1, i, i + 1))
    if s_next <= 0.0 or s_prev >= 1.0:
        return 0.0
    lam_prev, lam, lam_next = (math.log((1.0 - t) / t) for t in (s_prev, s, s_next))
    if lam == lam_prev:                       # (a repeated sigma: no step was taken between the two predictions)
        return 0.0
    return float(np.float32((1.0 - s_next / s) * (lam_next - lam) / (2.0 * (lam - lam_prev))))


class FlowMatchEulerDiscreteScheduler:
    """FLUX.1-dev scheduler config; sigma schedule on the host in fp64 -> fp32 like diffusers, step on the GPU. The step is the first-order
    Euler step, or with step(multistep=) the second-order multistep one at the same one model call per step: `order` stays 1."""
    order = 1

    def __init__(self, num_train_timesteps=1000, shift=3.0, use_dynamic_shifting=True, base_shift=0.5, max_shift=1.15,
                 base_image_seq_len=256, max_image_seq_len=4096):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, shift=shift, use_dynamic_shifting=use_dynamic_shifting,
                                      base_shift=base_shift, max_shift=max_shift, base_image_seq_len=base_image_seq_len,
                                      max_image_seq_len=max_image_seq_len)
        self.timesteps = self.sigmas = None
        self._step_index = self._begin_index = None

    def set_timesteps(self, num_inference_steps=None, device=None, sigmas=None, mu=None):
        if sigmas is None:
            sigmas = np.linspace(self.config.num_train_timesteps, 1, num_inference_steps) / self.config.num_train_timesteps
        sigmas = np.asarray(sigmas, dtype=np.float64)
        if self.config.use_dynamic_shifting:
            if mu is None:
                raise ValueError("use_dynamic_shifting=True needs mu")
            sigmas = math.exp(mu) / (math.exp(mu) + (1.0 / sigmas - 1.0))
        else:
            s = self.config.shift
            sigmas = s * sigmas / (1 + (s - 1) * sigmas)
        sig = sigmas.astype(np.float32)
        self._sig_host = np.concatenate([sig, np.zeros(1, np.float32)])
        self.timesteps_host = sig * np.float32(self.config.num_train_timesteps)      # same fp32 values as self.timesteps, no device sync
        self.timesteps = torch.from_numpy(self.timesteps_host).to(device)
        self.sigmas = torch.from_numpy(self._sig_host).to(device)
        self._step_index = self._begin_index = 0

    def set_begin_index(self, begin_index: int = 0):
        """diffusers' set_begin_index, called after set_timesteps (which puts it back to 0): the next step() is step `begin_index` of the
        schedule (an img2img / inpaint trajectory that starts part-way, LxFluxPipeline.get_timesteps)."""
        if self.timesteps is None or not 0 <= int(begin_index) < len(self.timesteps_host):
            raise ValueError(f"set_begin_index({begin_index}): call set_timesteps first; the index must lie inside its schedule")
        self._step_index = self._begin_index = int(begin_index)

    def _sigma_index(self, sigma_index_or_timestep) -> int:
        """A Python / numpy integer is an index into the schedule; anything else is one of its timesteps (exact match, as diffusers'
        index_for_timestep). Looked up in the host copy of the schedule."""
        s = sigma_index_or_timestep
        if isinstance(s, (int, np.integer)) and not isinstance(s, bool):
            if not 0 <= int(s) < len(self._sig_host):
                raise ValueError(f"sigma index {int(s)} outside the schedule of {len(self._sig_host)} sigmas")
            return int(s)
        hit = np.nonzero(self.timesteps_host == np.float32(float(s)))[0]
        if len(hit) == 0:
            raise ValueError(f"timestep {float(s)} is not in the schedule")
        return int(hit[0])

    def scale_noise(self, sample: torch.Tensor, sigma_index_or_timestep, noise: torch.Tensor) -> torch.Tensor:
        """diffusers' scale_noise: sigma * noise + (1 - sigma) * sample in fp32 (lx_scale_noise), sigma read from the host copy of the
        schedule: the start of an img2img trajectory."""
        if self.sigmas is None:
            raise ValueError("scale_noise: call set_timesteps first")
        sigma = float(self._sig_host[self._sigma_index(sigma_index_or_timestep)])
        return ops.scale_noise(sample.to(torch.float32).contiguous(), noise.to(torch.float32).contiguous(), sigma)

    def flowedit_inputs(self, state: "FlowEditState", noises) -> torch.Tensor:
        """The inputs of the n_avg forwards of FlowEdit's step at the current step index (lx_flowedit_inputs, one launch per forward), all
        formed from the same Z before any update of this step: for the k-th noise N_k (X's shape, fp32), row k of state.inputs becomes
        [Z + (S_k - X); S_k] with S_k = scale_noise(X, sigma_i, N_k). Returns state.inputs, [n_avg, 2·B·n, ...]; step(flowedit=state) then
        takes the forwards' outputs one by one, in this order. A mismatch is a ValueError before any launch."""
        if self.sigmas is None:
            raise ValueError("flowedit_inputs: call set_timesteps first")
        if not isinstance(state, FlowEditState):
            raise ValueError(f"flowedit_inputs: state must be a FlowEditState, got {type(state).__name__}")
        i = self._step_index
        if not 0 <= i < len(self.timesteps_host):
            raise ValueError(f"flowedit_inputs: step index {i} is past the schedule of {len(self.timesteps_host)} steps")
        if state.pending:
            raise ValueError(f"flowedit_inputs: {state.pending} forward(s) of the previous inputs have not been applied with step(flowedit=)")
        noises = list(noises)
        if len(noises) != state.n_avg:
            raise ValueError(f"flowedit_inputs: {len(noises)} noise tensor(s) for n_avg = {state.n_avg}")
        for k, nz in enumerate(noises):
            if not isinstance(nz, torch.Tensor) or tuple(nz.shape) != tuple(state.X.shape) or nz.device != state.X.device:
                raise ValueError(f"flowedit_inputs: noise {k} must have the source latents' shape {tuple(state.X.shape)} on their device, got "
                                 f"{tuple(nz.shape) if isinstance(nz, torch.Tensor) else type(nz).__name__}")
        if tuple(state.Z.shape) != tuple(state.X.shape) or state.Z.dtype != torch.float32 or not state.Z.is_contiguous():
            raise ValueError(f"flowedit_inputs: the edit state Z {tuple(state.Z.shape)} must be fp32, contiguous and of X's shape")
        sigma = float(self._sig_host[i])
        for k, nz in enumerate(noises):
            ops.flowedit_inputs(state.X, state.Z, nz.to(torch.float32).contiguous(), sigma, out=state.inputs[k])
        state.pending = state.n_avg
        return state.inputs

    def _flowedit_step(self, state: "FlowEditState", model_output: torch.Tensor):
        """step(flowedit=state): one forward's update, Z += mask * coef * (Vt - Vs) (lx_flowedit_step), coef = flowedit_coefficient(...);
        the step index advances after the n_avg-th."""
        if not isinstance(state, FlowEditState):
            raise ValueError(f"step(flowedit=...): expected a FlowEditState, got {type(state).__name__}")
        if not state.pending:
            raise ValueError("step(flowedit=...): no inputs are pending; call flowedit_inputs(state, noises) for this step first")
        i = self._step_index
        want = (2 * state.X.shape[0],) + tuple(state.X.shape[1:])
        if tuple(model_output.shape) != want or model_output.device != state.Z.device:
            raise ValueError(f"step(flowedit=...): model_output {tuple(model_output.shape)} must be [target; source] of shape {want} on the "
                             "state's device")
        v = model_output if model_output.dtype in (torch.float32, torch.bfloat16) else model_output.float()
        coef = flowedit_coefficient(self._sig_host, i, state.n_avg)
        ops.flowedit_step(state.Z, v.contiguous(), coef, state.mask)
        state.taken.append((i, float(self._sig_host[i]), coef))
        state.pending -= 1
        if not state.pending:
            self._step_index += 1
        return (state.Z,)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = False, inpaint=None, true_cfg_scale=None,
             brain_guidance_scale=None, apg=None, multistep=None, flowedit=None):
        """prev = sample(fp32) + (sigma_next - sigma) * model_output, cast to model_output.dtype (diffusers semantics).
        inpaint = (image_latents, noise, mask), fp32 contiguous in sample's shape: prev is then blended with the source noised to the next
        level, mask * prev + (1 - mask) * scale_noise(image_latents, sigma_next, noise), in the same launch (lx_euler_step_blend).
        true_cfg_scale = s: sample and model_output have a leading dimension 2B, [positive; negative]; both halves of prev are the step of
        the positive half along neg + s * (pos - neg) (diffusers' FluxPipeline true CFG), in one launch (lx_euler_step_cfg). inpaint then has
        the shape of one half.
        brain_guidance_scale = s_b (> 1; generate's guidance along the brain signal): alone, the leading dimension is 2B, [full; text], and
        the step is the same launch along text + s_b * (full - text). With true_cfg_scale = s_t as well the leading dimension is 3B,
        [full; text; negative], and all three parts of prev are the step of the first along neg + s_t * (text + s_b * (full - text) - neg),
        in one launch (lx_euler_step_cfg3). inpaint has the shape of one part.
        apg = an ApgState made for one part's shape (generate's apg_eta / apg_norm_threshold / apg_momentum): only together with
        true_cfg_scale and/or brain_guidance_scale. The same batch, stepped by lx_euler_step_apg instead: the total guidance update is
        clamped, given momentum and projected on the first branch's denoised prediction, per image; the state's next row of sums is written
        on the device. Without apg the method launches what it launched before.
        multistep = a MultistepState made for one part's shape (generate's solver="dpmpp_2m"): the step is DPM-Solver++(2M), the same step
        plus c * (D - D_prev) with D = sample - sigma * velocity the denoised prediction along whatever velocity the step runs (guided,
        projected under apg) and c = multistep_coefficient(...), 0 on the state's first step; one launch of lx_dpmpp2m_step, or of
        lx_dpmpp2m_step_apg with apg, in place of the Euler entries. The state keeps D and records c. Without it nothing changes.
        flowedit = a FlowEditState whose inputs flowedit_inputs() formed for this step (generate's source_prompt): model_output is one
        forward's [target; source] velocities, `sample` is not read, and the edit state gets Z += mask * coef * (Vt - Vs) in one launch
        of lx_flowedit_step, coef = (sigma_next - sigma) / n_avg; the step index advances after the n_avg-th forward. Returns (Z,), the
        state's own fp32 buffer. With none of the other keywords: FlowEdit's velocity is the difference of its two branches."""
        if flowedit is not None:
            if inpaint is not None or true_cfg_scale is not None or brain_guidance_scale is not None or apg is not None or multistep is not None:
                raise ValueError("step(flowedit=...): FlowEdit steps along the difference of its two branches; inpaint, true_cfg_scale, "
                                 "brain_guidance_scale, apg and multistep do not combine with it (its mask belongs to the state)")
            return self._flowedit_step(flowedit, model_output)
        if apg is not None and brain_guidance_scale is None and true_cfg_scale is None:
            raise ValueError("step(apg=...): adaptive projected guidance acts on a guidance update; pass true_cfg_scale and/or "
                             "brain_guidance_scale with it")
        i = self._step_index
        ds, sigma_next = float(np.float32(self._sig_host[i + 1]) - np.float32(self._sig_host[i])), float(self._sig_host[i + 1])
        x = sample.to(torch.float32).clone() if (sample.dtype != torch.float32 or not sample.is_contiguous()) else sample.clone()
        v = model_output if model_output.dtype in (torch.float32, torch.bfloat16) else model_output.float()
        half = tuple(x.shape)
        if brain_guidance_scale is not None and not float(brain_guidance_scale) > 1:
            raise ValueError(f"step(brain_guidance_scale={brain_guidance_scale}): must be > 1; without brain guidance pass None and the "
                             "batch without its text-only part")
        # the scales in the order the kernels take them; with them the batch has one more part, laid out as `layout` says
        scales = tuple(float(s) for s in (brain_guidance_scale, true_cfg_scale) if s is not None)
        parts = len(scales) + 1
        if parts > 1:
            keywords = ", ".join(k for k, s in (("true_cfg_scale=...", true_cfg_scale), ("brain_guidance_scale=...", brain_guidance_scale))
                                 if s is not None)
            layout = "[full; text; negative]" if parts == 3 else "[full; text]" if brain_guidance_scale is not None else "[positive; negative]"
            if x.dim() < 1 or x.shape[0] % parts or x.shape[0] == 0 or v.shape != x.shape:
                raise ValueError(f"step({keywords}): sample {tuple(x.shape)} and model_output {tuple(v.shape)} must have one shape with "
                                 f"{'a leading dimension that is a multiple of 3' if parts == 3 else 'an even leading dimension'}, {layout}")
            half = (x.shape[0] // parts,) + tuple(x.shape[1:])
        if inpaint is not None:
            x0, z, m = inpaint
            if not (tuple(x0.shape) == tuple(z.shape) == tuple(m.shape) == half):
                raise ValueError(f"step(inpaint=...): image_latents {tuple(x0.shape)}, noise {tuple(z.shape)} and mask {tuple(m.shape)} must "
                                 f"have the latents' shape {half}")
        if apg is not None:
            if tuple(apg.M.shape) != half or apg.M.dtype != torch.float32 or apg.sums.shape[1] != half[0] or not apg.step < apg.sums.shape[0]:
                raise ValueError(f"step(apg=...): the state (M {tuple(apg.M.shape)}, sums {tuple(apg.sums.shape)}, step {apg.step}) was not "
                                 f"made for parts of shape {half} or has run out of steps")
        if multistep is not None:
            if tuple(multistep.D.shape) != half or multistep.D.dtype != torch.float32:
                raise ValueError(f"step(multistep=...): the state (D {tuple(multistep.D.shape)}, {multistep.D.dtype}) was not made for parts "
                                 f"of shape {half} in float32")
            c = multistep_coefficient(self._sig_host, i, self._begin_index) if multistep.have else 0.0
            if apg is None:
                ops.dpmpp2m_step(x, v.contiguous(), float(self._sig_host[i]), ds, c, multistep.D, scales, inpaint, sigma_next)
            else:
                ops.dpmpp2m_step_apg(x, v.contiguous(), float(self._sig_host[i]), ds, c, multistep.D, scales, apg.eta, apg.norm_threshold,
                                     apg.momentum, apg.M, apg.sums[apg.step], apg.workspace, inpaint, sigma_next)
                apg.step += 1
            multistep.have = True
            multistep.coefficients.append(c)
        elif apg is not None:
            ops.euler_step_apg(x, v.contiguous(), float(self._sig_host[i]), ds, scales, apg.eta, apg.norm_threshold, apg.momentum, apg.M,
                               apg.sums[apg.step], apg.workspace, inpaint, sigma_next)
            apg.step += 1
        elif parts == 3:
            ops.euler_step_cfg3(x, v.contiguous(), ds, *scales, inpaint, sigma_next)
        elif parts == 2:
            ops.euler_step_cfg(x, v.contiguous(), ds, *scales, inpaint, sigma_next)
        elif inpaint is None:
            ops.euler_step(x, v.contiguous(), ds)
        else:
            ops.euler_step_blend(x, v.contiguous(), ds, x0, z, m, sigma_next)
        self._step_index += 1
        return (x.to(model_output.dtype),)


def retrieve_timesteps(scheduler, num_inference_steps=None, device=None, timesteps=None, sigmas=None, **kwargs):
    if timesteps is not None:
        raise ValueError("custom `timesteps` are not supported by the flow-match scheduler")
    scheduler.set_timesteps(num_inference_steps, device=device, sigmas=sigmas, **kwargs)
    return scheduler.timesteps, len(scheduler.timesteps)


class LxFluxPipeline:
    vae_scale_factor = 16
    default_sample_size = 64

    def __init__(self, transformer, scheduler=None, vae=None, text_encoder=None, image_processor=None):
        """vae: an `LxAutoencoderKL` (loongx_amd/vae.py) or any object with its encode / decode / config surface;
        text_encoder: a callable (prompt, prompt_2, max_sequence_length) -> (prompt_embeds, pooled), e.g. `FluxTextEncoders`;
        image_processor defaults to the diffusers-0.31 `VaeImageProcessor(vae_scale_factor=16)` when a VAE is given."""
        self.transformer = transformer
        self.scheduler = scheduler or FlowMatchEulerDiscreteScheduler()
        if vae is not None and image_processor is None:
            from ..vae import VaeImageProcessor
            image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor)
        self.vae, self.text_encoder, self.image_processor = vae, text_encoder, image_processor
        self.device = transformer.device
        self.dtype = torch.float32
        self._guidance_scale, self._joint_attention_kwargs, self._interrupt, self._num_timesteps = 3.5, None, False, 0

    # ---- properties generate() reads ------------------------------------------------------------
    @property
    def _execution_device(self):
        return self.device

    @property
    def interrupt(self):
        return self._interrupt

    @property
    def joint_attention_kwargs(self):
        return self._joint_attention_kwargs

    def to(self, *a, **k):
        return self

    @classmethod
    def from_pretrained(cls, path: str, device="cuda", dtype=torch.bfloat16, flux_config=None, lora_scale: float = 1.0,
                        load_vae: bool = True, load_text_encoders: bool = True):
        """A LOCAL diffusers-format FLUX.1 directory (the reference passes a hub id to FluxPipeline.from_pretrained,
        src/train/model.py:399-401; the box has no hub access): `transformer/` (safetensors, sharded or single) is packed for the
        MI355X engine; `vae/` becomes an `LxAutoencoderKL`; `text_encoder*/` + `tokenizer*/` a `FluxTextEncoders` (transformers on
        ROCm). Missing optional parts leave the corresponding slot empty. dtype float32 selects the engine's precise mode, float16 its
        fp16 operand mode (bfloat16: bf16 operands). The VAE follows the transformer into precise mode (`LxAutoencoderKL(precise=True)`:
        split-bf16 operand pairs) and into the fp16 operand mode (`LxAutoencoderKL(operands="fp16")`: fp16 operand images, saturation counted
        and reported per encode / decode under model_config["f16_overflow"]); bfloat16 runs it on bf16 operands."""
        import json
        import os
        from safetensors.torch import load_file
        from .transformer import LxFluxTransformer
        from .weights import FluxConfig

        def load_dir(d):
            idx = [f for f in os.listdir(d) if f.endswith(".safetensors.index.json")]
            if idx:
                files = sorted(set(json.load(open(os.path.join(d, idx[0])))["weight_map"].values()))
            else:
                files = sorted(f for f in os.listdir(d) if f.endswith(".safetensors"))
            if not files:
                raise FileNotFoundError(f"no .safetensors weights in {d}")
            sd = {}
            for f in files:
                sd.update(load_file(os.path.join(d, f)))
            return sd

        tdir = os.path.join(path, "transformer")
        if not os.path.isdir(tdir):
            raise FileNotFoundError(f"{path}: no transformer/ directory (expected a diffusers-format FLUX.1 checkpoint)")
        cfg = flux_config
        cj = os.path.join(tdir, "config.json")
        if cfg is None and os.path.isfile(cj):
            c = json.load(open(cj))
            cfg = FluxConfig(num_layers=c.get("num_layers", 19), num_single_layers=c.get("num_single_layers", 38),
                             num_attention_heads=c.get("num_attention_heads", 24), attention_head_dim=c.get("attention_head_dim", 128),
                             in_channels=c.get("in_channels", 64), joint_attention_dim=c.get("joint_attention_dim", 4096),
                             pooled_projection_dim=c.get("pooled_projection_dim", 768), guidance_embeds=c.get("guidance_embeds", True),
                             axes_dims_rope=tuple(c.get("axes_dims_rope", (16, 56, 56))))
        tsd = load_dir(tdir)
        tr = LxFluxTransformer.from_state_dict(tsd, cfg or FluxConfig.from_state_dict(tsd), device, lora_scale, precise=dtype == torch.float32,
                                              operands="fp16" if dtype == torch.float16 else "bf16")
        vae = text = None
        vdir = os.path.join(path, "vae")
        if load_vae and os.path.isdir(vdir):
            from ..vae import LxAutoencoderKL
            vc = json.load(open(os.path.join(vdir, "config.json"))) if os.path.isfile(os.path.join(vdir, "config.json")) else {}
            keep = ("in_channels", "out_channels", "latent_channels", "block_out_channels", "layers_per_block", "norm_num_groups",
                    "scaling_factor", "shift_factor")
            vae = LxAutoencoderKL(load_dir(vdir), {k: vc[k] for k in keep if k in vc}, device, precise=dtype == torch.float32,
                                  operands="fp16" if dtype == torch.float16 else "bf16")
        if load_text_encoders and all(os.path.isdir(os.path.join(path, d)) for d in ("text_encoder", "tokenizer", "text_encoder_2", "tokenizer_2")):
            from .text import FluxTextEncoders
            text = FluxTextEncoders.from_pretrained(path, device, dtype)
        return cls(tr, vae=vae, text_encoder=text)

    def load_lora_weights(self, path: str, weight_name: str = "pytorch_lora_weights.safetensors", lora_scale: float = 1.0,
                          adapter_name: Optional[str] = None, **kwargs):
        """diffusers `FluxPipeline.load_lora_weights` for the transformer (model.py:472): `path` is the directory the
        reference saves with `save_lora` (model.py:526-531) or the .safetensors file itself. Without `adapter_name` it replaces the
        adapters of the packed model in place (one adapter, "default", active). With a name it adds or replaces that adapter and leaves
        the others -- and a non-empty active set -- as they are: set_adapters selects. Either way every cached graph / conditioning
        that baked the old ones in is dropped."""
        import os
        from .weights import install_lora
        f = os.path.join(path, weight_name) if os.path.isdir(path) else path
        if not os.path.isfile(f):
            raise FileNotFoundError(f"no LoRA weights at {f}")
        if f.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(f)
        else:
            sd = torch.load(f, map_location="cpu")
        eng = self.transformer.engine
        n = install_lora(eng.w, sd, lora_scale=lora_scale, adapter_name=adapter_name)
        if adapter_name is None:
            eng.adapter_weights = {}
        self._adapters_changed()
        return n

    def _adapters_changed(self) -> None:
        self.transformer.engine.drop_graphs_and_shape()
        self.transformer.invalidate_conditioning()

    def set_adapters(self, adapter_names, adapter_weights=None):
        """diffusers `set_adapters`: run with the loaded adapters `adapter_names` (a name or a list; stacked in this order) at
        `adapter_weights`: a float for all of them, or one item per name, each a float or a sequence / tensor with one value per image
        of the batch (checked against the batch when the next image is conditioned). Default 1. engine.lora_scale (lora_controller)
        multiplies on top. An unknown name is a ValueError that lists the loaded ones and changes nothing."""
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        if adapter_weights is None:
            weights = {}
        elif isinstance(adapter_weights, (list, tuple)):
            if len(adapter_weights) != len(names):
                raise ValueError(f"{len(adapter_weights)} adapter weights for {len(names)} adapters")
            weights = dict(zip(names, adapter_weights))
        else:
            weights = {n: adapter_weights for n in names}
        eng = self.transformer.engine
        before = (eng.w.lora_version, eng.adapter_weights_key())
        eng.set_adapters(names, weights)
        if (eng.w.lora_version, eng.adapter_weights_key()) != before:       # (selecting what is selected keeps the step graphs)
            self._adapters_changed()

    def get_active_adapters(self):
        from .weights import active_adapters
        return active_adapters(self.transformer.engine.w)

    def get_list_adapters(self):
        """diffusers returns {component: [names]}; the transformer is the one component that carries adapters here."""
        from .weights import list_adapters
        return {"transformer": list_adapters(self.transformer.engine.w)}

    def delete_adapters(self, adapter_names):
        from .weights import delete_adapters
        eng = self.transformer.engine
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        delete_adapters(eng.w, names)
        eng.adapter_weights = {k: v for k, v in eng.adapter_weights.items() if k not in names}
        self._adapters_changed()

    def maybe_free_model_hooks(self):
        pass

    @contextmanager
    def progress_bar(self, total=None):
        yield SimpleNamespace(update=lambda *a, **k: None)

    # ---- input handling ---------------------------------------------------------------------------
    def check_inputs(self, prompt, prompt_2, height, width, prompt_embeds=None, pooled_prompt_embeds=None,
                     callback_on_step_end_tensor_inputs=None, max_sequence_length=None):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError("Cannot forward both `prompt` and `prompt_embeds`.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`.")
        if prompt is not None and not isinstance(prompt, (str, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if prompt_embeds is not None and pooled_prompt_embeds is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed.")
        if max_sequence_length is not None and max_sequence_length > 512:
            raise ValueError(f"`max_sequence_length` cannot be greater than 512 but is {max_sequence_length}")

    def encode_prompt(self, prompt=None, prompt_2=None, prompt_embeds=None, pooled_prompt_embeds=None, device=None,
                      num_images_per_prompt: int = 1, max_sequence_length: int = 512, lora_scale=None):
        if prompt_embeds is None:
            if self.text_encoder is None:
                raise NotImplementedError("T5/CLIP text encoding is outside the MI355X hot path: pass prompt_embeds / "
                                          "pooled_prompt_embeds, or construct LxFluxPipeline(text_encoder=callable)")
            prompt_embeds, pooled_prompt_embeds = self.text_encoder(prompt, prompt_2, max_sequence_length)
        if num_images_per_prompt != 1:
            prompt_embeds = prompt_embeds.repeat_interleave(num_images_per_prompt, dim=0)
            pooled_prompt_embeds = pooled_prompt_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        text_ids = torch.zeros(prompt_embeds.shape[1], 3, device=device or self.device, dtype=torch.float32)
        return prompt_embeds.to(device or self.device), pooled_prompt_embeds.to(device or self.device), text_ids

    # ---- latents -----------------------------------------------------------------------------------
    @staticmethod
    def _pack_latents(latents, batch_size, num_channels_latents, height, width):
        x = latents.view(batch_size, num_channels_latents, height // 2, 2, width // 2, 2).permute(0, 2, 4, 1, 3, 5)
        return x.reshape(batch_size, (height // 2) * (width // 2), num_channels_latents * 4)

    @staticmethod
    def _unpack_latents(latents, height, width, vae_scale_factor):
        b, n, ch = latents.shape
        h, w = height // vae_scale_factor, width // vae_scale_factor
        x = latents.view(b, h, w, ch // 4, 2, 2).permute(0, 3, 1, 4, 2, 5)
        return x.reshape(b, ch // 4, h * 2, w * 2)

    @staticmethod
    def _prepare_latent_image_ids(batch_size, height, width, device, dtype):
        """diffusers 0.31: `height`/`width` are the UNPACKED latent sizes; ids live on the (h/2, w/2) grid."""
        h2, w2 = height // 2, width // 2
        ids = torch.zeros(h2, w2, 3)
        ids[..., 1] += torch.arange(h2)[:, None]
        ids[..., 2] += torch.arange(w2)[None, :]
        return ids.reshape(h2 * w2, 3).to(device=device, dtype=dtype)

    # ---- img2img / inpaint (diffusers FluxImg2ImgPipeline / FluxInpaintPipeline) ---------------------------
    def get_timesteps(self, num_inference_steps, strength, device=None):
        """diffusers' get_timesteps, after the scheduler's set_timesteps: the tail of the schedule that `strength` leaves. Returns
        (timesteps[t_start:], num_inference_steps - t_start, timesteps_host[t_start:]) -- the third item is the host copy of the first, so
        that callers can hand the remaining schedule on without a device read -- and sets the scheduler's begin index to t_start."""
        init_timestep = min(num_inference_steps * strength, num_inference_steps)
        t_start = int(max(num_inference_steps - init_timestep, 0))
        if num_inference_steps - t_start < 1:
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline steps is "
                             f"{num_inference_steps - t_start} which is < 1 and not appropriate for this pipeline.")
        timesteps, _, timesteps_host = self.get_timesteps_from(t_start)
        return timesteps, num_inference_steps - t_start, timesteps_host

    def get_timesteps_from(self, t_start: int, device=None):
        """get_timesteps with the start given as a step of the schedule, not as a strength (FlowEdit begins at T - n_max): after the
        scheduler's set_timesteps, returns (timesteps[t_start:], T - t_start, timesteps_host[t_start:]) and sets the scheduler's begin index
        to t_start. Anything but an int in [0, T) is a ValueError."""
        sch = self.scheduler
        if sch.timesteps is None:
            raise ValueError("get_timesteps_from: call the scheduler's set_timesteps first")
        total = len(sch.timesteps_host) // sch.order
        if isinstance(t_start, bool) or not isinstance(t_start, (int, np.integer)) or not 0 <= int(t_start) < total:
            raise ValueError(f"get_timesteps_from({t_start!r}): the start must be an int in [0, {total})")
        t_start = int(t_start)
        sch.set_begin_index(t_start * sch.order)
        return sch.timesteps[t_start * sch.order:], total - t_start, sch.timesteps_host[t_start * sch.order:]

    @staticmethod
    def pack_mask(mask, batch, height, width):
        """A pixel mask (white / 1: repaint) -> the packed latent mask [batch, N, 64] fp32 of a height x width image, in diffusers' order
        (mask_processor, then FluxInpaintPipeline.prepare_mask_latents): binarise at 0.5, nearest-neighbour resize to the unpacked latent
        grid 2*(height//16) x 2*(width//16), repeat over the 16 latent channels, _pack_latents. `mask`: a PIL image (converted to "L"), a
        numpy array or a tensor of shape [H, W], [1, H, W] or [1|batch, 1, H, W]; integer types are 0..255, bool and floating types 0..1.
        Once per image in torch, on the mask's device (the CPU for PIL / numpy)."""
        if hasattr(mask, "convert") and hasattr(mask, "size"):                 # PIL
            mask = np.array(mask.convert("L"))
        if not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(mask))
        if mask.dtype == torch.bool:
            mask = mask.to(torch.float32)
        elif not mask.dtype.is_floating_point:
            mask = mask.to(torch.float32) / 255.0
        mask = mask.to(torch.float32)
        if mask.dim() == 2:
            mask = mask[None, None]
        elif mask.dim() == 3 and mask.shape[0] == 1:
            mask = mask[None]
        if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[0] not in (1, batch):
            raise ValueError(f"mask_image must be [H, W], [1, H, W] or [1|{batch}, 1, H, W], got {tuple(mask.shape)}")
        mask = (mask >= 0.5).to(torch.float32)
        h, w = 2 * (int(height) // LxFluxPipeline.vae_scale_factor), 2 * (int(width) // LxFluxPipeline.vae_scale_factor)
        mask = torch.nn.functional.interpolate(mask, size=(h, w), mode="nearest")
        mask = mask.expand(batch, 1, h, w).repeat(1, 16, 1, 1)
        return LxFluxPipeline._pack_latents(mask, batch, 16, h, w).contiguous()

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        height = 2 * (int(height) // self.vae_scale_factor)
        width = 2 * (int(width) // self.vae_scale_factor)
        ids = self._prepare_latent_image_ids(batch_size, height, width, device, torch.float32)
        if latents is not None:
            return latents.to(device=device, dtype=dtype), ids
        shape = (batch_size, num_channels_latents, height, width)
        gdev = generator.device if isinstance(generator, torch.Generator) else device
        noise = torch.randn(shape, generator=generator if isinstance(generator, torch.Generator) else None, device=gdev, dtype=dtype)
        return self._pack_latents(noise.to(device), batch_size, num_channels_latents, height, width), ids
