"""Mirror of the reference's src/flux/pipeline_tools.py (encode_images :7-30, prepare_text_input :33-52)."""
from __future__ import annotations

import torch


def encode_images(pipeline, images, f16_overflow=None):
    """VAE-encode + (x - shift) * scale + 2x2 pack + ids.  Needs `pipeline.vae`; VAE-free callers hand packed
    latents to `Condition(latents=...)` instead (the VAE is outside the denoise hot path).
    f16_overflow: model_config["f16_overflow"] for this call, for a VAE on fp16 operands (None: the VAE's own setting)."""
    from .generate import vae_f16_overflow
    if pipeline.vae is None or pipeline.image_processor is None:
        raise NotImplementedError("encode_images needs a VAE: construct LxFluxPipeline(vae=..., image_processor=...) or "
                                  "pass pre-encoded packed latents via Condition(latents=...)")
    images = pipeline.image_processor.preprocess(images)
    images = images.to(pipeline.device).to(pipeline.dtype)
    with vae_f16_overflow(pipeline.vae, f16_overflow):
        z = pipeline.vae.encode(images).latent_dist.sample()
    z = (z - pipeline.vae.config.shift_factor) * pipeline.vae.config.scaling_factor
    tokens = pipeline._pack_latents(z, *z.shape)
    ids = pipeline._prepare_latent_image_ids(z.shape[0], z.shape[2], z.shape[3], pipeline.device, torch.float32)
    if tokens.shape[1] != ids.shape[0]:   # pipelines whose id helper takes pre-halved sizes (reference :22-29)
        ids = pipeline._prepare_latent_image_ids(z.shape[0], z.shape[2] // 2, z.shape[3] // 2, pipeline.device, torch.float32)
    return tokens, ids


def prepare_text_input(pipeline, prompts, max_sequence_length: int = 512):
    return pipeline.encode_prompt(prompt=prompts, prompt_2=None, prompt_embeds=None, pooled_prompt_embeds=None,
                                  device=pipeline.device, num_images_per_prompt=1, max_sequence_length=max_sequence_length,
                                  lora_scale=None)


def text_padding_mask(lengths, T: int, N: int, C: int = 0) -> torch.Tensor:
    """Key-padding attention_mask for prompts padded to T tokens: bool [B, 1, 1, T + N + C] over the concatenated
    [text | image | condition] sequence, False on the text keys t >= lengths[b] and True everywhere else (image and condition keys
    included). Hand it to tranformer_forward / generate as attention_mask (on the transformer's device): the padded keys leave every
    softmax, and 64-key tiles that hold padding only are never staged or multiplied. Pure torch; the result lives on `lengths`' device
    (the CPU for a list)."""
    lengths = torch.as_tensor(lengths, dtype=torch.long).reshape(-1)
    if T < 0 or N < 0 or C < 0:
        raise ValueError(f"text_padding_mask: negative length (T={T}, N={N}, C={C})")
    if lengths.numel() and (int(lengths.min()) < 0 or int(lengths.max()) > T):
        raise ValueError(f"text_padding_mask: lengths must lie in [0, T={T}]")
    m = torch.ones(lengths.numel(), 1, 1, T + N + C, dtype=torch.bool, device=lengths.device)
    m[:, 0, 0, :T] = torch.arange(T, device=lengths.device)[None, :] < lengths[:, None]
    return m
