"""generate(image= | image_latents=, mask_image= | latent_mask=, strength=): diffusers' FluxImg2ImgPipeline / FluxInpaintPipeline semantics on
the tiny transformer and the inputs of tests/test_api_gpu.py::test_generate_matches_oracle_loop (2 + 2 blocks, 2 heads, 64x64 pixels = 16
tokens, 4 steps, latents in and out, one Condition(latents=...)).

What is promised bit for bit: the kept region of the result IS the source (in every operand mode, for every image of a batch, from pixels
as well as from latents), and a call that asks for nothing -- no source, or a source with strength 1 and a mask of ones or none -- returns
what it returned before the arguments existed. What is promised within the unmasked loop's tolerance: the loop restated on the oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_modules as fm  # noqa: E402
from oracle import flux_ref as fr  # noqa: E402
from tests.helpers import relerr  # noqa: E402
from tests.test_api_gpu import TOL_GEN, _mk_model  # noqa: E402  (the bound of the unmasked 4-step loops, and their model)

HW, N, STEPS = 4, 16, 4


@pytest.fixture(scope="module")
def S():
    """the model, the inputs, and the plain result that every "nothing changed" assertion compares with"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from types import SimpleNamespace
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    tr = fm.FluxTransformer2DModel(num_layers=2, num_single_layers=2, heads=2, head_dim=128, in_channels=64, joint_dim=4096,
                                   pooled_dim=768, guidance_embeds=True, lora=True)
    fm.init_synthetic_(tr, seed=4, std=0.03, bias_std=0.02, norm_jitter=0.1)
    tr.eval()
    _, model = _mk_model(tr)
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(1, N, 64, generator=g)
    cond = torch.randn(1, N, 64, generator=g)
    pe, pooled = torch.randn(1, 512, 4096, generator=g) * 0.1, torch.randn(1, 768, generator=g)
    x0 = torch.randn(1, N, 64, generator=g)
    lat2 = torch.randn(2, N, 64, generator=g)
    half = torch.zeros(1, N, 1)
    half[:, 8:] = 1.0
    soft = torch.full((1, N, 64), 0.25)
    soft[:, 8:] = 0.75
    s = SimpleNamespace(tr=tr, model=model, pipe=model.flux_pipe, lat=lat, cond=cond, pe=pe, pooled=pooled, x0=x0, lat2=lat2, half=half, soft=soft)

    def run(pipe=None, latents=lat, **kw):
        c = Condition("subject", latents=cond.cuda(), latent_hw=(HW, HW), position_delta=[0, -HW])
        kw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        kw.setdefault("model_config", {})
        return generate(model, pipe or model.flux_pipe, conditions=[c], height=HW * 16, width=HW * 16, num_inference_steps=STEPS,
                        latents=latents.cuda(), prompt_embeds=pe.cuda(), pooled_prompt_embeds=pooled.cuda(), output_type="latent",
                        default_lora=True, use_brain_condition=False, **kw).images
    s.run = run
    s.plain = run().clone()
    return s


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_kept_region_is_the_source_and_the_callback_sees_the_blend(S):
    """latent_mask 0 on tokens 0..7, 1 on 8..15, strength 1: after every step the kept tokens are the source noised to the next level (what
    lx_scale_noise gives for it, bit for bit), and after the last one the source itself."""
    from loongx_amd import ops
    seen = []

    def cb(pipe, i, t, kw):
        seen.append((i, kw["latents"].clone()))
        return {}
    out = S.run(image_latents=S.x0, latent_mask=S.half, strength=1.0, callback_on_step_end=cb)
    assert same_bits(out[:, :8], S.x0.cuda()[:, :8]), "the kept tokens are not the source"
    assert not torch.equal(out[:, 8:], S.x0.cuda()[:, 8:]) and not torch.equal(out[:, 8:], S.plain[:, 8:])      # (repainted, next to a kept half)
    assert [i for i, _ in seen] == list(range(STEPS))
    sig = S.pipe.scheduler._sig_host
    for i, l in seen:
        want = ops.scale_noise(S.x0.cuda(), S.lat.cuda(), float(sig[i + 1]))
        assert same_bits(l[:, :8], want[:, :8]), f"step {i}: the kept tokens are not the source at sigma[{i + 1}]"
    assert same_bits(seen[-1][1], out)


def ref_loop(S, strength, mask):
    """start = sigma z + (1 - sigma) x0 at sigma[t_start]; Euler; blend with the source at the next sigma: on the oracle, in fp32 torch"""
    sch = fm.FlowMatchEulerDiscreteScheduler()
    cfg = sch.config
    mu = fm.calculate_shift(N, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / STEPS, STEPS), device="cpu", mu=mu)
    t_start = int(max(STEPS - min(STEPS * strength, STEPS), 0))
    sig, z, x0 = sch.sigmas, S.lat, S.x0
    ids = fm.prepare_latent_image_ids(HW, HW)
    cids = ids.clone()
    cids[:, 2] -= HW
    x = sig[t_start] * z + (1 - sig[t_start]) * x0
    with torch.no_grad():
        for i in range(t_start, STEPS):
            v = fr.tranformer_forward(S.tr, S.cond, cids, None, {}, hidden_states=x, encoder_hidden_states=S.pe, pooled_projections=S.pooled,
                                      timestep=sch.timesteps[i].expand(1) / 1000, img_ids=ids, txt_ids=torch.zeros(512, 3),
                                      guidance=torch.full((1,), 3.5))[0]
            x = x + (sig[i + 1] - sig[i]) * v
            if mask is not None:
                x = mask * x + (1 - mask) * (sig[i + 1] * z + (1 - sig[i + 1]) * x0)
    return x, STEPS - t_start


@pytest.mark.parametrize("mask", ["none", "half", "soft"])
@pytest.mark.parametrize("strength", [1.0, 0.5])
def test_against_the_restated_loop(S, strength, mask):
    m = {"none": None, "half": S.half, "soft": S.soft}[mask]
    want, n_fwd = ref_loop(S, strength, m)
    calls = []

    def cb(pipe, i, t, kw):
        calls.append(i)
        return {}
    out = S.run(image_latents=S.x0, strength=strength, callback_on_step_end=cb, **({} if m is None else {"latent_mask": m}))
    err = relerr(out.cpu(), want)
    print(f"strength {strength} mask {mask}: relative L2 {err:.2e} (bound {TOL_GEN:.1e}), {len(calls)} forwards")
    assert err < TOL_GEN
    assert len(calls) == n_fwd == (2 if strength == 0.5 else STEPS)
    assert same_bits(S.run(), S.plain), "a plain call after a partial schedule changed"


def test_nothing_changes_when_nothing_is_asked(S):
    ones = torch.ones(1, N, 64)
    assert same_bits(S.run(image_latents=S.x0, latent_mask=ones, strength=1.0), S.plain)
    assert same_bits(S.run(image_latents=S.x0, strength=1.0), S.plain)
    assert same_bits(S.run(), S.plain)


@pytest.mark.parametrize("mode", ["fp16", "precise"])
def test_kept_region_in_the_other_operand_modes(S, mode):
    mc, pipe = {"operands": "fp16"}, None
    if mode == "precise":                                       # (the split mode needs weights packed with their bf16 rounding residuals)
        from loongx_amd.flux.pipeline import LxFluxPipeline
        from loongx_amd.flux.transformer import LxFluxTransformer
        from loongx_amd.flux.weights import FluxConfig
        cfg = FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2, in_channels=64, joint_attention_dim=4096,
                         pooled_projection_dim=768, guidance_embeds=True)
        mc, pipe = {"precise": True}, LxFluxPipeline(LxFluxTransformer.from_state_dict(S.tr.state_dict(), cfg, "cuda", precise=True))
    out = S.run(pipe=pipe, image_latents=S.x0, latent_mask=S.half, strength=1.0, model_config=mc)
    assert same_bits(out[:, :8], S.x0.cuda()[:, :8])
    assert bool(torch.isfinite(out).all()) and not torch.equal(out[:, 8:], S.x0.cuda()[:, 8:])


def test_batch_of_two_from_a_batch_one_source_and_mask(S):
    out = S.run(latents=S.lat2, image_latents=S.x0, latent_mask=S.half, strength=1.0, num_images_per_prompt=2)
    assert out.shape == (2, N, 64)
    for b in range(2):
        assert same_bits(out[b, :8], S.x0.cuda()[0, :8]), f"image {b}: the kept tokens are not the source"
    assert not torch.equal(out[0, 8:], out[1, 8:])


def test_pixels_in(S):
    """image= a 64x64 PIL photo through the tiny VAE of the checkpoint tests, mask_image= a PIL "L" mask whose upper half is black: the kept
    tokens are the tokens encode_images returns for the photo under the same seed (the source is generate's first draw from the global
    generator)."""
    from PIL import Image
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.pipeline_tools import encode_images
    from loongx_amd.vae import LxAutoencoderKL
    from tests import tiny_ckpt
    pipe = LxFluxPipeline(S.model.transformer, vae=LxAutoencoderKL(tiny_ckpt.tiny_vae().state_dict(), tiny_ckpt.VAE_CFG, "cuda"))
    photo = Image.fromarray((np.random.default_rng(7).random((64, 64, 3)) * 255).astype("uint8"))
    m = np.zeros((64, 64), np.uint8)
    m[32:] = 255                                                # latent rows 4..7 -> packed rows 2, 3 -> tokens 8..15 repainted
    torch.manual_seed(11)
    tokens, _ = encode_images(pipe, photo)
    assert tokens.shape == (1, N, 64)
    torch.manual_seed(11)
    out = S.run(pipe=pipe, image=photo, mask_image=Image.fromarray(m), strength=1.0)
    assert same_bits(out[:, :8], tokens.float()[:, :8])
    assert not torch.equal(out[:, 8:], tokens.float()[:, 8:])
    with pytest.raises(NotImplementedError, match="VAE"):      # (no VAE: what a condition image gets)
        S.run(image=photo, mask_image=Image.fromarray(m))
    assert same_bits(S.run(), S.plain)


def test_a_small_strength_leaves_one_step(S):
    """strength 0.2 of 4 steps: t_start = int(4 - 0.8) = 3, so one forward runs, from sigma[3]"""
    calls = []
    S.run(image_latents=S.x0, strength=0.2, callback_on_step_end=lambda p, i, t, k: calls.append(i) or {})
    assert calls == [0]
    assert same_bits(S.run(), S.plain)


def _bad(v):
    t = torch.full((1, N, 1), 0.5)
    t[0, 3, 0] = v
    return t


ERRORS = {
    "strength_above": dict(image_latents="x0", strength=1.5),
    "strength_below": dict(image_latents="x0", strength=-0.1),
    "strength_nan": dict(image_latents="x0", strength=float("nan")),
    "no_step_left": dict(image_latents="x0", strength=0.0),
    "image_and_latents": dict(image=object(), image_latents="x0"),
    "both_masks": dict(image_latents="x0", mask_image=np.ones((64, 64), np.float32), latent_mask="half"),
    "mask_without_source": dict(latent_mask="half"),
    "pixel_mask_without_source": dict(mask_image=np.ones((64, 64), np.float32)),
    "strength_without_source": dict(strength=0.5),
    "source_tokens": dict(image_latents=torch.zeros(1, N + 1, 64)),
    "source_batch": dict(image_latents=torch.zeros(3, N, 64)),
    "source_channels": dict(image_latents=torch.zeros(1, N, 16)),
    "mask_tokens": dict(image_latents="x0", latent_mask=torch.ones(1, N - 1, 64)),
    "mask_batch": dict(image_latents="x0", latent_mask=torch.ones(2, N, 1)),
    "mask_channels": dict(image_latents="x0", latent_mask=torch.ones(1, N, 2)),
    "mask_above_one": dict(image_latents="x0", latent_mask=_bad(1.5)),
    "mask_negative": dict(image_latents="x0", latent_mask=_bad(-0.25)),
    "mask_nan": dict(image_latents="x0", latent_mask=_bad(float("nan"))),
    "mask_inf": dict(image_latents="x0", latent_mask=_bad(float("inf"))),
}


@pytest.mark.parametrize("case", list(ERRORS))
def test_refusals_leave_the_pipeline_as_it_was(S, case):
    kw = {k: (getattr(S, v) if isinstance(v, str) else v) for k, v in ERRORS[case].items()}
    with pytest.raises(ValueError):
        S.run(condition_scale=2.0, **kw)                          # (a refused call must not leave its condition_scale behind either)
    assert S.model.transformer.c_factor is None
    assert same_bits(S.run(), S.plain), "a plain call after the refused one changed"


def test_fp16_fallback_restarts_the_same_trajectory(S):
    """model_config["f16_overflow"] = "fallback" on a model whose fp16 operands saturate (the planted bias of tests/test_f16_gpu.py): the
    image is computed again with bf16 operands from the same start latents, the same t_start and under the same blend -- bit-equal to asking
    for bf16 in the first place, two forwards each time at strength 0.5."""
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    from tests.test_f16_gpu import _planted_model
    model = _planted_model(bias_value=1.0e5)
    calls = []

    def run(mc):
        c = Condition("subject", latents=S.cond.cuda(), latent_hw=(HW, HW), position_delta=[0, -HW])
        return generate(model, model.flux_pipe, conditions=[c], height=HW * 16, width=HW * 16, num_inference_steps=STEPS, latents=S.lat.cuda(),
                        prompt_embeds=S.pe.cuda(), pooled_prompt_embeds=S.pooled.cuda(), output_type="latent", model_config=mc,
                        default_lora=True, use_brain_condition=False, image_latents=S.x0.cuda(), latent_mask=S.half.cuda(), strength=0.5,
                        callback_on_step_end=lambda p, i, t, k: calls.append(i) or {})
    want = run({"operands": "bf16"}).images.clone()
    assert calls == [0, 1]
    with pytest.warns(RuntimeWarning, match="recomputing this image with bf16 operands"):
        out = run({"operands": "fp16", "f16_overflow": "fallback"})
    assert calls == [0, 1, 0, 1, 0, 1] and out.lx_operands.startswith("bf16")
    assert same_bits(out.images, want) and same_bits(out.images[:, :8], S.x0.cuda()[:, :8])
