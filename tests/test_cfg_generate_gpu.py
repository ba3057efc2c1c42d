"""generate(negative_prompt_embeds=, negative_pooled_prompt_embeds=, true_cfg_scale=): diffusers' FluxPipeline true classifier-free guidance
on the tiny transformer and the inputs of tests/test_inpaint_generate_gpu.py (2 + 2 blocks, 16 tokens, 4 steps, latents in and out, one
Condition(latents=...)), with negative embeddings drawn next from the same generator.

Both branches run as ONE batch of 2B per step and one lx_euler_step_cfg updates both halves. What is promised bit for bit: a call that does
not turn guidance on is the plain call; under the batch-invariant launch plans (engine.pair_plan = False) the guided call is two plain
forwards per step followed by the guided step, and equal branches are the plain call at any scale; kept tokens of an inpainted image are the
source. What is promised within a bound: the loop restated on the oracle, (2s - 1) * TOL_GEN."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_modules as fm  # noqa: E402
from oracle import flux_ref as fr  # noqa: E402
from tests.helpers import relerr  # noqa: E402
from tests.test_api_gpu import TOL_GEN, _mk_model  # noqa: E402
from tests.test_inpaint_generate_gpu import HW, N, STEPS, S, same_bits  # noqa: E402,F401  (S: the fixture -- model, inputs, plain result)

T = 512


@pytest.fixture(scope="module")
def C(S):  # noqa: F811
    """S's fields plus the negative embeddings (the next draws of S's generator: its own draws are repeated first), a call that returns
    generate()'s whole output, and a second, freshly built model on the batch-invariant launch plans with its own plain result.
    The namespace must not become a reference cycle: `out` closes over locals, never over the namespace that holds it. An engine that sits
    in cyclic garbage is freed whenever the collector next runs -- possibly while another engine captures its step graph, where freeing a
    captured graph aborts the process. The teardown lets go of everything here and collects at once, with nothing in flight."""
    import gc
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(3)
    for shape in ((1, N, 64), (1, N, 64), (1, 512, 4096), (1, 768), (1, N, 64), (2, N, 64)):       # lat, cond, pe, pooled, x0, lat2
        torch.randn(*shape, generator=g)
    neg_pe, neg_pooled = torch.randn(1, T, 4096, generator=g) * 0.1, torch.randn(1, 768, generator=g)
    model, pipe0, lat, cond, pe, pooled = S.model, S.pipe, S.lat, S.cond, S.pe, S.pooled
    _, model_inv = _mk_model(S.tr)
    pipe_inv = model_inv.flux_pipe
    pipe_inv.transformer.engine.pair_plan = False                    # (before the first step: the plans that do not depend on the batch size)

    def out(pipe=None, latents=lat, **kw):
        from loongx_amd.flux.condition import Condition
        from loongx_amd.flux.generate import generate
        c = Condition("subject", latents=cond.cuda(), latent_hw=(HW, HW), position_delta=[0, -HW])
        kw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
        kw.setdefault("model_config", {})
        pipe = pipe or pipe0
        return generate(model_inv if pipe is pipe_inv else model, pipe, conditions=[c], height=HW * 16, width=HW * 16,
                        num_inference_steps=STEPS, latents=latents.cuda(), prompt_embeds=pe.cuda(), pooled_prompt_embeds=pooled.cuda(),
                        output_type="latent", default_lora=True, use_brain_condition=False, **kw)
    c = SimpleNamespace(**vars(S), neg_pe=neg_pe, neg_pooled=neg_pooled, model_inv=model_inv, pipe_inv=pipe_inv, out=out,
                        neg=dict(negative_prompt_embeds=neg_pe, negative_pooled_prompt_embeds=neg_pooled),
                        plain_inv=out(pipe=pipe_inv).images.clone())
    yield c
    import weakref
    engine = weakref.ref(pipe_inv.transformer.engine)
    vars(c).clear()
    del c, out, model, model_inv, pipe0, pipe_inv
    torch.cuda.synchronize()
    freed = engine() is None                                         # (by reference count alone: it was in no cycle)
    gc.collect()
    assert freed, "the second model's engine was left to the cycle collector"


def quiet(f, *a, **kw):
    """f(...) with every RuntimeWarning (generate's category) an error: a call that must not warn"""
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        return f(*a, **kw)


# ------------------------------------------------------------------------------------------------------------------ off is off
def test_off_is_the_plain_call(C):
    with pytest.warns(RuntimeWarning, match="guidance is off"):
        assert same_bits(C.run(true_cfg_scale=1.0, **C.neg), C.plain)
    with pytest.warns(RuntimeWarning, match="without a negative prompt"):
        assert same_bits(C.run(true_cfg_scale=3.0), C.plain)
    assert same_bits(quiet(C.run), C.plain)
    assert C.pipe.transformer.engine.adapter_weight_tiles == 1


def test_on_does_something(C):
    out = quiet(C.run, true_cfg_scale=2.0, **C.neg)
    assert out.shape == C.plain.shape and bool(torch.isfinite(out).all()) and not torch.equal(out, C.plain)
    assert same_bits(quiet(C.run, true_cfg_scale=2.0, **C.neg), out), "two guided calls differ"
    assert same_bits(C.run(), C.plain), "a plain call after a guided one changed"


# ------------------------------------------------------------------------------------------------------------------ bit for bit
def test_equal_to_two_plain_forwards_per_step(C):
    """Under engine.pair_plan = False: positive then negative forward at batch B per step, invalidate_conditioning between them, then
    ops.euler_step_cfg on their concatenation -- the guided generate() gives those latents bit for bit (the batch invariance that
    LX_PAIR_PLAN=0 promises, here across the halves of a batch of 2B)."""
    from loongx_amd import ops
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.pipeline import calculate_shift, retrieve_timesteps
    from loongx_amd.flux.transformer import tranformer_forward
    pipe, scale = C.pipe_inv, 2.0
    got = C.out(pipe=pipe, true_cfg_scale=scale, **C.neg).images.clone()
    tr, sch = pipe.transformer, pipe.scheduler
    tokens, cids, tids = Condition("subject", latents=C.cond.cuda(), latent_hw=(HW, HW), position_delta=[0, -HW]).encode(pipe)
    lat, ids = pipe.prepare_latents(1, 16, HW * 16, HW * 16, torch.float32, "cuda", None, C.lat.cuda())
    cfg = sch.config
    mu = calculate_shift(N, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    timesteps, _ = retrieve_timesteps(sch, STEPS, "cuda", None, np.linspace(1.0, 1 / STEPS, STEPS), mu=mu)
    sched_ts = (sch.timesteps_host / np.float32(1000)).tolist()
    guidance = torch.full((1,), 3.5, device="cuda")
    txt_ids = torch.zeros(T, 3, device="cuda")
    x = torch.cat([lat, lat]).contiguous()
    for i, t in enumerate(timesteps):
        vs = []
        for pe, pooled in ((C.pe, C.pooled), (C.neg_pe, C.neg_pooled)):
            tr.invalidate_conditioning()
            vs.append(tranformer_forward(tr, model_config={}, condition_latents=tokens, condition_ids=cids, condition_type_ids=tids,
                                         hidden_states=x[:1], timestep=t.expand(1) / 1000, guidance=guidance, pooled_projections=pooled.cuda(),
                                         encoder_hidden_states=pe.cuda(), txt_ids=txt_ids, img_ids=ids, joint_attention_kwargs=None,
                                         return_dict=False, lx_schedule=(i, sched_ts))[0])
        ops.euler_step_cfg(x, torch.cat(vs).contiguous(), float(np.float32(sch._sig_host[i + 1]) - np.float32(sch._sig_host[i])), scale)
    tr.invalidate_conditioning()
    assert same_bits(got, x[:1]), f"{int((got != x[:1]).sum())} of {got.numel()} elements differ, relative L2 {relerr(got.cpu(), x[:1].cpu()):.2e}"
    assert same_bits(C.out(pipe=pipe).images, C.plain_inv)


def test_equal_branches_are_the_plain_call_at_any_scale(C):
    out = C.out(pipe=C.pipe_inv, true_cfg_scale=5.0, negative_prompt_embeds=C.pe, negative_pooled_prompt_embeds=C.pooled).images
    assert same_bits(out, C.plain_inv)


def test_image_0_of_a_batch_is_the_batch_one_result(C):
    """batch 2 (one prompt, two images) with a batch-1 negative embedding: a forward at batch 4 per step"""
    two = C.out(pipe=C.pipe_inv, latents=C.lat2, num_images_per_prompt=2, true_cfg_scale=2.0, **C.neg).images
    assert two.shape == (2, N, 64) and not torch.equal(two[0], two[1])
    for b in range(2):
        one = C.out(pipe=C.pipe_inv, latents=C.lat2[b:b + 1], true_cfg_scale=2.0, **C.neg).images
        assert same_bits(two[b:b + 1], one), f"image {b}"


# ------------------------------------------------------------------------------------------------------------------ against the oracle
def ref_loop(C, scale):
    """two oracle forwards per step, neg + s (pos - neg), Euler: in fp32 torch. Returns (latents, the two velocities of step 0)"""
    sch = fm.FlowMatchEulerDiscreteScheduler()
    cfg = sch.config
    mu = fm.calculate_shift(N, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / STEPS, STEPS), device="cpu", mu=mu)
    sig, ids = sch.sigmas, fm.prepare_latent_image_ids(HW, HW)
    cids = ids.clone()
    cids[:, 2] -= HW
    x, first = C.lat, None
    with torch.no_grad():
        for i in range(STEPS):
            pos, neg = (fr.tranformer_forward(C.tr, C.cond, cids, None, {}, hidden_states=x, encoder_hidden_states=pe, pooled_projections=pooled,
                                              timestep=sch.timesteps[i].expand(1) / 1000, img_ids=ids, txt_ids=torch.zeros(T, 3),
                                              guidance=torch.full((1,), 3.5))[0] for pe, pooled in ((C.pe, C.pooled), (C.neg_pe, C.neg_pooled)))
            first = first or (pos, neg)
            x = x + (sig[i + 1] - sig[i]) * (neg + scale * (pos - neg))
    return x, first


def test_against_the_restated_loop(C):
    """s = 2: the guided velocity's error is s e_pos + (s - 1) e_neg, each branch inside the unguided loop's bound, so (2s - 1) * TOL_GEN by
    the triangle inequality. Measured on an MI355X: 1.48e-3, against the bound 9.6e-3."""
    scale = 2.0
    want, _ = ref_loop(C, scale)
    err = relerr(C.run(true_cfg_scale=scale, **C.neg).cpu(), want)
    print(f"guided loop, s = {scale}: relative L2 {err:.2e} (bound {(2 * scale - 1) * TOL_GEN:.1e})")
    assert err < (2 * scale - 1) * TOL_GEN


# ------------------------------------------------------------------------------------------------------------------ around the loop
def test_the_callback_sees_the_images_and_its_last_latents_are_the_result(C):
    seen = []

    def cb(pipe, i, t, kw):
        seen.append(kw["latents"].clone())
        return {}
    out = C.run(true_cfg_scale=2.0, callback_on_step_end=cb, **C.neg)
    assert len(seen) == STEPS and all(l.shape == (1, N, 64) for l in seen)
    assert same_bits(seen[-1], out) and same_bits(out, C.run(true_cfg_scale=2.0, **C.neg))

    def replace_at_1(pipe, i, t, kw):                               # latents a callback returns go to both halves
        return {"latents": C.x0.cuda().clone()} if i == 1 else {"latents": kw["latents"]}

    def restart_at_1(pipe, i, t, kw):
        return {"latents": C.x0.cuda().clone()} if i == 1 else {}
    a, b = C.run(true_cfg_scale=2.0, callback_on_step_end=replace_at_1, **C.neg), C.run(true_cfg_scale=2.0, callback_on_step_end=restart_at_1, **C.neg)
    assert a.shape == (1, N, 64) and same_bits(a, b) and not torch.equal(a, out)
    # equal branches under the batch-invariant plans: what the plain call makes of the same callback
    kw = dict(pipe=C.pipe_inv, callback_on_step_end=restart_at_1)
    assert same_bits(C.out(true_cfg_scale=4.0, negative_prompt_embeds=C.pe, negative_pooled_prompt_embeds=C.pooled, **kw).images, C.out(**kw).images)


@pytest.mark.parametrize("strength", [1.0, 0.5])
def test_with_inpainting(C, strength):
    kw = dict(image_latents=C.x0, latent_mask=C.half, strength=strength)
    calls = []
    out = C.run(true_cfg_scale=2.0, callback_on_step_end=lambda p, i, t, k: calls.append(i) or {}, **kw, **C.neg)
    assert same_bits(out[:, :8], C.x0.cuda()[:, :8]), "the kept tokens are not the source"
    assert len(calls) == (STEPS if strength == 1.0 else 2)
    unguided = C.run(**kw)
    assert same_bits(unguided[:, :8], C.x0.cuda()[:, :8]) and not torch.equal(out[:, 8:], unguided[:, 8:])
    assert same_bits(C.run(), C.plain)


def test_attention_mask_batches(C):
    """a bool key-padding mask over [text | image | condition] with the last 100 text keys padded, batch 2 = B: of batch 1 (shared), B (for
    both halves) and 2B ([pos; neg]) it is one and the same masked run; of batch 3 the engine's ValueError"""
    m = torch.ones(1, 1, 1, T + 2 * N, dtype=torch.bool, device="cuda")
    m[..., T - 100:T] = False
    kw = dict(latents=C.lat2, num_images_per_prompt=2, true_cfg_scale=2.0, **C.neg)
    outs = [C.run(joint_attention_kwargs={"attention_mask": m.expand(b, -1, -1, -1).contiguous()}, **kw) for b in (1, 2, 4)]
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2]) and not torch.equal(outs[0], C.run(**kw))
    with pytest.raises(ValueError, match="attention_mask"):
        C.run(joint_attention_kwargs={"attention_mask": m.expand(3, -1, -1, -1).contiguous()}, **kw)
    assert C.pipe.transformer.engine.adapter_weight_tiles == 1
    assert same_bits(C.run(), C.plain)


def test_per_image_adapter_weights(C):
    """set_adapters(names, [w per image]) with B = 2: the [B] table applies to both halves and equals the table tiled to [2B]; a table of
    length 3 is the engine's ValueError, and the next plain call works"""
    names = C.pipe.get_list_adapters()["transformer"]
    kw = dict(latents=C.lat2, num_images_per_prompt=2, true_cfg_scale=2.0, **C.neg)
    try:
        C.pipe.set_adapters(names, [[1.0, 0.25]] * len(names))
        per_image = C.run(**kw).clone()
        C.pipe.set_adapters(names, [[1.0, 0.25, 1.0, 0.25]] * len(names))
        tiled = C.run(**kw).clone()
        C.pipe.set_adapters(names, [[1.0, 0.25, 0.5]] * len(names))
        with pytest.raises(ValueError, match="per-image weights"):
            C.run(**kw)
        assert C.pipe.transformer.engine.adapter_weight_tiles == 1
    finally:
        C.pipe.set_adapters(names)
    all_ones = C.run(**kw)
    assert same_bits(per_image, tiled)
    assert not torch.equal(per_image[1:], all_ones[1:])            # (image 1 ran at weight 0.25)
    assert same_bits(C.run(), C.plain)


ERRORS = {
    "scale_nan": dict(true_cfg_scale=float("nan"), neg=True),
    "scale_inf": dict(true_cfg_scale=float("inf"), neg=True),
    "scale_not_a_number": dict(true_cfg_scale="2", neg=True),
    "prompt_and_embeds": dict(true_cfg_scale=2.0, neg=True, negative_prompt="blurry"),
    "embeds_without_pooled": dict(true_cfg_scale=2.0, negative_prompt_embeds=torch.zeros(1, T, 4096)),
    "pooled_without_embeds": dict(true_cfg_scale=2.0, negative_pooled_prompt_embeds=torch.zeros(1, 768)),
    "embeds_tokens": dict(true_cfg_scale=2.0, negative_prompt_embeds=torch.zeros(1, T - 1, 4096), negative_pooled_prompt_embeds=torch.zeros(1, 768)),
    "embeds_batch": dict(true_cfg_scale=2.0, negative_prompt_embeds=torch.zeros(2, T, 4096), negative_pooled_prompt_embeds=torch.zeros(2, 768)),
    "pooled_width": dict(true_cfg_scale=2.0, negative_prompt_embeds=torch.zeros(1, T, 4096), negative_pooled_prompt_embeds=torch.zeros(1, 767)),
    "prompt_list_length": dict(true_cfg_scale=2.0, negative_prompt=["a", "b"]),
}


@pytest.mark.parametrize("case", list(ERRORS))
def test_refusals_leave_the_pipeline_as_it_was(C, case):
    kw = dict(ERRORS[case])
    if kw.pop("neg", False):
        kw.update(C.neg)
    index = C.pipe.scheduler._step_index
    with pytest.raises(ValueError):
        C.run(condition_scale=2.0, **kw)                          # (a refused call must not leave its condition_scale behind either)
    assert C.model.transformer.c_factor is None and C.pipe.scheduler._step_index == index
    assert C.pipe.transformer.engine.adapter_weight_tiles == 1
    assert same_bits(C.run(), C.plain), "a plain call after the refused one changed"


def test_a_negative_string_needs_a_text_encoder(C):
    with pytest.raises(NotImplementedError, match="text"):
        C.run(true_cfg_scale=2.0, negative_prompt="blurry")
    assert same_bits(C.run(), C.plain)


# ------------------------------------------------------------------------------------------------------------------ operand modes
@pytest.mark.parametrize("mode", ["bf16", "fp16", "precise"])
def test_operand_modes(C, mode):
    mc, pipe = {"bf16": {}, "fp16": {"operands": "fp16", "f16_overflow": "fallback"}, "precise": {"precise": True}}[mode], None
    if mode == "precise":                                       # (the split mode needs weights packed with their bf16 rounding residuals)
        from loongx_amd.flux.pipeline import LxFluxPipeline
        from loongx_amd.flux.transformer import LxFluxTransformer
        from loongx_amd.flux.weights import FluxConfig
        cfg = FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2, in_channels=64, joint_attention_dim=4096,
                         pooled_projection_dim=768, guidance_embeds=True)
        pipe = LxFluxPipeline(LxFluxTransformer.from_state_dict(C.tr.state_dict(), cfg, "cuda", precise=True))
    guided = C.out(pipe=pipe, model_config=mc, true_cfg_scale=2.0, **C.neg)
    plain = C.out(pipe=pipe, model_config=mc).images
    assert bool(torch.isfinite(guided.images).all()) and not torch.equal(guided.images, plain)
    if mode == "fp16":
        assert guided.lx_operands == "fp16"                      # (these inputs do not saturate: no fallback, and both halves were counted)


def test_fp16_fallback_restarts_from_the_doubled_start_latents(C):
    """on the model whose fp16 operands saturate (the planted bias of tests/test_f16_gpu.py): the guided image is computed again with bf16
    operands from the same start, at the same scale -- bit-equal to asking for bf16 in the first place"""
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    from tests.test_f16_gpu import _planted_model
    model = _planted_model(bias_value=1.0e5)
    calls = []

    def run(mc):
        c = Condition("subject", latents=C.cond.cuda(), latent_hw=(HW, HW), position_delta=[0, -HW])
        return generate(model, model.flux_pipe, conditions=[c], height=HW * 16, width=HW * 16, num_inference_steps=STEPS, latents=C.lat.cuda(),
                        prompt_embeds=C.pe.cuda(), pooled_prompt_embeds=C.pooled.cuda(), output_type="latent", model_config=mc,
                        default_lora=True, use_brain_condition=False, true_cfg_scale=2.0, negative_prompt_embeds=C.neg_pe.cuda(),
                        negative_pooled_prompt_embeds=C.neg_pooled.cuda(), callback_on_step_end=lambda p, i, t, k: calls.append(i) or {})
    want = run({"operands": "bf16"}).images.clone()
    with pytest.warns(RuntimeWarning, match="recomputing this image with bf16 operands"):
        out = run({"operands": "fp16", "f16_overflow": "fallback"})
    assert calls == list(range(STEPS)) * 3 and out.lx_operands.startswith("bf16")
    assert out.images.shape == (1, N, 64) and same_bits(out.images, want)
