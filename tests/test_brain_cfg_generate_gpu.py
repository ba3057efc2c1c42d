"""generate(brain_guidance_scale=): guidance along the brain signal, on the tiny transformer with the CS3 encoders and the inputs of
tests/test_cfg_generate_gpu.py (2 + 2 blocks, 16 tokens, 4 steps, latents in and out, one Condition(latents=...)) plus an EEG and an fNIRS
recording that replace both text embeddings (fuse_flag=False, the reference's rule).

The branches -- full F (the embeddings after the brain section), text T (as encode_prompt left them), negative N (true CFG) -- run as ONE
batch of k·B·n per step; lx_euler_step_cfg steps [F; T], lx_euler_step_cfg3 steps [F; T; N]. The one model of this file runs on the
batch-invariant launch plans (engine.pair_plan = False). What is promised bit for bit: a call that does not turn brain guidance on is the
call without the keyword; the guided call is k plain forwards per step followed by the guided step; kept tokens of an inpainted image are
the source. What is promised within a bound: the loop restated on the oracle, (2 s_t s_b - 1) * TOL_GEN.

On the commit before the keyword existed prepare_params swallowed it, so every guided call here equalled the plain call: the first three
tests below fail there."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_modules as fm  # noqa: E402
from oracle import flux_ref as fr  # noqa: E402
from tests.helpers import relerr  # noqa: E402
from tests.test_api_gpu import TOL_GEN, _mk_model  # noqa: E402
from tests.test_inpaint_generate_gpu import same_bits  # noqa: E402

HW, N, STEPS, T = 4, 16, 4, 512
SIGNALS = ("eeg", "fnirs")


def _generate(model, pipe, I, latents=None, signals=SIGNALS, **kw):
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    c = Condition("subject", latents=I["cond"].cuda(), latent_hw=(HW, HW), position_delta=[0, -HW])
    kw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    kw.setdefault("model_config", {})
    kw.setdefault("prompt_embeds", I["pe"].cuda())
    kw.setdefault("pooled_prompt_embeds", I["pooled"].cuda())
    return generate(model, pipe, conditions=[c], height=HW * 16, width=HW * 16, num_inference_steps=STEPS,
                    latents=(I["lat"] if latents is None else latents).cuda(), output_type="latent", default_lora=True, fuse_flag=False,
                    additional_condition1=I["eeg"].cuda() if "eeg" in signals else None,
                    additional_condition2=I["fnirs"].cuda() if "fnirs" in signals else None, **kw)


@pytest.fixture(scope="module")
def W():
    """One model on the batch-invariant launch plans, the inputs, a call that returns generate()'s whole output (`out`) or its latents
    (`run`), and the result of the call without guidance. As in tests/test_cfg_generate_gpu.py the namespace must not become a reference
    cycle (an engine in cyclic garbage is freed whenever the collector next runs, possibly under another engine's graph capture): the
    closures hold locals, never the namespace, and the teardown lets go of everything and collects at once."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gc
    import weakref
    from types import SimpleNamespace
    tr = fm.FluxTransformer2DModel(num_layers=2, num_single_layers=2, heads=2, head_dim=128, in_channels=64, joint_dim=4096,
                                   pooled_dim=768, guidance_embeds=True, lora=True)
    fm.init_synthetic_(tr, seed=4, std=0.03, bias_std=0.02, norm_jitter=0.1)
    tr.eval()
    ref_cs3, model = _mk_model(tr)
    pipe = model.flux_pipe
    pipe.transformer.engine.pair_plan = False                        # (before the first step: the plans that do not depend on the batch size)
    g = torch.Generator().manual_seed(3)
    I = dict(lat=torch.randn(1, N, 64, generator=g), cond=torch.randn(1, N, 64, generator=g), pe=torch.randn(1, T, 4096, generator=g) * 0.1,
             pooled=torch.randn(1, 768, generator=g), x0=torch.randn(1, N, 64, generator=g), lat2=torch.randn(2, N, 64, generator=g),
             neg_pe=torch.randn(1, T, 4096, generator=g) * 0.1, neg_pooled=torch.randn(1, 768, generator=g),
             eeg=torch.randn(4, 3000, generator=g), fnirs=torch.randn(6, 600, generator=g))

    def out(**kw):
        return _generate(model, pipe, I, **kw)

    def run(**kw):
        return _generate(model, pipe, I, **kw).images
    half = torch.zeros(1, N, 1)
    half[:, 8:] = 1.0
    w = SimpleNamespace(tr=tr, ref_cs3=ref_cs3, model=model, pipe=pipe, I=I, out=out, run=run, half=half,
                        neg=dict(negative_prompt_embeds=I["neg_pe"], negative_pooled_prompt_embeds=I["neg_pooled"]),
                        plain=run().clone())
    yield w
    engine = weakref.ref(pipe.transformer.engine)
    vars(w).clear()
    del w, out, run, model, pipe
    torch.cuda.synchronize()
    freed = engine() is None                                         # (by reference count alone: it was in no cycle)
    gc.collect()
    assert freed, "the model's engine was left to the cycle collector"


def quiet(f, *a, **kw):
    """f(...) with every RuntimeWarning (generate's category) an error: a call that must not warn"""
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        return f(*a, **kw)


def full_embeds(model, I):
    """what generate()'s brain section makes of the EEG and the fNIRS recording: under fuse_flag=False with both sides present they replace
    prompt_embeds and pooled_prompt_embeds (the model's own encoders, called as generate() calls them)"""
    from loongx_amd.flux.generate import _signal
    eeg = _signal(I["eeg"].cuda(), "cuda", torch.float32, model.eeg_fixed_length, model)
    fnirs = _signal(I["fnirs"].cuda(), "cuda", torch.float32, model.fnirs_fixed_length, model)
    return model.eeg_projection(eeg), model.fnirs_projection(fnirs)


def hand_loop(model, pipe, I, s_b=None, s_t=None, mc=None, replace=None):
    """The guided loop written out: per step one plain batch-1 tranformer_forward per branch (F; T when s_b; N when s_t), invalidate_conditioning
    between them, then the step on their concatenation -- ops.euler_step_cfg3 for three branches, ops.euler_step_cfg for two.
    replace = {step: latents}: what a callback that returns latents after that step does, to every part."""
    from loongx_amd import ops
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.pipeline import calculate_shift, retrieve_timesteps
    from loongx_amd.flux.transformer import tranformer_forward
    tr, sch, mc = pipe.transformer, pipe.scheduler, mc or {}
    branches = [full_embeds(model, I)] + ([(I["pe"].cuda(), I["pooled"].cuda())] if s_b else []) + \
               ([(I["neg_pe"].cuda(), I["neg_pooled"].cuda())] if s_t else [])
    k = len(branches)
    tokens, cids, tids = Condition("subject", latents=I["cond"].cuda(), latent_hw=(HW, HW), position_delta=[0, -HW]).encode(pipe)
    lat, ids = pipe.prepare_latents(1, 16, HW * 16, HW * 16, torch.float32, "cuda", None, I["lat"].cuda())
    cfg = sch.config
    mu = calculate_shift(N, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    timesteps, _ = retrieve_timesteps(sch, STEPS, "cuda", None, np.linspace(1.0, 1 / STEPS, STEPS), mu=mu)
    sched_ts = (sch.timesteps_host / np.float32(1000)).tolist()
    guidance = torch.full((1,), 3.5, device="cuda")
    txt_ids = torch.zeros(T, 3, device="cuda")
    x = torch.cat([lat] * k).contiguous()
    for i, t in enumerate(timesteps):
        vs = []
        for pe, pooled in branches:
            tr.invalidate_conditioning()
            vs.append(tranformer_forward(tr, model_config=mc, condition_latents=tokens, condition_ids=cids, condition_type_ids=tids,
                                         hidden_states=x[:1], timestep=t.expand(1) / 1000, guidance=guidance, pooled_projections=pooled,
                                         encoder_hidden_states=pe, txt_ids=txt_ids, img_ids=ids, joint_attention_kwargs=None,
                                         return_dict=False, lx_schedule=(i, sched_ts))[0])
        v = torch.cat(vs).contiguous()
        assert v.dtype in (torch.float32, torch.bfloat16)
        ds = float(np.float32(sch._sig_host[i + 1]) - np.float32(sch._sig_host[i]))
        if k == 3:
            ops.euler_step_cfg3(x, v, ds, s_b, s_t)
        elif k == 2:
            ops.euler_step_cfg(x, v, ds, s_b or s_t)
        else:
            ops.euler_step(x, v, ds)
        if replace and i in replace:
            x = torch.cat([replace[i].cuda()] * k).contiguous()
    tr.invalidate_conditioning()
    return x[:1].clone()


def differ(got, want):
    return f"{int((got != want).sum())} of {got.numel()} elements differ, relative L2 {relerr(got.cpu(), want.cpu()):.2e}"


# ------------------------------------------------------------------------------------------------------------------ on: the written-out loop
def test_brain_guidance_changes_the_result_and_is_two_plain_forwards_per_step(W):
    got = quiet(W.run, brain_guidance_scale=2.0).clone()
    assert got.shape == W.plain.shape and bool(torch.isfinite(got).all())
    assert not torch.equal(got, W.plain), "brain_guidance_scale=2.0 returned the plain call's latents"
    want = hand_loop(W.model, W.pipe, W.I, s_b=2.0)
    assert same_bits(got, want), differ(got, want)
    assert same_bits(quiet(W.run, brain_guidance_scale=2.0), got), "two guided calls differ"
    assert same_bits(W.run(), W.plain), "a plain call after a guided one changed"
    assert same_bits(W.plain, hand_loop(W.model, W.pipe, W.I)), "the written-out loop without guidance is not the plain call"


def test_with_true_cfg_it_is_three_plain_forwards_per_step(W):
    cfg_only = quiet(W.run, true_cfg_scale=2.0, **W.neg).clone()
    got = quiet(W.run, brain_guidance_scale=2.0, true_cfg_scale=2.0, **W.neg).clone()
    assert got.shape == W.plain.shape and bool(torch.isfinite(got).all())
    assert not torch.equal(got, cfg_only), "brain_guidance_scale=2.0 under true CFG returned the true-CFG call's latents"
    want = hand_loop(W.model, W.pipe, W.I, s_b=2.0, s_t=2.0)
    assert same_bits(got, want), differ(got, want)
    assert same_bits(cfg_only, hand_loop(W.model, W.pipe, W.I, s_t=2.0))
    assert W.pipe.transformer.engine.adapter_weight_tiles == 1
    assert same_bits(W.run(), W.plain)


@pytest.mark.parametrize("mode", ["bf16", "fp16", "precise"])
def test_operand_modes(W, mode):
    """the written-out two-branch loop, bit for bit, on bf16, fp16 and split-bf16 (precise) operands"""
    mc = {"bf16": {"operands": "bf16"}, "fp16": {"operands": "fp16"}, "precise": {"precise": True}}[mode]
    model, pipe = W.model, W.pipe
    if mode == "precise":                                       # (the split mode needs weights packed with their bf16 rounding residuals)
        from loongx_amd.flux.pipeline import LxFluxPipeline
        from loongx_amd.flux.transformer import LxFluxTransformer
        from loongx_amd.flux.weights import FluxConfig
        from loongx_amd.train.model import OminiModel
        cfg = FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2, in_channels=64, joint_attention_dim=4096,
                         pooled_projection_dim=768, guidance_embeds=True)
        model = OminiModel.from_pipe(LxFluxPipeline(LxFluxTransformer.from_state_dict(W.tr.state_dict(), cfg, "cuda", precise=True)),
                                     W.ref_cs3.state_dict(), {}, "cuda")
        pipe = model.flux_pipe
        pipe.transformer.engine.pair_plan = False
    guided = _generate(model, pipe, W.I, model_config=mc, brain_guidance_scale=2.0)
    got = guided.images.clone()
    plain = _generate(model, pipe, W.I, model_config=mc).images.clone()
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, plain)
    if mode == "fp16":
        assert guided.lx_operands == "fp16"                      # (these inputs do not saturate: no fallback, and both branches were counted)
    want = hand_loop(model, pipe, W.I, s_b=2.0, mc=mc)
    assert same_bits(got, want), differ(got, want)


# ------------------------------------------------------------------------------------------------------------------ off is off
def test_scale_one_is_the_call_without_the_keyword(W):
    assert same_bits(quiet(W.run, brain_guidance_scale=1.0), W.plain)
    assert same_bits(quiet(W.run, brain_guidance_scale=1), W.plain)
    cfg_only = W.run(true_cfg_scale=2.0, **W.neg).clone()
    assert same_bits(quiet(W.run, brain_guidance_scale=1.0, true_cfg_scale=2.0, **W.neg), cfg_only)
    with pytest.warns(RuntimeWarning, match="guidance is off") as rec:
        assert same_bits(W.run(brain_guidance_scale=0.5), W.plain)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1


NOTHING_TO_GUIDE = {
    "no_signals": dict(signals=()),
    "use_brain_condition_false": dict(use_brain_condition=False),
    "eeg_only_under_both": dict(signals=("eeg",), brain_replace="both"),
}


@pytest.mark.parametrize("true_cfg", [False, True], ids=["cfg_off", "cfg_on"])
@pytest.mark.parametrize("case", list(NOTHING_TO_GUIDE))
def test_a_brain_that_changes_nothing_warns_once_and_runs_without(W, case, true_cfg):
    kw = dict(NOTHING_TO_GUIDE[case], **(dict(true_cfg_scale=2.0, **W.neg) if true_cfg else {}))
    want = quiet(W.run, **kw).clone()
    with pytest.warns(RuntimeWarning, match="brain_guidance_scale") as rec:
        got = W.run(brain_guidance_scale=2.0, **kw)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1, [str(r.message) for r in rec]
    assert same_bits(got, want)
    assert W.pipe.transformer.engine.adapter_weight_tiles == 1


# ------------------------------------------------------------------------------------------------------------------ against the oracle
def ref_loop(W, s_b, s_t):
    """k oracle forwards per step, v_b = v_T + s_b (v_F - v_T), g = v_N + s_t (v_b - v_N) (g = v_b without s_t), Euler: in fp32 torch, the
    F embeddings from the oracle's CS3 encoders"""
    I = W.I
    sch = fm.FlowMatchEulerDiscreteScheduler()
    cfg = sch.config
    mu = fm.calculate_shift(N, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / STEPS, STEPS), device="cpu", mu=mu)
    sig, ids = sch.sigmas, fm.prepare_latent_image_ids(HW, HW)
    cids = ids.clone()
    cids[:, 2] -= HW
    x = I["lat"]
    with torch.no_grad():
        full = W.ref_cs3.brain_embeds(I["pe"], I["pooled"], I["eeg"].unsqueeze(0), I["fnirs"].unsqueeze(0), None, None, fuse_flag=False,
                                      per_stream=False)
        branches = [full, (I["pe"], I["pooled"])] + ([(I["neg_pe"], I["neg_pooled"])] if s_t else [])
        for i in range(STEPS):
            vs = [fr.tranformer_forward(W.tr, I["cond"], cids, None, {}, hidden_states=x, encoder_hidden_states=pe, pooled_projections=pooled,
                                        timestep=sch.timesteps[i].expand(1) / 1000, img_ids=ids, txt_ids=torch.zeros(T, 3),
                                        guidance=torch.full((1,), 3.5))[0] for pe, pooled in branches]
            g = vs[1] + s_b * (vs[0] - vs[1])
            if s_t:
                g = vs[2] + s_t * (g - vs[2])
            x = x + (sig[i + 1] - sig[i]) * g
    return x


@pytest.mark.parametrize("s_b,s_t", [(2.0, None), (1.5, 1.5)], ids=["brain_2", "brain_1.5_text_1.5"])
def test_against_the_restated_loop(W, s_b, s_t):
    """g = s_t s_b v_F + s_t (1 - s_b) v_T + (1 - s_t) v_N (s_t = 1 without true CFG): each branch's velocity is inside the unguided loop's
    bound, so the guided loop is inside the sum of the absolute coefficients, s_t s_b + s_t (s_b - 1) + (s_t - 1) = 2 s_t s_b - 1, times
    TOL_GEN, by the triangle inequality. Measured on an MI355X: 1.50e-3 against 9.6e-3 at s_b = 2; 1.51e-3 against 1.1e-2 at s_b = s_t = 1.5."""
    factor = 2 * (s_t or 1.0) * s_b - 1
    want = ref_loop(W, s_b, s_t)
    kw = dict(true_cfg_scale=s_t, **W.neg) if s_t else {}
    err = relerr(W.run(brain_guidance_scale=s_b, **kw).cpu(), want)
    print(f"guided loop, s_b = {s_b}, s_t = {s_t}: relative L2 {err:.2e} (bound {factor * TOL_GEN:.1e})")
    assert err < factor * TOL_GEN


# ------------------------------------------------------------------------------------------------------------------ around the loop
BOTH_FORMS = {"brain": lambda W: dict(brain_guidance_scale=2.0), "brain_and_text": lambda W: dict(brain_guidance_scale=2.0, true_cfg_scale=2.0, **W.neg)}


@pytest.mark.parametrize("form", list(BOTH_FORMS))
def test_with_inpainting_the_kept_tokens_are_the_source(W, form):
    kw = dict(image_latents=W.I["x0"], latent_mask=W.half, strength=1.0)
    out = W.run(**kw, **BOTH_FORMS[form](W))
    x0 = W.I["x0"].cuda()
    assert same_bits(out[:, :8], x0[:, :8]), "the kept tokens are not the source"
    unguided = W.run(**kw)
    assert same_bits(unguided[:, :8], x0[:, :8]) and not torch.equal(out[:, 8:], unguided[:, 8:])
    assert same_bits(W.run(), W.plain)


def test_the_callback_sees_the_images_and_its_latents_reach_every_part(W):
    """B·n = 2: the callback sees [2, N, 64]; the latents it returns after step 1 go to all three parts -- the written-out loop with the same
    replacement (batch 1) gives the same bits, which it would not if a branch had run on from its own copy"""
    seen = []

    def cb(pipe, i, t, kw):
        seen.append(kw["latents"].clone())
        return {}
    form = BOTH_FORMS["brain_and_text"](W)
    out = W.run(latents=W.I["lat2"], num_images_per_prompt=2, callback_on_step_end=cb, **form)
    assert len(seen) == STEPS and all(s.shape == (2, N, 64) for s in seen) and same_bits(seen[-1], out)

    def restart_at_1(pipe, i, t, kw):
        return {"latents": W.I["x0"].cuda().clone()} if i == 1 else {}
    got = W.run(callback_on_step_end=restart_at_1, **form)
    want = hand_loop(W.model, W.pipe, W.I, s_b=2.0, s_t=2.0, replace={1: W.I["x0"]})
    assert got.shape == (1, N, 64) and same_bits(got, want), differ(got, want)
    assert not torch.equal(got, W.run(**form))


def test_per_image_adapter_weights_apply_to_every_part(W):
    """set_adapters(names, [w per image]) with B·n = 2 under three branches: the [2] table equals the table tiled to [6]"""
    names = W.pipe.get_list_adapters()["transformer"]
    kw = dict(latents=W.I["lat2"], num_images_per_prompt=2, **BOTH_FORMS["brain_and_text"](W))
    try:
        W.pipe.set_adapters(names, [[1.0, 0.25]] * len(names))
        per_image = W.run(**kw).clone()
        W.pipe.set_adapters(names, [[1.0, 0.25] * 3] * len(names))
        tiled = W.run(**kw).clone()
        assert W.pipe.transformer.engine.adapter_weight_tiles == 1
    finally:
        W.pipe.set_adapters(names)
    all_ones = W.run(**kw)
    assert same_bits(per_image, tiled)
    assert not torch.equal(per_image[1:], all_ones[1:])            # (image 1 ran at weight 0.25)
    assert same_bits(W.run(), W.plain)


def test_attention_mask_batches(W):
    """a bool key-padding mask over [text | image | condition] with the last 100 text keys padded, B·n = 2, k = 3: of batch 1 (shared), 2
    (tiled three times) and 6 (as given) it is one and the same masked run; of batch 7 the engine's ValueError"""
    m = torch.ones(1, 1, 1, T + 2 * N, dtype=torch.bool, device="cuda")
    m[..., T - 100:T] = False
    kw = dict(latents=W.I["lat2"], num_images_per_prompt=2, **BOTH_FORMS["brain_and_text"](W))
    outs = [W.run(joint_attention_kwargs={"attention_mask": m.expand(b, -1, -1, -1).contiguous()}, **kw).clone() for b in (1, 2, 6)]
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2]) and not torch.equal(outs[0], W.run(**kw))
    with pytest.raises(ValueError, match="attention_mask"):
        W.run(joint_attention_kwargs={"attention_mask": m.expand(7, -1, -1, -1).contiguous()}, **kw)
    assert W.pipe.transformer.engine.adapter_weight_tiles == 1
    assert same_bits(W.run(), W.plain)


def test_step_cache(W):
    """a threshold nothing stays under is the guided call bit for bit; one nothing reaches computes the first and the last step only"""
    form = BOTH_FORMS["brain_and_text"](W)
    want = W.run(**form).clone()
    always = W.out(model_config={"step_cache_thresh": 1e-30, "step_cache_coefficients": (1.0, 0.0)}, **form)
    assert same_bits(always.images, want) and always.lx_step_cache["computed"] == list(range(STEPS))
    never = W.out(model_config={"step_cache_thresh": 1e30, "step_cache_coefficients": (1.0, 0.0)}, **form)
    assert never.lx_step_cache["computed"] == [0, STEPS - 1] and bool(torch.isfinite(never.images).all())
    assert same_bits(W.run(), W.plain)


def test_fp16_fallback_restarts_from_the_same_start_latents(W):
    """on the model whose fp16 operands saturate (the planted bias of tests/test_f16_gpu.py): the guided image is computed again with bf16
    operands from the same three-fold start, at the same scales -- bit-equal to asking for bf16 in the first place"""
    from tests.test_f16_gpu import _planted_model
    model = _planted_model(bias_value=1.0e5)
    calls = []

    def run(mc):
        return _generate(model, model.flux_pipe, W.I, model_config=mc, callback_on_step_end=lambda p, i, t, k: calls.append(i) or {},
                         **BOTH_FORMS["brain_and_text"](W))
    want = run({"operands": "bf16"}).images.clone()
    with pytest.warns(RuntimeWarning, match="recomputing this image with bf16 operands"):
        out = run({"operands": "fp16", "f16_overflow": "fallback"})
    assert calls == list(range(STEPS)) * 3 and out.lx_operands.startswith("bf16")
    assert out.images.shape == (1, N, 64) and same_bits(out.images, want)


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("scale", [float("nan"), float("inf"), -1.0, True, "2"], ids=["nan", "inf", "negative", "bool", "str"])
def test_a_refused_scale_leaves_the_pipeline_as_it_was(W, scale):
    index = W.pipe.scheduler._step_index
    with pytest.raises(ValueError, match="brain_guidance_scale"):
        W.run(condition_scale=2.0, brain_guidance_scale=scale)      # (a refused call must not leave its condition_scale behind either)
    assert W.model.transformer.c_factor is None and W.pipe.scheduler._step_index == index
    assert W.pipe.transformer.engine.adapter_weight_tiles == 1
    assert same_bits(W.run(), W.plain), "a plain call after the refused one changed"


def test_branches_of_different_shapes_are_refused(W):
    """text embeddings of 256 tokens next to the EEG's 512: F and T cannot be rows of one batch; the message names both shapes"""
    short = W.I["pe"][:, :256].contiguous()
    with pytest.raises(ValueError, match=r"\(1, 512, 4096\).*\(1, 256, 4096\)"):
        W.run(prompt_embeds=short, brain_guidance_scale=2.0)
    assert W.pipe.transformer.engine.adapter_weight_tiles == 1
    assert same_bits(W.run(), W.plain)
