"""generate(apg_eta=, apg_norm_threshold=, apg_momentum=): adaptive projected guidance on the tiny model, the inputs and the branches of
tests/test_brain_cfg_generate_gpu.py (2 + 2 blocks, 16 tokens, 4 steps; full F, text T, negative N in ONE batch per step, on the
batch-invariant launch plans, engine.pair_plan = False).

What is promised bit for bit: the guided call with APG on is one plain batch-1 forward per branch per step followed by ops.euler_step_apg on
their concatenation, with one state (M, sums, workspace) for the call; with the three keywords at their defaults the call is the one without
them; on an unguided call they are one RuntimeWarning and the plain call; kept tokens of an inpainted image are the source; the fp16
fallback's second pass starts from empty momentum. What is promised within a bound: the loop restated on the oracle with the rule in float64.

On the commit before the keywords existed prepare_params swallowed them, so every call with them equalled the call without: the tests of the
written-out loop fail there."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_modules as fm  # noqa: E402
from oracle import flux_ref as fr  # noqa: E402
from tests.helpers import relerr  # noqa: E402
from tests.test_api_gpu import TOL_GEN  # noqa: E402
from tests.test_brain_cfg_generate_gpu import HW, N, STEPS, T, W, _generate, differ, full_embeds, quiet  # noqa: E402,F401  (W: the fixture)
from tests.test_inpaint_generate_gpu import same_bits  # noqa: E402

APG = dict(apg_eta=0.0, apg_norm_threshold=2.0, apg_momentum=-0.5)
# the branches of a guided call: [F; T], [F; N], [F; T; N] -> (generate's keywords, (s_b, s_t) of the written-out loop)
FORMS = {"F_T": (lambda W: dict(brain_guidance_scale=2.0), (2.0, None)),
         "F_N": (lambda W: dict(true_cfg_scale=2.5, **W.neg), (None, 2.5)),
         "F_T_N": (lambda W: dict(brain_guidance_scale=2.0, true_cfg_scale=2.5, **W.neg), (2.0, 2.5))}


def hand_loop(model, pipe, I, s_b, s_t, apg, mc=None, replace=None):
    """The guided loop under APG written out: per step one plain batch-1 tranformer_forward per branch (F; T when s_b; N when s_t),
    invalidate_conditioning between them, then ops.euler_step_apg on their concatenation with the step's sigma; one M (zero at the start),
    one [STEPS, 1, 3] sums and one workspace for the loop. replace = {step: latents}: what a callback that returns latents after that step
    does, to every part. Returns (the latents, the sums)."""
    from loongx_amd import ops
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.pipeline import calculate_shift, retrieve_timesteps
    from loongx_amd.flux.transformer import tranformer_forward
    tr, sch, mc = pipe.transformer, pipe.scheduler, mc or {}
    branches = [full_embeds(model, I)] + ([(I["pe"].cuda(), I["pooled"].cuda())] if s_b else []) + \
               ([(I["neg_pe"].cuda(), I["neg_pooled"].cuda())] if s_t else [])
    k, scales = len(branches), tuple(s for s in (s_b, s_t) if s)
    tokens, cids, tids = Condition("subject", latents=I["cond"].cuda(), latent_hw=(HW, HW), position_delta=[0, -HW]).encode(pipe)
    lat, ids = pipe.prepare_latents(1, 16, HW * 16, HW * 16, torch.float32, "cuda", None, I["lat"].cuda())
    cfg = sch.config
    mu = calculate_shift(N, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    timesteps, _ = retrieve_timesteps(sch, STEPS, "cuda", None, np.linspace(1.0, 1 / STEPS, STEPS), mu=mu)
    sched_ts = (sch.timesteps_host / np.float32(1000)).tolist()
    guidance = torch.full((1,), 3.5, device="cuda")
    txt_ids = torch.zeros(T, 3, device="cuda")
    x = torch.cat([lat] * k).contiguous()
    M = torch.zeros(1, N, 64, device="cuda")
    sums = torch.zeros(STEPS, 1, 3, dtype=torch.float64, device="cuda")
    ws = torch.empty(ops.apg_workspace_bytes(1, N * 64) // 8, dtype=torch.float64, device="cuda")
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
        ops.euler_step_apg(x, v, float(sch._sig_host[i]), ds, scales, apg["apg_eta"], apg["apg_norm_threshold"], apg["apg_momentum"], M,
                           sums[i], ws)
        if replace and i in replace:
            x = torch.cat([replace[i].cuda()] * k).contiguous()
    tr.invalidate_conditioning()
    return x[:1].clone(), sums


@pytest.fixture(scope="module")
def R(W):
    """a threshold that binds at step 0 of each form: half the norm of that form's first update, read from the sums of an unclamped call"""
    out = {}
    for form, (kw, _) in FORMS.items():
        s_dd = float(W.out(apg_eta=0.0, apg_momentum=-0.5, **kw(W)).lx_apg[0, 0, 0])
        out[form] = dict(APG, apg_norm_threshold=float(np.float32(0.5 * np.sqrt(s_dd))))
    return out


# ------------------------------------------------------------------------------------------------------------------ on: the written-out loop
@pytest.mark.parametrize("form", list(FORMS))
def test_apg_changes_the_result_and_is_the_written_out_loop(W, R, form):
    kw, (s_b, s_t) = FORMS[form]
    guided = quiet(W.run, **kw(W)).clone()
    out = quiet(W.out, **kw(W), **R[form])
    got = out.images.clone()
    assert got.shape == W.plain.shape and bool(torch.isfinite(got).all())
    assert not torch.equal(got, guided), "the APG keywords returned the plain guided call's latents"
    want, sums = hand_loop(W.model, W.pipe, W.I, s_b, s_t, R[form])
    assert same_bits(got, want), differ(got, want)
    # the sums: on the device, [steps, images, 3], finite, the written-out loop's bit for bit; the threshold bound at step 0
    assert out.lx_apg.is_cuda and out.lx_apg.dtype == torch.float64 and tuple(out.lx_apg.shape) == (STEPS, 1, 3)
    assert bool(torch.isfinite(out.lx_apg).all()) and torch.equal(out.lx_apg.view(torch.int64), sums.view(torch.int64))
    assert float(out.lx_apg[0, 0, 0]) > R[form]["apg_norm_threshold"] ** 2 and bool((out.lx_apg[:, 0, 2] > 0).all())
    assert same_bits(quiet(W.run, **kw(W), **R[form]), got), "two calls differ"
    assert same_bits(quiet(W.run, **kw(W)), guided), "a guided call after one with APG changed"
    assert same_bits(W.run(), W.plain), "a plain call after a guided one changed"


@pytest.mark.parametrize("mode", ["bf16", "fp16", "precise"])
def test_operand_modes(W, mode):
    """the written-out loops of all three forms, bit for bit, on bf16, fp16 and split-bf16 (precise) operands"""
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
    for form, (kw, (s_b, s_t)) in FORMS.items():
        out = _generate(model, pipe, W.I, model_config=mc, **kw(W), **APG)
        got = out.images.clone()
        guided = _generate(model, pipe, W.I, model_config=mc, **kw(W)).images
        assert bool(torch.isfinite(got).all()) and not torch.equal(got, guided), form
        if mode == "fp16":
            assert out.lx_operands == "fp16"                     # (these inputs do not saturate: no fallback)
        want, sums = hand_loop(model, pipe, W.I, s_b, s_t, APG, mc=mc)
        assert same_bits(got, want), f"{form}: {differ(got, want)}"
        assert torch.equal(out.lx_apg.view(torch.int64), sums.view(torch.int64)), form


# ------------------------------------------------------------------------------------------------------------------ off is off
@pytest.mark.parametrize("form", list(FORMS))
def test_the_defaults_are_the_call_without_the_keywords(W, form):
    kw = FORMS[form][0]
    want = quiet(W.out, **kw(W))
    assert want.lx_apg is None
    got = quiet(W.out, apg_eta=1.0, apg_norm_threshold=0.0, apg_momentum=0.0, **kw(W))
    assert got.lx_apg is None and same_bits(got.images, want.images)
    assert same_bits(quiet(W.run, apg_eta=1, apg_norm_threshold=0, apg_momentum=np.float32(0.0), **kw(W)), want.images)


@pytest.mark.parametrize("kw", [dict(), dict(brain_guidance_scale=1.0)], ids=["plain", "s_b_1"])
def test_on_an_unguided_call_they_warn_once_and_run_the_plain_call(W, kw):
    with pytest.warns(RuntimeWarning, match="not guided") as rec:
        out = W.out(**APG, **kw)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1, [str(r.message) for r in rec]
    assert out.lx_apg is None and same_bits(out.images, W.plain)


def test_brain_guidance_that_ends_up_off_warns_for_both(W):
    """no signals: brain guidance warns that it has nothing to guide along, APG that the call is not guided; the plain call's bits"""
    want = quiet(W.run, signals=()).clone()
    with pytest.warns(RuntimeWarning) as rec:
        out = W.out(signals=(), brain_guidance_scale=2.0, **APG)
    msgs = [str(r.message) for r in rec if issubclass(r.category, RuntimeWarning)]
    assert len(msgs) == 2 and sum("not guided" in m for m in msgs) == 1 and sum("nothing to guide along" in m for m in msgs) == 1, msgs
    assert out.lx_apg is None and same_bits(out.images, want)


# ------------------------------------------------------------------------------------------------------------------ against the oracle
def ref_loop(W, s_b, s_t, eta, momentum, r):
    """k oracle forwards per step (fp32 torch on the CPU), then the rule of include/lx.h in float64 with one image: g0 the nested guidance,
    D = -sigma (g0 - v_F) + momentum M, w = x - sigma v_F, c = min(1, r / |D|), a = <D, w> / <w, w>, u = c D - c (1 - eta) a w,
    x += dsigma (v_F - u / sigma). Returns (the latents, |D| per step)."""
    I = W.I
    sch = fm.FlowMatchEulerDiscreteScheduler()
    cfg = sch.config
    mu = fm.calculate_shift(N, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / STEPS, STEPS), device="cpu", mu=mu)
    sig, ids = sch.sigmas.double(), fm.prepare_latent_image_ids(HW, HW)
    cids = ids.clone()
    cids[:, 2] -= HW
    x, M, norms = I["lat"].double(), torch.zeros_like(I["lat"], dtype=torch.float64), []
    with torch.no_grad():
        full = W.ref_cs3.brain_embeds(I["pe"], I["pooled"], I["eeg"].unsqueeze(0), I["fnirs"].unsqueeze(0), None, None, fuse_flag=False,
                                      per_stream=False)
        branches = [full, (I["pe"], I["pooled"])] + ([(I["neg_pe"], I["neg_pooled"])] if s_t else [])
        for i in range(STEPS):
            vs = [fr.tranformer_forward(W.tr, I["cond"], cids, None, {}, hidden_states=x.float(), encoder_hidden_states=pe,
                                        pooled_projections=pooled, timestep=sch.timesteps[i].expand(1) / 1000, img_ids=ids,
                                        txt_ids=torch.zeros(T, 3), guidance=torch.full((1,), 3.5))[0].double() for pe, pooled in branches]
            g0 = vs[1] + s_b * (vs[0] - vs[1])
            if s_t:
                g0 = vs[2] + s_t * (g0 - vs[2])
            M = -sig[i] * (g0 - vs[0]) + momentum * M
            w = x - sig[i] * vs[0]
            norm = float(M.norm())
            norms.append(norm)
            c = r / norm if r > 0 and norm > r else 1.0
            a = float((M * w).sum() / (w * w).sum())
            u = c * M - c * (1 - eta) * a * w
            x = x + (sig[i + 1] - sig[i]) * (vs[0] - u / sig[i])
    return x, norms


@pytest.mark.parametrize("s_b,s_t", [(2.0, None), (2.0, 1.5)], ids=["brain_2", "brain_2_text_1.5"])
def test_against_the_restated_loop(W, s_b, s_t):
    """eta = 0, momentum = -0.5 and a threshold at half the oracle's own first |D|, which binds at step 0. The tolerance is derived to first
    order only: the guided velocity g0 is inside (2 s_t s_b - 1) TOL_GEN (tests/test_brain_cfg_generate_gpu.py: the sum of the absolute
    coefficients of the branches); the clamp is a projection onto a ball, so it is 1-Lipschitz; removing the part along w adds at most
    2 (1 - eta) |D| / |w| per unit of forward error, at most 2 more where |D| <= |w|, hence the factor 3; momentum sums the errors of the
    earlier steps geometrically, 1 / (1 - |momentum|). Asserted: 3 (2 s_t s_b - 1) TOL_GEN / (1 - |momentum|).
    Measured on an MI355X: 1.40e-3 against 5.8e-2 at s_b = 2; 1.66e-3 against 9.6e-2 at s_b = 2, s_t = 1.5: 0.02 of the bound."""
    eta, momentum = 0.0, -0.5
    _, norms = ref_loop(W, s_b, s_t, eta, momentum, 0.0)
    r = float(np.float32(0.5 * norms[0]))
    want, norms = ref_loop(W, s_b, s_t, eta, momentum, r)
    assert norms[0] > r * (1 + 1e-3) and all(abs(n / r - 1) > 1e-3 for n in norms), (norms, r)
    kw = dict(true_cfg_scale=s_t, **W.neg) if s_t else {}
    out = W.out(brain_guidance_scale=s_b, apg_eta=eta, apg_norm_threshold=r, apg_momentum=momentum, **kw)
    got_norms = out.lx_apg[:, 0, 0].sqrt().cpu().tolist()
    assert [n > r for n in got_norms] == [n > r for n in norms], (got_norms, norms, r)      # (the same steps were clamped)
    bound = 3 * (2 * (s_t or 1.0) * s_b - 1) * TOL_GEN / (1 - abs(momentum))
    err = relerr(out.images.cpu(), want)
    print(f"APG loop, s_b = {s_b}, s_t = {s_t}, r = {r:.4g}, |D| per step {['%.4g' % n for n in norms]}: relative L2 {err:.2e} "
          f"(bound {bound:.1e}; {err / bound:.2f} of it)")
    assert err < bound


# ------------------------------------------------------------------------------------------------------------------ around the loop
@pytest.mark.parametrize("form", list(FORMS))
def test_with_inpainting_the_kept_tokens_are_the_source(W, R, form):
    kw = dict(image_latents=W.I["x0"], latent_mask=W.half, strength=1.0)
    out = W.run(**kw, **FORMS[form][0](W), **R[form])
    x0 = W.I["x0"].cuda()
    assert same_bits(out[:, :8], x0[:, :8]), "the kept tokens are not the source"
    guided = W.run(**kw, **FORMS[form][0](W))
    assert same_bits(guided[:, :8], x0[:, :8]) and not torch.equal(out[:, 8:], guided[:, 8:])
    assert same_bits(W.run(), W.plain)


def test_the_callback_sees_the_images_and_its_latents_reach_every_part(W, R):
    """B·n = 2: the callback sees [2, N, 64] and the sums are per image; the latents it returns after step 1 go to all three parts -- the
    written-out loop with the same replacement (batch 1) gives the same bits"""
    seen = []

    def cb(pipe, i, t, kw):
        seen.append(kw["latents"].clone())
        return {}
    form = dict(FORMS["F_T_N"][0](W), **R["F_T_N"])
    out = W.out(latents=W.I["lat2"], num_images_per_prompt=2, callback_on_step_end=cb, **form)
    assert len(seen) == STEPS and all(s.shape == (2, N, 64) for s in seen) and same_bits(seen[-1], out.images)
    assert tuple(out.lx_apg.shape) == (STEPS, 2, 3) and bool(torch.isfinite(out.lx_apg).all())
    assert not torch.equal(out.lx_apg[:, 0], out.lx_apg[:, 1])

    def restart_at_1(pipe, i, t, kw):
        return {"latents": W.I["x0"].cuda().clone()} if i == 1 else {}
    got = W.run(callback_on_step_end=restart_at_1, **form)
    want, _ = hand_loop(W.model, W.pipe, W.I, 2.0, 2.5, R["F_T_N"], replace={1: W.I["x0"]})
    assert got.shape == (1, N, 64) and same_bits(got, want), differ(got, want)
    assert not torch.equal(got, W.run(**form))


def test_step_cache(W, R):
    """a threshold nothing stays under is the call bit for bit, sums included: APG acts on whatever velocity the forward returned"""
    form = dict(FORMS["F_T_N"][0](W), **R["F_T_N"])
    want = W.out(**form)
    want_x, want_sums = want.images.clone(), want.lx_apg.clone()
    always = W.out(model_config={"step_cache_thresh": 1e-30, "step_cache_coefficients": (1.0, 0.0)}, **form)
    assert same_bits(always.images, want_x) and always.lx_step_cache["computed"] == list(range(STEPS))
    assert torch.equal(always.lx_apg.view(torch.int64), want_sums.view(torch.int64))
    assert same_bits(W.run(), W.plain)


def test_fp16_fallback_starts_from_empty_momentum(W):
    """on the model whose fp16 operands saturate (the planted bias of tests/test_f16_gpu.py): the image is computed again with bf16 operands
    from the same start and an empty M -- bit-equal, sums included, to asking for bf16 in the first place"""
    from tests.test_f16_gpu import _planted_model
    model = _planted_model(bias_value=1.0e5)
    calls = []

    def run(mc):
        return _generate(model, model.flux_pipe, W.I, model_config=mc, callback_on_step_end=lambda p, i, t, k: calls.append(i) or {},
                         **FORMS["F_T_N"][0](W), **APG)
    want = run({"operands": "bf16"})
    want_x, want_sums = want.images.clone(), want.lx_apg.clone()
    with pytest.warns(RuntimeWarning, match="recomputing this image with bf16 operands"):
        out = run({"operands": "fp16", "f16_overflow": "fallback"})
    assert calls == list(range(STEPS)) * 3 and out.lx_operands.startswith("bf16")
    assert out.images.shape == (1, N, 64) and same_bits(out.images, want_x)
    assert torch.equal(out.lx_apg.view(torch.int64), want_sums.view(torch.int64))


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [dict(apg_eta=float("nan")), dict(apg_eta=1.5), dict(apg_norm_threshold=-1.0), dict(apg_momentum=1.0),
                                 dict(apg_momentum=True), dict(apg_eta="0")], ids=["nan", "eta_1.5", "negative", "momentum_1", "bool", "str"])
def test_a_refused_keyword_leaves_the_pipeline_as_it_was(W, bad):
    index = W.pipe.scheduler._step_index
    with pytest.raises(ValueError, match="apg_"):
        W.run(condition_scale=2.0, brain_guidance_scale=2.0, **bad)      # (a refused call must not leave its condition_scale behind either)
    assert W.model.transformer.c_factor is None and W.pipe.scheduler._step_index == index
    assert W.pipe.transformer.engine.adapter_weight_tiles == 1
    assert same_bits(W.run(), W.plain), "a plain call after the refused one changed"
