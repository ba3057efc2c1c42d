"""generate(solver="dpmpp_2m"): the second-order multistep sampler on the tiny model, the inputs and the branches of
tests/test_brain_cfg_generate_gpu.py (2 + 2 blocks, 16 tokens; full F, text T, negative N in ONE batch per step, on the batch-invariant
launch plans, engine.pair_plan = False), at 6 steps: on a full trajectory steps 0 and 1 are first order (no history; sigma_0 = 1) and so is
the last, which leaves three second-order steps where 4 steps would leave one.

What is promised bit for bit: the call is one plain batch-1 forward per branch per step followed by ops.dpmpp2m_step (ops.dpmpp2m_step_apg
under APG) on their concatenation, with one history buffer D for the call and the coefficients of pipeline.multistep_coefficient;
solver="euler" and no keyword are the call as it was; kept tokens of an inpainted image are the source; the fp16 fallback's second pass
starts without history. And on a field with a known answer, driven through scheduler.step alone, the second-order step is what it claims to
be: at 16 steps its end point is at least 5 times closer to the exact solution than Euler's.

On the commit before the keyword existed prepare_params swallowed it, so a call with solver="dpmpp_2m" returned Euler's latents: the tests
of the written-out loop fail there."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_modules as fm  # noqa: E402
from tests.test_api_gpu import _mk_model  # noqa: E402
from tests.test_apg_generate_gpu import FORMS as GUIDED  # noqa: E402
from tests.test_brain_cfg_generate_gpu import HW, N, T, differ, full_embeds, quiet  # noqa: E402
from tests.test_inpaint_generate_gpu import same_bits  # noqa: E402

STEPS = 6
SOLVER = dict(solver="dpmpp_2m")
APG = dict(apg_eta=0.0, apg_norm_threshold=2.0, apg_momentum=-0.5)
# the branches of a call: F alone, then the guided forms of the APG generate test -> (generate's keywords, (s_b, s_t) of the written-out loop)
FORMS = dict({"F": (lambda W: {}, (None, None))}, **GUIDED)


def _generate(model, pipe, I, latents=None, **kw):
    """tests/test_brain_cfg_generate_gpu.py's call at 6 steps"""
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    c = Condition("subject", latents=I["cond"].cuda(), latent_hw=(HW, HW), position_delta=[0, -HW])
    kw = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    kw.setdefault("model_config", {})
    kw.setdefault("prompt_embeds", I["pe"].cuda())
    kw.setdefault("pooled_prompt_embeds", I["pooled"].cuda())
    return generate(model, pipe, conditions=[c], height=HW * 16, width=HW * 16, num_inference_steps=STEPS,
                    latents=(I["lat"] if latents is None else latents).cuda(), output_type="latent", default_lora=True, fuse_flag=False,
                    additional_condition1=I["eeg"].cuda(), additional_condition2=I["fnirs"].cuda(), **kw)


@pytest.fixture(scope="module")
def W():
    """The model, the inputs and the calls of tests/test_brain_cfg_generate_gpu.py's fixture (the same seeds), at 6 steps; `plain` is the
    call without the keyword. As there, the namespace must not become a reference cycle."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gc
    import weakref
    from types import SimpleNamespace
    tr = fm.FluxTransformer2DModel(num_layers=2, num_single_layers=2, heads=2, head_dim=128, in_channels=64, joint_dim=4096,
                                   pooled_dim=768, guidance_embeds=True, lora=True)
    fm.init_synthetic_(tr, seed=4, std=0.03, bias_std=0.02, norm_jitter=0.1)
    tr.eval()
    _, model = _mk_model(tr)
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
    w = SimpleNamespace(model=model, pipe=pipe, I=I, out=out, run=run, half=half,
                        neg=dict(negative_prompt_embeds=I["neg_pe"], negative_pooled_prompt_embeds=I["neg_pooled"]), plain=run().clone())
    yield w
    engine = weakref.ref(pipe.transformer.engine)
    vars(w).clear()
    del w, out, run, model, pipe
    torch.cuda.synchronize()
    freed = engine() is None                                         # (by reference count alone: it was in no cycle)
    gc.collect()
    assert freed, "the model's engine was left to the cycle collector"


def hand_loop(model, pipe, I, s_b=None, s_t=None, solver=True, apg=None, inpaint=None, mc=None):
    """The loop written out: per step one plain batch-1 tranformer_forward per branch (F; T when s_b; N when s_t), invalidate_conditioning
    between them, then one step on their concatenation -- ops.dpmpp2m_step with one D (zero at the start) and the coefficient of
    multistep_coefficient, 0 on the first step taken; ops.dpmpp2m_step_apg with one M, sums and workspace where apg; the Euler entries where
    not solver. inpaint = (image_latents, mask [1, N, 1], strength): the trajectory starts part-way from the noised source and every step
    blends. Returns (the latents, the coefficients)."""
    from loongx_amd import ops
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.pipeline import calculate_shift, multistep_coefficient, retrieve_timesteps
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
    th, begin, blend = sch.timesteps_host, 0, None
    if inpaint is not None:
        x0, mask, strength = inpaint
        x0 = x0.cuda().to(torch.float32).contiguous()
        timesteps, _, th = pipe.get_timesteps(STEPS, strength, "cuda")
        begin = STEPS - len(timesteps)
        noise = lat.contiguous()
        lat = sch.scale_noise(x0, begin, noise)
        blend = (x0, noise, mask.cuda().to(torch.float32).expand(1, N, 64).contiguous())
    sched_ts = (th / np.float32(1000)).tolist()
    guidance = torch.full((1,), 3.5, device="cuda")
    txt_ids = torch.zeros(T, 3, device="cuda")
    x = torch.cat([lat] * k).contiguous()
    D = torch.zeros(1, N, 64, device="cuda")
    M = torch.zeros(1, N, 64, device="cuda")
    sums = torch.zeros(len(timesteps), 1, 3, dtype=torch.float64, device="cuda")
    ws = torch.empty(ops.apg_workspace_bytes(1, N * 64) // 8, dtype=torch.float64, device="cuda")
    coefficients = []
    for j, t in enumerate(timesteps):
        i = begin + j
        vs = []
        for pe, pooled in branches:
            tr.invalidate_conditioning()
            vs.append(tranformer_forward(tr, model_config=mc, condition_latents=tokens, condition_ids=cids, condition_type_ids=tids,
                                         hidden_states=x[:1], timestep=t.expand(1) / 1000, guidance=guidance, pooled_projections=pooled,
                                         encoder_hidden_states=pe, txt_ids=txt_ids, img_ids=ids, joint_attention_kwargs=None,
                                         return_dict=False, lx_schedule=(j, sched_ts))[0])
        v = torch.cat(vs).contiguous()
        assert v.dtype in (torch.float32, torch.bfloat16)
        sigma, sigma_next = float(sch._sig_host[i]), float(sch._sig_host[i + 1])
        ds = float(np.float32(sch._sig_host[i + 1]) - np.float32(sch._sig_host[i]))
        if solver:
            c = multistep_coefficient(sch._sig_host, i, begin) if j > 0 else 0.0
            coefficients.append(c)
            if apg is None:
                ops.dpmpp2m_step(x, v, sigma, ds, c, D, scales, blend, sigma_next)
            else:
                ops.dpmpp2m_step_apg(x, v, sigma, ds, c, D, scales, apg["apg_eta"], apg["apg_norm_threshold"], apg["apg_momentum"], M, sums[j],
                                     ws, blend, sigma_next)
        elif k == 3:
            ops.euler_step_cfg3(x, v, ds, *scales, blend, sigma_next)
        elif k == 2:
            ops.euler_step_cfg(x, v, ds, *scales, blend, sigma_next)
        elif blend is None:
            ops.euler_step(x, v, ds)
        else:
            ops.euler_step_blend(x, v, ds, *blend, sigma_next)
    tr.invalidate_conditioning()
    return x[:1].clone(), coefficients


# ------------------------------------------------------------------------------------------------------------------ on: the written-out loop
@pytest.mark.parametrize("form", list(FORMS))
def test_the_solver_changes_the_result_and_is_the_written_out_loop(W, form):
    kw, (s_b, s_t) = FORMS[form]
    euler = quiet(W.out, **kw(W))
    assert euler.lx_solver is None
    euler = euler.images.clone()
    out = quiet(W.out, **kw(W), **SOLVER)
    got = out.images.clone()
    assert got.shape == W.plain.shape and bool(torch.isfinite(got).all())
    assert not torch.equal(got, euler), 'solver="dpmpp_2m" returned the Euler call\'s latents'
    want, coefficients = hand_loop(W.model, W.pipe, W.I, s_b, s_t)
    assert same_bits(got, want), differ(got, want)
    assert out.lx_solver == {"solver": "dpmpp_2m", "coefficients": coefficients}
    c = out.lx_solver["coefficients"]
    assert len(c) == STEPS and c[0] == c[1] == c[-1] == 0.0 and all(x > 0.0 for x in c[2:-1]) and all(isinstance(x, float) for x in c)
    assert same_bits(euler, hand_loop(W.model, W.pipe, W.I, s_b, s_t, solver=False)[0]), "the written-out Euler loop is not the Euler call"


# ------------------------------------------------------------------------------------------------------------------ composition
def test_inpaint_starts_part_way_and_keeps_the_source(W):
    """strength 0.7 of 6 steps begins at step 1 (sigma_1 < 1): the first step taken is first order for want of history, and the one after
    it is already second order"""
    kw = dict(image_latents=W.I["x0"], latent_mask=W.half, strength=0.7)
    euler = W.run(**kw).clone()
    out = quiet(W.out, **kw, **SOLVER)
    got, c = out.images.clone(), out.lx_solver["coefficients"]
    x0 = W.I["x0"].cuda()
    assert same_bits(got[:, :8], x0[:, :8]), "the kept tokens are not the source"
    assert same_bits(euler[:, :8], x0[:, :8]) and not torch.equal(got[:, 8:], euler[:, 8:])
    assert len(c) == STEPS - 1 and c[0] == 0.0 and c[1] > 0.0 and c[-1] == 0.0, c
    want, coefficients = hand_loop(W.model, W.pipe, W.I, inpaint=(W.I["x0"], W.half, 0.7))
    assert same_bits(got, want), differ(got, want)
    assert c == coefficients
    assert same_bits(W.run(), W.plain)


@pytest.mark.parametrize("form", list(GUIDED))
def test_with_apg_it_is_the_written_out_loop(W, form):
    kw, (s_b, s_t) = GUIDED[form]
    apg_only = quiet(W.out, **kw(W), **APG)
    apg_x, apg_sums = apg_only.images.clone(), apg_only.lx_apg.clone()
    out = quiet(W.out, **kw(W), **APG, **SOLVER)
    got = out.images.clone()
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, apg_x)
    want, coefficients = hand_loop(W.model, W.pipe, W.I, s_b, s_t, apg=APG)
    assert same_bits(got, want), differ(got, want)
    assert out.lx_solver["coefficients"] == coefficients and tuple(out.lx_apg.shape) == (STEPS, 1, 3)
    # steps 0 and 1 are first order: their sums are the Euler call's bit for bit (step 1 starts from the same latents)
    assert torch.equal(out.lx_apg[:2].view(torch.int64), apg_sums[:2].view(torch.int64))
    assert same_bits(quiet(W.run, **kw(W), **APG), apg_x), "a call with APG alone after one with the solver changed"


def test_step_cache(W):
    """the scheduler never sees whether the blocks ran: with a threshold nothing reaches, only the first and the last step compute, and two
    identical calls report the same steps and agree bit for bit; with one nothing stays under, the call is the one without the cache"""
    want = W.run(**SOLVER).clone()
    always = W.out(model_config={"step_cache_thresh": 1e-30, "step_cache_coefficients": (1.0, 0.0)}, **SOLVER)
    assert same_bits(always.images, want) and always.lx_step_cache["computed"] == list(range(STEPS))
    mc = {"step_cache_thresh": 1e30, "step_cache_coefficients": (1.0, 0.0)}
    a = W.out(model_config=dict(mc), **SOLVER)
    a_x, a_computed = a.images.clone(), list(a.lx_step_cache["computed"])
    b = W.out(model_config=dict(mc), **SOLVER)
    assert a_computed == [0, STEPS - 1] and list(b.lx_step_cache["computed"]) == a_computed
    assert bool(torch.isfinite(a_x).all()) and same_bits(b.images, a_x) and not torch.equal(a_x, want)
    assert a.lx_solver == b.lx_solver == always.lx_solver
    assert same_bits(W.run(), W.plain)


def test_a_callback_that_returns_latents_keeps_the_history(W):
    """documented: the step after the replacement takes its difference against the prediction of the latents that were replaced"""
    def restart_at_2(pipe, i, t, kw):
        return {"latents": W.I["x0"].cuda().clone()} if i == 2 else {}
    out = W.out(callback_on_step_end=restart_at_2, **SOLVER)
    assert out.lx_solver["coefficients"] == W.out(**SOLVER).lx_solver["coefficients"] and bool(torch.isfinite(out.images).all())


# ------------------------------------------------------------------------------------------------------------------ isolation
def test_euler_is_the_call_without_the_keyword(W):
    assert same_bits(quiet(W.run, solver="euler"), W.plain)
    first = quiet(W.run, **SOLVER).clone()
    assert not torch.equal(first, W.plain)
    assert same_bits(W.run(), W.plain), "an Euler call after a solver call changed"
    assert same_bits(quiet(W.run, solver="euler"), W.plain)
    assert same_bits(quiet(W.run, **SOLVER), first), "two solver calls differ"
    assert W.out().lx_solver is None and W.out(solver="euler").lx_solver is None


@pytest.mark.parametrize("solver", ["heun", 2], ids=["heun", "int"])
def test_a_refused_solver_leaves_the_pipeline_as_it_was(W, solver):
    index = W.pipe.scheduler._step_index
    with pytest.raises(ValueError, match="solver"):
        W.run(condition_scale=2.0, solver=solver)
    assert W.model.transformer.c_factor is None and W.pipe.scheduler._step_index == index
    assert same_bits(W.run(), W.plain)


def test_fp16_fallback_starts_without_history(W):
    """on the model whose fp16 operands saturate (the planted bias of tests/test_f16_gpu.py): the image is computed again with bf16 operands
    from the same start and no history -- bit-equal, coefficients included, to asking for bf16 in the first place"""
    from tests.test_f16_gpu import _planted_model
    model = _planted_model(bias_value=1.0e5)
    calls = []

    def run(mc):
        return _generate(model, model.flux_pipe, W.I, model_config=mc, callback_on_step_end=lambda p, i, t, k: calls.append(i) or {},
                         **FORMS["F_T_N"][0](W), **SOLVER)
    want = run({"operands": "bf16"})
    want_x, want_c = want.images.clone(), want.lx_solver["coefficients"]
    with pytest.warns(RuntimeWarning, match="recomputing this image with bf16 operands"):
        out = run({"operands": "fp16", "f16_overflow": "fallback"})
    assert calls == list(range(STEPS)) * 3 and out.lx_operands.startswith("bf16")
    assert out.images.shape == (1, N, 64) and same_bits(out.images, want_x)
    assert out.lx_solver["coefficients"] == want_c and len(want_c) == STEPS and want_c[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------ a field with a known answer
def test_convergence_on_a_gaussian_flow():
    """No model: x0 ~ N(mean, sd^2) per coordinate, independent, eps ~ N(0, 1), x_s = (1 - s) x0 + s eps. The velocity of the probability
    flow is v(x, s) = E[eps - x0 | x_s = x] = k (x - a mean) - mean with a = 1 - s, k = (s - a sd^2) / (a^2 sd^2 + s^2), and the ODE
    dx/ds = v has the exact solution x(s1) = a1 mean + sqrt(a1^2 sd^2 + s1^2) / sqrt(a0^2 sd^2 + s0^2) (x(s0) - a0 mean). E = 4096
    coordinates, mean = 0.5 N(0, 1), sd = 0.3 + 0.5 |N(0, 1)|, numpy default_rng(0); the 1024-token schedule at 16 steps, from sigma = 1 to 0.

    First the float64 restatement of both loops on the host: Euler's relative L2 error at sigma = 0 must be at least 6 times the
    second-order loop's (7.2 with these statistics). Then scheduler.step on the GPU, fp32, once without and once with multistep=: each end
    point lies within 1e-4 relative L2 of its restatement -- fp32 rounding over 16 steps of O(1) values is about 1e-6, the errors compared
    are 1e-2 and 8e-2 -- so the GPU ratio is at least (8e-2 - 1e-4) / (8e-2 / 6 + 1e-4) > 5, asserted as well."""
    from loongx_amd.flux.pipeline import FlowMatchEulerDiscreteScheduler, MultistepState, calculate_shift
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    E, steps = 4096, 16
    rng = np.random.default_rng(0)
    mean, sd, z = rng.normal(size=E) * 0.5, np.abs(rng.normal(size=E)) * 0.5 + 0.3, rng.normal(size=E)
    sch = FlowMatchEulerDiscreteScheduler()
    cfg = sch.config
    mu = calculate_shift(1024, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)

    def k_and_am(s):
        a = 1.0 - s
        return (s - a * sd * sd) / (a * a * sd * sd + s * s), a * mean

    def restated(sig, second_order):
        lam = lambda t: math.log((1.0 - t) / t)  # noqa: E731
        x, D_prev = z.copy(), None
        for i in range(steps):
            s_prev, s, s_next = (sig[i - 1] if i else None), sig[i], sig[i + 1]
            k, am = k_and_am(s)
            g = k * (x - am) - mean
            D = x - s * g
            c = 0.0
            if second_order and i > 0 and s_next > 0.0 and s_prev < 1.0:
                c = (1.0 - s_next / s) * (lam(s_next) - lam(s)) / (2.0 * (lam(s) - lam(s_prev)))
            x = x + (s_next - s) * g + (c * (D - D_prev) if c else 0.0)
            D_prev = D
        return x

    def on_the_gpu(second_order):
        sch.set_timesteps(sigmas=np.linspace(1.0, 1 / steps, steps), device="cuda", mu=mu)
        state = MultistepState((1, 64, 64), "cuda") if second_order else None
        x = torch.from_numpy(z.astype(np.float32)).cuda().view(1, 64, 64)
        m32 = torch.from_numpy(mean.astype(np.float32)).cuda().view(1, 64, 64)
        for i in range(steps):
            k, am = (torch.from_numpy(t.astype(np.float32)).cuda().view(1, 64, 64) for t in k_and_am(float(sch._sig_host[i])))
            v = k * (x - am) - m32
            x = sch.step(v, sch.timesteps[i], x, **({"multistep": state} if second_order else {}))[0]
        if second_order:
            assert len(state.coefficients) == steps and state.coefficients[0] == state.coefficients[1] == state.coefficients[-1] == 0.0
            assert all(c > 0.0 for c in state.coefficients[2:-1])
        return x.double().cpu().numpy().reshape(E), sch._sig_host.astype(np.float64)

    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))  # noqa: E731
    got2, sig = on_the_gpu(True)
    got1, _ = on_the_gpu(False)
    assert sig[0] == 1.0 and sig[-1] == 0.0
    exact = mean + sd * z                                              # (a0 = 0, s0 = 1; a1 = 1, s1 = 0)
    want1, want2 = restated(sig, False), restated(sig, True)
    e1, e2 = rel(want1, exact), rel(want2, exact)
    print(f"float64: Euler {e1:.3e}, second order {e2:.3e}, ratio {e1 / e2:.2f}")
    assert e1 / e2 >= 6.0
    d1, d2 = rel(got1, want1), rel(got2, want2)
    g1, g2 = rel(got1, exact), rel(got2, exact)
    print(f"GPU against its restatement: Euler {d1:.3e}, second order {d2:.3e}; against the exact solution {g1:.3e}, {g2:.3e}, ratio {g1 / g2:.2f}")
    assert d1 <= 1e-4 and d2 <= 1e-4
    assert g1 / g2 >= 5.0
