"""generate(source_prompt_embeds=...): FlowEdit on the tiny model, the inputs and the embeddings of tests/test_brain_cfg_generate_gpu.py
(2 + 2 blocks, 16 tokens; on the batch-invariant launch plans, engine.pair_plan = False), at 6 steps with a seeded CPU torch.Generator. The
target branch is the brain-conditioned embeddings (branch F), the source description the `neg_pe` / `neg_pooled` embeddings of that
fixture, the source image its `x0`.

What is promised bit for bit: (a) the call is the loop written out -- per step and per noise ops.flowedit_inputs, one plain batch-1
tranformer_forward per branch (and per image) with its own guidance value, ops.flowedit_step on their concatenation; (b) kept tokens are
the source; (d) a call without the keywords is what it was, and the fp16 fallback's second pass is the written-out loop restarted from
Z = X with the generator's next draws. (c) is a field with a known answer, driven through the scheduler's functions alone.

On the commit before the keywords existed prepare_params swallowed them and the plain call's latents came back: the comparisons of (a)
fail there."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_brain_cfg_generate_gpu import HW, N, T, differ, full_embeds, quiet  # noqa: E402
from tests.test_inpaint_generate_gpu import same_bits  # noqa: E402
from tests.test_solver_generate_gpu import STEPS, W, _generate, hand_loop as euler_loop  # noqa: E402,F401  (W: the fixture)

SEED = 11
G_T, G_S = 3.5, 1.5                   # generate's defaults: guidance_scale and source_guidance_scale


def gen(skip=0, batch=1):
    """the seeded CPU generator, `skip` noise draws of `batch` images on"""
    g = torch.Generator().manual_seed(SEED)
    for _ in range(skip):
        torch.randn((batch, 16, 2 * HW, 2 * HW), generator=g, dtype=torch.float32)
    return g


def src(W):
    return dict(image_latents=W.I["x0"], source_prompt_embeds=W.I["neg_pe"], source_pooled_prompt_embeds=W.I["neg_pooled"])


def hand_loop(model, pipe, I, n_max, n_avg=1, mask=None, batch=1, generator=None, first_noise=True, mc=None, g_t=G_T, g_s=G_S):
    """FlowEdit written out. Z = X; for the last n_max steps of the 6-step schedule: n_avg noises (the first of the call is the caller's
    latents where first_noise, every other a prepare_latents draw from `generator`), ops.flowedit_inputs for each of them from the same Z,
    then per noise one plain batch-1 forward per branch and image -- the target's on inputs[0] with the brain-conditioned embeddings and
    guidance g_t, the source's on inputs[1] with the source embeddings and g_s, invalidate_conditioning between them -- and
    ops.flowedit_step on their concatenation with coef = fp32((s_{i+1} - s_i in fp32) / n_avg). Returns (Z, the (sigma, coef) taken)."""
    from loongx_amd import ops
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.pipeline import calculate_shift, retrieve_timesteps
    from loongx_amd.flux.transformer import tranformer_forward
    tr, sch, mc = pipe.transformer, pipe.scheduler, mc or {}
    branches = ((full_embeds(model, I), g_t), ((I["neg_pe"].cuda(), I["neg_pooled"].cuda()), g_s))
    tokens, cids, tids = Condition("subject", latents=I["cond"].cuda(), latent_hw=(HW, HW), position_delta=[0, -HW]).encode(pipe)
    lat, ids = pipe.prepare_latents(batch, 16, HW * 16, HW * 16, torch.float32, "cuda", None, (I["lat"] if batch == 1 else I["lat2"]).cuda())
    cfg = sch.config
    mu = calculate_shift(N, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
    retrieve_timesteps(sch, STEPS, "cuda", None, np.linspace(1.0, 1 / STEPS, STEPS), mu=mu)
    begin = STEPS - n_max
    timesteps, _, th = pipe.get_timesteps_from(begin, "cuda")
    sched_ts = (th / np.float32(1000)).tolist()
    txt_ids = torch.zeros(T, 3, device="cuda")
    X = I["x0"].cuda().to(torch.float32).expand(batch, -1, -1).contiguous()
    Z = X.clone()
    m = None if mask is None else mask.cuda().to(torch.float32).expand(batch, N, 64).contiguous()
    first = [lat.contiguous()] if first_noise else []
    taken = []
    for j, t in enumerate(timesteps):
        i = begin + j
        noises = [first.pop() if first else pipe.prepare_latents(batch, 16, HW * 16, HW * 16, torch.float32, "cuda", generator, None)[0]
                  for _ in range(n_avg)]
        sigma = float(sch._sig_host[i])
        inputs = [ops.flowedit_inputs(X, Z, nz, sigma) for nz in noises]                 # (all of them before any update of this step)
        coef = float(np.float32(np.float64(np.float32(sch._sig_host[i + 1]) - np.float32(sch._sig_host[i])) / n_avg))
        for inp in inputs:
            vs = []
            for part, ((pe, pooled), g) in enumerate(branches):
                for b in range(batch):
                    tr.invalidate_conditioning()
                    vs.append(tranformer_forward(tr, model_config=mc, condition_latents=tokens, condition_ids=cids, condition_type_ids=tids,
                                                 hidden_states=inp[part, b:b + 1], timestep=t.expand(1) / 1000,
                                                 guidance=torch.full((1,), g, device="cuda"), pooled_projections=pooled,
                                                 encoder_hidden_states=pe, txt_ids=txt_ids, img_ids=ids, joint_attention_kwargs=None,
                                                 return_dict=False, lx_schedule=(j, sched_ts))[0])
            v = torch.cat(vs).contiguous()
            assert v.dtype in (torch.float32, torch.bfloat16) and v.shape == (2 * batch, N, 64)
            ops.flowedit_step(Z, v, coef, m)
            taken.append((sigma, coef))
    tr.invalidate_conditioning()
    return Z.clone(), taken


# ------------------------------------------------------------------------------------------------------------------ (a) the written-out loop
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("n_avg", [1, 2])
@pytest.mark.parametrize("n_max", [6, 4])
def test_the_call_is_the_written_out_loop(W, n_max, n_avg, masked):
    kw = dict(src(W), flowedit_n_max=n_max, flowedit_n_avg=n_avg, **({"latent_mask": W.half} if masked else {}))
    out = quiet(W.out, generator=gen(), **kw)
    got = out.images.clone()
    assert got.shape == W.plain.shape and bool(torch.isfinite(got).all())
    assert not torch.equal(got, W.plain), "the FlowEdit keywords returned the plain call's latents"
    assert not torch.equal(got, W.I["x0"].cuda()), "the edit left the source as it was"
    want, taken = hand_loop(W.model, W.pipe, W.I, n_max, n_avg, W.half if masked else None, generator=gen())
    assert same_bits(got, want), differ(got, want)
    rep = out.lx_flowedit
    assert rep["n_max"] == n_max and rep["n_avg"] == n_avg and rep["begin_index"] == STEPS - n_max
    assert rep["guidance_scale"] == G_T and rep["source_guidance_scale"] == G_S
    assert list(zip(rep["sigmas"], rep["coefs"])) == taken and len(taken) == n_max * n_avg
    assert all(isinstance(x, float) for x in rep["sigmas"] + rep["coefs"]) and all(c < 0 for c in rep["coefs"])
    if masked:                                                                            # (b) kept tokens are the source, bit for bit
        assert same_bits(got[:, :8], W.I["x0"].cuda()[:, :8]) and not torch.equal(got[:, 8:], W.I["x0"].cuda()[:, 8:])
    assert same_bits(quiet(W.run, generator=gen(), **kw), got), "two FlowEdit calls from the same seed differ"
    assert W.pipe.transformer.engine.adapter_weight_tiles == 1
    assert same_bits(W.run(), W.plain), "a plain call after a FlowEdit call changed"


def test_the_default_n_max_and_the_guidance_values(W):
    """6 steps: T - T // 7 = 6. Each branch carries its own distilled-guidance value; the source's changes the result"""
    out = quiet(W.out, generator=gen(), **src(W))
    assert out.lx_flowedit["n_max"] == STEPS and out.lx_flowedit["begin_index"] == 0
    got = quiet(W.run, generator=gen(), guidance_scale=5.5, source_guidance_scale=2.5, **src(W)).clone()
    want, _ = hand_loop(W.model, W.pipe, W.I, STEPS, generator=gen(), g_t=5.5, g_s=2.5)
    assert same_bits(got, want), differ(got, want)
    assert not torch.equal(got, out.images)
    assert W.out().lx_flowedit is None


def test_batch_two_with_one_source_description(W):
    """two images of one prompt (latents [2, ...]), one source image and one source description for both: a forward at batch 4 per step,
    [target 0; target 1; source 0; source 1], and every noise draw is one draw of two images"""
    kw = dict(src(W), latents=W.I["lat2"], num_images_per_prompt=2, flowedit_n_max=4, flowedit_n_avg=2, latent_mask=W.half)
    got = quiet(W.run, generator=gen(), **kw).clone()
    assert got.shape == (2, N, 64) and not torch.equal(got[0], got[1])
    want, _ = hand_loop(W.model, W.pipe, W.I, 4, 2, W.half, batch=2, generator=gen())
    assert same_bits(got, want), differ(got, want)
    assert same_bits(got[:, :8], W.I["x0"].cuda().expand(2, -1, -1)[:, :8])


def test_a_callback_sees_and_may_replace_the_edit_state(W):
    seen = []

    def cb(pipe, i, t, kw):
        seen.append(kw["latents"].clone())
        return {}
    out = W.run(generator=gen(), callback_on_step_end=cb, flowedit_n_max=4, **src(W))
    assert len(seen) == 4 and all(s.shape == (1, N, 64) for s in seen) and same_bits(seen[-1], out)

    def back_to_the_source(pipe, i, t, kw):
        return {"latents": W.I["x0"].cuda().clone()} if i == 3 else {}
    got = W.run(generator=gen(), callback_on_step_end=back_to_the_source, flowedit_n_max=4, **src(W))
    assert same_bits(got, W.I["x0"].cuda())


@pytest.mark.parametrize("kw", [dict(flowedit_n_max=7), dict(flowedit_n_avg=0), dict(solver="dpmpp_2m"), dict(strength=0.5)],
                         ids=["n_max", "n_avg", "solver", "strength"])
def test_a_refused_call_leaves_the_pipeline_as_it_was(W, kw):
    index = W.pipe.scheduler._step_index
    with pytest.raises(ValueError):
        W.run(condition_scale=2.0, **dict(src(W), **kw))
    assert W.model.transformer.c_factor is None and W.pipe.scheduler._step_index == index
    assert same_bits(W.run(), W.plain)


# ------------------------------------------------------------------------------------------------------------------ (d) isolation, fallback
def test_a_call_without_the_keywords_is_what_it_was(W):
    """the plain call and the img2img / inpaint call are the loops written out with the Euler entries, as before the keywords existed, also
    after FlowEdit calls"""
    quiet(W.run, generator=gen(), **src(W))
    assert same_bits(W.run(), W.plain) and same_bits(W.plain, euler_loop(W.model, W.pipe, W.I, solver=False)[0])
    inpaint = W.run(image_latents=W.I["x0"], latent_mask=W.half, strength=0.7).clone()
    assert same_bits(inpaint, euler_loop(W.model, W.pipe, W.I, solver=False, inpaint=(W.I["x0"], W.half, 0.7))[0])
    out = W.out()
    assert out.lx_flowedit is None and out.lx_solver is None


def test_fp16_fallback_starts_from_the_source_and_draws_on(W):
    """on the model whose fp16 operands saturate (the planted bias of tests/test_f16_gpu.py): the image is computed again with bf16
    operands from Z = X at the begin index; the first pass used the caller's latents and n_max n_avg - 1 draws, the second pass takes the
    generator's next n_max n_avg"""
    from tests.test_f16_gpu import _planted_model
    model = _planted_model(bias_value=1.0e5)
    model.flux_pipe.transformer.engine.pair_plan = False
    n_max, n_avg, calls = 4, 2, []
    with pytest.warns(RuntimeWarning, match="recomputing this image with bf16 operands"):
        out = _generate(model, model.flux_pipe, W.I, model_config={"operands": "fp16", "f16_overflow": "fallback"}, generator=gen(),
                        callback_on_step_end=lambda p, i, t, k: calls.append(i) or {}, flowedit_n_max=n_max, flowedit_n_avg=n_avg,
                        latent_mask=W.half, **src(W))
    assert calls == list(range(n_max)) * 2 and out.lx_operands.startswith("bf16")
    want, taken = hand_loop(model, model.flux_pipe, W.I, n_max, n_avg, W.half, generator=gen(skip=n_max * n_avg - 1), first_noise=False,
                            mc={"operands": "bf16", "f16_overflow": "fallback"})
    assert same_bits(out.images, want), differ(out.images, want)
    assert list(zip(out.lx_flowedit["sigmas"], out.lx_flowedit["coefs"])) == taken and len(taken) == n_max * n_avg


# ------------------------------------------------------------------------------------------------------------------ (c) a known answer
U, O2 = 2.0 ** -24, 1 + 2.0 ** -20


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("n_max,n_avg", [(16, 1), (12, 2), (5, 3)])
def test_a_field_with_a_known_answer(n_max, n_avg, masked):
    """No model: v(z, sigma | mu) = (z - mu) / sigma, the flow towards a point mu. The branches differ by Delta = mu_t - mu_s, the noise
    cancels in Vt - Vs = (Z - X - Delta) / sigma, and Euler is exact for this field: Z_i = X + Delta (1 - s_i / s_begin) at every step, the
    end point X + Delta for any n_max and n_avg. 4096 coordinates, N(0, 1) X, mu and noise, the 1024-token schedule at 16 steps, driven
    through scheduler.flowedit_inputs and scheduler.step(flowedit=) alone; the velocities are formed in fp32 from the kernel's own inputs.

    The state is held to the float64 recurrence Zr' = Zr + n_avg coef m (Zr - X - Delta) / s with the recorded fp32 coef. Per forward the
    GPU's update differs from the recurrence's by what the stated operations round (u = 2^-24, first order, times O2):
      the target input r = fl(Z + fl(s_ - X)) misses Z + (s_ - X) by eps_r <= u (|s_ - X| + |r|), so (r - mu_t) - (s_ - mu_s) misses
        Z - X - Delta by eps_r (s_, the source input, is common to both and exact in the difference);
      each velocity fl(fl(a - mu) / s) carries 2 u |v|;   d = fl(vt - vs): u |d|;   fl(m d): u |m d|;   the fma: u |Z'|
        L = |coef| m (eps_r / s + 2 u (|vt| + |vs|) + 2 u |d|) + u |Z'|
    and an error e already in Z reaches Z' with the factor 1 + n_avg coef m / s = 1 - m (1 - s' / s), which lies in [0, 1]: the errors add,
    |Z - Zr| <= sum of L over the forwards so far. The recurrence itself misses the closed form by the rounding of coef alone: n_avg coef
    = (s' - s)(1 + 2u), each factor is off by at most 2 u in absolute terms and none exceeds 1, so |Zr_j - closed_j| <= 2 u j |Delta| O2.
    With a 0/1 mask the kept coordinates stay X, bit for bit."""
    from loongx_amd.flux.pipeline import FlowEditState, FlowMatchEulerDiscreteScheduler, calculate_shift
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    steps, shape = 16, (1, 64, 64)
    g = torch.Generator().manual_seed(5)
    X, mu_t, mu_s = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    m = (torch.rand(shape, generator=g) < 0.5).float().cuda() if masked else None
    sch = FlowMatchEulerDiscreteScheduler()
    cfg = sch.config
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / steps, steps), device="cuda",
                      mu=calculate_shift(1024, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift))
    begin = steps - n_max
    sch.set_begin_index(begin)
    st = FlowEditState(X, m, n_avg)
    sig = sch._sig_host.astype(np.float64)
    X64, D64 = X.double(), mu_t.double() - mu_s.double()
    m64 = torch.ones_like(X64) if m is None else m.double()
    Zr, bound = X64.clone(), torch.zeros_like(X64)
    for j in range(n_max):
        i = begin + j
        s = float(sig[i])
        s32 = torch.tensor(s, dtype=torch.float32, device="cuda")
        batches = sch.flowedit_inputs(st, [torch.randn(shape, generator=g).cuda() for _ in range(n_avg)])
        Zr_start = Zr.clone()
        for k in range(n_avg):
            r, s_ = batches[k, :1], batches[k, 1:]
            vt, vs = (r - mu_t) / s32, (s_ - mu_s) / s32
            eps_r = U * ((s_.double() - X64).abs() + r.double().abs())
            sch.step(torch.cat([vt, vs]), sch.timesteps[i], batches[k], flowedit=st)
            coef = st.taken[-1][2]
            d = (vt.double() - vs.double()).abs()
            bound += abs(coef) * m64 * (eps_r / s + 2 * U * (vt.double().abs() + vs.double().abs()) + 2 * U * d) + U * st.Z.double().abs()
            Zr = Zr + coef * m64 * (Zr_start - X64 - D64) / s
        assert st.taken[-1][:2] == (i, float(sch._sig_host[i])) and sch._step_index == i + 1
        err = (st.Z.double() - Zr).abs()
        assert bool((err <= bound * O2).all()), f"step {i}: {float((err / (bound * O2).clamp_min(1e-300)).max()):.3f} of the rounding bound"
        closed = X64 + m64 * D64 * (1.0 - sig[i + 1] / sig[begin])
        assert bool(((Zr - closed).abs() <= 2 * U * (j + 1) * D64.abs() * O2).all()), f"step {i}: the recurrence left the closed form"
    assert len(st.taken) == n_max * n_avg and sig[steps] == 0.0
    end = X64 + m64 * D64
    assert bool(((st.Z.double() - end).abs() <= (bound + 2 * U * n_max * D64.abs()) * O2).all())
    worst = float(((st.Z.double() - end).abs() / ((bound + 2 * U * n_max * D64.abs()) * O2).clamp_min(1e-300)).max())
    print(f"n_max={n_max} n_avg={n_avg}: end point within {worst:.3f} of the bound; relative L2 "
          f"{float((st.Z.double() - end).norm() / end.norm()):.2e}")
    if masked:
        assert torch.equal(st.Z[m == 0].view(torch.int32), X[m == 0].view(torch.int32)) and not torch.equal(st.Z[m == 1], X[m == 1])
    st.zero()
    assert torch.equal(st.Z, st.X) and st.taken == []
