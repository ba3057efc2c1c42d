"""model_config["step_cache_thresh"] through tranformer_forward(lx_schedule=...) and generate(output_type="latent") on the tiny transformer
(2 + 2 blocks, 2 heads, D = 256): T = 32 text tokens, 128 x 128 pixels = 64 image and 64 condition tokens, 6 steps, identity coefficients
(1, 0) everywhere, so that the threshold applies to the raw distances and nothing depends on the default fit.

Bit for bit: a threshold nothing stays under (1e-30) is the plain call in every operand mode, captured or eager, with the condition cache on;
under a threshold nothing reaches (1e30) only the first and last step compute and every skipped step is embed, X0 + R, final_layer with R
from step 0's own rows, captured or eager. Within the probe's summation bounds (tests/test_step_cache_kernel_gpu.py): every reported
distance against float64 on snapshots of the engine's m buffer. And the state: what resets the report, what forces a compute."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_modules as fm  # noqa: E402

T, HW, N, STEPS, D = 32, 8, 64, 6, 256
U32 = 2.0 ** -23
ID = (1.0, 0.0)
ALWAYS = {"step_cache_thresh": 1e-30, "step_cache_coefficients": ID}
NEVER = {"step_cache_thresh": 1e30, "step_cache_coefficients": ID}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def build_pipe(precise=False, tr=None):
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig
    if tr is None:
        tr = fm.FluxTransformer2DModel(num_layers=2, num_single_layers=2, heads=2, head_dim=128, in_channels=64, joint_dim=4096,
                                       pooled_dim=768, guidance_embeds=True, lora=True)
        fm.init_synthetic_(tr, seed=4, std=0.03, bias_std=0.02, norm_jitter=0.1)
        tr.eval()
    cfg = FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2, in_channels=64, joint_attention_dim=4096,
                     pooled_projection_dim=768, guidance_embeds=True)
    return LxFluxPipeline(LxFluxTransformer.from_state_dict(tr.state_dict(), cfg, "cuda", precise=precise))


class Inputs:
    def __init__(self):
        g = torch.Generator().manual_seed(11)
        self.lat = torch.randn(1, N, 64, generator=g).cuda()
        self.cond = torch.randn(1, N, 64, generator=g).cuda()
        self.pe, self.pooled = (torch.randn(1, T, 4096, generator=g) * 0.1).cuda(), torch.randn(1, 768, generator=g).cuda()
        self.x0 = torch.randn(1, N, 64, generator=g).cuda()
        self.neg_pe, self.neg_pooled = (torch.randn(1, T, 4096, generator=g) * 0.1).cuda(), torch.randn(1, 768, generator=g).cuda()
        self.half = torch.zeros(1, N, 1).cuda()
        self.half[:, N // 2:] = 1.0
        self.guidance = torch.full((1,), 3.5, device="cuda")
        self.txt_ids = torch.zeros(T, 3, device="cuda")


def gen(pipe, I, mc, model=None, **kw):
    """generate()'s whole output for latents in, latents out"""
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    c = Condition("subject", latents=I.cond, latent_hw=(HW, HW), position_delta=[0, -HW])
    return generate(model, pipe, conditions=[c], height=HW * 16, width=HW * 16, num_inference_steps=STEPS, latents=I.lat, prompt_embeds=I.pe,
                    pooled_prompt_embeds=I.pooled, output_type="latent", default_lora=True, use_brain_condition=False, model_config=dict(mc), **kw)


class Driver:
    """The denoise loop on tranformer_forward(lx_schedule=(i, timesteps)) with a plain fp32 Euler step; the conditioning tensors are made
    once, so that successive run() calls meet the same conditioning unless `fresh`."""

    def __init__(self, pipe, I):
        from loongx_amd.flux.condition import Condition
        from loongx_amd.flux.pipeline import calculate_shift, retrieve_timesteps
        self.pipe, self.I, self.tr, self.eng = pipe, I, pipe.transformer, pipe.transformer.engine
        self.tokens, self.cids, self.tids = Condition("subject", latents=I.cond, latent_hw=(HW, HW), position_delta=[0, -HW]).encode(pipe)
        self.lat, self.ids = pipe.prepare_latents(1, 16, HW * 16, HW * 16, torch.float32, "cuda", None, I.lat)
        sch, cfg = pipe.scheduler, pipe.scheduler.config
        mu = calculate_shift(N, cfg.base_image_seq_len, cfg.max_image_seq_len, cfg.base_shift, cfg.max_shift)
        self.timesteps, _ = retrieve_timesteps(sch, STEPS, "cuda", None, np.linspace(1.0, 1 / STEPS, STEPS), mu=mu)
        self.sched_ts = (sch.timesteps_host / np.float32(1000)).tolist()
        self.ds = [float(np.float32(sch._sig_host[i + 1]) - np.float32(sch._sig_host[i])) for i in range(STEPS)]

    def forward(self, mc, i, x, **over):
        from loongx_amd.flux.transformer import tranformer_forward
        I = self.I
        kw = dict(model_config=mc, condition_latents=self.tokens, condition_ids=self.cids, condition_type_ids=self.tids, hidden_states=x,
                  timestep=self.timesteps[i].expand(1) / 1000, guidance=I.guidance, pooled_projections=I.pooled, encoder_hidden_states=I.pe,
                  txt_ids=I.txt_ids, img_ids=self.ids, joint_attention_kwargs=None, return_dict=False, lx_schedule=(i, self.sched_ts))
        kw.update(over)
        return tranformer_forward(self.tr, **kw)[0]

    def run(self, mc, indices=None, fresh=True, after=None):
        """-> (velocities, the latents each forward saw)"""
        if fresh:
            self.tr.invalidate_conditioning()
        x, vs, xs = self.lat, [], []
        for i in (range(STEPS) if indices is None else indices):
            v = self.forward(mc, i, x).clone()
            vs.append(v)
            xs.append(x)
            if after is not None:
                after(i, x, v)
            x = x + self.ds[i] * v
        return vs, xs


@pytest.fixture(scope="module")
def W():
    """one tiny model and its inputs for the whole module, let go of at the end with nothing in flight"""
    import gc
    from types import SimpleNamespace
    I = Inputs()
    pipe = build_pipe()
    w = SimpleNamespace(I=I, pipe=pipe, drv=Driver(pipe, I), eng=pipe.transformer.engine)
    yield w
    vars(w).clear()
    del w, pipe
    torch.cuda.synchronize()
    gc.collect()


# ------------------------------------------------------------------------------------------------------------------ off is off
def test_with_the_key_absent_nothing_exists():
    """on an engine that has never seen the key (its own model: the module's has)"""
    I, pipe = Inputs(), build_pipe()
    eng = pipe.transformer.engine
    out = gen(pipe, I, {})
    assert out.lx_step_cache is None
    drv = Driver(pipe, I)
    drv.run({}, indices=[0, 1])
    assert eng.step_cache_report() is None and eng.step_cache is None
    assert all(getattr(eng, n) is None for n in ("sc_m", "sc_R", "sc_rows", "sc_sums", "sc_host"))
    for off in ({"step_cache_thresh": None}, {"step_cache_thresh": 0, "step_cache_coefficients": [1.0, 0.0]}):
        assert same_bits(gen(pipe, I, off).images, out.images) and eng.sc_m is None
    pipe.transformer.invalidate_conditioning()


# ------------------------------------------------------------------------------------------------------------------ always compute
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("mode", ["bf16", "fp16", "precise", "independent_condition"])
def test_a_threshold_nothing_stays_under_is_the_plain_call(W, mode, graph):
    mc = {"bf16": {}, "fp16": {"operands": "fp16", "f16_overflow": "fallback"}, "precise": {"precise": True},
          "independent_condition": {"independent_condition": True}}[mode]
    pipe = build_pipe(precise=True) if mode == "precise" else W.pipe
    eng = pipe.transformer.engine
    eng.use_graph = graph
    try:
        plain = gen(pipe, W.I, mc)
        cached = gen(pipe, W.I, dict(mc, **ALWAYS))
    finally:
        eng.use_graph = True
    assert plain.lx_step_cache is None and plain.lx_operands == cached.lx_operands
    rep = cached.lx_step_cache
    assert rep["steps"] == STEPS and rep["computed"] == list(range(STEPS)) and rep["rel"][0] is None and all(r > 0 for r in rep["rel"][1:])
    assert rep["acc"] == [0.0] * STEPS and rep["thresh"] == 1e-30 and rep["coefficients"] == ID
    assert same_bits(cached.images, plain.images), f"{int((cached.images != plain.images).sum())} elements differ"
    if mode == "independent_condition":
        assert eng.cond_cache_enabled and eng.cond_cache, "the condition cache was not on"
    assert same_bits(gen(pipe, W.I, mc).images, plain.images), "a plain call after the cached one changed"


# ------------------------------------------------------------------------------------------------------------------ never compute
def skipped_steps_restated(W, graph):
    eng, drv = W.eng, W.drv
    eng.use_graph = graph
    R, checked = [], []

    def after(i, x, v):
        torch.cuda.synchronize()
        if i == 0:                                   # R from step 0's own rows: the final image rows minus the embedded ones, one fp32 subtraction
            x_img = eng.rows(eng.X, "img").clone()
            x0 = torch.empty_like(x_img)
            eng.mode.embed(x.reshape(N, -1), "x_embedder", x0, lora=eng.latent_lora, step=True)
            R.append(x_img - x0)
            assert same_bits(R[0], eng.sc_R), "the engine's residual is not X_img - X0 of step 0"
        elif i < STEPS - 1:                          # a skipped step: embed, X0 + R, final_layer -- the engine's eager pieces
            eng.mods.copy_(eng.sched[1][i])
            rows = eng.rows(eng.X, "img")
            eng.mode.embed(x.reshape(N, -1), "x_embedder", rows, lora=eng.latent_lora, step=True)
            rows.copy_(rows + R[0])
            want = eng.final_layer().clone()
            assert same_bits(v, want), f"step {i}: {int((v != want).sum())} elements differ"
            checked.append(i)
    try:
        vs, _ = drv.run(NEVER, after=after)
    finally:
        eng.use_graph = True
    rep = eng.step_cache_report()
    assert rep["computed"] == [0, STEPS - 1] and rep["steps"] == STEPS and checked == list(range(1, STEPS - 1))
    assert rep["acc"][1:STEPS - 1] == list(np.cumsum(rep["rel"][1:STEPS - 1])) and rep["acc"][-1] == 0.0
    return vs, rep


def test_a_threshold_nothing_reaches_skips_all_but_the_ends(W):
    vs_g, rep_g = skipped_steps_restated(W, graph=True)
    vs_e, rep_e = skipped_steps_restated(W, graph=False)
    assert rep_g == rep_e
    for i, (a, b) in enumerate(zip(vs_g, vs_e)):
        assert same_bits(a, b), f"step {i}: captured and eager differ"
    plain, _ = W.drv.run({})
    assert same_bits(vs_g[0], plain[0]) and not torch.equal(vs_g[1], plain[1])
    out = gen(W.pipe, W.I, NEVER)
    assert out.lx_step_cache["computed"] == [0, STEPS - 1] and bool(torch.isfinite(out.images).all())


# ------------------------------------------------------------------------------------------------------------------ in between
def test_a_middle_threshold_replays_from_its_own_report(W):
    from loongx_amd.flux.step_cache import StepCacheState
    eng, drv = W.eng, W.drv
    drv.run(NEVER)
    first = eng.step_cache_report()["rel"]
    thresh = first[1] + 0.5 * first[2]               # step 1 stays under it, steps 1 + 2 together do not
    mc = {"step_cache_thresh": thresh, "step_cache_coefficients": ID}
    snaps = []
    drv.run(mc, after=lambda i, x, v: snaps.append(eng.sc_m.clone()))
    rep = eng.step_cache_report()
    assert rep["rel"][1] == first[1] and 1 not in rep["computed"] and 2 in rep["computed"] and len(rep["computed"]) < STEPS
    st = StepCacheState(thresh, ID)
    decisions = [st.step(i, STEPS, r) for i, r in enumerate(rep["rel"])]
    assert [i for i, c in enumerate(decisions) if c] == rep["computed"] and st.report() == rep
    # every distance against float64 on the m buffer's snapshots: S1 and S2 are each within their summation bound (no LayerNorm term:
    # the snapshots are the kernel's own m), so rel = S1 / S2 is within (a + b) / (1 - b) of the float64 ratio
    a, b = (D / 64 + 7) * U32, (D / 64 + 6) * U32
    for i in range(1, STEPS):
        m0, m1 = snaps[i - 1].double(), snaps[i].double()
        want = float((m1 - m0).abs().sum() / m0.abs().sum())
        share = abs(rep["rel"][i] - want) / want / ((a + b) / (1 - b))
        print(f"\nstep {i}: rel {rep['rel'][i]:.6e}, float64 {want:.6e}, share of the bound {share:.3f}")
        assert share <= 1.0


# ------------------------------------------------------------------------------------------------------------------ state
def test_what_resets_the_report_and_what_forces_a_compute(W):
    eng, drv = W.eng, W.drv
    drv.run(NEVER, indices=[0, 1, 2])
    assert eng.step_cache_report()["steps"] == 3
    drv.run(NEVER, indices=[0, 1], fresh=False)                      # the same conditioning: step 0 starts the report again
    rep = eng.step_cache_report()
    assert rep["steps"] == 2 and rep["indices"] == [0, 1] and rep["computed"] == [0]
    drv.run(NEVER, indices=[3, 4], fresh=False)                      # a jump computes, the step after it may skip again
    rep = eng.step_cache_report()
    assert rep["indices"] == [0, 1, 3, 4] and rep["computed"] == [0, 3]
    drv.run(NEVER, indices=[0], fresh=True)                          # a new conditioning: a new report
    rep = eng.step_cache_report()
    assert rep["steps"] == 1 and rep["computed"] == [0] and rep["rel"] == [None]
    drv.tr.invalidate_conditioning()
    assert eng.step_cache_report() is None
    drv.run({}, indices=[0, 1])                                      # and a conditioning without the key has none
    assert eng.step_cache_report() is None and eng.step_cache is None


def test_the_schedule_is_required(W):
    drv, eng = W.drv, W.eng
    drv.run({}, indices=[0])
    assert eng.cond_ready
    with pytest.raises(ValueError, match="lx_schedule"):
        drv.forward(NEVER, 0, drv.lat, lx_schedule=None)
    assert not eng.cond_ready and drv.tr._cond_key is None           # as the mask refusals: no conditioning left behind
    with pytest.raises(ValueError, match="step_cache_thresh"):
        drv.forward({"step_cache_thresh": -1.0}, 0, drv.lat)
    assert not eng.cond_ready
    drv.tr.invalidate_conditioning()
    eng.set_conditioning(drv.I.pe, drv.I.pooled, drv.I.guidance, drv.I.txt_ids, drv.ids, drv.tokens, drv.cids, model_config=dict(NEVER))
    with pytest.raises(ValueError, match="step_index"):              # the engine's own entry point: no schedule, no step cache
        eng.forward(drv.lat, drv.timesteps[0].expand(1) / 1000)
    drv.tr.invalidate_conditioning()


def test_the_fp16_fallback_recompute_reports_its_own_steps(W):
    """on the model whose fp16 operands saturate (the planted bias of tests/test_f16_gpu.py)"""
    from tests.test_f16_gpu import _planted_model
    model = _planted_model(bias_value=1.0e5)
    calls = []
    with pytest.warns(RuntimeWarning, match="recomputing this image with bf16 operands"):
        out = gen(model.flux_pipe, W.I, dict(NEVER, operands="fp16", f16_overflow="fallback"), model=model,
                  callback_on_step_end=lambda p, i, t, k: calls.append(i) or {})
    rep = out.lx_step_cache
    assert calls == list(range(STEPS)) * 2 and out.lx_operands.startswith("bf16")
    assert rep["steps"] == STEPS and rep["indices"] == list(range(STEPS)) and rep["computed"] == [0, STEPS - 1]
    want = gen(model.flux_pipe, W.I, dict(NEVER, operands="bf16"), model=model)
    assert same_bits(out.images, want.images) and want.lx_step_cache == rep


# ------------------------------------------------------------------------------------------------------------------ with the other keywords
def test_guided_inpainting_with_the_cache_on(W):
    I = W.I
    out = gen(W.pipe, I, NEVER, true_cfg_scale=2.0, negative_prompt_embeds=I.neg_pe, negative_pooled_prompt_embeds=I.neg_pooled,
              image_latents=I.x0, latent_mask=I.half)
    assert out.lx_step_cache["computed"] == [0, STEPS - 1] and out.lx_step_cache["steps"] == STEPS
    assert out.images.shape == (1, N, 64) and bool(torch.isfinite(out.images).all())
    assert same_bits(out.images[:, :N // 2], I.x0[:, :N // 2]), "where the mask is 0 the result is not the source"
    assert not torch.equal(out.images[:, N // 2:], I.x0[:, N // 2:])
