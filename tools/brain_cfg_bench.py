"""images/s of an image guided along the brain signal (generate(brain_guidance_scale=): one forward at batch 2B per step, [full; text]; with
true_cfg_scale and negative embeddings as well at batch 3B, [full; text; negative]) next to the plain calls of those batches, at the headline
shape: 512 text + 1024 image + 1024 condition tokens (512 x 512), 28 steps, bf16 operands, full depth (19 + 38 blocks), synthetic weights,
the EEG replacing the prompt embeddings (brain_replace="per_stream", as bench.py's headline does). Not part of bench.py.

  python tools/brain_cfg_bench.py [--images 3] [--brain_scale 2.0] [--text_scale 3.5] [--out profiles/brain_cfg.txt]

Five arms on one pipeline in one process, alternating image by image: the plain call at batch 1, 2 and 3, the two-branch guided call at
batch 1 and the three-branch guided call at batch 1. The first round is the warm-up (code objects, graph captures) and is not counted. Per
arm: ms per generate() call (host clock, device synchronised before and after), median / minimum / maximum over the counted rounds,
images/s = batch / median, ms per forward row (median / steps / forward batch), and the package power and shader clock over the arm's
counted calls (bench.PowerSampler). What to look for: a guided call and the plain call of its forward batch run the same forwards, so their
ms per call should agree within the box-to-box spread the README states (+-2.5 %); the guided call runs the CS3 encoders once for one image
instead of k, and one lx_euler_step_cfg / lx_euler_step_cfg3 in place of lx_euler_step."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, W, STEPS = 512, 32, 32, 28
# (name, batch, brain guidance, true CFG)
ARMS = (("plain, batch 1", 1, False, False), ("plain, batch 2", 2, False, False), ("plain, batch 3", 3, False, False),
        ("[F; T], batch 1", 1, True, False), ("[F; T; N], batch 1", 1, True, True))


def mean(v):
    v = [x for x in v if x is not None]
    return f"{sum(v) / len(v):.0f}" if v else "n/a"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3, help="counted rounds per arm (one more is the warm-up)")
    ap.add_argument("--brain_scale", type=float, default=2.0, help="brain_guidance_scale of the guided arms")
    ap.add_argument("--text_scale", type=float, default=3.5, help="true_cfg_scale of the three-branch arm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/brain_cfg_bench.py measures on the GPU: none found")
    from bench import PowerSampler
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig, synthetic_weights
    from loongx_amd.train.model import OminiModel, synthetic_cs3_state_dict
    dev = torch.device("cuda:0")
    mc = {"union_cond_attn": True}
    model = OminiModel.from_pipe(LxFluxPipeline(LxFluxTransformer(synthetic_weights(FluxConfig(), dev, seed=0), dev)),
                                 synthetic_cs3_state_dict(0), mc, dev)
    pipe = model.flux_pipe
    N = H * W
    recs = {arm[0]: [] for arm in ARMS}
    for rnd in range(a.images + 1):
        for name, B, brain, text in ARMS:
            g = torch.Generator(device=dev).manual_seed(1234 + rnd)
            lat, cond = torch.randn(B, N, 64, device=dev, generator=g), torch.randn(B, N, 64, device=dev, generator=g)
            pe, pooled = torch.randn(B, T, 4096, device=dev, generator=g) * 0.1, torch.randn(B, 768, device=dev, generator=g)
            eeg = torch.randn(B, 4, 4096, device=dev, generator=g)
            kw = {}
            if brain:
                kw["brain_guidance_scale"] = a.brain_scale
            if text:
                kw.update(true_cfg_scale=a.text_scale, negative_prompt_embeds=torch.randn(1, T, 4096, device=dev, generator=g) * 0.1,
                          negative_pooled_prompt_embeds=torch.randn(1, 768, device=dev, generator=g))
            c = Condition("subject", latents=cond, latent_hw=(H, W), position_delta=[0, -W])
            power = PowerSampler(dev.index)
            torch.cuda.synchronize()
            power.start()
            t0 = time.perf_counter()
            out = generate(model, pipe, conditions=[c], height=16 * H, width=16 * W, num_inference_steps=STEPS, latents=lat, prompt_embeds=pe,
                           pooled_prompt_embeds=pooled, output_type="latent", model_config=mc, default_lora=True, use_brain_condition=True,
                           fuse_flag=False, brain_replace="per_stream", additional_condition1=eeg, **kw).images
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            pw = power.stop() or {}
            pipe.transformer.engine.check_status(sync=True)
            assert out.shape == (B, N, 64) and bool(torch.isfinite(out).all())
            print(f"round {rnd} {name}: {ms:.1f} ms", flush=True)
            if rnd:
                recs[name].append(dict(ms=ms, W=pw.get("avg_W"), sclk=pw.get("sclk_MHz_avg")))
    lines = [f"# tools/brain_cfg_bench.py on {torch.cuda.get_device_name(0)}: 512 + 1024 + 1024 tokens, {STEPS} steps, bf16 operands, full depth, "
             f"EEG per_stream; ms per generate() call, {a.images} counted rounds per arm, arms alternating; brain_guidance_scale "
             f"{a.brain_scale}, true_cfg_scale {a.text_scale}",
             f"{'arm':20s} {'fwd batch':>9s} {'median':>9s} {'min':>9s} {'max':>9s} {'images/s':>9s} {'ms/fwd row':>10s} {'avg W':>7s} {'sclk MHz':>9s}"]
    med = {}
    for name, B, brain, text in ARMS:
        ms = [r["ms"] for r in recs[name]]
        med[name], rows = statistics.median(ms), B * (1 + brain + text)
        lines.append(f"{name:20s} {rows:9d} {med[name]:9.1f} {min(ms):9.1f} {max(ms):9.1f} {B * 1e3 / med[name]:9.3f} "
                     f"{med[name] / STEPS / rows:10.2f} {mean([r['W'] for r in recs[name]]):>7s} {mean([r['sclk'] for r in recs[name]]):>9s}")
    lines.append(f"# [F; T] batch 1 / plain batch 2, ms per call: {med['[F; T], batch 1'] / med['plain, batch 2']:.3f} "
                 "(the same forwards: expected within 1 +- 0.025)")
    lines.append(f"# [F; T; N] batch 1 / plain batch 3, ms per call: {med['[F; T; N], batch 1'] / med['plain, batch 3']:.3f} "
                 "(the same forwards: expected within 1 +- 0.025)")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
