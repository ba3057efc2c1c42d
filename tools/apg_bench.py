"""ms per call of a guided image with and without adaptive projected guidance (generate(apg_eta=, apg_norm_threshold=, apg_momentum=)) at the
headline shape: 512 text + 1024 image + 1024 condition tokens (512 x 512), 28 steps, bf16 operands, full depth (19 + 38 blocks), synthetic
weights, the EEG replacing the prompt embeddings (brain_replace="per_stream", as tools/brain_cfg_bench.py). Not part of bench.py.

  python tools/apg_bench.py [--images 3] [--brain_scale 2.0] [--text_scale 3.5] [--eta 0.0] [--norm_threshold 15.0] [--momentum -0.5]
                            [--out profiles/apg.txt]

Four arms on one pipeline in one process, alternating image by image: the two-branch guided call [F; T] and the three-branch one [F; T; N],
each as it is (lx_euler_step_cfg / lx_euler_step_cfg3 per step: the code path of the commit before APG) and with APG on (lx_euler_step_apg
per step: a reduce, a total and a step launch; one more read of v and one round trip of M, about 1 MB per image and step here). The first
round is the warm-up (code objects, graph captures) and is not counted. Per arm: ms per generate() call (host clock, device synchronised
before and after), median / minimum / maximum over the counted rounds, images/s, and the package power and shader clock over the arm's
counted calls (bench.PowerSampler). What to look for: the forwards are the same, so an APG arm over its plain arm should sit inside the
box-to-box spread the README states (+-2.5 %)."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, W, STEPS = 512, 32, 32, 28
# (name, true CFG, APG)
ARMS = (("[F; T]", False, False), ("[F; T] + APG", False, True), ("[F; T; N]", True, False), ("[F; T; N] + APG", True, True))


def mean(v):
    v = [x for x in v if x is not None]
    return f"{sum(v) / len(v):.0f}" if v else "n/a"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3, help="counted rounds per arm (one more is the warm-up)")
    ap.add_argument("--brain_scale", type=float, default=2.0, help="brain_guidance_scale of every arm")
    ap.add_argument("--text_scale", type=float, default=3.5, help="true_cfg_scale of the three-branch arms")
    ap.add_argument("--eta", type=float, default=0.0, help="apg_eta of the APG arms")
    ap.add_argument("--norm_threshold", type=float, default=15.0, help="apg_norm_threshold of the APG arms")
    ap.add_argument("--momentum", type=float, default=-0.5, help="apg_momentum of the APG arms")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/apg_bench.py measures on the GPU: none found")
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
    clamped = {arm[0]: None for arm in ARMS}
    for rnd in range(a.images + 1):
        for name, text, apg in ARMS:
            g = torch.Generator(device=dev).manual_seed(1234 + rnd)
            lat, cond = torch.randn(1, N, 64, device=dev, generator=g), torch.randn(1, N, 64, device=dev, generator=g)
            pe, pooled = torch.randn(1, T, 4096, device=dev, generator=g) * 0.1, torch.randn(1, 768, device=dev, generator=g)
            eeg = torch.randn(1, 4, 4096, device=dev, generator=g)
            kw = dict(brain_guidance_scale=a.brain_scale)
            if text:
                kw.update(true_cfg_scale=a.text_scale, negative_prompt_embeds=torch.randn(1, T, 4096, device=dev, generator=g) * 0.1,
                          negative_pooled_prompt_embeds=torch.randn(1, 768, device=dev, generator=g))
            if apg:
                kw.update(apg_eta=a.eta, apg_norm_threshold=a.norm_threshold, apg_momentum=a.momentum)
            c = Condition("subject", latents=cond, latent_hw=(H, W), position_delta=[0, -W])
            power = PowerSampler(dev.index)
            torch.cuda.synchronize()
            power.start()
            t0 = time.perf_counter()
            res = generate(model, pipe, conditions=[c], height=16 * H, width=16 * W, num_inference_steps=STEPS, latents=lat, prompt_embeds=pe,
                           pooled_prompt_embeds=pooled, output_type="latent", model_config=mc, default_lora=True, use_brain_condition=True,
                           fuse_flag=False, brain_replace="per_stream", additional_condition1=eeg, **kw)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            pw = power.stop() or {}
            pipe.transformer.engine.check_status(sync=True)
            out = res.images
            assert out.shape == (1, N, 64) and bool(torch.isfinite(out).all()) and (res.lx_apg is not None) == apg
            if apg:                                                    # (after the clock stopped: how many steps the threshold bound)
                clamped[name] = int((res.lx_apg[:, 0, 0] > a.norm_threshold ** 2).sum())
            print(f"round {rnd} {name}: {ms:.1f} ms", flush=True)
            if rnd:
                recs[name].append(dict(ms=ms, W=pw.get("avg_W"), sclk=pw.get("sclk_MHz_avg")))
    lines = [f"# tools/apg_bench.py on {torch.cuda.get_device_name(0)}: 512 + 1024 + 1024 tokens, {STEPS} steps, bf16 operands, full depth, EEG "
             f"per_stream; ms per generate() call at batch 1, {a.images} counted rounds per arm, arms alternating; brain_guidance_scale "
             f"{a.brain_scale}, true_cfg_scale {a.text_scale}; apg_eta {a.eta}, apg_norm_threshold {a.norm_threshold}, apg_momentum {a.momentum}",
             f"{'arm':18s} {'fwd batch':>9s} {'median':>9s} {'min':>9s} {'max':>9s} {'images/s':>9s} {'clamped':>8s} {'avg W':>7s} {'sclk MHz':>9s}"]
    med = {}
    for name, text, apg in ARMS:
        ms = [r["ms"] for r in recs[name]]
        med[name] = statistics.median(ms)
        steps = "-" if clamped[name] is None else f"{clamped[name]}/{STEPS}"
        lines.append(f"{name:18s} {2 + text:9d} {med[name]:9.1f} {min(ms):9.1f} {max(ms):9.1f} {1e3 / med[name]:9.3f} {steps:>8s} "
                     f"{mean([r['W'] for r in recs[name]]):>7s} {mean([r['sclk'] for r in recs[name]]):>9s}")
    for name in ("[F; T]", "[F; T; N]"):
        lines.append(f"# {name} + APG / {name}, ms per call: {med[name + ' + APG'] / med[name]:.4f} "
                     f"({(med[name + ' + APG'] - med[name]) / STEPS * 1e3:+.0f} us per step; the same forwards: expected within 1 +- 0.025)")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
