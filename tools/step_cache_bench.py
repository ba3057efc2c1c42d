"""images/s with model_config step_cache_thresh at the headline shape: full depth (19 + 38 blocks), synthetic weights, bf16 operands, batch
1, 512 text + 1024 image + 1024 condition tokens (512 x 512), 28 steps. Not part of bench.py.

  python tools/step_cache_bench.py [--images 3] [--out profiles/step_cache.txt]

Six arms in ONE process, alternating image by image on the same inputs (seeded by the round): plain (no key), always-compute
(thresh = 1e-30: every step probes, reads the two doubles and runs its blocks), and thresh 0.25 / 0.4 / 0.6 / 0.8 with the default
coefficients. The first round is the warm-up (code objects, graph captures) and is not counted. Per arm: ms per generate() call (host
clock, device synchronised before and after), median / minimum / maximum over the counted rounds, images/s = 1 / median, the computed
steps of 28, the relative L2 distance of the last round's final latents from the plain arm's, and the mean device time of a computed and
of a skipped step (events recorded by a step-end callback; step 0, which carries the conditioning, is left out) and of the probe part
alone (its captured graph replayed between two events after the image).

The weights are synthetic N(0, 0.02^2): they do not have a trained checkpoint's step-to-step statistics, so neither the number of
skipped steps at a threshold nor the distance from the plain arm says anything about a real model. The default coefficients are the
FLUX.1-dev fit of the TeaCache recipe quoted from memory, fitted without a condition stream. What the table does measure: the cost of
the probe and the host read (always-compute against plain) and how the rate follows the number of computed steps."""
import argparse
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
T, STEPS, HW = 512, 28, 32
ARMS = [("plain", {}), ("always", {"step_cache_thresh": 1e-30}), ("0.25", {"step_cache_thresh": 0.25}), ("0.4", {"step_cache_thresh": 0.4}),
        ("0.6", {"step_cache_thresh": 0.6}), ("0.8", {"step_cache_thresh": 0.8})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3, help="counted rounds per arm (one more is the warm-up)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/step_cache_bench.py measures on the GPU: none found")
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig, synthetic_weights
    dev = torch.device("cuda:0")
    pipe = LxFluxPipeline(LxFluxTransformer(synthetic_weights(FluxConfig(), dev, seed=0), dev))
    eng = pipe.transformer.engine
    N = HW * HW
    recs = {name: [] for name, _ in ARMS}
    last = {}

    def image(rnd, mc):
        g = torch.Generator(device=dev).manual_seed(1234 + rnd)
        x = dict(lat=torch.randn(1, N, 64, device=dev, generator=g), cond=torch.randn(1, N, 64, device=dev, generator=g),
                 pe=torch.randn(1, T, 4096, device=dev, generator=g) * 0.1, pooled=torch.randn(1, 768, device=dev, generator=g))
        cond = Condition("subject", latents=x["cond"], latent_hw=(HW, HW), position_delta=[0, -HW])
        events = [torch.cuda.Event(enable_timing=True) for _ in range(STEPS)]

        def mark(p, i, t, kw):
            events[i].record()
            return {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = generate(None, pipe, conditions=[cond], height=16 * HW, width=16 * HW, num_inference_steps=STEPS, latents=x["lat"],
                       prompt_embeds=x["pe"], pooled_prompt_embeds=x["pooled"], output_type="latent", model_config=dict(mc), default_lora=True,
                       use_brain_condition=False, callback_on_step_end=mark)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        eng.check_status(sync=True)
        assert bool(torch.isfinite(out.images).all())
        step_ms = [None] + [events[i - 1].elapsed_time(events[i]) for i in range(1, STEPS)]
        rep = out.lx_step_cache
        computed = set(range(STEPS)) if rep is None else set(rep["computed"])
        return dict(ms=ms, computed=len(computed), comp_ms=[step_ms[i] for i in range(1, STEPS) if i in computed],
                    skip_ms=[step_ms[i] for i in range(1, STEPS) if i not in computed]), out.images.double()

    for rnd in range(a.images + 1):
        for name, mc in ARMS:
            r, lat = image(rnd, mc)
            print(f"round {rnd} {name}: {r['ms']:.1f} ms, computed {r['computed']} of {STEPS}", flush=True)
            if rnd:
                recs[name].append(r)
            last[name] = lat
    # the probe part alone: the first graph of a step-cache entry (probe, body, reuse), replayed on the buffers the last image left
    probe_ms = None
    parts = [g for g in eng.graphs.values() if isinstance(g, tuple)]
    if parts:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        parts[0][0].replay()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(50):
            parts[0][0].replay()
        e1.record()
        torch.cuda.synchronize()
        probe_ms = e0.elapsed_time(e1) / 50

    def mean(v):
        return f"{sum(v) / len(v):.3f}" if v else "n/a"
    base = statistics.median(r["ms"] for r in recs["plain"])
    spread = (max(r["ms"] for r in recs["plain"]) - min(r["ms"] for r in recs["plain"])) / base
    lines = [f"# tools/step_cache_bench.py on {torch.cuda.get_device_name(0)}: bf16 operands, batch 1, {T} + {N} + {N} tokens, {STEPS} steps, full depth, "
             f"synthetic weights; {a.images} counted rounds per arm, arms alternating image by image in one process",
             "# synthetic N(0, 0.02^2) weights do not have a trained checkpoint's step-to-step statistics: the computed-step counts and the distances "
             "from the plain arm below say nothing about a real model; the default coefficients are quoted from memory (FLUX.1-dev, no condition stream)",
             f"{'arm':8s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'images/s':>9s} {'x plain':>8s} {'computed':>9s} {'28/k':>6s} {'rel L2':>10s} "
             f"{'computed step ms':>17s} {'skipped step ms':>16s}"]
    for name, _ in ARMS:
        ms = [r["ms"] for r in recs[name]]
        med = statistics.median(ms)
        k = recs[name][-1]["computed"]
        diff = float((last[name] - last["plain"]).norm() / last["plain"].norm())
        lines.append(f"{name:8s} {med:10.1f} {min(ms):9.1f} {max(ms):9.1f} {1e3 / med:9.3f} {base / med:8.3f} {k:6d}/{STEPS} {STEPS / k:6.2f} {diff:10.3e} "
                     f"{mean([v for r in recs[name] for v in r['comp_ms']]):>17s} {mean([v for r in recs[name] for v in r['skip_ms']]):>16s}")
    lines.append(f"# plain arm's spread (max - min) / median: {spread:.2%}; always-compute against plain: "
                 f"{statistics.median(r['ms'] for r in recs['always']) / base - 1:+.2%}")
    lines.append(f"# the probe part alone (image embed + lx_ln_modulate_delta, captured, mean of 50 replays): "
                 + (f"{probe_ms:.4f} ms" if probe_ms is not None else "n/a"))
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
