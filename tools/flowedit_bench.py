#!/usr/bin/env python3
"""What FlowEdit costs (generate(source_prompt_embeds=...)): images/s of a FlowEdit call next to a true-CFG call of as many steps, and the
two new launches from a kernel trace. Not part of bench.py.

    python tools/flowedit_bench.py bench [--images 3] --out DIR/bench.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace -- python tools/flowedit_bench.py trace --meta DIR/trace/meta.json
    python tools/flowedit_bench.py summary DIR/trace --bench DIR/bench.txt [--out profiles/flowedit.txt]

bench: the headline shape, 512 text + 1024 image + 1024 condition tokens (512 x 512), bf16 operands, full depth (19 + 38 blocks),
synthetic weights, batch 1. Two arms on one pipeline in one process, alternating image by image, the first round the warm-up: FlowEdit at
T = 28, n_max = 24, n_avg = 1 (24 forwards at batch 2, a noise draw, lx_flowedit_inputs and lx_flowedit_step per step) and true CFG at 24
steps (24 forwards at batch 2 and lx_euler_step_cfg per step). Both run one forward at batch 2 per step, so they are expected to be equal
up to the per-step noise draw. ms per generate() call on the host clock, device synchronised before and after.
trace: a tiny transformer (2 + 2 blocks, 2 heads), 512 + 1024 tokens (one part is 65536 elements), T = 28, n_max = 24; two calls without
a mask and two with one, the first of each the warm-up. Writes the format of v the step saw to --meta.
summary: per new kernel as traced, the launches of each pair's second call: their number, median / minimum / maximum of end - start in
microseconds, the algorithmic bytes -- 20 n for the inputs (three reads, two writes); for the step 8 n for Z, 4 n or 8 n for a bf16 or fp32
v, 4 n more with a mask -- and the bytes/s the median achieves."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, W, STEPS, N_MAX = 512, 32, 32, 28, 24
N = H * W * 64


def _imports():
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/flowedit_bench.py measures on the GPU: none found")
    return torch


def bench(a):
    torch = _imports()
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig, synthetic_weights
    dev = torch.device("cuda:0")
    pipe = LxFluxPipeline(LxFluxTransformer(synthetic_weights(FluxConfig(), dev, seed=0), dev))
    tokens = H * W
    arms = ("flowedit, 24 of 28", "true cfg, 24 steps")
    recs = {name: [] for name in arms}
    for rnd in range(a.images + 1):
        for name in arms:
            g = torch.Generator(device=dev).manual_seed(1234 + rnd)
            lat, cond, x0 = (torch.randn(1, tokens, 64, device=dev, generator=g) for _ in range(3))
            pe, pooled = torch.randn(1, T, 4096, device=dev, generator=g) * 0.1, torch.randn(1, 768, device=dev, generator=g)
            pe2, pooled2 = torch.randn(1, T, 4096, device=dev, generator=g) * 0.1, torch.randn(1, 768, device=dev, generator=g)
            if name.startswith("flowedit"):
                kw = dict(num_inference_steps=STEPS, flowedit_n_max=N_MAX, image_latents=x0, source_prompt_embeds=pe2,
                          source_pooled_prompt_embeds=pooled2, generator=g)
            else:
                kw = dict(num_inference_steps=N_MAX, true_cfg_scale=3.5, negative_prompt_embeds=pe2, negative_pooled_prompt_embeds=pooled2)
            c = Condition("subject", latents=cond, latent_hw=(H, W), position_delta=[0, -W])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = generate(None, pipe, conditions=[c], height=16 * H, width=16 * W, latents=lat, prompt_embeds=pe, pooled_prompt_embeds=pooled,
                           output_type="latent", model_config={}, default_lora=True, use_brain_condition=False, **kw)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            pipe.transformer.engine.check_status(sync=True)
            assert out.images.shape == (1, tokens, 64) and bool(torch.isfinite(out.images).all())
            assert (out.lx_flowedit is not None) == name.startswith("flowedit")
            print(f"round {rnd} {name}: {ms:.1f} ms", flush=True)
            if rnd:
                recs[name].append(ms)
    lines = [f"# tools/flowedit_bench.py bench on {torch.cuda.get_device_name(0)}: 512 + 1024 + 1024 tokens, bf16 operands, full depth, batch 1; "
             f"ms per generate() call, {a.images} counted rounds per arm, arms alternating; both arms run {N_MAX} forwards at batch 2",
             f"{'arm':20s} {'median':>9s} {'min':>9s} {'max':>9s} {'images/s':>9s}"]
    for name in arms:
        ms = recs[name]
        lines.append(f"{name:20s} {statistics.median(ms):9.1f} {min(ms):9.1f} {max(ms):9.1f} {1e3 / statistics.median(ms):9.3f}")
    fe, cfg = (statistics.median(recs[n]) for n in arms)
    lines.append(f"# flowedit / true cfg, ms per call: {fe / cfg:.3f}")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


def trace(a):
    torch = _imports()
    from loongx_amd.flux.generate import generate
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig, synthetic_weights
    dev = torch.device("cuda:0")
    cfg = FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2, in_channels=64, joint_attention_dim=4096,
                     pooled_projection_dim=768, guidance_embeds=True)
    pipe = LxFluxPipeline(LxFluxTransformer(synthetic_weights(cfg, dev, seed=0), dev))
    tokens, seen = H * W, set()
    step = pipe.scheduler.step

    def recording_step(model_output, *args, **kw):
        seen.add(str(model_output.dtype).replace("torch.", ""))
        return step(model_output, *args, **kw)
    pipe.scheduler.step = recording_step
    for masked in (False, True):
        for call in range(2):
            g = torch.Generator(device=dev).manual_seed(1234 + call)
            lat, x0 = (torch.randn(1, tokens, 64, device=dev, generator=g) for _ in range(2))
            pe, pooled = torch.randn(1, T, 4096, device=dev, generator=g) * 0.1, torch.randn(1, 768, device=dev, generator=g)
            pe2, pooled2 = torch.randn(1, T, 4096, device=dev, generator=g) * 0.1, torch.randn(1, 768, device=dev, generator=g)
            kw = {"latent_mask": (torch.rand(1, tokens, 1, device=dev, generator=g) < 0.5).float()} if masked else {}
            res = generate(None, pipe, height=16 * H, width=16 * W, num_inference_steps=STEPS, latents=lat, prompt_embeds=pe,
                           pooled_prompt_embeds=pooled, output_type="latent", model_config={}, use_brain_condition=False, image_latents=x0,
                           source_prompt_embeds=pe2, source_pooled_prompt_embeds=pooled2, flowedit_n_max=N_MAX, generator=g, **kw)
            torch.cuda.synchronize()
            pipe.transformer.engine.check_status(sync=True)
            assert res.images.shape == (1, tokens, 64) and bool(torch.isfinite(res.images).all()) and len(res.lx_flowedit["coefs"]) == N_MAX
            print(f"{'masked' if masked else 'unmasked'} call {call}: done", flush=True)
    if a.meta:
        os.makedirs(os.path.dirname(a.meta) or ".", exist_ok=True)
        json.dump({"v": sorted(seen), "n": N, "device": torch.cuda.get_device_name(0)}, open(a.meta, "w"))


def summary(a):
    meta = json.load(open(os.path.join(a.dir, "meta.json")))
    assert len(meta["v"]) == 1, meta
    v_bytes = {"float32": 8, "bfloat16": 4}[meta["v"][0]]
    rows = {}
    for path in sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                r = {k.strip().lower(): v for k, v in r.items() if k}
                name = r.get("kernel_name", "")
                if "flowedit_" in name:
                    name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                    rows.setdefault(name, []).append((int(r["start_timestamp"]), int(r["end_timestamp"])))
    lines = [f"# tools/flowedit_bench.py trace + summary on {meta['device']}: the new kernels' launches in a rocprofv3 kernel trace of FlowEdit "
             f"calls (T = {STEPS}, n_max = {N_MAX}, n_avg = 1) on a tiny transformer at {T} + {H * W} tokens: n = {N} elements, v {meta['v'][0]}; "
             "the counted call's launches; us per launch, algorithmic bytes, and the bytes/s of the median",
             f"{'kernel':44s} {'launches':>8s} {'median':>8s} {'min':>8s} {'max':>8s} {'bytes':>9s} {'GB/s':>8s}"]
    for name in sorted(rows):
        launches = sorted(rows[name])
        # inputs: both pairs of calls launch it (4 x n_max, the counted ones the 2nd and 4th call's); a step kernel: one pair (2 x n_max)
        if len(launches) not in (2 * N_MAX, 4 * N_MAX):
            sys.exit(f"{name}: {len(launches)} launches in the trace, expected {2 * N_MAX} or {4 * N_MAX}")
        counted = launches[N_MAX:2 * N_MAX] + launches[3 * N_MAX:]
        us = [(e - s) / 1e3 for s, e in counted]
        per_element = 20 if "inputs" in name else 8 + v_bytes + (4 if "true" in name else 0)
        med = statistics.median(us)
        lines.append(f"{name:44s} {len(us):8d} {med:8.2f} {min(us):8.2f} {max(us):8.2f} {per_element * N:9d} {per_element * N / med / 1e3:8.1f}")
    txt = (open(a.bench).read() if a.bench else "") + "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("bench")
    b.add_argument("--images", type=int, default=3, help="counted rounds per arm (one more is the warm-up)")
    b.add_argument("--out", default=None)
    t = sub.add_parser("trace")
    t.add_argument("--meta", default=None)
    s = sub.add_parser("summary")
    s.add_argument("dir")
    s.add_argument("--bench", default=None)
    s.add_argument("--out", default=None)
    a = ap.parse_args()
    {"bench": bench, "trace": trace, "summary": summary}[a.cmd](a)


if __name__ == "__main__":
    main()
