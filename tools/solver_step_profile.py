#!/usr/bin/env python3
"""What one launch of the scheduler step costs under each solver (generate(solver=)): lx_euler_step against lx_dpmpp2m_step, from a kernel
trace. Not part of bench.py.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/solver_step_profile.py run --solver euler --batch 1
    ... the same with --solver dpmpp_2m, and with --batch 16, each into a directory of its own ...
    python tools/solver_step_profile.py summary DIR [DIR ...] [--out profiles/solver_step.txt]

run: a tiny transformer (2 + 2 blocks, 2 heads, synthetic weights), 512 text + 1024 image tokens (a 512 x 512 image: one part of the step
is batch x 65536 elements), 28 steps, latents in and out, no condition image and no brain signals; two calls, the first the warm-up. Trace
only: the profiler slows the host, so no end-to-end time is taken here.
summary: per directory, the launches of the step kernel (euler_parts_kernel) in the kernel trace, the first call's dropped: their number,
the kernel's name as traced, and the median, minimum and maximum of end - start in microseconds."""
import argparse
import csv
import glob
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, W, STEPS = 512, 32, 32, 28


def run(a):
    sys.path.insert(0, HERE)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/solver_step_profile.py measures on the GPU: none found")
    from loongx_amd.flux.generate import generate
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig, synthetic_weights
    dev = torch.device("cuda:0")
    cfg = FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2, in_channels=64, joint_attention_dim=4096,
                     pooled_projection_dim=768, guidance_embeds=True)
    pipe = LxFluxPipeline(LxFluxTransformer(synthetic_weights(cfg, dev, seed=0), dev))
    B, N = a.batch, H * W
    for call in range(a.calls):
        g = torch.Generator(device=dev).manual_seed(1234 + call)
        lat = torch.randn(B, N, 64, device=dev, generator=g)
        pe, pooled = torch.randn(B, T, 4096, device=dev, generator=g) * 0.1, torch.randn(B, 768, device=dev, generator=g)
        res = generate(None, pipe, height=16 * H, width=16 * W, num_inference_steps=STEPS, latents=lat, prompt_embeds=pe,
                       pooled_prompt_embeds=pooled, output_type="latent", model_config={}, use_brain_condition=False, solver=a.solver)
        torch.cuda.synchronize()
        pipe.transformer.engine.check_status(sync=True)
        assert res.images.shape == (B, N, 64) and bool(torch.isfinite(res.images).all())
        assert (res.lx_solver is not None) == (a.solver == "dpmpp_2m")
        print(f"call {call}: solver {a.solver}, batch {B}, {STEPS} steps: done", flush=True)


def summary(a):
    lines = [f"# tools/solver_step_profile.py: the step kernel's launches in a rocprofv3 kernel trace of {STEPS}-step calls on a tiny transformer at "
             f"{T} + {H * W} tokens (one part of the step: batch x {H * W * 64} elements); the warm-up call's launches dropped; us per launch",
             f"{'trace':28s} {'launches':>8s} {'median':>8s} {'min':>8s} {'max':>8s}  kernel"]
    for d in a.dirs:
        rows = []
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    r = {k.strip().lower(): v for k, v in r.items() if k}
                    if "euler_parts_kernel" in r.get("kernel_name", ""):
                        rows.append((int(r["start_timestamp"]), int(r["end_timestamp"]), r["kernel_name"]))
        rows.sort()
        if len(rows) < 2 * STEPS or len(rows) % STEPS:
            sys.exit(f"{d}: {len(rows)} launches of the step kernel in the trace, expected a multiple of {STEPS}, at least two calls")
        rows = rows[STEPS:]
        us = [(e - s) / 1e3 for s, e, _ in rows]
        names = sorted({n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for _, _, n in rows})
        lines.append(f"{os.path.basename(os.path.normpath(d)):28s} {len(us):8d} {statistics.median(us):8.2f} {min(us):8.2f} {max(us):8.2f}  "
                     f"{', '.join(names)}")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--solver", choices=("euler", "dpmpp_2m"), required=True)
    r.add_argument("--batch", type=int, default=1)
    r.add_argument("--calls", type=int, default=2, help="calls of generate(); the first is the warm-up")
    s = sub.add_parser("summary")
    s.add_argument("dirs", nargs="+")
    s.add_argument("--out", default=None)
    a = ap.parse_args()
    (run if a.cmd == "run" else summary)(a)


if __name__ == "__main__":
    main()
