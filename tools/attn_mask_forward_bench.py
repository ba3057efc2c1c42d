"""Denoise step time with an attention_mask (generate(..., joint_attention_kwargs={"attention_mask": m})) against the same loop without
one: full depth (19 + 38 blocks), batch 1, 28 steps, T = 512 text tokens, one condition image. Not part of bench.py.

  python tools/attn_mask_forward_bench.py [--hw 32] [--images 5] [--cases none,all_true,keypad64] [--out profiles/attn_mask_forward.txt]

Cases: none (no mask: the unmasked kernels), all_true (bool [S, S], every tile FULL), keypad64 (text_padding_mask: 64 real text tokens,
the other 448 masked as keys for every query: 7 of the 8 text key tiles are EMPTY). The cases alternate image by image; the first round
is the warm-up (code objects, graph capture) and is not counted. Per case: ms per denoise step = the wall time of one generate() call
(host clock, device synchronised before and after) / 28; median, minimum and maximum over the counted images."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loongx_amd.flux.condition import Condition  # noqa: E402
from loongx_amd.flux.generate import generate  # noqa: E402
from loongx_amd.flux.pipeline import LxFluxPipeline  # noqa: E402
from loongx_amd.flux.transformer import LxFluxTransformer  # noqa: E402
from loongx_amd.flux.weights import FluxConfig, synthetic_weights  # noqa: E402

T, STEPS = 512, 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hw", type=int, default=32, help="packed latent grid side: 32 = 512x512, 64 = 1024x1024")
    ap.add_argument("--images", type=int, default=5, help="counted images per case (one more is the warm-up)")
    ap.add_argument("--cases", default="none,all_true,keypad64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cases = a.cases.split(",")
    pipe = LxFluxPipeline(LxFluxTransformer(synthetic_weights(FluxConfig(), dev, seed=0), dev))
    N = a.hw * a.hw
    S = T + 2 * N
    masks = {"none": None}
    if "all_true" in cases:
        masks["all_true"] = torch.ones(S, S, dtype=torch.bool, device=dev)
    if "keypad64" in cases:
        from loongx_amd.flux.pipeline_tools import text_padding_mask
        masks["keypad64"] = text_padding_mask([64], T, N, N).to(dev)
    g = torch.Generator(device=dev).manual_seed(1234)
    times = {c: [] for c in cases}
    for rnd in range(a.images + 1):
        x = dict(lat=torch.randn(1, N, 64, device=dev, generator=g), cond=torch.randn(1, N, 64, device=dev, generator=g),
                 pe=torch.randn(1, T, 4096, device=dev, generator=g) * 0.1, pooled=torch.randn(1, 768, device=dev, generator=g))
        for c in cases:
            cond = Condition("subject", latents=x["cond"], latent_hw=(a.hw, a.hw), position_delta=[0, -a.hw])
            kw = {} if masks[c] is None else {"joint_attention_kwargs": {"attention_mask": masks[c]}}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = generate(None, pipe, conditions=[cond], height=16 * a.hw, width=16 * a.hw, num_inference_steps=STEPS, latents=x["lat"],
                           prompt_embeds=x["pe"], pooled_prompt_embeds=x["pooled"], output_type="latent", model_config={"union_cond_attn": True},
                           default_lora=True, use_brain_condition=False, **kw).images
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / STEPS
            assert torch.isfinite(out).all()
            if rnd:
                times[c].append(ms)
            print(f"round {rnd} {c}: {ms:.3f} ms/step", flush=True)
    pipe.transformer.engine.check_status(sync=True)
    lines = [f"# tools/attn_mask_forward_bench.py on {torch.cuda.get_device_name(0)}: {16 * a.hw} x {16 * a.hw}, batch 1, {STEPS} steps, S = {S}; "
             f"ms per denoise step (generate() wall time / {STEPS}), {a.images} images per case, cases alternating",
             f"{'case':10s} {'median':>8s} {'min':>8s} {'max':>8s} {'x none':>7s}"]
    base = statistics.median(times[cases[0]])
    for c in cases:
        t = times[c]
        lines.append(f"{c:10s} {statistics.median(t):8.3f} {min(t):8.3f} {max(t):8.3f} {statistics.median(t) / base:7.3f}")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
