"""Precise mode with the step-invariant condition stream cached (model_config independent_condition; engine.cond_cache) against the same
build recomputing it every step (LX_COND_CACHE=0): full depth (19 + 38 blocks), synthetic weights, batch 1, 512 text + 1024 image +
1024 condition tokens, 28 steps. Not part of bench.py.

  python tools/precise_cond_cache_bench.py [--images 3] [--attn-reps 20] [--attn-brackets 7] [--out profiles/precise_cond_cache.txt]

The two arms alternate image by image in one process (the engine's cond_cache_enabled is what LX_COND_CACHE sets at construction; the step
graphs are keyed by it, so each arm replays its own); the first round is the warm-up (code objects, graph capture) and is not counted.
Per arm: ms per image = the wall time of one generate() call (host clock, device synchronised before and after); median, minimum and
maximum over the counted images. Then the split-bf16 attention kernel alone at this shape (24 heads), microseconds per launch (median,
minimum and maximum over --attn-brackets event brackets of --attn-reps launches each), for the three launch forms of a forward: all
queries, n_qseg = 2 (a cached step's) and the image segment only (the last single block's)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loongx_amd import ops  # noqa: E402
from loongx_amd.flux.condition import Condition  # noqa: E402
from loongx_amd.flux.generate import generate  # noqa: E402
from loongx_amd.flux.pipeline import LxFluxPipeline  # noqa: E402
from loongx_amd.flux.transformer import LxFluxTransformer  # noqa: E402
from loongx_amd.flux.weights import FluxConfig, synthetic_weights  # noqa: E402

T, HW, STEPS = 512, 32, 28
ARMS = (("LX_COND_CACHE=1", True), ("LX_COND_CACHE=0", False))


def attn_forms(dev, reps, brackets):
    """us per lx_attn_fwd_split launch at B = 1, H = 24, segments (512, 1024, 1024), condition queries masked from text and image keys"""
    B, H, lens = 1, 24, (T, HW * HW, HW * HW)
    D, M = H * 128, sum(lens)
    g = torch.Generator(device=dev).manual_seed(5)
    buf = torch.randn(M, 3 * D, device=dev, generator=g)
    row0, vt0 = [0, lens[0], lens[0] + lens[1]], [0, lens[0], lens[0] + lens[1]]
    QK2 = torch.zeros(M, 4 * D, dtype=torch.bfloat16, device=dev)
    VT2 = torch.zeros(2, B, H, 128, M, dtype=torch.bfloat16, device=dev)
    ops.qkv_prep_split_segs(buf, 2 * D, 0, D, [(row0[i], L, vt0[i], None, None, None, None) for i, L in enumerate(lens)], B, H, QK2,
                            q2_col=2 * D, k2_col=0, lo_off=D, VT2=VT2)
    O = torch.zeros(M, 2 * D, dtype=torch.bfloat16, device=dev)
    ninf = float("-inf")
    bias = [[0, 0, 0], [0, 0, 0], [ninf, ninf, 0]]
    forms = (("all queries", {}), ("n_qseg = 2", dict(n_qseg=2)), ("image only", dict(qseg_mask=0b010)))
    out = {name: [] for name, _ in forms}

    def run(kw):
        ops.attn_fwd_split(QK2, VT2, O, q_col=2 * D, k_col=0, qk_lo_off=D, o_col=0, o_lo_off=D, B=B, H=H, seg_row0=row0, seg_len=list(lens),
                           seg_vt0=vt0, bias=bias, **kw)
    for rnd in range(brackets + 1):                          # the forms alternate bracket by bracket; the first round is the warm-up
        for name, kw in forms:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                run(kw)
            e.record()
            torch.cuda.synchronize()
            if rnd:
                out[name].append(s.elapsed_time(e) * 1e3 / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3, help="counted images per arm (one more is the warm-up)")
    ap.add_argument("--attn-reps", type=int, default=20, help="launches per event bracket")
    ap.add_argument("--attn-brackets", type=int, default=7, help="counted event brackets per launch form (one more is the warm-up)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pipe = LxFluxPipeline(LxFluxTransformer(synthetic_weights(FluxConfig(), dev, seed=0), dev, precise=True))
    eng = pipe.transformer.engine
    N = HW * HW
    g = torch.Generator(device=dev).manual_seed(1234)
    times = {name: [] for name, _ in ARMS}
    for rnd in range(a.images + 1):
        x = dict(lat=torch.randn(1, N, 64, device=dev, generator=g), cond=torch.randn(1, N, 64, device=dev, generator=g),
                 pe=torch.randn(1, T, 4096, device=dev, generator=g) * 0.1, pooled=torch.randn(1, 768, device=dev, generator=g))
        for name, on in ARMS:
            eng.cond_cache_enabled = on
            cond = Condition("subject", latents=x["cond"], latent_hw=(HW, HW), position_delta=[0, -HW])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = generate(None, pipe, conditions=[cond], height=16 * HW, width=16 * HW, num_inference_steps=STEPS, latents=x["lat"],
                           prompt_embeds=x["pe"], pooled_prompt_embeds=x["pooled"], output_type="latent",
                           model_config={"independent_condition": True}, default_lora=True, use_brain_condition=False).images
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            assert torch.isfinite(out).all() and eng.precise and eng.cond_cache == on and eng.cond_cached == on
            if rnd:
                times[name].append(ms)
            print(f"round {rnd} {name}: {ms:.1f} ms/image", flush=True)
    eng.check_status(sync=True)
    lines = [f"# tools/precise_cond_cache_bench.py on {torch.cuda.get_device_name(0)}: precise mode, independent_condition, batch 1, "
             f"{T} + {N} + {N} tokens, {STEPS} steps; ms per image (generate() wall time), {a.images} images per arm, arms alternating",
             f"{'arm':16s} {'median':>9s} {'min':>9s} {'max':>9s} {'images/s':>9s} {'x recompute':>12s}"]
    base = statistics.median(times["LX_COND_CACHE=0"])
    for name, _ in ARMS:
        t = times[name]
        lines.append(f"{name:16s} {statistics.median(t):9.1f} {min(t):9.1f} {max(t):9.1f} {1e3 / statistics.median(t):9.3f} {statistics.median(t) / base:12.3f}")
    lines.append(f"# attn_split_kernel alone (B = 1, H = 24, condition queries see condition keys only): us per launch, {a.attn_brackets} event "
                 f"brackets of {a.attn_reps} launches per form, forms alternating")
    lines.append(f"{'form':16s} {'median':>9s} {'min':>9s} {'max':>9s}")
    for name, us in attn_forms(dev, a.attn_reps, a.attn_brackets).items():
        lines.append(f"{name:16s} {statistics.median(us):9.1f} {min(us):9.1f} {max(us):9.1f}")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
