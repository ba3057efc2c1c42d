"""images/s with model_config independent_condition in the two modes whose step-invariant condition stream was recomputed every step before
the per-layer e4m3 images (KC8 / VTC8) and lx_qkv_prep_kv_segs existed; full depth (19 + 38 blocks), synthetic weights, 28 steps:
  (a) attn_fp8, batch 4, 512 text + 4096 image + 4096 condition tokens (1024 x 1024: BASELINE configs[4]'s shape);
  (b) bf16 operands, batch 1, 512 + 1350 + 1350 tokens (720 x 480: no stream a multiple of 32, so no fused projection epilogue).
Not part of bench.py.

  python tools/cond_cache_modes_bench.py [--case a|b|both] [--images 3] [--parent DIR] [--out profiles/cond_cache_modes.txt]

Two arms, each a worker process of its own that imports the package from its own tree, alternating image by image on the same GPU (the
driver hands out one image at a time; the other worker idles meanwhile):
  this tree   -- the condition cache on (the default);
  --parent DIR: a checkout of the parent commit with its library built (`git worktree add DIR HEAD~1 && bash DIR/loongx_amd/csrc/build.sh`);
  without --parent the second arm is this tree under LX_COND_CACHE=0, which in these two modes launches what the parent commit launches.
The first round is the warm-up (code objects, graph captures) and is not counted. Per arm: ms per generate() call (host clock, device
synchronised before and after; one call = one batch), median / minimum / maximum over the counted rounds, images/s = batch / median, and
the package power and shader clock over the arm's counted calls (bench.PowerSampler: amdgpu hwmon, every 50 ms). The last round's
latents of the two arms are compared (relative L2): the arms compute the same images up to the rounding of launches of another extent."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, STEPS = 512, 28
CASES = {"a": dict(B=4, h=64, w=64, mc={"attn_fp8": True}, what="attn_fp8, batch 4, 512 + 4096 + 4096 tokens"),
         "b": dict(B=1, h=30, w=45, mc={}, what="bf16 operands, batch 1, 512 + 1350 + 1350 tokens")}


def worker(a) -> None:
    """One arm: builds the pipeline from the package under --tree, then one generate() per line read from stdin ("go <round>" -> one JSON
    line on stdout; "save <path>": the last latents; anything else ends it). Inputs are seeded by the round, so both arms edit the same images."""
    sys.path.insert(0, a.tree)
    import torch
    from bench import PowerSampler
    from loongx_amd.flux.condition import Condition
    from loongx_amd.flux.generate import generate
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig, synthetic_weights
    import loongx_amd
    assert os.path.realpath(os.path.dirname(os.path.dirname(loongx_amd.__file__))) == os.path.realpath(a.tree), loongx_amd.__file__
    c = CASES[a.case]
    B, h, w = c["B"], c["h"], c["w"]
    N = h * w
    dev = torch.device("cuda:0")
    pipe = LxFluxPipeline(LxFluxTransformer(synthetic_weights(FluxConfig(), dev, seed=0), dev))
    eng = pipe.transformer.engine
    mc = dict(c["mc"], independent_condition=True)
    out = None
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if cmd and cmd[0] == "save":
            torch.save(out.float().cpu(), cmd[1])
            print("saved", flush=True)
            continue
        if not cmd or cmd[0] != "go":
            break
        g = torch.Generator(device=dev).manual_seed(1234 + int(cmd[1]))
        x = dict(lat=torch.randn(B, N, 64, device=dev, generator=g), cond=torch.randn(B, N, 64, device=dev, generator=g),
                 pe=torch.randn(B, T, 4096, device=dev, generator=g) * 0.1, pooled=torch.randn(B, 768, device=dev, generator=g))
        cond = Condition("subject", latents=x["cond"], latent_hw=(h, w), position_delta=[0, -w])
        power = PowerSampler(dev.index)
        torch.cuda.synchronize()
        power.start()
        t0 = time.perf_counter()
        out = generate(None, pipe, conditions=[cond], height=16 * h, width=16 * w, num_inference_steps=STEPS, latents=x["lat"],
                       prompt_embeds=x["pe"], pooled_prompt_embeds=x["pooled"], output_type="latent", model_config=mc, default_lora=True,
                       use_brain_condition=False).images
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        pw = power.stop() or {}
        eng.check_status(sync=True)
        assert bool(torch.isfinite(out).all())
        print(json.dumps(dict(ms=ms, W=pw.get("avg_W"), sclk=pw.get("sclk_MHz_avg"), cond_cache=bool(eng.cond_cache), fused=bool(eng.qkv_fused),
                              images=sorted(n for n in ("KC", "KC2", "KC8") if getattr(eng, n, None) is not None))), flush=True)


class Arm:
    def __init__(self, name, tree, case, env):
        self.name, self.recs = name, []
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--case", case, "--tree", tree], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, env=dict(os.environ, **env))
        self.ask(None)

    def ask(self, cmd):
        if cmd is not None:
            self.p.stdin.write(cmd + "\n")
            self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"arm '{self.name}' ended with status {self.p.wait()}")
        return line.strip()

    def close(self):
        self.p.stdin.close()
        self.p.wait()


def mean(v):
    v = [x for x in v if x is not None]
    return f"{sum(v) / len(v):.0f}" if v else "n/a"


def run_case(case, a, lines) -> None:
    import torch
    c = CASES[case]
    arms = [Arm("this tree", HERE, case, {"LX_COND_CACHE": "1"}),
            Arm("parent commit", os.path.abspath(a.parent), case, {}) if a.parent else Arm("LX_COND_CACHE=0", HERE, case, {"LX_COND_CACHE": "0"})]
    try:
        for rnd in range(a.images + 1):
            for arm in arms:
                r = json.loads(arm.ask(f"go {rnd}"))
                print(f"case ({case}) round {rnd} {arm.name}: {r}", flush=True)
                if rnd:
                    arm.recs.append(r)
        with tempfile.TemporaryDirectory() as d:
            outs = []
            for i, arm in enumerate(arms):
                arm.ask(f"save {d}/{i}.pt")
                outs.append(torch.load(f"{d}/{i}.pt").double())
        diff = float((outs[0] - outs[1]).norm() / outs[1].norm())
    finally:
        for arm in arms:
            arm.close()
    assert arms[0].recs[-1]["cond_cache"] and not arms[1].recs[-1]["cond_cache"], "the arms are not cache on / cache off"
    base = statistics.median(r["ms"] for r in arms[1].recs)
    lines.append(f"# case ({case}): independent_condition, {c['what']}, {STEPS} steps; ms per generate() call of {c['B']} image(s), {a.images} counted "
                 f"rounds per arm, arms alternating; the removed work is C / (T + N + C) = {c['h'] * c['w'] / (T + 2 * c['h'] * c['w']):.0%} of the GEMM rows of a cached step")
    lines.append(f"{'arm':16s} {'cache':>8s} {'median':>9s} {'min':>9s} {'max':>9s} {'images/s':>9s} {'x arm 2':>8s} {'avg W':>7s} {'sclk MHz':>9s}")
    for arm in arms:
        ms = [r["ms"] for r in arm.recs]
        med = statistics.median(ms)
        images = "+".join(arm.recs[-1]["images"]) or "off"
        lines.append(f"{arm.name:16s} {images:>8s} {med:9.1f} {min(ms):9.1f} {max(ms):9.1f} {c['B'] * 1e3 / med:9.3f} {med / base:8.3f} "
                     f"{mean([r['W'] for r in arm.recs]):>7s} {mean([r['sclk'] for r in arm.recs]):>9s}")
    lines.append(f"# last round's latents, arm 1 against arm 2: relative L2 difference {diff:.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="both", choices=["a", "b", "both"])
    ap.add_argument("--images", type=int, default=3, help="counted rounds per arm (one more is the warm-up)")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: the second arm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/cond_cache_modes_bench.py measures on the GPU: none found")
    lines = [f"# tools/cond_cache_modes_bench.py on {torch.cuda.get_device_name(0)}; second arm: "
             + ("the parent commit's tree" if a.parent else "this tree under LX_COND_CACHE=0 (the parent commit's launches in these modes)")]
    for case in ("a", "b") if a.case == "both" else (a.case,):
        run_case(case, a, lines)
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
