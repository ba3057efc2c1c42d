"""What the precise-mode VAE costs: decode and encode at the full FLUX.1 VAE shape (84 M parameters, synthetic weights), batch 1, at
512x512 and 1024x1024, for the bf16-operand VAE and the split-bf16 one, the arms alternating in one process (HIP events around each call).
The precise arm runs twice: on weights rounded to bf16 (what a FLUX.1 checkpoint holds: k_segs = 2 launches, two passes over K) and on
the fp32 weights as they are (k_segs = 3: three passes, weight images twice as wide). Every GEMM's A operand -- im2col rows for the 3x3
convolutions -- is twice as wide in both. Prints a table; `--rounds N` counted rounds per arm (default 5), `--sizes 512,1024`.

    python tools/vae_precise_bench.py > profiles/vae_precise.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from loongx_amd.vae import LxAutoencoderKL  # noqa: E402
from oracle import vae as ovae  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="512,1024")
    a = ap.parse_args()
    dev = "cuda"
    sd = ovae.init_synthetic_(ovae.AutoencoderKL(), 3).state_dict()
    sd16 = {k: v.to(torch.bfloat16).to(v.dtype) for k, v in sd.items()}
    arms = [("bf16 operands", LxAutoencoderKL(sd16, {}, dev)),
            ("precise, k_segs=2", LxAutoencoderKL(sd16, {}, dev, precise=True)),
            ("precise, k_segs=3", LxAutoencoderKL(sd, {}, dev, precise=True))]
    print(f"# tools/vae_precise_bench.py on {torch.cuda.get_device_name(0)}: full FLUX.1 VAE shape, batch 1; ms per call, {a.rounds} counted rounds per arm "
          f"after one warm-up each, arms alternating")
    print(f"{'image':>10} {'op':>7} {'arm':>18} {'median':>9} {'min':>9} {'max':>9} {'x bf16':>7}")
    g = torch.Generator(device=dev).manual_seed(1)
    for size in (int(s) for s in a.sizes.split(",")):
        img = torch.rand(1, 3, size, size, device=dev, generator=g) * 2 - 1
        z = torch.randn(1, 16, size // 8, size // 8, device=dev, generator=g)
        for op, fn in (("decode", lambda m: m.decode(z, return_dict=False)[0]), ("encode", lambda m: m.encode(img).latent_dist.mean)):
            ms = [[] for _ in arms]
            for r in range(a.rounds + 1):
                for i, (_, m) in enumerate(arms):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    fn(m)
                    e.record()
                    torch.cuda.synchronize()
                    if r:
                        ms[i].append(s.elapsed_time(e))
            base = statistics.median(ms[0])
            for (name, _), t in zip(arms, ms):
                med = statistics.median(t)
                print(f"{size:>5}x{size:<4} {op:>7} {name:>18} {med:9.2f} {min(t):9.2f} {max(t):9.2f} {med / base:7.2f}", flush=True)
    print(f"# peak memory allocated: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")


if __name__ == "__main__":
    main()
