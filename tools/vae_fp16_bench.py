"""What the fp16-operand VAE costs and buys: decode and encode at the full FLUX.1 VAE shape (84 M parameters, synthetic weights rounded to
bf16: what a FLUX.1 checkpoint holds), batch 1, at 512x512 and 1024x1024, for the bf16-operand VAE and the fp16-operand one, the arms
alternating in one process (HIP events around each call; the fp16 arm's time includes its read of the overflow counter). The launch
count, the bytes moved and the MFMA rate are the same in both arms, so parity is the expectation. Then the error of both arms against the
fp32 oracle at 64x64, and sha256 of the bf16 arm's decode / encode outputs on fixed inputs.

The bf16 arm is meant to be the code as it was before the fp16 path existed. `--hash-only --tree DIR` prints the same digests from another
checkout (built; only its LxAutoencoderKL(state_dict, config, device) is used), `--parent-hashes FILE` compares them with this tree's:

    python tools/vae_fp16_bench.py --hash-only --tree ../parent > parent_hashes.txt
    python tools/vae_fp16_bench.py --parent-hashes parent_hashes.txt > profiles/vae_fp16.txt
"""
import argparse
import hashlib
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digests(LxAutoencoderKL, sd16, dev, torch):
    """sha256 of the bf16-operand VAE's outputs: decode of a 64x64 and a 9x7 latent (the padded key axis), encode of 512x512 and 72x56."""
    m = LxAutoencoderKL(sd16, {}, dev)
    g = torch.Generator().manual_seed(5)
    out = []
    for h, w in ((64, 64), (9, 7)):
        z = torch.randn(1, 16, h, w, generator=g).to(dev)
        img = (torch.rand(1, 3, 8 * h, 8 * w, generator=g) * 2 - 1).to(dev)
        out.append((f"decode {h}x{w} latent", m.decode(z, return_dict=False)[0]))
        out.append((f"encode {8 * h}x{8 * w} image", m.encode(img).latent_dist.mean))
    torch.cuda.synchronize()
    return [(n, hashlib.sha256(t.float().cpu().contiguous().numpy().tobytes()).hexdigest()) for n, t in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tree", default=HERE, help="root of the checkout whose loongx_amd is imported (default: this one)")
    ap.add_argument("--hash-only", action="store_true", help="print the bf16 arm's output digests and stop")
    ap.add_argument("--parent-hashes", default=None, help="output of --hash-only from the parent commit's tree, to compare with")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from loongx_amd.vae import LxAutoencoderKL
    from oracle import vae as ovae
    dev = "cuda"
    ref = ovae.init_synthetic_(ovae.AutoencoderKL(), 3)
    ref.load_state_dict({k: v.to(torch.bfloat16).to(v.dtype) for k, v in ref.state_dict().items()})
    sd16 = ref.state_dict()
    mine = digests(LxAutoencoderKL, sd16, dev, torch)
    if a.hash_only:
        for n, h in mine:
            print(f"{h}  {n}")
        return
    arms = [("bf16 operands", LxAutoencoderKL(sd16, {}, dev)), ("fp16 operands", LxAutoencoderKL(sd16, {}, dev, operands="fp16"))]
    print(f"# tools/vae_fp16_bench.py on {torch.cuda.get_device_name(0)}: full FLUX.1 VAE shape, bf16-representable weights, batch 1; ms per call, "
          f"{a.rounds} counted rounds per arm after one warm-up each, arms alternating")
    print(f"# fp16 weight images: w16_clipped {arms[1][1].w16_clipped}, w16_inexact_share {arms[1][1].w16_inexact_share:.3e}")
    print(f"{'image':>10} {'op':>7} {'arm':>14} {'median':>9} {'min':>9} {'max':>9} {'x bf16':>7}")
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
                print(f"{size:>5}x{size:<4} {op:>7} {name:>14} {med:9.2f} {min(t):9.2f} {max(t):9.2f} {med / base:7.2f}", flush=True)
    print(f"# peak memory allocated: {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")

    # error against the fp32 oracle at 64x64 (the inputs of tests/test_vae_precise_gpu.py's _precise_vs_oracle)
    def relerr(x, y):
        return float((x.double().cpu() - y.double()).norm() / y.double().norm())
    img = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)) * 2 - 1
    z = torch.randn(2, 16, 8, 8, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        wmean, wimg = ref.encode(img).latent_dist.mean, ref.decode(z, return_dict=False)[0]
    print("# relative error against the fp32 oracle at 64x64 (latent mean / decoded image)")
    for name, m in arms:
        print(f"{name:>14}  mean {relerr(m.encode(img.to(dev)).latent_dist.mean, wmean):.3e}  image {relerr(m.decode(z.to(dev), return_dict=False)[0], wimg):.3e}")
    print(f"# overflow counter of the fp16 arm after the last call: {int(arms[1][1].f16_ovf.item())}")
    print("# sha256 of the bf16 arm's outputs on fixed inputs" + (", against the parent commit's tree on the same inputs" if a.parent_hashes else ""))
    parent = {}
    if a.parent_hashes:
        for line in open(a.parent_hashes):
            if line.strip() and not line.startswith("#"):
                h, n = line.strip().split("  ", 1)
                parent[n] = h
    for n, h in mine:
        same = "" if not parent else ("  bit-equal with the parent" if parent.get(n) == h else f"  DIFFERS from the parent ({parent.get(n)})")
        print(f"{h[:16]}  {n}{same}")


if __name__ == "__main__":
    main()
