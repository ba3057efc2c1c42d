"""What fp16 GEMM operands buy the VAE, emulated on the CPU: oracle/vae.py with rounding hooks. The input and the weight of every
convolution / linear, and the attention's q, k, v^T, probabilities and output, are rounded to the operand format (bf16 | fp16, round to
nearest even); accumulation, biases, GroupNorm and the residual stream stay fp32 -- what LxAutoencoderKL does with operands="bf16" | "fp16".
Compared against the same model in float64 on the inputs of _precise_vs_oracle (tests/test_vae_precise_gpu.py): relative error of the
latent mean and of the decoded image. Then the mid-block attention alone at C = 512 for growing token counts (fp16 probabilities fall
below the normal range as 1 / P shrinks), and the largest |operand| seen. No GPU needed.

    python tools/vae_f16_emulation.py [--attn-tokens 1024,4096] [--skip-full]
"""
import argparse
import copy
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import vae as ovae  # noqa: E402

SMALL = dict(in_channels=3, out_channels=3, latent_channels=16, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32)
FMT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def relerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


class Rounder:
    """round(t) to the operand format and back to fp32; keeps the largest magnitude it was handed."""

    def __init__(self, fmt):
        self.dtype, self.amax = FMT[fmt], 0.0

    def __call__(self, t):
        self.amax = max(self.amax, float(t.abs().max()))
        return t.to(self.dtype).to(torch.float32)


def _attn_forward(self, x):
    """AttnBlock.forward the way LxAutoencoderKL._attn computes it: v^T = Wv n^T without its bias, which joins behind P v."""
    rd = self._rd
    b, c, h, w = x.shape
    n = rd(self.group_norm(x).view(b, c, h * w).transpose(1, 2))
    q, k = rd(self.to_q(n)), rd(self.to_k(n))
    v = rd(n @ self.to_v.weight.t())
    p = rd(torch.softmax(q @ k.transpose(1, 2) / math.sqrt(c), -1))
    o = rd(p @ v + self.to_v.bias)
    return x + self.to_out[0](o).transpose(1, 2).reshape(b, c, h, w)


def emulated(ref: nn.Module, fmt: str):
    """A copy of `ref` (fp32) whose GEMM operands are rounded to `fmt`; returns (model, rounder)."""
    m, rd = copy.deepcopy(ref).float(), Rounder(fmt)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, (nn.Conv2d, nn.Linear)):
                mod.weight.copy_(rd(mod.weight))
                mod.register_forward_pre_hook(lambda _m, a: (rd(a[0]),))
            if isinstance(mod, ovae.AttnBlock):
                mod._rd = rd
                mod.forward = _attn_forward.__get__(mod)          # (n, o are rounded there; the Linear hooks round them again: idempotent)
    return m, rd


def whole_vae(label, cfg, H, W, bf16_weights=False):
    ref = ovae.init_synthetic_(ovae.AutoencoderKL(**cfg), 3)
    if bf16_weights:
        ref.load_state_dict({k: v.to(torch.bfloat16).to(v.dtype) for k, v in ref.state_dict().items()})
    nd = len(ref.config.block_out_channels) - 1
    h, w = H >> nd, W >> nd
    img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(1)) * 2 - 1
    z = torch.randn(2, 16, h, w, generator=torch.Generator().manual_seed(3))
    r64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        wmean, wimg = r64.encode(img.double()).latent_dist.mean, r64.decode(z.double()).sample
        res = {}
        for fmt in FMT:
            m, rd = emulated(ref, fmt)
            res[fmt] = (relerr(m.encode(img).latent_dist.mean, wmean), relerr(m.decode(z).sample, wimg), rd.amax)
    b, f = res["bf16"], res["fp16"]
    print(f"| {label} | {b[0]:.2e} / {b[1]:.2e} | {f[0]:.2e} / {f[1]:.2e} | {b[0] / f[0]:.1f} / {b[1] / f[1]:.1f} | {f[2]:.1f} |", flush=True)


def attention_alone(P, C=512):
    ref = ovae.init_synthetic_(ovae.AttnBlock(C), 21)
    x = torch.randn(1, C, P, 1, generator=torch.Generator().manual_seed(22)) + 0.2
    with torch.no_grad():
        x64 = x.double()
        want = copy.deepcopy(ref).double()(x64) - x64
        out = []
        for fmt in FMT:
            m, _ = emulated(ref, fmt)
            out.append(relerr(m(x) - x, want))
    print(f"| P = {P} | {out[0]:.2e} | {out[1]:.2e} | {out[0] / out[1]:.1f} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--attn-tokens", default="1024,4096,16384", help="token counts of the attention-alone rows (16384 needs about 10 GB and minutes)")
    ap.add_argument("--skip-full", action="store_true", help="leave out the full FLUX.1 shape (84 M parameters)")
    a = ap.parse_args()
    torch.manual_seed(0)
    print("| case | bf16 mean / image | fp16 mean / image | ratio | max abs operand |\n|---|---|---|---|---|")
    whole_vae("SMALL 32x32", SMALL, 32, 32)
    whole_vae("SMALL 18x14 (63 tokens, padded keys)", SMALL, 18, 14)
    whole_vae("SMALL 32x32, weights rounded to bf16", SMALL, 32, 32, bf16_weights=True)
    if not a.skip_full:
        whole_vae("full shape 64x64", {}, 64, 64)
        whole_vae("full shape 64x64, bf16 weights", {}, 64, 64, bf16_weights=True)
        whole_vae("full shape 40x56", {}, 40, 56)
    print("\nmid-block attention alone, C = 512 (out - x against float64):\n| tokens | bf16 | fp16 | ratio |\n|---|---|---|---|")
    for P in (int(t) for t in a.attn_tokens.split(",") if t):
        attention_alone(P)


if __name__ == "__main__":
    main()
