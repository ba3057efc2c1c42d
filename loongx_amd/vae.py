"""FLUX VAE (diffusers `AutoencoderKL`) on MI355X -- the step either side of the denoise loop.

Reference call sites: `vae.decode(latents / scaling_factor + shift_factor)` (src/flux/generate.py:375-380) and
`vae.encode(images).latent_dist.sample()` (src/flux/pipeline_tools.py:8-14). Same surface here: `.config`, `.encode(x)`
-> object with `.latent_dist.sample() / .mode()`, `.decode(z, return_dict=False)` -> `(image,)`, NCHW tensors in and out.

Inside, activations are NHWC: the residual stream is fp32 `[B*H*W, C]`, GEMM operands bf16. Every convolution is an implicit
GEMM on the DiT's MFMA kernel (`lx_im2col3x3` rows x `[Cout, 9 Cin]` weights, bias / fp32-residual epilogues fused), the
mid-block attention is two GEMMs around `lx_softmax_rows`, GroupNorm+SiLU is `lx_groupnorm_silu` (csrc/vae.hip). torch owns
buffers and the NCHW<->NHWC layout moves only. Any latent grid decodes and any image whose sides the encoder can halve encodes: a
token count P = h*w that is no multiple of 64 pads the attention's key axis to Ppad = roundup(P, 64) and `lx_softmax_rows_valid`
gives the pad keys probability +0 (multiples of 64 take the unpadded launches). Scratch per image: P * Ppad * 6 bytes (fp32 scores
+ bf16 probabilities). Parameter names are diffusers' (`decoder.up_blocks.0.resnets.1.conv1.weight` ...),
so `vae/diffusion_pytorch_model.safetensors` of a FLUX.1 checkpoint loads as is.

`precise=True` (what `dtype=torch.float32` selects, as for the transformer) keeps the fp32 residual stream and makes every GEMM operand a
split-bf16 pair (hi = bf16(v), lo = bf16(v - hi), lo_off columns further in the same row): `lx_groupnorm_silu_split` writes pairs,
`lx_split_bf16` replaces the bf16 casts, `lx_im2col3x3_split` gathers [hi taps | lo taps] rows, the GEMMs run with k_segs = 2 (weights
that are bf16-representable, FLUX.1's) or 3 (weights packed as [W_hi | W_lo], decided per tensor at load time) and the attention's q, k,
v^T, probabilities (`lx_softmax_rows_split`) and output are pairs too. Biases and the GroupNorm affine are fp32 in both modes. Scratch per
image in precise mode: P * Ppad * 8 bytes (fp32 scores + the bf16 probability pair).

`operands="fp16"` (what `dtype=torch.float16` selects, as for the transformer; not with `precise`) keeps the bf16 path's launches one for one
and stores every GEMM operand as IEEE fp16 instead (11 significand bits for bf16's 8): `lx_groupnorm_silu_f16`, `lx_convert_f16` and
`lx_softmax_rows_f16` write the images, `lx_im2col3x3` gathers them as 16-bit words, the GEMMs are LX_OPERANDS_F16 launches on fp16 weight
images (`.w16`, rounded from the fp32 weights). fp16 has 5 exponent bits: every producer saturates at +-65504 and counts the waves that did in
`f16_ovf`; each encode / decode reads the counter once and applies `f16_overflow` ("raise" -> F16OverflowError, "warn", or "fallback": the call
is computed again on the bf16 images, which stay resident for that). Probabilities below 2^-14 are fp16 subnormals: through 128x128 latents
(P = 16384 tokens, 1024x1024 images) they cost nothing measurable, beyond that the attention's precision degrades towards bf16's.
"""
from __future__ import annotations

import math
import warnings
from types import SimpleNamespace
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import ops
from .ops import LX_EPI_RESID_F32, LX_EPI_STORE_BF16, LX_EPI_STORE_F32

FLUX_VAE_CONFIG = dict(in_channels=3, out_channels=3, latent_channels=16, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                       norm_num_groups=32, scaling_factor=0.3611, shift_factor=0.1159)


def _pad_to(n: int, m: int) -> int:
    return (n + m - 1) // m * m


OPERANDS = ("bf16", "fp16")
F16_OVERFLOW_POLICIES = ("raise", "warn", "fallback")              # flux.generate's, restated here: that module imports this one


class _Operands16:
    """The 16-bit operand format of the non-precise VAE in one place: the dtype of the operand buffers, the three row kernels that write them,
    the weight images and the flags of the GEMM launches. bf16: today's calls, argument for argument. fp16: the saturating, counting
    producers and LX_OPERANDS_F16 launches; `ovf` is the int32 device counter they share."""

    def __init__(self, name: str, weights: Dict[str, torch.Tensor], ovf: Optional[torch.Tensor] = None):
        self.name, self.f16, self.ovf = name, name == "fp16", ovf
        self.dtype = torch.float16 if self.f16 else torch.bfloat16
        self._w = weights

    def weight(self, name: str) -> torch.Tensor:
        return self._w[name] if self.f16 else self._w[name + ".w"]

    def groupnorm_silu(self, x, gamma, beta, y, groups, eps, silu) -> None:
        if self.f16:
            ops.groupnorm_silu_f16(x, gamma, beta, y, groups, eps, silu, f16_ovf=self.ovf)
        else:
            ops.groupnorm_silu(x, gamma, beta, y, groups, eps, silu)

    def convert(self, dst, src) -> None:
        if self.f16:
            ops.convert_f16(dst, src, f16_ovf=self.ovf)
        else:
            ops.convert(dst, src)

    def softmax_rows(self, S, P, scale, n_valid=None) -> None:
        if self.f16:
            ops.softmax_rows_f16(S, P, scale, n_valid)
        else:
            ops.softmax_rows(S, P, scale, n_valid=n_valid)

    def im2col3x3(self, x, out, mode) -> None:
        """A 16-bit gather: the fp16 images go in viewed as 16-bit words."""
        ops.im2col3x3(x.view(torch.bfloat16), out.view(torch.bfloat16), mode)

    def gemm(self, A, W, C_, **kw) -> None:
        if self.f16:
            kw.update(f16=True, f16_ovf=self.ovf)
        ops.gemm([ops.gemm_desc(A, W, C_, **kw)])


class _Pair(NamedTuple):
    """A GEMM operand of the precise mode: t bf16 [M, ld] with the hi halves of the C channels at columns [0, C), the lo halves at [lo, lo + C)."""
    t: torch.Tensor
    C: int
    lo: int


class DiagonalGaussianDistribution:
    """diffusers DiagonalGaussianDistribution: mean / clamped logvar from the encoder's 2*latent channels."""

    def __init__(self, parameters: torch.Tensor):
        self.mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def sample(self, generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        if noise is None:
            noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * noise.to(self.mean.device)

    def mode(self) -> torch.Tensor:
        return self.mean


class LxAutoencoderKL:
    def __init__(self, state_dict: Dict[str, torch.Tensor], config: Optional[dict] = None, device="cuda", precise: bool = False,
                 operands: str = "bf16", f16_overflow: str = "raise"):
        if operands not in OPERANDS:
            raise ValueError(f"operands = {operands!r}: one of {OPERANDS}")
        if f16_overflow not in F16_OVERFLOW_POLICIES:
            raise ValueError(f"f16_overflow = {f16_overflow!r}: one of {F16_OVERFLOW_POLICIES}")
        if precise and operands == "fp16":
            raise ValueError('operands="fp16" with precise=True: the precise mode runs on split-bf16 pairs')
        cfg = dict(FLUX_VAE_CONFIG)
        cfg.update(config or {})
        cfg["block_out_channels"] = tuple(cfg["block_out_channels"])
        self.config = SimpleNamespace(**cfg)
        self.device = torch.device(device)
        self.dtype = torch.float32
        self.precise = bool(precise)
        self.G = cfg["norm_num_groups"]
        self.w: Dict[str, torch.Tensor] = {}
        # fp16 operands: the fp16 weight images by layer name, the counter the producers share, and what building the images found
        # (the engine's counters of the same names): weights beyond +-65504 (clipped), and the share of elements of the bf16 images that
        # fp16 cannot hold exactly (magnitudes below 2^-14).
        self.w16: Dict[str, torch.Tensor] = {}
        self.f16_ovf: Optional[torch.Tensor] = None
        self.w16_clipped, self.w16_inexact_share = 0, 0.0
        self.f16_overflow = f16_overflow
        self._sd = sd = state_dict                                               # (a reference: set_operands("fp16") rounds .w16 from the fp32 weights)
        for k, v in sd.items():
            if k.endswith(".weight") and v.dim() == 4:
                self._pack_conv(k[: -len(".weight")], v, sd.get(k[: -len("weight")] + "bias"))
            elif k.endswith(".weight") and v.dim() == 2:
                self._pack_conv(k[: -len(".weight")], v[:, :, None, None], sd.get(k[: -len("weight")] + "bias"))
            elif k.endswith(".weight") and v.dim() == 1:                        # GroupNorm affine
                self.w[k[: -len(".weight")] + ".g"] = v.detach().to(self.device, torch.float32).contiguous()
                self.w[k[: -len(".weight")] + ".b"] = sd[k[: -len("weight")] + "bias"].detach().to(self.device, torch.float32).contiguous()
        self._op = _Operands16("bf16", self.w)
        self.set_operands(operands)

    @property
    def operands(self) -> str:
        return self._op.name

    def set_operands(self, operands: str) -> None:
        """Switch a non-precise instance between bf16 and fp16 operands. The fp16 weight images are built at the first switch to fp16 and
        kept; the bf16 images always stay (the overflow fallback runs on them)."""
        if operands not in OPERANDS:
            raise ValueError(f"operands = {operands!r}: one of {OPERANDS}")
        if operands == "fp16":
            if self.precise:
                raise ValueError('operands="fp16" with precise=True: the precise mode runs on split-bf16 pairs')
            if not self.w16:
                self._pack_w16()
        self._op = _Operands16(operands, self.w16 if operands == "fp16" else self.w, self.f16_ovf if operands == "fp16" else None)

    # ---- weights -------------------------------------------------------------------------------------------------------
    def _pack_conv(self, name: str, w: torch.Tensor, b: Optional[torch.Tensor]) -> None:
        """[Cout, Cin, kh, kw] -> bf16 [Npad, Kpad] with column = (dy*kw + dx)*Cin + c (the im2col order), zero padded to the
        GEMM's granules (K % 64, N % 8). Precise mode also records `<name>.segs` and widens the image to [Npad, 2 Kpad] =
        [W_hi | W_lo] where that is 3."""
        co, ci, kh, kw = w.shape
        W = w.detach().to(self.device, torch.float32).permute(0, 2, 3, 1).reshape(co, kh * kw * ci)
        Np, Kp = _pad_to(co, 8), _pad_to(kh * kw * ci, 64)
        Wh = W.to(torch.bfloat16)
        if self.precise:
            # k_segs of the launches on this tensor: 3 with the image [W_hi | W_lo] when any element has a bf16 residual, else 2 on the
            # plain image. to_v is the A operand of v^T = Wv n^T against the pair n (k_segs = 3), so it always carries a lo half.
            Wl = (W - Wh.float()).to(torch.bfloat16)
            segs = 3 if name.endswith(".to_v") or bool((Wl != 0).any()) else 2
            self.w[name + ".segs"] = segs
        Wp = torch.zeros(Np, Kp * (2 if self.precise and segs == 3 else 1), dtype=torch.bfloat16, device=self.device)
        Wp[:co, : kh * kw * ci] = Wh
        if self.precise and segs == 3:
            Wp[:co, Kp: Kp + kh * kw * ci] = Wl
        bp = torch.zeros(Np, dtype=torch.float32, device=self.device)
        if b is not None:
            bp[:co] = b.detach().to(self.device, torch.float32)
        self.w[name + ".w"], self.w[name + ".bias"] = Wp, bp
        self.w[name + ".shape"] = (co, ci, kh)

    def _pack_w16(self) -> None:
        """The fp16 image of every GEMM weight, in the layout of its bf16 image: the fp32 weight rounded to nearest even, SATURATED to
        +-65504 (never inf) with the clipped elements counted in `w16_clipped`; `w16_inexact_share` as the engine defines it. One host
        synchronisation."""
        self.f16_ovf = torch.zeros(1, dtype=torch.int32, device=self.device)
        stat = torch.zeros(2, dtype=torch.int64, device=self.device)            # [elements of the bf16 images fp16 cannot hold, clipped]
        total = 0
        for k, v in self._sd.items():
            if not k.endswith(".weight") or v.dim() not in (2, 4):
                continue
            name = k[: -len(".weight")]
            w = v if v.dim() == 4 else v[:, :, None, None]
            co, ci, kh, kw = w.shape
            W = w.detach().to(self.device, torch.float32).permute(0, 2, 3, 1).reshape(co, kh * kw * ci)
            Wb = self.w[name + ".w"]
            img = torch.zeros(Wb.shape, dtype=torch.float16, device=self.device)
            img[:co, : kh * kw * ci] = W.clamp(-65504.0, 65504.0).to(torch.float16)
            real = Wb[:co, : kh * kw * ci]
            stat[0] += (real.float().clamp(-65504.0, 65504.0).to(torch.float16).to(torch.bfloat16) != real).sum()
            stat[1] += (W.abs() > 65504.0).sum()
            total += W.numel()
            self.w16[name] = img
        lost, clipped = (int(n) for n in stat.tolist())
        self.w16_inexact_share, self.w16_clipped = lost / max(total, 1), clipped

    # ---- building blocks (x: fp32 [B*H*W, C]) ----------------------------------------------------------------------------
    def _gn(self, x: torch.Tensor, B: int, name: str, silu: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        C = x.shape[1]
        if self.precise:
            y = torch.empty(x.shape[0], 2 * C, dtype=torch.bfloat16, device=self.device) if out is None else out
            ops.groupnorm_silu_split(x.view(B, -1, C), self.w[name + ".g"], self.w[name + ".b"], y, C, self.G, 1e-6, silu)
            return _Pair(y, C, C)
        y = torch.empty(x.shape, dtype=self._op.dtype, device=self.device) if out is None else out
        self._op.groupnorm_silu(x.view(B, -1, C), self.w[name + ".g"], self.w[name + ".b"], y.view(B, -1, C), self.G, 1e-6, silu)
        return y

    def _conv3(self, h: torch.Tensor, B: int, H: int, W: int, name: str, mode: int = 0, out: Optional[torch.Tensor] = None,
               epilogue: int = LX_EPI_STORE_F32) -> Tuple[torch.Tensor, int, int]:
        """3x3 convolution of 16-bit NHWC h [B*H*W, Cin] as im2col + GEMM; image by image so the im2col scratch stays one image
        large. out: fp32 [B*Ho*Wo, Npad] (epilogue STORE_F32 / RESID_F32 accumulates into it) or the operand format (STORE_BF16).
        Precise mode: h is a _Pair, the rows are [hi taps | lo taps] and the GEMM takes them with k_segs = 2 | 3."""
        bias = self.w[name + ".bias"]
        Wt = self.w[name + ".w"] if self.precise else self._op.weight(name)
        Ho, Wo = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
        if self.precise:
            segs = self.w[name + ".segs"]
            Np, Kp = Wt.shape[0], Wt.shape[1] // (segs - 1)
            if out is None:
                out = torch.empty(B * Ho * Wo, Np, dtype=torch.bfloat16 if epilogue == LX_EPI_STORE_BF16 else torch.float32, device=self.device)
            cols = torch.empty(Ho * Wo, 2 * Kp, dtype=torch.bfloat16, device=self.device)
            hv = h.t.view(B, H, W, h.t.shape[1])
            for b in range(B):
                ops.im2col3x3_split(hv[b:b + 1], h.C, h.lo, cols, mode)
                ops.gemm([ops.gemm_desc(cols, Wt, out[b * Ho * Wo:(b + 1) * Ho * Wo], bias=bias, epilogue=epilogue, N=Np, K=Kp, k_segs=segs, a_lo_off=Kp)])
            return out, Ho, Wo
        op = self._op
        Cin = h.shape[1]
        Np, Kp = Wt.shape
        if out is None:
            out = torch.empty(B * Ho * Wo, Np, dtype=op.dtype if epilogue == LX_EPI_STORE_BF16 else torch.float32, device=self.device)
        cols = torch.empty(Ho * Wo, Kp, dtype=op.dtype, device=self.device)
        hv = h.view(B, H, W, Cin)
        for b in range(B):
            op.im2col3x3(hv[b:b + 1], cols, mode)
            op.gemm(cols, Wt, out[b * Ho * Wo:(b + 1) * Ho * Wo], bias=bias, epilogue=epilogue)
        return out, Ho, Wo

    def _lin(self, a: torch.Tensor, name: str, out: Optional[torch.Tensor] = None, epilogue: int = LX_EPI_STORE_BF16) -> torch.Tensor:
        """Precise mode: a is a _Pair with lo = K (channel counts here are multiples of 64), and a bf16 store writes the output pair
        [M, 2 Npad] (lo half Npad columns after the hi half)."""
        bias = self.w[name + ".bias"]
        Wt = self.w[name + ".w"] if self.precise else self._op.weight(name)
        if self.precise:
            segs = self.w[name + ".segs"]
            Np, Kp = Wt.shape[0], Wt.shape[1] // (segs - 1)
            assert a.C == Kp and a.lo == Kp, (name, a.C, a.lo, Kp)
            pair_out = epilogue == LX_EPI_STORE_BF16
            if out is None:
                out = torch.empty(a.t.shape[0], 2 * Np if pair_out else Np, dtype=torch.bfloat16 if pair_out else torch.float32, device=self.device)
            ops.gemm([ops.gemm_desc(a.t, Wt, out, bias=bias, epilogue=epilogue, N=Np, K=Kp, k_segs=segs, a_lo_off=Kp, c_lo_off=Np if pair_out else 0)])
            return out
        if out is None:
            out = torch.empty(a.shape[0], Wt.shape[0], dtype=self._op.dtype if epilogue == LX_EPI_STORE_BF16 else torch.float32, device=self.device)
        self._op.gemm(a, Wt, out, bias=bias, epilogue=epilogue)
        return out

    def _operand(self, x: torch.Tensor):
        """The fp32 stream x [M, C] as a GEMM operand: bf16 | fp16 [M, C], or in precise mode the pair [M, 2 * roundup(C, 8)] (`lx_split_bf16`; a
        channel count that is no multiple of 4 -- the encoder's RGB input -- is zero-padded to one first, which is torch plumbing)."""
        M, C = x.shape
        if not self.precise:
            xb = torch.empty(x.shape, dtype=self._op.dtype, device=self.device)
            self._op.convert(xb, x)
            return xb
        if C % 4:
            x = torch.nn.functional.pad(x, (0, _pad_to(C, 4) - C))
        lo = _pad_to(C, 8)
        y = torch.empty(M, 2 * lo, dtype=torch.bfloat16, device=self.device)
        ops.split_bf16(x, y, lo)
        return _Pair(y, C, lo)

    def _resnet(self, x: torch.Tensor, B: int, H: int, W: int, p: str) -> torch.Tensor:
        h = self._gn(x, B, p + ".norm1")
        h1, _, _ = self._conv3(h, B, H, W, p + ".conv1")
        t = self._gn(h1, B, p + ".norm2")
        if (p + ".conv_shortcut.w") in self.w:
            x = self._lin(self._operand(x), p + ".conv_shortcut", epilogue=LX_EPI_STORE_F32)
        self._conv3(t, B, H, W, p + ".conv2", out=x, epilogue=LX_EPI_RESID_F32)          # x += conv2(t)
        return x

    def _attn(self, x: torch.Tensor, B: int, P: int, p: str) -> torch.Tensor:
        """Single-head attention over the P = H*W tokens of each image (diffusers Attention, residual_connection=True)."""
        if self.precise:
            return self._attn_precise(x, B, P, p)
        if P % 64:
            return self._attn_ragged(x, B, P, p)
        C, op = x.shape[1], self._op
        n = self._gn(x, B, p + ".group_norm", silu=False)
        q, k = self._lin(n, p + ".to_q"), self._lin(n, p + ".to_k")
        Wv, bv = op.weight(p + ".to_v"), self.w[p + ".to_v.bias"]
        S = torch.empty(P, P, dtype=torch.float32, device=self.device)
        Pm = torch.empty(P, P, dtype=op.dtype, device=self.device)
        vT = torch.empty(C, P, dtype=op.dtype, device=self.device)
        o = torch.empty(B * P, C, dtype=op.dtype, device=self.device)
        for b in range(B):
            r = slice(b * P, (b + 1) * P)
            op.gemm(q[r], k[r], S, epilogue=LX_EPI_STORE_F32)                                         # S = q k^T
            op.softmax_rows(S, Pm, 1.0 / math.sqrt(C))
            op.gemm(Wv, n[r], vT, epilogue=LX_EPI_STORE_BF16)                                         # v^T = Wv n^T (bias added below)
            op.gemm(Pm, vT, o[r], bias=bv, epilogue=LX_EPI_STORE_BF16)                                # rows of P sum to 1: P (v + 1 bv^T) = P v + bv
        self._lin(o, p + ".to_out.0", out=x, epilogue=LX_EPI_RESID_F32)
        return x

    def _attn_ragged(self, x: torch.Tensor, B: int, P: int, p: str) -> torch.Tensor:
        """_attn for a token count that is no multiple of 64 (the GEMM's K granule; its N granule is 8): the key axis is padded to
        Ppad = roundup(P, 64). The images lie back to back in n and k ([B*P, C]), so the Ppad key rows of image b run into image b+1's
        rows and, for the last image, into a zero tail that both buffers carry: every row a GEMM reads lies inside its allocation and
        is finite (real rows of a neighbour, or zeros). Columns [P, Ppad) of S and of v^T are therefore finite garbage; the softmax
        reads none of the former and writes exact zeros for those keys, so the latter contribute nothing to P v."""
        C, op = x.shape[1], self._op
        Pp = _pad_to(P, 64)
        rows = (B - 1) * P + Pp                                                                       # the last image's Ppad rows end here
        n = torch.zeros(rows, C, dtype=op.dtype, device=self.device)
        k = torch.zeros(rows, C, dtype=op.dtype, device=self.device)
        self._gn(x, B, p + ".group_norm", silu=False, out=n[: B * P])
        q = self._lin(n[: B * P], p + ".to_q")
        self._lin(n[: B * P], p + ".to_k", out=k[: B * P])
        Wv, bv = op.weight(p + ".to_v"), self.w[p + ".to_v.bias"]
        S = torch.empty(P, Pp, dtype=torch.float32, device=self.device)
        Pm = torch.empty(P, Pp, dtype=op.dtype, device=self.device)
        vT = torch.empty(C, Pp, dtype=op.dtype, device=self.device)
        o = torch.empty(B * P, C, dtype=op.dtype, device=self.device)
        for b in range(B):
            r, rp = slice(b * P, (b + 1) * P), slice(b * P, b * P + Pp)
            op.gemm(q[r], k[rp], S, epilogue=LX_EPI_STORE_F32)                                        # S[:, :P] = q k^T
            op.softmax_rows(S, Pm, 1.0 / math.sqrt(C), n_valid=P)                                     # Pm[:, P:] = +0
            op.gemm(Wv, n[rp], vT, epilogue=LX_EPI_STORE_BF16)                                        # v^T[:, :P] = Wv n^T
            op.gemm(Pm, vT, o[r], bias=bv, epilogue=LX_EPI_STORE_BF16)
        self._lin(o, p + ".to_out.0", out=x, epilogue=LX_EPI_RESID_F32)
        return x

    def _attn_precise(self, x: torch.Tensor, B: int, P: int, p: str) -> torch.Tensor:
        """_attn on pairs, one path for every token count: the key axis is padded to Ppad = roundup(P, 64) as in _attn_ragged (zero-tailed n
        and k, both halves; Ppad == P when P is a multiple of 64). q, k, v^T, the probabilities and the attention output are pair images and
        all three products are k_segs = 3 launches (hi hi + lo hi + hi lo); to_out accumulates into the fp32 stream."""
        C = x.shape[1]
        Pp = _pad_to(P, 64)
        rows = (B - 1) * P + Pp
        n = torch.zeros(rows, 2 * C, dtype=torch.bfloat16, device=self.device)
        k = torch.zeros(rows, 2 * C, dtype=torch.bfloat16, device=self.device)
        self._gn(x, B, p + ".group_norm", silu=False, out=n[: B * P])
        np_ = _Pair(n[: B * P], C, C)
        q = self._lin(np_, p + ".to_q")
        self._lin(np_, p + ".to_k", out=k[: B * P])
        Wv, bv = self.w[p + ".to_v.w"], self.w[p + ".to_v.bias"]                                      # [C, 2C] = [Wv_hi | Wv_lo]
        assert Wv.shape == (C, 2 * C), (Wv.shape, C)
        S = torch.empty(P, Pp, dtype=torch.float32, device=self.device)
        Pm = torch.empty(P, 2 * Pp, dtype=torch.bfloat16, device=self.device)
        vT = torch.empty(C, 2 * Pp, dtype=torch.bfloat16, device=self.device)
        o = torch.empty(B * P, 2 * C, dtype=torch.bfloat16, device=self.device)
        for b in range(B):
            r, rp = slice(b * P, (b + 1) * P), slice(b * P, b * P + Pp)
            ops.gemm([ops.gemm_desc(q[r], k[rp], S, epilogue=LX_EPI_STORE_F32, N=Pp, K=C, k_segs=3, a_lo_off=C)])             # S[:, :P] = q k^T
            ops.softmax_rows_split(S, Pm, 1.0 / math.sqrt(C), P, Pp, Pp)                                                     # Pm[:, P:Pp] = +0, both halves
            ops.gemm([ops.gemm_desc(Wv, n[rp], vT, epilogue=LX_EPI_STORE_BF16, N=Pp, K=C, k_segs=3, a_lo_off=C, c_lo_off=Pp)])  # v^T[:, :P] = Wv n^T
            ops.gemm([ops.gemm_desc(Pm, vT, o[r], bias=bv, epilogue=LX_EPI_STORE_BF16, N=C, K=Pp, k_segs=3, a_lo_off=Pp, c_lo_off=C)])
        self._lin(_Pair(o, C, C), p + ".to_out.0", out=x, epilogue=LX_EPI_RESID_F32)
        return x

    def _mid(self, x, B, H, W, p):
        x = self._resnet(x, B, H, W, p + ".resnets.0")
        x = self._attn(x, B, H * W, p + ".attentions.0")
        return self._resnet(x, B, H, W, p + ".resnets.1")

    def _nhwc_bf16(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(self.device, torch.float32).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)

    def _input(self, t: torch.Tensor):
        """NCHW input -> the operand of conv_in: NHWC rows [B*H*W, C], bf16, fp16 (saturated and counted) or (precise mode) the pair of
        the fp32 values."""
        if self.precise or self._op.f16:
            return self._operand(t.to(self.device, torch.float32).permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous())
        return self._nhwc_bf16(t).view(-1, t.shape[1])

    def _checked(self, run, what: str):
        """run() under the fp16 overflow contract (a plain call in the other modes): the counter is zeroed, and read once when the call
        has been enqueued -- 4 bytes; the caller reads the result anyway."""
        if not self._op.f16:
            return run()
        policy = self.f16_overflow
        if policy not in F16_OVERFLOW_POLICIES:
            raise ValueError(f"f16_overflow = {policy!r}: one of {F16_OVERFLOW_POLICIES}")
        self.f16_ovf.zero_()
        out = run()
        n_sat = int(self.f16_ovf.item())
        if not n_sat and not self.w16_clipped:
            return out
        from .flux.generate import F16OverflowError
        msg = (f"VAE {what} on fp16 operands: {n_sat} producer wave(s) clipped an operand to +-65504, {self.w16_clipped} weight(s) were "
               f"clipped building the fp16 images")
        if policy == "raise":
            raise F16OverflowError(msg + '; f16_overflow="fallback" recomputes such calls with bf16 operands, "warn" keeps them')
        if policy == "warn":
            warnings.warn(msg + "; the result was kept", RuntimeWarning, stacklevel=3)
            return out
        warnings.warn(msg + f"; recomputing this {what} with bf16 operands", RuntimeWarning, stacklevel=3)
        f16, self._op = self._op, _Operands16("bf16", self.w)
        try:
            return run()
        finally:
            self._op = f16

    # ---- public surface -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = True, generator=None):
        """z [B, latent, h, w] (any h, w >= 1) -> image [B, 3, 8h, 8w] fp32."""
        img = self._checked(lambda: self._decode(z), "decode")
        return SimpleNamespace(sample=img) if return_dict else (img,)

    def _decode(self, z: torch.Tensor) -> torch.Tensor:
        cfg = self.config
        B, _, H, W = z.shape
        x, _, _ = self._conv3(self._input(z), B, H, W, "decoder.conv_in")
        x = self._mid(x, B, H, W, "decoder.mid_block")
        rev = list(reversed(cfg.block_out_channels))
        for i in range(len(rev)):
            for j in range(cfg.layers_per_block + 1):
                x = self._resnet(x, B, H, W, f"decoder.up_blocks.{i}.resnets.{j}")
            if i < len(rev) - 1:
                x, H, W = self._conv3(self._operand(x), B, H, W, f"decoder.up_blocks.{i}.upsamplers.0.conv", mode=2)
        h = self._gn(x, B, "decoder.conv_norm_out")
        y, _, _ = self._conv3(h, B, H, W, "decoder.conv_out")
        return y[:, : cfg.out_channels].reshape(B, H, W, cfg.out_channels).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def encode(self, images: torch.Tensor, return_dict: bool = True):
        """images [B, 3, H, W] in [-1, 1] -> latent_dist over [B, latent, H/8, W/8]."""
        cfg = self.config
        B, _, H, W = images.shape
        nd = len(cfg.block_out_channels) - 1
        if H % (1 << nd) or W % (1 << nd):
            raise ValueError(f"image {H}x{W}: sides must be multiples of {1 << nd} (the encoder halves them {nd} times)")
        d = DiagonalGaussianDistribution(self._checked(lambda: self._encode(images), "encode"))
        return SimpleNamespace(latent_dist=d) if return_dict else (d,)

    def _encode(self, images: torch.Tensor) -> torch.Tensor:
        cfg = self.config
        B, _, H, W = images.shape
        nd = len(cfg.block_out_channels) - 1
        x, _, _ = self._conv3(self._input(images), B, H, W, "encoder.conv_in")
        for i in range(len(cfg.block_out_channels)):
            for j in range(cfg.layers_per_block):
                x = self._resnet(x, B, H, W, f"encoder.down_blocks.{i}.resnets.{j}")
            if i < nd:
                x, H, W = self._conv3(self._operand(x), B, H, W, f"encoder.down_blocks.{i}.downsamplers.0.conv", mode=1)
        x = self._mid(x, B, H, W, "encoder.mid_block")
        h = self._gn(x, B, "encoder.conv_norm_out")
        y, _, _ = self._conv3(h, B, H, W, "encoder.conv_out")
        return y[:, : 2 * cfg.latent_channels].reshape(B, H, W, 2 * cfg.latent_channels).permute(0, 3, 1, 2).contiguous()

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def requires_grad_(self, *a, **k):
        return self


class VaeImageProcessor:
    """diffusers VaeImageProcessor(vae_scale_factor=16) as FluxPipeline 0.31.0 constructs it: PIL / array / tensor -> [B,3,H,W] in
    [-1, 1] with both sides floored to a multiple of the scale factor; and back (denormalise, clamp, PIL)."""

    def __init__(self, vae_scale_factor: int = 16, do_resize: bool = True, do_normalize: bool = True):
        self.vae_scale_factor, self.do_resize, self.do_normalize = vae_scale_factor, do_resize, do_normalize

    def preprocess(self, image, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
        import numpy as np
        if isinstance(image, torch.Tensor):
            x = image if image.dim() == 4 else image[None]
            x = x.float()
        else:
            imgs = image if isinstance(image, (list, tuple)) else [image]
            arrs = []
            for im in imgs:
                if hasattr(im, "convert"):                  # PIL
                    w, h = im.size
                    if self.do_resize:
                        w2 = (width or w) // self.vae_scale_factor * self.vae_scale_factor
                        h2 = (height or h) // self.vae_scale_factor * self.vae_scale_factor
                        if (w2, h2) != (w, h):
                            from PIL import Image
                            im = im.resize((w2, h2), resample=Image.LANCZOS)
                    arrs.append(np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0)
                else:
                    arrs.append(np.asarray(im, dtype=np.float32))
            x = torch.from_numpy(np.stack(arrs)).permute(0, 3, 1, 2).contiguous()
        if self.do_normalize:
            x = 2.0 * x - 1.0
        return x

    def postprocess(self, image: torch.Tensor, output_type: str = "pil"):
        if output_type == "latent":
            return image
        x = (image.float() / 2 + 0.5).clamp(0, 1) if self.do_normalize else image.float()
        if output_type == "pt":
            return x
        arr = x.cpu().permute(0, 2, 3, 1).numpy()
        if output_type == "np":
            return arr
        from PIL import Image
        return [Image.fromarray((a * 255).round().astype("uint8")) for a in arr]
