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

The layers (`_gn`, `_conv3`, `_lin`, `_operand`, `_input`, `_attn`) exist once, written against operand handles (`_Operand`: tensor,
channel count, lo offset) and the instance's operand policy `_op`, which owns what differs by format: buffers, the row kernels that
fill them, the weight images and their packing, and the GEMM descriptor. Three formats, two policy classes:

bf16 (`_Operands16`, the default): the launches named above.

`operands="fp16"` (`_Operands16` too; what `dtype=torch.float16` selects, as for the transformer; not with `precise`) keeps the bf16 path's
launches one for one and stores every GEMM operand as IEEE fp16 instead (11 significand bits for bf16's 8): `lx_groupnorm_silu_f16`,
`lx_convert_f16` and `lx_softmax_rows_f16` write the images, `lx_im2col3x3` gathers them as 16-bit words, the GEMMs are LX_OPERANDS_F16
launches on fp16 weight images (`.w16`, rounded from the fp32 weights). fp16 has 5 exponent bits: every producer saturates at +-65504 and
counts the waves that did in `f16_ovf`; each encode / decode reads the counter once and applies `f16_overflow` ("raise" -> F16OverflowError,
"warn", or "fallback": the call is computed again on the bf16 images, which stay resident for that). Probabilities below 2^-14 are fp16
subnormals: through 128x128 latents (P = 16384 tokens, 1024x1024 images) they cost nothing measurable, beyond that the attention's
precision degrades towards bf16's.

`precise=True` (`_OperandsSplit`; what `dtype=torch.float32` selects, as for the transformer) makes every GEMM operand a split-bf16 pair
(hi = bf16(v), lo = bf16(v - hi), lo columns further in the same row): `lx_groupnorm_silu_split` writes pairs, `lx_split_bf16` replaces
the casts, `lx_im2col3x3_split` gathers [hi taps | lo taps] rows, the GEMMs run with k_segs = 2 (weights that are bf16-representable,
FLUX.1's) or 3 (weights packed as [W_hi | W_lo], decided per tensor at load time) and the attention's q, k, v^T, probabilities
(`lx_softmax_rows_split`) and output are pairs too. Scratch per image: P * Ppad * 8 bytes (fp32 scores + the bf16 probability pair).

The residual stream, the biases and the GroupNorm affine are fp32 in every format.
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


class _Operand(NamedTuple):
    """A GEMM operand: t [M, ld] holds the C channels at columns [0, C) -- bf16 or fp16 values with lo = 0, or the hi halves of a split-bf16
    pair whose lo halves lie at [lo, lo + C) of the same row."""
    t: torch.Tensor
    C: int
    lo: int

    def rows(self, r: slice) -> "_Operand":
        return _Operand(self.t[r], self.C, self.lo)


def _im2col_weight(w: torch.Tensor, device) -> torch.Tensor:
    """[Cout, Cin, kh, kw] (a Linear's [Cout, Cin] is a 1x1) -> fp32 [Npad, Kpad] with column = (dy*kw + dx)*Cin + c (the im2col order), zero
    padded to the GEMM's granules (N % 8, K % 64). Every weight image is an elementwise rounding of this one, so its pads are +0 too."""
    if w.dim() == 2:
        w = w[:, :, None, None]
    co, ci, kh, kw = w.shape
    W = torch.zeros(_pad_to(co, 8), _pad_to(kh * kw * ci, 64), dtype=torch.float32, device=device)
    W[:co, : kh * kw * ci] = w.detach().to(device, torch.float32).permute(0, 2, 3, 1).reshape(co, kh * kw * ci)
    return W


class _Operands:
    """What the layers ask of an operand format. `weights` is the instance's `.w` (or `.w16`), shared, not copied."""
    name, f16, dtype = "bf16", False, torch.bfloat16

    def __init__(self, weights: Dict[str, torch.Tensor], device):
        self._w, self.device = weights, device

    def out(self, M: int, Np: int, epilogue: int):
        """The output of a GEMM: the fp32 stream [M, Np] (STORE_F32 / RESID_F32) or an operand (STORE_BF16)."""
        return self.operand(M, Np) if epilogue == LX_EPI_STORE_BF16 else torch.empty(M, Np, dtype=torch.float32, device=self.device)

    def input(self, t: torch.Tensor) -> _Operand:
        """NCHW input -> the operand of conv_in: NHWC rows [B*H*W, C]."""
        return self.from_stream(t.to(self.device, torch.float32).permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous())

    def gemm(self, A: _Operand, W: _Operand, out, *, N: int, K: int, bias=None, epilogue: int) -> None:
        """out (+)= A W^T (+ bias). W: a weight image (`weight(name)`) or another operand as the [N, K] matrix; out as `out()` gives it."""
        C_, c_lo = (out.t, out.lo) if isinstance(out, _Operand) else (out, 0)
        ops.gemm([ops.gemm_desc(A.t, W.t, C_, bias=bias, epilogue=epilogue, N=N, K=K, a_lo_off=A.lo, c_lo_off=c_lo, **self._gemm_kw(W))])


class _Operands16(_Operands):
    """bf16 and fp16: operands are [rows, C] in `dtype`. bf16: `lx_groupnorm_silu`, `lx_convert`, `lx_softmax_rows` / `_valid` on the `.w`
    images. fp16: the saturating, counting producers and LX_OPERANDS_F16 launches on the `.w16` images; `ovf` is the int32 device counter
    they share."""

    def __init__(self, name: str, weights: Dict[str, torch.Tensor], device, ovf: Optional[torch.Tensor] = None):
        super().__init__(weights, device)
        self.name, self.f16, self.ovf = name, name == "fp16", ovf
        self.dtype = torch.float16 if self.f16 else torch.bfloat16

    def operand(self, rows: int, C: int, zero: bool = False) -> _Operand:
        return _Operand((torch.zeros if zero else torch.empty)(rows, C, dtype=self.dtype, device=self.device), C, 0)

    def pack(self, name: str, W: torch.Tensor) -> torch.Tensor:
        return W.to(torch.bfloat16)

    def weight(self, name: str) -> _Operand:
        t = self._w[name] if self.f16 else self._w[name + ".w"]
        return _Operand(t, t.shape[1], 0)

    def _gemm_kw(self, W: _Operand) -> dict:
        return dict(f16=True, f16_ovf=self.ovf) if self.f16 else {}

    def groupnorm_silu(self, x, gamma, beta, y: _Operand, groups, eps, silu) -> None:
        if self.f16:
            ops.groupnorm_silu_f16(x, gamma, beta, y.t.view(x.shape), groups, eps, silu, f16_ovf=self.ovf)
        else:
            ops.groupnorm_silu(x, gamma, beta, y.t.view(x.shape), groups, eps, silu)

    def from_stream(self, x: torch.Tensor) -> _Operand:
        y = self.operand(*x.shape)
        if self.f16:
            ops.convert_f16(y.t, x, f16_ovf=self.ovf)
        else:
            ops.convert(y.t, x)
        return y

    def input(self, t: torch.Tensor) -> _Operand:
        if self.f16:                                                            # (saturated and counted)
            return super().input(t)
        C = t.shape[1]                                                          # bf16: a torch cast
        return _Operand(t.to(self.device, torch.float32).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).view(-1, C), C, 0)

    def im2col3x3(self, x: torch.Tensor, h: _Operand, cols: _Operand, mode: int) -> None:
        """A 16-bit gather: the fp16 images go in viewed as 16-bit words."""
        ops.im2col3x3(x.view(torch.bfloat16), cols.t.view(torch.bfloat16), mode)

    def softmax_rows(self, S, Pm: _Operand, scale, P: int, Ppad: int) -> None:
        n_valid = None if Ppad == P else P                                      # (bf16: lx_softmax_rows | lx_softmax_rows_valid)
        if self.f16:
            ops.softmax_rows_f16(S, Pm.t, scale, n_valid)
        else:
            ops.softmax_rows(S, Pm.t, scale, n_valid=n_valid)


class _OperandsSplit(_Operands):
    """precise: operands are bf16 pairs [rows, 2 lo] = [hi | lo] with lo = roundup(C, 8); a bf16 store writes a pair as well. A GEMM is a
    k_segs = 3 launch (hi hi + lo hi + hi lo) where W carries a lo half -- the weights packed as [W_hi | W_lo], and the attention's three
    products -- and a k_segs = 2 launch on a weight that is bf16-representable."""

    def operand(self, rows: int, C: int, zero: bool = False) -> _Operand:
        lo = _pad_to(C, 8)
        return _Operand((torch.zeros if zero else torch.empty)(rows, 2 * lo, dtype=torch.bfloat16, device=self.device), C, lo)

    def pack(self, name: str, W: torch.Tensor) -> torch.Tensor:
        """Records `<name>.segs`, the k_segs of the launches on this tensor: 3 with the image [W_hi | W_lo] when any element has a bf16
        residual, else 2 on the plain image. to_v is the A operand of v^T = Wv n^T against the pair n, so it always carries a lo half."""
        Wh = W.to(torch.bfloat16)
        Wl = (W - Wh.float()).to(torch.bfloat16)
        segs = self._w[name + ".segs"] = 3 if name.endswith(".to_v") or bool((Wl != 0).any()) else 2
        return torch.cat([Wh, Wl], 1) if segs == 3 else Wh

    def weight(self, name: str) -> _Operand:
        t = self._w[name + ".w"]
        Kp = t.shape[1] // (self._w[name + ".segs"] - 1)
        return _Operand(t, Kp, t.shape[1] - Kp)

    def _gemm_kw(self, W: _Operand) -> dict:
        return dict(k_segs=3 if W.lo else 2)

    def groupnorm_silu(self, x, gamma, beta, y: _Operand, groups, eps, silu) -> None:
        ops.groupnorm_silu_split(x, gamma, beta, y.t, y.lo, groups, eps, silu)

    def from_stream(self, x: torch.Tensor) -> _Operand:
        """`lx_split_bf16`; a channel count that is no multiple of 4 -- the encoder's RGB input -- is zero-padded to one first (torch plumbing)."""
        M, C = x.shape
        if C % 4:
            x = torch.nn.functional.pad(x, (0, _pad_to(C, 4) - C))
        y = self.operand(M, C)
        ops.split_bf16(x, y.t, y.lo)
        return y

    def im2col3x3(self, x: torch.Tensor, h: _Operand, cols: _Operand, mode: int) -> None:
        ops.im2col3x3_split(x, h.C, h.lo, cols.t, mode)

    def softmax_rows(self, S, Pm: _Operand, scale, P: int, Ppad: int) -> None:
        ops.softmax_rows_split(S, Pm.t, scale, P, Ppad, Pm.lo)                  # Pm[:, P:Ppad] = +0, both halves


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
        self._op = _OperandsSplit(self.w, self.device) if self.precise else _Operands16("bf16", self.w, self.device)
        for k, v in sd.items():
            if k.endswith(".weight") and v.dim() in (2, 4):                     # Linear | Conv2d
                self._pack_conv(k[: -len(".weight")], v, sd.get(k[: -len("weight")] + "bias"))
            elif k.endswith(".weight") and v.dim() == 1:                        # GroupNorm affine
                self.w[k[: -len(".weight")] + ".g"] = v.detach().to(self.device, torch.float32).contiguous()
                self.w[k[: -len(".weight")] + ".b"] = sd[k[: -len("weight")] + "bias"].detach().to(self.device, torch.float32).contiguous()
        self.set_operands(operands)

    @property
    def operands(self) -> str:
        return self._op.name

    def set_operands(self, operands: str) -> None:
        """Switch a non-precise instance between bf16 and fp16 operands. The fp16 weight images are built at the first switch to fp16 and
        kept; the bf16 images always stay (the overflow fallback runs on them)."""
        if operands not in OPERANDS:
            raise ValueError(f"operands = {operands!r}: one of {OPERANDS}")
        if operands == "fp16" and self.precise:
            raise ValueError('operands="fp16" with precise=True: the precise mode runs on split-bf16 pairs')
        if operands == "fp16" and not self.w16:
            self._pack_w16()
        if not self.precise:
            self._op = _Operands16(operands, self.w16 if operands == "fp16" else self.w, self.device, self.f16_ovf if operands == "fp16" else None)

    # ---- weights -------------------------------------------------------------------------------------------------------
    def _pack_conv(self, name: str, w: torch.Tensor, b: Optional[torch.Tensor]) -> None:
        """`<name>.w`: the policy's image of the weight in `_im2col_weight`'s layout (bf16 [Npad, Kpad]; precise mode: `<name>.segs`
        and, where that is 3, [Npad, 2 Kpad] = [W_hi | W_lo]); `<name>.bias`: fp32 [Npad]; `<name>.shape`: (Cout, Cin, kh)."""
        Wp = self._op.pack(name, _im2col_weight(w, self.device))
        bp = torch.zeros(Wp.shape[0], dtype=torch.float32, device=self.device)
        if b is not None:
            bp[: w.shape[0]] = b.detach().to(self.device, torch.float32)
        self.w[name + ".w"], self.w[name + ".bias"] = Wp, bp
        self.w[name + ".shape"] = (w.shape[0], w.shape[1], w.shape[2] if w.dim() == 4 else 1)

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
            W, Wb = _im2col_weight(v, self.device), self.w[name + ".w"]         # (the pads are zeros in both and count as exact)
            stat[0] += (Wb.float().clamp(-65504.0, 65504.0).to(torch.float16).to(torch.bfloat16) != Wb).sum()
            stat[1] += (W.abs() > 65504.0).sum()
            total += v.numel()
            self.w16[name] = W.clamp(-65504.0, 65504.0).to(torch.float16)
        lost, clipped = (int(n) for n in stat.tolist())
        self.w16_inexact_share, self.w16_clipped = lost / max(total, 1), clipped

    # ---- building blocks (x: fp32 [B*H*W, C]) ----------------------------------------------------------------------------
    def _gn(self, x: torch.Tensor, B: int, name: str, silu: bool = True, out: Optional[_Operand] = None) -> _Operand:
        C = x.shape[1]
        y = self._op.operand(x.shape[0], C) if out is None else out
        self._op.groupnorm_silu(x.view(B, -1, C), self.w[name + ".g"], self.w[name + ".b"], y, self.G, 1e-6, silu)
        return y

    def _conv3(self, h: _Operand, B: int, H: int, W: int, name: str, mode: int = 0, out: Optional[torch.Tensor] = None,
               epilogue: int = LX_EPI_STORE_F32) -> Tuple[torch.Tensor, int, int]:
        """3x3 convolution of the NHWC operand h [B*H*W, Cin] as im2col + GEMM; image by image so the im2col scratch stays one image
        large. out: the fp32 stream [B*Ho*Wo, Npad] (epilogue STORE_F32, or RESID_F32, which accumulates into it)."""
        op, Wt, bias = self._op, self._op.weight(name), self.w[name + ".bias"]
        Np, Kp = Wt.t.shape[0], Wt.C
        Ho, Wo = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
        if out is None:
            out = torch.empty(B * Ho * Wo, Np, dtype=torch.float32, device=self.device)
        cols = op.operand(Ho * Wo, Kp)                                                                # gather rows: [taps], or [hi taps | lo taps]
        hv = h.t.view(B, H, W, h.t.shape[1])
        for b in range(B):
            op.im2col3x3(hv[b:b + 1], h, cols, mode)
            op.gemm(cols, Wt, out[b * Ho * Wo:(b + 1) * Ho * Wo], N=Np, K=Kp, bias=bias, epilogue=epilogue)
        return out, Ho, Wo

    def _lin(self, a: _Operand, name: str, out=None, epilogue: int = LX_EPI_STORE_BF16):
        """a W^T + bias into `out`: an operand (STORE_BF16) or the fp32 stream (STORE_F32; RESID_F32 accumulates)."""
        Wt = self._op.weight(name)
        Np, Kp = Wt.t.shape[0], Wt.C
        assert a.C == Kp, (name, a.C, Kp)
        if out is None:
            out = self._op.out(a.t.shape[0], Np, epilogue)
        self._op.gemm(a, Wt, out, N=Np, K=Kp, bias=self.w[name + ".bias"], epilogue=epilogue)
        return out

    def _operand(self, x: torch.Tensor) -> _Operand:
        """The fp32 stream x [M, C] as a GEMM operand."""
        return self._op.from_stream(x)

    def _resnet(self, x: torch.Tensor, B: int, H: int, W: int, p: str) -> torch.Tensor:
        h = self._gn(x, B, p + ".norm1")
        h1, _, _ = self._conv3(h, B, H, W, p + ".conv1")
        t = self._gn(h1, B, p + ".norm2")
        if (p + ".conv_shortcut.w") in self.w:
            x = self._lin(self._operand(x), p + ".conv_shortcut", epilogue=LX_EPI_STORE_F32)
        self._conv3(t, B, H, W, p + ".conv2", out=x, epilogue=LX_EPI_RESID_F32)          # x += conv2(t)
        return x

    def _attn(self, x: torch.Tensor, B: int, P: int, p: str) -> torch.Tensor:
        """Single-head attention over the P = H*W tokens of each image (diffusers Attention, residual_connection=True), one path for every
        format and token count. The key axis is padded to Ppad = roundup(P, 64) (the GEMM's K granule; its N granule is 8). The images lie
        back to back in n and k ([B*P, C]), so the Ppad key rows of image b run into image b+1's rows and, for the last image, into a zero
        tail that both buffers carry when Ppad > P: every row a GEMM reads lies inside its allocation and is finite (real rows of a
        neighbour, or zeros). Columns [P, Ppad) of S and of v^T are therefore finite garbage; the softmax reads none of the former and
        writes exact zeros for those keys, so the latter contribute nothing to P v. At Ppad == P there is no tail and nothing to fill."""
        C, op = x.shape[1], self._op
        Pp = _pad_to(P, 64)
        rows, real = (B - 1) * P + Pp, slice(0, B * P)                                                # the last image's Ppad rows end at `rows`
        n, k = op.operand(rows, C, zero=Pp > P), op.operand(rows, C, zero=Pp > P)
        self._gn(x, B, p + ".group_norm", silu=False, out=n.rows(real))
        q = self._lin(n.rows(real), p + ".to_q")
        self._lin(n.rows(real), p + ".to_k", out=k.rows(real))
        Wv, bv = op.weight(p + ".to_v"), self.w[p + ".to_v.bias"]
        S = torch.empty(P, Pp, dtype=torch.float32, device=self.device)
        Pm, vT, o = op.operand(P, Pp), op.operand(C, Pp), op.operand(B * P, C)
        for b in range(B):
            r, rp = slice(b * P, (b + 1) * P), slice(b * P, b * P + Pp)
            op.gemm(q.rows(r), k.rows(rp), S, N=Pp, K=C, epilogue=LX_EPI_STORE_F32)                   # S[:, :P] = q k^T
            op.softmax_rows(S, Pm, 1.0 / math.sqrt(C), P, Pp)                                         # Pm[:, P:] = +0
            op.gemm(Wv, n.rows(rp), vT, N=Pp, K=C, epilogue=LX_EPI_STORE_BF16)                        # v^T[:, :P] = Wv n^T (bias added below)
            op.gemm(Pm, vT, o.rows(r), N=C, K=Pp, bias=bv, epilogue=LX_EPI_STORE_BF16)                # rows of P sum to 1: P (v + 1 bv^T) = P v + bv
        self._lin(o, p + ".to_out.0", out=x, epilogue=LX_EPI_RESID_F32)
        return x

    def _mid(self, x, B, H, W, p):
        x = self._resnet(x, B, H, W, p + ".resnets.0")
        x = self._attn(x, B, H * W, p + ".attentions.0")
        return self._resnet(x, B, H, W, p + ".resnets.1")

    def _input(self, t: torch.Tensor) -> _Operand:
        """NCHW input -> the operand of conv_in."""
        return self._op.input(t)

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
        f16, self._op = self._op, _Operands16("bf16", self.w, self.device)
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
