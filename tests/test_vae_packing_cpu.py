"""CPU-only: the weight images LxAutoencoderKL packs -- constructing one on device="cpu" packs and launches nothing. A hand-made state dict
of a 3x3 convolution whose Cout and K both need padding, a 1x1 convolution given as 4-D, two Linears (to_v, to_q) and a GroupNorm affine,
once with bf16-representable values and once with an fp32 residual. What the images must hold is worked out here with plain indexing,
independently of the layout helper that the bf16 / split packing and the fp16 packing share."""
import pytest
import torch

from loongx_amd.vae import LxAutoencoderKL

bf16, f16, f32 = torch.bfloat16, torch.float16, torch.float32
CONVS = {"enc.conv": (5, 3, 3, 3), "dec.proj": (6, 10, 1, 1), "mid.attn.to_v": (64, 64), "mid.attn.to_q": (64, 64)}


def _roundup(n, m):
    return (n + m - 1) // m * m


def _state_dict(residual: bool):
    g = torch.Generator().manual_seed(5)
    sd = {}
    for name, shape in CONVS.items():
        w = torch.randn(*shape, generator=g) * 0.1
        sd[name + ".weight"] = w if residual else w.to(bf16).to(f32)
        sd[name + ".bias"] = torch.randn(shape[0], generator=g)
    sd["mid.attn.group_norm.weight"] = 1.0 + 0.1 * torch.randn(64, generator=g)
    sd["mid.attn.group_norm.bias"] = 0.1 * torch.randn(64, generator=g)
    return sd


def _expected(w):
    """fp32 [roundup(co, 8), roundup(kh*kw*ci, 64)]: element (o, c, dy, dx) at row o, column (dy*kw + dx)*ci + c; zeros elsewhere."""
    w4 = w if w.dim() == 4 else w[:, :, None, None]
    co, ci, kh, kw = w4.shape
    img = torch.zeros(_roundup(co, 8), _roundup(kh * kw * ci, 64), dtype=f32)
    for dy in range(kh):
        for dx in range(kw):
            for c in range(ci):
                img[:co, (dy * kw + dx) * ci + c] = w4[:, c, dy, dx]
    return img, co, kh * kw * ci


def _pads_are_zero(img, co, k, Kp):
    """rows [co, Np) and, in every Kp-wide half, columns [k, Kp)"""
    ok = bool((img[co:] == 0).all())
    for h in range(img.shape[1] // Kp):
        ok = ok and bool((img[:, h * Kp + k:(h + 1) * Kp] == 0).all())
    return ok


@pytest.mark.parametrize("residual", [False, True], ids=["bf16_representable", "fp32_residual"])
def test_weight_images_in_every_format(residual):
    sd = _state_dict(residual)
    b, a = LxAutoencoderKL(sd, None, "cpu", precise=False), LxAutoencoderKL(sd, None, "cpu", precise=True)
    assert b.precise is False and a.precise is True
    assert {k for k in a.w if not k.endswith(".segs")} == set(b.w) and not any(k.endswith(".segs") for k in b.w)
    assert {k[:-5] for k in a.w if k.endswith(".segs")} == set(CONVS)
    for name, shape in CONVS.items():
        E, co, k = _expected(sd[name + ".weight"])
        Np, Kp = E.shape
        assert (Np, Kp) == (_roundup(co, 8), _roundup(k, 64))
        hi = E.to(bf16)
        lo = (E - hi.float()).to(bf16)
        assert bool((lo != 0).any()) == residual                                # the variant is what it says
        # the 16-bit image: bf16(W) in im2col column order, zero pads
        wb = b.w[name + ".w"]
        assert wb.dtype == bf16 and wb.shape == (Np, Kp) and torch.equal(wb, hi) and _pads_are_zero(wb, co, k, Kp)
        # the split image: the same hi half; [W_hi | W_lo] and segs 3 iff there is a residual -- to_v always
        wa, segs = a.w[name + ".w"], a.w[name + ".segs"]
        assert segs == (3 if residual or name.endswith(".to_v") else 2)
        assert wa.dtype == bf16 and wa.shape == (Np, Kp * (segs - 1)) and _pads_are_zero(wa, co, k, Kp)
        assert torch.equal(wa[:, :Kp], wb)
        if segs == 3:
            assert torch.equal(wa[:co, Kp:Kp + k], lo[:co, :k])
        for m in (a, b):
            bias = m.w[name + ".bias"]
            assert bias.dtype == f32 and bias.shape == (Np,) and torch.equal(bias[:co], sd[name + ".bias"]) and bool((bias[co:] == 0).all())
            assert m.w[name + ".shape"] == (shape[0], shape[1], shape[2] if len(shape) == 4 else 1)
    for m in (a, b):
        assert torch.equal(m.w["mid.attn.group_norm.g"], sd["mid.attn.group_norm.weight"])
        assert torch.equal(m.w["mid.attn.group_norm.b"], sd["mid.attn.group_norm.bias"])


@pytest.mark.parametrize("residual", [False, True], ids=["bf16_representable", "fp32_residual"])
def test_fp16_images_share_the_layout_and_count_a_clipped_weight(residual):
    sd = _state_dict(residual)
    sd["enc.conv.weight"][4, 2, 1, 2] = 1e5                                     # one weight beyond fp16's range
    lx = LxAutoencoderKL(sd, None, "cpu")
    assert not lx.w16 and lx.w16_clipped == 0
    lx.set_operands("fp16")
    assert lx.operands == "fp16" and lx.w16.keys() == set(CONVS) and lx.w16_clipped == 1
    for name in CONVS:
        E, co, k = _expected(sd[name + ".weight"])
        img = lx.w16[name]
        assert img.dtype == f16 and img.shape == lx.w[name + ".w"].shape == E.shape
        assert torch.equal(img, E.clamp(-65504.0, 65504.0).half()) and _pads_are_zero(img, co, k, E.shape[1])
    assert float(lx.w16["enc.conv"][4, (1 * 3 + 2) * 3 + 2]) == 65504.0
    assert torch.equal(lx.w["enc.conv.w"], LxAutoencoderKL(sd, None, "cpu").w["enc.conv.w"])          # the bf16 images stay as they were
