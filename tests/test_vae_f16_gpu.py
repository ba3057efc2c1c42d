"""The FLUX VAE on fp16 operands (LxAutoencoderKL(operands="fp16"), what dtype=torch.float16 selects): the three fp16-writing row kernels of
csrc/vae.hip against float64, the convolution and the mid-block attention on fp16 images, whole encode / decode against the fp32 oracle
beside the bf16-operand VAE on the same weights, the overflow contract, and generate() from pixels to pixels with a float16 pipeline.

Kernel bounds are derived: round to nearest into fp16's normal range is within 2^-12 = 2.44e-4 relative per element, so norm-wise too;
every kernel bound here sits under what bf16 bits would give (>= 1e-3). The layer-level figures "emulated" are those of
tools/vae_f16_emulation.py (the oracle with its GEMM operands rounded to the format, on the CPU):

    | case                                 | bf16 mean / image   | fp16 mean / image   | ratio     |
    | SMALL 32x32                          | 6.80e-3 / 7.06e-3   | 8.72e-4 / 8.86e-4   | 7.8 / 8.0 |
    | SMALL 18x14 (63 tokens, padded keys) | 6.73e-3 / 7.39e-3   | 8.19e-4 / 9.61e-4   | 8.2 / 7.7 |
    | SMALL 32x32, weights rounded to bf16 | 4.88e-3 / 4.97e-3   | 6.18e-4 / 6.22e-4   | 7.9 / 8.0 |
    | full shape 64x64                     | 1.10e-2 / 1.27e-2   | 1.29e-3 / 1.56e-3   | 8.5 / 8.2 |
    | full shape 64x64, bf16 weights       | 7.46e-3 / 9.26e-3   | 9.28e-4 / 1.17e-3   | 8.0 / 7.9 |
"""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import flux_modules as fm  # noqa: E402
from oracle import flux_ref as fr  # noqa: E402
from oracle import vae as ovae  # noqa: E402
from tests import tiny_ckpt  # noqa: E402
from tests.helpers import relerr  # noqa: E402
from tests.test_vae_anysize_gpu import SENTINEL, SMALL, SOFTMAX_CASES, _attn_branch, _nan, rnd  # noqa: E402
from tests.test_vae_precise_gpu import _conv_ref, _pad_to, _stats  # noqa: E402

DEV = "cuda"
bf16, f16, f32 = torch.bfloat16, torch.float16, torch.float32
F16_MAX = 65504.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


def _counter():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- 1. lx_groupnorm_silu_f16 -----------------------------------------------------------------------------------------------------------
GN_SHAPES = [(2, 60, 128, 32), (1, 300, 512, 32), (1, 4100, 128, 32)]
# Share of outputs that must be bit-equal with float64 -> fp32 -> fp16. The kernel keeps lx_groupnorm_silu's fp32 statistics (sum and sum of
# squares; inputs with mean / std = 8), and an fp32 two-pass emulation of exactly that arithmetic on the CPU (same chunking, same fold
# order) lands on the other side of an fp16 rounding boundary for 0.95-1.11 % / 1.32-1.41 % / 1.70-1.81 % of the elements of the three
# shapes: fp32 error of a few 1e-6 against a rounding interval of 2.4e-4 ... 4.9e-4. 99 % is therefore out of the arithmetic's reach on
# the two larger shapes; the floor is 1 - 2 x the emulated mismatch of the worst shape (1.81 %), the factor 2 for what the emulation
# leaves out (v_rsq_f32, v_exp_f32, contraction). bf16 bits would agree in about one element of eight, truncation in one of two.
# Measured on MI355X: 98.89 / 99.04 % (P = 60, silu / plain), 98.72 / 98.65 % (P = 300), 98.29 / 98.18 % (P = 4100).
GN_EXACT_SHARE = 0.963


@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "B%d_P%d_C%d_G%d" % s)
def test_groupnorm_silu_f16_vs_float64(ops, shape, silu):
    """GroupNorm (+ SiLU) of randn + 8 into an fp16 image against float64: 1 / 16 / 64 row chunks, the last of the 64 ragged. Bound 3e-4
    (one fp16 rounding, 2.44e-4, plus the fp32 statistics); emulated on the CPU 2.07e-4 ... 2.11e-4. The counter stays 0."""
    B, P, C, G = shape
    x = rnd(B, P, C, seed=41) + 8.0
    g, b = 1.0 + 0.2 * rnd(C, seed=42), 0.3 * rnd(C, seed=43)
    y = torch.full((B, P, C), float("nan"), dtype=f16, device=DEV)
    ovf = _counter()
    ops.groupnorm_silu_f16(x.to(DEV), g.to(DEV), b.to(DEV), y, G, 1e-6, silu, f16_ovf=ovf)
    torch.cuda.synchronize()
    want = F.group_norm(x.double().transpose(1, 2), G, g.double(), b.double(), 1e-6).transpose(1, 2)
    if silu:
        want = F.silu(want)
    y = y.cpu()
    err = relerr(y.double(), want)
    share = float((_bits(y) == _bits(want.float().to(f16))).float().mean())
    print(f"groupnorm_silu_f16 {shape} silu={silu}: relerr {err:.3e}, bit-equal with the rounded float64 reference {share:.4%}")
    assert err < 3e-4
    assert share >= GN_EXACT_SHARE, share
    assert int(ovf.item()) == 0


def test_groupnorm_silu_f16_saturates_and_counts(ops):
    """gamma scaled by 1e5: normalised values beyond +-0.655 leave fp16's range. Every stored value is finite and within +-65504, the
    elements whose reference is beyond the range are exactly +-65504, the counter moved; a launch on a benign gamma leaves it where it
    was, and a NULL counter is accepted (same image)."""
    B, P, C, G = 1, 300, 512, 32
    x = (rnd(B, P, C, seed=41) + 8.0).to(DEV)
    g, b = 1.0 + 0.2 * rnd(C, seed=42), 0.3 * rnd(C, seed=43)
    big = (g * 1e5).to(DEV)
    y, ovf = torch.empty(B, P, C, dtype=f16, device=DEV), _counter()
    ops.groupnorm_silu_f16(x, big, b.to(DEV), y, G, 1e-6, False, f16_ovf=ovf)
    n1 = int(ovf.item())
    want = F.group_norm(x.cpu().double().transpose(1, 2), G, g.double() * 1e5, b.double(), 1e-6).transpose(1, 2)
    yc = y.cpu().double()
    assert bool(torch.isfinite(yc).all()) and float(yc.abs().max()) == F16_MAX
    over = want.abs() > F16_MAX * 1.001                                       # (clear of the last rounding interval below the limit)
    assert int(over.sum()) > 1000 and torch.equal(yc[over], torch.sign(want[over]) * F16_MAX)
    assert relerr(yc[~over & (want.abs() < F16_MAX * 0.999)], want[~over & (want.abs() < F16_MAX * 0.999)]) < 3e-4
    assert n1 > 0
    y2 = torch.empty_like(y)
    ops.groupnorm_silu_f16(x, g.to(DEV), b.to(DEV), y2, G, 1e-6, False, f16_ovf=ovf)
    assert int(ovf.item()) == n1 and float(y2.float().abs().max()) < 100.0
    y3 = torch.empty_like(y)
    ops.groupnorm_silu_f16(x, big, b.to(DEV), y3, G, 1e-6, False)                # NULL counter
    torch.cuda.synchronize()
    assert torch.equal(_bits(y3), _bits(y))


# ---- 2. lx_softmax_rows_f16 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=lambda c: "M%d_valid%d_store%d_lds%d_ldp%d_off%d" % c)
def test_softmax_rows_f16(ops, case):
    """The cases of test_softmax_rows_valid with fp16 probabilities (lds 67 / ldp 70 and the base one float off take the scalar path): the
    pad columns of S hold NaN, P is prefilled with the sentinel. Bound 3e-4 against float64 softmax over [0, n_valid): one fp16 rounding
    plus __expf. [n_valid, n_store) is +0, the sentinels at and beyond n_store stay."""
    M, nv, ns, lds, ldp, off = case
    host = _nan((M, lds))
    host[:, :nv] = rnd(M, nv, seed=6, scale=3.0)
    flat = torch.empty(M * lds + off, dtype=f32, device=DEV)
    S = flat[off:].view(M, lds)
    S.copy_(host)
    Pfull = torch.full((M, ldp), SENTINEL, dtype=f16, device=DEV)
    ops.softmax_rows_f16(S, Pfull[:, :ns], 0.25, n_valid=nv)
    torch.cuda.synchronize()
    Pm = Pfull.cpu()
    want = torch.softmax(host[:, :nv].double() * 0.25, -1)
    err = relerr(Pm[:, :nv].double(), want)
    print(f"softmax_rows_f16 {case}: relerr {err:.3e}")
    assert err < 3e-4
    z = Pm[:, nv:ns]
    assert torch.equal(z, torch.zeros_like(z)) and not torch.signbit(z.float()).any()        # +0, not -0
    assert torch.equal(Pm[:, ns:], torch.full((M, ldp - ns), SENTINEL, dtype=f16))


def test_softmax_rows_f16_unpadded_is_the_same_entry_point(ops):
    """n_valid None: every column is a key (what _attn launches for P % 64 == 0); equal to the n_valid == n_store call bit for bit."""
    S = rnd(64, 64, seed=7, scale=3.0).to(DEV)
    a, b = torch.empty(64, 64, dtype=f16, device=DEV), torch.empty(64, 64, dtype=f16, device=DEV)
    ops.softmax_rows_f16(S, a, 0.25)
    ops.softmax_rows_f16(S, b, 0.25, n_valid=64)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b)) and relerr(a.cpu().double(), torch.softmax(S.cpu().double() * 0.25, -1)) < 3e-4


# ---- 3. lx_convert_f16 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_dtype", [f32, bf16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1000, 1 << 20])
def test_convert_f16_saturates_counts_and_keeps_nan(ops, n, src_dtype):
    """Every element is the nearest-even fp16 of its source (bit for bit), values beyond +-65504 and +-inf become +-65504 and are
    counted, NaN stays NaN; the same data without those values leaves the counter at 0."""
    src = (rnd(n, seed=8) * 100.0).to(src_dtype)
    benign = src.clone()
    special = torch.tensor([7e4, -7e4, float("inf"), float("-inf"), float("nan"), 3e38, -1e9], dtype=src_dtype)
    at = torch.arange(len(special)) * (n // len(special)) + 3                                # spread over the grid (several waves clip)
    src[at] = special
    dst, ovf = torch.full((n,), SENTINEL, dtype=f16, device=DEV), _counter()
    ops.convert_f16(dst, src.to(DEV), f16_ovf=ovf)
    count = int(ovf.item())
    got, want = dst.cpu(), src.float().clamp(-F16_MAX, F16_MAX).to(f16)
    nan = torch.isnan(src.float())
    assert int(nan.sum()) == 1 and torch.equal(torch.isnan(got.float()), nan)
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])
    assert got[at[:4]].tolist() == [F16_MAX, -F16_MAX, F16_MAX, -F16_MAX] and got[at[5:]].tolist() == [F16_MAX, -F16_MAX]
    assert 1 <= count <= 6, count                                                            # a wave counts once, whatever it clipped
    ops.convert_f16(dst, benign.to(DEV), f16_ovf=ovf)
    assert int(ovf.item()) == count
    fresh = _counter()
    ops.convert_f16(dst, benign.to(DEV), f16_ovf=fresh)
    ops.convert_f16(dst, src.to(DEV))                                                        # NULL counter
    torch.cuda.synchronize()
    assert int(fresh.item()) == 0 and torch.equal(_bits(dst.cpu())[~nan], _bits(want)[~nan])


# ---- 4. the convolution on fp16 images ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C", [3, 16, 128])
def test_im2col3x3_f16_gemm_vs_float64_conv(ops, C, mode):
    """test_im2col3x3_split_gemm_vs_float64_conv's data through the fp16 path: lx_convert_f16 makes the image, lx_im2col3x3 gathers it as
    16-bit words (C = 3 one element at a time, K padded 27 -> 64), an LX_OPERANDS_F16 launch multiplies by the fp16 weight image into fp32.
    Bound 5e-4: two rounded operands, 2 x 2^-12 (the bf16 product on such data is 2.3e-3). Pad columns exactly zero, the NaN rows behind
    the last output pixel untouched, nothing clipped."""
    B, H, W, Co = 2, 6, 10, 16
    x = rnd(B, C, H, W, seed=50 + C)
    w = rnd(Co, C, 3, 3, seed=51 + C) / (3.0 * C ** 0.5)
    Ho, Wo = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
    rows, Kp = B * Ho * Wo, _pad_to(9 * C, 64)
    ovf = _counter()
    img = torch.empty(B, H, W, C, dtype=f16, device=DEV)
    ops.convert_f16(img, x.permute(0, 2, 3, 1).contiguous().to(DEV), f16_ovf=ovf)
    cols = torch.full((rows + 3, Kp), float("nan"), dtype=f16, device=DEV)
    ops.im2col3x3(img.view(bf16), cols[:rows].view(bf16), mode)
    Wp = torch.zeros(Co, Kp, dtype=f16)
    Wp[:, :9 * C] = w.permute(0, 2, 3, 1).reshape(Co, 9 * C).to(f16)
    out = torch.empty(rows, Co, dtype=f32, device=DEV)
    ops.gemm([ops.gemm_desc(cols[:rows], Wp.to(DEV), out, epilogue=ops.LX_EPI_STORE_F32, f16=True, f16_ovf=ovf)])
    torch.cuda.synchronize()
    want = _conv_ref(x.double(), w.double(), mode).permute(0, 2, 3, 1).reshape(rows, Co)
    err = relerr(out.cpu(), want)
    print(f"im2col3x3 on fp16 C={C} mode={mode}: relerr {err:.3e}")
    assert err < 5e-4
    cols = cols.cpu()
    padc = cols[:rows, 9 * C:]
    assert padc.shape[1] == Kp - 9 * C and torch.equal(padc, torch.zeros_like(padc))
    assert bool(torch.isfinite(cols[:rows, :9 * C].float()).all()) and bool(torch.isnan(cols[rows:].float()).all())
    assert int(ovf.item()) == 0


def test_gemm_f16_weights_as_a_operand_with_an_fp16_store(ops):
    """The v^T = Wv n^T launch of _attn: the weight image is the A operand (M = C = 128, N = 64 tokens, K = C), the store is fp16 and
    carries the counter. Bound 7.4e-4, derived: two rounded operands and one rounded output, 3 x 2^-12; bf16 is at 3e-3 or worse."""
    C, P = 128, 64
    wv, n = rnd(C, C, seed=61) / C ** 0.5, rnd(P, C, seed=62)
    ovf = _counter()
    vT = torch.empty(C, P, dtype=f16, device=DEV)
    ops.gemm([ops.gemm_desc(wv.to(f16).to(DEV), n.to(f16).to(DEV), vT, epilogue=ops.LX_EPI_STORE_BF16, f16=True, f16_ovf=ovf)])
    torch.cuda.synchronize()
    err = relerr(vT.cpu().double(), wv.double() @ n.double().t())
    print(f"v^T = Wv n^T on fp16: relerr {err:.3e}")
    assert err < 7.4e-4 and int(ovf.item()) == 0


# ---- 5. the attention branch ----------------------------------------------------------------------------------------------------------------
ATTN_MEASURED = {9: 6.161e-4, 63: 4.641e-4, 64: 4.731e-4, 65: 4.655e-4, 240: 3.590e-4}       # MI355X, fp16 operands (the test asserts under 2 x these)


@pytest.mark.parametrize("P", [9, 63, 64, 65, 240])
def test_attn_f16_vs_float64_oracle(ops, P):
    """out - x of _attn on fp16 operands against the oracle AttnBlock in float64 (B = 2, C = 128; 64 takes the unpadded launches, the
    others a padded key axis), beside the bf16-operand instance on the same input: at most a quarter of its error (three more significand
    bits are a factor of 8 and the emulation gives 7.7-7.8; the divisor 4 leaves a factor of 2 for the fp32-side terms), and under twice
    the figure measured on MI355X. Emulated at C = 512: 2.59e-4 (bf16 2.09e-3) at 1024 tokens, 2.33e-4 (1.81e-3) at 4096, 2.27e-4 (1.76e-3) at 16384.
    Measured on MI355X at C = 128, fp16 (bf16): P = 9: 6.161e-4 (5.357e-3, x8.7), 63: 4.641e-4 (3.802e-3, x8.2), 64: 4.731e-4 (3.700e-3, x7.8),
    65: 4.655e-4 (3.745e-3, x8.0), 240: 3.590e-4 (3.012e-3, x8.4)."""
    from loongx_amd.vae import LxAutoencoderKL
    B, C = 2, 128
    ref = ovae.init_synthetic_(ovae.AttnBlock(C), 21)
    sd = {"a." + k: v for k, v in ref.state_dict().items()}
    lx16, lxb = LxAutoencoderKL(sd, SMALL, DEV, operands="fp16"), LxAutoencoderKL(sd, SMALL, DEV)
    x = rnd(B * P, C, seed=22 + P) + 0.2
    got16, gotb = _attn_branch(lx16, x, B, P), _attn_branch(lxb, x, B, P)
    ref = ref.double()
    with torch.no_grad():
        x4 = x.double().view(B, P, 1, C).permute(0, 3, 1, 2)
        want = (ref(x4) - x4).permute(0, 2, 3, 1).reshape(B * P, C)
    e16, eb = relerr(got16, want), relerr(gotb, want)
    print(f"_attn fp16 P={P}: relerr {e16:.3e} (bf16 {eb:.3e}, x{eb / e16:.1f})")
    assert e16 <= eb / 4.0, (e16, eb)
    assert e16 < 2.0 * ATTN_MEASURED[P], (e16, ATTN_MEASURED[P])
    assert int(lx16.f16_ovf.item()) == 0


# ---- 6. whole encoder and decoder -----------------------------------------------------------------------------------------------------------
def _models(cfg, bf16_weights=False):
    from loongx_amd.vae import LxAutoencoderKL
    ref = ovae.init_synthetic_(ovae.AutoencoderKL(**cfg), 3)
    if bf16_weights:
        ref.load_state_dict({k: v.to(bf16).to(v.dtype) for k, v in ref.state_dict().items()})
    sd = ref.state_dict()
    return ref, LxAutoencoderKL(sd, cfg, DEV, operands="fp16"), LxAutoencoderKL(sd, cfg, DEV)


@pytest.fixture(scope="module")
def small_models(ops):
    return _models(SMALL)


@pytest.fixture(scope="module")
def small_models_bf16_weights(ops):
    return _models(SMALL, bf16_weights=True)


@pytest.fixture(scope="module")
def full_models(ops):
    return _models({})


def _f16_vs_oracle(models, H, W, measured, label):
    """_precise_vs_oracle's inputs; per statistic: fp16 <= bf16 / 4 and fp16 < 2 x the MI355X figure. The counter is 0 (a clipped call would
    have raised: the instances run under f16_overflow="raise"); _stats checks fp32 outputs and that a second decode gives the same bits."""
    ref, lx16, lxb = models
    assert lx16.operands == "fp16" and lx16.f16_overflow == "raise" and lx16.w16_clipped == 0
    nd = len(ref.config.block_out_channels) - 1
    h, w = H >> nd, W >> nd
    img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(1)) * 2 - 1
    noise = torch.randn(2, 16, h, w, generator=torch.Generator().manual_seed(2))
    z = torch.randn(2, 16, h, w, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = ref.encode(img).latent_dist
        wimg = ref.decode(z, return_dict=False)[0]
    e16 = _stats(lx16, img, noise, z, want, wimg)
    assert int(lx16.f16_ovf.item()) == 0
    eb = _stats(lxb, img, noise, z, want, wimg)
    names = ("mean", "std", "sample", "image")
    print(f"VAE fp16 {label} {H}x{W} ({h * w} tokens): " + " ".join(f"{n} {p:.3e} (bf16 {b:.3e}, x{b / p:.1f})" for n, p, b in zip(names, e16, eb)))
    for n, p, b, m in zip(names, e16, eb, measured):
        assert p <= b / 4.0, (n, p, b)
        assert p < 2.0 * m, (n, p, m)


# measured on MI355X, per statistic (mean, std, sample, image), fp16 operands; the tests assert under 2 x these
M_SMALL_32 = (8.717e-4, 1.812e-4, 3.667e-4, 8.817e-4)
M_SMALL_18x14 = (8.150e-4, 1.689e-4, 3.391e-4, 9.903e-4)
M_SMALL_BF16W = (6.186e-4, 1.272e-4, 2.568e-4, 6.272e-4)
M_FULL_64 = (1.314e-3, 2.716e-4, 5.257e-4, 1.585e-3)
M_FULL_40x56 = (1.277e-3, 2.574e-4, 5.159e-4, 1.688e-3)


def test_vae_f16_small_32x32(small_models):
    """Two-level VAE at 32x32 (256 tokens), fp32 weights as they are (the fp16 images are rounded from them). Emulated: mean 8.72e-4,
    image 8.86e-4 (bf16 6.80e-3 / 7.06e-3). Measured on MI355X: mean 8.717e-4, std 1.812e-4,
    sample 3.667e-4, image 8.817e-4 (the bf16-operand VAE beside it: 6.874e-3, 1.455e-3, 2.853e-3, 7.008e-3: 7.8 ... 8.0 times those)."""
    _f16_vs_oracle(small_models, 32, 32, M_SMALL_32, "small")


def test_vae_f16_small_18x14(small_models):
    """... at 18x14: a 9x7 latent, 63 tokens, the padded key axis. Emulated: mean 8.19e-4, image 9.61e-4 (bf16 6.73e-3 / 7.39e-3).
    Measured on MI355X: mean 8.150e-4, std 1.689e-4, sample 3.391e-4, image 9.903e-4 (7.4 ... 8.4 times below the bf16-operand VAE)."""
    _f16_vs_oracle(small_models, 18, 14, M_SMALL_18x14, "small")


def test_vae_f16_small_bf16_weights(small_models_bf16_weights):
    """The state dict rounded to bf16 on both sides (what a FLUX.1 checkpoint holds): the fp16 weight images are exact but for the bf16
    values below 2^-17 or so, whose last bits fall under fp16's subnormal spacing 2^-24 -- for N(0, 0.02^2) weights about 3e-4 of them,
    which is what w16_inexact_share counts. Emulated: mean 6.18e-4, image 6.22e-4 (bf16 4.88e-3 / 4.97e-3). Measured on MI355X: mean
    6.186e-4, std 1.272e-4, sample 2.568e-4, image 6.272e-4 (7.8 ... 8.2 times below the bf16-operand VAE on the same weights)."""
    lx16 = small_models_bf16_weights[1]
    assert 0.0 < lx16.w16_inexact_share < 1e-3 and lx16.w16_clipped == 0
    _f16_vs_oracle(small_models_bf16_weights, 32, 32, M_SMALL_BF16W, "small, bf16 weights")


def test_vae_f16_full_64x64(full_models):
    """The full FLUX.1 VAE shape at 64x64 (64 tokens). Emulated: mean 1.29e-3, image 1.56e-3 (bf16 1.10e-2 / 1.27e-2). Measured on
    MI355X: mean 1.314e-3, std 2.716e-4, sample 5.257e-4, image 1.585e-3 (8.0 ... 8.4 times below the bf16-operand VAE: 1.092e-2, 2.226e-3,
    4.427e-3, 1.269e-2)."""
    _f16_vs_oracle(full_models, 64, 64, M_FULL_64, "full")


def test_vae_f16_full_40x56(full_models):
    """The full shape at 40x56: a 5x7 latent, 35 tokens. Emulated: mean 1.28e-3, image 1.72e-3 (bf16 1.06e-2 / 1.33e-2). Measured on MI355X:
    mean 1.277e-3, std 2.574e-4, sample 5.159e-4, image 1.688e-3 (8.0 ... 8.5 times below the bf16-operand VAE)."""
    _f16_vs_oracle(full_models, 40, 56, M_FULL_40x56, "full")


def test_f16_decode_ignores_stale_scratch(small_models):
    """As test_precise_decode_ignores_stale_scratch: the fp16 buffers' pad rows are zero-filled or never read, so a decode at 9x7 latents
    after the caching allocator was seeded with NaN blocks gives the same bits as before."""
    lx = small_models[1]
    z = rnd(2, 16, 9, 7, seed=31).to(DEV)
    before = lx.decode(z, return_dict=False)[0].clone()
    torch.cuda.synchronize()
    junk = [torch.full((n,), float("nan"), dtype=f32, device=DEV) for n in (1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24, 1 << 25)]
    junk += [torch.full((n,), float("nan"), dtype=f16, device=DEV) for n in (63 * 128, 63 * 512, 126 * 512, 190 * 512, 256 * 128, 1 << 21, 1 << 22)] * 4
    torch.cuda.synchronize()
    del junk
    after = lx.decode(z, return_dict=False)[0]
    assert bool(torch.isfinite(before).all()) and bool(torch.isfinite(after).all())
    assert torch.equal(before, after)


# ---- 7. the overflow contract -----------------------------------------------------------------------------------------------------------------
def _policy_walk(lx16, lxb, z, img):
    """raise / warn / fallback on a decode that clips; then an encode, which must not report."""
    from loongx_amd.flux.generate import F16OverflowError
    want = lxb.decode(z, return_dict=False)[0]
    lx16.f16_overflow = "raise"
    with pytest.raises(F16OverflowError, match="fp16 operands"):
        lx16.decode(z)
    lx16.f16_overflow = "warn"
    with pytest.warns(RuntimeWarning, match="the result was kept"):
        kept = lx16.decode(z, return_dict=False)[0]
    assert bool(torch.isfinite(kept).all()) and not torch.equal(kept, want)
    lx16.f16_overflow = "fallback"
    with pytest.warns(RuntimeWarning, match="with bf16 operands"):
        again = lx16.decode(z, return_dict=False)[0]
    assert torch.equal(again, want) and lx16.operands == "fp16"
    return want


def test_f16_overflow_policy_on_a_clipping_norm(ops):
    """SMALL VAE whose decoder.conv_norm_out gamma is 1e6 times too large: its fp16 image saturates. "raise" -> F16OverflowError, "warn" ->
    RuntimeWarning and a finite image, "fallback" -> RuntimeWarning and the bits of the bf16-operand instance; the encoder of the same
    object is healthy, and its call right after does not report (the counter is zeroed per call)."""
    from loongx_amd.vae import LxAutoencoderKL
    sd = {k: v.clone() for k, v in ovae.init_synthetic_(ovae.AutoencoderKL(**SMALL), 3).state_dict().items()}
    sd["decoder.conv_norm_out.weight"] *= 1e6
    lx16, lxb = LxAutoencoderKL(sd, SMALL, DEV, operands="fp16"), LxAutoencoderKL(sd, SMALL, DEV)
    assert lx16.w16_clipped == 0
    z = rnd(2, 16, 4, 4, seed=3).to(DEV)
    img = (torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    _policy_walk(lx16, lxb, z, img)
    lx16.f16_overflow = "raise"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mean = lx16.encode(img).latent_dist.mean
    assert bool(torch.isfinite(mean).all()) and int(lx16.f16_ovf.item()) == 0


def test_f16_overflow_policy_on_a_clipped_weight(ops):
    """A weight of 1e5 in the state dict: clipped to 65504 in the fp16 image, counted in w16_clipped and reported by every call the
    same way as a clipped activation."""
    from loongx_amd.flux.generate import F16OverflowError
    from loongx_amd.vae import LxAutoencoderKL
    sd = {k: v.clone() for k, v in ovae.init_synthetic_(ovae.AutoencoderKL(**SMALL), 3).state_dict().items()}
    sd["decoder.conv_in.weight"][0, 0, 0, 0] = 1e5
    lx16, lxb = LxAutoencoderKL(sd, SMALL, DEV, operands="fp16"), LxAutoencoderKL(sd, SMALL, DEV)
    assert lx16.w16_clipped == 1 and float(lx16.w16["decoder.conv_in"].float().abs().max()) == F16_MAX
    z = rnd(2, 16, 4, 4, seed=3).to(DEV)
    img = (torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    _policy_walk(lx16, lxb, z, img)
    lx16.f16_overflow = "raise"
    with pytest.raises(F16OverflowError, match="1 weight"):
        lx16.encode(img)


# ---- 8. the default is what it was ---------------------------------------------------------------------------------------------------------------
def test_bf16_operands_are_the_default_and_set_operands_returns_to_them(ops):
    from loongx_amd.vae import LxAutoencoderKL
    sd = ovae.init_synthetic_(ovae.AutoencoderKL(**SMALL), 3).state_dict()
    a, b = LxAutoencoderKL(sd, SMALL, DEV), LxAutoencoderKL(sd, SMALL, DEV, operands="bf16")
    c = LxAutoencoderKL(sd, SMALL, DEV, operands="fp16")
    assert a.operands == "bf16" and b.operands == "bf16" and a.precise is False
    assert a.w.keys() == b.w.keys() == c.w.keys() and not a.w16 and not b.w16 and a.f16_ovf is None
    assert all(torch.equal(v, b.w[k]) and torch.equal(v, c.w[k]) for k, v in a.w.items() if isinstance(v, torch.Tensor))
    assert c.w16.keys() == {k[:-2] for k in c.w if k.endswith(".w")}
    assert all(v.dtype == f16 and v.shape == c.w[k + ".w"].shape for k, v in c.w16.items())
    img = (torch.rand(2, 3, 18, 14, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    z = rnd(2, 16, 9, 7, seed=3).to(DEV)
    dec, enc = a.decode(z).sample, a.encode(img).latent_dist.mean
    assert torch.equal(dec, b.decode(z).sample) and torch.equal(enc, b.encode(img).latent_dist.mean)
    b.set_operands("fp16")
    assert b.operands == "fp16" and b.w16.keys() == c.w16.keys() and b.w.keys() == a.w.keys()
    d16 = b.decode(z).sample
    assert torch.equal(d16, c.decode(z).sample) and not torch.equal(d16, dec)
    b.set_operands("bf16")
    assert b.operands == "bf16"
    assert torch.equal(dec, b.decode(z).sample) and torch.equal(enc, b.encode(img).latent_dist.mean)
    with pytest.raises(ValueError, match="precise=True"):
        LxAutoencoderKL(sd, SMALL, DEV, precise=True, operands="fp16")
    with pytest.raises(ValueError, match="precise=True"):
        LxAutoencoderKL(sd, SMALL, DEV, precise=True).set_operands("fp16")


class _CountingLib:
    """loongx_amd.ops.lib with every call counted by entry point."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


def test_f16_issues_the_bf16_paths_launches_one_for_one(ops, small_models, monkeypatch):
    """Decode of an 8x8 latent (64 tokens: the unpadded attention launches) and of a 9x7 one (63: the padded ones), encode of 64x64: the
    fp16 instance makes the bf16 instance's calls into the library, entry point for entry point, with the three fp16 producers in the
    places of lx_groupnorm_silu, lx_softmax_rows / lx_softmax_rows_valid and lx_convert -- plus one lx_convert_f16 per call for the input,
    which the bf16 path casts in torch."""
    _, lx16, lxb = small_models
    same = {"lx_groupnorm_silu_f16": "lx_groupnorm_silu", "lx_softmax_rows_f16": "lx_softmax", "lx_softmax_rows": "lx_softmax",
            "lx_softmax_rows_valid": "lx_softmax", "lx_convert_f16": "lx_convert"}
    img = (torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    runs = [lambda m: m.decode(rnd(1, 16, 8, 8, seed=3).to(DEV)), lambda m: m.decode(rnd(1, 16, 9, 7, seed=3).to(DEV)), lambda m: m.encode(img)]
    for run in runs:
        counts = []
        for m in (lx16, lxb):
            lib = _CountingLib(ops.lib)
            monkeypatch.setattr(ops, "lib", lib)
            run(m)
            monkeypatch.undo()
            c = {}
            for k, v in lib.calls.items():
                c[same.get(k, k)] = c.get(same.get(k, k), 0) + v
            counts.append(c)
        c16, cb = counts
        assert c16.pop("lx_convert") == cb.pop("lx_convert", 0) + 1
        assert c16 == cb and cb["lx_gemm_bf16"] > 10 and cb["lx_softmax"] == 1, (c16, cb)


# ---- 9. selection ----------------------------------------------------------------------------------------------------------------------------------
def test_from_pretrained_float16_selects_the_fp16_vae(ops, tmp_path):
    from loongx_amd.flux.pipeline import LxFluxPipeline
    d = str(tmp_path / "flux_tiny")
    tiny_ckpt.build_flux_dir(d, with_text=False)
    p16 = LxFluxPipeline.from_pretrained(d, dtype=torch.float16, load_text_encoders=False)
    assert p16.vae.operands == "fp16" and p16.vae.precise is False and p16.vae.w16
    pb = LxFluxPipeline.from_pretrained(d, dtype=torch.bfloat16, load_text_encoders=False)
    assert pb.vae.operands == "bf16" and pb.vae.precise is False and not pb.vae.w16
    p32 = LxFluxPipeline.from_pretrained(d, dtype=torch.float32, load_text_encoders=False)
    assert p32.vae.precise is True and p32.vae.operands == "bf16"


# ---- 10. pixels to pixels ----------------------------------------------------------------------------------------------------------------------------
P2P_MEASURED = 4.765e-4       # MI355X, arm (a): see the docstring


def test_generate_80x48_float16_pixels_to_pixels(ops, tmp_path, monkeypatch):
    """The chain of test_generate_80x48_float32_pixels_to_pixels with OminiModel(dtype=torch.float16) and output_type="pt", against the
    oracle chain, three arms on the same model: (a) the fp16 VAE as selected, (b) pipe.vae swapped for a bf16-operand instance of the same
    weights, (c) swapped for a precise instance -- (c) is the fp16 DiT's own share of the pixel error. (a) must be at most half of (b) and
    under twice its measured figure. Measured on MI355X: (a) 4.765e-4, (b) 2.456e-3 (5.2 times (a)), (c) 3.727e-4: the fp16 DiT's share is most
    of what is left, so the factor between (a) and (b) is 5 here and not the VAE's own 8."""
    from PIL import Image
    from loongx_amd import vae as lxvae
    from src.flux.condition import Condition
    from src.flux.generate import generate
    from src.train.model import OminiModel
    d = str(tmp_path / "flux_tiny")
    tr, vae = tiny_ckpt.build_flux_dir(d)
    sd, _ = tiny_ckpt.loongx_state_dict(tr)
    monkeypatch.setattr(lxvae.DiagonalGaussianDistribution, "sample", lambda self, generator=None, noise=None: self.mean)
    model = OminiModel(flux_pipe_id=d, lora_config={"r": 4, "lora_alpha": 4}, device="cuda", dtype=torch.float16, model_config={})
    model.load_state_dict(sd)
    assert model.flux_pipe.vae.operands == "fp16" and model.flux_pipe.vae.precise is False
    Wpx, Hpx, steps, prompt = 80, 48, 4, "make the sky red"
    cimg = Image.fromarray((np.random.default_rng(3).random((Hpx, Wpx, 3)) * 255).astype("uint8"))
    lat0 = torch.randn(1, (Hpx // 16) * (Wpx // 16), 64, generator=torch.Generator().manual_seed(9))

    def run():
        cond = Condition("subject", raw_img=cimg, position_delta=[0, -5])
        out = generate(model, model.flux_pipe, conditions=[cond], prompt=prompt, height=Hpx, width=Wpx, latents=lat0.cuda(),
                       num_inference_steps=steps, output_type="pt", model_config=model.model_config, default_lora=True,
                       use_brain_condition=False, fuse_flag=False)
        assert out.lx_operands == "fp16"
        return out.images.float().cpu()
    got_a = run()
    assert got_a.shape == (1, 3, Hpx, Wpx) and int(model.flux_pipe.vae.f16_ovf.item()) == 0
    model.flux_pipe.vae = lxvae.LxAutoencoderKL(vae.state_dict(), tiny_ckpt.VAE_CFG, "cuda")
    got_b = run()
    model.flux_pipe.vae = lxvae.LxAutoencoderKL(vae.state_dict(), tiny_ckpt.VAE_CFG, "cuda", precise=True)
    got_c = run()
    te = model.flux_pipe.text_encoder
    with torch.no_grad():
        pe = te.t5_sequence([prompt]).float().cpu()
        pooled = te.clip_pooled([prompt]).float().cpu()
        x = model.flux_pipe.image_processor.preprocess(cimg)
        z = (vae.encode(x).latent_dist.mean - vae.config.shift_factor) * vae.config.scaling_factor
        tokens = fm.pack_latents(z)
        ids = fm.prepare_latent_image_ids(Hpx // 16, Wpx // 16)
        cids = ids.clone()
        cids[:, 2] -= 5
        final = fr.denoise_loop(tr, fm.FlowMatchEulerDiscreteScheduler(), lat0, pe, pooled, torch.zeros(512, 3), ids, tokens, cids,
                                num_inference_steps=steps)
        img = vae.decode(fm.unpack_latents(final, Hpx, Wpx) / vae.config.scaling_factor + vae.config.shift_factor, return_dict=False)[0]
    want = (img / 2 + 0.5).clamp(0, 1)
    ea, eb, ec = relerr(got_a, want), relerr(got_b, want), relerr(got_c, want)
    print(f"generate 80x48 float16: relerr (a) fp16 VAE {ea:.3e}; (b) bf16-operand VAE {eb:.3e} (x{eb / ea:.1f}); (c) precise VAE {ec:.3e}")
    assert ea <= eb / 2.0, (ea, eb, ec)
    assert ea < 2.0 * P2P_MEASURED, (ea, P2P_MEASURED)
