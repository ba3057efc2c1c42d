"""The FLUX VAE in precise mode (LxAutoencoderKL(precise=True), what dtype=torch.float32 selects): the three pair-image row kernels of
csrc/vae.hip against float64, the mid-block attention on pairs against the oracle AttnBlock in float64, whole encode / decode against the
fp32 oracle beside the bf16-operand VAE on the same weights, and generate() from pixels to pixels with a float32 pipeline.

A pair image holds v as hi = bf16(v) at column c and lo = bf16(v - hi) at column lo_off + c; hi + lo carries v to 16 significand bits, so
the rounding floor of a pair is 2^-17 / sqrt(3) ... 2^-17 relative: about 2.5e-6 in the norm-wise statistic used here."""
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

DEV = "cuda"
bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


def _pad_to(n, m):
    return (n + m - 1) // m * m


def _nan_bits(t):
    """True where a bf16 tensor still holds the NaN it was filled with."""
    return torch.isnan(t.float())


# ---- 1. lx_groupnorm_silu_split -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [True, False], ids=["silu", "plain"])
@pytest.mark.parametrize("shape", [(2, 60, 128, 32), (1, 300, 512, 32), (1, 4100, 128, 32)], ids=lambda s: "B%d_P%d_C%d_G%d" % s)
def test_groupnorm_silu_split_vs_float64(ops, shape, silu):
    """GroupNorm (+ SiLU) of randn + 8 (mean / std = 8: E[x^2] - mean^2 in fp32 would lose a factor of 10-40 here) into a pair image with
    y_lo_off = C + 8 and ldy = y_lo_off + C + 8, against float64. Bound 2e-5, derived: a two-pass fp32 emulation gives 2.7e-6 ... 7.5e-6 on
    these shapes, the sum-of-squares form 7.1e-5 at P = 4100; the pair rounding floor is 2.5e-6. P = 1 / 16 / 64 row chunks, the last of
    the 64 ragged (4100 = 63 * 65 + 5). The NaN-filled gaps between and behind the halves must stay as they were."""
    B, P, C, G = shape
    x = rnd(B, P, C, seed=41) + 8.0
    g, b = 1.0 + 0.2 * rnd(C, seed=42), 0.3 * rnd(C, seed=43)
    lo, ldy = C + 8, 2 * C + 16
    y = torch.full((B * P, ldy), float("nan"), dtype=bf16, device=DEV)
    ops.groupnorm_silu_split(x.to(DEV), g.to(DEV), b.to(DEV), y, lo, G, 1e-6, silu)
    torch.cuda.synchronize()
    want = F.group_norm(x.double().transpose(1, 2), G, g.double(), b.double(), 1e-6).transpose(1, 2)
    if silu:
        want = F.silu(want)
    y = y.cpu()
    got = y[:, :C].double() + y[:, lo:lo + C].double()
    err = relerr(got, want.reshape(B * P, C))
    print(f"groupnorm_silu_split {shape} silu={silu}: relerr {err:.3e}")
    assert err < 2e-5
    assert bool(_nan_bits(y[:, C:lo]).all()) and bool(_nan_bits(y[:, lo + C:]).all())


# ---- 2. lx_im2col3x3_split + a k_segs = 3 GEMM ------------------------------------------------------------------------------------------
def _conv_ref(x, w, mode):
    """float64 conv2d of NCHW x with the three gathers of lx_im2col3x3."""
    if mode == 1:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    if mode == 2:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return F.conv2d(x, w, padding=1)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C", [3, 16, 128])
def test_im2col3x3_split_gemm_vs_float64_conv(ops, C, mode):
    """fp32 inputs and weights with full fp32 mantissas, B = 2, 6x10 pixels (mode 1: -> 3x5, mode 2: -> 12x20), 16 output channels. The
    input pair comes from lx_split_bf16 (C = 3: four fp32 channels with the last zero, lo_off = 8, ld = 16 -- the encoder's conv_in; C = 16
    with a gap: lo_off = 24, ld = 48), the rows from lx_im2col3x3_split, the product from a k_segs = 3 launch on [W_hi | W_lo]. Bound 2e-5,
    derived: the three-term product emulates at 4.4e-6 (K = 1152, 4608); the bf16 product on such data is 2.3e-3. The pad columns of both
    halves are exactly zero and rows of `cols` behind the last output pixel keep their NaN."""
    B, H, W, Co = 2, 6, 10, 16
    x = rnd(B, C, H, W, seed=50 + C)
    w = rnd(Co, C, 3, 3, seed=51 + C) / (3.0 * C ** 0.5)
    Ho, Wo = (H // 2, W // 2) if mode == 1 else ((2 * H, 2 * W) if mode == 2 else (H, W))
    rows, Kp = B * Ho * Wo, _pad_to(9 * C, 64)
    Cs = _pad_to(C, 4)
    lo, ld = {3: (8, 16), 16: (24, 48), 128: (128, 256)}[C]
    xs = torch.zeros(B * H * W, Cs)
    xs[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    pair = torch.full((B * H * W, ld), float("nan"), dtype=bf16, device=DEV)
    ops.split_bf16(xs.to(DEV), pair, lo)
    cols = torch.full((rows + 3, 2 * Kp), float("nan"), dtype=bf16, device=DEV)
    ops.im2col3x3_split(pair.view(B, H, W, ld), C, lo, cols[:rows], mode)
    wm = w.permute(0, 2, 3, 1).reshape(Co, 9 * C)
    wh = wm.to(bf16)
    Wp = torch.zeros(Co, 2 * Kp, dtype=bf16)
    Wp[:, :9 * C], Wp[:, Kp:Kp + 9 * C] = wh, (wm - wh.float()).to(bf16)
    assert bool((Wp[:, Kp:] != 0).any())                                                     # the weights do have a bf16 residual
    out = torch.empty(rows, Co, dtype=torch.float32, device=DEV)
    ops.gemm([ops.gemm_desc(cols[:rows], Wp.to(DEV), out, epilogue=ops.LX_EPI_STORE_F32, N=Co, K=Kp, k_segs=3, a_lo_off=Kp)])
    torch.cuda.synchronize()
    want = _conv_ref(x.double(), w.double(), mode).permute(0, 2, 3, 1).reshape(rows, Co)
    err = relerr(out.cpu(), want)
    print(f"im2col3x3_split C={C} mode={mode}: relerr {err:.3e}")
    assert err < 2e-5
    cols = cols.cpu()
    for half in (0, 1):
        padc = cols[:rows, half * Kp + 9 * C:(half + 1) * Kp]
        assert padc.shape[1] == Kp - 9 * C and torch.equal(padc, torch.zeros_like(padc))    # (C = 128: 9 C = Kpad, no pad columns)
        assert bool(torch.isfinite(cols[:rows, half * Kp:half * Kp + 9 * C].float()).all())
    assert bool(_nan_bits(cols[rows:]).all())


# ---- 3. lx_softmax_rows_split ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=lambda c: "M%d_valid%d_store%d_lds%d_ldp%d_off%d" % c)
def test_softmax_rows_split(ops, case):
    """The cases of test_softmax_rows_valid with a pair output: the lo half starts p_lo_off = roundup(n_store, 8) + 8 columns in (a gap of
    8 ... 15 sentinel columns behind the hi half) and the row keeps the case's tail behind it, so ldp = 70 still is no multiple of 4
    (scalar accesses) and the others stay multiples of 4. The pad columns of S hold NaN. Bound 2e-5 against float64, derived: pair floor
    2.5e-6 plus __expf on arguments down to about -80."""
    M, nv, ns, lds, ldp, off = case
    plo = _pad_to(ns, 8) + 8
    ld = plo + ns + (ldp - ns)
    host = _nan((M, lds))
    host[:, :nv] = rnd(M, nv, seed=6, scale=3.0)
    flat = torch.empty(M * lds + off, dtype=torch.float32, device=DEV)
    S = flat[off:].view(M, lds)
    S.copy_(host)
    Pm = torch.full((M, ld), SENTINEL, dtype=bf16, device=DEV)
    ops.softmax_rows_split(S, Pm, 0.25, nv, ns, plo)
    torch.cuda.synchronize()
    Pm = Pm.cpu()
    want = torch.softmax(host[:, :nv].double() * 0.25, -1)
    err = relerr(Pm[:, :nv].double() + Pm[:, plo:plo + nv].double(), want)
    print(f"softmax_rows_split {case} p_lo_off={plo} ld={ld}: relerr {err:.3e}")
    assert err < 2e-5
    for h0 in (0, plo):
        z = Pm[:, h0 + nv:h0 + ns]
        assert torch.equal(z, torch.zeros_like(z)) and not torch.signbit(z.float()).any()   # +0, not -0
    sent = torch.full((M, 1), SENTINEL, dtype=bf16)
    assert torch.equal(Pm[:, ns:plo], sent.expand(M, plo - ns)) and torch.equal(Pm[:, plo + ns:], sent.expand(M, ld - plo - ns))


# ---- 4. the attention branch on pairs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [9, 63, 64, 65, 240])
def test_attn_precise_vs_float64_oracle(ops, P):
    """out - x of _attn with precise=True against the oracle AttnBlock in float64 (same weights, B = 2, C = 128; 64 takes Ppad == P, the
    others a padded key axis). Bound 4e-5, derived: emulated 8.4e-6 at C = 128, P = 65 and 7.1e-6 at C = 512, P = 240; the bf16 branch is at
    4-5e-3."""
    from loongx_amd.vae import LxAutoencoderKL
    B, C = 2, 128
    ref = ovae.init_synthetic_(ovae.AttnBlock(C), 21)
    lx = LxAutoencoderKL({"a." + k: v for k, v in ref.state_dict().items()}, SMALL, DEV, precise=True)
    x = rnd(B * P, C, seed=22 + P) + 0.2
    got = _attn_branch(lx, x, B, P)
    ref = ref.double()
    with torch.no_grad():
        x4 = x.double().view(B, P, 1, C).permute(0, 3, 1, 2)
        want = (ref(x4) - x4).permute(0, 2, 3, 1).reshape(B * P, C)
    err = relerr(got, want)
    print(f"_attn precise P={P}: relerr {err:.3e}")
    assert err < 4e-5


# ---- 5. whole encoder and decoder ----------------------------------------------------------------------------------------------------------
def _models(cfg, bf16_weights=False):
    from loongx_amd.vae import LxAutoencoderKL
    ref = ovae.init_synthetic_(ovae.AutoencoderKL(**cfg), 3)
    if bf16_weights:
        ref.load_state_dict({k: v.to(bf16).to(v.dtype) for k, v in ref.state_dict().items()})
    sd = ref.state_dict()
    return ref, LxAutoencoderKL(sd, cfg, DEV, precise=True), LxAutoencoderKL(sd, cfg, DEV, precise=False)


@pytest.fixture(scope="module")
def small_models(ops):
    return _models(SMALL)


@pytest.fixture(scope="module")
def small_models_bf16_weights(ops):
    return _models(SMALL, bf16_weights=True)


@pytest.fixture(scope="module")
def full_models(ops):
    return _models({})


def _stats(lx, img, noise, z, want, wimg):
    got = lx.encode(img.to(DEV)).latent_dist
    gimg = lx.decode(z.to(DEV), return_dict=False)[0]
    assert gimg.shape == wimg.shape and gimg.dtype == torch.float32 and got.mean.dtype == torch.float32
    assert torch.equal(gimg, lx.decode(z.to(DEV)).sample)                                   # a second decode: the same bits
    return (relerr(got.mean.cpu(), want.mean), relerr(got.std.cpu(), want.std),
            relerr(got.sample(noise=noise.to(DEV)).cpu(), want.sample(noise=noise)), relerr(gimg.cpu(), wimg))


def _precise_vs_oracle(models, H, W, bounds, label):
    ref, lxp, lxb = models
    nd = len(ref.config.block_out_channels) - 1
    h, w = H >> nd, W >> nd
    img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(1)) * 2 - 1       # test_vae_encode_decode_vs_oracle's inputs
    noise = torch.randn(2, 16, h, w, generator=torch.Generator().manual_seed(2))
    z = torch.randn(2, 16, h, w, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = ref.encode(img).latent_dist
        wimg = ref.decode(z, return_dict=False)[0]
    ep = _stats(lxp, img, noise, z, want, wimg)
    eb = _stats(lxb, img, noise, z, want, wimg)
    names = ("mean", "std", "sample", "image")
    print(f"VAE precise {label} {H}x{W} ({h * w} tokens): " + " ".join(f"{n} {p:.3e} (bf16 {b:.3e}, x{b / p:.0f})" for n, p, b in zip(names, ep, eb)))
    for n, p, b, bound in zip(names, ep, eb, bounds):
        assert p <= 1e-4, (n, p)                    # 4x the emulation's worst figure (2.44e-5)
        assert p <= b / 30.0, (n, p, b)             # eight more operand mantissa bits are a factor of 256; the emulation shows about 500
        assert p < bound, (n, p, bound)


# 2 x the figures measured on MI355X, per statistic (mean, std, sample, image); the figures stand in each test's docstring
B_SMALL_32 = (2.7e-5, 5.5e-6, 1.11e-5, 2.7e-5)
B_SMALL_18x14 = (2.6e-5, 5.3e-6, 1.06e-5, 2.74e-5)
B_SMALL_BF16W = (1.45e-5, 3.04e-6, 6.05e-6, 1.54e-5)
B_FULL_64 = (3.9e-5, 8.5e-6, 1.56e-5, 5.05e-5)
B_FULL_40x56 = (4.2e-5, 8.3e-6, 1.69e-5, 5.1e-5)


def test_vae_precise_small_32x32(small_models):
    """Two-level VAE at 32x32 (256 tokens), the oracle's fp32 weights as they are: every tensor has bf16 residuals, so every GEMM is a
    k_segs = 3 launch. Emulated on the CPU: mean 1.32e-5, std 2.7e-6, image 1.31e-5. Measured on MI355X: mean 1.337e-5, std 2.740e-6,
    sample 5.549e-6, image 1.337e-5 (the bf16-operand VAE beside it: 6.87e-3, 1.46e-3, 2.85e-3, 7.01e-3: 514 ... 531 times those)."""
    assert all(v == 3 for k, v in small_models[1].w.items() if k.endswith(".segs"))
    _precise_vs_oracle(small_models, 32, 32, B_SMALL_32, "small")


def test_vae_precise_small_18x14(small_models):
    """... at 18x14: a 9x7 latent, 63 tokens, the padded key axis. Emulated: mean 1.28e-5, std 2.5e-6, image 1.36e-5. Measured on MI355X:
    mean 1.287e-5, std 2.640e-6, sample 5.301e-6, image 1.370e-5 (533 ... 538 times below the bf16-operand VAE)."""
    _precise_vs_oracle(small_models, 18, 14, B_SMALL_18x14, "small")


def test_vae_precise_small_bf16_weights(small_models_bf16_weights):
    """The state dict rounded to bf16 on both sides (what a FLUX.1 checkpoint holds): every tensor packs as today and launches with
    k_segs = 2, except to_v (the A operand of v^T = Wv n^T, always [W_hi | W_lo]). Measured on MI355X: mean 7.265e-6, std 1.520e-6,
    sample 3.024e-6, image 7.680e-6 (653 ... 685 times below the bf16-operand VAE on the same weights)."""
    _, lxp, _ = small_models_bf16_weights
    segs = {k: v for k, v in lxp.w.items() if k.endswith(".segs")}
    assert segs and all(v == (3 if k.endswith(".to_v.segs") else 2) for k, v in segs.items()), segs
    _precise_vs_oracle(small_models_bf16_weights, 32, 32, B_SMALL_BF16W, "small, bf16 weights")


def test_vae_precise_full_64x64(full_models):
    """The full FLUX.1 VAE shape at 64x64 (64 tokens). Emulated: mean 1.97e-5, std 4.3e-6, image 2.44e-5. Measured on MI355X: mean 1.946e-5,
    std 4.243e-6, sample 7.797e-6, image 2.524e-5 (503 ... 568 times below the bf16-operand VAE: 1.09e-2, 2.23e-3, 4.43e-3, 1.27e-2)."""
    _precise_vs_oracle(full_models, 64, 64, B_FULL_64, "full")


def test_vae_precise_full_40x56(full_models):
    """The full shape at 40x56: a 5x7 latent, 35 tokens. Measured on MI355X: mean 2.099e-5, std 4.153e-6, sample 8.439e-6, image 2.548e-5
    (497 ... 527 times below the bf16-operand VAE)."""
    _precise_vs_oracle(full_models, 40, 56, B_FULL_40x56, "full")


def test_precise_decode_ignores_stale_scratch(small_models):
    """As test_decode_ignores_stale_scratch: the pair buffers' pad rows and columns are zero-filled or never read, so a decode after the
    caching allocator was seeded with NaN blocks gives the same bits as before."""
    lx = small_models[1]
    z = rnd(2, 16, 9, 7, seed=31).to(DEV)
    before = lx.decode(z, return_dict=False)[0].clone()
    torch.cuda.synchronize()
    junk = [torch.full((n,), float("nan"), dtype=torch.float32, device=DEV) for n in (1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24, 1 << 25)]
    junk += [torch.full((n,), float("nan"), dtype=bf16, device=DEV) for n in (63 * 128, 63 * 512, 126 * 512, 190 * 512, 256 * 128, 1 << 21, 1 << 22)] * 4
    torch.cuda.synchronize()
    del junk
    after = lx.decode(z, return_dict=False)[0]
    assert bool(torch.isfinite(before).all()) and bool(torch.isfinite(after).all())
    assert torch.equal(before, after)


# ---- 6. precise=False is what it was ---------------------------------------------------------------------------------------------------------
def test_precise_false_is_the_default_vae(ops):
    from loongx_amd.vae import LxAutoencoderKL
    sd = ovae.init_synthetic_(ovae.AutoencoderKL(**SMALL), 3).state_dict()
    a, b = LxAutoencoderKL(sd, SMALL, DEV), LxAutoencoderKL(sd, SMALL, DEV, precise=False)
    assert a.precise is False and b.precise is False and a.dtype == torch.float32
    assert a.w.keys() == b.w.keys() and not any(k.endswith(".segs") for k in a.w)
    for k, v in a.w.items():
        if k.endswith(".w"):
            co, ci, kh = a.w[k[:-2] + ".shape"]
            assert v.dtype == bf16 and v.shape == (_pad_to(co, 8), _pad_to(kh * kh * ci, 64)), (k, v.shape)     # no [W_hi | W_lo] image
            assert torch.equal(v, b.w[k])
    img = (torch.rand(2, 3, 18, 14, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    z = rnd(2, 16, 9, 7, seed=3).to(DEV)
    assert torch.equal(a.decode(z).sample, b.decode(z).sample)
    assert torch.equal(a.encode(img).latent_dist.mean, b.encode(img).latent_dist.mean)


# ---- 7. selection ----------------------------------------------------------------------------------------------------------------------------
def test_from_pretrained_float32_selects_the_precise_vae(ops, tmp_path):
    from loongx_amd.flux.pipeline import LxFluxPipeline
    d = str(tmp_path / "flux_tiny")
    tiny_ckpt.build_flux_dir(d, with_text=False)
    p32 = LxFluxPipeline.from_pretrained(d, dtype=torch.float32, load_text_encoders=False)
    assert p32.vae.precise is True and p32.vae.dtype == torch.float32
    assert LxFluxPipeline.from_pretrained(d, dtype=torch.bfloat16, load_text_encoders=False).vae.precise is False


# ---- 8. pixels to pixels ----------------------------------------------------------------------------------------------------------------------
P2P_BOUND = 9.3e-6       # 2 x the figure measured on MI355X: see the docstring


def test_generate_80x48_float32_pixels_to_pixels(ops, tmp_path, monkeypatch):
    """The chain of test_generate_80x48_pil_to_pil_matches_oracle_chain with OminiModel(dtype=torch.float32) and output_type="pt": the
    condition photo goes through the precise VAE encoder, the precise DiT denoises, the precise decoder makes the pixels. Compared with the
    oracle chain (relative error over the [0, 1] image), and with the same run after pipe.vae was swapped for a precise=False instance of
    the same weights: the float32 pipeline must be at least 20 times closer, which is what the user of dtype=float32 sees of the change. Measured on MI355X: 4.629e-6, and
    2.424e-3 with the bf16-operand VAE (524 times that)."""
    from PIL import Image
    from loongx_amd import vae as lxvae
    from src.flux.condition import Condition
    from src.flux.generate import generate
    from src.train.model import OminiModel
    d = str(tmp_path / "flux_tiny")
    tr, vae = tiny_ckpt.build_flux_dir(d)
    sd, _ = tiny_ckpt.loongx_state_dict(tr)
    monkeypatch.setattr(lxvae.DiagonalGaussianDistribution, "sample", lambda self, generator=None, noise=None: self.mean)
    model = OminiModel(flux_pipe_id=d, lora_config={"r": 4, "lora_alpha": 4}, device="cuda", dtype=torch.float32, model_config={})
    model.load_state_dict(sd)
    assert model.flux_pipe.vae.precise is True
    Wpx, Hpx, steps, prompt = 80, 48, 4, "make the sky red"
    cimg = Image.fromarray((np.random.default_rng(3).random((Hpx, Wpx, 3)) * 255).astype("uint8"))
    lat0 = torch.randn(1, (Hpx // 16) * (Wpx // 16), 64, generator=torch.Generator().manual_seed(9))

    def run():
        cond = Condition("subject", raw_img=cimg, position_delta=[0, -5])
        out = generate(model, model.flux_pipe, conditions=[cond], prompt=prompt, height=Hpx, width=Wpx, latents=lat0.cuda(),
                       num_inference_steps=steps, output_type="pt", model_config=model.model_config, default_lora=True,
                       use_brain_condition=False, fuse_flag=False).images
        return out.float().cpu()
    got = run()
    assert got.shape == (1, 3, Hpx, Wpx)
    model.flux_pipe.vae = lxvae.LxAutoencoderKL(vae.state_dict(), tiny_ckpt.VAE_CFG, "cuda", precise=False)
    got_bf16_vae = run()
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
    e32, e16 = relerr(got, want), relerr(got_bf16_vae, want)
    print(f"generate 80x48 float32: relerr {e32:.3e}; with the bf16-operand VAE {e16:.3e} (x{e16 / e32:.0f})")
    assert e32 <= e16 / 20.0, (e32, e16)
    assert e32 < P2P_BOUND, e32
