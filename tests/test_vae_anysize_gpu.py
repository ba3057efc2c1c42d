"""The FLUX VAE at image sizes whose latent grid is no multiple of 64 tokens: lx_softmax_rows_valid (csrc/vae.hip), the padded key axis of
LxAutoencoderKL._attn, whole encode / decode against the oracle (oracle/vae.py), and generate() from pixels to pixels at 80x48."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import flux_modules as fm  # noqa: E402
from oracle import flux_ref as fr  # noqa: E402
from oracle import vae as ovae  # noqa: E402
from tests import tiny_ckpt  # noqa: E402
from tests.helpers import relerr  # noqa: E402

DEV = "cuda"
SMALL = dict(in_channels=3, out_channels=3, latent_channels=16, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
# (M, n_valid, n_store, lds, ldp, first column of S inside its allocation). Row strides that are multiples of 4 elements on an aligned base
# take the 16 / 8 B accesses, the others (lds = 67, ldp = 70; a base one float off) the scalar ones; (6, 37, 50) ends both the valid and
# the stored columns off a multiple of 4 on the vector path.
SOFTMAX_CASES = [(5, 1, 64, 64, 64, 0), (3, 63, 64, 67, 70, 0), (7, 65, 128, 128, 136, 0), (4, 240, 256, 256, 256, 0),
                 (2, 4100, 4160, 4160, 4168, 0), (6, 37, 50, 52, 56, 0), (5, 65, 128, 132, 128, 1)]
SENTINEL = -7.0


def _softmax_run(ops, case, poison):
    M, nv, ns, lds, ldp, off = case
    host = poison((M, lds))
    host[:, :nv] = rnd(M, nv, seed=6, scale=3.0)
    flat = torch.empty(M * lds + off, dtype=torch.float32, device=DEV)
    S = flat[off:].view(M, lds)                                  # off = 1: rows that start 4 bytes off a 16-byte boundary
    S.copy_(host)
    Pfull = torch.full((M, ldp), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.softmax_rows(S, Pfull[:, :ns], 0.25, n_valid=nv)
    torch.cuda.synchronize()
    return S[:, :nv], Pfull


def _nan(shape):
    return torch.full(shape, float("nan"))


def _inf_and_huge(shape):
    t = torch.full(shape, float("inf"))
    t.view(-1)[1::2] = 1e30
    return t


@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=lambda c: "M%d_valid%d_store%d_lds%d_ldp%d_off%d" % c)
def test_softmax_rows_valid(ops, case):
    """softmax over the first n_valid columns, exact zeros up to n_store, nothing written beyond; the pad columns of S are poisoned (NaN in
    one run, +inf / 1e30 in the other) and must not reach the maximum, the sum or the output. 4e-3 is test_softmax_rows' bound (one bf16
    rounding of a probability)."""
    M, nv, ns, lds, ldp, off = case
    Sv, Pa = _softmax_run(ops, case, _nan)
    _, Pb = _softmax_run(ops, case, _inf_and_huge)
    want = torch.softmax(Sv.float() * 0.25, -1)
    err = relerr(Pa[:, :nv].float(), want)
    print(f"softmax_rows_valid {case}: relerr {err:.3e}")
    assert err < 4e-3
    assert torch.equal(Pa[:, nv:ns], torch.zeros(M, ns - nv, dtype=torch.bfloat16, device=DEV))
    assert not torch.signbit(Pa[:, nv:ns].float()).any()                                    # +0, not -0
    assert torch.equal(Pa.view(torch.int16), Pb.view(torch.int16))                          # the two poisons: bit-equal outputs
    assert torch.equal(Pa[:, ns:], torch.full((M, ldp - ns), SENTINEL, dtype=torch.bfloat16, device=DEV))


# ---- _attn ----------------------------------------------------------------------------------------------------------------------
def _attn_pair(C, seed, uniform_b=None):
    """oracle AttnBlock(C) with seeded weights and the HIP VAE holding the same weights under the prefix "a"."""
    from loongx_amd.vae import LxAutoencoderKL
    ref = ovae.init_synthetic_(ovae.AttnBlock(C), seed)
    if uniform_b is not None:
        with torch.no_grad():
            ref.to_q.weight.zero_()
            ref.to_k.weight.zero_()
            ref.to_q.bias.fill_(-uniform_b)
            ref.to_k.bias.fill_(uniform_b)
    lx = LxAutoencoderKL({"a." + k: v for k, v in ref.state_dict().items()}, SMALL, DEV)
    return ref, lx


def _attn_branch(lx, x, B, P):
    """out - x of LxAutoencoderKL._attn (which accumulates into its fp32 input) for x [B*P, C] fp32."""
    xin = x.to(DEV).contiguous()
    out = lx._attn(xin.clone(), B, P, "a")
    torch.cuda.synchronize()
    return (out - xin).cpu()


@pytest.mark.parametrize("P", [63, 65])
def test_attn_uniform_scores_ignore_pad_keys(ops, P):
    """Zero to_q / to_k weights with biases -b / +b: every real score is -C b^2 (scaled: -11.3), so attention is the mean of the value rows.
    A zero pad key would score 0 and take e^11.3 / (e^11.3 + P) of the weight: the output would be off by order 1."""
    B, C, b = 2, 128, 1.0
    ref, lx = _attn_pair(C, seed=11, uniform_b=b)
    x = rnd(B * P, C, seed=12) + 0.3
    got = _attn_branch(lx, x, B, P)
    with torch.no_grad():
        n = ref.group_norm(x.view(B, P, C).transpose(1, 2)).transpose(1, 2)                 # [B, P, C]
        vmean = ref.to_v(n).mean(1, keepdim=True)
        want = ref.to_out[0](vmean).expand(B, P, C).reshape(B * P, C)
    err = relerr(got, want)
    print(f"uniform scores P={P}: relerr {err:.3e}")
    assert err < 1e-2


ATTN_BOUND = 7.4e-3      # 2 x the larger figure of the two unpadded sizes: see test_attn_ragged_vs_oracle


def _attn_vs_oracle(P, B=2, C=128):
    ref, lx = _attn_pair(C, seed=21)
    x = rnd(B * P, C, seed=22 + P) + 0.2
    got = _attn_branch(lx, x, B, P)
    with torch.no_grad():
        x4 = x.view(B, P, 1, C).permute(0, 3, 1, 2)                                         # [B, C, P, 1]
        want = (ref(x4) - x4).permute(0, 2, 3, 1).reshape(B * P, C)
    return relerr(got, want)


@pytest.mark.parametrize("P", [9, 35, 63, 65, 240])
def test_attn_ragged_vs_oracle(ops, P):
    """The branch out - x of _attn against the oracle's AttnBlock (fp32) with the same weights, B = 2, C = 128. The bound comes from the
    sizes that take the unpadded launches, measured on MI355X with this file's _attn_vs_oracle (same generator, same statistic):
    P = 64: 3.70e-3, P = 256: 2.98e-3. The ragged sizes get 2 x the larger of the two (the project's usual factor; fewer keys average
    less rounding, so the unpadded figure itself would be too tight): 7.4e-3. Measured there: P = 9: 5.36e-3, 35: 3.89e-3, 63: 3.80e-3,
    65: 3.75e-3, 240: 3.01e-3. At 7.4e-3 a single pad key taking part at P = 63 could pass unnoticed here:
    test_attn_uniform_scores_ignore_pad_keys is the guard against that."""
    err = _attn_vs_oracle(P)
    print(f"_attn vs oracle P={P}: relerr {err:.3e}")
    assert err < ATTN_BOUND


# ---- whole VAE ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_pair(ops):
    from loongx_amd.vae import LxAutoencoderKL
    ref = ovae.init_synthetic_(ovae.AutoencoderKL(**SMALL), 3)
    return ref, LxAutoencoderKL(ref.state_dict(), SMALL, DEV)


@pytest.fixture(scope="module")
def full_pair(ops):
    from loongx_amd.vae import LxAutoencoderKL
    ref = ovae.init_synthetic_(ovae.AutoencoderKL(), 3)
    return ref, LxAutoencoderKL(ref.state_dict(), {}, DEV)


def test_decode_ignores_stale_scratch(small_pair):
    """The attention's pad rows and columns are zero-filled or never read, never torch.empty memory: a decode after the caching allocator
    was seeded with NaN blocks of every size gives the same bits as before."""
    _, lx = small_pair
    z = rnd(2, 16, 9, 7, seed=31).to(DEV)
    before = lx.decode(z, return_dict=False)[0].clone()
    torch.cuda.synchronize()
    junk = [torch.full((n,), float("nan"), dtype=torch.float32, device=DEV) for n in (1 << 8, 1 << 10, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24, 1 << 25)]
    junk += [torch.full((n,), float("nan"), dtype=torch.bfloat16, device=DEV) for n in (63 * 64, 63 * 256, 126 * 256, 190 * 256, 256 * 64, 1 << 21)] * 4
    torch.cuda.synchronize()
    del junk
    after = lx.decode(z, return_dict=False)[0]
    assert bool(torch.isfinite(before).all()) and bool(torch.isfinite(after).all())
    assert torch.equal(before, after)


def _encode_decode_vs_oracle(pair, full, H, W):
    b_mean, b_std, b_smp, b_img = (2e-2, 4.5e-3, 9e-3, 2e-2) if full else (1.4e-2, 3e-3, 6e-3, 1.4e-2)       # test_vae_encode_decode_vs_oracle's
    ref, lx = pair
    nd = len(ref.config.block_out_channels) - 1
    h, w = H >> nd, W >> nd
    img = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(1)) * 2 - 1
    with torch.no_grad():
        want = ref.encode(img).latent_dist
    got = lx.encode(img.to(DEV)).latent_dist
    assert got.mean.shape == (2, 16, h, w) and got.mean.dtype == torch.float32
    e_mean, e_std = relerr(got.mean.cpu(), want.mean), relerr(got.std.cpu(), want.std)
    noise = torch.randn(want.mean.shape, generator=torch.Generator().manual_seed(2))
    e_smp = relerr(got.sample(noise=noise.to(DEV)).cpu(), want.sample(noise=noise))
    assert torch.equal(got.mean, lx.encode(img.to(DEV)).latent_dist.mean)                   # deterministic
    z = torch.randn(2, 16, h, w, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        wimg = ref.decode(z, return_dict=False)[0]
    gimg = lx.decode(z.to(DEV), return_dict=False)[0]
    assert gimg.shape == (2, 3, H, W) and gimg.dtype == torch.float32
    e_img = relerr(gimg.cpu(), wimg)
    print(f"VAE {H}x{W} ({h * w} tokens, {'full' if full else 'small'}): mean {e_mean:.3e} std {e_std:.3e} sample {e_smp:.3e} image {e_img:.3e}")
    assert e_mean < b_mean and e_std < b_std and e_smp < b_smp and e_img < b_img
    assert torch.equal(gimg, lx.decode(z.to(DEV)).sample)                                   # deterministic


@pytest.mark.parametrize("H,W", [(18, 14), (10, 26), (24, 40)])
def test_vae_small_ragged_vs_oracle(small_pair, H, W):
    """Encoder and decoder of the two-level VAE at 63, 65 and 240 latent tokens against the fp32 oracle, with the bounds
    test_vae_encode_decode_vs_oracle uses for this configuration at 32x32."""
    _encode_decode_vs_oracle(small_pair, False, H, W)


def test_vae_full_ragged_vs_oracle(full_pair):
    """The full FLUX.1 VAE shape at 40x56 pixels: a 5x7 latent, 35 tokens in the mid-block attention; bounds as for 64x64."""
    _encode_decode_vs_oracle(full_pair, True, 40, 56)


def test_encode_rejects_sides_the_encoder_cannot_halve(small_pair, full_pair):
    with pytest.raises(ValueError, match="sides must be multiples of 2 "):
        small_pair[1].encode(torch.zeros(1, 3, 18, 15, device=DEV))
    with pytest.raises(ValueError, match="sides must be multiples of 8 "):
        full_pair[1].encode(torch.zeros(1, 3, 36, 56, device=DEV))


# ---- pixels to pixels -------------------------------------------------------------------------------------------------------------
def test_generate_80x48_pil_to_pil_matches_oracle_chain(ops, tmp_path, monkeypatch):
    """generate(height=48, width=80, output_type="pil") with a subject condition given as an 80x48 photo: the VAE (three halvings: a 6x10
    latent, 60 tokens) encodes the condition and decodes the result; the same chain on the oracle side, as
    test_inference_single_image_pil_to_pil_matches_oracle_chain builds it, with its bound."""
    from PIL import Image
    from loongx_amd import vae as lxvae
    from src.flux.condition import Condition
    from src.flux.generate import generate
    from src.train.model import OminiModel
    d = str(tmp_path / "flux_tiny")
    tr, vae = tiny_ckpt.build_flux_dir(d)
    sd, _ = tiny_ckpt.loongx_state_dict(tr)
    monkeypatch.setattr(lxvae.DiagonalGaussianDistribution, "sample", lambda self, generator=None, noise=None: self.mean)
    model = OminiModel(flux_pipe_id=d, lora_config={"r": 4, "lora_alpha": 4}, device="cuda", dtype=torch.bfloat16, model_config={})
    model.load_state_dict(sd)
    Wpx, Hpx, steps, prompt = 80, 48, 4, "make the sky red"
    cimg = Image.fromarray((np.random.default_rng(3).random((Hpx, Wpx, 3)) * 255).astype("uint8"))
    lat0 = torch.randn(1, (Hpx // 16) * (Wpx // 16), 64, generator=torch.Generator().manual_seed(9))

    def run():
        cond = Condition("subject", raw_img=cimg, position_delta=[0, -5])
        return generate(model, model.flux_pipe, conditions=[cond], prompt=prompt, height=Hpx, width=Wpx, latents=lat0.cuda(),
                        num_inference_steps=steps, output_type="pil", model_config=model.model_config, default_lora=True,
                        use_brain_condition=False, fuse_flag=False).images[0]
    out = run()
    assert out.size == (Wpx, Hpx) and out.mode == "RGB"
    assert np.array_equal(np.asarray(out), np.asarray(run()))
    te = model.flux_pipe.text_encoder
    with torch.no_grad():
        pe = te.t5_sequence([prompt]).float().cpu()
        pooled = te.clip_pooled([prompt]).float().cpu()
        x = model.flux_pipe.image_processor.preprocess(cimg)
        assert x.shape == (1, 3, Hpx, Wpx)
        z = (vae.encode(x).latent_dist.mean - vae.config.shift_factor) * vae.config.scaling_factor
        tokens = fm.pack_latents(z)
        ids = fm.prepare_latent_image_ids(Hpx // 16, Wpx // 16)
        cids = ids.clone()
        cids[:, 2] -= 5
        final = fr.denoise_loop(tr, fm.FlowMatchEulerDiscreteScheduler(), lat0, pe, pooled, torch.zeros(512, 3), ids, tokens, cids,
                                num_inference_steps=steps)
        img = vae.decode(fm.unpack_latents(final, Hpx, Wpx) / vae.config.scaling_factor + vae.config.shift_factor, return_dict=False)[0]
    want = (img / 2 + 0.5).clamp(0, 1)[0].permute(1, 2, 0).numpy()
    got = np.asarray(out).astype(np.float32) / 255.0
    diff = float(np.abs(got - want).mean())
    print(f"generate 80x48: mean absolute pixel difference {diff:.4f}")
    assert diff < 0.02, diff
