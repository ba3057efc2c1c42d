"""The float64 references that tests/test_cs3_tiles_gpu.py holds the CS3 / DGF kernels to (tests/helpers.py), checked on the CPU against
what they restate: the staged DUAN against oracle.cs3.DUAN in fp32 and against the goldens made by the real reference class; the FFT form
of the S4 convolution against the direct sum; the pooling, channel-mix and LayerNorm references against torch's own operators; and the
seeds of the full-size kept-set check against the condition the GPU test relies on (at most 1 % of the channels undecided)."""
import numpy as np
import pytest
import torch

from oracle import cs3, s4
from tests import helpers as H
from tests.helpers import load, relerr

F32_ROUNDING = 2e-5        # the project's DUAN bound against an fp32 evaluation (tests/test_kernels_gpu.py::test_duan_golden)


def _same_kept(y, ref):
    return torch.equal(y.abs().sum(2) > 0, ref.abs().sum(2) > 0)


@pytest.mark.parametrize("C,Hd,B,L,seed", [(1, 128, 2, 768, 0), (6, 128, 3, 130, 1), (16, 64, 2, 200, 2), (128, 128, 2, 260, 3),
                                           (256, 128, 2, 68, 4)])
def test_staged_duan_reproduces_the_fp32_oracle(C, Hd, B, L, seed):
    d, x, c = H.duan_case(C, Hd, B, L, seed)
    keep_k = max(1, int(C * 0.7))
    with torch.no_grad():
        want = d(x, c)
    st = H.duan_ref_stages(x, c, H.duan_params(d), keep_k, d.eps)
    undecided = H.kept_set_margin(st["imp"], keep_k, H.DUAN_KEPT_DELTA)
    assert not bool(undecided.any())                     # (these seeds have no near-tie: fp32 and float64 must keep the same channels)
    assert _same_kept(st["y"], want)
    assert relerr(st["y"], want) < F32_ROUNDING
    # the stages are consistent with one another: tile sums add up to the means the coefficients take
    assert torch.allclose(st["cpart"].sum(1) / L, st["cmean"], rtol=1e-12, atol=1e-14)
    assert st["gpart"].shape == (B, (L + 63) // 64, C) and st["hid"].shape == (B, Hd, L)


@pytest.mark.parametrize("name,C", [("c16", 16), ("c1", 1), ("c512", 512)])
def test_staged_duan_reproduces_the_goldens(name, C):
    G = load("cs3_dgf.npz")
    seed, hid = [int(v) for v in G[f"duan_{name}_seed"]]
    torch.manual_seed(seed)
    d = cs3.DUAN(C, hidden_dim=hid)
    st = H.duan_ref_stages(G[f"duan_{name}_x"], G[f"duan_{name}_c"], H.duan_params(d), max(1, int(C * 0.7)), d.eps)
    ref = G[f"duan_{name}_y"]
    assert _same_kept(st["y"], ref)
    assert relerr(st["y"], ref) < F32_ROUNDING


def test_tie_case_straddles_the_boundary_and_the_stable_sort_keeps_the_lower_index():
    d, x, c, keep_k = H.duan_tie_case()
    st = H.duan_ref_stages(x, c, H.duan_params(d), keep_k, d.eps)
    imp = st["imp"]
    for i in range(4):
        for r in range(1, 4):
            assert torch.equal(imp[:, i], imp[:, i + 4 * r])                  # bit-equal even in float64
    for b in range(imp.shape[0]):
        s = imp[b].sort(descending=True).values
        assert s[keep_k - 1] == s[keep_k] and s[3] > s[4] and s[7] > s[8]     # the cut is inside the second group of four
        second = sorted(int(i) for i in (imp[b] == s[keep_k]).nonzero().flatten())
        kept = set(int(i) for i in st["keep"][b].nonzero().flatten())
        assert len(kept) == keep_k and second[0] in kept and second[1] in kept and second[2] not in kept and second[3] not in kept


@pytest.mark.parametrize("C,L,seed,keep_k", H.DUAN_KEPT_CASES)
def test_full_size_seeds_leave_at_most_one_percent_undecided(C, L, seed, keep_k):
    d, x, c = H.duan_case(C, 128, 2, L, seed)
    st = H.duan_ref_stages(x, c, H.duan_params(d), keep_k, d.eps)
    undecided = H.kept_set_margin(st["imp"], keep_k, H.DUAN_KEPT_DELTA)
    print("undecided channels per batch element:", undecided.sum(1).tolist())
    assert int(undecided.sum(1).max()) <= C // 100
    assert bool((st["keep"].sum(1) == keep_k).all())


@pytest.mark.parametrize("Hc,N,L", [(4, 4, 64), (6, 6, 256), (64, 64, 128)])
def test_fft_convolution_equals_the_direct_sum(Hc, N, L):
    lay = s4.S4Layer(Hc, N, L, torch.Generator().manual_seed(3))
    pr = lay.params_np()
    K = s4.kernel_genfunc(pr, L)
    u = torch.randn(3, Hc, L, generator=torch.Generator().manual_seed(4)).numpy()
    want = s4.causal_conv_direct(u.transpose(0, 2, 1), K, pr["D"]).transpose(0, 2, 1)
    got = H.s4_fft_conv(u, K, pr["D"])
    assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())


def test_small_references_match_torch():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 50, generator=g)
    for sizes in ([7], [64, 3, 50], [128]):               # a size > L repeats samples, as nn.AdaptiveAvgPool1d does
        want = torch.cat([torch.nn.functional.adaptive_avg_pool1d(x.double(), s) for s in sizes], -1)
        assert torch.allclose(H.pyramid_pool_ref(x, sizes), want, rtol=1e-13, atol=1e-15)
    xi, W, b, res = torch.randn(2, 6, 33, generator=g), torch.randn(6, 6, generator=g), torch.randn(6, generator=g), torch.randn(2, 6, 33, generator=g)
    lg, lb = torch.randn(6, generator=g), torch.randn(6, generator=g)
    z = torch.einsum("oi,bil->bol", W.double(), torch.nn.functional.gelu(xi.double())) + b.double()[None, :, None] + res.double()
    want = torch.nn.functional.layer_norm(z.permute(0, 2, 1), (6,), lg.double(), lb.double(), 1e-5).permute(0, 2, 1)
    assert torch.allclose(H.chanmix_ref(xi, W, b, res, lg, lb, act=1), want, rtol=1e-12, atol=1e-13)
    xr, gg, bb = torch.randn(5, 100, generator=g) + 1e3, torch.randn(100, generator=g), torch.randn(100, generator=g)
    want = torch.relu(torch.nn.functional.layer_norm(xr.double(), (100,), gg.double(), bb.double(), 1e-5))
    assert torch.allclose(H.layernorm_relu_ref(xr, gg, bb), want, rtol=1e-10, atol=1e-11)
    z, mag = H.chan_gemm_ref(xi, W, b)
    assert torch.allclose(z, torch.einsum("oi,bil->bol", W.double(), xi.double()) + b.double()[None, :, None]) and bool((mag >= z.abs() - 1e-12).all())
    assert torch.equal(H.tile_sums(torch.ones(1, 2, 130, dtype=torch.float64)), torch.tensor([[[64., 64.], [64., 64.], [2., 2.]]], dtype=torch.float64))
