"""Pins the helpers tests/test_qkv_epilogue_tiles_gpu.py checks the kernels with (tests/helpers.py), on the CPU, so that the GPU test's
reference is not merely self-consistent: the float64 norm + RoPE against oracle.flux_modules, the V^T (de)interleave against the orders
spelled out in tests/test_kernels_gpu.py and include/lx.h, the restatement of the mixed plan's peel against the values csrc/gemm.hip's
loop gives for the test's launch shapes, and the share of elements an fp32 evaluation of the epilogue rounds differently from float64."""
import pytest
import torch

from oracle.flux_modules import RMSNorm, apply_rotary_emb, rope_tables
from tests.helpers import (QKV_D, QKV_DOUBLE, QKV_SINGLE, mixed_plan_keep_rows, qk_norm_rope_ref, qkv_double_shapes, qkv_epilogue_emulate_f32,
                           qkv_single_shape, rmsnorm_heads_ref, rope_pairs_ref, vt8_slot_keys, vt_interleave, vt_slot_keys, vt_stream_deinterleave)

H, D = 2, QKV_D
EMU_SHARE = 5e-4          # half of the GPU test's NEIGHBOUR_FRAC = 1e-3


def _table(L, shift=0):
    """rope_tables output for L positions on a 2-D grid, and the (cos, sin)-pair table [L, 128] the kernels take"""
    ids = torch.zeros(L, 3)
    ids[:, 1] = torch.arange(L) // 7 + shift
    ids[:, 2] = torch.arange(L) % 7 - 3
    cos, sin = rope_tables(ids)
    cs = torch.empty(L, 128)
    cs[:, 0::2], cs[:, 1::2] = cos[:, 0::2], sin[:, 0::2]
    return cos, sin, cs


def test_norm_and_rope_reference_equal_the_oracle():
    """B = 3 batch elements in row-major [B * L, D] order, and a row slice that starts inside an element (m_base % L != 0).
    oracle.apply_rotary_emb multiplies x.float(): it is given fp32-representable inputs, so its float64 arithmetic is exact to compare
    with (1e-13). oracle.RMSNorm computes the mean square in fp32, so it pins the norm to fp32 precision (1e-6); the float64 formula
    (x rsqrt(mean x^2 + eps) w per head, as tests/test_kernels_gpu.py restates block.py:60-67) pins it to 1e-13."""
    B, L = 3, 96
    g = torch.Generator().manual_seed(5)
    y = torch.randn(B * L, D, generator=g, dtype=torch.float64) * 1.3 + 0.1
    w = 1 + 0.1 * torch.randn(128, generator=g)
    cos, sin, cs = _table(L)
    # the norm
    x = rmsnorm_heads_ref(y, w)
    yh = y.view(B * L, H, 128)
    plain = (yh / torch.sqrt((yh * yh).sum(-1, keepdim=True) / 128 + 1e-6) * w.double()).view(B * L, D)
    assert float((x - plain).abs().max()) < 1e-13
    mod = RMSNorm(128)
    with torch.no_grad():
        mod.weight.copy_(w)
        xo = mod(yh.float()).double().view(B * L, D)
    assert float((x - xo).abs().max()) < 1e-6 * float(x.abs().max())
    # the rotation, on the fp32 image of the normalised rows
    x32 = x.float().double()
    got, mag = rope_pairs_ref(x32, cs, L)
    want = apply_rotary_emb(x32.view(B, L, H, 128).permute(0, 2, 1, 3), (cos.double(), sin.double())).permute(0, 2, 1, 3).reshape(B * L, D)
    assert want.dtype == torch.float64 and float((got - want).abs().max()) < 1e-13
    assert bool((mag >= got.abs() - 1e-15).all())
    # both in one call, and rows [m_base, m_base + n) of the stream
    full = qk_norm_rope_ref(y, w, cs, L)
    assert float((full - rope_pairs_ref(x, cs, L)[0]).abs().max()) == 0.0
    ref2 = apply_rotary_emb(x.float().double().view(B, L, H, 128).permute(0, 2, 1, 3), (cos.double(), sin.double()))
    assert float((full - ref2.permute(0, 2, 1, 3).reshape(B * L, D)).abs().max()) < 1e-6      # (x rounded to fp32 on the oracle's side)
    for m_base, n in ((64, 128), (160, 32), (L, L)):
        assert m_base % L != 0 or m_base == L
        part = qk_norm_rope_ref(y[m_base:m_base + n], w, cs, L, m_base)
        assert torch.equal(part, full[m_base:m_base + n])
    # a wrong position is a different result: the table's rows all differ
    assert float((qk_norm_rope_ref(y[64:96], w, cs, L, 0) - full[64:96]).abs().max()) > 1e-3
    # the error bound: non-negative, and zero input error leaves the roundings of the norm and the rotation only
    out, E = qk_norm_rope_ref(y, w, cs, L, 0, torch.zeros_like(y))
    assert torch.equal(out, full) and bool((E >= 0).all()) and float(E.max()) < 64 * 2.0 ** -23 * float(out.abs().max())
    _, E2 = qk_norm_rope_ref(y, w, cs, L, 0, 1e-4 * y.abs())
    assert bool((E2 >= E).all()) and float(E2.max()) > float(E.max())


@pytest.mark.parametrize("L", [128, 96, 160, 416])
def test_vt_deinterleave_inverts_both_key_orders(L):
    """L % 64 in {0, 32}. 16-bit image: slot s of every 16 holds key perm[s], the permutation tests/test_kernels_gpu.py::
    test_qkv_prep_rmsnorm_rope spells out. Byte image: byte j = g * 32 + p of a 64-key tile holds key (p >> 4) * 32 + 8 ((p & 15) >> 2) +
    4 g + (p & 3) (include/lx.h, qkv_vt8)."""
    assert L % 64 in (0, 32)
    n = (L + 63) // 64 * 64
    perm = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert vt_slot_keys(n).tolist() == [(s // 16) * 16 + perm[s % 16] for s in range(n)]
    want8 = []
    for j in range(n):
        t, g, p = j // 64, (j % 64) // 32, j % 32
        want8.append(t * 64 + (p >> 4) * 32 + 8 * ((p & 15) >> 2) + 4 * g + (p & 3))
    assert vt8_slot_keys(n).tolist() == want8 and sorted(want8) == list(range(n))
    v = torch.arange(3 * H * L * 128, dtype=torch.float32).view(3, H, L, 128)            # every (key, d) a different value
    for fp8, keys in ((False, vt_slot_keys(n)), (True, vt8_slot_keys(n))):
        img = vt_interleave(v, fp8)                                                        # [3, H, 128, n]
        for s in range(n):
            k = int(keys[s])
            col = img[..., s]
            assert torch.equal(col, v[..., k, :]) if k < L else not bool(col.any())
        pos0 = 192
        big = torch.full((3, H, 128, pos0 + n + 64), -1.0)
        big[..., pos0:pos0 + n] = img
        back, written = vt_stream_deinterleave(big, L, pos0, fp8)
        assert torch.equal(back, v)
        assert written.tolist() == [int(k) < L for k in keys] and int(written.sum()) == L
        if not fp8:
            assert written.tolist() == [s < L for s in range(n)]                           # the 16-bit image: exactly the slots [0, L)


def _gemm_hip_peel(shapes, ncu):
    """csrc/gemm.hip's loop, line by line (keep_rows / remain / full), independent of tests/helpers.py's restatement"""
    t256 = sum(((M + 255) // 256) * ((N + 255) // 256) for M, N in shapes)
    full = (t256 // ncu) * ncu
    if not (full > 0 and t256 > full):
        return None
    remain = t256
    keep_rows = [M for M, _ in shapes]
    i = len(shapes) - 1
    while i >= 0 and remain > full:
        tn = (shapes[i][1] + 255) // 256
        while remain > full and keep_rows[i] > 0:
            last_rows = keep_rows[i] % 256 if keep_rows[i] % 256 else 256
            keep_rows[i] -= last_rows
            remain -= tn
        i -= 1
    return keep_rows


@pytest.mark.parametrize("ncu,B0,keep1,Bs,keep_s", [(256, 51, 512, 73, 10752), (304, 61, 256, 85, 12800)])
def test_mixed_plan_peel_of_the_launch_shapes(ncu, B0, keep1, Bs, keep_s):
    """keep_rows worked out by hand from csrc/gemm.hip for both CU counts: the double-block launch is NCU + 17 / 20 tiles; p3 and p2 are peeled
    whole, p1 (864 rows of 96-row elements) keeps 512 / 256 rows -- m_base > 0 inside a batch element. The single-block launch is NCU + 20
    tiles of 6 columns: four tile rows go, 42 x 256 / 50 x 256 rows stay."""
    dbl, sgl = qkv_double_shapes(ncu), qkv_single_shape(ncu)
    d = QKV_DOUBLE
    assert dbl == [(B0 * 416, 768), (864, 768), (800, 512), (300, 264)] and sgl == [(Bs * 160, QKV_SINGLE["N"])]
    for shapes in (dbl, sgl):
        t = sum(-(-M // 256) * -(-N // 256) for M, N in shapes)
        assert 17 <= t - ncu <= 24 and (t - ncu) * 6 <= ncu
        assert mixed_plan_keep_rows(shapes, ncu) == _gemm_hip_peel(shapes, ncu)
    keep = mixed_plan_keep_rows(dbl, ncu)
    assert keep == [B0 * 416, keep1, 0, 0]
    assert 0 < keep[1] < dbl[1][0] and keep[1] % d["L"][1] != 0                             # the GPU test's m_base precondition
    assert mixed_plan_keep_rows(sgl, ncu) == [keep_s] and 0 < keep_s < sgl[0][0]
    if ncu == 256:
        assert keep_s % QKV_SINGLE["L"] != 0
    assert mixed_plan_keep_rows([(256 * 4, 256)], 4) is None and mixed_plan_keep_rows([(100, 256)], 256) is None


@pytest.mark.parametrize("K", [1536, 6144])
def test_fp32_emulation_rounds_like_float64(K):
    """M = 512 rows of the GPU test's input distributions: an fp32 evaluation of the whole epilogue differs from rne(float64) on at most
    half of NEIGHBOUR_FRAC of the bf16 elements and of the e4m3 bytes -- the inputs, not the kernel, keep the GPU test's cap honest."""
    from loongx_amd.ops import FP8_K_SCALE, FP8_Q_SCALE, FP8_V_SCALE
    M, L = 512, 128
    g = torch.Generator().manual_seed(K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(3 * D, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(3 * D, generator=g) * 0.3
    wk, wq = 1 + 0.1 * torch.randn(128, generator=g), 1 + 0.1 * torch.randn(128, generator=g)
    th = torch.randn(L, 64, generator=g) * 2.0
    cs = torch.empty(L, 128)
    cs[:, 0::2], cs[:, 1::2] = th.cos(), th.sin()
    y = A.double() @ W.double().T + bias.double()
    ref = (qk_norm_rope_ref(y[:, :D], wk, cs, L), y[:, D:2 * D], qk_norm_rope_ref(y[:, 2 * D:], wq, cs, L))
    emu = qkv_epilogue_emulate_f32(A, W, bias, wk, wq, cs, L)
    e4 = torch.float8_e4m3fn
    for name, r, e, sc in zip("kvq", ref, emu, (FP8_K_SCALE, FP8_V_SCALE, FP8_Q_SCALE)):
        assert float((e.double() - r).norm() / r.norm()) < 1e-5, name
        share16 = float((e.to(torch.bfloat16).view(torch.int16) != r.to(torch.bfloat16).view(torch.int16)).double().mean())
        assert float((r * sc).abs().max()) < 448.0
        share8 = float(((e * sc).to(e4).view(torch.uint8) != (r * sc).to(e4).view(torch.uint8)).double().mean())
        print(f"K={K} {name}: fp32 emulation differs from rne(float64) on {share16:.2e} of the bf16 elements, {share8:.2e} of the e4m3 bytes")
        assert share16 <= EMU_SHARE and share8 <= EMU_SHARE, (name, share16, share8)
