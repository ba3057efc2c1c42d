"""CPU-only: the float64 reference of tests/test_precise_attn_tiles_gpu.py (tests/helpers.py: seg_attn_ref, vt_deinterleave, the near-bound
input constructor) pinned to torch's own scaled_dot_product_attention, to the V^T permutation that test_qkv_prep_split spells out, and to
the bounded-score contract of include/lx.h."""
import math

import pytest
import torch

from tests.helpers import (NEAR_BOUND_LENS, NEAR_BOUND_PAIRS, NEAR_BOUND_TARGET, bf16_pair, max_abs_score_log2, near_bound_qkv, seg_attn_ref,
                           seg_edges, vt_deinterleave)

NEG = float("-inf")
BIASES = {
    "none": [[0.0] * 3] * 3,
    "cfactor": [[0, 0, math.log(0.5)], [0, 0, math.log(0.5)], [math.log(0.5), math.log(0.5), 0]],
    "nounion": [[0, 0, NEG], [0, 0, NEG], [NEG, NEG, 0]],
}
Q_LOG2_FACTOR = 1.4426950408889634 / math.sqrt(128.0)


@pytest.mark.parametrize("mode", list(BIASES))
@pytest.mark.parametrize("lens,scale", [((5, 9, 7), None), ((1, 63, 65), 0.1), ((33,), None)])
def test_seg_attn_ref_is_sdpa_with_the_dense_mask(lens, scale, mode):
    B, H, S = 2, 3, sum(lens)
    g = torch.Generator().manual_seed(len(lens) + S)
    q, k, v = (torch.randn(B, H, S, 128, generator=g, dtype=torch.float64) for _ in range(3))
    seg = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    dense = torch.tensor(BIASES[mode], dtype=torch.float64)[seg][:, seg]          # [S, S]: bias[segment of the query][segment of the key]
    want = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=dense, scale=scale)
    got = seg_attn_ref(q, k, v, lens, BIASES[mode], (1.0 / math.sqrt(128.0)) if scale is None else scale)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) < 1e-13
    # scores in log2 units (q carries scale x log2 e): the natural-log factor is ln 2
    f = ((1.0 / math.sqrt(128.0)) if scale is None else scale) * 1.4426950408889634
    got2 = seg_attn_ref(q * f, k, v, lens, BIASES[mode], math.log(2.0))
    assert float((got2 - want).abs().max()) < 1e-13


def test_seg_attn_ref_gives_nan_for_a_row_masked_from_every_key():
    q, k, v = (torch.randn(1, 1, 6, 128, dtype=torch.float64) for _ in range(3))
    o = seg_attn_ref(q, k, v, (2, 4), [[0.0, 0.0, 0.0], [NEG, NEG, 0.0], [0.0] * 3], 0.1)
    assert bool(torch.isfinite(o[:, :, :2]).all()) and bool(torch.isnan(o[:, :, 2:]).all())


def test_vt_deinterleave_inverts_the_permutation_of_test_qkv_prep_split():
    lens, vt0 = (70, 1, 33), (0, 128, 192)
    g = torch.Generator().manual_seed(4)
    v = [torch.randn(2, 3, L, 128, generator=g) for L in lens]
    perm = torch.tensor([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15])
    vt = torch.full((2, 3, 128, 256), float("nan"))
    for L, p0, vs in zip(lens, vt0, v):
        n = (L + 63) // 64 * 64
        padded = torch.zeros(2, 3, n, 128)
        padded[:, :, :L] = vs
        slots = (torch.arange(n) // 16) * 16 + perm[torch.arange(n) % 16]      # as in test_qkv_prep_split: slot j holds key slots[j]
        vt[:, :, :, p0:p0 + n] = padded[:, :, slots].permute(0, 1, 3, 2)
    assert torch.equal(vt_deinterleave(vt, lens, vt0), torch.cat(v, 2))


@pytest.mark.parametrize("mode", ["none", "cfactor"])
def test_near_bound_inputs_keep_the_bounded_score_contract(mode):
    """|q.k (log2 units) + bias log2 e| <= 100 over ALL pairs (include/lx.h, LX_ATTN_BOUNDED), on the fp32 rows and on the bf16 pairs the
    split producer makes of them; the constructed pairs sit at +-90 with both signs."""
    buf = near_bound_qkv(Q_LOG2_FACTOR)
    H, D = 2, 256
    e = seg_edges(NEAR_BOUND_LENS)
    for pair in (False, True):
        x = buf
        if pair:
            hi, lo = bf16_pair(buf)
            x = hi.double() + lo.double()
        q, k = (x[:, c:c + D].view(-1, H, 128).permute(1, 0, 2) for c in (2 * D, 0))
        worst = max_abs_score_log2(q, k, NEAR_BOUND_LENS, BIASES[mode])
        assert NEAR_BOUND_TARGET - 1.5 <= worst <= 100.0, worst
        s = torch.matmul(q.double(), k.double().transpose(-1, -2))[0]
        signs = set()
        for sq, qp, sk, kp, sign in NEAR_BOUND_PAIRS:
            got = float(s[e[sq] + qp, e[sk] + kp])
            assert abs(got - sign * NEAR_BOUND_TARGET) < 0.01, (got, sign)
            signs.add(sign)
        assert signs == {1.0, -1.0}
        # every other score of the spiked query rows is far below: the constructed one dominates (+) or vanishes (-) in the softmax
        rows = torch.tensor([e[sq] + qp for sq, qp, *_ in NEAR_BOUND_PAIRS])
        others = s[rows].clone()
        for i, (sq, qp, sk, kp, sign) in enumerate(NEAR_BOUND_PAIRS):
            others[i, e[sk] + kp] = 0.0
        assert float(others.abs().max()) < 50.0
