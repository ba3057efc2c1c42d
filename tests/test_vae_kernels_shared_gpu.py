"""The VAE glue kernels of csrc/vae.hip are one body per piece with the operand format as a store policy: exact identities between the
formats that one body must satisfy (torch.equal on the bits, no tolerance), and the GroupNorm chunk rule's edges in all three formats."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.helpers import relerr  # noqa: E402

DEV = "cuda"
bf16, f16 = torch.bfloat16, torch.float16
NAN_BITS = 0x7FC0          # float("nan") in bf16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def bits(t):
    return t.view(torch.int16).to(torch.int32) & 0xFFFF


def nan_image(rows, ld, offset, dtype=bf16):
    """[rows, ld] of NaN whose first element lies `offset` elements behind a 256-byte aligned address"""
    flat = torch.full((rows * ld + offset,), float("nan"), dtype=dtype, device=DEV)
    return flat[offset:].view(rows, ld)


# ---- row softmax ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["vector", "scalar"])
@pytest.mark.parametrize("n_valid", [1, 3, 63, 64, 65, 259])
def test_softmax_pair_hi_half_is_the_bf16_image(ops, n_valid, offset):
    """softmax_rows_split's hi half == softmax_rows(n_valid=...) bit for bit (split_bf16_pair's hi and pack_bf16x2 are one rounding), the pad
    columns of both halves are +0, and nothing outside [0, n_store) and [p_lo_off, p_lo_off + n_store) is written. M = 5: the last
    workgroup is ragged. offset 1: S and P start one element off, so every access is a scalar one."""
    M, n_store = 5, (n_valid + 63) // 64 * 64
    lo, ldp = n_store + 8, 2 * n_store + 16
    S = nan_image(M, n_store, offset, torch.float32)                        # the pad keys' scores are NaN: never loaded
    S[:, :n_valid] = (rnd(M, n_valid, seed=7) * 3.0).to(DEV)
    P1, P2 = nan_image(M, n_store + 8, offset), nan_image(M, ldp, offset)
    assert S.data_ptr() % 16 == 4 * offset and P1.data_ptr() % 8 == 2 * offset and P2.data_ptr() % 8 == 2 * offset
    ops.softmax_rows(S, P1[:, :n_store], 0.25, n_valid=n_valid)             # (n_store is the width of what it is handed)
    ops.softmax_rows_split(S, P2, 0.25, n_valid, n_store, lo)
    torch.cuda.synchronize()
    b1, b2 = bits(P1).cpu(), bits(P2).cpu()
    assert torch.equal(b2[:, :n_store], b1[:, :n_store])
    assert bool((b1[:, n_valid:n_store] == 0).all()) and bool((b2[:, lo + n_valid:lo + n_store] == 0).all())
    assert bool((b1[:, n_store:] == NAN_BITS).all())
    assert bool((b2[:, n_store:lo] == NAN_BITS).all()) and bool((b2[:, lo + n_store:] == NAN_BITS).all())


def test_softmax_rows_is_the_padded_form_without_padding(ops):
    M, N = 5, 260
    S = (rnd(M, N, seed=8) * 3.0).to(DEV)
    P1, P2 = nan_image(M, N, 0), nan_image(M, N, 0)
    ops.softmax_rows(S, P1, 0.25)
    ops.softmax_rows(S, P2, 0.25, n_valid=N)
    torch.cuda.synchronize()
    assert torch.equal(bits(P1), bits(P2)) and not bool(torch.isnan(P1).any())


# ---- im2col --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C", [3, 8, 24])
def test_im2col_pair_halves_are_the_single_image_gathers(ops, C, mode):
    """The hi and lo column blocks of im2col3x3_split each == im2col3x3 of that half alone. C = 3: scalar items; 8, 24: 16-byte items.
    Kpad > 9 C: a zero tail; the pair's pixel rows are wider than x_lo_off + C (the gaps hold NaN). Every column of every row is written."""
    B, H, W = 2, 4, 6
    lo = (C + 7) // 8 * 8 + 8
    ld = lo + lo
    Kpad = (9 * C + 63) // 64 * 64
    assert Kpad > 9 * C and ld > lo + C
    x = torch.full((B, H, W, ld), float("nan"), dtype=bf16, device=DEV)
    x[..., :C] = rnd(B, H, W, C, seed=11).to(DEV)
    x[..., lo:lo + C] = rnd(B, H, W, C, seed=12).to(DEV)
    Ho, Wo = {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[mode]
    rows = B * Ho * Wo
    pair = nan_image(rows, 2 * Kpad, 0)
    ops.im2col3x3_split(x, C, lo, pair, mode)
    for half, col0 in ((x[..., :C], 0), (x[..., lo:lo + C], Kpad)):
        one = nan_image(rows, Kpad, 0)
        ops.im2col3x3(half.contiguous(), one, mode)
        torch.cuda.synchronize()
        assert torch.equal(bits(pair[:, col0:col0 + Kpad]), bits(one))
        assert not bool(torch.isnan(one).any()) and bool((bits(one[:, 9 * C:]) == 0).all())
        # and the gather is the right one: the centre tap of modes 0 / 2 is the (upsampled) image itself, mode 1's tap 0 every other pixel
        img = half.float()
        want = {0: img, 1: img[:, ::2, ::2], 2: img.repeat_interleave(2, 1).repeat_interleave(2, 2)}[mode]
        tap = 0 if mode == 1 else 4
        assert torch.equal(one[:, tap * C:(tap + 1) * C].float(), want.reshape(rows, C))


# ---- GroupNorm -----------------------------------------------------------------------------------------------------------------
GN_SHAPES = [(128, 5), (128, 257), (512, 4097)]       # 1 chunk with fewer rows than a pass takes; 16 chunks, short last one; 64 chunks, 2 rows a pass
_gn_cache = {}


def _gn_case(C, P):
    """inputs of the existing GroupNorm tests (test_vae_gpu.py: 2 randn + 0.5; the fp16 and pair ones: randn + 8) and the float64 references"""
    if (C, P) not in _gn_cache:
        B, G = 2, 32
        g, b = 1.0 + 0.2 * rnd(C, seed=42), 0.3 * rnd(C, seed=43)

        def ref(x):
            return F.silu(F.group_norm(x.double().transpose(1, 2), G, g.double(), b.double(), 1e-6).transpose(1, 2))
        xa, xb = rnd(B, P, C, seed=1) * 2.0 + 0.5, rnd(B, P, C, seed=41) + 8.0
        _gn_cache[(C, P)] = dict(g=g.to(DEV), b=b.to(DEV), xa=xa.to(DEV), xb=xb.to(DEV), ref_a=ref(xa), ref_b=ref(xb))
    return _gn_cache[(C, P)]


@pytest.mark.parametrize("fmt", ["bf16", "f16", "split"])
@pytest.mark.parametrize("C,P", GN_SHAPES, ids=lambda v: str(v))
def test_groupnorm_chunk_rule_edges(ops, C, P, fmt):
    """Every format at the edges of the chunk rule that one gn_chunks decides: twice the same bits (no atomics in the statistics), and
    against float64 F.group_norm + SiLU at the bound of the format's own test (4e-3 test_vae_gpu.py, 3e-4 test_vae_f16_gpu.py, 2e-5
    test_vae_precise_gpu.py), on that test's kind of input."""
    B, G = 2, 32
    c = _gn_case(C, P)
    lo, ldy = C + 8, 2 * C + 16
    outs = []
    for _ in range(2):
        if fmt == "bf16":
            y = nan_image(B * P, C, 0).view(B, P, C)
            ops.groupnorm_silu(c["xa"], c["g"], c["b"], y, G, 1e-6, True)
        elif fmt == "f16":
            y = nan_image(B * P, C, 0, f16).view(B, P, C)
            ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.groupnorm_silu_f16(c["xb"], c["g"], c["b"], y, G, 1e-6, True, f16_ovf=ovf)
            assert int(ovf.item()) == 0
        else:
            y = nan_image(B * P, ldy, 0)
            ops.groupnorm_silu_split(c["xb"], c["g"], c["b"], y, lo, G, 1e-6, True)
        outs.append(y)
    torch.cuda.synchronize()
    assert torch.equal(bits(outs[0]), bits(outs[1]))
    y = outs[0].cpu()
    if fmt == "split":
        assert bool((bits(y[:, C:lo]) == NAN_BITS).all()) and bool((bits(y[:, lo + C:]) == NAN_BITS).all())
        got, want, bound = y[:, :C].double() + y[:, lo:lo + C].double(), c["ref_b"].reshape(B * P, C), 2e-5
    else:
        got, want, bound = y.double(), (c["ref_a"] if fmt == "bf16" else c["ref_b"]), (4e-3 if fmt == "bf16" else 3e-4)
    err = relerr(got, want)
    print(f"groupnorm {fmt} C={C} P={P}: relerr {err:.3e} (bound {bound:.0e})")
    assert err < bound
