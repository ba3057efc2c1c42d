"""lx_euler_step_cfg (csrc/step.hip) against float64: the step of a true-CFG image, both branches in one launch.

x and v hold [positive; negative] halves of n elements. The contract of include/lx.h is an operation order -- d = vp - vn rounded on its own;
g = fmaf(scale, d, vn); e = fmaf(dsigma, g, x[i]); then lx_euler_step_blend's blend of e where (x0, z, m) are given; x[i] = x[n + i] = the
result -- and the tests hold the kernel to it: element by element within the bound those roundings allow, bit for bit where the contract
promises an identity (vp == vn: the unguided step; m == 0: the source), on the 16-byte path and on the element path, and above all where
the two halves are aligned differently: the second halves start at x + n and v + n, so n % 4 != 0 misaligns them under aligned bases.

Worst measured error / bound over every case below: see test_within_the_rounding_bound's docstring."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_inpaint_kernels_gpu import DEV, SENT, TAIL, U, bits, choice, f32, ops, randn  # noqa: E402,F401  (ops: the fixture)

SIZES = (1, 3, 4, 5, 1027, 2 * 16 * 64)          # the last: a guided batch-1 step of the generate tests, [2, 16, 64] per half
SCALES = (1.0, 2.0, 7.5)
DS, SIGMA_NEXT = f32(-0.137), f32(0.6183)


def sentinel_buffer(src, offset):
    """src copied into a sentinel-filled buffer of its dtype, `offset` elements after the (256-byte aligned) start: (buffer, view of src)"""
    buf = torch.empty(offset + src.numel() + TAIL, dtype=src.dtype, device=DEV)
    bits(buf).fill_(SENT if src.dtype == torch.float32 else 0x7FC1)
    view = buf[offset:offset + src.numel()]
    view.copy_(src)
    return buf, view


def untouched(buf, offset, n):
    b, s = bits(buf), (SENT if buf.dtype == torch.float32 else 0x7FC1)
    return bool((b[:offset] == s).all()) and bool((b[offset + n:] == s).all())


def run_cfg(ops, x, vp, vn, ds, scale, blend=None, sigma_next=0.0, offset=0, seed=99):
    """One launch: x's positive half is `x`, its negative half junk (the kernel may not read it); x and v sit `offset` elements into sentinel
    buffers. Asserts the footprint, that both halves left equal, that v and the blend operands came back unchanged and that a second launch
    on the same inputs gives the same bits; returns one half."""
    n = x.numel()
    outs = []
    for _ in range(2):
        xb, xv = sentinel_buffer(torch.cat([x, randn(n, seed) * 3.0 + 5.0]), offset)
        vb, vv = sentinel_buffer(torch.cat([vp, vn]), offset)
        keep = [t.clone() for t in (vb,) + tuple(blend or ())]
        ops.euler_step_cfg(xv, vv, ds, scale, blend, sigma_next)
        torch.cuda.synchronize()
        assert untouched(xb, offset, 2 * n), "euler_step_cfg wrote outside x[0:2n]"
        for name, a, b in zip(("v and the sentinels around it", "x0", "z", "m"), keep, (vb,) + tuple(blend or ())):
            assert torch.equal(bits(a), bits(b)), f"euler_step_cfg changed {name}"
        assert torch.equal(bits(xv[:n]), bits(xv[n:])), f"the halves differ in {int((xv[:n] != xv[n:]).sum())} elements"
        outs.append(xv[:n].clone())
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two launches on the same inputs differ"
    return outs[0]


def step_bound(x, vp, vn, ds, scale):
    """E = x + ds G, G = vn + scale D, D = vp - vn exact. The kernel rounds three times -- d = D (1 + d1), g = (scale d + vn)(1 + d2),
    e = (ds g + x)(1 + d3), |d_i| <= u -- so e - E = ds scale D d1 + ds G d2 + E d3 + O(u^2): |e - E| <= u (|ds| (|scale D| + |G|) + |E|),
    times (1 + 2^-20) for the O(u^2) terms (3 u^2 of the same quantities) and the float64 reference's own 2^-53. Returns (E, the bound)."""
    D = vp.double() - vn.double()
    G = vn.double() + scale * D
    E = x.double() + ds * G
    return E, U * (abs(ds) * ((scale * D).abs() + G.abs()) + E.abs()) * (1 + 2.0 ** -20)


def blend_bound(E, be, x0, z, m, s):
    """The bound of tests/test_inpaint_kernels_gpu.py::test_general_coefficients_within_the_rounding_bound, 4 u (|m E| + |(1 - m) R| +
    (1 - m)(|s z| + |(1 - s) x0|)), whose e enters as m e: e's own error `be` (step_bound) is carried through with the weight m. Returns
    (X = m E + (1 - m) R, the bound)."""
    md, sz, sx = m.double(), s * z.double(), (1.0 - s) * x0.double()
    R = sz + sx
    return md * E + (1 - md) * R, md * be + 4 * U * ((md * E).abs() + ((1 - md) * R).abs() + (1 - md) * (sz.abs() + sx.abs()))


def operands(n, vdt, seed=0):
    x, vp, vn = randn(n, seed + 1), randn(n, seed + 2, vdt), randn(n, seed + 3, vdt)
    blend = (randn(n, seed + 4), randn(n, seed + 5), choice(n, seed + 6, (0.0, 0.25, 1.0)))
    return x, vp, vn, blend


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("n", SIZES)
def test_within_the_rounding_bound(ops, n, vdt):
    """N(0, 1) inputs, mask values in {0, 1/4, 1}, dsigma = -0.137, sigma_next = 0.6183; scale in {1, 2, 7.5}; x and v based 0 and 1
    elements into their allocations (1: the element path; 0: the 16-byte path where n % 4 == 0); with and without the blend. The bounds
    are step_bound's and blend_bound's, asserted as they stand.
    Worst measured error / bound on an MI355X: 0.947 (fp32 v, n = 1027 and 2048), 0.902 with bf16 v; 0.56 or less for n <= 5."""
    x, vp, vn, blend = operands(n, vdt)
    worst = 0.0
    for scale in SCALES:
        E, be = step_bound(x, vp, vn, DS, scale)
        X, bx = blend_bound(E, be, *blend, SIGMA_NEXT)
        for offset in (0, 1):
            for want, bound, kw in ((E, be, {}), (X, bx, dict(blend=blend, sigma_next=SIGMA_NEXT))):
                got = run_cfg(ops, x, vp, vn, DS, scale, offset=offset, **kw).double()
                err = (got - want).abs()
                ratio = float((err / bound.clamp_min(1e-300)).max())
                worst = max(worst, ratio)
                assert bool((err <= bound).all()), (f"scale={scale} offset={offset} blend={bool(kw)}: {int((err > bound).sum())} elements outside "
                                                    f"the rounding bound (worst {ratio:.3f} of it)")
    print(f"euler_step_cfg n={n} {vdt}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("n", [5, 1027, 2 * 16 * 64])
def test_equal_branches_are_the_unguided_step_bit_for_bit(ops, n, vdt):
    """vp == vn: d = 0 and g = vn exactly, whatever the scale: lx_euler_step, or lx_euler_step_blend, on a copy"""
    x, vp, _, blend = operands(n, vdt, seed=10)
    euler, blended = x.clone(), x.clone()
    ops.euler_step(euler, vp, DS)
    ops.euler_step_blend(blended, vp, DS, *blend, SIGMA_NEXT)
    for scale in SCALES + (-3.0, 1.0e30):
        for offset in (0, 1):
            assert torch.equal(bits(run_cfg(ops, x, vp, vp, DS, scale, offset=offset)), bits(euler)), f"scale={scale}: not lx_euler_step"
            got = run_cfg(ops, x, vp, vp, DS, scale, blend=blend, sigma_next=SIGMA_NEXT, offset=offset)
            assert torch.equal(bits(got), bits(blended)), f"scale={scale}: not lx_euler_step_blend"


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
def test_kept_elements_are_the_source(ops, vdt):
    """m == 0 with sigma_next == 0: x0 in both halves (run_cfg asserts the halves equal), whatever the branches predict; m == 1: the step"""
    n = 1024 + 5
    x, vp, vn, (x0, z, _) = operands(n, vdt, seed=20)
    zeros, ones = torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
    for offset in (0, 1):
        assert torch.equal(bits(run_cfg(ops, x, vp, vn, DS, 7.5, blend=(x0, z, zeros), sigma_next=0.0, offset=offset)), bits(x0))
        stepped = run_cfg(ops, x, vp, vn, DS, 7.5, offset=offset)
        assert torch.equal(bits(run_cfg(ops, x, vp, vn, DS, 7.5, blend=(x0, z, ones), sigma_next=SIGMA_NEXT, offset=offset)), bits(stepped))


@pytest.mark.parametrize("n", [1027, 6])
def test_misaligned_negative_half(ops, n):
    """bf16 v, n % 4 != 0, aligned bases: v + n is 2 bytes past a 4-byte boundary (n odd) or 4 bytes past an 8-byte one (n = 6), and x + n is
    off its 16 bytes as well, while the positive halves are aligned. Within the bound of float64, and the same bits as the same data run
    through the element path (bases one element in)."""
    x, vp, vn, blend = operands(n, torch.bfloat16, seed=30)
    for scale in SCALES:
        E, be = step_bound(x, vp, vn, DS, scale)
        X, bx = blend_bound(E, be, *blend, SIGMA_NEXT)
        for want, bound, kw in ((E, be, {}), (X, bx, dict(blend=blend, sigma_next=SIGMA_NEXT))):
            aligned = run_cfg(ops, x, vp, vn, DS, scale, offset=0, **kw)
            assert aligned.data_ptr() % 16 == 0
            element = run_cfg(ops, x, vp, vn, DS, scale, offset=1, **kw)
            assert torch.equal(bits(aligned), bits(element)), f"scale={scale}: {int((aligned != element).sum())} elements differ between the paths"
            err = (aligned.double() - want).abs()
            assert bool((err <= bound).all()), f"scale={scale}: {int((err > bound).sum())} elements outside the rounding bound"


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
def test_the_paths_agree_past_the_grid_cap(ops, vdt):
    """2048 x 256 items of 4 elements per round of the 16-byte path: a half of 2048 * 256 * 4 + 1024 elements goes round twice there and
    five times on the element path; the two give the same bits, and so does the float64 restatement at dyadic coefficients where every
    rounding of it is an fp32 rounding of an exact float64 value (scale 2, dsigma -1/16: products exact, sums within 2^28 of each other)."""
    n = 2048 * 256 * 4 + 1024
    x, vp, vn = randn(n, 41), randn(n, 42, vdt), randn(n, 43, vdt)
    d = (vp.double() - vn.double()).float()
    g = (2.0 * d.double() + vn.double()).float()
    ref = (x.double() - 0.0625 * g.double()).float()
    vec, elem = run_cfg(ops, x, vp, vn, -0.0625, 2.0, offset=0), run_cfg(ops, x, vp, vn, -0.0625, 2.0, offset=1)
    assert torch.equal(bits(vec), bits(elem)) and torch.equal(bits(vec), bits(ref)), int((vec != ref).sum())


def test_refusals_through_the_wrapper_and_neighbours_that_are_none(ops):
    """x0 / z / m inside x[0, 2n) -- the negative half included -- and an fp32 v on x are LxErrors that leave x as it was; operands that
    merely touch x's ends are accepted"""
    from loongx_amd._lib import LxError
    n = 1024
    buf = randn(4 * n, 51)
    x, before, after = buf[n:3 * n], buf[:n], buf[3 * n:]
    v, z, m = randn(2 * n, 52), randn(n, 53), torch.ones(n, device=DEV)
    was = buf.clone()
    for blend in ((x[n:], z, m), (z, x[:n], m), (z, z, x[n - 1:2 * n - 1])):
        with pytest.raises(LxError, match="lx_euler_step_cfg"):
            ops.euler_step_cfg(x, v, -0.1, 2.0, blend, 0.5)
    with pytest.raises(LxError, match="lx_euler_step_cfg"):
        ops.euler_step_cfg(x, buf[:2 * n], -0.1, 2.0)
    with pytest.raises(LxError, match="lx_euler_step_cfg"):
        ops.euler_step_cfg(x, v, -0.1, float("nan"))
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(was))
    ops.euler_step_cfg(x, v, -0.1, 2.0, (before, after, m), 0.5)          # x0 ends where x begins, z begins where x ends
    torch.cuda.synchronize()
    want = blend_bound(*step_bound(was[n:2 * n], v[:n], v[n:], f32(-0.1), 2.0), was[:n], was[3 * n:], m, 0.5)
    assert bool(((x[:n].double() - want[0]).abs() <= want[1]).all()) and torch.equal(bits(x[:n]), bits(x[n:]))
    assert torch.equal(bits(before), bits(was[:n])) and torch.equal(bits(after), bits(was[3 * n:]))
