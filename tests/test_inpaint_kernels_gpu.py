"""lx_scale_noise and lx_euler_step_blend (csrc/step.hip) against float64: the start of an img2img trajectory and the inpaint step.

The contract of include/lx.h is an operation order -- e = fmaf(ds, v, x); r = fmaf(s, z, (1 - s) * x0); x = fmaf(m, e, (1 - m) * r), the two
products and the two differences rounded on their own -- and the tests hold the kernels to it three ways:
  * bit for bit against that order restated in float64 with one fp32 rounding per rounding of the contract, at dyadic coefficients where
    every float64 step is exact; on the 16-byte path, on the element path (x and m one element off alignment), the two against each other,
    past the grid cap of either path, inside sentinel tails, with every input unchanged;
  * the identities that generate() relies on (m == 1: the Euler step; m == 0: the noised source; sigma_next == 0: the source itself;
    sigma == 1: the noise), bit for bit at arbitrary coefficients;
  * at arbitrary coefficients, element by element within the bound that the roundings of that order allow (derived at the test).
Refused calls return the error status, name their entry point and launch nothing."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x7FC0BEEF
TAIL = 64
U = 2.0 ** -24            # fp32 unit roundoff
# 777: the element tail of the 16-byte path; 4096: whole 16-byte items only; the last two make the grid-stride loop of the element path
# (2048 x 256 elements per round) and of the 16-byte path (2048 x 256 items of 4) go round more than twice
SIZES = (777, 4096, 2048 * 256 * 2 + 777, 2048 * 256 * 4 * 2 + 777)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


def f32(x):
    """a value that fp32 holds exactly, as a Python float (what the C ABI receives is then what the reference uses)"""
    return float(np.float32(x))


def randn(n, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, generator=g, device=DEV).to(dtype)


def choice(n, seed, values):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.tensor(values, device=DEV, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g, device=DEV)]


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def in_sentinel(src, offset=0):
    """src copied into a sentinel-filled buffer `offset` elements after its (256-byte aligned) start: (buffer, the view that holds src)"""
    buf = torch.empty(offset + src.numel() + TAIL, dtype=torch.float32, device=DEV)
    bits(buf).fill_(SENT)
    view = buf[offset:offset + src.numel()]
    view.copy_(src)
    return buf, view


def untouched(buf, offset, n):
    b = bits(buf)
    return bool((b[:offset] == SENT).all()) and bool((b[offset + n:] == SENT).all())


def scale_noise_ref(x0, z, s):
    """the contract in float64, one fp32 rounding where the kernel has one: p = fl((1 - s) x0), r = fl(s z + p)"""
    oms = f32(1.0 - s)
    p = (oms * x0.double()).float()
    return (s * z.double() + p.double()).float()


def blend_ref(x, v, ds, x0, z, m, s):
    e = (x.double() + ds * v.double()).float()
    r = scale_noise_ref(x0, z, s)
    k = (1.0 - m.double()).float()
    q = (k.double() * r.double()).float()
    return (m.double() * e.double() + q.double()).float()


def run_blend(ops, x, v, ds, x0, z, m, s, offset):
    """one launch with x and m `offset` elements off a 256-byte boundary, x inside a sentinel buffer; asserts the footprint and that the
    inputs came back unchanged; returns the new x"""
    n = x.numel()
    xb, xv = in_sentinel(x, offset)
    mb, mv = in_sentinel(m, offset)
    keep = [t.clone() for t in (v, x0, z, mb)]
    ops.euler_step_blend(xv, v, ds, x0, z, mv, s)
    torch.cuda.synchronize()
    assert untouched(xb, offset, n), "euler_step_blend wrote outside x[0:n]"
    for name, a, b in zip(("v", "x0", "z", "m"), keep, (v, x0, z, mb)):
        assert torch.equal(bits(a), bits(b)), f"euler_step_blend changed {name}"
    return xv.clone()


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("n", SIZES)
def test_blend_is_the_contract_bit_for_bit_on_both_paths(ops, n, vdt):
    """ds = -1/16, sigma_next in {0, 1/4, 1}, m in {0, 1/2, 1}: every product of the contract is then exact in float64 (a 24-bit
    significand times at most two bits), and every sum is too as long as its operands lie within 2^28 of each other -- beyond that the
    smaller one is too small to move the float64 sum onto an fp32 tie, so rounding it twice still equals the fused rounding. The float64
    restatement with one fp32 rounding per rounding of the contract is therefore what the kernel must return, bit for bit (the argument
    tests/test_rowops_gpu.py makes for lx_euler_step)."""
    x, v, x0, z = randn(n, 1), randn(n, 2, vdt), randn(n, 3), randn(n, 4)
    m = choice(n, 5, (0.0, 0.5, 1.0))
    for s in (0.0, 0.25, 1.0):
        ref = blend_ref(x, v, -0.0625, x0, z, m, s)
        got_vec = run_blend(ops, x, v, -0.0625, x0, z, m, s, offset=0)
        got_elem = run_blend(ops, x, v, -0.0625, x0, z, m, s, offset=1)
        assert torch.equal(bits(got_vec), bits(got_elem)), f"sigma_next={s}: the 16-byte and the element path differ in {int((got_vec != got_elem).sum())} elements"
        assert torch.equal(bits(got_vec), bits(ref)), f"sigma_next={s}: {int((got_vec != ref).sum())} elements differ from the contract"


@pytest.mark.parametrize("n", SIZES)
def test_scale_noise_is_the_contract_bit_for_bit_on_both_paths(ops, n):
    x0, z = randn(n, 6), randn(n, 7)
    for s in (0.0, 0.25, 1.0):
        ref = scale_noise_ref(x0, z, s)
        outs = []
        for offset in (0, 1):
            ob, ov = in_sentinel(torch.zeros(n, device=DEV), offset)
            keep = (x0.clone(), z.clone())
            assert ops.scale_noise(x0, z, s, out=ov) is ov
            torch.cuda.synchronize()
            assert untouched(ob, offset, n), "scale_noise wrote outside out[0:n]"
            assert torch.equal(bits(keep[0]), bits(x0)) and torch.equal(bits(keep[1]), bits(z)), "scale_noise changed an input"
            outs.append(ov.clone())
        assert torch.equal(bits(outs[0]), bits(outs[1])), f"sigma={s}: the 16-byte and the element path differ"
        assert torch.equal(bits(outs[0]), bits(ref)), f"sigma={s}: {int((outs[0] != ref).sum())} elements differ from the contract"


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
def test_identities_at_arbitrary_coefficients(ops, vdt):
    n = 4096 + 777
    ds, s = f32(-0.137), f32(0.6183)
    x, v, x0, z = randn(n, 11), randn(n, 12, vdt), randn(n, 13), randn(n, 14)
    ones, zeros = torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
    for offset in (0, 1):
        euler = x.clone()
        ops.euler_step(euler, v, ds)
        assert torch.equal(bits(run_blend(ops, x, v, ds, x0, z, ones, s, offset)), bits(euler)), "m == 1 is not lx_euler_step"
        noised = ops.scale_noise(x0, z, s)
        assert torch.equal(bits(run_blend(ops, x, v, ds, x0, z, zeros, s, offset)), bits(noised)), "m == 0 is not lx_scale_noise(x0, z, sigma_next)"
        assert torch.equal(bits(run_blend(ops, x, v, ds, x0, z, zeros, 0.0, offset)), bits(x0)), "sigma_next == 0, m == 0 is not x0"
    assert torch.equal(bits(ops.scale_noise(x0, z, 1.0)), bits(z)), "scale_noise at sigma == 1 is not z"
    assert torch.equal(bits(ops.scale_noise(x0, z, 0.0)), bits(x0)), "scale_noise at sigma == 0 is not x0"


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
def test_general_coefficients_within_the_rounding_bound(ops, vdt):
    """With E = x + ds v, R = s z + (1 - s) x0 and X = m E + (1 - m) R exact, u = 2^-24 and every |d_i| <= u, the kernel computes
        e = E (1 + d1)                                   c = (1 - s)(1 + d2)        (the difference 1 - sigma_next, taken on the host)
        p = c x0 (1 + d3)                                r = (s z + p)(1 + d4)
        k = (1 - m)(1 + d5)                              q = k r (1 + d6)           x = (m e + q)(1 + d7)
    so  r - R = R d4 + (1 - s) x0 (d2 + d3) + O(u^2)  and
        x - X = m E (d1 + d7) + (1 - m) [R (d4 + d5 + d6 + d7) + (1 - s) x0 (d2 + d3)] + O(u^2):
        |x - X| <= u (2 |m E| + 4 |(1 - m) R| + 2 (1 - m) |(1 - s) x0|) + O(u^2).
    Held to 4 u (|m E| + |(1 - m) R| + (1 - m)(|s z| + |(1 - s) x0|)): the first-order terms above with the coefficient 4 throughout; the
    O(u^2) terms (about 20 u^2 of the same quantities) and the float64 reference's own 2^-53 fit in what that rounds up, which is at
    least 2 u (|m E| + (1 - m)(|s z| + |(1 - s) x0|)). (The contract names five roundings; the two differences 1 - sigma_next and 1 - m are
    the other two and are exact for sigma_next, m >= 1/2.) No underflow at these magnitudes."""
    n = 4096 * 3 + 777
    x, v, x0, z = randn(n, 21), randn(n, 22, vdt), randn(n, 23), randn(n, 24)
    g = torch.Generator(device=DEV).manual_seed(25)
    m = torch.rand(n, generator=g, device=DEV)
    m[::7], m[1::7] = 0.0, 1.0
    worst = 0.0
    for ds, s in ((f32(-0.137), f32(0.6183)), (f32(-0.0421), f32(0.0917)), (f32(-0.31), f32(0.937))):
        for offset in (0, 1):
            got = run_blend(ops, x, v, ds, x0, z, m, s, offset).double()
            md, E = m.double(), x.double() + ds * v.double()
            sz, sx = s * z.double(), (1.0 - s) * x0.double()
            R = sz + sx
            bound = 4 * U * ((md * E).abs() + ((1 - md) * R).abs() + (1 - md) * (sz.abs() + sx.abs()))
            err = (got - (md * E + (1 - md) * R)).abs()
            ratio = float((err / bound.clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            print(f"blend {vdt} ds={ds:.4f} sigma_next={s:.4f} offset={offset}: worst error / bound = {ratio:.3f}")
            assert bool((err <= bound).all()), f"ds={ds} sigma_next={s}: {int((err > bound).sum())} elements outside the rounding bound (worst {ratio:.3f} of it)"
        sn = ops.scale_noise(x0, z, s).double()
        sz, sx = s * z.double(), (1.0 - s) * x0.double()
        err, bound = (sn - (sz + sx)).abs(), U * ((sz + sx).abs() + 2 * sx.abs()) * (1 + 2 ** -20)      # (r - R above, O(u^2) rounded up)
        print(f"scale_noise sigma={s:.4f}: worst error / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all())


def test_refused_calls_name_their_entry_point_and_launch_nothing(ops):
    from loongx_amd._lib import LxError, lib
    a, n = 0x10000, 1024                                                     # (fake, aligned addresses: nothing dereferences them)
    blend_args = lambda x, v, x0, z, m: (x, v, 0, ctypes.c_float(-0.1), x0, z, m, ctypes.c_float(0.5), n, None)      # noqa: E731
    for null in range(5):
        p = [a + i * 0x10000 for i in range(5)]
        p[null] = None
        assert lib.lx_euler_step_blend(*blend_args(*p)) == -1 and b"lx_euler_step_blend" in lib.lx_last_error(), null
    for alias in (2, 3, 4):                                                      # x0, z, m on x: the same address, and overlapping it
        for delta in (0, 4 * (n - 1), -4 * (n - 1)):
            p = [a + i * 0x10000 for i in range(5)]
            p[alias] = p[0] + delta
            assert lib.lx_euler_step_blend(*blend_args(*p)) == -1 and b"lx_euler_step_blend" in lib.lx_last_error(), (alias, delta)
    for null in range(3):
        p = [a, a + 0x10000, a + 0x20000]
        p[null] = None
        assert lib.lx_scale_noise(*p, ctypes.c_float(0.5), n, None) == -1 and b"lx_scale_noise" in lib.lx_last_error(), null
    # through the wrapper, on real tensors: the error surfaces as LxError and x is as it was
    x, v, z, m = randn(n, 31), randn(n, 32), randn(n, 33), torch.ones(n, device=DEV)
    before = x.clone()
    with pytest.raises(LxError, match="lx_euler_step_blend"):
        ops.euler_step_blend(x, v, -0.1, x, z, m, 0.5)
    with pytest.raises(LxError, match="lx_euler_step_blend"):
        ops.euler_step_blend(x, v, -0.1, z, z, x, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(bits(x), bits(before))
