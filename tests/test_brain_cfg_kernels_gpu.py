"""lx_euler_step_cfg3 (csrc/step.hip) against float64: the step of an image under brain guidance nested in true CFG, three branches in one
launch.

x and v hold [full; text; negative] parts of n elements. The contract of include/lx.h is an operation order -- db = vF - vT rounded on its
own; gb = fmaf(scale_brain, db, vT); dt = gb - vN rounded on its own; g = fmaf(scale_text, dt, vN); e = fmaf(dsigma, g, x[i]); then
lx_euler_step_blend's blend of e where (x0, z, m) are given; x[i] = x[n + i] = x[2n + i] = the result -- and the tests hold the kernel to it:
element by element within the bound those roundings allow, bit for bit where the contract promises an identity (vF == vT: the two-branch
guided step on [T; N]; all three equal: the unguided step; m == 0: the source), on the 16-byte path and on the element path, and where the
parts are aligned differently: the later parts start at x + n, x + 2n, v + n and v + 2n, so n % 4 != 0 misaligns them under aligned bases."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_cfg_kernels_gpu import blend_bound, sentinel_buffer, untouched  # noqa: E402
from tests.test_inpaint_kernels_gpu import DEV, U, bits, choice, f32, ops, randn  # noqa: E402,F401  (ops: the fixture)

SIZES = (1, 3, 4, 1027, 65540)                    # 65540 = 4 * 16385: whole 16-byte items, 65 blocks
SCALES = ((2.0, 3.5), (1.5, 1.5), (7.5, 2.0))     # (scale_brain, scale_text)
DS, SIGMA_NEXT = f32(-0.137), f32(0.6183)


def run_cfg3(ops, x, vf, vt, vn, ds, s_b, s_t, blend=None, sigma_next=0.0, offset=0, seed=99):
    """One launch: x's first part is `x`, the other two junk (the kernel may not read them); x and v sit `offset` elements into sentinel
    buffers. Asserts the footprint, that all three parts left equal, that v and the blend operands came back unchanged and that a second
    launch on the same inputs gives the same bits; returns one part."""
    n = x.numel()
    outs = []
    for _ in range(2):
        xb, xv = sentinel_buffer(torch.cat([x, randn(n, seed) * 3.0 + 5.0, randn(n, seed + 1) * 2.0 - 7.0]), offset)
        vb, vv = sentinel_buffer(torch.cat([vf, vt, vn]), offset)
        keep = [t.clone() for t in (vb,) + tuple(blend or ())]
        ops.euler_step_cfg3(xv, vv, ds, s_b, s_t, blend, sigma_next)
        torch.cuda.synchronize()
        assert untouched(xb, offset, 3 * n), "euler_step_cfg3 wrote outside x[0:3n]"
        for name, a, b in zip(("v and the sentinels around it", "x0", "z", "m"), keep, (vb,) + tuple(blend or ())):
            assert torch.equal(bits(a), bits(b)), f"euler_step_cfg3 changed {name}"
        for k in (1, 2):
            assert torch.equal(bits(xv[:n]), bits(xv[k * n:(k + 1) * n])), f"part {k} differs from part 0"
        outs.append(xv[:n].clone())
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two launches on the same inputs differ"
    return outs[0]


def step_bound3(x, vf, vt, vn, ds, s_b, s_t):
    """E = x + ds G, G = vN + s_t DT, DT = GB - vN, GB = vT + s_b DB, DB = vF - vT, all exact (float64; v as the kernel reads it, that is
    bf16-rounded where v is bf16). The kernel rounds five times, |d_i| <= u = 2^-24: db = DB (1 + d1), gb = (s_b db + vT)(1 + d2),
    dt = (gb - vN)(1 + d3), g = (s_t dt + vN)(1 + d4), e = (ds g + x)(1 + d5). To first order gb - GB = s_b DB d1 + GB d2,
    dt - DT = (gb - GB) + DT d3, g - G = s_t (dt - DT) + G d4, e - E = ds (g - G) + E d5:
        |e - E| <= u (|ds| (|s_t| (|s_b DB| + |GB| + |DT|) + |G|) + |E|).
    Returns (E, that bound)."""
    DB = vf.double() - vt.double()
    GB = vt.double() + s_b * DB
    DT = GB - vn.double()
    G = vn.double() + s_t * DT
    E = x.double() + ds * G
    return E, U * (abs(ds) * (abs(s_t) * ((s_b * DB).abs() + GB.abs() + DT.abs()) + G.abs()) + E.abs())


def operands(n, vdt, seed=0):
    x, vf, vt, vn = randn(n, seed + 1), randn(n, seed + 2, vdt), randn(n, seed + 3, vdt), randn(n, seed + 7, vdt)
    blend = (randn(n, seed + 4), randn(n, seed + 5), choice(n, seed + 6, (0.0, 0.25, 1.0)))
    return x, vf, vt, vn, blend


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("n", SIZES)
def test_within_the_rounding_bound(ops, n, vdt):
    """N(0, 1) inputs, mask values in {0, 1/4, 1}, dsigma = -0.137, sigma_next = 0.6183; (scale_brain, scale_text) in SCALES; x and v based 0
    and 1 elements into their allocations (1: the element path, also where n % 4 == 0; 0: the 16-byte path where n % 4 == 0); with and
    without the blend. The bounds are step_bound3's and, blending, tests/test_cfg_kernels_gpu.py's blend_bound on top of it, asserted as
    they stand. The two paths must give the same bits.
    Worst measured error / bound on an MI355X: 0.896 (fp32 v, n = 65540), 0.880 with bf16 v; 0.78 at n = 1027, 0.46 or less for n <= 4."""
    x, vf, vt, vn, blend = operands(n, vdt)
    worst = 0.0
    for s_b, s_t in SCALES:
        E, be = step_bound3(x, vf, vt, vn, DS, s_b, s_t)
        X, bx = blend_bound(E, be, *blend, SIGMA_NEXT)
        for want, bound, kw in ((E, be, {}), (X, bx, dict(blend=blend, sigma_next=SIGMA_NEXT))):
            by_path = []
            for offset in (0, 1):
                got = run_cfg3(ops, x, vf, vt, vn, DS, s_b, s_t, offset=offset, **kw)
                by_path.append(got)
                err = (got.double() - want).abs()
                ratio = float((err / bound.clamp_min(1e-300)).max())
                worst = max(worst, ratio)
                assert bool((err <= bound).all()), (f"scales=({s_b}, {s_t}) offset={offset} blend={bool(kw)}: {int((err > bound).sum())} "
                                                    f"elements outside the rounding bound (worst {ratio:.3f} of it)")
            assert torch.equal(bits(by_path[0]), bits(by_path[1])), f"scales=({s_b}, {s_t}): the 16-byte and the element path differ"
    print(f"euler_step_cfg3 n={n} {vdt}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("n", [3, 1027, 65540])
def test_full_equal_to_text_is_the_two_branch_step_bit_for_bit(ops, n, vdt):
    """vF == vT: db = 0 and gb = vT exactly, whatever scale_brain: lx_euler_step_cfg on [T; N] with scale_text, on a copy"""
    x, _, vt, vn, blend = operands(n, vdt, seed=10)
    for s_t in (2.0, 3.5):
        two, two_blended = torch.cat([x, x]), torch.cat([x, x])
        ops.euler_step_cfg(two, torch.cat([vt, vn]), DS, s_t)
        ops.euler_step_cfg(two_blended, torch.cat([vt, vn]), DS, s_t, blend, SIGMA_NEXT)
        for s_b in (2.0, 7.5, -3.0, 1.0e30):
            for offset in (0, 1):
                got = run_cfg3(ops, x, vt, vt, vn, DS, s_b, s_t, offset=offset)
                assert torch.equal(bits(got), bits(two[:n])), f"scales=({s_b}, {s_t}): not lx_euler_step_cfg"
                got = run_cfg3(ops, x, vt, vt, vn, DS, s_b, s_t, blend=blend, sigma_next=SIGMA_NEXT, offset=offset)
                assert torch.equal(bits(got), bits(two_blended[:n])), f"scales=({s_b}, {s_t}): not lx_euler_step_cfg with its blend"


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("n", [3, 1027, 65540])
def test_equal_branches_are_the_unguided_step_bit_for_bit(ops, n, vdt):
    """vF == vT == vN: g = v exactly, whatever the scales: lx_euler_step, or lx_euler_step_blend, on a copy"""
    x, v, _, _, blend = operands(n, vdt, seed=20)
    euler, blended = x.clone(), x.clone()
    ops.euler_step(euler, v, DS)
    ops.euler_step_blend(blended, v, DS, *blend, SIGMA_NEXT)
    for s_b, s_t in SCALES + ((-3.0, 1.0e30),):
        for offset in (0, 1):
            assert torch.equal(bits(run_cfg3(ops, x, v, v, v, DS, s_b, s_t, offset=offset)), bits(euler)), f"scales=({s_b}, {s_t}): not lx_euler_step"
            got = run_cfg3(ops, x, v, v, v, DS, s_b, s_t, blend=blend, sigma_next=SIGMA_NEXT, offset=offset)
            assert torch.equal(bits(got), bits(blended)), f"scales=({s_b}, {s_t}): not lx_euler_step_blend"


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
def test_kept_elements_are_the_source(ops, vdt):
    """m == 0 with sigma_next == 0: x0 in all parts (run_cfg3 asserts the parts equal), whatever the branches predict; m == 1: the step"""
    n = 1024 + 5
    x, vf, vt, vn, (x0, z, _) = operands(n, vdt, seed=30)
    zeros, ones = torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
    for offset in (0, 1):
        assert torch.equal(bits(run_cfg3(ops, x, vf, vt, vn, DS, 7.5, 3.5, blend=(x0, z, zeros), sigma_next=0.0, offset=offset)), bits(x0))
        stepped = run_cfg3(ops, x, vf, vt, vn, DS, 7.5, 3.5, offset=offset)
        got = run_cfg3(ops, x, vf, vt, vn, DS, 7.5, 3.5, blend=(x0, z, ones), sigma_next=SIGMA_NEXT, offset=offset)
        assert torch.equal(bits(got), bits(stepped))


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
def test_the_paths_agree_past_the_grid_cap(ops, vdt):
    """2048 x 256 items of 4 elements per round of the 16-byte path: a part of 2048 * 256 * 4 + 1024 elements goes round twice there and
    five times on the element path; the two give the same bits, and so does the float64 restatement at dyadic coefficients where every
    rounding of it is an fp32 rounding of an exact float64 value (scales 2 and 4, dsigma -1/16: products exact, sums within 2^28 of each
    other)."""
    n = 2048 * 256 * 4 + 1024
    x, vf, vt, vn = randn(n, 41), randn(n, 42, vdt), randn(n, 43, vdt), randn(n, 44, vdt)
    db = (vf.double() - vt.double()).float()
    gb = (2.0 * db.double() + vt.double()).float()
    dt = (gb.double() - vn.double()).float()
    g = (4.0 * dt.double() + vn.double()).float()
    ref = (x.double() - 0.0625 * g.double()).float()
    vec, elem = run_cfg3(ops, x, vf, vt, vn, -0.0625, 2.0, 4.0, offset=0), run_cfg3(ops, x, vf, vt, vn, -0.0625, 2.0, 4.0, offset=1)
    assert torch.equal(bits(vec), bits(elem)) and torch.equal(bits(vec), bits(ref)), int((vec != ref).sum())


def test_refusals_through_the_wrapper_and_neighbours_that_are_none(ops):
    """x0 / z / m inside x[0, 3n) -- the later parts included -- and an fp32 v on x are LxErrors that leave x as it was; operands that
    merely touch x's ends are accepted"""
    from loongx_amd._lib import LxError
    n = 1024
    buf = randn(5 * n, 51)
    x, before, after = buf[n:4 * n], buf[:n], buf[4 * n:]
    v, z, m = randn(3 * n, 52), randn(n, 53), torch.ones(n, device=DEV)
    was = buf.clone()
    for blend in ((x[2 * n:], z, m), (z, x[:n], m), (z, z, x[2 * n - 1:3 * n - 1])):
        with pytest.raises(LxError, match="lx_euler_step_cfg3"):
            ops.euler_step_cfg3(x, v, -0.1, 2.0, 3.0, blend, 0.5)
    with pytest.raises(LxError, match="lx_euler_step_cfg3"):
        ops.euler_step_cfg3(x, buf[:3 * n], -0.1, 2.0, 3.0)
    for scales in ((float("nan"), 2.0), (2.0, float("inf"))):
        with pytest.raises(LxError, match="lx_euler_step_cfg3"):
            ops.euler_step_cfg3(x, v, -0.1, *scales)
    with pytest.raises(AssertionError):
        ops.euler_step_cfg3(buf[:3 * n + 1], randn(3 * n + 1, 54), -0.1, 2.0, 3.0)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(was))
    ops.euler_step_cfg3(x, v, -0.1, 2.0, 3.0, (before, after, m), 0.5)          # x0 ends where x begins, z begins where x ends
    torch.cuda.synchronize()
    E, be = step_bound3(was[n:2 * n], v[:n], v[n:2 * n], v[2 * n:], f32(-0.1), 2.0, 3.0)
    want = blend_bound(E, be, was[:n], was[4 * n:], m, 0.5)
    assert bool(((x[:n].double() - want[0]).abs() <= want[1]).all())
    assert torch.equal(bits(x[:n]), bits(x[n:2 * n])) and torch.equal(bits(x[:n]), bits(x[2 * n:]))
    assert torch.equal(bits(before), bits(was[:n])) and torch.equal(bits(after), bits(was[4 * n:]))
