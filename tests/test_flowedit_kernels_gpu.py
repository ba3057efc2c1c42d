"""lx_flowedit_inputs and lx_flowedit_step (csrc/step.hip) against float64: the two launches of a FlowEdit step (generate's source_prompt).

The contract of include/lx.h, per element i < n:
  inputs   s = fmaf(sigma, noise, fl((1 - sigma) x_src)), lx_scale_noise's bits, to out[n + i]; out[i] = fl(z_fe + fl(s - x_src))
  step     d = fl(vt - vs); d = fl(m d) where m is given; z_fe[i] = m[i] == 0 ? z_fe[i] : fmaf(coef, d, z_fe[i])
What is checked, per case, at offset 0 (the 16-byte path where n % 4 == 0) and at offset 1 (the element path), with u = 2^-24 and
O2 = 1 + 2^-20 for the products of two errors and the float64 reference's own roundings:
  out[n:]  equals ops.scale_noise(x_src, noise, sigma) bit for bit
  out[:n]  against R = z + (S - x), S = sigma noise + oms x in float64 with oms = fl(1 - sigma), the value the rule names. s carries
           lx_scale_noise's two roundings, |s - S| <= u (|oms x| + |S|); the difference one, u |S - x|; the add one, u |R|:
               |out[i] - R| <= u (|oms x| + |S| + |S - x| + |R|) O2
  z_fe     against Z = z + coef m (vt - vs) in float64 (a bf16 v widens exactly). The difference is one rounding, u |D|, which reaches Z with
           weight |coef m|; the product with m one more, u |m D| with weight |coef|; the fma one, u |Z|:
               |z_fe' - Z| <= u (2 |coef m D| + |Z|) O2 with a mask,   u (|coef D| + |Z|) O2 without
  bits     both paths, and two launches, agree; nothing outside out[0, 2n) / z_fe[0, n) is written; the inputs are unchanged
and m == 0 elements keep their bits with NaN planted in v there, vt == vs leaves z_fe as it was, and the refusals through the wrapper."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_apg_kernels_gpu import O2, f64  # noqa: E402
from tests.test_cfg_kernels_gpu import sentinel_buffer, untouched  # noqa: E402
from tests.test_inpaint_kernels_gpu import DEV, U, bits, choice, f32, ops, randn  # noqa: E402,F401  (ops: the fixture)

B, F = torch.bfloat16, torch.float32
# 256: the smallest 16-byte launch; 1023: a ragged element path; 4100: a vector launch plus 4; 65536: the 512^2 latent
SIZES = (256, 1023, 4100, 65536)
SIGMAS = (f32(0.7313), 0.0, 1.0)
COEF = f32(-0.137 / 2)


def within(got, want, bound, tag, what):
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{tag}: worst error / bound of {what} = {worst:.3f}")
    assert (err <= bound).all(), f"{tag}: {int((err > bound).sum())} elements of {what} outside the rounding bound (worst {worst:.3f} of it)"


def launch_inputs(ops, x, z, noise, sigma, offset=0, z_offset=None):
    """Two launches on copies of the same inputs, every operand `offset` (z_fe: `z_offset`) elements into a sentinel buffer. Asserts the
    footprint, that the inputs came back unchanged and that the two launches agree bit for bit; returns out [2n]."""
    n = x.numel()
    z_offset = offset if z_offset is None else z_offset
    outs = []
    for _ in range(2):
        ob, ov = sentinel_buffer(randn(2 * n, 91) * 3.0 + 5.0, offset)
        ins = [sentinel_buffer(t, o) for t, o in ((x, offset), (z, z_offset), (noise, offset))]
        keep = [b.clone() for b, _ in ins]
        ops.flowedit_inputs(ins[0][1], ins[1][1], ins[2][1], sigma, out=ov)
        torch.cuda.synchronize()
        assert untouched(ob, offset, 2 * n), "wrote outside out[0, 2n)"
        for name, a, (b, _) in zip(("x_src", "z_fe", "noise"), keep, ins):
            assert torch.equal(bits(a), bits(b)), f"flowedit_inputs changed {name} or the sentinels around it"
        outs.append(ov.clone())
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two launches on the same inputs differ"
    return outs[0]


def launch_step(ops, z, vt, vs, coef, m=None, offset=0, m_offset=None):
    """Two launches on copies of the same inputs, z_fe, v and m in sentinel buffers; asserts the footprint, v and m unchanged and the two
    launches equal; returns z_fe [n]."""
    n = z.numel()
    m_offset = offset if m_offset is None else m_offset
    outs = []
    for _ in range(2):
        zb, zv = sentinel_buffer(z, offset)
        vb, vv = sentinel_buffer(torch.cat([vt, vs]), offset)
        mb, mv = (None, None) if m is None else sentinel_buffer(m, m_offset)
        keep = [t.clone() for t in (vb, mb) if t is not None]
        ops.flowedit_step(zv, vv, coef, mv)
        torch.cuda.synchronize()
        assert untouched(zb, offset, n), "wrote outside z_fe[0, n)"
        for name, a, b in zip(("v", "m"), keep, [t for t in (vb, mb) if t is not None]):
            assert torch.equal(bits(a), bits(b)), f"flowedit_step changed {name} or the sentinels around it"
        outs.append(zv.clone())
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two launches on the same inputs differ"
    return outs[0]


@pytest.mark.parametrize("sigma", SIGMAS, ids=lambda s: f"sigma{s:.4f}")
@pytest.mark.parametrize("n", SIZES)
def test_inputs_against_float64(ops, n, sigma):
    """N(0, 1) source and noise, the edit state the source plus an N(0, 1/4) edit; sigma = 0.7313, 0 and 1. The bound is the module
    docstring's, asserted as it stands. sigma == 0: out[n:] is x_src and out[:n] is z_fe, exactly."""
    x, noise = randn(n, 11), randn(n, 12)
    z = x + 0.5 * randn(n, 13)
    tag = f"inputs n={n} sigma={sigma}"
    by_offset = [launch_inputs(ops, x, z, noise, sigma, offset=o) for o in (0, 1)]
    assert torch.equal(bits(by_offset[0]), bits(by_offset[1])), f"{tag}: the 16-byte and the element path differ"
    # z_fe alone off its 16 bytes takes the element path too: the same bits
    assert torch.equal(bits(launch_inputs(ops, x, z, noise, sigma, offset=0, z_offset=1)), bits(by_offset[0])), f"{tag}: z_fe one element off"
    got = by_offset[0]
    assert torch.equal(bits(got[n:]), bits(ops.scale_noise(x, noise, sigma))), f"{tag}: out[n:] is not lx_scale_noise bit for bit"
    xs, zs, ns = f64(x), f64(z), f64(noise)
    oms = f32(1.0 - sigma)                                     # (1 - sigma in fp32, as the kernel's host forms it: sigma is an fp32 value)
    S = sigma * ns + oms * xs
    R = zs + (S - xs)
    within(got[:n], R, U * (np.abs(oms * xs) + np.abs(S) + np.abs(S - xs) + np.abs(R)) * O2, tag, "out[:n]")
    if sigma == 0.0:
        assert torch.equal(got[n:], x) and torch.equal(got[:n], z), f"{tag}: sigma == 0 is not (z_fe, x_src)"
    if sigma == 1.0:
        assert torch.equal(got[n:], noise), f"{tag}: sigma == 1 is not the noise"


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("vdt", [B, F], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("n", SIZES)
def test_step_against_float64(ops, n, vdt, masked):
    """N(0, 1) state and velocities, mask values in {0, 1/4, 1}, coef = -0.0685. The bound is the module docstring's, asserted as it stands;
    m == 0 elements keep their bits."""
    z, vt, vs = randn(n, 21), randn(n, 22, vdt), randn(n, 23, vdt)
    m = choice(n, 24, (0.0, 0.25, 1.0)) if masked else None
    tag = f"step n={n} {'bf16' if vdt is B else 'f32'} {'mask' if masked else 'nomask'}"
    by_offset = [launch_step(ops, z, vt, vs, COEF, m, offset=o) for o in (0, 1)]
    assert torch.equal(bits(by_offset[0]), bits(by_offset[1])), f"{tag}: the 16-byte and the element path differ"
    if masked:      # m alone off its 16 bytes takes the element path too
        assert torch.equal(bits(launch_step(ops, z, vt, vs, COEF, m, offset=0, m_offset=1)), bits(by_offset[0])), f"{tag}: m one element off"
    got = by_offset[0]
    zs, D = f64(z), f64(vt) - f64(vs)
    if masked:
        ms = f64(m)
        Z = zs + COEF * ms * D
        bound = U * (2 * np.abs(COEF * ms * D) + np.abs(Z)) * O2
        kept = m == 0
        assert torch.equal(bits(got[kept]), bits(z[kept])), f"{tag}: an m == 0 element changed"
    else:
        Z = zs + COEF * D
        bound = U * (np.abs(COEF * D) + np.abs(Z)) * O2
    within(got, Z, bound, tag, "z_fe")


@pytest.mark.parametrize("vdt", [B, F], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("n", [256, 1023])
def test_kept_elements_keep_their_bits_whatever_v_holds(ops, n, vdt):
    """NaN planted in both branches of v (and a NaN and an infinity in z_fe itself) where m == 0: those elements of z_fe come back in every
    bit, and every other element is what the launch on the clean v gives"""
    z, vt, vs = randn(n, 31), randn(n, 32, vdt), randn(n, 33, vdt)
    m = choice(n, 34, (0.0, 0.25, 1.0))
    kept = m == 0
    assert bool(kept.any()) and not bool(kept.all())
    clean = [launch_step(ops, z, vt, vs, COEF, m, offset=o) for o in (0, 1)]
    vt2, vs2, z2 = vt.clone(), vs.clone(), z.clone()
    vt2[kept] = float("nan")
    vs2[kept[:n]] = float("nan")
    first = torch.nonzero(kept)[:2, 0]
    z2[first[0]] = float("nan")
    z2[first[1]] = float("inf")
    for o in (0, 1):
        got = launch_step(ops, z2, vt2, vs2, COEF, m, offset=o)
        assert torch.equal(bits(got[kept]), bits(z2[kept])), "a kept element did not keep its bits"
        assert torch.equal(bits(got[~kept]), bits(clean[o][~kept])), "an edited element saw another element's v"


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("vdt", [B, F], ids=["v_bf16", "v_f32"])
def test_equal_branches_leave_the_state(ops, vdt, masked):
    """vt == vs bit for bit: d == 0 and fmaf(coef, 0, z) == z, on both paths"""
    n = 1023
    z, v = randn(n, 41), randn(n, 42, vdt)
    m = choice(n, 43, (0.0, 0.25, 1.0)) if masked else None
    for o in (0, 1):
        assert torch.equal(launch_step(ops, z, v, v.clone(), COEF, m, offset=o), z)


def test_one_flowedit_step_is_the_two_launches(ops):
    """inputs then step with v = the inputs themselves (a field v(x) = x): Z' = Z + coef (R - S) = Z + coef (Z - X) up to the stated
    roundings -- the two entries composed as the scheduler composes them, through the [2, ...] buffer ops.flowedit_inputs allocates"""
    n, sigma = 4100, f32(0.5)
    x, noise = randn(n, 51).view(1, n // 4, 4), randn(n, 52).view(1, n // 4, 4)
    z = (x + 0.5 * randn(n, 53).view_as(x)).contiguous()
    out = ops.flowedit_inputs(x, z, noise, sigma)
    assert tuple(out.shape) == (2,) + tuple(x.shape)
    z1 = z.clone()
    ops.flowedit_step(z1, out, COEF)
    Dd = f64(out[0]) - f64(out[1])
    Z = f64(z) + COEF * Dd
    within(z1, Z, U * (np.abs(COEF * Dd) + np.abs(Z)) * O2, "composed", "z_fe")


def test_refusals_through_the_wrapper(ops):
    """an overlap, a sigma outside [0, 1] and a coef that is not finite are LxErrors that leave everything as it was; a wrong element count is
    the wrapper's assertion"""
    from loongx_amd._lib import LxError
    n = 1024
    buf = randn(6 * n, 61)
    was = buf.clone()
    out, x, z, noise = buf[:2 * n], buf[2 * n:3 * n], buf[3 * n:4 * n], buf[4 * n:5 * n]
    for bad in (dict(x_src=out[:n]), dict(z_fe=out[n:]), dict(noise=buf[n + 1:2 * n + 1])):
        with pytest.raises(LxError, match="lx_flowedit_inputs"):
            ops.flowedit_inputs(**dict(dict(x_src=x, z_fe=z, noise=noise, sigma=0.5, out=out), **bad))
    for sigma in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(LxError, match="lx_flowedit_inputs"):
            ops.flowedit_inputs(x, z, noise, sigma, out=out)
    with pytest.raises(AssertionError):
        ops.flowedit_inputs(x, z, noise, 0.5, out=buf[:2 * n + 1])
    v = buf[:2 * n]
    for bad in (dict(z_fe=v[n:]), dict(z_fe=buf[2 * n - 1:3 * n - 1]), dict(m=z), dict(coef=float("nan")), dict(coef=float("inf"))):
        with pytest.raises(LxError, match="lx_flowedit_step"):
            ops.flowedit_step(**dict(dict(z_fe=z, v=v, coef=-0.1, m=None), **bad))
    vb = randn(2 * n, 62, B)
    with pytest.raises(LxError, match="lx_flowedit_step"):
        ops.flowedit_step(vb.view(torch.float32)[:n], vb, -0.1)          # (a bf16 v may not hold z_fe either)
    with pytest.raises(AssertionError):
        ops.flowedit_step(z, buf[:2 * n + 1], -0.1)
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(was))
