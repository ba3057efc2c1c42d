"""lx_dpmpp2m_step and lx_dpmpp2m_step_apg (csrc/step.hip) against float64: the second-order multistep step, the Euler step of one, two or
three branches plus one correction on the denoised prediction.

The contract of include/lx.h, per element: g the guided velocity of the part count; e = fmaf(dsigma, g, x); d = fmaf(-sigma, g, x);
o = c == 0 ? e : fmaf(c, d - D, e) with the difference rounded on its own; D = d; then lx_euler_step_blend's blend of o where (x0, z, m)
are given; the result to every part of x. What is checked, per case of CASES, at offset 0 (the 16-byte path where n % 4 == 0) and at
offset 1 (the element path):
  D      against the float64 x - sigma G of the inputs, within sigma dg + u |D|, dg the bound of the guided velocity (0 for one part)
  x      against the float64 x + dsigma G + c (D - D_prev), then the blend, within
         |dsigma| dg + u |E| + |c| (sigma dg + u |D| + u |D - D_prev|) + u |O|, times O2, carried through the blend as the inpaint test does
  bits   both paths, and two launches, agree in x and D; every part of x is equal; nothing outside x and D is written; v, x0, z and m are
         unchanged
  c = 0  x is the Euler entry of that part count and blend bit for bit, with D full of NaN beforehand, and D comes back finite
and two consecutive calls against the float64 two-step restatement, m == 0 keeping the source, and the APG entry: c == 0 is
lx_euler_step_apg bit for bit in x, M and sums; c != 0 is checked against the exact value given the kernel's own M and sums."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_apg_kernels_gpu import DS, O2, SCALES as APG_SCALES, SHAPES as APG_SHAPES, SIGMA, SIGMA_NEXT, f64, g0_ref, sentinel_f64  # noqa: E402
from tests.test_cfg_kernels_gpu import sentinel_buffer, untouched  # noqa: E402
from tests.test_inpaint_kernels_gpu import DEV, U, bits, choice, f32, ops, randn  # noqa: E402,F401  (ops: the fixture)

C = f32(0.25)
SCALES = {1: (), 2: APG_SCALES[2], 3: APG_SCALES[3]}
B, F = torch.bfloat16, torch.float32
# 256: the smallest 16-byte launch; 1023: the element path with a ragged tail; 4100: an APG chunk boundary plus 4; 65536: the 512^2 latent
SIZES = (256, 1023, 4100, 65536)
# (n, n_parts, v dtype, blend, c): every value of every axis at every size
CASES = [(n,) + rest for n in SIZES for rest in ((1, F, False, 0.0), (2, B, True, C), (3, F, True, C), (1, B, True, C), (2, F, False, C),
                                                 (3, B, False, 0.0), (1, F, False, C), (3, B, True, 0.0))]
for _n in SIZES:
    for _axis, _values in ((1, {1, 2, 3}), (2, {B, F}), (3, {True, False}), (4, {0.0, C})):
        assert {c[_axis] for c in CASES if c[0] == _n} == _values


def case_id(c):
    n, parts, vdt, blend, cc = c
    return f"{n}-{parts}parts-{'bf16' if vdt is B else 'f32'}-{'blend' if blend else 'step'}-c{cc}"


def inputs(n, parts, vdt, seed):
    x = randn(n, seed + 1)
    vparts = [randn(n, seed + 2 + k, vdt) for k in range(parts)]
    blend = (randn(n, seed + 6), randn(n, seed + 7), choice(n, seed + 8, (0.0, 0.25, 1.0)))
    return x, vparts, blend, randn(n, seed + 9)


def launch(ops, x, vparts, c, D_in, blend=None, sigma=SIGMA, ds=DS, sigma_next=SIGMA_NEXT, offset=0, d_offset=None):
    """Two launches on copies of the same inputs: x's first part is `x`, the others junk (the kernel may not read them); x, v and D sit
    `offset` (D: `d_offset`) elements into sentinel buffers. Asserts the footprint, that the parts left equal, that v and the blend operands
    came back unchanged and that the two launches agree bit for bit; returns (one part of x, D)."""
    n, parts = x.numel(), len(vparts)
    d_offset = offset if d_offset is None else d_offset
    outs = []
    for _ in range(2):
        junk = [randn(n, 90 + k) * 3.0 + 5.0 for k in range(parts - 1)]
        xb, xv = sentinel_buffer(torch.cat([x] + junk), offset)
        vb, vv = sentinel_buffer(torch.cat(vparts), offset)
        db, dv = sentinel_buffer(D_in, d_offset)
        keep = [t.clone() for t in (vb,) + tuple(blend or ())]
        ops.dpmpp2m_step(xv, vv, sigma, ds, c, dv, SCALES[parts], blend, sigma_next)
        torch.cuda.synchronize()
        assert untouched(xb, offset, parts * n), "wrote outside x[0, n_parts n)"
        assert untouched(db, d_offset, n), "wrote outside D[0, n)"
        for name, a, b in zip(("v and the sentinels around it", "x0", "z", "m"), keep, (vb,) + tuple(blend or ())):
            assert torch.equal(bits(a), bits(b)), f"dpmpp2m_step changed {name}"
        for k in range(1, parts):
            assert torch.equal(bits(xv[:n]), bits(xv[k * n:(k + 1) * n])), f"part {k} differs from part 0"
        outs.append((xv[:n].clone(), dv.clone()))
    for name, a, b in zip(("x", "D"), outs[0], outs[1]):
        assert torch.equal(bits(a), bits(b)), f"two launches on the same inputs differ in {name}"
    return outs[0]


def euler(ops, x, vparts, blend=None, ds=DS, sigma_next=SIGMA_NEXT):
    """the Euler entry of the part count and blend on copies of the same inputs; returns part 0 of x"""
    n, parts = x.numel(), len(vparts)
    xx, v = torch.cat([x] * parts), torch.cat(vparts)
    if parts == 1 and blend is None:
        ops.euler_step(xx, v, ds)
    elif parts == 1:
        ops.euler_step_blend(xx, v, ds, *blend, sigma_next)
    elif parts == 2:
        ops.euler_step_cfg(xx, v, ds, *SCALES[2], blend, sigma_next)
    else:
        ops.euler_step_cfg3(xx, v, ds, *SCALES[3], blend, sigma_next)
    return xx[:n].clone()


def velocity_ref(vs, parts):
    """(G exact, dg the bound on the kernel's g): the value itself for one part (a bf16 v widens exactly), else the APG test's g0_ref, which
    is the cfg tests' step_bound / step_bound3 without their Euler step"""
    return (vs[0], np.zeros_like(vs[0])) if parts == 1 else g0_ref(vs, SCALES[parts])


def step_ref(xs, G, dg, c, D_prev, sigma=SIGMA, ds=DS):
    """-> (Dx, its bound, O, its bound): the bounds of include/lx.h as written, O's times O2"""
    Dx = xs - sigma * G
    bd = sigma * dg + U * np.abs(Dx)
    E = xs + ds * G
    O = E + c * (Dx - D_prev) if c != 0 else E
    bo = (abs(ds) * dg + U * np.abs(E) + abs(c) * (sigma * dg + U * np.abs(Dx) + U * np.abs(Dx - D_prev)) + U * np.abs(O)) * O2
    return Dx, bd, O, bo


def blend_ref(O, bo, blend, sigma_next=SIGMA_NEXT):
    """tests/test_cfg_kernels_gpu.py's blend_bound in numpy: o's own error carried through with the weight m"""
    x0, z, m = (f64(t) for t in blend)
    sz, sx = sigma_next * z, (1.0 - sigma_next) * x0
    R = sz + sx
    return m * O + (1 - m) * R, m * bo + 4 * U * (np.abs(m * O) + np.abs((1 - m) * R) + (1 - m) * (np.abs(sz) + np.abs(sx)))


def within(got, want, bound, tag, what):
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{tag}: worst error / bound of {what} = {worst:.3f}")
    assert (err <= bound).all(), f"{tag}: {int((err > bound).sum())} elements of {what} outside the rounding bound (worst {worst:.3f} of it)"
    return worst


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_against_float64(ops, case):
    """N(0, 1) inputs and D_prev, mask values in {0, 1/4, 1}, sigma = 0.7313, dsigma = -0.137, sigma_next = 0.5943, scale 3.5 or (2, 3.5),
    c = 0 or 1/4. The bounds are those of the module docstring, asserted as they stand.
    Worst measured error / bound on an MI355X: 0.919 for x; 1.000 for D with one part, where dg = 0 and the bound u |D| is the one rounding
    of d itself (a half ulp just above a power of two), 0.94 or less with two or three parts."""
    n, parts, vdt, with_blend, c = case
    x, vparts, blend, D_prev = inputs(n, parts, vdt, seed=7 * parts)
    blend = blend if with_blend else None
    tag = case_id(case)
    by_offset = []
    for offset in (0, 1):
        D_in = D_prev if c != 0 else torch.full((n,), float("nan"), device=DEV)
        by_offset.append(launch(ops, x, vparts, c, D_in, blend, offset=offset))
    for name, a, b in zip(("x", "D"), *by_offset):
        assert torch.equal(bits(a), bits(b)), f"{tag}: the 16-byte and the element path differ in {name}"
    # D alone off its 16 bytes takes the element path too: the same bits
    got_x, got_D = launch(ops, x, vparts, c, D_prev, blend, offset=0, d_offset=1)
    assert torch.equal(bits(got_x), bits(by_offset[0][0])) and torch.equal(bits(got_D), bits(by_offset[0][1])), f"{tag}: D one element off"
    got_x, got_D = by_offset[0]
    assert bool(torch.isfinite(got_x).all()) and bool(torch.isfinite(got_D).all()), f"{tag}: not finite"
    xs, vs = f64(x), [f64(p) for p in vparts]
    G, dg = velocity_ref(vs, parts)
    Dx, bd, O, bo = step_ref(xs, G, dg, c, f64(D_prev))
    within(got_D, Dx, bd, tag, "D")
    want, bound = (O, bo) if blend is None else blend_ref(O, bo, blend)
    within(got_x, want, bound, tag, "x")
    if c == 0:
        assert torch.equal(bits(got_x), bits(euler(ops, x, vparts, blend))), f"{tag}: c == 0 is not the Euler entry bit for bit"


@pytest.mark.parametrize("vdt", [B, F], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("blend_on", [False, True], ids=["step", "blend"])
@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("n", [256, 1023])
def test_c_zero_is_the_euler_entry_bit_for_bit(ops, n, parts, blend_on, vdt):
    """every part count, blend and v format: c == 0 with D full of NaN is the Euler entry in every bit of x on both paths, and D comes back
    finite: the denoised prediction of this step, which the same call with c != 0 stores as well"""
    x, vparts, blend, D_prev = inputs(n, parts, vdt, seed=200)
    blend = blend if blend_on else None
    want = euler(ops, x, vparts, blend)
    nan = torch.full((n,), float("nan"), device=DEV)
    for offset in (0, 1):
        got, D0 = launch(ops, x, vparts, 0.0, nan, blend, offset=offset)
        assert torch.equal(bits(got), bits(want)), f"offset {offset}: not the Euler entry"
        assert bool(torch.isfinite(D0).all())
        _, D1 = launch(ops, x, vparts, C, D_prev, blend, offset=offset)
        assert torch.equal(bits(D0), bits(D1)), "D does not depend on c or on what it held"


@pytest.mark.parametrize("n,parts,vdt,blend_on", [(256, 1, F, False), (1023, 2, B, True), (4100, 3, F, True), (65536, 1, B, False),
                                                  (4100, 2, F, False)])
def test_two_consecutive_calls(ops, n, parts, vdt, blend_on):
    """c = 0, then c = 1/4 from the first call's x and D, as a trajectory starts; against the float64 two-step restatement. The second step
    X2 = m (X1 + ds G2 + c (X1 - sigma G2 - D1)) + (1 - m) R is linear in the first one's results with dX2/dX1 = m (1 + c) and
    dX2/dD1 = -m c (G2 is an input of its own), so the summed bound is the second call's own bound at the exact values plus
    m ((1 + |c|) b(x1) + |c| b(D1)), times O2 for the products of two errors."""
    x, v1, blend, _ = inputs(n, parts, vdt, seed=300)
    _, v2, _, _ = inputs(n, parts, vdt, seed=400)
    blend = blend if blend_on else None
    m = f64(blend[2]) if blend_on else 1.0
    xs, vs1, vs2 = f64(x), [f64(p) for p in v1], [f64(p) for p in v2]
    G1, dg1 = velocity_ref(vs1, parts)
    D1, bd1, O1, bo1 = step_ref(xs, G1, dg1, 0.0, 0.0)
    X1, bx1 = (O1, bo1) if blend is None else blend_ref(O1, bo1, blend)
    G2, dg2 = velocity_ref(vs2, parts)
    D2, bd2, O2_, bo2 = step_ref(X1, G2, dg2, C, D1)
    X2, bx2 = (O2_, bo2) if blend is None else blend_ref(O2_, bo2, blend)
    bx2 = (bx2 + m * ((1 + C) * bx1 + C * bd1)) * O2
    bd2 = (bd2 + bx1) * O2                                    # (D2 = X1 - sigma G2: the first step's error enters with weight 1)
    for offset in (0, 1):
        x1, d1 = launch(ops, x, v1, 0.0, torch.full((n,), float("nan"), device=DEV), blend, offset=offset)
        x2, d2 = launch(ops, x1, v2, C, d1, blend, offset=offset)
        tag = f"two calls n={n} parts={parts} offset={offset}"
        within(x1, X1, bx1, tag, "x after the first")
        within(d1, D1, bd1, tag, "D after the first")
        within(x2, X2, bx2, tag, "x after the second")
        within(d2, D2, bd2, tag, "D after the second")


@pytest.mark.parametrize("vdt", [B, F], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("parts", [1, 3])
def test_kept_elements_are_the_source(ops, parts, vdt):
    """m == 0 with sigma_next == 0: x0 in all parts, whatever the branches and the history say; m == 1: the step without a blend"""
    n = 1023
    x, vparts, (x0, z, _), D_prev = inputs(n, parts, vdt, seed=500)
    zeros, ones = torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
    for offset in (0, 1):
        got, _ = launch(ops, x, vparts, C, D_prev, (x0, z, zeros), sigma_next=0.0, offset=offset)
        assert torch.equal(bits(got), bits(x0))
        stepped, _ = launch(ops, x, vparts, C, D_prev, offset=offset)
        got, _ = launch(ops, x, vparts, C, D_prev, (x0, z, ones), offset=offset)
        assert torch.equal(bits(got), bits(stepped))


# ---- the APG entry ---------------------------------------------------------------------------------------------------------------------
ETA, MOMENTUM, THR = 0.5, -0.5, f32(20.0)
# (shape, n_parts, v dtype, blend): every shape of the APG kernel test
APG_CASES = [((1, 256), 2, F, False), ((3, 320), 3, B, True), ((2, 4100), 2, B, True), ((2, 4100), 3, F, False), ((2, 1023), 3, F, True),
             ((2, 1023), 2, B, False), ((2, 65536), 3, B, True), ((2, 65536), 2, F, False)]
assert {c[0] for c in APG_CASES} == set(APG_SHAPES)


def launch_apg(ops, x, vparts, c, D_in, M_in, n_images, blend, offset, multi=True):
    """tests/test_apg_kernels_gpu.py's launch with D: one launch of dpmpp2m_step_apg (or, multi=False, of euler_step_apg on the same
    buffers); asserts the footprint and the equal parts; returns (one part of x, D, M, sums)"""
    n, parts = x.numel(), len(vparts)
    junk = [randn(n, 90 + k) * 3.0 + 5.0 for k in range(parts - 1)]
    xb, xv = sentinel_buffer(torch.cat([x] + junk), offset)
    vb, vv = sentinel_buffer(torch.cat(vparts), offset)
    mb, mv = sentinel_buffer(M_in, offset)
    db, dv = sentinel_buffer(D_in, offset)
    sb, sv = sentinel_f64(3 * n_images, offset)
    ws_count = ops.apg_workspace_bytes(n_images, n // n_images) // 8
    wb, wv = sentinel_f64(ws_count, offset)
    keep = [t.clone() for t in (vb,) + tuple(blend or ())]
    if multi:
        ops.dpmpp2m_step_apg(xv, vv, SIGMA, DS, c, dv, APG_SCALES[parts], ETA, THR, MOMENTUM, mv, sv.view(n_images, 3), wv, blend, SIGMA_NEXT)
    else:
        ops.euler_step_apg(xv, vv, SIGMA, DS, APG_SCALES[parts], ETA, THR, MOMENTUM, mv, sv.view(n_images, 3), wv, blend, SIGMA_NEXT)
    torch.cuda.synchronize()
    assert untouched(xb, offset, parts * n) and untouched(mb, offset, n) and untouched(db, offset, n), "wrote outside x, M or D"
    assert untouched(sb, 2 * offset, 6 * n_images) and untouched(wb, 2 * offset, 2 * ws_count), "wrote outside sums or the workspace"
    for name, a, b in zip(("v and the sentinels around it", "x0", "z", "m"), keep, (vb,) + tuple(blend or ())):
        assert torch.equal(bits(a), bits(b)), f"the APG step changed {name}"
    for k in range(1, parts):
        assert torch.equal(bits(xv[:n]), bits(xv[k * n:(k + 1) * n])), f"part {k} differs from part 0"
    return xv[:n].clone(), dv.clone(), mv.clone(), sv.clone()


@pytest.mark.parametrize("case", APG_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}parts-{'bf16' if c[2] is B else 'f32'}-{'blend' if c[3] else 'step'}")
def test_apg_entry(ops, case):
    """eta = 0.5, momentum = -0.5 on an N(0, 1) M, threshold 20 (it binds: |Db| is about 2.6 sqrt(elems) or more). c == 0 with D full of
    NaN: lx_euler_step_apg in every bit of x, M and sums, and D finite. c = 1/4: M and sums are still lx_euler_step_apg's bit for bit, and x
    lies within the bound of the projected step given the kernel's own M and sums (tests/test_apg_kernels_gpu.py's check_call) plus the
    correction's: lx_dpmpp2m_step's bound with dg the APG bound on g. Both paths agree."""
    (n_images, elems), parts, vdt, with_blend = case
    n = n_images * elems
    x, vparts, blend, D_prev = inputs(n, parts, vdt, seed=600)
    blend = blend if with_blend else None
    M_in = randn(n, 699)
    nan = torch.full((n,), float("nan"), device=DEV)
    per_offset = []
    for offset in (0, 1):
        ex, _, eM, esums = launch_apg(ops, x, vparts, 0.0, nan, M_in, n_images, blend, offset, multi=False)
        x0_, D0, M0, sums0 = launch_apg(ops, x, vparts, 0.0, nan, M_in, n_images, blend, offset)
        assert torch.equal(bits(x0_), bits(ex)) and torch.equal(bits(M0), bits(eM)) and torch.equal(bits(sums0.view(F)), bits(esums.view(F))), \
            f"offset {offset}: c == 0 is not lx_euler_step_apg bit for bit"
        assert bool(torch.isfinite(D0).all())
        x1, D1, M1, sums1 = launch_apg(ops, x, vparts, C, D_prev, M_in, n_images, blend, offset)
        assert torch.equal(bits(M1), bits(eM)) and torch.equal(bits(sums1.view(F)), bits(esums.view(F))) and torch.equal(bits(D1), bits(D0))
        per_offset.append((x1, D1))
    for a, b in zip(*per_offset):
        assert torch.equal(bits(a), bits(b)), "the 16-byte and the element path differ"
    got_x, got_D = per_offset[0]
    # the projected velocity and its bound given the kernel's own M and sums, as the APG test's check_call forms them
    xs, vs = f64(x), [f64(p) for p in vparts]
    Db = eM.cpu().numpy().astype(np.float64).reshape(n_images, elems)
    S = esums.cpu().numpy().reshape(n_images, 3)
    S_dd, S_dw, S_ww = (S[:, k:k + 1] for k in range(3))
    r = float(THR)
    with np.errstate(divide="ignore", invalid="ignore"):
        cc = np.where((r > 0) & (S_dd > r * r), r / np.sqrt(S_dd), 1.0)
        a = np.where(S_ww > 0, S_dw / S_ww, 0.0)
    k = cc * (1.0 - ETA) * a
    W = (xs - SIGMA * vs[0]).reshape(n_images, elems)
    Uu = cc * Db - k * W
    G = (vs[0].reshape(n_images, elems) - Uu / SIGMA).reshape(n)
    bu = U * (np.abs(cc * Db) + 3 * np.abs(k * W) + np.abs(Uu))
    dg = ((bu + U * np.abs(Uu)) / SIGMA).reshape(n) + U * np.abs(G)
    Dx, bd, O, bo = step_ref(xs, G, dg, C, f64(D_prev))
    tag = f"apg {case[0]} {parts} parts"
    within(got_D, Dx, bd, tag, "D")
    want, bound = (O, bo) if blend is None else blend_ref(O, bo, blend)
    within(got_x, want, bound, tag, "x")


def test_refusals_through_the_wrapper(ops):
    """D inside x[0, n_parts n) or on v is an LxError that leaves everything as it was; a D of another size is the wrapper's assertion"""
    from loongx_amd._lib import LxError
    n = 1024
    buf = randn(5 * n, 51)
    x, was = buf[n:4 * n], buf.clone()
    v, D = randn(3 * n, 52), torch.zeros(n, device=DEV)
    for bad in (x[2 * n:], x[:n], v[n:2 * n]):
        with pytest.raises(LxError, match="lx_dpmpp2m_step"):
            ops.dpmpp2m_step(x, v, 0.7, -0.1, 0.25, bad, (2.0, 3.0))
    for kw in (dict(sigma=0.0), dict(c=float("inf")), dict(scales=(2.0, float("nan")))):
        with pytest.raises(LxError, match="lx_dpmpp2m_step"):
            ops.dpmpp2m_step(x, v, **dict(dict(sigma=0.7, dsigma=-0.1, c=0.25, D=D, scales=(2.0, 3.0)), **kw))
    with pytest.raises(AssertionError):
        ops.dpmpp2m_step(x, v, 0.7, -0.1, 0.25, torch.zeros(n + 1, device=DEV), (2.0, 3.0))
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(was)) and not bool(D.any())
