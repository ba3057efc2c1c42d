"""lx_euler_step_apg (csrc/step.hip) against a float64 numpy restatement of the rule in include/lx.h: the guided step under adaptive
projected guidance, a per-image reduction over the branch velocities and a fused project, clamp, Euler-step and blend.

x and v hold 2 or 3 parts of n = n_images * elems elements. Pass 1 leaves Db = (-sigma)(g0 - vc) [+ momentum M] in M and, per image, the
sums (sum Db^2, sum Db w, sum w^2) with w = fmaf(-sigma, vc, x), products and additions in double in a fixed order. Pass 2 reads the sums:
c = r / sqrt(S_dd) where the threshold binds, a = S_dw / S_ww, u = c32 Db - k32 w with k = c (1 - eta) a, g = vc - u / sigma, the Euler step
and the blend, stored to every part. What is checked, per case of CASES, on the 16-byte path (offset 0 where elems % 4 == 0) and on the
element path (offset 1):
  M      against the float64 Db of the inputs, within the roundings of g0, dv, D and the momentum fma
  sums   against the float64 sums of the kernel's own M and of w (reproduced bit for bit: one fma), within elems 2^-52 sum |terms|
  x      against the exact value given the kernel's own M and sums, within the bound of include/lx.h, asserted as it stands
  bits   both paths, and two launches, agree in x, M and sums; every part of x is equal; nothing outside x, M, sums and the workspace is
         written; v, x0, z and m are unchanged; with momentum 0 an M full of NaN is not read
and the identities of the contract: equal branches are lx_euler_step / lx_euler_step_blend, m == 0 keeps the source, eta == 0 leaves u
orthogonal to w, a binding threshold leaves |u| <= r."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_cfg_kernels_gpu import sentinel_buffer, untouched  # noqa: E402
from tests.test_inpaint_kernels_gpu import DEV, SENT, TAIL, U, bits, choice, f32, ops, randn  # noqa: E402,F401  (ops: the fixture)

SIGMA, DS, SIGMA_NEXT = f32(0.7313), f32(-0.137), f32(0.5943)
SCALES = {2: (3.5,), 3: (2.0, 3.5)}
O2 = 1 + 2.0 ** -20                  # the second-order terms of a first-order bound and the float64 reference's own 2^-53
# (n_images, elems): smallest; images that are no multiple of any chunk; a chunk boundary (4096) plus 4 elements per image; the element path
# with misaligned image starts; the 512^2 size (16 chunks per image)
SHAPES = ((1, 256), (3, 320), (2, 4100), (2, 1023), (2, 65536))
B, F = torch.bfloat16, torch.float32
# (shape, n_parts, v dtype, blend, eta, momentum, threshold); momentum -0.5 runs two consecutive calls, so that M is read
CASES = [
    ((1, 256), 2, F, False, 0.0, 0.0, True), ((1, 256), 3, B, True, 0.5, -0.5, False), ((1, 256), 3, F, True, 0.0, 0.0, True),
    ((1, 256), 2, B, False, 0.5, -0.5, True),
    ((3, 320), 3, F, False, 0.0, -0.5, True), ((3, 320), 2, B, True, 0.5, 0.0, True), ((3, 320), 2, F, True, 0.0, -0.5, False),
    ((3, 320), 3, B, False, 0.5, 0.0, False),
    ((2, 4100), 2, F, True, 0.5, -0.5, True), ((2, 4100), 3, B, False, 0.0, 0.0, True), ((2, 4100), 3, F, True, 0.5, 0.0, False),
    ((2, 4100), 2, B, False, 0.0, -0.5, False), ((2, 4100), 3, B, True, 0.0, -0.5, True),
    ((2, 1023), 3, F, True, 0.0, -0.5, True), ((2, 1023), 2, B, False, 0.5, 0.0, True), ((2, 1023), 2, F, False, 0.0, 0.0, False),
    ((2, 1023), 3, B, True, 0.5, -0.5, False), ((2, 1023), 2, F, True, 0.5, -0.5, True),
    ((2, 65536), 2, B, True, 0.0, -0.5, True), ((2, 65536), 3, F, False, 0.5, 0.0, True), ((2, 65536), 3, B, True, 0.0, 0.0, False),
    ((2, 65536), 2, F, False, 0.5, -0.5, False), ((2, 65536), 3, F, True, 0.0, -0.5, True),
]
assert {c[0] for c in CASES} == set(SHAPES)


def case_id(c):
    (b, e), parts, vdt, blend, eta, momentum, thr = c
    return f"{b}x{e}-{parts}parts-{'bf16' if vdt is B else 'f32'}-{'blend' if blend else 'step'}-eta{eta}-mom{momentum}-{'thr' if thr else 'nothr'}"


def f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def fma32(a, b, c):
    """float32(a * b + c) rounded once, as fmaf does: the product of two fp32 values is exact in long double, whose 64-bit significand leaves
    the sum one rounding 2^40 times finer than fp32's (where long double is double, 2^29 times: a tie is then still out of reach of these
    sizes in all but about one run in a thousand)"""
    LD = np.longdouble
    return (np.asarray(a, LD) * np.asarray(b, LD) + np.asarray(c, LD)).astype(np.float32)


def sentinel_f64(count, offset):
    """`count` doubles inside a sentinel-filled fp32 buffer, 2 * offset floats after its start (8-byte aligned): (buffer, the float64 view)"""
    buf = torch.empty(2 * offset + 2 * count + TAIL, dtype=torch.float32, device=DEV)
    bits(buf).fill_(SENT)
    return buf, buf[2 * offset:2 * offset + 2 * count].view(torch.float64)


def launch(ops, x, v, parts, scales, eta, thr, momentum, M_in, n_images, blend=None, sigma=SIGMA, ds=DS, sigma_next=SIGMA_NEXT, offset=0):
    """Two launches on copies of the same inputs: x's first part is `x`, the others junk (the kernel may not read them); x, v and M sit
    `offset` elements into sentinel buffers, sums and the workspace `offset` doubles into theirs. Asserts the footprint, that the parts left
    equal, that v and the blend operands came back unchanged and that the two launches agree bit for bit; returns (one part of x, M, sums)."""
    n = x.numel()
    outs = []
    for _ in range(2):
        junk = [randn(n, 90 + k) * 3.0 + 5.0 for k in range(parts - 1)]
        xb, xv = sentinel_buffer(torch.cat([x] + junk), offset)
        vb, vv = sentinel_buffer(v, offset)
        mb, mv = sentinel_buffer(M_in, offset)
        sb, sv = sentinel_f64(3 * n_images, offset)
        ws_count = ops.apg_workspace_bytes(n_images, n // n_images) // 8
        wb, wv = sentinel_f64(ws_count, offset)
        keep = [t.clone() for t in (vb,) + tuple(blend or ())]
        ops.euler_step_apg(xv, vv, sigma, ds, scales, eta, thr, momentum, mv, sv.view(n_images, 3), wv, blend, sigma_next)
        torch.cuda.synchronize()
        assert untouched(xb, offset, parts * n), "wrote outside x[0, n_parts n)"
        assert untouched(mb, offset, n), "wrote outside M[0, n)"
        assert untouched(sb, 2 * offset, 6 * n_images), "wrote outside sums"
        assert untouched(wb, 2 * offset, 2 * ws_count), "wrote outside the workspace"
        for name, a, b in zip(("v and the sentinels around it", "x0", "z", "m"), keep, (vb,) + tuple(blend or ())):
            assert torch.equal(bits(a), bits(b)), f"euler_step_apg changed {name}"
        for k in range(1, parts):
            assert torch.equal(bits(xv[:n]), bits(xv[k * n:(k + 1) * n])), f"part {k} differs from part 0"
        outs.append((xv[:n].clone(), mv.clone(), sv.clone()))
    for name, a, b in zip(("x", "M", "sums"), outs[0], outs[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"two launches on the same inputs differ in {name}"
    return outs[0]


def g0_ref(vs, scales):
    """(G0 exact, the bound on the kernel's g0): tests/test_cfg_kernels_gpu.py's step_bound and tests/test_brain_cfg_kernels_gpu.py's
    step_bound3 without their Euler step"""
    if len(vs) == 2:
        D = vs[0] - vs[1]
        G = vs[1] + scales[0] * D
        return G, U * (np.abs(scales[0] * D) + np.abs(G))
    s_b, s_t = scales
    DB = vs[0] - vs[1]
    GB = vs[1] + s_b * DB
    DT = GB - vs[2]
    G = vs[2] + s_t * DT
    return G, U * (abs(s_t) * (np.abs(s_b * DB) + np.abs(GB) + np.abs(DT)) + np.abs(G))


def db_ref(vs, scales, sigma, momentum, M_prev):
    """Db = (-sigma)(G0 - vc) + momentum M_prev exact, and the bound on the kernel's: dv = (g0 - vc)(1 + d1), D = -sigma dv (1 + d2),
    Db = (momentum M + D)(1 + d3): |Db - DB| <= sigma (|g0 - G0| + u |DV|) + u |D| + u |DB| (the last only with momentum)"""
    G0, bg = g0_ref(vs, scales)
    DV = G0 - vs[0]
    D = -sigma * DV
    bound = sigma * (bg + U * np.abs(DV)) + U * np.abs(D)
    if momentum == 0:
        return D, bound * O2
    DB = D + momentum * M_prev
    return DB, (bound + U * np.abs(DB)) * O2


def check_call(ops, x, vparts, scales, eta, thr, momentum, M_prev, n_images, blend, tag):
    """one call at offsets 0 and 1, everything the module docstring lists; returns (x, M, worst error / bound of x, the same of M)"""
    parts, n = len(vparts), x.numel()
    elems = n // n_images
    v = torch.cat(vparts)
    by_offset = []
    for offset in (0, 1):
        M_in = M_prev if momentum != 0 else torch.full((n,), float("nan"), device=DEV)
        by_offset.append(launch(ops, x, v, parts, scales, eta, thr, momentum, M_in, n_images, blend, offset=offset))
    for name, a, b in zip(("x", "M", "sums"), *by_offset):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{tag}: the 16-byte and the element path differ in {name}"
    got_x, got_M, got_sums = (t.cpu().numpy() for t in by_offset[0])
    got_sums = got_sums.reshape(n_images, 3)
    assert np.isfinite(got_x).all() and np.isfinite(got_M).all() and np.isfinite(got_sums).all(), f"{tag}: not finite"
    xs, vs = f64(x), [f64(p) for p in vparts]
    # M against the float64 Db of the inputs
    DB, bdb = db_ref(vs, scales, SIGMA, momentum, f64(M_prev))
    err = np.abs(got_M.astype(np.float64) - DB)
    worst_m = float((err / np.maximum(bdb, 1e-300)).max())
    assert (err <= bdb).all(), f"{tag}: {int((err > bdb).sum())} elements of M outside the rounding bound (worst {worst_m:.3f} of it)"
    # sums against the float64 sums of the kernel's own M and of w
    Db = got_M.astype(np.float64).reshape(n_images, elems)
    w = fma32(-SIGMA, vparts[0].float().cpu().numpy(), x.cpu().numpy()).astype(np.float64).reshape(n_images, elems)
    for k, terms in enumerate((Db * Db, Db * w, w * w)):
        want, tol = terms.sum(axis=1), elems * 2.0 ** -52 * np.abs(terms).sum(axis=1)
        assert (np.abs(got_sums[:, k] - want) <= tol).all(), f"{tag}: sums[:, {k}] = {got_sums[:, k]} against {want} (tolerance {tol})"
    # x against the exact value given the kernel's own M and sums
    S_dd, S_dw, S_ww = (got_sums[:, k:k + 1] for k in range(3))
    r = float(thr)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where((r > 0) & (S_dd > r * r), r / np.sqrt(S_dd), 1.0)
        a = np.where(S_ww > 0, S_dw / S_ww, 0.0)
    k = c * (1.0 - eta) * a
    W = (xs - SIGMA * vs[0]).reshape(n_images, elems)
    Uu = c * Db - k * W
    G = vs[0].reshape(n_images, elems) - Uu / SIGMA
    E = xs.reshape(n_images, elems) + DS * G
    bu = U * (np.abs(c * Db) + 3 * np.abs(k * W) + np.abs(Uu))
    bg = (bu + U * np.abs(Uu)) / SIGMA + U * np.abs(G)
    be = (abs(DS) * bg + U * np.abs(E)) * O2
    want, bound = E.reshape(n), be.reshape(n)
    if blend is not None:                 # tests/test_cfg_kernels_gpu.py's blend_bound, e's own error carried through with the weight m
        x0, z, m = (f64(t) for t in blend)
        sz, sx = SIGMA_NEXT * z, (1.0 - SIGMA_NEXT) * x0
        R = sz + sx
        want, bound = m * want + (1 - m) * R, m * bound + 4 * U * (np.abs(m * want) + np.abs((1 - m) * R) + (1 - m) * (np.abs(sz) + np.abs(sx)))
    err = np.abs(got_x.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), f"{tag}: {int((err > bound).sum())} elements of x outside the rounding bound (worst {worst:.3f} of it)"
    if eta == 0 and blend is None:
        # u is orthogonal to w up to what the bound allows: u recovered from x as sigma (vc - (e - x) / dsigma), whose error is
        # sigma be / |dsigma| per element (that holds |u - U| and the roundings of g and e). The exact U = c Db - k W has
        # sum W U = c (sum Db W - a sum W^2) with a = S_dw / S_ww taken over the fp32 w = W (1 + d): the two sums differ from S_dw and S_ww
        # by at most u sum |Db W| and 2 u sum W^2, which leaves |sum W U| <= u (|c| sum |Db W| + 2 |k| sum W^2).
        u_rec = SIGMA * (vs[0] - (got_x.astype(np.float64) - xs) / DS)
        dot = np.abs((W * u_rec.reshape(n_images, elems)).sum(axis=1))
        slack = (np.abs(W) * SIGMA * be / abs(DS)).sum(axis=1) + \
            U * O2 * (np.abs(c[:, 0]) * np.abs(Db * W).sum(axis=1) + 2 * np.abs(k[:, 0]) * (W * W).sum(axis=1))
        print(f"{tag}: |sum w u| / slack = {dot / slack}")
        assert (dot <= slack).all(), f"{tag}: eta = 0 but sum w u = {dot} (slack {slack})"
    return by_offset[0][0], by_offset[0][1], worst, worst_m


def inputs(shape, parts, vdt, seed):
    (n_images, elems), n = shape, shape[0] * shape[1]
    x = randn(n, seed + 1)
    vparts = [randn(n, seed + 2 + k, vdt) for k in range(parts)]
    blend = (randn(n, seed + 6), randn(n, seed + 7), choice(n, seed + 8, (0.0, 0.25, 1.0)))
    return x, vparts, blend


def spread_image0(vparts, elems, vdt, factor=4.0):
    """image 0's differences from the first branch scaled up, so that its update is the largest"""
    out = [vparts[0]]
    for p in vparts[1:]:
        p = p.clone()
        p[:elems] = (vparts[0][:elems].float() + factor * (p[:elems].float() - vparts[0][:elems].float())).to(vdt)
        out.append(p)
    return out


def threshold(vparts, scales, momentum, M_prev, n_images, sigma=SIGMA):
    """r from the reference's own |Db| per image: between image 0's and the largest of the others (one image: half its norm), as an fp32
    value; no image lies within 1e-3 relative of it, where one rounding could flip the comparison"""
    DB, _ = db_ref([f64(p) for p in vparts], scales, sigma, momentum, f64(M_prev))
    norms = np.sqrt((DB.reshape(n_images, -1) ** 2).sum(axis=1))
    r = f32(0.5 * norms[0] if n_images == 1 else np.sqrt(norms[0] * norms[1:].max()))
    assert norms[0] > r * (1 + 1e-3) and (norms[1:] < r * (1 - 1e-3)).all(), (norms, r)
    return r, norms


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_against_float64(ops, case):
    """N(0, 1) inputs, mask values in {0, 1/4, 1}, sigma = 0.7313, dsigma = -0.137, sigma_next = 0.5943, scale 3.5 or (2, 3.5).
    Worst measured error / bound on an MI355X: 0.887 for x (fp32 v, 2 x 65536, no blend) and 0.987 for M (the same case); 0.70 and 0.96 at
    2 x 1023; 0.69 and 0.59 or less at 1 x 256."""
    (n_images, elems), parts, vdt, with_blend, eta, momentum, with_thr = case
    scales, n = SCALES[parts], n_images * elems
    M = torch.zeros(n, device=DEV)
    worst, worst_m, x = 0.0, 0.0, None
    for call in range(2 if momentum != 0 else 1):
        x_in, vparts, blend = inputs((n_images, elems), parts, vdt, seed=100 * call)
        if x is not None:
            x_in = x                                           # (the second call goes on from the first one's latents and M)
        if with_thr:
            vparts = spread_image0(vparts, elems, vdt)
            thr, _ = threshold(vparts, scales, momentum, M, n_images)
        else:
            thr = 0.0
        x, M, w, wm = check_call(ops, x_in, vparts, scales, eta, thr, momentum, M, n_images, blend if with_blend else None,
                             f"{case_id(case)} call {call}")
        worst, worst_m = max(worst, w), max(worst_m, wm)
    print(f"euler_step_apg {case_id(case)}: worst error / bound = {worst:.3f} (x), {worst_m:.3f} (M)")


@pytest.mark.parametrize("vdt", [B, F], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("shape", [(1, 256), (2, 1023), (2, 4100)])
@pytest.mark.parametrize("parts", [2, 3])
def test_equal_branches_are_the_unguided_step_bit_for_bit(ops, shape, parts, vdt):
    """all branches equal: dv = 0, the sums of Db are 0, u = 0 and g = vc, whatever the scales, eta and the threshold: lx_euler_step, or
    lx_euler_step_blend, on a copy (N(0, 1) velocities: no zero whose sign could differ)"""
    n_images, n = shape[0], shape[0] * shape[1]
    x, (v, *_), blend = inputs(shape, parts, vdt, seed=300)
    euler, blended = x.clone(), x.clone()
    ops.euler_step(euler, v, DS)
    ops.euler_step_blend(blended, v, DS, *blend, SIGMA_NEXT)
    for scales, eta, thr in ((SCALES[parts], 0.0, 0.0), (SCALES[parts], 0.5, 2.0), ((7.5, -3.0)[:parts - 1], 1.0, 1e-3)):
        for offset in (0, 1):
            nan = torch.full((n,), float("nan"), device=DEV)
            got, M, sums = launch(ops, x, torch.cat([v] * parts), parts, scales, eta, thr, 0.0, nan, n_images, offset=offset)
            assert torch.equal(bits(got), bits(euler)), f"scales={scales} eta={eta}: not lx_euler_step"
            assert not bool(M.any()) and not bool(sums.view(n_images, 3)[:, :2].any())
            got, _, _ = launch(ops, x, torch.cat([v] * parts), parts, scales, eta, thr, 0.0, nan, n_images, blend, offset=offset)
            assert torch.equal(bits(got), bits(blended)), f"scales={scales} eta={eta}: not lx_euler_step_blend"


@pytest.mark.parametrize("vdt", [B, F], ids=["v_bf16", "v_f32"])
def test_kept_elements_are_the_source(ops, vdt):
    """m == 0 with sigma_next == 0: x0 in all parts (launch asserts the parts equal), whatever the branches predict; m == 1: the step"""
    shape = (2, 1023)
    x, vparts, (x0, z, _) = inputs(shape, 3, vdt, seed=400)
    n, v = x.numel(), torch.cat(vparts)
    zeros, ones, M0 = torch.zeros(n, device=DEV), torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
    for offset in (0, 1):
        got, _, _ = launch(ops, x, v, 3, SCALES[3], 0.0, 1.0, -0.5, M0, 2, (x0, z, zeros), sigma_next=0.0, offset=offset)
        assert torch.equal(bits(got), bits(x0))
        stepped, _, _ = launch(ops, x, v, 3, SCALES[3], 0.0, 1.0, -0.5, M0, 2, offset=offset)
        got, _, _ = launch(ops, x, v, 3, SCALES[3], 0.0, 1.0, -0.5, M0, 2, (x0, z, ones), offset=offset)
        assert torch.equal(bits(got), bits(stepped))


@pytest.mark.parametrize("shape", [(2, 4100), (2, 1023)])
def test_a_binding_threshold_bounds_the_update(ops, shape):
    """eta = 1, x = 0, vc = 0, sigma = 1, dsigma = -1: w = 0 and k = 0, g = fmaf(-1, u, 0) = -u and e = fmaf(-1, g, 0) = u exactly, so the
    kernel's own u is what it stores: |u| <= r (1 + 2^-20) for the image the threshold binds (image 0, update scaled up), and u = Db bit for
    bit for the image it leaves alone"""
    n_images, elems = shape
    n = n_images * elems
    zero = torch.zeros(n, device=DEV)
    vn = randn(n, 501)
    vn[:elems] *= 4.0
    r, norms = threshold([zero, vn], (3.5,), 0.0, zero, n_images, sigma=1.0)
    for offset in (0, 1):
        got, M, sums = launch(ops, zero, torch.cat([zero, vn]), 2, (3.5,), 1.0, r, 0.0, zero, n_images, sigma=1.0, ds=-1.0, offset=offset)
        u = got.double().view(n_images, elems)
        norm = u.pow(2).sum(dim=1).sqrt().cpu().numpy()
        print(f"binding threshold {shape} offset {offset}: |u| / r = {norm / r}, |Db| / r = {norms / r}")
        assert norm[0] <= r * (1 + 2.0 ** -20) and norm[0] >= r * (1 - 2.0 ** -20)
        assert torch.equal(bits(got[elems:]), bits(M[elems:])) and norm[1] < r


def test_refusals_through_the_wrapper(ops):
    """operands inside x[0, n_parts n) and an fp32 v on x are LxErrors that leave x as it was; so are a small workspace and bad values"""
    from loongx_amd._lib import LxError
    n = 1024
    buf = randn(5 * n, 51)
    x, was = buf[n:4 * n], buf.clone()
    v, z, m, M = randn(3 * n, 52), randn(n, 53), torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
    sums, ws = torch.zeros(1, 3, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV)
    good = dict(sigma=0.7, dsigma=-0.1, scales=(2.0, 3.0), eta=0.5, norm_threshold=1.0, momentum=-0.5, M=M, sums=sums, workspace=ws)
    for bad in (dict(M=x[2 * n:]), dict(inpaint=(x[n:2 * n], z, m)), dict(inpaint=(z, z, x[:n])), dict(workspace=ws[:2]), dict(eta=1.5),
                dict(norm_threshold=-1.0), dict(momentum=1.0), dict(sigma=0.0), dict(scales=(2.0, float("nan")))):
        with pytest.raises(LxError, match="lx_euler_step_apg"):
            ops.euler_step_apg(x, v, **dict(good, **bad))
    with pytest.raises(LxError, match="lx_euler_step_apg"):
        ops.euler_step_apg(x, buf[:3 * n], **good)
    with pytest.raises(AssertionError):
        ops.euler_step_apg(x, v, **dict(good, M=torch.zeros(n + 1, device=DEV)))
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(was)) and not bool(M.any()) and not bool(sums.any())
