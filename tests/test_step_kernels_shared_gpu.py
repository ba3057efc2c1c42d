"""The scheduler-step entry points share one kernel body and one 16-byte-path rule (csrc/step.hip). Two things follow that the tests of the
single entry points do not reach, and both are held bit for bit here:
  * a bf16 v that starts eight bytes past a 16-byte boundary takes the 16-byte path of EVERY entry (x, M, x0, z and m aligned), the inpaint
    step included: the result is that of the same data with every base one element in, which is the element path;
  * one body for one, two and three parts: three parts with vF == vT are two parts on [T; N], two parts with equal branches are the
    unguided step (or the inpaint step, with the blend), and the inpaint step with m == 1 is the unguided step up to the sign of a zero.
    `step_parts` is the one place where a further part count is added."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_apg_kernels_gpu import sentinel_f64  # noqa: E402
from tests.test_cfg_kernels_gpu import sentinel_buffer, untouched  # noqa: E402
from tests.test_inpaint_kernels_gpu import DEV, bits, choice, f32, ops, randn  # noqa: E402,F401  (ops: the fixture)

DS, SIGMA, SIGMA_NEXT = f32(-0.137), f32(0.7551), f32(0.6183)
SCALES = (2.0, 3.5)                                # (scale_brain, scale_text); two parts take the last one
APG = dict(eta=0.25, norm_threshold=1.5, momentum=0.5)


def step_parts(ops, parts, x, v, scales, blend):
    """the step on `parts` parts of x and v, in place: the entry point that part count has; scales holds parts - 1 values"""
    assert len(scales) == parts - 1
    if parts == 1 and blend is None:
        ops.euler_step(x, v, DS)
    elif parts == 1:
        ops.euler_step_blend(x, v, DS, *blend, SIGMA_NEXT)
    elif parts == 2:
        ops.euler_step_cfg(x, v, DS, scales[0], blend, SIGMA_NEXT)
    else:
        ops.euler_step_cfg3(x, v, DS, scales[0], scales[1], blend, SIGMA_NEXT)


def run(ops, x, vparts, blend, offset, v_offset, scales=None, apg_images=0):
    """One launch. x's first part is `x`, the others junk; x, M and the blend operands sit `offset` elements into sentinel buffers, v
    `v_offset` elements into its own. Asserts the footprint on x (and M) and that the parts left equal; returns (x's first part, M, sums) and
    the addresses of x and v."""
    parts, n = len(vparts), x.numel()
    xb, xv = sentinel_buffer(torch.cat([x] + [randn(n, 90 + k) * 3.0 + 5.0 for k in range(parts - 1)]), offset)
    vb, vv = sentinel_buffer(torch.cat(vparts), v_offset)
    held = None if blend is None else [sentinel_buffer(t, offset) for t in blend]
    bl = None if held is None else tuple(view for _, view in held)
    M = sums = None
    if apg_images:
        mb, M = sentinel_buffer(randn(n, 77), offset)
        _, sums = sentinel_f64(3 * apg_images, offset)
        _, ws = sentinel_f64(ops.apg_workspace_bytes(apg_images, n // apg_images) // 8, offset)
        ops.euler_step_apg(xv, vv, SIGMA, DS, scales, APG["eta"], APG["norm_threshold"], APG["momentum"], M, sums.view(apg_images, 3), ws, bl,
                           SIGMA_NEXT)
    else:
        step_parts(ops, parts, xv, vv, scales if scales is not None else SCALES[3 - parts:], bl)
    torch.cuda.synchronize()
    assert untouched(xb, offset, parts * n), "wrote outside x"
    assert untouched(vb, v_offset, parts * n), "wrote around v"
    if apg_images:
        assert untouched(mb, offset, n), "wrote outside M"
    for k in range(1, parts):
        assert torch.equal(bits(xv[:n]), bits(xv[k * n:(k + 1) * n])), f"part {k} differs from part 0"
    out = (xv[:n].clone(), None if M is None else M.clone(), None if sums is None else sums.clone())
    return out, xv.data_ptr(), vv.data_ptr()


def operands(n, parts, vdt, seed):
    x = randn(n, seed)
    vparts = [randn(n, seed + 1 + k, vdt) for k in range(parts)]
    blend = (randn(n, seed + 5), randn(n, seed + 6), choice(n, seed + 7, (0.0, 0.25, 1.0)))
    return x, vparts, blend


# (id, parts, images of an APG call or 0, sizes of one image, with / without the blend)
HALF_ALIGNED = [("blend", 1, 0, (8, 1027, 1028), (True,)),                  # 1027: the element tail behind whole items
                ("cfg", 2, 0, (8, 1028), (False, True)),
                ("cfg3", 3, 0, (8, 1028), (False, True)),
                ("apg2-1img", 2, 1, (8, 1028), (False, True)),
                ("apg2-2img", 2, 2, (8, 1028), (False, True)),
                ("apg3-1img", 3, 1, (8, 1028), (False, True)),
                ("apg3-2img", 3, 2, (8, 1028), (False, True))]


@pytest.mark.parametrize("case", HALF_ALIGNED, ids=[c[0] for c in HALF_ALIGNED])
def test_bf16_v_eight_bytes_past_a_16_byte_boundary(ops, case):
    _, parts, images, sizes, blends = case
    for elems in sizes:
        n = elems * max(images, 1)
        x, vparts, blend = operands(n, parts, torch.bfloat16, seed=100 + elems)
        for with_blend in blends:
            kw = dict(scales=SCALES[3 - parts:], apg_images=images)
            got, x_at, v_at = run(ops, x, vparts, blend if with_blend else None, 0, 4, **kw)
            assert x_at % 16 == 0 and v_at % 16 == 8
            want, x_at, v_at = run(ops, x, vparts, blend if with_blend else None, 1, 1, **kw)
            assert x_at % 16 == 4 and v_at % 4 == 2
            for name, a, b in zip(("x", "M", "sums"), got, want):
                if a is not None:
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                        f"elems={elems} blend={with_blend}: {name} differs between the half-aligned and the element path"


@pytest.mark.parametrize("vdt", [torch.bfloat16, torch.float32], ids=["v_bf16", "v_f32"])
@pytest.mark.parametrize("n", [5, 1028])
def test_one_body_three_part_counts(ops, n, vdt):
    x, (vt, vn, _), blend = operands(n, 3, vdt, seed=200 + n)
    for bl in (None, blend):
        # a first branch equal to the second drops out: `parts` parts are parts - 1 parts on what is left
        for parts, vs in ((3, [vt, vt, vn]), (2, [vn, vn])):
            more = run(ops, x, vs, bl, 0, 0, scales=SCALES[3 - parts:])[0][0]
            fewer = run(ops, x, vs[1:], bl, 0, 0, scales=SCALES[4 - parts:])[0][0]
            assert torch.equal(bits(more), bits(fewer)), f"{parts} parts with equal first branches are not {parts - 1} parts (blend={bl is not None})"
    # m == 1: the blend adds (1 - m) r = +-0 to the stepped value, which changes nothing but the sign of a zero
    plain = run(ops, x, [vn], None, 0, 0)[0][0]
    ones = run(ops, x, [vn], blend[:2] + (torch.ones(n, device=DEV),), 0, 0)[0][0]
    nonzero = plain != 0
    assert torch.equal(nonzero, ones != 0) and torch.equal(bits(plain)[nonzero], bits(ones)[nonzero])
