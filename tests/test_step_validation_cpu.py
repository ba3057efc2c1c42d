"""CPU-only: what the scheduler-step entry points (lx_euler_step, lx_scale_noise, lx_euler_step_blend, lx_euler_step_cfg, lx_euler_step_cfg3,
lx_euler_step_apg; lx_apg_workspace_bytes) reject on the host, which status they return and the complete lx_last_error() text, check order
included (the method of test_vae_validation_cpu.py). The addresses are fake and aligned, and every call here returns before any launch:
it is refused, or it is one of the n == 0 calls that three of the entries accept as nothing to do. Where an entry ACCEPTS a value that a
check would refuse one element further, the accepting call carries a later defect and the test pins that later message."""
import pytest

from loongx_amd import _lib

A = 0x100000                  # x (or out); the other operands follow 0x10000 apart
V, X0, Z, MASK, MOM, SUMS, WS = (A + k * 0x10000 for k in range(1, 8))
N = 1024                      # one part: 0x1000 bytes
INF, NAN = float("inf"), float("nan")
NOT_FINITE = (NAN, INF, -INF)


def _rejected(status, text):
    assert status == -1                  # LX_ERR_INVALID
    assert _lib.lib.lx_last_error().decode() == text


# ---- lx_euler_step, lx_scale_noise --------------------------------------------------------------------------------------------
def _step(x=A, v=V, bf16=0, n=N):
    return _lib.lib.lx_euler_step(x, v, bf16, -0.1, n, None)


def test_euler_step():
    _rejected(_step(x=None), "lx_euler_step: NULL operand")
    _rejected(_step(v=None), "lx_euler_step: NULL operand")
    _rejected(_step(v=None, n=0), "lx_euler_step: NULL operand")         # the operands come before the count
    assert _step(n=0) == 0                                               # LX_OK, nothing launched
    assert _step(v=A, n=0) == 0


def _noise(out=A, x0=X0, z=Z, n=N):
    return _lib.lib.lx_scale_noise(out, x0, z, 0.7, n, None)


def test_scale_noise():
    e = "lx_scale_noise"
    for op in ("out", "x0", "z"):
        _rejected(_noise(**{op: None}), f"{e}: NULL operand")
    for op in ("x0", "z"):
        for delta in (0, 4 * (N - 1), -4 * (N - 1), 4):
            _rejected(_noise(**{op: A + delta}), f"{e}: x0 and z may not alias out")
    _rejected(_noise(out=None, z=A), f"{e}: NULL operand")
    _rejected(_noise(x0=None, n=0), f"{e}: NULL operand")
    assert _noise(n=0) == 0
    assert _noise(x0=A, z=A, n=0) == 0                                   # empty ranges share no address


# ---- lx_euler_step_blend --------------------------------------------------------------------------------------------------------
def _blend(x=A, v=V, bf16=0, x0=X0, z=Z, m=MASK, n=N):
    return _lib.lib.lx_euler_step_blend(x, v, bf16, -0.1, x0, z, m, 0.5, n, None)


def test_euler_step_blend():
    e = "lx_euler_step_blend"
    for op in ("x", "v", "x0", "z", "m"):
        _rejected(_blend(**{op: None}), f"{e}: NULL operand")
    for op in ("x0", "z", "m"):
        for delta in (0, 4 * (N - 1), -4 * (N - 1)):
            _rejected(_blend(**{op: A + delta}), f"{e}: x0, z and m may not alias x (it is updated in place)")
    # order: operands, aliasing, the count
    _rejected(_blend(v=None, x0=A), f"{e}: NULL operand")
    _rejected(_blend(m=None, n=0), f"{e}: NULL operand")
    assert _blend(n=0) == 0
    assert _blend(bf16=1, n=0) == 0
    assert _blend(v=A, x0=A, n=0) == 0


# ---- lx_euler_step_cfg, lx_euler_step_cfg3 ------------------------------------------------------------------------------------
BLEND = dict(x0=X0, z=Z, m=MASK)
GUIDED = (("lx_euler_step_cfg", 2), ("lx_euler_step_cfg3", 3))


def _guided(entry, x=A, v=V, bf16=0, scales=(2.0, 3.0), x0=None, z=None, m=None, n=N):
    if entry == "lx_euler_step_cfg":
        return _lib.lib.lx_euler_step_cfg(x, v, bf16, -0.1, scales[0], x0, z, m, 0.5, n, None)
    return _lib.lib.lx_euler_step_cfg3(x, v, bf16, -0.1, scales[0], scales[1], x0, z, m, 0.5, n, None)


def _not_finite_text(entry):
    return f"{entry}: scale is not finite" if entry == "lx_euler_step_cfg" else f"{entry}: scale_brain or scale_text is not finite"


@pytest.mark.parametrize("entry,parts", GUIDED)
def test_guided_operands_and_count(entry, parts):
    for over in (dict(x=None), dict(v=None), dict(x=None, v=None), dict(x=None, **BLEND)):
        _rejected(_guided(entry, **over), f"{entry}: NULL x or v")
    _rejected(_guided(entry, n=0), f"{entry}: n == 0")
    _rejected(_guided(entry, n=0, **BLEND), f"{entry}: n == 0")
    for given in (("x0",), ("z",), ("m",), ("x0", "z"), ("x0", "m"), ("z", "m")):
        _rejected(_guided(entry, **{k: BLEND[k] for k in given}), f"{entry}: x0, z and m go together (all NULL: no blend)")


def test_cfg3_size():
    e = "lx_euler_step_cfg3"
    _rejected(_guided(e, n=2 ** 64 // 12 + 1), f"{e}: 3n elements do not fit an address")
    _rejected(_guided(e, n=2 ** 63), f"{e}: 3n elements do not fit an address")
    # the largest count that fits is accepted: refused for what comes next
    _rejected(_guided(e, n=2 ** 64 // 12, x0=X0), f"{e}: x0, z and m go together (all NULL: no blend)")


@pytest.mark.parametrize("entry,parts", GUIDED)
def test_guided_scales(entry, parts):
    for bad in NOT_FINITE:
        _rejected(_guided(entry, scales=(bad, 3.0)), _not_finite_text(entry))
        _rejected(_guided(entry, scales=(bad, 3.0), **BLEND), _not_finite_text(entry))
        if parts == 3:
            _rejected(_guided(entry, scales=(2.0, bad)), _not_finite_text(entry))
    # every finite value is a scale: 0, negative, huge -- shown on calls refused for fp32 v on x, which is checked later
    for ok in (0.0, -1.0, 3.0e38):
        _rejected(_guided(entry, scales=(ok, ok), v=A), f"{entry}: v may not alias x[0, {parts}n)")


@pytest.mark.parametrize("entry,parts", GUIDED)
def test_guided_aliasing(entry, parts):
    x0zm = f"{entry}: x0, z and m may not alias x[0, {parts}n) (it is updated in place)"
    v_on_x = f"{entry}: v may not alias x[0, {parts}n)"
    for op in ("x0", "z", "m"):
        # the same address, a later part, x's last element, ending on x's first element
        for delta in (0, 4 * N, 4 * (parts - 1) * N, 4 * (parts * N - 1), -4 * (N - 1)):
            _rejected(_guided(entry, **dict(BLEND, **{op: A + delta})), x0zm)
            _rejected(_guided(entry, bf16=1, **dict(BLEND, **{op: A + delta})), x0zm)
        # ending where x begins, beginning where x ends: accepted (the call is refused for v, checked next)
        for delta in (-4 * N, 4 * parts * N):
            _rejected(_guided(entry, v=A, **dict(BLEND, **{op: A + delta})), v_on_x)
    for delta in (0, 4 * (parts * N - 1), -4 * (parts * N - 1)):
        _rejected(_guided(entry, v=A + delta), v_on_x)
        _rejected(_guided(entry, v=A + delta, **BLEND), v_on_x)


@pytest.mark.parametrize("entry,parts", GUIDED)
def test_guided_order(entry, parts):
    """operands, count, (size,) triple, scales, x0 / z / m on x, v on x"""
    triple = f"{entry}: x0, z and m go together (all NULL: no blend)"
    _rejected(_guided(entry, v=None, n=0, x0=X0, scales=(NAN, NAN)), f"{entry}: NULL x or v")
    _rejected(_guided(entry, n=0, x0=X0, scales=(NAN, NAN)), f"{entry}: n == 0")
    _rejected(_guided(entry, x0=X0, scales=(NAN, NAN), v=A), triple)
    _rejected(_guided(entry, scales=(NAN, NAN), v=A, **dict(BLEND, z=A)), _not_finite_text(entry))
    _rejected(_guided(entry, v=A, **dict(BLEND, z=A)), f"{entry}: x0, z and m may not alias x[0, {parts}n) (it is updated in place)")
    if parts == 3:
        _rejected(_guided(entry, n=2 ** 63, x0=X0), f"{entry}: 3n elements do not fit an address")


# ---- lx_euler_step_apg, lx_apg_workspace_bytes ----------------------------------------------------------------------------------
IMAGES, ELEMS = 2, 512        # a part: 2 images of 512 elements = N


def _apg(x=A, v=V, bf16=0, n_parts=3, scale_a=2.0, scale_b=3.0, sigma=0.7, eta=0.5, thr=1.5, momentum=-0.5, M=MOM, sums=SUMS, ws=WS,
         ws_bytes=48, x0=None, z=None, m=None, n_images=IMAGES, elems=ELEMS):
    return _lib.lib.lx_euler_step_apg(x, v, bf16, n_parts, scale_a, scale_b, sigma, -0.1, eta, thr, momentum, M, sums, ws, ws_bytes, x0, z, m,
                                      0.5, n_images, elems, None)


E = "lx_euler_step_apg"
APG_NULL = f"{E}: NULL x, v, M, sums or workspace"
APG_SIZES = f"{E}: n_images < 1 or elems == 0"
APG_FIT = f"{E}: more than 65535 images, or the parts do not fit an address"
APG_SIGMA = f"{E}: sigma must be finite and > 0"
APG_SCALE = f"{E}: a scale is not finite"
APG_FINITE = f"{E}: eta, norm_threshold or momentum is not finite"
APG_ETA = f"{E}: eta must lie in [0, 1]"
APG_THR = f"{E}: norm_threshold must be >= 0"
APG_MOMENTUM = f"{E}: |momentum| must be < 1"
APG_TRIPLE = f"{E}: x0, z and m go together (all NULL: no blend)"
APG_WS = f"{E}: the workspace is smaller than lx_apg_workspace_bytes"
APG_ALIGN = f"{E}: the workspace and sums must be 8-byte aligned"
APG_STATE_ON_X = f"{E}: M, sums and the workspace may not overlap x[0, n_parts n)"
APG_X0ZM = f"{E}: x0, z and m may not alias x[0, n_parts n) (it is updated in place)"
APG_V_ON_X = f"{E}: v may not alias x[0, n_parts n)"
APG_M_ON_V = f"{E}: M may not overlap v (it is written while v is read)"


def test_apg_workspace_bytes():
    """3 doubles per chunk of 4096 elements per image; 0 where the step refuses the sizes"""
    ws = _lib.lib.lx_apg_workspace_bytes
    assert ws(1, 0) == 0 and ws(0, 1) == 0
    assert ws(1, 1) == 24
    assert ws(1, 4096) == 24 and ws(1, 4097) == 48                       # one chunk, two chunks
    assert ws(2, 4096) == 48 and ws(2, 4097) == 96


def test_apg_operands_parts_sizes():
    for op in ("x", "v", "M", "sums", "ws"):
        _rejected(_apg(**{op: None}), APG_NULL)
        _rejected(_apg(**{op: None}, **BLEND), APG_NULL)
    for n_parts in (0, 1, 4, -2):
        _rejected(_apg(n_parts=n_parts), f"{E}: n_parts={n_parts} must be 2 or 3")
    for over in (dict(n_images=0), dict(n_images=-1), dict(elems=0)):
        _rejected(_apg(**over), APG_SIZES)
    for over in (dict(n_images=65536, elems=4), dict(elems=2 ** 62), dict(n_images=1, elems=2 ** 64 // 12 + 1)):
        _rejected(_apg(**over), APG_FIT)


def test_apg_values():
    for bad in NOT_FINITE + (0.0, -0.5):
        _rejected(_apg(sigma=bad), APG_SIGMA)
    for bad in NOT_FINITE:
        _rejected(_apg(scale_a=bad), APG_SCALE)
        _rejected(_apg(scale_b=bad), APG_SCALE)
        _rejected(_apg(scale_a=bad, n_parts=2), APG_SCALE)
        _rejected(_apg(scale_b=bad, n_parts=2, eta=2.0), APG_ETA)          # scale_b is not read with two parts
        for name in ("eta", "thr", "momentum"):
            _rejected(_apg(**{name: bad}), APG_FINITE)
    for eta in (-0.001, 1.001, 2.0):
        _rejected(_apg(eta=eta), APG_ETA)
    for thr in (-1e-6, -3.0):
        _rejected(_apg(thr=thr), APG_THR)
    for momentum in (1.0, -1.0, 1.5, -7.0):
        _rejected(_apg(momentum=momentum), APG_MOMENTUM)
    # the ends of the ranges are accepted: eta 0 and 1, norm_threshold 0 -- refused for the workspace, checked later
    for over in (dict(eta=0.0), dict(eta=1.0), dict(thr=0.0), dict(momentum=0.0)):
        _rejected(_apg(ws_bytes=47, **over), APG_WS)


def test_apg_triple_workspace_alignment():
    for given in (("x0",), ("z",), ("m",), ("x0", "z"), ("x0", "m"), ("z", "m")):
        _rejected(_apg(**{k: BLEND[k] for k in given}), APG_TRIPLE)
    _rejected(_apg(ws_bytes=47), APG_WS)
    _rejected(_apg(ws_bytes=0), APG_WS)
    _rejected(_apg(elems=4097, ws_bytes=95), APG_WS)
    _rejected(_apg(ws=WS + 4), APG_ALIGN)
    _rejected(_apg(sums=SUMS + 4), APG_ALIGN)
    # a larger workspace and the exact size at a chunk boundary are accepted: refused for the alignment, checked next
    _rejected(_apg(ws_bytes=1 << 20, sums=SUMS + 4), APG_ALIGN)
    _rejected(_apg(elems=4096, ws_bytes=48, sums=SUMS + 4), APG_ALIGN)


@pytest.mark.parametrize("n_parts", [2, 3])
def test_apg_aliasing(n_parts):
    x_end = 4 * n_parts * N
    for delta in (0, 4 * N, x_end - 4, -4 * (N - 1)):
        _rejected(_apg(n_parts=n_parts, M=A + delta), APG_STATE_ON_X)
        for op in ("x0", "z", "m"):
            _rejected(_apg(n_parts=n_parts, **dict(BLEND, **{op: A + delta})), APG_X0ZM)
    for op, size in (("sums", IMAGES * 24), ("ws", 48)):
        for delta in (0, 4 * N, x_end - 8, 8 - size):
            _rejected(_apg(n_parts=n_parts, **{op: A + delta}), APG_STATE_ON_X)
    for delta in (0, x_end - 4, 4 - x_end):
        _rejected(_apg(n_parts=n_parts, v=A + delta), APG_V_ON_X)
    # M on v: fp32 v has n_parts n floats, bf16 v half the bytes
    for delta in (0, x_end - 4, -4 * (N - 1)):
        _rejected(_apg(n_parts=n_parts, M=V + delta), APG_M_ON_V)
    for delta in (0, x_end // 2 - 4, -4 * (N - 1)):
        _rejected(_apg(n_parts=n_parts, bf16=1, M=V + delta), APG_M_ON_V)
    # operands that end where x begins, or begin where x ends, pass the checks on x: the call is refused for M on v, checked last
    for op, before in (("x0", 4 * N), ("sums", IMAGES * 24), ("ws", 48)):
        for delta in (-before, x_end):
            _rejected(_apg(n_parts=n_parts, M=V, **dict(BLEND, **{op: A + delta})), APG_M_ON_V)


def test_apg_order():
    """operands, n_parts, sizes, fit, sigma, scales, finite values, eta, norm_threshold, momentum, triple, workspace size, alignment, state on
    x, x0 / z / m on x, v on x, M on v: each call breaks one rule and every later one it can"""
    late = dict(eta=2.0, thr=-1.0, momentum=1.0, x0=X0, ws_bytes=0, sums=SUMS + 4)
    _rejected(_apg(x=None, n_parts=4, n_images=0, sigma=NAN, scale_a=NAN, **late), APG_NULL)
    _rejected(_apg(n_parts=4, n_images=0, sigma=NAN, scale_a=NAN, **late), f"{E}: n_parts=4 must be 2 or 3")
    _rejected(_apg(n_images=0, sigma=NAN, scale_a=NAN, **late), APG_SIZES)
    _rejected(_apg(elems=2 ** 62, sigma=NAN, scale_a=NAN, **late), APG_FIT)
    _rejected(_apg(sigma=NAN, scale_a=NAN, **late), APG_SIGMA)
    _rejected(_apg(scale_a=NAN, **dict(late, eta=NAN)), APG_SCALE)
    _rejected(_apg(**dict(late, thr=NAN)), APG_FINITE)
    _rejected(_apg(**late), APG_ETA)
    _rejected(_apg(**dict(late, eta=0.5)), APG_THR)
    _rejected(_apg(**dict(late, eta=0.5, thr=0.0)), APG_MOMENTUM)
    _rejected(_apg(x0=X0, ws_bytes=0, sums=SUMS + 4), APG_TRIPLE)
    _rejected(_apg(ws_bytes=0, sums=SUMS + 4, M=A), APG_WS)
    _rejected(_apg(sums=SUMS + 4, M=A), APG_ALIGN)
    _rejected(_apg(M=A, v=A, **dict(BLEND, z=A)), APG_STATE_ON_X)
    _rejected(_apg(v=A, **dict(BLEND, z=A)), APG_X0ZM)
    _rejected(_apg(v=A + 4 * 2 * N, M=A + 4 * 3 * N), APG_V_ON_X)       # v on x's last part, M behind x and on v
