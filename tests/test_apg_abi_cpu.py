"""lx_euler_step_apg and lx_apg_workspace_bytes through the C ABI, without a GPU: both symbols are exported under the same ABI version, and
every refusal of include/lx.h returns LX_ERR_INVALID (-1) before any launch and names the entry point in lx_last_error(). The addresses are
fake and aligned, and every call made here is one that must be refused, so none is dereferenced."""
import ctypes

import pytest

A, IMAGES, ELEMS = 0x100000, 2, 512                 # x at A: 3 parts of 2 x 512 floats = 0x3000 bytes; the other operands 0x10000 apart
N = IMAGES * ELEMS
F = ctypes.c_float


def ws_bytes(n_images=IMAGES, elems=ELEMS):
    from loongx_amd._lib import lib
    return lib.lx_apg_workspace_bytes(n_images, elems)


def call(x=A, v=A + 0x10000, bf16=0, n_parts=3, scale_a=2.0, scale_b=3.0, sigma=0.7, eta=0.5, thr=1.5, momentum=-0.5, M=A + 0x20000,
         sums=A + 0x30000, ws=A + 0x40000, ws_bytes_=None, x0=None, z=None, m=None, n_images=IMAGES, elems=ELEMS):
    from loongx_amd._lib import lib
    if ws_bytes_ is None:
        ws_bytes_ = max(ws_bytes(n_images, elems), 48)
    status = lib.lx_euler_step_apg(x, v, bf16, n_parts, F(scale_a), F(scale_b), F(sigma), F(-0.1), F(eta), F(thr), F(momentum), M, sums, ws,
                                   ws_bytes_, x0, z, m, F(0.5), n_images, elems, None)
    return status, lib.lx_last_error()


def refused(**kw):
    status, msg = call(**kw)
    return status == -1 and b"lx_euler_step_apg" in msg


BLEND = dict(x0=A + 0x50000, z=A + 0x60000, m=A + 0x70000)
NOT_FINITE = [float("nan"), float("inf"), float("-inf")]


def test_the_symbols_are_exported_under_the_same_abi_version():
    from loongx_amd import _lib
    for name in ("lx_euler_step_apg", "lx_apg_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.lib.lx_version() == 404


def test_workspace_bytes():
    """3 doubles per chunk of 4096 elements per image; 0 on arguments the step refuses"""
    assert ws_bytes(1, 1) == 24 and ws_bytes(1, 4096) == 24 and ws_bytes(1, 4097) == 48 and ws_bytes(3, 65536) == 3 * 16 * 24
    assert ws_bytes(0, 512) == 0 and ws_bytes(-1, 512) == 0 and ws_bytes(2, 0) == 0
    assert ws_bytes(2, 2 ** 63) == 0 and ws_bytes(65536, 4) == 0


@pytest.mark.parametrize("which", ["x", "v", "M", "sums", "ws"])
def test_null_operands(which):
    assert refused(**{which: None}) and refused(**{which: None}, **BLEND)


def test_parts_and_sizes():
    for n_parts in (0, 1, 4, -2):
        assert refused(n_parts=n_parts)
    assert refused(n_images=0) and refused(n_images=-1) and refused(elems=0) and refused(n_images=65536, elems=4)
    assert refused(elems=2 ** 62)


@pytest.mark.parametrize("bad", NOT_FINITE + [0.0, -0.5])
def test_sigma(bad):
    assert refused(sigma=bad) and refused(sigma=bad, **BLEND)


@pytest.mark.parametrize("bad", NOT_FINITE)
def test_values_that_are_not_finite(bad):
    for name in ("scale_a", "scale_b", "eta", "thr", "momentum"):
        assert refused(**{name: bad}), name
    assert refused(scale_a=bad, n_parts=2)
    status, msg = call(scale_b=bad, n_parts=2, eta=2.0)          # (scale_b is ignored with two parts: refused for eta, not for the scale)
    assert status == -1 and b"eta" in msg


def test_ranges():
    for eta in (-0.001, 1.001, 2.0):
        assert refused(eta=eta)
    assert refused(thr=-1e-6) and refused(thr=-3.0)
    for momentum in (1.0, -1.0, 1.5, -7.0):
        assert refused(momentum=momentum)


@pytest.mark.parametrize("given", [("x0",), ("z",), ("m",), ("x0", "z"), ("x0", "m"), ("z", "m")])
def test_a_partly_null_blend_triple(given):
    assert refused(**{k: BLEND[k] for k in given})


def test_the_workspace():
    need = ws_bytes()
    assert need == 2 * 24
    assert refused(ws_bytes_=need - 1) and refused(ws_bytes_=0)
    assert refused(ws=A + 0x40004) and refused(sums=A + 0x30004)          # (doubles: 8-byte aligned)


@pytest.mark.parametrize("n_parts", [2, 3])
@pytest.mark.parametrize("which", ["M", "x0", "z", "m"])
def test_part_sized_operands_on_x(which, n_parts):
    """[n] floats that touch x[0, n_parts n): the same address, a later part, x's last element, or ending on x's first"""
    for delta in (0, 4 * N, 4 * (n_parts - 1) * N, 4 * (n_parts * N - 1), -4 * (N - 1)):
        assert refused(n_parts=n_parts, **dict(BLEND, **{which: A + delta})), delta


@pytest.mark.parametrize("which,size", [("sums", IMAGES * 24), ("ws", 48)])
def test_sums_and_workspace_on_x(which, size):
    for delta in (0, 4 * N, 4 * 3 * N - 8, 8 - size):
        assert refused(**{which: A + delta}), delta


def test_operands_next_to_x_are_not_what_is_refused():
    """the overlap test is exact: operands that end where x begins, or begin where x[3n) ends, pass it -- shown on a call refused for a
    reason that is checked later (M on v), by the message naming that reason"""
    for which, before in (("x0", 4 * N), ("sums", IMAGES * 24)):
        for delta in (-before, 4 * 3 * N):
            status, msg = call(v=A + 0x20000, **dict(BLEND, **{which: A + delta}))
            assert status == -1 and b"may not overlap v" in msg, (which, delta)


@pytest.mark.parametrize("delta", [0, 4 * (3 * N - 1), -4 * (3 * N - 1)])
def test_fp32_v_on_x(delta):
    assert refused(v=A + delta)
