"""lx_dpmpp2m_step and lx_dpmpp2m_step_apg through the C ABI, without a GPU: both symbols are exported under the same ABI version, and every
refusal of include/lx.h returns LX_ERR_INVALID (-1) before any launch and names the entry point in lx_last_error(). The addresses are fake
and aligned, and every call made here is one that must be refused, so none is dereferenced. The pattern of tests/test_apg_abi_cpu.py."""
import ctypes

import pytest

A, IMAGES, ELEMS = 0x100000, 2, 512                 # x at A: 3 parts of 2 x 512 floats = 0x3000 bytes; the other operands 0x10000 apart
N = IMAGES * ELEMS
F = ctypes.c_float
BLEND = dict(x0=A + 0x50000, z=A + 0x60000, m=A + 0x70000)
NOT_FINITE = [float("nan"), float("inf"), float("-inf")]


def step(x=A, v=A + 0x10000, bf16=0, n_parts=3, scale_a=2.0, scale_b=3.0, sigma=0.7, c=0.25, D=A + 0x80000, x0=None, z=None, m=None, n=N):
    from loongx_amd._lib import lib
    status = lib.lx_dpmpp2m_step(x, v, bf16, n_parts, F(scale_a), F(scale_b), F(sigma), F(-0.1), F(c), D, x0, z, m, F(0.5), n, None)
    return status, lib.lx_last_error()


def step_apg(x=A, v=A + 0x10000, bf16=0, n_parts=3, scale_a=2.0, scale_b=3.0, sigma=0.7, c=0.25, D=A + 0x80000, eta=0.5, thr=1.5,
             momentum=-0.5, M=A + 0x20000, sums=A + 0x30000, ws=A + 0x40000, ws_bytes=48, x0=None, z=None, m=None, n_images=IMAGES,
             elems=ELEMS):
    from loongx_amd._lib import lib
    status = lib.lx_dpmpp2m_step_apg(x, v, bf16, n_parts, F(scale_a), F(scale_b), F(sigma), F(-0.1), F(c), D, F(eta), F(thr), F(momentum), M,
                                     sums, ws, ws_bytes, x0, z, m, F(0.5), n_images, elems, None)
    return status, lib.lx_last_error()


ENTRIES = {"lx_dpmpp2m_step": step, "lx_dpmpp2m_step_apg": step_apg}


def refused(entry, **kw):
    status, msg = ENTRIES[entry](**kw)
    # (the APG entry's name contains the plain one's: the message has to name the entry that was called, up to its colon)
    return status == -1 and msg.startswith(entry.encode() + b":")


both = pytest.mark.parametrize("entry", list(ENTRIES))


def test_the_symbols_are_exported_under_the_same_abi_version():
    from loongx_amd import _lib
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.lib.lx_version() == 404


@both
@pytest.mark.parametrize("which", ["x", "v", "D"])
def test_null_operands(entry, which):
    assert refused(entry, **{which: None}) and refused(entry, **{which: None}, **BLEND)


@pytest.mark.parametrize("which", ["M", "sums", "ws"])
def test_null_operands_of_the_apg_entry(which):
    assert refused("lx_dpmpp2m_step_apg", **{which: None})


def test_parts_and_sizes():
    for n_parts in (0, 4, -2):
        assert refused("lx_dpmpp2m_step", n_parts=n_parts)
    for n_parts in (0, 1, 4, -2):
        assert refused("lx_dpmpp2m_step_apg", n_parts=n_parts)
    assert refused("lx_dpmpp2m_step", n=0) and refused("lx_dpmpp2m_step", n=0, n_parts=1)
    assert refused("lx_dpmpp2m_step", n=2 ** 62) and refused("lx_dpmpp2m_step", n=2 ** 62, n_parts=1)      # (3n floats past an address)
    assert refused("lx_dpmpp2m_step_apg", n_images=0) and refused("lx_dpmpp2m_step_apg", elems=0)
    assert refused("lx_dpmpp2m_step_apg", n_images=65536, elems=4) and refused("lx_dpmpp2m_step_apg", elems=2 ** 62)


@both
@pytest.mark.parametrize("bad", NOT_FINITE + [0.0, -0.5])
def test_sigma(entry, bad):
    assert refused(entry, sigma=bad) and refused(entry, sigma=bad, **BLEND)


@both
@pytest.mark.parametrize("bad", NOT_FINITE)
def test_values_that_are_not_finite(entry, bad):
    for name in ("c", "scale_a", "scale_b"):
        assert refused(entry, **{name: bad}), name
    assert refused(entry, scale_a=bad, n_parts=2)
    # a scale the part count does not use is ignored: the call is then refused for what is checked after the scales, half a blend triple
    for kw in (dict(scale_b=bad, n_parts=2),) + ((dict(scale_a=bad, scale_b=bad, n_parts=1),) if entry == "lx_dpmpp2m_step" else ()):
        status, msg = ENTRIES[entry](x0=BLEND["x0"], **kw)
        assert status == -1 and b"go together" in msg, kw


@both
@pytest.mark.parametrize("given", [("x0",), ("z",), ("m",), ("x0", "z"), ("x0", "m"), ("z", "m")])
def test_a_partly_null_blend_triple(entry, given):
    assert refused(entry, **{k: BLEND[k] for k in given})


@pytest.mark.parametrize("entry,n_parts", [("lx_dpmpp2m_step", 1), ("lx_dpmpp2m_step", 2), ("lx_dpmpp2m_step", 3),
                                           ("lx_dpmpp2m_step_apg", 2), ("lx_dpmpp2m_step_apg", 3)])
def test_D_on_x(entry, n_parts):
    """[n] floats that touch x[0, n_parts n): the same address, a later part, x's last element, or ending on x's first"""
    for delta in (0, 4 * (n_parts - 1) * N, 4 * (n_parts * N - 1), -4 * (N - 1)):
        status, msg = ENTRIES[entry](n_parts=n_parts, D=A + delta)
        assert status == -1 and msg.startswith(entry.encode() + b": D may not overlap x"), (delta, msg)


@both
@pytest.mark.parametrize("bf16", [0, 1])
def test_D_on_v(entry, bf16):
    """v is read by other work items while D is written: refused in either format, over v's own extent (3n elements of 4 or 2 bytes)"""
    vbytes = 3 * N * (2 if bf16 else 4)
    for delta in (0, vbytes - 4, -4 * (N - 1)):
        status, msg = ENTRIES[entry](bf16=bf16, D=A + 0x10000 + delta)
        assert status == -1 and msg.startswith(entry.encode() + b": D may not overlap v"), (delta, msg)
    # just past a bf16 v is not v: the call passes that test (and is refused for the next thing wrong with it)
    status, msg = ENTRIES[entry](bf16=1, D=A + 0x10000 + 3 * N * 2, x0=A + 0x10000 + 3 * N * 2, z=BLEND["z"], m=BLEND["m"])
    assert status == -1 and b"D may not overlap x0, z or m" in msg


@both
@pytest.mark.parametrize("which", ["x0", "z", "m"])
def test_D_on_a_blend_operand(entry, which):
    for delta in (0, 4 * (N - 1), -4 * (N - 1)):
        assert refused(entry, **dict(BLEND, D=BLEND[which] + delta)), delta


@pytest.mark.parametrize("which,size", [("M", 4 * N), ("sums", IMAGES * 24), ("ws", 48)])
def test_D_on_the_apg_operands(which, size):
    base = {"M": A + 0x20000, "sums": A + 0x30000, "ws": A + 0x40000}[which]
    for delta in (0, size - 4, -4 * (N - 1)):
        status, msg = step_apg(D=base + delta)
        assert status == -1 and msg.startswith(b"lx_dpmpp2m_step_apg: D may not overlap M, sums or the workspace"), (delta, msg)


@both
def test_the_existing_alias_rules(entry):
    """through check_step_aliases: x0, z or m on x, and an fp32 v on x"""
    for which in ("x0", "z", "m"):
        for delta in (0, 4 * N, 4 * (3 * N - 1), -4 * (N - 1)):
            assert refused(entry, **dict(BLEND, **{which: A + delta})), (which, delta)
    for delta in (0, 4 * (3 * N - 1), -4 * (3 * N - 1)):
        assert refused(entry, v=A + delta), delta


def test_the_apg_entry_keeps_the_apg_refusals():
    for kw in (dict(eta=1.5), dict(eta=-0.1), dict(thr=-1.0), dict(momentum=1.0), dict(ws_bytes=47), dict(ws=A + 0x40004), dict(sums=A + 0x30004),
               dict(M=A), dict(M=A + 0x10000), dict(sums=A + 4 * N), dict(eta=float("nan"))):
        assert refused("lx_dpmpp2m_step_apg", **kw), kw


def test_the_euler_apg_entry_still_names_itself():
    """the two APG entries share their checks: the one that was called is the one named"""
    from loongx_amd._lib import lib
    status = lib.lx_euler_step_apg(A, A + 0x10000, 0, 3, F(2.0), F(3.0), F(0.0), F(-0.1), F(0.5), F(1.5), F(-0.5), A + 0x20000, A + 0x30000,
                                   A + 0x40000, 48, None, None, None, F(0.5), IMAGES, ELEMS, None)
    assert status == -1 and lib.lx_last_error().startswith(b"lx_euler_step_apg: sigma")
