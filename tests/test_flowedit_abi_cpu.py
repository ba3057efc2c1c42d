"""lx_flowedit_inputs and lx_flowedit_step through the C ABI, without a GPU: both symbols are exported under the same ABI version, and every
refusal of include/lx.h returns LX_ERR_INVALID (-1) before any launch and names the entry point in lx_last_error(). The addresses are fake
and aligned, and every call made here is one that must be refused, so none is dereferenced. The pattern of tests/test_solver_abi_cpu.py."""
import ctypes

import pytest

A, N = 0x100000, 1024                                # out / v at A: 2 parts of 1024 floats = 0x2000 bytes; the other operands 0x10000 apart
F = ctypes.c_float
NOT_FINITE = [float("nan"), float("inf"), float("-inf")]
INPUTS = dict(x_src=A + 0x10000, z_fe=A + 0x20000, noise=A + 0x30000)


def inputs(out=A, x_src=INPUTS["x_src"], z_fe=INPUTS["z_fe"], noise=INPUTS["noise"], sigma=0.5, n=N):
    from loongx_amd._lib import lib
    status = lib.lx_flowedit_inputs(out, x_src, z_fe, noise, F(sigma), n, None)
    return status, lib.lx_last_error()


def step(z_fe=A + 0x20000, v=A, bf16=0, coef=-0.05, m=None, n=N):
    from loongx_amd._lib import lib
    status = lib.lx_flowedit_step(z_fe, v, bf16, F(coef), m, n, None)
    return status, lib.lx_last_error()


ENTRIES = {"lx_flowedit_inputs": inputs, "lx_flowedit_step": step}


def refused(entry, **kw):
    status, msg = ENTRIES[entry](**kw)
    return status == -1 and msg.startswith(entry.encode() + b":")


def test_the_symbols_are_exported_under_the_same_abi_version():
    from loongx_amd import _lib
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.lib.lx_version() == 404


@pytest.mark.parametrize("which", ["out", "x_src", "z_fe", "noise"])
def test_null_operands_of_the_inputs(which):
    assert refused("lx_flowedit_inputs", **{which: None})


@pytest.mark.parametrize("which", ["z_fe", "v"])
def test_null_operands_of_the_step(which):
    assert refused("lx_flowedit_step", **{which: None}) and refused("lx_flowedit_step", **{which: None}, m=A + 0x40000)


def test_sizes():
    assert refused("lx_flowedit_inputs", n=0) and refused("lx_flowedit_step", n=0) and refused("lx_flowedit_step", n=0, m=A + 0x40000)
    assert refused("lx_flowedit_inputs", n=2 ** 62) and refused("lx_flowedit_step", n=2 ** 62)          # (2n floats past an address)


@pytest.mark.parametrize("bad", NOT_FINITE + [-0.001, 1.001, -1.0, 2.0])
def test_sigma(bad):
    status, msg = inputs(sigma=bad)
    assert status == -1 and msg.startswith(b"lx_flowedit_inputs: sigma"), msg


@pytest.mark.parametrize("bad", NOT_FINITE)
def test_coef(bad):
    for kw in ({}, dict(m=A + 0x40000), dict(bf16=1)):
        status, msg = step(coef=bad, **kw)
        assert status == -1 and msg.startswith(b"lx_flowedit_step: coef"), msg


@pytest.mark.parametrize("which", ["x_src", "z_fe", "noise"])
def test_an_input_on_out(which):
    """[n] floats that touch out[0, 2n): the same address, the second part, out's last element, or ending on out's first"""
    for delta in (0, 4 * N, 4 * (2 * N - 1), -4 * (N - 1)):
        status, msg = inputs(**{which: A + delta})
        assert status == -1 and msg.startswith(b"lx_flowedit_inputs: x_src, z_fe and noise may not overlap out"), (delta, msg)


@pytest.mark.parametrize("bf16", [0, 1])
def test_v_on_z_fe(bf16):
    """v is read by other work items while z_fe is written: refused in either format, over v's own extent (2n elements of 4 or 2 bytes)"""
    vbytes = 2 * N * (2 if bf16 else 4)
    for delta in (0, vbytes - 4, -4 * (N - 1)):
        status, msg = step(bf16=bf16, z_fe=A + delta)
        assert status == -1 and msg.startswith(b"lx_flowedit_step: v may not overlap z_fe"), (delta, msg)
    # just past a bf16 v is not v: the call passes that test (and is refused for the next thing wrong with it)
    status, msg = step(bf16=1, z_fe=A + 2 * N * 2, m=A + 2 * N * 2)
    assert status == -1 and msg.startswith(b"lx_flowedit_step: m may not overlap z_fe"), msg


def test_m_on_z_fe():
    for delta in (0, 4 * (N - 1), -4 * (N - 1)):
        status, msg = step(m=A + 0x20000 + delta)
        assert status == -1 and msg.startswith(b"lx_flowedit_step: m may not overlap z_fe"), (delta, msg)
