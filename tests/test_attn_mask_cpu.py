"""CPU-only: the masked-attention ABI (include/lx.h lx_attn_mask_desc, lx_attn_mask_workspace / lx_attn_mask_prep / lx_attn_fwd_masked) --
the ctypes mirror has the C size, and every entry point validates its arguments on the host (status -1 and a message, nothing launched)."""
import ctypes
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from loongx_amd import _lib
    return _lib


def test_mask_desc_layout_matches_header(L):
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "sz.c")
        open(src, "w").write('#include "lx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu\\n", sizeof(lx_attn_mask_desc), '
                             'offsetof(lx_attn_mask_desc, strides), offsetof(lx_attn_mask_desc, workspace_bytes));return 0;}\n')
        exe = os.path.join(d, "sz")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        size, st, wb = map(int, subprocess.check_output([exe]).split())
    assert ctypes.sizeof(L.AttnMaskDesc) == size
    assert L.AttnMaskDesc.strides.offset == st and L.AttnMaskDesc.workspace_bytes.offset == wb


def _descs(L, lens=(40, 300, 90), B=2, H=3):
    """an attention descriptor with fake, aligned addresses (nothing dereferences them) and a matching [B, H, S, S] bool mask"""
    S = sum(lens)
    a = L.AttnDesc()
    a.Q = a.K = a.VT = a.O = 0x10000
    a.ldq = a.ldk = a.ldo = 3 * H * 128
    a.vt_ld = sum((x + 63) // 64 * 64 for x in lens)
    a.B, a.H, a.n_seg = B, H, len(lens)
    p = 0
    for i, x in enumerate(lens):
        a.seg_row0[i], a.seg_len[i], a.seg_vt0[i] = 0, x, p
        p += (x + 63) // 64 * 64
    a.scale = 128 ** -0.5
    m = L.AttnMaskDesc()
    m.mask, m.dtype = 0x20000, L.LX_ATTN_MASK_BOOL
    for i, (n, st) in enumerate(zip((B, H, S, S), (H * S * S, S * S, S, 1))):
        m.dims[i], m.strides[i] = n, st
    return a, m


def _need(L, a, m):
    n = ctypes.c_size_t(0)
    assert L.lib.lx_attn_mask_workspace(ctypes.byref(a), ctypes.byref(m), ctypes.byref(n)) == 0, L.lib.lx_last_error()
    return n.value


def test_workspace_size_and_broadcast(L):
    a, m = _descs(L)
    n_qt, n_kt = 1 + 2 + 1, 1 + 5 + 2
    full = _need(L, a, m)
    assert full >= 2 * 3 * n_qt * n_kt * 256 * 8                      # one bit per (row, padded key) of every tile
    m.dims[0] = m.dims[1] = 1                                          # [1, 1, S, S]: one plane
    one = _need(L, a, m)
    assert one < full and one >= n_qt * n_kt * 256 * 8
    m.dtype = L.LX_ATTN_MASK_F32                                       # fp32 bias image: 32x the bits
    assert _need(L, a, m) >= n_qt * n_kt * 256 * 64 * 4
    m.dims[2] = 1                                                      # key padding [1, 1, 1, S]
    assert _need(L, a, m) > 0


@pytest.mark.parametrize("case", ["dims_sk", "dims_b", "dims_h", "dims_sq", "stride", "dtype", "nseg", "empty_seg", "vt0"])
def test_workspace_validates(L, case):
    a, m = _descs(L)
    want = {"dims_sk": b"mask dims", "dims_b": b"mask dims", "dims_h": b"mask dims", "dims_sq": b"mask dims", "stride": b"stride",
            "dtype": b"dtype", "nseg": b"n_seg", "empty_seg": b"empty segment", "vt0": b"seg_vt0"}[case]
    if case == "dims_sk":
        m.dims[3] += 1
    elif case == "dims_b":
        m.dims[0] = 3
    elif case == "dims_h":
        m.dims[1] = 2
    elif case == "dims_sq":
        m.dims[2] = 7
    elif case == "stride":
        m.strides[3] = -1
    elif case == "dtype":
        m.dtype = 4
    elif case == "nseg":
        a.n_seg = 4
    elif case == "empty_seg":
        a.seg_len[1] = 0
    else:
        a.seg_vt0[2] = 32
    n = ctypes.c_size_t(0)
    assert L.lib.lx_attn_mask_workspace(ctypes.byref(a), ctypes.byref(m), ctypes.byref(n)) == -1
    assert want in L.lib.lx_last_error()
    # the other two entry points run the same checks first
    assert L.lib.lx_attn_mask_prep(ctypes.byref(a), ctypes.byref(m), None) == -1 and want in L.lib.lx_last_error()
    assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and want in L.lib.lx_last_error()


def test_prep_and_forward_validate_workspace(L):
    a, m = _descs(L)
    need = _need(L, a, m)
    m.workspace, m.workspace_bytes = 0x100000, need - 1                # too small
    for fn in (L.lib.lx_attn_mask_prep, L.lib.lx_attn_fwd_masked):
        assert fn(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"workspace" in L.lib.lx_last_error()
    m.workspace, m.workspace_bytes = 0x100010, need                    # misaligned
    assert L.lib.lx_attn_mask_prep(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"aligned" in L.lib.lx_last_error()
    m.workspace = None                                                 # missing
    assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"workspace" in L.lib.lx_last_error()
    m.workspace, m.mask = 0x100000, None                               # no mask to read
    assert L.lib.lx_attn_mask_prep(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"NULL mask" in L.lib.lx_last_error()
    n = ctypes.c_size_t(0)
    assert L.lib.lx_attn_mask_workspace(None, ctypes.byref(m), ctypes.byref(n)) == -1 and b"NULL" in L.lib.lx_last_error()


@pytest.mark.parametrize("flag", ["ATTN_BOUNDED", "ATTN_INVARIANT", "ATTN_PREFER_4WAVE", "ATTN_P_EXP2", "unknown"])
def test_forward_rejects_flags(L, flag):
    a, m = _descs(L)
    m.workspace, m.workspace_bytes = 0x100000, _need(L, a, m)
    a.flags = (getattr(L, "LX_" + flag) if flag != "unknown" else 1 << 12) | L.LX_ATTN_Q_LOG2
    assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"flags" in L.lib.lx_last_error()


def test_forward_validates_operands(L):
    a, m = _descs(L)
    m.workspace, m.workspace_bytes = 0x100000, _need(L, a, m)
    a.n_qseg = 2
    assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"n_qseg" in L.lib.lx_last_error()
    a.n_qseg, a.qseg_mask = 0, 0b010
    assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"qseg_mask" in L.lib.lx_last_error()
    a.qseg_mask, a.ldq = 0, 100
    assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"ldq" in L.lib.lx_last_error()
    a.ldq, a.vt_ld = a.ldk, a.vt_ld - 64                              # the last segment's V^T tiles would run past vt_ld
    assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"vt_ld" in L.lib.lx_last_error()
    a.vt_ld += 64
    a.K = None
    assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"NULL operand" in L.lib.lx_last_error()
