"""CPU-only: the three pair-image entry points of the precise-mode VAE (lx_groupnorm_silu_split, lx_im2col3x3_split,
lx_softmax_rows_split) are declared and bound without moving the ABI version, reject bad arguments before they launch anything, and the
ops wrappers hand them strides and offsets as the C ABI expects (the style of tests/test_vae_anysize_cpu.py)."""
import pytest
import torch

from loongx_amd import _lib, ops
from tests.test_ops_marshal_cpu import STREAM, FakeTensor, rec  # noqa: F401  (rec: the recording stand-in for the library)

bf16, f32 = torch.bfloat16, torch.float32
X, Y, G, B_, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # fake, aligned device addresses: validation dereferences nothing


def test_entry_points_are_declared_and_bound_at_abi_404():
    for n in ("lx_groupnorm_silu_split", "lx_im2col3x3_split", "lx_softmax_rows_split"):
        assert n in _lib.EXPORTS and hasattr(_lib.lib, n)
    assert _lib.lib.lx_version() == 404


def _last(prefix):
    msg = _lib.lib.lx_last_error()
    assert msg.startswith(prefix), msg
    return msg


@pytest.mark.parametrize("over,text", [
    (dict(x=None), b"NULL operand"),
    (dict(ws=None), b"NULL operand"),
    (dict(C=96), b"C/4 a divisor of 256"),
    (dict(lo=132), b"y_lo_off % 8 == 0"),                         # not a multiple of 8
    (dict(lo=120), b"C <= y_lo_off"),                             # the halves would overlap
    (dict(ldy=255), b"y_lo_off + C <= ldy"),                      # rows too short for both halves
    (dict(x=X + 4), b"misaligned"),
    (dict(ws_bytes=8), b"workspace too small"),
])
def test_groupnorm_silu_split_rejects_bad_arguments_without_gpu(over, text):
    a = dict(x=X, B=2, P=60, C=128, G=32, lo=128, ldy=256, ws=WS, ws_bytes=1 << 20)
    a.update(over)
    rc = _lib.lib.lx_groupnorm_silu_split(a["x"], a["B"], a["P"], a["C"], a["G"], G, B_, 1e-6, 1, Y, a["ldy"], a["lo"], a["ws"], a["ws_bytes"], None)
    assert rc == -1 and text in _last(b"lx_groupnorm_silu_split: ")


@pytest.mark.parametrize("over,text", [
    (dict(x=None), b"bad arguments"),
    (dict(mode=3), b"mode 0|1|2"),
    (dict(mode=1, H=5), b"mode 1 needs even H, W"),
    (dict(Kpad=1144), b"Kpad=1144"),                              # < 9 C
    (dict(lo=132), b"x_lo_off % 8 == 0"),
    (dict(lo=64), b"C <= x_lo_off"),
    (dict(ldx=248), b"x_lo_off + C <= ldx"),
])
def test_im2col3x3_split_rejects_bad_arguments_without_gpu(over, text):
    a = dict(x=X, ldx=256, lo=128, H=6, W=10, C=128, mode=0, Kpad=1152)
    a.update(over)
    rc = _lib.lib.lx_im2col3x3_split(a["x"], a["ldx"], a["lo"], 2, a["H"], a["W"], a["C"], a["mode"], Y, a["Kpad"], None)
    assert rc == -1 and text in _last(b"lx_im2col3x3_split: ")


@pytest.mark.parametrize("over,text", [
    (dict(S=None), b"NULL operand"),
    (dict(n_valid=0), b"1 <= n_valid <= n_store"),
    (dict(n_valid=65), b"1 <= n_valid <= n_store"),
    (dict(M=0), b"M > 0"),
    (dict(lds=59), b"lds >= n_valid"),
    (dict(plo=68), b"p_lo_off % 8 == 0"),
    (dict(plo=56), b"n_store <= p_lo_off"),
    (dict(ldp=127), b"p_lo_off + n_store <= ldp"),
])
def test_softmax_rows_split_rejects_bad_arguments_without_gpu(over, text):
    a = dict(S=X, lds=64, ldp=128, plo=64, M=4, n_valid=60, n_store=64)
    a.update(over)
    rc = _lib.lib.lx_softmax_rows_split(a["S"], a["lds"], 0.5, Y, a["ldp"], a["plo"], a["M"], a["n_valid"], a["n_store"], None)
    assert rc == -1 and text in _last(b"lx_softmax_rows_split: ")


# ---- the wrappers --------------------------------------------------------------------------------------------------------------------
class _Ws:
    """What torch.empty(nbytes, dtype=uint8) gives the wrapper: only the address matters."""
    def data_ptr(self):
        return WS


def test_groupnorm_silu_split_marshals_strides_and_offsets(rec, monkeypatch):  # noqa: F811
    monkeypatch.setattr(ops.torch, "empty", lambda *a, **k: _Ws())
    rec.lx_groupnorm_workspace_bytes = lambda B, P, Gn: 4096
    x, g, b = FakeTensor(X, (2, 60, 128), f32), FakeTensor(G, (128,), f32), FakeTensor(B_, (128,), f32)
    y = FakeTensor(Y, (120, 272), bf16)
    ops.groupnorm_silu_split(x, g, b, y, 136, 32, 1e-6, False)
    assert rec.log[-1] == ("lx_groupnorm_silu_split", (X, 2, 60, 128, 32, G, B_, 1e-6, 0, Y, 272, 136, WS, 4096, STREAM))


def test_im2col3x3_split_marshals_the_pixel_stride_and_half_the_row(rec):  # noqa: F811
    x = FakeTensor(X, (2, 6, 10, 16), bf16)                      # what lx_split_bf16 leaves of an RGB image: lo_off = 8, ld = 16
    out = FakeTensor(Y, (120, 128), bf16)
    ops.im2col3x3_split(x, 3, 8, out, 2)
    assert rec.log == [("lx_im2col3x3_split", (X, 16, 8, 2, 6, 10, 3, 2, Y, 64, STREAM))]


def test_softmax_rows_split_marshals_n_valid_n_store_and_p_lo_off(rec):  # noqa: F811
    S = FakeTensor(X, (63, 64), f32, strides=(72, 1))
    P = FakeTensor(Y, (63, 136), bf16, strides=(144, 1))
    ops.softmax_rows_split(S, P, 0.125, 63, 64, 72)
    assert rec.log == [("lx_softmax_rows_split", (X, 72, 0.125, Y, 144, 72, 63, 63, 64, STREAM))]


def test_wrappers_check_dtypes_offsets_and_row_lengths_before_the_call(rec):  # noqa: F811
    x, g = FakeTensor(X, (2, 60, 128), f32), FakeTensor(G, (128,), f32)
    with pytest.raises(TypeError, match="y: expected torch.bfloat16"):
        ops.groupnorm_silu_split(x, g, g, FakeTensor(Y, (120, 256), f32), 128)
    with pytest.raises(TypeError, match="x: expected torch.float32"):
        ops.groupnorm_silu_split(FakeTensor(X, (2, 60, 128), bf16), g, g, FakeTensor(Y, (120, 256), bf16), 128)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.groupnorm_silu_split(x, g, g, FakeTensor(Y, (120, 272), bf16), 132)
    with pytest.raises(ValueError, match="cannot hold a hi and a lo half"):
        ops.groupnorm_silu_split(x, g, g, FakeTensor(Y, (120, 248), bf16), 128)
    out = FakeTensor(Y, (120, 2304), bf16)
    with pytest.raises(TypeError, match="x: expected torch.bfloat16"):
        ops.im2col3x3_split(FakeTensor(X, (2, 6, 10, 256), f32), 128, 128, out)
    with pytest.raises(TypeError, match="out: expected torch.bfloat16"):
        ops.im2col3x3_split(FakeTensor(X, (2, 6, 10, 256), bf16), 128, 128, FakeTensor(Y, (120, 2304), f32))
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.im2col3x3_split(FakeTensor(X, (2, 6, 10, 16), bf16), 3, 4, out)
    with pytest.raises(ValueError, match="cannot hold a hi and a lo half"):
        ops.im2col3x3_split(FakeTensor(X, (2, 6, 10, 248), bf16), 128, 128, out)
    S = FakeTensor(X, (8, 64), f32)
    with pytest.raises(TypeError, match="P: expected torch.bfloat16"):
        ops.softmax_rows_split(S, FakeTensor(Y, (8, 128), f32), 1.0, 60, 64, 64)
    with pytest.raises(TypeError, match="S: expected torch.float32"):
        ops.softmax_rows_split(FakeTensor(X, (8, 64), bf16), FakeTensor(Y, (8, 128), bf16), 1.0, 60, 64, 64)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.softmax_rows_split(S, FakeTensor(Y, (8, 136), bf16), 1.0, 60, 64, 68)
    with pytest.raises(ValueError, match="cannot hold a hi and a lo half"):
        ops.softmax_rows_split(S, FakeTensor(Y, (8, 120), bf16), 1.0, 60, 64, 64)
    assert rec.log == []
