"""CPU-only: lx_softmax_rows_valid (the VAE's row softmax over a padded key axis) rejects bad arguments before it launches anything, and
ops.softmax_rows hands it n_valid / n_store as the C ABI expects (the style of tests/test_abi.py and tests/test_ops_marshal_cpu.py)."""
import pytest
import torch

from loongx_amd import _lib, ops
from tests.test_ops_marshal_cpu import STREAM, FakeTensor, rec  # noqa: F401  (rec: the recording stand-in for the library)

bf16, f32 = torch.bfloat16, torch.float32
S_PTR, P_PTR = 0x10000, 0x20000                 # fake, aligned device addresses: validation dereferences nothing


def _call(S=S_PTR, lds=64, P=P_PTR, ldp=64, M=4, n_valid=60, n_store=64):
    return _lib.lib.lx_softmax_rows_valid(S, lds, 0.5, P, ldp, M, n_valid, n_store, None)


@pytest.mark.parametrize("over,text", [
    (dict(S=None), b"NULL operand"),
    (dict(P=None), b"NULL operand"),
    (dict(n_valid=0), b"1 <= n_valid <= n_store"),
    (dict(n_valid=-3), b"1 <= n_valid <= n_store"),
    (dict(n_valid=65), b"1 <= n_valid <= n_store"),              # n_store < n_valid
    (dict(n_valid=1, n_store=0), b"1 <= n_valid <= n_store"),
    (dict(M=0), b"M > 0"),
    (dict(lds=59), b"lds >= n_valid"),
    (dict(ldp=63), b"ldp >= n_store"),
])
def test_softmax_rows_valid_rejects_bad_arguments_without_gpu(over, text):
    assert _call(**over) == -1                                   # LX_ERR_INVALID
    msg = _lib.lib.lx_last_error()
    assert msg.startswith(b"lx_softmax_rows_valid: ") and text in msg, msg


def test_softmax_rows_valid_is_declared_and_bound():
    assert "lx_softmax_rows_valid" in _lib.EXPORTS and _lib.lib.lx_version() == 404


def test_softmax_rows_marshals_n_valid_and_n_store(rec):  # noqa: F811
    S = FakeTensor(S_PTR, (63, 128), f32, strides=(136, 1))
    P = FakeTensor(P_PTR, (63, 64), bf16, strides=(72, 1))
    ops.softmax_rows(S, P, 0.125, n_valid=63)
    ops.softmax_rows(S, P, 0.125, n_valid=1)
    assert rec.log == [("lx_softmax_rows_valid", (S_PTR, 136, 0.125, P_PTR, 72, 63, 63, 64, STREAM)),
                       ("lx_softmax_rows_valid", (S_PTR, 136, 0.125, P_PTR, 72, 63, 1, 64, STREAM))]


def test_softmax_rows_without_n_valid_is_the_unpadded_call(rec):  # noqa: F811
    S = FakeTensor(S_PTR, (64, 128), f32, strides=(136, 1))
    P = FakeTensor(P_PTR, (64, 128), bf16, strides=(128, 1))
    ops.softmax_rows(S, P, 0.25)
    ops.softmax_rows(S, P, 0.25, n_valid=None)
    assert rec.log == [("lx_softmax_rows", (S_PTR, 136, 0.25, P_PTR, 128, 64, 128, STREAM))] * 2


def test_softmax_rows_checks_dtypes_and_shapes_before_the_call(rec):  # noqa: F811
    S = FakeTensor(S_PTR, (8, 64), f32)
    with pytest.raises(TypeError, match="P: expected torch.bfloat16"):
        ops.softmax_rows(S, FakeTensor(P_PTR, (8, 64), f32), 1.0, n_valid=60)
    with pytest.raises(TypeError, match="S: expected torch.float32"):
        ops.softmax_rows(FakeTensor(S_PTR, (8, 64), bf16), FakeTensor(P_PTR, (8, 64), bf16), 1.0, n_valid=60)
    with pytest.raises(AssertionError):                           # S holds fewer columns than there are keys
        ops.softmax_rows(S, FakeTensor(P_PTR, (8, 128), bf16), 1.0, n_valid=65)
    with pytest.raises(AssertionError):                           # one row of P per row of S
        ops.softmax_rows(S, FakeTensor(P_PTR, (7, 64), bf16), 1.0, n_valid=60)
    assert rec.log == []
