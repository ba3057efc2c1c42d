"""CPU-only: the three entry points of the fp16-operand VAE (lx_groupnorm_silu_f16, lx_softmax_rows_f16, lx_convert_f16) are declared and
bound without moving the ABI version, reject bad arguments before they launch anything, the ops wrappers hand them pointers, strides,
counts and the counter pointer (or NULL) as the C ABI expects, and LxAutoencoderKL validates operands / precise / f16_overflow before it
touches a device (the style of tests/test_vae_precise_cpu.py)."""
import pytest
import torch

from loongx_amd import _lib, ops
from tests.test_ops_marshal_cpu import STREAM, FakeTensor, rec  # noqa: F401  (rec: the recording stand-in for the library)

bf16, f16, f32, i32 = torch.bfloat16, torch.float16, torch.float32, torch.int32
X, Y, G, B_, WS, OVF = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000      # fake, aligned device addresses: validation dereferences nothing


def test_entry_points_are_declared_and_bound_at_abi_404():
    for n in ("lx_groupnorm_silu_f16", "lx_softmax_rows_f16", "lx_convert_f16"):
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
    (dict(x=X + 4), b"misaligned"),
    (dict(y=Y + 2), b"misaligned"),
    (dict(ovf=OVF + 2), b"misaligned"),
    (dict(ws_bytes=8), b"workspace too small"),
])
def test_groupnorm_silu_f16_rejects_bad_arguments_without_gpu(over, text):
    a = dict(x=X, y=Y, B=2, P=60, C=128, G=32, ws=WS, ws_bytes=1 << 20, ovf=OVF)
    a.update(over)
    rc = _lib.lib.lx_groupnorm_silu_f16(a["x"], a["B"], a["P"], a["C"], a["G"], G, B_, 1e-6, 1, a["y"], a["ws"], a["ws_bytes"], a["ovf"], None)
    assert rc == -1 and text in _last(b"lx_groupnorm_silu_f16: ")


@pytest.mark.parametrize("over,text", [
    (dict(S=None), b"NULL operand"),
    (dict(n_valid=0), b"1 <= n_valid <= n_store"),
    (dict(n_valid=65), b"1 <= n_valid <= n_store"),
    (dict(M=0), b"M > 0"),
    (dict(lds=59), b"lds >= n_valid"),
    (dict(ldp=63), b"ldp >= n_store"),
    (dict(S=X + 2), b"misaligned"),
    (dict(P=Y + 1), b"misaligned"),
])
def test_softmax_rows_f16_rejects_bad_arguments_without_gpu(over, text):
    a = dict(S=X, P=Y, lds=64, ldp=64, M=4, n_valid=60, n_store=64)
    a.update(over)
    rc = _lib.lib.lx_softmax_rows_f16(a["S"], a["lds"], 0.5, a["P"], a["ldp"], a["M"], a["n_valid"], a["n_store"], None)
    assert rc == -1 and text in _last(b"lx_softmax_rows_f16: ")


@pytest.mark.parametrize("over,text", [
    (dict(dst=None), b"NULL operand"),
    (dict(src=None), b"NULL operand"),
    (dict(dst=Y + 1), b"misaligned"),
    (dict(src=X + 2), b"misaligned"),                           # an fp32 source two bytes off
    (dict(src=X + 1, src_bf16=1), b"misaligned"),
    (dict(ovf=OVF + 1), b"misaligned"),
])
def test_convert_f16_rejects_bad_arguments_without_gpu(over, text):
    a = dict(dst=Y, src=X, src_bf16=0, ovf=OVF)
    a.update(over)
    rc = _lib.lib.lx_convert_f16(a["dst"], a["src"], a["src_bf16"], 1000, a["ovf"], None)
    assert rc == -1 and text in _last(b"lx_convert_f16: ")


def test_convert_f16_of_nothing_launches_nothing():
    assert _lib.lib.lx_convert_f16(Y, X, 0, 0, None, None) == 0


# ---- the wrappers --------------------------------------------------------------------------------------------------------------------
class _Ws:
    """What torch.empty(nbytes, dtype=uint8) gives the wrapper: only the address matters."""
    def data_ptr(self):
        return WS


def test_groupnorm_silu_f16_marshals_shape_counter_and_workspace(rec, monkeypatch):  # noqa: F811
    monkeypatch.setattr(ops.torch, "empty", lambda *a, **k: _Ws())
    rec.lx_groupnorm_workspace_bytes = lambda B, P, Gn: 4096
    x, g, b = FakeTensor(X, (2, 60, 128), f32), FakeTensor(G, (128,), f32), FakeTensor(B_, (128,), f32)
    y = FakeTensor(Y, (2, 60, 128), f16)
    ops.groupnorm_silu_f16(x, g, b, y, 32, 1e-6, False, f16_ovf=FakeTensor(OVF, (1,), i32))
    assert rec.log[-1] == ("lx_groupnorm_silu_f16", (X, 2, 60, 128, 32, G, B_, 1e-6, 0, Y, WS, 4096, OVF, STREAM))
    ops.groupnorm_silu_f16(x, g, b, FakeTensor(Y, (120, 128), f16), 32, 1e-6, True)                 # one row per pixel is the same bytes
    assert rec.log[-1] == ("lx_groupnorm_silu_f16", (X, 2, 60, 128, 32, G, B_, 1e-6, 1, Y, WS, 4096, None, STREAM))


def test_softmax_rows_f16_marshals_strides_n_valid_and_n_store(rec):  # noqa: F811
    S = FakeTensor(X, (63, 64), f32, strides=(72, 1))
    P = FakeTensor(Y, (63, 64), f16, strides=(80, 1))
    ops.softmax_rows_f16(S, P, 0.125, 63)
    assert rec.log == [("lx_softmax_rows_f16", (X, 72, 0.125, Y, 80, 63, 63, 64, STREAM))]
    ops.softmax_rows_f16(FakeTensor(X, (64, 64), f32), FakeTensor(Y, (64, 64), f16), 0.5)           # no padding: n_valid == n_store
    assert rec.log[-1] == ("lx_softmax_rows_f16", (X, 64, 0.5, Y, 64, 64, 64, 64, STREAM))


def test_convert_f16_marshals_source_format_count_and_counter(rec):  # noqa: F811
    ops.convert_f16(FakeTensor(Y, (10, 100), f16), FakeTensor(X, (10, 100), f32), f16_ovf=FakeTensor(OVF, (1,), i32))
    ops.convert_f16(FakeTensor(Y, (1000,), f16), FakeTensor(X, (1000,), bf16))
    assert rec.log == [("lx_convert_f16", (Y, X, 0, 1000, OVF, STREAM)), ("lx_convert_f16", (Y, X, 1, 1000, None, STREAM))]


def test_wrappers_check_dtypes_and_shapes_before_the_call(rec):  # noqa: F811
    x, g = FakeTensor(X, (2, 60, 128), f32), FakeTensor(G, (128,), f32)
    y = FakeTensor(Y, (2, 60, 128), f16)
    with pytest.raises(TypeError, match="y: expected torch.float16"):
        ops.groupnorm_silu_f16(x, g, g, FakeTensor(Y, (2, 60, 128), bf16))
    with pytest.raises(TypeError, match="x: expected torch.float32"):
        ops.groupnorm_silu_f16(FakeTensor(X, (2, 60, 128), bf16), g, g, y)
    with pytest.raises(TypeError, match="gamma: expected torch.float32"):
        ops.groupnorm_silu_f16(x, FakeTensor(G, (128,), bf16), g, y)
    with pytest.raises(TypeError, match="f16_ovf: expected torch.int32"):
        ops.groupnorm_silu_f16(x, g, g, y, f16_ovf=FakeTensor(OVF, (1,), f32))
    with pytest.raises(ValueError, match="as many elements as x"):
        ops.groupnorm_silu_f16(x, g, g, FakeTensor(Y, (2, 60, 64), f16))
    with pytest.raises(ValueError, match="contiguous"):
        ops.groupnorm_silu_f16(x, g, g, FakeTensor(Y, (120, 128), f16, strides=(256, 1)))
    S = FakeTensor(X, (8, 64), f32)
    with pytest.raises(TypeError, match="P: expected torch.float16"):
        ops.softmax_rows_f16(S, FakeTensor(Y, (8, 64), bf16), 1.0, 60)
    with pytest.raises(TypeError, match="S: expected torch.float32"):
        ops.softmax_rows_f16(FakeTensor(X, (8, 64), f16), FakeTensor(Y, (8, 64), f16), 1.0, 60)
    with pytest.raises(ValueError, match="same rows"):
        ops.softmax_rows_f16(S, FakeTensor(Y, (7, 64), f16), 1.0, 60)
    with pytest.raises(ValueError, match="at least n_valid columns"):
        ops.softmax_rows_f16(S, FakeTensor(Y, (8, 56), f16), 1.0, 60)
    with pytest.raises(ValueError, match="at least n_valid columns"):
        ops.softmax_rows_f16(S, FakeTensor(Y, (8, 128), f16), 1.0, 65)
    with pytest.raises(TypeError, match="dst: expected torch.float16"):
        ops.convert_f16(FakeTensor(Y, (1000,), bf16), FakeTensor(X, (1000,), f32))
    with pytest.raises(TypeError, match="src: expected torch.float32 or torch.bfloat16"):
        ops.convert_f16(FakeTensor(Y, (1000,), f16), FakeTensor(X, (1000,), f16))
    with pytest.raises(TypeError, match="f16_ovf: expected torch.int32"):
        ops.convert_f16(FakeTensor(Y, (1000,), f16), FakeTensor(X, (1000,), f32), f16_ovf=FakeTensor(OVF, (1,), f32))
    with pytest.raises(ValueError, match="same number of elements"):
        ops.convert_f16(FakeTensor(Y, (1000,), f16), FakeTensor(X, (999,), f32))
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.convert_f16(FakeTensor(Y, (1000,), f16, cuda=False), FakeTensor(X, (1000,), f32))
    assert rec.log == []


# ---- the constructor -------------------------------------------------------------------------------------------------------------------
def test_constructor_validates_operands_precise_and_policy_before_any_device_work():
    """The three checks come first: a device that does not exist is never reached."""
    from loongx_amd.vae import LxAutoencoderKL
    nowhere = "cuda:99"
    with pytest.raises(ValueError, match='operands = \'fp8\''):
        LxAutoencoderKL({}, None, nowhere, operands="fp8")
    with pytest.raises(ValueError, match='f16_overflow = \'ignore\''):
        LxAutoencoderKL({}, None, nowhere, operands="fp16", f16_overflow="ignore")
    with pytest.raises(ValueError, match='operands="fp16" with precise=True'):
        LxAutoencoderKL({}, None, nowhere, precise=True, operands="fp16")
    with pytest.raises(ValueError, match='operands="fp16" with precise=True'):
        LxAutoencoderKL({}, None, "cpu", precise=True).set_operands("fp16")
    lx = LxAutoencoderKL({}, None, "cpu")
    assert lx.operands == "bf16" and lx.precise is False and lx.f16_overflow == "raise" and not lx.w16 and lx.f16_ovf is None


def test_generate_hands_its_policy_to_a_vae_that_has_the_attribute_for_the_call_only():
    from types import SimpleNamespace
    from loongx_amd.flux.generate import vae_f16_overflow
    vae = SimpleNamespace(f16_overflow="raise")
    with vae_f16_overflow(vae, "fallback"):
        assert vae.f16_overflow == "fallback"
    assert vae.f16_overflow == "raise"
    with vae_f16_overflow(vae, None):
        assert vae.f16_overflow == "raise"
    with pytest.raises(ValueError, match="f16_overflow"):
        with vae_f16_overflow(vae, "ignore"):
            pass
    other = SimpleNamespace()
    with vae_f16_overflow(other, "warn"), vae_f16_overflow(None, "warn"):
        assert not hasattr(other, "f16_overflow")
