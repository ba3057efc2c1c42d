"""CPU-only: what loongx_amd.ops hands to the C ABI. ops.lib is replaced by a recorder and the tensors by stand-ins that expose only
what ops reads, so every test states the entry point called, each scalar argument and the bytes of the segment arrays / descriptors
with explicit expected values; the launch timer is a stub in its three states (not installed, installed and active, installed and
inactive)."""
import ctypes as C
import math
import struct

import pytest
import torch

from loongx_amd import _lib, ops

STREAM = 0x5EA0
bf16, f16, f32, u8, i32 = torch.bfloat16, torch.float16, torch.float32, torch.uint8, torch.int32


class FakeTensor:
    def __init__(self, ptr, shape, dtype, strides=None, cuda=True):
        self._ptr, self.shape, self.dtype, self.is_cuda, self.device = ptr, tuple(shape), dtype, cuda, "fake"
        if strides is None:
            strides, acc = [], 1
            for n in reversed(self.shape):
                strides.insert(0, acc)
                acc *= n
        self._strides = tuple(strides)

    def data_ptr(self):
        return self._ptr

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def element_size(self):
        return torch.empty(0, dtype=self.dtype).element_size()

    def numel(self):
        return math.prod(self.shape)

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._strides == FakeTensor(0, self.shape, self.dtype)._strides


class Recorder:
    """Stands in for the loaded library: every call is logged as (name, arguments) with ctypes arrays / structures (also behind
    byref) replaced by their bytes, and succeeds."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def call(*args):
            self.log.append((name, tuple(self._plain(a) for a in args)))
            return 0
        return call

    @staticmethod
    def _plain(a):
        if hasattr(a, "_obj"):
            a = a._obj
        return bytes(a) if isinstance(a, (C.Array, C.Structure)) else a


class StubTimer:
    def __init__(self, log, active):
        self.log, self.active = log, active

    def bracket(self, kind, flops, nbytes=0.0):
        self.log.append(("bracket", kind, flops, nbytes))
        outer = self

        class Event:
            def __init__(self, which):
                self.which = which

            def record(self):
                outer.log.append(("record", self.which))
        return Event("start"), Event("end")


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops, "lib", r)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    monkeypatch.setattr(ops, "TIMER", None)
    return r


def ln_seg_bytes(*rows):
    return b"".join(struct.pack("<4i2Q", row0, n_rows, rpb, 0, sh, sc) for row0, n_rows, rpb, sh, sc in rows)


def qkv_seg_bytes(*rows):
    return b"".join(struct.pack("<4i4Q", row0, rpb, vt0, 0, wq, wk, cos, sin) for row0, rpb, vt0, wq, wk, cos, sin in rows)


def attn_desc_bytes(Q, K, VT, O, ldq, ldk, ldo, vt_ld, q_col, k_col, o_col, B, H, n_seg, row0, length, vt0, bias, scale, n_qseg=0, flags=0,
                    qseg_mask=0, f16_ovf=0):
    b = struct.pack("<4Q19i10f3iQ", Q, K, VT, O, ldq, ldk, ldo, vt_ld, q_col, k_col, o_col, B, H, n_seg, *row0, *length, *vt0,
                    *[x for r in bias for x in r], scale, n_qseg, flags, qseg_mask, f16_ovf)
    assert len(b) == C.sizeof(_lib.AttnDesc)
    return b


def attn_f32_desc_bytes(QKV, ld, q_col, k_col, v_col, O, ldo, o_col, o_lo_off, B, H, n_seg, row0, length, bias, scale):
    b = struct.pack("<Q4iQ12i10f", QKV, ld, q_col, k_col, v_col, O, ldo, o_col, o_lo_off, B, H, n_seg, *row0, *length, *[x for r in bias for x in r], scale)
    assert len(b) == C.sizeof(_lib.AttnF32Desc)
    return b


ZERO3 = [[0.0] * 3] * 3
BIAS = [[0.0, 0.5, float("-inf")], [1.0, 0.0, -2.0], [0.25, 0.0, 0.0]]
SCALE = struct.unpack("<f", struct.pack("<f", 1.0 / math.sqrt(128.0)))[0]       # the default, as the float field holds it

# ---- ln-modulate -------------------------------------------------------------------------------------------------------------
X = FakeTensor(0x1000, (24, 256), f32, strides=(320, 1))
SH0, SC0, SH1, SC1 = (FakeTensor(p, (2, 256), f32, strides=(1536, 1)) for p in (0x2000, 0x2100, 0x2200, 0x2300))
LN_SEGS = [(0, 16, 8, SH0, SC0), (16, 8, 4, SH1, SC1)]
LN_BYTES = ln_seg_bytes((0, 16, 8, 0x2000, 0x2100), (16, 8, 4, 0x2200, 0x2300))
OVF = FakeTensor(0x7000, (1,), i32)
T_ = FakeTensor(0x6000, (8, 16), f32, strides=(24, 1))


def test_ln_modulate_segs_bf16(rec):
    Y = FakeTensor(0x3000, (24, 256), bf16, strides=(512, 1))
    ops.ln_modulate_segs(X, LN_SEGS, Y, 1536)
    assert rec.log == [("lx_ln_modulate_segs", (0x1000, 320, LN_BYTES, 2, 1536, 0x3000, 512, 256, 1e-6, STREAM))]


def test_ln_modulate_segs_f16(rec):
    Y = FakeTensor(0x3000, (24, 256), f16, strides=(512, 1))
    ops.ln_modulate_segs(X, LN_SEGS, Y, 1536, eps=1e-5, f16_ovf=OVF)
    ops.ln_modulate_segs(X, LN_SEGS[:1], Y, 1536)
    assert rec.log == [("lx_ln_modulate_f16_segs", (0x1000, 320, LN_BYTES, 2, 1536, 0x3000, 512, 256, 1e-5, 0x7000, STREAM)),
                       ("lx_ln_modulate_f16_segs", (0x1000, 320, LN_BYTES[:32], 1, 1536, 0x3000, 512, 256, 1e-6, None, STREAM))]


def test_ln_modulate_segs_lora_bf16(rec):
    Y = FakeTensor(0x3000, (24, 256), bf16, strides=(512, 1))
    Ad = FakeTensor(0x5000, (16, 256), bf16)
    ops.ln_modulate_segs(X, LN_SEGS, Y, 1536, lora=(Ad, T_, 16, 8))
    assert rec.log == [("lx_ln_modulate_lora_segs", (0x1000, 320, LN_BYTES, 2, 1536, 0x3000, 512, 256, 1e-6, 0x5000, 16, 0x6000, 24, 16, 8, STREAM))]
    with pytest.raises(TypeError, match="Adown: expected torch.bfloat16"):
        ops.ln_modulate_segs(X, LN_SEGS, Y, 1536, lora=(FakeTensor(0x5000, (16, 256), f16), T_, 16, 8))
    with pytest.raises(TypeError, match="T: expected torch.float32"):
        ops.ln_modulate_segs(X, LN_SEGS, Y, 1536, lora=(Ad, FakeTensor(0x6000, (8, 16), bf16), 16, 8))
    with pytest.raises(AssertionError):
        ops.ln_modulate_segs(X, LN_SEGS, Y, 1536, lora=(FakeTensor(0x5000, (16, 128), bf16), T_, 16, 8))
    assert len(rec.log) == 1


def test_ln_modulate_segs_lora_f16(rec):
    Y = FakeTensor(0x3000, (24, 256), f16, strides=(512, 1))
    Ad = FakeTensor(0x5000, (12, 256), f16)
    ops.ln_modulate_segs(X, LN_SEGS, Y, 1536, lora=(Ad, T_, 16, 8), f16_ovf=OVF)
    assert rec.log == [("lx_ln_modulate_lora_f16_segs",
                        (0x1000, 320, LN_BYTES, 2, 1536, 0x3000, 512, 256, 1e-6, 0x5000, 12, 0x6000, 24, 16, 8, 0x7000, STREAM))]
    with pytest.raises(TypeError, match="Adown: expected torch.float16"):
        ops.ln_modulate_segs(X, LN_SEGS, Y, 1536, lora=(FakeTensor(0x5000, (16, 256), bf16), T_, 16, 8))
    assert len(rec.log) == 1


def test_ln_modulate_one_segment_forms(rec):
    shift, scale = FakeTensor(0x2000, (3, 256), f32, strides=(1536, 1)), FakeTensor(0x2100, (3, 256), f32, strides=(1536, 1))
    ops.ln_modulate(X, shift, scale, FakeTensor(0x3000, (24, 256), bf16, strides=(512, 1)), 8)
    ops.ln_modulate(X, shift, scale, FakeTensor(0x3000, (24, 256), bf16, strides=(512, 1)), 8, eps=1e-5, mod_ld=768)
    ops.ln_modulate(X, shift, scale, FakeTensor(0x3800, (24, 256), f16, strides=(264, 1)), 8, f16_ovf=OVF)
    assert rec.log == [("lx_ln_modulate", (0x1000, 320, 0x2000, 0x2100, 1536, 0x3000, 512, 24, 256, 8, 1e-6, STREAM)),
                       ("lx_ln_modulate", (0x1000, 320, 0x2000, 0x2100, 768, 0x3000, 512, 24, 256, 8, 1e-5, STREAM)),
                       ("lx_ln_modulate_f16_segs", (0x1000, 320, ln_seg_bytes((0, 24, 8, 0x2000, 0x2100)), 1, 1536, 0x3800, 264, 256, 1e-6, 0x7000, STREAM))]
    with pytest.raises(TypeError, match="Y: expected torch.bfloat16"):
        ops.ln_modulate(X, shift, scale, FakeTensor(0x3000, (24, 256), f32), 8)


def test_ln_modulate_fp8_and_split_segs(rec):
    Y = FakeTensor(0x3000, (24, 512), bf16, strides=(520, 1))
    Y8 = FakeTensor(0x4000, (24, 256), u8, strides=(272, 1))
    ops.ln_modulate_fp8_segs(X, LN_SEGS, Y, Y8, 1536, 2)
    ops.ln_modulate_fp8_segs(X, LN_SEGS[1:], None, Y8, 1536, 0.5, eps=1e-5)
    ops.ln_modulate_split_segs(X, LN_SEGS, Y, 1536, 256)
    assert rec.log == [("lx_ln_modulate_fp8_segs", (0x1000, 320, LN_BYTES, 2, 1536, 0x3000, 520, 0x4000, 272, 2.0, 256, 1e-6, STREAM)),
                       ("lx_ln_modulate_fp8_segs", (0x1000, 320, LN_BYTES[32:], 1, 1536, None, 0, 0x4000, 272, 0.5, 256, 1e-5, STREAM)),
                       ("lx_ln_modulate_split_segs", (0x1000, 320, LN_BYTES, 2, 1536, 0x3000, 520, 256, 256, 1e-6, STREAM))]
    assert isinstance(rec.log[0][1][9], float)


# ---- qkv-prep ----------------------------------------------------------------------------------------------------------------
WQ, WK, COS, SIN = (FakeTensor(p, (128,), f32) for p in (0x8000, 0x8200, 0x8400, 0x8600))
QKV_SEGS = [(0, 64, 0, WQ, WK, COS, SIN), (128, 40, 64, None, None, None, None), (208, 8, 128, WQ, None, COS, SIN)]
QKV_BYTES = qkv_seg_bytes((0, 64, 0, 0x8000, 0x8200, 0x8400, 0x8600), (128, 40, 64, 0, 0, 0, 0), (208, 8, 128, 0x8000, 0, 0x8400, 0x8600))
QKV_BYTES_NO_VT = qkv_seg_bytes((0, 64, 0, 0x8000, 0x8200, 0x8400, 0x8600), (128, 40, 0, 0, 0, 0, 0), (208, 8, 0, 0x8000, 0, 0x8400, 0x8600))


@pytest.mark.parametrize("in_f16", (False, True))
def test_qkv_prep_segs(rec, in_f16):
    QKV = FakeTensor(0x9000, (224, 768), f16 if in_f16 else bf16, strides=(776, 1))
    VT = FakeTensor(0xA000, (2, 2, 128, 192), bf16)
    ops.qkv_prep_segs(QKV, 0, 256, 512, QKV_SEGS, 2, 2, VT, in_f16=in_f16)
    ops.qkv_prep_segs(QKV, 8, 264, 520, QKV_SEGS[:1], 2, 2, None, eps=1e-5, in_f16=in_f16)
    name = "lx_qkv_prep_f16in_segs" if in_f16 else "lx_qkv_prep_segs"
    assert rec.log == [(name, (0x9000, 776, 0, 256, 512, QKV_BYTES, 3, 2, 2, 1e-6, 0xA000, 192, STREAM)),
                       (name, (0x9000, 776, 8, 264, 520, QKV_BYTES[:48], 1, 2, 2, 1e-5, None, 0, STREAM))]


@pytest.mark.parametrize("in_f16", (False, True))
def test_qkv_prep_fp8_segs(rec, in_f16):
    QKV = FakeTensor(0x9000, (224, 768), f16 if in_f16 else bf16, strides=(776, 1))
    Q8, K8 = FakeTensor(0xB000, (224, 256), u8, strides=(288, 1)), FakeTensor(0xC000, (224, 256), u8, strides=(288, 1))
    VT8 = FakeTensor(0xD000, (2, 2, 128, 256), u8)
    ops.qkv_prep_fp8_segs(QKV, 0, 256, 512, QKV_SEGS, 2, 2, Q8, K8, VT8, in_f16=in_f16)
    name = "lx_qkv_prep_fp8_f16in_segs" if in_f16 else "lx_qkv_prep_fp8_segs"
    q_scale = 2048.0 * (1.0 / math.sqrt(128.0)) * 1.4426950408889634 / 16.0
    assert rec.log == [(name, (0x9000, 776, 0, 256, 512, QKV_BYTES, 3, 2, 2, 1e-6, 0xB000, 0xC000, 288, 0xD000, 256, q_scale, 16.0, 1.0, STREAM))]


def test_qkv_prep_f32_segs_zeroes_vt_pos0(rec):
    QKV = FakeTensor(0x9000, (224, 768), f32, strides=(776, 1))
    ops.qkv_prep_f32_segs(QKV, 0, 256, QKV_SEGS, 2, 2)
    assert rec.log == [("lx_qkv_prep_f32_segs", (0x9000, 776, 0, 256, QKV_BYTES_NO_VT, 3, 2, 2, 1e-6, STREAM))]
    with pytest.raises(TypeError, match="QKV: expected torch.float32"):
        ops.qkv_prep_f32_segs(FakeTensor(0x9000, (224, 768), bf16), 0, 256, QKV_SEGS, 2, 2)


def test_qkv_prep_split_segs(rec):
    QKV = FakeTensor(0x9000, (224, 768), f32, strides=(776, 1))
    QK2 = FakeTensor(0xB000, (224, 1024), bf16, strides=(1040, 1))
    VT2 = FakeTensor(0xD000, (2, 2, 2, 128, 192), bf16)
    ops.qkv_prep_split_segs(QKV, 0, 256, 512, QKV_SEGS, 2, 2, QK2, 0, 256, 512, VT2, eps=1e-5)
    assert rec.log == [("lx_qkv_prep_split_segs", (0x9000, 776, 0, 256, 512, QKV_BYTES, 3, 2, 2, 1e-5, 0xB000, 1040, 0, 256, 512, 0xD000, 192,
                                                   2 * 2 * 128 * 192, STREAM))]


# ---- LoRA down-projection ----------------------------------------------------------------------------------------------------
def test_lora_down_bf16_and_f16(rec):
    for dt, name in ((bf16, "lx_lora_down"), (f16, "lx_lora_down_f16")):
        Xl, Ad = FakeTensor(0x1000, (48, 3072), dt, strides=(3104, 1)), FakeTensor(0x5000, (12, 3072), dt)
        ops.lora_down(Xl, Ad, T_)
        ops.lora_down(Xl, Ad, T_, n_split=4, split_stride=1152)
        assert rec.log == [(name, (0x1000, 3104, 0x5000, 0x6000, 24, 48, 3072, 12, 1, 0, STREAM)),
                           (name, (0x1000, 3104, 0x5000, 0x6000, 24, 48, 3072, 12, 4, 1152, STREAM))]
        del rec.log[:]
        other = f16 if dt is bf16 else bf16
        with pytest.raises(TypeError, match=f"Adown: expected {dt}"):
            ops.lora_down(Xl, FakeTensor(0x5000, (12, 3072), other), T_)
        with pytest.raises(ValueError, match="X: must live on the GPU"):
            ops.lora_down(FakeTensor(0x1000, (48, 3072), dt, cuda=False), Ad, T_)
        with pytest.raises(TypeError, match="T: expected torch.float32"):
            ops.lora_down(Xl, Ad, FakeTensor(0x6000, (8, 16), bf16))
    with pytest.raises(TypeError, match="X: expected torch.bfloat16, got torch.float32"):
        ops.lora_down(FakeTensor(0x1000, (48, 3072), f32), FakeTensor(0x5000, (12, 3072), bf16), T_)
    assert rec.log == []


# ---- attention ---------------------------------------------------------------------------------------------------------------
Q = FakeTensor(0x10000, (288, 768), bf16, strides=(776, 1))
K_ = FakeTensor(0x20000, (288, 256), bf16, strides=(264, 1))
VT = FakeTensor(0x30000, (2, 2, 128, 192), bf16)
O = FakeTensor(0x40000, (288, 256), bf16, strides=(272, 1))
SEG = dict(B=2, H=2, seg_row0=[0, 64, 224], seg_len=[32, 80, 17], seg_vt0=[0, 64, 128])
S = 32 + 80 + 17


def test_attn_fwd_descriptor(rec):
    ops.attn_fwd(Q, K_, VT, O, q_col=512, k_col=0, o_col=8, **SEG)
    ops.attn_fwd(Q, K_, VT, O, q_col=512, k_col=0, o_col=8, bias=BIAS, scale=0.125, n_qseg=2, flags=ops.ATTN_Q_LOG2 | ops.ATTN_O_F16, f16_ovf=OVF,
                 qseg_mask=5, B=1, H=3, seg_row0=[0, 64], seg_len=[32, 80], seg_vt0=[0, 64])
    assert rec.log == [
        ("lx_attn_fwd", (attn_desc_bytes(0x10000, 0x20000, 0x30000, 0x40000, 776, 264, 272, 192, 512, 0, 8, 2, 2, 3, [0, 64, 224], [32, 80, 17],
                                         [0, 64, 128], ZERO3, SCALE), STREAM)),
        ("lx_attn_fwd", (attn_desc_bytes(0x10000, 0x20000, 0x30000, 0x40000, 776, 264, 272, 192, 512, 0, 8, 1, 3, 2, [0, 64, 0], [32, 80, 0],
                                         [0, 64, 0], BIAS, 0.125, n_qseg=2, flags=9, qseg_mask=5, f16_ovf=0x7000), STREAM))]


def test_attn_fwd_fp8_descriptor(rec):
    Q8, K8 = FakeTensor(0x10000, (288, 256), u8, strides=(288, 1)), FakeTensor(0x20000, (288, 256), u8, strides=(320, 1))
    VT8 = FakeTensor(0x30000, (2, 2, 128, 256), u8)
    ops.attn_fwd_fp8(Q8, K8, VT8, O, o_col=8, bias=BIAS, flags=ops.ATTN_P_EXP2, f16_ovf=OVF, qseg_mask=6, **SEG)
    q_scale = 2048.0 * (1.0 / math.sqrt(128.0)) * 1.4426950408889634 / 16.0
    assert rec.log == [("lx_attn_fwd_fp8", (attn_desc_bytes(0x10000, 0x20000, 0x30000, 0x40000, 288, 320, 272, 256, 0, 0, 8, 2, 2, 3, [0, 64, 224],
                                                            [32, 80, 17], [0, 64, 128], BIAS, SCALE, flags=32, qseg_mask=6, f16_ovf=0x7000),
                                            1.0 / (q_scale * 16.0), 1.0, STREAM))]


MASK = FakeTensor(0x50000, (1, 1, S, S), torch.bool)
WS = FakeTensor(0x60000, (4096,), u8)
MASK_BYTES = struct.pack("<Qi4i4x4qQQ", 0x50000, 0, 1, 1, S, S, S * S, S * S, S, 1, 0x60000, 4096)


def test_attn_fwd_masked_descriptor(rec):
    assert len(MASK_BYTES) == C.sizeof(_lib.AttnMaskDesc)
    out = ops.attn_fwd_masked(Q, K_, VT, O, MASK, q_col=512, k_col=0, o_col=8, bias=BIAS, flags=ops.ATTN_Q_LOG2, f16_ovf=OVF, workspace=WS, n_qseg=2,
                              **SEG)
    assert out is WS
    d = attn_desc_bytes(0x10000, 0x20000, 0x30000, 0x40000, 776, 264, 272, 192, 512, 0, 8, 2, 2, 3, [0, 64, 224], [32, 80, 17], [0, 64, 128], BIAS,
                        SCALE, n_qseg=2, flags=1, f16_ovf=0x7000)
    assert rec.log == [("lx_attn_mask_prep", (d, MASK_BYTES, STREAM)), ("lx_attn_fwd_masked", (d, MASK_BYTES, STREAM))]
    del rec.log[:]
    ops.attn_fwd_masked(Q, K_, VT, O, MASK, q_col=512, k_col=0, o_col=8, bias=BIAS, flags=ops.ATTN_Q_LOG2, f16_ovf=OVF, workspace=WS, n_qseg=2,
                        prepped=True, **SEG)
    assert rec.log == [("lx_attn_fwd_masked", (d, MASK_BYTES, STREAM))]


def test_attn_mask_prep_descriptor_has_segments_and_bias_only(rec):
    ops.attn_mask_prep(MASK, WS, bias=BIAS, B=2, H=2, seg_len=[32, 80, 17], seg_vt0=[0, 64, 128])
    d = attn_desc_bytes(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 3, [0, 0, 0], [32, 80, 17], [0, 64, 128], BIAS, 0.0)
    assert rec.log == [("lx_attn_mask_prep", (d, MASK_BYTES, STREAM))]


def test_attn_fwd_f32_descriptor(rec):
    QKV = FakeTensor(0x10000, (288, 768), f32, strides=(776, 1))
    ops.attn_fwd_f32(QKV, O, q_col=0, k_col=256, v_col=512, o_col=8, o_lo_off=128, bias=BIAS, **{k: v for k, v in SEG.items() if k != "seg_vt0"})
    ops.attn_fwd_f32(QKV, O, q_col=0, k_col=256, v_col=512, o_col=8, o_lo_off=0, scale=0.25, B=1, H=2, seg_row0=[16], seg_len=[40])
    assert rec.log == [
        ("lx_attn_fwd_f32", (attn_f32_desc_bytes(0x10000, 776, 0, 256, 512, 0x40000, 272, 8, 128, 2, 2, 3, [0, 64, 224], [32, 80, 17], BIAS, SCALE), STREAM)),
        ("lx_attn_fwd_f32", (attn_f32_desc_bytes(0x10000, 776, 0, 256, 512, 0x40000, 272, 8, 0, 1, 2, 1, [16, 0, 0], [40, 0, 0], ZERO3, 0.25), STREAM))]


def test_attn_fwd_split_descriptor(rec):
    QK2 = FakeTensor(0x10000, (288, 1024), bf16, strides=(1040, 1))
    VT2 = FakeTensor(0x30000, (2, 2, 2, 128, 192), bf16)
    ops.attn_fwd_split(QK2, VT2, O, q_col=0, k_col=256, qk_lo_off=512, o_col=8, o_lo_off=128, bias=BIAS, flags=ops.ATTN_Q_LOG2, **SEG)
    assert rec.log == [("lx_attn_fwd_split", (attn_desc_bytes(0x10000, 0x10000, 0x30000, 0x40000, 1040, 1040, 272, 192, 0, 256, 8, 2, 2, 3, [0, 64, 224],
                                                              [32, 80, 17], [0, 64, 128], BIAS, SCALE, flags=1), 512, 2 * 2 * 128 * 192, 128, STREAM))]


# ---- the launch timer --------------------------------------------------------------------------------------------------------
def _gemm_problems():
    a, b = _lib.GemmDesc(), _lib.GemmDesc()
    a.M, a.N, a.K, a.epilogue = 96, 512, 64, _lib.LX_EPI_STORE_BF16 | _lib.LX_EPI_GELU
    b.M, b.N, b.K, b.epilogue = 32, 256, 128, _lib.LX_EPI_RESID_F32
    return [a, b]


GEMM_FLOPS = 2.0 * 96 * 512 * 64 + 2.0 * 32 * 256 * 128
GEMM_BYTES = (2.0 * 96 * 64 + 2.0 * 512 * 64 + 2.0 * 96 * 512) + (2.0 * 32 * 128 + 2.0 * 256 * 128 + 8.0 * 32 * 256)
QKV32 = FakeTensor(0x10000, (288, 768), f32, strides=(776, 1))
QK2 = FakeTensor(0x10000, (288, 1024), bf16, strides=(1040, 1))
VT2 = FakeTensor(0x30000, (2, 2, 2, 128, 192), bf16)
Q8 = FakeTensor(0x10000, (288, 256), u8)
VT8 = FakeTensor(0x30000, (2, 2, 128, 256), u8)

# (name of the timed entry point, kind, flops, bytes, the call). Queries: all S rows, or the segments n_qseg / qseg_mask select.
TIMED = [
    ("lx_gemm_bf16", "gemm", GEMM_FLOPS, GEMM_BYTES, lambda: ops.gemm(_gemm_problems())),
    ("lx_gemm_bf16_ws", "gemm", GEMM_FLOPS, GEMM_BYTES, lambda: ops.gemm(_gemm_problems(), workspace=WS)),
    ("lx_attn_fwd", "attn", 4.0 * 2 * 2 * S * S * 128, 0.0, lambda: ops.attn_fwd(Q, K_, VT, O, q_col=512, k_col=0, o_col=8, **SEG)),
    ("lx_attn_fwd", "attn", 4.0 * 2 * 2 * (32 + 80) * S * 128, 0.0, lambda: ops.attn_fwd(Q, K_, VT, O, q_col=512, k_col=0, o_col=8, n_qseg=2, **SEG)),
    ("lx_attn_fwd", "attn", 4.0 * 2 * 2 * (32 + 17) * S * 128, 0.0, lambda: ops.attn_fwd(Q, K_, VT, O, q_col=512, k_col=0, o_col=8, qseg_mask=5, **SEG)),
    ("lx_attn_fwd_fp8", "attn", 4.0 * 2 * 2 * (80 + 17) * S * 128, 0.0, lambda: ops.attn_fwd_fp8(Q8, Q8, VT8, O, o_col=8, qseg_mask=6, **SEG)),
    ("lx_attn_fwd_masked", "attn", 4.0 * 2 * 2 * 32 * S * 128, 0.0,
     lambda: ops.attn_fwd_masked(Q, K_, VT, O, MASK, q_col=512, k_col=0, o_col=8, workspace=WS, prepped=True, n_qseg=1, **SEG)),
    ("lx_attn_fwd_f32", "attn", 4.0 * 2 * 2 * S * S * 128, 0.0,
     lambda: ops.attn_fwd_f32(QKV32, O, q_col=0, k_col=256, v_col=512, o_col=8, o_lo_off=128, **{k: v for k, v in SEG.items() if k != "seg_vt0"})),
    ("lx_attn_fwd_split", "attn", 4.0 * 2 * 2 * S * S * 128, 0.0,
     lambda: ops.attn_fwd_split(QK2, VT2, O, q_col=0, k_col=256, qk_lo_off=512, o_col=8, o_lo_off=128, **SEG)),
]


@pytest.mark.parametrize("case", range(len(TIMED)))
def test_launch_timer_brackets_only_when_installed_and_active(rec, monkeypatch, case):
    """LaunchTimer's contract: an installed timer that is not `active` (a forward call outside only_calls) brackets nothing."""
    name, kind, flops, nbytes, call = TIMED[case]
    call()                                                       # not installed
    assert [e[0] for e in rec.log] == [name]
    launch = rec.log[0]
    del rec.log[:]
    monkeypatch.setattr(ops, "TIMER", StubTimer(rec.log, active=True))
    call()
    assert rec.log == [("bracket", kind, flops, nbytes), ("record", "start"), launch, ("record", "end")]
    del rec.log[:]
    monkeypatch.setattr(ops, "TIMER", StubTimer(rec.log, active=False))
    call()
    assert rec.log == [launch]


def test_masked_attention_prepares_outside_the_bracket(rec, monkeypatch):
    monkeypatch.setattr(ops, "TIMER", StubTimer(rec.log, active=True))
    ops.attn_fwd_masked(Q, K_, VT, O, MASK, q_col=512, k_col=0, o_col=8, workspace=WS, **SEG)
    assert [e[0] for e in rec.log] == ["lx_attn_mask_prep", "bracket", "record", "lx_attn_fwd_masked", "record"]
