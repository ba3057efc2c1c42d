"""CPU-only: the host layer of precise mode's condition cache. What ops.attn_fwd_split and ops.qkv_prep_split_kv_segs hand to the C ABI
(ops.lib replaced by a recorder, tensors by stand-ins: the style of tests/test_ops_marshal_cpu.py), what the launch timer is told, and
what lx_attn_fwd_split / lx_qkv_prep_split_kv_segs refuse on the host before anything is launched (fake, aligned addresses)."""
import ctypes as C
import math
import struct

import pytest
import torch

from loongx_amd import _lib, ops

STREAM = 0x5EA0
bf16, f32 = torch.bfloat16, torch.float32


class FakeTensor:
    def __init__(self, ptr, shape, dtype, strides=None):
        self._ptr, self.shape, self.dtype, self.is_cuda, self.device = ptr, tuple(shape), dtype, True, "fake"
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

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._strides == FakeTensor(0, self.shape, self.dtype)._strides


class Recorder:
    """Stands in for the loaded library: every call is logged as (name, arguments), structures and arrays as their bytes, and succeeds."""

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
    active = True

    def __init__(self, log):
        self.log = log

    def bracket(self, kind, flops, nbytes=0.0):
        self.log.append(("bracket", kind, flops, nbytes))

        class Event:
            def record(self):
                pass
        return Event(), Event()


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(ops, "lib", r)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    monkeypatch.setattr(ops, "TIMER", None)
    return r


def attn_desc_bytes(Q, K, VT, O, ldq, ldk, ldo, vt_ld, q_col, k_col, o_col, B, H, n_seg, row0, length, vt0, bias, scale, n_qseg=0, flags=0,
                    qseg_mask=0, f16_ovf=0):
    b = struct.pack("<4Q19i10f3iQ", Q, K, VT, O, ldq, ldk, ldo, vt_ld, q_col, k_col, o_col, B, H, n_seg, *row0, *length, *vt0,
                    *[x for r in bias for x in r], scale, n_qseg, flags, qseg_mask, f16_ovf)
    assert len(b) == C.sizeof(_lib.AttnDesc)
    return b


ZERO3 = [[0.0] * 3] * 3
SCALE = struct.unpack("<f", struct.pack("<f", 1.0 / math.sqrt(128.0)))[0]
QK2 = FakeTensor(0x10000, (288, 1024), bf16, strides=(1040, 1))
KIMG = FakeTensor(0x20000, (288, 512), bf16, strides=(536, 1))                # a key image of another leading dimension
VT2 = FakeTensor(0x30000, (2, 2, 2, 128, 192), bf16)
VTIMG = FakeTensor(0x50000, (2, 2, 2, 128, 256), bf16)                        # V^T images of another vt_ld
O = FakeTensor(0x40000, (288, 256), bf16, strides=(272, 1))
SEG = dict(B=2, H=2, seg_row0=[0, 64, 224], seg_len=[32, 80, 17], seg_vt0=[0, 64, 128])
S = 32 + 80 + 17
KW = dict(q_col=512, k_col=0, qk_lo_off=256, o_col=8, o_lo_off=128)


def _desc(K=0x10000, VT=0x30000, ldk=1040, vt_ld=192, **kw):
    return attn_desc_bytes(0x10000, K, VT, 0x40000, 1040, ldk, 272, vt_ld, 512, 0, 8, 2, 2, 3, [0, 64, 224], [32, 80, 17], [0, 64, 128], ZERO3,
                           SCALE, **kw)


def test_attn_fwd_split_defaults_read_keys_and_vt_from_the_query_buffers(rec):
    ops.attn_fwd_split(QK2, VT2, O, **KW, **SEG)
    assert rec.log == [("lx_attn_fwd_split", (_desc(), 256, 2 * 2 * 128 * 192, 128, STREAM))]


def test_attn_fwd_split_marshals_key_image_vt_image_and_query_subsets(rec):
    ops.attn_fwd_split(QK2, VT2, O, K=KIMG, VT=VTIMG, n_qseg=2, **KW, **SEG)
    ops.attn_fwd_split(QK2, VT2, O, K=KIMG, qseg_mask=0b101, flags=ops.ATTN_Q_LOG2 | ops.ATTN_BOUNDED, **KW, **SEG)
    ops.attn_fwd_split(QK2, VT2, O, VT=VTIMG, n_qseg=1, qseg_mask=0b010, **KW, **SEG)
    assert rec.log == [
        # pointers, ldk and vt_ld of the separate images; the lo V^T image sits VT.stride(0) elements behind the hi image of the SAME tensor
        ("lx_attn_fwd_split", (_desc(K=0x20000, VT=0x50000, ldk=536, vt_ld=256, n_qseg=2), 256, 2 * 2 * 128 * 256, 128, STREAM)),
        ("lx_attn_fwd_split", (_desc(K=0x20000, ldk=536, qseg_mask=5, flags=3), 256, 2 * 2 * 128 * 192, 128, STREAM)),
        ("lx_attn_fwd_split", (_desc(VT=0x50000, vt_ld=256, n_qseg=1, qseg_mask=2), 256, 2 * 2 * 128 * 256, 128, STREAM))]


def test_attn_fwd_split_operand_types():
    with pytest.raises(TypeError, match="K: expected torch.bfloat16"):
        ops.attn_fwd_split(QK2, VT2, O, K=FakeTensor(0x20000, (288, 512), f32), **KW, **SEG)
    with pytest.raises(TypeError, match="VT: expected torch.bfloat16"):
        ops.attn_fwd_split(QK2, VT2, O, VT=FakeTensor(0x50000, (2, 2, 2, 128, 256), f32), **KW, **SEG)


@pytest.mark.parametrize("kw,q_rows", [({}, S), (dict(n_qseg=2), 32 + 80), (dict(qseg_mask=0b010), 80), (dict(qseg_mask=0b101), 32 + 17),
                                       (dict(n_qseg=1, qseg_mask=0b110), 80 + 17)])
def test_attn_fwd_split_timed_cost_counts_query_rows_only(rec, monkeypatch, kw, q_rows):
    monkeypatch.setattr(ops, "TIMER", StubTimer(rec.log))
    ops.attn_fwd_split(QK2, VT2, O, K=KIMG, VT=VTIMG, **kw, **KW, **SEG)
    assert rec.log[0] == ("bracket", "attn", 4.0 * 2 * 2 * q_rows * S * 128, 0.0)      # every key, the queries of the query segments
    assert [e[0] for e in rec.log] == ["bracket", "lx_attn_fwd_split"]


def test_qkv_prep_split_kv_segs_marshals_its_destinations(rec):
    QKV = FakeTensor(0x9000, (224, 768), f32, strides=(776, 1))
    W1, W2, COS, SIN = (FakeTensor(p, (128,), f32) for p in (0xA000, 0xA100, 0xA200, 0xA300))
    segs = [(0, 32, 0, W1, W2, COS, SIN), (64, 80, 64, W1, W2, None, None)]
    ops.qkv_prep_split_kv_segs(QKV, 0, 256, 512, segs, 2, 2, QK2, 512, KIMG, 8, 256, VTIMG, eps=1e-5)
    seg_bytes = struct.pack("<4i4Q", 0, 32, 0, 0, 0xA000, 0xA100, 0xA200, 0xA300) + struct.pack("<4i4Q", 64, 80, 64, 0, 0xA000, 0xA100, 0, 0)
    assert rec.log == [("lx_qkv_prep_split_kv_segs", (0x9000, 776, 0, 256, 512, seg_bytes, 2, 2, 2, 1e-5, 0x10000, 1040, 512, 0x20000, 536, 8, 256,
                                                      0x50000, 256, 2 * 2 * 128 * 256, STREAM))]
    with pytest.raises(TypeError, match="K2: expected torch.bfloat16"):
        ops.qkv_prep_split_kv_segs(QKV, 0, 256, 512, segs, 2, 2, QK2, 512, FakeTensor(0x20000, (288, 512), f32), 8, 256, VTIMG)


# ---- what the two entry points refuse on the host (the real library; nothing is launched) ---------------------------------------------
A = 0x10000
NINF = float("-inf")


def _rejected(status, text):
    assert status == -1                  # LX_ERR_INVALID
    assert _lib.lib.lx_last_error().decode() == text


def _attn(n_qseg=0, qseg_mask=0, row0=(0, 80, 280), vt_ld=320, bias=None, n_seg=3):
    d = _lib.AttnDesc()
    d.Q = d.K = d.VT = d.O = A
    d.ldq = d.ldk = 1024
    d.ldo, d.vt_ld = 512, vt_ld
    d.q_col, d.k_col, d.o_col, d.B, d.H, d.n_seg = 512, 0, 0, 2, 2, n_seg
    for i, (r, L, v) in enumerate(zip(row0, (40, 100, 70), (0, 64, 192))):
        d.seg_row0[i], d.seg_len[i], d.seg_vt0[i] = r, L, v
    for i in range(3):
        for j in range(3):
            d.bias[i][j] = 0.0 if bias is None else bias[i][j]
    d.scale, d.n_qseg, d.qseg_mask = 0.088, n_qseg, qseg_mask
    return _lib.lib.lx_attn_fwd_split(C.byref(d), 256, 2 * 2 * 128 * vt_ld, 256, None)


def test_attn_fwd_split_refuses_bad_query_subsets():
    _rejected(_attn(n_qseg=4), "lx_attn_fwd_split: n_qseg=4 must be 0..n_seg")
    _rejected(_attn(n_qseg=-1), "lx_attn_fwd_split: n_qseg=-1 must be 0..n_seg")
    _rejected(_attn(n_qseg=3, n_seg=2), "lx_attn_fwd_split: n_qseg=3 must be 0..n_seg")
    _rejected(_attn(qseg_mask=8), "lx_attn_fwd_split: qseg_mask=8 names a segment >= n_seg")
    _rejected(_attn(qseg_mask=4, n_seg=2), "lx_attn_fwd_split: qseg_mask=4 names a segment >= n_seg")
    _rejected(_attn(qseg_mask=-1), "lx_attn_fwd_split: qseg_mask=-1 names a segment >= n_seg")


def test_attn_fwd_split_refuses_unwritable_rows_that_a_query_segment_writes():
    # segment 2 has no queries, and its rows [200, 340) of O lie inside segment 1's [80, 280)
    _rejected(_attn(n_qseg=2, row0=(0, 80, 200)),
              "lx_attn_fwd_split: n_qseg / qseg_mask leave segment 2 without queries, but its rows [200, 340) of O overlap query segment 1's rows [80, 280)")
    _rejected(_attn(qseg_mask=0b100, row0=(0, 80, 40)),
              "lx_attn_fwd_split: n_qseg / qseg_mask leave segment 0 without queries, but its rows [0, 80) of O overlap query segment 2's rows [40, 180)")


def test_attn_fwd_split_fully_masked_check_is_for_query_segments():
    dead2 = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [NINF, NINF, NINF]]
    _rejected(_attn(bias=dead2), "lx_attn_fwd_split: query segment 2 is masked from every key segment")
    _rejected(_attn(bias=dead2, qseg_mask=0b110), "lx_attn_fwd_split: query segment 2 is masked from every key segment")
    # (with segment 2 a key-only segment the table is accepted: tests/test_precise_cond_cache_gpu.py launches it)


def test_attn_fwd_split_refuses_vt_tiles_past_vt_ld():
    # segment 2: vt0 = 192, 70 keys -> two 64-slot tiles, ending at 320
    _rejected(_attn(vt_ld=256), "lx_attn_fwd_split: segment 2's V^T tiles end at 320 > vt_ld=256")
    _rejected(_attn(vt_ld=256, n_qseg=2), "lx_attn_fwd_split: segment 2's V^T tiles end at 320 > vt_ld=256")      # a key-only segment is read too
    _rejected(_attn(vt_ld=128, n_seg=2), "lx_attn_fwd_split: segment 1's V^T tiles end at 192 > vt_ld=128")


def _prep(ldq2=1024, ldk2=512, k2_col=0, q2_col=512, lo_off=256, vt_ld=128, K2=A, rows=((0, 64, 0), (64, 40, 64))):
    seg = (_lib.QkvSeg * len(rows))()
    for i, (row0, rpb, vt0) in enumerate(rows):
        seg[i].row0, seg[i].rows_per_batch, seg[i].vt_pos0 = row0, rpb, vt0
    return _lib.lib.lx_qkv_prep_split_kv_segs(A, 768, 512, 0, 256, seg, len(rows), 1, 2, 1e-6, A, ldq2, q2_col, K2, ldk2, k2_col, lo_off, A, vt_ld,
                                              2 * 128 * vt_ld, None)


def test_qkv_prep_split_kv_segs_refuses_destinations_that_do_not_fit():
    e = "lx_qkv_prep_split_kv_segs"
    _rejected(_prep(K2=None), f"{e}: bad arguments")
    _rejected(_prep(ldk2=516), f"{e}: ldk2 must be a multiple of 8, K2 16-byte aligned")
    _rejected(_prep(K2=A + 4), f"{e}: ldk2 must be a multiple of 8, K2 16-byte aligned")
    _rejected(_prep(ldk2=504), f"{e}: q2_col / k2_col + lo_off + H*128 must fit ldq2=1024 / ldk2=504")
    _rejected(_prep(k2_col=8), f"{e}: q2_col / k2_col + lo_off + H*128 must fit ldq2=1024 / ldk2=512")
    _rejected(_prep(ldq2=1016), f"{e}: q2_col / k2_col + lo_off + H*128 must fit ldq2=1016 / ldk2=512")
    _rejected(_prep(vt_ld=64), f"{e}: segment 1's V^T tiles end at 128 > vt_ld=64")
    _rejected(_prep(rows=((0, 64, 0), (64, 70, 64))), f"{e}: segment 1's V^T tiles end at 192 > vt_ld=128")
