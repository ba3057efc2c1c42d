"""CPU-only: what the ln-modulate, qkv-prep and attention entry points reject on the host, which status they return and the complete
lx_last_error() text, check order included. Every call here is refused before anything is launched (fake, aligned addresses:
nothing dereferences them), so a call that would pass validation never appears -- where an entry point ACCEPTS a value that
another one rejects, the accepting call carries a later defect (an empty segment 1) and the test pins that later message.
(lx_attn_mask_workspace launches nothing: its accepting call is here.)"""
import ctypes as C

import pytest

from loongx_amd import _lib

A = 0x10000          # 16-byte aligned
A4 = 0x10004         # 4-byte aligned only
A2 = 0x10002         # 2-byte aligned only


def _rejected(status, text):
    assert status == -1                  # LX_ERR_INVALID
    assert _lib.lib.lx_last_error().decode() == text


def _ln_segs(rows):
    arr = (_lib.LnSeg * max(len(rows), 1))()
    for i, (row0, n_rows, rpb, sh, sc) in enumerate(rows):
        arr[i].row0, arr[i].n_rows, arr[i].rows_per_batch, arr[i].shift, arr[i].scale = row0, n_rows, rpb, sh, sc
    return arr


def _qkv_segs(rows):
    arr = (_lib.QkvSeg * max(len(rows), 1))()
    for i, (row0, rpb, vt0, wq, wk, cos, sin) in enumerate(rows):
        arr[i].row0, arr[i].rows_per_batch, arr[i].vt_pos0 = row0, rpb, vt0
        arr[i].wq, arr[i].wk, arr[i].cos_tab, arr[i].sin_tab = wq, wk, cos, sin
    return arr


LN_GOOD = [(0, 8, 8, A, A), (8, 8, 4, A, A)]
QKV_GOOD = [(0, 64, 0, A, A, A, A), (64, 64, 64, A, A, A, A)]


def _seg_rows(good, seg, field, value):
    rows = [list(r) for r in good]
    rows[seg][field] = value
    return [tuple(r) for r in rows]


# ---- ln-modulate -------------------------------------------------------------------------------------------------------------
LN_DEFAULTS = dict(X=A, ldx=256, rows=LN_GOOD, seg=True, n_seg=2, mod_ld=256, Y=A, ldy=512, D=256, eps=1e-6, Adown=A, R=16, T=A, ldt=16,
                   lora_row0=0, lora_rows=8, f16_ovf=None, Y8=A, ldy8=256, y8_scale=1.0, y_lo_off=256)


def _ln_call(entry, **over):
    a = dict(LN_DEFAULTS, **over)
    seg = _ln_segs(a["rows"]) if a["seg"] else None
    head = (a["X"], a["ldx"], seg, a["n_seg"], a["mod_ld"], a["Y"], a["ldy"])
    lora = (a["Adown"], a["R"], a["T"], a["ldt"], a["lora_row0"], a["lora_rows"])
    lib = _lib.lib
    if entry == "lx_ln_modulate_segs":
        return lib.lx_ln_modulate_segs(*head, a["D"], a["eps"], None)
    if entry == "lx_ln_modulate_f16_segs":
        return lib.lx_ln_modulate_f16_segs(*head, a["D"], a["eps"], a["f16_ovf"], None)
    if entry == "lx_ln_modulate_lora_segs":
        return lib.lx_ln_modulate_lora_segs(*head, a["D"], a["eps"], *lora, None)
    if entry == "lx_ln_modulate_lora_f16_segs":
        return lib.lx_ln_modulate_lora_f16_segs(*head, a["D"], a["eps"], *lora, a["f16_ovf"], None)
    if entry == "lx_ln_modulate_fp8_segs":
        return lib.lx_ln_modulate_fp8_segs(*head, a["Y8"], a["ldy8"], a["y8_scale"], a["D"], a["eps"], None)
    if entry == "lx_ln_modulate_split_segs":
        return lib.lx_ln_modulate_split_segs(*head, a["y_lo_off"], a["D"], a["eps"], None)
    raise KeyError(entry)


ROWOPS_LN = ("lx_ln_modulate_segs", "lx_ln_modulate_f16_segs", "lx_ln_modulate_lora_segs", "lx_ln_modulate_lora_f16_segs")
LN_ALL = ROWOPS_LN + ("lx_ln_modulate_fp8_segs", "lx_ln_modulate_split_segs")


@pytest.mark.parametrize("entry", LN_ALL)
def test_ln_segment_list(entry):
    # the rowops.hip forms report their segment defects under the name of the plain entry point, whichever form was called
    seg_name = "lx_ln_modulate" if entry in ROWOPS_LN else entry
    for over in (dict(seg=False), dict(n_seg=0), dict(n_seg=4)):
        _rejected(_ln_call(entry, **over), f"{entry}: 1..3 segments")
    _rejected(_ln_call(entry, rows=_seg_rows(LN_GOOD, 0, 3, None)), f"{seg_name}: bad segment 0")
    _rejected(_ln_call(entry, rows=_seg_rows(LN_GOOD, 1, 4, None)), f"{seg_name}: bad segment 1")
    _rejected(_ln_call(entry, rows=_seg_rows(LN_GOOD, 1, 1, 0)), f"{seg_name}: bad segment 1")
    _rejected(_ln_call(entry, rows=_seg_rows(LN_GOOD, 1, 2, 0)), f"{seg_name}: bad segment 1")
    _rejected(_ln_call(entry, rows=_seg_rows(LN_GOOD, 0, 3, A4)), f"{seg_name}: misaligned modulation table")
    _rejected(_ln_call(entry, rows=_seg_rows(LN_GOOD, 1, 4, A4)), f"{seg_name}: misaligned modulation table")
    # segment 0 is looked at completely before segment 1
    _rejected(_ln_call(entry, rows=[(0, 8, 8, A4, A), (8, 0, 4, A, A)]), f"{seg_name}: misaligned modulation table")
    # the segment count comes first
    _rejected(_ln_call(entry, n_seg=4, D=258), f"{entry}: 1..3 segments")
    _rejected(_ln_call(entry, n_seg=0, X=None), f"{entry}: 1..3 segments")


@pytest.mark.parametrize("entry", ROWOPS_LN)
def test_ln_rowops_operands(entry):
    _rejected(_ln_call(entry, X=None), "lx_ln_modulate: NULL operand")
    _rejected(_ln_call(entry, Y=None), "lx_ln_modulate: NULL operand")
    _rejected(_ln_call(entry, D=258), "lx_ln_modulate: D=258 must be a multiple of 4 and <= 16384")
    _rejected(_ln_call(entry, D=0), "lx_ln_modulate: D=0 must be a multiple of 4 and <= 16384")
    _rejected(_ln_call(entry, D=16388), "lx_ln_modulate: D=16388 must be a multiple of 4 and <= 16384")
    for over in (dict(ldx=258), dict(ldy=514), dict(mod_ld=258)):
        _rejected(_ln_call(entry, **over), "lx_ln_modulate: ldx/ldy/mod_ld must be multiples of 4")
    _rejected(_ln_call(entry, X=A4), "lx_ln_modulate: misaligned operand")
    _rejected(_ln_call(entry, Y=A4), "lx_ln_modulate: misaligned operand")
    # here the segments are checked BEFORE the operands (the fp8 and split forms do it the other way round)
    _rejected(_ln_call(entry, D=258, rows=_seg_rows(LN_GOOD, 1, 1, 0)), "lx_ln_modulate: bad segment 1")
    _rejected(_ln_call(entry, X=None, D=258, ldx=258), "lx_ln_modulate: NULL operand")
    _rejected(_ln_call(entry, D=258, ldx=258, Y=A4), "lx_ln_modulate: D=258 must be a multiple of 4 and <= 16384")


@pytest.mark.parametrize("entry", ("lx_ln_modulate_lora_segs", "lx_ln_modulate_lora_f16_segs"))
def test_ln_lora_arguments(entry):
    # (both adapter forms report under the bf16 form's name)
    _rejected(_ln_call(entry, D=512), "lx_ln_modulate_lora_segs: the fused down-projection exists for D = 3072 and 256 (D=512): use lx_lora_down")
    _rejected(_ln_call(entry, R=17), "lx_ln_modulate_lora_segs: bad adapter arguments (R=17)")
    _rejected(_ln_call(entry, R=0), "lx_ln_modulate_lora_segs: bad adapter arguments (R=0)")
    for over in (dict(Adown=None), dict(T=None), dict(ldt=8), dict(lora_rows=0), dict(lora_row0=-1)):
        _rejected(_ln_call(entry, **over), "lx_ln_modulate_lora_segs: bad adapter arguments (R=16)")
    _rejected(_ln_call(entry, Adown=A4), "lx_ln_modulate_lora_segs: Adown must be 16-byte aligned")
    # the adapter is looked at last
    _rejected(_ln_call(entry, D=512, X=A4), "lx_ln_modulate: misaligned operand")
    _rejected(_ln_call(entry, D=512, R=17, Adown=A4), "lx_ln_modulate_lora_segs: the fused down-projection exists for D = 3072 and 256 (D=512): use lx_lora_down")
    _rejected(_ln_call(entry, R=17, Adown=A4), "lx_ln_modulate_lora_segs: bad adapter arguments (R=17)")


@pytest.mark.parametrize("entry", ("lx_ln_modulate_f16_segs", "lx_ln_modulate_lora_f16_segs"))
def test_ln_f16_overflow_word(entry):
    _rejected(_ln_call(entry, f16_ovf=A2), f"{entry}: f16_ovf must be 4-byte aligned")
    # between the segment count and the segments themselves
    _rejected(_ln_call(entry, f16_ovf=A2, n_seg=4), f"{entry}: 1..3 segments")
    _rejected(_ln_call(entry, f16_ovf=A2, rows=_seg_rows(LN_GOOD, 0, 3, None)), f"{entry}: f16_ovf must be 4-byte aligned")
    _rejected(_ln_call(entry, f16_ovf=A4, D=258), "lx_ln_modulate: D=258 must be a multiple of 4 and <= 16384")


def _ln_plain(X=A, ldx=256, shift=A, scale=A, mod_ld=256, Y=A, ldy=256, M=16, D=256, rpb=8):
    return _lib.lib.lx_ln_modulate(X, ldx, shift, scale, mod_ld, Y, ldy, M, D, rpb, 1e-6, None)


def test_ln_modulate_single_segment_form():
    _rejected(_ln_plain(M=0), "lx_ln_modulate: M must be > 0")
    _rejected(_ln_plain(M=-4, D=258), "lx_ln_modulate: M must be > 0")
    _rejected(_ln_plain(shift=None), "lx_ln_modulate: bad segment 0")
    _rejected(_ln_plain(scale=None), "lx_ln_modulate: bad segment 0")
    _rejected(_ln_plain(rpb=0), "lx_ln_modulate: bad segment 0")
    _rejected(_ln_plain(shift=A4), "lx_ln_modulate: misaligned modulation table")
    _rejected(_ln_plain(scale=A4), "lx_ln_modulate: misaligned modulation table")
    _rejected(_ln_plain(X=None), "lx_ln_modulate: NULL operand")
    _rejected(_ln_plain(D=258), "lx_ln_modulate: D=258 must be a multiple of 4 and <= 16384")
    _rejected(_ln_plain(ldx=258), "lx_ln_modulate: ldx/ldy/mod_ld must be multiples of 4")
    _rejected(_ln_plain(Y=A4), "lx_ln_modulate: misaligned operand")
    _rejected(_ln_plain(rpb=0, D=258), "lx_ln_modulate: bad segment 0")


def test_ln_fp8_operands():
    e = "lx_ln_modulate_fp8_segs"
    for over in (dict(X=None), dict(Y8=None), dict(D=258), dict(D=0), dict(y8_scale=0.0)):
        _rejected(_ln_call(e, **over), f"{e}: bad arguments")
    for over in (dict(ldx=258), dict(ldy=514), dict(ldy8=258), dict(mod_ld=258), dict(X=A4), dict(Y=A4), dict(Y8=A2)):
        _rejected(_ln_call(e, **over), f"{e}: leading dimensions must be multiples of 4, operands aligned")
    # operands before segments
    _rejected(_ln_call(e, D=258, rows=_seg_rows(LN_GOOD, 1, 1, 0)), f"{e}: bad arguments")
    _rejected(_ln_call(e, ldx=258, rows=_seg_rows(LN_GOOD, 0, 3, A4)), f"{e}: leading dimensions must be multiples of 4, operands aligned")
    _rejected(_ln_call(e, D=258, ldx=258), f"{e}: bad arguments")


def test_ln_split_operands():
    e = "lx_ln_modulate_split_segs"
    for over in (dict(X=None), dict(Y=None), dict(D=258), dict(D=0)):
        _rejected(_ln_call(e, **over), f"{e}: bad arguments")
    for over in (dict(ldx=258), dict(ldy=514), dict(mod_ld=258), dict(y_lo_off=258), dict(y_lo_off=128), dict(ldy=508)):
        _rejected(_ln_call(e, **over), f"{e}: ldx/ldy/mod_ld/y_lo_off must be multiples of 4 and D <= y_lo_off, y_lo_off + D <= ldy")
    _rejected(_ln_call(e, X=A4), f"{e}: misaligned operand")
    _rejected(_ln_call(e, Y=A4), f"{e}: misaligned operand")
    _rejected(_ln_call(e, D=258, rows=_seg_rows(LN_GOOD, 1, 1, 0)), f"{e}: bad arguments")
    _rejected(_ln_call(e, X=A4, rows=_seg_rows(LN_GOOD, 0, 3, A4)), f"{e}: misaligned operand")


# ---- qkv-prep ----------------------------------------------------------------------------------------------------------------
QKV_DEFAULTS = dict(QKV=A, ld=768, q_col=0, k_col=256, v_col=512, rows=QKV_GOOD, seg=True, n_seg=2, n_batches=1, H=2, eps=1e-6, VT=A, vt_ld=128,
                    Q8=A, K8=A, ld8=256, q_scale=16.0, k_scale=16.0, v_scale=1.0, QK2=A, ld2=1024, q2_col=0, k2_col=256, lo_off=512,
                    vt_lo_off=2 * 128 * 128)


def _qkv_call(entry, **over):
    a = dict(QKV_DEFAULTS, **over)
    seg = _qkv_segs(a["rows"]) if a["seg"] else None
    head = (a["QKV"], a["ld"], a["q_col"], a["k_col"], a["v_col"], seg, a["n_seg"], a["n_batches"], a["H"], a["eps"])
    lib = _lib.lib
    if entry in ("lx_qkv_prep_segs", "lx_qkv_prep_f16in_segs"):
        return getattr(lib, entry)(*head, a["VT"], a["vt_ld"], None)
    if entry in ("lx_qkv_prep_fp8_segs", "lx_qkv_prep_fp8_f16in_segs"):
        return getattr(lib, entry)(*head, a["Q8"], a["K8"], a["ld8"], a["VT"], a["vt_ld"], a["q_scale"], a["k_scale"], a["v_scale"], None)
    if entry == "lx_qkv_prep_f32_segs":
        return lib.lx_qkv_prep_f32_segs(a["QKV"], a["ld"], a["q_col"], a["k_col"], seg, a["n_seg"], a["n_batches"], a["H"], a["eps"], None)
    if entry == "lx_qkv_prep_split_segs":
        return lib.lx_qkv_prep_split_segs(*head, a["QK2"], a["ld2"], a["q2_col"], a["k2_col"], a["lo_off"], a["VT"], a["vt_ld"], a["vt_lo_off"], None)
    raise KeyError(entry)


# entry point -> (the name its segment-count message carries, the name every other message carries)
QKV_NAMES = {
    "lx_qkv_prep_segs": ("lx_qkv_prep_segs", "lx_qkv_prep"),
    "lx_qkv_prep_f16in_segs": ("lx_qkv_prep_segs", "lx_qkv_prep"),
    "lx_qkv_prep_fp8_segs": ("lx_qkv_prep_fp8_segs", "lx_qkv_prep_fp8_segs"),
    "lx_qkv_prep_fp8_f16in_segs": ("lx_qkv_prep_fp8_segs", "lx_qkv_prep_fp8_segs"),
    "lx_qkv_prep_f32_segs": ("lx_qkv_prep_f32_segs", "lx_qkv_prep_f32_segs"),
    "lx_qkv_prep_split_segs": ("lx_qkv_prep_split_segs", "lx_qkv_prep_split_segs"),
}
EMPTY_1 = _seg_rows(QKV_GOOD, 1, 1, 0)


@pytest.mark.parametrize("entry", sorted(QKV_NAMES))
def test_qkv_segment_list(entry):
    count_name, name = QKV_NAMES[entry]
    for over in (dict(seg=False), dict(n_seg=0), dict(n_seg=4)):
        _rejected(_qkv_call(entry, **over), f"{count_name}: 1..3 segments")
    _rejected(_qkv_call(entry, n_seg=4, ld=770), f"{count_name}: 1..3 segments")
    _rejected(_qkv_call(entry, n_seg=0, QKV=None), f"{count_name}: 1..3 segments")
    _rejected(_qkv_call(entry, rows=_seg_rows(QKV_GOOD, 0, 1, 0)), f"{name}: empty segment 0")
    _rejected(_qkv_call(entry, rows=EMPTY_1), f"{name}: empty segment 1")
    _rejected(_qkv_call(entry, rows=_seg_rows(QKV_GOOD, 1, 6, None)), f"{name}: cos/sin tables must come together")
    _rejected(_qkv_call(entry, rows=_seg_rows(QKV_GOOD, 0, 5, None)), f"{name}: cos/sin tables must come together")
    # segment 0 is looked at completely before segment 1; within a segment: empty, cos/sin, vt_pos0
    _rejected(_qkv_call(entry, rows=[(0, 64, 0, A, A, A, None), (64, 0, 64, A, A, A, A)]), f"{name}: cos/sin tables must come together")
    _rejected(_qkv_call(entry, rows=[(0, 0, 32, A, A, A, None), (64, 64, 64, A, A, A, A)]), f"{name}: empty segment 0")
    _rejected(_qkv_call(entry, rows=[(0, 64, 32, A, A, A, None), (64, 64, 64, A, A, A, A)]), f"{name}: cos/sin tables must come together")
    # operands before segments
    _rejected(_qkv_call(entry, QKV=None, rows=EMPTY_1), f"{name}: bad arguments")
    _rejected(_qkv_call(entry, n_batches=0), f"{name}: bad arguments")
    _rejected(_qkv_call(entry, H=0), f"{name}: bad arguments")


@pytest.mark.parametrize("entry", sorted(QKV_NAMES))
def test_qkv_vt_pos0(entry):
    """Which vt_pos0 values each form rejects: the bf16 forms only with a V^T image, the fp8 forms always, the split form also a
    negative one, the fp32 form none (it writes no V^T image)."""
    _, name = QKV_NAMES[entry]
    bad = f"{name}: vt_pos0 must be a multiple of 64"
    later = f"{name}: empty segment 1"

    def call(vt0, **over):
        return _qkv_call(entry, rows=[(0, 64, vt0, A, A, A, A), (64, 0, 64, A, A, A, A)], **over)
    if entry in ("lx_qkv_prep_segs", "lx_qkv_prep_f16in_segs"):
        _rejected(call(32), bad)
        _rejected(call(32, VT=None, vt_ld=0), later)
        _rejected(call(-64), later)
        _rejected(_qkv_call(entry, rows=_seg_rows(QKV_GOOD, 1, 2, 96)), bad)
    elif entry in ("lx_qkv_prep_fp8_segs", "lx_qkv_prep_fp8_f16in_segs"):
        _rejected(call(32), bad)
        _rejected(call(-64), later)
        _rejected(_qkv_call(entry, rows=_seg_rows(QKV_GOOD, 1, 2, 96)), bad)
    elif entry == "lx_qkv_prep_f32_segs":
        _rejected(call(32), later)
        _rejected(call(-64), later)
    else:
        _rejected(call(32), bad)
        _rejected(call(-64), bad)
        _rejected(_qkv_call(entry, rows=_seg_rows(QKV_GOOD, 1, 2, 96)), bad)
        _rejected(_qkv_call(entry, rows=_seg_rows(QKV_GOOD, 1, 2, -64)), bad)


@pytest.mark.parametrize("entry", ("lx_qkv_prep_segs", "lx_qkv_prep_f16in_segs"))
def test_qkv_bf16_operands(entry):
    for over in (dict(ld=772), dict(q_col=4), dict(k_col=260), dict(v_col=516)):
        _rejected(_qkv_call(entry, **over), "lx_qkv_prep: ld and column offsets must be multiples of 8")
    _rejected(_qkv_call(entry, vt_ld=96), "lx_qkv_prep: vt_ld must be a multiple of 64")
    _rejected(_qkv_call(entry, vt_ld=96, VT=None, rows=EMPTY_1), "lx_qkv_prep: empty segment 1")
    _rejected(_qkv_call(entry, ld=772, vt_ld=96, rows=EMPTY_1), "lx_qkv_prep: ld and column offsets must be multiples of 8")
    _rejected(_qkv_call(entry, vt_ld=96, rows=EMPTY_1), "lx_qkv_prep: vt_ld must be a multiple of 64")


@pytest.mark.parametrize("entry", ("lx_qkv_prep_fp8_segs", "lx_qkv_prep_fp8_f16in_segs"))
def test_qkv_fp8_operands(entry):
    e = "lx_qkv_prep_fp8_segs"          # (both forms report under this name)
    for over in (dict(Q8=None), dict(K8=None), dict(VT=None)):
        _rejected(_qkv_call(entry, **over), f"{e}: bad arguments")
    for over in (dict(ld=772), dict(q_col=4), dict(k_col=260), dict(v_col=516)):
        _rejected(_qkv_call(entry, **over), f"{e}: ld and column offsets must be multiples of 8")
    _rejected(_qkv_call(entry, ld8=264), f"{e}: ld8 % 16 and vt8_ld % 64 required")
    _rejected(_qkv_call(entry, vt_ld=96), f"{e}: ld8 % 16 and vt8_ld % 64 required")
    for over in (dict(q_scale=0.0), dict(k_scale=-1.0), dict(v_scale=0.0)):
        _rejected(_qkv_call(entry, **over), f"{e}: scales must be positive")
    _rejected(_qkv_call(entry, ld=772, ld8=264, q_scale=0.0, rows=EMPTY_1), f"{e}: ld and column offsets must be multiples of 8")
    _rejected(_qkv_call(entry, ld8=264, q_scale=0.0, rows=EMPTY_1), f"{e}: ld8 % 16 and vt8_ld % 64 required")
    _rejected(_qkv_call(entry, q_scale=0.0, rows=EMPTY_1), f"{e}: scales must be positive")


def test_qkv_f32_operands():
    e = "lx_qkv_prep_f32_segs"
    for over in (dict(ld=770), dict(q_col=2), dict(k_col=258), dict(QKV=A4)):
        _rejected(_qkv_call(e, **over), f"{e}: ld / column offsets must be multiples of 4, QKV 16-byte aligned")
    _rejected(_qkv_call(e, ld=770, rows=EMPTY_1), f"{e}: ld / column offsets must be multiples of 4, QKV 16-byte aligned")


def test_qkv_split_operands():
    e = "lx_qkv_prep_split_segs"
    for over in (dict(QK2=None), dict(VT=None)):
        _rejected(_qkv_call(e, **over), f"{e}: bad arguments")
    for over in (dict(ld=770), dict(q_col=2), dict(k_col=258), dict(v_col=514), dict(QKV=A4)):
        _rejected(_qkv_call(e, **over), f"{e}: ld / column offsets must be multiples of 4, QKV 16-byte aligned")
    for over in (dict(ld2=1028), dict(q2_col=4), dict(k2_col=260), dict(lo_off=516), dict(lo_off=128), dict(QK2=A4)):
        _rejected(_qkv_call(e, **over), f"{e}: ld2 / q2_col / k2_col / lo_off must be multiples of 8 (lo_off >= H*128), QK2 16-byte aligned")
    for over in (dict(vt_ld=96), dict(vt_lo_off=2 * 128 * 128 + 4), dict(vt_lo_off=2 * 128 * 128 - 8), dict(VT=A4)):
        _rejected(_qkv_call(e, **over), f"{e}: vt_ld % 64, vt_lo_off % 8 and the lo V^T image behind the hi image required")
    _rejected(_qkv_call(e, ld=770, ld2=1028, vt_ld=96, rows=EMPTY_1), f"{e}: ld / column offsets must be multiples of 4, QKV 16-byte aligned")
    _rejected(_qkv_call(e, vt_ld=96, rows=EMPTY_1), f"{e}: vt_ld % 64, vt_lo_off % 8 and the lo V^T image behind the hi image required")


def _qkv_plain(QKV=A, ld=768, q_col=0, k_col=256, v_col=512, row0=0, n_rows=128, rpb=64, H=2, wq=A, wk=A, cos=A, sin=A, VT=A, vt_ld=128, vt_pos0=0):
    return _lib.lib.lx_qkv_prep(QKV, ld, q_col, k_col, v_col, row0, n_rows, rpb, H, wq, wk, 1e-6, cos, sin, VT, vt_ld, vt_pos0, None)


def test_qkv_prep_single_segment_form():
    """(Without a V^T image this form accepts any vt_pos0 and has no later check to be caught by: only the rejecting side is here.)"""
    _rejected(_qkv_plain(rpb=0), "lx_qkv_prep: n_rows=128 must be a multiple of rows_per_batch=0")
    _rejected(_qkv_plain(n_rows=0), "lx_qkv_prep: n_rows=0 must be a multiple of rows_per_batch=64")
    _rejected(_qkv_plain(n_rows=100), "lx_qkv_prep: n_rows=100 must be a multiple of rows_per_batch=64")
    _rejected(_qkv_plain(rpb=0, QKV=None), "lx_qkv_prep: n_rows=128 must be a multiple of rows_per_batch=0")
    _rejected(_qkv_plain(QKV=None), "lx_qkv_prep: bad arguments")
    _rejected(_qkv_plain(H=0), "lx_qkv_prep: bad arguments")
    for over in (dict(ld=772), dict(q_col=4), dict(k_col=260), dict(v_col=516)):
        _rejected(_qkv_plain(**over), "lx_qkv_prep: ld and column offsets must be multiples of 8")
    _rejected(_qkv_plain(vt_ld=96), "lx_qkv_prep: vt_ld must be a multiple of 64")
    _rejected(_qkv_plain(sin=None), "lx_qkv_prep: cos/sin tables must come together")
    _rejected(_qkv_plain(cos=None), "lx_qkv_prep: cos/sin tables must come together")
    _rejected(_qkv_plain(sin=None, VT=None), "lx_qkv_prep: cos/sin tables must come together")
    _rejected(_qkv_plain(vt_pos0=32), "lx_qkv_prep: vt_pos0 must be a multiple of 64")
    _rejected(_qkv_plain(vt_pos0=32, sin=None), "lx_qkv_prep: cos/sin tables must come together")
    _rejected(_qkv_plain(ld=772, vt_ld=96, vt_pos0=32), "lx_qkv_prep: ld and column offsets must be multiples of 8")


# ---- precise attention: a query segment without a single key ------------------------------------------------------------------------
NINF = float("-inf")
DEAD2 = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [NINF, NINF, NINF]]


def _attn_f32(bias, n_seg=3, seg_len=(40, 100, 70), o_lo_off=256):
    d = _lib.AttnF32Desc()
    d.QKV = d.O = A
    d.ld, d.q_col, d.k_col, d.v_col = 768, 512, 0, 256
    d.ldo, d.o_col, d.o_lo_off = 512, 0, o_lo_off
    d.B, d.H, d.n_seg = 2, 2, n_seg
    for i, (r, L) in enumerate(zip((0, 80, 280), seg_len)):
        d.seg_row0[i], d.seg_len[i] = r, L
    for i in range(3):
        for j in range(3):
            d.bias[i][j] = bias[i][j]
    d.scale = 0.088
    return _lib.lib.lx_attn_fwd_f32(C.byref(d), None)


def _attn_split(bias, n_seg=3):
    d = _lib.AttnDesc()
    d.Q = d.K = d.VT = d.O = A
    d.ldq = d.ldk = 1024
    d.ldo, d.vt_ld = 512, 320
    d.q_col, d.k_col, d.o_col, d.B, d.H, d.n_seg = 512, 0, 0, 2, 2, n_seg
    for i, (r, L, v) in enumerate(zip((0, 80, 280), (40, 100, 70), (0, 64, 192))):
        d.seg_row0[i], d.seg_len[i], d.seg_vt0[i] = r, L, v
    for i in range(3):
        for j in range(3):
            d.bias[i][j] = bias[i][j]
    d.scale = 0.088
    return _lib.lib.lx_attn_fwd_split(C.byref(d), 256, 2 * 2 * 128 * 320, 256, None)


def test_precise_attention_refuses_a_query_segment_masked_from_every_key():
    """Both precise attention entry points, the same message, before any launch (the reference's softmax of such a row is NaN; the engine's
    bias table always keeps the diagonal). lx_attn_fwd_f32 has no query-segment subset: every segment is a query segment."""
    _rejected(_attn_split(DEAD2), "lx_attn_fwd_split: query segment 2 is masked from every key segment")
    _rejected(_attn_f32(DEAD2), "lx_attn_fwd_f32: query segment 2 is masked from every key segment")
    dead0 = [[NINF, NINF, NINF], [0.0, 0.0, 0.0], [NINF, NINF, NINF]]
    _rejected(_attn_f32(dead0), "lx_attn_fwd_f32: query segment 0 is masked from every key segment")
    # columns of segments past n_seg do not count as keys; rows past n_seg are not looked at
    _rejected(_attn_f32([[0.0, 0.0, 0.0], [NINF, NINF, 0.0], [0.0, 0.0, 0.0]], n_seg=2), "lx_attn_fwd_f32: query segment 1 is masked from every key segment")
    _rejected(_attn_f32([[0.0, NINF, 0.0], [NINF, 0.0, 0.0], DEAD2[2]], n_seg=2, seg_len=(40, 0, 70)), "lx_attn_fwd_f32: empty segment 1")
    # the earlier checks still come first
    _rejected(_attn_f32(DEAD2, o_lo_off=258), "lx_attn_fwd_f32: ldo / o_col / o_lo_off must be multiples of 4")


# ---- lx_attn_desc: one validator behind every entry point that takes the descriptor ---------------------------------------------------
ATTN_ENTRIES = ("lx_attn_fwd", "lx_attn_fwd_fp8", "lx_attn_fwd_split", "lx_attn_fwd_masked")
ATTN_DEFAULTS = dict(Q=A, K=A, VT=A, O=A, ldq=1024, ldk=1024, ldo=512, vt_ld=320, q_col=512, k_col=0, o_col=0, B=2, H=2, n_seg=3,
                     row0=(0, 80, 280), seg_len=(40, 100, 70), vt0=(0, 64, 192), bias=None, n_qseg=0, qseg_mask=0, flags=0, ws_short=0)
WS = 0x100000        # 256-byte aligned
BAD_FLAG = 1 << 12
ATTN_FLAG_TEXT = {
    "lx_attn_fwd": "lx_attn_fwd: flags=4096: unknown bit, LX_ATTN_BOUNDED without LX_ATTN_Q_LOG2, or LX_ATTN_INVARIANT with LX_ATTN_PREFER_4WAVE",
    "lx_attn_fwd_fp8": "lx_attn_fwd_fp8: the flags are LX_ATTN_O_F16 and LX_ATTN_P_EXP2 (the e4m3 kernels fold their own scales)",
    "lx_attn_fwd_split": "lx_attn_fwd_split: flags=4096: unknown bit, or LX_ATTN_BOUNDED without LX_ATTN_Q_LOG2",
    "lx_attn_fwd_masked": "lx_attn_fwd_masked: flags=4096: only LX_ATTN_Q_LOG2 and LX_ATTN_O_F16 are accepted",
}


def _attn_desc(a):
    d = _lib.AttnDesc()
    d.Q, d.K, d.VT, d.O = a["Q"], a["K"], a["VT"], a["O"]
    d.ldq, d.ldk, d.ldo, d.vt_ld = a["ldq"], a["ldk"], a["ldo"], a["vt_ld"]
    d.q_col, d.k_col, d.o_col, d.B, d.H, d.n_seg = a["q_col"], a["k_col"], a["o_col"], a["B"], a["H"], a["n_seg"]
    for i in range(3):
        d.seg_row0[i], d.seg_len[i], d.seg_vt0[i] = a["row0"][i], a["seg_len"][i], a["vt0"][i]
        for j in range(3):
            d.bias[i][j] = 0.0 if a["bias"] is None else a["bias"][i][j]
    d.scale, d.n_qseg, d.qseg_mask, d.flags = 0.088, a["n_qseg"], a["qseg_mask"], a["flags"]
    return d


def _attn_mask_desc(a, workspace=None, workspace_bytes=0):
    S = sum(a["seg_len"][:3])
    m = _lib.AttnMaskDesc()
    m.mask, m.dtype = 0x20000, _lib.LX_ATTN_MASK_BOOL
    for i, (n, st) in enumerate(zip((a["B"], a["H"], S, S), (a["H"] * S * S, S * S, S, 1))):
        m.dims[i], m.strides[i] = n, st
    m.workspace, m.workspace_bytes = workspace, workspace_bytes
    return m


def _attn_ws_need():
    """the workspace of the valid base descriptor (every launching case below keeps its segment lengths, B and H, or fails before the mask)"""
    n = C.c_size_t(0)
    assert _lib.lib.lx_attn_mask_workspace(C.byref(_attn_desc(ATTN_DEFAULTS)), C.byref(_attn_mask_desc(ATTN_DEFAULTS)), C.byref(n)) == 0
    return n.value


def _attn_call(entry, **over):
    a = dict(ATTN_DEFAULTS, **over)
    d = _attn_desc(a)
    lib = _lib.lib
    if entry == "lx_attn_fwd":
        return lib.lx_attn_fwd(C.byref(d), None)
    if entry == "lx_attn_fwd_fp8":
        return lib.lx_attn_fwd_fp8(C.byref(d), 0.01, 0.5, None)
    if entry == "lx_attn_fwd_split":
        return lib.lx_attn_fwd_split(C.byref(d), 256, 2 * 2 * 128 * 320, 256, None)
    if entry == "lx_attn_fwd_masked":
        m = _attn_mask_desc(ATTN_DEFAULTS, WS, _attn_ws_need() - a["ws_short"])
        return lib.lx_attn_fwd_masked(C.byref(d), C.byref(m), None)
    raise KeyError(entry)


@pytest.mark.parametrize("entry", ATTN_ENTRIES)
def test_attn_descriptor_rules(entry):
    """Each shared rule violated alone on one valid 3-segment descriptor: the same text behind every entry point, with its name in front."""
    for op in ("Q", "K", "VT", "O"):
        _rejected(_attn_call(entry, **{op: None}), f"{entry}: NULL operand")
    _rejected(_attn_call(entry, n_seg=0), f"{entry}: n_seg=0 must be 1..3")
    _rejected(_attn_call(entry, n_seg=4), f"{entry}: n_seg=4 must be 1..3")
    _rejected(_attn_call(entry, B=0), f"{entry}: bad B/H")
    if entry == "lx_attn_fwd_fp8":
        _rejected(_attn_call(entry, ldk=1032), f"{entry}: ldq/ldk % 16 (bytes), ldo % 4, vt_ld % 64 required")     # a multiple of 8 is not enough in bytes
    else:
        _rejected(_attn_call(entry, ldk=1028), f"{entry}: ldq/ldk % 8, ldo % 4, vt_ld % 64 required")
    _rejected(_attn_call(entry, n_qseg=-1), f"{entry}: n_qseg=-1 must be 0..n_seg")
    _rejected(_attn_call(entry, n_qseg=4), f"{entry}: n_qseg=4 must be 0..n_seg")
    _rejected(_attn_call(entry, qseg_mask=8), f"{entry}: qseg_mask=8 names a segment >= n_seg")
    _rejected(_attn_call(entry, qseg_mask=-1), f"{entry}: qseg_mask=-1 names a segment >= n_seg")
    _rejected(_attn_call(entry, seg_len=(40, 0, 70)), f"{entry}: empty segment 1")
    # what keeps the K / V^T staging inside the caller's V^T rows
    _rejected(_attn_call(entry, vt0=(0, 32, 192)), f"{entry}: seg_vt0 must be 64-aligned")
    _rejected(_attn_call(entry, vt0=(-64, 64, 192)), f"{entry}: seg_vt0 must be 64-aligned")
    _rejected(_attn_call(entry, vt_ld=256), f"{entry}: segment 2's V^T tiles end at 320 > vt_ld=256")
    _rejected(_attn_call(entry, vt_ld=256, n_qseg=2), f"{entry}: segment 2's V^T tiles end at 320 > vt_ld=256")       # a key-only segment is read too
    # a key-only segment's rows of O are promised untouched: no query segment may share them
    _rejected(_attn_call(entry, n_qseg=2, row0=(0, 80, 200)),
              f"{entry}: n_qseg / qseg_mask leave segment 2 without queries, but its rows [200, 340) of O overlap query segment 1's rows [80, 280)")
    _rejected(_attn_call(entry, qseg_mask=0b100, row0=(0, 80, 40)),
              f"{entry}: n_qseg / qseg_mask leave segment 0 without queries, but its rows [0, 80) of O overlap query segment 2's rows [40, 180)")
    _rejected(_attn_call(entry, flags=BAD_FLAG), ATTN_FLAG_TEXT[entry])
    # the descriptor is looked at before the entry point's own flags
    _rejected(_attn_call(entry, flags=BAD_FLAG, seg_len=(40, 0, 70)), f"{entry}: empty segment 1")


@pytest.mark.parametrize("entry", ATTN_ENTRIES[:3])
def test_attn_fully_masked_query_segment(entry):
    text = f"{entry}: query segment 2 is masked from every key segment"
    _rejected(_attn_call(entry, bias=DEAD2), text)
    _rejected(_attn_call(entry, bias=DEAD2, qseg_mask=0b110), text)
    _rejected(_attn_call(entry, bias=DEAD2, flags=BAD_FLAG), text)
    # key-only, segment 2 needs no key of its own: the call gets as far as the flag bit broken on purpose
    _rejected(_attn_call(entry, bias=DEAD2, n_qseg=2, flags=BAD_FLAG), ATTN_FLAG_TEXT[entry])
    _rejected(_attn_call(entry, bias=DEAD2, qseg_mask=0b011, flags=BAD_FLAG), ATTN_FLAG_TEXT[entry])


def test_attn_masked_accepts_a_fully_masked_query_segment():
    """lx_attn_fwd_masked does not apply that rule (a mask can empty any row; such rows are written as zeros): the descriptor gets past it
    and fails on the workspace, one byte short on purpose."""
    need = _attn_ws_need()
    _rejected(_attn_call("lx_attn_fwd_masked", bias=DEAD2, ws_short=1),
              f"lx_attn_fwd_masked: workspace of {need - 1} bytes, {need} needed (lx_attn_mask_workspace)")
    _rejected(_attn_call("lx_attn_fwd_masked", ws_short=1), f"lx_attn_fwd_masked: workspace of {need - 1} bytes, {need} needed (lx_attn_mask_workspace)")


def test_attn_mask_workspace_checks_the_segment_part_only():
    e = "lx_attn_mask_workspace"
    n = C.c_size_t(0)

    def call(**over):
        a = dict(ATTN_DEFAULTS, Q=None, K=None, VT=None, O=None, vt_ld=0, ldk=1028, n_qseg=7, row0=(0, 0, 0), flags=BAD_FLAG, **over)
        return _lib.lib.lx_attn_mask_workspace(C.byref(_attn_desc(a)), C.byref(_attn_mask_desc(ATTN_DEFAULTS)), C.byref(n))
    assert call() == 0 and n.value == _attn_ws_need() > 0        # no operands, no vt_ld, no query subset: a size all the same
    _rejected(call(n_seg=0), f"{e}: n_seg=0 must be 1..3")
    _rejected(call(n_seg=4), f"{e}: n_seg=4 must be 1..3")
    _rejected(call(B=0), f"{e}: bad B/H")
    _rejected(call(seg_len=(40, 0, 70)), f"{e}: empty segment 1")
    _rejected(call(vt0=(0, 32, 192)), f"{e}: seg_vt0 must be 64-aligned")
    _rejected(call(vt0=(-64, 64, 192)), f"{e}: seg_vt0 must be 64-aligned")
