"""CPU-only: what lx_qkv_prep_kv_segs / lx_qkv_prep_kv_f16in_segs (the 16-bit q / k / v pass with the keys in an image of their own) reject
on the host, in the style of tests/test_host_validation_cpu.py: every call is refused before anything is launched (fake, aligned
addresses: nothing dereferences them), with LX_ERR_INVALID and a message that names the entry point."""
import pytest

from loongx_amd import _lib

A = 0x10000          # 16-byte aligned
A4 = 0x10004         # 4-byte aligned only

GOOD = [(0, 64, 0, A, A, A, A), (64, 40, 64, A, A, A, A)]      # (row0, rows_per_batch, vt_pos0, wq, wk, cos, sin): tiles [0, 64) and [64, 128)
DEFAULTS = dict(QKV=A, ld=768, q_col=512, k_col=0, v_col=256, rows=GOOD, seg=True, n_seg=2, n_batches=1, H=2, eps=1e-6, K2=A, ldk2=256, k2_col=0,
                VT=A, vt_ld=128)
ENTRIES = ("lx_qkv_prep_kv_segs", "lx_qkv_prep_kv_f16in_segs")


def _segs(rows):
    arr = (_lib.QkvSeg * max(len(rows), 1))()
    for i, (row0, rpb, vt0, wq, wk, cos, sin) in enumerate(rows):
        arr[i].row0, arr[i].rows_per_batch, arr[i].vt_pos0 = row0, rpb, vt0
        arr[i].wq, arr[i].wk, arr[i].cos_tab, arr[i].sin_tab = wq, wk, cos, sin
    return arr


def _call(entry, **over):
    a = dict(DEFAULTS, **over)
    seg = _segs(a["rows"]) if a["seg"] else None
    return getattr(_lib.lib, entry)(a["QKV"], a["ld"], a["q_col"], a["k_col"], a["v_col"], seg, a["n_seg"], a["n_batches"], a["H"], a["eps"],
                                    a["K2"], a["ldk2"], a["k2_col"], a["VT"], a["vt_ld"], None)


def _rejected(status, text):
    assert status == -1                  # LX_ERR_INVALID
    assert _lib.lib.lx_last_error().decode() == text


def _rows(seg, field, value):
    rows = [list(r) for r in GOOD]
    rows[seg][field] = value
    return [tuple(r) for r in rows]


def test_the_entry_points_are_exported():
    assert set(ENTRIES) <= set(_lib.EXPORTS)
    assert _lib.lib.lx_version() == 404


@pytest.mark.parametrize("entry", ENTRIES)
def test_segment_count(entry):
    for over in (dict(seg=False), dict(n_seg=0), dict(n_seg=4)):
        _rejected(_call(entry, **over), f"{entry}: 1..3 segments")
    # the segment count comes first
    _rejected(_call(entry, n_seg=4, ld=770, K2=None), f"{entry}: 1..3 segments")


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_operands(entry):
    for over in (dict(K2=None), dict(QKV=None), dict(VT=None), dict(n_batches=0), dict(H=0)):
        _rejected(_call(entry, **over), f"{entry}: bad arguments")


@pytest.mark.parametrize("entry", ENTRIES)
def test_alignment(entry):
    for over in (dict(ld=772), dict(q_col=516), dict(k_col=4), dict(v_col=260), dict(QKV=A4)):
        _rejected(_call(entry, **over), f"{entry}: ld and column offsets must be multiples of 8, QKV 16-byte aligned")
    for over in (dict(ldk2=260), dict(k2_col=4, ldk2=264), dict(K2=A4), dict(k2_col=-8), dict(ldk2=248), dict(k2_col=8)):
        a = dict(DEFAULTS, **over)
        _rejected(_call(entry, **over), f"{entry}: ldk2={a['ldk2']} / k2_col={a['k2_col']} must be multiples of 8 with k2_col + H*128 <= ldk2, "
                                        "K2 16-byte aligned")
    for over in (dict(vt_ld=96), dict(vt_ld=160), dict(VT=A4)):
        _rejected(_call(entry, **over), f"{entry}: vt_ld must be a multiple of 64, VT 16-byte aligned")
    # in that order
    _rejected(_call(entry, ld=772, ldk2=260, vt_ld=96), f"{entry}: ld and column offsets must be multiples of 8, QKV 16-byte aligned")
    _rejected(_call(entry, ldk2=260, vt_ld=96), f"{entry}: ldk2=260 / k2_col=0 must be multiples of 8 with k2_col + H*128 <= ldk2, K2 16-byte aligned")


@pytest.mark.parametrize("entry", ENTRIES)
def test_segments_and_their_tiles(entry):
    _rejected(_call(entry, rows=_rows(1, 1, 0)), f"{entry}: empty segment 1")
    _rejected(_call(entry, rows=_rows(0, 6, None)), f"{entry}: cos/sin tables must come together")
    for vt0 in (32, 96, -64):                                # a multiple of 64, and not negative: the tiles are the launch's own
        _rejected(_call(entry, rows=_rows(1, 2, vt0)), f"{entry}: vt_pos0 must be a multiple of 64")
    _rejected(_call(entry, rows=_rows(0, 2, 32)), f"{entry}: vt_pos0 must be a multiple of 64")
    # a tile running past vt_ld: 40 rows from slot 128 end at 192; 65 rows from slot 0 end at 128 only when rounded up
    _rejected(_call(entry, rows=_rows(1, 2, 128)), f"{entry}: segment 1's V^T tiles end at 192 > vt_ld=128")
    _rejected(_call(entry, vt_ld=64), f"{entry}: segment 1's V^T tiles end at 128 > vt_ld=64")
    _rejected(_call(entry, rows=[(0, 129, 0, A, A, A, A)], n_seg=1), f"{entry}: segment 0's V^T tiles end at 192 > vt_ld=128")
    # the operands are looked at before the segments
    _rejected(_call(entry, K2=None, rows=_rows(1, 2, 128)), f"{entry}: bad arguments")
