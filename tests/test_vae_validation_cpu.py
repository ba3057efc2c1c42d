"""CPU-only: what the VAE glue entry points of vae.hip reject on the host, which status they return and the complete lx_last_error()
text, check order included (the method of test_host_validation_cpu.py). Every call here is refused before anything is launched (fake
addresses: nothing dereferences them); where an entry point ACCEPTS a value that a sibling rejects, the accepting call carries a later
defect and the test pins that later message. (lx_groupnorm_workspace_bytes launches nothing, and lx_convert_f16 of n = 0 elements
returns before its launch: their accepting calls are here.)"""
import pytest

from loongx_amd import _lib

A = 0x10000          # 16-byte aligned
A8 = 0x10008         # 8-byte aligned only
A4 = 0x10004         # 4-byte aligned only
A2 = 0x10002         # 2-byte aligned only
A1 = 0x10001         # odd


def _rejected(status, text):
    assert status == -1                  # LX_ERR_INVALID
    assert _lib.lib.lx_last_error().decode() == text


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------
GN_ENTRIES = ("lx_groupnorm_silu", "lx_groupnorm_silu_f16", "lx_groupnorm_silu_split")
GN_DEFAULTS = dict(x=A, x_is_bf16=0, B=2, P=256, C=128, G=32, gamma=A, beta=A, eps=1e-6, silu=1, y=A, ws=A, ws_bytes=8192, f16_ovf=None,
                   ldy=256, y_lo_off=128)


def _gn_call(entry, **over):
    a = dict(GN_DEFAULTS, **over)
    dims = (a["B"], a["P"], a["C"], a["G"], a["gamma"], a["beta"], a["eps"], a["silu"], a["y"])
    lib = _lib.lib
    if entry == "lx_groupnorm_silu":
        return lib.lx_groupnorm_silu(a["x"], a["x_is_bf16"], *dims, a["ws"], a["ws_bytes"], None)
    if entry == "lx_groupnorm_silu_f16":
        return lib.lx_groupnorm_silu_f16(a["x"], *dims, a["ws"], a["ws_bytes"], a["f16_ovf"], None)
    if entry == "lx_groupnorm_silu_split":
        return lib.lx_groupnorm_silu_split(a["x"], *dims, a["ldy"], a["y_lo_off"], a["ws"], a["ws_bytes"], None)
    raise KeyError(entry)


def test_groupnorm_workspace_bytes():
    """One partial (sum, sumsq) per image, row chunk and group: 1 chunk below 256 pixels, 16 from there, 64 from 4096."""
    ws = _lib.lib.lx_groupnorm_workspace_bytes
    assert ws(2, 255, 32) == 2 * 1 * 32 * 8 == 512
    assert ws(2, 256, 32) == 2 * 16 * 32 * 8 == 8192
    assert ws(2, 4096, 32) == 2 * 64 * 32 * 8 == 32768


@pytest.mark.parametrize("entry", GN_ENTRIES)
def test_groupnorm_shared_rules(entry):
    for op in ("x", "y", "gamma", "beta", "ws"):
        _rejected(_gn_call(entry, **{op: None}), f"{entry}: NULL operand")

    def shape(C_, G):
        return f"{entry}: need G <= 64, C % G == 0, (C/G) % 4 == 0, C/4 a divisor of 256 (C={C_} G={G})"
    _rejected(_gn_call(entry, B=0), shape(128, 32))
    _rejected(_gn_call(entry, P=0), shape(128, 32))
    _rejected(_gn_call(entry, C=0), shape(0, 32))
    _rejected(_gn_call(entry, G=0), shape(128, 0))
    _rejected(_gn_call(entry, C=260, G=65), shape(260, 65))          # G <= 64
    _rejected(_gn_call(entry, C=100), shape(100, 32))                # C % G
    _rejected(_gn_call(entry, C=64), shape(64, 32))                  # (C/G) % 4
    _rejected(_gn_call(entry, C=2048), shape(2048, 32))              # C <= 1024
    _rejected(_gn_call(entry, C=96, G=8), shape(96, 8))              # C/4 = 24 does not divide 256
    _rejected(_gn_call(entry, ws_bytes=8191), f"{entry}: workspace too small")
    _rejected(_gn_call(entry, P=255, ws_bytes=511), f"{entry}: workspace too small")
    _rejected(_gn_call(entry, P=4096, ws_bytes=32767), f"{entry}: workspace too small")
    # order: operands, shape, ..., workspace
    _rejected(_gn_call(entry, x=None, C=100, ws_bytes=0), f"{entry}: NULL operand")
    _rejected(_gn_call(entry, C=100, ws_bytes=0), shape(100, 32))


def test_groupnorm_bf16_form_checks_no_alignment():
    e = "lx_groupnorm_silu"
    for over in (dict(x=A2), dict(y=A2), dict(gamma=A4), dict(beta=A4), dict(x=A2, x_is_bf16=1)):
        _rejected(_gn_call(e, ws_bytes=8191, **over), f"{e}: workspace too small")


def test_groupnorm_f16_alignment():
    e = "lx_groupnorm_silu_f16"
    for over in (dict(x=A8), dict(y=A4), dict(gamma=A8), dict(beta=A8), dict(f16_ovf=A2)):
        _rejected(_gn_call(e, **over), f"{e}: misaligned operand")
    # y needs 8 bytes, the counter 4, and a NULL counter is accepted
    _rejected(_gn_call(e, y=A8, f16_ovf=A4, ws_bytes=8191), f"{e}: workspace too small")
    _rejected(_gn_call(e, f16_ovf=None, ws_bytes=8191), f"{e}: workspace too small")
    # between the shape and the workspace
    _rejected(_gn_call(e, x=A8, C=100), f"{e}: need G <= 64, C % G == 0, (C/G) % 4 == 0, C/4 a divisor of 256 (C=100 G=32)")
    _rejected(_gn_call(e, x=A8, ws_bytes=0), f"{e}: misaligned operand")


def test_groupnorm_split_layout_and_alignment():
    e = "lx_groupnorm_silu_split"

    def pair(ldy, off, C_=128):
        return f"{e}: need y_lo_off % 8 == 0, C <= y_lo_off, y_lo_off + C <= ldy, ldy % 4 == 0 (C={C_} ldy={ldy} y_lo_off={off})"
    _rejected(_gn_call(e, y_lo_off=132, ldy=264), pair(264, 132))    # y_lo_off % 8
    _rejected(_gn_call(e, y_lo_off=120), pair(256, 120))             # C <= y_lo_off
    _rejected(_gn_call(e, ldy=258), pair(258, 128))                  # ldy % 4
    _rejected(_gn_call(e, ldy=252), pair(252, 128))                  # y_lo_off + C <= ldy
    for over in (dict(x=A8), dict(y=A4), dict(gamma=A8), dict(beta=A8)):
        _rejected(_gn_call(e, **over), f"{e}: misaligned operand")
    # a wider row and an 8-byte aligned y are accepted
    _rejected(_gn_call(e, y=A8, ldy=260, ws_bytes=8191), f"{e}: workspace too small")
    # order: shape, pair layout, alignment, workspace
    _rejected(_gn_call(e, C=100, ldy=258), f"{e}: need G <= 64, C % G == 0, (C/G) % 4 == 0, C/4 a divisor of 256 (C=100 G=32)")
    _rejected(_gn_call(e, ldy=258, x=A8, ws_bytes=0), pair(258, 128))
    _rejected(_gn_call(e, x=A8, ws_bytes=0), f"{e}: misaligned operand")


# ---- im2col ------------------------------------------------------------------------------------------------------------------
IM_ENTRIES = ("lx_im2col3x3", "lx_im2col3x3_split")
IM_DEFAULTS = dict(x=A, ldx=48, x_lo_off=24, B=2, H=4, W=6, C=24, mode=0, out=A, Kpad=256)


def _im_call(entry, **over):
    a = dict(IM_DEFAULTS, **over)
    tail = (a["B"], a["H"], a["W"], a["C"], a["mode"], a["out"], a["Kpad"], None)
    if entry == "lx_im2col3x3":
        return _lib.lib.lx_im2col3x3(a["x"], *tail)
    return _lib.lib.lx_im2col3x3_split(a["x"], a["ldx"], a["x_lo_off"], *tail)


@pytest.mark.parametrize("entry", IM_ENTRIES)
def test_im2col_shared_rules(entry):
    for over in (dict(x=None), dict(out=None), dict(B=0), dict(H=0), dict(W=0), dict(C=0)):
        _rejected(_im_call(entry, **over), f"{entry}: bad arguments")
    for over in (dict(mode=-1), dict(mode=3), dict(mode=1, H=5), dict(mode=1, W=7)):
        _rejected(_im_call(entry, **over), f"{entry}: mode 0|1|2 (mode 1 needs even H, W)")
    _rejected(_im_call(entry, Kpad=208), f"{entry}: Kpad=208 must be >= 9*C and a multiple of 8")
    _rejected(_im_call(entry, Kpad=220), f"{entry}: Kpad=220 must be >= 9*C and a multiple of 8")
    # odd sizes pass in modes 0 and 2, and no operand alignment is asked for: the calls get as far as Kpad
    for over in (dict(mode=0, H=5, W=7), dict(mode=2, H=5, W=7), dict(x=A2), dict(out=A2), dict(C=3)):
        _rejected(_im_call(entry, Kpad=220, **over), f"{entry}: Kpad=220 must be >= 9*C and a multiple of 8")
    # order: arguments, mode, Kpad
    _rejected(_im_call(entry, B=0, mode=3, Kpad=220), f"{entry}: bad arguments")
    _rejected(_im_call(entry, mode=3, Kpad=220), f"{entry}: mode 0|1|2 (mode 1 needs even H, W)")


def test_im2col_split_pair_layout():
    e = "lx_im2col3x3_split"

    def pair(ldx, off, C_=24):
        return f"{e}: need x_lo_off % 8 == 0 and C <= x_lo_off, x_lo_off + C <= ldx (C={C_} ldx={ldx} x_lo_off={off})"
    _rejected(_im_call(e, x_lo_off=28, ldx=56), pair(56, 28))        # x_lo_off % 8
    _rejected(_im_call(e, x_lo_off=16), pair(48, 16))                # C <= x_lo_off
    _rejected(_im_call(e, ldx=47), pair(47, 24))                     # x_lo_off + C <= ldx
    _rejected(_im_call(e, C=3, x_lo_off=0, ldx=8), pair(8, 0, 3))
    # after Kpad
    _rejected(_im_call(e, Kpad=220, ldx=47), f"{e}: Kpad=220 must be >= 9*C and a multiple of 8")


# ---- row softmax ---------------------------------------------------------------------------------------------------------------
def _sm_plain(S=A, lds=260, scale=0.125, P=A, ldp=260, M=5, N=260):
    return _lib.lib.lx_softmax_rows(S, lds, scale, P, ldp, M, N, None)


def test_softmax_rows_plain_form():
    text = "lx_softmax_rows: N, lds, ldp must be multiples of 4"
    for over in (dict(S=None), dict(P=None), dict(M=0), dict(N=0), dict(N=258), dict(lds=262), dict(ldp=262)):
        _rejected(_sm_plain(**over), text)


SM_ENTRIES = ("lx_softmax_rows_valid", "lx_softmax_rows_f16", "lx_softmax_rows_split")
SM_DEFAULTS = dict(S=A, lds=320, scale=0.125, P=A, ldp=640, p_lo_off=320, M=5, n_valid=259, n_store=320)


def _sm_call(entry, **over):
    a = dict(SM_DEFAULTS, **over)
    head = (a["S"], a["lds"], a["scale"], a["P"], a["ldp"])
    tail = (a["M"], a["n_valid"], a["n_store"], None)
    if entry == "lx_softmax_rows_split":
        return _lib.lib.lx_softmax_rows_split(*head, a["p_lo_off"], *tail)
    return getattr(_lib.lib, entry)(*head, *tail)


@pytest.mark.parametrize("entry", SM_ENTRIES)
def test_softmax_shared_rules(entry):
    _rejected(_sm_call(entry, S=None), f"{entry}: NULL operand")
    _rejected(_sm_call(entry, P=None), f"{entry}: NULL operand")

    def counts(M, nv, ns):
        return f"{entry}: need M > 0 and 1 <= n_valid <= n_store (M={M} n_valid={nv} n_store={ns})"
    _rejected(_sm_call(entry, M=0), counts(0, 259, 320))
    _rejected(_sm_call(entry, n_valid=0), counts(5, 0, 320))
    _rejected(_sm_call(entry, n_store=258), counts(5, 259, 258))
    # order: operands, counts, leading dimensions
    _rejected(_sm_call(entry, S=None, M=0, lds=8), f"{entry}: NULL operand")
    _rejected(_sm_call(entry, M=0, lds=8), counts(0, 259, 320))


@pytest.mark.parametrize("entry", SM_ENTRIES[:2])
def test_softmax_single_image_leading_dimensions(entry):
    def lds(lds_, ldp):
        return f"{entry}: need lds >= n_valid and ldp >= n_store (lds={lds_} ldp={ldp} n_valid=259 n_store=320)"
    _rejected(_sm_call(entry, lds=258), lds(258, 640))
    _rejected(_sm_call(entry, ldp=319), lds(320, 319))
    # lds = n_valid, odd, and ldp = n_store are accepted: the bf16 form has nothing after this check, so only the fp16 one shows it
    if entry == "lx_softmax_rows_f16":
        _rejected(_sm_call(entry, lds=259, ldp=320, S=A2), f"{entry}: misaligned operand")


def test_softmax_f16_alignment():
    e = "lx_softmax_rows_f16"
    _rejected(_sm_call(e, S=A2), f"{e}: misaligned operand")
    _rejected(_sm_call(e, S=A1), f"{e}: misaligned operand")
    _rejected(_sm_call(e, P=A1), f"{e}: misaligned operand")
    # the alignment line is the last one
    _rejected(_sm_call(e, S=A2, ldp=319), f"{e}: need lds >= n_valid and ldp >= n_store (lds=320 ldp=319 n_valid=259 n_store=320)")


def test_softmax_split_pair_layout():
    e = "lx_softmax_rows_split"

    def pair(lds, ldp, off, nv=259, ns=320):
        return (f"{e}: need lds >= n_valid, p_lo_off % 8 == 0 and n_store <= p_lo_off, p_lo_off + n_store <= ldp "
                f"(lds={lds} ldp={ldp} p_lo_off={off} n_valid={nv} n_store={ns})")
    _rejected(_sm_call(e, lds=258), pair(258, 640, 320))
    _rejected(_sm_call(e, p_lo_off=324, ldp=648), pair(320, 648, 324))         # p_lo_off % 8
    _rejected(_sm_call(e, p_lo_off=312), pair(320, 640, 312))                  # n_store <= p_lo_off
    _rejected(_sm_call(e, ldp=639), pair(320, 639, 320))                       # p_lo_off + n_store <= ldp


# ---- lx_convert_f16 ------------------------------------------------------------------------------------------------------------
def _cv(dst=A, src=A, src_bf16=0, n=0, f16_ovf=None):
    return _lib.lib.lx_convert_f16(dst, src, src_bf16, n, f16_ovf, None)


def test_convert_f16():
    e = "lx_convert_f16"
    _rejected(_cv(dst=None), f"{e}: NULL operand")
    _rejected(_cv(src=None), f"{e}: NULL operand")
    _rejected(_cv(dst=None, src=A1), f"{e}: NULL operand")
    _rejected(_cv(dst=A1), f"{e}: misaligned operand")
    _rejected(_cv(src=A2), f"{e}: misaligned operand")                        # an fp32 source needs 4 bytes
    _rejected(_cv(src=A1, src_bf16=1), f"{e}: misaligned operand")            # a bf16 one 2
    _rejected(_cv(f16_ovf=A2), f"{e}: misaligned operand")
    _rejected(_cv(dst=A1, n=16), f"{e}: misaligned operand")
    # accepted, and nothing to do for n = 0: status LX_OK without a launch
    assert _cv() == 0
    assert _cv(dst=A2, src=A4, f16_ovf=A4) == 0
    assert _cv(dst=A2, src=A2, src_bf16=1) == 0
