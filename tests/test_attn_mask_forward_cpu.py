"""attention_mask on the public surface, the parts that need no GPU: the text_padding_mask helper and the argument checks that run before
anything touches the device."""
import pytest
import torch

from loongx_amd.flux.pipeline_tools import text_padding_mask


def test_text_padding_mask_shape_dtype_values():
    T, N, C = 12, 8, 4
    m = text_padding_mask([5, 12, 0], T, N, C)
    assert m.shape == (3, 1, 1, T + N + C) and m.dtype == torch.bool and m.device.type == "cpu"
    for b, n in enumerate((5, 12, 0)):
        row = m[b, 0, 0]
        assert row[:n].all() and not row[n:T].any(), b            # text keys t >= lengths[b] are False
        assert row[T:].all(), b                                   # image and condition keys stay True
    # a tensor of lengths, no condition stream
    m2 = text_padding_mask(torch.tensor([3]), 4, 2, 0)
    assert m2.shape == (1, 1, 1, 6) and m2[0, 0, 0].tolist() == [True, True, True, False, True, True]
    assert text_padding_mask([4], 4, 2).all()                     # nothing padded: all True (C defaults to 0)


def test_text_padding_mask_rejects_bad_lengths():
    for bad in ([13], [-1]):
        with pytest.raises(ValueError):
            text_padding_mask(bad, 12, 8, 0)


def test_the_src_alias_exports_the_helper():
    from src.flux import pipeline_tools as alias
    assert alias.text_padding_mask is text_padding_mask


@pytest.mark.parametrize("bad", [torch.ones(7), torch.tensor(True), [[True, False]], "mask", 1.0])
def test_rank1_or_non_tensor_mask_is_rejected_without_a_gpu(bad):
    from loongx_amd.flux.engine import mask_argument
    from loongx_amd.flux.transformer import tranformer_forward
    with pytest.raises(NotImplementedError, match="rank 2..4"):
        mask_argument(bad)
    # the public entry point checks it before it looks at the transformer or any other argument
    with pytest.raises(NotImplementedError, match="rank 2..4"):
        tranformer_forward(None, None, None, None, hidden_states=None, attention_mask=bad)
    with pytest.raises(NotImplementedError, match="rank 2..4"):
        tranformer_forward(None, None, None, None, hidden_states=None, joint_attention_kwargs={"attention_mask": bad})


def test_both_keyword_forms_at_once_is_a_value_error_without_a_gpu():
    from loongx_amd.flux.transformer import tranformer_forward
    m = torch.ones(4, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="twice"):
        tranformer_forward(None, None, None, None, hidden_states=None, attention_mask=m, joint_attention_kwargs={"attention_mask": m})


def test_refused_modes_name_the_mode():
    from loongx_amd.flux.engine import refuse_masked_modes
    refuse_masked_modes({}, False)
    refuse_masked_modes({"precise": False}, True)                 # a call's model_config overrides the default either way
    for mc, default, word in (({"precise": True}, False, "precise"), ({}, True, "precise"), ({"attn_fp8": True}, False, "attn_fp8")):
        with pytest.raises(NotImplementedError, match=word):
            refuse_masked_modes(mc, default)


def test_query_subset_with_shared_rows_is_rejected_on_the_host():
    """a segment without queries must keep its rows of O: lx_attn_fwd_masked refuses a subset whose query rows overlap them (status -1,
    nothing launched); out-of-range n_qseg / qseg_mask are refused as lx_attn_fwd refuses them"""
    import ctypes
    from loongx_amd import _lib as L
    from tests.test_attn_mask_cpu import _descs, _need
    a, m = _descs(L)                                               # (its three segments all start at row 0)
    m.workspace, m.workspace_bytes = 0x100000, _need(L, a, m)
    a.seg_row0[1], a.seg_row0[2] = a.B * 40 - 1, a.B * (40 + 300)   # segment 1 starts on segment 0's last row
    a.qseg_mask = 0b010
    assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and b"overlap" in L.lib.lx_last_error()
    a.qseg_mask = 0
    for field, bad, word in (("n_qseg", 4, b"n_qseg"), ("n_qseg", -1, b"n_qseg"), ("qseg_mask", 0b1000, b"qseg_mask"), ("qseg_mask", -1, b"qseg_mask")):
        setattr(a, field, bad)
        assert L.lib.lx_attn_fwd_masked(ctypes.byref(a), ctypes.byref(m), None) == -1 and word in L.lib.lx_last_error()
        setattr(a, field, 0)
