"""lx_attn_fwd_masked (csrc/attn_mask.hip) and attn_forward(..., attention_mask=...) on the GPU.

Kernel checks, tile by tile: every (batch, head, query segment, 256-row query tile) of the output against float64 SDPA with the same mask on
the bf16 q / k / v the kernel read, relative L2 over the tile's rows x 128; the MAXIMUM over tiles is bounded by the 6e-3 of
test_attn_items_gpu. A tile whose reference is all zeros (every row masked from every key) must be exactly zero. O starts as a NaN pattern;
columns outside [o_col, o_col + H*128) keep it bit for bit. Two launches are bit-identical.

API checks: the tiny transformer's attn_forward with a mask against the CPU oracle whose SDPA receives the same mask (TOL_ATTN of
test_api_gpu), the reference's replacement rules (union_cond_attn = False, independent_condition, c_factor: the mask is ignored) and the
errors (precise / attn_fp8 modes, bad shapes or devices)."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests.test_kernels_gpu import DEV, _qkv_buffer, _segments, ops  # noqa: E402,F401

TOL = 6e-3
QT = 256
SENT = {torch.bfloat16: 0x7FA5, torch.float16: 0x7E5A}
PAD_L, PAD_R = 128, 64

# name -> (lens, B, H)
LAYOUTS = {
    "one": ((333,), 2, 3),
    "two": ((70, 300), 2, 3),
    "three": ((40, 300, 90), 2, 3),
    "engine": ((512, 1024, 1024), 1, 24),
}


class _Lay:
    def __init__(self, ops, name, q_log2):
        self.lens, self.B, self.H = LAYOUTS[name]
        self.S = sum(self.lens)
        D = self.H * 128
        self.row0, self.vt0, vt_len = _segments(self.B, self.lens)
        self.buf = _qkv_buffer(self.B, self.lens, self.H, seed=7 + len(self.lens) + self.H)
        self.VT = torch.zeros(self.B, self.H, 128, vt_len, dtype=torch.bfloat16, device=DEV)
        one = torch.ones(128, device=DEV)
        wq, wk = (one * ops.Q_LOG2_FACTOR, one) if q_log2 else (None, None)
        ops.qkv_prep_segs(self.buf, 2 * D, 0, D, [(self.row0[s], L, self.vt0[s], wq, wk, None, None) for s, L in enumerate(self.lens)],
                          self.B, self.H, self.VT)
        self.qscale = ops.Q_LOG2_FACTOR if q_log2 else 1.0
        self.edges = [0]
        for L in self.lens:
            self.edges.append(self.edges[-1] + L)

    def qkv64(self, b):
        D, H = self.H * 128, self.H
        def cat(col):
            return torch.cat([self.buf[self.row0[s] + b * L: self.row0[s] + (b + 1) * L, col: col + D].double().cpu().view(L, H, 128)
                              for s, L in enumerate(self.lens)]).permute(1, 0, 2)
        return cat(2 * D) / self.qscale, cat(0), cat(D)

    def run(self, ops, mask, *, flags=0, bias=None, o_dtype=torch.bfloat16, f16_ovf=None):
        D = self.H * 128
        M = self.buf.shape[0]
        O = torch.full((M, PAD_L + D + PAD_R), SENT[o_dtype], dtype=torch.int16, device=DEV).view(o_dtype)
        ops.attn_fwd_masked(self.buf, self.buf, self.VT, O, mask, q_col=2 * D, k_col=0, o_col=PAD_L, B=self.B, H=self.H, seg_row0=self.row0,
                            seg_len=list(self.lens), seg_vt0=self.vt0, bias=bias, flags=flags, f16_ovf=f16_ovf)
        torch.cuda.synchronize()
        return O

    def reference(self, b, mask, bias=None):
        """float64 SDPA over the concatenated segments of batch b, with the segment bias table and the mask ([Bm, Hm, Sq, S] or lower rank)"""
        q, k, v = self.qkv64(b)
        add = torch.zeros(self.S, self.S, dtype=torch.float64)
        if bias is not None:
            for i in range(len(self.lens)):
                for j in range(len(self.lens)):
                    add[self.edges[i]:self.edges[i + 1], self.edges[j]:self.edges[j + 1]] = bias[i][j]
        m = mask
        while m.dim() < 4:
            m = m.unsqueeze(0)
        m = m[b if m.shape[0] > 1 else 0].cpu()
        if m.dtype == torch.bool:
            m = torch.zeros(m.shape, dtype=torch.float64).masked_fill(~m, float("-inf"))
        add = add + m.double()                                   # [Hm, Sq, S] + [S, S]
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=add.expand(self.H, self.S, self.S))
        return o.nan_to_num(0.0)                                 # [H, S, 128] (an all -inf row: zeros, as the kernel writes)

    def out_rows(self, O, b):
        D = self.H * 128
        return torch.cat([O[self.row0[s] + b * L: self.row0[s] + (b + 1) * L, PAD_L: PAD_L + D].double().cpu().view(L, self.H, 128)
                          for s, L in enumerate(self.lens)]).permute(1, 0, 2)

    def check(self, O, mask, bias=None, o_dtype=torch.bfloat16):
        """largest per-tile relative error; asserts zero tiles are exact and the sentinel columns are untouched"""
        D = self.H * 128
        raw = O.view(torch.int16)
        assert (raw[:, :PAD_L] == SENT[o_dtype]).all() and (raw[:, PAD_L + D:] == SENT[o_dtype]).all(), "write outside the head columns"
        worst = 0.0
        for b in range(self.B):
            ref, got = self.reference(b, mask, bias), self.out_rows(O, b)
            assert torch.isfinite(got).all()
            for s, L in enumerate(self.lens):
                for t0 in range(0, L, QT):
                    r = ref[:, self.edges[s] + t0: self.edges[s] + min(L, t0 + QT)]
                    g = got[:, self.edges[s] + t0: self.edges[s] + min(L, t0 + QT)]
                    for h in range(self.H):
                        n = float(r[h].norm())
                        if n == 0.0:
                            assert (g[h] == 0).all(), f"fully masked tile b={b} h={h} seg={s} row {t0} not zero"
                        else:
                            worst = max(worst, float((g[h] - r[h]).norm()) / n)
        return worst


_LAY = {}


def _lay(ops, name, q_log2=False):
    key = (name, q_log2)
    if key not in _LAY:
        _LAY[key] = _Lay(ops, name, q_log2)
    return _LAY[key]


# ---- masks ----------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dense_bool(lay, shape, seed):
    g = _gen(seed)
    m = torch.rand(*shape, generator=g) < 0.6
    m[..., 3, :] = False                                          # whole rows masked: exact zeros
    m[..., lay.S - 1, :] = False
    return m.to(DEV)


def _block_bool(lay, seed):
    """[S, S] with a class per (segment-local 256-row query tile, 64-key tile): EMPTY, FULL or PARTIAL; the second query tile of the
    longest segment is EMPTY everywhere"""
    g = _gen(seed)
    m = torch.zeros(lay.S, lay.S, dtype=torch.bool)
    for sq, Lq in enumerate(lay.lens):
        for q0 in range(0, Lq, QT):
            for sk, Lk in enumerate(lay.lens):
                for k0 in range(0, Lk, 64):
                    rq = slice(lay.edges[sq] + q0, lay.edges[sq] + min(Lq, q0 + QT))
                    rk = slice(lay.edges[sk] + k0, lay.edges[sk] + min(Lk, k0 + 64))
                    c = int(torch.randint(0, 3, (1,), generator=g))
                    if c == 1:
                        m[rq, rk] = True
                    elif c == 2:
                        m[rq, rk] = torch.rand(rq.stop - rq.start, rk.stop - rk.start, generator=g) < 0.5
    s = max(range(len(lay.lens)), key=lambda i: lay.lens[i])
    if lay.lens[s] > QT:
        m[lay.edges[s] + QT: lay.edges[s] + min(lay.lens[s], 2 * QT)] = False
    return m.to(DEV)


def _keypad(lay, seed):
    g = _gen(seed)
    m = torch.ones(lay.B, 1, 1, lay.S, dtype=torch.bool)
    for b in range(lay.B):
        keep = torch.rand(lay.S, generator=g) < 0.75
        keep[0] = True
        m[b, 0, 0] &= keep
    return m.to(DEV)


def _additive(lay, shape, dtype, seed):
    g = _gen(seed)
    m = torch.randn(*shape, generator=g) * 2.0
    u = torch.rand(*shape, generator=g)
    m[u < 0.15] = float("-inf")
    m[(u >= 0.15) & (u < 0.2)] = -1e4
    m[..., 5, :] = float("-inf")
    return m.to(dtype).to(DEV)


def _mask(lay, kind, seed=0):
    B, H, S = lay.B, lay.H, lay.S
    if kind == "dense_bool_SS":
        return _dense_bool(lay, (S, S), seed)
    if kind == "dense_bool_B1SS":
        return _dense_bool(lay, (B, 1, S, S), seed)
    if kind == "dense_bool_1HSS":
        return _dense_bool(lay, (1, H, S, S), seed)
    if kind == "dense_bool_BHSS":
        return _dense_bool(lay, (B, H, S, S), seed)
    if kind == "dense_bool_noncontig":                             # a column slice of a wider tensor, then transposed: strides (1, S + 5)
        return _dense_bool(lay, (S + 5, S), seed)[:S].t()
    if kind == "block_bool":
        return _block_bool(lay, seed)
    if kind == "keypad":
        return _keypad(lay, seed)
    if kind == "f32_1HSS":
        return _additive(lay, (1, H, S, S), torch.float32, seed)
    if kind == "f32_noncontig":
        return _additive(lay, (B, S, S + 3), torch.float32, seed)[:, :, :S].unsqueeze(1)
    if kind == "bf16_B1SS":
        return _additive(lay, (B, 1, S, S), torch.bfloat16, seed)
    if kind == "f16_SS":
        return _additive(lay, (S, S), torch.float16, seed)
    raise KeyError(kind)


KINDS = ["dense_bool_SS", "dense_bool_B1SS", "dense_bool_1HSS", "dense_bool_BHSS", "dense_bool_noncontig", "block_bool", "keypad",
         "f32_1HSS", "f32_noncontig", "bf16_B1SS", "f16_SS"]


@pytest.mark.parametrize("layout", ["one", "two", "three"])
@pytest.mark.parametrize("kind", KINDS)
def test_masked_kernel_tiles(ops, layout, kind):
    lay = _lay(ops, layout)
    mask = _mask(lay, kind, seed=zlib.crc32(f"{layout}/{kind}".encode()) % 1000)
    O = lay.run(ops, mask)
    assert lay.check(O, mask) <= TOL
    O2 = lay.run(ops, mask)
    assert torch.equal(O.view(torch.int16), O2.view(torch.int16)), "two launches differ"


@pytest.mark.parametrize("kind", ["block_bool", "keypad", "f32_1HSS"])
def test_masked_kernel_q_log2_and_segment_bias(ops, kind):
    lay = _lay(ops, "three", q_log2=True)
    mask = _mask(lay, kind, seed=11)
    cf = math.log(0.5)
    bias = [[0, 0, cf], [0, 0, cf], [cf, cf, 0]]
    assert lay.check(lay.run(ops, mask, flags=ops.ATTN_Q_LOG2, bias=bias), mask, bias) <= TOL
    nu = [[0, 0, float("-inf")], [0, 0, float("-inf")], [float("-inf"), float("-inf"), 0]]   # a -inf pair: its tiles are EMPTY
    assert lay.check(lay.run(ops, mask, flags=ops.ATTN_Q_LOG2, bias=nu), mask, nu) <= TOL


def test_masked_kernel_f16_output(ops):
    lay = _lay(ops, "two")
    mask = _mask(lay, "block_bool", seed=5)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    O = lay.run(ops, mask, flags=ops.ATTN_O_F16, o_dtype=torch.float16, f16_ovf=ovf)
    assert lay.check(O, mask, o_dtype=torch.float16) <= TOL and int(ovf.item()) == 0


@pytest.mark.parametrize("kind", ["block_bool", "dense_bool_SS", "keypad", "f32_1HSS"])
def test_masked_kernel_engine_layout(ops, kind):
    lay = _lay(ops, "engine", q_log2=True)
    mask = _mask(lay, kind, seed=3)
    assert lay.check(lay.run(ops, mask, flags=ops.ATTN_Q_LOG2), mask) <= TOL


@pytest.mark.parametrize("layout", ["three", "engine"])
def test_all_true_mask_matches_unmasked_kernel(ops, layout):
    """an all-True mask (every tile FULL) computes the lx_attn_fwd contract: both against the reference, and against each other"""
    lay = _lay(ops, layout)
    mask = torch.ones(lay.S, lay.S, dtype=torch.bool, device=DEV)
    O = lay.run(ops, mask)
    assert lay.check(O, mask) <= TOL
    D = lay.H * 128
    U = torch.full_like(O.view(torch.int16), SENT[torch.bfloat16]).view(torch.bfloat16)
    ops.attn_fwd(lay.buf, lay.buf, lay.VT, U, q_col=2 * D, k_col=0, o_col=PAD_L, B=lay.B, H=lay.H, seg_row0=lay.row0, seg_len=list(lay.lens),
                 seg_vt0=lay.vt0, flags=ops.ATTN_INVARIANT)
    torch.cuda.synchronize()
    assert lay.check(U, mask) <= TOL
    for b in range(lay.B):
        a, u = lay.out_rows(O, b), lay.out_rows(U, b)
        assert float((a - u).norm() / u.norm()) <= TOL


def test_prep_once_attend_twice(ops):
    """ops.attn_mask_prep + attn_fwd_masked(prepped=True) on the same workspace equals the one-call form bit for bit"""
    lay = _lay(ops, "three")
    mask = _mask(lay, "block_bool", seed=9)
    D = lay.H * 128
    ws = ops.attn_mask_workspace(mask, B=lay.B, H=lay.H, seg_len=list(lay.lens), seg_vt0=lay.vt0)
    ops.attn_mask_prep(mask, ws, B=lay.B, H=lay.H, seg_len=list(lay.lens), seg_vt0=lay.vt0)
    O = torch.full((lay.buf.shape[0], PAD_L + D + PAD_R), SENT[torch.bfloat16], dtype=torch.int16, device=DEV).view(torch.bfloat16)
    ops.attn_fwd_masked(lay.buf, lay.buf, lay.VT, O, mask, q_col=2 * D, k_col=0, o_col=PAD_L, B=lay.B, H=lay.H, seg_row0=lay.row0,
                        seg_len=list(lay.lens), seg_vt0=lay.vt0, workspace=ws, prepped=True)
    torch.cuda.synchronize()
    assert torch.equal(O.view(torch.int16), lay.run(ops, mask).view(torch.int16))


# ---- attn_forward(..., attention_mask=...) ---------------------------------------------------------------------------------------------------
TOL_ATTN = 1.2e-2     # test_api_gpu's bound for the attn_forward mirrors


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import FluxConfig
    from tests.helpers import load, tiny_transformer
    G = load("flux_tiny.npz")
    tr = tiny_transformer()
    cfg = FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2, in_channels=64, joint_attention_dim=64,
                     pooled_projection_dim=32, guidance_embeds=True)
    lx = LxFluxTransformer.from_state_dict(tr.state_dict(), cfg, "cuda")
    main = tr.pos_embed(torch.cat([G["in_txt_ids"], G["in_img_ids"]], 0))
    cond = tr.pos_embed(G["in_cond_ids"])
    return G, tr, lx, main, cond


class _MaskedF:
    """torch.nn.functional for the oracle, whose SDPA receives `mask` wherever the oracle itself passes none"""
    def __init__(self, mask):
        self.mask = mask

    def __getattr__(self, name):
        return getattr(F, name)

    def scaled_dot_product_attention(self, q, k, v, attn_mask=None, **kw):
        return F.scaled_dot_product_attention(q, k, v, attn_mask=self.mask if attn_mask is None else attn_mask, **kw)


def _api_mask(kind, B, H, S):
    g = _gen(21)
    if kind == "bool_B1SS":
        m = torch.rand(B, 1, S, S, generator=g) < 0.7
        m[:, :, 2] = False
        return m
    if kind == "keypad":
        m = torch.ones(B, 1, 1, S, dtype=torch.bool)
        m[1, 0, 0, S // 3: S // 2] = False
        return m
    m = torch.randn(1, H, S, S, generator=g)                      # additive fp32 [1, H, S, S]
    m[torch.rand(1, H, S, S, generator=g) < 0.2] = float("-inf")
    return m


@pytest.mark.parametrize("kind", ["bool_B1SS", "keypad", "f32_1HSS"])
@pytest.mark.parametrize("with_cond", [True, False])
def test_attn_forward_with_mask(api, monkeypatch, kind, with_cond):
    from loongx_amd.flux.block import attn_forward
    from oracle import flux_ref as fr
    from tests.helpers import relerr
    G, tr, lx, main, crope = api
    hid, enc, cond = G["hid"], G["enc"], G["cond"] if with_cond else None
    B, T, N, C = hid.shape[0], enc.shape[1], hid.shape[1], (cond.shape[1] if with_cond else 0)
    S = T + N + C
    mask = _api_mask(kind, B, 2, S)
    cr = crope if with_cond else None
    d, s = lx.transformer_blocks[0].attn, lx.single_transformer_blocks[0].attn
    s.text_len = T
    cu = (lambda t: None if t is None else t.cuda())
    got_d = attn_forward(d, cu(hid), cu(enc), cu(cond), mask.cuda(), main, cr, {})
    got_s = attn_forward(s, cu(torch.cat([enc, hid], 1)), None, cu(cond), mask.cuda(), main, cr, {})
    monkeypatch.setattr(fr, "F", _MaskedF(mask))
    with torch.no_grad():
        want_d = fr.attn_forward(tr.transformer_blocks[0].attn, hid, enc, cond, None, main, cr, {})
        want_s = fr.attn_forward(tr.single_transformer_blocks[0].attn, torch.cat([enc, hid], 1), None, cond, None, main, cr, {})
    want_s = want_s if isinstance(want_s, tuple) else (want_s,)
    got_s = got_s if isinstance(got_s, tuple) else (got_s,)
    assert len(got_d) == len(want_d) and len(got_s) == len(want_s)
    for g_, w_ in list(zip(got_d, want_d)) + list(zip(got_s, want_s)):
        assert relerr(g_.float().cpu(), w_.float()) < TOL_ATTN
    # the mask made a difference (the no-mask call is not within the bound of the masked oracle)
    plain = attn_forward(d, cu(hid), cu(enc), cu(cond), None, main, cr, {})
    assert relerr(plain[0].float().cpu(), want_d[0].float()) > TOL_ATTN


@pytest.mark.parametrize("rule", ["no_union", "independent", "cfactor"])
def test_reference_rules_replace_the_mask(api, rule):
    from loongx_amd.flux.block import attn_forward
    G, tr, lx, main, crope = api
    hid, enc, cond = (G[k].cuda() for k in ("hid", "enc", "cond"))
    S = enc.shape[1] + hid.shape[1] + cond.shape[1]
    mask = (torch.rand(S, S, generator=_gen(4)) < 0.5).cuda()
    mc = {"no_union": {"union_cond_attn": False}, "independent": {"independent_condition": True}, "cfactor": {}}[rule]
    d, s = lx.transformer_blocks[0].attn, lx.single_transformer_blocks[0].attn
    s.text_len = enc.shape[1]
    try:
        if rule == "cfactor":
            d.c_factor = s.c_factor = torch.ones(1, 1) * 0.5
        for a, args in ((d, (hid, enc, cond)), (s, (torch.cat([enc, hid], 1), None, cond))):
            with_mask = attn_forward(a, *args, mask, main, crope, mc)
            without = attn_forward(a, *args, None, main, crope, mc)
            for x, y in zip(with_mask, without):
                assert torch.equal(x, y)
    finally:
        for a in (d, s):
            if hasattr(a, "c_factor"):
                del a.c_factor


def test_attn_forward_mask_errors(api):
    from loongx_amd.flux.block import attn_forward
    G, tr, lx, main, crope = api
    hid, enc, cond = (G[k].cuda() for k in ("hid", "enc", "cond"))
    S = enc.shape[1] + hid.shape[1] + cond.shape[1]
    d = lx.transformer_blocks[0].attn
    ok = torch.ones(S, S, dtype=torch.bool, device="cuda")
    for mc, word in (({"precise": True}, "precise"), ({"attn_fp8": True}, "attn_fp8")):
        with pytest.raises(NotImplementedError, match=word):
            attn_forward(d, hid, enc, cond, ok, main, crope, mc)
    for bad in (torch.ones(S, S + 1, dtype=torch.bool, device="cuda"), torch.ones(3, 1, S, S, dtype=torch.bool, device="cuda"),
                torch.ones(1, 5, S, S, dtype=torch.bool, device="cuda"), torch.ones(S, S, dtype=torch.bool),
                torch.ones(S, S, dtype=torch.int32, device="cuda"), torch.ones(1, 1, 1, S, S, dtype=torch.bool, device="cuda")):
        with pytest.raises(ValueError):
            attn_forward(d, hid, enc, cond, bad, main, crope, {})
    with pytest.raises(NotImplementedError):
        attn_forward(d, hid, enc, cond, torch.ones(S, device="cuda"), main, crope, {})
    # the engine keeps no mask after a call, also after a failed one
    assert lx.transformer_blocks[0].attn.engine.attn_mask is None
