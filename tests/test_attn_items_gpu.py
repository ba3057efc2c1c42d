"""Every attention kernel's work-item decode (attn_common.h lx_item_decode: workgroup / persistent item index -> (query tile, batch-head),
head-major per XCD, heads interleaved in groups of G = 2 / 4 / 8 past 12 query tiles per head, a partial last group when B*H % G != 0) and
its segment lookup, checked tile by tile on the device.

Three checks per launch, on the 8-wave kernels (max-tracking; bounded scores without / with a bias), the persistent 4-wave kernel (without /
with a bias) and the e4m3 kernel (log-linear probability bytes, the exponential form, the generic-scale path):
  * per-tile error: every (batch, head, query segment, 256-row query tile) against float64 SDPA on the operands the kernel read (the
    prepped bf16 q / k / v; the dequantised Q8 / K8 / VT8 images), relative L2 over the tile's rows x 128. The MAXIMUM over tiles is bounded,
    so one wrong, duplicated or unwritten tile cannot hide in a segment-wide norm.
  * sentinel coverage: O starts as a NaN pattern. Afterwards every query row is finite, and rows of segments without queries and columns
    outside [o_col, o_col + H*128) still hold the pattern bit for bit.
  * bit equality under another decode: (b, h) relaunched alone (B = H = 1: one partial group, other workgroup indices, no persistent loop)
    reproduces the big launch's rows bit for bit, and writes nothing else.

Measured on MI355X, largest per-tile error of each arm over the whole matrix [bound]: 8-wave max-tracking 2.5e-3, 8-wave bounded 2.5e-3 / with
bias 2.5e-3, 4-wave 2.5e-3 / with bias 2.5e-3 [6e-3]; e4m3 log-linear bytes 3.7e-2, exponential form 3.1e-2, generic scale 2.9e-2 [TOL_FP8 =
7e-2: lower than the 4.5e-2 .. 5.4e-2 of test_fp8_gpu, whose reference does not see the e4m3 rounding of q / k / v]; fp16 O 1.8e-3 (8- and
4-wave), 3.3e-2 (e4m3). The worst tile is usually the 1-row last tile of one_seg: noisier than a full tile, but within the same relative bound,
so no ragged tile needs an absolute form. The module runs in ~10 s of GPU time."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_fp8_gpu import TOL_FP8  # noqa: E402
from tests.test_kernels_gpu import BIASES, DEV, _qkv_buffer, _segments, ops  # noqa: E402,F401

TOL_BF16 = 6e-3
QT = 256                                   # query rows per work item (every attention kernel)
SENT = {torch.bfloat16: 0x7FA5, torch.float16: 0x7E5A}      # NaN bit patterns with a payload no kernel produces
PAD_L, PAD_R = 128, 64                     # O columns left / right of the attention output: must keep the sentinel

# (lens, B, H, qseg_mask): n_qt = sum(ceil(len / 256)) over query segments; G = 1 up to 12, 2 up to 24, 4 up to 48, then 8
CASES = {
    "g1_edge": ((512, 1280, 1280), 1, 3, 0),           # n_qt 12 -> G 1; 36 items, 36 % 8 != 0
    "g2_partial": ((520, 1280, 1280), 1, 3, 0),        # 13 -> 2, BH % G = 1; ragged 8-row query tile and 8-key tile
    "g2_bh6": ((512, 2816, 2816), 2, 3, 0),            # 24 -> 2 (last G = 2)
    "g4_bh6": ((520, 2816, 2816), 2, 3, 0),            # 25 -> 4 (first G = 4), BH % G = 2
    "g8_bh3": ((512, 6144, 6144), 1, 3, 0),            # 50 -> 8, one partial group (BH < G)
    "g8_bh10": ((512, 6144, 6144), 2, 5, 0),           # 50 -> 8, a full group + a partial one
    "one_seg": ((3073,), 1, 3, 0),                     # n_seg 1, 13 -> 2; a 1-row last tile, 3073 % 64 = 1 ragged keys
    **{f"tiny_h{h}": ((40,), 1, h, 0) for h in range(1, 6)},   # fewer items than XCDs
    "engine": ((512, 4096, 4096), 1, 24, 0),           # the 1024^2 forward: 34 -> 4
    "engine_img": ((512, 4096, 4096), 1, 24, 0b010),   # last single block, image queries only: 16 -> 2, segment 0 has no tiles
    "mask_mid_g1": ((520, 1280, 1280), 2, 3, 0b101),   # 8 -> 1, qt_start[1] == qt_start[2]
    "mask_mid_g2": ((520, 2816, 2816), 2, 3, 0b101),   # 14 -> 2
}

# arm -> (family, flags by name, bias, scale, lx_attn_last_kernel); family "raw": q / k as stored, "bnd": RMS-normalised with scale x log2 e
# folded into q (ATTN_Q_LOG2), "fp8": e4m3 images
_BND = ("ATTN_Q_LOG2", "ATTN_BOUNDED")
ARMS = {
    "8w_max": ("raw", (), "cfactor", None, 1),
    "8w_bnd": ("bnd", _BND + ("ATTN_INVARIANT",), "none", None, 1),
    "8w_bnd_bias": ("bnd", _BND + ("ATTN_INVARIANT",), "cfactor", None, 1),
    "4w": ("bnd", _BND + ("ATTN_PREFER_4WAVE",), "none", None, 2),
    "4w_bias": ("bnd", _BND + ("ATTN_PREFER_4WAVE",), "cfactor", None, 2),
    "fp8_loglin": ("fp8", (), "cfactor", None, None),
    "fp8_exp2": ("fp8", ("ATTN_P_EXP2",), "cfactor", None, None),
    "fp8_generic": ("fp8", (), "cfactor", 0.1, None),   # not a power of two: the one-fma-per-score path
}
F16_CASE, F16_ARMS = "g4_bh6", ("8w_bnd_bias", "4w_bias", "fp8_loglin")


def _n_qt(lens, mask):
    return sum((L + QT - 1) // QT for s, L in enumerate(lens) if not mask or (mask >> s) & 1)


def _group(n_qt):
    G = 1
    while n_qt > 12 * G and G < 8:
        G *= 2
    return G


def _sample(BH, n_qt):
    """(b, h) indices relaunched alone: all of them on small launches; else the first, a middle one, the last and the partial group's"""
    if BH <= 6:
        return list(range(BH))
    G = _group(n_qt)
    return sorted({0, BH // 2 - 1, BH - 1} | set(range(BH // G * G, BH)))


# ---- operands (built once per case and family) ---------------------------------------------------------------------------------------
class _Case:
    def __init__(self, ops, name, family):
        lens, B, H, mask = CASES[name]
        self.name, self.lens, self.B, self.H, self.mask, self.family = name, lens, B, H, mask, family
        self.refs = {}                     # (bias, scale) -> float64 reference
        D = H * 128
        self.row0, self.vt0, vt_len = _segments(B, lens)
        self.buf = _qkv_buffer(B, lens, H, seed=31 + len(lens) + H)
        M = self.buf.shape[0]
        if family == "fp8":
            self.Q8 = torch.zeros(M, D, dtype=torch.uint8, device=DEV)
            self.K8 = torch.zeros(M, D, dtype=torch.uint8, device=DEV)
            self.VT = torch.zeros(B, H, 128, vt_len, dtype=torch.uint8, device=DEV)
            ops.qkv_prep_fp8_segs(self.buf, 2 * D, 0, D, [(self.row0[s], lens[s], self.vt0[s], None, None, None, None) for s in range(len(lens))],
                                  B, H, self.Q8, self.K8, self.VT)
        else:
            self.VT = torch.zeros(B, H, 128, vt_len, dtype=torch.bfloat16, device=DEV)
            one = torch.ones(128, device=DEV)
            wq, wk = (one * ops.Q_LOG2_FACTOR, one) if family == "bnd" else (None, None)
            ops.qkv_prep_segs(self.buf, 2 * D, 0, D, [(self.row0[s], lens[s], self.vt0[s], wq, wk, None, None) for s in range(len(lens))],
                              B, H, self.VT)

    def qkv64(self, ops, b):
        """float64 q, k, v of batch b as the kernel reads them: [H, S, 128] over the concatenated segments"""
        D, H = self.H * 128, self.H
        def rows(col, s):
            r = self.row0[s] + b * self.lens[s]
            return self.buf[r: r + self.lens[s], col: col + D].double().view(-1, H, 128)
        if self.family == "fp8":
            def img(t, s, scale):
                r = self.row0[s] + b * self.lens[s]
                return t[r: r + self.lens[s]].view(torch.float8_e4m3fn).float().double().view(-1, H, 128) / scale
            q = torch.cat([img(self.Q8, s, ops.FP8_Q_SCALE) for s in range(len(self.lens))])
            k = torch.cat([img(self.K8, s, ops.FP8_K_SCALE) for s in range(len(self.lens))])
            # VT8: byte j = g*32 + p of a 64-key tile row holds key (p >> 4)*32 + 8*((p & 15) >> 2) + 4*g + (p & 3) (test_fp8_gpu)
            j = torch.arange(64)
            g, p = j >> 5, j & 31
            inv = torch.empty(64, dtype=torch.long)
            inv[(p >> 4) * 32 + 8 * ((p & 15) >> 2) + 4 * g + (p & 3)] = j
            idx = torch.cat([self.vt0[s] + (torch.arange(L) // 64) * 64 + inv[torch.arange(L) % 64] for s, L in enumerate(self.lens)])
            v = self.VT[b][:, :, idx.to(DEV)].view(torch.float8_e4m3fn).float().double().permute(2, 0, 1) / ops.FP8_V_SCALE
        else:
            q = torch.cat([rows(2 * D, s) for s in range(len(self.lens))])
            k = torch.cat([rows(0, s) for s in range(len(self.lens))])
            v = torch.cat([rows(D, s) for s in range(len(self.lens))])
        return q.permute(1, 0, 2), k.permute(1, 0, 2), v.permute(1, 0, 2)


_CACHE = {}


def _case(ops, name, family):
    key = (name, family)
    if key not in _CACHE:
        _CACHE.clear()                     # one case's operands / references at a time
        _CACHE[key] = _Case(ops, name, family)
    return _CACHE[key]


def _reference(ops, c, bias_name, scale):
    """float64 SDPA with the segment bias, per batch: {(b, s): [H, len_s, 128]} for the query segments; score blocks kept under ~1 GB"""
    key = (bias_name, scale)
    if key in c.refs:
        return c.refs[key]
    bias = BIASES[bias_name]
    S = sum(c.lens)
    edges = [0]
    for L in c.lens:
        edges.append(edges[-1] + L)
    # natural-log score factor: q carries scale x log2 e under ATTN_Q_LOG2 (scores in log2 units)
    f = math.log(2.0) if c.family == "bnd" else (scale if scale is not None else 1.0 / math.sqrt(128.0))
    chunk = max(64, (1 << 30) // (8 * c.H * S))
    out = {}
    for b in range(c.B):
        q, k, v = c.qkv64(ops, b)
        kt = k.transpose(1, 2) * f
        for s, L in enumerate(c.lens):
            if c.mask and not (c.mask >> s) & 1:
                continue
            bvec = torch.cat([torch.full((Lk,), float(bias[s][t]), dtype=torch.float64, device=DEV) for t, Lk in enumerate(c.lens)])
            o = torch.empty(c.H, L, 128, dtype=torch.float64, device=DEV)
            for r in range(0, L, chunk):
                sc = torch.matmul(q[:, edges[s] + r: edges[s] + min(L, r + chunk)], kt) + bvec
                o[:, r: r + chunk] = torch.matmul(torch.softmax(sc, -1), v)
            out[(b, s)] = o
    c.refs[key] = out
    return out


# ---- launches --------------------------------------------------------------------------------------------------------------------------
def _sentinel_o(c, dtype):
    O = torch.empty(c.buf.shape[0], PAD_L + c.H * 128 + PAD_R, dtype=dtype, device=DEV)
    O.view(torch.int16).fill_(SENT[dtype])
    return O


def _launch(ops, c, arm, O, ovf, f16, bh=None):
    """the arm's kernel on the whole case, or (bh = (b, h)) on that batch-head alone as B = H = 1"""
    family, fl, bias_name, scale, kernel = ARMS[arm]
    flags = 0
    for n in fl:
        flags |= getattr(ops, n)
    if f16:
        flags |= ops.ATTN_O_F16
    B, H, D = c.B, c.H, c.H * 128
    row0, o_col = c.row0, PAD_L
    Q = K = c.buf
    q_col, k_col, VT = 2 * D, 0, c.VT
    if family == "fp8":
        Q, K, q_col = c.Q8, c.K8, 0
    if bh is not None:
        b, h = bh
        row0 = [c.row0[s] + b * L for s, L in enumerate(c.lens)]
        o_col += h * 128
        VT = c.VT[b: b + 1, h: h + 1]
        if family == "fp8":
            Q, K = c.Q8[:, h * 128: (h + 1) * 128], c.K8[:, h * 128: (h + 1) * 128]
        else:
            q_col, k_col = q_col + h * 128, k_col + h * 128
        B = H = 1
    kw = dict(o_col=o_col, B=B, H=H, seg_row0=row0, seg_len=list(c.lens), seg_vt0=c.vt0, bias=BIASES[bias_name], scale=scale, flags=flags,
              f16_ovf=ovf, qseg_mask=c.mask)
    if family == "fp8":
        ops.attn_fwd_fp8(Q, K, VT, O, **kw)
    else:
        ops.attn_fwd(Q, K, VT, O, q_col=q_col, k_col=k_col, **kw)
        assert ops.lib.lx_attn_last_kernel() == kernel, f"{arm}: the planner moved this launch to kernel {ops.lib.lx_attn_last_kernel()}"


def _q_rows(c, b=None):
    """boolean [M] mask of the query rows (of batch b only, when given)"""
    m = torch.zeros(c.buf.shape[0], dtype=torch.bool, device=DEV)
    for s, L in enumerate(c.lens):
        if c.mask and not (c.mask >> s) & 1:
            continue
        if b is None:
            m[c.row0[s]: c.row0[s] + c.B * L] = True
        else:
            m[c.row0[s] + b * L: c.row0[s] + (b + 1) * L] = True
    return m


def _check(ops, name, arm, f16=False):
    family, _, bias_name, scale, _ = ARMS[arm]
    c = _case(ops, name, family)
    dtype = torch.float16 if f16 else torch.bfloat16
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV) if f16 else None
    O = _sentinel_o(c, dtype)
    _launch(ops, c, arm, O, ovf, f16)
    torch.cuda.synchronize()
    cols = slice(PAD_L, PAD_L + c.H * 128)
    sent = SENT[dtype]

    # 1. coverage: query rows finite, everything else untouched
    qrows = _q_rows(c)
    Oi = O.view(torch.int16)
    assert bool(torch.isfinite(O[qrows][:, cols]).all()), f"{arm}: a query row was not written (or is not finite)"
    assert bool((Oi[~qrows] == sent).all()), f"{arm}: rows of a segment without queries were written"
    assert bool((Oi[:, :PAD_L] == sent).all()) and bool((Oi[:, PAD_L + c.H * 128:] == sent).all()), f"{arm}: columns outside the head block written"
    if f16:
        assert int(ovf.item()) == 0

    # 2. per-tile error against float64
    ref = _reference(ops, c, bias_name, scale)
    tol = TOL_FP8 if family == "fp8" else TOL_BF16
    worst, worst_at, worst_small = 0.0, None, 0.0
    for (b, s), r in ref.items():
        L = c.lens[s]
        o = O[c.row0[s] + b * L: c.row0[s] + (b + 1) * L, cols].double().view(L, c.H, 128).permute(1, 0, 2)
        n_t = (L + QT - 1) // QT
        pad = n_t * QT - L
        d2 = torch.nn.functional.pad(((o - r) ** 2).sum(-1), (0, pad)).view(c.H, n_t, QT).sum(-1)
        r2 = torch.nn.functional.pad((r ** 2).sum(-1), (0, pad)).view(c.H, n_t, QT).sum(-1)
        e = (d2 / r2).sqrt()                                           # [H, n_t]
        m = float(e.max())
        if not m <= worst:                                             # (NaN propagates)
            h, t = divmod(int(e.argmax()), n_t)
            worst, worst_at = m, (b, h, s, t)
        if L % QT:
            worst_small = max(worst_small, float(e[:, -1].max()))
    print(f"ITEMS {name} {arm}{' f16' if f16 else ''}: max tile err {worst:.3e} at (b, h, seg, tile) {worst_at}; ragged last tiles {worst_small:.3e}")
    assert worst < tol, f"{arm}: tile (b, h, seg, tile) = {worst_at}: relative error {worst:.3e} >= {tol}"

    # 3. bit equality: a batch-head launched alone (other decode) reproduces its rows and writes nothing else
    n_qt = _n_qt(c.lens, c.mask)
    for b, h in [divmod(x, c.H) for x in _sample(c.B * c.H, n_qt)]:
        O1 = _sentinel_o(c, dtype)
        _launch(ops, c, arm, O1, ovf, f16, bh=(b, h))
        rows = _q_rows(c, b)
        hc = slice(PAD_L + h * 128, PAD_L + (h + 1) * 128)
        O1i = O1.view(torch.int16)
        assert torch.equal(O1i[rows][:, hc], Oi[rows][:, hc]), f"{arm}: (b, h) = ({b}, {h}) alone differs from the batched launch"
        O1i[rows, hc] = sent
        assert bool((O1i == sent).all()), f"{arm}: (b, h) = ({b}, {h}) alone wrote outside its rows / head"
    if f16:
        assert int(ovf.item()) == 0


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("case", list(CASES))
def test_attention_items_tile_by_tile(ops, case, arm):
    """per-tile float64 error, sentinel coverage and lone-head bit equality for one (shape, kernel arm); measured maxima in the module
    docstring"""
    _check(ops, case, arm)


@pytest.mark.parametrize("arm", F16_ARMS)
def test_attention_items_f16_output(ops, arm):
    """ATTN_O_F16 at the first G = 4 shape on each family: same per-tile bound, overflow counter stays 0, same coverage and bit equality"""
    _check(ops, F16_CASE, arm, f16=True)
