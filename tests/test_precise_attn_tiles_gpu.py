"""The two precise-mode attention kernels of loongx_amd/csrc/precise.hip, tile by tile against float64: attn_split_kernel<BOUNDED>
(lx_attn_fwd_split: hi.hi + hi.lo + lo.hi on the bf16 MFMA, 256-row query tiles, 64-key tiles, work item = blockIdx.x % (B*H) /
blockIdx.x / (B*H) + the qq_start segment lookup) and attn_f32_kernel (lx_attn_fwd_f32: fp32 MFMA, 128-row query tiles, 32-key tiles).
Modelled on tests/test_attn_items_gpu.py.

The reference is float64 joint attention (tests/helpers.py seg_attn_ref, pinned on the CPU by tests/test_precise_attn_ref_cpu.py) on the
operands the kernel READ: hi + lo of the q, k and V^T images that lx_qkv_prep_split_segs wrote (V^T de-interleaved) for the split kernel,
the fp32 rows for the f32 kernel. The input rounding of the pairs is therefore not part of the error. Compared: O_hi + O_lo in float64; in
the hi-only arms O_hi against the bf16 rounding of the reference.

Four checks per launch:
  * per-tile error: relative L2 over every (batch, head, query segment, query tile)'s rows x 128; the MAXIMUM over tiles is bounded.
  * sentinel coverage: O starts as the NaN pattern 0x7FA5 with slack columns left of the hi block, between hi and lo and right of lo. Every
    query row's hi (and, with o_lo_off != 0, lo) columns come out finite; every other element keeps the pattern bit for bit (slack, rows of
    segments without queries, the lo block when o_lo_off = 0).
  * a genuine pair: hi is a bf16 nearest to hi + lo and lo == bf16((hi + lo) - hi). (Not literally hi == bf16(hi + lo): when the fp32
    result x lies within 2^-17 |x| of the midpoint of two bf16 values, lo = bf16(x - hi) rounds to exactly half an ulp of hi, hi + lo IS
    the midpoint, and round-to-nearest-even of it picks hi's neighbour half of the time -- about one element in 2^10, for a correct
    kernel. The check therefore accepts an exact tie and nothing else; the number of ties is printed.)
  * bit equality under another decode: every (b, h) relaunched alone as B = H = 1 (row offsets b * len, column offset h * 128, a contiguous
    copy of VT2[:, b, h]) reproduces the big launch's rows bit for bit and writes nothing else; the same launch twice gives the same bits.

Score extremes on (70, 200): a 6x aligned key in the first key tile / at a tile's last key / in the ragged last tile / in the second
segment (the spiked row's own error is asserted); q x 50 (scores of hundreds of log2 units, a nearly one-hot softmax); and, for the
bounded form, rows at +-90 log2 units against the contract's 100 (checked on the host, on the images, before the launch), compared with
float64 and with the max-tracking launch on the same images.

Measured on MI355X, worst tile of each arm over its cases [asserted bound]:
  split  max 6.4e-6 [1.3e-5], max_scale 6.8e-6 [1.4e-5], qlog2 6.0e-6 [1.2e-5], bnd 6.4e-6 [1.3e-5], bnd_bias 6.4e-6 [1.3e-5],
         nounion 6.5e-6 [1.3e-5], nounion_bnd 6.4e-6 [1.3e-5], o_col 6.4e-6 [1.3e-5], hi_only 6.5e-4 [1.3e-3]
  f32    none 2.8e-6 [5.6e-6], cfactor 2.9e-6 [5.8e-6], nounion 3.0e-6 [6.0e-6], scale 2.9e-6 [5.9e-6], o_col 2.9e-6 [5.8e-6],
         hi_only 5.5e-4 [1.1e-3]
  large scores: split 2.2e-5 [3e-5, the starting bound], f32 4.1e-6 [8.3e-6]; spikes: tiles 5.0e-6 / 2.6e-6, the spiked row 5.9e-9 / 3.1e-6
(the existing per-segment bounds against the fp32 inputs are 3e-5 / 2e-5: most of the f32 kernel's 2.8e-6 is the output pair's own
rounding). The worst tiles are ragged ones -- the 1-row last tile of 769, the 1-row tile of 513, the 1-row segment of (1, 63, 65) for the
hi-only arm (128 elements against the bf16 rounding of the reference) -- and stay within the arm's relative bound: no ragged tile has a
bound of its own. The one-key case (1,) is exact (0) on the max-tracking split arms: p = 1 and v's pair passes through.
The module runs in ~4 s of GPU time."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import (NEAR_BOUND_LENS, NEAR_BOUND_PAIRS, max_abs_score_log2, near_bound_qkv, seg_attn_ref, seg_edges,  # noqa: E402
                           vt_deinterleave)
from tests.test_kernels_gpu import BIASES, DEV, _segments, ops  # noqa: E402,F401

SENT = 0x7FA5                              # a NaN bit pattern with a payload no kernel produces
PAD_L, MID, PAD_R = 128, 64, 64            # O columns left of hi, between hi and lo, right of lo: must keep the sentinel
QT = {"split": 256, "f32": 128}            # query rows per work item
START = {"split": 3e-5, "f32": 2e-5}       # the bounds tests/test_precise_gpu.py asserts per segment: never exceeded here
TOL_HI = 4e-3                              # the hi image alone is the bf16 result (tests/test_precise_gpu.py)

# (lens, B, H, qseg_mask); B * H = 6 is neither a power of two nor symmetric in b and h
CASES = {
    "split": {
        "1_63_65": ((1, 63, 65), 2, 3, 0),               # a one-key / one-query segment, 63 = tile - 1, 65 = tile + 1 keys
        "64_256_257": ((64, 256, 257), 2, 3, 0),         # whole key tile, whole query tile, a 1-row second query tile
        "255_513_128": ((255, 513, 128), 2, 3, 0),       # query tile - 1, two query tiles + 1 row and eight key tiles + 1 key
        "769": ((769,), 2, 3, 0),                        # four query tiles with a 1-row last tile and one ragged key
        "1": ((1,), 1, 1, 0),                            # one item, one key
        "mask101": ((300, 520, 260), 2, 3, 0b101),       # qq_start[1] == qq_start[2]
        "mask010": ((300, 520, 260), 2, 3, 0b010),       # segment 0 has no tiles
    },
    "f32": {
        "1_31_33": ((1, 31, 33), 2, 3, 0),
        "32_128_129": ((32, 128, 129), 2, 3, 0),
        "127_257_64": ((127, 257, 64), 2, 3, 0),
        "385": ((385,), 2, 3, 0),
        "1": ((1,), 1, 1, 0),
    },
}
_BND = ("ATTN_Q_LOG2", "ATTN_BOUNDED")
# arm -> (family, flags by name, bias, scale, hi only, o_col = 128); family "raw": q as stored, the kernel applies scale; "log2": scale x log2 e
# folded into q in fp32 before the split (LX_ATTN_Q_LOG2)
ARMS = {
    "split": {
        "max": ("raw", (), "cfactor", None, False, False),
        "max_scale": ("raw", (), "cfactor", 0.1, False, False),
        "qlog2": ("log2", ("ATTN_Q_LOG2",), "cfactor", None, False, False),           # the c2 = 1 max-tracking path
        "bnd": ("log2", _BND, "none", None, False, False),
        "bnd_bias": ("log2", _BND, "cfactor", None, False, False),
        "nounion": ("raw", (), "no_union", None, False, False),
        "nounion_bnd": ("log2", _BND, "no_union", None, False, False),
        "hi_only": ("raw", (), "cfactor", None, True, False),
        "o_col": ("raw", (), "cfactor", None, False, True),
    },
    "f32": {
        "none": ("raw", (), "none", None, False, False),
        "cfactor": ("raw", (), "cfactor", None, False, False),
        "nounion": ("raw", (), "no_union", None, False, False),
        "scale": ("raw", (), "cfactor", 0.1, False, False),
        "hi_only": ("raw", (), "cfactor", None, True, False),
        "o_col": ("raw", (), "cfactor", None, False, True),
    },
}
# the worst tile of every arm over its cases, measured on MI355X, and the asserted bound: 2 x that, never above START / TOL_HI
MEASURED = {
    "split": {"max": 6.434e-6, "max_scale": 6.773e-6, "qlog2": 5.990e-6, "bnd": 6.364e-6, "bnd_bias": 6.364e-6, "nounion": 6.462e-6,
              "nounion_bnd": 6.406e-6, "hi_only": 6.521e-4, "o_col": 6.434e-6},
    "f32": {"none": 2.802e-6, "cfactor": 2.900e-6, "nounion": 2.993e-6, "scale": 2.934e-6, "hi_only": 5.534e-4, "o_col": 2.900e-6},
}
TOL = {k: {a: min(2 * m, TOL_HI if a == "hi_only" else START[k]) for a, m in MEASURED[k].items()} for k in MEASURED}


# ---- operands (one case at a time) -----------------------------------------------------------------------------------------------------
class _Case:
    """fp32 [k | v | q] rows and, for the split kernel, the pair images lx_qkv_prep_split_segs makes of them (norm weights None: q, k pass
    through). family "log2": ops.Q_LOG2_FACTOR folded into q in fp32 first (`folded`: the given buf already carries it)."""

    def __init__(self, ops, kernel, lens, B, H, mask, family, buf=None, folded=False, seed=7):
        self.kernel, self.lens, self.B, self.H, self.mask, self.family = kernel, tuple(lens), B, H, mask, family
        self.refs = {}
        D = H * 128
        self.row0, self.vt0, vt_len = _segments(B, lens)
        if buf is None:
            g = torch.Generator().manual_seed(seed + len(lens) + sum(lens))
            buf = torch.randn(B * sum(lens), 3 * D, generator=g)
        self.buf = buf.to(DEV).clone()
        if family == "log2" and not folded:
            self.buf[:, 2 * D:] *= ops.Q_LOG2_FACTOR
        if kernel == "split":
            self.QK2 = torch.zeros(self.buf.shape[0], 4 * D, dtype=torch.bfloat16, device=DEV)      # [k_hi | k_lo | q_hi | q_lo]
            self.VT2 = torch.zeros(2, B, H, 128, vt_len, dtype=torch.bfloat16, device=DEV)
            segs = [(self.row0[s], L, self.vt0[s], None, None, None, None) for s, L in enumerate(lens)]
            ops.qkv_prep_split_segs(self.buf, 2 * D, 0, D, segs, B, H, self.QK2, q2_col=2 * D, k2_col=0, lo_off=D, VT2=self.VT2)

    def qkv64(self, b):
        """float64 q, k, v of batch b as the kernel reads them: [H, S, 128] over the concatenated segments"""
        D, H = self.H * 128, self.H

        def rows(t, col):
            parts = [t[self.row0[s] + b * L: self.row0[s] + (b + 1) * L, col: col + D].double() for s, L in enumerate(self.lens)]
            return torch.cat(parts).view(-1, H, 128).permute(1, 0, 2)
        if self.kernel == "f32":
            return rows(self.buf, 2 * D), rows(self.buf, 0), rows(self.buf, D)
        q = rows(self.QK2, 2 * D) + rows(self.QK2, 3 * D)
        k = rows(self.QK2, 0) + rows(self.QK2, D)
        v = vt_deinterleave(self.VT2[0, b].double() + self.VT2[1, b].double(), self.lens, self.vt0)
        return q, k, v

    def reference(self, bias_name, scale):
        """{(b, s): [H, len_s, 128]} for the query segments"""
        key = (bias_name, scale)
        if key not in self.refs:
            # natural-log score factor: q carries scale x log2 e under LX_ATTN_Q_LOG2 (scores in log2 units)
            f = math.log(2.0) if self.family == "log2" else (scale if scale is not None else 1.0 / math.sqrt(128.0))
            e = seg_edges(self.lens)
            out = {}
            for b in range(self.B):
                o = seg_attn_ref(*self.qkv64(b), self.lens, BIASES[bias_name], f)
                for s in range(len(self.lens)):
                    if not self.mask or (self.mask >> s) & 1:
                        out[(b, s)] = o[:, e[s]: e[s + 1]]
            self.refs[key] = out
        return self.refs[key]

    def q_rows(self, b=None):
        """boolean [M] mask of the query rows (of batch b only, when given)"""
        m = torch.zeros(self.buf.shape[0], dtype=torch.bool, device=DEV)
        for s, L in enumerate(self.lens):
            if self.mask and not (self.mask >> s) & 1:
                continue
            lo, hi = (0, self.B) if b is None else (b, b + 1)
            m[self.row0[s] + lo * L: self.row0[s] + hi * L] = True
        return m


_CACHE = {}


def _case(ops, kernel, name, family):
    key = (kernel, name, family)
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = _Case(ops, kernel, *CASES[kernel][name], family)
    return _CACHE[key]


# ---- launches --------------------------------------------------------------------------------------------------------------------------
def _sentinel_o(c):
    O = torch.empty(c.buf.shape[0], PAD_L + 2 * c.H * 128 + MID + PAD_R, dtype=torch.bfloat16, device=DEV)
    O.view(torch.int16).fill_(SENT)
    return O


def _launch(ops, c, arm, O, bh=None):
    """the arm's launch on the whole case, or (bh = (b, h)) on that batch-head alone as B = H = 1. The hi block is O[:, PAD_L: PAD_L + D]
    either way: o_col = 0 on a view that starts there, or (the o_col arms) o_col = PAD_L on the whole buffer."""
    _, fl, bias_name, scale, hi_only, with_o_col = ARMS[c.kernel][arm]
    flags = 0
    for n in fl:
        flags |= getattr(ops, n)
    B, H, D = c.B, c.H, c.H * 128
    row0, head = c.row0, 0
    o_col, Ov = (PAD_L, O) if with_o_col else (0, O[:, PAD_L:])
    if bh is not None:
        b, h = bh
        row0 = [c.row0[s] + b * L for s, L in enumerate(c.lens)]
        head, B, H = h * 128, 1, 1
    common = dict(o_col=o_col + head, o_lo_off=0 if hi_only else D + MID, B=B, H=H, seg_row0=row0, seg_len=list(c.lens),
                  bias=BIASES[bias_name], scale=scale)
    if c.kernel == "f32":
        ops.attn_fwd_f32(c.buf, Ov, q_col=2 * D + head, k_col=head, v_col=D + head, **common)
    else:
        VT = c.VT2 if bh is None else c.VT2[:, bh[0]: bh[0] + 1, bh[1]: bh[1] + 1].contiguous()      # [2, 1, 1, 128, Spad]
        ops.attn_fwd_split(c.QK2, VT, Ov, q_col=2 * D + head, k_col=head, qk_lo_off=D, seg_vt0=c.vt0, flags=flags, qseg_mask=c.mask, **common)


def _tile_errors(c, got, ref, tag, rows=()):
    """max over (b, h, query segment, tile) of the relative L2 error over the tile's rows x 128; got: float64 [M, D] (the hi block, or
    hi + lo). Returns (worst over all tiles, worst over the ragged last tiles, [relative error of each (b, seg, pos, h) in rows])"""
    qt = QT[c.kernel]
    worst, worst_at, worst_small = 0.0, None, 0.0
    for (b, s), r in ref.items():
        L = c.lens[s]
        o = got[c.row0[s] + b * L: c.row0[s] + (b + 1) * L].view(L, c.H, 128).permute(1, 0, 2)
        n_t = (L + qt - 1) // qt
        pad = n_t * qt - L
        d2 = torch.nn.functional.pad(((o - r) ** 2).sum(-1), (0, pad)).view(c.H, n_t, qt).sum(-1)
        r2 = torch.nn.functional.pad((r ** 2).sum(-1), (0, pad)).view(c.H, n_t, qt).sum(-1)
        e = (d2 / r2).sqrt()                                           # [H, n_t]
        m = float(e.max())
        if not m <= worst:                                             # (NaN propagates)
            h, t = divmod(int(e.argmax()), n_t)
            worst, worst_at = m, (b, h, s, t)
        if L % qt:
            worst_small = max(worst_small, float(e[:, -1].max()))
    row_err = []
    for (b, s, pos, h) in rows:
        o = got[c.row0[s] + b * c.lens[s] + pos].view(c.H, 128)[h]
        r = ref[(b, s)][h, pos]
        row_err.append(float((o - r).norm() / r.norm()))
    print(f"PRECISE_TILES {tag}: max tile err {worst:.3e} at (b, h, seg, tile) {worst_at}; ragged last tiles {worst_small:.3e}; rows {row_err}")
    return worst, worst_small, row_err


def _check(ops, c, arm, tag, tol, rows=(), relaunch=True):
    _, _, bias_name, scale, hi_only, _ = ARMS[c.kernel][arm]
    D = c.H * 128
    O = _sentinel_o(c)
    _launch(ops, c, arm, O)
    again = _sentinel_o(c)
    _launch(ops, c, arm, again)
    torch.cuda.synchronize()
    Oi = O.view(torch.int16)
    assert torch.equal(Oi, again.view(torch.int16)), f"{tag}: the same launch twice gives different bits"
    hc, lc = slice(PAD_L, PAD_L + D), slice(PAD_L + D + MID, PAD_L + 2 * D + MID)

    # 1. coverage: query rows' hi (and lo) columns finite, everything else untouched
    qrows = c.q_rows()
    written = torch.zeros_like(Oi, dtype=torch.bool)
    written[qrows, hc] = True
    if not hi_only:
        written[qrows, lc] = True
    assert bool(torch.isfinite(O[written]).all()), f"{tag}: a query row was not written (or is not finite)"
    assert bool((Oi[~written] == SENT).all()), f"{tag}: written outside the query rows' hi / lo columns"

    # 2. a genuine pair
    hi = O[:, hc].double().contiguous()
    got = hi
    if not hi_only:
        lo = O[:, lc].double()
        y = torch.where(qrows[:, None], hi + lo, torch.zeros_like(hi))
        hi_q = torch.where(qrows[:, None], hi, torch.zeros_like(hi))
        r = y.float().to(torch.bfloat16).double()                      # (y has at most 24 significant bits: exact in fp32)
        tie = (r != hi_q) & ((y - r).abs() == (y - hi_q).abs())
        print(f"PRECISE_TILES {tag}: {int(tie.sum())} of {int(qrows.sum()) * D} elements sit on a bf16 tie")
        assert bool(((r == hi_q) | tie).all()), f"{tag}: hi is not a bf16 nearest to hi + lo"
        lo_q = torch.where(qrows[:, None], lo, torch.zeros_like(lo))
        assert torch.equal(lo_q, (y - hi_q).float().to(torch.bfloat16).double()), f"{tag}: lo != bf16((hi + lo) - hi)"
        assert int(tie.sum()) * 64 <= y.numel() and bool((lo_q != 0).any()), f"{tag}: not a pair"
        got = hi + lo

    # 3. per-tile error against float64
    ref = c.reference(bias_name, scale)
    if hi_only:
        ref = {k: v.float().to(torch.bfloat16).double() for k, v in ref.items()}
    worst, worst_small, row_err = _tile_errors(c, got, ref, tag, rows)
    assert worst < tol, f"{tag}: relative tile error {worst:.3e} >= {tol}"

    # 4. bit equality: a batch-head launched alone (another decode) reproduces its rows and writes nothing else
    if relaunch:
        for b in range(c.B):
            for h in range(c.H):
                O1 = _sentinel_o(c)
                _launch(ops, c, arm, O1, bh=(b, h))
                O1i = O1.view(torch.int16)
                rows_b = c.q_rows(b)
                for cols in ((hc,) if hi_only else (hc, lc)):
                    mine = slice(cols.start + h * 128, cols.start + (h + 1) * 128)
                    assert torch.equal(O1i[rows_b][:, mine], Oi[rows_b][:, mine]), f"{tag}: (b, h) = ({b}, {h}) alone differs from the batched launch"
                    O1i[rows_b, mine] = SENT
                assert bool((O1i == SENT).all()), f"{tag}: (b, h) = ({b}, {h}) alone wrote outside its rows / head"
    return O, row_err


# (the arms of one operand family together: a case's images and references are built once per family)
_MATRIX = [(k, case, arm) for k in ("split", "f32") for case in CASES[k] for arm in sorted(ARMS[k], key=lambda a: ARMS[k][a][0] != "raw")]


@pytest.mark.parametrize("kernel,case,arm", _MATRIX, ids=[f"{k}-{c}-{a}" for k, c, a in _MATRIX])
def test_precise_attention_tile_by_tile(ops, kernel, case, arm):
    """per-tile float64 error, sentinel coverage, the pair property, determinism and lone-head bit equality for one (kernel, shape, arm);
    measured maxima in the module docstring"""
    c = _case(ops, kernel, case, ARMS[kernel][arm][0])
    _check(ops, c, arm, f"{kernel} {case} {arm}", TOL[kernel][arm])


# ---- score extremes --------------------------------------------------------------------------------------------------------------------
X_LENS, X_B, X_H = (70, 200), 1, 2
X_ARM = {"split": "max", "f32": "cfactor"}
X_QUERY = (1, 170)                          # (segment, position) of the spiked query of head 0: in the f32 kernel's second query tile


def _x_buf(seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(X_B * sum(X_LENS), 3 * X_H * 128, generator=g)


# (segment, position) of the aligned key, per kernel: key tiles are 64 (split) / 32 (f32) keys
SPIKES = {
    "first_tile": {"split": (0, 5), "f32": (0, 5)},
    "tile_last_key": {"split": (0, 63), "f32": (0, 31)},
    "ragged_last_tile": {"split": (0, 69), "f32": (0, 69)},          # 70 = 64 + 6 = 2 * 32 + 6
    "second_segment": {"split": (1, 100), "f32": (1, 100)},
}


@pytest.mark.parametrize("where", list(SPIKES))
@pytest.mark.parametrize("kernel", ["split", "f32"])
def test_precise_attention_spiked_scores(ops, kernel, where):
    """One key of head 0 aligned with one query at 6x its magnitude (raw q.k / sqrt(128) ~ 68 above the row's other scores, as in
    test_attention_split_spiked_scores): the running maximum jumps there and every accumulator is rescaled. The spiked row's own error is
    bounded, not only its tile's: the row is one-hot on the spiked key, so what remains is the rounding of the output pair (<= 2^-17 =
    7.6e-6 per element) and of the normalisation -- the arm's tile bound holds for the row alone. Measured row errors: split <= 5.9e-9 (v's
    pair passes through exactly), f32 <= 3.1e-6; tiles 5.0e-6 / 2.6e-6."""
    D = X_H * 128
    e = seg_edges(X_LENS)
    buf = _x_buf()
    ks, kp = SPIKES[where][kernel]
    buf[e[ks] + kp, :128] = buf[e[X_QUERY[0]] + X_QUERY[1], 2 * D:2 * D + 128] * 6.0
    c = _Case(ops, kernel, X_LENS, X_B, X_H, 0, "raw", buf=buf)
    arm = X_ARM[kernel]
    _, row_err = _check(ops, c, arm, f"{kernel} spike {where}", TOL[kernel][arm], rows=[(0, X_QUERY[0], X_QUERY[1], 0)], relaunch=False)
    assert row_err[0] < TOL[kernel][arm], row_err


MEASURED_LARGE = {"split": 2.191e-5, "f32": 4.144e-6}
TOL_LARGE = {k: min(2 * m, START[k]) for k, m in MEASURED_LARGE.items()}      # split: the starting bound itself


@pytest.mark.parametrize("kernel", ["split", "f32"])
def test_precise_attention_large_scores(ops, kernel):
    """q x 50: raw q.k up to ~2000, scores up to ~250 log2 units, a nearly one-hot softmax; the same float64 reference. An arm of its own
    in the measurements (split 2.2e-5, f32 4.1e-6): the bound is 2 x that and never above the starting bound, which for the split kernel
    is the starting 3e-5 itself -- nothing is loosened. Why the split kernel sits higher here than on unit-scale inputs: a partial sum of
    magnitude ~2000 has an fp32 ulp of 2.4e-4, so every rounding of the running q.k moves the score by ~1.5e-5 log2 units and a handful
    of them the probability by ~1e-5 relative; rows whose two largest scores lie within a few units of each other (not one-hot) show it."""
    D = X_H * 128
    buf = _x_buf(seed=12)
    buf[:, 2 * D:] *= 50.0
    c = _Case(ops, kernel, X_LENS, X_B, X_H, 0, "raw", buf=buf)
    _check(ops, c, X_ARM[kernel], f"{kernel} large scores", TOL_LARGE[kernel], relaunch=False)


TOL_NEAR_ROW = 2e-5      # one row alone is noisier than a tile: 2 x the measured 1.02e-5 (a row at -90, an ordinary softmax row), below START


def test_precise_attention_bounded_scores_near_the_bound(ops):
    """LX_ATTN_BOUNDED close to its contract: |q.k (log2 units) + bias log2 e| <= 100 (include/lx.h), here ~90 with either sign for four
    query rows (tests/helpers.py near_bound_qkv). The condition is asserted on the host, in float64, on the images the kernel will read,
    BEFORE the launch: it is the caller's side of the contract. The bounded launch must agree with float64 per tile and on the spiked
    rows, and with the max-tracking launch (LX_ATTN_Q_LOG2 alone) on the same images: both are within their own bound of the same
    float64 values, so within the sum of the two of each other. Measured: tiles 6.4e-6 (bounded) / 5.1e-6 (max-tracking) against float64,
    6.1e-6 against each other; rows <= 8.1e-6 / 1.02e-5 / 6.6e-6 (the rows at +90 are one-hot and exact)."""
    H = 2
    c = _Case(ops, "split", NEAR_BOUND_LENS, 1, H, 0, "log2", buf=near_bound_qkv(ops.Q_LOG2_FACTOR), folded=True)
    q, k, _ = c.qkv64(0)
    worst = max_abs_score_log2(q, k, NEAR_BOUND_LENS, BIASES["cfactor"])
    print(f"PRECISE_TILES near bound: max |score| {worst:.3f} log2 units")
    assert 88.0 <= worst <= 100.0, worst
    rows = [(0, sq, qp, 0) for sq, qp, *_ in NEAR_BOUND_PAIRS]
    Ob, err_b = _check(ops, c, "bnd_bias", "split near bound bnd_bias", TOL["split"]["bnd_bias"], rows=rows, relaunch=False)
    Om, err_m = _check(ops, c, "qlog2", "split near bound qlog2", TOL["split"]["qlog2"], rows=rows, relaunch=False)
    assert max(err_b) < TOL_NEAR_ROW and max(err_m) < TOL_NEAR_ROW, (err_b, err_m)
    D = H * 128
    hc, lc = slice(PAD_L, PAD_L + D), slice(PAD_L + D + MID, PAD_L + 2 * D + MID)
    gb, gm = (O[:, hc].double() + O[:, lc].double() for O in (Ob, Om))
    e = seg_edges(NEAR_BOUND_LENS)
    as_ref = {(0, s): gm[e[s]: e[s + 1]].view(-1, H, 128).permute(1, 0, 2) for s in range(2)}
    worst, _, row_err = _tile_errors(c, gb, as_ref, "split near bound bnd_bias vs qlog2", rows)
    assert worst < TOL["split"]["bnd_bias"] + TOL["split"]["qlog2"]
    assert max(row_err) < 2 * TOL_NEAR_ROW, row_err
