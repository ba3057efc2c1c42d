"""Every 16- and 8-bit store's rounding, saturation and non-finite rule, BIT FOR BIT (no tolerance appears in this file): the final rounding
of an fp32 value into bf16, fp16, e4m3 or a bf16 hi/lo pair, which the relative-L2 bounds of the other suites cannot see.

  A  the converters (lx_convert, lx_convert_f16, lx_convert_fp8, lx_split_bf16) over the full edge sets of tests/store_formats.py;
  B  the GEMM epilogue stores on accumulators that are exact in fp32 whatever the summation order (store_formats.gemm_probe), under every
     launch plan tests/test_gemm_tiles_gpu.py reaches (its arm tables and CU-derived launch shapes, imported), the plan asserted after
     every launch; the fp32 store of the same launch must return the exact sums first (else the probe is void); all plans agree bit for
     bit; then +-inf / NaN through one A element per chosen row and +-inf / NaN / +-1e30 through one bias entry per chosen column;
     the V columns of LX_EPI_QKV launches (the transposed bf16 V^T slots and the e4m3 V^T bytes) on the same exact accumulators;
  C  the computed row producers (the ln_modulate family, GroupNorm) by value class through their additive operand and through one
     non-finite input element; the attention kernels' O store (finite classes: a constant V column within, and beyond, fp16's range).

CONTRACT below is the table of include/lx.h ("Store contract"); the assertions read their expectations from it. Run with -s to print it.
Outputs live inside sentinel-filled buffers; bytes outside the destination keep their bits."""
import pytest
import torch

from tests import store_formats as sf
from tests.test_gemm_tiles_gpu import ARMS16, ARMS_SPLIT, DEV, IVIEW, K_FP8, K_LONG, K_MAIN, K_SPLIT, PAD, SENT, XCOLS, _p, main_rows0, ncu, set_env, workspace

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the contract
# producer, format -> rounding | x beyond the largest finite | +-inf | NaN | counted in f16_ovf?
#   rne            round to nearest even, target subnormals honoured, fp32 subnormal inputs not flushed
#   inf / max      +-inf / +-the largest finite value (65504, 448), of x's sign
#   nan            some NaN code
#   -max           the NEGATIVE largest finite value whatever the NaN's sign (what the clamp makes of a NaN)
#   -max; s: +max  ... of a quiet NaN; a SIGNALLING NaN (quiet bit clear, either sign) gives the POSITIVE largest value. Only lx_convert can
#                  meet one: everywhere else arithmetic (a scale, a bias, a normalisation) has quieted the NaN before the clamp
#   (a, b)         the hi and lo words of a pair
#   none           no contract (not tested)
#   -              cannot occur / does not apply
CONTRACT = {
    ("lx_convert", "bf16"): dict(rounding="rne", beyond="inf", inf="inf", nan="nan", counted="-"),
    ("lx_convert", "f16"): dict(rounding="rne", beyond="max", inf="max", nan="-max; s: +max", counted="no counter"),
    ("lx_convert_f16", "f16"): dict(rounding="rne", beyond="max", inf="max", nan="nan", counted="beyond, inf"),
    ("lx_convert_fp8", "e4m3"): dict(rounding="rne", beyond="max", inf="max", nan="-max", counted="-"),
    ("lx_split_bf16", "pair"): dict(rounding="rne", beyond="(inf, -inf)", inf="(inf, nan)", nan="(nan, nan)", counted="-"),
    ("lx_gemm_bf16 epilogue", "bf16"): dict(rounding="rne", beyond="inf", inf="inf", nan="nan", counted="-"),
    ("lx_gemm_bf16 epilogue", "f16"): dict(rounding="rne", beyond="max", inf="max", nan="-max", counted="beyond, inf; NaN not"),
    ("lx_gemm_bf16 epilogue", "e4m3"): dict(rounding="rne", beyond="max", inf="max", nan="-max", counted="-"),
    ("lx_gemm_bf16 epilogue", "pair"): dict(rounding="rne", beyond="(inf, -inf)", inf="(inf, nan)", nan="(nan, nan)", counted="-"),
    ("lx_ln_modulate*", "bf16"): dict(rounding="rne", beyond="inf", inf="inf", nan="nan", counted="-"),
    ("lx_ln_modulate*", "f16"): dict(rounding="rne", beyond="max", inf="max", nan="-max", counted="beyond, inf; NaN not"),
    ("lx_ln_modulate*", "e4m3"): dict(rounding="rne", beyond="max", inf="max", nan="-max", counted="-"),
    ("lx_ln_modulate*", "pair"): dict(rounding="rne", beyond="(inf, -inf)", inf="(inf, nan)", nan="(nan, nan)", counted="-"),
    ("lx_groupnorm_silu*", "bf16"): dict(rounding="rne", beyond="inf", inf="inf", nan="nan", counted="-"),
    ("lx_groupnorm_silu*", "f16"): dict(rounding="rne", beyond="max", inf="max", nan="-max", counted="beyond, inf; NaN not"),
    ("lx_groupnorm_silu*", "pair"): dict(rounding="rne", beyond="(inf, -inf)", inf="(inf, nan)", nan="(nan, nan)", counted="-"),
    # built with -fno-honor-nans: finite operands only, no contract for NaN / +-inf. O is a computed value (probabilities times V): held
    # here by class -- within an ulp of a constant V column, saturation and counter of the fp16 store. No finite V reaches past bf16's range.
    ("lx_attn_fwd* O", "bf16"): dict(rounding="rne", beyond="-", inf="none", nan="none", counted="-"),
    ("lx_attn_fwd* O", "f16"): dict(rounding="rne", beyond="max", inf="none", nan="none", counted="beyond"),
}
# classes pinned by other suites (left there, named here): saturation + counter of the fp16 GEMM / LayerNorm / GroupNorm producers on random
# data that exceeds the range -- tests/test_f16_gpu.py, tests/test_vae_f16_gpu.py; "saturates instead of producing NaN" of the e4m3 store -- tests/test_fp8_gemm_gpu.py;
# lx_convert_f16's NaN -- tests/test_vae_f16_gpu.py::test_convert_f16_saturates_counts_and_keeps_nan


def contract_text():
    lines = [f"{'producer':24s} {'format':6s} {'rounding':8s} {'beyond range':13s} {'+-inf':11s} {'NaN':14s} counted in f16_ovf"]
    for (prod, fmt), r in CONTRACT.items():
        lines.append(f"{prod:24s} {fmt:6s} {r['rounding']:8s} {r['beyond']:13s} {r['inf']:11s} {r['nan']:14s} {r['counted']}")
    return "\n".join(lines)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    yield o
    print("\nSTORE CONTRACT (include/lx.h):\n" + contract_text())


# ------------------------------------------------------------------------------------------------ expectations from the table
MAXW = {"f16": 0x7BFF, "e4m3": 0x7E}
SIGN = {"bf16": 0x8000, "f16": 0x8000, "e4m3": 0x80}


def is_nan_word(fmt, w):
    if fmt == "e4m3":
        return (w & 0x7F) == 0x7F
    eb, mb, _ = sf.FORMATS[fmt]
    return ((w >> mb) & (2 ** eb - 1) == 2 ** eb - 1) & (w & (2 ** mb - 1) != 0)


def expected_words(producer, fmt, xw, scale=1.0):
    """fp32 words the store receives -> (words it must write, mask where only 'some NaN' is asked). pair: a list of two such."""
    row = CONTRACT[(producer, fmt)]
    x = sf.f32_from_bits(xw)
    if fmt == "pair":
        assert (row["beyond"], row["inf"], row["nan"]) == ("(inf, -inf)", "(inf, nan)", "(nan, nan)")
        hi, lo, ok = sf.ref_pair(xw)
        hi_nan = torch.isnan(x)
        neg = (hi & 0x8000) != 0
        lo = torch.where(ok, lo, torch.where(neg, torch.full_like(lo, 0x7F80), torch.full_like(lo, 0xFF80)))     # beyond: lo = -hi
        return [(hi, hi_nan), (lo, ~torch.isfinite(x))]                                                            # inf, NaN: lo is a NaN
    if fmt == "bf16":
        assert (row["beyond"], row["inf"], row["nan"]) == ("inf", "inf", "nan")
        return sf.ref_bf16(xw)
    want, nan = sf.ref_f16_sat(xw) if fmt == "f16" else sf.ref_e4m3(xw, scale)
    assert (row["beyond"], row["inf"]) == ("max", "max") and row["nan"] in ("nan", "-max", "-max; s: +max")
    if row["nan"] != "nan":
        signalling = (xw & 0x00400000) == 0 if row["nan"] == "-max; s: +max" else torch.zeros_like(nan)
        want = torch.where(nan, torch.where(signalling, MAXW[fmt], MAXW[fmt] | SIGN[fmt]), want)
        nan = torch.zeros_like(nan)
    return want, nan


def assert_words(what, fmt, got, want, nan_mask, xw=None):
    f = "bf16" if fmt == "pair" else fmt
    ok = torch.where(nan_mask, is_nan_word(f, got), got == want)
    if not bool(ok.all()):
        i = (~ok).nonzero()[0]
        at = tuple(i.tolist())
        src = "" if xw is None else f" of x = 0x{int(xw[at]):08x} ({float(sf.f32_from_bits(xw[at].reshape(1))[0])!r})"
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} words differ; first at {at}: got 0x{int(got[at]):x}, want "
                             f"{'a NaN' if bool(nan_mask[at]) else hex(int(want[at]))}{src}")


def words_of(t):
    if t.dtype == torch.uint8:
        return t.to(torch.int64)
    if t.dtype == torch.float32:
        return sf.bits_from_f32(t)
    return sf.bits16(t)


def tensor16(words, dtype):
    w = words.to(torch.int64)
    return torch.where(w >= 32768, w - 65536, w).to(torch.int16).view(dtype)


class Guarded:
    """a 2-D output [rows, cols] inside a sentinel-filled buffer: PAD rows above and below, XCOLS columns to the right"""

    def __init__(self, dtype, rows, cols, xcols=XCOLS):
        self.dtype, self.rows, self.cols = dtype, rows, cols
        self.buf = torch.empty(rows + 2 * PAD, cols + xcols, dtype=dtype, device=DEV)
        self.fill()
        self.out = self.buf[PAD:PAD + rows, :cols]

    def fill(self):
        s = SENT[self.dtype]
        self.buf.view(IVIEW[self.dtype]).fill_(s if s < 2 ** 31 else s - 2 ** 32)

    def words(self):
        return words_of(self.out)

    def check_outside(self, what, written=None):
        """everything outside the column ranges `written` (default: all of out) of the output rows keeps the sentinel"""
        w = words_of(self.buf) != SENT[self.dtype]
        for c0, c1 in (written or [(0, self.cols)]):
            w[PAD:PAD + self.rows, c0:c1] = False
        assert not bool(w.any()), f"{what}: {int(w.sum())} elements outside the destination changed (first at {w.nonzero()[0].tolist()})"


def sync():
    torch.cuda.synchronize()


# ================================================================================================ A. the converters
G1 = 64          # sentinel elements before and after a 1-D destination


def convert_1d(call, dst_dtype, src):
    n = src.numel()
    buf = torch.empty(n + 2 * G1, dtype=dst_dtype, device=DEV)
    s = SENT[dst_dtype]
    buf.view(IVIEW[dst_dtype]).fill_(s if s < 2 ** 31 else s - 2 ** 32)
    call(buf[G1:G1 + n], src)
    sync()
    w = words_of(buf)
    assert bool((w[:G1] == s).all()) and bool((w[G1 + n:] == s).all()), "the converter wrote outside its destination"
    return w[G1:G1 + n]


@pytest.fixture(scope="module")
def edges():
    e = {"bf16": sf.edge_set("bf16").to(DEV), "f16": sf.edge_set("f16").to(DEV), "allbf16": sf.all_bf16_words().to(DEV)}
    for s in (1.0, 16.0, 0.125):
        e[("e4m3", s)] = sf.edge_set("e4m3", s).to(DEV)
    return e


def test_convert_f32_to_bf16(ops, edges):
    for name in ("bf16", "f16"):
        xw = edges[name]
        got = convert_1d(ops.convert, torch.bfloat16, sf.f32_from_bits(xw))
        assert_words(f"lx_convert fp32 -> bf16 ({name} edges)", "bf16", got, *expected_words("lx_convert", "bf16", xw), xw)


def test_convert_f32_to_f16_saturates_uncounted(ops, edges):
    for name in ("f16", "bf16"):
        xw = edges[name]
        got = convert_1d(ops.convert, torch.float16, sf.f32_from_bits(xw))
        assert_words(f"lx_convert fp32 -> fp16 ({name} edges)", "f16", got, *expected_words("lx_convert", "f16", xw), xw)


def test_convert_bf16_to_f16_f32_and_f32_to_f32(ops, edges):
    bw = edges["allbf16"]
    xw = sf.bf16_words_as_f32_words(bw)
    src = tensor16(bw, torch.bfloat16)
    got = convert_1d(ops.convert, torch.float16, src)
    assert_words("lx_convert bf16 -> fp16", "f16", got, *expected_words("lx_convert", "f16", xw), xw)
    nan = torch.isnan(sf.f32_from_bits(xw))
    got = convert_1d(ops.convert, torch.float32, src)
    assert bool(torch.where(nan, torch.isnan(sf.f32_from_bits(got)), got == xw).all()), "lx_convert bf16 -> fp32 is not the word shifted up"
    for name in ("bf16", "f16"):
        xw = edges[name]
        nan = torch.isnan(sf.f32_from_bits(xw))
        got = convert_1d(ops.convert, torch.float32, sf.f32_from_bits(xw))
        assert bool(torch.where(nan, torch.isnan(sf.f32_from_bits(got)), got == xw).all()), "lx_convert fp32 -> fp32 changed a value"


@pytest.mark.parametrize("src", ["f32", "bf16"])
def test_convert_f16_rounds_saturates_counts_and_keeps_nan(ops, edges, src):
    if src == "f32":
        xw = torch.cat([edges["f16"], edges["bf16"]])
        x = sf.f32_from_bits(xw)
    else:
        xw = sf.bf16_words_as_f32_words(edges["allbf16"])
        x = tensor16(edges["allbf16"], torch.bfloat16)
    counted = sf.counted_f16(xw)
    assert bool(counted.any())
    for sub, name in ((torch.ones_like(counted), "the full set"), (~counted, "the subset without |x| > 65504")):
        ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = convert_1d(lambda d, s: ops.convert_f16(d, s, f16_ovf=ovf), torch.float16, x[sub].contiguous())
        assert_words(f"lx_convert_f16 from {src}, {name}", "f16", got, *expected_words("lx_convert_f16", "f16", xw[sub]), xw[sub])
        assert (int(ovf) > 0) == bool(counted[sub].any()), f"lx_convert_f16 from {src}, {name}: f16_ovf = {int(ovf)}"


FP8_K, FP8_SCALES = 72, (1.0, 16.0, 0.125, 0.3)


def rows_of(x, K, fill):
    """1-D -> [M, K] padded with `fill`"""
    M = -(-x.numel() // K)
    out = torch.full((M * K,), fill, dtype=x.dtype, device=x.device)
    out[:x.numel()] = x
    return out.view(M, K)


@pytest.mark.parametrize("scale", FP8_SCALES)
@pytest.mark.parametrize("src", ["f32", "bf16"])
def test_convert_fp8(ops, edges, src, scale):
    if src == "f32":
        xw = rows_of(edges[("e4m3", scale if scale != 0.3 else 1.0)], FP8_K, 0)
        x = sf.f32_from_bits(xw)
    else:
        bw = rows_of(edges["allbf16"], FP8_K, 0)
        xw, x = sf.bf16_words_as_f32_words(bw), tensor16(bw, torch.bfloat16)
    M = x.shape[0]
    xs = torch.zeros(M, FP8_K + 8, dtype=x.dtype, device=DEV)          # lds = K + 8
    xs[:, :FP8_K] = x
    out = Guarded(torch.uint8, M, FP8_K, xcols=16)                      # ldd = K + 16
    ops.convert_fp8(xs[:, :FP8_K], out.out, scale)
    sync()
    out.check_outside(f"lx_convert_fp8 from {src}")
    assert_words(f"lx_convert_fp8 from {src} at scale {scale}", "e4m3", out.words(), *expected_words("lx_convert_fp8", "e4m3", xw, scale), xw)


SPLIT_K = 68


def test_split_bf16(ops, edges):
    xw = rows_of(torch.cat([edges["bf16"], edges["f16"]]), SPLIT_K, 0)
    M = xw.shape[0]
    xs = torch.zeros(M, SPLIT_K + 4, dtype=torch.float32, device=DEV)
    xs[:, :SPLIT_K] = sf.f32_from_bits(xw)
    lo_off = SPLIT_K + 4
    out = Guarded(torch.bfloat16, M, lo_off + SPLIT_K, xcols=12)
    ops.split_bf16(xs[:, :SPLIT_K], out.buf[PAD:PAD + M], lo_off)
    sync()
    out.check_outside("lx_split_bf16", [(0, SPLIT_K), (lo_off, lo_off + SPLIT_K)])
    w = out.words()
    (hi, hi_nan), (lo, lo_nan) = expected_words("lx_split_bf16", "pair", xw)
    assert_words("lx_split_bf16 hi", "pair", w[:, :SPLIT_K], hi, hi_nan, xw)
    assert_words("lx_split_bf16 lo", "pair", w[:, lo_off:], lo, lo_nan, xw)


# ================================================================================================ B. GEMM epilogue stores
# probe name -> (operand format of store_formats, target, target scale, pair columns, descriptor format)
PROBES = {
    "bf16": ("bf16", "bf16", 1.0, False, "bf16"),
    "f16": ("f16", "f16", 1.0, False, "f16"),
    "fp8/bf16": ("e4m3", "bf16", 1.0, False, "fp8"),
    "fp8/e4m3": ("e4m3", "e4m3", 0.5, False, "fp8"),
    "split2": ("bf16", "bf16", 1.0, True, "split2"),
    "split3": ("bf16", "bf16", 1.0, True, "split3"),
}
STORES = {"bf16": ("bf16",), "f16": ("f16",), "fp8/bf16": ("bf16",), "fp8/e4m3": ("e4m3",), "split2": ("bf16", "pair"), "split3": ("bf16", "pair")}
OP_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "e4m3": torch.float8_e4m3fn}
SHAPES, ROW0 = sf.PROBE_SHAPES, sf.PROBE_ROW0        # (tests/test_store_formats_ref_cpu.py: p3 holds nothing beyond fp16's range, p1 does)


class ProbeProblem:
    def __init__(self, probe, i, M, N, K):
        opfmt, target, scale, pair, fmt = PROBES[probe]
        self.probe, self.M, self.N, self.K, self.fmt, self.target, self.scale = probe, M, N, K, fmt, target, scale
        a0, a1, w0, w1 = sf.gemm_probe(opfmt, target, M, N, ROW0[i], scale, pair)        # (host tensors: operands are made there)
        self.a0, self.a1, self.w0, self.w1 = a0, a1, w0, w1
        self.acc = sf.probe_acc(a0.to(DEV), a1.to(DEV), w0.to(DEV), w1.to(DEV))        # float64, exact
        self.accw = sf.f32_words_from_exact(self.acc)                                  # ... as fp32 words
        self.dt = dt = OP_DTYPE[opfmt]
        segs = int(fmt[-1]) if fmt.startswith("split") else 1
        self.segs, self.a_lo = segs, K + 64
        store_dt = torch.uint8 if fmt == "fp8" else dt
        self.A = torch.zeros(M, K if segs == 1 else 2 * K + 128, dtype=store_dt, device=DEV)        # (all-zero words are +0 in every format)
        self.W = torch.zeros(N, 2 * K if segs == 3 else K, dtype=store_dt, device=DEV)
        self.put(self.A, 0, a0)
        self.put(self.A, K - 1, a1)                                                     # first and last column of K: a split-K plan separates them
        self.put(self.W, 0, w0)
        self.put(self.W, K - 1, w1)
        self.ovf = torch.zeros(1, dtype=torch.int32, device=DEV) if fmt == "f16" else None
        self.bias = None

    def put(self, T, col, v64):
        """column `col` of an operand image = the float64 values, which the operand format must hold exactly (non-finite ones aside)"""
        v64 = v64.cpu()
        v = v64.float().to(self.dt)
        fin = torch.isfinite(v64)
        assert torch.equal(v.float().double()[fin], v64[fin]), "an operand is not a value of the operand format"
        iv = torch.uint8 if self.dt == torch.float8_e4m3fn else torch.int16
        T.view(iv)[:, col] = v.view(iv).to(DEV)

    def set_a0(self, a0):
        self.put(self.A, 0, a0)

    def out(self, store):
        dt = {"f32": torch.float32, "bf16": torch.bfloat16, "pair": torch.bfloat16, "f16": torch.float16, "e4m3": torch.uint8}[store]
        return Guarded(dt, self.M, 2 * self.N + 8 if store == "pair" else self.N)

    def desc(self, ops, store, g):
        kw = dict(M=self.M, N=self.N, K=self.K, bias=self.bias)
        epi = {"f32": ops.LX_EPI_STORE_F32, "e4m3": ops.LX_EPI_STORE_FP8}.get(store, ops.LX_EPI_STORE_BF16)
        if self.fmt == "fp8":
            kw.update(fp8=True)
            if store == "e4m3":
                kw["out_scale"] = self.scale
        elif self.fmt == "f16":
            kw.update(f16=True, f16_ovf=self.ovf)
        elif self.segs > 1:
            kw.update(k_segs=self.segs, a_lo_off=self.a_lo)
            if store == "pair":
                kw["c_lo_off"] = self.N + 8
        C_ = g.buf[PAD:PAD + self.M] if store == "pair" else g.out
        return ops.gemm_desc(self.A, self.W, C_, epilogue=epi, **kw)


_PROBLEMS = {}


def problems(probe, size):
    key = (probe, size, ncu())
    if key not in _PROBLEMS:
        rows0, K = (1, K_LONG) if size == "long" else (main_rows0() if size == "main" else 1, {"fp8": K_FP8, "split2": K_SPLIT, "split3": K_SPLIT}.get(PROBES[probe][4], K_MAIN))
        M0 = 20 if rows0 == 1 else 256 * (rows0 - 1) + 1
        _PROBLEMS[key] = [ProbeProblem(probe, i, M0 if M is None else M, N, K) for i, (M, N) in enumerate(SHAPES)]
    return _PROBLEMS[key]


def launch(ops, probs, store, ws, plan, what):
    gs = [p.out(store) for p in probs]
    for p in probs:
        if p.ovf is not None:
            p.ovf.zero_()
    ops.gemm([p.desc(ops, store, g) for p, g in zip(probs, gs)], ws)
    got = ops.gemm_last_plan()
    assert got == plan, f"{what}: the planner chose plan {got}, not {plan} ({ncu()} CUs)"
    if ws is not None:
        assert ops.lib.lx_gemm_workspace_status(ws.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    sync()
    for p, g in zip(probs, gs):
        g.check_outside(what, [(0, p.N), (p.N + 8, 2 * p.N + 8)] if store == "pair" else None)
    return gs


def check_store(what, p, store, g, xw, producer="lx_gemm_bf16 epilogue"):
    w = g.buf[PAD:PAD + p.M]
    if store == "pair":
        (hi, hi_nan), (lo, lo_nan) = expected_words(producer, "pair", xw)
        ww = words_of(w)
        assert_words(what + " hi", "pair", ww[:, :p.N], hi, hi_nan, xw)
        assert_words(what + " lo", "pair", ww[:, p.N + 8:2 * p.N + 8], lo, lo_nan, xw)
    else:
        assert_words(what, store, g.words(), *expected_words(producer, store, xw, p.scale), xw)


def exact_probe(ops, monkeypatch, probe, arm, env, use_ws, plan, size):
    probs = problems(probe, size)
    ws = workspace(ops) if use_ws else None
    set_env(ops, monkeypatch, env)
    what = f"{probe} {arm}"
    # precondition: the fp32 store of the same operands under the same plan returns the exact sums
    for p, g in zip(probs, launch(ops, probs, "f32", ws, _p(plan), what + " f32")):
        got = g.words()
        bad = (got != p.accw) & (((got | p.accw) & 0x7FFFFFFF) != 0)                  # (+-0 compare equal)
        assert not bool(bad.any()), f"{what}: THE PROBE IS VOID -- the fp32 store is not the exact sum at {int(bad.sum())} elements (first " \
                                    f"{bad.nonzero()[0].tolist()}: 0x{int(got[bad][0]):08x} for 0x{int(p.accw[bad][0]):08x}); nothing is said about the narrow stores"
    clean = {}                                           # store -> the words of every problem's buffer
    for store in STORES[probe]:
        gs = launch(ops, probs, store, ws, _p(plan), f"{what} {store}")
        for i, (p, g) in enumerate(zip(probs, gs)):
            xw = p.accw
            check_store(f"{what} {store} p{i} [{p.M} x {p.N}]", p, store, g, xw)
            if p.ovf is not None:
                some = bool(sf.counted_f16(xw).any())
                if i in (1, 3):
                    assert some == (i == 1), "the probe's layout: p3 holds nothing beyond fp16's range, p1 something"
                assert (int(p.ovf) > 0) == some, f"{what} p{i}: f16_ovf = {int(p.ovf)} with{'' if some else 'out'} |x| > 65504 in the launch"
        clean[store] = [words_of(g.buf) for g in gs]
    return probs, ws, clean


# ---- non-finite values through a GEMM: one A element per chosen row, one bias entry per chosen column
INF, NAN = float("inf"), float("nan")


def inject(ops, probs, ws, plan, probe, arm, clean_bits):
    """p0 ... p2: rows 1, 5, 9 take a0 = +inf, -inf, NaN (e4m3 operands: NaN only); columns 2, 11, 20, 29, 38 take bias +inf, -inf, NaN,
    1e30, -1e30. p3 takes NaN alone (row 3, column 7): its fp16 counter says whether a NaN is counted. The value every element holds
    before the store is then the fp32 sum of the exact accumulator (non-finite in the chosen rows) and the bias."""
    opfmt = PROBES[probe][0]
    saved = []
    for i, p in enumerate(probs):
        a0 = p.a0.clone()
        bias = torch.zeros(p.N, dtype=torch.float32, device=DEV)
        if i == 3:
            a0[3] = NAN
            bias[7] = NAN
        else:
            for r, v in ((1, INF), (5, -INF), (9, NAN)):
                if opfmt != "e4m3" or v != v:
                    a0[r] = v
            for c, v in ((2, INF), (11, -INF), (20, NAN), (29, 1e30), (38, -1e30)):
                bias[c] = v
        saved.append((p.a0, a0, bias))
    try:
        for p, (_, a0, bias) in zip(probs, saved):
            p.set_a0(a0)
            p.bias = bias
        for store in STORES[probe]:
            gs = launch(ops, probs, store, ws, plan, f"{probe} {arm} {store} non-finite")
            for i, (p, g, (clean, a0, bias)) in enumerate(zip(probs, gs, saved)):
                what = f"{probe} {arm} {store} p{i} non-finite"
                touched = ~torch.isfinite(a0).to(DEV)[:, None] | (bias != 0)[None, :]
                acc = sf.f32_from_bits(p.accw)
                bad_row = (a0.to(DEV)[:, None] * p.w0.to(DEV)[None, :]).float()
                if p.segs == 3:                       # k_segs = 3 also multiplies A by W's lo image, which is zero here: inf * 0
                    bad_row = torch.full_like(bad_row, NAN)
                acc = torch.where(~torch.isfinite(a0).to(DEV)[:, None], bad_row, acc)   # +-inf, NaN rows
                x = torch.where(touched, acc + bias[None, :], acc)                   # one fp32 addition (never near fp32's subnormals)
                # classes: the stores of the chosen rows and columns are what the table says of that class; where the sum is finite
                # and in range only that is asked (the bias may join the sum at another point of a split plan)
                fin = torch.isfinite(x) & touched
                target = "bf16" if store == "pair" else store
                cls_fin = fin & (x.abs() <= sf.max_finite(target) / p.scale * (1 - 2.0 ** -6))
                big = fin & ~cls_fin
                # finite in-range sums of the +-1e30 columns (bf16, pair: 1e30 is in range): where one term is below a quarter of an ulp
                # of the other (2^-26) the sum is the larger term wherever the bias joins it, and the store is held to the reference; in
                # between only "finite" is asked, and at the top of bf16's range (where the class depends on the order) nothing.
                # Everything else -- non-finite classes, saturating formats, untouched elements -- is held to the reference store of x
                order_free = (acc.abs() < 1e30 * 2.0 ** -26) | (acc.abs() * 2.0 ** -26 > 1e30)
                sel = (~cls_fin & ~big) | (cls_fin & order_free) if target == "bf16" else ~cls_fin
                xw = sf.bits_from_f32(x)
                ww = words_of(g.buf[PAD:PAD + p.M])
                if store != "pair":
                    w = ww[:, :p.N]
                    okc = ~is_nan_word(store, w) & (((w & 0x7F80) != 0x7F80) if store == "bf16" else ((w & 0x7C00) != 0x7C00) if store == "f16" else (w >= 0))
                    assert bool(okc[cls_fin].all()), f"{what}: a finite in-range sum was stored as a non-finite code"
                    want, nan = expected_words("lx_gemm_bf16 epilogue", store, xw, p.scale)
                    assert_words(what, store, w[sel], want[sel], nan[sel], xw[sel])
                else:
                    (hi, hi_nan), (lo, lo_nan) = expected_words("lx_gemm_bf16 epilogue", "pair", xw)
                    assert_words(what + " hi", "pair", ww[:, :p.N][sel], hi[sel], hi_nan[sel], xw[sel])
                    assert_words(what + " lo", "pair", ww[:, p.N + 8:2 * p.N + 8][sel], lo[sel], lo_nan[sel], xw[sel])
                    assert bool(((ww[:, :p.N][cls_fin] & 0x7F80) != 0x7F80).all()), f"{what}: a finite in-range sum was stored as a non-finite code"
                if p.ovf is not None:
                    counted = bool((sf.counted_f16(sf.bits_from_f32(x))).any())
                    nan_counts = "NaN not" not in CONTRACT[("lx_gemm_bf16 epilogue", "f16")]["counted"]
                    if i == 3:
                        assert not counted and (int(p.ovf) > 0) == nan_counts, f"{what}: f16_ovf = {int(p.ovf)} for a launch whose only specials are NaNs"
                    else:
                        assert int(p.ovf) > 0
                # untouched rows and columns keep the bits of the clean launch
                cleanw = clean_bits[store][i][PAD:PAD + p.M]
                noww = words_of(g.buf[PAD:PAD + p.M])
                keep = ~touched
                if store == "pair":
                    keep = torch.cat([keep, torch.zeros(p.M, 8, dtype=torch.bool, device=DEV), keep, torch.zeros(p.M, XCOLS, dtype=torch.bool, device=DEV)], 1)
                    assert torch.equal(noww[keep], cleanw[keep]), f"{what}: an untouched element changed"
                else:
                    assert torch.equal(noww[:, :p.N][keep], cleanw[:, :p.N][keep]), f"{what}: an untouched element changed"
    finally:
        for p, (clean, _, _) in zip(probs, saved):
            p.set_a0(clean)
            p.bias = None


@pytest.mark.parametrize("arm", list(ARMS16))
@pytest.mark.parametrize("probe", ["bf16", "f16"])
def test_gemm_stores_16bit_operands(ops, monkeypatch, probe, arm):
    env, use_ws, plan, size = ARMS16[arm]
    probs, ws, clean = exact_probe(ops, monkeypatch, probe, arm, env, use_ws, plan, size)
    inject(ops, probs, ws, _p(plan), probe, arm, clean)


@pytest.mark.parametrize("arm", ["w256", "w128"])
@pytest.mark.parametrize("probe", ["fp8/bf16", "fp8/e4m3"])
def test_gemm_stores_fp8_operands(ops, monkeypatch, probe, arm):
    plan = "8WAVE_" + arm[1:]
    probs, ws, clean = exact_probe(ops, monkeypatch, probe, arm, {"LX_GEMM_BM": arm[1:]}, False, plan, "main")
    inject(ops, probs, ws, _p(plan), probe, arm, clean)


@pytest.mark.parametrize("arm", list(ARMS_SPLIT))
@pytest.mark.parametrize("probe", ["split2", "split3"])
def test_gemm_stores_split_bf16(ops, monkeypatch, probe, arm):
    env, use_ws, plan = ARMS_SPLIT[arm]
    probs, ws, clean = exact_probe(ops, monkeypatch, probe, arm, env, use_ws, plan, "small")
    inject(ops, probs, ws, _p(plan), probe, arm, clean)


def probe_arms(probe):
    """(arm, environment, workspace?, plan, launch size) of every plan a probe runs under"""
    if probe in ("bf16", "f16"):
        return [(a,) + ARMS16[a] for a in ARMS16]
    if probe.startswith("fp8"):
        return [(a, {"LX_GEMM_BM": a[1:]}, False, "8WAVE_" + a[1:], "main") for a in ("w256", "w128")]
    return [(a,) + ARMS_SPLIT[a] + ("small",) for a in ARMS_SPLIT]


@pytest.mark.parametrize("probe", list(PROBES))
def test_gemm_stores_agree_across_plans(ops, monkeypatch, probe):
    """On exact accumulators all plans of one operand format write the same bits (the case XPLAN_TOL16 of tests/test_gemm_tiles_gpu.py
    has to excuse on random data): every narrow store of every problem, sentinels included; p1 ... p3 are the same problems in the
    main and the long-K launches, p0 is compared among the launches of its size."""
    first = {}
    for arm, env, use_ws, plan, size in probe_arms(probe):
        probs = problems(probe, size)
        set_env(ops, monkeypatch, env)
        for store in STORES[probe]:
            gs = launch(ops, probs, store, workspace(ops) if use_ws else None, _p(plan), f"{probe} {arm} {store}")
            for i, g in enumerate(gs):
                key = (store, i if i else (size, 0))
                bits = words_of(g.buf)
                if key in first:
                    assert torch.equal(first[key][1], bits), f"{probe} {store} p{i}: plan {arm} differs from plan {first[key][0]} on exact accumulators"
                else:
                    first[key] = (arm, bits)


# ---- the v columns of an LX_EPI_QKV launch: the transposed V^T store (bf16 slots) and the e4m3 V^T bytes, on the same exact accumulators.
# One [k | v | q | mlp] problem of tests/test_qkv_epilogue_tiles_gpu.py's single-block launch (its shape, arms, Stream / Launch / run and
# slot decode, imported); W is zero outside the v rows, so k and q are RMSNorm + RoPE of zeros. The k and q columns are left out here.
QKV_ARMS = {"bf16": ("w256", "w128", "mixed", "g4", "sk2", "sk3"), "e4m3": ("w256", "w128", "mixed")}
_QKV = {}


def qkv_probe(ops, target):
    from tests import test_qkv_epilogue_tiles_gpu as tq
    from tests.helpers import QKV_SINGLE, qkv_single_shape
    if target not in _QKV:
        shapes = qkv_single_shape(ncu())
        if shapes is None:
            pytest.skip(f"no single-block launch shape for {ncu()} CUs")
        L, N, D = QKV_SINGLE["L"], QKV_SINGLE["N"], tq.D
        M = shapes[0][0]
        scale = 1.0 if target == "bf16" else float(ops.FP8_V_SCALE)
        assert scale == 2.0 ** round(torch.log2(torch.tensor(scale)).item()), "qkv_v_scale must be a power of two for an exact probe"
        st = tq.Stream(f"probe/{target}", "bf16", M // L, L, N, tq.K_MAIN, 1700, gelu=True)
        a0, a1, w0, w1 = sf.gemm_probe("bf16", target, M, D, 0, scale)
        st.A.zero_(), st.W.zero_(), st.bias.zero_()
        K = st.K
        st.A[:, 0], st.A[:, K - 1] = a0.float().to(torch.bfloat16).to(DEV), a1.float().to(torch.bfloat16).to(DEV)
        st.W[D:2 * D, 0], st.W[D:2 * D, K - 1] = w0.float().to(torch.bfloat16).to(DEV), w1.float().to(torch.bfloat16).to(DEV)
        assert torch.equal(st.A[:, 0].cpu().double(), a0) and torch.equal(st.A[:, K - 1].cpu().double(), a1)
        assert torch.equal(st.W[D:2 * D, 0].cpu().double(), w0) and torch.equal(st.W[D:2 * D, K - 1].cpu().double(), w1)
        accw = sf.f32_words_from_exact(sf.probe_acc(a0.to(DEV), a1.to(DEV), w0.to(DEV), w1.to(DEV)))
        _QKV[target] = (tq.Launch(f"probe/{target}", [st], None, target == "e4m3"), accw, scale)
    return _QKV[target]


@pytest.mark.parametrize("target,arm", [(t, a) for t in QKV_ARMS for a in QKV_ARMS[t]])
def test_qkv_epilogue_v_columns(ops, monkeypatch, target, arm):
    from tests import test_qkv_epilogue_tiles_gpu as tq
    from tests.helpers import vt8_slot_keys, vt_slot_keys
    lau, accw, scale = qkv_probe(ops, target)
    st = lau.streams[0]
    D = tq.D
    env, use_ws, plan = tq.ARMS[arm]
    what = f"LX_EPI_QKV v columns, {target} V^T, plan {arm}"
    # precondition: the fp32 store of the same operands and shape under the same plan returns the exact sums in the v columns
    set_env(ops, monkeypatch, env)
    g = Guarded(torch.float32, st.M, st.N)
    ops.gemm([ops.gemm_desc(st.A, st.W, g.out, epilogue=ops.LX_EPI_STORE_F32)], workspace(ops) if use_ws else None)
    assert ops.gemm_last_plan() == _p(plan), f"{what}: the fp32 launch ran under plan {ops.gemm_last_plan()}, not {_p(plan)}"
    sync()
    got = g.words()[:, D:2 * D]
    bad = (got != accw) & (((got | accw) & 0x7FFFFFFF) != 0)
    assert not bool(bad.any()), f"{what}: THE PROBE IS VOID -- the fp32 store is not the exact sum at {int(bad.sum())} elements; nothing is said about the V^T stores"
    o = tq.run(ops, monkeypatch, lau, arm, check=False)                 # (asserts the plan; two runs give the same bits)
    v = lau.got(ops, o, 0)["v"][0]                                       # [M, D] in key order, decoded from the V^T slots
    assert_words(what, target, words_of(v), *expected_words("lx_gemm_bf16 epilogue", target, accw, scale), accw)
    # footprint of the V^T image: exactly the slots of keys that exist are written
    n = (st.L + 63) // 64 * 64
    written = torch.zeros(lau.vt_ld, dtype=torch.bool)
    written[:n] = (vt8_slot_keys(n) if lau.f8 else vt_slot_keys(n)) < st.L
    vt = words_of(o["VT"])
    kept = vt == SENT[o["VT"].dtype]
    assert not bool((~kept & ~written.to(DEV)).any()), f"{what}: V^T slots outside the stream's keys were written"
    if o["VT16"] is not None:
        assert bool((words_of(o["VT16"]) == SENT[torch.bfloat16]).all()), f"{what}: the bf16 V^T image was written beside the e4m3 one"


# ================================================================================================ C. computed row producers, by class
# value classes of an fp32 value on its way into a store
FIN, BIG, PINF, NINF, CNAN = 0, 1, 2, 3, 4


def class_value(k, negative):
    return {BIG: -1e30 if negative else 1e30, PINF: INF, NINF: -INF, CNAN: NAN}[k]


def check_classes(what, producer, fmt, w, cls, neg, scale=1.0):
    """w: the stored words (pair: (hi, lo)); cls: the class of every element's fp32 value, neg: its sign where the class has one"""
    row = CONTRACT[(producer, fmt)]
    if fmt == "pair":
        hi, lo = w
        assert bool((((hi & 0x7F80) != 0x7F80) & ((lo & 0x7F80) != 0x7F80))[(cls == FIN) | (cls == BIG)].all()), f"{what}: finite values (1e30 is in bf16's range) must give a finite pair"
        inf = (cls == PINF) | (cls == NINF)
        assert row["inf"] == "(inf, nan)" and row["nan"] == "(nan, nan)"
        assert bool((hi[inf] == torch.where(cls[inf] == NINF, 0xFF80, 0x7F80)).all()) and bool(is_nan_word("bf16", lo[inf]).all()), f"{what}: +-inf must give (+-inf, NaN)"
        assert bool(is_nan_word("bf16", hi[cls == CNAN]).all()) and bool(is_nan_word("bf16", lo[cls == CNAN]).all()), f"{what}: NaN must give (NaN, NaN)"
        return
    if fmt == "bf16":
        assert bool(((w & 0x7F80) != 0x7F80)[(cls == FIN) | (cls == BIG)].all()), f"{what}: finite values (1e30 is in bf16's range) must stay finite"
        assert bool((w[cls == PINF] == 0x7F80).all()) and bool((w[cls == NINF] == 0xFF80).all()), f"{what}: +-inf must stay +-inf"
        assert bool(is_nan_word("bf16", w[cls == CNAN]).all()), f"{what}: NaN must stay NaN"
        return
    assert bool((~is_nan_word(fmt, w) & ((w & 0x7C00) != 0x7C00 if fmt == "f16" else torch.ones_like(w, dtype=torch.bool)))[cls == FIN].all()), f"{what}: a finite value left the range"
    sat = (cls == BIG) | (cls == PINF) | (cls == NINF)
    want = torch.where(neg, MAXW[fmt] | SIGN[fmt], MAXW[fmt])
    assert bool((w[sat] == want[sat]).all()), f"{what}: beyond the range and +-inf must saturate to the largest finite value of their sign"
    if row["nan"] == "-max":
        assert bool((w[cls == CNAN] == (MAXW[fmt] | SIGN[fmt])).all()), f"{what}: the table says NaN -> -max; got {[hex(int(v)) for v in w[cls == CNAN].unique()[:4]]}"
    else:
        assert bool(is_nan_word(fmt, w[cls == CNAN]).all()), f"{what}: NaN must stay NaN"


def check_counter(what, producer, ovf, cls):
    some = bool(((cls == BIG) | (cls == PINF) | (cls == NINF)).any())
    nan_counts = "NaN not" not in CONTRACT[(producer, "f16")]["counted"]
    want = some or (nan_counts and bool((cls == CNAN).any()))
    assert (int(ovf) > 0) == want, f"{what}: f16_ovf = {int(ovf)}, classes present {cls.unique().tolist()}"


LN_ROWS, LN_B = 8, 2
LN_INJECT = {"shift": [(0, 5, BIG, False), (0, 14, BIG, True), (1, 23, PINF, False), (1, 32, NINF, True), (0, 41, CNAN, False)],      # (batch, column, class, negative)
             "x": [(2, 3, PINF), (5, 10, NINF), (11, 17, CNAN)]}                                                                          # (row, column, class) -> the whole row is NaN


def ln_case(D, via, only_nan=False):
    g = torch.Generator(device=DEV).manual_seed(D)
    M = LN_ROWS * LN_B
    X = torch.randn(M, D, generator=g, device=DEV)
    shift = torch.randn(LN_B, D, generator=g, device=DEV) * 0.1
    scale = torch.randn(LN_B, D, generator=g, device=DEV) * 0.1
    cls = torch.zeros(M, D, dtype=torch.int64, device=DEV)
    neg = torch.zeros(M, D, dtype=torch.bool, device=DEV)
    if via == "shift":
        for b, c, k, n in LN_INJECT["shift"]:
            if only_nan and k != CNAN:
                continue
            shift[b, c] = class_value(k, n)
            cls[b * LN_ROWS:(b + 1) * LN_ROWS, c] = k
            neg[b * LN_ROWS:(b + 1) * LN_ROWS, c] = n
    else:
        for r, c, k in LN_INJECT["x"]:
            if only_nan and k != CNAN:
                continue
            X[r, c] = class_value(k, False)
            cls[r] = CNAN                                 # mean and variance of the row are no longer numbers
    return X, shift, scale, cls, neg


@pytest.mark.parametrize("via", ["shift", "x"])
@pytest.mark.parametrize("D", [3072, 200])
@pytest.mark.parametrize("fmt", ["bf16", "f16", "e4m3", "pair"])
def test_ln_modulate_stores_by_class(ops, fmt, D, via):
    for only_nan in (False, True):
        X, shift, scale, cls, neg = ln_case(D, via, only_nan)
        M = X.shape[0]
        segs = [(0, M, LN_ROWS, shift, scale)]
        what = f"ln_modulate {fmt} D={D} via {via}{' (NaN only)' if only_nan else ''}"
        if fmt == "bf16":
            g = Guarded(torch.bfloat16, M, D)
            ops.ln_modulate(X, shift, scale, g.out, LN_ROWS)
            sync()
            g.check_outside(what)
            check_classes(what, "lx_ln_modulate*", "bf16", g.words(), cls, neg)
        elif fmt == "f16":
            g = Guarded(torch.float16, M, D)
            ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.ln_modulate(X, shift, scale, g.out, LN_ROWS, f16_ovf=ovf)
            sync()
            g.check_outside(what)
            check_classes(what, "lx_ln_modulate*", "f16", g.words(), cls, neg)
            check_counter(what, "lx_ln_modulate*", ovf, cls)
        elif fmt == "e4m3":
            g, g8 = Guarded(torch.bfloat16, M, D), Guarded(torch.uint8, M, D, xcols=16)
            ops.ln_modulate_fp8_segs(X, segs, g.out, g8.out, D, 16.0)
            sync()
            g.check_outside(what)
            g8.check_outside(what)
            check_classes(what + " Y", "lx_ln_modulate*", "bf16", g.words(), cls, neg)
            check_classes(what + " Y8", "lx_ln_modulate*", "e4m3", g8.words(), cls, neg, 16.0)
        else:
            lo_off = D + 8
            g = Guarded(torch.bfloat16, M, lo_off + D)
            ops.ln_modulate_split_segs(X, segs, g.buf[PAD:PAD + M], D, lo_off)
            sync()
            g.check_outside(what, [(0, D), (lo_off, lo_off + D)])
            w = g.words()
            check_classes(what, "lx_ln_modulate*", "pair", (w[:, :D], w[:, lo_off:]), cls, neg)


GN_INJECT = [(5, BIG, False), (14, BIG, True), (23, PINF, False), (32, NINF, True), (41, CNAN, False)]      # (channel, class, negative) of beta


@pytest.mark.parametrize("via", ["beta", "x"])
@pytest.mark.parametrize("shape", [(2, 60, 128, 32), (1, 300, 512, 32)])
@pytest.mark.parametrize("fmt", ["bf16", "f16", "pair"])
def test_groupnorm_stores_by_class(ops, fmt, shape, via):
    B, P, C, G = shape
    for only_nan in (False, True):
        g = torch.Generator(device=DEV).manual_seed(C)
        x = torch.randn(B, P, C, generator=g, device=DEV)
        gamma = 1 + 0.1 * torch.randn(C, generator=g, device=DEV)
        beta = 0.1 * torch.randn(C, generator=g, device=DEV)
        cls = torch.zeros(B, P, C, dtype=torch.int64, device=DEV)
        neg = torch.zeros(B, P, C, dtype=torch.bool, device=DEV)
        if via == "beta":
            for c, k, n in GN_INJECT:
                if only_nan and k != CNAN:
                    continue
                beta[c] = class_value(k, n)
                cls[:, :, c], neg[:, :, c] = k, n
        else:
            cg = C // G
            # a NaN makes the group's sums, its mean and so every output of the group a NaN. A +inf makes the mean +inf and the variance
            # inf - inf = NaN, which the kernel's max(variance, 0) turns into 0: rstd = 1 / sqrt(eps), finite, and every OTHER element of
            # the group is (x - inf) * rstd * gamma + beta = -inf (gamma > 0 here); the element itself is inf - inf = NaN
            assert bool((gamma > 0).all())
            for (b, p, c), k in (((0, 7, 3), PINF), ((B - 1, P - 1, C - 2), CNAN)):
                if only_nan and k != CNAN:
                    continue
                x[b, p, c] = class_value(k, False)
                grp = slice(c // cg * cg, (c // cg + 1) * cg)
                cls[b, :, grp] = CNAN if k == CNAN else NINF
                neg[b, :, grp] = k != CNAN
                cls[b, p, c] = CNAN
        what = f"groupnorm {fmt} {shape} via {via}{' (NaN only)' if only_nan else ''}"
        cls2, neg2 = cls.view(B * P, C), neg.view(B * P, C)
        if fmt == "pair":
            lo_off = C + 8
            o = Guarded(torch.bfloat16, B * P, lo_off + C)
            ops.groupnorm_silu_split(x, gamma, beta, o.buf[PAD:PAD + B * P], lo_off, groups=G, silu=False)
            sync()
            o.check_outside(what, [(0, C), (lo_off, lo_off + C)])
            w = o.words()
            check_classes(what, "lx_groupnorm_silu*", "pair", (w[:, :C], w[:, lo_off:]), cls2, neg2)
            continue
        dt = torch.float16 if fmt == "f16" else torch.bfloat16
        buf = torch.empty(B * P + 2 * PAD, C, dtype=dt, device=DEV)              # (y is contiguous: sentinel rows above and below)
        buf.view(torch.int16).fill_(SENT[dt])
        y = buf[PAD:PAD + B * P].view(B, P, C)
        if fmt == "f16":
            ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.groupnorm_silu_f16(x, gamma, beta, y, groups=G, silu=False, f16_ovf=ovf)
        else:
            ops.groupnorm_silu(x, gamma, beta, y, groups=G, silu=False)
        sync()
        wb = words_of(buf)
        assert bool((wb[:PAD] == SENT[dt]).all()) and bool((wb[PAD + B * P:] == SENT[dt]).all()), f"{what}: wrote outside y"
        check_classes(what, "lx_groupnorm_silu*", fmt, wb[PAD:PAD + B * P], cls2, neg2)
        if fmt == "f16":
            check_counter(what, "lx_groupnorm_silu*", ovf, cls)


# ---- attention O: finite classes only (CONTRACT: no contract for NaN / +-inf operands). A V image whose whole d-column is the constant c
# makes O of that column c times (sum of the stored probabilities / their fp32 sum): c to within the probabilities' rounding and O's own.
ATTN_LENS, ATTN_B, ATTN_H = (16, 16, 16), 2, 3
# (head, d) -> c. "big" launches hold columns beyond fp16's range, "small" ones none. The e4m3 kernel's V bytes reach +-448: its columns are
# +-448 and +-192 under a V descale of 200 (+-89600, +-38400).
ATTN_COLS = {"big": {(0, 5): 7e4, (1, 77): -7e4, (2, 127): 3e4, (0, 64): -3e4}, "small": {(2, 127): 3e4, (0, 64): -3e4}}
E4M3_V_DESCALE = 200.0
# how far O may lie from c, relatively. 16-bit probabilities: each is rounded to bf16 (2^-9), so is O (2^-9), the fp32 sums over 48 keys add
# less than 2^-17: within 2^-8 + 2^-17 < 2^-7 (an ulp of bf16 at the top of a binade). e4m3 probabilities: bytes of 3 significand bits taken
# as the chord of 2^f over a mantissa step (include/lx.h LX_ATTN_P_EXP2): each within 2^-3 of its value, so O within 2^-3 + 2^-9 < 0.15.
ATTN_REL = {"16": 2.0 ** -7, "e4m3": 0.15}


def attn_launch(ops, kernel, cols, o_dtype):
    import ctypes
    from tests.test_kernels_gpu import _qkv_buffer, _segments
    B, H, lens = ATTN_B, ATTN_H, ATTN_LENS
    D = H * 128
    row0, vt0, vt_len = _segments(B, lens)
    buf = _qkv_buffer(B, lens, H, seed=11)
    M = buf.shape[0]
    for (h, d), c in cols.items():
        if kernel == "e4m3":
            c = {7e4: 448.0, 3e4: 192.0}[abs(c)] * (1 if c > 0 else -1)
        buf[:, D + h * 128 + d] = c
        assert float(buf[0, D + h * 128 + d]) != 0
    one = torch.ones(128, device=DEV)
    f16 = o_dtype == torch.float16
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    g = Guarded(o_dtype, M, D)
    of = ops.ATTN_O_F16 if f16 else 0
    kw = dict(o_col=0, B=B, H=H, seg_row0=row0, seg_len=list(lens), seg_vt0=vt0)
    if kernel == "e4m3":
        Q8 = torch.zeros(M, D, dtype=torch.uint8, device=DEV)
        K8 = torch.zeros_like(Q8)
        VT8 = torch.zeros(B, H, 128, vt_len, dtype=torch.uint8, device=DEV)
        ops.qkv_prep_fp8_segs(buf, 2 * D, 0, D, [(row0[s], L, vt0[s], None, None, None, None) for s, L in enumerate(lens)], B, H, Q8, K8, VT8)
        d = ops._attn_desc(Q8, K8, VT8, g.out, 0, 0, 0, B, H, row0, list(lens), vt0, None, None)
        d.flags, d.f16_ovf = of, ovf.data_ptr() if f16 else None
        ops.check(ops.lib.lx_attn_fwd_fp8(ctypes.byref(d), 1.0 / (ops.FP8_Q_SCALE * ops.FP8_K_SCALE), E4M3_V_DESCALE / ops.FP8_V_SCALE,
                                          torch.cuda.current_stream().cuda_stream), "lx_attn_fwd_fp8")
    else:
        log2 = kernel in ("bounded", "4wave")
        wq, wk = (one * ops.Q_LOG2_FACTOR, one) if log2 else (None, None)
        VT = torch.zeros(B, H, 128, vt_len, dtype=torch.bfloat16, device=DEV)
        ops.qkv_prep_segs(buf, 2 * D, 0, D, [(row0[s], L, vt0[s], wq, wk, None, None) for s, L in enumerate(lens)], B, H, VT)
        if kernel == "masked":
            S = sum(lens)
            mask = torch.rand(S, S, generator=torch.Generator().manual_seed(3)) < 0.6
            mask |= torch.eye(S, dtype=torch.bool)                      # every query keeps a key: no all-masked (exactly zero) rows
            ops.attn_fwd_masked(buf, buf, VT, g.out, mask.to(DEV), q_col=2 * D, k_col=0, flags=of, f16_ovf=ovf if f16 else None, **kw)
        else:
            flags = {"8wave": 0, "bounded": ops.ATTN_Q_LOG2 | ops.ATTN_BOUNDED | ops.ATTN_INVARIANT,
                     "4wave": ops.ATTN_Q_LOG2 | ops.ATTN_BOUNDED | ops.ATTN_PREFER_4WAVE}[kernel]
            ops.attn_fwd(buf, buf, VT, g.out, q_col=2 * D, k_col=0, flags=flags | of, f16_ovf=ovf if f16 else None, **kw)
            assert ops.lib.lx_attn_last_kernel() == (2 if kernel == "4wave" else 1), f"{kernel}: lx_attn_fwd launched kernel {ops.lib.lx_attn_last_kernel()}"
    sync()
    g.check_outside(f"attention {kernel}")
    return g, int(ovf)


@pytest.mark.parametrize("kernel", ["8wave", "bounded", "4wave", "masked", "e4m3"])
def test_attention_o_store_by_class(ops, kernel):
    rel = ATTN_REL["e4m3" if kernel == "e4m3" else "16"]
    D = ATTN_H * 128
    for which, cols in ATTN_COLS.items():
        for o_dtype in (torch.bfloat16, torch.float16):
            fmt = "f16" if o_dtype == torch.float16 else "bf16"
            row = CONTRACT[("lx_attn_fwd* O", fmt)]
            what = f"attention {kernel} O {fmt}, {which} columns"
            g, ovf = attn_launch(ops, kernel, cols, o_dtype)
            w = g.words()
            fin = ~is_nan_word(fmt, w) & ((w & 0x7F80) != 0x7F80 if fmt == "bf16" else (w & 0x7C00) != 0x7C00)
            assert bool(fin.all()), f"{what}: {int((~fin).sum())} outputs are not finite"
            val = sf.decode(fmt, w)
            chosen = torch.zeros(D, dtype=torch.bool, device=DEV)
            for (h, d), c in cols.items():
                if kernel == "e4m3":
                    c = {7e4: 448.0, 3e4: 192.0}[abs(c)] * E4M3_V_DESCALE * (1 if c > 0 else -1)
                else:
                    c = float(torch.tensor(c).to(torch.bfloat16))           # the V image holds bf16(c)
                col = val[:, h * 128 + d]
                chosen[h * 128 + d] = True
                if fmt == "f16" and abs(c) * (1 - rel) > sf.F16_MAX:
                    assert row["beyond"] == "max"
                    want = MAXW["f16"] | (SIGN["f16"] if c < 0 else 0)
                    assert bool((w[:, h * 128 + d] == want).all()), f"{what}: column {(h, d)} = {c} must be stored as exactly {'-' if c < 0 else ''}65504"
                else:
                    assert abs(c) * (1 + rel) < sf.F16_MAX or fmt == "bf16"
                    err = float(((col - c) / c).abs().max())
                    assert err <= rel, f"{what}: column {(h, d)} = {c} came out {err:.3e} away (relative), more than {rel:.3e}"
            lim = 64 * (E4M3_V_DESCALE if kernel == "e4m3" else 1.0)          # (an average of standard normal values, times the V descale)
            assert bool((val[:, ~chosen].abs() < lim).all()), f"{what}: an output of a random V column is out of proportion"
            if fmt == "f16":
                assert row["counted"] == "beyond"
                assert (ovf > 0) == (which == "big"), f"{what}: f16_ovf = {ovf}"
