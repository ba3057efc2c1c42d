"""Edge sets, reference stores and exact-accumulator GEMM operands for the bit-for-bit tests of the 16- and 8-bit stores
(tests/test_store_formats_ref_cpu.py pins this module on the CPU, tests/test_store_formats_gpu.py holds the kernels to it).

fp32 values travel as BIT PATTERNS (int64 tensors holding the 32-bit word) so that NaN payloads, the sign of zero and subnormals survive
every hop; the references work on whichever device their argument lives on. The reference stores are written in float64 arithmetic
(quantum of the binade, floor and a half-to-even rule; powers of two built from their bits) -- the CPU test compares them with an integer shift / sticky / even-rule model.

Formats: (exponent bits, stored significand bits, bias); e4m3 is the OCP "fn" flavour (no inf, one NaN code 0x7f, largest finite 448)."""
import torch

FORMATS = {"bf16": (8, 7, 127), "f16": (5, 10, 15), "e4m3": (4, 3, 7)}
F16_MAX, E4M3_MAX = 65504.0, 448.0
NAN16 = {"bf16": 0x7FC0, "f16": 0x7E00}
QUIET_NAN, PAYLOAD_NAN, NEG_NAN = 0x7FC00000, 0x7FA12345, 0xFFC00000
FLT_MAX_BITS, MIN_SUB_BITS, MAX_SUB_BITS, INF_BITS = 0x7F7FFFFF, 0x00000001, 0x007FFFFF, 0x7F800000


# ------------------------------------------------------------------------------------------------ bit patterns <-> values
def f32_from_bits(b):
    """int64 words -> float32 values (same device)"""
    b = b.to(torch.int64) & 0xFFFFFFFF
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(torch.float32)


def bits_from_f32(x):
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def f64_from_f32_words(w):
    """fp32 words -> float64 values through integers (no conversion instruction: a device that flushes fp32 subnormals cannot)"""
    w = w.to(torch.int64) & 0xFFFFFFFF
    E, M = (w >> 23) & 0xFF, w & 0x7FFFFF
    v = torch.where(E > 0, M | (1 << 23), M).double() * pow2(E.clamp_min(1) - 150)
    v = torch.where(E == 0xFF, torch.where(M == 0, torch.full_like(v, float("inf")), torch.full_like(v, float("nan"))), v)
    return torch.where(w >> 31 == 1, -v, v)


def f32_words_from_exact(v):
    """finite float64 values that ARE fp32 values -> their fp32 words, through integers"""
    a = v.abs()
    e = floor_log2(a).clamp_min(-126)
    n = (a / pow2(e - 23)).to(torch.int64)                       # 24-bit significand (subnormals: fewer)
    w = torch.where(n >= 1 << 23, ((e + 127) << 23) | (n - (1 << 23)), n)
    return w | (torch.signbit(v).to(torch.int64) << 31)


def bits16(t):
    """a bf16 / fp16 tensor -> its words as int64"""
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def pow2(k):
    """2^k as float64, built from its bits (k an int64 tensor, -1022 <= k <= 1023): exact on every device"""
    return ((k.to(torch.int64) + 1023) << 52).view(torch.float64)


def floor_log2(a):
    """floor(log2 a) of positive normal float64 values, from the exponent field (0 for a = 0)"""
    return torch.where(a > 0, ((a.contiguous().view(torch.int64) >> 52) & 0x7FF) - 1023, torch.zeros_like(a, dtype=torch.int64))


def round_half_even(v):
    """non-negative float64 -> nearest integer, ties to even; floor and compare only (no device rounding mode enters)"""
    n = torch.floor(v)
    f = v - n
    return n + ((f > 0.5) | ((f == 0.5) & (torch.fmod(n, 2.0) == 1.0))).double()


def decode(fmt, bits):
    """words of a narrow format -> float64 values (NaN codes -> NaN, bf16 / fp16 infinities -> inf)"""
    eb, mb, bias = FORMATS[fmt]
    bits = bits.to(torch.int64)
    s = (bits >> (eb + mb)) & 1
    e = (bits >> mb) & (2 ** eb - 1)
    m = bits & (2 ** mb - 1)
    sub = m.double() * 2.0 ** (1 - bias - mb)
    nor = (1.0 + m.double() * 2.0 ** -mb) * pow2(e - bias)
    v = torch.where(e == 0, sub, nor)
    if fmt == "e4m3":
        v = torch.where((e == 15) & (m == 7), torch.full_like(v, float("nan")), v)
    else:
        v = torch.where(e == 2 ** eb - 1, torch.where(m == 0, torch.full_like(v, float("inf")), torch.full_like(v, float("nan"))), v)
    return torch.where(s == 1, -v, v)


def finite_codes(fmt):
    """the non-negative finite codes of a format, ascending (their values ascend with them)"""
    eb, mb, _ = FORMATS[fmt]
    top = 0x7E if fmt == "e4m3" else ((2 ** eb - 1) << mb) - 1
    return torch.arange(0, top + 1, dtype=torch.int64)


def max_finite(fmt):
    return float(decode(fmt, finite_codes(fmt)[-1:])[0])


def n_subnormals(fmt):
    return 2 ** FORMATS[fmt][1] - 1


# ------------------------------------------------------------------------------------------------ edge sets (fp32 inputs, as words)
def _neighbours(x32):
    """x and its fp32 predecessor and successor"""
    return torch.cat([torch.nextafter(x32, torch.full_like(x32, -float("inf"))), x32, torch.nextafter(x32, torch.full_like(x32, float("inf")))])


def edge_set(fmt, scale=1.0):
    """fp32 inputs (words, int64) at which a store to `fmt` of x * scale can go wrong; scale a power of two (1 for bf16 / fp16).
    Both signs of: every midpoint between adjacent finite target values with its fp32 neighbours (the lowest: 0 | smallest subnormal),
    every target subnormal, the top of the range (largest, largest + half an ulp, largest + an ulp, each with its fp32 neighbours), 0,
    the smallest and largest fp32 subnormals, FLT_MAX, inf; then a quiet NaN, a NaN with a payload and a negative NaN."""
    v = decode(fmt, finite_codes(fmt))
    mid = (v[:-1] + v[1:]) / 2 / scale
    assert torch.equal(mid.float().double(), mid), "a midpoint is not an fp32 value"
    top, ulp = v[-1], v[-1] - v[-2]
    parts = [_neighbours(mid.float()),
             (v[1:n_subnormals(fmt) + 1] / scale).float(),
             _neighbours((torch.stack([top, top + ulp / 2, top + ulp]) / scale).float())]
    pos = torch.cat(parts)
    words = bits_from_f32(torch.cat([pos, -pos]))
    special = []
    for w in (0, MIN_SUB_BITS, MAX_SUB_BITS, FLT_MAX_BITS, INF_BITS):
        special += [w, w | 0x80000000]
    special += [QUIET_NAN, PAYLOAD_NAN, NEG_NAN]
    return torch.cat([words, torch.tensor(special, dtype=torch.int64)])


def all_bf16_words():
    """all 65536 bf16 patterns (a source set for the converters that read bf16)"""
    return torch.arange(0, 65536, dtype=torch.int64)


def bf16_words_as_f32_words(w):
    return w.to(torch.int64) << 16


# ------------------------------------------------------------------------------------------------ reference stores
def _rne(fmt, y):
    """float64 y (finite or inf, no NaN) -> (words of fmt without the sign, rounded value); beyond the largest finite: the inf code
    (bf16, fp16) -- callers of e4m3 clamp first"""
    eb, mb, bias = FORMATS[fmt]
    emin = 1 - bias
    a = y.abs()
    fin = torch.isfinite(a)
    a0 = torch.where(fin, a, torch.zeros_like(a))
    e = floor_log2(a0)
    e = torch.where(a0 == 0, torch.full_like(e, emin), e).clamp_min(emin)
    q = pow2(e - mb)                                                 # the quantum of a's binade in fmt
    n = round_half_even(a0 / q)                                      # a0 / q is exact (a power-of-two divisor)
    r = n * q
    # encode: n in [0, 2^(mb+1)]; 2^(mb+1) is the next binade's 1.0
    up = n >= 2.0 ** (mb + 1)
    e = torch.where(up, e + 1, e)
    n = torch.where(up, n / 2, n).to(torch.int64)
    words = torch.where(n < 2 ** mb, n, ((e + bias) << mb) | (n - 2 ** mb))
    inf_code = (2 ** eb - 1) << mb
    over = ~fin | (words >= inf_code) if fmt != "e4m3" else torch.zeros_like(fin)
    words = torch.where(over, torch.full_like(words, inf_code), words)
    r = torch.where(over, torch.full_like(r, float("inf")), r)
    return words, r


def _signed(fmt, words, neg):
    eb, mb, _ = FORMATS[fmt]
    return words | (neg.to(torch.int64) << (eb + mb))


def ref_bf16(xw):
    """fp32 words -> (bf16 words, NaN mask): round to nearest even, overflow to +-inf; where the mask is set the word is a quiet NaN of
    the input's sign and only the class is specified"""
    x = f64_from_f32_words(xw)
    nan = torch.isnan(x)
    w, _ = _rne("bf16", torch.where(nan, torch.zeros_like(x), x))
    neg = (xw.to(torch.int64) >> 31) & 1 == 1
    return torch.where(nan, _signed("bf16", torch.full_like(w, NAN16["bf16"]), neg), _signed("bf16", w, neg)), nan


def ref_f16_sat(xw):
    """fp32 words -> (fp16 words, NaN mask): clamped to +-65504 (so +-inf too), then round to nearest even; NaN is a class of its own"""
    x = f64_from_f32_words(xw)
    nan = torch.isnan(x)
    w, _ = _rne("f16", torch.where(nan, torch.zeros_like(x), x).clamp(-F16_MAX, F16_MAX))
    neg = (xw.to(torch.int64) >> 31) & 1 == 1
    return torch.where(nan, torch.full_like(w, NAN16["f16"]), _signed("f16", w, neg)), nan


def counted_f16(xw):
    """what a saturating fp16 store reports: |x| > 65504 BEFORE rounding (+-inf included; 65519.99 rounds to 65504 and still counts)"""
    x = f32_from_bits(xw)
    return x.abs() > F16_MAX


def ref_e4m3(xw, scale):
    """fp32 words -> (e4m3 bytes of fp32(x * scale) clamped to +-448, NaN mask)"""
    y = (f32_from_bits(xw) * torch.tensor(scale, dtype=torch.float32, device=xw.device))
    nan = torch.isnan(y)
    neg = torch.signbit(y)
    yd = torch.where(nan, torch.zeros_like(y), y).clamp(-E4M3_MAX, E4M3_MAX)
    yd = f64_from_f32_words(bits_from_f32(yd))
    w, _ = _rne("e4m3", yd)
    return torch.where(nan, torch.full_like(w, 0x7F), _signed("e4m3", w, neg)), nan


def ref_pair(xw):
    """fp32 words -> (hi words, lo words, mask of inputs whose pair is specified): hi = bf16(x), lo = bf16(x - hi); the difference is an
    fp32 value (the CPU test checks it), so no rounding enters before lo's. The pair is specified for finite x that bf16 does not
    overflow; x = hi gives lo = +0."""
    hi, nan = ref_bf16(xw)
    h = decode("bf16", hi)
    ok = ~nan & torch.isfinite(h)
    d = torch.where(ok, f64_from_f32_words(xw) - h, torch.zeros_like(h))
    lo, _ = _rne("bf16", d)
    return hi, _signed("bf16", lo, d < 0), ok


def same16(fmt, got, want, want_nan):
    """got words == want words, NaN by class (any NaN code)"""
    eb, mb, _ = FORMATS[fmt]
    got_nan = ((got >> mb) & (2 ** eb - 1) == 2 ** eb - 1) & (got & (2 ** mb - 1) != 0)
    return torch.where(want_nan, got_nan, got == want)


# ------------------------------------------------------------------------------------------------ exact-accumulator GEMM operands
# acc[m, n] = a0[m] w0[n] + a1[m] w1[n]: a0 a value of the store's target format that the operand format holds, a1 = 2^A1_SHIFT times half
# an ulp (target format) of a0, w0 a power of two (1, or LIFT in the last quarter of the columns), w1 = w0 * v * 2^-A1_SHIFT with v from
# VARIANTS (period 5 along n: coprime to the 8 lanes of a vector store). Every product has at most 16 significand bits and the sum is
# t (1 + v / 2^(mb+1)) L: exact in fp32 in any order.
OPERAND_SIG = {"bf16": 8, "f16": 11, "e4m3": 4}
A1_SHIFT = {"bf16": 8, "f16": 10, "e4m3": 3}
# just below / just above the tie: the operand format's neighbours of 1
VARIANTS = {"bf16": (0.0, 1.0, 1 - 2.0 ** -8, 1 + 2.0 ** -7, -1.0), "f16": (0.0, 1.0, 1 - 2.0 ** -10, 1 + 2.0 ** -9, -1.0),
            "e4m3": (0.0, 1.0, 1 - 2.0 ** -4, 1 + 2.0 ** -3, -1.0)}
# the pair store: w0 = 1 - 2^-8 gives x 16 significand bits, w1 adds 8 more below them, so x - bf16(x) needs a rounding of its own
PAIR_EXTRA = ((1 - 2.0 ** -8, (1 + 2.0 ** -7) * 2.0 ** -7), (1 - 2.0 ** -8, -(1 - 2.0 ** -7) * 2.0 ** -7))
# (bf16: twice the top binade is past fp32 as well; its largest value plus more than half an ulp is what goes beyond the range)
LIFT = {"bf16": 1.0, "f16": 2.0, "e4m3": 2.0}        # by TARGET format


def _representable(opfmt, v):
    """float64 values the operand format holds exactly"""
    w, r = _rne(opfmt, v)
    return (r == v.abs()) & torch.isfinite(r) & (v.abs() <= max_finite(opfmt))


def probe_rows(opfmt, target, target_scale=1.0):
    """(a0, a1) float64: the rows of a probe for a store to `target` (of acc * target_scale) from `opfmt` operands. Target codes: every
    significand at the lowest normal exponent, at 1.0 and at the highest exponent; every exponent at significands 0, 1, 2 and all-ones;
    every subnormal; the top of the range; both signs -- those of them that the operand format holds together with their a1."""
    eb, mb, bias = FORMATS[target]
    codes = finite_codes(target)
    e, m = codes >> mb, codes & (2 ** mb - 1)
    emax = int(e.max())
    keep = (e == 0) | (e == 1) | (e == bias) | (e == emax) | (m <= 2) | (m == 2 ** mb - 1) | (target == "e4m3")   # (e4m3: all 126)
    codes = codes[keep & (codes > 0)]
    t = decode(target, codes) / target_scale
    ee = (codes >> mb).clamp_min(1)
    hu = pow2(ee - bias - mb - 1) / target_scale
    a1 = hu * 2.0 ** A1_SHIFT[opfmt]
    ok = _representable(opfmt, t) & _representable(opfmt, a1)
    t, a1 = t[ok], a1[ok]
    return torch.cat([t, -t]), torch.cat([a1, a1])


def probe_cols(opfmt, N, pair=False, lift=None):
    """(w0, w1) float64 [N]; lift: the power of two of the last quarter of the columns (default: LIFT of the operand format; gemm_probe passes the target's)"""
    var = [(1.0, v * 2.0 ** -A1_SHIFT[opfmt]) for v in VARIANTS[opfmt]]
    if pair:
        var += [(a, b * 2.0 ** -A1_SHIFT[opfmt] * 2) for a, b in PAIR_EXTRA]
    n = torch.arange(N)
    w0 = torch.tensor([v[0] for v in var], dtype=torch.float64)[n % len(var)]
    w1 = torch.tensor([v[1] for v in var], dtype=torch.float64)[n % len(var)]
    lift = torch.where(n >= N - N // 4, LIFT[opfmt] if lift is None else lift, 1.0).double()
    return w0 * lift, w1 * lift


# the problems of a probe launch (those of tests/test_gemm_tiles_gpu.py's group(); M None: from the device's CU count) and the first row of
# the row list each takes: p3, p2, p1, p0 in that order, so that p3 (641 rows from the bottom of the target's range) holds nothing beyond
# fp16's range -- the launch whose overflow counter must stay 0 -- and p1 reaches the top
PROBE_SHAPES = [(None, 2040), (2303, 776), (1055, 264), (641, 64)]
PROBE_ROW0 = {3: 0, 2: 641, 1: 641 + 1055, 0: 641 + 1055 + 2303}


def gemm_probe(opfmt, target, M, N, row0=0, target_scale=1.0, pair=False, lift=None):
    """a0, a1 [M], w0, w1 [N] (float64, each exactly a value of opfmt): rows row0 ... of the probe's row list, cyclically"""
    a0, a1 = probe_rows(opfmt, target, target_scale)
    idx = (row0 + torch.arange(M)) % a0.numel()
    w0, w1 = probe_cols(opfmt, N, pair, LIFT[target] if lift is None else lift)
    return a0[idx], a1[idx], w0, w1


def probe_acc(a0, a1, w0, w1):
    """the accumulator every element of the launch must hold, in float64"""
    return a0[:, None] * w0[None, :] + a1[:, None] * w1[None, :]


def edge_classes(target, acc, target_scale=1.0):
    """name -> mask over float64 accumulators (exact fp32 values) of the classes a probe has to contain"""
    eb, mb, bias = FORMATS[target]
    y = acc * target_scale
    if target == "e4m3":
        w, r = _rne(target, y.clamp(-E4M3_MAX, E4M3_MAX))
    else:
        w, r = _rne(target, y)
    a = y.abs()
    top = max_finite(target)
    e = floor_log2(a).clamp_min(1 - bias)
    q = pow2(e - mb)
    frac = a / q - torch.floor(a / q)
    inr = a <= top
    tie = (frac == 0.5) & inr
    top_half_ulp = 2.0 ** (int(floor_log2(torch.tensor(top, dtype=torch.float64))) - mb) / 2
    return {"exact": (frac == 0) & inr, "tie to even down": tie & (r < a), "tie to even up": tie & (r > a),
            "just below": (frac > 0.4) & (frac < 0.5) & inr, "just above": (frac > 0.5) & (frac < 0.6) & inr,
            "target subnormal": (a > 0) & (a < 2.0 ** (1 - bias)), "beyond range": a > top, "tie at the top": a == top + top_half_ulp}
