"""tests/store_formats.py on the CPU: the reference stores against an independent integer model of round-half-even written from the format
definitions (shift, sticky bits, even rule, subnormal shift; no floating-point cast anywhere), over the full edge sets; and the
exact-accumulator operand generator: every accumulator is an fp32 value and every edge class is there for every probe -- the condition
under which the GPU tests of tests/test_store_formats_gpu.py mean something."""
import pytest
import torch

from tests import store_formats as sf

E4M3_SCALES = (1.0, 16.0, 0.125)


# ------------------------------------------------------------------------------------------------ the integer model
def int_round(fmt, xw):
    """fp32 words (finite) -> words of fmt without the sign, IEEE round half to even; past the largest finite: the inf code (e4m3: 0x7f)"""
    eb, mb, bias = sf.FORMATS[fmt]
    xw = xw.to(torch.int64)
    E, M = (xw >> 23) & 0xFF, xw & 0x7FFFFF
    sig = torch.where(E > 0, M | (1 << 23), M)                    # value = sig * 2^e2
    e2 = E.clamp_min(1) - 127 - 23
    lead = torch.zeros_like(sig)                                  # position of sig's leading bit (0 for sig = 0)
    for k in range(1, 24):
        lead += (sig >> k > 0).to(torch.int64)
    te = (lead + e2).clamp_min(1 - bias)                          # the exponent the target encodes the value at (subnormals: emin)
    shift = te - mb - e2                                          # bits of sig below the target's last place
    assert int(shift.min()) >= 1
    shift = shift.clamp_max(40)                                   # sig < 2^24: from 25 on, everything is below half a quantum
    keep, rem, half = sig >> shift, sig & ((1 << shift) - 1), 1 << (shift - 1)
    keep = keep + ((rem > half) | ((rem == half) & (keep & 1 == 1))).to(torch.int64)
    carry = keep == 1 << (mb + 1)                                 # rounded up into the next binade
    keep = torch.where(carry, keep >> 1, keep)
    te = torch.where(carry, te + 1, te)
    words = torch.where(keep < (1 << mb), keep, ((te + bias) << mb) | (keep - (1 << mb)))
    top = 0x7F if fmt == "e4m3" else ((1 << eb) - 1) << mb
    return torch.where(words >= top, torch.full_like(words, top), words)


def split_words(xw):
    xw = xw.to(torch.int64)
    sign, E, M = xw >> 31 & 1, (xw >> 23) & 0xFF, xw & 0x7FFFFF
    return sign, (E == 0xFF) & (M == 0), (E == 0xFF) & (M != 0)


def sources():
    yield "bf16 edges", sf.edge_set("bf16")
    yield "f16 edges", sf.edge_set("f16")
    for s in E4M3_SCALES:
        yield f"e4m3 edges at scale {s}", sf.edge_set("e4m3", s)
    yield "all bf16 words", sf.bf16_words_as_f32_words(sf.all_bf16_words())


SOURCES = dict(sources())


def test_edge_sets_hold_what_they_promise():
    for fmt, n_sub in (("bf16", 127), ("f16", 1023), ("e4m3", 7)):
        assert sf.n_subnormals(fmt) == n_sub
    for fmt, lo, hi in (("bf16", 1.9e5, 2.1e5), ("f16", 1.8e5, 2.1e5)):
        assert lo < sf.edge_set(fmt).numel() < hi
    x = sf.f32_from_bits(sf.edge_set("f16")).double()
    for v in (65504.0, 65520.0, 65536.0, float.fromhex("0x1.ffdffep+15"), float.fromhex("0x1.ffe002p+15"), 2.0 ** -24, 2.0 ** -25, 1023 * 2.0 ** -24):
        assert bool((x == v).any()) and bool((x == -v).any()), v
    x = sf.f32_from_bits(sf.edge_set("e4m3", 16.0)).double()
    for v in (448.0, 464.0, 480.0, 2.0 ** -9, 2.0 ** -10, 7 * 2.0 ** -9):
        assert bool((x == v / 16).any()) and bool((x == -v / 16).any()), v
    x = sf.f32_from_bits(sf.edge_set("bf16")).double()
    big = float.fromhex("0x1.fep+127")
    for v in (big, big + 2.0 ** 119, 2.0 ** -133, 2.0 ** -134, 127 * 2.0 ** -133, 2.0 ** -149, float("inf"), 0.0):
        assert bool((x == v).any()) and bool((x == -v).any()), v
    for name, w in SOURCES.items():
        if "edges" in name:
            assert int(torch.isnan(sf.f32_from_bits(w)).sum()) == 3, name
            assert bool((w == sf.PAYLOAD_NAN).any()) and bool((w == sf.NEG_NAN).any()) and bool((w == 0x80000000).any())


@pytest.mark.parametrize("name", list(SOURCES))
def test_reference_bf16_is_the_integer_model(name):
    xw = SOURCES[name]
    sign, inf, nan = split_words(xw)
    want = torch.where(inf, torch.full_like(xw, 0x7F80), int_round("bf16", torch.where(inf | nan, torch.zeros_like(xw), xw))) | (sign << 15)
    got, got_nan = sf.ref_bf16(xw)
    assert torch.equal(got_nan, nan)
    assert torch.equal(got[~nan], want[~nan])
    assert bool(sf.same16("bf16", got, want, nan).all())


@pytest.mark.parametrize("name", list(SOURCES))
def test_reference_f16_is_the_integer_model_saturated(name):
    xw = SOURCES[name]
    sign, inf, nan = split_words(xw)
    w = int_round("f16", torch.where(inf | nan, torch.zeros_like(xw), xw))
    w = torch.where(inf | (w == 0x7C00), torch.full_like(w, 0x7BFF), w) | (sign << 15)       # IEEE rounding, then inf -> 65504
    got, got_nan = sf.ref_f16_sat(xw)
    assert torch.equal(got_nan, nan)
    assert torch.equal(got[~nan], w[~nan])
    assert not bool(((got[~nan] & 0x7FFF) >= 0x7C00).any()), "an inf left the saturating reference"
    # counted: |x| > 65504 on the words themselves
    mag = xw & 0x7FFFFFFF
    assert torch.equal(sf.counted_f16(xw), (mag > 0x477FE000) & ~nan)


@pytest.mark.parametrize("scale", E4M3_SCALES + (0.3,))
@pytest.mark.parametrize("name", list(SOURCES))
def test_reference_e4m3_is_the_integer_model_clamped(name, scale):
    xw = SOURCES[name]
    yw = sf.bits_from_f32(sf.f32_from_bits(xw) * torch.tensor(scale, dtype=torch.float32))        # the fp32 product, as the kernels form it
    sign, inf, nan = split_words(yw)
    w = int_round("e4m3", torch.where(inf | nan, torch.zeros_like(yw), yw))
    w = torch.where(inf | (w >= 0x7F), torch.full_like(w, 0x7E), w) | (sign << 7)                  # rounding, then saturation at 448
    got, got_nan = sf.ref_e4m3(xw, scale)
    assert torch.equal(got_nan, nan)
    assert torch.equal(got[~nan], w[~nan])


@pytest.mark.parametrize("name", list(SOURCES))
def test_reference_pair_is_two_integer_roundings(name):
    xw = SOURCES[name]
    hi, lo, ok = sf.ref_pair(xw)
    sign, inf, nan = split_words(xw)
    whi = int_round("bf16", torch.where(inf | nan, torch.zeros_like(xw), xw)) | (sign << 15)
    fin = ~inf & ~nan & ((whi & 0x7FFF) < 0x7F80)
    assert torch.equal(ok, fin)
    assert torch.equal(hi[ok], whi[ok])
    # x - hi in integers: both are multiples of 2^-149 below 2^128
    x = sf.f32_from_bits(xw[ok]).double()
    d = x - sf.decode("bf16", whi[ok])
    dw = sf.bits_from_f32(d.float())
    assert torch.equal(d.float().double(), d), "x - bf16(x) is an fp32 value"
    wlo = int_round("bf16", dw & 0x7FFFFFFF) | (dw >> 31 << 15)
    assert torch.equal(lo[ok] & 0x7FFF, wlo & 0x7FFF)
    nz = (wlo & 0x7FFF) != 0
    assert torch.equal(lo[ok][nz], wlo[nz])
    # hi + lo carries x to 16 significand bits
    err = (sf.decode("bf16", hi[ok]) + sf.decode("bf16", lo[ok]) - x).abs()
    assert bool((err <= x.abs() * 2.0 ** -16 + 2.0 ** -134).all())


# ------------------------------------------------------------------------------------------------ the operand generator
# (operand format, target format, target scale, pair columns?) -> the classes the probe cannot contain, and why
# the probes whose operand format holds every value of the target (the others: fewer significand bits, or the rows are t / scale)
OPERANDS_HOLD_TARGET = {("bf16", "bf16", 1.0, False), ("bf16", "bf16", 1.0, True), ("f16", "f16", 1.0, False)}
PROBES = {
    ("bf16", "bf16", 1.0, False): (),
    ("bf16", "bf16", 1.0, True): (),
    ("f16", "f16", 1.0, False): (),
    ("e4m3", "e4m3", 0.5, False): (),
    ("bf16", "e4m3", 1.0, False): (),       # the e4m3 V^T bytes of an LX_EPI_QKV launch
    # e4m3 operands reach +-448 * 2 at most and hold no bf16 subnormal: the bf16 store of an fp8 launch sees neither end of bf16's range
    ("e4m3", "bf16", 1.0, False): ("target subnormal", "beyond range", "tie at the top"),
}
SHAPES = tuple((M or 6913, N) for M, N in sf.PROBE_SHAPES) + ((20, 2040),)


@pytest.mark.parametrize("probe", list(PROBES))
def test_probe_accumulators_are_exact_and_hold_every_class(probe):
    opfmt, target, scale, pair = probe
    a0, a1 = sf.probe_rows(opfmt, target, scale)
    for v in (a0, a1):
        assert bool(sf._representable(opfmt, v).all())
    seen = {}
    row0 = 0
    for M, N in SHAPES:
        a0, a1, w0, w1 = sf.gemm_probe(opfmt, target, M, N, row0, scale, pair)
        row0 += M
        for v in (w0, w1):
            assert bool(sf._representable(opfmt, v).all())
        acc = sf.probe_acc(a0, a1, w0, w1)
        for part in (a0[:, None] * w0[None, :], a1[:, None] * w1[None, :], acc):
            assert torch.equal(part.float().double(), part), "not an fp32 value"
        for k, m in sf.edge_classes(target, acc, scale).items():
            seen[k] = seen.get(k, 0) + int(m.sum())
        if pair:
            hi, lo, ok = sf.ref_pair(sf.bits_from_f32(acc.float()))
            d = acc - sf.decode("bf16", hi)
            inexact = ok & (sf.decode("bf16", lo) != d)
            seen["lo rounds"] = seen.get("lo rounds", 0) + int(inexact.sum())
            seen["lo rounds, truncation differs"] = seen.get("lo rounds, truncation differs", 0) + \
                int((inexact & (sf.decode("bf16", lo).abs() > d.abs())).sum())
    for k, n in seen.items():
        if k in PROBES[probe]:
            assert n == 0, f"{probe}: class '{k}' is there after all: take it off the exclusion list"
        else:
            assert n > 0, f"{probe}: no accumulator of class '{k}'"
    # the row list covers what is asked of it, as far as the operand format holds it
    eb, mb, bias = sf.FORMATS[target]
    t = sf.probe_rows(opfmt, target, scale)[0] * scale
    assert bool((t > 0).any()) and bool((t < 0).any())
    if probe in OPERANDS_HOLD_TARGET:
        for e in (1 - bias, 0, int(sf.finite_codes(target)[-1] >> mb) - bias):
            n = int(((t >= 2.0 ** e) & (t < 2.0 ** (e + 1))).sum())
            assert n == 2 ** mb, (probe, e, n)
        assert int(((t > 0) & (t < 2.0 ** (1 - bias))).sum()) == sf.n_subnormals(target)
        assert bool((t == sf.max_finite(target)).any())


def test_f16_probe_has_a_launch_without_overflow_and_one_with():
    """The fp16 counter's two cases rest on the probe's layout: p3's rows hold nothing beyond 65504 (its counter must stay 0), p1's do."""
    for i, want in ((3, False), (1, True)):
        M, N = sf.PROBE_SHAPES[i]
        acc = sf.probe_acc(*sf.gemm_probe("f16", "f16", M, N, sf.PROBE_ROW0[i]))
        assert bool(sf.counted_f16(sf.f32_words_from_exact(acc)).any()) == want, i
    assert sf.PROBE_SHAPES[0][0] is None      # p0's rows follow from the CU count: what it holds is computed where it runs
