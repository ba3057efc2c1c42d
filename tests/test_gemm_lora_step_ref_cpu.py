"""The arithmetic of the GEMM's LoRA step, restated in torch on the CPU, against the float64 reference tests/test_gemm_lora_plans_gpu.py
holds the kernels to (lora_term64 of tests/test_gemm_tiles_gpu.py), at every (rank, slab count) class that module runs:

  * the restatement -- slabs added in slab order in fp32, t and up each split into bf16 hi + lo, the four cross terms added to an fp32
    product (lora_issue / lora_sum / lora_apply of csrc/gemm8.h, the LoRA step of csrc/gemm4.h) -- stays under the worst-tile bound of
    the fp32 outputs, BOUND[("bf16", "f32")] = 2e-5, with a margin of 5: the bound leaves room for what the step is meant to do;
  * five wrong restatements do not: the slabs past the fourth dropped, the last partial rank block dropped, toff of the second module
    taken as 0, the term added twice -- each at least 100 x the bound in every class where it differs from the right one -- and t_lo
    dropped. The last one cannot reach 100 x: it leaves a relative error of at most 2^-9 = 1.95e-3 in the adapter term alone, below
    100 x 2e-5 whatever the inputs; measured here it is 9 ... 71 x the bound (the adapter term is 0.09 ... 1.34 of the main product's
    rms), and it is asserted to exceed the bound in every class, which is what makes the GPU check fail on it.

Measured: the restatement's worst tile is 3.6e-7 (r = 2, one slab) ... 2.8e-6 (r = 64, seven slabs); the four other wrong restatements
are 4.8e3 ... 5.9e4 x the bound.

So the GPU module's checks bite on these faults without a wrong kernel ever being built. Run with -s for the figures."""
import pytest
import torch

from tests.test_gemm_tiles_gpu import BOUND, lora_term64, tile_worst

M, N, K, MOD_COLS, TOFF_MAX = 300, 776, 1536, 256, 1      # 3 x 4 tiles of 128 x 256: a ragged last tile row, an 8-column last tile column
BOUND_F32 = BOUND[("bf16", "f32")]


def lora_class(R, nsplit, t_col0=0, ldt=None):
    """Adapter inputs of one test class (the keywords of Prob.set_lora): row stride 2 R + 4 unless given, so that every slab row ends in
    columns the step must not read."""
    return dict(R=R, nsplit=nsplit, ldt=2 * R + 4 if ldt is None else ldt, t_col0=t_col0)


def class_id(c):
    return f"r{c['R']}s{c['nsplit']}" + (f"c{c['t_col0']}" if c["t_col0"] else "") + (f"ld{c['ldt']}" if c["ldt"] != 2 * c["R"] + 4 else "")


# the classes of tests/test_gemm_lora_plans_gpu.py
CLASSES_8WAVE = [lora_class(4, 4), lora_class(3, 1), lora_class(4, 5), lora_class(6, 2), lora_class(8, 4, t_col0=1), lora_class(16, 4),
                 lora_class(18, 3), lora_class(64, 4), lora_class(64, 7)]
CLASSES_G4 = [lora_class(2, 1), lora_class(4, 4), lora_class(6, 3), lora_class(8, 4), lora_class(8, 1)]
CLASSES_FALLBACK = [lora_class(5, 2), lora_class(10, 2), lora_class(4, 5), lora_class(8, 4, t_col0=1), lora_class(6, 2, ldt=15)]
CLASSES_SPLIT = [lora_class(4, 4), lora_class(6, 2), lora_class(16, 4), lora_class(16, 5)]
CLASSES_FP8 = [lora_class(4, 4), lora_class(3, 1), lora_class(2, 3)]
CLASSES_PEEL = [lora_class(4, 4), lora_class(6, 2), lora_class(64, 5)]
CLASSES_SHARD = [lora_class(6, 2), lora_class(64, 4)]
RANK_SLABS = sorted({(c["R"], c["nsplit"]) for cs in (CLASSES_8WAVE, CLASSES_G4, CLASSES_FALLBACK, CLASSES_SPLIT, CLASSES_FP8, CLASSES_PEEL,
                                                       CLASSES_SHARD) for c in cs})


def bf16_hi_lo(x):
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def lora_step_f32(main32, slabs, up, R, mod_cols, toff_max, wrong=None):
    """main32 [M, N] fp32 + the adapter term as the kernels compute it. slabs [nsplit, M, >= (toff_max + 1) R] fp32, up [N, R] fp32.
    wrong: None | 'slabs4' | 'partial' | 'toff0' | 'twice' | 't_lo' -- the wrong restatements of the module docstring."""
    ns = slabs.shape[0] if wrong != "slabs4" else min(slabs.shape[0], 4)
    t = slabs[0].clone()
    for s in range(1, ns):                     # (((s0 + s1) + s2) + s3) ... in fp32
        t += slabs[s]
    th, tl = bf16_hi_lo(t)
    uh, ul = bf16_hi_lo(up)
    if wrong == "t_lo":
        tl = torch.zeros_like(tl)
    r_end = R - R % 4 if wrong == "partial" else R
    out = main32.clone()
    Nn = up.shape[0]
    for rep in range(2 if wrong == "twice" else 1):
        for b in range(-(-Nn // mod_cols)):
            m = 0 if wrong == "toff0" else min(b, toff_max) * R
            c = slice(b * mod_cols, min(Nn, (b + 1) * mod_cols))
            for x, w in ((th, uh), (th, ul), (tl, uh), (tl, ul)):          # every product of two bf16 values is exact in fp32
                out[:, c] += x[:, m:m + r_end] @ w[c, :r_end].T
    return out


def differs(wrong, R, nsplit):
    return {"slabs4": nsplit > 4, "partial": R % 4 != 0}.get(wrong, True)


@pytest.fixture(scope="module")
def main():
    """The operands of the GPU module's problems (the same distributions: A ~ N(0, 1), W ~ 0.02 N(0, 1), bias ~ 0.1 N(0, 1), as bf16),
    their float64 product and an fp32 one accumulated over K tiles of 64."""
    g = torch.Generator().manual_seed(7)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    bias = torch.randn(N, generator=g) * 0.1
    y64 = A.double() @ W.double().T + bias.double()
    y32 = torch.zeros(M, N)
    for k0 in range(0, K, 64):
        y32 += A[:, k0:k0 + 64].float() @ W[:, k0:k0 + 64].float().T
    y32 += bias
    return y64, y32


def draw(R, nsplit):
    g = torch.Generator().manual_seed(1000 * R + nsplit)
    slabs = torch.randn(nsplit, M, (TOFF_MAX + 1) * R, generator=g) * 0.5
    up = torch.randn(N, R, generator=g) * 0.1
    return slabs, up


@pytest.mark.parametrize("R,nsplit", RANK_SLABS)
def test_lora_step_restatement_and_its_mutants(main, R, nsplit):
    y64, y32 = main
    slabs, up = draw(R, nsplit)
    term = lora_term64(slabs, up, R, MOD_COLS, TOFF_MAX)
    ref = y64 + term
    ratio = float(term.norm() / (y64 - y64.mean()).norm())
    err, at = tile_worst(lora_step_f32(y32, slabs, up, R, MOD_COLS, TOFF_MAX), ref)
    print(f"\nLORA_STEP_REF r={R} nsplit={nsplit}: adapter term {ratio:.2f} x the main product; restatement worst tile {err:.2e} at {at}", end="")
    assert err < BOUND_F32 / 5, f"r={R} nsplit={nsplit}: the restatement's worst tile at {at}: {err:.3e} >= {BOUND_F32 / 5:.0e}"
    for wrong, factor in (("slabs4", 100), ("partial", 100), ("toff0", 100), ("twice", 100), ("t_lo", 1)):
        if not differs(wrong, R, nsplit):
            continue
        e, _ = tile_worst(lora_step_f32(y32, slabs, up, R, MOD_COLS, TOFF_MAX, wrong=wrong), ref)
        print(f"; {wrong} {e / BOUND_F32:.0f}x", end="")
        assert e > factor * BOUND_F32, f"r={R} nsplit={nsplit}: the wrong restatement '{wrong}' is only {e / BOUND_F32:.1f} x the bound"


def test_lora_reference_modules_and_slabs():
    """lora_term64 against its definition element by element on a small case: the second and later modules read columns [R, 2 R) of t
    (toff_max = 1), every slab counts, the last column block may be partial."""
    g = torch.Generator().manual_seed(3)
    R, ns, n, m = 3, 5, 20, 7
    slabs = torch.randn(ns, m, 2 * R, generator=g)
    up = torch.randn(n, R, generator=g)
    got = lora_term64(slabs, up, R, 8, 1)
    for i in range(m):
        for j in range(n):
            o = R * min(j // 8, 1)
            want = sum(float(slabs[s, i, o + r].double() * up[j, r].double()) for s in range(ns) for r in range(R))
            assert abs(float(got[i, j]) - want) < 1e-12
