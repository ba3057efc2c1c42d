"""The GEMM's LoRA step -- acc += t[m, toff : toff + r] . up[n, :r] -- at every rank and slab count class, under every launch plan that
runs it. Three pieces of code apply the term: the 8-wave kernels' prologue (r <= 4, <= 4 slabs: one batch of loads, vector or element
loads), their epilogue walk (everything else up to r = 64: ranks four at a time, slabs four at a time) and lx_gemm4_kernel's own step
(r in {2, 4, 6, 8}, <= 4 slabs, 8-byte loads, once per tile also where the tile is split over K). The planner of csrc/gemm.hip sends a
launch whose adapter shape lx_gemm4_kernel cannot take to the 8-wave kernels.

Everything here is the harness of tests/test_gemm_tiles_gpu.py with the adapter inputs made per-problem (Prob.set_lora): the plan is
asserted after every launch, C lies inside sentinels, the slabs lie inside NaN sentinels (rows and trailing columns) and must keep their
bits, the worst 128 x 256 tile is held to the format's bound against float64 of the operands the kernel read, and two launches agree bit
for bit. The launches are the tile module's 'main' group (K = 1536, NCU + 17 ... 24 tiles) and its 'long' group for the split-all forms:
p1 (2303 x 776, fp32 store, modules of 256 columns, toff_max = 1) has rows in both tile heights of the mixed plan and a ragged last tile
row among the split tiles; p3 (641 x 64) is a gated residual WITH the adapter term here -- one partial column tile, up rows clamped -- and
is also held, element by element, to the fp32 chain bound of tests/test_lora_wide_gpu.py::test_gemm_lora_step_ranks.

That these checks fail on a lost slab, a lost rank block, a doubled term, a wrong toff or a dropped t_lo is shown on the CPU by
tests/test_gemm_lora_step_ref_cpu.py; the same restatement, evaluated on p1's operands, is reported next to each 16-bit arm's figure
(profiles/gemm_lora_plans.txt). Run with -s for the table; LX_GEMM_TILES_REPORT=<file> appends it as JSON lines.

Measured on MI355X (256 CUs): the module's 174 cases take 4.4 s."""
import json
import os

import pytest
import torch

from tests.helpers import U24, gamma_n
from tests.test_gemm_lora_step_ref_cpu import (CLASSES_8WAVE, CLASSES_FALLBACK, CLASSES_FP8, CLASSES_G4, CLASSES_PEEL, CLASSES_SHARD, CLASSES_SPLIT,
                                               class_id, lora_class, lora_step_f32)
from tests.test_gemm_tiles_gpu import (ARMS16, ARMS_SPLIT, DEV, K_FP8, K_LONG, K_MAIN, K_SPLIT, REPORT, XPLAN_TOL, XPLAN_TOL16, _no_ws_bits, _p,
                                       block_of, close, descs_of, group, lora_term64, main_rows0, ncu, peel_into_a_shared_buffer, run, set_env,
                                       tile_worst, tiles256, workspace)

pytestmark = pytest.mark.gpu

G4_ARMS = ("g4", "sk2", "sk3", "splitall2", "splitall3")
LORA_REPORT = []          # (arm, class, plan, worst tile error, bound, the restatement's worst tile or None)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    yield o
    if LORA_REPORT:
        rows = {}
        for arm, cls, plan, err, bound, emu in LORA_REPORT:
            k = (arm, cls, plan)
            if k not in rows or err / bound > rows[k][0] / rows[k][1]:
                rows[k] = (err, bound, emu)
        print("\nGEMM_LORA_PLANS worst tile of the fp32 outputs per arm and class (restated = the CPU module's restatement of the step on "
              "p1's operands; plan 1 8WAVE_256, 2 8WAVE_128, 3 MIXED, 5 G4, 6 G4_SPLIT2, 7 G4_SPLIT3):")
        for (arm, cls, plan), (err, bound, emu) in sorted(rows.items()):
            print(f"  {arm:30s} {cls:10s} plan {plan}  worst {err:.3e}  bound {bound:.0e}  restated {'-' if emu is None else f'{emu:.3e}'}")
        out = os.environ.get("LX_GEMM_TILES_REPORT")
        if out:
            with open(out, "a") as f:
                for (arm, cls, plan), (err, bound, emu) in sorted(rows.items()):
                    f.write(json.dumps({"arm": arm, "class": cls, "plan": plan, "worst": err, "bound": bound, "restated": emu}) + "\n")


_GROUPS = {}


def lora_group(fmt, K, rows0, cls, seed=100):
    """The tile module's four-problem launch with p1 and p3 carrying the adapter term; built once per (format, K, size), the adapter
    inputs redrawn per class (the same class gives the same inputs)."""
    key = (fmt, K, rows0)
    if key not in _GROUPS:
        _GROUPS[key] = group(fmt, K, rows0, seed=seed, lora_p3=True, **cls)
    probs = _GROUPS[key]
    for p in probs:
        if p.lora:
            p.set_lora(**cls)
    return probs


def restated(p):
    """worst tile of the CPU module's restatement of the step on problem p's operands (16-bit formats): fp32 product over K tiles of 64"""
    if p.fmt not in ("bf16", "f16"):
        return None
    if getattr(p, "_main32", None) is None:
        y = torch.zeros(p.M, p.N, dtype=torch.float32, device=DEV)
        for k0 in range(0, p.K, 64):
            y += p.A[:, k0:k0 + 64].float() @ p.W[:, k0:k0 + 64].float().T
        p._main32 = y + p.bias
    return tile_worst(lora_step_f32(p._main32, p.slabs, p.up, p.R, p.MOD_COLS, p.TOFF_MAX), p.y())[0]


def take_report(n0, cls, emu=None):
    """move what Prob.check reported since REPORT had n0 rows into this module's table"""
    for arm, plan, err, bound in REPORT[n0:]:
        if arm.endswith(("/f32", "/lora")):          # the fp32 outputs: p1 and p3 carry the term (p0's 16-bit store has none)
            LORA_REPORT.append((arm, class_id(cls), plan, err, bound, emu))
    del REPORT[n0:]


def check_chain_bound(p, got, what):
    """A gated residual with the adapter term, element by element: one fp32 chain over everything the accumulator receives (K products,
    bias, the slab sums and the 4 r hi / lo products; a split tile's exchange is one more addition), the hi / lo split's 2^-16 of the
    adapter term, and the roundings of the gate product and the residual sum -- the bound of test_gemm_lora_step_ranks."""
    assert p.epi == "res" and p.lora and p.fmt in ("bf16", "f16")
    if getattr(p, "_mag", None) is None:
        p._mag = p.A64.abs() @ p.W64.abs().T + p.bias.double().abs()
    lmag = lora_term64(p.slabs.abs(), p.up.abs(), p.R, p.MOD_COLS, p.TOFF_MAX)
    g = p.gate.double().repeat_interleave(p.rpb, 0)[:p.M]
    ref, X0 = p.y(), p.X0.double()
    gy = ref - X0
    lim = g.abs() * (gamma_n(p.K + 4 * p.R + p.NSPLIT + 3) * (p._mag + lmag) + 2.0 ** -16 * lmag) + 2 * U24 * (gy.abs() + X0.abs()) + U24 * ref.abs()
    err = (got[:, :p.N].double() - ref).abs()
    over = err > lim
    assert not bool(over.any()), (f"{what}: {int(over.sum())} residual elements beyond the derived bound (worst ratio "
                                  f"{float((err / lim).max()):.3g} at {over.nonzero()[0].tolist()})")


def g4_takes(cls):
    """the planner's rule for lx_gemm4_kernel's LoRA step (csrc/gemm.hip): even rank <= 8, 1 ... 4 slabs, even strides, 8-byte aligned t"""
    return cls["R"] <= 8 and cls["R"] % 2 == 0 and 1 <= cls["nsplit"] <= 4 and cls["ldt"] % 2 == 0 and cls["t_col0"] % 2 == 0


def probs16(fmt, arm, cls):
    size = ARMS16[arm][3]
    if size == "long":
        probs = lora_group(fmt, K_LONG, 1, cls)
        t = tiles256(probs)
        assert t <= 128 and (arm == "splitall2" or 3 * t <= min(256, ncu())), t
        return probs
    return lora_group(fmt, K_MAIN, main_rows0(), cls)


def run16(ops, monkeypatch, fmt, arm, cls, plan=None):
    env, use_ws, arm_plan, _ = ARMS16[arm]
    probs = probs16(fmt, arm, cls)
    set_env(ops, monkeypatch, env)
    n0 = len(REPORT)
    bufs = run(ops, probs, workspace(ops) if use_ws else None, _p(plan or arm_plan), f"lora/{arm}")
    take_report(n0, cls, restated(probs[1]))
    check_chain_bound(probs[3], block_of(probs[3], bufs[3]), f"{fmt} {arm} {class_id(cls)} p3")
    return probs, bufs


# ------------------------------------------------------------------------------------------------ bf16 / fp16 operands
@pytest.mark.parametrize("cls", CLASSES_8WAVE, ids=class_id)
@pytest.mark.parametrize("arm", ["w256", "w128", "mixed"])
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lora_step_8wave_plans(ops, monkeypatch, fmt, arm, cls):
    """(4,4) the shipped shape and (3,1) with element loads run in the prologue; the others in the epilogue walk: (4,5) a second slab round
    with three of its four loads clamped, (6,2) two valid ranks in the second rank block and toff = 6, (8,4) at a 4-byte aligned base,
    (16,4), (18,3) with a partial fifth rank block, (64,4) and (64,7) with sixteen rank blocks, the latter of two slab rounds each."""
    run16(ops, monkeypatch, fmt, arm, cls)


@pytest.mark.parametrize("cls", CLASSES_G4, ids=class_id)
@pytest.mark.parametrize("arm", G4_ARMS)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lora_step_gemm4_plans(ops, monkeypatch, fmt, arm, cls):
    """lx_gemm4_kernel's own step, whole tiles and tiles split two and three ways (the term must arrive exactly once), and against the
    8-wave kernels on the same inputs: the same products, another fp32 summation order."""
    assert g4_takes(cls)
    probs, bufs = run16(ops, monkeypatch, fmt, arm, cls)
    set_env(ops, monkeypatch, {"LX_GEMM_BM": "256"})
    n0 = len(REPORT)
    ref = run(ops, probs, None, _p("8WAVE_256"), f"lora/{arm}/w256", check=False)
    del REPORT[n0:]
    for p, b, r in zip(probs, bufs, ref):
        e = close(p, block_of(p, b), block_of(p, r))
        tol = XPLAN_TOL16[fmt] if p.epi == "store" else XPLAN_TOL
        assert e < tol, f"{arm} vs 8-wave {class_id(cls)}: {p.epi} rel err {e:.3e} >= {tol:.0e}"


@pytest.mark.parametrize("cls", CLASSES_FALLBACK, ids=class_id)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lora_step_planner_fallbacks(ops, monkeypatch, fmt, cls):
    """Under the environment that gives every other launch to lx_gemm4_kernel (LX_GEMM4 = 2, with a workspace), an adapter shape its step
    cannot take -- odd rank, rank > 8, five slabs, a t base or a row stride that is not 8-byte aligned -- goes to the 8-wave kernels: this
    launch to their mixed plan, as without the switch."""
    assert not g4_takes(cls)
    run16(ops, monkeypatch, fmt, "g4", cls, plan="MIXED")


# ------------------------------------------------------------------------------------------------ split-bf16 (precise) operands
def refused(ops, probs, ws, what):
    """the launch is an LxError and leaves every output buffer and every slab as it was"""
    from loongx_amd._lib import LxError
    bufs = [p.own_buf() for p in probs]
    with pytest.raises(LxError):
        ops.gemm(descs_of(ops, probs, bufs), ws)
    torch.cuda.synchronize()
    for p, b in zip(probs, bufs):
        assert torch.equal(b.buf.view(b.iv), b.init.view(b.iv)), f"{what}: a refused launch wrote to C"
        p.check_inputs(what)


@pytest.mark.parametrize("cls", CLASSES_SPLIT, ids=class_id)
@pytest.mark.parametrize("arm", list(ARMS_SPLIT))
@pytest.mark.parametrize("segs", [2, 3])
def test_lora_step_split_bf16(ops, monkeypatch, segs, arm, cls):
    """Precise mode: ranks up to 16. Rank 16 and five slabs are beyond lx_gemm4_kernel's step: its arms then get an 8-wave plan."""
    env, use_ws, plan = ARMS_SPLIT[arm]
    probs = lora_group(f"split{segs}", K_SPLIT, 1, cls)
    set_env(ops, monkeypatch, env)
    if plan.startswith("G4") and not g4_takes(cls):
        plan = (_p("8WAVE_256"), _p("8WAVE_128"))
    else:
        plan = _p(plan)
    n0 = len(REPORT)
    bufs = run(ops, probs, workspace(ops) if use_ws else None, plan, f"lora/{arm}")
    take_report(n0, cls)
    if arm != "w256":
        set_env(ops, monkeypatch, {"LX_GEMM_BM": "256"})
        n0 = len(REPORT)
        ref = run(ops, probs, None, _p("8WAVE_256"), f"lora/{arm}/w256", check=False)
        del REPORT[n0:]
        for p, b, r in zip(probs, bufs, ref):
            if p.epi != "pair":
                e = close(p, block_of(p, b), block_of(p, r))
                assert e < XPLAN_TOL, f"{arm} vs 8-wave {class_id(cls)}: {p.epi} rel err {e:.3e}"


@pytest.mark.parametrize("arm", list(ARMS_SPLIT))
@pytest.mark.parametrize("segs", [2, 3])
def test_lora_step_split_bf16_refuses_rank_18(ops, monkeypatch, segs, arm):
    env, use_ws, _ = ARMS_SPLIT[arm]
    probs = lora_group(f"split{segs}", K_SPLIT, 1, lora_class(18, 3))
    set_env(ops, monkeypatch, env)
    refused(ops, probs, workspace(ops) if use_ws else None, f"split{segs} {arm} r=18")


# ------------------------------------------------------------------------------------------------ e4m3 operands
@pytest.mark.parametrize("cls", CLASSES_FP8, ids=class_id)
@pytest.mark.parametrize("arm", ["w256", "w128"])
def test_lora_step_fp8_operands(ops, monkeypatch, arm, cls):
    """The e4m3 kernels have the prologue form only: the shipped shape, element loads of three ranks, two ranks from three slabs."""
    set_env(ops, monkeypatch, {"LX_GEMM_BM": arm[1:]})
    n0 = len(REPORT)
    run(ops, lora_group("fp8", K_FP8, main_rows0(), cls), None, _p("8WAVE_" + arm[1:]), f"lora/{arm}")
    take_report(n0, cls)


@pytest.mark.parametrize("cls", [lora_class(5, 2), lora_class(4, 5)], ids=class_id)
@pytest.mark.parametrize("arm", ["w256", "w128"])
def test_lora_step_fp8_refuses_the_epilogue_form(ops, monkeypatch, arm, cls):
    set_env(ops, monkeypatch, {"LX_GEMM_BM": arm[1:]})
    refused(ops, lora_group("fp8", K_FP8, main_rows0(), cls), None, f"fp8 {arm} {class_id(cls)}")


# ------------------------------------------------------------------------------------------------ the mixed plan's peel, shards
@pytest.mark.parametrize("cls", CLASSES_PEEL, ids=class_id)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lora_step_mixed_plan_peel(ops, monkeypatch, fmt, cls):
    """The peel test's launch (four gated residuals with the adapter term in one buffer, the mixed plan's tail starting at m_base = 768
    inside a batch): float64 tile by tile, footprint, bit for bit under the mixed, 256-row and 128-row plans and each problem alone --
    with the prologue's shipped shape, the epilogue walk's partial rank block, and sixteen rank blocks of two slab rounds."""
    n0 = len(REPORT)
    probs, views, out = peel_into_a_shared_buffer(ops, monkeypatch, fmt, **cls)
    take_report(n0, cls)
    for i, (p, v) in enumerate(zip(probs, views)):
        r = v.blocks[0][0]
        check_chain_bound(p, out[r:r + p.M], f"peel {fmt} {class_id(cls)} q{i}")


@pytest.mark.parametrize("cls", CLASSES_SHARD, ids=class_id)
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_lora_step_shards_are_bit_identical(ops, monkeypatch, fmt, cls):
    """include/lx.h: a data-parallel shard reproduces the batch bit for bit -- on the epilogue walk as on the prologue: the group under
    the three no-workspace plans, each problem alone, and a row slice with r0 % 32 != 0."""
    n0 = len(REPORT)
    _no_ws_bits(ops, monkeypatch, fmt, K_MAIN, [("w256", {"LX_GEMM_BM": "256"}, "8WAVE_256"), ("w128", {"LX_GEMM_BM": "128"}, "8WAVE_128"),
                                                 ("mixed", {}, "MIXED")], lora_p3=True, **cls)
    take_report(n0, cls)
