"""Every adapter-carrying Linear of the tiny model, ONE module at a time, in every operand mode, against the float64 reference of
tests/lora_modules.py.

Per case: install_lora the one-entry adapter, set_conditioning, forward -> y1; the same adapter with `up` zeroed -> y0 (the same
launches on the same rows, so what the operand format does to the base model is common to both); delta_eng = y1 - y0 is held to
relerr(delta_eng, delta_ref) <= BOUND[mode] <= lora_modules.CAP = 0.30. tests/test_lora_modules_cpu.py shows that an engine which drops
the adapter, halves it, applies it to the wrong rows, reads the wrong slab of a fused group or the neighbouring block's adapter is at
least 0.45 away. An entry whose adapter cannot reach the output must give torch.equal(y1, y0). y0 itself is held to the mode's
whole-output bound (tests/engine_walk.BOUNDS), so that a broken base model cannot pose as a clean noise floor.

BOUND[mode] = 2 x the worst case of the mode measured on MI355X (one significant digit, never above the cap; the factor covers other
seeds and shapes), separately for the entries that meet rho's window and for the six of bounded reach (lora_modules.bounded_reach:
x_embedder and the residual projections without latent_lora, whose rho stays below the window whatever the adapter). Those run with an
up matrix chosen where the output is most sensitive and the largest gain at which a half-scale adapter is still 0.47 from the right one
(rho 0.03 ... 0.1). That clears the noise of every mode but gemm_fp8, whose error on these deltas is of fixed size, 1.3 ... 3 % of the
output (relerr x rho stays put as the gain grows); as the cap stays, that mode runs them at a raised gain (rho 0.09 ... 0.16), up to
where the half-scale mutant is still 0.34 away -- beyond the cap -- and every other mutant 0.45 (tests/test_lora_modules_cpu.py).
The measured value stands beside each bound and profiles/lora_modules.txt has the worst case of every mode."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lora_modules as lm  # noqa: E402
from tests.engine_walk import BOUNDS as WHOLE_OUTPUT_BOUNDS  # noqa: E402
from tests.helpers import relerr  # noqa: E402
from tests.test_lora_rank_cpu import _cfg  # noqa: E402

DEV = "cuda"
MODES = {"bf16": {}, "fp16": {"operands": "fp16"}, "precise": {"precise": True}, "gemm_fp8": {"gemm_fp8": True}, "attn_fp8": {"attn_fp8": True}}
# mode -> (bound, measured worst case) of the whole-model deltas, for the entries that meet rho's window (0.33 ... 0.5 here) and for those
# of bounded reach (rho 0.03 ... 0.1; gemm_fp8 0.09 ... 0.16). 2 x measured, one significant digit, never above the cap.
BOUND = {"bf16": ((0.02, 1.21e-2), (0.2, 7.9e-2)), "fp16": ((0.02, 7.6e-3), (0.02, 1.22e-2)), "precise": ((1e-4, 5.1e-5), (4e-4, 1.78e-4)),
         "gemm_fp8": ((0.2, 1.10e-1), (lm.CAP, 2.78e-1)), "attn_fp8": ((0.1, 5.2e-2), (0.2, 1.21e-1))}
# the block-level arm (block_forward / single_block_forward have no e4m3 path; every entry meets the window there)
BLOCK_BOUND = {"bf16": (0.02, 8.4e-3), "fp16": (0.009, 4.5e-3), "precise": (3e-5, 1.7e-5)}
NAMES = [e.name for e in lm.GOVERNED]


@pytest.fixture(scope="module")
def engines():
    """mode -> the engine it runs on: one packed with precise=True for the precise arm, one without for the others; no step graphs."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd.flux.engine import DiTEngine
    from loongx_amd.flux.weights import pack_state_dict
    built = {}

    def get(mode):
        precise = mode == "precise"
        if precise not in built:
            eng = DiTEngine(pack_state_dict(lm.base_state_dict(), _cfg(lm.base_model()), DEV, precise=precise), DEV)
            eng.use_graph = False
            built[precise] = eng
        return built[precise]
    return get


_DEV = {}


def dev(d, key):
    if key not in _DEV:
        mv = lambda v: v.to(DEV) if isinstance(v, torch.Tensor) else (tuple(mv(x) for x in v) if isinstance(v, tuple) else v)
        _DEV[key] = {k: ([tuple(mv(x) for x in s) for s in v] if k == "steps" else mv(v)) for k, v in d.items()}
    return _DEV[key]


def install(eng, entry, gain, zero_up, up=None):
    from loongx_amd.flux.weights import install_lora
    ad = lm.adapter(entry, gain, zero_up=zero_up, up=up)
    assert install_lora(eng.w, lm.lora_state_dict(ad)) == len(ad)
    eng.drop_graphs_and_shape()             # what LxFluxPipeline.load_lora_weights does after an install
    eng.drop_conditioning()


def forward(eng, entry, shape, config, mode, gain, zero_up, up=None):
    install(eng, entry, gain, zero_up, up)
    eng.set_lora_scale(lm.CONFIGS[config][1])
    d = dev(lm.data(shape), ("model", shape))
    mc = dict(lm.CONFIGS[config][0], **MODES[mode])
    eng.set_conditioning(d["enc"], d["pooled"], d["guid"], d["tids"], d["ids"], d["cond"], d["cids"], c_t=0.0, model_config=mc)
    for k in range(lm.step_of(config) + 1):
        y = eng.forward(*d["steps"][k])
    return y.float().cpu().clone()


@pytest.mark.parametrize("config", list(lm.CONFIGS))
@pytest.mark.parametrize("shape", list(lm.SHAPES))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", list(MODES))
def test_one_module(engines, mode, name, shape, config):
    entry, eng = lm.ENTRY[name], engines(mode)
    ref = lm.reference(name, shape, config)
    if mode == "gemm_fp8" and ref.raised is not None:      # bounded reach: this mode's noise needs the raised gain (lora_modules.HALF_AT_RAISED)
        ref = ref.raised
    y0 = forward(eng, entry, shape, config, mode, ref.gain, True, ref.up)
    y1 = forward(eng, entry, shape, config, mode, ref.gain, False, ref.up)
    e0 = relerr(y0, ref.y0)
    if lm.unreachable(entry, config):
        print(f"LORA_MODULE mode={mode} entry={name} shape={shape} config={config} rho=0 unreachable y0err={e0:.3e}")
        assert torch.equal(y1, y0)
    else:
        e = relerr(y1 - y0, ref.delta)
        print(f"LORA_MODULE mode={mode} entry={name} shape={shape} config={config} rho={ref.rho:.3f} relerr={e:.3e} y0err={e0:.3e}")
        assert e <= BOUND[mode][lm.bounded_reach(entry, config)][0], (mode, name, shape, config, e, ref.rho)
    assert e0 < WHOLE_OUTPUT_BOUNDS[mode], (mode, name, shape, config, e0)


# ------------------------------------------------------------------------------------------------------------------ block level
def block_call(eng, entry, shape, config, mode, gain, zero_up):
    from loongx_amd.flux.block import LxBlock, block_forward, single_block_forward
    install(eng, entry, gain, zero_up)
    eng.set_lora_scale(1.0)
    d = dev(lm.block_data(shape), ("block", shape))
    mc = dict(lm.CONFIGS[config][0], **MODES[mode])
    kind, idx = entry.block
    blk = LxBlock(eng, kind, idx)
    if kind == "double":
        out = block_forward(blk, d["hid"], d["enc"], d["cond"], d["temb"], d["ctemb"], d["rope_cond"], d["rope_main"], mc)
    else:
        blk.text_len = d["T"]
        out = single_block_forward(blk, torch.cat([d["enc"], d["hid"]], 1), d["temb"], d["rope_main"], d["cond"], d["ctemb"], d["rope_cond"], mc)
    return [o.float().cpu().clone() for o in out]


@pytest.mark.parametrize("config", ["plain", "latent_lora"])
@pytest.mark.parametrize("shape", list(lm.SHAPES))
@pytest.mark.parametrize("name", [e.name for e in lm.GOVERNED if e.block is not None])
@pytest.mark.parametrize("mode", list(BLOCK_BOUND))
def test_one_module_block_level(engines, mode, name, shape, config):
    """block_forward / single_block_forward on the entry's block against the oracle's block functions: the delta over the returned
    streams, and a stream the reference leaves exactly untouched (the text and image rows under a residual projection's adapter without
    latent_lora) bit-equal between the two arms -- where a wrong row range shows directly."""
    entry, eng = lm.ENTRY[name], engines(mode)
    ref = lm.block_reference(name, shape, config)
    y0 = block_call(eng, entry, shape, config, mode, ref.gain, True)
    y1 = block_call(eng, entry, shape, config, mode, ref.gain, False)
    assert len(y1) == len(ref.delta)
    moved = [bool(ds.any()) for ds in ref.delta]
    for k, m in enumerate(moved):
        assert m or torch.equal(y1[k], y0[k]), f"stream {k} of {name} differs between the arms; the reference leaves it untouched"
    de = torch.cat([(a - b).reshape(-1) for a, b, m in zip(y1, y0, moved) if m])
    dr = torch.cat([ds.reshape(-1) for ds, m in zip(ref.delta, moved) if m])
    e = relerr(de, dr)
    per = " ".join("untouched" if not m else f"{relerr(a - b, ds):.2e}" for a, b, ds, m in zip(y1, y0, ref.delta, moved))
    e0 = max(relerr(a, r) for a, r in zip(y0, ref.y0))
    print(f"LORA_BLOCK mode={mode} entry={name} shape={shape} config={config} rho={ref.rho:.3f} relerr={e:.3e} streams=[{per}] y0err={e0:.3e}")
    assert e <= BLOCK_BOUND[mode][0], (mode, name, shape, config, e, ref.rho)
    assert e0 < WHOLE_OUTPUT_BOUNDS[mode], (mode, name, shape, config, e0)
