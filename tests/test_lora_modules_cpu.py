"""The per-module LoRA reference (tests/lora_modules.py) must discriminate before anything runs on a GPU, the catalogue must cover every
Linear the loaders know, and the loaders must refuse an adapter on a module the engine does not evaluate.

The GPU test caps relerr(delta_engine, delta_ref) at lora_modules.CAP = 0.30. That cap tells a right engine from a wrong one only if
every plausible wrong one is further away: here each mutant of the reference -- adapter dropped, at half scale, on the wrong rows, the
slabs of a fused group rotated, the neighbouring block's adapter -- is held to relerr >= MUTANT_FLOOR = 0.45. (At the raised gain that
the gemm_fp8 arm needs for the six entries of bounded reach, the half-scale mutant is held to 0.34: closer, and still beyond the cap.)"""
import copy

import pytest
import torch

from tests import lora_modules as lm
from tests.test_lora_rank_cpu import _cfg

SHAPES = list(lm.SHAPES)
FLOOR_CONFIGS = ("plain", "latent_lora")          # the two row rules; the other configs change neither the rows nor the adapter


def test_catalogue_covers_the_layout_and_the_refused_modules():
    from loongx_amd.flux.weights import lora_layout, unevaluated_lora_modules
    cfg = _cfg(lm.base_model())
    fused, mods = lora_layout(cfg)
    gov = {e.name: list(e.modules) for e in lm.GOVERNED if not e.mod}
    assert gov == dict(fused)
    assert [e.modules[0] for e in lm.GOVERNED if e.mod] == mods == lm.MOD_MODULES
    always = [m for e in lm.ALWAYS_ON for m in e.modules]
    refused = unevaluated_lora_modules(cfg)
    assert len(set(always)) == len(always) and set(always) <= set(refused)
    # (one time_text_embed Linear stands for the six)
    assert all(m.startswith("time_text_embed.") for m in set(refused) - set(always)) and len(set(refused) - set(always)) == 5
    # every Linear of the model is in exactly one of the two lists
    linears = {n for n, m in lm.base_model().named_modules()
               if isinstance(m, (torch.nn.Linear, lm.fm.LoraLinear)) and ".lora_" not in n and not n.endswith(".base_layer")}
    named = [m for _, ms in fused for m in ms] + mods + refused
    assert len(named) == len(set(named)) and set(named) == linears, sorted(set(named) ^ linears)


@pytest.mark.parametrize("config", list(lm.CONFIGS))
@pytest.mark.parametrize("shape", SHAPES)
def test_rho_lands_in_its_window(shape, config):
    """(lm.reference asserts the window; here every governed entry is taken through it, and the unreachable one is exactly that)"""
    rhos = {e.name: lm.reference(e.name, shape, config).rho for e in lm.GOVERNED}
    print(f"RHO {shape} {config}: " + " ".join(f"{k}={v:.3f}" for k, v in rhos.items()))
    zero = [k for k, v in rhos.items() if v == 0.0]
    assert zero == [e.name for e in lm.GOVERNED if lm.unreachable(e, config)]


def test_bounded_reach_entries_cannot_meet_the_window():
    """What excuses lora_modules.bounded_reach's entries from rho's window is the reference itself: with the adapter 1000 times the size
    the test runs with, drawn or chosen for sensitivity, rho is still below the window's lower edge -- and every other entry meets the
    window (asserted by reference())."""
    tr = lm.ref_model()
    for e in lm.GOVERNED:
        if not lm.bounded_reach(e, "plain"):
            continue
        ref = lm.reference(e.name, "aligned", "plain")
        for up in (ref.up, None):
            lm.assign(tr, lm.adapter(e, 1000.0 * ref.gain * (1.0 if up is not None else 1.0 / float(lm.drawn(e.modules[0])[1].norm())), up=up))
            y = lm.oracle_forward(tr, "aligned", "plain")
            lm.assign(tr, {})
            ceiling = float((y - ref.y0).norm() / y.norm())
            print(f"CEILING {e.name} ({'chosen' if up is not None else 'drawn'} up): rho {ceiling:.3f}; the test runs at rho {ref.rho:.3f}, gemm_fp8 at {ref.raised.rho:.3f}")
            assert ceiling < lm.RHO_WINDOW[0], (e.name, ceiling)


_SMALLEST = {}


@pytest.mark.parametrize("config", FLOOR_CONFIGS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", [e.name for e in lm.GOVERNED])
def test_every_mutant_of_the_reference_is_far_from_it(name, shape, config):
    entry = lm.ENTRY[name]
    ref = lm.reference(name, shape, config)
    if lm.unreachable(entry, config):
        # nothing to be far from: the one mutant that reaches the output must differ at all
        assert bool(lm.mutant_delta(name, shape, config, "rows").any())
        return
    for mutant in lm.MUTANTS:
        d = lm.mutant_delta(name, shape, config, mutant)
        if d is None:
            continue
        e = lm.relerr(d, ref.delta)
        if e < _SMALLEST.get("e", 1e30):
            _SMALLEST.update(e=e, where=(name, shape, config, mutant))
        print(f"MUTANT {name} {shape} {config} {mutant}: {e:.3f} (rho {ref.rho:.3f})")
        assert e >= lm.MUTANT_FLOOR, (name, shape, config, mutant, e, ref.rho)
    print(f"SMALLEST MUTANT DISTANCE SO FAR: {_SMALLEST['e']:.3f} at {_SMALLEST['where']}")
    if lm.bounded_reach(entry, config):
        # the raised gain of the gemm_fp8 arm: the half-scale mutant is closer there, and still further than the cap; the others keep the floor
        for mutant in lm.MUTANTS:
            d = lm.mutant_delta(name, shape, config, mutant, raised=True)
            if d is None:
                continue
            e = lm.relerr(d, ref.raised.delta)
            print(f"MUTANT AT THE RAISED GAIN {name} {shape} {config} {mutant}: {e:.3f} (rho {ref.raised.rho:.3f})")
            assert e >= (lm.HALF_AT_RAISED if mutant == "half" else lm.MUTANT_FLOOR) > lm.CAP, (name, shape, config, mutant, e)


@pytest.mark.parametrize("name", [e.name for e in lm.GOVERNED if e.block is not None])
def test_block_level_reference(name):
    """The block-level reference: rho in its window (asserted there), and the streams the adapter cannot reach exactly unchanged --
    without latent_lora a residual projection's adapter (to_out.0, ff.net.2, proj_out) moves the condition stream alone."""
    for shape in SHAPES:
        ref = lm.block_reference(name, shape, "plain")
        moved = [bool(s.any()) for s in ref.delta]
        if name.endswith((".out", ".ff2")):
            assert moved == [False] * (len(moved) - 1) + [True], (name, moved)
        else:
            assert all(moved), (name, moved)
        assert all(bool(s.any()) for s in lm.block_reference(name, shape, "latent_lora").delta[1:])


# ------------------------------------------------------------------------------------------------------------------ loader refusals
def _snapshot(pw):
    from loongx_amd.flux.weights import _registry
    reg = {n: {k: v.clone() for k, v in a.tensors().items()} for n, a in _registry(pw).items()}
    lora = {k: (lo.down.clone(), lo.up.clone(), None if lo.down_lo is None else lo.down_lo.clone()) for k, lo in pw.lora.items()}
    return dict(t={k: v.clone() for k, v in pw.t.items()}, lora=lora, reg=reg, active=list(pw.active), r=pw.cfg.lora_r, v=pw.lora_version)


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def _assert_unchanged(pw, snap):
    now = _snapshot(pw)
    assert set(now["t"]) == set(snap["t"]) and all(torch.equal(now["t"][k], v) for k, v in snap["t"].items())
    assert set(now["lora"]) == set(snap["lora"]) and all(_same(x, y) for k in snap["lora"] for x, y in zip(now["lora"][k], snap["lora"][k]))
    assert list(now["reg"]) == list(snap["reg"]) and now["active"] == snap["active"] and (now["r"], now["v"]) == (snap["r"], snap["v"])
    for n, ts in snap["reg"].items():
        assert set(now["reg"][n]) == set(ts) and all(torch.equal(now["reg"][n][k], v) for k, v in ts.items())


@pytest.fixture(scope="module")
def loaded():
    """A packed tiny model that carries a governed adapter already, as an LxFluxPipeline on the CPU (no kernel runs)."""
    from loongx_amd.flux.pipeline import LxFluxPipeline
    from loongx_amd.flux.transformer import LxFluxTransformer
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    pw = pack_state_dict(lm.base_state_dict(), _cfg(lm.base_model()), "cpu")
    assert install_lora(pw, lm.lora_state_dict(lm.adapter(lm.ENTRY["d0.qkv"], 1.0))) == 3
    return LxFluxPipeline(LxFluxTransformer(pw, "cpu"))


@pytest.mark.parametrize("name", [e.name for e in lm.ALWAYS_ON])
def test_loaders_refuse_an_always_on_adapter_and_leave_the_model_alone(loaded, name, tmp_path):
    from safetensors.torch import save_file
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    entry = lm.ENTRY[name]
    pw = loaded.transformer.engine.w
    snap = _snapshot(pw)
    # the always-on adapter alone, and beside an accepted one
    alone = lm.adapter(entry, 1.0)
    beside = {**lm.adapter(lm.ENTRY["s1.out"], 1.0), **alone}
    for ad in (alone, beside):
        with pytest.raises(ValueError) as ei:
            install_lora(pw, lm.lora_state_dict(ad))
        assert all(m in str(ei.value) for m in entry.modules), str(ei.value)
        _assert_unchanged(pw, snap)
        with pytest.raises(ValueError) as ei:
            install_lora(pw, lm.lora_state_dict(ad), adapter_name="other")
        assert all(m in str(ei.value) for m in entry.modules)
        _assert_unchanged(pw, snap)
        with pytest.raises(ValueError) as ei:
            pack_state_dict(lm.wrapped_state_dict(ad), copy.copy(pw.cfg), "cpu")
        assert all(m in str(ei.value) for m in entry.modules), str(ei.value)
        f = tmp_path / f"{len(ad)}" / "pytorch_lora_weights.safetensors"
        f.parent.mkdir()
        save_file(lm.lora_state_dict(ad), str(f))
        with pytest.raises(ValueError) as ei:
            loaded.load_lora_weights(str(f.parent))
        assert all(m in str(ei.value) for m in entry.modules)
        _assert_unchanged(pw, snap)


def test_one_refusal_lists_every_offending_module():
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    pw = pack_state_dict(lm.base_state_dict(), _cfg(lm.base_model()), "cpu")
    ad = {}
    for e in lm.ALWAYS_ON:
        ad.update(lm.adapter(e, 1.0))
    with pytest.raises(ValueError) as ei:
        install_lora(pw, lm.lora_state_dict(ad))
    assert all(m in str(ei.value) for m in ad), str(ei.value)
    assert not pw.lora and pw.adapters is None


def test_every_governed_entry_loads_alone_both_ways():
    """install_lora of the one-entry file == pack_state_dict of the wrapped dict, and only that entry's tensors appear."""
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    cfg = _cfg(lm.base_model())
    for e in lm.GOVERNED:
        ad = lm.adapter(e, 0.5)
        pw = pack_state_dict(lm.base_state_dict(), copy.copy(cfg), "cpu")
        assert install_lora(pw, lm.lora_state_dict(ad)) == len(ad)
        want = pack_state_dict(lm.wrapped_state_dict(ad), copy.copy(cfg), "cpu")
        assert set(pw.lora) == set(want.lora) == (set() if e.mod else {e.name})
        for k, lo in want.lora.items():
            assert torch.equal(pw.lora[k].down, lo.down) and torch.equal(pw.lora[k].up, lo.up)
        assert set(pw.t) == set(want.t) and all(torch.equal(pw.t[k], v) for k, v in want.t.items())
        assert ("mod.lora_down" in pw.t) == e.mod
