"""The plan of the engine walk (tests/engine_walk.py), checked without a GPU against the catalogue object the GPU test walks: every ordered
pair of states is a transition of the plan, the data sets alternate, the chunks the GPU tests run cover the plan, every state's
configuration is one the fp32 oracle accepts, and the catalogue's adapter sets fit the model packed for precise mode."""
import pytest
import torch

from tests import engine_walk as ew

REQUIRED = [  # (shape, model_config, B, (T, N, C), c_factor, mask, adapters): the 18 states the walk started from
    ("aligned", {}, 2, (32, 64, 64), None, None, ("default",)),
    ("ragged", {}, 2, (24, 60, 60), None, None, ("default",)),
    ("aligned", {}, 2, (32, 64, 0), None, None, ("default",)),
    ("aligned", {}, 1, (32, 64, 64), None, None, ("default",)),
    ("aligned", {}, 2, (32, 64, 32), None, None, ("default",)),
    ("aligned", {"independent_condition": True}, 2, (32, 64, 64), None, None, ("default",)),
    ("ragged", {"union_cond_attn": False, "latent_lora": True}, 2, (24, 60, 60), None, None, ("default",)),
    ("aligned", {}, 2, (32, 64, 64), 0.5, None, ("default",)),
    ("aligned", {"add_cond_attn": True}, 2, (32, 64, 64), None, None, ("default",)),
    ("aligned", {"operands": "fp16"}, 2, (32, 64, 64), None, None, ("default",)),
    ("ragged", {"operands": "fp16", "independent_condition": True}, 2, (24, 60, 60), None, None, ("default",)),
    ("aligned", {"attn_fp8": True, "independent_condition": True}, 2, (32, 64, 64), None, None, ("default",)),
    ("aligned", {"gemm_fp8": True}, 2, (32, 64, 64), None, None, ("default",)),
    ("aligned", {"precise": True, "independent_condition": True}, 2, (32, 64, 64), None, None, ("default",)),
    ("ragged", {"precise": True}, 2, (24, 60, 60), None, None, ("default",)),
    ("aligned", {}, 2, (32, 64, 64), None, "keypad", ("default",)),
    ("aligned", {}, 2, (32, 64, 64), None, "additive", ("default",)),
    ("aligned", {}, 2, (32, 64, 64), None, None, ("default", "b")),
]


def test_the_catalogue_holds_the_required_states():
    got = [(s.shape, s.model_config, s.B, s.dims(), s.c_factor, s.mask, s.adapters) for s in ew.CATALOGUE]
    assert got[:18] == REQUIRED and ew.N_STATES >= 18
    assert len({s.name for s in ew.CATALOGUE}) == ew.N_STATES
    two = ew.CATALOGUE[17]
    assert dict(two.weights) == {"b": (0.3, 1.0)} and two.lora_scale == 0.5
    for s in ew.CATALOGUE:
        if s.adapters == ("default",):                            # states that say nothing about adapters
            assert s.weights == () and s.lora_scale == 1.0
        assert s.mode in ew.BOUNDS
        want = ("precise" if s.model_config.get("precise") else "gemm_fp8" if s.model_config.get("gemm_fp8") else
                "attn_fp8" if s.model_config.get("attn_fp8") else "fp16" if s.model_config.get("operands") == "fp16" else "bf16")
        assert s.mode == want, s.name


def test_every_ordered_pair_is_a_transition_of_the_plan():
    p = ew.plan()
    n = ew.N_STATES
    pairs = [(a.state, b.state) for a, b in zip(p, p[1:])]
    assert len(p) == n * n + 1 and len(pairs) == len(set(pairs)) == n * n
    assert set(pairs) == {(a, b) for a in range(n) for b in range(n)}
    for k, v in enumerate(p):                                     # what a failure message names: the states visited before
        assert v.prev == tuple(u.state for u in p[max(k - 2, 0):k])


def test_the_data_sets_alternate():
    p = ew.plan()
    for s in range(ew.N_STATES):
        seeds = [v.seed for v in p if v.state == s]
        assert len(seeds) >= ew.N_STATES and seeds == [k % 2 for k in range(len(seeds))], s
    loops = [(a, b) for a, b in zip(p, p[1:]) if a.state == b.state]
    assert len(loops) == ew.N_STATES and all(a.seed != b.seed for a, b in loops)


def test_the_chunks_cover_the_plan_in_order():
    c = ew.chunks()
    assert len(c) == ew.N_STATES and c[0][0] == 0 and c[-1][1] == len(ew.plan())
    assert all(a[1] == b[0] for a, b in zip(c, c[1:])) and all(0 < e - s <= ew.N_STATES + 2 for s, e in c)


def test_the_two_data_sets_of_a_state_differ():
    for i, st in enumerate(ew.CATALOGUE):
        a, b = ew.data(st, 0), ew.data(st, 1)
        T, N, C = st.dims()
        assert a["enc"].shape == (st.B, T, 64) and a["steps"][0][0].shape == (st.B, N, 64) and (a["cond"] is None) == (C == 0)
        assert C == 0 or (a["cond"].shape == (st.B, C, 64) and a["cids"].shape == (C, 3))
        for key in ("enc", "pooled", "guid") + (("cond",) if C else ()) + (("mask",) if st.mask else ()):
            assert not torch.equal(a[key], b[key]), (st.name, key)
        assert not torch.equal(a["steps"][0][0], b["steps"][0][0]) and not torch.equal(a["steps"][0][0], a["steps"][1][0])
        assert a["steps"][2][0] is a["steps"][0][0] and [float(t[0]) for _, t in a["steps"]] == [pytest.approx(v) for v in ew.TIMESTEPS]
        if st.mask:
            S = T + N + C
            assert a["mask"].shape == ((st.B, 1, 1, S) if st.mask == "keypad" else (1, ew.H, S, S))
            assert a["mask"].dtype == (torch.bool if st.mask == "keypad" else torch.float32)
            if st.mask == "additive":
                assert bool(torch.isinf(a["mask"]).any())


@pytest.mark.parametrize("i", range(ew.N_STATES), ids=[s.name for s in ew.CATALOGUE])
def test_the_oracle_accepts_the_state(i):
    st = ew.CATALOGUE[i]
    a, b = ew.oracle(st, 0), ew.oracle(st, 1)
    T, N, C = st.dims()
    for o in a + b:
        assert o.shape == (st.B, N, 64) and bool(torch.isfinite(o).all())
    assert a[2] is a[0] and not torch.equal(a[0], a[1]) and not torch.equal(a[0], b[0])
    known = {"independent_condition", "union_cond_attn", "latent_lora", "add_cond_attn", "operands", "attn_fp8", "gemm_fp8", "precise"}
    assert set(st.model_config) <= known


def test_the_oracle_sees_what_distinguishes_the_states():
    """States that share a data set differ in the oracle wherever their difference is not the arithmetic format alone."""
    same_math = {"fp16": "plain", "gemm_fp8": "plain", "attn_fp8_union": "plain", "attn_fp8_independent": "independent",
                 "precise_independent": "independent", "attn_fp8_union_ragged": "plain_ragged", "precise_ragged": "plain_ragged"}
    for name, twin in same_math.items():
        assert torch.equal(ew.oracle(ew.STATE[name], 0)[0], ew.oracle(ew.STATE[twin], 0)[0]), name
    plain = ew.oracle(ew.STATE["plain"], 0)[0]
    for name in ("independent", "c_factor", "add_cond_attn", "keypad_mask", "additive_mask", "two_adapters", "no_condition", "short_condition"):
        assert not torch.equal(ew.oracle(ew.STATE[name], 0)[0], plain), name


def test_the_adapter_sets_fit_the_model_packed_for_precise_mode():
    from loongx_amd.flux.weights import active_adapters, list_adapters, set_active_adapters
    pw = ew.packed("cpu")
    assert pw.precise_ready and list_adapters(pw) == ["default", "b"] and active_adapters(pw) == ["default"] and pw.cfg.lora_r == ew.RANK
    set_active_adapters(pw, ["default", "b"])
    assert pw.cfg.lora_r == 2 * ew.RANK and max(lo.down.shape[0] for lo in pw.lora.values()) == 16      # one slab: every mode takes it
    assert not torch.equal(pw.adapters["default"].lora["d0.qkv"].down, pw.adapters["b"].lora["d0.qkv"].down)
    set_active_adapters(pw, ["default"])
    assert pw.cfg.lora_r == ew.RANK
