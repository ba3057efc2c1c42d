"""ONE engine taken through every ordered pair of the states of tests/engine_walk.py, and through the events that happen inside a
conditioning, compared bit for bit with what a freshly built engine gives for the same visit.

The host layer (flux/engine.py, transformer.py, block.py) keeps captured step graphs, per-mode scratch, the per-layer condition cache, fp16 /
e4m3 weight images, adapter tables, a mask workspace, a prepared schedule and tranformer_forward's conditioning key alive across
conditionings and invalidates each by hand. A missed invalidation gives a plausible velocity that no kernel test can see; here it shows as
a walked result that differs from the fresh one. The kernels are run-to-run deterministic under every launch plan, so a fresh engine
differs from the walked one only in buffer addresses and in what the buffers held before: the comparison is torch.equal, no tolerance.

Two anchors keep the walk from comparing the code with itself: every fresh result is within its mode's existing bound of the fp32 oracle
(measured on MI355X, relative L2 per forward, the worst of a mode's states, data sets and forwards against the bound in brackets:
bf16 4.32e-3 [9e-3], fp16 3.34e-3 [9e-3], precise 1.48e-5 [2e-4], attn_fp8 5.68e-3 [7e-2], gemm_fp8 3.26e-2 [0.15]; no state needed a
bound of its own; profiles/engine_walk.txt has every state), and no two fresh results are bit-equal, so a stale replay of another state
or of the other data set cannot pass."""
import hashlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import engine_walk as ew  # noqa: E402
from tests.engine_walk import CATALOGUE, STATE, condition, fresh, set_cond, step, visit  # noqa: E402
from tests.helpers import relerr  # noqa: E402

DEV = "cuda"
NAMES = [s.name for s in CATALOGUE]


@pytest.fixture(scope="module")
def eng():
    """The engine that lives through the whole module."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ew.new_engine()


def same(got, want) -> bool:
    return len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want))


def first_diff(got, want):
    return next((k for k, (g, w) in enumerate(zip(got, want)) if not torch.equal(g, w)), None)


def assert_fresh(got, st, seed, where):
    k = first_diff(got, fresh(st, seed))
    assert k is None, f"{where}: forward {k} of state {st.name!r} (data set {seed}) differs from a fresh engine's"


# ---------------------------------------------------------------------------------------------------- what "right" is
@pytest.mark.parametrize("i", range(ew.N_STATES), ids=NAMES)
def test_fresh_engine_is_within_the_modes_bound_of_the_oracle(eng, i):
    st = CATALOGUE[i]
    for seed in (0, 1):
        errs = [relerr(g, w) for g, w in zip(fresh(st, seed), ew.oracle(st, seed))]
        print(f"FRESH_VS_ORACLE {st.name} data set {seed}: " + " ".join(f"{e:.3e}" for e in errs) + f"  [{st.mode}: {ew.BOUNDS[st.mode]:.1e}]")
        assert max(errs) < ew.BOUNDS[st.mode], (st.name, seed, errs)


def test_no_two_fresh_results_are_bit_equal(eng):
    """Across states and data sets (the third forward of a visit repeats the first's inputs: within one visit those two may coincide)."""
    seen = {}
    for st in CATALOGUE:
        for seed in (0, 1):
            outs = fresh(st, seed)
            assert not torch.equal(outs[0], outs[1]), (st.name, seed)
            for k, o in enumerate(outs):
                h = (tuple(o.shape), hashlib.sha256(o.numpy().tobytes()).hexdigest())
                other = seen.setdefault(h, (st.name, seed, k))
                assert other[:2] == (st.name, seed), f"{(st.name, seed, k)} is bit-equal to {other}"


# ---------------------------------------------------------------------------------------------------- the transition matrix
@pytest.mark.parametrize("chunk", ew.chunks(), ids=[f"visits{a}-{b - 1}" for a, b in ew.chunks()])
def test_walk(eng, chunk):
    """Consecutive visits of the plan (an Eulerian circuit of the complete digraph on the states, self-loops included; the tests of this
    parametrisation run in order on the one engine and together take every ordered pair once)."""
    plan = ew.plan()
    for n in range(*chunk):
        v = plan[n]
        st = CATALOGUE[v.state]
        got = visit(eng, st, v.seed)
        k = first_diff(got, fresh(st, v.seed))
        assert k is None, (f"visit {n}: forward {k} of state {st.name!r} (data set {v.seed}) differs from a fresh engine's; last three states "
                           f"visited: {' -> '.join([NAMES[p] for p in v.prev] + [st.name])}")


# ---------------------------------------------------------------------------------------------------- events inside a conditioning
PLAIN, INDEP = STATE["plain"], STATE["independent"]


def refused_forward(eng, st=PLAIN):
    with pytest.raises(RuntimeError, match="set_conditioning"):
        step(eng, st, 0, 0)


def test_adapter_changes_and_back(eng):
    """lora_scale 0.5 and back, a second adapter with per-image weights and back: each change leaves the engine unconditioned, each
    conditioning after it equals the fresh engine's in that adapter state."""
    half = PLAIN._replace(name="plain_half_scale", lora_scale=0.5)
    two = PLAIN._replace(name="plain_two_adapters", adapters=("default", "b"), weights=(("b", (0.3, 1.0)),))
    assert_fresh(visit(eng, PLAIN, 0), PLAIN, 0, "before any change")
    eng.set_lora_scale(0.5)
    refused_forward(eng)
    set_cond(eng, PLAIN, 1)
    assert_fresh([step(eng, PLAIN, 1, k) for k in range(3)], half, 1, "at lora_scale 0.5")
    eng.set_lora_scale(1.0)
    refused_forward(eng)
    set_cond(eng, PLAIN, 0)
    assert_fresh([step(eng, PLAIN, 0, k) for k in range(3)], PLAIN, 0, "back at lora_scale 1")
    eng.set_adapters(["default", "b"], {"b": (0.3, 1.0)})
    refused_forward(eng)
    set_cond(eng, PLAIN, 1)
    assert_fresh([step(eng, PLAIN, 1, k) for k in range(3)], two, 1, "with adapters default + b")
    eng.set_adapters(["default"])
    refused_forward(eng)
    set_cond(eng, PLAIN, 1)
    assert_fresh([step(eng, PLAIN, 1, k) for k in range(3)], PLAIN, 1, "back at adapter default")
    assert not torch.equal(fresh(half, 1)[0], fresh(PLAIN, 1)[0]) and not torch.equal(fresh(two, 1)[0], fresh(PLAIN, 1)[0])


_PRE = {}


def fresh_prepared(st, seed):
    """The three forwards of a visit taken from a prepared schedule, on a new engine."""
    if (st, seed) not in _PRE:
        e = ew.new_engine()
        condition(e, st, seed)
        e.prepare_schedule(torch.tensor(ew.TIMESTEPS))
        _PRE[(st, seed)] = [step(e, st, seed, k, step_index=k) for k in range(3)]
    return _PRE[(st, seed)]


@pytest.mark.parametrize("name", ["plain", "no_union_latent_lora_ragged"])
def test_prepared_schedule_interleaved_with_per_step_forwards(eng, name):
    """forward(step_index=i) from prepare_schedule()'s table and the per-step forward of the same timesteps, interleaved on one conditioning
    (pre, per-step, pre; then per-step, pre, per-step): each form gives what a fresh engine gives for that form."""
    st = STATE[name]
    pre, per = fresh_prepared(st, 1), fresh(st, 1)
    condition(eng, st, 1)
    eng.prepare_schedule(torch.tensor(ew.TIMESTEPS))
    for order in (("pre", "per", "pre"), ("per", "pre", "per")):
        for k, form in enumerate(order):
            got = step(eng, st, 1, k, step_index=k) if form == "pre" else step(eng, st, 1, k)
            assert torch.equal(got, (pre if form == "pre" else per)[k]), (order, k, form)
    set_cond(eng, st, 0)                                            # a new conditioning drops the table: step_index is then ignored
    assert eng.sched is None
    assert_fresh([step(eng, st, 0, k, step_index=k) for k in range(3)], st, 0, "after the schedule was dropped")


def test_graph_toggled_within_a_conditioning(eng):
    """use_graph off and on between the forwards of one conditioning (with the condition stream cached by the first)."""
    for st in (INDEP, PLAIN):
        condition(eng, st, 0)
        got = [step(eng, st, 0, 0)]
        eng.use_graph = False
        try:
            got.append(step(eng, st, 0, 1))
        finally:
            eng.use_graph = True
        got.append(step(eng, st, 0, 2))
        assert_fresh(got, st, 0, "graph, eager, graph")
        eng.use_graph = False
        try:
            got = [step(eng, st, 0, 0)]
        finally:
            eng.use_graph = True
        got += [step(eng, st, 0, 1), step(eng, st, 0, 2)]
        assert_fresh(got, st, 0, "eager, graph, graph")


def test_more_than_four_graph_keys_on_one_shape(eng):
    """Five graph keys without a shape change (the fifth capture clears the four before it), then the first again."""
    visit(eng, STATE["plain_ragged"], 0)                            # (another shape: setup() starts the aligned shape without graphs)
    condition(eng, PLAIN, 0)
    assert eng.graphs == {}
    order = [(PLAIN, 0), (INDEP, 0), (STATE["c_factor"], 0), (STATE["add_cond_attn"], 0), (PLAIN, 1), (INDEP, 1)]
    counts = []
    for st, seed in order:
        assert_fresh(visit(eng, st, seed), st, seed, f"graph keys so far: {counts}")
        counts.append(len(eng.graphs))
    assert counts == [1, 3, 4, 1, 2, 4], counts                     # plain 1 key, independent 2 (with and without the condition rows), ...


def test_refused_conditionings_leave_nothing_behind(eng):
    """A conditioning that raises, between valid ones: the engine is unconditioned and without a mask, and the next conditioning equals the
    fresh engine's. (The fourth refusal, a rank-16 adapter with gemm_fp8, needs weights packed without precise: see the transformer's.)"""
    keypad, short = STATE["keypad_mask"], STATE["short_condition"]

    def refused(exc, what, st=keypad, before=None, **over):
        assert_fresh(visit(eng, keypad, 0), keypad, 0, f"before {what}")
        assert eng.cond_mask is not None and eng.cond_ready
        if before is not None:
            before()
        with pytest.raises(exc):
            set_cond(eng, st, 1, **over)
        refused_forward(eng)
        assert eng.cond_mask is None and not eng.cond_ready

    refused(NotImplementedError, "a mask in precise mode", model_config={"precise": True})
    assert_fresh(visit(eng, keypad, 1), keypad, 1, "after a mask in precise mode")
    refused(ValueError, "three per-image weights for two images", before=lambda: eng.set_adapter_weights({"default": (1.0, 0.5, 0.25)}))
    eng.set_adapter_weights({})
    set_cond(eng, PLAIN, 1)
    assert_fresh([step(eng, PLAIN, 1, k) for k in range(3)], PLAIN, 1, "after per-image weights of the wrong length")
    refused(ValueError, "add_cond_attn with C != N", st=short, model_config={"add_cond_attn": True})
    assert_fresh(visit(eng, short, 0), short, 0, "after add_cond_attn with C != N")
    assert_fresh(visit(eng, PLAIN, 0), PLAIN, 0, "after add_cond_attn with C != N")


def test_weights_overwritten_in_place_and_back(eng):
    """weights_version, the key element no catalogue state moves: another weight set written over the packed tensors in place (what a
    broadcast does to a receiving rank), after the engine has built everything it derives from the weights -- the e4m3 images of gemm_fp8,
    the fp16 images, the scaled norm_q tensors, step graphs of five modes. Every mode then equals a fresh engine packed from the other
    set; with the first set written back, the first fresh results."""
    states = [STATE[n] for n in ("gemm_fp8", "fp16", "attn_fp8_union", "precise_ragged", "plain")]
    for st in states:
        assert_fresh(visit(eng, st, 0), st, 0, "before the weights change")
    ew.overwrite_weights(eng.w, ew.packed(sd=ew.other_state_dict()))
    for st in states:
        want = fresh(st, 1, True)
        k = first_diff(visit(eng, st, 1), want)
        assert k is None, f"forward {k} of state {st.name!r} after the weights were overwritten differs from a fresh engine's on those weights"
        assert not torch.equal(want[0], fresh(st, 1)[0])
        e = max(relerr(g, w) for g, w in zip(want, fresh(st, 1)))
        assert e > 1e-3, (st.name, e)                               # (the other weights are another model)
    ew.overwrite_weights(eng.w, ew.packed())
    for st in states:
        assert_fresh(visit(eng, st, 0), st, 0, "with the first weights written back")


# ---------------------------------------------------------------------------------------------------- the transformer's cache key
def _rank4_files(tmp):
    from safetensors.torch import save_file
    from tests.test_lora_rank_cpu import _lora_only
    from tests.test_lora_wide_gpu import rank_model
    for r in (4, 16):
        (tmp / f"r{r}").mkdir()
        save_file(_lora_only(rank_model(r)[1]), str(tmp / f"r{r}" / "pytorch_lora_weights.safetensors"))
    return tmp


def new_transformer():
    """The tiny model with its own rank-4 adapter, packed without precise (so that a rank-16 file loads), as an LxFluxTransformer."""
    from loongx_amd.flux.transformer import LxFluxTransformer
    from tests.test_lora_rank_cpu import _cfg
    from tests.test_lora_wide_gpu import rank_model
    tr, sd, _ = rank_model(4)
    return LxFluxTransformer.from_state_dict(sd, _cfg(tr), DEV)


@pytest.fixture(scope="module")
def lx(eng):
    """The transformer that lives through the rest of the module."""
    return new_transformer()


def tf_step(lx, st, seed, k):
    from loongx_amd.flux.transformer import tranformer_forward
    d = ew.device_data(st, seed)
    lat, t = d["steps"][k]
    lx.c_factor = st.c_factor
    return tranformer_forward(lx, d["cond"], d["cids"], None, st.model_config, return_dict=False, hidden_states=lat, encoder_hidden_states=d["enc"],
                              pooled_projections=d["pooled"], timestep=t, img_ids=d["ids"], txt_ids=d["tids"], guidance=d["guid"],
                              attention_mask=d["mask"])[0].float().cpu().clone()


def tf_visit(lx, st, seed):
    return [tf_step(lx, st, seed, k) for k in range(3)]


_TF = {}


def tf_fresh(st, seed, r=4, tmp=None):
    """tranformer_forward's three outputs on a newly built transformer (with the rank-r file loaded over its adapter when r != 4)."""
    if (st, seed, r) not in _TF:
        new = new_transformer()
        if r != 4:
            from loongx_amd.flux.pipeline import LxFluxPipeline
            assert LxFluxPipeline(new).load_lora_weights(str(tmp / f"r{r}")) == 25
        _TF[(st, seed, r)] = tf_visit(new, st, seed)
    return _TF[(st, seed, r)]


def _block_call(lx, kind):
    """One block-level mirror call on block 0 under another model_config and another cond_temb than the transformer's conditioning."""
    from loongx_amd.flux.block import attn_forward, block_forward, single_block_forward
    from tests.test_lora_wide_gpu import rank_model
    tr = rank_model(4)[0]
    d = ew.data(PLAIN, 0)
    T, N, C = PLAIN.dims()
    g = torch.Generator().manual_seed(77)
    hid, enc, cond = (torch.randn(2, L, 256, generator=g).to(DEV) * 0.5 for L in (N, T, C))
    temb, ctemb = torch.randn(2, 256, generator=g).to(DEV), torch.randn(2, 256, generator=g).to(DEV)
    main, rc = tr.pos_embed(torch.cat([d["tids"], d["ids"]], 0)), tr.pos_embed(d["cids"])
    mc = {"independent_condition": True}
    if kind == "attn":
        out = attn_forward(lx.transformer_blocks[0].attn, hid, enc, cond, None, main, rc, mc)
    elif kind == "block":
        out = block_forward(lx.transformer_blocks[0], hid, enc, cond, temb, ctemb, rc, main, mc)
    else:
        blk = lx.single_transformer_blocks[0]
        blk.text_len = T
        out = single_block_forward(blk, torch.cat([enc, hid], 1), temb, main, cond, ctemb, rc, mc)
    return [o.float().cpu().clone() for o in out]


_BLOCK = {}


@pytest.mark.parametrize("kind", ["attn", "block", "single"])
def test_block_level_call_between_two_identical_tranformer_forward_calls(lx, kind):
    """attn_forward / block_forward / single_block_forward configure the SAME engine: another model_config, attention bias and RoPE
    tables, and a slice of the modulation tables overwritten. tranformer_forward's conditioning key cannot see that; the engine's
    cond_ready must, or the second forward replays under the block call's configuration."""
    want = tf_fresh(PLAIN, 0)
    assert same(tf_visit(lx, PLAIN, 0), want)
    if kind not in _BLOCK:
        _BLOCK[kind] = _block_call(new_transformer(), kind)
    assert same(_block_call(lx, kind), _BLOCK[kind])                # the mirror itself: as on a new transformer
    k = first_diff(tf_visit(lx, PLAIN, 0), want)
    assert k is None, f"forward {k} after a {kind} call differs from the same forward before it"


def test_load_lora_weights_of_another_rank_and_back(lx, tmp_path):
    """A rank-16 file over the rank-4 model and the rank-4 file again on the long-lived transformer; with the rank-16 adapter, gemm_fp8 is
    refused and leaves nothing behind."""
    from loongx_amd.flux.pipeline import LxFluxPipeline
    tmp = _rank4_files(tmp_path)
    pipe, e = LxFluxPipeline(lx), lx.engine
    assert same(tf_visit(lx, INDEP, 0), tf_fresh(INDEP, 0))
    assert pipe.load_lora_weights(str(tmp / "r16")) == 25
    with pytest.raises(RuntimeError, match="set_conditioning"):
        step(e, INDEP, 0, 0)
    assert e.cfg.lora_r == 16
    assert same(tf_visit(lx, INDEP, 0), tf_fresh(INDEP, 0, 16, tmp))
    with pytest.raises(ValueError, match="gemm_fp8"):
        tf_step(lx, STATE["gemm_fp8"], 0, 0)
    with pytest.raises(RuntimeError, match="set_conditioning"):
        step(e, PLAIN, 0, 0)
    assert e.cond_mask is None and lx._cond_key is None
    assert same(tf_visit(lx, PLAIN, 1), tf_fresh(PLAIN, 1, 16, tmp))
    assert pipe.load_lora_weights(str(tmp / "r4")) == 25
    with pytest.raises(RuntimeError, match="set_conditioning"):
        step(e, PLAIN, 1, 0)
    assert same(tf_visit(lx, PLAIN, 1), tf_fresh(PLAIN, 1))
    assert same(tf_visit(lx, INDEP, 0), tf_fresh(INDEP, 0))
    assert not torch.equal(tf_fresh(PLAIN, 1)[0], tf_fresh(PLAIN, 1, 16, tmp)[0])
