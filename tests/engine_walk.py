"""The engine walk: a catalogue of engine states, their inputs, what a freshly built engine gives for each, and the plan that takes ONE
long-lived engine through every ordered pair of them (tests/test_engine_walk_cpu.py checks the plan, tests/test_engine_walk_gpu.py walks it).

A state is everything set_conditioning() is given besides the data: shape, batch, model_config, c_factor, the form of the attention mask,
the active adapters with their weights and lora_scale. Visiting a state = selecting its adapters, one set_conditioning() and three
forward() calls (a capture, a replay -- with the condition stream cached where the mode caches it -- and the first input again).
Every state has two data sets; consecutive visits to one state alternate between them, so data left behind by the previous conditioning
(a cached condition stream, a mask prep, modulation tables) shows as surely as a mode left behind.

The model is the tiny one (tests.helpers.tiny_transformer(seed=5): 2 + 2 blocks, D = 256) packed with precise=True, so that one engine can
reach every mode. Weights packed for precise mode take adapters of at most 4 stacked columns per module (weights._one_lora_rank: the fused
single-block GEMM evaluates four adapters from one 16-column slab), so the two named adapters that state "two_adapters" stacks are
rank 2 each: "default" is tests/test_lora_wide_gpu.rank_model(2)'s set, "b" the same modules redrawn from another seed
(tests/test_lora_rank_cpu.with_rank). The events that need a wider adapter (a rank-16 file) run on a transformer packed without precise.

`fresh(state, seed)` is the reference of the walk: the three outputs of a newly packed model on a new engine taken through that one visit."""
import contextlib
import copy
import functools
import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from oracle import flux_modules as fm
from oracle import flux_ref as fr
from tests.test_attn_mask_gpu import _MaskedF
from tests.test_engine_gpu import TOL
from tests.test_fp8_gpu import TOL_FP8                      # 7e-2: what test_lora_wide_gpu / test_cond_cache_modes_gpu hold attn_fp8 forwards to
from tests.test_lora_rank_cpu import _cfg, _lora_only, with_rank
from tests.test_lora_wide_gpu import rank_model
from tests.test_precise_cond_cache_gpu import TOL_P

TOL_GEMM_FP8 = 0.15      # test_fp8_gemm_gpu.test_engine_fp8_gemm_mode_against_reference_goldens' bound (a literal there: nothing to import)
BOUNDS = {"bf16": TOL, "fp16": TOL, "precise": TOL_P, "attn_fp8": TOL_FP8, "gemm_fp8": TOL_GEMM_FP8}

RANK = 2                                                     # per adapter; "default" + "b" stack to 4
SEED_B = 102                                                 # with_rank's seed for adapter "b" ("default" is rank_model(2): seed 2)
SHAPES = {"aligned": (32, 8, 8), "ragged": (24, 6, 10)}     # (T, h, w) as in tests/test_cond_cache_modes_gpu.py: N = 64 | 60
TIMESTEPS = (0.8, 0.3, 0.8)
H = 2                                                        # attention heads of the tiny model


class State(NamedTuple):
    name: str
    shape: str                                   # key of SHAPES
    mc: Tuple = ()                               # model_config items
    mode: str = "bf16"                           # key of BOUNDS: the arithmetic mode the config selects
    B: int = 2
    cond: Optional[Tuple[int, int]] = None       # (h, w) of the condition image; None: the image's own; (0, 0): no condition stream
    c_factor: Optional[float] = None
    mask: Optional[str] = None                   # "keypad": bool [B, 1, 1, S] | "additive": fp32 [1, H, S, S] with -inf entries
    adapters: Tuple = ("default",)
    weights: Tuple = ()                          # set_adapters' weights, as items
    lora_scale: float = 1.0

    @property
    def model_config(self) -> Dict:
        return dict(self.mc)

    def dims(self) -> Tuple[int, int, int]:
        """(T, N, C)"""
        T, h, w = SHAPES[self.shape]
        ch, cw = (h, w) if self.cond is None else self.cond
        return T, h * w, ch * cw


def _mc(**kw):
    return tuple(sorted(kw.items()))


CATALOGUE: List[State] = [
    State("plain", "aligned"),
    State("plain_ragged", "ragged"),
    State("no_condition", "aligned", cond=(0, 0)),
    State("batch1", "aligned", B=1),
    State("short_condition", "aligned", cond=(4, 8)),                                     # C = 32 != N
    State("independent", "aligned", _mc(independent_condition=True)),
    State("no_union_latent_lora_ragged", "ragged", _mc(union_cond_attn=False, latent_lora=True)),
    State("c_factor", "aligned", c_factor=0.5),
    State("add_cond_attn", "aligned", _mc(add_cond_attn=True)),
    State("fp16", "aligned", _mc(operands="fp16"), "fp16"),
    State("fp16_independent_ragged", "ragged", _mc(operands="fp16", independent_condition=True), "fp16"),
    State("attn_fp8_independent", "aligned", _mc(attn_fp8=True, independent_condition=True), "attn_fp8"),
    State("gemm_fp8", "aligned", _mc(gemm_fp8=True), "gemm_fp8"),
    State("precise_independent", "aligned", _mc(precise=True, independent_condition=True), "precise"),
    State("precise_ragged", "ragged", _mc(precise=True), "precise"),
    State("keypad_mask", "aligned", mask="keypad"),
    State("additive_mask", "aligned", mask="additive"),
    State("two_adapters", "aligned", adapters=("default", "b"), weights=(("b", (0.3, 1.0)),), lora_scale=0.5),
    # Beyond the 18 the walk started from. attn_fp8 under union attention: no condition cache, so q / k / V^T go to the shared e4m3 images
    # Q8 / K8 / VT8, which "attn_fp8_independent" never writes (its keys and V^T live in the per-layer KC8 / VTC8). Aligned: written by the
    # projection epilogue; ragged: by lx_qkv_prep_fp8_segs, with pad slots in every 64-key tile of VT8.
    State("attn_fp8_union", "aligned", _mc(attn_fp8=True), "attn_fp8"),
    State("attn_fp8_union_ragged", "ragged", _mc(attn_fp8=True), "attn_fp8"),
]
N_STATES = len(CATALOGUE)
INDEX = {s.name: i for i, s in enumerate(CATALOGUE)}
STATE = {s.name: s for s in CATALOGUE}


# ------------------------------------------------------------------------------------------------------------------ the plan
def euler_circuit(n: int) -> List[int]:
    """A closed walk over the complete digraph on n nodes, self-loops included, that takes each of its n^2 edges once (Hierholzer; every
    node has n edges in and n out, so the circuit exists). n^2 + 1 nodes, first = last = 0."""
    stride = next(s for s in (7, 11, 13, 1) if math.gcd(s, n) == 1)          # (an order of the edges that does not simply count up)
    nxt = [[(a + 1 + stride * k) % n for k in range(n)] for a in range(n)]    # unused edges out of every node, popped from the end
    stack, walk = [0], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


class Visit(NamedTuple):
    state: int
    seed: int            # the data set: alternates over the visits to this state
    prev: Tuple          # the (up to two) states visited before, oldest first


@functools.lru_cache(maxsize=None)
def plan() -> Tuple[Visit, ...]:
    seen = [0] * N_STATES
    out, walk = [], euler_circuit(N_STATES)
    for k, s in enumerate(walk):
        out.append(Visit(s, seen[s] % 2, tuple(walk[max(k - 2, 0):k])))
        seen[s] += 1
    return tuple(out)


def chunks() -> List[Tuple[int, int]]:
    """The plan in N_STATES pieces of consecutive visits, as [first, end) index pairs: one test each."""
    n = len(plan())
    edges = [round(k * n / N_STATES) for k in range(N_STATES + 1)]
    return list(zip(edges[:-1], edges[1:]))


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def data(st: State, seed: int) -> Dict:
    """Data set `seed` of a state (CPU tensors). States of one shape share the text, pooled and latent tensors of a seed, so that two of
    them differ by their mode alone; the masks differ per data set."""
    T, h, w = SHAPES[st.shape]
    N, B = h * w, st.B
    g = torch.Generator().manual_seed(1000 + 10 * seed + (0 if st.shape == "aligned" else 1))
    d = dict(enc=torch.randn(2, T, 64, generator=g)[:B] * 0.5, pooled=torch.randn(2, 32, generator=g)[:B],
             lats=[torch.randn(2, N, 64, generator=g)[:B].contiguous() for _ in range(2)], guid=torch.full((B,), 3.5 - seed),
             ids=fm.prepare_latent_image_ids(h, w), tids=torch.zeros(T, 3), cond=None, cids=None, mask=None)
    ch, cw = (h, w) if st.cond is None else st.cond
    cond = torch.randn(2, h * w, 64, generator=g)[:B, : ch * cw].contiguous()
    if ch * cw:
        d["cond"] = cond
        d["cids"] = fm.prepare_latent_image_ids(ch, cw)
        d["cids"][:, 2] -= w
    S = T + N + ch * cw
    if st.mask == "keypad":                      # the text keys past each image's prompt length are padding
        keep = [(T // 2, T // 2 - 1), (T - 12, 9)][seed]
        m = torch.ones(B, 1, 1, S, dtype=torch.bool)
        for b in range(B):
            m[b, 0, 0, keep[b]:T] = False
        d["mask"] = m
    elif st.mask == "additive":                  # every query keeps its own key (a row without keys is NaN in the oracle's SDPA)
        gm = torch.Generator().manual_seed(31 + seed)
        m = torch.randn(1, H, S, S, generator=gm)
        m[torch.rand(1, H, S, S, generator=gm) < 0.25] = float("-inf")
        m[0, :, torch.arange(S), torch.arange(S)] = 0.0
        d["mask"] = m
    d["enc"], d["pooled"] = d["enc"].contiguous(), d["pooled"].contiguous()
    d["steps"] = [(d["lats"][k % 2], torch.full((B,), TIMESTEPS[k])) for k in range(3)]
    return d


# ------------------------------------------------------------------------------------------------------------------ model, oracle
@functools.lru_cache(maxsize=None)
def adapter_b_sd() -> Dict[str, torch.Tensor]:
    """The rank-2 model's state dict with every adapter redrawn from SEED_B: adapter "b" under the oracle's "default" key names"""
    return with_rank(rank_model(RANK)[1], RANK, seed=SEED_B)


def packed(device="cuda", precise=True, sd=None):
    """A newly packed model: adapter "default" (active) from the checkpoint `sd` (default: rank_model(RANK)'s), "b" installed beside it."""
    from loongx_amd.flux.weights import install_lora, pack_state_dict
    tr, sd0, _ = rank_model(RANK)
    pw = pack_state_dict(sd0 if sd is None else sd, _cfg(tr), device, precise=precise)
    assert install_lora(pw, _lora_only(adapter_b_sd()), adapter_name="b") == 25
    return pw


def new_engine(device="cuda", sd=None):
    from loongx_amd.flux.engine import DiTEngine
    return DiTEngine(packed(device, sd=sd), device)


@functools.lru_cache(maxsize=None)
def other_state_dict() -> Dict[str, torch.Tensor]:
    """Another weight set of the same names and shapes: every tensor of the checkpoint moved by N(0, 0.01^2)."""
    g = torch.Generator().manual_seed(4242)
    return {k: v + 0.01 * torch.randn(v.shape, generator=g) for k, v in rank_model(RANK)[1].items()}


def overwrite_weights(pw, src) -> None:
    """What dist.broadcast_packed_weights does to a receiving rank, without the process group: every tensor the engine dereferences is
    overwritten IN PLACE with `src`'s (same names and shapes), weights_version moves and the bounded-score table is refreshed."""
    from loongx_amd.dist import refresh_q_log2
    assert set(pw.t) == set(src.t) and set(pw.lora) == set(src.lora) and list(pw.adapters) == list(src.adapters) and pw.active == src.active
    for k, t in pw.t.items():
        t.copy_(src.t[k])
    for k, lo in pw.lora.items():
        for a in ("down", "up", "down_lo"):
            if getattr(lo, a) is not None:
                getattr(lo, a).copy_(getattr(src.lora[k], a))
    for name, ad in pw.adapters.items():
        theirs = src.adapters[name].tensors()
        for k, v in ad.tensors().items():
            v.copy_(theirs[k])
    pw.weights_version = getattr(pw, "weights_version", 0) + 1
    refresh_q_log2(pw)


@functools.lru_cache(maxsize=None)
def oracle_model(adapters: Tuple, scalings: Tuple):
    """The oracle module with `adapters` active at `scalings` (one float each): as tests/test_lora_adapters_cpu.split_oracle builds it,
    the unmodified oracle.flux_modules.LoraLinear looping over its active adapters."""
    tr = copy.deepcopy(rank_model(RANK)[0])
    sdb = adapter_b_sd()
    for name, m in tr.named_modules():
        if isinstance(m, fm.LoraLinear):
            m.lora_A["b"] = torch.nn.Linear(m.in_features, RANK, bias=False)
            m.lora_B["b"] = torch.nn.Linear(RANK, m.out_features, bias=False)
            m.lora_A["b"].weight.data.copy_(sdb[f"{name}.lora_A.default.weight"])
            m.lora_B["b"].weight.data.copy_(sdb[f"{name}.lora_B.default.weight"])
            for a, s in zip(adapters, scalings):
                m.scaling[a] = float(s)
            m.active_adapters = list(adapters)
    return tr.eval()


@contextlib.contextmanager
def _oracle_mask(mask):
    """The oracle's SDPA receives `mask` wherever the oracle itself passes none (tests/test_attn_mask_forward_gpu.py's substitution)."""
    if mask is None:
        yield
        return
    real = fr.F
    fr.F = _MaskedF(mask)
    try:
        yield
    finally:
        fr.F = real


@functools.lru_cache(maxsize=None)
def oracle(st: State, seed: int) -> Tuple[torch.Tensor, ...]:
    """oracle.flux_ref.tranformer_forward (fp32, CPU) for the three forwards of a visit. Per-image adapter weights: image b comes from the
    oracle run whose scalings are image b's (tests/test_lora_adapters_gpu.test_per_image_weights)."""
    d = data(st, seed)
    wts = dict(st.weights)
    per_image = []
    for b in range(st.B):
        sc = []
        for a in st.adapters:
            w = wts.get(a, 1.0)
            sc.append(st.lora_scale * (w[b] if isinstance(w, tuple) else w))
        per_image.append(tuple(sc))
    outs = []
    for k in range(2):                           # the third forward repeats the first's inputs
        lat, t = d["steps"][k]
        rows = {}
        for sc in set(per_image):
            tr = oracle_model(st.adapters, sc)
            if st.c_factor is not None:
                tr = copy.deepcopy(tr)
                for m in tr.modules():
                    if hasattr(m, "to_q"):
                        m.c_factor = torch.ones(1, 1) * st.c_factor
            with torch.no_grad(), _oracle_mask(d["mask"]):
                rows[sc] = fr.tranformer_forward(tr, d["cond"], d["cids"], None, st.model_config, hidden_states=lat,
                                                 encoder_hidden_states=d["enc"], pooled_projections=d["pooled"], timestep=t,
                                                 img_ids=d["ids"], txt_ids=d["tids"], guidance=d["guid"])[0].float()
        outs.append(torch.stack([rows[per_image[b]][b] for b in range(st.B)]))
    return outs[0], outs[1], outs[0]


# ------------------------------------------------------------------------------------------------------------------ visiting
@functools.lru_cache(maxsize=None)
def device_data(st: State, seed: int) -> Dict:
    d = data(st, seed)
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items() if k not in ("lats", "steps")}
    dev["steps"] = [(lat.cuda(), t.cuda()) for lat, t in d["steps"]]
    return dev


def select_adapters(eng, st: State) -> None:
    eng.set_adapters(list(st.adapters), dict(st.weights) or None)
    eng.set_lora_scale(st.lora_scale)


def set_cond(eng, st: State, seed: int, **over) -> None:
    """set_conditioning() alone, with the adapters as they are; `over` replaces keyword arguments."""
    d = device_data(st, seed)
    kw = dict(c_t=0.0, model_config=st.model_config, c_factor=st.c_factor, attention_mask=d["mask"])
    kw.update(over)
    eng.set_conditioning(d["enc"], d["pooled"], d["guid"], d["tids"], d["ids"], d["cond"], d["cids"], **kw)


def condition(eng, st: State, seed: int) -> None:
    select_adapters(eng, st)
    set_cond(eng, st, seed)


def step(eng, st: State, seed: int, k: int, **kw) -> torch.Tensor:
    lat, t = device_data(st, seed)["steps"][k]
    return eng.forward(lat, t, **kw).float().cpu().clone()


def visit(eng, st: State, seed: int) -> List[torch.Tensor]:
    condition(eng, st, seed)
    return [step(eng, st, seed, k) for k in range(3)]


@functools.lru_cache(maxsize=None)
def fresh(st: State, seed: int, other: bool = False) -> Tuple[torch.Tensor, ...]:
    """The three outputs of a newly packed model on a new engine taken through this one visit (other: packed from other_state_dict())."""
    return tuple(visit(new_engine(sd=other_state_dict() if other else None), st, seed))
