"""Every Linear of the tiny model (tests.helpers.TINY: D = 256, 2 + 2 blocks) that a LoRA file can name, ONE module at a time: the
catalogue, the adapter values, the inputs and a float64 reference of what the adapter of one entry does to the output
(tests/test_lora_modules_cpu.py checks that the reference discriminates, tests/test_lora_modules_gpu.py holds the engine to it).

Entries are grouped the way the loaders group them (weights.lora_layout): the q/k/v Linears of a double block are one entry, to_k, to_v,
to_q and proj_mlp of a single block one. An entry is
  governed   the module is in one of the reference's enable_lora(...) lists (src/flux/block.py:23,152,191,256,294,325 and
             transformer.py:91 of the reference): its adapter is on for the condition rows, and for the image rows (the single blocks'
             text rows with them) under model_config["latent_lora"];
  always_on  it is in none: peft evaluates the adapter on every row that passes through the module. The engine cannot, and the loaders
             refuse such a checkpoint (weights.unevaluated_lora_modules).
The modulation Linears (norm1.linear / norm.linear) are installed for all blocks or none: "one module" is every block present, with a
zero up matrix except in the block under test.

The reference is the oracle (oracle.flux_ref) in float64 on a copy of the tiny model in which every lora_B is zero except the entry's.
always_on modules are plain nn.Linear in the oracle model; the copy holds an oracle.flux_modules.LoraLinear with the same base weights
in their place, which the oracle's mod(x) call sites evaluate on every row.

Adapter values: rank 4, A ~ N(0, 1/sqrt(K)) rounded to bf16 (what the engine's `down` holds), B ~ N(0, 1) fp32 times a gain found on the
CPU so that rho = |delta_ref| / |y_ref| lies in RHO_WINDOW, delta_ref = y_ref(with the adapter) - y_ref(up = 0). The gain aims at the
lower part of the window: there the output is still nearly linear in the adapter, so that a half-scale adapter is ~0.5 away from the
right one (the CPU test's mutant floor) and not hidden by saturation. An adapter that cannot reach the output (delta_ref exactly 0) is
flagged unreachable: the last single block's `out` without latent_lora, which acts on condition rows nothing reads afterwards.
Six entries reach the output only through the LayerNorm of the condition stream when latent_lora is off (bounded_reach()): their rho
saturates below the window whatever the adapter. Their B is not drawn but chosen where the output is most sensitive (sensitive_up), and
their gain is as large as the half-scale mutant's floor allows (rho 0.04 ... 0.1); the gemm_fp8 arm runs them at a raised gain."""
import contextlib
import copy
import functools
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from oracle import flux_modules as fm
from oracle import flux_ref as fr
from tests.helpers import TINY, tiny_transformer

RANK = 4
MODEL_SEED = 5
D = TINY["heads"] * TINY["head_dim"]
RHO_WINDOW = (0.3, 1.0)
RHO_AIM = (0.33, 0.5)               # where the gain search stops
# Entries of bounded reach (bounded_reach()): rho saturates below the window whatever the adapter, so the window cannot be met. Their up
# matrix is chosen where the output is most sensitive (sensitive_up) and their gain is the largest of a ladder at which the half-scale
# mutant is still HALF_AT_GAIN from the reference (the floor 0.45 with a margin): as much signal as the linear range holds. The gemm_fp8
# arm, whose noise that signal does not clear, runs with the gain raised until the half-scale mutant is HALF_AT_RAISED away: still above CAP.
HALF_AT_GAIN = 0.47
HALF_AT_RAISED = 0.34
CAP = 0.30                           # the GPU test's cap on relerr(delta_eng, delta_ref), every mode
MUTANT_FLOOR = 0.45                  # every mutant of the reference is at least this far from it: what makes CAP discriminate

SHAPES = {"aligned": (32, 8, 8), "ragged": (20, 6, 8)}          # (T, h, w): N = C = h w = 64 | 48
TIMESTEPS = (0.8, 0.3)
# name -> (model_config, lora_scale). "independent": the second of two forwards at different timesteps, so that the engine's cached
# condition stream is the one the adapter produced. The *_half arms leave the LayerNorm-fused down-projection (lora_scale != 1).
CONFIGS = {"plain": ((), 1.0), "latent_lora": ((("latent_lora", True),), 1.0), "independent": ((("independent_condition", True),), 1.0),
           "plain_half": ((), 0.5), "latent_lora_half": ((("latent_lora", True),), 0.5)}


class Entry(NamedTuple):
    name: str                        # the loaders' fused name ("d0.qkv", "s1.fused", "x_embedder"), or "<block>.<modulation Linear>"
    kind: str                        # "governed" | "always_on"
    modules: Tuple[str, ...]         # diffusers module names, in the fused GEMM's row order
    block: Optional[Tuple[str, int]] = None      # ("double", i) | ("single", j) | None: a global module
    mod: bool = False                # a modulation Linear: installed for every block, up = 0 except here

    def neighbour(self) -> Optional[str]:
        """the same entry of the other block"""
        if self.block is None:
            return None
        return self.name.replace(f"{self.name[0]}{self.block[1]}.", f"{self.name[0]}{1 - self.block[1]}.", 1)


def _catalogue() -> List[Entry]:
    out = []
    for i in range(TINY["num_layers"]):
        p, b = f"transformer_blocks.{i}.", ("double", i)
        g = lambda n, *m: out.append(Entry(f"d{i}.{n}", "governed", tuple(p + x for x in m), b))
        a = lambda n, *m: out.append(Entry(f"d{i}.{n}", "always_on", tuple(p + x for x in m), b))
        g("qkv", "attn.to_k", "attn.to_v", "attn.to_q"); g("out", "attn.to_out.0"); g("ff2", "ff.net.2")
        a("ff1", "ff.net.0.proj"); a("qkv_txt", "attn.add_k_proj", "attn.add_v_proj", "attn.add_q_proj"); a("out_txt", "attn.to_add_out")
        a("ff1_txt", "ff_context.net.0.proj"); a("ff2_txt", "ff_context.net.2")
        out.append(Entry(f"d{i}.norm1.linear", "governed", (p + "norm1.linear",), b, True))
        a("norm1_context.linear", "norm1_context.linear")
    for j in range(TINY["num_single_layers"]):
        p, b = f"single_transformer_blocks.{j}.", ("single", j)
        out.append(Entry(f"s{j}.fused", "governed", tuple(p + x for x in ("attn.to_k", "attn.to_v", "attn.to_q", "proj_mlp")), b))
        out.append(Entry(f"s{j}.out", "governed", (p + "proj_out",), b))
        out.append(Entry(f"s{j}.norm.linear", "governed", (p + "norm.linear",), b, True))
    out.append(Entry("x_embedder", "governed", ("x_embedder",)))
    out += [Entry(n, "always_on", (n,)) for n in ("context_embedder", "proj_out", "norm_out.linear")]
    out.append(Entry("time_text_embed", "always_on", ("time_text_embed.timestep_embedder.linear_1",)))
    return out


CATALOGUE = _catalogue()
ENTRY = {e.name: e for e in CATALOGUE}
GOVERNED = [e for e in CATALOGUE if e.kind == "governed"]
ALWAYS_ON = [e for e in CATALOGUE if e.kind == "always_on"]
MOD_MODULES = [e.modules[0] for e in CATALOGUE if e.mod]            # in packed order: double blocks, then single blocks
_LAST_SINGLE_OUT = f"s{TINY['num_single_layers'] - 1}.out"


def unreachable(entry: Entry, config: str) -> bool:
    """The adapter acts only on rows nothing reads afterwards: the last single block's proj_out on the condition rows."""
    return entry.name == _LAST_SINGLE_OUT and not dict(CONFIGS[config][0]).get("latent_lora", False)


def bounded_reach(entry: Entry, config: str) -> bool:
    """Without latent_lora the adapters of x_embedder and of the residual projections (to_out.0, ff.net.2, proj_out) move the condition
    stream's residual alone. The image rows see that only through the keys and values of the following blocks, which are projections of
    the LayerNorm of that residual: however large the adapter, the condition tokens' keys and values stay of the same size and the image
    rows give them the same share of their attention. Measured on the float64 reference (aligned shape, gains 0.01 ... 100 on B ~ N(0, 1)),
    rho saturates at: d0.out 0.115, d0.ff2 0.087, d1.out 0.097, d1.ff2 0.086, s0.out 0.059, x_embedder 0.108 -- against 1.1 ... 1.4 for
    every other entry, and for these too under latent_lora. With the up matrix of sensitive_up the ceilings are 0.13 ... 0.24: still
    below the window."""
    if dict(CONFIGS[config][0]).get("latent_lora", False) or unreachable(entry, config):
        return False
    return entry.name == "x_embedder" or entry.name.endswith((".out", ".ff2"))


def relerr(a, b) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------ model, adapters
def _get(root, path: str):
    for p in path.split("."):
        root = root[int(p)] if p.isdigit() else getattr(root, p)
    return root


def _set(root, path: str, new) -> None:
    head, _, last = path.rpartition(".")
    parent = _get(root, head) if head else root
    if last.isdigit():
        parent[int(last)] = new
    else:
        setattr(parent, last, new)


@functools.lru_cache(maxsize=None)
def base_model():
    """tiny_transformer(lora=True), fp32, as the checkpoint holds it (its own adapters are not used: base_state_dict drops them)."""
    return tiny_transformer(seed=MODEL_SEED)


@functools.lru_cache(maxsize=None)
def base_state_dict() -> Dict[str, torch.Tensor]:
    """The tiny model without adapters, under the plain diffusers names: what the engines of the GPU test are packed from."""
    return {k.replace(".base_layer.", "."): v.detach().clone() for k, v in base_model().state_dict().items() if ".lora_" not in k}


@functools.lru_cache(maxsize=None)
def ref_model():
    """The float64 copy the reference runs on: every catalogue module a LoraLinear (the always_on ones swapped in over the same base
    weights), every lora_B zero. assign() writes the adapters of one run into it."""
    tr = copy.deepcopy(base_model()).double()
    for e in CATALOGUE:
        for path in e.modules:
            m = _get(tr, path)
            if not isinstance(m, fm.LoraLinear):
                new = fm.LoraLinear(m.in_features, m.out_features, r=RANK, lora_alpha=float(RANK)).double()
                new.base_layer.weight.data.copy_(m.weight.data)
                new.base_layer.bias.data.copy_(m.bias.data)
                _set(tr, path, new)
    for m in tr.modules():
        if isinstance(m, fm.LoraLinear):
            assert m.r == RANK and m.scaling["default"] == 1.0
            m.lora_B["default"].weight.data.zero_()
    return tr.eval()


@functools.lru_cache(maxsize=None)
def drawn(path: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(A [r, K] fp32 holding bf16 values, B [N, r] fp32 ~ N(0, 1)) of one module, from a seed of its own"""
    m = _get(ref_model(), path)
    g = torch.Generator().manual_seed(7000 + sorted(p for e in CATALOGUE for p in e.modules).index(path))
    A = (torch.randn(RANK, m.in_features, generator=g) / m.in_features ** 0.5).to(torch.bfloat16).float()
    return A, torch.randn(m.out_features, RANK, generator=g)


def adapter(entry: Entry, gain: float, values_of: Optional[Entry] = None, rotate: int = 0, zero_up: bool = False,
            up: Optional[torch.Tensor] = None) -> Dict[str, Tuple]:
    """module -> (A, B) of the one-entry adapter. values_of: the (A, B) drawn for another entry of the same form (the neighbouring
    block's); rotate: module j's up matrix reads module j + rotate's down-projection (the slabs of a fused group out of place).
    up: the unit-norm up matrix chosen for a one-module entry of bounded reach (sensitive_up) in place of the drawn one; the neighbour's
    drawn matrix is then brought to unit norm too."""
    src = (values_of or entry).modules
    n = len(src)
    out = {}
    for j, path in enumerate(entry.modules):
        B = drawn(src[j])[1] * gain
        if up is not None:
            B = (up if values_of is None else drawn(src[j])[1] / drawn(src[j])[1].norm()) * gain
        out[path] = (drawn(src[(j + rotate) % n])[0], torch.zeros_like(B) if zero_up else B)
    if entry.mod:
        for path in MOD_MODULES:
            if path not in out:
                out[path] = (drawn(path)[0], torch.zeros_like(drawn(path)[1]))
    return out


def lora_state_dict(ad: Dict[str, Tuple], prefix: str = "transformer.") -> Dict[str, torch.Tensor]:
    """The LoRA-only state dict of an adapter (the keys of a pytorch_lora_weights.safetensors)"""
    sd = {}
    for path, (A, B) in ad.items():
        sd[f"{prefix}{path}.lora_A.weight"], sd[f"{prefix}{path}.lora_B.weight"] = A.contiguous(), B.contiguous()
    return sd


def wrapped_state_dict(ad: Dict[str, Tuple]) -> Dict[str, torch.Tensor]:
    """The whole model as a PEFT-wrapped state dict with this adapter (base_layer / lora_A.default / lora_B.default keys)"""
    sd = {}
    for k, v in base_state_dict().items():
        path, _, what = k.rpartition(".")
        sd[f"{path}.base_layer.{what}" if path in ad else k] = v
    for path, (A, B) in ad.items():
        sd[f"{path}.lora_A.default.weight"], sd[f"{path}.lora_B.default.weight"] = A.contiguous(), B.contiguous()
    return sd


def assign(tr, ad: Dict[str, Tuple], scale: float = 1.0) -> None:
    """Make `ad` at `scale` the only adapter of the reference model."""
    for m in tr.modules():
        if isinstance(m, fm.LoraLinear):
            m.lora_B["default"].weight.data.zero_()
            m.scaling["default"] = 1.0
    for path, (A, B) in ad.items():
        m = _get(tr, path)
        m.lora_A["default"].weight.data.copy_(A)
        m.lora_B["default"].weight.data.copy_(B)
        m.scaling["default"] = float(scale)


@contextlib.contextmanager
def row_rule(mods, rule: Optional[str]):
    """Mutants of the oracle's row selection for the modules `mods`: "image_too" = the adapter on for every call, "cond_only" = on for
    the condition call alone. (The oracle calls each governed module once for the image rows, then once for the condition rows.)"""
    if rule is None:
        yield
        return
    ids, count, real = {id(m) for m in mods}, {}, fr._linear

    def lin(mod, x, lora_on):
        if id(mod) in ids:
            k = count[id(mod)] = count.get(id(mod), -1) + 1
            lora_on = True if rule == "image_too" else k % 2 == 1
        return real(mod, x, lora_on)

    fr._linear = lin
    try:
        yield
    finally:
        fr._linear = real
        assert all((c + 1) % 2 == 0 for c in count.values()), count


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def data(shape: str) -> Dict:
    """CPU fp32 inputs of a shape, B = 2: two (latents, timestep) steps on one conditioning."""
    T, h, w = SHAPES[shape]
    N, B = h * w, 2
    g = torch.Generator().manual_seed(300 + len(shape))
    d = dict(enc=torch.randn(B, T, TINY["joint_dim"], generator=g) * 0.5, pooled=torch.randn(B, TINY["pooled_dim"], generator=g),
             guid=torch.full((B,), 3.5), ids=fm.prepare_latent_image_ids(h, w), tids=torch.zeros(T, 3),
             cond=torch.randn(B, N, TINY["in_channels"], generator=g), cids=fm.prepare_latent_image_ids(h, w))
    d["cids"][:, 2] -= w
    d["steps"] = [(torch.randn(B, N, TINY["in_channels"], generator=g), torch.full((B,), t)) for t in TIMESTEPS]
    return d


def step_of(config: str) -> int:
    return 1 if config == "independent" else 0


def oracle_forward(tr, shape: str, config: str, grad: bool = False) -> torch.Tensor:
    d = data(shape)
    lat, t = d["steps"][step_of(config)]
    f = torch.float64
    with torch.enable_grad() if grad else torch.no_grad():
        return fr.tranformer_forward(tr, d["cond"].to(f), d["cids"], None, dict(CONFIGS[config][0]), hidden_states=lat.to(f),
                                     encoder_hidden_states=d["enc"].to(f), pooled_projections=d["pooled"].to(f), timestep=t.to(f),
                                     img_ids=d["ids"], txt_ids=d["tids"], guidance=d["guid"].to(f))[0]


@functools.lru_cache(maxsize=None)
def block_data(shape: str) -> Dict:
    """Inputs of a block-level call: the three streams, temb, cond_temb, the RoPE tables."""
    T, h, w = SHAPES[shape]
    N, B = h * w, 2
    g = torch.Generator().manual_seed(400 + len(shape))
    d = data(shape)
    pe = fm.FluxPosEmbed(10000.0, (16, 56, 56))
    return dict(hid=torch.randn(B, N, D, generator=g) * 0.5, enc=torch.randn(B, T, D, generator=g) * 0.5, cond=torch.randn(B, N, D, generator=g) * 0.5,
                temb=torch.randn(B, D, generator=g), ctemb=torch.randn(B, D, generator=g), T=T,
                rope_main=pe(torch.cat([d["tids"], d["ids"]], 0)), rope_cond=pe(d["cids"]))


def oracle_block(tr, entry: Entry, shape: str, config: str) -> Tuple[torch.Tensor, ...]:
    """The streams oracle.flux_ref.block_forward / single_block_forward return for the entry's block: (text, image, condition) or
    ([text; image], condition)."""
    d, f = block_data(shape), torch.float64
    kind, idx = entry.block
    mc = dict(CONFIGS[config][0])
    hid, enc, cond, temb, ctemb = (d[k].to(f) for k in ("hid", "enc", "cond", "temb", "ctemb"))
    with torch.no_grad():
        if kind == "double":
            return tuple(fr.block_forward(tr.transformer_blocks[idx], hid, enc, cond, temb, ctemb, d["rope_cond"], d["rope_main"], mc))
        return tuple(fr.single_block_forward(tr.single_transformer_blocks[idx], torch.cat([enc, hid], 1), temb, d["rope_main"], cond, ctemb,
                                             d["rope_cond"], mc))


# ------------------------------------------------------------------------------------------------------------------ the reference
class Ref(NamedTuple):
    gain: float                      # on the drawn B
    rho: float                       # |delta| / |y1| (0.0: unreachable)
    y0: object                       # the output with up = 0 (a tensor, or a tuple of streams for a block-level reference)
    y1: object
    delta: object
    up: Optional[torch.Tensor] = None      # bounded reach: the chosen unit-norm up matrix (adapter(up=...))
    raised: Optional["Ref"] = None         # bounded reach: the same at the larger gain the gemm_fp8 arm runs with (y0 shared)


def _cat(y):
    return y if isinstance(y, torch.Tensor) else torch.cat([s.reshape(-1) for s in y])


def _sub(a, b):
    return a - b if isinstance(a, torch.Tensor) else tuple(x - y for x, y in zip(a, b))


def _reference(run, entry: Entry, config: str, aim=RHO_AIM) -> Ref:
    """The gain search: `run(adapter, scale)` is the float64 forward. rho grows with the gain; a few steps of gain *= aim / rho land it."""
    tr, scale = ref_model(), CONFIGS[config][1]
    y0 = run(adapter(entry, 1.0, zero_up=True), scale)
    gain = 0.25
    for _ in range(12):
        y1 = run(adapter(entry, gain), scale)
        delta = _sub(y1, y0)
        rho = float(_cat(delta).norm() / _cat(y1).norm())
        if rho == 0.0 or aim[0] <= rho <= aim[1]:
            break
        gain *= min(max(0.5 * (aim[0] + aim[1]) / rho, 0.1), 10.0)
    assign(tr, {})
    return Ref(gain, rho, y0, y1, delta)


@functools.lru_cache(maxsize=None)
def sensitive_up(name: str, shape: str) -> torch.Tensor:
    """The unit-norm up matrix of a bounded-reach entry (one module): from the drawn B, two steps of power iteration on J^T J, J the
    Jacobian of the reference's output with respect to B at B = 0 (config "plain") -- J B by a small finite step, J^T u by autograd. The
    direction in which a perturbation of the condition stream's residual of a given size moves the output most (6 ... 8 times a random
    one): more delta before the LayerNorm of that residual saturates."""
    entry, tr = ENTRY[name], ref_model()
    (path,) = entry.modules
    A, B = drawn(path)
    w = _get(tr, path).lora_B["default"].weight
    assign(tr, {path: (A, torch.zeros_like(B))})
    y0 = oracle_forward(tr, shape, "plain")
    B = B / B.norm()
    for _ in range(2):
        assign(tr, {path: (A, 1e-3 * B)})
        u = oracle_forward(tr, shape, "plain") - y0
        assign(tr, {path: (A, torch.zeros_like(B))})
        w.grad = None
        (u / u.norm() * oracle_forward(tr, shape, "plain", grad=True)).sum().backward()
        B = (w.grad / w.grad.norm()).float()
        w.grad = None
    for p in tr.parameters():
        p.grad = None
    assign(tr, {})
    return B


@functools.lru_cache(maxsize=None)
def _bounded_gains(name: str, shape: str, base: str) -> Tuple[float, float]:
    """(gain, raised gain) of a bounded-reach entry at lora_scale 1 under config `base` ("plain" | "independent"): the largest gain of
    a ladder (x 1.5 from rho ~ 0.03) at which the half-scale mutant is still HALF_AT_GAIN from the reference, and -- three bisection
    steps past the ladder's last such rung -- the largest at which it is still HALF_AT_RAISED away."""
    entry, tr, up = ENTRY[name], ref_model(), sensitive_up(name, shape)

    def delta(gain, scale):
        assign(tr, adapter(entry, gain, up=up), scale)
        y = oracle_forward(tr, shape, base)
        return y - y0, y

    def half(gain):
        return relerr(delta(gain, 0.5)[0], delta(gain, 1.0)[0])

    assign(tr, {})
    y0 = oracle_forward(tr, shape, base)
    d, y = delta(1.0, 1.0)
    g = 0.03 / float(d.norm() / y.norm())
    gain = raised = None
    for _ in range(16):
        h = half(g)
        if h >= HALF_AT_GAIN:
            gain = g
        if h < HALF_AT_RAISED:
            break
        raised = g
        g *= 1.5
    assert gain is not None and raised is not None and raised > gain, (name, shape, base, gain, raised)
    lo, hi = raised, g
    for _ in range(3):
        mid = (lo * hi) ** 0.5
        lo, hi = (mid, hi) if half(mid) >= HALF_AT_RAISED else (lo, mid)
    assign(tr, {})
    return gain, lo


@functools.lru_cache(maxsize=None)
def reference(name: str, shape: str, config: str) -> Ref:
    """delta_ref of one entry at one shape under one config, whole model. Asserts rho's window (exactly 0 for an unreachable entry; for
    an entry of bounded reach: below the window, which is why it is one)."""
    entry, tr = ENTRY[name], ref_model()

    def run(ad, scale):
        assign(tr, ad, scale)
        return oracle_forward(tr, shape, config)

    if bounded_reach(entry, config):
        up, scale = sensitive_up(name, shape), CONFIGS[config][1]
        y0 = run(adapter(entry, 1.0, zero_up=True, up=up), scale)
        refs = []
        for g in _bounded_gains(name, shape, "independent" if config == "independent" else "plain"):
            y1 = run(adapter(entry, g / scale, up=up), scale)
            refs.append(Ref(g / scale, float((y1 - y0).norm() / y1.norm()), y0, y1, y1 - y0, up))
        assign(tr, {})
        assert 0.0 < refs[0].rho < refs[1].rho < RHO_WINDOW[0], (name, shape, config, refs[0].rho, refs[1].rho)
        return refs[0]._replace(raised=refs[1])
    ref = _reference(run, entry, config)
    if unreachable(entry, config):
        assert ref.rho == 0.0 and not bool(ref.delta.any()), (name, shape, config, ref.rho)
    else:
        assert RHO_WINDOW[0] <= ref.rho <= RHO_WINDOW[1], (name, shape, config, ref.rho)
    return ref


@functools.lru_cache(maxsize=None)
def block_reference(name: str, shape: str, config: str) -> Ref:
    """The same for the block-level call on the entry's block: y0, y1, delta are tuples of streams; rho over all of them. (Every
    adapter reaches a stream a block returns.)"""
    entry, tr = ENTRY[name], ref_model()

    def run(ad, scale):
        assign(tr, ad, scale)
        return oracle_block(tr, entry, shape, config)

    ref = _reference(run, entry, config)
    assert RHO_WINDOW[0] <= ref.rho <= RHO_WINDOW[1], (name, shape, config, ref.rho)
    return ref


def mutant_delta(name: str, shape: str, config: str, mutant: str, raised: bool = False) -> Optional[torch.Tensor]:
    """delta of a mutant of the reference of (entry, shape, config), at the reference's gain (raised: at its raised gain, bounded-reach
    entries only); None where the mutant does not exist.
      dropped     no adapter term            half        the adapter at half scale
      rows        condition rows only where latent_lora says image too, and image rows too where it does not
      rotated     the slabs of a fused group rotated by one (module j's up matrix on module j + 1's down-projection)
      neighbour   the adapter drawn for the same entry of the other block"""
    entry, tr, ref = ENTRY[name], ref_model(), reference(name, shape, config)
    if raised:
        ref = ref.raised
    scale, rule = CONFIGS[config][1], None
    ad = adapter(entry, ref.gain, up=ref.up)
    if mutant == "dropped":
        ad = adapter(entry, ref.gain, zero_up=True, up=ref.up)
    elif mutant == "half":
        scale *= 0.5
    elif mutant == "rows":
        rule = "cond_only" if dict(CONFIGS[config][0]).get("latent_lora", False) else "image_too"
    elif mutant == "rotated":
        if len(entry.modules) == 1:
            return None
        ad = adapter(entry, ref.gain, rotate=1)
    elif mutant == "neighbour":
        if entry.neighbour() is None:
            return None
        ad = adapter(entry, ref.gain, values_of=ENTRY[entry.neighbour()], up=ref.up)
    else:
        raise KeyError(mutant)
    assign(tr, ad, scale)
    with row_rule([_get(tr, p) for p in entry.modules], rule):
        y = oracle_forward(tr, shape, config)
    assign(tr, {})
    return y - ref.y0


MUTANTS = ("dropped", "half", "rows", "rotated", "neighbour")
