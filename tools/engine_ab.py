#!/usr/bin/env python3
"""Bit-for-bit A/B of two versions of loongx_amd/flux/engine.py on the tiny model: the acceptance check of a refactor of that file.

    git show <commit>:loongx_amd/flux/engine.py > /tmp/engine_other.py
    python tools/engine_ab.py /tmp/engine_other.py

The other file is loaded as a sibling module inside the loongx_amd.flux package, so its relative imports resolve against the same ops and
the same library. One DiTEngine of each module is built on the same PackedWeights; every case runs set_conditioning and two forwards on
identical inputs and requires torch.equal on both velocities and on the final X, and equal f16_overflow_count(); a case both modules
must refuse requires the same exception from both. Weights:
tests/helpers.tiny_transformer() (2 + 2 blocks, 2 heads, D = 256). Inputs: tests/golden/flux_tiny.npz (16 / 16 / 16 tokens, which no
stream of 32 divides: the separate q / k / v pass) and a seeded 32 / 64 / 64 set (the fused projection epilogue and, with
independent_condition, the cached condition stream in the second forward). One line per case; exits non-zero on the first difference."""
import contextlib
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from loongx_amd import ops
from loongx_amd.flux import engine as engine_here
from loongx_amd.flux.weights import pack_state_dict
from oracle import flux_modules as fm
from tests.helpers import load, tiny_transformer
from tests.test_lora_rank_cpu import _cfg, with_rank

DEV = "cuda"


def load_sibling(path):
    spec = importlib.util.spec_from_file_location("loongx_amd.flux._engine_other", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def golden_inputs():
    G = load("flux_tiny.npz")
    return dict(enc=G["in_enc"], pooled=G["in_pooled"], guidance=G["in_guidance"], txt_ids=G["in_txt_ids"], img_ids=G["in_img_ids"],
                cond=G["in_cond"], cond_ids=G["in_cond_ids"], latents=G["in_latents"], timestep=G["in_timestep"])


def fused_inputs():
    g = torch.Generator().manual_seed(7)
    B, T, hw = 2, 32, 8
    N = hw * hw
    cids = fm.prepare_latent_image_ids(hw, hw)
    cids[:, 2] -= hw
    return dict(latents=torch.randn(B, N, 64, generator=g), enc=torch.randn(B, T, 64, generator=g) * 0.5, pooled=torch.randn(B, 32, generator=g),
                timestep=torch.tensor([0.8, 0.3]), img_ids=fm.prepare_latent_image_ids(hw, hw), txt_ids=torch.zeros(T, 3),
                guidance=torch.full((B,), 3.5), cond=torch.randn(B, N, 64, generator=g), cond_ids=cids)


@contextlib.contextmanager
def environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def forward_case(mod, W, I, mc=None, c_factor=None, cond=True, graph=True, attrs=None, env=None, lora_scale=None, mask=False, sched=False):
    """set_conditioning + two forwards on one fresh engine of `mod` -> [velocity, X, velocity, X, saturation count]"""
    I = {k: v.to(DEV) for k, v in I.items()}
    with environ(env or {}):
        eng = mod.DiTEngine(W, DEV)
        eng.use_graph = graph
        for k, v in (attrs or {}).items():
            setattr(eng, k, v)
        if lora_scale is not None:
            eng.set_lora_scale(lora_scale)
        B, T, N = I["enc"].shape[0], I["enc"].shape[1], I["latents"].shape[1]
        S = T + N + (N if cond else 0)
        m = None
        if mask:          # a bool mask that hides a band of keys from every query, broadcast over batch and heads
            m = torch.ones(S, S, dtype=torch.bool, device=DEV)
            m[:, 3:T // 2] = False
            m[T:T + 5, T + N // 2:T + N] = False
        eng.set_conditioning(I["enc"], I["pooled"], I["guidance"], I["txt_ids"], I["img_ids"], I["cond"] if cond else None,
                             I["cond_ids"] if cond else None, c_t=0.0, model_config=dict(mc or {}), c_factor=c_factor, attention_mask=m)
        ts = [0.8731, 0.25]
        if sched:
            eng.prepare_schedule(torch.tensor(ts))
        out = []
        for k in range(2):
            t = torch.full((B,), ts[k], device=DEV) if sched else I["timestep"]
            v = eng.forward(I["latents"], t, step_index=k if sched else None)
            out += [v.clone(), eng.X.clone()]
        out.append(eng.f16_overflow_count())
        eng.check_status()
    return out


def block_case(mod, W, kind, mc=None):
    """The block-level entry points on the goldens' block inputs: configure, load_streams, block_mods, double_block / single_block, then
    attention_module on the same streams as normalised activations."""
    G = {k: v.to(DEV) for k, v in load("flux_tiny.npz").items()}
    eng = mod.DiTEngine(W, DEV)
    B, T, N, C = 2, 16, 16, 16
    rope = lambda ids: ops.rope_table(ids.to(DEV, torch.float32).reshape(-1, 3), eng.cfg.axes_dims_rope)
    eng.configure(B, T, N, C, dict(mc or {}), None, rope(torch.cat([G["in_txt_ids"], G["in_img_ids"]], 0)), rope(G["in_cond_ids"]))
    hid = G["hid"] if kind == "double" else G["single_hid"][:, T:]
    enc = G["enc"] if kind == "double" else G["single_hid"][:, :T]
    cond = G["cond"] if kind == "double" else G["single_cond"]
    out = []
    eng.load_streams(enc, hid, cond)
    eng.block_mods(kind, 1, G["temb"], G["ctemb"])
    eng.double_block(1) if kind == "double" else eng.single_block(1)
    out += [eng.X.clone(), eng.read_stream("img", N), eng.read_stream("cond", C)]
    if not eng.precise:          # (attn_forward's engine path runs the 16-bit kernels only)
        eng.load_streams(enc, hid, cond, dst="XN")
        eng.attention_module(kind, 1, project_out=kind == "double")
        out += [eng.X.clone(), eng.Y.clone()]
    return out + [eng.f16_overflow_count()]


def outcome(fn, *a, raises=None, **kw):
    """fn's result; for a case that must be refused, the exception's text (exits if nothing was raised)."""
    if raises is None:
        return fn(*a, **kw)
    try:
        fn(*a, **kw)
    except raises as e:
        return [f"{type(e).__name__}: {e}"]
    sys.exit(f"{fn.__name__}{kw}: expected {raises.__name__}, nothing was raised")


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a, b))


@torch.no_grad()
def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    other = load_sibling(sys.argv[1])
    tr = tiny_transformer()
    sd = {k: v.detach().clone() for k, v in tr.state_dict().items()}
    W = pack_state_dict(sd, _cfg(tr), DEV)
    Wp = pack_state_dict(sd, _cfg(tr), DEV, precise=True)
    W16 = pack_state_dict(with_rank(sd, 16, seed=16), _cfg(tr), DEV)          # every adapter redrawn at rank 16 (tests/test_lora_wide_gpu.py)
    unfused = dict(qkv_epilogue=False, ln_lora=False)
    core = [("default", {}), ("no condition stream", dict(cond=False)), ("latent_lora", dict(mc={"latent_lora": True})),
            ("add_cond_attn", dict(mc={"add_cond_attn": True})), ("union_cond_attn False", dict(mc={"union_cond_attn": False})),
            ("independent_condition", dict(mc={"independent_condition": True})), ("c_factor 0.5", dict(c_factor=0.5)),
            ("operands fp16", dict(mc={"operands": "fp16"})), ("precise", dict(W=Wp, mc={"precise": True})),
            ("precise LX_PRECISE_ATTN=f32", dict(W=Wp, mc={"precise": True}, env={"LX_PRECISE_ATTN": "f32"})),
            ("precise latent_lora add_cond_attn", dict(W=Wp, mc={"precise": True, "latent_lora": True, "add_cond_attn": True})),
            ("attn_fp8", dict(mc={"attn_fp8": True})), ("gemm_fp8", dict(mc={"gemm_fp8": True})),
            ("gemm_fp8 latent_lora", dict(mc={"gemm_fp8": True, "latent_lora": True})),
            ("gemm_fp8 + attn_fp8", dict(mc={"gemm_fp8": True, "attn_fp8": True})),
            # the mode and path combinations that meet in the blocks written once for all operand modes: the per-layer condition cache
            # through the shared block's layer index, the masked-off condition stream on split operands, the refusal, a wide adapter
            ("precise independent_condition", dict(W=Wp, mc={"precise": True, "independent_condition": True})),
            ("attn_fp8 independent_condition", dict(mc={"attn_fp8": True, "independent_condition": True})),
            ("operands fp16 independent_condition", dict(mc={"operands": "fp16", "independent_condition": True})),
            ("precise union_cond_attn False", dict(W=Wp, mc={"precise": True, "union_cond_attn": False})),
            ("gemm_fp8 add_cond_attn (refused)", dict(mc={"gemm_fp8": True, "add_cond_attn": True}, raises=NotImplementedError)),
            ("rank-16 adapters add_cond_attn", dict(W=W16, mc={"add_cond_attn": True}))]
    cases = [(f"{name}, graph {'on' if g else 'off'}", dict(kw, graph=g)) for name, kw in core for g in (True, False)]
    cases += [("default, unfused", dict(attrs=unfused)), ("operands fp16, unfused", dict(mc={"operands": "fp16"}, attrs=unfused)),
              ("latent_lora, unfused", dict(mc={"latent_lora": True}, attrs=unfused)),
              ("pair_plan False", dict(attrs=dict(pair_plan=False))), ("pair_plan False, precise", dict(W=Wp, mc={"precise": True}, attrs=dict(pair_plan=False))),
              ("set_lora_scale(0.5)", dict(lora_scale=0.5)), ("set_lora_scale(0.5), precise", dict(W=Wp, mc={"precise": True}, lora_scale=0.5)),
              ("set_lora_scale(0.5), gemm_fp8", dict(mc={"gemm_fp8": True}, lora_scale=0.5)),
              ("bool attention_mask", dict(mask=True)), ("bool attention_mask, graph off", dict(mask=True, graph=False)),
              ("prepared schedule", dict(sched=True)), ("prepared schedule, latent_lora", dict(mc={"latent_lora": True}, sched=True)),
              ("rank-16 adapters", dict(W=W16)), ("rank-16 adapters, fp16 latent_lora", dict(W=W16, mc={"operands": "fp16", "latent_lora": True}))]
    n = 0
    for inputs_name, I in (("golden 16/16/16", golden_inputs()), ("seeded 32/64/64", fused_inputs())):
        for name, kw in cases:
            kw = dict(kw)
            Wc = kw.pop("W", W)
            ok = same(outcome(forward_case, engine_here, Wc, I, **kw), outcome(forward_case, other, Wc, I, **kw))
            print(f"{'equal' if ok else 'DIFFERENT':9s} {inputs_name}: {name}", flush=True)
            if not ok:
                sys.exit(1)
            n += 1
    for kind in ("double", "single"):
        for name, Wc, mc in (("bf16", W, {}), ("fp16 latent_lora", W, {"operands": "fp16", "latent_lora": True}),
                             ("add_cond_attn", W, {"add_cond_attn": True}), ("precise", Wp, {"precise": True}), ("attn_fp8", W, {"attn_fp8": True})):
            ok = same(block_case(engine_here, Wc, kind, mc), block_case(other, Wc, kind, mc))
            print(f"{'equal' if ok else 'DIFFERENT':9s} block-level entry points, {kind} block: {name}", flush=True)
            if not ok:
                sys.exit(1)
            n += 1
    print(f"all {n} cases bit-equal")


if __name__ == "__main__":
    main()
