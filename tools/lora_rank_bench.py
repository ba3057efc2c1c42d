"""What a LoRA rank costs: ms per denoise step at B = 1, 512 text + 1024 image + 1024 condition tokens, full width, bf16 operands, with
synthetic adapters of rank 4, 16 and 64 on every target (three engines over ONE set of base weights, alternating blocks of steps), and
the per-launch time of the down-projection (lx_lora_down) at M = 1024, K = 3072 and 15360 for the slab widths those ranks need.
    python tools/lora_rank_bench.py [--rounds 5] [--steps 20] [--ranks 4 16 64]
The comparison value is the rank-4 step of the same run. Prints one JSON line at the end."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loongx_amd import ops
from loongx_amd.flux.engine import DiTEngine
from loongx_amd.flux.weights import FluxConfig, Lora, PackedWeights, synthetic_weights

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--ranks", type=int, nargs="+", default=[4, 16, 64])
ap.add_argument("--tiny", action="store_true", help="2 + 2 blocks of width 256 (a rehearsal of the control flow)")
a = ap.parse_args()
dev = "cuda"
cfg = FluxConfig(num_layers=2, num_single_layers=2, num_attention_heads=2) if a.tiny else FluxConfig()
base = synthetic_weights(cfg, dev, lora=False)
D = cfg.inner_dim
g = torch.Generator(device=dev).manual_seed(1)


def rn(*shape, dtype=torch.bfloat16):
    return torch.empty(*shape, dtype=dtype, device=dev).normal_(0.0, 0.02, generator=g)


def with_adapters(r):
    """The base weights (shared tensors) with rank-r adapters on every target, the modulation Linears included."""
    pw = PackedWeights(dataclasses.replace(cfg, lora_r=r), dict(base.t))
    targets = [(f"d{i}.{n}", m) for i in range(cfg.num_layers) for n, m in (("qkv", 3), ("out", 1), ("ff2", 1))]
    targets += [(f"s{j}.{n}", m) for j in range(cfg.num_single_layers) for n, m in (("fused", 4), ("out", 1))] + [("x_embedder", 1)]
    for name, m in targets:
        W = base.t[name + ".w"]
        pw.lora[name] = Lora(rn(m * r, W.shape[1]), rn(W.shape[0], r, dtype=torch.float32))
    nb = cfg.num_layers + cfg.num_single_layers
    pw.t["mod.lora_down"] = rn(nb * r, D)
    for idx in range(nb):
        pw.t[f"mod.lora_up.{idx}"] = rn(6 * D if idx < cfg.num_layers else 3 * D, r, dtype=torch.float32)
    return pw


B, T, hw = 1, 512, 32
N = hw * hw
lat, cond = torch.randn(B, N, 64, device=dev, generator=g), torch.randn(B, N, 64, device=dev, generator=g)
pe, pooled = torch.randn(B, T, cfg.joint_attention_dim, device=dev, generator=g) * 0.1, torch.randn(B, cfg.pooled_projection_dim, device=dev, generator=g)
ids = torch.zeros(hw, hw, 3, device=dev)
ids[..., 1] = torch.arange(hw, device=dev)[:, None]
ids[..., 2] = torch.arange(hw, device=dev)[None, :]
img_ids = ids.reshape(-1, 3)
cond_ids = img_ids.clone()
cond_ids[:, 2] -= hw
ts = torch.full((B,), 0.5, device=dev)
engines = {}
for r in a.ranks:
    eng = DiTEngine(with_adapters(r), dev)
    eng.set_conditioning(pe, pooled, torch.full((B,), 3.5, device=dev), torch.zeros(T, 3, device=dev), img_ids, cond, cond_ids, model_config={})
    for _ in range(3):                      # eager pass, capture, first replay
        eng.forward(lat, ts)
    engines[r] = eng
torch.cuda.synchronize()
res = {r: [] for r in a.ranks}
for rd in range(a.rounds):
    for r in (a.ranks if rd % 2 == 0 else a.ranks[::-1]):
        eng = engines[r]
        for _ in range(2):
            eng.forward(lat, ts)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            eng.forward(lat, ts)
        torch.cuda.synchronize()
        res[r].append((time.perf_counter() - t0) / a.steps * 1e3)
line = {"shape": [B, T, N, N], "steps": a.steps, "rounds": a.rounds, "step_ms": {}, "down_us": {}}
r0 = a.ranks[0]
for r in a.ranks:
    med = statistics.median(res[r])
    line["step_ms"][str(r)] = {"median": round(med, 3), "min": round(min(res[r]), 3), "max": round(max(res[r]), 3),
                               "ratio_to_r%d" % r0: round(med / statistics.median(res[r0]), 4)}
    print(f"rank {r:2d}: median {med:.3f} ms/step, min {min(res[r]):.3f}, max {max(res[r]):.3f}  ({[round(x, 2) for x in res[r]]})")

# the down-projection alone: back-to-back launches between two events (throughput of the launch, the engine's four K-split slabs)
M = 1024
for K in (D, 5 * D):
    X = rn(M, K)
    for R in sorted({16} | {m * r for r in a.ranks for m in (1, 4) if m * r > 16}):
        A = rn(R, K)
        Tl = torch.zeros(4, M, R, dtype=torch.float32, device=dev)
        for _ in range(10):
            ops.lora_down(X, A, Tl[0], n_split=4, split_stride=Tl.stride(0))
        reps, best = 200, 1e30
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.lora_down(X, A, Tl[0], n_split=4, split_stride=Tl.stride(0))
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / reps * 1e3)
        line["down_us"][f"K{K}_R{R}"] = round(best, 2)
        print(f"lx_lora_down M={M} K={K} R={R} n_split=4: {best:.2f} us per launch ({'narrow' if R <= 16 else 'wide'} kernel)")
print(json.dumps(line))
