"""Masked joint attention (lx_attn_fwd_masked, csrc/attn_mask.hip) against the unmasked max-tracking kernel, B = 1, H = 24, at
S = 2560 (512 / 1024 / 1024) and S = 8704 (512 / 4096 / 4096). Not part of bench.py.

  python tools/attn_mask_bench.py [--iters 30] [--out profiles/attn_mask_bench.txt]

Per case: microseconds per attention launch (mean of --iters launches between events, after warm-up), the mask prep pass on its own,
and the fraction of (query tile, key tile) pairs that are not EMPTY (read back from the prep pass's work lists)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from loongx_amd import ops  # noqa: E402

DEV = "cuda"
B, H = 1, 24


def _time(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def _tile_mask(lens, frac_empty, seed):
    """[S, S] bool, each (segment-local 256-row query tile, 64-key tile) either all False (probability frac_empty) or all True"""
    g = torch.Generator().manual_seed(seed)
    S = sum(lens)
    edges = [0]
    for L in lens:
        edges.append(edges[-1] + L)
    m = torch.zeros(S, S, dtype=torch.bool)
    for sq, Lq in enumerate(lens):
        for q0 in range(0, Lq, 256):
            for sk, Lk in enumerate(lens):
                for k0 in range(0, Lk, 64):
                    if float(torch.rand(1, generator=g)) >= frac_empty:
                        m[edges[sq] + q0: edges[sq] + min(Lq, q0 + 256), edges[sk] + k0: edges[sk] + min(Lk, k0 + 64)] = True
    return m


def run(lens, iters):
    D = H * 128
    S = sum(lens)
    row0 = [sum(B * L for L in lens[:i]) for i in range(len(lens))]
    vt0 = [sum((L + 63) // 64 * 64 for L in lens[:i]) for i in range(len(lens))]
    vt_len = sum((L + 63) // 64 * 64 for L in lens)
    g = torch.Generator().manual_seed(0)
    buf = torch.randn(B * S, 3 * D, generator=g).to(torch.bfloat16).to(DEV)
    VT = torch.zeros(B, H, 128, vt_len, dtype=torch.bfloat16, device=DEV)
    one = torch.ones(128, device=DEV)
    ops.qkv_prep_segs(buf, 2 * D, 0, D, [(row0[i], L, vt0[i], one, one, None, None) for i, L in enumerate(lens)], B, H, VT)
    O = torch.zeros(B * S, D, dtype=torch.bfloat16, device=DEV)
    kw = dict(q_col=2 * D, k_col=0, o_col=0, B=B, H=H, seg_row0=row0, seg_len=list(lens), seg_vt0=vt0)
    flops = 4.0 * B * H * S * S * 128
    rows = []
    us = _time(lambda: ops.attn_fwd(buf, buf, VT, O, flags=ops.ATTN_INVARIANT, **kw), iters)
    rows.append(dict(case="unmasked lx_attn_fwd (max-tracking)", us=us, prep_us=0.0, nonempty=1.0, tflops=flops / us / 1e6))
    pad = torch.ones(1, 1, 1, S, dtype=torch.bool)
    pad[..., S - S // 4:] = False                                        # the last 25 % of the keys masked
    cases = [
        ("all-FULL bool", torch.ones(S, S, dtype=torch.bool)),
        ("dense random bool (all PARTIAL)", torch.rand(S, S, generator=g) < 0.5),
        ("dense fp32 additive", torch.randn(S, S, generator=g)),
        ("key padding, 25 % of keys masked", pad),
        ("block-sparse, 50 % of tiles EMPTY", _tile_mask(lens, 0.5, 1)),
        ("block-sparse, 75 % of tiles EMPTY", _tile_mask(lens, 0.75, 2)),
    ]
    for name, m in cases:
        m = m.to(DEV)
        ws = ops.attn_mask_workspace(m, B=B, H=H, seg_len=list(lens), seg_vt0=vt0)
        prep_us = _time(lambda: ops.attn_mask_prep(m, ws, B=B, H=H, seg_len=list(lens), seg_vt0=vt0), max(3, iters // 3))
        us = _time(lambda: ops.attn_fwd_masked(buf, buf, VT, O, m, workspace=ws, prepped=True, **kw), iters)
        n_qt = sum((L + 255) // 256 for L in lens)
        n_kt = sum((L + 63) // 64 for L in lens)
        lst = ws[: n_qt * (n_kt + 1) * 4].view(torch.int32).view(n_qt, n_kt + 1).cpu()
        rows.append(dict(case=name, us=us, prep_us=prep_us, nonempty=float(lst[:, 0].sum()) / (n_qt * n_kt), tflops=flops / us / 1e6))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"# tools/attn_mask_bench.py on {torch.cuda.get_device_name(0)}: B = {B}, H = {H}; us per launch (mean of {a.iters}); "
             "TF/s counts the dense S x S work whatever the mask skips"]
    for lens in ((512, 1024, 1024), (512, 4096, 4096)):
        S = sum(lens)
        rows = run(lens, a.iters)
        base = rows[0]["us"]
        lines.append(f"\nS = {S} ({' / '.join(map(str, lens))})")
        lines.append(f"{'case':38s} {'attn us':>9s} {'x unmasked':>10s} {'non-EMPTY':>9s} {'prep us':>8s} {'TF/s':>6s}")
        for r in rows:
            lines.append(f"{r['case']:38s} {r['us']:9.1f} {r['us'] / base:10.2f} {r['nonempty']:9.3f} {r['prep_us']:8.1f} {r['tflops']:6.0f}")
            print(json.dumps(dict(S=S, **r)), flush=True)
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(txt)


if __name__ == "__main__":
    main()
