#!/usr/bin/env python3
"""A/B of two versions of loongx_amd/vae.py: the acceptance check of a refactor of that file.

    git show <commit>:loongx_amd/vae.py > /tmp/vae_other.py
    python tools/vae_ab.py /tmp/vae_other.py

The other file is loaded as a sibling module inside the loongx_amd package, so its relative imports bind to the same ops and the same
library: one process, one LxAutoencoderKL of each module per arm, built on the same state dict (oracle/vae.py synthetic weights).
Arms: bf16, fp16 and precise on fp32 weights (precise: k_segs = 3) and precise on the weights rounded to bf16 (k_segs = 2).

(a) Bit equality on the two-level VAE of the tests and on the full FLUX.1 shape: decode of 8x8 and 9x7 latents, encode of 64x64 and 72x56
    images, batch 1 and 2, the full shape also at a 64x64 latent / 512x512 image; and the fp16 overflow fallback on a clipping GroupNorm gain
    (outputs and warning texts). Every output torch.equal.
(b) Call trace, on the two-level VAE: every call into ops.lib with its scalar arguments and, of a descriptor structure, every field that
    is not a pointer (of a pointer only whether it is NULL: the allocator decides the rest). The two traces must be equal element for
    element: shapes, strides, lo offsets, k_segs and epilogue flags.
(c) Time, full shape, batch 1: decode 64x64 / encode 512x512 and the launch-bound decode 8x8 / encode 64x64 in each format, the two modules
    alternating in this process, HIP events around each call, one warm-up and ROUNDS counted rounds per arm. A row is within its bound when
    this tree's median is at most the other's median plus the other's own (max - min) over the same rounds.

Exits non-zero on the first difference of (a) / (b), and after the table when a row of (c) misses."""
import ctypes as C
import importlib.util
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from loongx_amd import ops
from loongx_amd import vae as vae_here
from oracle import vae as ovae

DEV = "cuda"
ROUNDS = 9
SMALL = dict(in_channels=3, out_channels=3, latent_channels=16, block_out_channels=(128, 256), layers_per_block=1, norm_num_groups=32)
ARMS = [("bf16", dict(), False), ("fp16", dict(operands="fp16"), False), ("precise", dict(precise=True), False),
        ("precise, bf16 weights", dict(precise=True), True)]


def load_sibling(path):
    spec = importlib.util.spec_from_file_location("loongx_amd._vae_other", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _field(v, t):
    if t is C.c_void_p:
        return v is not None and v != 0
    if isinstance(t, type) and issubclass(t, C.Array):
        return tuple(bool(e) if t._type_ is C.c_void_p else e for e in v)
    return v


def _arg(v, t):
    if t is C.c_void_p:
        return v is not None and v != 0
    if isinstance(t, type) and issubclass(t, C._Pointer):
        if not issubclass(t._type_, C.Structure):
            return v is not None
        objs = list(v) if isinstance(v, C.Array) else [v._obj]
        return tuple(tuple((n, _field(getattr(o, n), ft)) for n, ft in o._fields_) for o in objs)
    return v


class TracingLib:
    """loongx_amd.ops.lib with every call logged: (entry point, argument, ...) as _arg describes them."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        types = fn.argtypes or ()

        def call(*a):
            self.log.append((name,) + tuple(_arg(v, t) for v, t in zip(a, types)))
            return fn(*a)
        return call


def traced(fn):
    real = ops.lib
    ops.lib = lib = TracingLib(real)
    try:
        out = fn()
    finally:
        ops.lib = real
    return out, lib.log


def state_dict(cfg, rounded):
    sd = ovae.init_synthetic_(ovae.AutoencoderKL(**cfg), 3).state_dict()
    return {k: (v.to(torch.bfloat16).to(v.dtype) if rounded else v.clone()) for k, v in sd.items()}


def calls(full):
    out = []
    for B in (1, 2):
        for h, w in [(8, 8), (9, 7)] + ([(64, 64)] if full else []):
            out.append((f"decode {h}x{w} latent, batch {B}", lambda m, B=B, h=h, w=w: m.decode(rnd(B, 16, h, w, seed=3)).sample))
        for H, W in [(64, 64), (72, 56)] + ([(512, 512)] if full else []):
            out.append((f"encode {H}x{W}, batch {B}", lambda m, B=B, H=H, W=W: m.encode(rnd(B, 3, H, W, seed=1).clamp(-1, 1)).latent_dist.mean))
    return out


def fail(what):
    print(f"DIFFERENT {what}", flush=True)
    sys.exit(1)


def equality_and_trace(other):
    n = 0
    for shape, cfg, full in (("two-level", SMALL, False), ("full", {}, True)):
        for arm, kw, rounded in ARMS:
            sd = state_dict(cfg, rounded)
            a, b = vae_here.LxAutoencoderKL(sd, cfg, DEV, **kw), other.LxAutoencoderKL(sd, cfg, DEV, **kw)
            for name, run in calls(full):
                (ya, ta), (yb, tb) = traced(lambda: run(a)), traced(lambda: run(b))
                torch.cuda.synchronize()
                if not torch.equal(ya, yb):
                    fail(f"output: {shape}, {arm}: {name}")
                if not full:
                    if len(ta) != len(tb):
                        fail(f"trace: {shape}, {arm}: {name}: {len(ta)} calls here, {len(tb)} there")
                    for i, (ca, cb) in enumerate(zip(ta, tb)):
                        if ca != cb:
                            fail(f"trace: {shape}, {arm}: {name}: call {i}\n  here  {ca}\n  there {cb}")
                print(f"equal     {shape}, {arm}: {name}" + ("" if full else f"; trace equal, {len(ta)} calls"), flush=True)
                n += 1
            del a, b
    # the fp16 overflow fallback: decoder.conv_norm_out's gain 1e6 times too large saturates its fp16 image
    sd = state_dict(SMALL, False)
    sd["decoder.conv_norm_out.weight"] *= 1e6
    got = []
    for mod in (vae_here, other):
        lx = mod.LxAutoencoderKL(sd, SMALL, DEV, operands="fp16", f16_overflow="fallback")
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            (y, t) = traced(lambda: lx.decode(rnd(2, 16, 4, 4, seed=3)).sample)
        got.append((y, [str(w.message) for w in rec], t, lx.operands))
    (ya, wa, ta, oa), (yb, wb, tb, ob) = got
    if not (torch.equal(ya, yb) and wa == wb and len(wa) == 1 and "with bf16 operands" in wa[0] and ta == tb and oa == ob == "fp16"):
        fail(f"fp16 overflow fallback: warnings {wa} / {wb}")
    print(f"equal     two-level, fp16 overflow fallback: output, warning text, trace ({len(ta)} calls)")
    print(f"all {n + 1} cases bit-equal, every trace equal", flush=True)


def timed(fn):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def timing(other):
    print(f"\ntime in ms, full shape, batch 1, {ROUNDS} rounds after one warm-up, the two modules alternating: median (min .. max)")
    missed = 0
    for arm, kw, rounded in ARMS[:3]:
        sd = state_dict({}, rounded)
        here, there = vae_here.LxAutoencoderKL(sd, {}, DEV, **kw), other.LxAutoencoderKL(sd, {}, DEV, **kw)
        rows = [("decode 64x64 latent", "decode", rnd(1, 16, 64, 64, seed=3)), ("encode 512x512", "encode", rnd(1, 3, 512, 512, seed=1).clamp(-1, 1)),
                ("decode 8x8 latent", "decode", rnd(1, 16, 8, 8, seed=3)), ("encode 64x64", "encode", rnd(1, 3, 64, 64, seed=1).clamp(-1, 1))]
        for name, what, x in rows:
            t = {id(here): [], id(there): []}
            for r in range(ROUNDS + 1):
                for m in ((here, there) if r % 2 else (there, here)):
                    ms = timed(lambda: getattr(m, what)(x))
                    if r:
                        t[id(m)].append(ms)
            th, to = t[id(here)], t[id(there)]
            bound = statistics.median(to) + (max(to) - min(to))
            ok = statistics.median(th) <= bound
            missed += not ok
            print(f"{'within' if ok else 'MISSED':7s} {arm:8s} {name:20s} here {statistics.median(th):8.3f} ({min(th):8.3f} .. {max(th):8.3f})   "
                  f"other {statistics.median(to):8.3f} ({min(to):8.3f} .. {max(to):8.3f})   bound {bound:8.3f}", flush=True)
        del here, there
    return missed


@torch.no_grad()
def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    other = load_sibling(sys.argv[1])
    equality_and_trace(other)
    missed = timing(other)
    if missed:
        sys.exit(f"{missed} timing row(s) beyond their bound")
    print("every timing row within its bound")


if __name__ == "__main__":
    main()
