#!/usr/bin/env python3
"""A/B of two builds of loongx_amd/csrc/vae.hip, launch by launch: the acceptance check of a refactor of that file.

    LX_AMD_LIB=/path/to/parent/liblx_amd.so python tools/vae_kernels_ab.py run > parent_1.txt     # the processes alternate:
    python tools/vae_kernels_ab.py run > here_1.txt                                                # parent, here, parent, here
    ...
    python tools/vae_kernels_ab.py compare --parent parent_1.txt parent_2.txt --here here_1.txt here_2.txt

run: against the library LX_AMD_LIB names (default: this tree's), one line per case: the sha256 of the output image's bytes and the times
of 9 launches after one warm-up, HIP events around each launch. The cases of every entry point of vae.hip: the shapes of
tests/test_vae_kernels_shared_gpu.py, and every distinct launch of a decode of a 64x64 latent and an encode of a 512x512 image at the
full FLUX.1 VAE shape, batch 1, on bf16, fp16 and precise operands -- taken from a trace of the calls into the library (vae_ab.TracingLib)
and replayed on seeded inputs of the traced sizes. Then the whole decode and encode per format, digest and times alike.

compare: exits non-zero unless (a) every digest is the same in all files and (b) for every row this tree's median is at most the parent's
median plus the parent's own (max - min), both over the counted launches of all of an arm's runs (tools/kernels_ab.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels_ab  # noqa: E402
from kernels_ab import counted, row  # noqa: E402

NAN16 = 0x7FC0
VAE_ENTRIES = ("lx_groupnorm_silu", "lx_groupnorm_silu_f16", "lx_groupnorm_silu_split", "lx_im2col3x3", "lx_im2col3x3_split", "lx_softmax_rows",
               "lx_softmax_rows_valid", "lx_softmax_rows_f16", "lx_softmax_rows_split", "lx_convert_f16")
FORMATS = [("bf16", dict()), ("fp16", dict(operands="fp16")), ("precise", dict(precise=True))]
P_ = True                  # a pointer argument in a case, as the trace shows it: only whether it is there


def test_shape_cases():
    """(entry point, arguments as TracingLib logs them, offset): the launches of tests/test_vae_kernels_shared_gpu.py. offset 1: S and P
    start one element off a 16-byte boundary (the scalar kernels)."""
    out = []
    for off in (0, 1):
        for nv in (1, 3, 63, 64, 65, 259):
            ns = (nv + 63) // 64 * 64
            out.append(("lx_softmax_rows_valid", (P_, ns, 0.25, P_, ns + 8, 5, nv, ns, P_), off))
            out.append(("lx_softmax_rows_f16", (P_, ns, 0.25, P_, ns + 8, 5, nv, ns, P_), off))
            out.append(("lx_softmax_rows_split", (P_, ns, 0.25, P_, 2 * ns + 16, ns + 8, 5, nv, ns, P_), off))
    out.append(("lx_softmax_rows", (P_, 260, 0.25, P_, 260, 5, 260, P_), 0))
    out.append(("lx_softmax_rows_valid", (P_, 260, 0.25, P_, 260, 5, 260, 260, P_), 0))
    for Cc in (3, 8, 24):
        lo, Kpad = (Cc + 7) // 8 * 8 + 8, (9 * Cc + 63) // 64 * 64
        for mode in (0, 1, 2):
            out.append(("lx_im2col3x3", (P_, 2, 4, 6, Cc, mode, P_, Kpad, P_), 0))
            out.append(("lx_im2col3x3_split", (P_, 2 * lo, lo, 2, 4, 6, Cc, mode, P_, Kpad, P_), 0))
    for Cc, P in ((128, 5), (128, 257), (512, 4097)):
        nb = 2 * (64 if P >= 4096 else 16 if P >= 256 else 1) * 32 * 8
        for xb in (0, 1):
            out.append(("lx_groupnorm_silu", (P_, xb, 2, P, Cc, 32, P_, P_, 1e-6, 1, P_, P_, nb, P_), 0))
        out.append(("lx_groupnorm_silu_f16", (P_, 2, P, Cc, 32, P_, P_, 1e-6, 1, P_, P_, nb, P_, P_), 0))
        out.append(("lx_groupnorm_silu_split", (P_, 2, P, Cc, 32, P_, P_, 1e-6, 1, P_, 2 * Cc + 16, Cc + 8, P_, nb, P_), 0))
    out.append(("lx_convert_f16", (P_, P_, 0, 100003, P_, P_), 0))
    out.append(("lx_convert_f16", (P_, P_, 1, 100003, P_, P_), 0))
    return out


def run():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tools")]
    import torch
    from loongx_amd import _lib, ops
    from loongx_amd.vae import LxAutoencoderKL
    from vae_ab import rnd, state_dict, traced
    dev, lib = "cuda", ops.lib
    gen = torch.Generator(device=dev)

    def randn(*shape, dtype=torch.float32, off=0, seed=0, scale=1.0, shift=0.0):
        """seeded scale * N(0, 1) + shift whose first element lies `off` elements behind an aligned address"""
        gen.manual_seed(seed)
        n = 1
        for s in shape:
            n *= s
        return (torch.randn(n + off, device=dev, generator=gen) * scale + shift).to(dtype)[off:].view(*shape)

    def image16(rows, ld, off=0):
        """16-bit output image, prefilled: what a launch leaves alone is part of the digest"""
        return torch.full((rows * ld + off,), NAN16, dtype=torch.int16, device=dev)[off:].view(rows, ld)

    def launch(name, a, off):
        """-> (call, output, operands to keep alive): the launch of entry point `name` with the scalar arguments of `a` on seeded operands of
        the sizes they imply"""
        ptr = lambda t: t.data_ptr()
        counter = lambda there: torch.zeros(1, dtype=torch.int32, device=dev) if there else None
        if name.startswith("lx_groupnorm_silu"):
            ovf = None
            if name == "lx_groupnorm_silu":
                _, xb, B, P, Cc, G, _, _, eps, silu, _, _, nb, _ = a
            elif name == "lx_groupnorm_silu_f16":
                _, B, P, Cc, G, _, _, eps, silu, _, _, nb, has_ovf, _ = a
            else:
                _, B, P, Cc, G, _, _, eps, silu, _, ldy, lo, _, nb, _ = a
            x = randn(B, P, Cc, dtype=torch.bfloat16 if name == "lx_groupnorm_silu" and xb else torch.float32, seed=1, scale=2.0, shift=0.5)
            g, b = randn(Cc, seed=2, scale=0.2, shift=1.0), randn(Cc, seed=3, scale=0.2)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            y = image16(B * P, ldy if name.endswith("_split") else Cc)
            head = (B, P, Cc, G, ptr(g), ptr(b), eps, silu, ptr(y))
            if name == "lx_groupnorm_silu":
                args = (ptr(x), xb) + head + (ptr(ws), nb)
            elif name == "lx_groupnorm_silu_f16":
                ovf = counter(has_ovf)
                args = (ptr(x),) + head + (ptr(ws), nb, ops._p(ovf))
            else:
                args = (ptr(x),) + head + (ldy, lo, ptr(ws), nb)
            keep = (x, g, b, ws, ovf)
        elif name.startswith("lx_im2col3x3"):
            if name == "lx_im2col3x3":
                _, B, H, W, Cc, mode, _, Kpad, _ = a
                ldx, nh, lead = Cc, 1, ()
            else:
                _, ldx, lo, B, H, W, Cc, mode, _, Kpad, _ = a
                nh, lead = 2, (ldx, lo)
            x = randn(B, H, W, ldx, dtype=torch.bfloat16, seed=4)
            Ho, Wo = {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[mode]
            y = image16(B * Ho * Wo, nh * Kpad)
            args, keep = (ptr(x),) + lead + (B, H, W, Cc, mode, ptr(y), Kpad), (x,)
        elif name.startswith("lx_softmax_rows"):
            if name == "lx_softmax_rows":
                _, lds, scale, _, ldp, M, N, _ = a
                tail = (M, N)
            elif name == "lx_softmax_rows_split":
                _, lds, scale, _, ldp, lo, M, nv, ns, _ = a
                tail = (lo, M, nv, ns)
            else:
                _, lds, scale, _, ldp, M, nv, ns, _ = a
                tail = (M, nv, ns)
            S = randn(M, lds, off=off, seed=5, scale=3.0)
            y = image16(M, ldp, off)
            args, keep = (ptr(S), lds, scale, ptr(y), ldp) + tail, (S,)
        elif name == "lx_convert_f16":
            _, _, sb, n, has_ovf, _ = a
            src, y, ovf = randn(n, dtype=torch.bfloat16 if sb else torch.float32, seed=6, scale=3e4), image16(1, n), counter(has_ovf)
            args, keep = (ptr(y), ptr(src), sb, n, ops._p(ovf)), (src, ovf)
        else:
            raise KeyError(name)
        fn = getattr(lib, name)
        return (lambda: ops.check(fn(*args, ops._stream()), name)), y, keep

    print(f"# tools/vae_kernels_ab.py run on {torch.cuda.get_device_name(0)}, library {_lib.LIB_PATH}")
    cases, seen, whole = [], set(), []
    with torch.no_grad():
        for fmt, kw in FORMATS:
            m = LxAutoencoderKL(state_dict({}, False), {}, dev, **kw)
            z, img = rnd(1, 16, 64, 64, seed=3), rnd(1, 3, 512, 512, seed=1).clamp(-1, 1)
            for what, fn in ((f"decode 64x64 latent, {fmt}", lambda: m.decode(z).sample), (f"encode 512x512, {fmt}", lambda: m.encode(img).latent_dist.mean)):
                _, log = traced(fn)
                cases += [(c[0], c[1:], 0) for c in log if c[0] in VAE_ENTRIES]
                whole.append((what,) + counted(fn))
            del m
        for name, a, off in test_shape_cases() + cases:
            key = f"{name}{a}" + (" +1 element" if off else "")
            if key in seen:
                continue
            seen.add(key)
            call, y, keep = launch(name, a, off)
            _, ms = counted(call)
            row(key, y, ms)
            del call, y, keep
        for what, out, ms in whole:
            row(what, out, ms)


if __name__ == "__main__":
    kernels_ab.main(run, __doc__)
