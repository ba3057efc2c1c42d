#!/usr/bin/env python3
"""A/B of two builds of the scheduler-step entry points (loongx_amd/csrc/step.hip), launch by launch: the acceptance check of a refactor
of that file.

    LX_AMD_LIB=/path/to/parent/liblx_amd.so python tools/step_kernels_ab.py run > parent_1.txt     # the processes alternate:
    python tools/step_kernels_ab.py run > here_1.txt                                                # parent, here, parent, here
    ...
    python tools/step_kernels_ab.py compare --parent parent_1.txt parent_2.txt --here here_1.txt here_2.txt

run: against the library LX_AMD_LIB names (default: this tree's), one line per case: a sha256 and the times of 9 calls after one warm-up, HIP
events around each call (tools/kernels_ab.py). The cases: lx_euler_step, lx_euler_step_blend, lx_euler_step_cfg, lx_euler_step_cfg3 and
lx_euler_step_apg on two and on three parts, each with v in bf16 and in fp32, with and without the blend where the entry has the choice,
every base 0 and 1 elements behind an aligned address, and parts of 1027 elements, of one 512x512 image (1 x 1024 x 64) and of four
1024x1024 images (4 x 4096 x 64; for APG four images of 262144 elements); lx_scale_noise at the same sizes. The calls run in place, one after
the other on the same x. An APG call is two consecutive steps with momentum 0.5, so that M is read as well as written. The digest is over
x with the sentinel margins around it; for APG over M (with its margins) and the sums as well.

compare: see tools/kernels_ab.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernels_ab  # noqa: E402
from kernels_ab import counted, row  # noqa: E402

SENT, MARGIN = 0x7FC0BEEF, 64
SIZES = ((1, 1027), (1, 1 * 1024 * 64), (4, 4096 * 64))          # (images, elements of one image): a part holds images * elements
DS, SIGMA, SIGMA_NEXT = -0.137, 0.7551, 0.6183
# (name, parts, scales, the blend options of the entry)
ENTRIES = (("lx_euler_step", 1, (), (False,)), ("lx_euler_step_blend", 1, (), (True,)), ("lx_euler_step_cfg", 2, (3.5,), (False, True)),
           ("lx_euler_step_cfg3", 3, (2.0, 3.5), (False, True)), ("lx_euler_step_apg", 2, (3.5,), (False, True)),
           ("lx_euler_step_apg", 3, (2.0, 3.5), (False, True)))


def run():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    from loongx_amd import _lib, ops
    dev = "cuda"
    gen = torch.Generator(device=dev)

    def placed(n, off, seed, dtype=torch.float32):
        """seeded N(0, 1) values `off` elements behind an aligned address, sentinel margins on both sides: (buffer, the view of the values)"""
        gen.manual_seed(seed)
        lead = 64 + off                                        # (64 elements: 128 or 256 bytes, the view stays `off` elements off 16 bytes)
        buf = torch.empty(lead + n + MARGIN, dtype=dtype, device=dev)
        buf.view(torch.int32 if dtype == torch.float32 else torch.int16).fill_(SENT if dtype == torch.float32 else 0x7FC1)
        view = buf[lead:lead + n]
        view.copy_(torch.randn(n, device=dev, generator=gen).to(dtype))
        return buf, view

    print(f"# tools/step_kernels_ab.py run on {torch.cuda.get_device_name(0)}, library {_lib.LIB_PATH}")
    for images, elems in SIZES:
        n = images * elems
        for off in (0, 1):
            where = f"n={images}x{elems} base+{off}"
            out_buf, out = placed(n, off, 1)
            (_, x0), (_, z), (_, m) = placed(n, off, 2), placed(n, off, 3), placed(n, off, 4)
            m.copy_(torch.tensor([0.0, 0.25, 1.0], device=dev)[torch.randint(0, 3, (n,), generator=gen, device=dev)])
            _, ms = counted(lambda: ops.scale_noise(x0, z, SIGMA, out))
            row(f"lx_scale_noise {where}", out_buf, ms)
            for name, parts, scales, blends in ENTRIES:
                for vdt in (torch.bfloat16, torch.float32):
                    for blend in blends:
                        x_buf, x = placed(parts * n, off, 5)
                        _, v = placed(parts * n, off, 6, vdt)
                        bl = (x0, z, m) if blend else None
                        digest = [x_buf]
                        if name == "lx_euler_step":
                            call = lambda: ops.euler_step(x, v, DS)                                        # noqa: E731
                        elif name == "lx_euler_step_blend":
                            call = lambda: ops.euler_step_blend(x, v, DS, x0, z, m, SIGMA_NEXT)            # noqa: E731
                        elif name == "lx_euler_step_cfg":
                            call = lambda: ops.euler_step_cfg(x, v, DS, scales[0], bl, SIGMA_NEXT)         # noqa: E731
                        elif name == "lx_euler_step_cfg3":
                            call = lambda: ops.euler_step_cfg3(x, v, DS, scales[0], scales[1], bl, SIGMA_NEXT)   # noqa: E731
                        else:
                            M_buf, M = placed(n, off, 7)
                            sums = torch.zeros(2, images, 3, dtype=torch.float64, device=dev)
                            ws = torch.empty(ops.apg_workspace_bytes(images, elems), dtype=torch.uint8, device=dev)
                            digest += [M_buf, sums]

                            def call():
                                for step in range(2):
                                    ops.euler_step_apg(x, v, SIGMA, DS, scales, 0.25, 1.5, 0.5, M, sums[step], ws, bl, SIGMA_NEXT)
                        _, ms = counted(call)
                        row(f"{name} parts={parts} v={str(vdt).split('.')[-1]} blend={int(blend)} {where}", digest, ms)


if __name__ == "__main__":
    kernels_ab.main(run, __doc__)
