"""The calls LxAutoencoderKL makes into the library, by entry point, in each operand format (bf16, fp16, precise) on the two-level VAE:
decode of an 8x8 latent (P = 64 tokens, the unpadded attention launches) and of a 9x7 one (P = 63, padded key axis), encode of 64x64
(mid-block P = 1024) and of 72x56 (P = 36 * 28 = 1008, padded). Batch 1, seeded synthetic weights.

TABLE is recorded data: this file, run on the tree of the commit before the layers were written once against the operand policies
(three copies of every layer then), printed these counts. It uses the public surface only, so it runs there unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vae as ovae  # noqa: E402
from tests.test_vae_anysize_gpu import SMALL, rnd  # noqa: E402
from tests.test_vae_f16_gpu import _CountingLib  # noqa: E402

DEV = "cuda"
FORMATS = {"bf16": dict(), "fp16": dict(operands="fp16"), "precise": dict(precise=True)}
CALLS = {"decode 8x8": ("decode", (1, 16, 8, 8)), "decode 9x7": ("decode", (1, 16, 9, 7)),
         "encode 64x64": ("encode", (1, 3, 64, 64)), "encode 72x56": ("encode", (1, 3, 72, 56))}
PADDED = {"decode 8x8": False, "decode 9x7": True, "encode 64x64": False, "encode 72x56": True}

TABLE = {
    ("bf16", "decode 8x8"): {'lx_convert': 2, 'lx_gemm_bf16': 22, 'lx_groupnorm_silu': 14, 'lx_groupnorm_workspace_bytes': 14, 'lx_im2col3x3': 15, 'lx_softmax_rows': 1},
    ("bf16", "decode 9x7"): {'lx_convert': 2, 'lx_gemm_bf16': 22, 'lx_groupnorm_silu': 14, 'lx_groupnorm_workspace_bytes': 14, 'lx_im2col3x3': 15, 'lx_softmax_rows_valid': 1},
    ("bf16", "encode 64x64"): {'lx_convert': 2, 'lx_gemm_bf16': 18, 'lx_groupnorm_silu': 10, 'lx_groupnorm_workspace_bytes': 10, 'lx_im2col3x3': 11, 'lx_softmax_rows': 1},
    ("bf16", "encode 72x56"): {'lx_convert': 2, 'lx_gemm_bf16': 18, 'lx_groupnorm_silu': 10, 'lx_groupnorm_workspace_bytes': 10, 'lx_im2col3x3': 11, 'lx_softmax_rows_valid': 1},
    ("fp16", "decode 8x8"): {'lx_convert_f16': 3, 'lx_gemm_bf16': 22, 'lx_groupnorm_silu_f16': 14, 'lx_groupnorm_workspace_bytes': 14, 'lx_im2col3x3': 15, 'lx_softmax_rows_f16': 1},
    ("fp16", "decode 9x7"): {'lx_convert_f16': 3, 'lx_gemm_bf16': 22, 'lx_groupnorm_silu_f16': 14, 'lx_groupnorm_workspace_bytes': 14, 'lx_im2col3x3': 15, 'lx_softmax_rows_f16': 1},
    ("fp16", "encode 64x64"): {'lx_convert_f16': 3, 'lx_gemm_bf16': 18, 'lx_groupnorm_silu_f16': 10, 'lx_groupnorm_workspace_bytes': 10, 'lx_im2col3x3': 11, 'lx_softmax_rows_f16': 1},
    ("fp16", "encode 72x56"): {'lx_convert_f16': 3, 'lx_gemm_bf16': 18, 'lx_groupnorm_silu_f16': 10, 'lx_groupnorm_workspace_bytes': 10, 'lx_im2col3x3': 11, 'lx_softmax_rows_f16': 1},
    ("precise", "decode 8x8"): {'lx_gemm_bf16': 22, 'lx_groupnorm_silu_split': 14, 'lx_groupnorm_workspace_bytes': 14, 'lx_im2col3x3_split': 15, 'lx_softmax_rows_split': 1, 'lx_split_bf16': 3},
    ("precise", "decode 9x7"): {'lx_gemm_bf16': 22, 'lx_groupnorm_silu_split': 14, 'lx_groupnorm_workspace_bytes': 14, 'lx_im2col3x3_split': 15, 'lx_softmax_rows_split': 1, 'lx_split_bf16': 3},
    ("precise", "encode 64x64"): {'lx_gemm_bf16': 18, 'lx_groupnorm_silu_split': 10, 'lx_groupnorm_workspace_bytes': 10, 'lx_im2col3x3_split': 11, 'lx_softmax_rows_split': 1, 'lx_split_bf16': 3},
    ("precise", "encode 72x56"): {'lx_gemm_bf16': 18, 'lx_groupnorm_silu_split': 10, 'lx_groupnorm_workspace_bytes': 10, 'lx_im2col3x3_split': 11, 'lx_softmax_rows_split': 1, 'lx_split_bf16': 3},
}


@pytest.fixture(scope="module")
def counts():
    """{(format, call): {entry point: calls}}, every call made once."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops
    from loongx_amd.vae import LxAutoencoderKL
    sd = ovae.init_synthetic_(ovae.AutoencoderKL(**SMALL), 3).state_dict()
    out = {}
    for fmt, kw in FORMATS.items():
        lx = LxAutoencoderKL(sd, SMALL, DEV, **kw)
        for call, (what, shape) in CALLS.items():
            x = rnd(*shape, seed=3).to(DEV)
            real = ops.lib
            ops.lib = lib = _CountingLib(real)
            try:
                getattr(lx, what)(x)
            finally:
                ops.lib = real
            out[fmt, call] = dict(sorted(lib.calls.items()))
            print(f'    ("{fmt}", "{call}"): {out[fmt, call]},')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_calls_into_the_library_are_the_recorded_ones(counts, fmt, call):
    assert counts[fmt, call] == TABLE[fmt, call]


def test_precise_makes_none_of_the_16_bit_producers_calls(counts):
    never = {"lx_groupnorm_silu", "lx_groupnorm_silu_f16", "lx_softmax_rows", "lx_softmax_rows_valid", "lx_softmax_rows_f16", "lx_im2col3x3"}
    for call in CALLS:
        assert not never & counts["precise", call].keys(), (call, counts["precise", call])


def test_bf16_softmax_entry_point_follows_the_padding(counts):
    """lx_softmax_rows at P = 64 / 1024, lx_softmax_rows_valid at P = 63 / 1008: once per call (batch 1), never the other one."""
    for call, padded in PADDED.items():
        c = counts["bf16", call]
        assert c.get("lx_softmax_rows", 0) == (0 if padded else 1) and c.get("lx_softmax_rows_valid", 0) == (1 if padded else 0), (call, c)
