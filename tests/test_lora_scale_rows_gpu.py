"""lx_lora_scale_rows (ops.lora_scale_rows): T_s[row, c] *= W[b, c % period] on the adapter scratch, b = ((row - row0) // rows_per_batch) %
n_batches. One IEEE fp32 multiply per element, so the result is torch's `T * W` bit for bit; rows outside the segments, columns >= R, the
row padding and the gaps between the slabs keep their bits (sentinel footprint of tests/test_rowops_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_rowops_gpu import check_footprint, randn, sentinel  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from loongx_amd import ops as o
    return o


def run_case(ops, rows, R, ldt, n_slab, period, segs, n_batches, base=16, stride_pad=8):
    """`rows` rows of R columns (row stride ldt) per slab, random data in every one of them and sentinels everywhere else; scale the
    segments' rows and compare with torch."""
    what = f"lora_scale_rows rows={rows} R={R} ldt={ldt} n_slab={n_slab} period={period} segs={segs} n_batches={n_batches} base={base}"
    stride = (rows - 1) * ldt + R + stride_pad               # sentinel elements between the slabs
    buf = sentinel((base + n_slab * stride + 32,), torch.float32)
    data = randn(n_slab, rows, R, seed=R + rows)
    for s in range(n_slab):
        buf[base + s * stride:].as_strided((rows, R), (ldt, 1)).copy_(data[s])
    init = buf.clone()
    w_ld = period + 3
    Wfull = randn(n_batches, w_ld, seed=3)
    W = Wfull[:, :period]
    T = buf[base:].as_strided((rows, R), (ldt, 1))
    ops.lora_scale_rows(T, segs, W, period, n_slab=n_slab, slab_stride=stride if n_slab > 1 else 0)
    torch.cuda.synchronize()
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    cols = torch.arange(R, device=DEV) % period
    for s in range(n_slab):
        got = buf[base + s * stride:].as_strided((rows, R), (ldt, 1))
        mask = inside[base + s * stride:].as_strided((rows, R), (ldt, 1))
        for row0, n_rows, rpb in segs:
            b = (torch.arange(n_rows, device=DEV) // rpb) % n_batches
            want = data[s, row0:row0 + n_rows] * W[b][:, cols]
            assert torch.equal(got[row0:row0 + n_rows], want), f"{what}: slab {s}, segment at row {row0}"
            mask[row0:row0 + n_rows] = True
    check_footprint(what, buf, inside, init=init)


@pytest.mark.parametrize("R", [1, 6, 16, 18, 64, 256, 3648])
def test_one_segment_batches_wrap(ops, R):
    """rows_per_batch = 1 and three table rows (the modulation scratch of a whole schedule: row = step * B + sample), at every row count,
    row stride and slab count. R = 18 with ldt = 22 and the slab strides that are no multiple of 4 take the element path; M = 513,
    R = 3648 is more work than the capped grid holds, so the grid-stride loop runs more than once."""
    for M in (1, 70, 513):
        for ldt in (R, R + 4):
            for n_slab in (1, 3, 4):
                run_case(ops, M, R, ldt, n_slab, R, [(0, M, 1)], 3)
                if ldt % 4 == 0 and n_slab == 3:
                    run_case(ops, M, R, ldt, n_slab, R, [(0, M, 1)], 3, stride_pad=8 + (-((M - 1) * ldt + R)) % 4)      # slab_stride % 4 == 0: 16-byte accesses


@pytest.mark.parametrize("R,ldt", [(1, 4), (6, 8), (9, 16), (18, 24), (3, 64)])
def test_partial_last_chunk_of_an_aligned_row(ops, R, ldt):
    """The engine's scratch: a row stride that is a multiple of 4 under an R that is not (three modules of rank 3 in 16-column slabs):
    16-byte accesses up to the last whole chunk, elements after it, nothing past column R."""
    for M in (1, 70, 513):
        for n_slab in (1, 4):
            run_case(ops, M, R, ldt, n_slab, min(R, 3), [(0, M, 2)], 3, stride_pad=8 + (-((M - 1) * ldt + R)) % 4)


def test_element_path_beyond_the_grid_cap(ops):
    """T 4-byte aligned only: element accesses, 513 x 3648 x 2 of them under a grid of 2048 x 256 threads."""
    run_case(ops, 513, 3648, 3648, 2, 3648, [(0, 513, 1)], 3, base=17)


@pytest.mark.parametrize("R,period", [(6, 1), (64, 1), (24, 6), (18, 6), (256, 64)])
def test_period_shorter_than_the_row(ops, R, period):
    """The fused GEMMs' scratch: R / period modules side by side, all read the same period table columns; w_ld > period."""
    for M in (1, 70):
        for ldt in (R, R + 4):
            run_case(ops, M, R, ldt, 3, period, [(0, M, 1)], 3, stride_pad=8 + (-((M - 1) * ldt + R)) % 4)
            run_case(ops, M, R, ldt, 1, period, [(0, M, 5)], 2)


@pytest.mark.parametrize("R", [16, 18, 256])
def test_segments(ops, R):
    """Two token streams inside 70 rows (rows 0-4 and 37-39 belong to neither and keep their bits), and three with different rows per
    image."""
    for ldt in (R, R + 4):
        for n_slab in (1, 4):
            pad = 8 + (-(69 * ldt + R)) % 4
            run_case(ops, 70, R, ldt, n_slab, R, [(5, 32, 16), (40, 30, 15)], 2, stride_pad=pad)
            run_case(ops, 70, R, ldt, n_slab, R, [(0, 12, 4), (14, 20, 10), (40, 30, 6)], 3, stride_pad=pad)
            run_case(ops, 70, R, ldt, n_slab, R, [(40, 30, 15), (5, 32, 16)], 2)                 # segments need not be in row order
