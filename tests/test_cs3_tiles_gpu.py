"""The CS3 / DGF kernels (csrc/cs3.hip, csrc/dgf.hip) launch by launch against float64 (tests/helpers.py; pinned on the CPU by
tests/test_cs3_ref_cpu.py): every template instance the dispatch code can choose, per output row / 64-position tile / sequence, in
sentinel-filled and over-allocated buffers with strided views, plus determinism, batch-position invariance, tile-choice independence,
the top-k tie rule and the kept set at full size. lx_duan_fwd is read stage by stage out of a workspace the test owns, at the layout
documented in include/lx.h; every stage's reference takes what the PREVIOUS launch left on the GPU, so each launch is judged alone, and
the final y is also held to the end-to-end float64 DUAN.

Two checks per launch:
  * the worst row / tile / sequence inside the project's whole-tensor bound for that kernel (BOUND below);
  * a derived per-element bound from float64 magnitudes (u = 2^-24, gamma_n = n u / (1 - n u), mag = sum_k |w_k||x_k| + |bias|):
      exact-fp32 dot products      gamma_(K+c) mag + u |ref|  (c = the epilogue's operations), any summation order;
      split-bf16 GEMMs             x = xh + xl + rx with |xl| <= 2^-9 (1 + 2^-9)|x|, |rx| <= 2^-18 |x| (two round-to-nearest bf16 steps), W
                                   likewise; the kernels sum Wh Xl + Wl Xh + Wh Xh, so w x - (sum) = wl xl + rw x + (wh + wl) rx
                                   <= 3 * 2^-18 (1 + 2^-8) |w||x|; the 3K bf16 x bf16 products are exact in fp32 and their fp32 accumulation
                                   (plus bias and epilogue) adds gamma_(3K+3) (1 + 2^-6) mag;
      sigmoid                      slope <= 1/4 on the argument's error; __expf is v_exp_f32 (1 ulp, CDNA ISA guide) of a * log2(e) rounded
                                   once (relative u on the argument = |a| u on the result: the HIP math API lists __expf as an
                                   argument-dependent intrinsic for this reason): (|a| + 2) u relative on e, times s (1 - s); 1 + e and the
                                   division / v_rcp_f32 (1 ulp) add 3 u s;
      a 64-position tile sum       64 u times the sum: holds for any summation order.
Run with -s for the table of the worst value of every kernel family against its bound.

Worst value per kernel family on an MI355X, against its bound ("derived" rows: the largest |error| / derived bound over all elements):
  family                      project bound: worst / bound     derived bound: worst ratio
  chan_gemm_f32 (epi 0-2)     9.0e-7 / 2e-6                    0.45
  chan_gemm_f32 part (epi 3)  (within the 2e-6 above)          0.036
  linear_f32 skinny           1.0e-7 / 3e-6                    0.003
  linear_f32 tiled            5.4e-7 / 1e-5                    0.44
  chanmix                     7.5e-7 / 1e-5                    0.40 (plain variants)
  pyramid_pool                1.2e-7 / 1e-6                    0.31
  layernorm_relu              1.8e-7 / 1e-5 (2.04e-5 before    0.008
                              the statistics were taken of x - x[0]: rows offset by 1e3)
  s4_scan, both modes         5.6e-8 / 2e-5                    -
  s4_conv (L = 8192)          9.1e-8 / 2e-5                    0.001
  duan y, end to end          2.7e-7 / 2e-5                    0.999 (apply: one fma, bound u |y|)
  duan stats mean / var / cmean                                0.013 / 0.012 / 0.013
  duan hid (split-bf16)                                        0.68
  duan gpart split-bf16 / scalar gate                          0.050 / 0.009
  duan cpart / coef A / coef Bc / imp                          0.028 / 0.083 / 0.043 / 0.027
The variance bound gamma_(L+4) var is wider than 1 / L at L >= 4098: a variance divided by L - 1 in the generic statistics body is caught
by the end-to-end y bound (5.9e-5 and 1.2e-4 against 2e-5), not by the stage bound."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests.helpers import U24, gamma_n  # noqa: E402
from tests.test_kernels_gpu import DEV, ops  # noqa: E402,F401
from tests.test_rowops_gpu import bits, check_footprint, sentinel  # noqa: E402

F32 = torch.float32
# the project's whole-tensor bounds (tests/test_kernels_gpu.py, tests/test_cs3_gpu.py), here held by the WORST row / tile / sequence
BOUND = {"chan_gemm_f32": 2e-6, "linear_skinny": 3e-6, "linear_tiled": 1e-5, "chanmix": 1e-5, "layernorm_relu": 1e-5, "pyramid_pool": 1e-6,
         "s4": 2e-5, "duan_y": 2e-5}
SPLIT_DROP = 3 * 2.0 ** -18 * (1 + 2.0 ** -8)
REPORT = {}               # family -> (worst / bound ratio, worst, bound)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\nCS3 / DGF worst value per kernel family (worst, bound, ratio):")
        for k, (r, w, b) in sorted(REPORT.items()):
            print(f"  {k:34s} {w:.3e}  {b:.3e}  {r:.3f}")


def note(family, worst, bound):
    worst, bound = float(worst), float(bound)
    r = worst / bound if bound > 0 else (0.0 if worst == 0 else float("inf"))
    if family not in REPORT or r > REPORT[family][0]:
        REPORT[family] = (r, worst, bound)


def hold(family, worst, bound, what=""):
    """record, then assert worst < bound"""
    note(family, worst, bound)
    assert float(worst) < bound, f"{family} {what}: worst {float(worst):.3e} >= bound {bound:.3e}"


def hold_elem(family, got, ref, bound, what=""):
    """per-element derived bound: max of |got - ref| / bound must stay below 1"""
    err = (got.double() - ref.double()).abs()
    ratio = err / bound.clamp_min(1e-300)
    i = int(ratio.argmax())
    r = float(ratio.flatten()[i])
    note(family + " (derived, err/bound)", r, 1.0)
    assert r <= 1.0, (f"{family} {what}: element {np.unravel_index(i, tuple(ratio.shape))} off by {float(err.flatten()[i]):.3e}, derived bound "
                      f"{float(bound.flatten()[i]):.3e} (ratio {r:.2f})")


def rows_rel(got, ref):
    """relative L2 error of every row (last dim)"""
    got, ref = got.double(), ref.double()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def padded(shape, lead=64, tail=64):
    """a sentinel-filled flat fp32 buffer with `lead` / `tail` extra words around a contiguous view of `shape` (lead % 4 == 0: 16-byte aligned)"""
    n = int(np.prod(shape))
    flat = sentinel((lead + n + tail,), F32)
    inside = torch.zeros(lead + n + tail, dtype=torch.bool, device=DEV)
    inside[lead:lead + n] = True
    return flat, flat[lead:lead + n].view(*shape), inside


def strided(shape, ld, bstride=None, lead=64, tail=64):
    """sentinel-filled [.., R, ld]-strided view of logical `shape` ([B,] R, L): returns (flat, view, inside mask over flat)"""
    if len(shape) == 2:
        R, L = shape
        n = R * ld
        flat = sentinel((lead + n + tail,), F32)
        view = flat[lead:lead + n].view(R, ld)[:, :L]
        inside = torch.zeros_like(flat, dtype=torch.bool)
        inside[lead:lead + n].view(R, ld)[:, :L] = True
        return flat, view, inside
    Bn, R, L = shape
    bstride = bstride or R * ld
    n = Bn * bstride
    flat = sentinel((lead + n + tail,), F32)
    view = flat[lead:lead + n].view(Bn, bstride)[:, :R * ld].view(Bn, R, ld)[:, :, :L]
    inside = torch.zeros_like(flat, dtype=torch.bool)
    inside[lead:lead + n].view(Bn, bstride)[:, :R * ld].view(Bn, R, ld)[:, :, :L] = True
    return flat, view, inside


def stream():
    return torch.cuda.current_stream().cuda_stream


def untouched(flat, what):
    sent = bits(sentinel((1,), F32))[0]
    assert bool((bits(flat) == sent).all()), f"{what}: a rejected call wrote to its output"


# ================================================================================================ lx_s4_scan / lx_s4_conv
S4_L = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
_S4 = {}


def _s4_layer(Hc, N, L):
    """(lam, w, D, K) of a seeded layer; for L >= 2048 the 64-mode layer keeps N = 64 but 8 channels, so the float64 kernel stays in seconds"""
    from oracle import s4
    if Hc == 64 and L >= 2048:
        Hc = 8
    key = (Hc, N, L)
    if key not in _S4:
        pr = s4.S4Layer(Hc, N, L, torch.Generator().manual_seed(3)).params_np()
        lam, w = s4.diagonalize(pr, L)
        _S4[key] = (Hc, lam, w, pr["D"], s4.kernel_genfunc(pr, L))
    return _S4[key]


@pytest.mark.parametrize("mode", ["default", "one_wave"])
@pytest.mark.parametrize("HN", [(4, 4), (6, 6), (64, 64)])
@pytest.mark.parametrize("L", S4_L)
def test_s4_scan_every_instance_per_sequence(ops, monkeypatch, mode, HN, L):
    """default: s4_scan_mw_kernel<1,2> (128), <1,4> (256), <2,4>, <4,4>, <8,4>, <16,4>, <32,4> (8192) and the one-wave fallback at L = 64;
    LX_S4_MULTIWAVE=0: s4_scan_kernel<1 ... 64> (L = 64 ... 4096); L = 8192 has no one-wave instance and must be refused untouched."""
    Hc, lam, w, D, K = _s4_layer(HN[0], HN[1], L)
    B = 3
    u = rnd(B, Hc, L, seed=L + Hc)
    u[2] = u[0]                                                    # batch-position invariance
    lam_t = torch.from_numpy(np.stack([lam.real, lam.imag], -1)).to(DEV)
    w_t = torch.from_numpy(np.stack([w.real, w.imag], -1)).to(DEV)
    Dk = torch.from_numpy(D).float().to(DEV)
    if mode == "one_wave":
        monkeypatch.setenv("LX_S4_MULTIWAVE", "0")
    flat, y, inside = padded((B, Hc, L))
    rc = ops.lib.lx_s4_scan(u.data_ptr(), lam_t.data_ptr(), w_t.data_ptr(), Dk.data_ptr(), y.data_ptr(), B, Hc, L, HN[1], stream())
    torch.cuda.synchronize()
    if mode == "one_wave" and L == 8192:
        assert rc == -2                                            # LX_ERR_UNSUPPORTED
        untouched(flat, "lx_s4_scan L=8192 one-wave")
        return
    assert rc == 0
    check_footprint("s4_scan", flat, inside)
    ref = H.s4_fft_conv(u.cpu().numpy(), K, D.astype(np.float32).astype(np.float64))
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref).max(-1)                     # per (b, h) sequence
    bound = BOUND["s4"] * np.maximum(1.0, np.abs(ref).max(-1))
    i = int((err / bound).argmax())
    hold(f"s4_scan {mode}", err.flatten()[i] / bound.flatten()[i] * BOUND["s4"], BOUND["s4"], f"sequence {np.unravel_index(i, err.shape)}")
    assert torch.equal(y[2], y[0])
    flat2, y2, _ = padded((B, Hc, L))
    ops.s4_scan(u, lam_t, w_t, Dk, y2)
    assert torch.equal(bits(flat2), bits(flat))                     # run-to-run determinism, footprint included
    ops.s4_scan(u[1:2].contiguous(), lam_t, w_t, Dk, y1 := torch.empty(1, Hc, L, device=DEV))
    assert torch.equal(y1[0], y[1])                                # a sample alone in a launch gives the same bits


@pytest.mark.parametrize("mode", ["default", "one_wave"])
def test_s4_scan_rejects_l_192_untouched(ops, monkeypatch, mode):
    if mode == "one_wave":
        monkeypatch.setenv("LX_S4_MULTIWAVE", "0")
    Hc, lam, w, D, _ = _s4_layer(4, 4, 256)
    u = rnd(2, Hc, 192, seed=1)
    lam_t = torch.from_numpy(np.stack([lam.real, lam.imag], -1)).to(DEV)
    w_t = torch.from_numpy(np.stack([w.real, w.imag], -1)).to(DEV)
    Dk = torch.from_numpy(D).float().to(DEV)
    flat, y, _ = padded((2, Hc, 192))
    assert ops.lib.lx_s4_scan(u.data_ptr(), lam_t.data_ptr(), w_t.data_ptr(), Dk.data_ptr(), y.data_ptr(), 2, Hc, 192, 4, stream()) == -2
    torch.cuda.synchronize()
    untouched(flat, "lx_s4_scan L=192")


def test_s4_conv_at_its_limit_and_past_it(ops):
    L = 8192
    Hc, lam, w, D, K = _s4_layer(4, 4, L)
    B = 3
    u = rnd(B, Hc, L, seed=11)
    u[2] = u[0]
    Kf = torch.from_numpy(K).float().to(DEV)
    Dk = torch.from_numpy(D).float().to(DEV)
    flat, y, inside = padded((B, Hc, L))
    ops.s4_conv(u, Kf, Dk, y)
    check_footprint("s4_conv", flat, inside)
    ref = H.s4_fft_conv(u.cpu().numpy(), Kf.cpu().numpy(), Dk.cpu().numpy())        # the kernel as the GPU read it (fp32-rounded)
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref).max(-1)
    bound = BOUND["s4"] * np.maximum(1.0, np.abs(ref).max(-1))
    hold("s4_conv", (err / bound).max() * BOUND["s4"], BOUND["s4"])
    # derived: an fp32 fma chain of l + 1 terms in two halves: gamma_(L/2 + 3) sum |K||u|
    mag = H.s4_fft_conv(np.abs(u.cpu().numpy()), np.abs(Kf.cpu().numpy()), np.abs(Dk.cpu().numpy()))
    hold_elem("s4_conv", y.cpu(), torch.from_numpy(ref), torch.from_numpy(gamma_n(L // 2 + 3) * mag + U24 * np.abs(ref)))
    assert torch.equal(y[2], y[0])
    flat1, y1, _ = padded((B, Hc, L))
    ops.s4_conv(u, Kf, Dk, y1)
    assert torch.equal(bits(flat1), bits(flat))                    # run-to-run determinism, footprint included
    from loongx_amd._lib import LxError
    flat2, y2, _ = padded((1, Hc, 8193))
    with pytest.raises(LxError):
        ops.s4_conv(rnd(1, Hc, 8193, seed=1), rnd(Hc, 8193, seed=2), Dk, y2)
    torch.cuda.synchronize()
    untouched(flat2, "lx_s4_conv L=8193")


# ================================================================================================ lx_chan_gemm_f32
def _chan_gemm(ops, X, W, ldw, bias, Y, N, K, L, epi, part=None):
    rc = ops.lib.lx_chan_gemm_f32(X.data_ptr(), X.stride(0), X.stride(1), W.data_ptr(), ldw, None if bias is None else bias.data_ptr(),
                                  None if Y is None else Y.data_ptr(), 0 if Y is None else Y.stride(0), 0 if Y is None else Y.stride(1),
                                  X.shape[0], N, K, L, epi, None if part is None else part.data_ptr(), stream())
    assert rc == 0, ops.lib.lx_last_error()


@pytest.mark.parametrize("K", [4, 36, 1024])
@pytest.mark.parametrize("L", [48, 200, 4100])
@pytest.mark.parametrize("N", [8, 130, 512])
def test_chan_gemm_f32_every_epilogue_per_row_and_tile(ops, N, L, K):
    B = 3
    ldx, ldy, ldw = L + 4, L + 12, K + 8                           # strided views: rows wider than the data, batch strides larger than C L
    xs = strided((B, K, L), ldx, bstride=K * ldx + 16)
    xs[1].copy_(rnd(B, K, L, seed=1))
    xs[1][2] = xs[1][0]
    X = xs[1]
    Wf = rnd(N, ldw, seed=2, scale=0.1)
    W, bias = Wf[:, :K], rnd(N, seed=3)
    z, mag = H.chan_gemm_ref(X, W, bias)
    eb = gamma_n(K + 2) * mag
    for epi in (0, 1, 2):
        flat, Y, inside = strided((B, N, L), ldy, bstride=N * ldy + 20)
        ref, init = z, None
        if epi == 1:
            Y.copy_(rnd(B, N, L, seed=4))
            Y[2] = Y[0]
            init = flat.clone()
            ref = z + Y.double()
        elif epi == 2:
            ref = torch.relu(z)
        start = flat.clone()
        _chan_gemm(ops, X, W, ldw, bias, Y, N, K, L, epi)
        check_footprint(f"chan_gemm_f32 epi {epi}", flat, inside, init)
        hold_elem("chan_gemm_f32", Y, ref, eb + 2 * U24 * ref.abs(), f"epilogue {epi}")
        # worst (b, n) row; a ReLU row is measured against the norm of its pre-activation row: ReLU is 1-Lipschitz, so the row's error is
        # bounded by the GEMM row's, while what is left of a row under a negative bias can be arbitrarily small next to it
        rel = (Y.double() - ref).norm(dim=-1) / (z if epi == 2 else ref).norm(dim=-1).clamp_min(1e-300)
        hold("chan_gemm_f32", rel.max(), BOUND["chan_gemm_f32"], f"epilogue {epi}: worst (b, n) row")
        assert torch.equal(Y[2], Y[0])
        flat2 = start.clone()                                      # the same launch on the same initial buffer: the same bits
        Y2 = flat2.as_strided(Y.shape, Y.stride(), Y.storage_offset())
        _chan_gemm(ops, X, W, ldw, bias, Y2, N, K, L, epi)
        assert torch.equal(bits(flat2), bits(flat))
    nt = (L + 63) // 64
    flat, part, inside = padded((B, nt, N))
    _chan_gemm(ops, X, W, ldw, bias, None, N, K, L, 3, part)
    check_footprint("chan_gemm_f32 epi 3", flat, inside)
    s = torch.sigmoid(z)
    es = eb / 4 + s * (1 - s) * (z.abs() + 2) * U24 + 3 * U24 * s
    ref = H.tile_sums(s)
    hold_elem("chan_gemm_f32 part", part, ref, H.tile_sums(es) + 64 * U24 * ref, "per (b, tile, n)")
    hold("chan_gemm_f32", rows_rel(part, ref).max(), BOUND["chan_gemm_f32"], "worst part[b][tile] row")
    assert torch.equal(part[2], part[0])
    flat2, part2, _ = padded((B, nt, N))
    _chan_gemm(ops, X, W, ldw, bias, None, N, K, L, 3, part2)
    assert torch.equal(bits(flat2), bits(flat))


# ================================================================================================ lx_linear_f32
LINEAR = [  # (M, N, K, x misaligned, kernel family)
    (4, 64, 512, False, "skinny"), (5, 64, 512, False, "skinny"), (16, 70, 256, False, "skinny"), (17, 70, 256, False, "tiled"),
    (3, 13, 252, False, "tiled"), (3, 13, 256, False, "skinny"), (2, 9, 260, False, "skinny"), (16, 771, 1356, False, "skinny"),
    (1, 8, 1024, False, "skinny"), (3, 64, 512, True, "tiled"), (67, 130, 36, False, "tiled")]


@pytest.mark.parametrize("M,N,K,misaligned,family", LINEAR)
def test_linear_f32_dispatch_edges_per_row(ops, M, N, K, misaligned, family):
    """M = 4 | 5 (skinny <4> | <16>), 16 | 17 (skinny | tiled), K = 252 | 256, K % 256 != 0, N % 8 != 0, an X that is not 16-byte aligned."""
    ldx, ldw, ldy = K + 4, K + 8, N + 5
    xflat = torch.zeros(M * ldx + 8, device=DEV)
    off = 1 if misaligned else 0
    X = xflat[off:off + M * ldx].view(M, ldx)[:, :K]
    X.copy_(rnd(M, K, seed=4))
    W = rnd(N, ldw, seed=5, scale=0.05)[:, :K]
    bias = rnd(N, seed=6)
    ref, mag = H.linear_ref(X, W, bias)
    fam = "linear_" + family
    flat, Y, inside = strided((M, N), ldy)
    ops.linear_f32(X, W, bias, Y, M=M, N=N, K=K, ldx=ldx, ldy=ldy, ldw=ldw)
    check_footprint(fam, flat, inside)
    hold_elem(fam, Y, ref, gamma_n(K + 2) * mag + U24 * ref.abs())
    hold(fam, rows_rel(Y, ref).max(), BOUND[fam], "worst row")
    flat2, Y2, _ = strided((M, N), ldy)
    ops.linear_f32(X, W, bias, Y2, M=M, N=N, K=K, ldx=ldx, ldy=ldy, ldw=ldw)
    assert torch.equal(bits(flat2), bits(flat))
    init = flat.clone()
    y0 = Y.double().clone()
    ops.linear_f32(X, W, None, Y, M=M, N=N, K=K, ldx=ldx, ldy=ldy, ldw=ldw, accumulate=True)
    check_footprint(fam + " accumulate", flat, inside, init)
    ref2, mag2 = H.linear_ref(X, W, None)
    hold_elem(fam, Y, y0 + ref2, gamma_n(K + 2) * mag2 + U24 * (y0 + ref2).abs(), "accumulate")
    # row-position invariance: rows 1.. launched alone keep their bits (M = 16 -> 15 stays on skinny <16>, 67 -> 66 on the tiled kernel)
    if M in (16, 67):
        _, Y1, _ = strided((M, N), ldy)
        ops.linear_f32(X[1:], W, bias, Y1, M=M - 1, N=N, K=K, ldx=ldx, ldy=ldy, ldw=ldw)
        assert torch.equal(Y1[:M - 1], Y2[1:])


@pytest.mark.parametrize("M,N,K", [(67, 130, 36), (5, 9, 300), (130, 65, 8)])
def test_linear_f32_transposed_ragged(ops, M, N, K):
    X, W, bias = rnd(M, K, seed=7), rnd(N, K, seed=8, scale=0.1), rnd(N, seed=9)
    ref, mag = H.linear_ref(X, W, bias)
    ldx, ldy = M + 3, M + 6
    Xt = torch.zeros(K, ldx, device=DEV)
    Xt[:, :M] = X.T
    flat, Yt, inside = strided((N, M), ldy)
    ops.linear_f32(Xt, W, bias, Yt, M=M, N=N, K=K, ldx=ldx, ldy=ldy, x_trans=True, y_trans=True)
    check_footprint("linear_tiled transposed", flat, inside)
    hold_elem("linear_tiled", Yt.T, ref, gamma_n(K + 2) * mag + U24 * ref.abs(), "x_trans / y_trans")
    hold("linear_tiled", rows_rel(Yt.T, ref).max(), BOUND["linear_tiled"], "worst row, transposed")
    flat2, Yt2, _ = strided((N, M), ldy)
    ops.linear_f32(Xt, W, bias, Yt2, M=M, N=N, K=K, ldx=ldx, ldy=ldy, x_trans=True, y_trans=True)
    assert torch.equal(bits(flat2), bits(flat))
    _, Yt1, _ = strided((N, M), ldy)                               # rows 1.. of X alone (columns of Xt): the same bits
    ops.linear_f32(Xt[:, 1:], W, bias, Yt1, M=M - 1, N=N, K=K, ldx=ldx, ldy=ldy, x_trans=True, y_trans=True)
    assert torch.equal(Yt1[:, :M - 1], Yt[:, 1:])
    init, y0 = flat.clone(), Yt.T.double().clone()
    ops.linear_f32(Xt, W, None, Yt, M=M, N=N, K=K, ldx=ldx, ldy=ldy, x_trans=True, y_trans=True, accumulate=True)
    check_footprint("linear_tiled transposed accumulate", flat, inside, init)
    ref2, mag2 = H.linear_ref(X, W, None)
    hold_elem("linear_tiled", Yt.T, y0 + ref2, gamma_n(K + 2) * mag2 + U24 * (y0 + ref2).abs(), "transposed accumulate")


# ================================================================================================ lx_chanmix
@pytest.mark.parametrize("L", [1, 255, 256, 257, 4096])
@pytest.mark.parametrize("hin,hout", [(4, 64), (64, 64), (4, 4), (6, 6)])
def test_chanmix_every_instance_per_position(ops, hin, hout, L):
    B = 3
    x, W, b = rnd(B, hin, L, seed=1), rnd(hout, hin, seed=2, scale=0.3), rnd(hout, seed=3)
    x[2] = x[0]
    res = rnd(B, hout, L, seed=4)
    res[2] = res[0]
    g, be = 1 + 0.1 * rnd(hout, seed=5), rnd(hout, seed=6, scale=0.1)
    variants = [("gelu+resid+ln", dict(bias=b, resid=res, ln_g=g, ln_b=be, act=1)), ("bare", dict(bias=b, act=0)),
                ("resid", dict(bias=None, resid=res, act=0)), ("gelu+ln", dict(bias=b, ln_g=g, ln_b=be, act=1))]
    for name, kw in variants:
        flat, y, inside = padded((B, hout, L))
        ops.chanmix(x, W, kw.get("bias"), kw.get("resid"), kw.get("ln_g"), kw.get("ln_b"), y, act=kw["act"])
        check_footprint(f"chanmix {name}", flat, inside)
        ref = H.chanmix_ref(x, W, **kw)
        hold("chanmix", rows_rel(y.permute(0, 2, 1), ref.permute(0, 2, 1)).max(), BOUND["chanmix"], f"{name}: worst position")
        # derived bound: only where the launch is an exact-fp32 fma chain + bias + residual. The GELU / LayerNorm variants get the project's
        # bound alone: a per-element bound there needs erff's error, which the device library does not state as a guaranteed figure, and
        # the LayerNorm's 1 / sqrt(var) conditioning over 4 or 6 channels makes a worst-case bound vacuous at near-constant positions.
        if kw["act"] == 0 and "ln_g" not in kw:
            z, mag = H.chan_gemm_ref(x, W, kw.get("bias"))
            if "resid" in kw:
                mag = mag + res.double().abs()
            hold_elem("chanmix", y, ref, gamma_n(hin + 3) * mag + U24 * ref.abs(), name)
        assert torch.equal(y[2], y[0])
        flat2, y2, _ = padded((B, hout, L))
        ops.chanmix(x, W, kw.get("bias"), kw.get("resid"), kw.get("ln_g"), kw.get("ln_b"), y2, act=kw["act"])
        assert torch.equal(bits(flat2), bits(flat))


# ================================================================================================ lx_pyramid_pool / lx_layernorm_relu
@pytest.mark.parametrize("L,sizes", [(50, [7, 64, 3]), (4096, [128, 100, 33]), (130, [129, 1, 8, 131]), (256, [64, 128, 256])])
def test_pyramid_pool_columns_and_footprint(ops, L, sizes):
    """y_col0 > 0, ldy wider than the columns written, sizes that do not divide L and sizes > L (nn.AdaptiveAvgPool1d repeats samples)."""
    B, Cc, col0 = 3, 5, 5
    tot = sum(sizes)
    ldy = col0 + tot + 7
    x = rnd(B, Cc, L, seed=2) + 0.5
    x[2] = x[0]
    flat, yv, inside = strided((B, Cc, ldy), ldy)
    inside &= False
    inside[64:64 + B * Cc * ldy].view(B, Cc, ldy)[:, :, col0:col0 + tot] = True
    ops.pyramid_pool(x, yv, sizes, y_col0=col0)
    check_footprint("pyramid_pool", flat, inside)
    got = yv[:, :, col0:col0 + tot]
    ref = H.pyramid_pool_ref(x, sizes)
    hold("pyramid_pool", rows_rel(got, ref).max(), BOUND["pyramid_pool"], "worst row")
    longest = max(-(-L // s) + 1 for s in sizes)
    hold_elem("pyramid_pool", got, ref, gamma_n(longest + 1) * H.pyramid_pool_ref(x.abs(), sizes))
    assert torch.equal(got[2], got[0])
    flat2, yv2, _ = strided((B, Cc, ldy), ldy)
    ops.pyramid_pool(x, yv2, sizes, y_col0=col0)
    assert torch.equal(bits(flat2), bits(flat))


@pytest.mark.parametrize("offset", [0.0, 1e3])
@pytest.mark.parametrize("D", [1, 255, 256, 1000, 2048])
def test_layernorm_relu_per_row(ops, D, offset):
    M = 7
    x0 = rnd(M, D, seed=1, scale=3.0) + offset
    x0[6] = x0[0]
    g, b = 1 + 0.1 * rnd(D, seed=2), rnd(D, seed=3, scale=0.2)
    flat, x, inside = padded((M, D))
    x.copy_(x0)
    init = flat.clone()
    ops.layernorm_relu(x, g, b)
    check_footprint("layernorm_relu", flat, inside, init)
    ref = H.layernorm_relu_ref(x0, g, b)
    if D > 1:
        hold("layernorm_relu", rows_rel(x, ref).max(), BOUND["layernorm_relu"], f"worst row (offset {offset:g})")
    # derived, for statistics taken of t = x - x[0] as the kernel takes them: t_i carries u |t_i|, the mean of t over D terms in any order
    # is off by em <= gamma_(D+2) mean|t|, so x_i - mean moves by e1 = em + u max|t| (+ u |d_i| for its own rounding) whatever offset the
    # row sits on; the variance's relative error (gamma_(D+4) on the sum of squares, 2 e1 mean|d| + e1^2 from the shifted deviations)
    # halves into rstd (rsqrtf: 1 ulp); the affine and the store add 4 u
    xd = x0.double()
    t = xd - xd[:, :1]
    m = xd.mean(-1, keepdim=True)
    d = xd - m
    var = (d * d).mean(-1, keepdim=True)
    absd = d.abs().mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-5)
    e1 = gamma_n(D + 2) * t.abs().mean(-1, keepdim=True) + U24 * t.abs().amax(-1, keepdim=True)
    evar = gamma_n(D + 4) * (var + 2 * e1 * absd + e1 * e1) + 2 * e1 * absd + e1 * e1
    erel = 0.5 * evar / (var + 1e-5) + 3 * U24
    pre = d * rstd * g.double()
    bound = (e1 + U24 * d.abs()) * rstd * g.double().abs() + pre.abs() * (erel + 4 * U24) + 2 * U24 * (pre.abs() + b.double().abs())
    hold_elem("layernorm_relu", x, ref, bound, f"offset {offset:g}")
    flat2 = init.clone()
    ops.layernorm_relu(flat2[64:64 + M * D].view(M, D), g, b)
    assert torch.equal(bits(flat2), bits(flat))                    # run-to-run determinism
    assert torch.equal(x[6], x[0])


# ================================================================================================ lx_duan_fwd, stage by stage
def _align(p, a=256):
    return (p + a - 1) // a * a


class DuanRun:
    """One lx_duan_fwd call on a sentinel-filled, over-allocated workspace the test owns, read back at the layout of include/lx.h."""

    def __init__(self, ops, p, x, c, keep_k, eps=1e-3, misalign_gb1=False):
        B, Cc, L = x.shape
        Hd = p["gate.0.weight"].shape[0]
        self.B, self.C, self.L, self.Hd, self.keep_k, self.eps = B, Cc, L, Hd, keep_k, eps
        self.p = {k: v.to(DEV).contiguous() for k, v in p.items()}
        if misalign_gb1:
            hold_buf = torch.zeros(Hd + 4, device=DEV)
            hold_buf[1:Hd + 1] = self.p["gate.0.bias"]
            self.p["gate.0.bias"] = hold_buf[1:Hd + 1]
        self.x, self.c = x.to(DEV).contiguous(), c.to(DEV).contiguous()
        gb1, gb2 = self.p["gate.0.bias"].data_ptr(), self.p["gate.2.bias"].data_ptr()
        self.mfma = Cc % 4 == 0 and Hd % 4 == 0 and L % 4 == 0
        self.wide = self.mfma and Hd % 128 == 0 and Cc % 128 == 0 and Cc > 128 and (gb1 | gb2) % 16 == 0
        self.tile = 128 if self.wide and B * ((L + 127) // 128) >= 512 else 64
        self.ntile = nt = (L + 63) // 64
        self.nbytes = int(ops.lib.lx_duan_workspace_bytes(B, Cc, L, Hd))
        extra = 4096
        self.ws = sentinel(((self.nbytes + 3) // 4 + extra,), F32)
        base = self.ws.data_ptr()
        o_stats = _align(base) - base
        o_gpart = o_stats + 4 * B * Cc * 4
        o_coef = o_gpart + 4 * B * nt * Cc
        o_imp = o_coef + 4 * B * Cc * 2
        o_hid = _align(base + o_imp + 4 * B * Cc) - base
        o_cpart = _align(base + o_hid + 4 * B * Hd * L) - base
        o_w = _align(base + o_cpart + 4 * B * nt * Cc) - base
        self.off = dict(stats=o_stats, gpart=o_gpart, coef=o_coef, imp=o_imp, hid=o_hid, cpart=o_cpart, w=o_w, end=o_w + 8 * Hd * Cc)
        assert self.off["end"] <= self.nbytes
        self.yflat, self.y, self.yinside = padded((B, Cc, L))
        q = self.p
        rc = ops.lib.lx_duan_fwd(self.x.data_ptr(), self.c.data_ptr(), q["gate.0.weight"].data_ptr(), gb1, q["gate.2.weight"].data_ptr(), gb2,
                                 q["mlp.0.weight"].data_ptr(), q["mlp.0.bias"].data_ptr(), q["mlp.2.weight"].data_ptr(),
                                 q["mlp.2.bias"].data_ptr(), self.y.data_ptr(), B, Cc, L, Hd, eps, keep_k, self.ws.data_ptr(), self.nbytes, stream())
        assert rc == 0, ops.lib.lx_last_error()
        torch.cuda.synchronize()

    def words(self, name, n):
        o = self.off[name] // 4
        return self.ws[o:o + n]

    @property
    def stats(self):
        return self.words("stats", self.B * self.C * 4).view(self.B, self.C, 4)

    @property
    def gpart(self):
        return self.words("gpart", self.B * self.ntile * self.C).view(self.B, self.ntile, self.C)

    @property
    def coef(self):
        return self.words("coef", self.B * self.C * 2).view(self.B, self.C, 2)

    @property
    def imp(self):
        return self.words("imp", self.B * self.C).view(self.B, self.C)

    @property
    def hid(self):
        return self.words("hid", self.B * self.Hd * self.L).view(self.B, self.Hd, self.L)

    @property
    def cpart(self):
        return self.words("cpart", self.B * self.ntile * self.C).view(self.B, self.ntile, self.C)

    def check_footprint(self):
        """the workspace holds exactly the documented regions; stats[..][3] is never written, stats[..][2] only on the non-wide path,
        hid only by the MFMA gate, cpart and the weight images only by the wide form; nothing at or past lx_duan_workspace_bytes changes"""
        sent = bits(sentinel((1,), F32))[0]
        w = bits(self.ws)
        inside = torch.zeros_like(w, dtype=torch.bool)

        def mark(name, n):
            inside[self.off[name] // 4: self.off[name] // 4 + n] = True
        B, Cc, L, Hd, nt = self.B, self.C, self.L, self.Hd, self.ntile
        mark("stats", B * Cc * 4)
        sv = inside[self.off["stats"] // 4: self.off["stats"] // 4 + B * Cc * 4].view(B, Cc, 4)
        sv[:, :, 3] = False
        if self.wide:
            sv[:, :, 2] = False
        mark("gpart", B * nt * Cc), mark("coef", B * Cc * 2), mark("imp", B * Cc)
        if self.mfma:
            mark("hid", B * Hd * L)
        if self.wide:
            mark("cpart", B * nt * Cc)
        images = torch.zeros_like(inside)
        if self.wide:
            images[self.off["w"] // 4: self.off["end"] // 4] = True
        changed = w != sent
        stray = changed & ~inside & ~images
        assert not bool(stray.any()), f"workspace: {int(stray.sum())} words outside the documented regions changed (first at word {int(stray.nonzero()[0])})"
        assert not bool(changed[(self.nbytes + 3) // 4:].any()), "workspace: written past lx_duan_workspace_bytes"
        vals = self.ws[inside]
        assert bool(torch.isfinite(vals).all()) and not bool((bits(vals) == sent).any()), "workspace: a documented region was left unwritten"
        check_footprint("duan y", self.yflat, self.yinside)


def _bound_split(K, mag, ref):
    return (SPLIT_DROP + gamma_n(3 * K + 3) * (1 + 2.0 ** -6)) * mag + U24 * ref.abs()


def _sigmoid_err(z, ez):
    s = torch.sigmoid(z)
    return s, ez / 4 + s * (1 - s) * (z.abs() + 2) * U24 + 3 * U24 * s


def check_duan_stages(r, name):
    """every launch of lx_duan_fwd against float64 of what the previous launch left on the GPU"""
    B, Cc, L, Hd, p = r.B, r.C, r.L, r.Hd, r.p
    x, c = r.x.double(), r.c.double()
    r.check_footprint()
    # ---- 1 stats: two-pass mean / variance per row (any summation order), the condition's mean on the non-wide path
    mean, absx = x.mean(2), x.abs().mean(2)
    d = x - mean[:, :, None]
    var, absd = (d * d).mean(2), d.abs().mean(2)
    em = gamma_n(L + 1) * absx
    hold_elem("duan stats mean", r.stats[:, :, 0], mean, em + U24 * mean.abs(), name)
    evar = gamma_n(L + 4) * (var + 2 * em * absd + em * em) + 2 * em * absd + em * em
    hold_elem("duan stats var", r.stats[:, :, 1], var, evar, name)
    if not r.wide:
        hold_elem("duan stats cmean", r.stats[:, :, 2], c.mean(2), gamma_n(L + 1) * c.abs().mean(2), name)
    # ---- 2 gate
    w1, b1, w2, b2 = p["gate.0.weight"], p["gate.0.bias"], p["gate.2.weight"], p["gate.2.bias"]
    if r.mfma:
        h, hmag = H.chan_gemm_ref(r.c, w1, b1)
        hold_elem("duan hid (split-bf16)", r.hid, torch.relu(h), _bound_split(Cc, hmag, h), name)
        z, zmag = H.chan_gemm_ref(r.hid, w2, b2)                   # from the hid the GPU wrote
        ez = _bound_split(Hd, zmag, z)
    else:                                                          # scalar gate: hid stays in LDS; both layers are exact-fp32 fma chains
        hid, hmag, z, zmag = H.duan_gate_ref(r.c, p)
        ehid = gamma_n(Cc + 2) * hmag
        ez = torch.einsum("nk,bkl->bnl", w2.double().abs(), ehid) * (1 + gamma_n(Hd + 2)) + gamma_n(Hd + 2) * zmag
    s, es = _sigmoid_err(z, ez)
    gref = H.tile_sums(s)
    hold_elem("duan gpart" + (" (split-bf16)" if r.mfma else " (scalar)"), r.gpart, gref, H.tile_sums(es) + 64 * U24 * gref, name)
    if r.wide:
        hold_elem("duan cpart", r.cpart, H.tile_sums(c), 64 * U24 * H.tile_sums(c.abs()), name)
    # ---- 3 coef, from the GPU's stats / gpart / cpart
    gm, gv = r.stats[:, :, 0].double(), r.stats[:, :, 1].double()
    nt = r.ntile
    g = r.gpart.double().sum(1) / L
    eg = gamma_n(nt + 2) * g
    if r.wide:
        mc = r.cpart.double().sum(1) / L
        emc = gamma_n(nt + 2) * r.cpart.double().abs().sum(1) / L
    else:
        mc, emc = r.stats[:, :, 2].double(), torch.zeros_like(gm)
    A, Bc = H.duan_coef_ref(gm, gv, g, mc, p, r.eps)
    mw1, mb1, mw2, mb2 = (p[k].double() for k in ("mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"))
    hid2 = torch.relu(mc @ mw1.T + mb1)
    ehid2 = emc @ mw1.abs().T + gamma_n(Cc + 2) * (mc.abs() @ mw1.abs().T + mb1.abs())
    egb = ehid2 @ mw2.abs().T + gamma_n(Hd + 2) * ((hid2 + ehid2) @ mw2.abs().T + mb2.abs())
    gam, bet = (hid2 @ mw2.T + mb2)[:, :Cc], (hid2 @ mw2.T + mb2)[:, Cc:]
    egam, ebet = egb[:, :Cc], egb[:, Cc:]
    mu_l = gm.mean(1, keepdim=True)
    var_l = (gv + (gm - mu_l) ** 2).mean(1, keepdim=True)
    sig_l, sc = torch.sqrt(var_l + r.eps), torch.sqrt(gv + r.eps)
    emul, esigl = U24 * mu_l.abs(), 2.5 * U24 * sig_l               # fp64 in the kernel, rounded once; (float)var + eps, sqrtf
    mu = g * gm + (1 - g) * mu_l
    sig = g * sc + (1 - g) * sig_l
    emu = eg * (gm.abs() + mu_l.abs()) + (1 - g) * emul + 3 * U24 * ((g * gm).abs() + ((1 - g) * mu_l).abs())
    esig = eg * (sc + sig_l) + (1 - g) * esigl + 4 * U24 * sig
    eA = (egam + U24 * (1 + gam).abs()) / sig + A.abs() * esig / sig + U24 * A.abs()
    eBc = ebet + eA * mu.abs() + A.abs() * emu + 2 * U24 * (bet.abs() + (A * mu).abs())
    hold_elem("duan coef A", r.coef[:, :, 0], A, eA * 1.001, name)                  # (first-order propagation: 0.1 % for the products of errors)
    hold_elem("duan coef Bc", r.coef[:, :, 1], Bc, eBc * 1.001, name)
    # ---- 4 apply: one fma per element from the GPU's (A, Bc); importance = mean |y| in any order
    yfull = r.coef[:, :, 0:1].double() * x + r.coef[:, :, 1:2].double()
    imp = yfull.abs().mean(2)
    hold_elem("duan imp", r.imp, imp, gamma_n(L + 2) * imp, name)
    # ---- 5 mask: a stable descending sort of the GPU's own importances, no tolerance
    keep = H.stable_topk_mask(r.imp, r.keep_k)
    kept_gpu = r.y.abs().sum(2) > 0
    assert torch.equal(kept_gpu, keep), f"{name}: kept set differs from the stable top-k of the kernel's own importances"
    assert bool((r.y[~keep] == 0).all())
    yk = yfull * keep[:, :, None]
    hold_elem("duan y (apply)", r.y, yk, U24 * yk.abs() * 1.001 + 1e-300, name)
    return dict(imp=imp, keep=keep)


def check_duan_end_to_end(r, name, delta=H.DUAN_KEPT_DELTA, max_undecided=None):
    """y against the float64 DUAN: same kept channels except those within delta of the rank boundary; worst kept row within the y bound"""
    st = H.duan_ref_stages(r.x, r.c, r.p, r.keep_k, r.eps)
    undecided = H.kept_set_margin(st["imp"], r.keep_k, delta)
    if max_undecided is not None:
        assert int(undecided.sum(1).max()) <= max_undecided
    kept_gpu = r.y.abs().sum(2) > 0
    diff = (kept_gpu != st["keep"]) & ~undecided
    assert not bool(diff.any()), f"{name}: kept set differs from float64 at decided channels {diff.nonzero().tolist()[:8]}"
    both = kept_gpu & st["keep"]
    if bool(both.any()):
        hold("duan y (end to end)", rows_rel(r.y, st["y_full"])[both].max(), BOUND["duan_y"], f"{name}: worst kept row")
    return st


DUAN_SHAPES = [  # (name, B, C, L, Hd, misaligned gb1)
    ("scalar c1 l768", 3, 1, 768, 128, False), ("scalar c6", 2, 6, 200, 128, False), ("scalar c16 l4098", 2, 16, 4098, 128, False),
    ("scalar c16 l49", 2, 16, 49, 64, False),
    ("split c16", 2, 16, 200, 128, False), ("split c128", 2, 128, 260, 128, False), ("split c16 hd64", 3, 16, 196, 64, False),
    ("split c16 l8192", 2, 16, 8192, 128, False), ("split c256 gb1+4", 2, 256, 196, 128, True),
    ("wide c256 l196", 3, 256, 196, 128, False), ("wide c384 l132", 2, 384, 132, 128, False), ("wide c512 l192", 2, 512, 192, 128, False),
    ("wide c1024 l256", 2, 1024, 256, 128, False), ("wide c256 l8192", 1, 256, 8192, 128, False),
    ("wide128 c256 b64 l1024", 64, 256, 1024, 128, False), ("wide128 c256 b128 l516", 128, 256, 516, 128, False),
    ("wide128 c256 b103 l612", 103, 256, 612, 128, False), ("wide128 c256 b128 l548", 128, 256, 548, 128, False),
    ("wide128 c256 b128 l576", 128, 256, 576, 128, False), ("wide128 c256 b128 l580", 128, 256, 580, 128, False),
    ("wide c256 l228", 2, 256, 228, 128, False), ("wide128 c512 b16 l4096", 16, 512, 4096, 128, False)]
# L % 128: 196 -> 68, 132 -> 4, 192 -> 64 at tile 64; at tile 128: 516 -> 4 and 576 -> 64 (the whole second half-tile out of range), 580 -> 68
# (four positions of it in range); 228 -> 100, 548 -> 36 and 612 -> 100 (the
# first position past L falls in the second 32-position block of a 64-position row: where a `<=` for `<` in the tile sum would show)


@pytest.mark.parametrize("name,B,C,L,Hd,mis", DUAN_SHAPES, ids=[s[0].replace(" ", "_") for s in DUAN_SHAPES])
def test_duan_stage_by_stage(ops, name, B, C, L, Hd, mis):
    d, x, c = H.duan_case(C, Hd, B, L, seed=C + L)
    if B > 1:
        x[B - 1], c[B - 1] = x[0], c[0]                            # batch-position invariance
    keep_k = max(1, int(C * 0.7))
    r = DuanRun(ops, H.duan_params(d), x, c, keep_k, d.eps, misalign_gb1=mis)
    assert r.wide == name.startswith("wide") and r.mfma == (not name.startswith("scalar")) and (r.tile == 128) == name.startswith("wide128")
    check_duan_stages(r, name)
    check_duan_end_to_end(r, name)
    if B > 1:
        for what in ("stats", "gpart", "coef", "imp"):
            t = getattr(r, what)
            assert torch.equal(bits(t[B - 1]), bits(t[0])), f"{name}: {what} depends on the batch position"
        assert torch.equal(r.y[B - 1], r.y[0])
    r2 = DuanRun(ops, H.duan_params(d), x, c, keep_k, d.eps, misalign_gb1=mis)
    assert torch.equal(bits(r2.ws), bits(r.ws)) and torch.equal(bits(r2.yflat), bits(r.yflat)), f"{name}: not deterministic"


def test_duan_tile_choice_independence(ops):
    """(C = 512, L = 4096): batch 16 runs the gate's second GEMM on 128-position tiles, two batches of 8 on 64-position tiles; a
    data-parallel shard must reproduce the full batch bit for bit."""
    d, x, c = H.duan_case(512, 128, 16, 4096, seed=5)
    p = H.duan_params(d)
    full = DuanRun(ops, p, x, c, 358, d.eps)
    assert full.tile == 128
    for lo in (0, 8):
        part = DuanRun(ops, p, x[lo:lo + 8], c[lo:lo + 8], 358, d.eps)
        assert part.tile == 64 and part.wide
        for what in ("stats", "gpart", "cpart", "coef", "imp", "hid"):
            a, b = getattr(part, what), getattr(full, what)[lo:lo + 8]
            if what == "stats":
                a, b = a[:, :, :2], b[:, :, :2]
            assert torch.equal(bits(a.contiguous()), bits(b.contiguous())), f"{what} of samples {lo}..{lo + 7} depends on the tile"
        assert torch.equal(part.y, full.y[lo:lo + 8])


def test_duan_top_k_ties_keep_the_lower_channel(ops):
    d, x, c, keep_k = H.duan_tie_case()
    r = DuanRun(ops, H.duan_params(d), x, c, keep_k, d.eps)
    check_duan_stages(r, "ties")
    imp = r.imp
    for i in range(4):
        for k in range(1, 4):
            assert torch.equal(bits(imp[:, i]), bits(imp[:, i + 4 * k])), "duplicated channels must have bit-equal importance"
    st = H.duan_ref_stages(x, c, H.duan_params(d), keep_k, d.eps)          # float64, stable descending argsort (torch.topk's tie order is unspecified)
    kept_gpu = (r.y.abs().sum(2) > 0).cpu()
    assert torch.equal(kept_gpu, st["keep"].cpu())
    for b in range(x.shape[0]):
        s = imp[b].sort(descending=True).values
        assert s[keep_k - 1] == s[keep_k]                          # the cut is inside a group of equal importances
        group = sorted(int(i) for i in (imp[b] == s[keep_k]).nonzero().flatten())
        assert [bool(kept_gpu[b, i]) for i in group] == [True, True, False, False]


@pytest.mark.parametrize("C,L,seed,keep_k", H.DUAN_KEPT_CASES)
def test_duan_kept_set_at_full_size(ops, C, L, seed, keep_k):
    d, x, c = H.duan_case(C, 128, 2, L, seed)
    r = DuanRun(ops, H.duan_params(d), x, c, keep_k, d.eps)
    check_duan_end_to_end(r, f"full size seed {seed}", max_undecided=C // 100)
    assert bool(((r.y.abs().sum(2) > 0).sum(1) == keep_k).all())
