"""Shared helpers for the parity tests (rebuild the seeded tiny modules the goldens were made with)."""
import os

import numpy as np
import torch

from oracle import flux_modules as fm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TINY = dict(num_layers=2, num_single_layers=2, heads=2, head_dim=128, in_channels=64, joint_dim=64,
            pooled_dim=32, guidance_embeds=True, lora=True)


def tiny_transformer(seed=0, **over):
    cfg = dict(TINY)
    cfg.update(over)
    tr = fm.FluxTransformer2DModel(**cfg)
    fm.init_synthetic_(tr, seed=seed, std=0.05, bias_std=0.02, norm_jitter=0.1)
    return tr.eval()


def load(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def relerr(a, b):
    a, b = a.double(), b.double()
    e = float((a - b).norm() / b.norm().clamp_min(1e-30))
    rec = os.environ.get("LX_TEST_RECORD")      # tolerance audit: every measured relative error, per test, to a JSON-lines file
    if rec:
        import inspect
        import json
        fr = inspect.stack()[1]
        with open(rec, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], "line": fr.lineno, "relerr": e}) + "\n")
    return e


# ------------------------------------------------------------------------------------------------ CS3 / DGF float64 references
# Plain float64 restatements of csrc/cs3.hip and csrc/dgf.hip, one function per launch (tests/test_cs3_tiles_gpu.py compares every launch
# with them; tests/test_cs3_ref_cpu.py pins them to oracle.cs3.DUAN and the goldens on the CPU). Inputs may live on any device.
U24 = 2.0 ** -24          # fp32 unit roundoff


def gamma_n(n):
    """(1 + u)^n - 1 <= n u / (1 - n u): the classic bound on n chained fp32 roundings, in any order."""
    return n * U24 / (1.0 - n * U24)


def chan_gemm_ref(X, W, bias=None):
    """z[b, n, l] = sum_k W[n, k] X[b, k, l] + bias[n] in float64, and mag = sum_k |W||X| + |bias| (what a rounding error is relative to)."""
    X, W = X.double(), W.double()
    z = torch.einsum("nk,bkl->bnl", W, X)
    mag = torch.einsum("nk,bkl->bnl", W.abs(), X.abs())
    if bias is not None:
        z = z + bias.double()[None, :, None]
        mag = mag + bias.double().abs()[None, :, None]
    return z, mag


def tile_sums(v, tile=64):
    """[B, C, L] -> [B, ceil(L / tile), C]: sums over each `tile` positions (the ragged last tile sums what it has)."""
    B, C, L = v.shape
    nt = (L + tile - 1) // tile
    p = torch.zeros(B, C, nt * tile, dtype=v.dtype, device=v.device)
    p[:, :, :L] = v
    return p.view(B, C, nt, tile).sum(3).permute(0, 2, 1).contiguous()


def linear_ref(X, W, bias=None):
    """X [M, K] W[N, K]^T + bias in float64, and the magnitude sum_k |x||w| + |bias|."""
    X, W = X.double(), W.double()
    y, mag = X @ W.T, X.abs() @ W.abs().T
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    return y, mag


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def chanmix_ref(x, W, bias=None, resid=None, ln_g=None, ln_b=None, act=0, eps=1e-5):
    """y[b, o, l] = LN_o(sum_i W[o, i] act(x[b, i, l]) + bias[o] + resid[b, o, l]); exact-erf GELU when act = 1; LayerNorm over channels."""
    x = x.double()
    if act == 1:
        x = gelu_erf(x)
    z = torch.einsum("oi,bil->bol", W.double(), x)
    if bias is not None:
        z = z + bias.double()[None, :, None]
    if resid is not None:
        z = z + resid.double()
    if ln_g is not None:
        m = z.mean(1, keepdim=True)
        v = ((z - m) ** 2).mean(1, keepdim=True)
        z = (z - m) / torch.sqrt(v + eps) * ln_g.double()[None, :, None] + ln_b.double()[None, :, None]
    return z


def pyramid_pool_ref(x, sizes):
    """nn.AdaptiveAvgPool1d's bins (start = floor(j L / s), end = ceil((j + 1) L / s)) for every size, concatenated; float64."""
    x = x.double()
    L = x.shape[-1]
    cols = []
    for s in sizes:
        for j in range(s):
            st, en = (j * L) // s, -((-(j + 1) * L) // s)
            cols.append(x[..., st:en].mean(-1))
    return torch.stack(cols, -1)


def layernorm_relu_ref(x, g, b, eps=1e-5):
    x = x.double()
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return torch.relu((x - m) / torch.sqrt(v + eps) * g.double() + b.double())


def s4_fft_conv(u, K, D):
    """y[b, h, l] = sum_{j <= l} K[h, j] u[b, h, l - j] + D[h] u[b, h, l] by a zero-padded float64 FFT (u [B, H, L], K [H, L], numpy)."""
    u, K = np.asarray(u, np.float64), np.asarray(K, np.float64)
    L = u.shape[-1]
    y = np.fft.irfft(np.fft.rfft(u, 2 * L, axis=-1) * np.fft.rfft(K, 2 * L, axis=-1)[None], 2 * L, axis=-1)[..., :L]
    return y + np.asarray(D, np.float64)[None, :, None] * u


def stable_topk_mask(imp, keep_k):
    """[B, C] bool: the keep_k largest importances of every batch element, ties to the lower channel index (a stable descending sort)."""
    B, C = imp.shape
    keep = torch.zeros(B, C, dtype=torch.bool)
    for b in range(B):
        v = imp[b].detach().cpu().double().numpy()
        order = np.argsort(-v, kind="stable")
        keep[b, torch.from_numpy(order[:keep_k].copy())] = True
    return keep.to(imp.device)


def duan_params(d):
    """oracle.cs3.DUAN state dict -> the [out, in] matrices lx_duan_fwd takes."""
    return {k: (v.detach().reshape(v.shape[0], -1) if v.dim() == 3 else v.detach()).contiguous() for k, v in d.state_dict().items()}


def duan_gate_ref(c, p):
    """hid = relu(W1 c + b1) [B, Hd, L], its magnitude, and z = W2 hid + b2 [B, C, L] with its magnitude; float64."""
    h, hmag = chan_gemm_ref(c, p["gate.0.weight"], p["gate.0.bias"])
    hid = torch.relu(h)
    z, zmag = chan_gemm_ref(hid, p["gate.2.weight"], p["gate.2.bias"])
    return hid, hmag, z, zmag


def duan_coef_ref(mean, var, gmean, cmean, p, eps):
    """(A, Bc) of y = A x + Bc per (b, c) from the row statistics, the gate's mean over L and the condition's mean over L; float64.
    The layer statistics combine the rows exactly: mu_l = mean_c mean, var_l = mean_c (var + (mean - mu_l)^2)."""
    mean, var, gmean, cmean = mean.double(), var.double(), gmean.double(), cmean.double()
    C = mean.shape[1]
    mu_l = mean.mean(1, keepdim=True)
    var_l = (var + (mean - mu_l) ** 2).mean(1, keepdim=True)
    hid2 = torch.relu(cmean @ p["mlp.0.weight"].double().T + p["mlp.0.bias"].double())
    gb = hid2 @ p["mlp.2.weight"].double().T + p["mlp.2.bias"].double()
    gam, bet = gb[:, :C], gb[:, C:]
    mu = gmean * mean + (1 - gmean) * mu_l
    sig = gmean * torch.sqrt(var + eps) + (1 - gmean) * torch.sqrt(var_l + eps)
    A = (1 + gam) / sig
    return A, bet - A * mu


def duan_ref_stages(x, c, p, keep_k, eps=1e-3):
    """The DUAN in float64, split at the places lx_duan_fwd leaves intermediate results: every value of the dict is what one launch writes."""
    x, c = x.double(), c.double()
    L = x.shape[2]
    st = {"mean": x.mean(2), "cmean": c.mean(2)}
    st["var"] = ((x - st["mean"][:, :, None]) ** 2).mean(2)
    st["hid"], st["hid_mag"], st["z"], st["z_mag"] = duan_gate_ref(c, p)
    st["gpart"] = tile_sums(torch.sigmoid(st["z"]))
    st["cpart"] = tile_sums(c)
    st["gmean"] = st["gpart"].sum(1) / L
    st["A"], st["Bc"] = duan_coef_ref(st["mean"], st["var"], st["gmean"], st["cmean"], p, eps)
    st["y_full"] = st["A"][:, :, None] * x + st["Bc"][:, :, None]
    st["imp"] = st["y_full"].abs().mean(2)
    st["keep"] = stable_topk_mask(st["imp"], keep_k)
    st["y"] = st["y_full"] * st["keep"][:, :, None]
    return st


def kept_set_margin(imp, keep_k, delta):
    """[B, C] bool: channels whose float64 importance lies within delta (relative) of the boundary between ranks keep_k - 1 and keep_k
    (the mean of the two importances there). Either outcome is acceptable for them; nothing is undecided when keep_k == C."""
    B, C = imp.shape
    if keep_k >= C:
        return torch.zeros(B, C, dtype=torch.bool, device=imp.device)
    s = imp.double().sort(1, descending=True).values
    edge = 0.5 * (s[:, keep_k - 1] + s[:, keep_k])[:, None]
    return (imp.double() - edge).abs() <= delta * edge


def duan_case(C, Hd, B, L, seed, x_offset=0.0):
    """A seeded oracle.cs3.DUAN(C, Hd) with non-trivial biases, and its inputs x, c [B, C, L] (fp32, CPU)."""
    from oracle import cs3
    torch.manual_seed(seed)
    d = cs3.DUAN(C, hidden_dim=Hd).eval()
    g = torch.Generator().manual_seed(seed + 1000)
    x = torch.randn(B, C, L, generator=g) * (0.5 + torch.rand(1, C, 1, generator=g)) + x_offset + 0.3 * torch.randn(1, C, 1, generator=g)
    c = torch.randn(B, C, L, generator=g)
    return d, x, c


# (C, L, seed, keep_k) of the full-size kept-set check: seeds for which the float64 reference itself leaves at most 1 % of the channels of
# every batch element within 2e-5 of the rank boundary (tests/test_cs3_ref_cpu.py verifies that on the CPU)
DUAN_KEPT_CASES = [(512, 4096, 1, 358), (512, 4096, 7, 358)]
DUAN_KEPT_DELTA = 2e-5     # the DUAN's y bound: importance is a mean of |y|


def duan_tie_case(seed=3):
    """Ties across the top-k boundary: gate.2.weight = mlp.2.weight = 0 and channel-constant biases make g, gamma, beta the same for every
    channel, and the 16 rows of x are 4 distinct rows repeated 4 times (channel i is row i % 4): channels i, i + 4, i + 8, i + 12 have
    equal importance, and keep_k = 6 cuts through the second group, of which the two LOWEST channel indices must survive."""
    C, Hd, B, L, keep_k = 16, 64, 3, 256, 6
    d, x, c = duan_case(C, Hd, B, L, seed)
    with torch.no_grad():
        d.gate[2].weight.zero_()
        d.mlp[2].weight.zero_()
        d.gate[2].bias.fill_(0.3)
        d.mlp[2].bias[:C].fill_(0.2)
        d.mlp[2].bias[C:].fill_(0.1)
    scale = torch.tensor([1.0, 2.0, 0.5, 3.0]).view(1, 4, 1)
    x = (x[:, :4] * scale).repeat(1, 4, 1).contiguous()
    return d, x, c, keep_k


# ------------------------------------------------------------------------------------------------ precise attention, float64
# The reference of tests/test_precise_attn_tiles_gpu.py (tests/test_precise_attn_ref_cpu.py pins it to torch's own SDPA on the CPU).
VT_PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)     # slot j of every 16 holds key VT_PERM16[j] (an involution)


def seg_edges(lens):
    e = [0]
    for L in lens:
        e.append(e[-1] + L)
    return e


def seg_attn_ref(q, k, v, lens, bias, factor):
    """Joint attention over the concatenated segments in float64: softmax_k(factor * q.k + bias[query segment][key segment]) v, natural-log
    units, -inf masks a pair (a row masked from every key comes out NaN, as torch's softmax gives it). q, k, v [..., S, 128], S = sum(lens)."""
    e = seg_edges(lens)
    m = torch.zeros(e[-1], e[-1], dtype=torch.float64, device=q.device)
    for i in range(len(lens)):
        for j in range(len(lens)):
            m[e[i]:e[i + 1], e[j]:e[j + 1]] = float(bias[i][j])
    s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * factor + m
    return torch.matmul(torch.softmax(s, -1), v.double())


def vt_deinterleave(vt, lens, vt0):
    """V^T image [..., 128, Spad] (segment s at slots vt0[s] .., keys in the 16-key order [0-3, 8-11, 4-7, 12-15]) -> v [..., S, 128] in
    key order over the concatenated segments."""
    perm = torch.tensor(VT_PERM16)
    idx = torch.cat([p0 + (torch.arange(L) & ~15) + perm[torch.arange(L) & 15] for L, p0 in zip(lens, vt0)])
    return vt[..., idx.to(vt.device)].transpose(-1, -2)


def bf16_pair(x):
    """(hi, lo) = (bf16(x), bf16(x - hi)) of an fp32 tensor, as fp32: what the split producers write."""
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


NEAR_BOUND_TARGET = 90.0      # the constructed |score| in log2 units; lx.h's contract for LX_ATTN_BOUNDED is <= 100
NEAR_BOUND_LENS = (70, 200)
# (query segment, query position, key segment, key position, sign): the key of head 0 there is made parallel to that query; the keys sit
# in a first tile, at a 64-key tile's last key, in a ragged last tile and in the second segment
NEAR_BOUND_PAIRS = ((0, 3, 0, 63, 1.0), (0, 40, 1, 199, -1.0), (1, 5, 0, 69, -1.0), (1, 150, 1, 17, 1.0))


def near_bound_qkv(q_factor, seed=29):
    """fp32 [k | v | q] rows (B = 1, H = 2, segments NEAR_BOUND_LENS; q already carries q_factor = scale * log2 e) in which, for every
    entry of NEAR_BOUND_PAIRS, q.k of head 0 is sign * NEAR_BOUND_TARGET log2 units. Every other score stays far smaller: such a key is
    ~5.5x a random key's length, so the other queries see it at ~8 +- and at most ~35."""
    H, D = 2, 256
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(sum(NEAR_BOUND_LENS), 3 * D, generator=g)
    buf[:, 2 * D:] *= q_factor
    for sq, qp, sk, kp, sign in NEAR_BOUND_PAIRS:
        q = buf[seg_edges(NEAR_BOUND_LENS)[sq] + qp, 2 * D:2 * D + 128].double()
        buf[seg_edges(NEAR_BOUND_LENS)[sk] + kp, :128] = (sign * NEAR_BOUND_TARGET / float(q @ q) * q).float()
    return buf


def max_abs_score_log2(q, k, lens, bias):
    """max over all (query, key) pairs of |q.k + bias * log2 e| in float64 (q carries scale * log2 e); q, k [..., S, 128]. Pairs masked
    by -inf are skipped by the kernel and do not count."""
    e = seg_edges(lens)
    s = torch.matmul(q.double(), k.double().transpose(-1, -2))
    worst = 0.0
    for i in range(len(lens)):
        for j in range(len(lens)):
            if bias[i][j] != float("-inf"):
                worst = max(worst, float((s[..., e[i]:e[i + 1], e[j]:e[j + 1]] + bias[i][j] * 1.4426950408889634).abs().max()))
    return worst


# ------------------------------------------------------------------------------------------------ LX_EPI_QKV, float64
# The reference of tests/test_qkv_epilogue_tiles_gpu.py: what the q/k/v projection epilogue (csrc/gemm8.h gemm_epilogue_qkv, csrc/gemm4.h)
# makes of the fp32 sums, restated in float64 (tests/test_qkv_epilogue_ref_cpu.py pins it to oracle.flux_modules on the CPU).
U32 = 2.0 ** -23          # fp32 ulp at 1 (twice the unit roundoff: the error terms below are upper bounds)


def rmsnorm_heads_ref(y, w, Ey=None, eps=1e-6):
    """RMSNorm(128, w, eps) over every head of y [M, H * 128], float64. With Ey (a bound on the error of y as the kernel holds it) also a
    bound on the error of the result: the propagated Ey -- |r w| Ey on the element itself, and through r = rsqrt(mean y^2 + eps):
    |dr / r| <= sum_j |y_j| Ey_j / (128 (mean y^2 + eps)). (The fp32 roundings of the norm itself are added by qk_norm_rope_ref.)"""
    M = y.shape[0]
    x = y.double().view(M, -1, 128)
    ms = x.pow(2).mean(-1, keepdim=True) + eps
    out = x * torch.rsqrt(ms) * w.double()
    if Ey is None:
        return out.view(M, -1)
    Ey = Ey.double().view(M, -1, 128)
    E = (torch.rsqrt(ms) * w.double()).abs() * Ey + out.abs() * (x.abs() * Ey).sum(-1, keepdim=True) / (128.0 * ms)
    return out.view(M, -1), E.view(M, -1)


def rope_pairs_ref(x, cs, L, m_base=0):
    """Interleaved-pair RoPE of x [M, H * 128] (float64): row m is position (m_base + m) % L of its batch element, cs [L, 128] holds
    (cos, sin) of pair i at [2i, 2i + 1]. Returns (out, |x cos| + |x' sin|): the magnitude a rounding error of the rotation is relative to."""
    M = x.shape[0]
    x = x.double().view(M, -1, 64, 2)
    pos = (m_base + torch.arange(M, device=x.device)) % L
    c, s = cs.double()[pos, 0::2][:, None, :], cs.double()[pos, 1::2][:, None, :]          # [M, 1, 64]
    e, o = x[..., 0], x[..., 1]
    out = torch.stack([e * c - o * s, o * c + e * s], -1)
    mag = torch.stack([(e * c).abs() + (o * s).abs(), (o * c).abs() + (e * s).abs()], -1)
    return out.view(M, -1), mag.view(M, -1)


def qk_norm_rope_ref(y, w, cs, L, m_base=0, Ey=None):
    """k or q of LX_EPI_QKV in float64 from the projection y [M, H * 128] (rows m_base .. of a stream of L-row batch elements, row-major
    [B * L, D]). With Ey also E, the fp32 error bound of the kernel's expression, built as tests/test_rowops_gpu.py::qk_ref builds it --
    RMSNorm: 128 squares summed, rsqrtf and two products: relative <= 12 U32 on x r w; RoPE x c - x' s: two products and a difference,
    <= 4 U32 (|x c| + |x' s|) on top -- plus Ey carried through both steps."""
    if Ey is None:
        return rope_pairs_ref(rmsnorm_heads_ref(y, w), cs, L, m_base)[0]
    x, Ex = rmsnorm_heads_ref(y, w, Ey)
    out, mag = rope_pairs_ref(x, cs, L, m_base)
    Eo = rope_pairs_ref(Ex, cs, L, m_base)[1]                  # |c| Ex + |s| Ex': the magnitude of the rotation of the (non-negative) Ex
    return out, Eo + 16 * U32 * mag


def vt_slot_keys(n):
    """key held by slot j of a 16-bit V^T image, j in [0, n): the 16-key order [0-3, 8-11, 4-7, 12-15] (an involution)"""
    j = torch.arange(n)
    return (j & ~15) + torch.tensor(VT_PERM16)[j & 15]


def vt8_slot_keys(n):
    """key held by byte j of an e4m3 V^T image row, j in [0, n), n % 64 == 0: within a 64-key tile byte g * 32 + p holds key
    (p >> 4) * 32 + 8 ((p & 15) >> 2) + 4 g + (p & 3) (include/lx.h: the f8f6f4 MFMA's operand order)"""
    j = torch.arange(n)
    g, p = (j & 63) >> 5, j & 31
    return (j & ~63) + (p >> 4) * 32 + 8 * ((p & 15) >> 2) + 4 * g + (p & 3)


def vt_interleave(v, fp8=False):
    """v [..., L, 128] in key order -> the V^T image rows [..., 128, pad64(L)] (slots of keys that do not exist: zero)"""
    L = v.shape[-2]
    n = (L + 63) // 64 * 64
    keys = (vt8_slot_keys(n) if fp8 else vt_slot_keys(n)).to(v.device)
    out = torch.zeros(*v.shape[:-2], n, 128, dtype=v.dtype, device=v.device)
    ok = keys < L
    out[..., ok, :] = v[..., keys[ok], :]
    return out.transpose(-1, -2)


def vt_stream_deinterleave(vt, L, pos0, fp8=False):
    """One stream's slots [pos0, pos0 + pad64(L)) of a V^T image [..., 128, ld] -> (v [..., L, 128] in key order, written [pad64(L)] bool:
    the slots that hold a key that exists)."""
    n = (L + 63) // 64 * 64
    keys = vt8_slot_keys(n) if fp8 else vt_slot_keys(n)
    written = keys < L
    slot_of_key = torch.argsort(keys)[:L]                      # keys is a permutation of [0, n)
    return vt[..., (pos0 + slot_of_key).to(vt.device)].transpose(-1, -2), written


def mixed_plan_keep_rows(shapes, ncu):
    """The peel of the GEMM planner's mixed plan (csrc/gemm.hip, lx_gemm_bf16_ws): shapes = [(M, N)] in launch order. 256-row tile rows come
    off the ends of the problems, last problem first, until the rest fits whole rounds of ncu tiles; problem i keeps rows [0, keep[i]) on
    256-row tiles and its rows from m_base = keep[i] on go to the 128-row tail. None when the planner has no such candidate."""
    t256 = sum(-(-M // 256) * -(-N // 256) for M, N in shapes)
    full = t256 // ncu * ncu
    if full == 0 or t256 == full:
        return None
    remain, keep = t256, [M for M, _ in shapes]
    for i in range(len(shapes) - 1, -1, -1):
        tn = -(-shapes[i][1] // 256)
        while remain > full and keep[i] > 0:
            keep[i] -= keep[i] % 256 or 256
            remain -= tn
    return keep


# launch shapes of tests/test_qkv_epilogue_tiles_gpu.py (H = 2 heads, D = 256): rows per batch element and column counts
QKV_D = 256
QKV_DOUBLE = dict(L=(416, 96, 160), B=(None, 9, 5), N=(768, 768, 512), M3=300, N3=264)      # p0's batch count follows from the CU count
QKV_SINGLE = dict(L=160, N=3 * 256 + 520)


def qkv_double_shapes(ncu):
    """[(M, N)] of the double-block launch: NCU + tail tiles of 256 x 256, tail in [17, 24] and at most a sixth of a round (the three-way
    split form's limit), p0 = B0 batch elements of 416 rows. None when no B0 gives such a launch."""
    d = QKV_DOUBLE
    rest = [(d["B"][i] * d["L"][i], d["N"][i]) for i in (1, 2)] + [(d["M3"], d["N3"])]
    t_rest = sum(-(-M // 256) * -(-N // 256) for M, N in rest)
    for B0 in range(1, 4096):
        tail = 3 * -(-B0 * d["L"][0] // 256) + t_rest - ncu
        if 17 <= tail <= 24 and tail * 6 <= ncu:
            return [(B0 * d["L"][0], d["N"][0])] + rest
        if tail > 24:
            return None
    return None


def qkv_single_shape(ncu):
    """[(M, N)] of the single-block launch: one [k | v | q | mlp] problem of 160-row batch elements, sized like qkv_double_shapes"""
    d = QKV_SINGLE
    tn = -(-d["N"] // 256)
    for B in range(1, 4096):
        tail = tn * -(-B * d["L"] // 256) - ncu
        if 17 <= tail <= 24 and tail * 6 <= ncu:
            return [(B * d["L"], d["N"])]
        if tail > 24:
            return None
    return None


def qkv_epilogue_emulate_f32(A, W, bias, wk, wq, cs, L, D=QKV_D):
    """The whole epilogue in fp32 on the CPU, one operation at a time as the kernels write it (fp32 product sums, + bias, sum of squares,
    rsqrt, x r w, the rotation): (k, v, q) fp32 [M, D] before the single rounding. A, W hold bf16-representable values."""
    f = torch.float32
    y = A.to(f) @ W.to(f).T + bias.to(f)
    M = y.shape[0]
    pos = torch.arange(M) % L
    c, s = cs.to(f)[pos, 0::2][:, None, :], cs.to(f)[pos, 1::2][:, None, :]

    def nr(x, w):
        x = x.reshape(M, -1, 128)
        r = torch.rsqrt((x * x).sum(-1, keepdim=True) * (1.0 / 128.0) + 1e-6)
        x = (x * r * w.to(f)).view(M, -1, 64, 2)
        e, o = x[..., 0], x[..., 1]
        return torch.stack([e * c - o * s, o * c + e * s], -1).reshape(M, -1)
    return nr(y[:, :D], wk), y[:, D:2 * D].contiguous(), nr(y[:, 2 * D:3 * D], wq)
