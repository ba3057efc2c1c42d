"""lx_ln_modulate_delta (csrc/rowops.hip), the step cache's probe, against float64: m = LN(x) * (1 + scale) + shift in fp32 replaces P, and
the sums of |m - P| and |P| over P as found come back per row (fp32) and in total (double).

D in {256, 3072} x (batches, rows per batch) in {(1, 3), (2, 5), (2, 67)}: fewer rows than a workgroup's four, a batch boundary inside a
workgroup, 134 rows = 33 workgroups and a ragged last one (and three 64-row rounds of the one-wave total). ldx, ldp and mod_ld are larger
than D, every third row sits at 1e3 + N(0, 1).

The bounds. E is tests/test_rowops_gpu.py's LnCase.ln_ref bound on the fp32 evaluation of m, restated here. A lane adds D / 64 terms in
sequence, the wave tree adds 6 levels, |m - P| costs one rounding more: with U32 = 2^-23 (two unit roundoffs)
    |S1 - S1_64| <= sum E + (D / 64 + 7) U32 sum |m - P|        |S2 - S2_64| <= (D / 64 + 6) U32 sum |P|
for every row and, the double additions being 2^-29 of that, for the totals.
Worst measured share of a bound on an MI355X (run with -s to print them): P 0.455 of E (D = 3072, 134 rows); a row's S1 0.030 and S2 0.102
(D = 256, 134 rows); the totals S1 below 0.001 and S2 0.010."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 2                              # sentinel rows above and below P and row_sums
U32 = 2.0 ** -23
SENT = 0x7FC0BEEF                    # a NaN pattern: nothing that reads it stays finite
EPS = 1e-6

SHAPES = [(1, 3), (2, 5), (2, 67)]


def randn(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


def bits(t):
    return t.contiguous().view(torch.int32)


class Case:
    def __init__(self, D, B, rpb):
        self.D, self.B, self.rpb, self.M = D, B, rpb, B * rpb
        M = self.M
        self.ldx, self.ldp, self.mod_ld = D + 8, D + 12, 6 * D + 8
        self.X = randn(M, self.ldx, seed=D + B + rpb, scale=2.0) + 0.3
        off = torch.arange(M, device=DEV) % 3 == 1
        self.X[off] = 1e3 + randn(int(off.sum()), self.ldx, seed=D + 1)
        self.tab = randn(B, self.mod_ld, seed=D + 2, scale=0.5)
        self.shift, self.scale = self.tab[:, 4:], self.tab[:, 3 * D + 4:]          # (16-byte aligned column offsets)
        self.P0 = randn(M, D, seed=D + 3, scale=1.5)
        # float64 reference
        b_of = torch.arange(M, device=DEV) // rpb
        x = self.X[:, :D].double()
        sh, sc = self.shift[b_of, :D].double(), self.scale[b_of, :D].double()
        eps = float(torch.tensor(EPS, dtype=torch.float32))
        mean = x.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
        t = (x - mean) * rstd * (1.0 + sc)
        self.m = t + sh
        c = D / 256 + 9                                                            # LnCase.ln_ref's E, restated
        self.E = t.abs() * (c / 2 + 6) * U32 + rstd * (1.0 + sc).abs() * c * U32 * x.abs().mean(1, keepdim=True) + U32 * (t.abs() + sh.abs())

    def buffers(self, P_rows=None):
        P = torch.empty(self.M + 2 * PAD, self.ldp, dtype=torch.float32, device=DEV)
        bits(P).fill_(SENT)
        P[PAD:PAD + self.M, :self.D] = self.P0 if P_rows is None else P_rows
        rs = torch.empty(self.M + 2 * PAD, 2, dtype=torch.float32, device=DEV)
        bits(rs).fill_(SENT)
        sums = torch.full((4,), -7.0, dtype=torch.float64, device=DEV)
        return P, rs, sums

    def launch(self, P, rs, sums):
        from loongx_amd import ops
        ops.ln_modulate_delta(self.X[:, :self.D], self.shift, self.scale, P[PAD:PAD + self.M, :self.D], self.rpb, rs[PAD:PAD + self.M],
                              sums[1:3], eps=EPS, mod_ld=self.mod_ld)
        torch.cuda.synchronize()


@pytest.fixture(scope="module", params=[(D, B, rpb) for D in (256, 3072) for B, rpb in SHAPES], ids=lambda p: "D%d-B%d-rpb%d" % p)
def case(request):
    c = Case(*request.param)
    c.X_before = c.X.clone()
    c.out = c.buffers()
    c.launch(*c.out)
    return c


def test_p_is_m_within_the_layernorm_bound(case):
    c = case
    P = c.out[0][PAD:PAD + c.M, :c.D].double()
    share = float(((P - c.m).abs() / c.E).max())
    print(f"\nD={c.D} M={c.M}: worst |P - m| / E = {share:.3f}")
    assert bool(torch.isfinite(P).all()) and share <= 1.0


def test_sums_against_float64(case):
    c = case
    P, rs, sums = c.out
    d64, p64 = (c.m - c.P0.double()).abs(), c.P0.double().abs()
    b1 = c.E.sum(1) + (c.D / 64 + 7) * U32 * d64.sum(1)
    b2 = (c.D / 64 + 6) * U32 * p64.sum(1)
    rows = rs[PAD:PAD + c.M].double()
    r1, r2 = (rows[:, 0] - d64.sum(1)).abs() / b1, (rows[:, 1] - p64.sum(1)).abs() / b2
    s1, s2 = float(sums[1]), float(sums[2])
    t1, t2 = abs(s1 - float(d64.sum())) / float(b1.sum()), abs(s2 - float(p64.sum())) / float(b2.sum())
    print(f"\nD={c.D} M={c.M}: worst share of the bound: rows S1 {float(r1.max()):.3f} S2 {float(r2.max()):.3f}; totals S1 {t1:.3f} S2 {t2:.3f}")
    assert float(r1.max()) <= 1.0 and float(r2.max()) <= 1.0
    assert t1 <= 1.0 and t2 <= 1.0
    # the totals ARE the row pairs added in row order, in double
    a = b = 0.0
    for v1, v2 in rs[PAD:PAD + c.M].tolist():
        a, b = a + v1, b + v2
    assert (s1, s2) == (a, b)


def test_nothing_else_is_written(case):
    c = case
    P, rs, sums = c.out
    assert torch.equal(bits(c.X), bits(c.X_before)), "X was written"
    assert bool((bits(P[:PAD]) == SENT).all()) and bool((bits(P[PAD + c.M:]) == SENT).all()), "sentinel rows of P"
    assert bool((bits(P[PAD:PAD + c.M, c.D:]) == SENT).all()), "pad columns of P"
    assert bool((bits(rs[:PAD]) == SENT).all()) and bool((bits(rs[PAD + c.M:]) == SENT).all()), "sentinel rows of row_sums"
    assert float(sums[0]) == -7.0 and float(sums[3]) == -7.0, "around sums"


def test_two_launches_agree_bit_for_bit(case):
    c = case
    again = c.buffers()
    c.launch(*again)
    for a, b, what in zip(c.out, again, ("P", "row_sums", "sums")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def test_p_equal_to_m_gives_a_zero_distance(case):
    c = case
    m = c.out[0][PAD:PAD + c.M, :c.D].clone()
    P, rs, sums = c.buffers(P_rows=m)
    c.launch(P, rs, sums)
    assert float(sums[1]) == 0.0 and bool((rs[PAD:PAD + c.M, 0] == 0.0).all())
    assert torch.equal(bits(P[PAD:PAD + c.M, :c.D]), bits(m))
    assert float(sums[2]) > 0.0
