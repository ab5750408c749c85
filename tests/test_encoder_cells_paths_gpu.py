"""Every kernel instantiation behind the first routing encoder layer and the recurrent cells' pointwise entry points
(csrc/gm_netmon.hip): gm_routing_node_encoder[_bits] (k_routing_enc<CPL, AC>, six instantiations in two LDS
classes), gm_lnlstm_fwd / gm_lnlstm_pointwise (k_lnlstm_pw<1|2|4|8>), gm_lnlstm_bwd (k_lnlstm_bwd<1|2|4|8>),
gm_gru_pointwise / gm_gru_bwd and gm_lstm_pointwise / gm_lstm_pointwise_bwd. Every case calls the C entry point,
asserts the kernel gm_last_kernel() names (gm_last_lnlstm_pw() for the LayerNorm-LSTM forward, which names its
kernel there and leaves gm_last_kernel as it found it), and compares with an fp64 CPU reference written from the operation's
definition (encoder_cells_util.py; no other kernel of the library takes part). Outputs are NaN-filled, strided
where the entry point takes a stride, and carry one guard row: the payload ends finite, the padding and the guard
row stay NaN.

Routing encoder. Synthetic rows in the documented layout (random valid neighbour table, random scalar features,
i.i.d. W), x with NaN padding; the reference is the dense fp64 product. Per-element bound 16 * 2^-24 * (|b| +
sum |w_k x_k|) for none / leaky_relu (RoutingCase.bound), for tanh / gelu that bound times sup |f'| plus
test_act_gpu's 2e-6 * max(1, max|ref| / 8). The sign words equal y > 0 of the returned y bit for bit and agree with
the reference's sign wherever that is beyond doubt (test_encoder_cells_ref.py: under 1e-5 of the elements are left
out). Contract: nbr holds three valid neighbours per node (the helpers assert it of every table used here, the
environment's included); y is 8-byte aligned.

LayerNorm-LSTM forward. h' and c' within the bounds test_cells_gpu.py holds the cell to (norm-wise relative 2e-6,
absolute 1e-5 / 2e-5) at every H, those above 256 included (none needed a measured bound). Saved statistics within
relative 1e-6: each 1 / sqrt(var + eps) against itself; each mean against the mean magnitude of what it sums (a mean
of mixed signs cancels, the rounding error of its fp32 sum scales with sum |x| / n, not with the result): mean|x| of
the gi and gh rows, mean(|sigma(f) c| + |sigma(i) tanh(g)|) of the cell row, whose entries are themselves sums of
two rounded products (at H = 1 a row with sigma(f) c = -0.1953, sigma(i) tanh(g) = 0.1938 has the mean -0.0015).
"""
import importlib
import math

import pytest
import torch

import encoder_cells_util as E
from test_cells_gpu import _ref_lnlstm

pytestmark = pytest.mark.gpu

L = importlib.import_module("graph-marl_amd._lib")
INVALID_ARG, UNSUPPORTED = -1, -5
NAN = float("nan")
FILL = 0x5A5A5A5A  # sign words before the call

# (N, G, n) -> the kernel's columns per lane and LDS class; <CPL,AC> is completed per activation class
RENC = {
    (4, 13, 128): "k_routing_enc<2,%s>",      # one partial 64-row group
    (10, 53, 256): "k_routing_enc<2,%s>",     # 512 rows / block, 2 row blocks, grid.y = 2
    (20, 27, 64): "k_routing_enc<1,%s>",      # n % 128 != 0
    (30, 35, 128): "k_routing_enc<2,%s>",     # K = 128: the last K with two columns per lane; 1024 rows / block
    (32, 33, 128): "k_routing_enc<1,%s>",     # K = 136
    (50, 21, 192): "k_routing_enc<1,%s>",     # grid.y = 3
    (64, 17, 64): "k_routing_enc<1,%s>/lds>64K",    # 66 KB: the first shape that raises the LDS limit
    (128, 9, 128): "k_routing_enc<1,%s>/lds>64K",   # the environment's largest N, 130 KB
}
AC_OF = {E.ACT_LEAKY: "1", E.ACT_NONE: "0", E.ACT_TANH: "-1", E.ACT_GELU: "-1"}
RENC_CASES = [(N, G, n, act) for (N, G, n) in RENC
              for act in (E.RENC_ACTS if N in E.RENC_ALL_ACTS else (E.ACT_LEAKY,))]
assert list(RENC) == E.RENC_SHAPES


def nan_rows(rows, ld, guard=1):
    return torch.full((rows + guard, ld), NAN, device="cuda")


def padded(x2d, ld, guard=0):
    """the rows of x2d (CPU) at the start of a NaN device buffer of row stride ld"""
    rows, w = x2d.shape
    buf = nan_rows(rows, ld, guard)
    buf[:rows, :w] = x2d.float().cuda()
    return buf


def check_guard(buf, rows, w, what=""):
    assert torch.isfinite(buf[:rows, :w]).all(), f"{what}: payload not finite"
    assert torch.isnan(buf[:rows, w:]).all() and torch.isnan(buf[rows:]).all(), f"{what}: padding or guard row written"


def vec(t):
    return t.detach().float().cuda().contiguous()


# ---------------------------------------------------------------------------------------------------------
# routing encoder
# ---------------------------------------------------------------------------------------------------------
class RencRun:
    """Device operands of one RoutingCase and one call of the entry point on fresh outputs."""

    def __init__(self, case):
        self.c = case
        K = 4 * case.N + 8
        self.M = case.G * case.N
        self.x = padded(case.x, K + 3)  # ldx > 4N + 8, NaN behind every row
        self.nbr = case.nbr.cuda().contiguous()
        self.wt = case.w.t().contiguous().cuda()
        self.b = case.b.cuda()
        self.W = case.n // 32

    def outputs(self):
        y = nan_rows(self.M, self.c.n + 2)
        sb = torch.full((self.M + 1, self.W + 1), FILL, dtype=torch.int32, device="cuda")  # ldsb > n / 32
        return y, sb

    def call(self, act, y, sb, bias=True, plain=False, over=()):
        c = self.c
        a = dict(x=self.x.data_ptr(), ldx=self.x.stride(0), nbr=self.nbr.data_ptr(), G=c.G, N=c.N,
                 wt=self.wt.data_ptr(), b=self.b.data_ptr() if bias else None, n=c.n, act=act, y=y.data_ptr(),
                 ldy=y.stride(0), sb=None if sb is None else sb.data_ptr(), ldsb=0 if sb is None else sb.stride(0))
        a.update(over)  # single arguments replaced (the refusal cases)
        head = (a["x"], a["ldx"], a["nbr"], a["G"], a["N"], a["wt"], a["b"], a["n"], a["act"], a["y"], a["ldy"])
        if plain:
            return L.lib().gm_routing_node_encoder(*head, L.stream_ptr())
        return L.lib().gm_routing_node_encoder_bits(*head, a["sb"], a["ldsb"], L.stream_ptr())

    def untouched(self, y, sb):
        torch.cuda.synchronize()
        return bool(torch.isnan(y).all()) and bool((sb == FILL).all())


def check_renc(run, case, act, y, sb, name):
    """y against the fp64 reference within the per-element tolerance; the guard; the sign words against the
    returned y (exact) and against the reference's sign where that is beyond doubt."""
    M, n, W = run.M, case.n, run.W
    assert L.last_kernel() == name
    torch.cuda.synchronize()
    check_guard(y, M, n, name)
    got = y[:M, :n].cpu().double()
    ref, tol = E.act_ref(case, act)
    ratio = ((got - ref).abs() / tol).max().item()
    print(f"{name} N={case.N} n={n} act={act}: max |y - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)
    if sb is not None:
        words = sb.cpu()
        assert torch.equal(words[:M, :W], E.pack_bits(got > 0)), f"{name}: sign words != (y > 0)"
        assert bool((words[:M, W:] == FILL).all()) and bool((words[M:] == FILL).all()), f"{name}: padding words"
        want, sure = E.sign_check(case, act)
        assert 1.0 - sure.double().mean().item() < 0.01
        assert bool(((got > 0) == want)[sure].all()), f"{name}: sign of y against the reference"


@pytest.mark.parametrize("N,G,n,act", RENC_CASES)
def test_routing_encoder_vs_fp64(N, G, n, act):
    case = E.routing_case(N, G, n)
    run = RencRun(case)
    y, sb = run.outputs()
    L.check(run.call(act, y, sb))
    check_renc(run, case, act, y, sb, RENC[(N, G, n)] % AC_OF[act])


@pytest.mark.parametrize("N,G,n", [(10, 53, 256), (20, 27, 64)])
def test_routing_encoder_null_bias_and_null_bits(N, G, n):
    """b = NULL is a zero bias (bit-equal to a vector of zeros, within the bound of the bias-free reference);
    gm_routing_node_encoder, _bits with sbits = NULL and _bits with sign words write the same y."""
    case = E.routing_case(N, G, n)
    run = RencRun(case)
    name = RENC[(N, G, n)] % "1"
    y0, sb0 = run.outputs()
    L.check(run.call(E.ACT_LEAKY, y0, sb0))
    assert L.last_kernel() == name
    for kw in (dict(plain=True), dict()):
        y1, _ = run.outputs()
        L.check(run.call(E.ACT_LEAKY, y1, None, **kw))
        assert L.last_kernel() == name
        torch.cuda.synchronize()
        check_guard(y1, run.M, n, name)
        assert torch.equal(y1[:run.M, :n], y0[:run.M, :n]), kw
    nob = case.without_bias()
    y2, sb2 = run.outputs()
    L.check(run.call(E.ACT_LEAKY, y2, sb2, bias=False))
    check_renc(run, nob, E.ACT_LEAKY, y2, sb2, name)
    y3, sb3 = run.outputs()
    zeros = torch.zeros(n, device="cuda")
    L.check(run.call(E.ACT_LEAKY, y3, sb3, over=dict(b=zeros.data_ptr())))
    torch.cuda.synchronize()
    assert torch.equal(y3[:run.M, :n], y2[:run.M, :n]) and torch.equal(sb3, sb2)


def test_routing_encoder_on_environment_rows():
    """Real env.node_obs at N = 20: the synthetic layout is the environment's (the rows rebuild from their own
    table and scalar columns exactly, the table meets the precondition), and the kernel meets the same bound."""
    gm = importlib.import_module("graph-marl_amd")
    N, B, A, n = 20, 27, 20, 64
    env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A, n_env=B, seed=5)
    env.reset()
    gen = torch.Generator().manual_seed(0)
    for _ in range(5):
        env.step_(torch.randint(0, 4, (B, A), generator=gen, dtype=torch.int32).cuda())
    x = env.node_obs.reshape(-1, 4 * N + 8).cpu()
    nbr = env.nbr.cpu().to(torch.int32).reshape(B, N, 3)
    E.check_table(nbr, N)
    assert torch.equal(E.node_rows(nbr, E.scalars_of(x, N)), x), "node_obs is not the documented layout"
    case = E.routing_case_from(nbr, x, n, gen)
    run = RencRun(case)
    y, sb = run.outputs()
    L.check(run.call(E.ACT_LEAKY, y, sb))
    check_renc(run, case, E.ACT_LEAKY, y, sb, "k_routing_enc<1,1>")


def test_routing_encoder_refusals():
    """Bad arguments are refused before any launch: nothing is written. A y that is not 8-byte aligned is refused
    (two columns per lane store float2); N = 160 needs more than the 160 KB of LDS."""
    case = E.routing_case(10, 53, 256)
    run = RencRun(case)
    K = 4 * case.N + 8
    y, sb = run.outputs()
    odd = nan_rows(run.M, case.n + 3)
    for what, kw, yb in (("n % 64", dict(n=96), y), ("odd ldy", dict(y=odd.data_ptr(), ldy=odd.stride(0)), odd),
                         ("ldx < 4N + 8", dict(ldx=K - 1), y), ("misaligned wt", dict(wt=run.wt.data_ptr() + 4), y),
                         ("ldsb < n / 32", dict(ldsb=case.n // 32 - 1), y),
                         ("misaligned y", dict(y=y.data_ptr() + 4), y), ("act", dict(act=19), y)):
        assert run.call(E.ACT_LEAKY, y, sb, over=kw) == INVALID_ARG, what
        assert b"gm_routing_node_encoder" in L.lib().gm_last_error(), what
        assert run.untouched(yb, sb), what
    # N = 160: K = 648, 162 KB at one column per lane (operands of the full size: nothing may be launched)
    N, G, n = 160, 1, 64
    gen = torch.Generator().manual_seed(1)
    nbr = E.neighbour_table(G, N, gen)
    run = RencRun(E.routing_case_from(nbr, E.node_rows(nbr, torch.rand(G * N, 8, generator=gen)), n, gen))
    y, sb = run.outputs()
    assert run.call(E.ACT_LEAKY, y, sb) == UNSUPPORTED
    assert b"LDS" in L.lib().gm_last_error()
    assert run.untouched(y, sb)


# ---------------------------------------------------------------------------------------------------------
# LayerNorm-LSTM forward and backward
# ---------------------------------------------------------------------------------------------------------
class LnOperands:
    """Device operands of one cell, every row operand on a stride of its own: gi, gh and c separately and as the
    [gi | gh] single buffer of gm_lnlstm_pointwise (ldg > 8H)."""

    def __init__(self, leaves, m, H):
        gi, gh, c = (t.detach() for t in leaves[:3])
        self.gi, self.gh, self.c = padded(gi, 4 * H + 1), padded(gh, 4 * H + 3), padded(c, H + 2)
        self.g = padded(torch.cat([gi, gh], 1), 8 * H + 3)
        self.ps = [vec(t) for t in leaves[3:]]
        self.pp = [p.data_ptr() for p in self.ps]


def ln_outputs(m, H):
    return nan_rows(m, H + 5), nan_rows(m, H + 4), nan_rows(m, 8)  # h', c', stats


@pytest.mark.parametrize("m", [1, 5, 70])
@pytest.mark.parametrize("H", list(E.LN_H))
def test_lnlstm_forward_vs_fp64(H, m):
    """gm_lnlstm_fwd and gm_lnlstm_pointwise against fp64 _ref_lnlstm: h' and c' within test_cells_gpu.py's bounds
    (norm-wise relative 2e-6, absolute 1e-5 / 2e-5), the six saved statistics per row within relative 1e-6 (module
    docstring), the same bits from both entry points."""
    leaves = E.lnlstm_leaves(m, H, 1000 * m + H)
    with torch.no_grad():
        rh, rc = _ref_lnlstm(*leaves)
    st_ref, mag = E.lnlstm_stats(leaves)
    op = LnOperands(leaves, m, H)
    name = f"k_lnlstm_pw<{E.LN_H[H]}>"
    h1, c1, st = ln_outputs(m, H)
    before = L.last_kernel()
    L.check(L.lib().gm_lnlstm_fwd(op.gi.data_ptr(), op.gi.stride(0), op.gh.data_ptr(), op.gh.stride(0),
                                  op.c.data_ptr(), op.c.stride(0), *op.pp, m, H, 1e-5, h1.data_ptr(), h1.stride(0),
                                  c1.data_ptr(), c1.stride(0), st.data_ptr(), L.stream_ptr()))
    assert L.last_lnlstm_pw() == name and L.last_kernel() == before
    h2, c2, _ = ln_outputs(m, H)
    L.check(L.lib().gm_lnlstm_pointwise(op.g.data_ptr(), op.g.stride(0), op.c.data_ptr(), op.c.stride(0), *op.pp, m,
                                        H, 1e-5, h2.data_ptr(), h2.stride(0), c2.data_ptr(), c2.stride(0),
                                        L.stream_ptr()))
    assert L.last_lnlstm_pw() == name and L.last_kernel() == before
    torch.cuda.synchronize()
    for hh, cc, who in ((h1, c1, "fwd"), (h2, c2, "pointwise")):
        check_guard(hh, m, H, who), check_guard(cc, m, H, who)
        gh_, gc_ = hh[:m, :H].cpu(), cc[:m, :H].cpu()
        errs = (E.rel(gh_, rh), E.rel(gc_, rc), (gh_.double() - rh).abs().max().item(),
                (gc_.double() - rc).abs().max().item())
        print(f"{name} {who} H={H} m={m}: rel h' {errs[0]:.2e} c' {errs[1]:.2e}, abs h' {errs[2]:.2e} c' {errs[3]:.2e}")
        assert errs[0] < 2e-6 and errs[1] < 2e-6 and errs[2] < 1e-5 and errs[3] < 2e-5, (who, errs)
    assert torch.equal(h1[:m, :H], h2[:m, :H]) and torch.equal(c1[:m, :H], c2[:m, :H])
    check_guard(st, m, 6, "stats")
    got = st[:m, :6].cpu().double()
    scale = st_ref.abs().clone()
    scale[:, 0::2] = mag  # the means against the mean magnitude of what they sum
    ratio = ((got - st_ref).abs() / scale).max().item()
    print(f"{name} H={H} m={m}: max stats error / scale = {ratio:.2e}")
    assert ratio < 1e-6


@pytest.mark.parametrize("rpw", [1, 8])
@pytest.mark.parametrize("H", list(E.LN_H))
def test_lnlstm_bwd_vs_fp64_autograd(H, rpw):
    """gm_lnlstm_bwd on 70 rows (a partial last wave at 8 rows per wave, a partial last block at both): dgi, dgh,
    dc and the summed parameter partials against fp64 autograd of _ref_lnlstm within norm-wise relative 1e-5 (the
    bound of test_lnlstm_cell_fwd_bwd); the statistics it reads are the fp64 ones rounded to fp32.

    H = 1: LayerNorm over one unit is the constant ln_cell_b, so dc and d ln_cell_w are identically zero. The
    reference states that (fp64 autograd leaves 1e-13 of its own rounding there, times 1 / sqrt(eps) = 316), and the
    kernel has to return exact zeros."""
    m = 70
    assert m % 8 and -(-m // rpw) % 4
    leaves = E.lnlstm_leaves(m, H, 77 * H + rpw)
    gen = torch.Generator().manual_seed(H)
    dh, dc = torch.randn(m, H, generator=gen), torch.randn(m, H, generator=gen)
    rh, rc = _ref_lnlstm(*leaves)
    want = list(torch.autograd.grad([rh, rc], leaves, [dh.double(), dc.double()]))
    if H == 1:
        assert want[2].abs().max() < 1e-10 and want[8].abs().max() < 1e-10
        want[2], want[8] = torch.zeros_like(want[2]), torch.zeros_like(want[8])
    st = torch.zeros(m, 8)
    st[:, :6] = E.lnlstm_stats(leaves)[0].float()
    op = LnOperands(leaves, m, H)
    st_d, dh_d, dc_d = st.cuda(), padded(dh, H + 1), padded(dc, H + 7)
    nw = -(-m // rpw)
    dgi, dgh, dco = nan_rows(m, 4 * H + 2), nan_rows(m, 4 * H + 6), nan_rows(m, H + 3)
    part = nan_rows(nw, 14 * H)
    L.check(L.lib().gm_lnlstm_bwd(op.gi.data_ptr(), op.gi.stride(0), op.gh.data_ptr(), op.gh.stride(0),
                                  op.c.data_ptr(), op.c.stride(0), *op.pp, st_d.data_ptr(), dh_d.data_ptr(),
                                  dh_d.stride(0), dc_d.data_ptr(), dc_d.stride(0), m, H, rpw, dgi.data_ptr(),
                                  dgi.stride(0), dgh.data_ptr(), dgh.stride(0), dco.data_ptr(), dco.stride(0),
                                  part.data_ptr(), L.stream_ptr()))
    name = f"k_lnlstm_bwd<{E.LN_H[H]}>"
    assert L.last_kernel() == name
    torch.cuda.synchronize()
    H4 = 4 * H
    check_guard(dgi, m, H4, "dgi"), check_guard(dgh, m, H4, "dgh"), check_guard(dco, m, H, "dc")
    check_guard(part, nw, 14 * H, "part")
    ps = part[:nw].cpu().double().sum(0)
    errs = {"dgi": E.rel(dgi[:m, :H4].cpu(), want[0]), "dgh": E.rel(dgh[:m, :H4].cpu(), want[1]),
            "dc": E.rel(dco[:m, :H].cpu(), want[2])}
    for nm, got, ref in (("ln_in_w", ps[:H4], want[3]), ("ln_hid_w", ps[H4:2 * H4], want[5]),
                         ("bias", ps[2 * H4:3 * H4], want[7]), ("ln_in_b", ps[2 * H4:3 * H4], want[4]),
                         ("ln_hid_b", ps[2 * H4:3 * H4], want[6]), ("ln_cell_w", ps[3 * H4:3 * H4 + H], want[8]),
                         ("ln_cell_b", ps[3 * H4 + H:], want[9])):
        errs[nm] = E.rel(got, ref)
    print(f"{name} H={H} rpw={rpw}: rel err vs fp64", {k: f"{v:.1e}" for k, v in errs.items()})
    for nm, e in errs.items():
        assert e < 1e-5, (nm, e)


@pytest.mark.parametrize("H", [544, 1024])
def test_lnlstm_entry_points_reject_wide_hidden(H):
    """H > 512 has no instantiation: gm_lnlstm_fwd, gm_lnlstm_pointwise and gm_lnlstm_bwd refuse it through
    gm_fail and launch nothing."""
    m = 4
    g = torch.randn(m, 8 * H, device="cuda")
    c = torch.randn(m, H, device="cuda")
    pp = [torch.ones(k, device="cuda") for k in (4 * H,) * 5 + (H, H)]
    ptr = [p.data_ptr() for p in pp]
    out = torch.full((5, m, 4 * H), NAN, device="cuda")
    st = torch.ones(m, 8, device="cuda")
    lib = L.lib()
    rc = lib.gm_lnlstm_fwd(g.data_ptr(), 8 * H, g.data_ptr() + 16 * H, 8 * H, c.data_ptr(), H, *ptr, m, H, 1e-5,
                           out[0].data_ptr(), H, out[1].data_ptr(), H, out[2].data_ptr(), L.stream_ptr())
    assert rc == INVALID_ARG and b"gm_lnlstm_fwd" in lib.gm_last_error()
    rc = lib.gm_lnlstm_pointwise(g.data_ptr(), 8 * H, c.data_ptr(), H, *ptr, m, H, 1e-5, out[0].data_ptr(), H,
                                 out[1].data_ptr(), H, L.stream_ptr())
    assert rc == INVALID_ARG and b"gm_lnlstm_pointwise" in lib.gm_last_error()
    rc = lib.gm_lnlstm_bwd(g.data_ptr(), 8 * H, g.data_ptr() + 16 * H, 8 * H, c.data_ptr(), H, *ptr, st.data_ptr(),
                           c.data_ptr(), H, c.data_ptr(), H, m, H, 8, out[0].data_ptr(), 4 * H, out[1].data_ptr(),
                           4 * H, out[2].data_ptr(), H, out[3].data_ptr(), L.stream_ptr())
    assert rc == INVALID_ARG and b"gm_lnlstm_bwd" in lib.gm_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------
# GRU and plain LSTM pointwise
# ---------------------------------------------------------------------------------------------------------
CELL_SHAPES = [(1, 1), (5, 33), (70, 64), (9, 320)]


@pytest.mark.parametrize("m,H", CELL_SHAPES)
def test_gru_pointwise_and_bwd_vs_fp64(m, H):
    """gm_gru_pointwise / gm_gru_bwd against the fp64 torch.nn.GRUCell formula and its autograd, every stride
    different: absolute 1e-6 forward, norm-wise relative 1e-6 backward (test_gru_cell_fwd_bwd's bounds)."""
    gen = torch.Generator().manual_seed(100 * m + H)
    a, b, h = (torch.randn(m, k, generator=gen).double().requires_grad_() for k in (3 * H, 3 * H, H))
    g = torch.randn(m, H, generator=gen)
    r = torch.sigmoid(a[:, :H] + b[:, :H])
    z = torch.sigmoid(a[:, H:2 * H] + b[:, H:2 * H])
    nn_ = torch.tanh(a[:, 2 * H:] + r * b[:, 2 * H:])
    ref = (1 - z) * nn_ + z * h
    want = torch.autograd.grad(ref, (a, b, h), g.double())
    gi, gh, hh = padded(a.detach(), 3 * H + 1), padded(b.detach(), 3 * H + 2), padded(h.detach(), H + 3)
    h1 = nan_rows(m, H + 4)
    L.check(L.lib().gm_gru_pointwise(gi.data_ptr(), gi.stride(0), gh.data_ptr(), gh.stride(0), hh.data_ptr(),
                                     hh.stride(0), m, H, h1.data_ptr(), h1.stride(0), L.stream_ptr()))
    assert L.last_kernel() == "k_gru_pw"
    torch.cuda.synchronize()
    check_guard(h1, m, H, "h'")
    err = (h1[:m, :H].cpu().double() - ref.detach()).abs().max().item()
    print(f"k_gru_pw m={m} H={H}: max abs err {err:.2e}")
    assert err < 1e-6
    dy = padded(g, H + 5)
    dgi, dgh, dh = nan_rows(m, 3 * H + 6), nan_rows(m, 3 * H + 7), nan_rows(m, H + 8)
    L.check(L.lib().gm_gru_bwd(gi.data_ptr(), gi.stride(0), gh.data_ptr(), gh.stride(0), hh.data_ptr(), hh.stride(0),
                               dy.data_ptr(), dy.stride(0), m, H, dgi.data_ptr(), dgi.stride(0), dgh.data_ptr(),
                               dgh.stride(0), dh.data_ptr(), dh.stride(0), L.stream_ptr()))
    assert L.last_kernel() == "k_gru_bwd"
    torch.cuda.synchronize()
    for nm, buf, w, ref_g in (("dgi", dgi, 3 * H, want[0]), ("dgh", dgh, 3 * H, want[1]), ("dh", dh, H, want[2])):
        check_guard(buf, m, w, nm)
        e = E.rel(buf[:m, :w].cpu(), ref_g)
        print(f"k_gru_bwd m={m} H={H} {nm}: rel err {e:.2e}")
        assert e < 1e-6, (nm, e)


@pytest.mark.parametrize("m,H", CELL_SHAPES)
def test_lstm_pointwise_and_bwd_vs_fp64(m, H):
    """gm_lstm_pointwise / gm_lstm_pointwise_bwd (contiguous rows, one guard row) against the fp64 nn.LSTMCell gate
    formula and its autograd within absolute 1e-5 (test_lstm_pointwise_fwd_bwd's bound). The backward reads the
    fp64 activations and c' rounded to fp32. It publishes max |dgates| as the operand scale gm_absmax_finish makes
    of it, 2^(14 - e) with the max in [2^(e-1), 2^e): that must be the scale of the returned buffer's max exactly."""
    gen = torch.Generator().manual_seed(10 * m + H)
    gates = torch.randn(m, 4 * H, generator=gen).double().requires_grad_()
    c = torch.randn(m, H, generator=gen).double().requires_grad_()
    i, f, gg, o = gates.chunk(4, 1)
    acts = (torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o))
    rc = acts[1] * c + acts[0] * acts[2]
    rh = acts[3] * torch.tanh(rc)
    ga, gb = torch.randn(m, H, generator=gen), torch.randn(m, H, generator=gen)
    want = torch.autograd.grad([rh, rc], (gates, c), [ga.double(), gb.double()])
    gd, cd = vec(gates), vec(c)
    h1, c1, act = nan_rows(m, H), nan_rows(m, H), nan_rows(m, 4 * H)
    L.check(L.lib().gm_lstm_pointwise(gd.data_ptr(), cd.data_ptr(), m, H, h1.data_ptr(), c1.data_ptr(),
                                      act.data_ptr(), L.stream_ptr()))
    assert L.last_kernel() == "k_lstm_pw"
    h2, c2 = nan_rows(m, H), nan_rows(m, H)
    L.check(L.lib().gm_lstm_pointwise(gd.data_ptr(), cd.data_ptr(), m, H, h2.data_ptr(), c2.data_ptr(), None,
                                      L.stream_ptr()))
    torch.cuda.synchronize()
    ref_act = torch.cat(acts, 1).detach()
    for nm, buf, w, ref in (("h'", h1, H, rh), ("c'", c1, H, rc), ("act", act, 4 * H, ref_act)):
        check_guard(buf, m, w, nm)
        e = (buf[:m].cpu().double() - ref.detach()).abs().max().item()
        print(f"k_lstm_pw m={m} H={H} {nm}: max abs err {e:.2e}")
        assert e < 1e-5, (nm, e)
    assert torch.equal(h2[:m], h1[:m]) and torch.equal(c2[:m], c1[:m]) and torch.isnan(h2[m:]).all()
    dg, dc = nan_rows(m, 4 * H), nan_rows(m, H)
    sc = torch.full((2,), NAN, device="cuda")
    ins = [vec(t) for t in (ga, gb, ref_act, c, rc)]
    L.check(L.lib().gm_lstm_pointwise_bwd(*(t.data_ptr() for t in ins), m, H, dg.data_ptr(), dc.data_ptr(),
                                          sc.data_ptr(), L.stream_ptr()))
    assert L.last_kernel() == "k_lstm_pw_bwd"
    torch.cuda.synchronize()
    for nm, buf, w, ref in (("dgates", dg, 4 * H, want[0]), ("dc", dc, H, want[1])):
        check_guard(buf, m, w, nm)
        e = (buf[:m].cpu().double() - ref).abs().max().item()
        print(f"k_lstm_pw_bwd m={m} H={H} {nm}: max abs err {e:.2e}")
        assert e < 1e-5, (nm, e)
    mx = dg[:m].abs().max().item()
    assert mx > 0
    assert sc[0].item() == 2.0 ** (14 - math.frexp(mx)[1]) and math.isnan(sc[1].item())
