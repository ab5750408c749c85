"""CPU-side helpers of test_encoder_cells_paths_gpu.py (plain torch, no device, no library call): synthetic routing
node-observation rows in the documented layout, the fp64 reference of the first encoder layer with its per-element
rounding bound, sign-bit packing, and fp64 leaves / LayerNorm statistics of the LayerNorm-LSTM cell.
test_encoder_cells_ref.py checks these helpers on the CPU."""
import dataclasses
import functools

import torch
import torch.nn.functional as F

U = 2.0 ** -24  # unit roundoff of fp32
ACT_NONE, ACT_LEAKY, ACT_TANH, ACT_GELU = 0, 1, 4, 14  # GM_ACT_* (include/graph_marl_amd.h)
ACT_FN = {ACT_NONE: lambda z: z, ACT_LEAKY: lambda z: F.leaky_relu(z, 0.01), ACT_TANH: torch.tanh, ACT_GELU: F.gelu}
# sup |f'| of the run-time codes: what an error of the pre-activation can grow to in the output
ACT_LIP = {ACT_TANH: 1.0, ACT_GELU: 1.13}

# (N, G, n): the dispatcher's rules for columns per lane, rows per block and the LDS class, each at the smallest
# G * N that crosses a block boundary (test_encoder_cells_paths_gpu.RENC holds the kernel name of each)
RENC_SHAPES = [(4, 13, 128), (10, 53, 256), (20, 27, 64), (30, 35, 128), (32, 33, 128), (50, 21, 192), (64, 17, 64),
               (128, 9, 128)]
RENC_ALL_ACTS = (10, 20, 64)  # the N whose shapes run every activation class
RENC_ACTS = (ACT_LEAKY, ACT_NONE, ACT_TANH, ACT_GELU)


# ---------------------------------------------------------------------------------------------------------
# routing node observations
# ---------------------------------------------------------------------------------------------------------
def check_table(nbr, N):
    """The precondition of gm_routing_node_encoder: degree 3, every entry a node id in [0, N), the three of a
    node distinct (no -1: the kernel does not mask a missing neighbour)."""
    assert nbr.dim() == 3 and nbr.shape[1] == N and nbr.shape[2] == 3, nbr.shape
    assert bool(((nbr >= 0) & (nbr < N)).all()), "neighbour ids outside [0, N)"
    s = nbr.sort(-1).values
    assert bool((s[..., 1:] != s[..., :-1]).all()), "repeated neighbour"


def neighbour_table(G, N, gen):
    """int32 [G, N, 3]: three distinct neighbours per node, none the node itself, ascending."""
    r = torch.rand(G, N, N, generator=gen)
    idx = torch.arange(N)
    r[:, idx, idx] = 2.0  # never drawn
    nbr = r.argsort(-1)[..., :3].sort(-1).values.to(torch.int32)
    check_table(nbr, N)
    assert bool((nbr != idx.view(1, N, 1)).all())
    return nbr


def node_rows(nbr, scal):
    """Rows [G * N, 4N + 8] of [onehot(n) | cnt | load | 3 x (onehot(nbr_k) | len_k | load_k)] from the table
    nbr [G, N, 3] and scal [G * N, 8] = (cnt, load, len_0, load_0, len_1, load_1, len_2, load_2)."""
    G, N, _ = nbr.shape
    M = G * N
    x = torch.zeros(M, 4 * N + 8, dtype=scal.dtype)
    r = torch.arange(M)
    x[r, r % N] = 1
    x[:, N], x[:, N + 1] = scal[:, 0], scal[:, 1]
    nb = nbr.reshape(M, 3).long()
    for k in range(3):
        off = N + 2 + k * (N + 2)
        x[r, off + nb[:, k]] = 1
        x[:, off + N], x[:, off + N + 1] = scal[:, 2 + 2 * k], scal[:, 3 + 2 * k]
    return x


def scalars_of(x, N):
    """The eight scalar features of node rows x [M, 4N + 8] (node_rows' scal)."""
    cols = [N, N + 1]
    for k in range(3):
        off = N + 2 + k * (N + 2)
        cols += [off + N, off + N + 1]
    return x[:, cols].clone()


@dataclasses.dataclass
class RoutingCase:
    G: int
    N: int
    n: int
    nbr: torch.Tensor   # int32 [G, N, 3]
    x: torch.Tensor     # fp32 [G * N, 4N + 8]
    w: torch.Tensor     # fp32 [n, 4N + 8]
    b: torch.Tensor     # fp32 [n]
    pre: torch.Tensor   # fp64 W x + b
    mag: torch.Tensor   # fp64 |b| + sum_k |w_k x_k|

    @property
    def bound(self):
        """The kernel sums 13 fp32 terms (bias, 4 one-hot weight rows, 8 scalar products) one after the other:
        at most 12 roundings of a partial sum and 8 of a product (none where the compiler contracts to an fma),
        each within 2^-24 of a partial sum that |b| + sum |w_k x_k| bounds: 16 * 2^-24 * that sum."""
        return 16 * U * self.mag

    def without_bias(self):
        return dataclasses.replace(self, b=torch.zeros_like(self.b), pre=self.pre - self.b.double(),
                                   mag=self.mag - self.b.double().abs())


def routing_case_from(nbr, x, n, gen):
    """Random W (i.i.d. N(0, 1/4): a wrong row or column shows) and b for the rows x; fp64 dense reference."""
    G, N, _ = nbr.shape
    check_table(nbr, N)
    K = 4 * N + 8
    assert x.shape == (G * N, K) and x.dtype == torch.float32
    w = torch.randn(n, K, generator=gen) * 0.5
    b = torch.randn(n, generator=gen)
    xd, wd, bd = x.double(), w.double(), b.double()
    return RoutingCase(G, N, n, nbr, x, w, b, xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs())


@functools.lru_cache(maxsize=None)
def routing_case(N, G, n, seed=None):
    """Synthetic rows: a random valid table, scalar features uniform in [0, 4)."""
    gen = torch.Generator().manual_seed(1000 * N + n if seed is None else seed)
    nbr = neighbour_table(G, N, gen)
    x = node_rows(nbr, torch.rand(G * N, 8, generator=gen) * 4)
    return routing_case_from(nbr, x, n, gen)


def act_ref(case, act):
    """(fp64 reference of y, per-element tolerance). none / leaky_relu: the propagated linear bound (slopes <= 1).
    Run-time codes: that bound times sup |f'|, plus the activation kernels' own 2e-6 scaled as test_act_gpu
    scales it (max(1, max|ref| / 8))."""
    ref = ACT_FN[act](case.pre)
    if act in (ACT_NONE, ACT_LEAKY):
        return ref, case.bound
    return ref, ACT_LIP[act] * case.bound + 2e-6 * max(1.0, ref.abs().max().item() / 8)


def sign_check(case, act):
    """(want, sure): the sign bit the reference gives and where it is beyond doubt. none / leaky_relu / gelu are
    positive exactly where the pre-activation is (gelu's erf form gives z (1 + erf) / 2 <= 0 for z < 0, though far
    below any tolerance from z = -5 on): sure where |pre| exceeds its bound. tanh (the hardware-approximate form
    may round a tiny value to 0): sure where |ref y| exceeds y's tolerance."""
    if act != ACT_TANH:
        return case.pre > 0, case.pre.abs() > case.bound
    ref, tol = act_ref(case, act)
    return ref > 0, ref.abs() > tol


def excluded_share(case, act):
    return 1.0 - sign_check(case, act)[1].double().mean().item()


def pack_bits(mask):
    """bool [M, n] (n % 32 == 0) -> int32 [M, n / 32]: bit j of word w = mask[:, 32 w + j]."""
    M, n = mask.shape
    v = (mask.view(M, n // 32, 32).long() << torch.arange(32)).sum(-1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def routing_f32_restatement(case, act_leaky=True):
    """The kernel's 13-term sum in its order, every product and sum rounded to fp32 (no fma) on the CPU: what
    the bound has to admit."""
    N, M = case.N, case.G * case.N
    wt = case.w.t().contiguous()  # [K, n]
    r = torch.arange(M)
    nb = case.nbr.reshape(M, 3).long()
    x = case.x
    acc = case.b.unsqueeze(0) + wt[r % N]
    acc = acc + x[:, N:N + 1] * wt[N]
    acc = acc + x[:, N + 1:N + 2] * wt[N + 1]
    for k in range(3):
        off = N + 2 + k * (N + 2)
        acc = acc + wt[off + nb[:, k]]
        acc = acc + x[:, off + N:off + N + 1] * wt[off + N]
        acc = acc + x[:, off + N + 1:off + N + 2] * wt[off + N + 1]
    return F.leaky_relu(acc, 0.01) if act_leaky else acc


# ---------------------------------------------------------------------------------------------------------
# LayerNorm-LSTM cell
# ---------------------------------------------------------------------------------------------------------
# H -> units per lane of k_lnlstm_pw / k_lnlstm_bwd: every threshold (64|65, 128|129, 256|257) and a partial last
# 64-lane group per instantiation (1, 33; 65; 129, 200; 257, 320, 500)
LN_H = {1: 1, 33: 1, 64: 1, 65: 2, 128: 2, 129: 4, 200: 4, 256: 4, 257: 8, 320: 8, 500: 8, 512: 8}


def lnlstm_leaves(m, H, seed):
    """fp64 leaves of one cell holding fp32 values (gi, gh, c and the seven parameter vectors: LayerNorm weights
    around 1, biases around 0, none trivial), the distributions of test_lnlstm_cell_fwd_bwd."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    leaves = [r(m, 4 * H) * 0.7 + 0.1, r(m, 4 * H) * 0.5 - 0.2, r(m, H), 1 + 0.1 * r(4 * H), 0.1 * r(4 * H),
              1 + 0.1 * r(4 * H), 0.1 * r(4 * H), 0.1 * r(4 * H), 1 + 0.1 * r(H), 0.1 * r(H)]
    return [t.double().requires_grad_() for t in leaves]


def lnlstm_stats(leaves, eps=1e-5):
    """fp64 [m, 6] = (mean, 1 / sqrt(var + eps)) of gi, of gh and of the cell pre-normalisation sigma(f) c +
    sigma(i) tanh(g): what gm_lnlstm_fwd saves per row; and [m, 3], the scale of each mean's rounding error (a
    mean of mixed signs cancels, its error does not): the mean magnitude mean|x| of the gi and gh rows, and for the
    cell row, itself a sum of two rounded products, the mean of |sigma(f) c| + |sigma(i) tanh(g)|."""
    gi, gh, c, wi, bi, wh, bh, bias, wc, bc = (t.detach() for t in leaves)
    H = c.shape[1]
    ln = F.layer_norm
    g = ln(gi, (4 * H,), wi, bi, eps) + ln(gh, (4 * H,), wh, bh, eps) + bias
    i, f, gg, _ = g.chunk(4, 1)
    t0, t1 = torch.sigmoid(f) * c, torch.sigmoid(i) * torch.tanh(gg)
    cols, mags = [], []
    for t, mag in ((gi, gi.abs()), (gh, gh.abs()), (t0 + t1, t0.abs() + t1.abs())):
        cols += [t.mean(1), 1.0 / torch.sqrt(t.var(1, unbiased=False) + eps)]
        mags.append(mag.mean(1))
    return torch.stack(cols, 1), torch.stack(mags, 1)


def rel(a, b):
    """norm-wise relative error, as test_cells_gpu._rel"""
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()
