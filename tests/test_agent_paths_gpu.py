"""Every dispatch path of the agent attention / communication kernels (csrc/gm_agents.hip): the five launchers
gm_agent_attention, gm_agent_comm, gm_agent_comm_bwd, gm_agent_attention_bwd and gm_agent_attention_kl pick among
eleven kernel instantiations and name the one they launch through gm_last_kernel(). CASES maps every name to the
cases that run it; every case asserts the name, so a changed dispatch condition fails here instead of silently
dropping a path. The backward and KL kernels run one existing case of test_dgn_seq_gpu / test_agent_seq_gpu per
name (those files hold their numerics); the two forward kernels get their numerics here.

Forward conventions: q, k, v are column views of one [v | k | q] + 4 buffer (AttModel.forward_rows' layout) whose 4
padding columns hold NaN; outputs are strided with 4 padding columns and one guard row, all NaN before the call:
afterwards the payload is finite and the padding and the guard row are still NaN. Adjacencies are asymmetric with an
all-zero row and a self-only row (attention) or a mixed diagonal, an agent without a neighbour and one adjacent to
all (comm). Two runs give equal bits and the rows of env b equal a B = 1 call on that env's slices bit for bit.

Attention is compared with an fp64 torch restatement of AttModel's core (masked_fill(-1e9), softmax, p @ v + v) in
two regimes: N(0, 1) inputs within the project's 1e-5 absolute contract, and a sharp softmax (q, k = 3 N(0, 1):
scores reach tens, the softmax is nearly one-hot) within a bound derived from fp32 rounding, with u = 2^-24:
    delta_ij = (dk + 1) u scale sum_d |q_id k_jd|          rounding of the score (dk fmas and the scaling)
    |w - w_ref| <= delta_ij + u |w_ref|
    |out - ref| <= (4 Delta_i + (A + 16) u) max_j |v_jhd| + 2 u |ref|,   Delta_i = max_j delta_ij
(a score error Delta moves each softmax weight by a factor within e^(+-2 Delta); the exponentials, the sum of A
terms, the A fmas of p @ v, the division and the skip add give the (A + 16) u). The CPU tests check that a float32
torch restatement stays inside both bounds and that a reference with one neighbour dropped breaks them.

Comm is compared with the fp64 mean form h_i + sum_j h_j / max(cnt_i, 1) within (A + 3) 2^-23 max|h| (an fp32 sum of
at most A - 1 terms, the reciprocal, the product and the add); h is drawn with |h| >= 0.25, so a missing or doubled
neighbour term (>= min|h| / A) exceeds the bound. One dyadic case (neighbour counts in {0, 1, 2, 4, 8}) is exact and
ties the forward to gm_agent_comm_bwd through the adjoint identity sum out g == sum h dh.
"""
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph-marl_amd", "csrc", "gm_agents.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")
INVALID_ARG, UNSUPPORTED = -1, -5
U = 2.0 ** -24
NAN = float("nan")

# kernel name (gm_last_kernel) -> [(test below, case), ...]
#   attention:     (B, A, heads, dk, dv)
#   comm:          (B, A, H, ldh, ldo); comm_exact: the same, dyadic
#   comm_bwd:      an entry of test_agent_seq_gpu.COMM_CASES
#   attention_bwd: an entry of test_dgn_seq_gpu.CASES + the mode; attention_kl: an entry of test_dgn_seq_gpu.CASES
CASES = {
    "k_agent_attention<16>": [("attention", (2, 1, 8, 16, 16)),  # A = 1
                              ("attention", (5, 20, 8, 16, 16)),  # workload shape
                              ("attention", (1, 64, 8, 16, 16))],  # 64 KB of LDS exactly
    "k_agent_attention<0>": [("attention", (2, 7, 3, 8, 24)),  # dk < dv
                             ("attention", (2, 5, 2, 24, 8)),  # dk > dv
                             ("attention", (1, 4, 1, 64, 64)),  # widest head
                             ("attention", (1, 64, 8, 24, 24)),  # 96 KB of LDS
                             ("attention", (1, 64, 8, 32, 48))],  # 160 KB exactly: the largest the host check admits
    "k_agent_comm": [("comm", (3, 5, 48, 96, 52)),  # the h half of [h | c] rows
                     ("comm", (2, 20, 256, 512, 512)),  # workload shape
                     ("comm", (1, 64, 64, 64, 64)),  # A = 64
                     ("comm", (2, 1, 64, 64, 64)),  # A = 1: out is bit-equal to h
                     ("comm", (2, 7, 130, 131, 133)),  # odd strides
                     ("comm", (2, 3, 1, 1, 1)),  # H = 1
                     ("comm", (1, 64, 1024, 1024, 1024)),  # widest H
                     ("comm_exact", (2, 12, 132, 136, 140))],
    "k_agent_comm_bwd<4>": [("comm_bwd", (3, 5, 48, 52, True)), ("comm_exact", (2, 12, 132, 136, 140))],
    "k_agent_comm_bwd<1>": [("comm_bwd", (3, 5, 48, 51, True))],
    "k_agent_attention_bwd<16,reg>": [("attention_bwd", (3, 3, 2, 16, 16, "reg_r"))],
    "k_agent_attention_bwd<16,plain>": [("attention_bwd", (3, 3, 2, 16, 16, "plain"))],
    "k_agent_attention_bwd<0,reg>": [("attention_bwd", (2, 7, 3, 8, 24, "reg_no_r"))],
    "k_agent_attention_bwd<0,plain>": [("attention_bwd", (2, 7, 3, 8, 24, "plain"))],
    "k_agent_attention_kl<16>": [("attention_kl", (3, 3, 2, 16, 16))],
    "k_agent_attention_kl<0>": [("attention_kl", (2, 7, 3, 8, 24))],
}
# names the launchers can set that no test can make them launch, with the reason
UNREACHABLE = {}
LAUNCHERS = ("gm_agent_attention", "gm_agent_comm", "gm_agent_comm_bwd", "gm_agent_attention_bwd",
             "gm_agent_attention_kl")
REGIMES = ("normal", "sharp")


def cases(test):
    return [(k,) + p for k, entries in CASES.items() for t, p in entries if t == test]


ATT = [c[1:] for c in cases("attention")]
COMM = [c[1:] for c in cases("comm")]


# ---------------------------------------------------------------------------------------------------------
# CPU: the CASES table against the launch sites in the source
# ---------------------------------------------------------------------------------------------------------
def _expand_macros(body):
    """Textual expansion of the function-like macros a launcher defines for itself (GM_ATT_BWD): parameters
    substituted, `"a<" #P ",b"` stringification joined into one literal."""
    for m in list(re.finditer(r"^#define (\w+)\(([^)]*)\)((?:.*\\\n)*.*\n)", body, flags=re.M)):
        name, params = m.group(1), [p.strip() for p in m.group(2).split(",")]
        text = m.group(3).replace("\\\n", "\n")
        body = body.replace(m.group(0), "")
        body = re.sub(r"^#undef " + name + r"\n", "", body, flags=re.M)

        def use(u, params=params, text=text):
            t = text
            for p, a in zip(params, [a.strip() for a in u.group(1).split(",")]):
                t = re.sub(r'"\s*#' + p + r'\s*"', a, t)
                t = re.sub(r"\b" + p + r"\b", a, t)
            return t

        body = re.sub(r"\b" + name + r"\(([^()]*)\);?", use, body)
    return body


def _launch_names(src):
    """(launcher, kernel as launched, name set before it) of every hipLaunchKernelGGL of the five launchers."""
    found = []
    for fn in LAUNCHERS:
        m = re.search(r'^extern "C" int ' + fn + r"\(.*?^\}", src, flags=re.S | re.M)
        assert m, fn
        body = _expand_macros(m.group(0))
        assert "#define" not in body, fn
        sets = [(s.start(), s.group(1).strip()) for s in re.finditer(r"gm_set_last_kernel\((.*?)\);", body, flags=re.S)]
        launches = list(re.finditer(r"hipLaunchKernelGGL\(\(*\s*(k_\w+(?:<[^>]*>)?)", body))
        assert launches, fn
        prev = -1
        for la in launches:
            before = [(pos, arg) for pos, arg in sets if prev < pos < la.start()]
            assert before, f"{fn}: launch of {la.group(1)} without a name"
            arg = before[-1][1]
            t = re.fullmatch(r'\((true|false)\)\s*\?\s*"([^"]+)"\s*:\s*"([^"]+)"', arg)
            if t:
                name = t.group(2) if t.group(1) == "true" else t.group(3)
            else:
                lit = re.fullmatch(r'"([^"]+)"', arg)
                assert lit, f"{fn}: name of {la.group(1)} is no literal: {arg}"
                name = lit.group(1)
            found.append((fn, la.group(1), name))
            prev = la.start()
    return found


def _as_named(kernel):
    """k_agent_attention_bwd<16, true> -> k_agent_attention_bwd<16,reg>: the naming rule of the file."""
    k = kernel.replace(" ", "")
    if k.startswith("k_agent_attention_bwd<"):
        k = k.replace(",true>", ",reg>").replace(",false>", ",plain>")
    return k


def test_every_dispatched_kernel_has_a_case():
    """Every launch of the five launchers (those GM_ATT_BWD expands to included) is preceded by a name of its own
    that says which instantiation it is, and the set of names equals CASES + UNREACHABLE: a new launch cannot go
    untested unnoticed and a stale entry fails too."""
    found = _launch_names(open(SRC).read())
    for fn, kernel, name in found:
        assert _as_named(kernel) == name, (fn, kernel, name)
    names = {name for _, _, name in found}
    assert len(names) == len(found) == 11
    assert not set(CASES) & set(UNREACHABLE)
    assert names - set(CASES) - set(UNREACHABLE) == set(), "launched kernels without a case"
    assert (set(CASES) | set(UNREACHABLE)) - names == set(), "stale names in CASES / UNREACHABLE"
    assert all(CASES.values())
    assert UNREACHABLE == {}


# ---------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------
def lib():
    return importlib.import_module("graph-marl_amd._lib")


def att_adjacency(B, A, gen):
    """test_dgn_seq_gpu._adjacency on the CPU (test_adjacencies_are_the_existing_ones holds the two equal): random
    asymmetric, per env one all-zero row and one self-only row (A = 1: the two kinds in different envs)."""
    adj = torch.rand(B, A, A, generator=gen) < 0.4
    if A >= 3:
        adj[:, 0] = False
        adj[:, 1] = False
        adj[:, 1, 1] = True
        assert not torch.equal(adj, adj.transpose(1, 2))
    else:
        adj[::2] = False
        adj[1::2] = True
    return adj.to(torch.int8)


def comm_adjacency(B, A, gen):
    """test_agent_seq_gpu._adjacency on the CPU: the diagonal set in some rows and clear in others, agent 0 without
    a neighbour, agent 1 adjacent to all others."""
    adj = (torch.rand(B, A, A, generator=gen) < 0.3)
    eye = torch.eye(A, dtype=torch.bool)
    adj &= ~eye
    if A > 2:
        adj[:, 0] = False
        adj[:, 1] = ~eye[1]
    diag = torch.zeros(B, A, dtype=torch.bool)
    diag[::2, ::2] = True
    if A > 1:
        diag[1::2, 1::2] = True
    adj |= torch.diag_embed(diag)
    d = torch.diagonal(adj, dim1=1, dim2=2)
    assert d.any() and not d.all()
    return adj.to(torch.int8)


def _cols(buf, nh, dk, dv):
    """(q, k, v) column views of a [v | k | q] buffer"""
    return buf[:, nh * (dv + dk):nh * (dv + 2 * dk)], buf[:, nh * dv:nh * (dv + dk)], buf[:, :nh * dv]


def _heads(x, B, A, nh, d):
    return x.reshape(B, A, nh, d).transpose(1, 2)


def att_core(q, k, v, adj, B, A, nh, dk, dv, dtype):
    """AttModel's core in `dtype`: raw scores [B, heads, A, A] and out rows [B A, heads dv]"""
    qh, kh, vh = (_heads(t.to(dtype), B, A, nh, d) for t, d in ((q, dk), (k, dk), (v, dv)))
    w = torch.matmul(qh, kh.transpose(2, 3)) * torch.tensor(1 / dk ** 0.5, dtype=dtype)
    p = torch.softmax(w.masked_fill(adj.unsqueeze(1) == 0, -1e9), dim=-1)
    out = (torch.matmul(p, vh) + vh).transpose(1, 2).reshape(B * A, nh * dv)
    return w, out


@functools.lru_cache(maxsize=None)
def att_case(B, A, nh, dk, dv, regime):
    """The inputs (CPU), the fp64 reference and the derived bounds of one case; computed once, never modified."""
    gen = torch.Generator().manual_seed(1000 * A + 100 * nh + dk + 3 * dv + (7 if regime == "sharp" else 0))
    n = nh * (dv + 2 * dk)
    buf = torch.randn(B * A, n + 4, generator=gen)
    if regime == "sharp":
        buf[:, nh * dv:n] *= 3.0
    buf[:, n:] = NAN
    adj = att_adjacency(B, A, gen)
    q, k, v = _cols(buf, nh, dk, dv)
    w, out = att_core(q, k, v, adj, B, A, nh, dk, dv, torch.float64)
    qa, ka = _heads(q.double().abs(), B, A, nh, dk), _heads(k.double().abs(), B, A, nh, dk)
    delta = (dk + 1) * U * (1 / dk ** 0.5) * torch.matmul(qa, ka.transpose(2, 3))  # [B, heads, A, A]
    Delta = delta.max(-1).values  # [B, heads, A]
    vmax = _heads(v.double().abs(), B, A, nh, dv).max(2).values  # [B, heads, dv]
    wtol = delta + U * w.abs()
    otol = (4 * Delta.unsqueeze(-1) + (A + 16) * U) * vmax.unsqueeze(2)  # [B, heads, A, dv]
    otol = otol.transpose(1, 2).reshape(B * A, nh * dv) + 2 * U * out.abs()
    if regime == "normal":  # the project's contract on N(0, 1) inputs
        wtol, otol = torch.full_like(wtol, 1e-5), torch.full_like(otol, 1e-5)
    return dict(buf=buf, adj=adj, w=w, out=out, wtol=wtol, otol=otol)


def att_ratios(c, w, out):
    """worst |error| / tolerance of scores and out rows"""
    return ((w.double() - c["w"]).abs() / c["wtol"]).max().item(), ((out.double() - c["out"]).abs() / c["otol"]).max().item()


def run_attention(L, buf, adj, B, A, nh, dk, dv, kernel, with_w=True):
    """gm_agent_attention on poisoned outputs; returns out rows [B A, heads dv] and the scores (CPU)"""
    n, no = nh * (dv + 2 * dk), nh * dv
    q, k, v = _cols(buf, nh, dk, dv)
    out = torch.full((B * A + 1, no + 4), NAN, device="cuda")
    nw = B * nh * A * A
    w = torch.full((nw + 64,), NAN, device="cuda") if with_w else None
    L.check(L.lib().gm_agent_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), buf.stride(0), adj.data_ptr(), B, A, nh,
                                       dk, dv, out.data_ptr(), out.stride(0), L.ptr(w), L.stream_ptr()))
    assert L.last_kernel() == kernel
    o = out.cpu()
    assert torch.isfinite(o[:B * A, :no]).all()
    assert torch.isnan(o[:B * A, no:]).all() and torch.isnan(o[B * A:]).all(), "wrote outside the payload"
    if not with_w:
        return o[:B * A, :no], None
    wc = w.cpu()
    assert torch.isfinite(wc[:nw]).all(), "att_weights not fully written"
    assert torch.isnan(wc[nw:]).all()
    return o[:B * A, :no], wc[:nw].view(B, nh, A, A)


# ---------------------------------------------------------------------------------------------------------
# gm_agent_attention
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("B,A,nh,dk,dv", ATT)
def test_attention_bounds_admit_float32_and_catch_a_dropped_neighbour(B, A, nh, dk, dv, regime):
    """CPU: a float32 torch restatement of the core stays inside both bounds of every case, and (A > 1) the fp64
    reference with one neighbour dropped (the one with the largest softmax weight in a row that keeps another)
    leaves the out bound: the bounds are neither too tight for correct fp32 nor loose enough for a wrong row."""
    c = att_case(B, A, nh, dk, dv, regime)
    q, k, v = _cols(c["buf"], nh, dk, dv)
    w32, o32 = att_core(q, k, v, c["adj"], B, A, nh, dk, dv, torch.float32)
    rw, ro = att_ratios(c, w32, o32)
    print(f"float32 restatement {(B, A, nh, dk, dv)} {regime}: worst error / tolerance w {rw:.3g}, out {ro:.3g}")
    assert rw <= 1 and ro <= 1
    if regime == "sharp":
        p = torch.softmax(c["w"].masked_fill(c["adj"].unsqueeze(1) == 0, -1e9), -1)
        print(f"  max |score| {c['w'].abs().max().item():.3g}, median of the rows' largest softmax weight "
              f"{p.max(-1).values.median().item():.3g}")
        assert c["w"].abs().max() >= 10  # scores reach tens
    if A > 1:
        adj = c["adj"].clone()
        p = torch.softmax(c["w"].masked_fill(adj.unsqueeze(1) == 0, -1e9), -1).max(1).values  # [B, A, A]
        p = p * (adj != 0) * (adj.sum(-1, keepdim=True) >= 2)
        assert p.max() > 0, "no row with two neighbours"
        b, i, j = np.unravel_index(int(p.argmax()), p.shape)
        adj[b, i, j] = 0
        _, wrong = att_core(q, k, v, adj, B, A, nh, dk, dv, torch.float64)
        ratio = ((wrong - c["out"]).abs() / c["otol"]).max().item()
        print(f"  one neighbour dropped: error / tolerance {ratio:.3g}")
        assert ratio > 1


@gpu
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("kernel,B,A,nh,dk,dv", cases("attention"))
def test_attention_paths(kernel, B, A, nh, dk, dv, regime):
    """out and att_weights (the raw score, masked pairs included) against fp64: 1e-5 on N(0, 1), the derived bound
    on the sharp softmax; att_weights given or null gives the same out bits; two runs and per-env calls too."""
    L = lib()
    c = att_case(B, A, nh, dk, dv, regime)
    buf, adj = c["buf"].cuda(), c["adj"].cuda()
    out, w = run_attention(L, buf, adj, B, A, nh, dk, dv, kernel)
    rw, ro = att_ratios(c, w, out)
    print(f"gm_agent_attention {kernel} {(B, A, nh, dk, dv)} {regime}: worst error / tolerance w {rw:.3g}, "
          f"out {ro:.3g}; max |w| {c['w'].abs().max().item():.3g}")
    assert rw <= 1 and ro <= 1
    out2, w2 = run_attention(L, buf, adj, B, A, nh, dk, dv, kernel)
    assert torch.equal(out, out2) and torch.equal(w, w2)
    out3, _ = run_attention(L, buf, adj, B, A, nh, dk, dv, kernel, with_w=False)
    assert torch.equal(out, out3)
    if B > 1:
        for b in range(B):
            ob, wb = run_attention(L, buf[b * A:(b + 1) * A], adj[b:b + 1], 1, A, nh, dk, dv, kernel)
            assert torch.equal(ob, out[b * A:(b + 1) * A]) and torch.equal(wb[0], w[b]), b


@gpu
@pytest.mark.parametrize("what", ["A65", "dk65", "dv65", "null_v", "ld", "ldo", "lds"])
def test_attention_refuses(what):
    """GM_ERR_INVALID_ARG for A = 65, dk = 65, dv = 65, a null v, ld < heads max(dk, dv) and ldo < heads dv;
    GM_ERR_UNSUPPORTED for (1, 64, 8, 48, 33), which needs more than 160 KB of LDS. Nothing is launched: the outputs
    keep their NaNs and gm_last_error names the function."""
    L = lib()
    B, A, nh, dk, dv = {"A65": (1, 65, 2, 16, 16), "dk65": (1, 4, 2, 65, 16), "dv65": (1, 4, 2, 16, 65),
                        "lds": (1, 64, 8, 48, 33)}.get(what, (1, 4, 2, 16, 24))
    n, no = nh * (dv + 2 * dk), nh * dv
    buf = torch.randn(B * A, n, device="cuda")
    adj = torch.ones(B, A, A, dtype=torch.int8, device="cuda")
    out = torch.full((B * A, no), NAN, device="cuda")
    w = torch.full((B, nh, A, A), NAN, device="cuda")
    q, k, v = _cols(buf, nh, dk, dv)
    ld = nh * max(dk, dv) - 1 if what == "ld" else n
    ldo = no - 1 if what == "ldo" else no
    rc = L.lib().gm_agent_attention(q.data_ptr(), k.data_ptr(), None if what == "null_v" else v.data_ptr(), ld,
                                    adj.data_ptr(), B, A, nh, dk, dv, out.data_ptr(), ldo, w.data_ptr(), L.stream_ptr())
    assert rc == (UNSUPPORTED if what == "lds" else INVALID_ARG)
    assert b"gm_agent_attention:" in L.lib().gm_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(w).all()


# ---------------------------------------------------------------------------------------------------------
# gm_agent_comm
# ---------------------------------------------------------------------------------------------------------
def comm_ref(h, adj, extra=None):
    """fp64 mean form h_i + sum_{j != i, adj_ij} h_j / max(cnt_i, 1), h [B, A, H]; extra [B, A, A]: added to the
    summed terms' weights with the counts kept (a missing or doubled term)"""
    A = h.shape[1]
    m = (adj != 0).double() * (1 - torch.eye(A, dtype=torch.float64))
    cnt = m.sum(-1, keepdim=True).clamp_min(1)
    return h.double() + ((m if extra is None else m + extra) @ h.double()) / cnt


@functools.lru_cache(maxsize=None)
def comm_case(B, A, H, ldh, ldo):
    gen = torch.Generator().manual_seed(1000 * A + H + ldh)
    adj = comm_adjacency(B, A, gen)
    h = torch.randn(B * A, H, generator=gen)
    h = h + 0.25 * torch.where(h >= 0, 1.0, -1.0)  # |h| >= 0.25
    ref = comm_ref(h.view(B, A, H), adj).view(B * A, H)
    return dict(h=h, adj=adj, ref=ref, bound=(A + 3) * 2.0 ** -23 * h.abs().max().item())


def run_comm(L, h, ldh, adj, B, A, H, ldo):
    """gm_agent_comm on rows of stride ldh (NaN past the payload) into poisoned rows of stride ldo; out rows (CPU)"""
    hb = torch.full((B * A + 1, ldh), NAN, device="cuda")
    hb[:B * A, :H] = h
    out = torch.full((B * A + 1, ldo), NAN, device="cuda")
    L.check(L.lib().gm_agent_comm(hb.data_ptr(), ldh, adj.data_ptr(), B, A, H, out.data_ptr(), ldo, L.stream_ptr()))
    assert L.last_kernel() == "k_agent_comm"
    o = out.cpu()
    assert torch.isfinite(o[:B * A, :H]).all()
    assert torch.isnan(o[:B * A, H:]).all() and torch.isnan(o[B * A:]).all(), "wrote outside the payload"
    return o[:B * A, :H]


@pytest.mark.parametrize("B,A,H,ldh,ldo", COMM)
def test_comm_bound_catches_a_missing_or_doubled_neighbour(B, A, H, ldh, ldo):
    """CPU: with |h| >= 0.25, leaving one neighbour term out of a row's sum, or adding it twice, moves the row by at
    least min|h| / A, which is above the bound of the GPU test in every case with A > 1."""
    c = comm_case(B, A, H, ldh, ldo)
    h = c["h"].view(B, A, H)
    assert h.abs().min() >= 0.25
    if A == 1:
        assert torch.equal(c["ref"].float(), c["h"])  # no neighbour: the mean form is h itself
        return
    m = (c["adj"] != 0) & ~torch.eye(A, dtype=torch.bool)
    b, i, j = (int(x[0]) for x in torch.nonzero(m * (m.sum(-1, keepdim=True) >= 2), as_tuple=True))
    for sign in (-1.0, 1.0):
        extra = torch.zeros(B, A, A, dtype=torch.float64)
        extra[b, i, j] = sign
        shift = (comm_ref(h, c["adj"], extra) - c["ref"].view(B, A, H)).abs()[b, i].max().item()
        print(f"comm {(B, A, H)}: term {'doubled' if sign > 0 else 'missing'}: shift {shift:.3g}, bound {c['bound']:.3g}")
        assert shift >= h.abs().min().item() / A > c["bound"]


@gpu
@pytest.mark.parametrize("kernel,B,A,H,ldh,ldo", cases("comm"))
def test_comm_paths(kernel, B, A, H, ldh, ldo):
    L = lib()
    c = comm_case(B, A, H, ldh, ldo)
    h, adj = c["h"].cuda(), c["adj"].cuda()
    out = run_comm(L, h, ldh, adj, B, A, H, ldo)
    err = (out.double() - c["ref"]).abs().max().item()
    print(f"gm_agent_comm {(B, A, H, ldh, ldo)}: worst error / tolerance {err / c['bound']:.3g}")
    assert err <= c["bound"]
    if A == 1:
        assert torch.equal(out, c["h"])
    assert torch.equal(out, run_comm(L, h, ldh, adj, B, A, H, ldo))
    if B > 1:
        for b in range(B):
            ob = run_comm(L, h[b * A:(b + 1) * A], ldh, adj[b:b + 1], 1, A, H, ldo)
            assert torch.equal(ob, out[b * A:(b + 1) * A]), b


@gpu
@pytest.mark.parametrize("kernel,B,A,H,ldh,ldo", [c for c in cases("comm_exact") if c[0] == "k_agent_comm"])
def test_comm_exact_and_adjoint(kernel, B, A, H, ldh, ldo):
    """Every row has 0, 1, 2, 4 or 8 neighbours (the diagonal set in some rows and clear in others) and h, g are
    small integers times 2^-3: every sum, mean and product is exact, so out equals the fp64 mean form bit for bit
    (a kernel that counts the diagonal divides by 3, 5 or 9), and with dh = gm_agent_comm_bwd(g) the adjoint
    identity sum out g == sum h dh holds exactly in fp64."""
    L = lib()
    gen = torch.Generator().manual_seed(3)
    counts = [0, 1, 2, 4, 8]
    adj = torch.zeros(B, A, A, dtype=torch.int8)
    for b in range(B):
        for i in range(A):
            others = [j for j in range(A) if j != i]
            for t in torch.randperm(A - 1, generator=gen)[:counts[(i + b) % 5]].tolist():
                adj[b, i, others[t]] = 1
            adj[b, i, i] = (i + b) % 2
    off = adj * (1 - torch.eye(A, dtype=torch.int8))
    assert sorted(set(off.sum(-1).flatten().tolist())) == counts and not torch.equal(adj, adj.transpose(1, 2))
    h = torch.randint(-64, 65, (B * A, H), generator=gen).float() / 8
    g = torch.randint(-64, 65, (B * A, H), generator=gen).float() / 8
    ref = comm_ref(h.view(B, A, H), adj).view(B * A, H)
    adjc = adj.cuda()
    out = run_comm(L, h.cuda(), ldh, adjc, B, A, H, ldo)
    assert torch.equal(out.double(), ref)
    gb = torch.full((B * A + 1, ldh), NAN, device="cuda")
    gb[:B * A, :H] = g.cuda()
    dh = torch.full((B * A + 1, ldo), NAN, device="cuda")
    L.check(L.lib().gm_agent_comm_bwd(gb.data_ptr(), ldh, None, 0, adjc.data_ptr(), B, A, H, dh.data_ptr(), ldo,
                                      L.stream_ptr()))
    assert L.last_kernel() == "k_agent_comm_bwd<4>"
    d = dh.cpu()
    assert torch.isnan(d[:B * A, H:]).all() and torch.isnan(d[B * A:]).all()
    lhs, rhs = (out.double() * g.double()).sum().item(), (h.double() * d[:B * A, :H].double()).sum().item()
    print(f"adjoint: sum out g = {lhs!r}, sum h dh = {rhs!r}")
    assert lhs == rhs


@gpu
@pytest.mark.parametrize("what", ["A65", "alias", "ldh", "ldo"])
def test_comm_refuses(what):
    """GM_ERR_INVALID_ARG for A = 65, out == h, ldh < H and ldo < H; the output keeps its NaNs."""
    L = lib()
    B, A, H = 2, 65 if what == "A65" else 5, 48
    h = torch.randn(B * A, H, device="cuda")
    adj = torch.ones(B, A, A, dtype=torch.int8, device="cuda")
    out = torch.full((B * A, H), NAN, device="cuda")
    rc = L.lib().gm_agent_comm(h.data_ptr(), H - 1 if what == "ldh" else H, adj.data_ptr(), B, A, H,
                               h.data_ptr() if what == "alias" else out.data_ptr(), H - 1 if what == "ldo" else H,
                               L.stream_ptr())
    assert rc == INVALID_ARG
    assert b"gm_agent_comm:" in L.lib().gm_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isfinite(h).all()


# ---------------------------------------------------------------------------------------------------------
# the backward and KL kernels: one existing case per name
# ---------------------------------------------------------------------------------------------------------
@gpu
def test_adjacencies_are_the_existing_ones():
    """att_adjacency / comm_adjacency restate test_dgn_seq_gpu._adjacency / test_agent_seq_gpu._adjacency on the CPU
    (the CPU tests above need them without a GPU): equal for equal generators, in every case's (B, A)."""
    import test_agent_seq_gpu as AS
    import test_dgn_seq_gpu as DS

    for mine, theirs, shapes in ((att_adjacency, DS._adjacency, {c[:2] for c in ATT}),
                                 (comm_adjacency, AS._adjacency, {c[:2] for c in COMM})):
        for B, A in sorted(shapes):
            g1, g2 = torch.Generator().manual_seed(B + A), torch.Generator().manual_seed(B + A)
            assert torch.equal(mine(B, A, g1), theirs(B, A, g2).cpu())


@gpu
@pytest.mark.parametrize("kernel,B,A,nh,dk,dv,mode", cases("attention_bwd"))
def test_attention_bwd_names(kernel, B, A, nh, dk, dv, mode):
    import test_dgn_seq_gpu as DS

    assert (B, A, nh, dk, dv) in DS.CASES
    DS.test_agent_attention_bwd_vs_fp64(B, A, nh, dk, dv, mode)
    assert lib().last_kernel() == kernel


@gpu
@pytest.mark.parametrize("kernel,B,A,nh,dk,dv", cases("attention_kl"))
def test_attention_kl_names(kernel, B, A, nh, dk, dv):
    import test_dgn_seq_gpu as DS

    assert (B, A, nh, dk, dv) in DS.CASES
    DS.test_agent_attention_kl_vs_fp64(B, A, nh, dk, dv)
    assert lib().last_kernel() == kernel


@gpu
@pytest.mark.parametrize("kernel,B,A,H,ld,two", cases("comm_bwd"))
def test_comm_bwd_names(kernel, B, A, H, ld, two):
    import test_agent_seq_gpu as AS

    assert (B, A, H, ld, two) in AS.COMM_CASES
    AS.test_agent_comm_bwd_vs_fp64(B, A, H, ld, two)
    assert lib().last_kernel() == kernel


# ---------------------------------------------------------------------------------------------------------
# the models on both sides of A = 64
# ---------------------------------------------------------------------------------------------------------
def _golden_model(M, name):
    G = np.load(os.path.join(GOLDEN, "models.npz"))
    D = G["obs"].shape[-1]
    m = M.DGN(D, [64], 4, 3, 1) if name == "dgn_small" else M.CommNet(D, [128, 64], 4, 2)
    m.load_state_dict({k[len(name) + 3:]: torch.as_tensor(G[k]) for k in G.files if k.startswith(name + "_w_")})
    return m.cuda(), torch.as_tensor(G["obs"]).reshape(-1, D)


def _golden_obs(rows, B, A, gen):
    """[B, A, D] observations drawn with replacement from the goldens' observation rows: the distribution for which
    the 1e-5 tolerance of test_models_gpu.py is known to hold"""
    return rows[torch.randint(0, rows.shape[0], (B * A,), generator=gen)].view(B, A, -1).cuda()


def _spy(monkeypatch, L, name):
    """Record gm_last_kernel right after every call of one launcher. The GEMMs around the agent kernels name their
    kernels too, so the name has to be read before the model's next call (as test_netmon_paths_gpu does)."""
    ran, real = [], getattr(L.lib(), name)

    def spy(*a):
        rc = real(*a)
        ran.append(L.last_kernel())
        return rc

    monkeypatch.setattr(L.lib(), name, spy)
    return ran


@gpu
@pytest.mark.parametrize("A", [1, 20, 64, 65])
def test_dgn_forward_on_both_sides_of_64_agents(A, monkeypatch):
    """DGN.forward without grad (the HIP attention core up to A = 64, torch above) against DGN.forward with grad
    (torch): q and every att_weights entry within 1e-5. Up to 64 agents every attention layer launches
    k_agent_attention<16>; at 65 the launcher is not called and the name another launcher left (a sentinel from
    gm_agent_comm) is never replaced by an attention kernel's."""
    L = lib()
    M = importlib.import_module("graph-marl_amd.model")
    m, rows = _golden_model(M, "dgn_small")
    gen = torch.Generator().manual_seed(A)
    B = 2
    x = _golden_obs(rows, B, A, gen)
    adj = att_adjacency(B, A, gen).float().cuda()
    with torch.enable_grad():
        q1 = m(x, adj).detach()
        w1 = [w.detach() for w in m.att_weights]
    run_comm(L, torch.ones(2, 4, device="cuda"), 4, torch.ones(1, 2, 2, dtype=torch.int8, device="cuda"), 1, 2, 4, 4)
    assert L.last_kernel() == "k_agent_comm"  # the sentinel
    ran = _spy(monkeypatch, L, "gm_agent_attention")
    with torch.no_grad():
        q0 = m(x, adj)
        w0 = list(m.att_weights)
    if A <= 64:
        assert ran == ["k_agent_attention<16>"] * len(m.att_layers)
    else:
        assert ran == [] and not L.last_kernel().startswith("k_agent_attention")
    assert len(w0) == len(w1) == len(m.att_layers)
    err = max([(q0 - q1).abs().max().item()] + [(a - b).abs().max().item() for a, b in zip(w0, w1)])
    print(f"DGN A={A}: no-grad vs autograd forward, worst difference of q and att_weights {err:.3g}")
    assert err <= 1e-5


@gpu
def test_commnet_rollout_matches_autograd_at_64_agents(monkeypatch):
    """CommNet.forward_rows (gm_agent_comm once per round) against its autograd forward at A = 64: q and the
    recurrent state within 1e-5."""
    L = lib()
    M = importlib.import_module("graph-marl_amd.model")
    m, rows = _golden_model(M, "commnet")
    gen = torch.Generator().manual_seed(64)
    B, A = 2, 64
    x = _golden_obs(rows, B, A, gen)
    adj = comm_adjacency(B, A, gen).cuda()
    m.state = None
    with torch.enable_grad():
        q1 = m(x, adj.float()).detach()
        s1 = m.state.detach()
    ran = _spy(monkeypatch, L, "gm_agent_comm")
    m.state = None
    scratch = {}

    def get(key, r, c):
        if (key, r, c) not in scratch:
            scratch[(key, r, c)] = torch.empty(r, c, device="cuda")
        return scratch[(key, r, c)]

    with torch.no_grad():
        q0 = m.forward_rows(x.reshape(B * A, -1), x.shape[-1], x.shape[-1], get, adj=adj, B=B, A=A).view(B, A, -1)
    assert ran == ["k_agent_comm"] * m.comm_rounds
    eq, es = (q0 - q1).abs().max().item(), (m.state - s1).abs().max().item()
    print(f"CommNet A=64: rollout vs autograd forward, worst difference q {eq:.3g}, state {es:.3g}")
    assert eq <= 1e-5 and es <= 1e-5
