"""Every dispatch path of the NetMon gather / scatter kernels (csrc/gm_netmon.hip): the host entry points
gm_netmon_readout_ld, gm_netmon_readout_bwd[_sym], gm_mp_aggregate[_rows|_bwd], gm_lstm_cell_bwd and
gm_qhead_bwd each pick one of several kernels from H, R, N, deg, pointer alignment and strides. CASES maps every
kernel name those dispatchers can report through gm_last_kernel() to the cases that run it; every case asserts
the name, so a change of a dispatch threshold fails here instead of silently dropping a path.

Inputs are dyadic (small integers times 2^-3, |x| <= 8): every sum of up to a few thousand terms is exact in
fp32, so the kernels are compared bit for bit (torch.equal) with a plain fp64 torch reference (index_add_ over
(row, segment) -> node, no library call). Neighbour tables are built here (symmetric unless stated, with -1
entries, one isolated node); agent maps repeat nodes and leave a node unread. Outputs, the padding columns past
each row's payload and a guard row past each buffer are NaN before the call: a kernel that reads padding or
leaves an element unwritten fails the comparison, one that writes past a row fails the guard check.

k_readout_bwd_nodes<long long> needs more than 2^31 (node, 16-byte chunk) items (32 GB of gradient): out of
reach of a seconds-long test, listed in UNREACHABLE.
"""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "graph-marl_amd", "csrc", "gm_netmon.hip")

# kernel name (gm_last_kernel) -> (test below, its cases)
#   readout_bwd: (G, N, R, H, how); how = "map" (agent map), "map+odd" (agent map, dout stride 4H + 1) or
#                "sym" (no map through the opt-in gm_netmon_readout_bwd_sym)
#   readout_fwd: H (every H runs with and without an agent map, rows % 4 in {0, 1, 2, 3})
#   aggregate:   (direction, deg, H)
#   lstm_cell_bwd: (H, ld_dg - 4H); qhead_bwd: (cols, nq)
CASES = {
    "k_readout_bwd_nodes<unsigned>": ("readout_bwd", [(3, 10, 10, 8, "sym")]),
    "k_readout_bwd_cs<1>/S=4": ("readout_bwd", [(3, 10, 7, 16, "map"), (2, 20, 64, 16, "map")]),
    "k_readout_bwd_cs<1>/S=8": ("readout_bwd", [(2, 20, 64, 256, "map")]),  # R H > 12288, R <= 64
    "k_readout_bwd_cs<2>/S=4": ("readout_bwd", [(2, 20, 65, 16, "map"), (2, 20, 128, 16, "map")]),  # R > 64
    "k_readout_bwd_cs<2>/S=8": ("readout_bwd", [(2, 128, 128, 128, "map")]),  # R H > 12288
    "k_readout_bwd_lds": ("readout_bwd", [(3, 10, 7, 40, "map")]),  # (H / 4) % 4 != 0
    "k_readout_bwd_g<4>": ("readout_bwd", [(2, 20, 64, 72, "map")]),  # LDS need > 48 KB, (H / 4) % 4 != 0
    "k_readout_bwd_g<2>": ("readout_bwd", [(3, 10, 7, 6, "map")]),
    "k_readout_bwd_g<1>": ("readout_bwd", [(3, 10, 7, 5, "map"), (3, 10, 7, 8, "map+odd")]),
    "k_readout_bwd<4>": ("readout_bwd", [(2, 20, 130, 16, "map")]),  # R > 128
    "k_readout_bwd<2>": ("readout_bwd", [(2, 20, 65, 6, "map")]),  # R > 64, V < 4
    "k_readout_bwd<1>": ("readout_bwd", [(2, 100, 20, 11, "map")]),  # N H > 1024
    "k_readout_rows": ("readout_fwd", [128, 256, 132]),  # 256: the wide-row tail loop; 132: W4 straddles 128
    "k_readout<2>": ("readout_fwd", [6]),
    "k_readout<1>": ("readout_fwd", [5]),
    "k_mp_aggregate3<4>": ("aggregate", [("fwd", 3, 128)]),
    "k_mp_aggregate3<2>": ("aggregate", [("fwd", 3, 6)]),
    "k_mp_aggregate3<1>": ("aggregate", [("fwd", 3, 5)]),
    "k_mp_aggregate<fwd,4>": ("aggregate", [("fwd", d, 128) for d in (2, 5, 8)]),
    "k_mp_aggregate<fwd,2>": ("aggregate", [("fwd", d, 6) for d in (2, 5, 8)]),
    "k_mp_aggregate<fwd,1>": ("aggregate", [("fwd", d, 5) for d in (2, 5, 8)]),
    "k_mp_aggregate<bwd,4>": ("aggregate", [("bwd", d, 128) for d in (2, 3, 5, 8)]),
    "k_mp_aggregate<bwd,2>": ("aggregate", [("bwd", d, 6) for d in (2, 3, 5, 8)]),
    "k_mp_aggregate<bwd,1>": ("aggregate", [("bwd", d, 5) for d in (2, 3, 5, 8)]),
    "k_lstm_cell_bwd4": ("lstm_cell_bwd", [(512, 0)]),
    "k_lstm_cell_bwd": ("lstm_cell_bwd", [(96, 0), (320, 0), (128, 1)]),  # 128 with ld_dg = 4H + 1
    "k_qhead_bwd4": ("qhead_bwd", [(1024, 1), (1024, 4)]),
    "k_qhead_bwd": ("qhead_bwd", [(260, 1), (260, 4)]),
}
# names the dispatchers can set that no test can make them launch, with the reason
UNREACHABLE = {
    "k_readout_bwd_nodes<long long>": "needs more than 2^31 (node, chunk) items: 32 GB of gradient",
    "k_readout<4>": "gm_netmon_readout_ld sends V == 4 to k_readout_rows; GM_VLAUNCH names a form it never launches",
}
# the five dispatchers (the two readout-backward exports share the static readout_bwd)
DISPATCHERS = ("gm_netmon_readout_ld", "readout_bwd", "launch_agg", "gm_lstm_cell_bwd", "gm_qhead_bwd")


def cases(test):
    return [(k,) + (p if isinstance(p, tuple) else (p,)) for k, (t, ps) in CASES.items() if t == test for p in ps]


# ---------------------------------------------------------------------------------------------------------
# CPU: the CASES table against the launch sites in the source
# ---------------------------------------------------------------------------------------------------------
def _dispatcher_bodies():
    src = open(SRC).read()
    bodies = {}
    for name in DISPATCHERS:
        m = re.search(r'^(?:extern "C" |static )int ' + name + r"\(.*?^\}", src, flags=re.S | re.M)
        assert m, name
        bodies[name] = m.group(0)
    return src, bodies


def test_every_dispatched_kernel_has_a_case():
    """Every launch site of the five dispatchers names its kernel for gm_last_kernel (GM_RAN, or GM_VLAUNCH
    which does it itself), and every name they can set is in CASES or in UNREACHABLE with a reason: a newly
    added kernel cannot go untested unnoticed."""
    src, bodies = _dispatcher_bodies()
    assert re.search(r"#define GM_VLAUNCH\(KER, V, GRID, \.\.\.\)[^\n]*\n[^\n]*\n\s*GM_RAN\(", src)
    names = set()
    for fn, body in bodies.items():
        rans = [(m.start(), m.group(1)) for m in re.finditer(r"GM_RAN\((.*?)\);", body, flags=re.S)]
        for _, arg in rans:
            found = re.findall(r'"([^"]+)"', arg)
            assert found, (fn, arg)
            names.update(found)
        for m in re.finditer(r"GM_VLAUNCH\((\w+),", body):
            names.update(f"{m.group(1)}<{v}>" for v in (4, 2, 1))
        launches = list(re.finditer(r"hipLaunchKernelGGL\(\(*(k_\w+)", body))
        assert launches or "GM_VLAUNCH(" in body, fn
        for m in launches:  # the nearest GM_RAN before a launch names that launch's kernel
            before = [arg for pos, arg in rans if pos < m.start()]
            assert before and re.search(r'"%s[</"]' % m.group(1), before[-1]), (fn, m.group(1))
    assert names, "no kernel names found"
    assert not set(CASES) & set(UNREACHABLE)
    assert names - set(CASES) - set(UNREACHABLE) == set(), "dispatched kernels without a case"
    assert (set(CASES) | set(UNREACHABLE)) - names == set(), "stale names in CASES / UNREACHABLE"
    assert all(ps for _, ps in CASES.values())


# ---------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------
def lib():
    return importlib.import_module("graph-marl_amd._lib")


def dyadic(shape, gen):
    """small integers times 2^-3, |x| <= 8"""
    return torch.randint(-64, 65, shape, generator=gen).float() / 8


def sym_table(G, N, deg, seed, shuffle=False):
    """Symmetric neighbour tables [G, N, deg] without repeated entries: random edges while both ends have a free
    slot (so some lists stay short: -1 entries), node N - 2 isolated (nobody reads it as a neighbour). Lists
    ascending with the -1 last, as dense_to_nbr writes them; shuffle: ids and holes in random slots."""
    gen = torch.Generator().manual_seed(seed)
    nbr = torch.full((G, N, deg), -1, dtype=torch.int32)
    for b in range(G):
        lists = [[] for _ in range(N)]
        for u, v in torch.randint(0, N, (N * deg, 2), generator=gen).tolist():
            if u != v and N - 2 not in (u, v) and v not in lists[u] and len(lists[u]) < deg and len(lists[v]) < deg:
                lists[u].append(v)
                lists[v].append(u)
        for n in range(N):
            ids = sorted(lists[n])
            slots = list(range(len(ids)))
            if shuffle:
                slots = torch.randperm(deg, generator=gen)[:len(ids)].tolist()
                ids = [ids[i] for i in torch.randperm(len(ids), generator=gen).tolist()]
            for s, v in zip(slots, ids):
                nbr[b, n, s] = v
    assert (nbr < 0).any() and (nbr >= 0).any()
    return nbr


def agent_map(G, N, R, seed):
    """agent -> node [G, R] with a repeated node; node N - 1 is nobody's node"""
    gen = torch.Generator().manual_seed(seed)
    an = torch.randint(0, N - 1, (G, R), generator=gen, dtype=torch.int32)
    if R > 1:
        an[:, 1] = an[:, 0]
    return an


def padded(x2d, ld, guard=1):
    """the rows of x2d (CPU) at the start of a NaN device buffer of row stride ld, with `guard` NaN rows behind"""
    rows, w = x2d.shape
    buf = torch.full((rows + guard, ld), float("nan"), device="cuda")
    buf[:rows, :w] = x2d.cuda()
    return buf


def pad_of(H):
    """padding columns that keep the vector width H allows (4, 2 or 1 floats)"""
    return 4 if H % 4 == 0 else 2 if H % 2 == 0 else 3


# ---------------------------------------------------------------------------------------------------------
# readout backward
# ---------------------------------------------------------------------------------------------------------
def readout_bwd_ref(dout, nbr, an):
    """fp64 scatter of dout [G, R, deg + 1, H] (CPU): index_add_ over (row, segment) -> node. Returns dh_final,
    dh_prev [G * N, H] (double) and which nodes each of them was read from at all."""
    G, R, S, H = dout.shape
    N, deg = nbr.shape[1], nbr.shape[2]
    u = (torch.arange(N).expand(G, N) if an is None else an).long()  # [G, R]
    off = (torch.arange(G) * N).view(G, 1)
    d = dout.double()
    dhf = torch.zeros(G * N, H, dtype=torch.float64)
    dhf.index_add_(0, (off + u).flatten(), d[:, :, 0].reshape(G * R, H))
    nb = torch.gather(nbr.long(), 1, u.unsqueeze(-1).expand(G, R, deg))  # [G, R, deg]
    ok = nb >= 0
    dhp = torch.zeros(G * N, H, dtype=torch.float64)
    dhp.index_add_(0, (off.unsqueeze(-1) + nb)[ok], d[:, :, 1:][ok])
    readf = torch.bincount((off + u).flatten(), minlength=G * N) > 0
    readp = torch.bincount((off.unsqueeze(-1) + nb)[ok], minlength=G * N) > 0
    return dhf, dhp, readf, readp


def readout_bwd_ordered_f32(dout, nbr, an):
    """fp32 sums taken in ascending (row, segment) order on the CPU: what every kernel's comment promises"""
    G, R, S, H = dout.shape
    N = nbr.shape[1]
    dhf, dhp = torch.zeros(G * N, H), torch.zeros(G * N, H)
    for g in range(G):
        for r in range(R):
            u = r if an is None else int(an[g, r])
            dhf[g * N + u] += dout[g, r, 0]
            for k, v in enumerate(nbr[g, u].tolist()):
                if v >= 0:
                    dhp[g * N + v] += dout[g, r, k + 1]
    return dhf, dhp


def run_readout_bwd(dout, nbr, an, H, which, stride, sym=False):
    """the library call on poisoned buffers; returns dh_final, dh_prev (CPU, None when not asked for)"""
    L = lib()
    G, R, S, _ = dout.shape
    N, deg = nbr.shape[1], nbr.shape[2]
    dbuf = padded(dout.reshape(G * R, S * H), stride)
    nb, a = nbr.cuda(), None if an is None else an.cuda()
    of = torch.full((G * N + 1, H), float("nan"), device="cuda") if "f" in which else None
    op = torch.full((G * N + 1, H), float("nan"), device="cuda") if "p" in which else None
    if sym:
        assert an is None
        L.check(L.lib().gm_netmon_readout_bwd_sym(dbuf.data_ptr(), stride, nb.data_ptr(), G, N, deg, H, L.ptr(of),
                                                  L.ptr(op), L.stream_ptr()))
    else:
        L.check(L.lib().gm_netmon_readout_bwd(dbuf.data_ptr(), stride, nb.data_ptr(), L.ptr(a), G, N, R, deg, H,
                                              L.ptr(of), L.ptr(op), L.stream_ptr()))
    kernel = L.last_kernel()
    torch.cuda.synchronize()
    res = []
    for o in (of, op):
        if o is not None:
            assert torch.isnan(o[G * N:]).all(), "wrote past the last node row"
        res.append(None if o is None else o[:G * N].cpu())
    return res[0], res[1], kernel


def readout_bwd_inputs(G, N, R, H, how, normal=False):
    deg = 3
    gen = torch.Generator().manual_seed(1000 * N + 10 * R + H)
    nbr = sym_table(G, N, deg, seed=N + R + H)
    an = None if how == "sym" else agent_map(G, N, R, seed=R + H)
    shape = (G, R, deg + 1, H)
    dout = torch.randn(shape, generator=gen) if normal else dyadic(shape, gen)
    W = (deg + 1) * H
    stride = W + (1 if how == "map+odd" else pad_of(H))
    return dout, nbr, an, stride


@gpu
@pytest.mark.parametrize("kernel,G,N,R,H,how", cases("readout_bwd"))
def test_readout_bwd_paths(kernel, G, N, R, H, how):
    """dh_final only, dh_prev only and both, bit-equal to the fp64 scatter; never-read nodes exactly zero."""
    dout, nbr, an, stride = readout_bwd_inputs(G, N, R, H, how)
    rf, rp, readf, readp = readout_bwd_ref(dout, nbr, an)
    assert not readp.all() and (an is None or not readf.all())  # some node is never read
    for which in ("f", "p", "fp"):
        of, op, ran = run_readout_bwd(dout, nbr, an, H, which, stride, sym=how == "sym")
        assert ran == kernel, (ran, which)
        if of is not None:
            assert torch.equal(of, rf.float()), which
            assert (of[~readf] == 0).all()
        if op is not None:
            assert torch.equal(op, rp.float()), which
            assert (op[~readp] == 0).all()


@gpu
@pytest.mark.parametrize("kernel", ["k_readout_bwd_nodes<unsigned>", "k_readout_bwd_cs<2>/S=4", "k_readout_bwd_lds",
                                    "k_readout_bwd_g<4>", "k_readout_bwd<4>"])
def test_readout_bwd_summation_order(kernel):
    """One kernel of every family on random normal gradients: bit-equal to the fp32 sum taken in ascending
    (row, segment) order (ascending neighbour lists), the order each kernel's comment claims."""
    G, N, R, H, how = CASES[kernel][1][0]
    dout, nbr, an, stride = readout_bwd_inputs(G, N, R, H, how, normal=True)
    rf, rp = readout_bwd_ordered_f32(dout, nbr, an)
    of, op, ran = run_readout_bwd(dout, nbr, an, H, "fp", stride, sym=how == "sym")
    assert ran == kernel
    assert torch.equal(of, rf) and torch.equal(op, rp)


def _directed_tables(G, N, seed):
    """dense_to_nbr of a directed adjacency (up to 3 out-neighbours per node): an asymmetric table"""
    M = importlib.import_module("graph-marl_amd.model")
    gen = torch.Generator().manual_seed(seed)
    mask = torch.eye(N).repeat(G, 1, 1)
    for b in range(G):
        for n in range(N):
            k = int(torch.randint(0, 4, (1,), generator=gen))
            for v in torch.randperm(N, generator=gen)[:k].tolist():
                mask[b, n, v] = 1.0
    nbr = M.dense_to_nbr(mask.cuda(), max_degree=3).cpu()
    adj = mask.bool() & ~torch.eye(N, dtype=torch.bool)
    assert not torch.equal(adj, adj.transpose(1, 2))
    return nbr


@gpu
@pytest.mark.parametrize("table", ["symmetric_unsorted", "asymmetric"])
def test_readout_bwd_without_map_takes_any_table(table):
    """The contract of gm_netmon_readout_bwd: correct for ANY neighbour table, also without an agent map. The
    gather kernel k_readout_bwd_nodes is only correct on symmetric tables without repeated entries, so only
    gm_netmon_readout_bwd_sym (the caller vouches for its tables) may launch it; it takes unsorted symmetric
    tables too. The asymmetric table also goes through the public autograd op model.netmon_readout(...,
    agent_node=None), which hands the library whatever dense_to_nbr produced."""
    G, N, H, deg = 3, 10, 8, 3
    gen = torch.Generator().manual_seed(5)
    nbr = sym_table(G, N, deg, seed=9, shuffle=True) if table == "symmetric_unsorted" else _directed_tables(G, N, 9)
    dout = dyadic((G, N, deg + 1, H), gen)
    rf, rp, _, _ = readout_bwd_ref(dout, nbr, None)
    of, op, ran = run_readout_bwd(dout, nbr, None, H, "fp", (deg + 1) * H)
    print(f"{table}: {ran}, max |dh_prev - ref| = {(op.double() - rp).abs().max().item()}")
    assert ran == "k_readout_bwd_lds"  # not the gather
    assert torch.equal(of, rf.float()) and torch.equal(op, rp.float())
    if table == "symmetric_unsorted":
        of, op, ran = run_readout_bwd(dout, nbr, None, H, "fp", (deg + 1) * H, sym=True)
        assert ran == "k_readout_bwd_nodes<unsigned>"
        assert torch.equal(of, rf.float()) and torch.equal(op, rp.float())
    else:
        M = importlib.import_module("graph-marl_amd.model")
        hf = torch.zeros(G * N, H, device="cuda", requires_grad=True)
        hp = torch.zeros(G * N, H, device="cuda", requires_grad=True)
        M.netmon_readout(hf, hp, nbr.cuda(), None).backward(dout.reshape(G * N, -1).cuda())
        assert torch.equal(hf.grad.cpu(), rf.float()) and torch.equal(hp.grad.cpu(), rp.float())


@gpu
def test_config5_unroll_still_takes_the_gather_kernel(monkeypatch):
    """The supervised driver's sequence-batched unroll (sl_seq.py, config 5) knows its tables are the routing
    env's and opts in: its readout backward reports k_readout_bwd_nodes through the hook."""
    SL = importlib.import_module("graph-marl_amd.sl")
    import argparse

    L = lib()
    n, H = 20, 32
    args = argparse.Namespace(netmon_dim=H, netmon_encoder_dim="64,48", netmon_iterations=1, netmon_rnn_type="lstm",
                              netmon_rnn_carryover=1, netmon_agg_type="sum", netmon_last_neighbors=1,
                              netmon_global=False, num_targets=n)
    torch.manual_seed(0)
    model = SL.NetMonSL(args, 4 * n + 8, 4, n).cuda()
    assert SL.SQ.seq_ok(model.netmon)
    data = SL.build_dataset(n, 20, 4, 7)
    ran = []
    real = L.lib().gm_netmon_readout_bwd_sym

    def spy(*a):
        rc = real(*a)
        ran.append(L.last_kernel())  # same thread as the call (autograd's backward thread)
        return rc

    monkeypatch.setattr(L.lib(), "gm_netmon_readout_bwd_sym", spy)
    model.netmon.state = None
    pred = model.forward_seq(data.node_obs, data.nbr, 2)
    (pred - data.targets_all).pow(2).mean().backward()
    assert ran == ["k_readout_bwd_nodes<unsigned>"] * 2


# ---------------------------------------------------------------------------------------------------------
# readout forward
# ---------------------------------------------------------------------------------------------------------
# (G, N, R or None = no map, deg): G R % 4 = 1, 2, 3, 2, 0; deg 5 at H >= 128: more tail columns
READOUT_SHAPES = [(3, 10, 7, 3), (2, 10, 7, 3), (3, 10, 5, 3), (3, 10, None, 3), (2, 10, None, 3), (3, 10, 7, 5)]


@gpu
@pytest.mark.parametrize("G,N,R,deg", READOUT_SHAPES)
@pytest.mark.parametrize("kernel,H", cases("readout_fwd"))
def test_readout_fwd_paths(kernel, H, G, N, R, deg):
    """gm_netmon_readout_ld on [h | c] rows (ldf = ldp = 2H, the c half NaN) into rows wider than (deg + 1) H:
    a pure copy, bit-equal; -1 neighbours read as zeros; four rows per wave iteration with the last group
    clamped (rows % 4 of every kind)."""
    L = lib()
    gen = torch.Generator().manual_seed(H + G + (R or 0) + deg)
    nbr = sym_table(G, N, deg, seed=H + deg)
    an = None if R is None else agent_map(G, N, R, seed=H)
    R = R or N
    hf, hp = dyadic((G * N, H), gen), dyadic((G * N, H), gen)
    W = (deg + 1) * H
    stride = W + pad_of(H)
    fbuf, pbuf = padded(hf, 2 * H), padded(hp, 2 * H)
    out = torch.full((G * R + 1, stride), float("nan"), device="cuda")
    nb, a = nbr.cuda(), None if an is None else an.cuda()
    L.check(L.lib().gm_netmon_readout_ld(fbuf.data_ptr(), 2 * H, pbuf.data_ptr(), 2 * H, nb.data_ptr(), L.ptr(a), G, N,
                                         R, deg, H, out.data_ptr(), stride, L.stream_ptr()))
    assert L.last_kernel() == kernel
    u = (torch.arange(N).expand(G, N) if an is None else an).long()
    nbu = torch.gather(nbr.long(), 1, u.unsqueeze(-1).expand(G, R, deg))
    hpz = torch.cat([hp.view(G, N, H), torch.zeros(G, 1, H)], 1)  # index N = the zero row of a -1 neighbour
    segs = [torch.gather(hf.view(G, N, H), 1, u.unsqueeze(-1).expand(G, R, H))]
    for k in range(deg):
        idx = torch.where(nbu[..., k] >= 0, nbu[..., k], torch.full_like(nbu[..., k], N))
        segs.append(torch.gather(hpz, 1, idx.unsqueeze(-1).expand(G, R, H)))
    ref = torch.cat(segs, -1).reshape(G * R, W)
    o = out.cpu()
    assert torch.equal(o[:G * R, :W], ref)
    assert torch.isnan(o[:G * R, W:]).all() and torch.isnan(o[G * R:]).all()


# ---------------------------------------------------------------------------------------------------------
# aggregate
# ---------------------------------------------------------------------------------------------------------
def aggregate_ref(x, nbr, mode, bwd):
    """fp64 on the CPU, x [G * N, H]: forward out[n] = sum over {n} u nbr(n) of x (/ count for mean); backward
    the transpose dh[j] = sum over the n that hold j of x[n] (/ count(n)), as a scatter: no symmetry assumed.
    Returns the result, the sum of |terms| per output, the member counts and the sum before the mean's division."""
    G, N, deg = nbr.shape
    H = x.shape[1]
    rows = torch.arange(G * N)
    off = (rows // N * N).view(-1, 1)
    nb = nbr.long().view(G * N, deg)
    ok = nb >= 0
    cnt = (1 + ok.sum(-1)).double().view(-1, 1)
    owner = torch.cat([rows, rows.view(-1, 1).expand(-1, deg)[ok]])  # the row n of every (n, member) pair
    member = torch.cat([rows, (off + nb)[ok]])
    d = x.double()
    out, mag = torch.zeros(G * N, H, dtype=torch.float64), torch.zeros(G * N, H, dtype=torch.float64)
    if not bwd:
        out.index_add_(0, owner, d[member])
        mag.index_add_(0, owner, d[member].abs())
        total = out
        if mode == 1:
            out, mag = out / cnt, mag / cnt
    else:
        t = d / cnt if mode == 1 else d
        out.index_add_(0, member, t[owner])
        mag.index_add_(0, member, t[owner].abs())
        total = out
    return out, mag, cnt, total


@gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kernel,direction,deg,H", cases("aggregate"))
def test_aggregate_paths(kernel, direction, deg, H, mode):
    """Symmetric ascending tables with -1 padding, every vector width and degree. Sum (both directions): exact on
    dyadic inputs, bit-equal. Mean forward: the exact sum divided by the count as an fp32 tensor division,
    bit-equal. Mean backward: each term x * (1 / count) is rounded twice and at most deg + 1 terms are summed:
    within (deg + 3) 2^-24 sum |terms| of fp64. Forward rows are the h half of [h | c] rows (ldh = 2H) into a
    padded output (ldo > H); the backward entry point is contiguous."""
    L = lib()
    G, N = 3, 10
    gen = torch.Generator().manual_seed(100 * deg + H + mode)
    nbr = sym_table(G, N, deg, seed=deg + H)
    x = dyadic((G * N, H), gen)
    bwd = direction == "bwd"
    ref, mag, cnt, total = aggregate_ref(x, nbr, mode, bwd)
    nb = nbr.cuda()
    if bwd:
        xb = x.cuda()
        out = torch.full((G * N + 1, H), float("nan"), device="cuda")
        L.check(L.lib().gm_mp_aggregate_bwd(xb.data_ptr(), nb.data_ptr(), G, N, deg, H, mode, out.data_ptr(),
                                            L.stream_ptr()))
    else:
        xb = padded(x, 2 * H)
        out = torch.full((G * N + 1, H + pad_of(H)), float("nan"), device="cuda")
        L.check(L.lib().gm_mp_aggregate_rows(xb.data_ptr(), 2 * H, nb.data_ptr(), G, N, deg, H, mode, out.data_ptr(),
                                             out.stride(0), L.stream_ptr()))
    assert L.last_kernel() == kernel
    o = out.cpu()
    assert torch.isnan(o[:G * N, H:]).all() and torch.isnan(o[G * N:]).all()
    o = o[:G * N, :H]
    if mode == 0:
        assert torch.equal(o, ref.float())
    elif not bwd:
        exact_sum = total.float()  # the dyadic sum, exact in fp32
        assert torch.equal(exact_sum.double(), total)
        assert torch.equal(o, exact_sum / cnt.float().expand(-1, H))
    else:
        err = (o.double() - ref).abs()
        assert (err <= (deg + 3) * 2.0 ** -24 * mag).all(), (err - (deg + 3) * 2.0 ** -24 * mag).max().item()


@gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_aggregate_member_order_contract(mode):
    """The contract: neighbour lists in ascending id order (as dense_to_nbr writes them) are required for
    bit-equality with the dense (I + A) product, whose row sum runs over ascending node ids. k_mp_aggregate3 sorts
    its members, the general kernel (members()) keeps the list order with the node itself slotted in, so on an
    ascending table the two agree bit for bit, and on an unsorted table they may differ by fp32 reassociation
    only: both stay within 4 * 2^-24 * sum |terms| of fp64 (at most 4 terms, 3 roundings, + 1 for the mean's
    division)."""
    L = lib()
    G, N, H = 3, 10, 128
    gen = torch.Generator().manual_seed(mode)
    x = torch.randn(G * N, H, generator=gen)
    res = {}
    for order in ("ascending", "unsorted"):
        nbr3 = sym_table(G, N, 3, seed=4, shuffle=order == "unsorted")
        nbr4 = torch.cat([nbr3, torch.full((G, N, 1), -1, dtype=torch.int32)], -1).contiguous()
        ref, mag, _, _ = aggregate_ref(x, nbr3, mode, False)
        for nbr, kernel in ((nbr3, "k_mp_aggregate3<4>"), (nbr4, "k_mp_aggregate<fwd,4>")):
            out = torch.full((G * N, H), float("nan"), device="cuda")
            xb, nb = x.cuda(), nbr.cuda()
            L.check(L.lib().gm_mp_aggregate(xb.data_ptr(), nb.data_ptr(), G, N, nbr.shape[-1], H, mode, out.data_ptr(),
                                            L.stream_ptr()))
            assert L.last_kernel() == kernel
            res[order, kernel] = out.cpu()
            assert ((out.cpu().double() - ref).abs() <= 4 * 2.0 ** -24 * mag).all(), (order, kernel)
    assert torch.equal(res["ascending", "k_mp_aggregate3<4>"], res["ascending", "k_mp_aggregate<fwd,4>"])


# ---------------------------------------------------------------------------------------------------------
# LSTM cell backward and Q-head backward: the reference construction and tolerances of test_train_seq_gpu.py
# ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("kernel,H,dg_pad", cases("lstm_cell_bwd"))
def test_lstm_cell_bwd_paths(kernel, H, dg_pad, mean):
    """m = 130 rows (13 graphs of 10 nodes): the last 64-row block holds 2 rows. H = 96: H % 4 == 0 but 10 row
    lanes x 24 threads are no whole waves -> scalar kernel with 2 x 96 threads; H = 320: one row lane of 320
    threads; H = 512: the vector kernel with 2 x 128 threads; ld_dg = 4H + 1: misaligned gate-gradient rows
    force the scalar kernel at H = 128."""
    from test_train_seq_gpu import lstm_cell_bwd_case

    B, N = 13, 10
    lstm_cell_bwd_case(sym_table(B, N, 3, seed=H).cuda(), B, N, H, mean, ld_dg=4 * H + dg_pad)
    assert lib().last_kernel() == kernel


@gpu
@pytest.mark.parametrize("kernel,cols,nq", cases("qhead_bwd"))
def test_qhead_bwd_paths(kernel, cols, nq):
    """cols = 1024: the widest layer, one row lane of 256 threads x 4 columns; cols = 260: 65 column quads are no
    whole waves -> scalar kernel with 320 threads (60 idle); rows = 130."""
    from test_train_seq_gpu import qhead_bwd_case

    qhead_bwd_case(130, cols, nq)
    assert lib().last_kernel() == kernel
