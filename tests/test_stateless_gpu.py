"""The stateless NetMon (--netmon-rnn-type none) on the GPU: gm_mp_iterate / gm_mp_iterate_bwd bit for bit against
the chained per-round launches and against fp64, their argument checks, NetMon.forward_graph against the reference's
golden outputs, the fused rollout against the unfused wrapper (eager, stream groups, graph replay), the per-step
and the sequence-batched update against the reference's golden updates and against each other, a reference-written checkpoint and a CLI training run."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import golden_update as GU
from test_netmon_paths_gpu import sym_table

pytestmark = pytest.mark.gpu
GOLDEN = GU.GOLDEN


def mods():
    names = ("", ".model", ".fused", ".wrapper", ".policy", ".rollout", "._lib")
    return tuple(importlib.import_module("graph-marl_amd" + n) for n in names)


def leaky_rows(rows, cols, seed):
    """Rows as the encoder hands them over: leaky_relu(0.01) of normal values (mostly positive, a few small
    negatives), so K rounds of sums grow like the product's and the fp64 bounds below are relative to that growth."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    return torch.where(x > 0, x, 0.01 * x).cuda()


def dense_p(nbr, mode):
    """fp64 aggregation operator [G, N, N] of a neighbour table: I + A, row-normalised for mean."""
    G, N, deg = nbr.shape
    P = torch.eye(N, dtype=torch.float64).repeat(G, 1, 1)
    for k in range(deg):
        col = nbr[..., k].long()
        ok = col >= 0
        P[torch.nonzero(ok, as_tuple=True) + (col[ok],)] = 1.0
    if mode == 1:
        P = P / P.sum(-1, keepdim=True).clamp(min=1)
    return P


@pytest.fixture
def iterate_form():
    """Sets gm_mp_iterate's form for a test and restores the per-shape default."""
    L = importlib.import_module("graph-marl_amd._lib")
    yield lambda f: L.check(L.lib().gm_mp_iterate_set_form(f))
    L.lib().gm_mp_iterate_set_form(-1)


def strided(x, ld):
    """x [rows, H] in the first H columns of NaN-filled rows of width ld."""
    buf = torch.full((x.shape[0], ld), float("nan"), device="cuda")
    buf[:, :x.shape[1]] = x
    return buf


# (N, H, deg, LDS-eligible): the issue's grid, N = 150 at H = 128 (157 KB of the 160 KB a block may take), the two
# fallback shapes (H = 18: rows that are no 16-byte lanes; N = 200, H = 128: 205 KB of images), H = 20 (16-byte
# lanes of 5 per row: 255-thread blocks) and a degree-5 table
SHAPES = [(6, 32, 3, True), (6, 128, 3, True), (20, 32, 3, True), (20, 128, 3, True), (100, 32, 3, True),
          (100, 128, 3, True), (150, 128, 3, True), (20, 20, 3, True), (20, 64, 5, True), (20, 18, 3, False),
          (200, 128, 3, False)]


def block_lds_bytes(N, H, deg):
    """LDS of one block of the LDS form, restated from its layout: gpb graphs (packed until 256 lanes are busy,
    within 40 KB), each two [N, P] fp32 images, the member lists and two words per node."""
    per = N * (2 * (H if H % 64 == 0 else H + 4) * 4 + (deg + 1) * 4 + 8)
    gpb = 1
    while gpb < 16 and gpb * N * (H // 4) < 256 and (gpb + 1) * per <= 40 * 1024:
        gpb += 1
    return gpb * per


def chain_fwd(L, x, nbr, mode, K):
    G, N, deg = nbr.shape
    H = x.shape[1]
    h, prev = x.clone(), torch.zeros_like(x)
    for _ in range(K):
        nxt = torch.empty_like(h)
        L.check(L.lib().gm_mp_aggregate_rows(h.data_ptr(), H, nbr.data_ptr(), G, N, deg, H, mode, nxt.data_ptr(), H,
                                             L.stream_ptr()))
        prev, h = h, nxt
    return h, prev


@pytest.mark.parametrize("N,H,deg,lds", SHAPES)
def test_mp_iterate_bit_identical_to_chained_launches(N, H, deg, lds, iterate_form):
    gm, M, FU, W, P, RO, L = mods()
    G = 3
    nbr = sym_table(G, N, deg, seed=N + H).cuda()
    small = block_lds_bytes(N, H, deg) <= 40 * 1024  # K = 1 runs the LDS form by default in this class only
    x = leaky_rows(G * N, H, seed=N * H)
    for mode in (0, 1):
        Pm = dense_p(nbr.cpu(), mode)
        for K in (0, 1, 2, 3, 8):
            ref_out, ref_prev = chain_fwd(L, x, nbr, mode, K)
            h64, p64 = x.double().cpu().view(G, N, H), torch.zeros(G, N, H, dtype=torch.float64)
            for _ in range(K):
                p64, h64 = h64, Pm @ h64
            for form, ld in ((1, 2 * H), (1, H), (-1, 2 * H)):
                iterate_form(form)
                xin = strided(x, ld)
                out = torch.full((G * N, ld), float("nan"), device="cuda")
                prev = torch.full((G * N, ld), float("nan"), device="cuda")
                L.check(L.lib().gm_mp_iterate(xin.data_ptr(), ld, nbr.data_ptr(), G, N, deg, H, mode, K, out.data_ptr(),
                                              ld, prev.data_ptr(), ld, L.stream_ptr()))
                what = (mode, K, form, ld)
                if K >= 1:
                    assert (L.last_kernel() == "k_mp_iterate<fwd>") == (lds and (form == 1 or K >= 2 or small)), what
                assert torch.equal(out[:, :H], ref_out), what
                assert torch.equal(prev[:, :H], ref_prev), what
                assert torch.isnan(out[:, H:]).all() and torch.isnan(prev[:, H:]).all(), what
                assert torch.equal(xin[:, :H], x) and torch.isnan(xin[:, H:]).all(), what
            for got, ref in ((ref_out, h64), (ref_prev, p64)):
                bound = 1e-6 * max(1.0, ref.abs().max().item())
                assert (got.double().cpu().view(G, N, H) - ref).abs().max().item() <= bound, (mode, K)
    # K = 0 takes a NULL prev
    out = torch.empty_like(x)
    L.check(L.lib().gm_mp_iterate(x.data_ptr(), H, nbr.data_ptr(), G, N, deg, H, 0, 0, out.data_ptr(), H, None, 0,
                                  L.stream_ptr()))
    assert torch.equal(out, x)


def chain_bwd(L, dy, dz, nbr, mode, K):
    G, N, deg = nbr.shape
    H = dy.shape[1]
    g = dy.clone()
    for r in range(K):
        nxt = torch.empty_like(g)
        L.check(L.lib().gm_mp_aggregate_bwd(g.data_ptr(), nbr.data_ptr(), G, N, deg, H, mode, nxt.data_ptr(),
                                            L.stream_ptr()))
        g = nxt + dz if r == 0 else nxt
    return g


@pytest.mark.parametrize("N,H,deg,lds", SHAPES)
def test_mp_iterate_bwd_bit_identical_and_adjoint(N, H, deg, lds, iterate_form):
    """Chained gm_mp_aggregate_bwd + the add, bit for bit; and <h_K(x), y> + <h_{K-1}(x), z> = <x, bwd(y, z)>
    in fp64 within 1e-5 relative (x, y, z mostly positive: the products do not cancel)."""
    gm, M, FU, W, P, RO, L = mods()
    G = 3
    nbr = sym_table(G, N, deg, seed=N + H + 1).cuda()
    small = block_lds_bytes(N, H, deg) <= 40 * 1024
    x, y, z = (leaky_rows(G * N, H, seed=N * H + i) for i in range(3))
    for mode in (0, 1):
        for K in (0, 1, 3, 8):
            ref = chain_bwd(L, y, z, nbr, mode, K)
            for form, ld in ((1, 2 * H), (1, H), (-1, 2 * H)):
                iterate_form(form)
                yin, zin = strided(y, ld), strided(z, ld)
                dh = torch.full((G * N, ld), float("nan"), device="cuda")
                L.check(L.lib().gm_mp_iterate_bwd(yin.data_ptr(), ld, zin.data_ptr(), ld, nbr.data_ptr(), G, N, deg, H,
                                                  mode, K, dh.data_ptr(), ld, L.stream_ptr()))
                what = (mode, K, form, ld)
                if K >= 1:
                    assert (L.last_kernel() == "k_mp_iterate<bwd>") == (lds and (form == 1 or K >= 2 or small)), what
                assert torch.equal(dh[:, :H], ref), what
                assert torch.isnan(dh[:, H:]).all(), what
            out, prev = chain_fwd(L, x, nbr, mode, K)
            lhs = (out.double() * y.double()).sum().item() + (prev.double() * z.double()).sum().item()
            rhs = (x.double() * ref.double()).sum().item()
            assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (mode, K, lhs, rhs)
    # no gradient on h_{K-1}: NULL d_prev is the chain without the add
    iterate_form(1)
    dh = torch.empty_like(y)
    L.check(L.lib().gm_mp_iterate_bwd(y.data_ptr(), H, None, 0, nbr.data_ptr(), G, N, deg, H, 1, 3, dh.data_ptr(), H,
                                      L.stream_ptr()))
    assert torch.equal(dh, chain_bwd(L, y, torch.zeros_like(z), nbr, 1, 3))


def test_mp_iterate_partial_block_and_autograd(iterate_form):
    """7 graphs of 6 nodes at H = 32 pack 6 to a block: the second block holds one. And the autograd node
    (model.mp_iterate) against the chained autograd nodes, with and without a gradient on h_{K-1}."""
    gm, M, FU, W, P, RO, L = mods()
    G, N, H, K = 7, 6, 32, 3
    nbr = sym_table(G, N, 3, seed=9).cuda()
    x = leaky_rows(G * N, H, seed=4)
    for mode in (0, 1):
        ref_out, ref_prev = chain_fwd(L, x, nbr, mode, K)
        a = x.clone().requires_grad_(True)
        out, prev = M.mp_iterate(a, nbr, mode, K)
        assert L.last_kernel() == "k_mp_iterate<fwd>"
        assert torch.equal(out, ref_out) and torch.equal(prev, ref_prev)
        b = x.clone().requires_grad_(True)
        hs = [b]
        for _ in range(K):
            hs.append(M.mp_aggregate(hs[-1], nbr, mode))
        gy, gz = leaky_rows(G * N, H, 5), leaky_rows(G * N, H, 6)
        (out * gy).sum().backward(retain_graph=True)
        (hs[-1] * gy).sum().backward(retain_graph=True)
        assert torch.equal(a.grad, b.grad)
        a.grad = b.grad = None
        ((out * gy).sum() + (prev * gz).sum()).backward()
        ((hs[-1] * gy).sum() + (hs[-2] * gz).sum()).backward()
        torch.testing.assert_close(a.grad, b.grad, rtol=1e-6, atol=1e-6)  # autograd adds the two branches elsewhere


def test_mp_iterate_argument_errors():
    """Every refusal comes before any launch. The buffers are real device allocations of the default shape, so a
    check that regressed would fail an assertion here, not touch unmapped memory."""
    gm, M, FU, W, P, RO, L = mods()
    lib, vp = L.lib(), ctypes.c_void_p
    bufs = [torch.zeros(3 * 6, 32, device="cuda") for _ in range(3)]
    table = sym_table(3, 6, 3, seed=1).cuda()
    a, b, c = (vp(x.data_ptr()) for x in bufs)
    t = vp(table.data_ptr())

    def fwd(h0=a, ld0=32, G=3, N=6, deg=3, H=32, mode=0, K=2, out=b, ldo=32, prev=c, ldp=32):
        return lib.gm_mp_iterate(h0, ld0, t, G, N, deg, H, mode, K, out, ldo, prev, ldp, None)

    def bwd(dy=a, ldd=32, dz=b, ldq=32, G=3, N=6, deg=3, H=32, mode=0, K=2, dh=c, ld=32):
        return lib.gm_mp_iterate_bwd(dy, ldd, dz, ldq, t, G, N, deg, H, mode, K, dh, ld, None)

    for f, name in ((fwd, b"gm_mp_iterate:"), (bwd, b"gm_mp_iterate_bwd:")):
        for bad in (dict(K=-1), dict(N=65537), dict(N=0), dict(G=0), dict(deg=9), dict(H=0), dict(mode=2)):
            assert f(**bad) != 0, bad
            assert name in lib.gm_last_error(), (bad, lib.gm_last_error())
    assert fwd(prev=None) != 0 and b"prev" in lib.gm_last_error()
    assert fwd(K=-3) != 0 and b"iters" in lib.gm_last_error()
    for bad in (dict(h0=None), dict(out=None), dict(ld0=31), dict(ldo=16), dict(ldp=8), dict(out=a), dict(prev=a),
                dict(prev=b)):
        assert fwd(**bad) != 0, bad
    for bad in (dict(dy=None), dict(dh=None), dict(ldd=31), dict(ld=16), dict(ldq=8), dict(dh=a), dict(dh=b)):
        assert bwd(**bad) != 0, bad
    assert lib.gm_mp_iterate_set_form(2) != 0 and lib.gm_mp_iterate_set_form(-1) == 0


def _golden_netmon(M, g, vi):
    rnn, agg, K, H, enc, glob = str(g["variants"][vi]).split("|")
    nm = M.NetMon(g["node_obs"].shape[-1], int(H), [int(e) for e in enc.split(",")], int(K), rnn_type=rnn,
                  agg_type=agg, output_global_hidden=bool(int(glob))).cuda()
    nm.load_state_dict({k[len(f"v{vi}_w_"):]: torch.as_tensor(g[k]) for k in g.files if k.startswith(f"v{vi}_w_")})
    return nm


def close(actual, ref, what, rel=1e-5):
    ref = np.asarray(ref, np.float64)
    bound = rel * max(1.0, np.abs(ref).max())
    err = np.abs(actual.detach().double().cpu().numpy() - ref).max()
    assert err <= bound, f"{what}: {err} > {bound}"


@pytest.mark.parametrize("vi", range(5))
def test_stateless_forward_vs_reference_golden(vi):
    gm, M, FU, W, P, RO, L = mods()
    g = np.load(os.path.join(GOLDEN, "netmon_stateless.npz"))
    nm = _golden_netmon(M, g, vi)
    with torch.no_grad():
        for t in range(3):
            x = torch.as_tensor(g["node_obs"][t], device="cuda")
            m = torch.as_tensor(g["node_adj"][t], device="cuda").float()
            na = torch.as_tensor(g["node_agent"][t], device="cuda").float()
            h = nm(x, m, na, no_agent_mapping=True)
            close(h, g[f"v{vi}_h_{t}"], f"h step {t}")
            close(nm.state, g[f"v{vi}_state_{t}"], f"state step {t}")
            close(nm(x, m, na), g[f"v{vi}_mapped_{t}"], f"mapped step {t}")
            # the fused step: state rows and the readout gathered from its two tables
            nbr, an = M.dense_to_nbr(m), M.node_agent_to_index(na)
            state, hprev = FU.netmon_step(nm, x, nbr, None)
            close(state, g[f"v{vi}_state_{t}"], f"fused state step {t}")
            B, N, H = state.shape
            ro = M.netmon_readout(state.reshape(B * N, H), hprev, nbr, an).view(B, -1, 4 * H)
            ref = g[f"v{vi}_mapped_{t}"]
            if nm.output_global_hidden:
                ref = np.concatenate([ref[..., :H], ref[..., 2 * H:]], -1)
            close(ro, ref, f"fused readout step {t}")


def _wrapped(fused, agg, K, glob, B=64, seed=5):
    gm, M, FU, W, P, RO, L = mods()
    N, A, H = 20, 20, 128
    gw = (5 if glob else 4) * H
    env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A, n_env=B, seed=seed,
                     obs_extra=gw, agent_adjacency=False)
    torch.manual_seed(1)
    nm = M.NetMon(4 * N + 8, H, [512, 256], K, rnn_type="none", agg_type=agg, output_global_hidden=glob).cuda()
    return env, nm, W.NetMonWrapper(env, nm, 2, fused=fused), gw


@pytest.mark.parametrize("agg,K,glob", [("mean", 3, False), ("sum", 8, False), ("mean", 3, True)])
def test_fused_stateless_rollout_matches_unfused(agg, K, glob):
    """64 envs x 12 steps with a reset after step 6 (2 start-up NetMon steps each, idempotent here): the fused
    wrapper's materialised observation against the unfused wrapper's, the same ε-greedy actions from either, and a
    launch trace with one gm_mp_iterate per NetMon step and no per-round aggregate."""
    gm, M, FU, W, P, RO, L = mods()
    e1, nm1, w1, gw = _wrapped(True, agg, K, glob)
    e2, nm2, w2, _ = _wrapped(False, agg, K, glob)
    assert FU.fused_ok(nm1) and w1.fused and not w2.fused
    torch.manual_seed(2)
    dqn = M.DQN(e1.obs_dim + gw, [512, 256], 4).cuda()
    p1 = P.EpsilonGreedy(w1, dqn, epsilon=0.5, epsilon_decay=1.0, step_before_train=0)
    p2 = P.EpsilonGreedy(w2, dqn, epsilon=0.5, epsilon_decay=1.0, step_before_train=0)
    L.TRACE = trace = []
    try:
        w1.reset()
        w2.reset()
        for t in range(12):
            if t == 6:
                w1.reset()
                w2.reset()
            # the fused road first (readout gathered in the DQN's first GEMM), then the materialised observation
            q1 = p1._fused_q(w1).view(e1.n_env, e1.n_data, -1).clone()
            o1, o2 = w1.obs, w2.obs
            close(o1, o2.cpu().numpy(), f"obs step {t}")
            q2 = p2.q_values(o2)
            close(q1, q2.cpu().numpy(), f"q step {t}")
            a1 = p1.select(q1).clone()
            a2 = p2.select(q2).clone()
            assert torch.equal(a1, a2), f"actions differ at step {t}"
            w1.step_(a1)
            w2.step_(a2)
            close(w1.current_netmon_state, w2.current_netmon_state.cpu().numpy(), f"state step {t}")
        close(w1.obs, w2.obs.cpu().numpy(), "last obs")
    finally:
        L.TRACE = None
    fused_tags = [t for t in trace if t.startswith("mp_")]
    assert any(t.startswith("mp_iterate:") for t in fused_tags)
    # the unfused wrapper runs the autograd node's forward: gm_mp_iterate as well, never the per-round launches
    assert not any(t.startswith("mp_aggregate") for t in fused_tags), fused_tags


def test_stateless_streamed_rollout_graph_replay_dqn():
    """DQN, 2 stream groups, per-group graphs of 2 steps replayed across resets == the eager run, bit for bit."""
    import test_rollout_gpu as TR

    gm, M, FU, W, P, RO, L = mods()
    N, A = TR.N, TR.A

    def build():
        net = gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS, device=0)
        torch.manual_seed(3)
        nm = M.NetMon(4 * N + 8, 128, [512, 256], 8, rnn_type="none").cuda()
        dqn = M.DQN(6 * N + 10 + 512, [512, 256], 4).cuda()
        return RO.StreamedRollout(net, A, 8, nm, dqn, groups=2, seed=0, epsilon=0.3, episode_steps=10, device=0)

    eager = build()
    eager.reset()
    eager.run(24)
    ref = TR.snapshot(eager)
    ro = build()
    ro.reset()
    for _ in range(4):
        ro.step()
    ro.capture(2, per_group=True)
    ro.run(20)
    assert ro._graphs is not None and len(ro._graphs) == 2
    for a, b in zip(TR.snapshot(ro), ref):
        TR.assert_same(a, b)


def test_stateless_streamed_rollout_graph_replay_dgn():
    """DGN on the fused agent road (readout gathered in the first encoder GEMM) over a stateless NetMon."""
    import test_agent_rollout_gpu as TA

    gm, M, FU, W, P, RO, L = mods()
    torch.manual_seed(3)
    nm = M.NetMon(4 * TA.N + 8, TA.H_S, [64, 32], 3, rnn_type="none", agg_type="mean").cuda()
    model = TA.make_model(M, "dgn", 6 * TA.N + 10 + 4 * TA.H_S, (48, 32)).cuda()
    eager = TA.build_ro("dgn", 2, shared=(nm, model))
    eager.reset()
    eager.run(20)
    ref = TA.snapshot(eager)
    ro = TA.build_ro("dgn", 2, shared=(nm, model))
    ro.reset()
    ro.run(4)
    ro.capture(4, per_group=True)
    ro.run(16)
    assert ro._graphs is not None and len(ro._graphs) == 2
    for a, b in zip(TA.snapshot(ro), ref):
        TA.assert_same(a, b)


@pytest.mark.parametrize("path", ["per_step", "seq"])
@pytest.mark.parametrize("name", ["train_stateless.npz", "train_stateless_l1.npz"])
def test_stateless_update_matches_reference_golden(name, path):
    """The per-step update (train.dqn_loss on NetMon.forward_graph: _MpIterate forward and backward) and the
    sequence-batched update (stateless_seq.seq_loss: all L steps as one batch) against the
    reference's update of a stateless NetMon + DQN: Q, targets, loss, gradients, AdamW step and the soft target
    update at test_train_gpu's tolerances, the absolute ones scaled by max(1, max|ref|) (sum aggregation at
    K = 8 grows the rows about 4^K)."""
    import test_train_gpu as TT

    M, T, RB = TT.mods()
    g = np.load(os.path.join(GOLDEN, name))
    dev = torch.device("cuda")
    netmon, model, target, state0 = GU.build(g, M, dev)
    assert netmon.rnn_type == "none"
    batches = TT.golden_batches(g, M, RB, dev, state0)
    params = list(model.parameters()) + list(netmon.parameters())
    names = [f"model_{k}" for k, _ in model.named_parameters()] + [f"netmon_{k}" for k, _ in netmon.named_parameters()]
    assert names == list(g["param_names"])
    opt = torch.optim.AdamW(params, lr=float(g["lr"]))
    netmon.train()
    model.train()
    if path == "seq":
        from test_train_seq_gpu import _golden_seq

        SS = importlib.import_module("graph-marl_amd.stateless_seq")
        assert SS.stateless_seq_ok(netmon, model, target)
        seq = _golden_seq(g, dev, netmon, RB, state0)
        loss, qs, qts = SS.seq_loss(netmon, model, target, seq, float(g["gamma"]))
    else:
        loss, qs, qts = T.dqn_loss(netmon, model, target, batches, float(g["gamma"]))
    for t in range(len(batches)):
        close(qs[t], g[f"q_{t}"], f"q_{t}")
        close(qts[t], g[f"qtarget_{t}"], f"qtarget_{t}")
    np.testing.assert_allclose(loss.item(), g["loss"].item(), rtol=1e-5, atol=1e-6)
    opt.zero_grad()
    loss.backward()
    for n, p in zip(names, params):
        ref = g["grad_raw_" + n]
        GU.check(g, "grad_raw_" + n, p.grad, 1e-5 * max(1.0, np.abs(ref).max()), 1e-4)
    torch.nn.utils.clip_grad_value_(params, 0.5)
    norm = torch.nn.utils.clip_grad_norm_(params, 1.0)
    np.testing.assert_allclose(norm.item(), float(g["clip_total_norm"]), rtol=1e-4)
    for n, p in zip(names, params):  # clipped: every |g| <= 0.5, no scaling
        GU.check(g, "grad_clip_" + n, p.grad, 1e-5, 1e-4)
    # the AdamW step and the target update exactly as test_train_gpu.check_update bounds them
    lr, eps, gatol = float(g["lr"]), 1e-8, 1e-5
    step_tol = []
    for p in params:
        ga = p.grad.abs()
        t = torch.clamp(1e-6 + lr * eps * (gatol + 1e-4 * ga) / (ga + eps) ** 2, max=2 * lr)
        step_tol.append(torch.where(ga < gatol, t, torch.full_like(t, 1e-6)))
    opt.step()
    off = total = 0
    for n, p, t in zip(names, params, step_tol):
        GU.check(g, "param_after_" + n, p, t.cpu().numpy(), 0)
        o, c = GU.count_excess(g, "param_after_" + n, p, 1e-6)
        off, total = off + o, total + c
    assert off <= 0.01 * total, f"{off} of {total} AdamW-step elements needed the relaxed tolerance"
    T.interpolate_model(model, target, float(g["tau"]), target)
    for k, v in target.state_dict().items():
        GU.check(g, "target_after_" + k, v, 1e-6, 0)


def test_stateless_update_paths_agree_on_replayed_rollout():
    """A second, random batch: 5 sequences of 2 steps sampled from a replayed fused rollout (16 envs, 12 steps, an
    episode end after step 6, so some targets take the separate NetMon pass) through train.dqn_loss and
    through stateless_seq.seq_loss. Same q, targets and loss within the 1e-5 contract of each path (2e-5 between
    them, scaled by max(1, max|ref|)); gradients within 1e-3 Frobenius-relative: the two paths run their GEMMs at
    different row counts, i.e. on kernels whose fp32-order sums differ in the last bits, and a pre-activation
    within rounding of 0 may take the other side of leaky_relu's kink (test_train_seq_gpu bounds the same effect
    by 1e-3)."""
    gm, M, FU, W, P, RO, L = mods()
    T = importlib.import_module("graph-marl_amd.train")
    RB = importlib.import_module("graph-marl_amd.replaybuffer")
    SS = importlib.import_module("graph-marl_amd.stateless_seq")
    B, N, A, H = 16, 20, 20, 32
    env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A, n_env=B, seed=7,
                     obs_extra=4 * H, agent_adjacency=False)
    torch.manual_seed(4)
    netmon = M.NetMon(4 * N + 8, H, [64, 48], 3, rnn_type="none", agg_type="mean").cuda()
    model = M.DQN(6 * N + 10 + 4 * H, [64, 32], 4).cuda()
    target = M.DQN(6 * N + 10 + 4 * H, [64, 32], 4).cuda()
    target.load_state_dict(model.state_dict())
    with torch.no_grad():
        for p in target.parameters():
            p.add_(0.01 * torch.randn_like(p))
    wenv = W.NetMonWrapper(env, netmon, 1)
    pol = P.EpsilonGreedy(wenv, model, epsilon=0.5, epsilon_decay=1.0, epsilon_update_freq=100, step_before_train=0)
    rb = RB.ReplayBuffer(0, 16 * B, B, A, env.obs_dim, N, 4 * N + 8, netmon.get_state_size(), "cuda")
    wenv.reset()
    for t in range(12):
        obs = env.obs.clone()
        node_obs, agent_node = env.node_obs.clone(), env.agent_node.clone()
        state_in = wenv.last_netmon_state
        act = pol(wenv.obs)
        wenv.step_(act)
        rb.add(obs, act, env.reward, env.obs, env.done.bool(), t == 5, state_in, node_obs, env.nbr, agent_node,
               env.node_obs, env.agent_node)
        if t == 5:
            wenv.reset()
    assert SS.stateless_seq_ok(netmon, model, target)
    params = list(model.parameters()) + list(netmon.parameters())
    netmon.train()
    model.train()
    for trial in range(32):  # draw until a sampled sequence crosses the episode end at its first step
        rng0 = rb.rng.clone()
        seq = rb.get_sequences(5, 2)
        if seq.episode_done[:-1].any():
            break
    assert seq.episode_done[:-1].any()
    rb.rng.copy_(rng0)
    batches = list(rb.get_batch(5, sequence_length=2, lazy_next=True))
    assert all(torch.equal(b.idx[0], seq.idx[0][t]) for t, b in enumerate(batches))
    l0, q0, t0 = T.dqn_loss(netmon, model, target, batches, 0.98, consecutive=True)
    l0.backward()
    g0 = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    netmon.state = None
    l1, q1, t1 = SS.seq_loss(netmon, model, target, seq, 0.98)
    l1.backward()
    for t in range(2):
        close(q1[t], q0[t].detach().cpu().numpy(), f"q_{t}", rel=2e-5)
        close(t1[t], t0[t].cpu().numpy(), f"qtarget_{t}", rel=2e-5)
    np.testing.assert_allclose(l1.item(), l0.item(), rtol=1e-5, atol=1e-6)
    for (n, p), a in zip(list(model.named_parameters()) + list(netmon.named_parameters()), g0):
        err = ((p.grad - a).norm() / a.norm().clamp(min=1e-30)).item()
        assert err < 1e-3, (n, err)


def test_reference_stateless_checkpoint_eval(gm):
    """A checkpoint the reference wrote for rnn_type none: the loaded models reproduce the reference's Q, and
    main.py --eval runs from the file with the architecture taken from its args."""
    main = importlib.import_module("graph-marl_amd.main")
    M = importlib.import_module("graph-marl_amd.model")
    pt = os.path.join(GOLDEN, "ref_checkpoint_stateless.pt")
    ck = main.load_checkpoint(pt)
    args = main.build_parser().parse_args([])
    for k, v in ck["args"].items():
        if k in main.MODEL_ARG_KEYS:
            setattr(args, k, v)
    assert args.netmon_rnn_type == "none" and args.netmon_iterations == 3 and args.netmon_agg_type == "mean"
    dev, N = torch.device("cuda"), ck["args"]["n_router"]
    netmon = M.NetMon(4 * N + 8, args.netmon_dim, main.dim_str_to_list(args.netmon_encoder_dim),
                      args.netmon_iterations, rnn_type=args.netmon_rnn_type,
                      rnn_carryover=bool(args.netmon_rnn_carryover), agg_type=args.netmon_agg_type,
                      output_neighbor_hidden=True, output_global_hidden=args.netmon_global).to(dev)
    model = main.build_model(args, 6 * N + 10 + netmon.get_out_features(), 4).to(dev)
    assert list(netmon.state_dict()) == list(ck["netmon_state_dict"])
    main.load_state_dict(ck, model, netmon)  # strict
    g = np.load(os.path.join(GOLDEN, "ref_checkpoint_stateless.npz"))
    with torch.no_grad():
        for t in range(3):
            f = lambda k: torch.as_tensor(g[k][t], device=dev)  # noqa: E731
            h = netmon(f("node_obs"), f("node_adj"), f("node_agent"))
            q = model(torch.cat([f("agent_obs"), h], -1), None)
            np.testing.assert_allclose(q.cpu().numpy(), g[f"q_{t}"], atol=1e-5, rtol=0, err_msg=f"step {t}")
    m = main.main(["--env-type=routing", "--eval", f"--model-load-path={pt}", "--n-env=16", "--eval-episodes=16",
                   "--eval-episode-steps=20", "--disable-progressbar"])
    assert np.isfinite(m["reward_mean"])


@pytest.mark.parametrize("seq_len,module,fn", [(1, "train", "dqn_update"),
                                               (4, "stateless_seq", "dqn_update_stateless_seq")])
def test_cli_stateless_training_run(tmp_path, monkeypatch, seq_len, module, fn):
    """300 steps of 16 envs at rnn-type none, 8 iterations. Sequence length 1 (the reference run script's form)
    updates through the per-step path, sequence length 4 through the sequence-batched update (main.py's measured
    dispatch); every loss is finite."""
    main = importlib.import_module("graph-marl_amd.main")
    T = importlib.import_module("graph-marl_amd." + module)
    losses, update = [], getattr(T, fn)

    def recording(*a, **kw):
        res = update(*a, **kw)
        losses.append(res[0].detach())
        return res

    monkeypatch.setattr(T, fn, recording)
    m = main.main(["--env-type=routing", "--model=dqn", "--netmon", "--netmon-rnn-type=none", "--netmon-iterations=8",
                   f"--sequence-length={seq_len}", "--n-env=16", "--total-steps=300", "--step-before-train=100",
                   "--mini-batch-size=32", "--episode-steps=50", "--capacity=20000", "--eval-episodes=16",
                   "--eval-episode-steps=20", "--disable-progressbar", f"--log-dir={tmp_path}"])
    assert np.isfinite(m["reward_mean"])
    assert (tmp_path / "model_last.pt").exists()
    assert len(losses) >= 100 and torch.isfinite(torch.stack(losses)).all()
