"""Global-mean NetMon readout (--netmon-global, reference src/model.py:458-469, 624-627) on the fused rollout and
the sequence-batched update: the two kernels (gm_netmon_global_rows / gm_netmon_global_bwd) against fp64 torch, the
fused NetMonWrapper + DQN against the unfused path (NetMon.forward_graph + joint observation) and the reference's
golden file, train_seq.seq_loss against train.dqn_loss, and the dispatch conditions."""
import importlib
import os

import numpy as np
import pytest
import torch

import golden_replay as R

pytestmark = pytest.mark.gpu

GM_ERR_INVALID_ARG = -1


def mods():
    names = ("", ".model", ".fused", ".wrapper", ".policy", ".train", ".train_seq", ".replaybuffer", "._lib")
    return tuple(importlib.import_module("graph-marl_amd" + n) for n in names)


# ---------------------------------------------------------------------------------------------------------
# 1. kernels against fp64 torch
# ---------------------------------------------------------------------------------------------------------
G = 3
# (N, H, rows_per_graph, first written column, row width, vector form). The joint observation's graph part starts
# at column 6N+10: 8-byte but not 16-byte aligned, so float2 lanes.
KERNEL_CASES = [(N, H, rows, 6 * N + 10, 6 * N + 10 + 96 + 10, 2)
                for N in (4, 6, 20) for H in (32, 96) for rows in sorted({1, 5, N})]
# the other forms: an odd start and stride (dword lanes), 16-byte lanes (the update's readout buffer), and the
# widest row on dword lanes (1024 column chunks for 256 threads: the per-thread loop)
KERNEL_CASES += [(6, 96, 5, 47, 145, 1), (20, 32, 5, 0, 32, 4), (20, 96, 20, 384, 480, 4), (4, 1024, 1, 1, 1027, 1)]


@pytest.mark.parametrize("N,H,rows,col0,width,V", KERNEL_CASES)
def test_global_rows_vs_fp64(N, H, rows, col0, width, V):
    """m = mean over the graph's nodes of the h half of [h | c] rows (ld_state = 2H), written to H columns of a
    wider row. Bound per element, derived: the fp32 sum of N terms in any fixed order is within (N - 1) 2^-24
    sum_n |h| of the exact sum, and 1/N and the product round once each: < N 2^-23 mean_n |h|. Every other
    column keeps its sentinel."""
    gm, M, FU, W, P, T, S, RB, L = mods()
    torch.manual_seed(N * 1000 + H + rows)
    state = torch.randn(G * N, 2 * H, device="cuda")
    state[:, H:] = float("nan")  # the c half must not be read
    out = torch.full((G * rows, width), -7.25, device="cuda")
    L.check(L.lib().gm_netmon_global_rows(state.data_ptr(), 2 * H, G, N, H, rows, out.data_ptr() + 4 * col0, width,
                                          L.stream_ptr()))
    assert L.last_kernel() == f"k_global_rows<{V}>"
    h = state[:, :H].double().view(G, N, H)
    ref = h.mean(1, keepdim=True).expand(G, rows, H).reshape(G * rows, H)
    bound = (N * 2.0 ** -23 * h.abs().mean(1, keepdim=True)).expand(G, rows, H).reshape(G * rows, H)
    err = (out[:, col0:col0 + H].double() - ref).abs()
    print("max err / bound:", (err / bound).max().item())
    assert (err <= bound).all()
    assert (out[:, :col0] == -7.25).all() and (out[:, col0 + H:] == -7.25).all()


@pytest.mark.parametrize("N,H,rows,col0,width,V", KERNEL_CASES)
def test_global_bwd_vs_fp64(N, H, rows, col0, width, V):
    """dh[n] += (1/N) sum_r d_rows[r] for every node n of the graph, onto random dh (an overwrite fails). The same
    bound with rows_per_graph in place of N (the row sum, 1/N and the product), plus the rounding of the final
    add (2^-24 |dh'|)."""
    gm, M, FU, W, P, T, S, RB, L = mods()
    torch.manual_seed(N * 1000 + H + rows + 1)
    d = torch.randn(G * rows, width, device="cuda")
    dh0 = torch.randn(G * N, H, device="cuda")
    dh = dh0.clone()
    L.check(L.lib().gm_netmon_global_bwd(d.data_ptr() + 4 * col0, width, G, N, H, rows, dh.data_ptr(), H,
                                         L.stream_ptr()))
    assert L.last_kernel() == f"k_global_bwd<{V}>"
    dd = d[:, col0:col0 + H].double().view(G, rows, H)
    add = (dd.sum(1, keepdim=True) / N).expand(G, N, H).reshape(G * N, H)
    ref = dh0.double() + add
    # e1: the added term's error (rows = 1: exactly the two roundings of 1/N and the product, with their
    # second-order term 2^-48); the add rounds its fp32 operands' exact sum, which is within e1 of ref
    e1 = ((rows * 2.0 ** -23 + 2.0 ** -46) * dd.abs().sum(1, keepdim=True) / N).expand(G, N, H).reshape(G * N, H)
    bound = e1 + 2.0 ** -24 * (ref.abs() + e1)
    err = (dh.double() - ref).abs()
    print("max err / bound:", (err / bound).max().item())
    assert (err <= bound).all()


def test_global_kernels_refuse_bad_hidden():
    """H = 48 (not a multiple of 32): GM_ERR_INVALID_ARG, nothing launched, the outputs untouched."""
    gm, M, FU, W, P, T, S, RB, L = mods()
    N, H, rows = 6, 48, 5
    state = torch.randn(G * N, H, device="cuda")
    out = torch.full((G * rows, H), 3.5, device="cuda")
    dh = torch.full((G * N, H), 2.5, device="cuda")
    lib = L.lib()
    assert lib.gm_netmon_global_rows(state.data_ptr(), H, G, N, H, rows, out.data_ptr(), H,
                                     L.stream_ptr()) == GM_ERR_INVALID_ARG
    assert lib.gm_netmon_global_bwd(out.data_ptr(), H, G, N, H, rows, dh.data_ptr(), H,
                                    L.stream_ptr()) == GM_ERR_INVALID_ARG
    assert lib.gm_netmon_global_rows(state.data_ptr(), H, G, 129, 32, rows, out.data_ptr(), H,
                                     L.stream_ptr()) == GM_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out == 3.5).all() and (dh == 2.5).all()


# ---------------------------------------------------------------------------------------------------------
# 2. rollout parity
# ---------------------------------------------------------------------------------------------------------
B_RO, N_RO, A_RO, H_RO = 8, 10, 10, 32
UNFUSED_ONLY = ("netmon_readout:", "lstm_pointwise:")  # launch tags of NetMon.forward_graph alone (model.py)


def _wrapped(gm, M, W, fused, rnn, K, glob=True, carry=True, B=B_RO, seed=5):
    env = gm.Routing(gm.Network(N_RO, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A_RO, n_env=B, seed=seed,
                     obs_extra=5 * H_RO, agent_adjacency=False)
    torch.manual_seed(1)
    nm = M.NetMon(4 * N_RO + 8, H_RO, [64, 48], K, rnn_type=rnn, output_global_hidden=glob,
                  rnn_carryover=carry).cuda()
    return env, nm, W.NetMonWrapper(env, nm, 1, fused=fused)


@pytest.mark.parametrize("rnn", ["lstm", "gru"])
@pytest.mark.parametrize("K", [1, 2])
def test_fused_global_rollout_matches_unfused(rnn, K):
    """6 steps across an episode reset: Q of the fused path (READOUT source + [env obs | global] rows) within 1e-5
    of the DQN on the unfused joint observation, `.obs` within 1e-6 in the reference layout, also when `.obs`
    reads and Q passes alternate without an env step; the fused run launches gm_netmon_global_rows and nothing
    that only NetMon.forward_graph launches."""
    gm, M, FU, W, P, T, S, RB, L = mods()
    e1, nm1, w1 = _wrapped(gm, M, W, True, rnn, K)
    e2, nm2, w2 = _wrapped(gm, M, W, False, rnn, K)
    assert FU.fused_ok(nm1) and w1.fused and w1.global_cols and e1.obs_gemm is None
    torch.manual_seed(2)
    dqn = M.DQN(e1.obs_dim + 5 * H_RO, [64, 32], 4).cuda()
    p1 = P.EpsilonGreedy(w1, dqn, epsilon=0.5, epsilon_decay=1.0, step_before_train=0)
    p2 = P.EpsilonGreedy(w2, dqn, epsilon=0.5, epsilon_decay=1.0, step_before_train=0)
    trace = []

    def fused_run(fn):
        L.TRACE = []
        try:
            return fn()
        finally:
            trace.extend(L.TRACE)
            L.TRACE = None

    fused_run(w1.reset_)
    w2.reset_()
    for t in range(6):
        if t == 3:  # episode end: new topologies, NetMon state from zero
            fused_run(w1.reset_)
            w2.reset_()
        q1 = fused_run(lambda: p1._fused_q(w1)).view(B_RO, A_RO, -1).clone()
        q2 = p2.q_values(w2.obs)
        print(f"step {t}: max |dq| = {(q1 - q2).abs().max().item():.3g}")
        torch.testing.assert_close(q1, q2, atol=1e-5, rtol=0)
        o2 = w2.obs
        o1 = w1.obs.clone()  # materialises the reference layout over the scratch columns
        print(f"step {t}: max |dobs| = {(o1 - o2).abs().max().item():.3g}")
        torch.testing.assert_close(o1, o2, atol=1e-6, rtol=0)
        q1b = fused_run(lambda: p1._fused_q(w1)).view(B_RO, A_RO, -1).clone()  # rewrites the scratch columns
        assert torch.equal(q1b, q1)
        assert torch.equal(w1.obs, o1) and torch.equal(w1.obs, o1)  # and back, twice
        assert torch.equal(fused_run(lambda: p1._fused_q(w1)).view(B_RO, A_RO, -1), q1)
        # the same Q rows to both envs' ε-greedy draws (each env stream draws once per step), through both step
        # forms of the fused path: select + step_, and the draws as the env step kernel's prologue
        act = p2.select(q2).clone()
        if t % 2:
            a1 = p1.select(q2).clone()
            fused_run(lambda: w1.step_(a1))
        else:
            fused_run(lambda: w1.policy_step_(q2.contiguous(), 0.5, p1.actions))
            a1 = p1.actions
        assert torch.equal(a1, act)
        w2.step_(act)
        assert torch.equal(e1.obs, e2.obs)
    assert any(tag.startswith("gm_netmon_global_rows:") for tag in trace)
    assert not [tag for tag in trace if tag.startswith(UNFUSED_ONLY)]


def test_fused_global_step_vs_reference_golden():
    """The fused NetMon step + the 4H readout + gm_netmon_global_rows in the reference layout [h | global | nbr x 3]
    against netmon_global.npz over 3 carried steps, at the tolerance of
    test_netmon_gpu.py::test_netmon_global_readout_vs_reference_golden (1e-5)."""
    gm, M, FU, W, P, T, S, RB, L = mods()
    g = np.load(os.path.join(R.GOLDEN, "netmon_global.npz"))
    H = 32
    for vi, K in enumerate((1, 2)):
        nm = M.NetMon(g["node_obs"].shape[-1], H, [64, 48], K, output_global_hidden=True).cuda()
        nm.load_state_dict({k[len(f"v{vi}_w_"):]: torch.as_tensor(g[k]) for k in g.files if k.startswith(f"v{vi}_w_")})
        assert FU.fused_ok(nm)
        state = None
        for t in range(3):
            x = torch.as_tensor(g["node_obs"][t], device="cuda")
            nbr = M.dense_to_nbr(torch.as_tensor(g["node_adj"][t], device="cuda"))
            an = M.node_agent_to_index(torch.as_tensor(g["node_agent"][t], device="cuda"))
            state, hprev = FU.netmon_step(nm, x, nbr, state)
            Bg, N = x.shape[:2]
            A = an.shape[1]
            rd = torch.empty(Bg * A, 4 * H, device="cuda")
            L.check(L.lib().gm_netmon_readout_ld(state.data_ptr(), 2 * H, hprev.data_ptr(), hprev.stride(0),
                                                 nbr.data_ptr(), an.data_ptr(), Bg, N, A, 3, H, rd.data_ptr(), 4 * H,
                                                 L.stream_ptr()))
            gl = torch.empty(Bg * A, H, device="cuda")
            FU.global_rows(state.data_ptr(), 2 * H, Bg, N, H, A, gl.data_ptr(), H)
            mapped = torch.cat([rd[:, :H], gl, rd[:, H:]], 1).view(Bg, A, 5 * H)
            np.testing.assert_allclose(mapped.cpu().numpy(), g[f"v{vi}_mapped_{t}"], atol=1e-5, rtol=0)
            np.testing.assert_allclose(state.cpu().numpy(), g[f"v{vi}_state_{t}"], atol=1e-5, rtol=0)


# ---------------------------------------------------------------------------------------------------------
# 3. update parity
# ---------------------------------------------------------------------------------------------------------
def _fro(a, b):
    return (a.double() - b.double()).norm().item() / max(b.double().norm().item(), 1e-30)


def _replayed(rnn, K, agg, ep_end, glob=True, n_seq=4):
    """4 envs, N = 10, H = 32: two warm-up steps, then 4 recorded steps (the ring then holds exactly one start
    slot for L = 3, so every sampled sequence is steps 0..2); ep_end: the episode ends at recorded step 1 (the
    wrapper resets), inside every sequence. Returns (netmon, model, target, batches, seq, params)."""
    gm, M, FU, W, P, T, S, RB, L = mods()
    B, N, A, H, Lq = 4, N_RO, A_RO, H_RO, 3
    env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A, n_env=B, seed=7,
                     obs_extra=5 * H, agent_adjacency=False)
    torch.manual_seed(K + len(rnn))
    netmon = M.NetMon(4 * N + 8, H, [64, 48], K, rnn_type=rnn, agg_type=agg, output_global_hidden=glob).cuda()
    gw = (5 if glob else 4) * H
    model = M.DQN(6 * N + 10 + gw, [64, 32], 4).cuda()
    target = M.DQN(6 * N + 10 + gw, [64, 32], 4).cuda()
    target.load_state_dict(model.state_dict())
    with torch.no_grad():
        for p in target.parameters():
            p.add_(0.01 * torch.randn_like(p))
    wenv = W.NetMonWrapper(env, netmon, 1)
    pol = P.EpsilonGreedy(wenv, model, epsilon=0.5, epsilon_decay=1.0, epsilon_update_freq=100, step_before_train=0)
    rb = RB.ReplayBuffer(0, 8 * B, B, A, env.obs_dim, N, 4 * N + 8, netmon.get_state_size(), "cuda")
    wenv.reset()
    for t in range(-2, 4):
        obs = env.obs.clone()
        node_obs, agent_node = env.node_obs.clone(), env.agent_node.clone()
        state_in = wenv.last_netmon_state
        act = pol.act(wenv).clone()
        wenv.step_(act)
        done_ep = ep_end and t == 1
        if t >= 0:
            rb.add(obs, act, env.reward, env.obs, env.done.bool(), done_ep, state_in, node_obs, env.nbr, agent_node,
                   env.node_obs, env.agent_node)
        if done_ep:
            wenv.reset()
    params = list(model.parameters()) + list(netmon.parameters())
    rng0 = rb.rng.clone()
    batches = list(rb.get_batch(n_seq, sequence_length=Lq, lazy_next=True))
    rb.rng.copy_(rng0)
    seq = rb.get_sequences(n_seq, Lq)
    assert all(torch.equal(b.idx[0], seq.idx[0][t]) for t, b in enumerate(batches))
    assert bool(seq.episode_done[:-1].any()) == bool(ep_end)
    netmon.train()
    model.train()
    return netmon, model, target, batches, seq, params


@pytest.mark.parametrize("rnn", ["lstm", "gru", "lnlstm"])
@pytest.mark.parametrize("K,agg,ep_end", [(1, "sum", False), (2, "mean", True)])
def test_seq_update_with_global_matches_autograd_path(rnn, K, agg, ep_end):
    """train_seq.seq_loss == train.dqn_loss on the same replayed sequences with output_global_hidden: q and
    targets (atol 2e-5), the loss (rtol 1e-5), and every parameter gradient, the first DQN layer's in the
    reference column order, at the bounds of test_train_seq_gpu.py::_compare_paths on a common GEMM tile
    (Frobenius-relative error against the exact-fp32 autograd gradients below max(2e-5, twice the autograd
    path's own)). K = 2: the episode ends inside the sequence, so the state-gradient mask and the global
    gradient meet."""
    gm, M, FU, W, P, T, S, RB, L = mods()
    netmon, model, target, batches, seq, params = _replayed(rnn, K, agg, ep_end)
    assert S.seq_ok(netmon, model, target)
    lib = FU._setup()
    lib.gm_gemm_set_tile(0)
    try:
        l0, q0, t0 = T.dqn_loss(netmon, model, target, batches, 0.98, consecutive=True)
        for p in params:
            p.grad = None
        l0.backward()
        g0 = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        netmon.state = None
        l1, q1, t1 = S.seq_loss(netmon, model, target, seq, 0.98, params)
        l1.backward()
        g1 = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        netmon.state = None
        old = L.GEMM_MODE
        L.GEMM_MODE = "f32"  # exact-fp32 reference: the autograd path with every GEMM in fp32
        try:
            lf, _, _ = T.dqn_loss(netmon, model, target, batches, 0.98, consecutive=True)
            lf.backward()
        finally:
            L.GEMM_MODE = old
        gf = [p.grad.clone() for p in params]
    finally:
        lib.gm_gemm_set_tile(-1)
    for t in range(len(batches)):
        print(f"step {t}: max |dq| {(q1[t] - q0[t]).abs().max().item():.3g}, max |dtarget| "
              f"{(t1[t] - t0[t]).abs().max().item():.3g}")
    print("loss", l1.item(), l0.item())
    names = [n for n, _ in list(model.named_parameters()) + list(netmon.named_parameters())]
    errs = {n: (_fro(a, c), _fro(b, c)) for n, a, b, c in zip(names, g0, g1, gf)}
    print("Frobenius-relative gradient error vs exact fp32 (autograd x3, sequence-batched x3):", errs)
    for t in range(len(batches)):
        torch.testing.assert_close(q1[t], q0[t].detach(), rtol=0, atol=2e-5)
        torch.testing.assert_close(t1[t], t0[t], rtol=0, atol=2e-5)
    torch.testing.assert_close(l1, l0.detach(), rtol=1e-5, atol=1e-8)
    assert g1[0].shape == model.encoder.linear_layers[0].weight.shape
    for n, (e_old, e_new) in errs.items():
        assert e_new < max(2e-5, 2 * e_old), (n, e_old, e_new)


# ---------------------------------------------------------------------------------------------------------
# 4. dispatch
# ---------------------------------------------------------------------------------------------------------
def test_dispatch_conditions():
    """fused_ok / seq_ok accept the global readout with carry-over and still refuse rnn_carryover=False."""
    gm, M, FU, W, P, T, S, RB, L = mods()
    for rnn in ("lstm", "gru", "lnlstm"):
        nm = M.NetMon(48, 32, [64, 48], 1, rnn_type=rnn, output_global_hidden=True).cuda()
        dq = M.DQN(70 + 160, [64, 32], 4).cuda()
        assert FU.fused_ok(nm) and S.seq_ok(nm, dq, dq)
        nc = M.NetMon(48, 32, [64, 48], 1, rnn_type=rnn, output_global_hidden=True, rnn_carryover=False).cuda()
        assert not FU.fused_ok(nc) and not S.seq_ok(nc, dq, dq)
        nc = M.NetMon(48, 32, [64, 48], 1, rnn_type=rnn, rnn_carryover=False).cuda()
        assert not FU.fused_ok(nc) and not S.seq_ok(nc, dq, dq)


def test_flag_off_launches_are_unchanged(monkeypatch):
    """Without the flag one rollout step and one update launch exactly what they launched before the global paths
    existed: the tag trace (_lib.TRACE) and the kernel names (gm_last_kernel after every library call) of a run
    in which every global entry point raises equal those of a normal run, and neither names a global kernel."""
    gm, M, FU, W, P, T, S, RB, L = mods()
    lib = L.lib()

    def run(block):
        if block:
            def boom(*a, **k):
                raise AssertionError("global readout code reached with the flag off")
            for mod, name in ((FU, "global_rows"), (FU, "global_first_cols"), (lib, "gm_netmon_global_rows"),
                              (lib, "gm_netmon_global_bwd")):
                monkeypatch.setattr(mod, name, boom)
        torch.manual_seed(0)
        netmon, model, target, batches, seq, params = _replayed("lstm", 1, "sum", False, glob=False)
        e, nm, w = _wrapped(gm, M, W, None, "lstm", 1, glob=False)
        M.tag_modules(nm, "netmon.")
        M.tag_modules(model, "dqn.")
        assert w.fused and not w.global_cols and e.obs_gemm is not None
        pol = P.EpsilonGreedy(w, model, epsilon=0.5, epsilon_decay=1.0, step_before_train=0)
        w.reset_()
        names = []
        real = L.check

        def spy(rc):
            real(rc)
            names.append(L.last_kernel())
        monkeypatch.setattr(L, "check", spy)
        L.TRACE = []
        try:
            pol.act_step(w)
            _ = w.obs
            pol.act(w)
            loss, _, _ = S.seq_loss(netmon, model, target, seq, 0.98, params)
            loss.backward()
        finally:
            tags, L.TRACE = L.TRACE, None
            monkeypatch.setattr(L, "check", real)
        if block:
            monkeypatch.undo()
        return tags, names

    tags0, names0 = run(block=True)
    tags1, names1 = run(block=False)
    assert tags0 and names0
    assert tags0 == tags1 and names0 == names1
    assert not [x for x in tags1 + names1 if "global" in x]
    assert lib.gm_netmon_global_rows is not None and lib.gm_netmon_global_bwd is not None
