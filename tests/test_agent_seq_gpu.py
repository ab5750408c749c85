"""GPU tests of the sequence-batched update of the recurrent agent models (graph-marl_amd/agent_seq.py: DQNR and
CommNet without NetMon): gm_agent_comm_bwd against fp64 autograd and its refusals, the whole update against the
reference's golden updates (tests/golden/train_dqnr.npz, train_commnet.npz; src/main.py:840-1026), against the
per-step autograd path (train.dqn_loss) on sequences sampled from a replay buffer, and the dispatch predicate."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_replay as R

pytestmark = pytest.mark.gpu


def mods():
    return (importlib.import_module("graph-marl_amd.model"), importlib.import_module("graph-marl_amd.train"),
            importlib.import_module("graph-marl_amd.agent_seq"), importlib.import_module("graph-marl_amd.replaybuffer"),
            importlib.import_module("graph-marl_amd._lib"))


def _adjacency(B, A, gen):
    """Random asymmetric int8 adjacency [B, A, A]: the diagonal set in even envs' even agents and clear elsewhere
    (both in every env with A > 1, across the envs otherwise), agent 0 without a neighbour, agent 1 adjacent to
    all others."""
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
    if A > 2:
        assert not torch.equal(adj, adj.transpose(1, 2))
    return adj.to(torch.int8).cuda()


def _comm_bwd_ref(g, adj):
    """fp64 autograd of out_i = h_i + sum_{j != i, adj_ij} h_j / max(cnt_i, 1) with upstream gradient g [B, A, H]."""
    B, A, H = g.shape
    m = (adj != 0).double() * (1 - torch.eye(A, dtype=torch.float64, device=g.device))
    h = torch.zeros(B, A, H, dtype=torch.float64, device=g.device, requires_grad=True)
    out = h + (m @ h) / m.sum(-1, keepdim=True).clamp_min(1)
    return torch.autograd.grad(out, h, g.double())[0]


# (B, A, H, row stride of g0 / g1 / dh, g1 given); the last two: the scalar kernel (rows that are no 16-byte lanes)
COMM_CASES = [(3, 5, 48, 52, True), (2, 20, 256, 256, True), (1, 64, 64, 64, True), (2, 1, 64, 64, True),
              (2, 20, 256, 256, False), (3, 5, 48, 51, True), (2, 7, 130, 131, False)]


@pytest.mark.parametrize("B,A,H,ld,two", COMM_CASES)
def test_agent_comm_bwd_vs_fp64(B, A, H, ld, two):
    """|got - ref| <= (A + 3) 2^-23 (max|g0| + max|g1|) A: the forward-error bound of an fp32 sum of at most
    A + 1 terms of that size; a missing or doubled neighbour term is at least max|g| / A."""
    M, T, AS, RB, L = mods()
    gen = torch.Generator().manual_seed(1000 * A + H + ld)
    adj = _adjacency(B, A, gen)
    g0 = torch.randn(B * A, ld, generator=gen).cuda()
    g1 = torch.randn(B * A, ld, generator=gen).cuda() if two else None
    dh = torch.full((B * A, ld), float("nan"), device="cuda")
    L.check(L.lib().gm_agent_comm_bwd(L.ptr(g0), ld, L.ptr(g1), ld, L.ptr(adj), B, A, H, L.ptr(dh), ld,
                                      L.stream_ptr()))
    g = g0[:, :H] + (g1[:, :H] if two else 0)
    ref = _comm_bwd_ref(g.view(B, A, H), adj).view(B * A, H)
    mx = g0[:, :H].abs().max().item() + (g1[:, :H].abs().max().item() if two else 0.0)
    bound = (A + 3) * 2.0 ** -23 * mx * A
    err = (dh[:, :H].double() - ref).abs().max().item()
    print(f"gm_agent_comm_bwd B={B} A={A} H={H} ld={ld}: max error {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    assert torch.isnan(dh[:, H:]).all()  # the padding columns of the output rows stay untouched


@pytest.mark.parametrize("A,H", [(65, 64), (20, 1025)])
def test_agent_comm_bwd_refuses(A, H):
    M, T, AS, RB, L = mods()
    B = 2
    g0 = torch.randn(B * A, H, device="cuda")
    adj = torch.ones(B, A, A, dtype=torch.int8, device="cuda")
    dh = torch.full((B * A, H), float("nan"), device="cuda")
    rc = L.lib().gm_agent_comm_bwd(L.ptr(g0), H, None, 0, L.ptr(adj), B, A, H, L.ptr(dh), H, L.stream_ptr())
    assert rc == -5  # GM_ERR_UNSUPPORTED
    assert b"gm_agent_comm_bwd" in L.lib().gm_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dh).all()


def _golden_models(M, g):
    name = str(g["arch_model"])
    D = g["agent_obs"].shape[-1]
    make = {"dqnr": lambda: M.DQNR(D, [64, 48], 4), "commnet": lambda: M.CommNet(D, [64, 48], 4, 2)}[name]
    sd = lambda p: {k[len(p):]: torch.as_tensor(g[k]) for k in g.files  # noqa: E731
                    if k.startswith(p) and not k.startswith(p + "after_")}
    m, tar = make(), make()
    m.load_state_dict(sd("model_"))
    tar.load_state_dict(sd("target_"))
    return m.cuda(), tar.cuda()


@pytest.mark.parametrize("name", ["dqnr", "commnet"])
def test_agent_seq_update_matches_reference_golden(name):
    """The reference's own update (4 sequences x 20 agents, L = 3, H = 48, done agents, episode ends at steps 1 and
    2, agents without a neighbour) through agent_seq_loss at the tolerances of
    test_models_gpu.test_model_update_matches_reference_golden."""
    from test_train_gpu import check_update

    M, T, AS, RB, L = mods()
    g = np.load(os.path.join(R.GOLDEN, f"train_{name}.npz"))
    m, tar = _golden_models(M, g)
    assert AS.agent_seq_ok(m, tar, None, 0.0, None)
    f = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    Lq = g["actions"].shape[0]
    od = g["agent_obs"].shape[-1]
    obs = F.pad(f(g["agent_obs"]), (0, (od + 3) // 4 * 4 - od))  # [L + 1, B, A, odp]
    adj = f(g["agent_adj"]).to(torch.int8) if "agent_adj" in g.files else None
    seq = AS.AgentSeqBatch(obs[:Lq].contiguous(), od, f(g["actions"]).long(), f(g["reward"]), f(g["done"]).bool(),
                           f(g["episode_done"]).bool(), None if adj is None else adj[:Lq].contiguous(),
                           obs[1:Lq + 1].contiguous(), None if adj is None else adj[1:Lq + 1].contiguous(),
                           f(g["agent_state0"]))
    params = list(m.parameters())
    names = [f"model_{k}" for k, _ in m.named_parameters()]
    assert names == list(g["param_names"])
    opt = torch.optim.AdamW(params, lr=float(g["lr"]))
    m.train()
    parts = {}
    loss, q, qt = AS.agent_seq_loss(m, tar, seq, float(g["gamma"]), params, parts=parts)
    for t in range(Lq):
        np.testing.assert_allclose(q[t].detach().cpu().numpy(), g[f"q_{t}"], atol=1e-5, rtol=0, err_msg=f"q_{t}")
        np.testing.assert_allclose(qt[t].cpu().numpy(), g[f"qtarget_{t}"], atol=1e-5, rtol=0, err_msg=f"qtarget_{t}")
    np.testing.assert_allclose(parts["loss_q"].item(), g["loss_q"].item(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(loss.item(), g["loss"].item(), rtol=1e-5, atol=1e-6)
    opt.zero_grad()
    loss.backward()
    check_update(g, names, params, opt, m, tar, T)


def _fro(a, b):
    return (a.double() - b.double()).norm().item() / max(b.double().norm().item(), 1e-30)


def _filled_buffer(RB, state_len, D, B=8, A=6, steps=12):
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()  # noqa: E731
    rb = RB.ReplayBuffer(3, steps * B, B, A, D, 0, 0, 0, torch.device("cuda"), agent_state_size=state_len,
                         store_adj=True)
    adj = (torch.rand(B, A, A, generator=gen) < 0.4).cuda()
    for t in range(steps):
        nadj = (torch.rand(B, A, A, generator=gen) < 0.4).cuda()
        rb.add_pre(rnd(B, A, D), adj=adj, agent_state=torch.tanh(rnd(B, A, state_len)))
        rb.add_post(torch.randint(0, 4, (B, A), generator=gen).cuda(), rnd(B, A), rnd(B, A, D),
                    (torch.rand(B, A, generator=gen) < 0.2).cuda(), t in (4, 9), next_adj=nadj)
        adj = nadj
    return rb


@pytest.mark.parametrize("name", ["dqnr", "commnet"])
def test_agent_seq_matches_per_step_path_on_buffer(name):
    """16 sequences x L = 4 drawn twice from equal seeds (get_batch, get_agent_sequences): the gathered fields are
    equal bit for bit, and train.dqn_loss (per-step autograd) and agent_seq_loss give the same q, targets, loss and
    gradients (the scheme of test_train_seq_gpu._compare_paths: Frobenius-relative gradient error against the
    exact-fp32 per-step run below max(2e-5, 2 x the per-step split-f16 path's)."""
    M, T, AS, RB, L = mods()
    D, Lq, nseq = 30, 4, 16
    torch.manual_seed(11)
    make = (lambda: M.DQNR(D, [64, 64], 4)) if name == "dqnr" else (lambda: M.CommNet(D, [64, 64], 4, 2))
    m, tar = make().cuda(), make().cuda()
    assert AS.agent_seq_ok(m, tar, None, 0.0, None)
    rb = _filled_buffer(RB, m.get_state_len(), D)
    rng0 = rb.rng.clone()
    batches = list(rb.get_batch(nseq, sequence_length=Lq))
    rb.rng.copy_(rng0)
    seq = rb.get_agent_sequences(nseq, Lq)
    assert seq.episode_done.any() and seq.done.any()
    assert not torch.equal(seq.adj, seq.adj.transpose(-1, -2))
    for t, b in enumerate(batches):
        assert torch.equal(b.idx[0], seq.idx[0][t]) and torch.equal(b.idx[1], seq.idx[1])
        assert torch.equal(seq.obs[t][..., :D], b.obs) and torch.equal(seq.next_obs[t][..., :D], b.next_obs)
        assert torch.equal(seq.action[t], b.action) and torch.equal(seq.reward[t], b.reward)
        assert torch.equal(seq.done[t], b.done) and torch.equal(seq.episode_done[t], b.episode_done)
        assert seq.adj.dtype == torch.int8 and seq.next_adj.dtype == torch.int8
        assert torch.equal(seq.adj[t], b.adj.to(torch.int8)) and torch.equal(seq.next_adj[t], b.next_adj.to(torch.int8))
    assert torch.equal(seq.agent_state, batches[0].agent_state)
    params = list(m.parameters())
    m.train()

    def per_step():
        for p in params:
            p.grad = None
        m.state = None
        l, q, qt = T.dqn_loss(None, m, tar, batches, 0.98)
        l.backward()
        return l.detach(), q, qt, [p.grad.clone() for p in params]

    l0, q0, t0, g0 = per_step()
    for p in params:
        p.grad = None
    l1, q1, t1 = AS.agent_seq_loss(m, tar, seq, 0.98, params)
    l1.backward()
    g1 = [p.grad.clone() for p in params]
    old = L.GEMM_MODE
    L.GEMM_MODE = "f32"  # exact-fp32 reference: the per-step path with every GEMM in fp32
    try:
        _, _, _, gf = per_step()
    finally:
        L.GEMM_MODE = old
    for t in range(Lq):
        torch.testing.assert_close(q1[t], q0[t].detach(), rtol=0, atol=2e-5)
        torch.testing.assert_close(t1[t], t0[t], rtol=0, atol=2e-5)
    torch.testing.assert_close(l1, l0, rtol=1e-5, atol=1e-8)
    errs = {n: (_fro(a, c), _fro(b, c)) for (n, _), a, b, c in zip(m.named_parameters(), g0, g1, gf)}
    print("Frobenius-relative gradient error vs exact fp32 (per-step x3, sequence-batched x3):", errs)
    for n, (e_old, e_new) in errs.items():
        assert e_new < max(2e-5, 2 * e_old), (n, e_old, e_new)


def test_agent_seq_ok_dispatch():
    M, T, AS, RB, L = mods()
    D = 30
    pairs = [(M.DQNR(D, [64, 64], 4), M.DQNR(D, [64, 64], 4)), (M.CommNet(D, [64, 64], 4, 2), M.CommNet(D, [64, 64], 4, 2)),
             (M.DQNR(D, [64, 48], 4), M.DQNR(D, [64, 48], 4)), (M.CommNet(D, [64, 48], 4, 2), M.CommNet(D, [64, 48], 4, 2))]
    for m, tar in pairs:
        assert AS.agent_seq_ok(m, tar, None, 0.0, None)
    m, tar = pairs[1]
    assert not AS.agent_seq_ok(m, tar, M.NetMon(8, 32, [32], 1), 0.0, None)
    assert not AS.agent_seq_ok(m, tar, None, 0.03, None)
    assert not AS.agent_seq_ok(m, tar, None, 0.0, M.MLP(8, [8, 4], activation_on_output=False))
    assert not AS.agent_seq_ok(M.DGN(D, [64], 4, 3, 1), M.DGN(D, [64], 4, 3, 1), None, 0.0, None)
    assert not AS.agent_seq_ok(M.DQN(D, [64, 64], 4), M.DQN(D, [64, 64], 4), None, 0.0, None)
    assert not AS.agent_seq_ok(m, pairs[0][1], None, 0.0, None)  # online and target of different types
    assert AS.agent_seq_ok(m, tar, None, 0.0, None, 64) and not AS.agent_seq_ok(m, tar, None, 0.0, None, 65)
    old = L.GEMM_MODE
    L.GEMM_MODE = "f32"
    try:
        assert not AS.agent_seq_ok(m, tar, None, 0.0, None)
    finally:
        L.GEMM_MODE = old
