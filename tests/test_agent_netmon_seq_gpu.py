"""Sequence-batched DQNR / CommNet + NetMon update (graph-marl_amd/agent_netmon_seq.py): against the per-step
autograd path (train.dqn_loss / train.dqn_update) on the same sampled transitions, against the reference's golden
updates (tests/golden/train_dqnr_netmon.npz, train_commnet_netmon.npz), the sampler against get_batch, the dispatch
predicate and the CLI branch, run-to-run bit equality, and the launch lists of the paths the hooks were added to
(tests/golden/agent_seq_trace.json, train_seq_trace.json).

Small shape (agent_netmon_util.py): N = 10 nodes, A = 5 (and 7) agents, NetMon H = 32 with encoder (64, 32), agent
encoder (64, 32), CommNet with 2 rounds, B = 3 sequences, L = 3 (and 2)."""
import copy
import importlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import agent_netmon_util as U
import dgn_netmon_util as DU
import golden_replay as R

gpu = pytest.mark.gpu

# (rnn, K, agg, global, A, L): lstm / gru / lnlstm cells, K = 1 and 3, sum and mean, the global mean, a second agent
# count, and L = 2 (the step after an episode end is the last step)
CASES = [("lstm", 1, "sum", False, 5, 3), ("lstm", 3, "mean", False, 5, 3), ("gru", 1, "sum", False, 5, 3),
         ("gru", 3, "mean", False, 5, 3), ("lnlstm", 1, "mean", False, 5, 3), ("lnlstm", 3, "sum", False, 5, 3),
         ("lstm", 1, "sum", True, 5, 3), ("lstm", 3, "mean", True, 5, 3), ("lstm", 1, "sum", False, 7, 3),
         ("lstm", 3, "sum", False, 5, 2)]


@gpu
@pytest.mark.parametrize("kind", ["dqnr", "commnet"])
@pytest.mark.parametrize("rnn,K,agg,glob,A,Lq", CASES)
def test_matches_per_step_path(kind, rnn, K, agg, glob, A, Lq):
    """The transitions get_batch draws through train.dqn_loss and through agent_netmon_seq_loss.

    The case (lstm, K = 1, sum, A = 5, L = 3) rejected each of four mutations for both models when they were
    applied one at a time (not committed): the agent-state kill mask dropped in agent_seq._forward (loss 26 / 5.9
    times its tolerance for dqnr / commnet), the episode_done mask on the NetMon state gradient dropped in
    train_seq._backward_netmon (NetMon gradients 0.3 - 0.6 off in Frobenius-relative terms), agent_seq._target_max
    started from the state after the mask (q_target_0 1779 / 253 times), and the first layer's weight-gradient
    column blocks swapped in dgn_netmon_seq.first_backward (that gradient 252 / 97 times)."""
    gm, M, FU, W, T, AS, ANS, RB, L = U.mods()
    netmon, model, target, rb, params = U.replayed(kind, rnn, K, glob, agg, A=A, Lq=Lq)
    assert ANS.agent_netmon_seq_ok(netmon, model, target, 0.0, None, A)
    batches, seq, _ = U.sample(rb, 3, Lq)
    U.sequence_conditions(seq)
    assert not torch.equal(seq.agent_node[0, 0].long().cpu(), torch.arange(A))  # agent -> node: no identity gather
    U.compare_with_per_step(netmon, model, target, batches, seq, params)


@gpu
@pytest.mark.parametrize("kind", ["dqnr", "commnet"])
@pytest.mark.parametrize("Lq", [1, 2, 3])
def test_sampler_fields(kind, Lq):
    """get_agent_netmon_sequences draws get_batch's indices from the same stream state and leaves the stream where
    get_batch leaves it (U.sample); its fields are the bits get_batch gathers."""
    gm, M, FU, W, T, AS, ANS, RB, L = U.mods()
    netmon, model, target, rb, params = U.replayed(kind, Lq=max(Lq, 2))
    n_seq = 4
    batches, seq, rng0 = U.sample(rb, n_seq, Lq)
    od = rb.obs_dim
    assert seq.obs_dim == od
    comm = kind == "commnet"
    assert (seq.adj is not None) == comm and (seq.next_adj is not None) == comm
    for t, b in enumerate(batches):
        nf = seq.next_fields(t, None)
        fields = [("obs", seq.obs[t][..., :od], b.obs), ("action", seq.action[t], b.action),
                  ("reward", seq.reward[t], b.reward), ("done", seq.done[t], b.done),
                  ("episode_done", seq.episode_done[t].expand(n_seq), b.episode_done.expand(n_seq)),
                  ("node_obs", seq.node_obs[t], b.node_obs), ("nbr", seq.nbr[t], b.nbr),
                  ("agent_node", seq.agent_node[t], b.agent_node),
                  ("next_obs", seq.next_obs[t][..., :od], b.next_obs), ("next_fields obs", nf[0][..., :od], b.next_obs),
                  ("next_node_obs", nf[1], b.next_node_obs), ("next_agent_node", nf[2], b.next_agent_node)]
        if comm:
            assert seq.adj.dtype == torch.int8 and seq.next_adj.dtype == torch.int8
            fields += [("adj", seq.adj[t], b.adj.to(torch.int8)), ("next_adj", seq.next_adj[t], b.next_adj.to(torch.int8))]
        for name, got, want in fields:
            assert got.dtype == want.dtype and torch.equal(got, want), (t, name)
    assert torch.equal(seq.node_state, batches[0].node_state)
    assert torch.equal(seq.agent_state, batches[0].agent_state) and seq.agent_state.abs().max() > 0
    r = torch.tensor([2, 0], device="cuda")
    for a, b in zip(seq.next_fields(Lq - 1, r), seq.next_fields(Lq - 1, None)):
        assert torch.equal(a, b[r])


def test_dispatch_predicate():
    """True for the reference configuration (both models; lstm, gru, lnlstm, the global mean); False for the aux
    loss, --netmon-rnn-carryover 0, a tanh agent activation, 65 agents, GM_GEMM=f32, no NetMon and the other
    models."""
    gm, M, FU, W, T, AS, ANS, RB, L = U.mods()
    ok = ANS.agent_netmon_seq_ok
    D = 130 + 512
    dqnr = lambda **kw: M.DQNR(D, [512, 256], 4, **kw)  # noqa: E731
    comm = lambda **kw: M.CommNet(D, [512, 256], 4, 2, **kw)  # noqa: E731
    nm = lambda **kw: M.NetMon(88, 128, [512, 256], 1, **kw)  # noqa: E731
    n = nm()
    for make in (dqnr, comm):
        m, tar = make(), make()
        assert ok(n, m, tar, 0.0, None, 20) and ok(n, m, tar, 0.0, None, 64) and ok(n, m, tar)
        for rnn in ("gru", "lnlstm"):
            assert ok(nm(rnn_type=rnn), m, tar, 0.0, None, 20)
        assert not ok(n, m, tar, 0.0, M.MLP(256, [256, 20], activation_on_output=False), 20)  # aux head
        assert not ok(nm(rnn_carryover=False), m, tar, 0.0, None, 20)
        assert not ok(n, make(activation="tanh"), make(activation="tanh"), 0.0, None, 20)
        assert not ok(nm(activation="relu"), m, tar, 0.0, None, 20)
        assert not ok(n, m, tar, 0.0, None, 65)
        assert not ok(None, m, tar, 0.0, None, 20)
        assert not AS.agent_seq_ok(m, tar, n, 0.0, None, 20)  # agent_seq keeps refusing NetMon
        old = L.GEMM_MODE
        L.GEMM_MODE = "f32"
        try:
            assert not ok(n, m, tar, 0.0, None, 20)
        finally:
            L.GEMM_MODE = old
    g = M.DQNR(D + 128, [512, 256], 4)
    assert ok(nm(output_global_hidden=True), g, g, 0.0, None, 20)
    sm = U.make_model(M, "commnet", 46 + 128)
    assert ok(M.NetMon(48, 32, [64, 32], 3), sm, sm, 0.0, None, 5)
    assert not ok(n, dqnr(), comm(), 0.0, None, 20)  # online and target of different types
    assert not ok(n, M.DQN(D, [512, 256], 4), M.DQN(D, [512, 256], 4), 0.0, None, 20)
    assert not ok(n, M.DGN(D, [512, 256], 4, 8, 2), M.DGN(D, [512, 256], 4, 8, 2), 0.0, None, 20)


@gpu
def test_cli_dispatch(tmp_path, monkeypatch):
    """main.main with --netmon --model=dqnr at the small shape, 30 steps, --sequence-length 3 and 3 sequences per
    update: every update goes through agent_netmon_update_seq. (The same run at --sequence-length 1 is not repeated
    here: it ended in an illegal memory access when it was run together with a fused rollout Q pass for DQNR that is
    not part of the tree, and the cause is not known; main.py's `sequence_length > 1` condition on this branch has
    no test.)"""
    Lq, n_seq = 3, 3
    main = importlib.import_module("graph-marl_amd.main")
    ANS = U.mods()[6]
    calls = []
    real = ANS.agent_netmon_update_seq

    def spy(*a, **kw):
        calls.append(a[5].action.shape)
        return real(*a, **kw)

    monkeypatch.setattr(ANS, "agent_netmon_update_seq", spy)
    m = main.main(["--env-type=routing", "--model=dqnr", "--netmon", "--n-router=10", "--n-data=5",
                   "--hidden-dim=64,32", "--netmon-dim=32", "--netmon-encoder-dim=64,32", "--netmon-iterations=1",
                   "--n-env=2", "--total-steps=30", "--step-before-train=10", f"--mini-batch-size={n_seq}",
                   f"--sequence-length={Lq}", "--episode-steps=12", "--capacity=200", "--eval-episodes=2",
                   "--eval-episode-steps=5", "--disable-progressbar", f"--log-dir={tmp_path}"])
    monkeypatch.undo()
    assert m is not None
    assert len(calls) >= 15 and all(tuple(s) == (Lq, n_seq, 5) for s in calls), calls  # steps 10..30: one update each


def _state(mods_):
    return [copy.deepcopy(m.state_dict()) for m in mods_]


@gpu
@pytest.mark.parametrize("kind", ["dqnr", "commnet"])
def test_update_is_bit_reproducible_and_matches_per_step_update(kind):
    """agent_netmon_update_seq twice from the same state: loss, gradients, the parameters after AdamW and the target
    after its update are bit-equal. Once against train.dqn_update on the same batch, at the bounds of
    test_dgn_netmon_seq_gpu.py's test of the same name: the agent model's clipped gradients at 1e-5 + 1e-4 relative,
    the parameters after the AdamW step at 1e-6 (where |g| < 1e-5 the first step lr g / (|g| + eps) amplifies the
    gradient's own tolerance: that much more room, capped at 2 lr, for at most 1 % of the elements), the target
    after the soft update at 1e-6."""
    gm, M, FU, W, T, AS, ANS, RB, L = U.mods()
    netmon, model, target, rb, params = U.replayed(kind, "lstm", 3)
    batches, seq, _ = U.sample(rb, 3, 3)
    U.sequence_conditions(seq)
    lr, eps, gatol = 1e-3, 1e-8, 1e-5
    mods_ = (netmon, model, target)
    s0 = _state(mods_)

    def run(fn):
        for m, s in zip(mods_, s0):
            m.load_state_dict(s)
        netmon.state = None
        model.state = None
        for p in params:
            p.grad = None
        opt = torch.optim.AdamW(params, lr=lr)
        loss = fn(opt)
        netmon.state = None
        model.state = None
        return loss, [p.detach().clone() for p in params], [p.grad.clone() for p in params], _state((target,))[0]

    new = lambda opt: ANS.agent_netmon_update_seq(netmon, model, target, opt, params, seq, 0.98, 0.01)[0]  # noqa: E731
    la, pa, ga, ta = run(new)
    lb, pb, gb, tb = run(new)
    assert torch.equal(la, lb)
    for a, b in zip(pa + ga + list(ta.values()), pb + gb + list(tb.values())):
        assert torch.equal(a, b)
    lib = FU._setup()
    lib.gm_gemm_set_tile(0)  # both paths on one GEMM tile, as in compare_with_per_step
    try:
        la, pa, ga, ta = run(new)
        lc, pc, gc, tc = run(lambda opt: T.dqn_update(netmon, model, target, opt, params, batches, 0.98, 0.01,
                                                      consecutive=True)[0])
    finally:
        lib.gm_gemm_set_tile(-1)
    torch.testing.assert_close(la, lc, rtol=1e-4, atol=1e-5)
    names = [n for n, _ in list(model.named_parameters()) + list(netmon.named_parameters())]
    off = total = 0
    n_model = len(list(model.parameters()))
    for i, (n, p1, p2, g1, g2) in enumerate(zip(names, pa, pc, ga, gc)):
        if i < n_model:  # (NetMon's gradients: compare_with_per_step's Frobenius bound, checked there)
            torch.testing.assert_close(g1, g2, rtol=1e-4, atol=1e-5, msg=lambda s, n=n: f"clipped grad {n}: {s}")
        gabs = g2.abs()
        tol = torch.clamp(1e-6 + lr * eps * (gatol + 1e-4 * gabs) / (gabs + eps) ** 2, max=2 * lr)
        tol = torch.where(gabs < gatol, tol, torch.full_like(tol, 1e-6))
        d = (p1 - p2).abs()
        assert (d <= tol).all(), (n, (d - tol).max().item())
        off, total = off + int((d > 1e-6).sum()), total + d.numel()
    print(f"AdamW step: {off} of {total} elements beyond 1e-6")
    assert off <= 0.01 * total
    for k in ta:
        torch.testing.assert_close(ta[k], tc[k], rtol=0, atol=1e-6)


@gpu
@pytest.mark.parametrize("kind", ["dqnr", "commnet"])
def test_agent_seq_update_launches_unchanged(kind):
    """One agent_seq.agent_update_seq call (no NetMon) launches what it launched before _forward / _backward /
    _target_max took their hooks: the launch tags and the kernel after every library call equal the lists recorded
    at the parent commit (tests/golden/agent_seq_trace.json)."""
    with open(os.path.join(R.GOLDEN, "agent_seq_trace.json")) as f:
        want = json.load(f)[kind]
    got = U.agent_update_trace(kind)
    assert len(got["kernels"]) > 20
    assert got["tags"] == want["tags"]
    assert got["kernels"] == want["kernels"]


@gpu
@pytest.mark.parametrize("case", sorted(DU.TRACE_CASES))
def test_dqn_netmon_update_launches_unchanged(case):
    """The DQN + NetMon update's launch list still equals tests/golden/train_seq_trace.json."""
    with open(os.path.join(R.GOLDEN, "train_seq_trace.json")) as f:
        want = json.load(f)[case]
    got = DU.dqn_update_trace(case)
    assert got["tags"] == want["tags"]
    assert got["kernels"] == want["kernels"]


def _golden(kind):
    """The reference's DQNR / CommNet + NetMon update (tests/golden/make_golden_agent_netmon.py): (g, netmon, model,
    target, the AgentNetMonSeqBatch, the per-step TransitionBatches, parameter names)."""
    gm, M, FU, W, T, AS, ANS, RB, L = U.mods()
    g = np.load(os.path.join(R.GOLDEN, f"train_{kind}_netmon.npz"))
    assert str(g["arch_model"]) == kind
    _, _, K, H, enc, hidden = str(g["arch"]).split("|")
    K, H, hidden = int(K), int(H), [int(h) for h in hidden.split(",")]
    f = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    sd = lambda p: {k[len(p):]: torch.as_tensor(g[k]) for k in g.files if k.startswith(p)}  # noqa: E731
    od = g["agent_obs"].shape[-1]
    netmon = M.NetMon(g["node_obs"].shape[-1], H, [int(e) for e in enc.split(",")], K)
    make = (lambda: M.DQNR(od + 4 * H, hidden, 4)) if kind == "dqnr" else (lambda: M.CommNet(od + 4 * H, hidden, 4, 2))
    model, target = make(), make()
    netmon.load_state_dict(sd("netmon_"))
    model.load_state_dict(sd("model_"))
    target.load_state_dict({k: v for k, v in sd("target_").items() if not k.startswith("after_")})
    netmon, model, target = netmon.cuda().train(), model.cuda().train(), target.cuda()
    Lq = g["actions"].shape[0]
    odp = (od + 3) // 4 * 4
    obs = F.pad(f(g["agent_obs"]), (0, odp - od))  # [L + 1, B, A, odp]
    nbr = torch.stack([M.dense_to_nbr(f(g["node_adj"][t]).float()) for t in range(Lq + 1)])
    an = torch.stack([M.node_agent_to_index(f(g["node_agent"][t]).float()) for t in range(Lq + 1)])
    node_obs, adj = f(g["node_obs"]), f(g["agent_adj"]).to(torch.int8)
    comm = kind == "commnet"

    def next_fields(t, rows):
        r = slice(None) if rows is None else rows
        return obs[t + 1][r], node_obs[t + 1][r], an[t + 1][r].contiguous()

    act, rew, done, ep = f(g["actions"]).long(), f(g["reward"]), f(g["done"]).bool(), f(g["episode_done"]).bool()
    seq = ANS.AgentNetMonSeqBatch(obs[:Lq].contiguous(), od, act, rew, done, ep, node_obs[:Lq].contiguous(),
                                  nbr[:Lq].contiguous(), an[:Lq].contiguous(), f(g["node_state0"]), next_fields,
                                  adj[:Lq].contiguous() if comm else None, obs[1:].contiguous(),
                                  adj[1:].contiguous() if comm else None, f(g["agent_state0"]))
    batches = [RB.TransitionBatch(None, obs[t][..., :od], act[t], rew[t], obs[t + 1][..., :od], done[t], ep[t],
                                  node_obs[t], nbr[t].contiguous(), f(g["node_state0"]) if t == 0 else None,
                                  an[t].contiguous(), node_obs[t + 1], an[t + 1].contiguous(), adj[t].float(),
                                  adj[t + 1].float(), f(g["agent_state0"]) if t == 0 else None) for t in range(Lq)]
    names = [f"model_{k}" for k, _ in model.named_parameters()] + [f"netmon_{k}" for k, _ in netmon.named_parameters()]
    assert names == list(g["param_names"])
    return g, netmon, model, target, seq, batches, names


@gpu
@pytest.mark.parametrize("path", ["per_step", "batched"])
@pytest.mark.parametrize("kind", ["dqnr", "commnet"])
def test_update_matches_reference_golden(kind, path):
    """The reference's own DQNR / CommNet + NetMon update (6 nodes, 5 agents, NetMon H = 32 with encoder (16, 32),
    K = 2, agent encoder (24, 32), L = 3, B = 3; episode ends at steps 0 and 1, done agents in two sequences, one
    sequence with neither) at the tolerances test_agent_seq_gpu.py applies to train_dqnr.npz / train_commnet.npz: q
    and targets 1e-5, the loss 1e-5 relative, then test_train_gpu.check_update (raw and clipped gradients, AdamW
    step, target update). "per_step": train.dqn_loss on the same fixture (it passes without agent_netmon_seq.py
    too), so a failure can be attributed to one side."""
    from test_train_gpu import check_update

    gm, M, FU, W, T, AS, ANS, RB, L = U.mods()
    g, netmon, model, target, seq, batches, names = _golden(kind)
    U.sequence_conditions(seq)
    gamma = float(g["gamma"])
    params = list(model.parameters()) + list(netmon.parameters())
    opt = torch.optim.AdamW(params, lr=float(g["lr"]))
    parts = {}
    if path == "batched":
        assert ANS.agent_netmon_seq_ok(netmon, model, target, 0.0, None, seq.action.shape[2])
        loss, q, qt = ANS.agent_netmon_seq_loss(netmon, model, target, seq, gamma, params, parts)
    else:
        loss, q, qt = T.dqn_loss(netmon, model, target, batches, gamma, parts=parts, consecutive=True)
    for t in range(len(batches)):
        print(f"{kind} {path} step {t}: max |dq| {np.abs(q[t].detach().cpu().numpy() - g[f'q_{t}']).max():.3g}, "
              f"max |dtarget| {np.abs(qt[t].cpu().numpy() - g[f'qtarget_{t}']).max():.3g}")
    print(f"{kind} {path}: loss {loss.item():.8g} (golden {g['loss'].item():.8g})")
    for t in range(len(batches)):
        np.testing.assert_allclose(q[t].detach().cpu().numpy(), g[f"q_{t}"], atol=1e-5, rtol=0, err_msg=f"q_{t}")
        np.testing.assert_allclose(qt[t].cpu().numpy(), g[f"qtarget_{t}"], atol=1e-5, rtol=0, err_msg=f"qtarget_{t}")
    np.testing.assert_allclose(parts["loss_q"].item(), g["loss_q"].item(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(loss.item(), g["loss"].item(), rtol=1e-5, atol=1e-6)
    opt.zero_grad()
    loss.backward()
    netmon.state = None
    check_update(g, names, params, opt, model, target, T)
