"""Sequence-batched DGN + NetMon update (graph-marl_amd/dgn_netmon_seq.py): against the per-step autograd path
(train.dqn_loss / train.dqn_update) on the same sampled transitions, the sampler against get_batch / get_sequences /
get_dgn_sequences, the dispatch predicate and the CLI branch, run-to-run bit equality of the update, and the launch
list of the DQN + NetMon update (train_seq.dqn_update_seq) against the list recorded before train_seq.py was split
at the readout boundary (tests/golden/train_seq_trace.json).

Small shape (dgn_netmon_util.py): N = 6 nodes, H = 32, NetMon encoder (16, 32), DGN hidden 32 with 2 attention layers
of 2 heads, dk = dv = 8; A = 5 agents (several share a node: the readout backward accumulates), L = 3, B = 2, one
sequence with episode_done at step 1 (the state mask and the target's own NetMon step), one done agent per step."""
import copy
import importlib
import json
import os

import pytest
import torch

import dgn_netmon_util as U
import golden_replay as R

gpu = pytest.mark.gpu


def dns():
    return importlib.import_module("graph-marl_amd.dgn_netmon_seq")


def _fro(a, b):
    return (a.double() - b.double()).norm().item() / max(b.double().norm().item(), 1e-30)


def _sample(rb, n_seq, Lq):
    """The same draw through get_batch and get_dgn_netmon_sequences; the stream ends in the same state."""
    rng0 = rb.rng.clone()
    batches = list(rb.get_batch(n_seq, sequence_length=Lq))
    rng1, st1 = rb.rng.clone(), rb.rng_state()
    rb.rng.copy_(rng0)
    seq = rb.get_dgn_netmon_sequences(n_seq, Lq)
    assert torch.equal(rb.rng, rng1) and rb.rng_state() == st1
    for t, b in enumerate(batches):
        assert torch.equal(b.idx[0], seq.idx[0][t]) and torch.equal(b.idx[1], seq.idx[1])
    return batches, seq, rng0


def _grads(params, loss):
    for p in params:
        p.grad = None
    loss.backward()
    return [p.grad.clone() for p in params]


def _compare_with_per_step(netmon, model, target, batches, seq, params, coeff):
    """loss, loss_q, loss_att, q, targets and DGN's gradients at the bounds of test_dgn_seq_gpu.py::
    _compare_with_per_step (1e-5 + 1e-4 relative); NetMon's gradients at the bound of test_train_seq_gpu.py::
    _compare_paths on a common GEMM tile (Frobenius-relative error against the exact-fp32 per-step gradients below
    max(2e-5, twice the per-step path's own)). Returns the worst error / tolerance ratio."""
    gm, M, FU, W, T, S, DS, RB, L = U.mods()
    DNS = dns()
    lib = FU._setup()
    lib.gm_gemm_set_tile(0)
    try:
        p0 = {}
        netmon.state = None
        l0, q0, t0 = T.dqn_loss(netmon, model, target, batches, 0.98, att_coeff=coeff, parts=p0, consecutive=True)
        g0 = _grads(params, l0)
        netmon.state = None
        p1 = {}
        l1, q1, t1 = DNS.dgn_netmon_seq_loss(netmon, model, target, seq, 0.98, params, coeff, p1)
        g1 = _grads(params, l1)
        netmon.state = None
        old = L.GEMM_MODE
        L.GEMM_MODE = "f32"  # exact-fp32 reference: the per-step path with every GEMM in fp32
        try:
            lf, _, _ = T.dqn_loss(netmon, model, target, batches, 0.98, att_coeff=coeff, consecutive=True)
            gf = _grads(params, lf)
        finally:
            L.GEMM_MODE = old
    finally:
        lib.gm_gemm_set_tile(-1)
        netmon.state = None
    rtol, atol = 1e-4, 1e-5
    worst = 0.0

    def ratio(a, b):
        a, b = a.detach().double(), b.detach().double()
        return ((a - b).abs() / (atol + rtol * b.abs())).max().item()

    pairs = [("loss", l1, l0), ("loss_q", p1["loss_q"], p0["loss_q"])]
    if coeff > 0:
        pairs.append(("loss_att", p1["loss_att"], p0["loss_att"]))
    else:
        assert p1["loss_att"] is None and p0["loss_att"] is None
    for t in range(len(batches)):
        pairs += [(f"q_{t}", q1[t], q0[t]), (f"q_target_{t}", t1[t], t0[t])]
    names = [n for n, _ in list(model.named_parameters()) + list(netmon.named_parameters())]
    n_model = len(list(model.parameters()))
    for n, a, b in zip(names[:n_model], g1, g0):
        assert a.shape == b.shape, n
        pairs.append(("grad " + n, a, b))
    fails = []
    for n, a, b in pairs:
        r = ratio(a, b)
        print(f"{n}: error / tolerance {r:.3g}")
        worst = max(worst, r)
        if not r <= 1:
            fails.append((n, r))
    for n, a, b, c in zip(names[n_model:], g0[n_model:], g1[n_model:], gf[n_model:]):
        e_old, e_new = _fro(a, c), _fro(b, c)
        bound = max(2e-5, 2 * e_old)
        print(f"grad netmon.{n}: Frobenius-relative error vs exact fp32: per-step {e_old:.3g}, batched {e_new:.3g} "
              f"(bound {bound:.3g})")
        worst = max(worst, e_new / bound)
        if not e_new < bound:
            fails.append((n, e_old, e_new))
    print(f"worst error / tolerance: {worst:.3g}")
    assert not fails, fails
    return worst


# (rnn, K, global, A, N, L): the main case at K = 1 and 2, one case each for gru, lnlstm and the global mean, and the
# default CLI shape class (A = N = 20, L = 1)
CASES = [("lstm", 1, False, 5, 6, 3), ("lstm", 2, False, 5, 6, 3), ("gru", 1, False, 5, 6, 3),
         ("lnlstm", 1, False, 5, 6, 3), ("lstm", 1, True, 5, 6, 3), ("lstm", 1, False, 20, 20, 1)]


@gpu
@pytest.mark.parametrize("coeff", [0.0, 0.03])
@pytest.mark.parametrize("rnn,K,glob,A,N,Lq", CASES)
def test_matches_per_step_path(rnn, K, glob, A, N, Lq, coeff):
    """The transitions get_batch draws through train.dqn_loss and through dgn_netmon_seq_loss."""
    gm, M, FU, W, T, S, DS, RB, L = U.mods()
    netmon, model, target, rb, params = U.replayed("dgn", rnn, K, glob, A=A, N=N)
    assert dns().dgn_netmon_seq_ok(netmon, model, target, coeff, None, A)
    batches, seq, _ = _sample(rb, 2, Lq)
    if Lq == 3:
        assert seq.episode_done[1].tolist() == [True, False] and not seq.episode_done[0].any()
    assert all(seq.done[t].any() and not seq.done[t].all() for t in range(Lq))
    _compare_with_per_step(netmon, model, target, batches, seq, params, coeff)


@gpu
@pytest.mark.parametrize("Lq", [1, 3])
def test_sampler_fields(Lq):
    """get_dgn_netmon_sequences draws get_batch's indices from the same stream state and leaves the stream where
    get_batch leaves it (_sample); its fields are the bits get_batch, get_dgn_sequences and (L = 3; at L = 1
    get_sequences draws start slots, not get_batch's uniform (slot, env) pairs) get_sequences gather."""
    gm, M, FU, W, T, S, DS, RB, L = U.mods()
    netmon, model, target, rb, params = U.replayed("dgn")
    n_seq = 4
    batches, seq, rng0 = _sample(rb, n_seq, Lq)
    od = rb.obs_dim
    assert seq.adj.dtype == torch.int8 and seq.next_adj.dtype == torch.int8 and seq.obs_dim == od
    for t, b in enumerate(batches):
        nf = seq.next_fields(t, None)
        for name, got, want in (
                ("obs", seq.obs[t][..., :od], b.obs), ("action", seq.action[t], b.action),
                ("reward", seq.reward[t], b.reward), ("done", seq.done[t], b.done),
                ("episode_done", seq.episode_done[t].expand(n_seq), b.episode_done.expand(n_seq)),
                ("node_obs", seq.node_obs[t], b.node_obs), ("nbr", seq.nbr[t], b.nbr),
                ("agent_node", seq.agent_node[t], b.agent_node), ("adj", seq.adj[t], b.adj.to(torch.int8)),
                ("next_adj", seq.next_adj[t], b.next_adj.to(torch.int8)),
                ("next_obs", seq.next_obs[t][..., :od], b.next_obs), ("next_fields obs", nf[0][..., :od], b.next_obs),
                ("next_node_obs", nf[1], b.next_node_obs), ("next_agent_node", nf[2], b.next_agent_node)):
            assert got.dtype == want.dtype and torch.equal(got, want), (t, name)
    assert torch.equal(seq.node_state, batches[0].node_state)
    r = torch.tensor([2, 0], device="cuda")
    for a, b in zip(seq.next_fields(Lq - 1, r), seq.next_fields(Lq - 1, None)):
        assert torch.equal(a, b[r])
    rb.rng.copy_(rng0)
    d = rb.get_dgn_sequences(n_seq, Lq)
    others = [(d, ("obs", "action", "reward", "done", "episode_done", "adj", "next_obs", "next_adj"))]
    if Lq > 1:
        rb.rng.copy_(rng0)
        others.append((rb.get_sequences(n_seq, Lq), ("obs", "action", "reward", "done", "episode_done", "node_obs",
                                                     "nbr", "agent_node", "node_state")))
    for o, fields in others:
        assert torch.equal(o.idx[0], seq.idx[0]) and torch.equal(o.idx[1], seq.idx[1]) and o.obs_dim == seq.obs_dim
        for f in fields:
            got, want = getattr(seq, f), getattr(o, f)
            assert got.dtype == want.dtype and torch.equal(got, want), f
    if Lq > 1:
        for a, b in zip(seq.next_fields(1, r), others[1][0].next_fields(1, r)):
            assert torch.equal(a, b)


def test_dispatch_predicate():
    """True for the default configuration (lstm, gru, lnlstm, the global mean); False for the aux loss,
    --netmon-rnn-carryover 0, another activation (either half), GM_GEMM=f32, more than 64 agents, no NetMon, and
    the models of the other batched paths."""
    gm, M, FU, W, T, S, DS, RB, L = U.mods()
    ok = dns().dgn_netmon_seq_ok
    D = 130 + 512
    dgn = lambda **kw: M.DGN(D, [512, 256], 4, 8, 2, **kw)  # noqa: E731
    nm = lambda **kw: M.NetMon(88, 128, [512, 256], 1, **kw)  # noqa: E731
    m, tar, n = dgn(), dgn(), nm()
    assert ok(n, m, tar, 0.03, None, 20) and ok(n, m, tar, 0.0, None, 64) and ok(n, m, tar, 0.03)
    for rnn in ("gru", "lnlstm"):
        assert ok(nm(rnn_type=rnn), m, tar, 0.03, None, 20)
    assert ok(nm(output_global_hidden=True), M.DGN(D + 128, [512, 256], 4, 8, 2), M.DGN(D + 128, [512, 256], 4, 8, 2),
              0.03, None, 20)
    sm = U.small_dgn(M, 46 + 128)
    assert ok(M.NetMon(32, 32, [16, 32], 2), sm, sm, 0.03, None, 5)
    assert not ok(n, m, tar, 0.03, M.MLP(256, [256, 20], activation_on_output=False), 20)  # aux loss
    assert not ok(nm(rnn_carryover=False), m, tar, 0.03, None, 20)
    assert not ok(nm(activation="relu"), m, tar, 0.03, None, 20)
    assert not ok(n, dgn(activation="relu"), dgn(activation="relu"), 0.03, None, 20)
    assert not ok(n, m, tar, 0.03, None, 65)
    assert not ok(None, m, tar, 0.03, None, 20)
    assert not ok(M.NetMon(88, 48, [512, 256], 1), m, tar, 0.03, None, 20)  # H % 32
    assert not ok(n, M.DQN(D, [512, 256], 4), M.DQN(D, [512, 256], 4), 0.0, None, 20)
    assert not ok(n, m, tar, -0.1, None, 20)
    # the other batched paths keep refusing this configuration
    assert not S.seq_ok(n, m, tar, 0.03, None) and not DS.dgn_seq_ok(m, tar, n, 0.03, None, 20)
    old = L.GEMM_MODE
    L.GEMM_MODE = "f32"
    try:
        assert not ok(n, m, tar, 0.03, None, 20)
    finally:
        L.GEMM_MODE = old


@gpu
def test_cli_takes_the_batched_branch(tmp_path, monkeypatch):
    """main.main with --netmon --model=dgn at the small shape, 30 steps: gm_agent_attention_bwd and a NetMon cell
    backward are launched within one update (between two L.check_range calls), which only the batched node does:
    the per-step path's attention core is torch."""
    gm, M, FU, W, T, S, DS, RB, L = U.mods()
    main = importlib.import_module("graph-marl_amd.main")
    segments = [[]]
    real_check, real_range = L.check, L.check_range

    def spy(rc):
        real_check(rc)
        segments[-1].append(L.last_kernel())

    def range_spy():
        segments.append([])
        return real_range()

    monkeypatch.setattr(L, "check", spy)
    monkeypatch.setattr(L, "check_range", range_spy)
    m = main.main(["--env-type=routing", "--model=dgn", "--netmon", "--n-router=6", "--n-data=5", "--hidden-dim=32",
                   "--num-heads=2", "--netmon-dim=32", "--netmon-encoder-dim=16,32", "--netmon-iterations=1",
                   "--n-env=2", "--total-steps=30", "--step-before-train=10", "--mini-batch-size=2",
                   "--sequence-length=3", "--episode-steps=12", "--capacity=200", "--eval-episodes=2",
                   "--eval-episode-steps=5", "--disable-progressbar", f"--log-dir={tmp_path}"])
    monkeypatch.undo()
    assert m is not None
    both = [s for s in segments if any(k.startswith("k_agent_attention_bwd") for k in s)
            and any(k.startswith("k_lstm_cell_bwd") for k in s)]
    assert len(both) >= 15, len(both)  # steps 10..30 each end with one update
    assert all(any(k.startswith("k_agent_attention_kl") for k in s) for s in both)  # the default coefficient 0.03


def _state(mods_):
    return [copy.deepcopy(m.state_dict()) for m in mods_]


@gpu
def test_update_is_bit_reproducible_and_matches_per_step_update():
    """dgn_netmon_update_seq twice from the same state: the parameters after AdamW and the target update are
    bit-equal (no atomics on this path). Once against train.dqn_update on the same batch: DGN's clipped gradients at
    1e-5 + 1e-4 relative, the parameters after the AdamW step at test_train_gpu.check_update's tolerance (1e-6;
    where |g| < 1e-5 the first step lr g / (|g| + eps) amplifies the gradient's own tolerance: that much more room,
    capped at 2 lr, for at most 1 % of the elements), the target after the soft update at 1e-6."""
    gm, M, FU, W, T, S, DS, RB, L = U.mods()
    DNS = dns()
    netmon, model, target, rb, params = U.replayed("dgn", "lstm", 2)
    batches, seq, _ = _sample(rb, 2, 3)
    lr, eps, gatol = 1e-3, 1e-8, 1e-5
    mods_ = (netmon, model, target)
    s0 = _state(mods_)

    def run(fn):
        for m, s in zip(mods_, s0):
            m.load_state_dict(s)
        netmon.state = None
        for p in params:
            p.grad = None
        opt = torch.optim.AdamW(params, lr=lr)
        loss = fn(opt)
        netmon.state = None
        return loss, [p.detach().clone() for p in params], [p.grad.clone() for p in params], _state((target,))[0]

    new = lambda opt: DNS.dgn_netmon_update_seq(netmon, model, target, opt, params, seq, 0.98, 0.01,  # noqa: E731
                                                att_coeff=0.03)[0]
    la, pa, ga, ta = run(new)
    lb, pb, gb, tb = run(new)
    assert torch.equal(la, lb)
    for a, b in zip(pa + ga + list(ta.values()), pb + gb + list(tb.values())):
        assert torch.equal(a, b)
    lib = FU._setup()
    lib.gm_gemm_set_tile(0)  # both paths on one GEMM tile, as in _compare_with_per_step
    try:
        la, pa, ga, ta = run(new)
        lc, pc, gc, tc = run(lambda opt: T.dqn_update(netmon, model, target, opt, params, batches, 0.98, 0.01,
                                                      att_coeff=0.03, consecutive=True)[0])
    finally:
        lib.gm_gemm_set_tile(-1)
    torch.testing.assert_close(la, lc, rtol=1e-4, atol=1e-5)
    names = [n for n, _ in list(model.named_parameters()) + list(netmon.named_parameters())]
    off = total = 0
    n_model = len(list(model.parameters()))
    for i, (n, p1, p2, g1, g2) in enumerate(zip(names, pa, pc, ga, gc)):
        if i < n_model:  # (NetMon's gradients: _compare_with_per_step's Frobenius bound, checked there)
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
@pytest.mark.parametrize("case", sorted(U.TRACE_CASES))
def test_dqn_netmon_update_launches_unchanged(case):
    """One train_seq.dqn_update_seq call at the small shape launches what it launched before _forward / _backward
    were split into their NetMon and DQN parts: the launch tags and the kernel after every library call equal the
    lists recorded at the parent commit (lstm, gru, lnlstm, global mean)."""
    with open(os.path.join(R.GOLDEN, "train_seq_trace.json")) as f:
        want = json.load(f)[case]
    got = U.dqn_update_trace(case)
    assert got["tags"] == want["tags"]
    assert got["kernels"] == want["kernels"]


def _golden():
    """The reference's DGN + NetMon update (tests/golden/make_golden_dgn_netmon.py): (g, netmon, model, target, the
    DGNNetMonSeqBatch, the per-step TransitionBatches, parameter names)."""
    import numpy as np
    import torch.nn.functional as F

    gm, M, FU, W, T, S, DS, RB, L = U.mods()
    g = np.load(os.path.join(R.GOLDEN, "train_dgn_netmon.npz"))
    _, _, K, H, enc, hidden, heads, layers = str(g["arch"]).split("|")
    K, H, heads, layers = int(K), int(H), int(heads), int(layers)
    f = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    sd = lambda p: {k[len(p):]: torch.as_tensor(g[k]) for k in g.files if k.startswith(p)}  # noqa: E731
    od = g["agent_obs"].shape[-1]
    netmon = M.NetMon(g["node_obs"].shape[-1], H, [int(e) for e in enc.split(",")], K)
    model = M.DGN(od + 4 * H, [int(hidden)], 4, heads, layers)
    target = M.DGN(od + 4 * H, [int(hidden)], 4, heads, layers)
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

    def next_fields(t, rows):
        r = slice(None) if rows is None else rows
        return obs[t + 1][r], node_obs[t + 1][r], an[t + 1][r].contiguous()

    act, rew, done, ep = f(g["actions"]).long(), f(g["reward"]), f(g["done"]).bool(), f(g["episode_done"]).bool()
    seq = dns().DGNNetMonSeqBatch(obs[:Lq].contiguous(), od, act, rew, done, ep, node_obs[:Lq].contiguous(),
                                  nbr[:Lq].contiguous(), an[:Lq].contiguous(), f(g["node_state0"]), next_fields,
                                  adj[:Lq].contiguous(), obs[1:].contiguous(), adj[1:].contiguous())
    batches = [RB.TransitionBatch(None, obs[t][..., :od], act[t], rew[t], obs[t + 1][..., :od], done[t], ep[t],
                                  node_obs[t], nbr[t].contiguous(), f(g["node_state0"]) if t == 0 else None,
                                  an[t].contiguous(), node_obs[t + 1], an[t + 1].contiguous(), adj[t].float(),
                                  adj[t + 1].float(), None) for t in range(Lq)]
    names = [f"model_{k}" for k, _ in model.named_parameters()] + [f"netmon_{k}" for k, _ in netmon.named_parameters()]
    assert names == list(g["param_names"])
    return g, netmon, model, target, seq, batches, names


@gpu
@pytest.mark.parametrize("path", ["per_step", "batched"])
def test_update_matches_reference_golden(path):
    """The reference's own DGN + NetMon update (6 nodes, 5 agents, NetMon H = 32 with encoder (16, 32), K = 2, DGN
    hidden 32 with 2 heads and 2 layers, L = 3, B = 2, one episode end at step 1, a done agent per step, coefficient
    0.03) at the bounds test_models_gpu.py uses for train_dgn.npz: q and targets 1e-5, loss_q and the loss 1e-5
    relative, loss_att 2e-3 relative, then test_train_gpu.check_update (raw and clipped gradients, AdamW step,
    target update). "per_step": train.dqn_loss on the same fixture (it passes without dgn_netmon_seq.py too), so a
    failure can be attributed to one side."""
    import numpy as np
    from test_train_gpu import check_update

    gm, M, FU, W, T, S, DS, RB, L = U.mods()
    g, netmon, model, target, seq, batches, names = _golden()
    coeff, gamma = float(g["att_coeff"]), float(g["gamma"])
    params = list(model.parameters()) + list(netmon.parameters())
    opt = torch.optim.AdamW(params, lr=float(g["lr"]))
    parts = {}
    if path == "batched":
        assert dns().dgn_netmon_seq_ok(netmon, model, target, coeff, None, seq.action.shape[2])
        loss, q, qt = dns().dgn_netmon_seq_loss(netmon, model, target, seq, gamma, params, coeff, parts)
    else:
        loss, q, qt = T.dqn_loss(netmon, model, target, batches, gamma, att_coeff=coeff, parts=parts, consecutive=True)
    for t in range(len(batches)):
        print(f"{path} step {t}: max |dq| {np.abs(q[t].detach().cpu().numpy() - g[f'q_{t}']).max():.3g}, max |dtarget| "
              f"{np.abs(qt[t].cpu().numpy() - g[f'qtarget_{t}']).max():.3g}")
    print(f"{path}: loss_q {parts['loss_q'].item():.8g} (golden {g['loss_q'].item():.8g}), loss_att "
          f"{parts['loss_att'].item():.8g} (golden {g['loss_att'].item():.8g})")
    for t in range(len(batches)):
        np.testing.assert_allclose(q[t].detach().cpu().numpy(), g[f"q_{t}"], atol=1e-5, rtol=0, err_msg=f"q_{t}")
        np.testing.assert_allclose(qt[t].cpu().numpy(), g[f"qtarget_{t}"], atol=1e-5, rtol=0, err_msg=f"qtarget_{t}")
    np.testing.assert_allclose(parts["loss_q"].item(), g["loss_q"].item(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(loss.item(), g["loss"].item(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(parts["loss_att"].item(), g["loss_att"].item(), rtol=2e-3, atol=1e-7)
    opt.zero_grad()
    loss.backward()
    netmon.state = None
    check_update(g, names, params, opt, model, target, T)
