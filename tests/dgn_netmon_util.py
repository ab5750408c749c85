"""Shared fixtures of tests/test_dgn_netmon_seq_gpu.py: a small replayed rollout with NetMon graph observations and
agent adjacencies, and a recorder of the library launches one call makes."""
import importlib

import torch

N_S, H_S, ENC_S = 6, 32, [16, 32]  # the small shape: 6 nodes, NetMon hidden 32, encoder (16, 32)
RB_SEED = 1  # np.random.default_rng(1).choice(6, 2) = [2, 3]: the sequences (env 0, start slot 2), (env 1, start slot 0)


def mods():
    names = ("", ".model", ".fused", ".wrapper", ".train", ".train_seq", ".dgn_seq", ".replaybuffer", "._lib")
    return tuple(importlib.import_module("graph-marl_amd" + n) for n in names)


def small_dgn(M, in_features, hidden=32, heads=2, layers=2, d=8, activation="leaky_relu"):
    """DGN with hidden 32, 2 attention layers of 2 heads with dk = dv = 8 (the constructor's layers are 16 wide)."""
    m = M.DGN(in_features, [hidden], 4, heads, layers, activation=activation)
    m.att_layers = torch.nn.ModuleList([M.AttModel(hidden, d, d, hidden, heads, activation) for _ in range(layers)])
    return m


def replayed(kind, rnn="lstm", K=1, glob=False, agg="sum", A=5, N=N_S, n_env=2, slots=6, ep_end=3, seed=7,
             model_fn=None):
    """n_env routing envs with N nodes and A agents under a NetMonWrapper (H = 32, encoder (16, 32)): two warm-up
    steps with random actions, then `slots` recorded steps; the episode ends at recorded step `ep_end` (the wrapper
    resets). Agent (slot + env) % A is marked done in every slot, so every step of every sequence has a done agent
    (and not only done agents). kind "dgn": DGN (hidden 32, 2 layers, 2 heads, dk = dv = 8) with the agent
    adjacency stored; "dqn": DQN [32, 32]. Returns (netmon, model, target, rb, params)."""
    gm, M, FU, W, T, S, DS, RB, L = mods()
    H = H_S
    gw = (5 if glob else 4) * H
    env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A, n_env=n_env, seed=seed,
                     obs_extra=gw, agent_adjacency=kind == "dgn")
    torch.manual_seed(100 * K + len(rnn) + int(glob))
    netmon = M.NetMon(4 * N + 8, H, list(ENC_S), K, rnn_type=rnn, agg_type=agg, output_global_hidden=glob).cuda()
    D = env.obs_dim + gw
    if model_fn is not None:
        model, target = model_fn(D).cuda(), model_fn(D).cuda()
    elif kind == "dgn":
        model, target = small_dgn(M, D).cuda(), small_dgn(M, D).cuda()
    else:
        model, target = M.DQN(D, [32, 32], 4).cuda(), M.DQN(D, [32, 32], 4).cuda()
    target.load_state_dict(model.state_dict())
    with torch.no_grad():  # the attention query / key weights perturbed more, so that the KL is not ~0
        for k, p in target.named_parameters():
            p.add_((0.3 if ("fc_q" in k or "fc_k" in k) else 0.01) * torch.randn_like(p))
    wenv = W.NetMonWrapper(env, netmon, 1)
    rb = RB.ReplayBuffer(RB_SEED, 8 * n_env, n_env, A, env.obs_dim, N, 4 * N + 8, netmon.get_state_size(), "cuda",
                         store_adj=kind == "dgn")
    wenv.reset_()
    gen = torch.Generator().manual_seed(seed)
    for t in range(-2, slots):
        if t >= 0:
            rb.add_pre(env.obs, wenv.last_netmon_state, env.node_obs, env.nbr, env.agent_node,
                       adj=env.agent_adj if kind == "dgn" else None)
        act = torch.randint(0, 4, (n_env, A), generator=gen).to(torch.int32).cuda()
        wenv.step_(act)
        if t >= 0:
            done = env.done.bool().clone()
            done[:] = False
            for e in range(n_env):
                done[e, (t + e) % A] = True
            rb.add_post(act, env.reward, env.obs, done, t == ep_end, env.node_obs, env.agent_node,
                        next_adj=env.agent_adj if kind == "dgn" else None)
        if t == ep_end:
            wenv.reset_()
    netmon.state = None
    netmon.train()
    model.train()
    params = list(model.parameters()) + list(netmon.parameters())
    return netmon, model, target, rb, params


def launch_trace(fn):
    """(tags, names) of fn(): the launch tags (_lib.TRACE) and gm_last_kernel after every checked library call."""
    L = mods()[-1]
    names = []
    real = L.check

    def spy(rc):
        real(rc)
        names.append(L.last_kernel())

    L.check = spy
    L.TRACE = []
    try:
        fn()
    finally:
        tags, L.TRACE = L.TRACE, None
        L.check = real
    return tags, names


TRACE_CASES = {"lstm": ("lstm", 1, False), "gru": ("gru", 2, False), "lnlstm": ("lnlstm", 1, False),
               "global": ("lstm", 2, True)}


def dqn_update_trace(case):
    """The launches of one train_seq.dqn_update_seq call (DQN + NetMon, L = 3, 2 sequences) at the small shape."""
    gm, M, FU, W, T, S, DS, RB, L = mods()
    rnn, K, glob = TRACE_CASES[case]
    netmon, model, target, rb, params = replayed("dqn", rnn, K, glob)
    M.tag_modules(netmon, "netmon.")
    M.tag_modules(model, "dqn.")
    M.tag_modules(target, "dqn_tar.")
    assert S.seq_ok(netmon, model, target)
    seq = rb.get_sequences(2, 3)
    opt = torch.optim.AdamW(params, lr=1e-3)
    tags, names = launch_trace(lambda: S.dqn_update_seq(netmon, model, target, opt, params, seq, 0.98, 0.01))
    torch.cuda.synchronize()
    return {"tags": tags, "kernels": names}
