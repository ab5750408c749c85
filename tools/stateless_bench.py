#!/usr/bin/env python3
"""The stateless NetMon (--netmon-rnn-type none), interleaved A/B in one process.

Kernel: gm_mp_iterate in its LDS-resident form (gm_mp_iterate_set_form(1)) against its chained form (form 0: K
gm_mp_aggregate_rows launches between the two outputs, plus the copy of h0 at K = 1), at G = 4096 graphs, H = 128,
N in {20, 100}, K in {1, 3, 8}, sum and mean; device-event time over `--reps` back-to-back calls, medians over
`--rounds` alternating rounds. Bytes moved: the LDS form reads the rows once and writes two images (3 G N H 4
bytes), the chain reads and writes one image per round (2 K of them, 4 at K = 1; the gathered reads hit L2). The
calls repeat on the same three images: at N = 20 (42 MB each) they stay in the 256 MB Infinity Cache, so those
rates are cache-hot rates, not HBM rates; at N = 100 (210 MB each) they do not fit.

Rollout: 4096 routing envs, N = 20 nodes and agents, NetMon H = 128, encoder 512,256, K = 8, sum, DQN 512,256;
NetMonWrapper(fused=True) (fused.netmon_step: encoder chain + one gm_mp_iterate, readout gathered in the DQN's first
GEMM) against NetMonWrapper(fused=False) (NetMon.forward_graph and a materialised joint observation), each on its
own envs; env-steps/s over `--steps` vector steps between device synchronisations.

Update: one full update, sampling included, on a replayed fused rollout (K = 8, sum): the sequence-batched update
(stateless_seq.dqn_update_stateless_seq) against the per-step path (train.dqn_update), alternating, at 32 sequences
x L = 1 and L = 8 (64 envs in the buffer) and 13 108 x 8 (4096 envs); ms per update, medians over the rounds.

Prints one JSON line. Usage: python tools/stateless_bench.py [--part kernel|rollout|update|all] [--rounds 7]
                                                             [--reps 200] [--steps 50] [--update-reps 3]
"""
import argparse
import copy
import importlib
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

G, H = 4096, 128


def mods():
    names = ("", ".model", ".wrapper", ".policy", "._lib")
    return tuple(importlib.import_module("graph-marl_amd" + n) for n in names)


def spread(v, med):
    return round((max(v) - min(v)) / med, 4)


def kernel(a):
    gm, M, W, P, L = mods()
    lib = L.lib()
    out = []
    for N in (20, 100):
        env = gm.Routing(gm.Network(N, random_topology=True), 4, n_env=G, seed=0, agent_adjacency=False)
        env.reset_()
        nbr = env.nbr.contiguous()
        deg = nbr.shape[-1]
        x = torch.nn.functional.leaky_relu(torch.randn(G * N, H, device="cuda"), 0.01)
        o, p = torch.empty_like(x), torch.empty_like(x)
        st = L.stream_ptr()
        for mode in (0, 1):
            for K in (1, 3, 8):
                def call():
                    L.check(lib.gm_mp_iterate(x.data_ptr(), H, nbr.data_ptr(), G, N, deg, H, mode, K, o.data_ptr(), H,
                                              p.data_ptr(), H, st))

                def timed(form):
                    L.check(lib.gm_mp_iterate_set_form(form))
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    return 1e3 * e0.elapsed_time(e1) / a.reps  # us per call

                L.check(lib.gm_mp_iterate_set_form(1))
                call()
                assert L.last_kernel() == "k_mp_iterate<fwd>", L.last_kernel()
                a_out, a_prev = o.clone(), p.clone()
                L.check(lib.gm_mp_iterate_set_form(0))
                call()
                assert L.last_kernel().startswith("k_mp_aggregate"), L.last_kernel()
                assert torch.equal(a_out, o) and torch.equal(a_prev, p), "forms differ"
                us = {"lds": [], "chain": []}
                for form in (1, 0):
                    timed(form)
                for _ in range(a.rounds):
                    us["lds"].append(timed(1))
                    us["chain"].append(timed(0))
                L.check(lib.gm_mp_iterate_set_form(-1))
                med = {k: statistics.median(v) for k, v in us.items()}
                img = G * N * H * 4
                out.append({"nodes": N, "mode": "mean" if mode else "sum", "iters": K,
                            "us": {k: round(v, 2) for k, v in med.items()},
                            "lds_over_chain": round(med["lds"] / med["chain"], 4),
                            "gbytes_per_s": {"lds": round(3 * img / med["lds"] / 1e3, 1),
                                             "chain": round(2 * max(K, 2) * img / med["chain"] / 1e3, 1)},
                            "spread": {k: spread(v, med[k]) for k, v in us.items()}})
    return out


def rollout(a):
    gm, M, W, P, L = mods()
    n_env, N, K = 4096, 20, 8
    torch.manual_seed(0)
    netmon = M.NetMon(4 * N + 8, H, [512, 256], K, rnn_type="none").cuda()
    model = M.DQN(6 * N + 10 + 4 * H, [512, 256], 4).cuda()
    runs = {}
    for name, fused in (("fused", True), ("unfused", False)):
        env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), N, n_env=n_env, seed=0,
                         obs_extra=4 * H, agent_adjacency=False)
        wenv = W.NetMonWrapper(env, copy.deepcopy(netmon), 1, fused=fused)
        assert wenv.fused == fused
        pol = P.EpsilonGreedy(wenv, model, epsilon=0.5, epsilon_decay=1.0, epsilon_update_freq=100,
                              step_before_train=0)
        wenv.reset_()
        runs[name] = (wenv, pol)

    def timed(name):
        wenv, pol = runs[name]
        with torch.no_grad():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                pol.act_step(wenv)
            torch.cuda.synchronize()
        return n_env * a.steps / (time.perf_counter() - t0)

    for name in runs:
        timed(name)
    sps = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name in runs:
            sps[name].append(timed(name))
    med = {k: statistics.median(v) for k, v in sps.items()}
    return {"envs": n_env, "nodes": N, "hidden": H, "iterations": K, "steps_per_round": a.steps,
            "env_steps_per_s": {k: round(v) for k, v in med.items()},
            "fused_over_unfused": round(med["fused"] / med["unfused"], 4),
            "spread": {k: spread(v, med[k]) for k, v in sps.items()}}


def update(a, n_env, bsz, Lq):
    gm, M, W, P, L = mods()
    T = importlib.import_module("graph-marl_amd.train")
    SS = importlib.import_module("graph-marl_amd.stateless_seq")
    RB = importlib.import_module("graph-marl_amd.replaybuffer")
    N = A = 20
    torch.manual_seed(0)
    netmon = M.NetMon(4 * N + 8, H, [512, 256], 8, rnn_type="none").cuda()
    model = M.DQN(6 * N + 10 + 4 * H, [512, 256], 4).cuda()
    model_tar = copy.deepcopy(model)
    params = list(model.parameters()) + list(netmon.parameters())
    opt = torch.optim.AdamW(params, lr=1e-4)
    assert SS.stateless_seq_ok(netmon, model, model_tar)
    env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A, n_env=n_env, seed=0,
                     obs_extra=4 * H, agent_adjacency=False)
    wenv = W.NetMonWrapper(env, netmon, 1, fused=True)
    pol = P.EpsilonGreedy(wenv, model, epsilon=0.5, epsilon_decay=1.0, epsilon_update_freq=100, step_before_train=0)
    buff = RB.ReplayBuffer(0, 12 * n_env, n_env, A, env.obs_dim, N, 4 * N + 8, netmon.get_state_size(),
                           torch.device("cuda", 0))
    wenv.reset_()
    with torch.no_grad():
        for t in range(12):
            buff.add_pre(env.obs, wenv.last_netmon_state, env.node_obs, env.nbr, env.agent_node)
            actions = pol.act_step(wenv)
            buff.add_post(actions, env.reward, env.obs, env.done.bool(), False, env.node_obs, env.agent_node)

    def seq():
        SS.dqn_update_stateless_seq(netmon, model, model_tar, opt, params, buff.get_sequences(bsz, Lq), 0.98, 0.01)

    def per_step():
        batches = list(buff.get_batch(bsz, sequence_length=Lq, lazy_next=True))
        T.dqn_update(netmon, model, model_tar, opt, params, batches, 0.98, 0.01, consecutive=True)
        netmon.state = None

    def timed(fn):
        model.train()
        netmon.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.update_reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.update_reps

    for fn in (seq, per_step):
        timed(fn)
    ms = {"seq": [], "per_step": []}
    for _ in range(a.rounds):
        ms["seq"].append(timed(seq))
        ms["per_step"].append(timed(per_step))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"sequences": bsz, "seq_len": Lq, "envs": n_env, "ms_per_update": {k: round(v, 3) for k, v in med.items()},
            "seq_over_per_step": round(med["seq"] / med["per_step"], 4),
            "spread": {k: spread(v, med[k]) for k, v in ms.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--update-reps", type=int, default=3)
    p.add_argument("--part", default="all", choices=["kernel", "rollout", "update", "all"])
    a = p.parse_args()
    out = {}
    if a.part in ("kernel", "all"):
        out["kernel"] = kernel(a)
        torch.cuda.empty_cache()
    if a.part in ("rollout", "all"):
        out["rollout"] = rollout(a)
        torch.cuda.empty_cache()
    if a.part in ("update", "all"):
        out["update"] = []
        for n_env, bsz, Lq in ((64, 32, 1), (64, 32, 8), (4096, 13108, 8)):
            out["update"].append(update(a, n_env, bsz, Lq))
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
