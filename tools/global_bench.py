#!/usr/bin/env python3
"""--netmon-global (NetMon output_global_hidden): the fused rollout against the unfused one, and the
sequence-batched update (train_seq.dqn_update_seq) against the per-step autograd update (train.dqn_update),
interleaved in one process.

Rollout: 4096 routing envs, N = 20 nodes and agents, NetMon H = 128, encoder 512,256, K = 1, DQN 512,256;
NetMonWrapper(fused=True) (state tables + gm_netmon_global_rows, ε-greedy in the env step kernel) against
NetMonWrapper(fused=False) (NetMon.forward_graph and a materialised joint observation after every env step), each
on its own envs; env-steps/s over `--steps` vector steps between device synchronisations.

Update: one full update, sampling included, sequence length 8, on a replayed fused rollout (12 vector steps), at

  paper:  32 sequences (the reference's --mini-batch-size), 64 envs in the buffer
  bench:  13 108 sequences (bench.py's replay ratio at 4096 envs), 4096 envs in the buffer

Rounds alternate A and B; the medians over the rounds and every round's value are reported (the spread of the rounds
is the A/B's run-to-run noise).

Prints one JSON line. Usage: python tools/global_bench.py [--part rollout|update|both] [--shape paper|bench|both]
                                                          [--rounds 5] [--reps 3] [--steps 50]
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

SHAPES = {"paper": (64, 32), "bench": (4096, 13108)}  # (envs in the buffer, sequences per update)
N = A = 20
H, L_ = 128, 8


def mods():
    names = ("", ".model", ".wrapper", ".policy", ".train", ".train_seq", ".replaybuffer")
    return tuple(importlib.import_module("graph-marl_amd" + n) for n in names)


def models(M):
    torch.manual_seed(0)
    netmon = M.NetMon(4 * N + 8, H, [512, 256], 1, output_global_hidden=True).cuda()
    model = M.DQN(6 * N + 10 + 5 * H, [512, 256], 4).cuda()
    return netmon, model


def wrapped(gm, W, P, netmon, model, n_env, fused, seed=0):
    env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A, n_env=n_env, seed=seed,
                     obs_extra=5 * H, agent_adjacency=False)
    wenv = W.NetMonWrapper(env, netmon, 1, fused=fused)
    pol = P.EpsilonGreedy(wenv, model, epsilon=0.5, epsilon_decay=1.0, epsilon_update_freq=100, step_before_train=0)
    return env, wenv, pol


def spread(v, med):
    return round((max(v) - min(v)) / med, 4)


def rollout(a):
    gm, M, W, P, T, S, RB = mods()
    n_env = 4096
    netmon, model = models(M)
    runs = {}
    for name, fused in (("fused", True), ("unfused", False)):
        # each wrapper steps its own copy of NetMon: the module carries the state of the wrapper that ran last
        env, wenv, pol = wrapped(gm, W, P, copy.deepcopy(netmon), model, n_env, fused)
        assert wenv.fused == fused
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
    return {"envs": n_env, "nodes": N, "hidden": H, "iterations": 1, "steps_per_round": a.steps,
            "env_steps_per_s": {k: round(v) for k, v in med.items()},
            "fused_over_unfused": round(med["fused"] / med["unfused"], 4),
            "spread": {k: spread(v, med[k]) for k, v in sps.items()},
            "rounds": {k: [round(x) for x in v] for k, v in sps.items()}}


def update(a, shape):
    gm, M, W, P, T, S, RB = mods()
    n_env, bsz = SHAPES[shape]
    netmon, model = models(M)
    model_tar = copy.deepcopy(model)
    params = list(model.parameters()) + list(netmon.parameters())
    opt = torch.optim.AdamW(params, lr=1e-4)
    assert S.seq_ok(netmon, model, model_tar), "the sequence-batched path does not take this configuration"
    env, wenv, pol = wrapped(gm, W, P, netmon, model, n_env, True)
    buff = RB.ReplayBuffer(0, (L_ + 4) * n_env, n_env, A, env.obs_dim, N, 4 * N + 8, netmon.get_state_size(),
                           torch.device("cuda", 0))
    wenv.reset_()
    with torch.no_grad():
        for t in range(L_ + 4):
            buff.add_pre(env.obs, wenv.last_netmon_state, env.node_obs, env.nbr, env.agent_node)
            actions = pol.act_step(wenv)
            buff.add_post(actions, env.reward, env.obs, env.done.bool(), False, env.node_obs, env.agent_node)

    def seq():
        S.dqn_update_seq(netmon, model, model_tar, opt, params, buff.get_sequences(bsz, L_), 0.98, 0.01)

    def per_step():
        batches = list(buff.get_batch(bsz, sequence_length=L_, lazy_next=True))
        T.dqn_update(netmon, model, model_tar, opt, params, batches, 0.98, 0.01, consecutive=True)
        netmon.state = None

    def timed(fn):
        model.train()
        netmon.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.reps

    for fn in (seq, per_step):  # warm up every shape both paths use
        timed(fn)
    ms = {"seq": [], "per_step": []}
    for _ in range(a.rounds):
        ms["seq"].append(timed(seq))
        ms["per_step"].append(timed(per_step))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"shape": shape, "sequences": bsz, "seq_len": L_, "agents": A, "hidden": H,
            "ms_per_update": {k: round(v, 3) for k, v in med.items()},
            "seq_over_per_step": round(med["seq"] / med["per_step"], 4),
            "spread": {k: spread(v, med[k]) for k, v in ms.items()},
            "rounds_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--part", default="both", choices=["rollout", "update", "both"])
    p.add_argument("--shape", default="both", choices=["paper", "bench", "both"])
    a = p.parse_args()
    out = {}
    if a.part in ("rollout", "both"):
        out["rollout"] = rollout(a)
        torch.cuda.empty_cache()
    if a.part in ("update", "both"):
        out["update"] = []
        for shape in (("paper", "bench") if a.shape == "both" else (a.shape,)):
            out["update"].append(update(a, shape))
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
