#!/usr/bin/env python3
"""DQNR / CommNet training on NetMon graph observations: the batched update
(agent_netmon_seq.agent_netmon_update_seq) against the per-step autograd update (train.dqn_update, what these
configurations ran before), interleaved in one process.

One full update, sampling included, at the reference model sizes (NetMon 128 with encoder 512,256, K = 1; agent
encoder 512,256, CommNet with 2 rounds; A = N = 20) on a replayed rollout of the routing env under a NetMonWrapper
(random actions, random stored agent states, one episode end inside the ring), at sequence length 8 and two batch
sizes (sequences per update):

  l8_paper:  (8, 32)       the reference's --mini-batch-size
  l8_bench:  (8, 13 108)   bench.py's replay ratio at 4096 envs

Rounds alternate A (batched) and B (per-step); each round times `--reps` updates between device synchronisations; the
medians over the rounds and every round's time are reported (the spread of the rounds is the A/B's run-to-run noise).

Prints one JSON line. Usage: python tools/agent_netmon_bench.py [--model dqnr|commnet|all] [--shape l8_paper|l8_bench|all]
                                                                 [--rounds 5] [--reps 3] [--sequences N]
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

# (sequence length, envs in the buffer, sequences per update)
SHAPES = {"l8_paper": (8, 64, 32), "l8_bench": (8, 4096, 13108)}


def pair(a, kind, shape):
    gm = importlib.import_module("graph-marl_amd")
    M = importlib.import_module("graph-marl_amd.model")
    T = importlib.import_module("graph-marl_amd.train")
    W = importlib.import_module("graph-marl_amd.wrapper")
    ANS = importlib.import_module("graph-marl_amd.agent_netmon_seq")
    RB = importlib.import_module("graph-marl_amd.replaybuffer")
    LB = importlib.import_module("graph-marl_amd._lib")
    L_, n_env, bsz = SHAPES[shape]
    bsz = a.sequences or bsz
    N = A = 20
    H = 128
    comm = kind == "commnet"
    env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A, n_env=n_env, seed=0,
                     obs_extra=4 * H, agent_adjacency=comm)
    torch.manual_seed(0)
    netmon = M.NetMon(4 * N + 8, H, [512, 256], 1).cuda()
    D = env.obs_dim + 4 * H
    model = (M.CommNet(D, [512, 256], 4, 2) if comm else M.DQNR(D, [512, 256], 4)).cuda()
    model_tar = copy.deepcopy(model)
    params = list(model.parameters()) + list(netmon.parameters())
    opt = torch.optim.AdamW(params, lr=1e-4)
    assert ANS.agent_netmon_seq_ok(netmon, model, model_tar, 0.0, None, A), "the batched path does not take this"
    wenv = W.NetMonWrapper(env, netmon, 1)
    slots = L_ + 4
    SL = model.get_state_len()
    buff = RB.ReplayBuffer(0, slots * n_env, n_env, A, env.obs_dim, N, 4 * N + 8, netmon.get_state_size(),
                           torch.device("cuda", 0), agent_state_size=SL, store_adj=comm)
    wenv.reset_()
    for t in range(slots):
        buff.add_pre(env.obs, wenv.last_netmon_state, env.node_obs, env.nbr, env.agent_node,
                     adj=env.agent_adj if comm else None,
                     agent_state=0.5 * torch.tanh(torch.randn(n_env, A, SL, device="cuda")))
        act = torch.randint(0, 4, (n_env, A), dtype=torch.int32, device="cuda")
        wenv.step_(act)
        end = t == slots // 2
        buff.add_post(act, env.reward, env.obs, env.done.bool(), end, env.node_obs, env.agent_node,
                      next_adj=env.agent_adj if comm else None)
        if end:
            wenv.reset_()
    netmon.state = None

    def batched():
        ANS.agent_netmon_update_seq(netmon, model, model_tar, opt, params, buff.get_agent_netmon_sequences(bsz, L_),
                                    0.98, 0.01)
        netmon.state = None

    def per_step():
        batches = list(buff.get_batch(bsz, sequence_length=L_, lazy_next=True))
        T.dqn_update(netmon, model, model_tar, opt, params, batches, 0.98, 0.01, consecutive=True)
        netmon.state = None
        model.state = None

    def timed(fn):
        model.train()
        netmon.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.reps

    for fn in (batched, per_step):  # warm up every shape both paths use
        timed(fn)
    ms = {"batched": [], "per_step": []}
    for _ in range(a.rounds):
        ms["batched"].append(timed(batched))
        ms["per_step"].append(timed(per_step))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"model": kind, "shape": shape, "sequences": bsz, "seq_len": L_, "agents": A,
            "src": LB.build_info().get("src"),
            "ms_per_update": {k: round(v, 3) for k, v in med.items()},
            "per_step_over_batched": round(med["per_step"] / med["batched"], 3),
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
            "rounds_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--sequences", type=int, default=0, help="override the shape's sequences per update")
    p.add_argument("--model", default="all", choices=["dqnr", "commnet", "all"])
    p.add_argument("--shape", default="all", choices=list(SHAPES) + ["all"])
    a = p.parse_args()
    out = []
    for kind in (("dqnr", "commnet") if a.model == "all" else (a.model,)):
        for shape in (tuple(SHAPES) if a.shape == "all" else (a.shape,)):
            out.append(pair(a, kind, shape))
            print(json.dumps(out[-1]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    print(json.dumps({"pairs": out}))


if __name__ == "__main__":
    main()
