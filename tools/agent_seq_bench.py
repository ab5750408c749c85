#!/usr/bin/env python3
"""DQNR / CommNet training without NetMon: the sequence-batched update (agent_seq.agent_update_seq) against the
per-step autograd update (train.dqn_update), interleaved in one process.

One full update, sampling included, at the routing observation width (6 N + 10, N = 20 agents' nodes) with
--hidden-dim 512,256 (H = 256) and sequence length 8, on synthetic replay contents (random observations, 20 %
adjacency, 5 % done agents, no episode end inside a sequence), at two shapes:

  paper:  32 sequences (the reference's --mini-batch-size) x 8 steps x 20 agents
  bench:  13 108 sequences x 8 steps x 20 agents (bench.py's replay ratio at 4096 envs)

Rounds alternate A (sequence-batched) and B (per-step); each round times `--reps` updates between device
synchronisations; the medians over the rounds and every round's time are reported (the spread of the rounds is the
A/B's run-to-run noise).

Prints one JSON line. Usage: python tools/agent_seq_bench.py [--model dqnr|commnet|both] [--shape paper|bench|both]
                                                              [--rounds 5] [--reps 3]
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


def pair(a, name, shape):
    M = importlib.import_module("graph-marl_amd.model")
    T = importlib.import_module("graph-marl_amd.train")
    AS = importlib.import_module("graph-marl_amd.agent_seq")
    RB = importlib.import_module("graph-marl_amd.replaybuffer")
    n_env, bsz = SHAPES[shape]
    N = A = 20
    D, L_ = 6 * N + 10, 8
    torch.manual_seed(0)
    model = (M.DQNR(D, [512, 256], 4) if name == "dqnr" else M.CommNet(D, [512, 256], 4, 2)).cuda()
    model_tar = copy.deepcopy(model)
    params = list(model.parameters())
    opt = torch.optim.AdamW(params, lr=1e-4)
    assert AS.agent_seq_ok(model, model_tar, None, 0.0, None, A), "the sequence-batched path does not take this model"
    S = model.get_state_len()
    buff = RB.ReplayBuffer(0, (L_ + 4) * n_env, n_env, A, D, 0, 0, 0, torch.device("cuda", 0), agent_state_size=S,
                           store_adj=True)
    adj = torch.rand(n_env, A, A, device="cuda") < 0.2
    for t in range(L_ + 4):
        nadj = torch.rand(n_env, A, A, device="cuda") < 0.2
        buff.add_pre(torch.randn(n_env, A, D, device="cuda"), adj=adj,
                     agent_state=torch.tanh(torch.randn(n_env, A, S, device="cuda")))
        buff.add_post(torch.randint(0, 4, (n_env, A), device="cuda"), torch.randn(n_env, A, device="cuda"),
                      torch.randn(n_env, A, D, device="cuda"), torch.rand(n_env, A, device="cuda") < 0.05, False,
                      next_adj=nadj)
        adj = nadj

    def seq():
        AS.agent_update_seq(model, model_tar, opt, params, buff.get_agent_sequences(bsz, L_), 0.98, 0.01)

    def per_step():
        batches = list(buff.get_batch(bsz, sequence_length=L_, lazy_next=True))
        T.dqn_update(None, model, model_tar, opt, params, batches, 0.98, 0.01, consecutive=True)
        model.state = None

    def timed(fn):
        model.train()
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
    return {"model": name, "shape": shape, "sequences": bsz, "seq_len": L_, "agents": A, "hidden": 256,
            "ms_per_update": {k: round(v, 3) for k, v in med.items()},
            "seq_over_per_step": round(med["seq"] / med["per_step"], 4),
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
            "rounds_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--model", default="both", choices=["dqnr", "commnet", "both"])
    p.add_argument("--shape", default="both", choices=["paper", "bench", "both"])
    a = p.parse_args()
    out = []
    for name in (("dqnr", "commnet") if a.model == "both" else (a.model,)):
        for shape in (("paper", "bench") if a.shape == "both" else (a.shape,)):
            out.append(pair(a, name, shape))
            torch.cuda.empty_cache()
    print(json.dumps({"pairs": out}))


if __name__ == "__main__":
    main()
