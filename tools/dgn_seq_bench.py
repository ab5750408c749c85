#!/usr/bin/env python3
"""DGN training without NetMon: the batched update on the HIP attention kernels (dgn_seq.dgn_update_seq) against the
per-step autograd update (train.dqn_update), interleaved in one process.

One full update, sampling included, at the routing observation width (6 N + 10, N = 20 agents' nodes) with the CLI's
default DGN (--hidden-dim 512,256, 8 heads, 2 attention layers, --att-regularization-coeff 0.03), on synthetic replay
contents (random observations, 20 % adjacency + self, 5 % done agents, no episode end), at four shapes (sequence
length, sequences per update):

  l1_small:  (1, 10)       DGN's default sequence length at a small mini-batch
  l1_batch:  (1, 1024)
  l8_paper:  (8, 32)       the reference's --mini-batch-size
  l8_bench:  (8, 13 108)   bench.py's replay ratio at 4096 envs

Rounds alternate A (batched) and B (per-step); each round times `--reps` updates between device synchronisations; the
medians over the rounds and every round's time are reported (the spread of the rounds is the A/B's run-to-run noise).

Prints one JSON line. Usage: python tools/dgn_seq_bench.py [--shape l1_small|l1_batch|l8_paper|l8_bench|all]
                                                            [--rounds 5] [--reps 3] [--att-coeff 0.03]
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
SHAPES = {"l1_small": (1, 64, 10), "l1_batch": (1, 64, 1024), "l8_paper": (8, 64, 32), "l8_bench": (8, 4096, 13108)}


def pair(a, shape):
    M = importlib.import_module("graph-marl_amd.model")
    T = importlib.import_module("graph-marl_amd.train")
    DS = importlib.import_module("graph-marl_amd.dgn_seq")
    RB = importlib.import_module("graph-marl_amd.replaybuffer")
    L_, n_env, bsz = SHAPES[shape]
    N = A = 20
    D = 6 * N + 10
    coeff = a.att_coeff
    torch.manual_seed(0)
    model = M.DGN(D, [512, 256], 4, 8, 2).cuda()
    model_tar = copy.deepcopy(model)
    params = list(model.parameters())
    opt = torch.optim.AdamW(params, lr=1e-4)
    assert DS.dgn_seq_ok(model, model_tar, None, coeff, None, A), "the batched path does not take this model"
    slots = L_ + 4
    buff = RB.ReplayBuffer(0, slots * n_env, n_env, A, D, 0, 0, 0, torch.device("cuda", 0), store_adj=True)
    eye = torch.eye(A, dtype=torch.bool, device="cuda")
    adj = (torch.rand(n_env, A, A, device="cuda") < 0.2) | eye
    for t in range(slots):
        nadj = (torch.rand(n_env, A, A, device="cuda") < 0.2) | eye
        buff.add_pre(torch.randn(n_env, A, D, device="cuda"), adj=adj)
        buff.add_post(torch.randint(0, 4, (n_env, A), device="cuda"), torch.randn(n_env, A, device="cuda"),
                      torch.randn(n_env, A, D, device="cuda"), torch.rand(n_env, A, device="cuda") < 0.05, False,
                      next_adj=nadj)
        adj = nadj

    def batched():
        DS.dgn_update_seq(model, model_tar, opt, params, buff.get_dgn_sequences(bsz, L_), 0.98, 0.01, att_coeff=coeff)

    def per_step():
        batches = list(buff.get_batch(bsz, sequence_length=L_, lazy_next=True))
        T.dqn_update(None, model, model_tar, opt, params, batches, 0.98, 0.01, att_coeff=coeff, consecutive=True)

    def timed(fn):
        model.train()
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
    return {"shape": shape, "sequences": bsz, "seq_len": L_, "agents": A, "att_coeff": coeff,
            "ms_per_update": {k: round(v, 3) for k, v in med.items()},
            "batched_over_per_step": round(med["batched"] / med["per_step"], 4),
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
            "rounds_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--att-coeff", type=float, default=0.03)
    p.add_argument("--shape", default="all", choices=list(SHAPES) + ["all"])
    a = p.parse_args()
    out = []
    for shape in (tuple(SHAPES) if a.shape == "all" else (a.shape,)):
        out.append(pair(a, shape))
        torch.cuda.empty_cache()
    print(json.dumps({"pairs": out}))


if __name__ == "__main__":
    main()
