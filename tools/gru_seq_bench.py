#!/usr/bin/env python3
"""GRU / LN-LSTM NetMon training (--rnn-type gru | lnlstm | lstm): the sequence-batched paths against the per-step
autograd paths, interleaved in one process.

  update:  one DQN + NetMon update at bench.py's training shape (4096 envs, N = 20, H = 128, K = 1,
           13 108 sequences x 8 steps) on train_seq.dqn_update_seq and on train.dqn_update, sampling included.
           Rounds alternate A (sequence-batched) and B (autograd); each round times `--reps` updates between
           device synchronisations; the medians over the rounds are reported.
  config5: src/sl.py's iteration (N = 100, batch 8192, sequence length 8, K = 1) with --netmon-rnn-type <rnn-type> on
           sl_seq and with --sl-autograd, alternating whole sl.main(--bench) runs.

Prints one JSON line. Usage: python tools/gru_seq_bench.py [--rnn-type gru] [--rounds 3] [--reps 3] [--skip-config5]
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


def update_pair(a):
    gm = importlib.import_module("graph-marl_amd")
    M = importlib.import_module("graph-marl_amd.model")
    W = importlib.import_module("graph-marl_amd.wrapper")
    P = importlib.import_module("graph-marl_amd.policy")
    T = importlib.import_module("graph-marl_amd.train")
    TS = importlib.import_module("graph-marl_amd.train_seq")
    RB = importlib.import_module("graph-marl_amd.replaybuffer")
    B, N, L_ = a.n_env, 20, 8
    torch.manual_seed(0)
    net = gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS)
    netmon = M.NetMon(4 * N + 8, 128, [512, 256], 1, rnn_type=a.rnn_type).cuda()
    dqn = M.DQN(6 * N + 10 + netmon.get_out_features(), [512, 256], 4).cuda()
    env = gm.Routing(net, 20, n_env=B, seed=0, obs_extra=netmon.get_out_features(), agent_adjacency=False)
    wenv = W.NetMonWrapper(env, netmon, 1)
    policy = P.EpsilonGreedy(wenv, dqn, epsilon=0.5, epsilon_decay=1.0, epsilon_update_freq=100, step_before_train=0)
    bsz = (32 * B + 9) // 10
    model_tar = copy.deepcopy(dqn)
    params = list(dqn.parameters()) + list(netmon.parameters())
    opt = torch.optim.AdamW(params, lr=1e-4)
    buff = RB.ReplayBuffer(0, (L_ + 8) * B, B, env.n_data, env.obs_dim, env.n_nodes, env.node_obs_dim,
                           netmon.get_state_size(), torch.device("cuda", 0), nbr_width=env.nbr.shape[-1])
    assert TS.seq_ok(netmon, dqn, model_tar), "the sequence-batched path does not take this NetMon"
    wenv.reset()
    for t in range(L_ + 4):  # fill the replay past one sequence (episodes of 300 steps: no episode end inside)
        buff.add_pre(env.obs, wenv.last_netmon_state, env.node_obs, env.nbr, env.agent_node)
        with torch.no_grad():
            act = policy.act_step(wenv)
        buff.add_post(act, env.reward, env.obs, env.done.bool(), False, env.node_obs, env.agent_node)

    def seq():
        TS.dqn_update_seq(netmon, dqn, model_tar, opt, params, buff.get_sequences(bsz, L_), 0.98, 0.01)

    def autograd():
        batches = list(buff.get_batch(bsz, sequence_length=L_, lazy_next=True))
        T.dqn_update(netmon, dqn, model_tar, opt, params, batches, 0.98, 0.01, consecutive=True)

    def timed(fn):
        dqn.train()
        netmon.train()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
            netmon.state = None
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.reps

    for fn in (seq, autograd):  # warm up every shape both paths use
        timed(fn)
    ms = {"seq": [], "autograd": []}
    for _ in range(a.rounds):
        ms["seq"].append(timed(seq))
        ms["autograd"].append(timed(autograd))
    return {"shape": {"n_env": B, "nodes": N, "hidden": 128, "iterations": 1, "sequences": bsz, "seq_len": L_,
                      "rnn_type": a.rnn_type},
            "ms_per_update": {k: round(statistics.median(v), 2) for k, v in ms.items()},
            "rounds_ms": {k: [round(x, 2) for x in v] for k, v in ms.items()}}


def config5_pair(a):
    SL = importlib.import_module("graph-marl_amd.sl")
    base = ["--bench", "--n-nodes", "100", "--batch-size", "8192", "--sequence-length", "8", "--netmon-iterations",
            "1", "--netmon-rnn-type", a.rnn_type, "--iterations", "3", "--warmup", "2"]
    ms = {"seq": [], "autograd": []}
    if a.rnn_type not in SL.SEQ_RNN_TYPES:  # a cell type sl.py keeps on the autograd path: time its unroll anyway
        assert SL.SQ.TS.cell_ok(argparse.Namespace(rnn_type=a.rnn_type, hidden_features=128))
        SL.SEQ_RNN_TYPES += (a.rnn_type,)
    for _ in range(max(1, a.rounds - 1)):
        ms["seq"].append(SL.main(base, quiet=True)["ms_per_iteration"])
        torch.cuda.empty_cache()
        ms["autograd"].append(SL.main(base + ["--sl-autograd"], quiet=True)["ms_per_iteration"])
        torch.cuda.empty_cache()
    return {"ms_per_iteration": {k: round(statistics.median(v), 1) for k, v in ms.items()},
            "rounds_ms": {k: [round(x, 1) for x in v] for k, v in ms.items()}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--n-env", type=int, default=4096)
    p.add_argument("--rnn-type", default="gru", choices=["gru", "lnlstm", "lstm"])
    p.add_argument("--skip-config5", action="store_true")
    a = p.parse_args()
    out = {"update": update_pair(a)}
    torch.cuda.empty_cache()
    if not a.skip_config5:
        out["config5"] = config5_pair(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
