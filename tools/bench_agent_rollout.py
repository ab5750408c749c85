"""Rollout throughput of DGN, DQNR and CommNet on NetMon graph observations: the fused road (policy.FUSED_AGENTS,
model.forward_fused under rollout.StreamedRollout with 2 stream groups, eager and with per-group graph replay) against
the road before it (FUSED_AGENTS = False: `.obs` materialised every step, a dense first layer, ε-greedy as its own
launch, one stream, envs that write both observation copies), interleaved in one process.

    timeout -k 10 300 python tools/bench_agent_rollout.py --model dgn && \\
    timeout -k 10 300 python tools/bench_agent_rollout.py --model dqnr && \\
    timeout -k 10 300 python tools/bench_agent_rollout.py --model commnet

Shape: 4096 envs, N = 20 routers, A = 20 agents, NetMon H = 128 with K = 1, --hidden-dim 512,256, ε = 0.5, 50-step
episodes. Every leg is warmed up, then timed with HIP events over `--steps` vector steps, `--rounds` times in turn
with the others; the line printed per leg is env-steps/s (median, min, max over the rounds) as JSON.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["dgn", "dqnr", "commnet"], default="dgn")
    ap.add_argument("--n-env", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    args = ap.parse_args()
    gm = importlib.import_module("graph-marl_amd")
    M = importlib.import_module("graph-marl_amd.model")
    P = importlib.import_module("graph-marl_amd.policy")
    RO = importlib.import_module("graph-marl_amd.rollout")
    N = A = 20
    torch.manual_seed(0)
    netmon = M.NetMon(4 * N + 8, 128, [512, 256], 1).cuda()
    D = 6 * N + 10 + netmon.get_out_features()
    model = {"dgn": lambda: M.DGN(D, [512, 256], 4, 8, 2), "dqnr": lambda: M.DQNR(D, [512, 256], 4),
             "commnet": lambda: M.CommNet(D, [512, 256], 4, 2)}[args.model]().cuda()
    net = gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS, device=0)

    def build(groups, lazy):
        RO.LAZY_OBS = lazy
        try:
            return RO.StreamedRollout(net, A, args.n_env, netmon, model, groups=groups, seed=0, epsilon=0.5,
                                      episode_steps=50, device=0)
        finally:
            RO.LAZY_OBS = True

    legs = {"materialised_1stream": (build(1, False), False), "fused_2groups_eager": (build(2, True), True),
            "fused_2groups_graph": (build(2, True), True)}
    for name, (ro, fused) in legs.items():  # warm-up: packed weights, scratch, one episode reset
        P.FUSED_AGENTS = fused
        ro.reset()
        ro.run(60)
        if name.endswith("graph"):
            ro.run(40)  # to an episode boundary: replays start at a multiple of the captured length
            ro.capture(10, per_group=True)
            ro.run(50)
        ro.join()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, (ro, fused) in legs.items():
            P.FUSED_AGENTS = fused
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            ro.run(args.steps)
            ro.join()
            e.record()
            torch.cuda.synchronize()
            times[name].append(args.n_env * args.steps / (s.elapsed_time(e) * 1e-3))
    P.FUSED_AGENTS = True
    res = {"model": args.model, "n_env": args.n_env, "steps": args.steps,
           "env_steps_per_s": {k: {"median": round(statistics.median(v)), "min": round(min(v)), "max": round(max(v))}
                               for k, v in times.items()}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
