#!/usr/bin/env python3
"""Golden vectors of the stateless NetMon (--netmon-rnn-type none, src/model.py:394-396, 553-554, 574-576), recorded
from the *reference* implementation like make_golden.py's (whose helpers this script imports; it runs only where the
reference is present, on the CPU):

  netmon_stateless.npz          NetMon(rnn_type="none") at N = 20, B = 4, 3 steps, H = 32, encoder 64,48, for
                                (sum, K=0), (sum, K=1), (mean, K=3), (mean, K=8), (sum, K=8, global mean): per step the
                                node output h, the readout mapped to the agents and .state
  train_stateless.npz           gen_train(rnn_type="none", agg="mean", K=3, B=3, L=3)
  train_stateless_l1.npz        gen_train(rnn_type="none", agg="sum", K=8, B=3, L=1): the reference run script's form
  ref_checkpoint_stateless.pt   a checkpoint written by the reference's get_state_dict for a stateless NetMon + DQN,
  ref_checkpoint_stateless.npz  and the reference models' Q-values on 3 steps of 2 graphs

Usage:  python tests/golden/make_golden_stateless.py [--ref /root/reference/src]
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import collect_graph_inputs, gen_train, sd_to_npz, write_stubs  # noqa: E402

VARIANTS = [("sum", 0, False), ("sum", 1, False), ("mean", 3, False), ("mean", 8, False), ("sum", 8, True)]
H, ENC = 32, (64, 48)


def gen_netmon_stateless(out, Network, Routing, EVAL_SEEDS, NetMon):
    import torch
    import torch.nn.functional as F

    d = {}
    n, a, B, steps = 20, 20, 4, 3
    node_obs, node_adj, node_agent, _ = collect_graph_inputs(Network, Routing, EVAL_SEEDS, n, a, B, steps, 500)
    d["node_obs"], d["node_adj"], d["node_agent"] = node_obs, node_adj.astype(np.int8), node_agent.astype(np.int8)
    d["variants"] = np.array([f"none|{g}|{k}|{H}|{ENC[0]},{ENC[1]}|{int(gl)}" for g, k, gl in VARIANTS])
    for vi, (agg, K, glob) in enumerate(VARIANTS):
        torch.manual_seed(70 + vi)
        nm = NetMon(node_obs.shape[-1], H, list(ENC), K, F.leaky_relu, rnn_type="none", rnn_carryover=True,
                    agg_type=agg, output_neighbor_hidden=True, output_global_hidden=glob)
        nm.eval()
        sd_to_npz(f"v{vi}_w_", nm.state_dict(), d)
        d[f"v{vi}_keys"] = np.array(list(nm.state_dict().keys()))
        d[f"v{vi}_out_features"] = np.int64(nm.get_out_features())
        d[f"v{vi}_state_size"] = np.int64(nm.get_state_size())
        nm.state = None
        with torch.no_grad():
            for t in range(steps):
                x, m, na = torch.tensor(node_obs[t]), torch.tensor(node_adj[t]), torch.tensor(node_agent[t])
                h = nm(x, m, na, no_agent_mapping=True)
                d[f"v{vi}_h_{t}"] = h.numpy()
                d[f"v{vi}_mapped_{t}"] = NetMon.output_to_network_obs(h, na).numpy()
                d[f"v{vi}_state_{t}"] = nm.state.numpy()
    np.savez_compressed(out, **d)
    print("netmon_stateless done", flush=True)


def gen_checkpoint_stateless(out_pt, out_npz, ref, Network, Routing, EVAL_SEEDS, NetMon, DQN, get_state_dict):
    """make_golden.gen_checkpoint with --netmon-rnn-type=none: the reference's own parser, get_state_dict and
    torch.save (src/main.py:40-381, 812-817, src/util.py:26-35)."""
    import torch
    import torch.nn.functional as F

    tb = types.ModuleType("torch.utils.tensorboard")
    tbw = types.ModuleType("torch.utils.tensorboard.writer")
    tbw.SummaryWriter = type("SummaryWriter", (), {})
    tb.writer = tbw
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    sys.modules.setdefault("torch.utils.tensorboard.writer", tbw)
    src = open(os.path.join(ref, "main.py")).read()
    ns = {"__name__": "reference_main_parser"}
    exec(compile(src[: src.index("args = parser.parse_args()")], "main.py", "exec"), ns)
    args = ns["parser"].parse_args(["--env-type=routing", "--model=dqn", "--netmon", "--netmon-dim=16",
                                    "--netmon-encoder-dim=32,16", "--netmon-iterations=3", "--netmon-rnn-type=none",
                                    "--netmon-agg-type=mean", "--hidden-dim=32,24", "--seed=3"])
    n, a, B, steps = 20, 20, 2, 3
    node_obs, node_adj, node_agent, agent_obs = collect_graph_inputs(Network, Routing, EVAL_SEEDS, n, a, B, steps, 300)
    torch.manual_seed(22)
    act = getattr(F, args.activation_function)
    netmon = NetMon(node_obs.shape[-1], args.netmon_dim, [int(x) for x in args.netmon_encoder_dim.split(",")],
                    args.netmon_iterations, activation_fn=act, rnn_type=args.netmon_rnn_type,
                    rnn_carryover=args.netmon_rnn_carryover, agg_type=args.netmon_agg_type,
                    output_neighbor_hidden=True, output_global_hidden=args.netmon_global)
    model = DQN(agent_obs.shape[-1] + netmon.get_out_features(), [int(x) for x in args.hidden_dim.split(",")], 4, act)
    torch.save(get_state_dict(model, netmon, args.__dict__), out_pt)
    d = {"node_obs": node_obs, "node_adj": node_adj, "node_agent": node_agent, "agent_obs": agent_obs}
    netmon.eval()
    model.eval()
    netmon.state = None
    with torch.no_grad():
        for t in range(steps):
            h = netmon(torch.tensor(node_obs[t]), torch.tensor(node_adj[t]), torch.tensor(node_agent[t]))
            d[f"q_{t}"] = model(torch.cat([torch.tensor(agent_obs[t]), h], -1), None).numpy()
    np.savez_compressed(out_npz, **d)
    print("checkpoint:", out_pt, out_npz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference/src")
    args = ap.parse_args()
    stub_dir = tempfile.mkdtemp(prefix="gm_ref_stubs_")
    write_stubs(stub_dir)
    sys.path[:0] = [stub_dir, args.ref]

    from env.constants import EVAL_SEEDS  # noqa: E402
    from env.network import Network  # noqa: E402
    from env.routing import Routing  # noqa: E402
    from model import DQN, NetMon  # noqa: E402
    from util import get_state_dict, interpolate_model  # noqa: E402

    gen_netmon_stateless(os.path.join(HERE, "netmon_stateless.npz"), Network, Routing, EVAL_SEEDS, NetMon)
    gen_train(os.path.join(HERE, "train_stateless.npz"), Network, Routing, EVAL_SEEDS, NetMon, DQN, interpolate_model,
              rnn_type="none", agg="mean", K=3, B=3, L=3)
    gen_train(os.path.join(HERE, "train_stateless_l1.npz"), Network, Routing, EVAL_SEEDS, NetMon, DQN,
              interpolate_model, rnn_type="none", agg="sum", K=8, B=3, L=1)
    gen_checkpoint_stateless(os.path.join(HERE, "ref_checkpoint_stateless.pt"),
                             os.path.join(HERE, "ref_checkpoint_stateless.npz"), args.ref, Network, Routing,
                             EVAL_SEEDS, NetMon, DQN, get_state_dict)


if __name__ == "__main__":
    main()
