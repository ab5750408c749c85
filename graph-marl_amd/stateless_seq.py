"""Sequence-batched DQN update on a stateless NetMon (--netmon-rnn-type none, src/main.py:840-1026).

Without recurrence the L steps of the B sampled sequences are one batch (as in dgn_seq.py): one encoder pass over
L·B·N node rows, one gm_mp_iterate over L·B graphs (model._MpIterate: forward and backward on the LDS-resident
kernels), the readout, and the online DQN once over all L·B·A agent rows (two-source first layer, _JointLinearFn);
one backward through those nodes. The target DQN runs once over all rows too. Its next-step graph observation is
the online readout of step t + 1 wherever that step continues step t (nothing is carried between steps, so the
NetMon output depends on the step's node observations alone and the reuse is exact; train._reused_next_q proves the
same for the carried cells); the rows of the last step and of episode ends get one separate no-grad NetMon pass on
their stored next observations, all of them in one batch. So an update runs two NetMon passes, not 2 L.

Scope: model DQN, sum / mean, leaky activations, neighbour readout with or without the global mean, every sequence
length >= 1. The aux loss and the other agent models stay on the per-step path (train.dqn_update).
"""
import torch

from . import _lib as L
from . import model as MD


def stateless_seq_ok(netmon, model, model_tar, att_coeff=0.0, aux_model=None):
    """A stateless NetMon with the neighbour readout and a leaky encoder, a leaky DQN with a linear head on both
    sides, no attention regulariser and no aux head."""
    if netmon is None or att_coeff != 0 or aux_model is not None:
        return False
    if type(model) is not MD.DQN or type(model_tar) is not MD.DQN:
        return False
    dq = list(model.encoder.linear_layers)
    return (netmon.rnn_type == "none" and netmon.output_neighbor_hidden and netmon.iterations >= 0
            and all(l.act == 1 for l in netmon.encode.linear_layers) and all(l.act == 1 for l in dq)
            and model.q_net.fc.act == 0)


def _graph_obs(netmon, node_obs, nbr, agent_node):
    """NetMon.forward_graph on stacked graphs; the module's .state is left as it was."""
    keep = netmon.save_state()
    out = netmon.forward_graph(node_obs, nbr, agent_node)
    netmon.restore_state(keep)
    return out


def seq_loss(netmon, model, model_tar, seq, gamma):
    """(loss, q [L, B, A, actions], q_target [L, B, A, actions]) of a train_seq.SeqBatch; loss carries the graph of
    the online pass (loss.backward() fills the gradients of model and netmon)."""
    Lq, B, A, _ = seq.obs.shape
    od = seq.obs_dim
    N, Fd = seq.node_obs.shape[2:]
    R = Lq * B
    nbr = seq.nbr.reshape(R, N, -1)
    graph = _graph_obs(netmon, seq.node_obs.reshape(R, N, Fd), nbr, seq.agent_node.reshape(R, A))  # [R, A, G]
    G = graph.shape[-1]
    q = model.forward_split(seq.obs.reshape(R, A, -1)[..., :od], graph).view(Lq, B, A, -1)
    with torch.no_grad():
        # next observations: step t + 1's, except at the last step and at episode ends (the stored ones)
        obs_l, node_l, an_l = seq.next_fields(Lq - 1, None)
        next_env = torch.cat((seq.obs[1:], obs_l.unsqueeze(0)))
        next_graph = torch.empty(Lq, B, A, G, device=graph.device)
        next_graph[:-1] = graph.detach().view(Lq, B, A, G)[1:]
        xs, nbrs, ans, where = [node_l], [seq.nbr[Lq - 1]], [an_l], [(Lq - 1, None)]
        if Lq > 1:
            ends = seq.episode_done[:-1].nonzero().cpu()  # one host read per update
            for t in ends[:, 0].unique().tolist():
                rows = ends[ends[:, 0] == t, 1].to(graph.device)
                o, x, an = seq.next_fields(t, rows)
                next_env[t, rows] = o
                xs.append(x)
                nbrs.append(seq.nbr[t][rows])
                ans.append(an)
                where.append((t, rows))
        sep = _graph_obs(netmon, torch.cat(xs), torch.cat(nbrs).contiguous(), torch.cat(ans).contiguous())
        at = 0
        for (t, rows), x in zip(where, xs):
            part = sep[at:at + x.shape[0]]
            if rows is None:
                next_graph[t] = part
            else:
                next_graph[t, rows] = part
            at += x.shape[0]
        next_q = model_tar.forward_split(next_env.reshape(R, A, -1)[..., :od], next_graph.view(R, A, G))
        next_max = next_q.view(Lq, B, A, -1).max(dim=3)[0]
        target = seq.reward + (~seq.done) * gamma * next_max
        q_target = torch.scatter(q.detach(), -1, seq.action.unsqueeze(-1), target.unsqueeze(-1))
    # src/main.py:980-1000: the mean of every step's MSE
    loss = (q - q_target).pow(2).reshape(Lq, -1).mean(1).sum() / Lq
    return loss, q, q_target


def dqn_update_stateless_seq(netmon, model, model_tar, optimizer, params, seq, gamma, tau, target_update_steps=0,
                             iteration=1, group=None):
    """One update (src/main.py:840-1026) on a SeqBatch: seq_loss, the gradient all-reduce across ranks, clip by
    value (0.5) and norm (1.0), AdamW, target update."""
    from .train import allreduce_gradients, interpolate_model

    loss, q, qt = seq_loss(netmon, model, model_tar, seq, gamma)
    optimizer.zero_grad(set_to_none=False)
    loss.backward()
    allreduce_gradients(params, group)
    torch.nn.utils.clip_grad_value_(params, 0.5)
    torch.nn.utils.clip_grad_norm_(params, 1.0)
    optimizer.step()
    if target_update_steps <= 0:
        interpolate_model(model, model_tar, tau, model_tar)
    elif iteration % target_update_steps == 0:
        model_tar.load_state_dict(model.state_dict())
    L.check_range()
    return loss.detach(), q, qt
