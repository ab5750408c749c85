"""Sequence-batched DQN update for the agent models with a carried state, DQNR and CommNet, on NetMon graph
observations (reference src/main.py:840-1026 with --netmon and --model dqnr / commnet; src/model.py:451-631, 653-794),
with a hand-written backward: one autograd node (`_AgentNetMonFn`) that joins the NetMon half of train_seq.py and the
agent half of agent_seq.py at the readout buffer, as dgn_netmon_seq.py does for DGN.

  * forward: train_seq._forward_netmon (the encoder once over L*B*N rows, the cells and the aggregate per step, the
    state masked at episode ends, src/main.py:857-859, the readout into [L*B*A, 4H], 5H with the global mean), then
    agent_seq._forward with the encoder's first layer reading its two sources [readout rows | env obs] on the weight
    packed as train_seq._dqn_first_x3 packs the DQN's first layer; from the second layer on nothing differs (the
    per-step LSTM cells with the state killed by done | episode_done, CommNet's gm_agent_comm rounds, the Q head
    over all steps);
  * the target model runs once, no-grad, over all L steps' rows of [next graph obs | next env obs] (with next_adj),
    every step starting from the online model's state after that step, before the kill mask (src/main.py:899-902,
    920-926; agent_seq._target_max). NetMon has no target copy: the next graph rows are
    dgn_netmon_seq._next_graph_rows (the online readout of step t + 1, or a NetMon step of their own where episode
    t ended and at the last step);
  * backward: agent_seq._backward down to the encoder's first layer; that layer's weight gradient from its two
    sources in one launch, mapped back to the reference column order [env obs | graph obs], its input gradient over
    the readout columns only; then train_seq._backward_netmon (gm_netmon_readout_bwd, gm_netmon_global_bwd with the
    global mean, the cells' backward per step in reverse with the episode_done mask on the state gradient, the
    batched encoder backward).

Every GEMM runs in the split-f16 form with fp32 accumulation. train.dqn_loss remains the path for the aux loss,
--netmon-rnn-carryover 0, other activations, GM_GEMM=f32, more than 64 agents and sequence length 1.
"""
from collections import namedtuple

import torch

from . import _lib as L
from . import agent_seq as AS
from . import dgn_netmon_seq as DNS
from . import fused as FU
from . import train_seq as TS

AgentNetMonSeqBatch = namedtuple("AgentNetMonSeqBatch", ["obs", "obs_dim", "action", "reward", "done", "episode_done",
                                                         "node_obs", "nbr", "agent_node", "node_state", "next_fields",
                                                         "adj", "next_obs", "next_adj", "agent_state", "idx"],
                                 defaults=(None,))
"""dgn_netmon_seq.DGNNetMonSeqBatch's fields (adj, next_adj [L, B, A, A] int8: None for DQNR, which does not
communicate) plus agent_state [B, A, 2H], the agent state before step 0 ([h | c]), as agent_seq.AgentSeqBatch."""


def agent_netmon_seq_ok(netmon, model, model_tar, att_coeff=0.0, aux_model=None, n_agents=None):
    """The NetMon conditions of train_seq.netmon_seq_ok and the agent conditions of agent_seq.agent_seq_ok together:
    lstm / gru / lnlstm NetMon cells with carry-over, neighbour readout (with or without the global mean), K >= 1,
    H % 32 == 0; DQNR or CommNet with leaky layers and biases, a head of at most 4 actions, a hidden size
    gm_lstm_cell_bwd takes, at most 64 agents; split-f16 GEMMs, no aux loss."""
    if netmon is None or aux_model is not None or L.GEMM_MODE != "x3":
        return False
    return TS.netmon_seq_ok(netmon) and AS.agent_seq_ok(model, model_tar, None, att_coeff, None, n_agents)


def _plans(netmon, model, seq, params):
    pn, pa = TS._Plan(), TS._Plan()
    pn.netmon, pn.seq = netmon, seq
    pa.model, pa.seq, pa.params = model, seq, list(params)
    return pn, pa


@torch.no_grad()
def _target(pn, pa, model_tar):
    """max_a Q_target [L, B, A]: agent_seq._target_max with the target encoder on [next graph obs | next env obs]."""
    Ls, B, A, N, F, od, odp, H, K, M, Ma = pn.dims
    LM = Ls * Ma
    Rn = DNS._next_graph_rows(pn)
    env = pn.seq.next_obs.reshape(LM, odp)

    def encode(encoder, rows, scratch):
        h = ld = kk = None
        for i, lin in enumerate(encoder.linear_layers):
            dst = scratch(("mlp", id(encoder), i), rows, lin.out_features)
            if i == 0:
                DNS.target_first(pn, lin, Rn, env, dst)
            else:
                FU.linear_rows(lin, h, ld, rows, dst, dst.stride(0), k=kk)
            h, ld, kk = dst, dst.stride(0), lin.out_features
        return h

    return AS._target_max(pa, model_tar, encode=encode)


def _forward(pn, pa, model_tar):
    """q [L*B*A, nq]; pa.next_max = the target pass's max_a Q [L, B, A]."""
    TS._forward_netmon(pn)
    q = AS._forward(pa, first=DNS.first_forward(pn))
    pa.next_max = _target(pn, pa, model_tar)
    return q


def _backward(pn, pa, dq):
    hold = {}
    grads = AS._backward(pa, dq, first=DNS.first_backward(pn, hold))
    TS._backward_netmon(pn, hold["dR"], grads)
    return grads


class _AgentNetMonFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pn, pa, model_tar, *params):
        ctx.plans = (pn, pa)
        with torch.no_grad():
            return _forward(pn, pa, model_tar)

    @staticmethod
    def backward(ctx, dq):
        pn, pa = ctx.plans
        grads = _backward(pn, pa, dq)
        ctx.plans = None
        return (None, None, None) + tuple(grads.get(w) for w in pa.params)


def agent_netmon_seq_loss(netmon, model, model_tar, seq, gamma, params, parts=None):
    """TD loss of src/main.py:840-1000 over an AgentNetMonSeqBatch: (loss, q [L, B, A, nq], q_target)."""
    Ls, B, A = seq.action.shape
    if A > AS.MAX_AGENTS:
        raise ValueError(f"agent_netmon_seq_loss: at most {AS.MAX_AGENTS} agents")
    pn, pa = _plans(netmon, model, seq, params)
    q = _AgentNetMonFn.apply(pn, pa, model_tar, *pa.params).view(Ls, B, A, -1)
    target = seq.reward + (~seq.done) * gamma * pa.next_max
    q_target = torch.scatter(q.detach(), -1, seq.action.unsqueeze(-1), target.unsqueeze(-1))
    loss = (q - q_target).pow(2).mean(dim=(1, 2, 3)).sum() / Ls
    if parts is not None:
        parts.update(loss_q=loss, loss_att=None, loss_aux=None)
    return loss, q, q_target


def agent_netmon_update_seq(netmon, model, model_tar, optimizer, params, seq, gamma, tau, target_update_steps=0,
                            iteration=1, group=None, parts=None):
    """One update (src/main.py:840-1026) on an AgentNetMonSeqBatch: the batched loss and backward, the gradient
    all-reduce across ranks, clip by value (0.5) and norm (1.0), AdamW, target update."""
    from .train import allreduce_gradients, interpolate_model

    loss, q, qt = agent_netmon_seq_loss(netmon, model, model_tar, seq, gamma, params, parts)
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
