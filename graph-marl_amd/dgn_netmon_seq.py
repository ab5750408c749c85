"""Sequence-batched DQN update for DGN on NetMon graph observations (reference src/main.py:840-1026 with --netmon and
--model dgn; src/model.py:45-176, 451-631), with a hand-written backward: one autograd node (`_DGNNetMonFn`) that
joins the NetMon half of train_seq.py and the DGN half of dgn_seq.py at the readout buffer.

  * forward: train_seq._forward_netmon (the encoder once over L*B*N rows, the cells and the aggregate per step, the
    state masked at episode ends, gm_netmon_readout_ld into [L*B*A, 4H], 5H with the global mean), then
    dgn_seq._forward with the encoder's first layer reading its two sources [readout rows | env obs] on the weight
    packed as train_seq._dqn_first_x3 packs the DQN's first layer; from the second layer on nothing differs
    (attention layers, head, the regulariser's KL rows);
  * the target model runs once, no-grad, over all L steps' rows of [next graph obs | next env obs] with next_adj.
    NetMon has no target copy (src/main.py:909-915): the next graph observation of step t is the online readout of
    step t + 1, except where episode t ended and at the last step, which get a NetMon step of their own from the
    online state after step t (fused.netmon_step on the stored next node observations, as train_seq._target_max).
    The target's per-layer qkv rows feed gm_agent_attention_kl and the regulariser term of gm_agent_attention_bwd;
  * backward: dgn_seq._backward down to the encoder's first layer; that layer's weight gradient from its two sources
    in one launch, mapped back to the reference column order, its input gradient over the readout columns only;
    then train_seq._backward_netmon (gm_netmon_readout_bwd, gm_netmon_global_bwd with the global mean, the cells'
    backward per step in reverse, the batched encoder backward).

Every GEMM runs in the split-f16 form with fp32 accumulation. train.dqn_loss remains the path for the aux loss,
--netmon-rnn-carryover 0, other activations, GM_GEMM=f32 and more than 64 agents.
"""
from collections import namedtuple

import torch

from . import _lib as L
from . import dgn_seq as DS
from . import fused as FU
from . import model as MD
from . import train_seq as TS

DGNNetMonSeqBatch = namedtuple("DGNNetMonSeqBatch", ["obs", "obs_dim", "action", "reward", "done", "episode_done",
                                                     "node_obs", "nbr", "agent_node", "node_state", "next_fields",
                                                     "adj", "next_obs", "next_adj", "idx"], defaults=(None,))
"""train_seq.SeqBatch's fields (next_fields(t, rows) included: the target's own NetMon steps read the stored next
node observations on demand), plus adj, next_adj [L, B, A, A] int8 and the stored next env observations next_obs
[L, B, A, odp] in full (the target model reads them at every step), as dgn_seq.DGNSeqBatch."""


def dgn_netmon_seq_ok(netmon, model, model_tar, att_coeff=0.0, aux_model=None, n_agents=None):
    """The NetMon conditions of train_seq.seq_ok and the DGN conditions of dgn_seq.dgn_seq_ok together: lstm / gru /
    lnlstm cells with carry-over, neighbour readout (with or without the global mean), K >= 1, H % 32 == 0, leaky
    layers with biases everywhere, at most 64 agents within the attention kernels' LDS bound, split-f16 GEMMs, no
    aux loss."""
    if netmon is None or aux_model is not None or L.GEMM_MODE != "x3":
        return False
    return TS.netmon_seq_ok(netmon) and DS.dgn_seq_ok(model, model_tar, None, att_coeff, None, n_agents)


def _next_graph_rows(pn):
    """The target's graph observations [L*B*A, GW], detached: the online readout of step t + 1 for step t, and a
    NetMon step of their own (from the online state after step t, on the stored next node observations) for the
    sequences whose episode ended at t and for the last step."""
    Ls, B, A, N, F, od, odp, H, K, M, Ma = pn.dims
    sb, netmon, GW = pn.seq, pn.netmon, pn.GW
    S2 = netmon.state_size
    dev = pn.R.device
    Rn = torch.empty(Ls, B, A, GW, device=dev)
    lib = L.lib()

    def own(t, r):
        _, nno, nan_ = sb.next_fields(t, r)
        st = pn.S[K, t].view(B, N, S2)
        nb = sb.nbr[t]
        if r is not None:
            st, nb = st[r], nb[r]
        nb = nb.contiguous()
        n = nno.shape[0]
        keep = netmon.save_state()
        st2, hp = FU.netmon_step(netmon, nno, nb, st.detach().contiguous())
        netmon.restore_state(keep)
        rows = torch.empty(n * A, GW, device=dev)
        L.check(lib.gm_netmon_readout_ld(st2.data_ptr(), S2, hp.data_ptr(), hp.stride(0), nb.data_ptr(),
                                         nan_.data_ptr(), n, N, A, nb.shape[-1], H, rows.data_ptr(), GW,
                                         L.stream_ptr()))
        if pn.glob:
            FU.global_rows(st2.data_ptr(), S2, n, N, H, A, rows.data_ptr() + 16 * H, GW)
        return rows.view(n, A, GW)

    if Ls > 1:
        Rn[:-1].copy_(pn.R.view(Ls, B, A, GW)[1:])
        done_rows = sb.episode_done[:-1].nonzero().cpu()  # one host read per update
        for t in torch.unique(done_rows[:, 0]).tolist():
            r = done_rows[done_rows[:, 0] == t, 1].to(dev)
            Rn[t, r] = own(t, r)
    Rn[-1].copy_(own(Ls - 1, None))
    return Rn.view(Ls * Ma, GW)


def target_first(pn, lin, Rn, env, dst):
    """The target model's first encoder layer on its two dense sources [next graph rows Rn | next env obs rows env]
    into the rows dst (no-grad; the weight packed as fused.pack_dqn_first packs it for dense graph rows)."""
    Ls, B, A, N, F, od, odp, H, K, M, Ma = pn.dims
    LM, GW, n = Ls * Ma, pn.GW, lin.out_features
    wp, ldw, b, x3 = FU.pack_dqn_first(lin, od, global_h=H if pn.glob else None, order="global_env")
    FU.gemm(FU.dense(Rn.data_ptr(), GW, GW), FU.dense(env.data_ptr(), odp, od), wp.data_ptr(), ldw,
            b.data_ptr(), LM, n, FU._epi(lin.act), dst.data_ptr(), dst.stride(0),
            tag=lin.tag and f"linear:{lin.tag}:{LM}x{n}x{GW}+{od}", x3=x3)


def first_forward(pn):
    """The `first` hook of dgn_seq._forward / agent_seq._forward on NetMon graph observations: the online encoder's
    first layer on its two sources [readout rows pn.R | env obs rows pn.env]."""
    Ls, B, A, N, F, od, odp, H, K, M, Ma = pn.dims
    R, GW, glob = pn.R, pn.GW, pn.glob

    def first(lin, y, ldy, yb):
        sx = TS._zeros1(R.device)
        TS._gemm_amax(R, GW, GW, TS._dqn_first_x3(lin, od, H if glob else None), lin.bias, Ls * Ma, lin.out_features,
                      FU.GM_EPI_BIAS_LEAKY, y, ldy, sx, a1=(pn.env, odp, od), sbits=yb)
        return sx

    return first


def first_backward(pn, hold):
    """The `first` hook of dgn_seq._backward / agent_seq._backward: the first layer's weight gradient from its two
    sources in one launch, mapped back to the reference column order, and hold["dR"] = its input gradient over the
    readout columns, for train_seq._backward_netmon."""
    Ls, B, A, N, F, od, odp, H, K, M, Ma = pn.dims
    GW, glob = pn.GW, pn.glob
    LMa = Ls * Ma

    def first(lin, g, sc, s_in, grads):
        w_r, w_env = MD._wgrad_pair(g, pn.R, GW, pn.env, od, sc, s_in, s_in)  # one launch
        # the reference's column order: [env | h | nbr x 3], with the global readout [env | h | global | nbr x 3]
        grads[lin.weight] = (torch.cat([w_env, w_r[:, :H], w_r[:, 4 * H:], w_r[:, H:4 * H]], 1) if glob
                             else torch.cat([w_env, w_r], 1))
        dR = torch.empty(LMa, GW, device=g.device)
        TS._dgrad(g, lin.out_features, lin.out_features, sc, TS._dqn_first_x3t(lin, od, H, glob), LMa, GW, GW,
                  None, 0, dR, GW)
        hold["dR"] = dR

    return first


@torch.no_grad()
def _target(pn, pd, model_tar):
    """max_a Q_target [L, B, A] of the target DGN on [next graph obs | next env obs] with next_adj, all L steps'
    rows in one no-grad pass (DGN.forward_rows with the first encoder layer on its two dense sources); pd.tar_qkv =
    its per-layer qkv rows for the regulariser."""
    Ls, B, A, N, F, od, odp, H, K, M, Ma = pn.dims
    sb = pn.seq
    LM = Ls * Ma
    GW = pn.GW
    Rn = _next_graph_rows(pn)
    env = sb.next_obs.reshape(LM, odp)
    nadj = sb.next_adj.reshape(Ls * B, A, A)
    nadj = nadj if nadj.is_contiguous() else nadj.contiguous()
    bufs = {}
    scratch = MD._scratch_dict(bufs)
    hid = model_tar.encoder.out_features
    nl = len(model_tar.att_layers)
    qin = scratch(("dgn_qin", id(model_tar)), LM, hid * (nl + 1))
    layers = list(model_tar.encoder.linear_layers)
    h = ld = kk = None
    for i, lin in enumerate(layers):
        n = lin.out_features
        dst = qin if i == len(layers) - 1 else scratch(("mlp", id(model_tar.encoder), i), LM, n)
        if i == 0:
            target_first(pn, lin, Rn, env, dst)
        else:
            FU.linear_rows(lin, h, ld, LM, dst, dst.stride(0), k=kk)
        h, ld, kk = dst, dst.stride(0), n
    for li, layer in enumerate(model_tar.att_layers):
        layer.forward_rows(qin[:, li * hid:], qin.stride(0), nadj, Ls * B, A, qin[:, (li + 1) * hid:], qin.stride(0),
                           scratch)
    fc = model_tar.q_net.fc
    q = torch.empty(LM, fc.out_features, device=qin.device)
    FU.linear_rows(fc, qin, qin.stride(0), LM, q, q.stride(0))
    pd.tar_qkv = [bufs[(("qkv", id(a)), LM, a.num_heads * (a.v_features + 2 * a.k_features))]
                  for a in model_tar.att_layers]
    return q.view(Ls, B, A, -1).max(dim=-1)[0]


def _forward(pn, pd):
    """(q [L*B*A, nq], kl [L*B*A] or None); pd.next_max = the target pass's max_a Q [L, B, A]."""
    TS._forward_netmon(pn)
    pd.next_max = _target(pn, pd, pd.model_tar)
    return DS._forward(pd, first=first_forward(pn))


def _backward(pn, pd, dq, r):
    hold = {}
    grads = DS._backward(pd, dq, r, first=first_backward(pn, hold))
    TS._backward_netmon(pn, hold["dR"], grads)
    return grads


class _DGNNetMonFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pn, pd, *params):
        ctx.plans = (pn, pd)
        with torch.no_grad():
            q, kl = _forward(pn, pd)
        if kl is None:
            return q
        return q, kl

    @staticmethod
    def backward(ctx, dq, dkl=None):
        pn, pd = ctx.plans
        if dq is None:
            dq = torch.zeros(pd.dims[-1], pd.model.q_net.fc.out_features, device=pd.qin.device)
        grads = _backward(pn, pd, dq, None if dkl is None else dkl.contiguous())
        ctx.plans = None
        return (None, None) + tuple(grads.get(w) for w in pd.params)


def dgn_netmon_seq_loss(netmon, model, model_tar, seq, gamma, params, att_coeff=0.0, parts=None):
    """TD loss of src/main.py:840-1000 over a DGNNetMonSeqBatch, plus att_coeff times the attention regulariser when
    att_coeff > 0: (loss, q [L, B, A, nq], q_target)."""
    Ls, B, A = seq.action.shape
    if A > DS.MAX_AGENTS:
        raise ValueError(f"dgn_netmon_seq_loss: at most {DS.MAX_AGENTS} agents")
    pn, pd = TS._Plan(), TS._Plan()
    pn.netmon, pn.seq = netmon, seq
    pd.model, pd.model_tar, pd.seq, pd.params = model, model_tar, seq, list(params)
    pd.reg = att_coeff > 0
    out = _DGNNetMonFn.apply(pn, pd, *pd.params)
    q, kl = out if pd.reg else (out, None)
    q = q.view(Ls, B, A, -1)
    target = seq.reward + (~seq.done) * gamma * pd.next_max
    q_target = torch.scatter(q.detach(), -1, seq.action.unsqueeze(-1), target.unsqueeze(-1))
    loss_q = (q - q_target).pow(2).mean(dim=(1, 2, 3)).sum() / Ls
    loss, loss_att = loss_q, None
    if pd.reg:  # train.attention_kl per step: the mean over the agents that are not done; steps averaged
        nd = ~seq.done
        loss_att = ((kl.view(Ls, B * A) * nd.view(Ls, B * A)).sum(1)
                    / torch.clamp(nd.view(Ls, B * A).sum(1), min=1)).sum() / Ls
        loss = loss_q + att_coeff * loss_att
    if parts is not None:
        parts.update(loss_q=loss_q, loss_att=loss_att, loss_aux=None)
    return loss, q, q_target


def dgn_netmon_update_seq(netmon, model, model_tar, optimizer, params, seq, gamma, tau, target_update_steps=0,
                          iteration=1, group=None, att_coeff=0.0, parts=None):
    """One update (src/main.py:840-1026) on a DGNNetMonSeqBatch: the batched loss and backward, the gradient
    all-reduce across ranks, clip by value (0.5) and norm (1.0), AdamW, target update."""
    from .train import allreduce_gradients, interpolate_model

    loss, q, qt = dgn_netmon_seq_loss(netmon, model, model_tar, seq, gamma, params, att_coeff, parts)
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
