"""Sequence-batched DQN update for the agent models with a carried state, DQNR and CommNet, without NetMon
(reference src/main.py:840-1000 on replay sequences; src/model.py:653-794), with a hand-written backward.

The reference runs, per step t of a sampled sequence of L consecutive transitions, the model on the stored
observation (agent state carried from the stored start state, zeroed for done agents and at episode ends), the
target model on the stored next observation starting from the online model's state after the step, and
backpropagates the summed TD loss through all of it with autograd (train.dqn_loss). Here the same computation is
one autograd node over the whole sequence (`_AgentSeqFn`), organised like train_seq.py:

  * everything without recurrence runs ONCE over all L steps' rows: the encoder MLP (L*B*A rows, sign bits of
    every leaky output saved for the backward), the Q head on the final h rows, the encoder's and the LSTM's
    weight gradients, and the whole target model: it starts every step from the online state of that step and
    has no recurrence of its own, so its encoder, LSTM cell, CommNet rounds (on next_adj) and head are one
    no-grad pass over all steps' rows;
  * only the LSTM cells and CommNet's communication run per step. Forward: one [x | h] GEMM per cell with the gate
    math in its epilogue (hidden sizes that are no multiple of 32 have no gate-tile packing: one GM_EPI_BIAS GEMM on
    the concatenated rows + gm_lstm_pointwise); CommNet follows the obs cell with comm_rounds cells on x = h =
    gm_agent_comm(h): the same rows are both GEMM sources and c comes from the previous state rows, so no
    [h + comm | c] rows are built. Backward, steps and cells reversed: gm_lstm_cell_bwd sums the cell's gradient
    sources (the head's dh, the next round's gm_agent_comm_bwd output, the next step's state gradient under the
    per-agent-row mask ~done & ~episode_done), then one gm_gemm_x3_dgrad on [W_ih | W_hh]^T gives [dx | dh]; a
    comm-round cell's x and h are the same tensor, so gm_agent_comm_bwd takes the two halves as its two sources;
  * gm_qhead_bwd (act = 0: the head reads h directly) gives every step's dh and the head's gradients in one call;
    the obs cell's dx rows of all steps land in one buffer, masked by the encoder's last leaky derivative, for the
    batched encoder backward.

DQNR / CommNet on NetMon graph observations: agent_netmon_seq.py, which calls _forward / _backward / _target_max here
with the encoder's first layer in its own hands (`first`, `encode`). Every other configuration (aux loss, GM_GEMM=f32)
keeps train.dqn_loss; DGN, attention regularisation included, has its own batched updates (dgn_seq.py without NetMon,
dgn_netmon_seq.py with it).
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L
from . import fused as FU
from . import model as MD
from . import train_seq as TS

AgentSeqBatch = namedtuple("AgentSeqBatch", ["obs", "obs_dim", "action", "reward", "done", "episode_done", "adj",
                                             "next_obs", "next_adj", "agent_state", "idx"], defaults=(None,))
"""All L steps of B replay sequences, stacked: obs, next_obs [L, B, A, odp] (first obs_dim columns valid), action
[L, B, A] long, reward [L, B, A], done [L, B, A] bool, episode_done [L, B] bool, adj, next_adj [L, B, A, A] int8
(None for models without communication), agent_state [B, A, 2H] (the agent state before step 0, [h | c])."""

MAX_AGENTS = 64  # gm_agent_comm / gm_agent_comm_bwd


def _cell_bwd_ok(H):
    """Hidden sizes gm_lstm_cell_bwd accepts (its launch code: any H <= 256, or a multiple of 64 up to 1024);
    H % 4: 16-byte state rows."""
    return H % 4 == 0 and (H <= 256 or (H % 64 == 0 and H <= 1024))


def agent_seq_ok(model, model_tar, netmon=None, att_coeff=0.0, aux_model=None, n_agents=None):
    """The sequence-batched path covers DQNR and CommNet without NetMon: leaky MLPs with biases, a head of at most
    4 actions, a hidden size gm_lstm_cell_bwd takes, at most 64 agents, split-f16 GEMMs."""
    if netmon is not None or aux_model is not None or att_coeff != 0 or L.GEMM_MODE != "x3":
        return False
    if type(model) not in (MD.DQNR, MD.CommNet) or type(model_tar) is not type(model):
        return False
    if n_agents is not None and n_agents > MAX_AGENTS:
        return False
    for m in (model, model_tar):
        layers = list(m.encoder.linear_layers)
        fc = m.q_net.fc
        if not (all(l.act == 1 and l.bias is not None for l in layers) and fc.act == 0 and fc.bias is not None
                and fc.out_features <= 4 and _cell_bwd_ok(m.lstm.hidden_size)
                and m.lstm.input_size == m.lstm.hidden_size):
            return False
    return (model.lstm.hidden_size == model_tar.lstm.hidden_size
            and getattr(model, "comm_rounds", 0) == getattr(model_tar, "comm_rounds", 0))


def _rows16(x2d, k):
    """x2d's rows as a 16-byte-aligned buffer (a zero-padded copy when the stride or base is not)."""
    if x2d.stride(1) == 1 and x2d.stride(0) % 4 == 0 and x2d.data_ptr() % 16 == 0:
        return x2d
    xp = torch.zeros(x2d.shape[0], (k + 3) // 4 * 4, device=x2d.device)
    xp[:, :k] = x2d[:, :k]
    return xp


def _lstm_nat(cell):
    """(X3 of [W_ih | W_hh] in natural gate order, b_ih + b_hh): the cell's gates as one GM_EPI_BIAS GEMM."""
    def build():
        with torch.no_grad():
            return (TS._x3(torch.cat([cell.weight_ih.detach(), cell.weight_hh.detach()], 1)),
                    (cell.bias_ih.detach() + cell.bias_hh.detach()).contiguous())
    return TS._cache(cell).get("nat", FU._key(cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), build)


def _cell_fwd(cell, x, h, c, out, act=None, slot=None):
    """One LSTMCell on M rows: x, h, c [M, H] row views (any 16-byte row stride), out [M, 2H] = [h' | c'];
    act [M, 4H] (optional) receives the gate activations, slot (optional) max |[x | h]|."""
    M, H = x.shape
    amax = None if slot is None else slot.data_ptr()
    if H % 32 == 0:  # gate tiles: the gate math in the GEMM's epilogue
        wp, ldw, bp, x3 = TS._lstm_fwd(cell)
        FU.gemm(FU.dense(x.data_ptr(), x.stride(0), H, amax=amax), FU.dense(h.data_ptr(), h.stride(0), H),
                wp.data_ptr(), ldw, bp.data_ptr(), M, 4 * H, FU.GM_EPI_LSTM, out.data_ptr(), 2 * H,
                out.data_ptr() + 4 * H, 2 * H, c.data_ptr(), c.stride(0), None if act is None else act.data_ptr(),
                x3=x3)
        return
    x3, b = _lstm_nat(cell)
    xh = torch.cat([x, h], 1)
    gates = torch.empty(M, 4 * H, device=x.device)
    FU.gemm(FU.dense(xh.data_ptr(), 2 * H, 2 * H, amax=amax), None, None, 0, b.data_ptr(), M, 4 * H, FU.GM_EPI_BIAS,
            gates.data_ptr(), 4 * H, x3=x3)
    h1, c1 = torch.empty(M, H, device=x.device), torch.empty(M, H, device=x.device)
    L.check(L.lib().gm_lstm_pointwise(L.ptr(gates), L.ptr(c.contiguous()), M, H, L.ptr(h1), L.ptr(c1), L.ptr(act),
                                      L.stream_ptr()))
    out[:, :H].copy_(h1)
    out[:, H:].copy_(c1)


def _comm(h_rows, adj, n_env, A, H, out):
    """out [n_env * A, H] = gm_agent_comm of the h half of the [h | c] rows h_rows."""
    L.check(L.lib().gm_agent_comm(h_rows.data_ptr(), h_rows.stride(0), adj.data_ptr(), n_env, A, H, out.data_ptr(),
                                  out.stride(0), L.stream_ptr()))


def _forward(p, first=None):
    """first (agent_netmon_seq.py): the encoder's first layer in the caller's hands, first(lin, y, ldy, sign bits) ->
    the zeroed max |input| slot its GEMM published into; the env observation rows are then not read here."""
    model, sb = p.model, p.seq
    dev = sb.obs.device
    Ls, B, A, odp = sb.obs.shape
    od = sb.obs_dim
    H = model.lstm.hidden_size
    R = getattr(model, "comm_rounds", 0)
    M = B * A
    LM = Ls * M
    p.dims = (Ls, B, A, od, H, R, M)
    X = _rows16(sb.obs.reshape(LM, odp), od) if first is None else None

    # ---- encoder over all steps ----
    enc = list(model.encoder.linear_layers)
    p.enc_in, p.enc_out, p.enc_bits = [], [], []
    x, ldx, kx = (X, X.stride(0), od) if first is None else (None, 0, 0)
    for i, lin in enumerate(enc):
        n = lin.out_features
        y = torch.empty(LM, n, device=dev)
        yb = TS._sign_bits(LM, n, dev)  # the leaky mask of this output for the backward
        if i == 0 and first is not None:
            sx = first(lin, y, n, yb)
        else:
            sx = TS._zeros1(dev)
            TS._gemm_amax(x, ldx, kx, TS._lin_x3(lin), lin.bias, LM, n, FU.GM_EPI_BIAS_LEAKY, y, n, sx, sbits=yb)
        # with a `first` hook layer 0's entry is (None, 0, 0, scale): _backward hands that layer to its own hook and
        # never reads the input rows
        p.enc_in.append((x, ldx, kx, TS._finish(sx)))
        p.enc_out.append(y)
        p.enc_bits.append(yb)
        x, ldx, kx = y, n, n
    E = p.enc_out[-1].view(Ls, M, H)  # the obs cell's x

    # ---- LSTM cells (and communication rounds), per step ----
    S_in = torch.empty(Ls, M, 2 * H, device=dev)
    S = torch.empty(R + 1, Ls, M, 2 * H, device=dev)  # cell outputs [h | c]: 0 obs cell, 1..R comm rounds
    act = torch.empty(R + 1, Ls, M, 4 * H, device=dev)
    HC = torch.empty(R, Ls, M, H, device=dev)  # h + comm: x and h of the comm-round cells
    s_cell = TS._zeros1(dev)  # max |[x | h]| over every cell (one weight)
    kill = (sb.done | sb.episode_done.unsqueeze(-1)).reshape(Ls, M)  # rows whose state restarts after step t
    keep = (~kill).to(torch.float32).unsqueeze(-1)
    S_in[0].copy_(sb.agent_state.reshape(M, 2 * H))
    adj = None if R == 0 else sb.adj.reshape(Ls, B, A, A)
    for t in range(Ls):
        if t > 0:  # the state carried from step t-1, zeroed for done agents and at its episode end (956-964)
            torch.mul(S[R, t - 1], keep[t - 1], out=S_in[t])
        _cell_fwd(model.lstm, E[t], S_in[t][:, :H], S_in[t][:, H:], S[0, t], act[0, t], s_cell)
        for r in range(1, R + 1):
            prev = S[r - 1, t]
            _comm(prev, adj[t], B, A, H, HC[r - 1, t])
            _cell_fwd(model.lstm, HC[r - 1, t], HC[r - 1, t], prev[:, H:], S[r, t], act[r, t], s_cell)
    TS._finish(s_cell)
    p.S_in, p.S, p.act, p.HC, p.s_cell, p.kill = S_in, S, act, HC, s_cell, kill.to(torch.uint8).contiguous()

    # ---- Q head over all steps ----
    fc = model.q_net.fc
    q = torch.empty(LM, fc.out_features, device=dev)
    FU.linear_rows(fc, S[R], 2 * H, LM, q, q.stride(0), k=H)
    return q


def _backward(p, dq, first=None):
    """first (agent_netmon_seq.py): first(lin, g, its scale, the layer input's scale, grads) takes the encoder's first
    layer's weight gradient (and whatever lies below it) in place of the one-source weight gradient here."""
    model, sb = p.model, p.seq
    Ls, B, A, od, H, R, M = p.dims
    dev = dq.device
    LM = Ls * M
    lib = L.lib()
    grads = {}
    dq = dq.contiguous()
    cell = model.lstm

    # ---- Q head: its gradients and every step's dh in one pass ----
    fc = model.q_net.fc
    nq = fc.out_features
    rpb = 512
    nb = (LM + rpb - 1) // rpb
    dhf = torch.empty(Ls, M, H, device=dev)
    part_b = torch.empty(nb, H, device=dev)  # (the column sums of dh: no bias sits between the cell and the head)
    part_wq = torch.empty(nb, nq, H, device=dev)
    part_bq = torch.empty(nb, nq, device=dev)
    wq = fc.weight.detach().contiguous()
    L.check(lib.gm_qhead_bwd(dq.data_ptr(), nq, nq, wq.data_ptr(), wq.stride(0), p.S[R].data_ptr(), 2 * H, LM, H, 0,
                             dhf.data_ptr(), H, part_b.data_ptr(), part_wq.data_ptr(), part_bq.data_ptr(), rpb, None,
                             L.stream_ptr()))
    grads[fc.weight] = part_wq.sum(0)
    grads[fc.bias] = part_bq.sum(0)

    # ---- LSTM cells, per step and round, in reverse ----
    dG = torch.empty(R + 1, Ls, M, 4 * H, device=dev)
    rpb_c = 64
    bpart = torch.empty(R + 1, Ls, (M + rpb_c - 1) // rpb_c, 4 * H, device=dev)
    gmax_cell = TS._zeros1(dev)
    sc_cell = torch.empty(1, device=dev)
    Eb = p.enc_bits[-1]
    gE = torch.empty(Ls, M, H, device=dev)
    partE = torch.empty(Ls, (M + 127) // 128, H, device=dev)
    gmaxE = TS._zeros1(dev)
    wt = TS._lstm_x3t(cell)
    D = torch.empty(M, 2 * H, device=dev)    # a comm-round cell's [dx | dh]
    dhc = torch.empty(M, H, device=dev)      # its gm_agent_comm_bwd: the previous cell's dh
    dh0_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    # every cell's dc source is the dc output of the cell processed just before it: two buffers in turn
    dc_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    adj = None if R == 0 else sb.adj.reshape(Ls, B, A, A)
    dh_ext = dc_ext = None
    calls = 0
    for t in range(Ls - 1, -1, -1):
        dc_next = None
        for j in range(R, -1, -1):
            a = L.LSTMBwdArgs()
            a.act, a.ld_act = p.act[j, t].data_ptr(), 4 * H
            cin = p.S_in[t] if j == 0 else p.S[j - 1, t]
            a.c_in, a.ld_cin = cin.data_ptr() + 4 * H, 2 * H
            a.c_out, a.ld_cout = p.S[j, t].data_ptr() + 4 * H, 2 * H
            if j == R:
                a.dh0, a.ld_dh0 = dhf[t].data_ptr(), H
                if dh_ext is not None:  # step t+1's input-state gradient, zero for the rows whose state restarted
                    a.dh_ext, a.ld_ext = dh_ext.data_ptr(), H
                    a.dc_ext, a.ld_dcext = dc_ext.data_ptr(), H
                    a.ext_mask, a.rows_per_sample = p.kill[t].data_ptr(), 1
            else:
                a.dh0, a.ld_dh0 = dhc.data_ptr(), H
            if dc_next is not None:
                a.dc, a.ld_dc = dc_next.data_ptr(), H
            a.m, a.hidden = M, H
            a.dgates, a.ld_dg = dG[j, t].data_ptr(), 4 * H
            dco = None
            if j > 0 or t > 0:  # the gradient w.r.t. the replayed start state is not needed
                dco = dc_buf[calls % 2]
                a.dc_out, a.ld_dco = dco.data_ptr(), H
            calls += 1
            a.bias_part, a.rows_per_block = bpart[j, t].data_ptr(), rpb_c
            a.dg_scale = sc_cell.data_ptr()
            a.dg_max = gmax_cell.data_ptr()
            L.check(lib.gm_lstm_cell_bwd(C.byref(a), L.stream_ptr()))
            if j > 0:
                # x = h = h_prev + comm(h_prev): both halves of [dx | dh] go through the transposed communication
                TS._dgrad(dG[j, t], 4 * H, 4 * H, sc_cell, wt, M, 2 * H, 2 * H, None, 0, D, 2 * H)
                L.check(lib.gm_agent_comm_bwd(D.data_ptr(), 2 * H, D.data_ptr() + 4 * H, 2 * H, adj[t].data_ptr(), B,
                                              A, H, dhc.data_ptr(), H, L.stream_ptr()))
            else:
                # the obs cell: x part through the encoder's last leaky_relu (bias partials and max for the batched
                # encoder backward), h part = the state gradient of step t-1
                dh0 = dh0_buf[t % 2]
                TS._dgrad(dG[0, t], 4 * H, 4 * H, sc_cell, wt, M, 2 * H, H, Eb[t * M:(t + 1) * M], Eb.stride(0),
                          gE[t], H, dh0, H, part=partE[t], gmax=gmaxE)
                dh_ext, dc_ext = dh0, dco
            dc_next = dco

    # ---- LSTM weight / bias gradients over all steps and rounds ----
    sa = TS._finish(gmax_cell)
    sx = p.s_cell
    gi, gh = MD._wgrad_pair(dG[0].view(LM, 4 * H), p.enc_out[-1], H, p.S_in.view(LM, 2 * H), H, sa, sx, sx)
    if R:  # x and h of a comm-round cell are the same rows: one product serves W_ih and W_hh
        gr = TS._wgrad(dG[1:].reshape(R * LM, 4 * H), sa, p.HC.view(R * LM, H), H, sx)
        gi, gh = gi + gr, gh + gr
    grads[cell.weight_ih], grads[cell.weight_hh] = gi, gh
    bg = bpart.reshape(-1, 4 * H).sum(0)
    grads[cell.bias_ih], grads[cell.bias_hh] = bg, bg.clone()

    # ---- encoder over all steps ----
    enc = list(model.encoder.linear_layers)
    g, sc = gE.view(LM, H), TS._finish(gmaxE)
    grads[enc[-1].bias] = partE.reshape(-1, H).sum(0)
    for i in range(len(enc) - 1, -1, -1):
        lin = enc[i]
        xin, ldx, kin, sxi = p.enc_in[i]
        if i == 0 and first is not None:
            first(lin, g, sc, sxi, grads)
        else:
            grads[lin.weight] = TS._wgrad(g, sc, xin, kin, sxi)
        if i > 0:
            gn = torch.empty(LM, kin, device=dev)
            part = torch.empty((LM + 127) // 128, kin, device=dev)
            gmax = TS._zeros1(dev)
            xb = p.enc_bits[i - 1]
            TS._dgrad(g, lin.out_features, lin.out_features, sc, TS._lin_x3t(lin), LM, kin, kin, xb, xb.stride(0), gn,
                      kin, part=part, gmax=gmax)
            grads[enc[i - 1].bias] = part.sum(0)
            g, sc = gn, TS._finish(gmax)
    return grads


class _AgentSeqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, *params):
        ctx.plan = plan
        with torch.no_grad():
            return _forward(plan)

    @staticmethod
    def backward(ctx, dq):
        p = ctx.plan
        grads = _backward(p, dq)
        ctx.plan = None
        return (None,) + tuple(grads.get(w) for w in p.params)


@torch.no_grad()
def _target_max(p, model_tar, encode=None):
    """max_a Q_target(next obs) [L, B, A]: the target model starts step t from the online model's state after
    step t, before the done / episode-end mask (src/main.py:899-902), and carries nothing from step to step, so
    all L steps are one pass over L*B*A rows: encoder on the stored next observations, one LSTM cell, CommNet's
    rounds on next_adj, head, max. encode (agent_netmon_seq.py): encode(encoder, rows, scratch) -> the target
    encoder's output rows, in place of the encoder pass on the stored next observations."""
    Ls, B, A, od, H, R, M = p.dims
    sb = p.seq
    dev = sb.next_obs.device
    LM = Ls * M
    if encode is None:
        X = _rows16(sb.next_obs.reshape(LM, sb.next_obs.shape[-1]), od)
        E = FU.mlp_rows(model_tar.encoder, X, X.stride(0), od, LM, MD._scratch_dict({}))
    else:
        E = encode(model_tar.encoder, LM, MD._scratch_dict({}))
    st = p.S[R].view(LM, 2 * H)
    S = torch.empty(LM, 2 * H, device=dev)
    _cell_fwd(model_tar.lstm, E, st[:, :H], st[:, H:], S)
    for _ in range(R):
        hc = torch.empty(LM, H, device=dev)
        _comm(S, sb.next_adj, Ls * B, A, H, hc)
        S2 = torch.empty(LM, 2 * H, device=dev)
        _cell_fwd(model_tar.lstm, hc, hc, S[:, H:], S2)
        S = S2
    fc = model_tar.q_net.fc
    q = torch.empty(LM, fc.out_features, device=dev)
    FU.linear_rows(fc, S, 2 * H, LM, q, q.stride(0), k=H)
    return q.view(Ls, B, A, -1).max(dim=-1)[0]


def agent_seq_loss(model, model_tar, seq, gamma, params, parts=None):
    """TD loss of src/main.py:840-1000 over an AgentSeqBatch: (loss, q [L, B, A, nq], q_target)."""
    p = TS._Plan()
    p.model, p.seq, p.params = model, seq, list(params)
    Ls, B, A = seq.action.shape
    if A > MAX_AGENTS:
        raise ValueError(f"agent_seq_loss: at most {MAX_AGENTS} agents")
    q = _AgentSeqFn.apply(p, *p.params).view(Ls, B, A, -1)
    nxt = _target_max(p, model_tar)
    target = seq.reward + (~seq.done) * gamma * nxt
    q_target = torch.scatter(q.detach(), -1, seq.action.unsqueeze(-1), target.unsqueeze(-1))
    loss = (q - q_target).pow(2).mean(dim=(1, 2, 3)).sum() / Ls
    if parts is not None:
        parts.update(loss_q=loss, loss_att=None, loss_aux=None)
    return loss, q, q_target


def agent_update_seq(model, model_tar, optimizer, params, seq, gamma, tau, target_update_steps=0, iteration=1,
                     group=None):
    """One update (src/main.py:840-1026) on an AgentSeqBatch: the sequence-batched loss and backward, the gradient
    all-reduce across ranks, clip by value (0.5) and norm (1.0), AdamW, target update."""
    from .train import allreduce_gradients, interpolate_model

    loss, q, qt = agent_seq_loss(model, model_tar, seq, gamma, params)
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
