"""Batched DQN update for DGN without NetMon (reference src/main.py:840-1000; src/model.py:45-176), with a
hand-written backward on the HIP attention kernels.

DGN has no recurrence, so the L steps of a sampled sequence are one batch of L*B*A rows for the online model and
for the target model alike: no per-step loop. The update is one autograd node over the whole sequence (`_DGNSeqFn`),
organised like agent_seq.py:

  * forward, once over all rows: the encoder MLP into the first segment of the head's input buffer [LM, hidden *
    (layers + 1)] (sign bits of every leaky output saved for the backward), per attention layer one GEMM on the
    concatenated [W_v; W_k; W_q], gm_agent_attention on the columns of that qkv buffer, and the fc_out GEMM into the
    layer's segment; the Q head reads the whole buffer;
  * the target model runs once, no-grad, on the stored next observations / next adjacency through DGN.forward_rows;
    its per-layer qkv rows are kept for the attention regulariser;
  * the regulariser (src/main.py:924-985, train.attention_kl) never materialises att_weights: gm_agent_attention_kl
    gives KL(softmax(target scores) || softmax(online scores)) per source agent from the q / k rows; the sum over the
    layers, the ~done mask, the division by clamp(#not done, 1) and by L are torch ops on those [LM] rows, so the
    row gradient the node receives for them is the scale r of the backward's regulariser term (coefficient and
    upstream gradient included; no host sync);
  * backward: gm_qhead_bwd gives the head's gradients and, with the leaky derivative of every segment, the head's
    part of each segment's gradient; per layer in reverse: the fc_out weight / bias / input gradients,
    gm_agent_attention_bwd (with the regulariser term when att_coeff > 0), the leaky derivative of q / k / v
    (gm_leaky_bwd: bias partials and the operand scale in the same pass), one weight gradient and one input-gradient
    GEMM on the concatenated [W_v; W_k; W_q] (the layer input's leaky derivative fused), added to the input segment's
    gradient; then the batched encoder backward.

Every GEMM runs in the split-f16 form with fp32 accumulation, as in train.dqn_loss, which remains the path for every
other configuration (other activations, aux loss, GM_GEMM=f32, more than 64 agents). DGN with NetMon:
dgn_netmon_seq.py, which calls _forward / _backward here with the encoder's first layer in its own hands (`first`).
"""
from collections import namedtuple

import torch

from . import _lib as L
from . import agent_seq as AS
from . import fused as FU
from . import model as MD
from . import train_seq as TS

DGNSeqBatch = namedtuple("DGNSeqBatch", ["obs", "obs_dim", "action", "reward", "done", "episode_done", "adj",
                                         "next_obs", "next_adj", "idx"], defaults=(None,))
"""All L steps of B replay sequences, stacked: obs, next_obs [L, B, A, odp] (first obs_dim columns valid), action
[L, B, A] long, reward [L, B, A], done [L, B, A] bool, episode_done [L, B] bool, adj, next_adj [L, B, A, A] int8."""

MAX_AGENTS = 64  # gm_agent_attention / gm_agent_attention_bwd / gm_agent_attention_kl
MAX_D = 64       # their per-head key / value width
MAX_LDS = 160 * 1024


def bwd_lds_bytes(A, heads, dk, dv, reg):
    """LDS bytes gm_agent_attention_bwd needs per env: the k, v (and k_tar) rows (q, dout, q_tar take their place in
    its second phase), the row statistics and adj."""
    return 4 * A * heads * ((2 if reg else 1) * dk + dv + (8 if reg else 3)) + (A * A + 15) // 16 * 16


def dgn_seq_ok(model, model_tar, netmon=None, att_coeff=0.0, aux_model=None, n_agents=None):
    """The batched path covers DGN without NetMon: leaky layers with biases (the attention layers' fc_v / k / q / out
    too), a linear head of at most 4 actions on at most 1024 inputs, at most 64 agents, dk, dv <= 64 within the
    kernels' LDS bound, split-f16 GEMMs, att_coeff >= 0."""
    if netmon is not None or aux_model is not None or att_coeff < 0 or L.GEMM_MODE != "x3":
        return False
    if type(model) is not MD.DGN or type(model_tar) is not MD.DGN:
        return False
    if n_agents is not None and n_agents > MAX_AGENTS:
        return False
    if len(model.att_layers) != len(model_tar.att_layers) or not len(model.att_layers):
        return False
    for m in (model, model_tar):
        hid = m.encoder.out_features
        fc = m.q_net.fc
        lins = list(m.encoder.linear_layers)
        for a in m.att_layers:
            lins += [a.fc_v, a.fc_k, a.fc_q, a.fc_out]
            nh, dk, dv = a.num_heads, a.k_features, a.v_features
            if dk > MAX_D or dv > MAX_D or (nh * dv) % 4 or (nh * (dv + 2 * dk)) % 4:
                return False
            if bwd_lds_bytes(n_agents or 1, nh, dk, dv, att_coeff > 0) > MAX_LDS:
                return False
        if not (all(l.act == 1 and l.bias is not None for l in lins) and fc.act == 0 and fc.bias is not None
                and fc.out_features <= 4 and fc.in_features == hid * (len(m.att_layers) + 1)
                and fc.in_features <= 1024 and hid % 4 == 0):
            return False
    return True


def _cat(layer):
    """The layer's fc_v, fc_k, fc_q as one Linear ([W_v; W_k; W_q], AttModel.forward_rows' column order)."""
    return FU.concat_linears(layer, (layer.fc_v, layer.fc_k, layer.fc_q))


def _qkv_ptrs(buf, layer):
    """(q, k, v) column pointers into a [M, heads * (dv + 2 dk)] qkv buffer."""
    nh, dk, dv = layer.num_heads, layer.k_features, layer.v_features
    p = buf.data_ptr()
    return p + 4 * nh * (dv + dk), p + 4 * nh * dv, p


def _forward(p, first=None):
    """first (dgn_netmon_seq.py): the encoder's first layer in the caller's hands, first(lin, y, ldy, sign bits) ->
    the zeroed max |input| slot its GEMM published into; the env observation rows are then not read here."""
    model, sb = p.model, p.seq
    dev = sb.obs.device
    Ls, B, A, odp = sb.obs.shape
    od = sb.obs_dim
    hid = model.encoder.out_features
    nl = len(model.att_layers)
    Hq = hid * (nl + 1)
    LM = Ls * B * A
    p.dims = (Ls, B, A, od, hid, nl, Hq, LM)
    lib = L.lib()
    X = AS._rows16(sb.obs.reshape(LM, odp), od) if first is None else None
    qin = torch.empty(LM, Hq, device=dev)  # [h_enc | h_1 | ...]: the head's input, every segment a leaky output
    p.qin = qin

    # ---- encoder over all rows, the last layer into segment 0 ----
    enc = list(model.encoder.linear_layers)
    p.enc_in, p.enc_bits, p.bits = [], [], []
    x, ldx, kx = (X, X.stride(0), od) if first is None else (None, 0, 0)
    for i, lin in enumerate(enc):
        n = lin.out_features
        last = i == len(enc) - 1
        y, ldy = (qin, Hq) if last else (torch.empty(LM, n, device=dev), n)
        yb = TS._sign_bits(LM, n, dev)
        if i == 0 and first is not None:
            sx = first(lin, y, ldy, yb)
        else:
            sx = TS._zeros1(dev)
            TS._gemm_amax(x, ldx, kx, TS._lin_x3(lin), lin.bias, LM, n, FU.GM_EPI_BIAS_LEAKY, y, ldy, sx, sbits=yb)
        p.enc_in.append((x, ldx, kx, TS._finish(sx)))
        if last:
            p.bits.append(yb)  # bits[s]: the sign bits of segment s
        else:
            p.enc_bits.append(yb)
        x, ldx, kx = y, ldy, n

    # ---- attention layers ----
    adj = sb.adj.reshape(Ls * B, A, A)
    adj = adj if adj.is_contiguous() else adj.contiguous()
    p.adj = adj
    p.qkv, p.core, p.s_x, p.s_core = [], [], [], []
    for li, layer in enumerate(model.att_layers):
        nh, dk, dv = layer.num_heads, layer.k_features, layer.v_features
        cat = _cat(layer)
        nqkv = cat.out_features
        xl = qin[:, li * hid:]
        qkv = torch.empty(LM, nqkv, device=dev)
        sx = TS._zeros1(dev)
        TS._gemm_amax(xl, Hq, hid, TS._lin_x3(cat), cat.bias, LM, nqkv, FU.GM_EPI_BIAS_LEAKY, qkv, nqkv, sx)
        core = torch.empty(LM, nh * dv, device=dev)
        qp, kp, vp = _qkv_ptrs(qkv, layer)
        L.check(lib.gm_agent_attention(qp, kp, vp, nqkv, adj.data_ptr(), Ls * B, A, nh, dk, dv, core.data_ptr(),
                                       nh * dv, None, L.stream_ptr()))
        yb = TS._sign_bits(LM, hid, dev)
        sc = TS._zeros1(dev)
        fo = layer.fc_out
        TS._gemm_amax(core, nh * dv, nh * dv, TS._lin_x3(fo), fo.bias, LM, hid, FU.GM_EPI_BIAS_LEAKY,
                      qin[:, (li + 1) * hid:], Hq, sc, sbits=yb)
        p.qkv.append(qkv)
        p.core.append(core)
        p.s_x.append(TS._finish(sx))
        p.s_core.append(TS._finish(sc))
        p.bits.append(yb)

    # ---- Q head over the whole buffer ----
    fc = model.q_net.fc
    q = torch.empty(LM, fc.out_features, device=dev)
    FU.linear_rows(fc, qin, Hq, LM, q, q.stride(0))

    # ---- the regulariser's value per source agent, summed over the layers ----
    kl = None
    if p.reg:
        kl = torch.zeros(LM, device=dev)
        row = torch.empty(LM, device=dev)
        for layer, lt, qkv, tqkv in zip(model.att_layers, p.model_tar.att_layers, p.qkv, p.tar_qkv):
            qp, kp, _ = _qkv_ptrs(qkv, layer)
            tq, tk, _ = _qkv_ptrs(tqkv, lt)
            L.check(lib.gm_agent_attention_kl(qp, kp, qkv.stride(0), tq, tk, tqkv.stride(0), Ls * B, A,
                                              layer.num_heads, layer.k_features, row.data_ptr(), L.stream_ptr()))
            kl += row
    return q, kl


def _backward(p, dq, r, first=None):
    """first (dgn_netmon_seq.py): first(lin, g, its scale, the layer input's scale, grads) takes the encoder's first
    layer's weight gradient (and whatever lies below it) in place of the one-source weight gradient here."""
    model = p.model
    Ls, B, A, od, hid, nl, Hq, LM = p.dims
    dev = dq.device
    lib = L.lib()
    grads = {}
    dq = dq.contiguous()

    # ---- Q head: its gradients and, through every segment's leaky derivative, the head's part of each segment ----
    fc = model.q_net.fc
    nq = fc.out_features
    rpb = 512
    nb = (LM + rpb - 1) // rpb
    G = torch.empty(LM, Hq, device=dev)
    part_b = torch.empty(nb, Hq, device=dev)
    part_wq = torch.empty(nb, nq, Hq, device=dev)
    part_bq = torch.empty(nb, nq, device=dev)
    wq = fc.weight.detach().contiguous()
    L.check(lib.gm_qhead_bwd(dq.data_ptr(), nq, nq, wq.data_ptr(), wq.stride(0), p.qin.data_ptr(), Hq, LM, Hq, 1,
                             G.data_ptr(), Hq, part_b.data_ptr(), part_wq.data_ptr(), part_bq.data_ptr(), rpb, None,
                             L.stream_ptr()))
    grads[fc.weight] = part_wq.sum(0)
    grads[fc.bias] = part_bq.sum(0)
    pb = part_b.sum(0)

    # ---- attention layers in reverse: gz = the gradient of segment li + 1 before its leaky_relu ----
    gz, gb = G[:, nl * hid:].contiguous(), pb[nl * hid:]
    rpb_l = 256
    for li in range(nl - 1, -1, -1):
        layer = model.att_layers[li]
        nh, dk, dv = layer.num_heads, layer.k_features, layer.v_features
        cat = _cat(layer)
        nqkv = cat.out_features
        fo = layer.fc_out
        core, qkv = p.core[li], p.qkv[li]
        sc = MD._gy_scale(gz)
        grads[fo.bias] = gb
        grads[fo.weight] = TS._wgrad(gz, sc, core, nh * dv, p.s_core[li])
        dcore = torch.empty(LM, nh * dv, device=dev)
        TS._dgrad(gz, hid, hid, sc, TS._lin_x3t(fo), LM, nh * dv, nh * dv, None, 0, dcore, nh * dv)
        # the attention core's transpose: [dv | dk | dq] as the columns of one buffer, like the forward's qkv
        dqkv = torch.empty(LM, nqkv, device=dev)
        qp, kp, vp = _qkv_ptrs(qkv, layer)
        dqp, dkp, dvp = _qkv_ptrs(dqkv, layer)
        tq = tk = ldt = rp = None
        if r is not None:
            tqkv = p.tar_qkv[li]
            tq, tk, _ = _qkv_ptrs(tqkv, p.model_tar.att_layers[li])
            ldt, rp = tqkv.stride(0), r.data_ptr()
        L.check(lib.gm_agent_attention_bwd(qp, kp, vp, nqkv, p.adj.data_ptr(), Ls * B, A, nh, dk, dv, dcore.data_ptr(),
                                           nh * dv, tq, tk, ldt or 0, rp, dqp, dkp, dvp, nqkv, L.stream_ptr()))
        # q, k, v are leaky outputs: derivative, bias partials and the operand scale in one pass
        g2 = torch.empty(LM, nqkv, device=dev)
        part = torch.empty((LM + rpb_l - 1) // rpb_l, nqkv, device=dev)
        sc2 = torch.empty(1, device=dev)
        L.check(lib.gm_leaky_bwd(dqkv.data_ptr(), qkv.data_ptr(), LM, nqkv, 0.01, g2.data_ptr(), part.data_ptr(), rpb_l,
                                 sc2.data_ptr(), L.stream_ptr()))
        gbc = part.sum(0)
        gw = TS._wgrad(g2, sc2, p.qin[:, li * hid:(li + 1) * hid], hid, p.s_x[li])
        o = 0
        for lin in (layer.fc_v, layer.fc_k, layer.fc_q):
            n = lin.out_features
            grads[lin.weight], grads[lin.bias] = gw[o:o + n], gbc[o:o + n]
            o += n
        # the layer input's gradient through [W_v; W_k; W_q] and segment li's leaky derivative, added to the head's part
        xb = p.bits[li]
        T = torch.empty(LM, hid, device=dev)
        partT = torch.empty((LM + 127) // 128, hid, device=dev)
        TS._dgrad(g2, nqkv, nqkv, sc2, TS._lin_x3t(cat), LM, hid, hid, xb, xb.stride(0), T, hid, part=partT)
        gz = T.add_(G[:, li * hid:(li + 1) * hid])
        gb = pb[li * hid:(li + 1) * hid] + partT.sum(0)

    # ---- encoder over all rows ----
    enc = list(model.encoder.linear_layers)
    g, sc = gz, MD._gy_scale(gz)
    grads[enc[-1].bias] = gb
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


class _DGNSeqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, *params):
        ctx.plan = plan
        with torch.no_grad():
            q, kl = _forward(plan)
        if kl is None:
            return q
        return q, kl

    @staticmethod
    def backward(ctx, dq, dkl=None):
        p = ctx.plan
        if dq is None:
            dq = torch.zeros(p.dims[-1], p.model.q_net.fc.out_features, device=p.qin.device)
        grads = _backward(p, dq, None if dkl is None else dkl.contiguous())
        ctx.plan = None
        return (None,) + tuple(grads.get(w) for w in p.params)


@torch.no_grad()
def _target(p, model_tar):
    """The target model on the stored next observations / next adjacency, all L steps' rows in one no-grad pass
    (DGN.forward_rows): max_a Q_target [L, B, A]; p.tar_qkv = its per-layer qkv rows (the regulariser reads the q
    and k columns: the target's attention weights on the NEXT observation, src/main.py:899-902, 924-954)."""
    sb = p.seq
    Ls, B, A, odp = sb.next_obs.shape
    od = sb.obs_dim
    LM = Ls * B * A
    X = AS._rows16(sb.next_obs.reshape(LM, odp), od)
    nadj = sb.next_adj.reshape(Ls * B, A, A)
    nadj = nadj if nadj.is_contiguous() else nadj.contiguous()
    bufs = {}
    q = model_tar.forward_rows(X, X.stride(0), od, MD._scratch_dict(bufs), adj=nadj, B=Ls * B, A=A)
    p.tar_qkv = [bufs[(("qkv", id(a)), LM, a.num_heads * (a.v_features + 2 * a.k_features))]
                 for a in model_tar.att_layers]
    return q.view(Ls, B, A, -1).max(dim=-1)[0]


def dgn_seq_loss(model, model_tar, seq, gamma, params, att_coeff=0.0, parts=None):
    """TD loss of src/main.py:840-1000 over a DGNSeqBatch, plus att_coeff times the attention regulariser when
    att_coeff > 0: (loss, q [L, B, A, nq], q_target)."""
    p = TS._Plan()
    p.model, p.model_tar, p.seq, p.params = model, model_tar, seq, list(params)
    p.reg = att_coeff > 0
    Ls, B, A = seq.action.shape
    if A > MAX_AGENTS:
        raise ValueError(f"dgn_seq_loss: at most {MAX_AGENTS} agents")
    nxt = _target(p, model_tar)
    out = _DGNSeqFn.apply(p, *p.params)
    q, kl = out if p.reg else (out, None)
    q = q.view(Ls, B, A, -1)
    target = seq.reward + (~seq.done) * gamma * nxt
    q_target = torch.scatter(q.detach(), -1, seq.action.unsqueeze(-1), target.unsqueeze(-1))
    loss_q = (q - q_target).pow(2).mean(dim=(1, 2, 3)).sum() / Ls
    loss, loss_att = loss_q, None
    if p.reg:  # train.attention_kl per step: the mean over the agents that are not done; steps averaged
        nd = ~seq.done
        loss_att = ((kl.view(Ls, B * A) * nd.view(Ls, B * A)).sum(1)
                    / torch.clamp(nd.view(Ls, B * A).sum(1), min=1)).sum() / Ls
        loss = loss_q + att_coeff * loss_att
    if parts is not None:
        parts.update(loss_q=loss_q, loss_att=loss_att, loss_aux=None)
    return loss, q, q_target


def dgn_update_seq(model, model_tar, optimizer, params, seq, gamma, tau, target_update_steps=0, iteration=1,
                   group=None, att_coeff=0.0, parts=None):
    """One update (src/main.py:840-1026) on a DGNSeqBatch: the batched loss and backward, the gradient all-reduce
    across ranks, clip by value (0.5) and norm (1.0), AdamW, target update."""
    from .train import allreduce_gradients, interpolate_model

    loss, q, qt = dgn_seq_loss(model, model_tar, seq, gamma, params, att_coeff, parts)
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
