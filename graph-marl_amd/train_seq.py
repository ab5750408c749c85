"""Sequence-batched DQN + NetMon update (reference src/main.py:840-1026 on replay sequences,
src/replaybuffer.py:103-130) with a hand-written backward.

The reference runs, per step t of a sampled sequence of L consecutive transitions, NetMon on
the stored node observations (state carried from the stored start state, reset at episode
ends), the DQN on [env obs | NetMon readout], the target DQN on the next observation, and
backpropagates the summed TD loss through all of it with autograd. Here the same computation
is one autograd node over the whole sequence (`_SeqFn`), organised for the GPU:

  * everything without recurrence runs ONCE over all L steps' rows: the NetMon encoder MLP
    (L*B*N rows), the readout, the DQN (L*B*A rows), their weight gradients, and the target
    DQN of steps 0..L-2 (whose next observations are the online ones of steps 1..L-1);
  * only the LSTM cells and the aggregate run per step (forward: one [x | h] GEMM per cell with
    the gate math in its epilogue; backward: gm_lstm_cell_bwd, which sums every gradient source
    of the cell — readout, the next cell's input gradient, the transposed aggregate, the next
    step's state gradient masked at episode ends — and one input-gradient GEMM per cell);
  * GRU cells (--netmon-rnn-type gru) take the same route on the four-tile weight W4 of
    fused.pack_gru in natural row order: forward one GM_EPI_BIAS GEMM giving [a_r | a_z | a_nx |
    a_nh], then gm_gru_cell_fwd (h', and G = [r | z | n | a_nh] saved in place); backward
    gm_gru_cell_bwd and one input-gradient GEMM on W4^T giving [dx | dh_w]. The state rows are H
    wide, and a cell's h gradient arrives in two parts (dh_w through W4 and the direct g z), which
    the previous cell's call sums as two sources; the W4 weight gradient is mapped back to torch's
    weight_ih / weight_hh / bias layout (gru_param_grads);
  * LayerNorm-LSTM cells (--netmon-rnn-type lnlstm, H <= 512) keep [h | c] state rows; per cell two no-bias GEMMs
    (x W_ih^T, h W_hh^T) into saved raw products + gm_lnlstm_fwd (row statistics saved); the obs cell's x W_ih^T has
    no recurrence and runs as ONE GEMM over all L steps' rows. Backward: gm_lnlstm_cell_bwd (sums the sources,
    recomputes the activations, publishes the scales of dgi and dgh apart) and the input-gradient GEMMs dgh @ W_hh
    and dgi @ W_ih, the obs cell's dgi @ W_ih once over all steps after the loop (_lnlstm_cells_bwd);
  * the leaky_relu derivative, the bias-gradient column sums and the gradient scales are fused
    into the kernels that produce the gradients (gm_gemm_x3_dgrad, gm_qhead_bwd,
    gm_lstm_cell_bwd / gm_gru_cell_bwd / gm_lnlstm_cell_bwd), so no activation gradient is re-read for them.

Every GEMM runs in the split-f16 form with fp32 accumulation (gm_gemm_x3 / gm_gemm_x3_wgrad),
as in the autograd path (train.dqn_loss), which remains the path for every other configuration
(no carry-over, an aux head aux_ok refuses, GM_GEMM=f32; DQNR / CommNet without NetMon: agent_seq.py, with NetMon:
agent_netmon_seq.py; DGN without NetMon: dgn_seq.py; DGN with NetMon: dgn_netmon_seq.py, which runs the NetMon half of this
module, _forward_netmon / _backward_netmon, around the DGN half of dgn_seq.py).

Aux loss (--aux-loss-coeff, src/main.py:586-594, 868-875, 996-1000; seq_loss(aux_model=...)): the head MLP(S, [S,
n_aux]) runs once over S[K] of all L steps viewed as [L*B*N, S] (the state after each step, before the episode mask)
against SeqBatch.node_aux, and the node returns loss_aux = sum res^2 / (L*B*N*n_aux) as a second output (_forward_aux).
Layer 1 is a batched leaky GEMM with sign bits like the encoder's; layer 2, the residual and the squared sum are
gm_aux_head_mse in fp32 (no GEMM tile is n_aux = 20 columns wide, and the layer's output would be written and read
back). Backward (_backward_aux): gm_aux_head_mse_bwd gives layer 1's output gradient (leaky mask, 2 * upstream /
(L*B*N*n_aux) folded in), both bias partials and the gradient's scale; W2's gradient res^T y is _wgrad on the two
operand scales the forward kernel published; layer 1's input gradient [dh_aux | dc_aux] is one _dgrad split at H: dh_aux
is added onto dh_final before the cell loop, dc_aux[t] is the dc source of step t's last update cell (gm_lstm_bwd_args.dc
/ gm_lnlstm_cell_bwd_args.dc, unused at j == K otherwise; gru has no c). Without an aux model nothing of this is
launched or allocated.

Global readout (NetMon output_global_hidden, --netmon-global; graph observation [h | global | nbr x 3] with
global = the mean of h over the graph's nodes, src/model.py:458-469): the readout buffer is [L*B*A, 5H] =
[h | nbr x 3 | global]; gm_netmon_readout_ld writes the first 4H columns (ld 5H), gm_netmon_global_rows the last H
from S[K] of all L*B graphs in one launch, and the first DQN layer's weight columns are packed in that order
(_dqn_first_x3; its gradient is mapped back to the reference order). Backward: the layer's input gradient is 5H
wide; gm_netmon_global_bwd adds the mean's transpose onto dh_final once over all steps, right after
gm_netmon_readout_bwd, so the cells' backward is the same. The target pass reads the same 5H rows for steps
0..L-2 and takes the rollout's global path (train._fused_next_q) for its own NetMon steps.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib as L
from . import fused as FU
from . import model as MD

SeqBatch = namedtuple("SeqBatch", ["obs", "obs_dim", "action", "reward", "done", "episode_done", "node_obs", "nbr",
                                   "agent_node", "node_state", "next_fields", "idx", "node_aux"],
                      defaults=(None, None))
"""All L steps of B replay sequences, stacked: obs [L, B, A, odp] (rows padded to 16 bytes, first
obs_dim columns valid), action [L, B, A] long, reward [L, B, A], done [L, B, A] bool, episode_done
[L, B] bool, node_obs [L, B, N, F], nbr [L, B, N, deg] int32, agent_node [L, B, A] int32,
node_state [B, N, state_size] (the NetMon state before step 0: [h | c], gru: h). next_fields(t, rows) -> (next_obs
[len, A, odp], next_node_obs [len, N, F], next_agent_node [len, A] int32) of step t for the
sequences `rows` (None = all). node_aux [L, B, N, n_aux] (the aux head's targets) when the ring stores them."""


def cell_ok(netmon):
    """lstm, gru at a hidden size gm_gru_cell_bwd takes (H <= 256 dividing 256, or a multiple of 64), or lnlstm at
    one gm_lnlstm_cell_bwd takes (H <= 512)."""
    H = netmon.hidden_features
    return (netmon.rnn_type == "lstm" or (netmon.rnn_type == "gru" and (256 % H == 0 or H % 64 == 0))
            or (netmon.rnn_type == "lnlstm" and H <= 512))


def netmon_seq_ok(netmon):
    """The NetMon half's conditions (shared with dgn_netmon_seq.py): a cell cell_ok takes, carry-over, the neighbour
    readout, K >= 1, H % 32 == 0, a leaky encoder with biases."""
    H = netmon.hidden_features
    enc = list(netmon.encode.linear_layers)
    return (cell_ok(netmon) and netmon.rnn_carryover and netmon.output_neighbor_hidden
            and netmon.iterations >= 1 and H % 32 == 0 and H <= 1024
            and all(l.act == 1 and l.bias is not None for l in enc))


def aux_ok(netmon, aux_model):
    """The aux head _forward_aux takes (main.py's MLP(S, [S, n_aux], activation_on_output=False) on the NetMon state
    row of S floats): exactly two Linear layers with biases, the first leaky and S -> S, the second without
    activation, S <= 1024 and n_aux <= 128 (gm_aux_head_mse)."""
    ll = list(getattr(aux_model, "linear_layers", []))
    S = netmon.state_size
    return (type(aux_model) is MD.MLP and len(ll) == 2 and all(l.bias is not None for l in ll)
            and ll[0].act == 1 and ll[1].act == 0 and ll[0].in_features == S and ll[0].out_features == S
            and ll[1].in_features == S and S <= 1024 and S % 32 == 0 and 1 <= ll[1].out_features <= 128)


def seq_ok(netmon, model, model_tar, att_coeff=0.0, aux_model=None):
    """The sequence-batched path covers the reference's NetMon + DQN configuration: LSTM, GRU or LayerNorm-LSTM
    cells with carry-over, sum / mean aggregation, neighbour readout (with or without the global mean), leaky MLPs,
    split-f16 GEMMs, with or without the aux loss on a head aux_ok takes."""
    if netmon is None or att_coeff != 0 or L.GEMM_MODE != "x3":
        return False
    if aux_model is not None and not aux_ok(netmon, aux_model):
        return False
    if type(model) is not MD.DQN or type(model_tar) is not MD.DQN:
        return False
    dq = list(model.encoder.linear_layers)
    fc = model.q_net.fc
    return (netmon_seq_ok(netmon) and all(l.act == 1 for l in dq) and fc.act == 0
            and fc.out_features <= 4 and all(l.bias is not None for l in dq + [fc])
            and dq[-1].out_features <= 1024)


def _zeros1(dev):
    return torch.zeros(1, device=dev)


def _finish(slot):
    L.check(FU._setup().gm_absmax_finish(slot.data_ptr(), L.stream_ptr()))
    return slot


class _X3Cache:
    """Split-f16 packs a module's training GEMMs need, refreshed when a parameter changes."""

    def __init__(self):
        self.p = {}

    def get(self, name, key, fn):
        k, v = self.p.get(name, (None, None))
        if k != key:
            v = fn()
            self.p[name] = (key, v)
        return v


def _cache(mod):
    if not hasattr(mod, "_seq_x3"):
        mod._seq_x3 = _X3Cache()
    return mod._seq_x3


def _x3(w):
    """X3 of an [n][k] weight (any n: the narrow tiles too)."""
    wp, ldw = FU._pad_cols(w.detach())
    return FU.X3(wp, ldw, w.shape[0], w.shape[1])


def _lin_x3(lin):
    return _cache(lin).get("fwd", FU._key(lin.weight), lambda: _x3(lin.weight))


def _lin_x3t(lin, cols=None):
    """X3 of W^T (or of W[:, cols]^T) for the input gradient gx = g @ W."""
    def build():
        w = lin.weight.detach() if cols is None else lin.weight.detach()[:, cols]
        return _x3(w.t().contiguous())
    return _cache(lin).get(("t", None if cols is None else (cols.start, cols.stop)), FU._key(lin.weight), build)


def _dqn_first_x3(lin, od, global_h=None):
    """First DQN layer with columns reordered to [graph | env obs] (the GEMM's two sources); global_h = H (global
    readout): [h | nbr x 3 | global | env obs] (FU.global_first_cols)."""
    def build():
        with torch.no_grad():
            if global_h is not None:
                return _x3(FU.global_first_cols(lin.weight, od, global_h, "global_env"))
            w = torch.cat([lin.weight[:, od:], lin.weight[:, :od]], 1)
            return _x3(w)
    return _cache(lin).get(("first", od, global_h), FU._key(lin.weight), build)


def _dqn_first_x3t(lin, od, H, glob):
    """X3 of W[:, graph columns]^T for the first DQN layer's graph-input gradient, the columns in the readout
    buffer's order ([h | nbr x 3], with the global readout [h | nbr x 3 | global])."""
    if not glob:
        return _lin_x3t(lin, slice(od, od + 4 * H))

    def build():
        w = FU.global_first_cols(lin.weight.detach(), od, H, "global_env")[:, :5 * H]
        return _x3(w.t().contiguous())
    return _cache(lin).get(("t_global", od, H), FU._key(lin.weight), build)


def _lstm_x3t(cell):
    """X3 of [W_ih | W_hh]^T ([2H][4H], natural gate order) for d[x | h] = dgates @ [W_ih | W_hh]."""
    def build():
        w = torch.cat([cell.weight_ih.detach(), cell.weight_hh.detach()], 1)
        return _x3(w.t().contiguous())
    return _cache(cell).get("t", FU._key(cell.weight_ih, cell.weight_hh), build)


def _lstm_fwd(cell):
    """Interleaved gate-tile pack of the cell (fused.pack_lstm) with its split-f16 form forced."""
    wp, ldw, bp, x3 = FU.pack_lstm(cell)
    if x3 is None:
        x3 = _cache(cell).get("fwdx3", FU._key(cell.weight_ih, cell.weight_hh), lambda: FU.X3(wp, ldw, wp.shape[0],
                                                                                                2 * cell.hidden_size))
    return wp, ldw, bp, x3


def _gru_w4(cell):
    """The four-tile weight of fused.pack_gru in natural row order: W4 [4H][2H] on A = [x | h] with row blocks r, z:
    [W_i | W_h], n_x: [W_in | 0], n_h: [0 | W_hn], and its biases [b_ir + b_hr | b_iz + b_hz | b_in | b_hn]."""
    H = cell.hidden_size
    wi, wh, bi, bh = (t.detach() for t in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh))
    z = torch.zeros(H, H, device=wi.device)
    w = torch.cat([torch.cat([wi[:2 * H], wh[:2 * H]], 1), torch.cat([wi[2 * H:], z], 1),
                   torch.cat([z, wh[2 * H:]], 1)], 0)
    return w, torch.cat([bi[:2 * H] + bh[:2 * H], bi[2 * H:], bh[2 * H:]])


def _gru_fwd(cell):
    """(b4, X3 of W4) for the cell's one GM_EPI_BIAS GEMM: P = [x | h] W4^T + b4 = [a_r | a_z | a_nx | a_nh]."""
    def build():
        w, b = _gru_w4(cell)
        return b.contiguous(), _x3(w)
    return _cache(cell).get("gru_fwd", FU._key(cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), build)


def _gru_x3t(cell):
    """X3 of W4^T ([2H][4H], natural order) for d[x | h] = dgates @ W4."""
    return _cache(cell).get("gru_t", FU._key(cell.weight_ih, cell.weight_hh),
                            lambda: _x3(_gru_w4(cell)[0].t().contiguous()))


def gru_cell_fwd(x, h, ldh, b4, x3, M, H, slot, G, out, ldo):
    """One GRU cell: G [M][4H] = [x | h] W4^T + b4 (max |A| into slot), then gm_gru_cell_fwd: out = h' (strided
    rows), G overwritten with [r | z | n | a_nh] for gm_gru_cell_bwd."""
    FU.gemm(FU.dense(_ptr(x), H, H, amax=slot.data_ptr()), FU.dense(_ptr(h), ldh, H), None, 0, b4.data_ptr(), M,
            4 * H, FU.GM_EPI_BIAS, _ptr(G), 4 * H, x3=x3)
    L.check(L.lib().gm_gru_cell_fwd(_ptr(G), 4 * H, _ptr(h), ldh, M, H, _ptr(out), ldo, L.stream_ptr()))


def gru_param_grads(cell, grads, gx, gh, bg):
    """torch's GRUCell parameter layout from the W4 gradients: gx / gh [4H][H] = the x and h column halves of
    dW4 (row blocks r, z, n_x, n_h; gx's n_h block and gh's n_x block belong to W4's zeros), bg [4H] the column
    sums of the gate gradients (da_r, da_z, da_nx, da_nh)."""
    H = cell.hidden_size
    grads[cell.weight_ih] = gx[:3 * H]
    grads[cell.weight_hh] = torch.cat([gh[:2 * H], gh[3 * H:]], 0)
    grads[cell.bias_ih] = bg[:3 * H]
    grads[cell.bias_hh] = torch.cat([bg[:2 * H], bg[3 * H:]])


def _lnl_x3t(cell):
    """(X3 of W_ih^T [I][4H], X3 of W_hh^T [H][4H]) of a LayerNormLSTMCell for dx = dgi @ W_ih, dh = dgh @ W_hh."""
    return _cache(cell).get("lnl_t", FU._key(cell.weight_ih, cell.weight_hh),
                            lambda: (_x3(cell.weight_ih.detach().t().contiguous()),
                                     _x3(cell.weight_hh.detach().t().contiguous())))


def lnl_gemm(x, ldx, cell, hh, M, H, slot, G, ldg):
    """Raw gate product of a LayerNormLSTMCell, no bias: G [M][4H] (row stride ldg) = x[:, :H] W_hh^T (hh) or
    x W_ih^T, max |x| into slot."""
    wp, ldw, x3 = FU.pack_lnlstm(cell)[1 if hh else 0]
    FU.gemm(FU.dense(_ptr(x), ldx, H, amax=slot.data_ptr()), None, wp.data_ptr(), ldw, None, M, 4 * H, FU.GM_EPI_BIAS,
            _ptr(G), ldg, x3=x3)


def lnl_cell_fwd(cell, gi, ldgi, gh, ldgh, s_in, out, M, H, stats):
    """gm_lnlstm_fwd on the raw products gi, gh and the c half of the [h | c] rows s_in: [h' | c'] into the rows
    out (both 2H wide), the row statistics into stats [M][8]."""
    li, lh, lc = cell.ln_input, cell.ln_hidden, cell.ln_cell
    L.check(L.lib().gm_lnlstm_fwd(_ptr(gi), ldgi, _ptr(gh), ldgh, _ptr(s_in) + 4 * H, 2 * H, li.weight.data_ptr(),
                                  li.bias.data_ptr(), lh.weight.data_ptr(), lh.bias.data_ptr(), cell.bias_ih.data_ptr(),
                                  lc.weight.data_ptr(), lc.bias.data_ptr(), M, H, float(li.eps), _ptr(out), 2 * H,
                                  _ptr(out) + 4 * H, 2 * H, stats.data_ptr(), L.stream_ptr()))


LNL_RPW = 16  # rows per wave of gm_lnlstm_cell_bwd: one 14H partial row per 16 cell rows


def lnl_bwd_args(cell, gi, ldgi, gh, ldgh, s_in, stats, M, H):
    """gm_lnlstm_cell_bwd_args with the cell's saved forward operands filled in."""
    li, lh, lc = cell.ln_input, cell.ln_hidden, cell.ln_cell
    a = L.LNLSTMBwdArgs()
    a.gi, a.ld_gi, a.gh, a.ld_gh = _ptr(gi), ldgi, _ptr(gh), ldgh
    a.c_in, a.ld_cin = _ptr(s_in) + 4 * H, 2 * H
    a.ln_in_w, a.ln_in_b, a.ln_hid_w, a.ln_hid_b = (t.data_ptr() for t in (li.weight, li.bias, lh.weight, lh.bias))
    a.bias, a.ln_cell_w, a.ln_cell_b = cell.bias_ih.data_ptr(), lc.weight.data_ptr(), lc.bias.data_ptr()
    a.eps, a.stats = float(li.eps), stats.data_ptr()
    a.m, a.hidden, a.rows_per_wave = M, H, LNL_RPW
    return a


def lnl_param_grads(cell, grads, gwi, gwh, ps):
    """The cell's parameter gradients from the two weight gradients and the summed 14H partials ps = [d ln_input.w |
    d ln_hidden.w | d bias | d ln_cell.w | d ln_cell.b]; d ln_input.bias = d ln_hidden.bias = d bias_ih as separate
    tensors (each may become a .grad modified in place)."""
    H4 = 4 * cell.hidden_size
    H = cell.hidden_size
    grads[cell.weight_ih], grads[cell.weight_hh] = gwi, gwh
    grads[cell.ln_input.weight], grads[cell.ln_hidden.weight] = ps[:H4], ps[H4:2 * H4]
    db = ps[2 * H4:3 * H4]
    grads[cell.bias_ih], grads[cell.ln_input.bias], grads[cell.ln_hidden.bias] = db, db.clone(), db.clone()
    grads[cell.ln_cell.weight], grads[cell.ln_cell.bias] = ps[3 * H4:3 * H4 + H], ps[3 * H4 + H:]


def _ptr(t):
    return t if isinstance(t, int) else t.data_ptr()


def _sign_bits(rows, n, dev):
    """uint32 sign words of an activation (bit c % 32 of word c / 32: value > 0), int32 storage."""
    return torch.empty(rows, (n + 31) // 32, dtype=torch.int32, device=dev)


def _gemm_amax(x, ldx, k, x3, b, m, n, epi, y, ldy, slot, a1=None, sbits=None):
    """y = epi([x | a1] @ W^T + b) in split-f16 form, max |A| published into slot; a1 = (tensor, ld,
    k1) or None; sbits (optional) receives y's sign bits."""
    src1 = None if a1 is None else FU.dense(_ptr(a1[0]), a1[1], a1[2])
    FU.gemm(FU.dense(_ptr(x), ldx, k, amax=slot.data_ptr()), src1, None, 0, None if b is None else b.data_ptr(), m,
            n, epi, _ptr(y), ldy, ldc=0 if sbits is None else sbits.stride(0),
            act_out=None if sbits is None else sbits.data_ptr(), x3=x3)


def _dgrad(g, ldg, k, sc, x3t, m, n, split, mask, ldm, y, ldy, y2=None, ldy2=0, part=None, gmax=None):
    """gm_gemm_x3_dgrad (part rows = 128-row tiles); mask = the layer input's sign bits (int32 words,
    ldm words per row) or None."""
    a = FU.dense(_ptr(g), ldg, k, scale=sc.data_ptr())
    L.check(FU._setup().gm_gemm_x3_dgrad(C.byref(a), x3t.wp.data_ptr(), x3t.sinv.data_ptr(), m, n, split,
                                         None if mask is None else _ptr(mask), ldm, _ptr(y), ldy,
                                         None if y2 is None else _ptr(y2), ldy2, None if part is None else part.data_ptr(),
                                         None if gmax is None else gmax.data_ptr(), L.stream_ptr()))


class _Plan:
    """Inputs, modules and the forward's saved tensors of one sequence update."""
    pass


def _forward_netmon(p):
    """The NetMon half of the forward (p.netmon on p.seq), up to and including the readout buffer: returns p.R
    [L*B*A, GW] = [h | nbr x 3] (global readout: [h | nbr x 3 | global]); sets p.dims, p.env (the env obs rows) and
    the tensors _backward_netmon reads."""
    netmon = p.netmon
    sb = p.seq
    dev = sb.obs.device
    Ls, B, A, odp = sb.obs.shape
    N, F = sb.node_obs.shape[2], sb.node_obs.shape[3]
    od = sb.obs_dim
    H = netmon.hidden_features
    gru = netmon.rnn_type == "gru"
    S2 = H if gru else 2 * H  # state row: h, or [h | c]
    K = netmon.iterations
    M, Ma = B * N, B * A
    LM, LMa = Ls * M, Ls * Ma
    p.dims = (Ls, B, A, N, F, od, odp, H, K, M, Ma)
    mean = int(netmon.agg_mode == 1)
    X = sb.node_obs.reshape(LM, F)
    if X.stride(0) % 4 or X.data_ptr() % 16:
        Xp = torch.zeros(LM, (F + 3) // 4 * 4, device=dev)
        Xp[:, :F] = X
        X = Xp
    nbr = sb.nbr.reshape(Ls * B, N, -1).contiguous()
    an = sb.agent_node.reshape(Ls * B, A).contiguous()
    p.nbr, p.an = nbr, an
    deg = nbr.shape[-1]

    # ---- NetMon encoder over all steps ----
    enc = list(netmon.encode.linear_layers)
    p.enc_in, p.enc_out, p.enc_bits = [], [], []
    x, ldx, kx = X, X.stride(0), F
    for i, lin in enumerate(enc):
        n = lin.out_features
        y = torch.empty(LM, n, device=dev)
        yb = _sign_bits(LM, n, dev)  # the leaky mask of this output for the backward
        if i == 0 and FU.routing_encoder_ok(lin, N, F, nbr):
            FU.routing_encoder(lin, X, nbr, Ls * B, N, y, sbits=yb)
            sx = torch.empty(1, device=dev)
            L.check(FU._setup().gm_absmax_scale_rows(X.data_ptr(), LM, F, X.stride(0), sx.data_ptr(), L.stream_ptr()))
        else:
            sx = _zeros1(dev)
            _gemm_amax(x, ldx, kx, _lin_x3(lin), lin.bias, LM, n, FU.GM_EPI_BIAS_LEAKY, y, n, sx, sbits=yb)
            _finish(sx)
        p.enc_in.append((x, ldx, kx, sx))
        p.enc_out.append(y)
        p.enc_bits.append(yb)
        x, ldx, kx = y, n, n
    E = p.enc_out[-1]  # [LM][H], the obs cell's x

    # ---- recurrent cells, per step ----
    S_in = torch.empty(Ls, M, S2, device=dev)
    S = torch.empty(K + 1, Ls, M, S2, device=dev)  # cell outputs [h | c] (gru: h): j = 0 obs, 1..K update
    lnl = netmon.rnn_type == "lnlstm"
    # gate activations (gru: G = [r | z | n | a_nh]); lnlstm keeps the raw gate products instead
    act = None if lnl else torch.empty(K + 1, Ls, M, 4 * H, device=dev)
    agg = torch.empty(K, Ls, M, H, device=dev)
    s_obs, s_upd = _zeros1(dev), _zeros1(dev)
    keep = (~sb.episode_done).to(torch.float32)  # [L, B]
    S_in[0].copy_(sb.node_state.reshape(M, S2))
    lib = L.lib()
    if lnl:
        # raw gate products: the obs cell's gi = E W_ih^T has no recurrence (its LayerNorm sees it alone), so ONE
        # GEMM over all L steps' rows; gh and the update cell's [gi | gh] per step
        co, cu = netmon.rnn_obs, netmon.rnn_update
        p.gi_obs = torch.empty(Ls, M, 4 * H, device=dev)
        p.gh_obs = torch.empty(Ls, M, 4 * H, device=dev)
        p.g_upd = torch.empty(K, Ls, M, 8 * H, device=dev)
        p.stats = torch.empty(K + 1, Ls, M, 8, device=dev)
        p.sh_obs, p.sh_upd = _zeros1(dev), _zeros1(dev)  # max |h| of the two cells' h operands
        lnl_gemm(E, H, co, False, LM, H, s_obs, p.gi_obs, 4 * H)
        for t in range(Ls):
            if t > 0:
                torch.mul(S[K, t - 1].view(B, N * S2), keep[t - 1].view(B, 1), out=S_in[t].view(B, N * S2))
            lnl_gemm(S_in[t], S2, co, True, M, H, p.sh_obs, p.gh_obs[t], 4 * H)
            lnl_cell_fwd(co, p.gi_obs[t], 4 * H, p.gh_obs[t], 4 * H, S_in[t], S[0, t], M, H, p.stats[0, t])
            for j in range(1, K + 1):
                prev, G = S[j - 1, t], p.g_upd[j - 1, t]
                L.check(lib.gm_mp_aggregate_rows(prev.data_ptr(), S2, nbr[t * B:(t + 1) * B].data_ptr(), B, N, deg,
                                                 H, mean, agg[j - 1, t].data_ptr(), H, L.stream_ptr()))
                lnl_gemm(agg[j - 1, t], H, cu, False, M, H, s_upd, G, 8 * H)
                lnl_gemm(prev, S2, cu, True, M, H, p.sh_upd, G.data_ptr() + 16 * H, 8 * H)
                lnl_cell_fwd(cu, G, 8 * H, G.data_ptr() + 16 * H, 8 * H, prev, S[j, t], M, H, p.stats[j, t])
        _finish(p.sh_obs)
        _finish(p.sh_upd)
    elif gru:
        wo, wu = _gru_fwd(netmon.rnn_obs), _gru_fwd(netmon.rnn_update)
        for t in range(Ls):
            if t > 0:
                torch.mul(S[K, t - 1].view(B, N * H), keep[t - 1].view(B, 1), out=S_in[t].view(B, N * H))
            for j in range(K + 1):
                if j == 0:
                    gru_cell_fwd(E[t * M:(t + 1) * M], S_in[t], H, *wo, M, H, s_obs, act[0, t], S[0, t], H)
                else:
                    prev = S[j - 1, t]
                    L.check(lib.gm_mp_aggregate_rows(prev.data_ptr(), H, nbr[t * B:(t + 1) * B].data_ptr(), B, N, deg,
                                                     H, mean, agg[j - 1, t].data_ptr(), H, L.stream_ptr()))
                    gru_cell_fwd(agg[j - 1, t], prev, H, *wu, M, H, s_upd, act[j, t], S[j, t], H)
    else:
        wo = _lstm_fwd(netmon.rnn_obs)
        wu = _lstm_fwd(netmon.rnn_update)
        for t in range(Ls):
            if t > 0:  # the state carried from step t-1, zeroed at its episode end (src/main.py:858-866)
                torch.mul(S[K, t - 1].view(B, N * S2), keep[t - 1].view(B, 1), out=S_in[t].view(B, N * S2))
            src, sh = E[t * M:(t + 1) * M], S_in[t]
            for j in range(K + 1):
                wp, ldw, bp, x3 = wo if j == 0 else wu
                if j == 0:
                    xa, hsrc = FU.dense(src.data_ptr(), H, H, amax=s_obs.data_ptr()), sh
                else:
                    prev = S[j - 1, t]
                    L.check(lib.gm_mp_aggregate_rows(prev.data_ptr(), S2, nbr[t * B:(t + 1) * B].data_ptr(), B, N, deg,
                                                     H, mean, agg[j - 1, t].data_ptr(), H, L.stream_ptr()))
                    xa, hsrc = FU.dense(agg[j - 1, t].data_ptr(), H, H, amax=s_upd.data_ptr()), prev
                out = S[j, t]
                FU.gemm(xa, FU.dense(hsrc.data_ptr(), S2, H), wp.data_ptr(), ldw, bp.data_ptr(), M, 4 * H,
                        FU.GM_EPI_LSTM, out.data_ptr(), S2, out.data_ptr() + 4 * H, S2, hsrc.data_ptr() + 4 * H, S2,
                        act[j, t].data_ptr(), x3=x3)
    _finish(s_obs)
    _finish(s_upd)
    p.S_in, p.S, p.act, p.agg, p.s_obs, p.s_upd = S_in, S, act, agg, s_obs, s_upd

    # ---- readout over all steps ----
    glob = netmon.output_global_hidden
    GW = (5 if glob else 4) * H  # readout row: [h | nbr x 3], global readout: [h | nbr x 3 | global]
    p.glob, p.GW = glob, GW
    R = torch.empty(LMa, GW, device=dev)
    hp = S[K - 1] if K >= 1 else torch.zeros_like(S[K])
    L.check(lib.gm_netmon_readout_ld(S[K].data_ptr(), S2, hp.data_ptr(), S2, nbr.data_ptr(), an.data_ptr(), Ls * B, N,
                                     A, deg, H, R.data_ptr(), GW, L.stream_ptr()))
    if glob:
        FU.global_rows(S[K].data_ptr(), S2, Ls * B, N, H, A, R.data_ptr() + 16 * H, GW)
    p.R = R
    p.env = sb.obs.reshape(LMa, odp)
    return R


def _forward(p):
    R = _forward_netmon(p)
    dqn = p.dqn
    Ls, B, A, N, F, od, odp, H, K, M, Ma = p.dims
    LMa = Ls * Ma
    dev = R.device
    glob, GW, env = p.glob, p.GW, p.env

    # ---- DQN over all steps ----
    dl = list(dqn.encoder.linear_layers)
    fc = dqn.q_net.fc
    nq = fc.out_features
    p.d, p.d_in_scale, p.d_bits = [], [], []
    q = torch.empty(LMa, nq, device=dev)
    for i, lin in enumerate(dl):
        n = lin.out_features
        y = torch.empty(LMa, n, device=dev)
        sx = _zeros1(dev)
        last = i == len(dl) - 1
        yb = None if last else _sign_bits(LMa, n, dev)
        p.d_bits.append(yb)
        if i == 0:
            _gemm_amax(R, GW, GW, _dqn_first_x3(lin, od, H if glob else None), lin.bias, LMa, n,
                       FU.GM_EPI_BIAS_LEAKY, y, n, sx, a1=(env, odp, od), sbits=yb)
            if last:
                torch.addmm(fc.bias.detach(), y, fc.weight.detach().t(), out=q)
        elif last and n <= 256:  # last hidden layer + Q head in one kernel (hidden output written too)
            prev = p.d[-1]
            kp = prev.shape[1]
            x3 = _lin_x3(lin)
            wq = fc.weight.detach().contiguous()
            L.check(FU._setup().gm_gemm_x3_head(
                C.byref(FU.dense(prev.data_ptr(), kp, kp, amax=sx.data_ptr())), x3.wp.data_ptr(), x3.sinv.data_ptr(),
                lin.bias.data_ptr(), LMa, n, 1, wq.data_ptr(), wq.stride(0), fc.bias.data_ptr(), nq, q.data_ptr(), nq,
                y.data_ptr(), n, L.stream_ptr()))
        else:
            prev = p.d[-1]
            _gemm_amax(prev, prev.shape[1], prev.shape[1], _lin_x3(lin), lin.bias, LMa, n, FU.GM_EPI_BIAS_LEAKY, y, n,
                       sx, sbits=yb)
            if last:
                torch.addmm(fc.bias.detach(), y, fc.weight.detach().t(), out=q)
        p.d.append(y)
        p.d_in_scale.append(_finish(sx))
    return q


def _wgrad(g, sa, x, k, sb_):
    """dW = g^T x[:, :k] (split-K split-f16 kernel; both operand scales given)."""
    return MD._wgrad(g, x, k, sa, sb_)


AUX_RPB = 64  # rows per block of gm_aux_head_mse / gm_aux_head_mse_bwd


def _forward_aux(p):
    """The NetMon aux loss (src/main.py:586-594, 868-875) after _forward_netmon: the head p.aux once over S[K] of all
    steps viewed as [L*B*N, S] (the state after each step, before the episode mask) against seq.node_aux. Layer 1
    is a batched leaky GEMM like the encoder's; layer 2, the residual and the squared sum are gm_aux_head_mse.
    Returns sum res^2 / (L*B*N*n_aux) = the reference's sum_t mean_t / L (every step has the same row count)."""
    Ls, B, A, N, F, od, odp, H, K, M, Ma = p.dims
    l1, l2 = p.aux.linear_layers
    SK = p.S[K]
    S2 = SK.shape[-1]
    LM = Ls * M
    dev = SK.device
    na = l2.out_features
    tgt = p.seq.node_aux.reshape(LM, na).to(torch.float32).contiguous()
    y = torch.empty(LM, S2, device=dev)
    yb = _sign_bits(LM, S2, dev)
    sx = _zeros1(dev)
    _gemm_amax(SK, S2, S2, _lin_x3(l1), l1.bias, LM, S2, FU.GM_EPI_BIAS_LEAKY, y, S2, sx, sbits=yb)
    _finish(sx)
    res = torch.empty(LM, na, device=dev)
    part = torch.empty((LM + AUX_RPB - 1) // AUX_RPB, device=dev)
    sr, sy = _zeros1(dev), _zeros1(dev)  # max |res|, max |y|: the operand scales of W2's gradient GEMM
    w2 = l2.weight.detach()
    L.check(L.lib().gm_aux_head_mse(y.data_ptr(), S2, LM, S2, w2.data_ptr(), w2.stride(0), l2.bias.data_ptr(), na,
                                    tgt.data_ptr(), na, res.data_ptr(), na, part.data_ptr(), AUX_RPB, sr.data_ptr(),
                                    sy.data_ptr(), L.stream_ptr()))
    p.aux_saved = (y, yb, sx, res, _finish(sr), _finish(sy))
    return part.sum() / (LM * na)


def _backward_aux(p, daux, grads):
    """Backward of _forward_aux from daux, the upstream gradient of its loss (it carries aux_coeff): the head's
    parameter gradients into grads; returns the gradient of S[K] of all steps as (dh_aux [L*B*N, H], dc_aux (the
    same shape; gru: None)), layer 1's input gradient in one GEMM split at H."""
    Ls, B, A, N, F, od, odp, H, K, M, Ma = p.dims
    l1, l2 = p.aux.linear_layers
    y, yb, sx, res, sr, sy = p.aux_saved
    LM, S2 = y.shape
    na = l2.out_features
    dev = y.device
    nb = (LM + AUX_RPB - 1) // AUX_RPB
    g = torch.empty(LM, S2, device=dev)
    pb1, pb2 = torch.empty(nb, S2, device=dev), torch.empty(nb, na, device=dev)
    sc = torch.empty(1, device=dev)
    up = daux.detach().reshape(1).to(torch.float32).contiguous()
    scale = 2.0 / (LM * na)
    w2 = l2.weight.detach()
    L.check(L.lib().gm_aux_head_mse_bwd(res.data_ptr(), na, na, w2.data_ptr(), w2.stride(0), yb.data_ptr(),
                                        yb.stride(0), 1, LM, S2, scale, up.data_ptr(), g.data_ptr(), S2,
                                        pb1.data_ptr(), pb2.data_ptr(), AUX_RPB, sc.data_ptr(), L.stream_ptr()))
    grads[l2.weight] = _wgrad(res, sr, y, S2, sy) * (up * scale)
    grads[l2.bias] = pb2.sum(0)
    grads[l1.bias] = pb1.sum(0)
    grads[l1.weight] = _wgrad(g, sc, p.S[K].view(LM, S2), S2, sx)
    dh = torch.empty(LM, H, device=dev)
    dc = torch.empty(LM, H, device=dev) if S2 > H else None
    _dgrad(g, S2, S2, sc, _lin_x3t(l1), LM, S2, H, None, 0, dh, H, dc, H)
    return dh, dc


def _gru_cells_bwd(p, dhf, dhp, grads):
    """GRU cells of _backward, per step and cell in reverse: gm_gru_cell_bwd (sums the cell's gradient sources,
    writes the gate gradients dG and the direct h gradient g z), then one input-gradient GEMM on W4^T giving
    D = [dx | dh_w]. The h input's gradient is dh_w + dh_dir: the previous cell's call takes the two as separate
    sources; for the obs cell they are added once into the buffer that is step t-1's external state gradient.
    Fills the cells' parameter gradients; returns (gE, partE, gmaxE) for the batched encoder backward."""
    netmon = p.netmon
    Ls, B, A, N, F, od, odp, H, K, M, Ma = p.dims
    dev = dhf.device
    LM = Ls * M
    lib = L.lib()
    dG = torch.empty(K + 1, Ls, M, 4 * H, device=dev)
    rpb_c = 64
    nbc = (M + rpb_c - 1) // rpb_c
    bpart = torch.empty(K + 1, Ls, nbc, 4 * H, device=dev)
    gmax_obs, gmax_upd = _zeros1(dev), _zeros1(dev)
    E = p.enc_out[-1]
    Eb = p.enc_bits[-1]
    gE = torch.empty(LM, H, device=dev)
    partE = torch.empty(Ls, (M + 127) // 128, H, device=dev)
    gmaxE = _zeros1(dev)
    wt_obs, wt_upd = _gru_x3t(netmon.rnn_obs), _gru_x3t(netmon.rnn_update)
    ep_done = p.seq.episode_done.to(torch.uint8).contiguous()  # [L, B]
    sc_cell = torch.empty(1, device=dev)
    D = torch.empty(M, 2 * H, device=dev)
    dhd_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]  # dh_dir of the cell just processed
    ext_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    dh_ext = None
    calls = 0
    mean = int(netmon.agg_mode == 1)
    deg = p.nbr.shape[-1]
    for t in range(Ls - 1, -1, -1):
        nbr_t = p.nbr[t * B:(t + 1) * B]
        dhd_next = None
        for j in range(K, -1, -1):
            a = L.GRUBwdArgs()
            a.act, a.ld_act = p.act[j, t].data_ptr(), 4 * H
            hin = p.S_in[t] if j == 0 else p.S[j - 1, t]
            a.h, a.ld_h = hin.data_ptr(), H
            if j == K:
                a.dh0, a.ld_dh0 = dhf[t * M:(t + 1) * M].data_ptr(), H
                if dh_ext is not None:  # step t+1's input-state gradient, zero where episode t ended
                    a.dh_ext, a.ld_ext = dh_ext.data_ptr(), H
                    a.ext_mask, a.rows_per_sample = ep_done[t].data_ptr(), N
            else:
                a.dh0, a.ld_dh0 = D.data_ptr() + 4 * H, 2 * H  # h part of the next cell's input gradient ...
                a.dh2, a.ld_dh2 = dhd_next.data_ptr(), H       # ... and its direct part g z
                a.dm, a.ld_dm = D.data_ptr(), 2 * H            # its aggregate part, transposed
                a.nbr, a.n_nodes, a.deg, a.mean = nbr_t.data_ptr(), N, deg, mean
            if j == K - 1:
                a.dh1, a.ld_dh1 = dhp[t * M:(t + 1) * M].data_ptr(), H
            a.m, a.hidden = M, H
            a.dgates, a.ld_dg = dG[j, t].data_ptr(), 4 * H
            dhd = None
            if j > 0 or t > 0:  # the gradient w.r.t. the replayed start state is not needed
                dhd = dhd_buf[calls % 2]
                a.dh_dir, a.ld_dhd = dhd.data_ptr(), H
            calls += 1
            a.bias_part, a.rows_per_block = bpart[j, t].data_ptr(), rpb_c
            a.dg_scale = sc_cell.data_ptr()
            a.dg_max = (gmax_obs if j == 0 else gmax_upd).data_ptr()
            L.check(lib.gm_gru_cell_bwd(C.byref(a), L.stream_ptr()))
            if j > 0:
                _dgrad(dG[j, t], 4 * H, 4 * H, sc_cell, wt_upd, M, 2 * H, 2 * H, None, 0, D, 2 * H)
            else:
                # [x | h] input gradient of the obs cell: x part through the encoder's last leaky_relu (bias
                # partials and max for the batched encoder backward), h part + g z = the state gradient
                ext = ext_buf[t % 2]
                _dgrad(dG[0, t], 4 * H, 4 * H, sc_cell, wt_obs, M, 2 * H, H, Eb[t * M:(t + 1) * M], Eb.stride(0),
                       gE[t * M:(t + 1) * M], H, ext, H, part=partE[t], gmax=gmaxE)
                if t > 0:
                    ext.add_(dhd)
                dh_ext = ext
            dhd_next = dhd
    for j0, cell, gm_, sx, xs, hs in ((0, netmon.rnn_obs, gmax_obs, p.s_obs, E, p.S_in.reshape(LM, H)),
                                      (1, netmon.rnn_update, gmax_upd, p.s_upd, p.agg.reshape(K * LM, H),
                                       p.S[:K].reshape(K * LM, H))):
        n = 1 if j0 == 0 else K
        gx, gh = MD._wgrad_pair(dG[j0:j0 + n].reshape(-1, 4 * H), xs, H, hs, H, _finish(gm_), sx, sx)
        gru_param_grads(cell, grads, gx, gh, bpart[j0:j0 + n].reshape(-1, 4 * H).sum(0))
    return gE, partE, gmaxE


def _lnlstm_cells_bwd(p, dhf, dhp, grads, dc_aux=None):
    """LayerNorm-LSTM cells of _backward, per step and cell in reverse: gm_lnlstm_cell_bwd (sums the cell's gradient
    sources; writes dgi, dgh, the c gradient, parameter partials, the two scales and maxima), then the input
    gradients dgh @ W_hh (h part) and, for the update cell, dgi @ W_ih (the previous cell's transposed-aggregate
    source). The obs cell's dgi of all steps goes through W_ih and the encoder's last leaky mask in ONE GEMM after
    the loop, on the scale finished from the accumulated max. dc_aux [L*M, H] (optional): the aux head's gradient of
    every step's final c, the dc source of the step's last update cell. Fills the cells' parameter gradients; returns
    (gE, partE, gmaxE) for the batched encoder backward."""
    netmon = p.netmon
    Ls, B, A, N, F, od, odp, H, K, M, Ma = p.dims
    S2 = 2 * H
    dev = dhf.device
    LM = Ls * M
    lib = L.lib()
    co, cu = netmon.rnn_obs, netmon.rnn_update
    dgi_obs = torch.empty(Ls, M, 4 * H, device=dev)
    dgh_obs = torch.empty(Ls, M, 4 * H, device=dev)
    dgi_upd = torch.empty(K, Ls, M, 4 * H, device=dev)
    dgh_upd = torch.empty(K, Ls, M, 4 * H, device=dev)
    nw = (M + LNL_RPW - 1) // LNL_RPW
    part = torch.empty(nw, 14 * H, device=dev)  # one call's per-wave partials, summed into psum right after it
    psum = torch.empty(K + 1, Ls, 14 * H, device=dev)
    mx = {k: _zeros1(dev) for k in ("gi_obs", "gh_obs", "gi_upd", "gh_upd")}
    sc_i, sc_h = torch.empty(1, device=dev), torch.empty(1, device=dev)
    (wti_obs, wth_obs), (wti_upd, wth_upd) = _lnl_x3t(co), _lnl_x3t(cu)
    ep_done = p.seq.episode_done.to(torch.uint8).contiguous()  # [L, B]
    Dx, Dh = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)
    dh0_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    # every cell's dc source is the dc output of the cell processed just before it: two buffers in turn
    dc_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    dh_ext = dc_ext = None
    calls = 0
    mean = int(netmon.agg_mode == 1)
    deg = p.nbr.shape[-1]
    for t in range(Ls - 1, -1, -1):
        nbr_t = p.nbr[t * B:(t + 1) * B]
        dc_next = None
        for j in range(K, -1, -1):
            if j == 0:
                a = lnl_bwd_args(co, p.gi_obs[t], 4 * H, p.gh_obs[t], 4 * H, p.S_in[t], p.stats[0, t], M, H)
                dgi, dgh = dgi_obs[t], dgh_obs[t]
            else:
                G = p.g_upd[j - 1, t]
                a = lnl_bwd_args(cu, G, 8 * H, G.data_ptr() + 16 * H, 8 * H, p.S[j - 1, t], p.stats[j, t], M, H)
                dgi, dgh = dgi_upd[j - 1, t], dgh_upd[j - 1, t]
            if j == K:
                a.dh0, a.ld_dh0 = dhf[t * M:(t + 1) * M].data_ptr(), H
            else:
                a.dh0, a.ld_dh0 = Dh.data_ptr(), H  # h part of the next cell's input gradient
                a.dm, a.ld_dm = Dx.data_ptr(), H    # its aggregate part, transposed
                a.nbr, a.n_nodes, a.deg, a.mean = nbr_t.data_ptr(), N, deg, mean
            if j == K - 1:
                a.dh1, a.ld_dh1 = dhp[t * M:(t + 1) * M].data_ptr(), H
            if j == K and dh_ext is not None:  # step t+1's input-state gradient, zero where episode t ended
                a.dh_ext, a.ld_ext = dh_ext.data_ptr(), H
                a.dc_ext, a.ld_dcext = dc_ext.data_ptr(), H
                a.ext_mask, a.rows_per_sample = ep_done[t].data_ptr(), N
            if j == K and dc_aux is not None:
                dc_next = dc_aux[t * M:(t + 1) * M]
            if dc_next is not None:
                a.dc, a.ld_dc = dc_next.data_ptr(), H
            a.dgi, a.ld_dgi, a.dgh, a.ld_dgh = dgi.data_ptr(), 4 * H, dgh.data_ptr(), 4 * H
            dco = None
            if j > 0 or t > 0:  # the gradient w.r.t. the replayed start state is not needed
                dco = dc_buf[calls % 2]
                a.dc_out, a.ld_dco = dco.data_ptr(), H
            calls += 1
            a.part = part.data_ptr()
            a.dgi_max = mx["gi_obs" if j == 0 else "gi_upd"].data_ptr()
            a.dgh_max = mx["gh_obs" if j == 0 else "gh_upd"].data_ptr()
            if j > 0:
                a.dgi_scale = sc_i.data_ptr()
            if j > 0 or t > 0:
                a.dgh_scale = sc_h.data_ptr()
            L.check(lib.gm_lnlstm_cell_bwd(C.byref(a), L.stream_ptr()))
            torch.sum(part, 0, out=psum[j, t])
            if j > 0:
                _dgrad(dgi, 4 * H, 4 * H, sc_i, wti_upd, M, H, H, None, 0, Dx, H)
                _dgrad(dgh, 4 * H, 4 * H, sc_h, wth_upd, M, H, H, None, 0, Dh, H)
            elif t > 0:  # the h part = step t-1's state gradient
                dh0 = dh0_buf[t % 2]
                _dgrad(dgh, 4 * H, 4 * H, sc_h, wth_obs, M, H, H, None, 0, dh0, H)
                dh_ext, dc_ext = dh0, dco
            dc_next = dco
    sa = {k: _finish(v) for k, v in mx.items()}
    # the obs cell's x gradient of all steps through the encoder's last leaky_relu (bias partials and max for the
    # batched encoder backward)
    E, Eb = p.enc_out[-1], p.enc_bits[-1]
    gE = torch.empty(LM, H, device=dev)
    partE = torch.empty((LM + 127) // 128, H, device=dev)
    gmaxE = _zeros1(dev)
    _dgrad(dgi_obs, 4 * H, 4 * H, sa["gi_obs"], wti_obs, LM, H, H, Eb, Eb.stride(0), gE, H, part=partE, gmax=gmaxE)
    # weight gradients over all steps (and update iterations), each operand with its own scale
    lnl_param_grads(co, grads, _wgrad(dgi_obs.view(LM, 4 * H), sa["gi_obs"], E, H, p.s_obs),
                    _wgrad(dgh_obs.view(LM, 4 * H), sa["gh_obs"], p.S_in.view(LM, S2), H, p.sh_obs),
                    psum[0].sum(0))
    lnl_param_grads(cu, grads, _wgrad(dgi_upd.view(K * LM, 4 * H), sa["gi_upd"], p.agg.view(K * LM, H), H, p.s_upd),
                    _wgrad(dgh_upd.view(K * LM, 4 * H), sa["gh_upd"], p.S[:K].reshape(K * LM, S2), H, p.sh_upd),
                    psum[1:].reshape(-1, 14 * H).sum(0))
    return gE, partE, gmaxE


def _backward(p, dq, daux=None):
    dqn = p.dqn
    Ls, B, A, N, F, od, odp, H, K, M, Ma = p.dims
    dev = dq.device
    LMa = Ls * Ma
    lib = L.lib()
    grads = {}
    dq = dq.contiguous()

    # ---- DQN ----
    dl = list(dqn.encoder.linear_layers)
    fc = dqn.q_net.fc
    nq = fc.out_features
    nl = len(dl)
    dlast = p.d[-1]
    n_last = dlast.shape[1]
    rpb = 512
    nb = (LMa + rpb - 1) // rpb
    g = torch.empty(LMa, n_last, device=dev)
    part_b = torch.empty(nb, n_last, device=dev)
    part_wq = torch.empty(nb, nq, n_last, device=dev)
    part_bq = torch.empty(nb, nq, device=dev)
    sc = torch.empty(1, device=dev)
    wq = fc.weight.detach().contiguous()
    L.check(lib.gm_qhead_bwd(dq.data_ptr(), nq, nq, wq.data_ptr(), wq.stride(0), dlast.data_ptr(), n_last, LMa, n_last,
                             1, g.data_ptr(), n_last, part_b.data_ptr(), part_wq.data_ptr(), part_bq.data_ptr(), rpb,
                             sc.data_ptr(), L.stream_ptr()))
    grads[fc.weight] = part_wq.sum(0)
    grads[fc.bias] = part_bq.sum(0)
    grads[dl[-1].bias] = part_b.sum(0)
    for i in range(nl - 1, 0, -1):
        lin = dl[i]
        xin = p.d[i - 1]
        kin = xin.shape[1]
        grads[lin.weight] = _wgrad(g, sc, xin, kin, p.d_in_scale[i])
        gn = torch.empty(LMa, kin, device=dev)
        part = torch.empty((LMa + 127) // 128, kin, device=dev)
        gmax = _zeros1(dev)
        xb = p.d_bits[i - 1]
        _dgrad(g, lin.out_features, lin.out_features, sc, _lin_x3t(lin), LMa, kin, kin, xb, xb.stride(0), gn, kin,
               part=part, gmax=gmax)
        grads[dl[i - 1].bias] = part.sum(0)
        g, sc = gn, _finish(gmax)
    lin0 = dl[0]
    s_in0 = p.d_in_scale[0]
    glob, GW = p.glob, p.GW
    w_r, w_env = MD._wgrad_pair(g, p.R, GW, p.env, od, sc, s_in0, s_in0)  # one launch: g read once per k chunk
    # the reference's column order: [env | h | nbr x 3], with the global readout [env | h | global | nbr x 3]
    grads[lin0.weight] = (torch.cat([w_env, w_r[:, :H], w_r[:, 4 * H:], w_r[:, H:4 * H]], 1) if glob
                          else torch.cat([w_env, w_r], 1))
    dR = torch.empty(LMa, GW, device=dev)
    _dgrad(g, lin0.out_features, lin0.out_features, sc, _dqn_first_x3t(lin0, od, H, glob), LMa, GW, GW,
           None, 0, dR, GW)
    return _backward_netmon(p, dR, grads, daux)


def _backward_netmon(p, dR, grads, daux=None):
    """The NetMon half of the backward from dR [L*B*A, GW], the gradient of the readout buffer p.R: the readout's
    transpose, the cells per step in reverse, the batched encoder backward. daux (with p.aux): the upstream
    gradient of _forward_aux's loss, whose state gradient joins the readout's before the cell loop. Adds NetMon's
    (and the aux head's) parameter gradients to grads and returns it."""
    netmon = p.netmon
    Ls, B, A, N, F, od, odp, H, K, M, Ma = p.dims
    S2 = 2 * H  # (lstm branch)
    dev = dR.device
    LM = Ls * M
    lib = L.lib()
    glob, GW = p.glob, p.GW

    # ---- readout over all steps ----
    dhf = torch.empty(LM, H, device=dev)
    dhp = torch.empty(LM, H, device=dev)
    L.check(lib.gm_netmon_readout_bwd(dR.data_ptr(), GW, p.nbr.data_ptr(), p.an.data_ptr(), Ls * B, N, A,
                                      p.nbr.shape[-1], H, dhf.data_ptr(), dhp.data_ptr(), L.stream_ptr()))
    if glob:  # the mean's transpose, added onto dh_final for every node of the graph
        with L.timed(f"gm_netmon_global_bwd:{LM}x{H}"):
            L.check(lib.gm_netmon_global_bwd(dR.data_ptr() + 16 * H, GW, Ls * B, N, H, A, dhf.data_ptr(), H,
                                             L.stream_ptr()))
    dc_aux = None
    if daux is not None:  # [dh_aux | dc_aux] of S[K] of all steps: h joins dh_final, c the last update cell's dc
        dh_aux, dc_aux = _backward_aux(p, daux, grads)
        dhf.add_(dh_aux)

    # ---- recurrent cells, per step, in reverse ----
    if netmon.rnn_type == "gru":
        gE, partE, gmaxE = _gru_cells_bwd(p, dhf, dhp, grads)
    elif netmon.rnn_type == "lnlstm":
        gE, partE, gmaxE = _lnlstm_cells_bwd(p, dhf, dhp, grads, dc_aux)
    else:
        dG = torch.empty(K + 1, Ls, M, 4 * H, device=dev)
        rpb_c = 64
        nbc = (M + rpb_c - 1) // rpb_c
        bpart = torch.empty(K + 1, Ls, nbc, 4 * H, device=dev)
        gmax_obs, gmax_upd = _zeros1(dev), _zeros1(dev)
        E = p.enc_out[-1]
        gE = torch.empty(LM, H, device=dev)
        nbe = (M + 127) // 128
        partE = torch.empty(Ls, nbe, H, device=dev)
        gmaxE = _zeros1(dev)
        wt_obs, wt_upd = _lstm_x3t(netmon.rnn_obs), _lstm_x3t(netmon.rnn_update)
        ep_done = p.seq.episode_done.to(torch.uint8).contiguous()  # [L, B]
        dh_ext = dc_ext = None
        sc_cell = torch.empty(1, device=dev)
        D = torch.empty(M, S2, device=dev)
        dh0_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
        # every cell's dc source is the dc output of the cell processed just before it (the next cell
        # of the step, or step t+1's obs cell): two buffers in turn
        dc_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
        calls = 0
        mean = int(netmon.agg_mode == 1)
        deg = p.nbr.shape[-1]
        for t in range(Ls - 1, -1, -1):
            nbr_t = p.nbr[t * B:(t + 1) * B]
            dc_next = None
            have_D = False
            for j in range(K, -1, -1):
                a = L.LSTMBwdArgs()
                a.act, a.ld_act = p.act[j, t].data_ptr(), 4 * H
                cin = p.S_in[t] if j == 0 else p.S[j - 1, t]
                a.c_in, a.ld_cin = cin.data_ptr() + 4 * H, S2
                a.c_out, a.ld_cout = p.S[j, t].data_ptr() + 4 * H, S2
                if j == K:
                    a.dh0, a.ld_dh0 = dhf[t * M:(t + 1) * M].data_ptr(), H
                else:
                    a.dh0, a.ld_dh0 = D.data_ptr() + 4 * H, S2  # h part of the next cell's input gradient
                    a.dm, a.ld_dm = D.data_ptr(), S2            # its aggregate part, transposed
                    a.nbr, a.n_nodes, a.deg, a.mean = nbr_t.data_ptr(), N, deg, mean
                if j == K - 1:
                    a.dh1, a.ld_dh1 = dhp[t * M:(t + 1) * M].data_ptr(), H
                if j == K and dh_ext is not None:  # step t+1's input-state gradient, zero where episode t ended
                    a.dh_ext, a.ld_ext = dh_ext.data_ptr(), H
                    a.dc_ext, a.ld_dcext = dc_ext.data_ptr(), H
                    a.ext_mask, a.rows_per_sample = ep_done[t].data_ptr(), N
                if j == K and dc_aux is not None:  # the aux head's gradient of this step's final c
                    dc_next = dc_aux[t * M:(t + 1) * M]
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
                a.dg_max = (gmax_obs if j == 0 else gmax_upd).data_ptr()
                L.check(lib.gm_lstm_cell_bwd(C.byref(a), L.stream_ptr()))
                if j > 0:
                    _dgrad(dG[j, t], 4 * H, 4 * H, sc_cell, wt_upd, M, S2, S2, None, 0, D, S2)
                else:
                    # [x | h] input gradient of the obs cell: x part through the encoder's last leaky_relu
                    # (bias partials and max for the batched encoder backward), h part = the state gradient
                    dh0 = dh0_buf[t % 2]
                    Eb = p.enc_bits[-1]
                    _dgrad(dG[0, t], 4 * H, 4 * H, sc_cell, wt_obs, M, S2, H, Eb[t * M:(t + 1) * M], Eb.stride(0),
                           gE[t * M:(t + 1) * M], H, dh0, H, part=partE[t], gmax=gmaxE)
                    dh_ext, dc_ext = dh0, dco
                dc_next = dco
        # LSTM weight / bias gradients over all steps (and update iterations)
        for j0, cell, gm_, sx, xs, hs in ((0, netmon.rnn_obs, gmax_obs, p.s_obs, E, p.S_in.reshape(LM, S2)),
                                          (1, netmon.rnn_update, gmax_upd, p.s_upd, p.agg.reshape(K * LM, H),
                                           p.S[:K].reshape(K * LM, S2))):
            gs = dG[j0:j0 + (1 if j0 == 0 else K)].reshape(-1, 4 * H)
            sa = _finish(gm_)
            grads[cell.weight_ih], grads[cell.weight_hh] = MD._wgrad_pair(gs, xs, H, hs, H, sa, sx, sx)
            bg = bpart[j0:j0 + (1 if j0 == 0 else K)].reshape(-1, 4 * H).sum(0)
            grads[cell.bias_ih] = bg
            grads[cell.bias_hh] = bg.clone()

    # ---- NetMon encoder over all steps ----
    enc = list(netmon.encode.linear_layers)
    g, sc = gE, _finish(gmaxE)
    grads[enc[-1].bias] = partE.reshape(-1, H).sum(0)
    for i in range(len(enc) - 1, -1, -1):
        lin = enc[i]
        xin, ldx, kin, sx = p.enc_in[i]
        grads[lin.weight] = _wgrad(g, sc, xin, kin, sx)
        if i > 0:
            gn = torch.empty(LM, kin, device=dev)
            part = torch.empty((LM + 127) // 128, kin, device=dev)
            gmax = _zeros1(dev)
            xb = p.enc_bits[i - 1]
            _dgrad(g, lin.out_features, lin.out_features, sc, _lin_x3t(lin), LM, kin, kin, xb, xb.stride(0), gn, kin,
                   part=part, gmax=gmax)
            grads[enc[i - 1].bias] = part.sum(0)
            g, sc = gn, _finish(gmax)
    return grads


class _SeqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, *params):
        ctx.plan = plan
        with torch.no_grad():
            q = _forward(plan)
            if plan.aux is None:
                return q
            return q, _forward_aux(plan)

    @staticmethod
    def backward(ctx, dq, daux=None):
        p = ctx.plan
        grads = _backward(p, dq, daux)
        ctx.plan = None
        return (None,) + tuple(grads.get(w) for w in p.params)


@torch.no_grad()
def _target_max(p, model_tar, gamma_unused=None):
    """max_a Q_target(next obs) [L, B, A]: steps 0..L-2 on the online observations of steps 1..L-1
    (one batched no-grad DQN pass; the target NetMon is the online NetMon, so its step t+1 is the
    online step t+1), except the sequences whose episode ended at t, which get their own NetMon
    step on the stored next observation; the last step runs its own NetMon step for all
    (src/main.py:878-915)."""
    from .train import _fused_next_q

    Ls, B, A, N, F, od, odp, H, K, M, Ma = p.dims
    sb = p.seq
    netmon = p.netmon
    dev = p.R.device
    out = torch.empty(Ls, B, A, device=dev)
    if Ls > 1:
        env = sb.obs[1:].reshape((Ls - 1) * B, A, odp)[..., :od]
        graph = p.R[Ma:].view((Ls - 1) * B, A, p.GW)
        q = FU.dqn_q_dense(model_tar, env, graph, lambda i, m, n: torch.empty(m, n, device=dev),
                           global_h=H if p.glob else None)
        out[:-1] = q.view(Ls - 1, B, A, -1).max(dim=-1)[0]
        done_rows = sb.episode_done[:-1].nonzero().cpu()  # one host read per update
        for t in torch.unique(done_rows[:, 0]).tolist():
            r = done_rows[done_rows[:, 0] == t, 1].to(dev)
            no, nno, nan_ = sb.next_fields(t, r)
            st = p.S[K, t].view(B, N, netmon.state_size)[r]
            nb = sb.nbr[t][r]
            out[t, r] = _fused_next_q(netmon, model_tar, no[..., :od], nno, nb, nan_, st).max(dim=2)[0]
    no, nno, nan_ = sb.next_fields(Ls - 1, None)
    out[-1] = _fused_next_q(netmon, model_tar, no[..., :od], nno, sb.nbr[-1], nan_,
                            p.S[K, Ls - 1].view(B, N, netmon.state_size)).max(dim=2)[0]
    return out


def seq_loss(netmon, model, model_tar, seq, gamma, params, parts=None, aux_model=None, aux_coeff=0.0):
    """Loss of src/main.py:840-1000 over a SeqBatch: (loss, q [L, B, A, nq], q_target). aux_model (aux_ok): the
    NetMon aux loss against seq.node_aux, weighted by aux_coeff, is added (params then includes the head's);
    parts (a dict) receives the loss terms."""
    p = _Plan()
    p.netmon, p.dqn, p.seq, p.params, p.aux = netmon, model, seq, list(params), aux_model
    loss_aux = None
    if aux_model is None:
        q = _SeqFn.apply(p, *p.params)
    else:
        if seq.node_aux is None:
            raise ValueError("seq_loss: the aux loss needs SeqBatch.node_aux (ReplayBuffer(node_aux_size=...))")
        want = (*seq.node_obs.shape[:3], aux_model.linear_layers[-1].out_features)
        if tuple(seq.node_aux.shape) != want:
            raise ValueError(f"seq_loss: SeqBatch.node_aux is {tuple(seq.node_aux.shape)}, the aux head wants {want} "
                             "([L, B, N, n_aux])")
        q, loss_aux = _SeqFn.apply(p, *p.params)
    Ls, B, A = seq.action.shape
    q = q.view(Ls, B, A, -1)
    nxt = _target_max(p, model_tar)
    target = seq.reward + (~seq.done) * gamma * nxt
    q_target = torch.scatter(q.detach(), -1, seq.action.unsqueeze(-1), target.unsqueeze(-1))
    loss_q = (q - q_target).pow(2).mean(dim=(1, 2, 3)).sum() / Ls
    loss = loss_q if loss_aux is None else loss_q + aux_coeff * loss_aux
    if parts is not None:
        parts.update(loss_q=loss_q, loss_att=None, loss_aux=loss_aux)
    return loss, q, q_target


def dqn_update_seq(netmon, model, model_tar, optimizer, params, seq, gamma, tau, target_update_steps=0, iteration=1,
                   group=None, aux_model=None, aux_coeff=0.0, parts=None):
    """One update (src/main.py:840-1026) on a SeqBatch: the sequence-batched loss and backward, the
    gradient all-reduce across ranks, clip by value (0.5) and norm (1.0), AdamW, target update. params must
    include aux_model's parameters when the aux loss is on (src/main.py:594)."""
    from .train import allreduce_gradients, interpolate_model

    loss, q, qt = seq_loss(netmon, model, model_tar, seq, gamma, params, parts, aux_model, aux_coeff)
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
