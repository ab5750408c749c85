"""Sequence-batched NetMon for the supervised driver (BASELINE config 5, reference src/sl.py:360-424)
with a hand-written backward.

The reference unrolls NetMon `sequence_length` times on the same graphs from a zero state
(src/sl.py:363-368), reads out every node after each step (NetMon without agent mapping,
src/sl.py:132-168, src/model.py:451-631) and backpropagates the mean of the per-step losses through
all of it with autograd. Here the NetMon part of the whole unroll is one autograd node (`_Fn`): its
output is the readout of every node at every step, [L, B*N, 4H]; the heads and the loss stay in
autograd and run once over all L steps' rows (sl.NetMonSL.forward_seq).

GRU cells (--netmon-rnn-type gru) run the same unroll with train_seq.py's GRU pieces: one GM_EPI_BIAS GEMM on
the four-tile weight W4 + gm_gru_cell_fwd forward (state rows H wide, G = [r | z | n | a_nh] saved), and
gm_gru_cell_bwd + one input-gradient GEMM on W4^T backward (_forward_gru / _backward_gru below).

LayerNorm-LSTM cells (--netmon-rnn-type lnlstm) run it with train_seq.py's LN-LSTM pieces (_forward_lnl /
_backward_lnl): two no-bias GEMMs per cell into saved raw products + gm_lnlstm_fwd, and gm_lnlstm_cell_bwd + the
input-gradient GEMMs backward. The obs cell's x is the same encoder output at every step and its LayerNorm sees
x W_ih^T alone, so that product is computed once and its gradient is summed over the steps before one W_ih weight
gradient and the one encoder backward. (sl.py itself keeps lnlstm on the autograd path: DESIGN §5a.)

Forward (LSTM): the encoder MLP once (the observations are the same at every step), then per step the obs
LSTM cell ([encoder output | h] as the GEMM's two sources, gate math in the epilogue) and K x
(aggregate, update cell), the state carried in place (S[K, t-1] is step t's input state), the
readout of every step.

Backward (the sequence-batched update's kernels, train_seq.py): the readout backward of every step,
then per step and cell, in reverse, gm_lstm_cell_bwd (sums the readout gradient, the next cell's h
gradient, the transposed aggregate of its x gradient and the next step's state gradient; writes the
gate gradients, bias partials and their scale) and one input-gradient GEMM per cell; the weight
gradients of the update cell over all steps at once; the encoder's gradient summed over the steps
(its output fed every step) before ONE encoder backward. No autograd accumulation of the h / c / encoder
gradients (the reference's graph adds them tensor by tensor).
"""
import ctypes as C

import torch

from . import _lib as L
from . import fused as FU
from . import train_seq as TS


def seq_bytes(netmon, rows, steps):
    """Device bytes the unroll keeps for its backward at M = rows node rows and L = steps: per cell and
    step the [h | c] output (2H; gru: h, H), the gate activations (4H) and their gradient (4H), plus the K
    aggregates (H), all fp32; lnlstm: the tensors _forward_lnl / _backward_lnl keep (kept_lnl)."""
    H, K = netmon.hidden_features, netmon.iterations
    if netmon.rnn_type == "lnlstm":
        # per cell and step the [h | c] row (2H) and the 8 statistics; the raw gate products and their gradients:
        # the obs cell's gi once (its x is the same at every step) with its gradient summed over the steps (one
        # step's buffer + the sum), its gh (4H) and d gh (4H) per step, the update cells' 8H + 8H per step; the
        # K aggregates (H)
        per_step = (K + 1) * (2 * H + 8) + 8 * H + K * 16 * H + K * H
        return 4 * rows * (steps * per_step + 12 * H)
    per_cell = 9 if netmon.rnn_type == "gru" else 10
    return 4 * steps * rows * ((K + 1) * per_cell * H + K * H)


def _device_room(dev):
    free, _ = torch.cuda.mem_get_info(dev)
    return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)


def seq_ok(netmon, rows=None, steps=None):
    """The configurations this path covers: LSTM, GRU or LayerNorm-LSTM cells with carry-over, sum / mean aggregation,
    neighbour readout without the global mean, leaky encoder layers with biases, split-f16 GEMMs;
    with rows / steps given, also that the unroll's saved tensors (seq_bytes) fit the device with a
    margin (otherwise the caller runs the per-step autograd path instead of failing with OOM)."""
    if netmon is None or L.GEMM_MODE != "x3":
        return False
    enc = list(netmon.encode.linear_layers)
    H = netmon.hidden_features
    ok = (TS.cell_ok(netmon) and netmon.rnn_carryover and netmon.output_neighbor_hidden
          and not netmon.output_global_hidden and netmon.iterations >= 1 and H % 32 == 0 and H <= 1024
          and len(enc) >= 1 and all(l.act == 1 and l.bias is not None for l in enc))
    if ok and rows is not None and steps is not None:
        # decided once per (module, rows, steps) shape: the allocator's free memory moves from step to
        # step, and the path (and with it the summation order) must not flip mid-run
        key = (rows, steps)
        cache = netmon.__dict__.setdefault("_sl_seq_fits", {})
        if key not in cache:
            dev = next(netmon.parameters()).device
            cache[key] = 1.25 * seq_bytes(netmon, rows, steps) < _device_room(dev)
        ok = cache[key]
    return ok


class _Plan:
    pass


def _encode(p, X, M, N, B, nbr):
    """The encoder MLP once over the M node rows (sign bits and operand scales kept for the backward)."""
    netmon = p.netmon
    dev = X.device
    F = p.x.shape[2]
    enc = list(netmon.encode.linear_layers)
    p.enc_in, p.enc_out, p.enc_bits = [], [], []
    x, ldx, kx = X, X.stride(0), F
    for i, lin in enumerate(enc):
        n = lin.out_features
        y = torch.empty(M, n, device=dev)
        yb = TS._sign_bits(M, n, dev)
        if i == 0 and FU.routing_encoder_ok(lin, N, F, nbr):
            FU.routing_encoder(lin, X, nbr, B, N, y, sbits=yb)
            sx = torch.empty(1, device=dev)
            L.check(FU._setup().gm_absmax_scale_rows(X.data_ptr(), M, F, X.stride(0), sx.data_ptr(), L.stream_ptr()))
        else:
            sx = TS._zeros1(dev)
            TS._gemm_amax(x, ldx, kx, TS._lin_x3(lin), lin.bias, M, n, FU.GM_EPI_BIAS_LEAKY, y, n, sx, sbits=yb)
            TS._finish(sx)
        p.enc_in.append((x, ldx, kx, sx))
        p.enc_out.append(y)
        p.enc_bits.append(yb)
        x, ldx, kx = y, n, n
    return p.enc_out[-1]


def _encoder_bwd(p, gEs, partE, grads):
    """The encoder backward, once, on the gradient summed over the steps."""
    Ls, B, N, F, H, K, M = p.dims
    dev = gEs.device
    enc = list(p.netmon.encode.linear_layers)
    g = gEs.sum(0) if Ls > 1 else gEs[0]
    sc = torch.empty(1, device=dev)
    L.check(FU._setup().gm_absmax_scale(g.data_ptr(), g.numel(), sc.data_ptr(), L.stream_ptr()))
    grads[enc[-1].bias] = partE.reshape(-1, H).sum(0)
    for i in range(len(enc) - 1, -1, -1):
        lin = enc[i]
        xin, ldx, kin, sx = p.enc_in[i]
        grads[lin.weight] = TS._wgrad(g, sc, xin, kin, sx)
        if i > 0:
            gn = torch.empty(M, kin, device=dev)
            part = torch.empty((M + 127) // 128, kin, device=dev)
            gmax = TS._zeros1(dev)
            xb = p.enc_bits[i - 1]
            TS._dgrad(g, lin.out_features, lin.out_features, sc, TS._lin_x3t(lin), M, kin, kin, xb, xb.stride(0), gn,
                      kin, part=part, gmax=gmax)
            grads[enc[i - 1].bias] = part.sum(0)
            g, sc = gn, TS._finish(gmax)
    return grads


def _forward_gru(p):
    """_forward for GRU cells: state rows [M][H]; per cell one W4 GEMM + gm_gru_cell_fwd (train_seq.gru_cell_fwd)."""
    netmon = p.netmon
    X3d, nbr, Ls = p.x, p.nbr, p.steps
    dev = X3d.device
    B, N, F = X3d.shape
    H, K = netmon.hidden_features, netmon.iterations
    M = B * N
    p.dims = (Ls, B, N, F, H, K, M)
    mean = int(netmon.agg_mode == 1)
    X = X3d.reshape(M, F)
    if X.stride(0) % 4 or X.data_ptr() % 16:
        Xp = torch.zeros(M, (F + 3) // 4 * 4, device=dev)
        Xp[:, :F] = X
        X = Xp
    deg = nbr.shape[-1]
    lib = L.lib()
    E = _encode(p, X, M, N, B, nbr)  # [M][H], every step's obs-cell input
    S = torch.empty(K + 1, Ls, M, H, device=dev)  # cell outputs h: j = 0 obs, 1..K update
    act = torch.empty(K + 1, Ls, M, 4 * H, device=dev)  # G = [r | z | n | a_nh]
    agg = torch.empty(K, Ls, M, H, device=dev)
    Z = torch.zeros(M, H, device=dev)  # the state starts at zero (src/sl.py:365)
    s_obs, s_upd = TS._zeros1(dev), TS._zeros1(dev)
    wo, wu = TS._gru_fwd(netmon.rnn_obs), TS._gru_fwd(netmon.rnn_update)
    for t in range(Ls):
        TS.gru_cell_fwd(E, Z if t == 0 else S[K, t - 1], H, *wo, M, H, s_obs, act[0, t], S[0, t], H)
        for j in range(1, K + 1):
            prev = S[j - 1, t]
            L.check(lib.gm_mp_aggregate_rows(prev.data_ptr(), H, nbr.data_ptr(), B, N, deg, H, mean,
                                             agg[j - 1, t].data_ptr(), H, L.stream_ptr()))
            TS.gru_cell_fwd(agg[j - 1, t], prev, H, *wu, M, H, s_upd, act[j, t], S[j, t], H)
    TS._finish(s_obs)
    TS._finish(s_upd)
    p.S, p.act, p.agg, p.Z, p.s_obs, p.s_upd = S, act, agg, Z, s_obs, s_upd
    R = torch.empty(Ls * M, 4 * H, device=dev)
    for t in range(Ls):
        L.check(lib.gm_netmon_readout_ld(S[K, t].data_ptr(), H, S[K - 1, t].data_ptr(), H, nbr.data_ptr(), None, B, N,
                                         N, deg, H, R[t * M:(t + 1) * M].data_ptr(), 4 * H, L.stream_ptr()))
    netmon.state = S[K, Ls - 1].view(B, N, H)  # the state after the last step
    return R.view(Ls, M, 4 * H)


def _backward_gru(p, dR):
    """_backward for GRU cells: gm_gru_cell_bwd + one input-gradient GEMM on W4^T per step and cell; a cell's h
    gradient = the GEMM's h part + the direct part g z (two sources of the previous cell's call; added once for
    the obs cell into step t-1's state gradient); W4's gradients mapped back to torch's layout."""
    netmon = p.netmon
    Ls, B, N, F, H, K, M = p.dims
    dev = dR.device
    nbr = p.nbr
    deg = nbr.shape[-1]
    lib = L.lib()
    grads = {}
    dR = dR.reshape(Ls * M, 4 * H).contiguous()
    dhp = torch.empty(Ls * M, H, device=dev)
    for t in range(Ls):
        L.check(lib.gm_netmon_readout_bwd_sym(dR[t * M:(t + 1) * M].data_ptr(), 4 * H, nbr.data_ptr(), B, N, deg,
                                              H, None, dhp[t * M:(t + 1) * M].data_ptr(), L.stream_ptr()))
    S, act, Z = p.S, p.act, p.Z
    dG = torch.empty(K + 1, Ls, M, 4 * H, device=dev)
    rpb_c = 64
    bpart = torch.empty(K + 1, Ls, (M + rpb_c - 1) // rpb_c, 4 * H, device=dev)
    gmax_obs, gmax_upd = TS._zeros1(dev), TS._zeros1(dev)
    gEs = torch.empty(Ls, M, H, device=dev)  # the encoder output's gradient from each step's obs cell
    partE = torch.empty(Ls, (M + 127) // 128, H, device=dev)
    wt_obs, wt_upd = TS._gru_x3t(netmon.rnn_obs), TS._gru_x3t(netmon.rnn_update)
    sc_cell = torch.empty(1, device=dev)
    D = torch.empty(M, 2 * H, device=dev)
    dhd_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    ext_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    Eb = p.enc_bits[-1]
    mean = int(netmon.agg_mode == 1)
    dh_ext = None
    calls = 0
    for t in range(Ls - 1, -1, -1):
        dhd_next = None
        for j in range(K, -1, -1):
            a = L.GRUBwdArgs()
            a.act, a.ld_act = act[j, t].data_ptr(), 4 * H
            hin = (Z if t == 0 else S[K, t - 1]) if j == 0 else S[j - 1, t]
            a.h, a.ld_h = hin.data_ptr(), H
            if j == K:
                a.dh0, a.ld_dh0 = dR[t * M:(t + 1) * M].data_ptr(), 4 * H  # dh_final: segment 0 of dR
                if dh_ext is not None:  # step t+1's input-state gradient (no episode ends here)
                    a.dh_ext, a.ld_ext = dh_ext.data_ptr(), H
            else:
                a.dh0, a.ld_dh0 = D.data_ptr() + 4 * H, 2 * H  # h part of the next cell's input gradient ...
                a.dh2, a.ld_dh2 = dhd_next.data_ptr(), H       # ... and its direct part g z
                a.dm, a.ld_dm = D.data_ptr(), 2 * H            # its aggregate part, transposed
                a.nbr, a.n_nodes, a.deg, a.mean = nbr.data_ptr(), N, deg, mean
            if j == K - 1:
                a.dh1, a.ld_dh1 = dhp[t * M:(t + 1) * M].data_ptr(), H
            a.m, a.hidden = M, H
            a.dgates, a.ld_dg = dG[j, t].data_ptr(), 4 * H
            dhd = None
            if j > 0 or t > 0:  # the gradient w.r.t. the zero start state is not needed
                dhd = dhd_buf[calls % 2]
                a.dh_dir, a.ld_dhd = dhd.data_ptr(), H
            calls += 1
            a.bias_part, a.rows_per_block = bpart[j, t].data_ptr(), rpb_c
            a.dg_scale = sc_cell.data_ptr()
            a.dg_max = (gmax_obs if j == 0 else gmax_upd).data_ptr()
            L.check(lib.gm_gru_cell_bwd(C.byref(a), L.stream_ptr()))
            if j > 0:
                TS._dgrad(dG[j, t], 4 * H, 4 * H, sc_cell, wt_upd, M, 2 * H, 2 * H, None, 0, D, 2 * H)
            else:
                ext = ext_buf[t % 2]
                TS._dgrad(dG[0, t], 4 * H, 4 * H, sc_cell, wt_obs, M, 2 * H, H, Eb, Eb.stride(0), gEs[t], H, ext, H,
                          part=partE[t])
                if t > 0:
                    ext.add_(dhd)
                dh_ext = ext
            dhd_next = dhd

    # ---- cell weight / bias gradients: dW4's x and h halves, mapped back to torch's layout ----
    sa_obs, sa_upd = TS._finish(gmax_obs), TS._finish(gmax_upd)
    E = p.enc_out[-1]
    # x half of the obs cell: every step's x is the same E (row map period M), as in the LSTM unroll
    r = TS.MD._wgrad2(dG[0].reshape(Ls * M, 4 * H), [(E, H, p.s_obs, M, 0)], sa_obs) if Ls > 1 else None
    if r is not None:
        gx = r[0]
    else:
        gx = None
        for t in range(Ls):
            w_t = TS._wgrad(dG[0, t], sa_obs, E, H, p.s_obs)
            gx = w_t if gx is None else gx.add_(w_t)
    # h half: step 0's h is zero; step t's is S[K, t-1] (contiguous over t = 1..L-1)
    if Ls > 1:
        gh = TS._wgrad(dG[0, 1:].reshape(-1, 4 * H), sa_obs, S[K, :Ls - 1].reshape(-1, H), H, p.s_obs)
    else:
        gh = torch.zeros(4 * H, H, device=dev)
    TS.gru_param_grads(netmon.rnn_obs, grads, gx, gh, bpart[0].reshape(-1, 4 * H).sum(0))
    gx, gh = TS.MD._wgrad_pair(dG[1:].reshape(-1, 4 * H), p.agg.reshape(K * Ls * M, H), H,
                               S[:K].reshape(K * Ls * M, H), H, sa_upd, p.s_upd, p.s_upd)
    TS.gru_param_grads(netmon.rnn_update, grads, gx, gh, bpart[1:].reshape(-1, 4 * H).sum(0))
    return _encoder_bwd(p, gEs, partE, grads)


def kept_lnl(p):
    """The tensors the LayerNorm-LSTM unroll keeps between its forward and the end of its backward (what seq_bytes
    counts for lnlstm)."""
    return [p.S, p.stats, p.agg, p.gi_obs, p.gh_obs, p.g_upd] + list(getattr(p, "bwd_kept", []))


def _forward_lnl(p):
    """_forward for LayerNorm-LSTM cells: state rows [h | c]; per cell two no-bias GEMMs (x W_ih^T, h W_hh^T) into
    saved raw products + gm_lnlstm_fwd. The obs cell's x is the encoder output at every step and its LayerNorm
    sees x W_ih^T alone: gi_obs is computed once."""
    netmon = p.netmon
    X3d, nbr, Ls = p.x, p.nbr, p.steps
    dev = X3d.device
    B, N, F = X3d.shape
    H, K = netmon.hidden_features, netmon.iterations
    S2 = 2 * H
    M = B * N
    p.dims = (Ls, B, N, F, H, K, M)
    mean = int(netmon.agg_mode == 1)
    X = X3d.reshape(M, F)
    if X.stride(0) % 4 or X.data_ptr() % 16:
        Xp = torch.zeros(M, (F + 3) // 4 * 4, device=dev)
        Xp[:, :F] = X
        X = Xp
    deg = nbr.shape[-1]
    lib = L.lib()
    E = _encode(p, X, M, N, B, nbr)  # [M][H], every step's obs-cell input
    co, cu = netmon.rnn_obs, netmon.rnn_update
    S = torch.empty(K + 1, Ls, M, S2, device=dev)  # cell outputs [h | c]: j = 0 obs, 1..K update
    stats = torch.empty(K + 1, Ls, M, 8, device=dev)
    agg = torch.empty(K, Ls, M, H, device=dev)
    gi_obs = torch.empty(M, 4 * H, device=dev)
    gh_obs = torch.empty(Ls, M, 4 * H, device=dev)
    g_upd = torch.empty(K, Ls, M, 8 * H, device=dev)
    Z = torch.zeros(M, S2, device=dev)  # the state starts at zero (src/sl.py:365)
    s_obs, s_upd, sh_obs, sh_upd = (TS._zeros1(dev) for _ in range(4))
    TS.lnl_gemm(E, H, co, False, M, H, s_obs, gi_obs, 4 * H)
    for t in range(Ls):
        sh = Z if t == 0 else S[K, t - 1]
        TS.lnl_gemm(sh, S2, co, True, M, H, sh_obs, gh_obs[t], 4 * H)
        TS.lnl_cell_fwd(co, gi_obs, 4 * H, gh_obs[t], 4 * H, sh, S[0, t], M, H, stats[0, t])
        for j in range(1, K + 1):
            prev, G = S[j - 1, t], g_upd[j - 1, t]
            L.check(lib.gm_mp_aggregate_rows(prev.data_ptr(), S2, nbr.data_ptr(), B, N, deg, H, mean,
                                             agg[j - 1, t].data_ptr(), H, L.stream_ptr()))
            TS.lnl_gemm(agg[j - 1, t], H, cu, False, M, H, s_upd, G, 8 * H)
            TS.lnl_gemm(prev, S2, cu, True, M, H, sh_upd, G.data_ptr() + 16 * H, 8 * H)
            TS.lnl_cell_fwd(cu, G, 8 * H, G.data_ptr() + 16 * H, 8 * H, prev, S[j, t], M, H, stats[j, t])
    for sl in (s_obs, s_upd, sh_obs, sh_upd):
        TS._finish(sl)
    p.S, p.stats, p.agg, p.Z, p.gi_obs, p.gh_obs, p.g_upd = S, stats, agg, Z, gi_obs, gh_obs, g_upd
    p.s_obs, p.s_upd, p.sh_obs, p.sh_upd = s_obs, s_upd, sh_obs, sh_upd
    R = torch.empty(Ls * M, 4 * H, device=dev)
    for t in range(Ls):
        L.check(lib.gm_netmon_readout_ld(S[K, t].data_ptr(), S2, S[K - 1, t].data_ptr(), S2, nbr.data_ptr(), None, B,
                                         N, N, deg, H, R[t * M:(t + 1) * M].data_ptr(), 4 * H, L.stream_ptr()))
    netmon.set_state_hc(S[K, Ls - 1, :, :H], S[K, Ls - 1, :, H:], B, N)  # the state after the last step
    return R.view(Ls, M, 4 * H)


def _backward_lnl(p, dR):
    """_backward for LayerNorm-LSTM cells: gm_lnlstm_cell_bwd per step and cell in reverse, then dgh @ W_hh (h
    part) and, for the update cell, dgi @ W_ih (the previous cell's transposed-aggregate source). The obs cell's
    dgi is summed over the steps (its x is the same E at every step): one W_ih weight gradient and one input
    gradient through the encoder's last leaky mask on the sum, before the one encoder backward."""
    netmon = p.netmon
    Ls, B, N, F, H, K, M = p.dims
    S2 = 2 * H
    dev = dR.device
    nbr = p.nbr
    deg = nbr.shape[-1]
    lib = L.lib()
    grads = {}
    dR = dR.reshape(Ls * M, 4 * H).contiguous()
    dhp = torch.empty(Ls * M, H, device=dev)
    for t in range(Ls):
        L.check(lib.gm_netmon_readout_bwd_sym(dR[t * M:(t + 1) * M].data_ptr(), 4 * H, nbr.data_ptr(), B, N, deg,
                                              H, None, dhp[t * M:(t + 1) * M].data_ptr(), L.stream_ptr()))
    S, Z = p.S, p.Z
    co, cu = netmon.rnn_obs, netmon.rnn_update
    dgi_t = torch.empty(M, 4 * H, device=dev)      # the obs cell's dgi of one step ...
    dgi_sum = torch.empty(M, 4 * H, device=dev)    # ... and its sum over the steps
    dgh_obs = torch.empty(Ls, M, 4 * H, device=dev)
    dgi_upd = torch.empty(K, Ls, M, 4 * H, device=dev)
    dgh_upd = torch.empty(K, Ls, M, 4 * H, device=dev)
    p.bwd_kept = [dgi_t, dgi_sum, dgh_obs, dgi_upd, dgh_upd]
    nw = (M + TS.LNL_RPW - 1) // TS.LNL_RPW
    part = torch.empty(nw, 14 * H, device=dev)  # one call's per-wave partials, summed into psum right after it
    psum = torch.empty(K + 1, Ls, 14 * H, device=dev)
    mx = {k: TS._zeros1(dev) for k in ("gh_obs", "gi_upd", "gh_upd")}
    sc_i, sc_h = torch.empty(1, device=dev), torch.empty(1, device=dev)
    (wti_obs, wth_obs), (wti_upd, wth_upd) = TS._lnl_x3t(co), TS._lnl_x3t(cu)
    Dx, Dh = torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)
    dh0_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    dc_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    mean = int(netmon.agg_mode == 1)
    dh_ext = dc_ext = None
    calls = 0
    for t in range(Ls - 1, -1, -1):
        dc_next = None
        for j in range(K, -1, -1):
            if j == 0:
                a = TS.lnl_bwd_args(co, p.gi_obs, 4 * H, p.gh_obs[t], 4 * H, Z if t == 0 else S[K, t - 1],
                                    p.stats[0, t], M, H)
                dgi, dgh = dgi_sum if t == Ls - 1 else dgi_t, dgh_obs[t]
            else:
                G = p.g_upd[j - 1, t]
                a = TS.lnl_bwd_args(cu, G, 8 * H, G.data_ptr() + 16 * H, 8 * H, S[j - 1, t], p.stats[j, t], M, H)
                dgi, dgh = dgi_upd[j - 1, t], dgh_upd[j - 1, t]
            if j == K:
                a.dh0, a.ld_dh0 = dR[t * M:(t + 1) * M].data_ptr(), 4 * H  # dh_final: segment 0 of dR
            else:
                a.dh0, a.ld_dh0 = Dh.data_ptr(), H  # h part of the next cell's input gradient
                a.dm, a.ld_dm = Dx.data_ptr(), H    # its aggregate part, transposed
                a.nbr, a.n_nodes, a.deg, a.mean = nbr.data_ptr(), N, deg, mean
            if j == K - 1:
                a.dh1, a.ld_dh1 = dhp[t * M:(t + 1) * M].data_ptr(), H
            if j == K and dh_ext is not None:  # step t+1's input-state gradient (no episode ends here)
                a.dh_ext, a.ld_ext = dh_ext.data_ptr(), H
                a.dc_ext, a.ld_dcext = dc_ext.data_ptr(), H
            if dc_next is not None:
                a.dc, a.ld_dc = dc_next.data_ptr(), H
            a.dgi, a.ld_dgi, a.dgh, a.ld_dgh = dgi.data_ptr(), 4 * H, dgh.data_ptr(), 4 * H
            dco = None
            if j > 0 or t > 0:  # the gradient w.r.t. the zero start state is not needed
                dco = dc_buf[calls % 2]
                a.dc_out, a.ld_dco = dco.data_ptr(), H
            calls += 1
            a.part = part.data_ptr()
            if j > 0:
                a.dgi_scale, a.dgi_max = sc_i.data_ptr(), mx["gi_upd"].data_ptr()
            a.dgh_max = mx["gh_obs" if j == 0 else "gh_upd"].data_ptr()
            if j > 0 or t > 0:
                a.dgh_scale = sc_h.data_ptr()
            L.check(lib.gm_lnlstm_cell_bwd(C.byref(a), L.stream_ptr()))
            torch.sum(part, 0, out=psum[j, t])
            if j > 0:
                TS._dgrad(dgi, 4 * H, 4 * H, sc_i, wti_upd, M, H, H, None, 0, Dx, H)
                TS._dgrad(dgh, 4 * H, 4 * H, sc_h, wth_upd, M, H, H, None, 0, Dh, H)
            else:
                if t < Ls - 1:
                    dgi_sum.add_(dgi_t)
                if t > 0:  # the h part = step t-1's state gradient
                    dh0 = dh0_buf[t % 2]
                    TS._dgrad(dgh, 4 * H, 4 * H, sc_h, wth_obs, M, H, H, None, 0, dh0, H)
                    dh_ext, dc_ext = dh0, dco
            dc_next = dco

    # ---- the obs cell's x side on the summed dgi: W_ih's gradient and the encoder output's gradient ----
    E, Eb = p.enc_out[-1], p.enc_bits[-1]
    sa_sum = torch.empty(1, device=dev)
    L.check(FU._setup().gm_absmax_scale(dgi_sum.data_ptr(), dgi_sum.numel(), sa_sum.data_ptr(), L.stream_ptr()))
    gEs = torch.empty(1, M, H, device=dev)
    partE = torch.empty(1, (M + 127) // 128, H, device=dev)
    TS._dgrad(dgi_sum, 4 * H, 4 * H, sa_sum, wti_obs, M, H, H, Eb, Eb.stride(0), gEs[0], H, part=partE[0])
    gwi = TS._wgrad(dgi_sum, sa_sum, E, H, p.s_obs)
    # W_hh: step 0's h is zero; step t's is S[K, t-1] (contiguous over t = 1..L-1)
    sa = {k: TS._finish(v) for k, v in mx.items()}
    if Ls > 1:
        gwh = TS._wgrad(dgh_obs[1:].reshape(-1, 4 * H), sa["gh_obs"], S[K, :Ls - 1].reshape(-1, S2), H, p.sh_obs)
    else:
        gwh = torch.zeros_like(co.weight_hh)
    TS.lnl_param_grads(co, grads, gwi, gwh, psum[0].sum(0))
    KLM = K * Ls * M
    TS.lnl_param_grads(cu, grads, TS._wgrad(dgi_upd.view(KLM, 4 * H), sa["gi_upd"], p.agg.view(KLM, H), H, p.s_upd),
                       TS._wgrad(dgh_upd.view(KLM, 4 * H), sa["gh_upd"], S[:K].reshape(KLM, S2), H, p.sh_upd),
                       psum[1:].reshape(-1, 14 * H).sum(0))
    return _encoder_bwd(p, gEs, partE, grads)


def _forward(p):
    netmon = p.netmon
    if netmon.rnn_type == "gru":
        return _forward_gru(p)
    if netmon.rnn_type == "lnlstm":
        return _forward_lnl(p)
    X3d, nbr, Ls = p.x, p.nbr, p.steps
    dev = X3d.device
    B, N, F = X3d.shape
    H = netmon.hidden_features
    S2 = 2 * H
    K = netmon.iterations
    M = B * N
    p.dims = (Ls, B, N, F, H, K, M)
    mean = int(netmon.agg_mode == 1)
    X = X3d.reshape(M, F)
    if X.stride(0) % 4 or X.data_ptr() % 16:
        Xp = torch.zeros(M, (F + 3) // 4 * 4, device=dev)
        Xp[:, :F] = X
        X = Xp
    deg = nbr.shape[-1]
    lib = L.lib()

    E = _encode(p, X, M, N, B, nbr)  # [M][H], every step's obs-cell input

    # ---- LSTM cells, per step; the state starts at zero (src/sl.py:365) ----
    S = torch.empty(K + 1, Ls, M, S2, device=dev)  # cell outputs [h | c]: j = 0 obs, 1..K update
    act = torch.empty(K + 1, Ls, M, 4 * H, device=dev)
    agg = torch.empty(K, Ls, M, H, device=dev)
    Z = torch.zeros(M, S2, device=dev)
    s_obs, s_upd = TS._zeros1(dev), TS._zeros1(dev)
    wo = TS._lstm_fwd(netmon.rnn_obs)
    wu = TS._lstm_fwd(netmon.rnn_update)
    for t in range(Ls):
        sh = Z if t == 0 else S[K, t - 1]
        for j in range(K + 1):
            wp, ldw, bp, x3 = wo if j == 0 else wu
            if j == 0:
                xa, hsrc = FU.dense(E.data_ptr(), H, H, amax=s_obs.data_ptr()), sh
            else:
                prev = S[j - 1, t]
                L.check(lib.gm_mp_aggregate_rows(prev.data_ptr(), S2, nbr.data_ptr(), B, N, deg, H, mean,
                                                 agg[j - 1, t].data_ptr(), H, L.stream_ptr()))
                xa, hsrc = FU.dense(agg[j - 1, t].data_ptr(), H, H, amax=s_upd.data_ptr()), prev
            out = S[j, t]
            FU.gemm(xa, FU.dense(hsrc.data_ptr(), S2, H), wp.data_ptr(), ldw, bp.data_ptr(), M, 4 * H, FU.GM_EPI_LSTM,
                    out.data_ptr(), S2, out.data_ptr() + 4 * H, S2, hsrc.data_ptr() + 4 * H, S2, act[j, t].data_ptr(),
                    x3=x3)
    TS._finish(s_obs)
    TS._finish(s_upd)
    p.S, p.act, p.agg, p.Z, p.s_obs, p.s_upd = S, act, agg, Z, s_obs, s_upd

    # ---- readout of every node at every step: [h_final | h before the last update of 3 neighbours] ----
    R = torch.empty(Ls * M, 4 * H, device=dev)
    for t in range(Ls):
        L.check(lib.gm_netmon_readout_ld(S[K, t].data_ptr(), S2, S[K - 1, t].data_ptr(), S2, nbr.data_ptr(), None, B,
                                         N, N, deg, H, R[t * M:(t + 1) * M].data_ptr(), 4 * H, L.stream_ptr()))
    netmon.set_state_hc(S[K, Ls - 1, :, :H], S[K, Ls - 1, :, H:], B, N)  # the state after the last step
    return R.view(Ls, M, 4 * H)


def _backward(p, dR):
    netmon = p.netmon
    if netmon.rnn_type == "gru":
        return _backward_gru(p, dR)
    if netmon.rnn_type == "lnlstm":
        return _backward_lnl(p, dR)
    Ls, B, N, F, H, K, M = p.dims
    S2 = 2 * H
    dev = dR.device
    nbr = p.nbr
    deg = nbr.shape[-1]
    lib = L.lib()
    grads = {}
    dR = dR.reshape(Ls * M, 4 * H).contiguous()

    # ---- readout, every step: dh_final of node v is row v's first segment of dR (read in place by the
    # cell backward, ld 4H); dh_prev gathered from the neighbours' segments. The supervised driver's tables
    # are the routing env's own (sl.py's dataset clones env.nbr: symmetric, no repeated entries), so this caller opts
    # in to the gather kernel (gm_netmon_readout_bwd_sym); gm_netmon_readout_bwd takes any table
    dhp = torch.empty(Ls * M, H, device=dev)
    for t in range(Ls):
        L.check(lib.gm_netmon_readout_bwd_sym(dR[t * M:(t + 1) * M].data_ptr(), 4 * H, nbr.data_ptr(), B, N, deg,
                                              H, None, dhp[t * M:(t + 1) * M].data_ptr(), L.stream_ptr()))

    # ---- LSTM cells, per step, in reverse ----
    S, act, Z = p.S, p.act, p.Z
    dG = torch.empty(K + 1, Ls, M, 4 * H, device=dev)
    rpb_c = 64
    nbc = (M + rpb_c - 1) // rpb_c
    bpart = torch.empty(K + 1, Ls, nbc, 4 * H, device=dev)
    gmax_obs, gmax_upd = TS._zeros1(dev), TS._zeros1(dev)
    gEs = torch.empty(Ls, M, H, device=dev)  # the encoder output's gradient from each step's obs cell
    nbe = (M + 127) // 128
    partE = torch.empty(Ls, nbe, H, device=dev)
    wt_obs, wt_upd = TS._lstm_x3t(netmon.rnn_obs), TS._lstm_x3t(netmon.rnn_update)
    sc_cell = torch.empty(1, device=dev)
    D = torch.empty(M, S2, device=dev)
    dh0_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    dc_buf = [torch.empty(M, H, device=dev), torch.empty(M, H, device=dev)]
    Eb = p.enc_bits[-1]
    mean = int(netmon.agg_mode == 1)
    dh_ext = dc_ext = None
    calls = 0
    for t in range(Ls - 1, -1, -1):
        dc_next = None
        for j in range(K, -1, -1):
            a = L.LSTMBwdArgs()
            a.act, a.ld_act = act[j, t].data_ptr(), 4 * H
            cin = (Z if t == 0 else S[K, t - 1]) if j == 0 else S[j - 1, t]
            a.c_in, a.ld_cin = cin.data_ptr() + 4 * H, S2
            a.c_out, a.ld_cout = S[j, t].data_ptr() + 4 * H, S2
            if j == K:
                a.dh0, a.ld_dh0 = dR[t * M:(t + 1) * M].data_ptr(), 4 * H  # dh_final: segment 0 of dR
            else:
                a.dh0, a.ld_dh0 = D.data_ptr() + 4 * H, S2  # h part of the next cell's input gradient
                a.dm, a.ld_dm = D.data_ptr(), S2            # its aggregate part, transposed
                a.nbr, a.n_nodes, a.deg, a.mean = nbr.data_ptr(), N, deg, mean
            if j == K - 1:
                a.dh1, a.ld_dh1 = dhp[t * M:(t + 1) * M].data_ptr(), H
            if j == K and dh_ext is not None:  # step t+1's input-state gradient (no episode ends here)
                a.dh_ext, a.ld_ext = dh_ext.data_ptr(), H
                a.dc_ext, a.ld_dcext = dc_ext.data_ptr(), H
            if dc_next is not None:
                a.dc, a.ld_dc = dc_next.data_ptr(), H
            a.m, a.hidden = M, H
            a.dgates, a.ld_dg = dG[j, t].data_ptr(), 4 * H
            dco = None
            if j > 0 or t > 0:  # the gradient w.r.t. the zero start state is not needed
                dco = dc_buf[calls % 2]
                a.dc_out, a.ld_dco = dco.data_ptr(), H
            calls += 1
            a.bias_part, a.rows_per_block = bpart[j, t].data_ptr(), rpb_c
            a.dg_scale = sc_cell.data_ptr()
            a.dg_max = (gmax_obs if j == 0 else gmax_upd).data_ptr()
            L.check(lib.gm_lstm_cell_bwd(C.byref(a), L.stream_ptr()))
            if j > 0:
                TS._dgrad(dG[j, t], 4 * H, 4 * H, sc_cell, wt_upd, M, S2, S2, None, 0, D, S2)
            else:
                # [x | h] input gradient of the obs cell: x part through the encoder's last leaky_relu
                # (bias partials per step), h part = the state gradient of step t - 1
                dh0 = dh0_buf[t % 2]
                TS._dgrad(dG[0, t], 4 * H, 4 * H, sc_cell, wt_obs, M, S2, H, Eb, Eb.stride(0), gEs[t], H, dh0, H,
                          part=partE[t])
                dh_ext, dc_ext = dh0, dco
            dc_next = dco

    # ---- LSTM weight / bias gradients ----
    sa_obs, sa_upd = TS._finish(gmax_obs), TS._finish(gmax_upd)
    E = p.enc_out[-1]
    cell = netmon.rnn_obs
    # W_ih: every step's x is the same encoder output E: ONE launch over all L steps' gate gradients with E's
    # rows repeated (row map period M), instead of L launches of M rows (each at ~0.35 of the large-batch rate)
    r = TS.MD._wgrad2(dG[0].reshape(Ls * M, 4 * H), [(E, H, p.s_obs, M, 0)], sa_obs) if Ls > 1 else None
    if r is not None:
        grads[cell.weight_ih] = r[0]
    else:
        gw = None
        for t in range(Ls):
            w_t = TS._wgrad(dG[0, t], sa_obs, E, H, p.s_obs)
            gw = w_t if gw is None else gw.add_(w_t)
        grads[cell.weight_ih] = gw
    # W_hh: step 0's h is zero; step t's is S[K, t-1] (contiguous over t = 1..L-1)
    if Ls > 1:
        grads[cell.weight_hh] = TS._wgrad(dG[0, 1:].reshape(-1, 4 * H), sa_obs, S[K, :Ls - 1].reshape(-1, S2), H,
                                          p.s_obs)
    else:
        grads[cell.weight_hh] = torch.zeros_like(cell.weight_hh)
    bg = bpart[0].reshape(-1, 4 * H).sum(0)
    grads[cell.bias_ih] = bg
    grads[cell.bias_hh] = bg.clone()
    cell = netmon.rnn_update
    gs = dG[1:].reshape(-1, 4 * H)
    grads[cell.weight_ih], grads[cell.weight_hh] = TS.MD._wgrad_pair(gs, p.agg.reshape(K * Ls * M, H), H,
                                                                  S[:K].reshape(K * Ls * M, S2), H, sa_upd, p.s_upd,
                                                                  p.s_upd)
    bg = bpart[1:].reshape(-1, 4 * H).sum(0)
    grads[cell.bias_ih] = bg
    grads[cell.bias_hh] = bg.clone()

    return _encoder_bwd(p, gEs, partE, grads)


class _Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, *params):
        ctx.plan = plan
        with torch.no_grad():
            return _forward(plan)

    @staticmethod
    def backward(ctx, dR):
        p = ctx.plan
        grads = _backward(p, dR)
        ctx.plan = None
        return (None,) + tuple(grads.get(w) for w in p.params)


def readout_seq(netmon, x, nbr, steps):
    """NetMon unrolled `steps` times from a zero state on node observations x [B, N, F] with
    neighbour table nbr [B, N, deg] (int32): the readout of every node after every step,
    [steps, B*N, 4H], differentiable w.r.t. the NetMon parameters."""
    p = _Plan()
    p.netmon, p.x, p.nbr, p.steps = netmon, x, nbr.contiguous(), steps
    p.params = [w for w in netmon.parameters()]
    return _Fn.apply(p, *p.params)
