"""LayerNorm-LSTM NetMon on the sequence-batched training paths (train_seq.py, sl_seq.py): the cell backward
gm_lnlstm_cell_bwd against torch fp64 autograd of the reference formula and against gm_lnlstm_bwd bit for bit, the
whole update against the reference's golden LN-LSTM update (train_lnlstm.npz) and against the per-step autograd
path on replayed rollout data, and config 5's unroll against its per-step autograd path. The whole-update tests
run the LSTM tests' own setup with the cell type switched to lnlstm."""
import ctypes as C
import importlib

import pytest
import torch

import test_sl_seq_gpu as TSL
import test_train_seq_gpu as TTS
from test_cells_gpu import _ref_lnlstm
from test_gru_seq_gpu import _members_mask
from test_netmon_paths_gpu import sym_table

pytestmark = pytest.mark.gpu

# (m, H): a half-empty wave, ..., (35, 512) the largest units-per-lane, (70, 96) a partial second lane group
SHAPES = [(777, 32), (130, 64), (197, 128), (65, 256), (35, 512), (70, 96)]
RPW = 8  # rows per wave: a block of 4 waves owns 32 rows


def _lib():
    return importlib.import_module("graph-marl_amd._lib")


def _inputs(m, H, seed):
    """fp64 leaves of one cell (gi, gh, c and the seven parameter vectors), test_lnlstm_cell_fwd_bwd's distributions."""
    torch.manual_seed(seed)
    r = lambda *s: torch.randn(*s, dtype=torch.float64)  # noqa: E731
    leaves = [r(m, 4 * H) * 0.7 + 0.1, r(m, 4 * H) * 0.5 - 0.2, r(m, H), 1 + 0.1 * r(4 * H), 0.1 * r(4 * H),
              1 + 0.1 * r(4 * H), 0.1 * r(4 * H), 0.1 * r(4 * H), 1 + 0.1 * r(H), 0.1 * r(H)]
    return [t.requires_grad_() for t in leaves]


def _device_cell(L, leaves, m, H):
    """fp32 device copies: gi, gh, the [h | c] rows holding c, the parameters, and gm_lnlstm_fwd's stats; the args
    struct with the forward operands filled in."""
    gi, gh = (t.detach().float().cuda().contiguous() for t in leaves[:2])
    hc = torch.randn(m, 2 * H, device="cuda")
    hc[:, H:] = leaves[2].detach().float().cuda()
    ps = [t.detach().float().cuda().contiguous() for t in leaves[3:]]
    stats = torch.empty(m, 8, device="cuda")
    out = torch.empty(m, 2 * H, device="cuda")
    L.check(L.lib().gm_lnlstm_fwd(gi.data_ptr(), 4 * H, gh.data_ptr(), 4 * H, hc.data_ptr() + 4 * H, 2 * H,
                                  *(p.data_ptr() for p in ps), m, H, 1e-5, out.data_ptr(), 2 * H,
                                  out.data_ptr() + 4 * H, 2 * H, stats.data_ptr(), L.stream_ptr()))
    a = L.LNLSTMBwdArgs()
    a.gi, a.ld_gi, a.gh, a.ld_gh = gi.data_ptr(), 4 * H, gh.data_ptr(), 4 * H
    a.c_in, a.ld_cin = hc.data_ptr() + 4 * H, 2 * H
    (a.ln_in_w, a.ln_in_b, a.ln_hid_w, a.ln_hid_b, a.bias, a.ln_cell_w, a.ln_cell_b) = (p.data_ptr() for p in ps)
    a.eps, a.stats, a.m, a.hidden, a.rows_per_wave = 1e-5, stats.data_ptr(), m, H, RPW
    return a, (gi, gh, hc, ps, stats, out)


def _outputs(a, m, H, pad):
    """NaN-filled strided outputs with one guard row."""
    nan = lambda r, c: torch.full((r, c), float("nan"), device="cuda")  # noqa: E731
    dgi, dgh, dco = nan(m + 1, 4 * H + pad), nan(m + 1, 4 * H + 2 * pad), nan(m + 1, H + pad)
    a.dgi, a.ld_dgi, a.dgh, a.ld_dgh = dgi.data_ptr(), dgi.stride(0), dgh.data_ptr(), dgh.stride(0)
    return dgi, dgh, dco


@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("N", [4, 20])
@pytest.mark.parametrize("m,H", SHAPES)
def test_lnlstm_cell_bwd_vs_fp64_autograd(m, H, N, mean):
    """Every gradient source (dh0, dh1, the transposed aggregate of dm on tables with -1 entries in sum and mean,
    dh_ext / dc_ext under an ext_mask that zeroes some graphs but not all, dc) and every output against fp64
    autograd of the reference formula: dgi, dgh, dc_out and every summed parameter partial within rel 1e-5 (the
    bound test_lnlstm_cell_fwd_bwd holds gm_lnlstm_bwd to); the published max and scale of dgi and of dgh exact.
    Strided outputs: the padding and the guard row stay NaN."""
    L = _lib()
    FU = importlib.import_module("graph-marl_amd.fused")
    assert m % N and m % RPW and m % (4 * RPW), "m must leave a partial graph, wave and block"
    leaves = _inputs(m, H, m + H + N + mean)
    G_ = (m + N - 1) // N
    rows = G_ * N
    nbr = sym_table(G_, N, 3, seed=H + N)
    dh0, dh1, dhe, dce, dc = (torch.randn(m, H).cuda() for _ in range(5))
    dm = torch.randn(rows, H).cuda()
    emask = torch.rand(G_) < 0.4
    emask[0], emask[-1] = True, False
    cnt = (nbr >= 0).sum(-1).double() + 1  # |{n} U nbr(n)|
    s = (1.0 / cnt if mean else torch.ones_like(cnt)).unsqueeze(-1)
    agg = torch.einsum("grn,gnh->grh", _members_mask(nbr), dm.cpu().double().view(G_, N, H) * s)
    keep = (~emask).double().repeat_interleave(N)[:m].unsqueeze(1)
    g_h = dh0.cpu().double() + dh1.cpu().double() + agg.reshape(rows, H)[:m] + keep * dhe.cpu().double()
    g_c = dc.cpu().double() + keep * dce.cpu().double()
    h1, c1 = _ref_lnlstm(*leaves)
    want = torch.autograd.grad([h1, c1], leaves, [g_h, g_c])

    a, hold = _device_cell(L, leaves, m, H)
    dgi, dgh, dco = _outputs(a, m, H, 4)
    a.dc_out, a.ld_dco = dco.data_ptr(), dco.stride(0)
    nbr_d, em = nbr.cuda().contiguous(), emask.to(torch.uint8).cuda()
    a.dh0, a.ld_dh0, a.dh1, a.ld_dh1 = dh0.data_ptr(), H, dh1.data_ptr(), H
    a.dm, a.ld_dm, a.nbr, a.n_nodes, a.deg, a.mean = dm.data_ptr(), H, nbr_d.data_ptr(), N, 3, mean
    a.dh_ext, a.ld_ext, a.dc_ext, a.ld_dcext = dhe.data_ptr(), H, dce.data_ptr(), H
    a.ext_mask, a.rows_per_sample = em.data_ptr(), N
    a.dc, a.ld_dc = dc.data_ptr(), H
    part = torch.empty((m + RPW - 1) // RPW, 14 * H, device="cuda")
    sc = torch.empty(2, device="cuda")
    mx = torch.zeros(2, device="cuda")
    a.part = part.data_ptr()
    a.dgi_scale, a.dgh_scale = sc.data_ptr(), sc.data_ptr() + 4
    a.dgi_max, a.dgh_max = mx.data_ptr(), mx.data_ptr() + 4
    L.check(L.lib().gm_lnlstm_cell_bwd(C.byref(a), L.stream_ptr()))
    assert L.last_kernel() == "k_lnlstm_cell_bwd"
    H4 = 4 * H
    errs = {"dgi": TTS._rel(dgi[:m, :H4], want[0].cuda()), "dgh": TTS._rel(dgh[:m, :H4], want[1].cuda()),
            "dc": TTS._rel(dco[:m, :H], want[2].cuda())}
    ps = part.sum(0)
    for name, got, ref in (("ln_in_w", ps[:H4], want[3]), ("ln_hid_w", ps[H4:2 * H4], want[5]),
                           ("bias", ps[2 * H4:3 * H4], want[7]), ("ln_in_b", ps[2 * H4:3 * H4], want[4]),
                           ("ln_hid_b", ps[2 * H4:3 * H4], want[6]), ("ln_cell_w", ps[3 * H4:3 * H4 + H], want[8]),
                           ("ln_cell_b", ps[3 * H4 + H:], want[9])):
        errs[name] = TTS._rel(got, ref.cuda())
    print("rel err vs fp64:", errs)
    for name, e in errs.items():
        assert e < 1e-5, (name, e)
    for buf, w in ((dgi, H4), (dgh, H4), (dco, H)):
        assert torch.isnan(buf[:m, w:]).all() and torch.isnan(buf[m]).all()
    for k, buf in enumerate((dgi, dgh)):
        dg = buf[:m, :H4].contiguous()
        assert mx[k].item() == dg.abs().max().item()
        e = torch.empty(1, device="cuda")
        L.check(FU._setup().gm_absmax_scale(dg.data_ptr(), dg.numel(), e.data_ptr(), L.stream_ptr()))
        assert sc[k].item() == e.item()
    assert mx[0].item() != mx[1].item()
    del hold


@pytest.mark.parametrize("srcs", ["both", "h", "c"])
@pytest.mark.parametrize("m,H", SHAPES)
def test_lnlstm_cell_bwd_bit_equal_to_lnlstm_bwd(m, H, srcs):
    """Only dh0 and / or dc given, the same inputs and rows per wave: dgi, dgh, dc_out and the partials are
    gm_lnlstm_bwd's bit for bit (the two kernels share the row math)."""
    L = _lib()
    leaves = _inputs(m, H, m + H)
    a, (gi, gh, hc, ps, stats, _) = _device_cell(L, leaves, m, H)
    dh = torch.randn(m, H, device="cuda") if srcs != "c" else None
    dc = torch.randn(m, H, device="cuda") if srcs != "h" else None
    nw = (m + RPW - 1) // RPW
    r_dgi, r_dgh = torch.empty(m, 4 * H, device="cuda"), torch.empty(m, 4 * H, device="cuda")
    r_dc, r_part = torch.empty(m, H, device="cuda"), torch.empty(nw, 14 * H, device="cuda")
    L.check(L.lib().gm_lnlstm_bwd(gi.data_ptr(), 4 * H, gh.data_ptr(), 4 * H, hc.data_ptr() + 4 * H, 2 * H,
                                  *(p.data_ptr() for p in ps), stats.data_ptr(), L.ptr(dh), H, L.ptr(dc), H, m, H, RPW,
                                  r_dgi.data_ptr(), 4 * H, r_dgh.data_ptr(), 4 * H, r_dc.data_ptr(), H,
                                  r_part.data_ptr(), L.stream_ptr()))
    dgi, dgh, dco = _outputs(a, m, H, 4)
    a.dc_out, a.ld_dco = dco.data_ptr(), dco.stride(0)
    part = torch.empty(nw, 14 * H, device="cuda")
    a.part = part.data_ptr()
    if dh is not None:
        a.dh0, a.ld_dh0 = dh.data_ptr(), H
    if dc is not None:
        a.dc, a.ld_dc = dc.data_ptr(), H
    L.check(L.lib().gm_lnlstm_cell_bwd(C.byref(a), L.stream_ptr()))
    assert torch.equal(dgi[:m, :4 * H], r_dgi) and torch.equal(dgh[:m, :4 * H], r_dgh)
    assert torch.equal(dco[:m, :H], r_dc)
    assert torch.equal(part, r_part)


def test_lnlstm_cell_bwd_optional_pointers_null():
    """No source at all: zero gate gradients. dh0 alone and no optional output: the call succeeds and gives
    gm_lnlstm_bwd's gate gradients."""
    L = _lib()
    m, H = 130, 64
    leaves = _inputs(m, H, 5)
    a, (gi, gh, hc, ps, stats, _) = _device_cell(L, leaves, m, H)
    dgi, dgh, _ = _outputs(a, m, H, 0)
    L.check(L.lib().gm_lnlstm_cell_bwd(C.byref(a), L.stream_ptr()))
    assert torch.equal(dgi[:m], torch.zeros_like(dgi[:m])) and torch.equal(dgh[:m], torch.zeros_like(dgh[:m]))
    assert torch.isnan(dgi[m]).all() and torch.isnan(dgh[m]).all()
    dh = torch.randn(m, H, device="cuda")
    a.dh0, a.ld_dh0 = dh.data_ptr(), H
    L.check(L.lib().gm_lnlstm_cell_bwd(C.byref(a), L.stream_ptr()))
    r_dgi, r_dgh = torch.empty(m, 4 * H, device="cuda"), torch.empty(m, 4 * H, device="cuda")
    r_dc, r_part = torch.empty(m, H, device="cuda"), torch.empty((m + RPW - 1) // RPW, 14 * H, device="cuda")
    L.check(L.lib().gm_lnlstm_bwd(gi.data_ptr(), 4 * H, gh.data_ptr(), 4 * H, hc.data_ptr() + 4 * H, 2 * H,
                                  *(p.data_ptr() for p in ps), stats.data_ptr(), dh.data_ptr(), H, None, H, m, H, RPW,
                                  r_dgi.data_ptr(), 4 * H, r_dgh.data_ptr(), 4 * H, r_dc.data_ptr(), H,
                                  r_part.data_ptr(), L.stream_ptr()))
    assert torch.equal(dgi[:m], r_dgi) and torch.equal(dgh[:m], r_dgh)


@pytest.mark.parametrize("H", [544, 1024])
def test_lnlstm_cell_bwd_rejects_other_hidden_sizes(H):
    """H > 512: GM_ERR_UNSUPPORTED through gm_fail, nothing launched."""
    L = _lib()
    m = 8
    gi, gh = torch.randn(m, 4 * H, device="cuda"), torch.randn(m, 4 * H, device="cuda")
    hc = torch.randn(m, 2 * H, device="cuda")
    ps = [torch.ones(n, device="cuda") for n in (4 * H,) * 5 + (H, H)]
    stats = torch.ones(m, 8, device="cuda")
    dg = torch.full((2, m, 4 * H), float("nan"), device="cuda")
    dh = torch.randn(m, H, device="cuda")
    a = L.LNLSTMBwdArgs()
    a.gi, a.ld_gi, a.gh, a.ld_gh = gi.data_ptr(), 4 * H, gh.data_ptr(), 4 * H
    a.c_in, a.ld_cin = hc.data_ptr() + 4 * H, 2 * H
    (a.ln_in_w, a.ln_in_b, a.ln_hid_w, a.ln_hid_b, a.bias, a.ln_cell_w, a.ln_cell_b) = (p.data_ptr() for p in ps)
    a.eps, a.stats, a.m, a.hidden = 1e-5, stats.data_ptr(), m, H
    a.dh0, a.ld_dh0 = dh.data_ptr(), H
    a.dgi, a.ld_dgi, a.dgh, a.ld_dgh = dg[0].data_ptr(), 4 * H, dg[1].data_ptr(), 4 * H
    assert L.lib().gm_lnlstm_cell_bwd(C.byref(a), L.stream_ptr()) == -5
    assert b"gm_lnlstm_cell_bwd" in L.lib().gm_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dg).all()


def test_lnlstm_seq_update_matches_reference_golden():
    """train_lnlstm.npz (lnlstm, mean, K = 2, 4 graphs) through seq_loss + check_update: seq_ok asserted first,
    then the LSTM golden test's body with its tolerances."""
    import numpy as np

    import golden_update as GU
    M = TTS.mods()[0]
    g = np.load(f"{TTS.R.GOLDEN}/train_lnlstm.npz")
    assert GU.arch(g)[0] == "lnlstm"
    netmon, model, target, _ = GU.build(g, M, torch.device("cuda"))
    assert TTS.mods()[2].seq_ok(netmon, model, target)
    TTS.test_seq_update_matches_reference_golden("train_lnlstm.npz")


def _compare_paths_q_bound(M, T, S, L, netmon, model, target, batches, seq, params, kink_tolerant=False):
    """TTS._compare_paths with the q / target bound computed in-test: the larger of its 2e-5 and twice the measured
    |q(autograd, x3) - q(autograd, exact fp32)| (both from the per-step autograd path). The loss and gradient
    bounds are _compare_paths' own."""
    l0, q0, t0 = T.dqn_loss(netmon, model, target, batches, 0.98, consecutive=True)
    for p in params:
        p.grad = None
    l0.backward()
    g0 = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    netmon.state = None
    l1, q1, t1 = S.seq_loss(netmon, model, target, seq, 0.98, params)
    l1.backward()
    g1 = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    netmon.state = None
    old = L.GEMM_MODE
    L.GEMM_MODE = "f32"
    try:
        lf, qf, tf = T.dqn_loss(netmon, model, target, batches, 0.98, consecutive=True)
        lf.backward()
    finally:
        L.GEMM_MODE = old
    gf = [p.grad.clone() for p in params]
    drift_q = max(float((q0[t].detach() - qf[t].detach()).abs().max()) for t in range(8))
    drift_t = max(float((t0[t] - tf[t]).abs().max()) for t in range(8))
    new_q = max(float((q1[t].detach() - q0[t].detach()).abs().max()) for t in range(8))
    new_t = max(float((t1[t] - t0[t]).abs().max()) for t in range(8))
    print(f"max |q(autograd x3) - q(autograd f32)| = {drift_q:.3e} (targets {drift_t:.3e}); "
          f"max |q(seq) - q(autograd x3)| = {new_q:.3e} (targets {new_t:.3e})")
    assert new_q <= max(2e-5, 2 * drift_q) and new_t <= max(2e-5, 2 * drift_t)
    torch.testing.assert_close(l1, l0.detach(), rtol=1e-5, atol=1e-8)
    errs = {}
    for (n, _), a, b, c in zip(list(model.named_parameters()) + list(netmon.named_parameters()), g0, g1, gf):
        errs[n] = (TTS._fro(a, c), TTS._fro(b, c))
    print("Frobenius-relative gradient error vs exact fp32 (autograd x3, sequence-batched x3):", errs)
    for n, (e_old, e_new) in errs.items():
        assert e_new < (max(1e-3, 4 * e_old) if kink_tolerant else max(2e-5, 2 * e_old)), (n, e_old, e_new)


@pytest.mark.parametrize("K,agg,tiles", [(1, "sum", "common"), (2, "mean", "common"), (1, "sum", "default")])
def test_lnlstm_seq_update_matches_autograd_path_on_rollout(K, agg, tiles, monkeypatch):
    """test_seq_update_matches_autograd_path_on_rollout (64 envs x 30 steps, 512 sequences x 8) with every NetMon
    it builds an lnlstm one. Gradients and loss: _compare_paths' own bounds. q / targets: _compare_paths_q_bound.
    Measured on an MI355X: max |q(autograd, x3) - q(autograd, exact fp32)| = 2.5e-7 / 3.9e-7 / 2.7e-7 for the three
    cases (targets 2.8e-7 / 6.6e-7 / 3.1e-7) and max |q(seq) - q(autograd, x3)| = 1.1e-7 / 1.3e-7 / 1.2e-7, so the
    bound in force is _compare_paths' 2e-5: the carried LN-LSTM state does not drift visibly over 8 steps."""
    M, T, S, FU, L = TTS.mods()
    made = []
    orig = M.NetMon

    def lnl_netmon(*a, **kw):
        made.append(orig(*a, rnn_type="lnlstm", **kw))
        return made[-1]

    monkeypatch.setattr(M, "NetMon", lnl_netmon)
    monkeypatch.setattr(TTS, "_compare_paths", _compare_paths_q_bound)
    TTS.test_seq_update_matches_autograd_path_on_rollout(K, agg, tiles)
    assert len(made) == 1 and made[0].rnn_type == "lnlstm" and made[0].state_size == 256
    model = M.DQN(6 * 20 + 10 + 512, [512, 256], 4).cuda()
    assert S.seq_ok(made[0], model, model)


def _lnl_sl_args(*a, **kw):
    ns = TSL._args(*a, **kw)
    ns.netmon_rnn_type = "lnlstm"
    return ns


@pytest.mark.parametrize("K,agg,steps", [(1, "sum", 4), (2, "mean", 3), (1, "sum", 1)])
def test_lnlstm_sl_seq_matches_autograd_path(K, agg, steps):
    """Config 5's unroll with LN-LSTM cells: test_sl_seq_matches_autograd_path's small case (its loss and gradient
    bounds) on lnlstm NetMonSL models; seq_ok accepts them with and without rows / steps. Predictions: the larger
    of its 2e-5 and twice the measured |pred(autograd, x3) - pred(autograd, exact fp32)| (measured on an MI355X:
    1.5e-6 / 1.7e-6 / 8.9e-7, and the unroll's predictions equal to the autograd path's bit for bit, so the bound
    in force is 2e-5). seq_bytes equals the bytes of the tensors the plan keeps."""
    SL, M = TSL._mods()
    L = _lib()
    n, H, B = 20, 128, 256
    models = []
    for _ in range(3):
        torch.manual_seed(3)
        models.append(SL.NetMonSL(_lnl_sl_args(n, H, "512,256", K, agg), 4 * n + 8, 4, n).cuda())
    a, b, f = models
    assert b.netmon.rnn_type == "lnlstm" and SL.SQ.seq_ok(b.netmon)
    assert SL.SQ.seq_ok(b.netmon, rows=B * n, steps=steps)
    data = SL.build_dataset(n, 20, B, 7)
    x, nbr, tgt = data.node_obs, data.nbr, data.targets_all

    def autograd_path(mod):
        mod.netmon.state = None
        enc = mod.netmon.encode_nodes(x, nbr)
        seq, preds = [], []
        for _ in range(steps):
            _, _, pa = mod(x, nbr, enc)
            preds.append(pa.detach())
            seq.append(torch.nn.functional.mse_loss(pa, tgt))
        la = torch.mean(torch.stack(seq))
        la.backward()
        return preds, la

    preds, la = autograd_path(a)
    old = L.GEMM_MODE
    L.GEMM_MODE = "f32"
    try:
        preds_f, _ = autograd_path(f)
    finally:
        L.GEMM_MODE = old
    plans = []
    orig_bwd = SL.SQ._backward_lnl

    def keep_plan(p, dR):
        plans.append(p)
        return orig_bwd(p, dR)

    SL.SQ._backward_lnl = keep_plan
    try:
        b.netmon.state = None
        pb = b.forward_seq(x, nbr, steps)
        lb = (pb - tgt).pow(2).mean(dim=(1, 2, 3)).mean()
        lb.backward()
    finally:
        SL.SQ._backward_lnl = orig_bwd
    kept = sum(t.numel() * t.element_size() for t in SL.SQ.kept_lnl(plans[0]))
    assert SL.SQ.seq_bytes(b.netmon, B * n, steps) == kept
    drift = max(float((preds[t] - preds_f[t]).abs().max()) for t in range(steps))
    new = max(float((pb[t].detach() - preds[t]).abs().max()) for t in range(steps))
    print(f"max |pred(autograd x3) - pred(autograd f32)| = {drift:.3e}; max |pred(seq) - pred(autograd x3)| = {new:.3e}")
    assert new <= max(2e-5, 2 * drift)
    torch.testing.assert_close(lb, la, atol=0, rtol=1e-5)
    pa_, pb_ = dict(a.named_parameters()), dict(b.named_parameters())
    for s, p in pa_.items():
        if s.startswith("linear.") or s.startswith("linear_reg."):
            continue
        ga, gb = p.grad, pb_[s].grad
        scale = float(ga.abs().max()) + 1e-12
        err = float((ga - gb).abs().max()) / scale
        assert err < 2e-4, (s, err)
