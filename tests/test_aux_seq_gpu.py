"""The NetMon aux loss on the sequence-batched DQN + NetMon update (graph-marl_amd/train_seq.py, --aux-loss-coeff):
gm_aux_head_mse / gm_aux_head_mse_bwd against fp64 (tests/aux_util.py), the update against the reference's golden
(tests/golden/train_aux.npz) and against the per-step autograd path on a replayed rollout, the sampler's node_aux,
the predicate, and main.py's dispatch."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import aux_util as U
import golden_replay as R

pytestmark = pytest.mark.gpu

GM_ERR_INVALID_ARG = -1  # include/graph_marl_amd.h


def _operands(rows, cols, n_out, seed):
    torch.manual_seed(seed)
    y = torch.randn(rows, cols, device="cuda")
    y[0, : min(cols, 7)] = 0.0  # exact zeros take the slope
    w2 = torch.randn(n_out, cols, device="cuda") / cols ** 0.5
    b2 = torch.randn(n_out, device="cuda")
    tgt = 3 * torch.rand(rows, n_out, device="cuda")
    return y, w2, b2, tgt


def _run_fwd(L, yb, ldy, rows, cols, wb, ldw, b2, n_out, tb, ldt, rb, ldr, part, rpb, ra, ya):
    return L.lib().gm_aux_head_mse(yb.data_ptr(), ldy, rows, cols, wb.data_ptr(), ldw, b2.data_ptr(), n_out,
                                   tb.data_ptr(), ldt, rb.data_ptr(), ldr, part.data_ptr(), rpb,
                                   None if ra is None else ra.data_ptr(), None if ya is None else ya.data_ptr(),
                                   L.stream_ptr())


# rows x cols x n_out x rows_per_block: every rows / cols / n_out of the contract's edges, rows below, at and above a
# block, rows no multiple of rows_per_block, more than one block, 1024 x 128 together
FWD_CASES = [(1, 32, 4, 64), (63, 64, 20, 64), (64, 64, 50, 64), (65, 256, 20, 64), (257, 256, 128, 64),
             (257, 1024, 128, 64), (65, 1024, 4, 8), (63, 32, 128, 16), (1, 1024, 50, 8), (64, 256, 20, 24),
             (257, 64, 4, 40), (65, 32, 50, 56)]


@pytest.mark.parametrize("rows,cols,n_out,rpb", FWD_CASES)
def test_aux_head_mse_vs_fp64(rows, cols, n_out, rpb):
    """res, the block partials' sum and the two published maxima of gm_aux_head_mse within the derived bounds of
    aux_util.fwd_ref / loss_bound; strided operands with NaN padding and guard rows, which stay bitwise untouched;
    a second run gives the same bits."""
    L = U.mods()[-1]
    y, w2, b2, tgt = _operands(rows, cols, n_out, rows + cols + n_out)
    ldy, ldw, ldt, ldr = cols + 4, cols + 8, n_out + 3, n_out + 1
    yb, _ = U.strided(y, ldy)
    wb, _ = U.strided(w2, ldw)
    tb, _ = U.strided(tgt, ldt)
    nb = (rows + rpb - 1) // rpb
    outs = []
    for _ in range(2):
        rb = torch.full((rows + U.GUARD, ldr), float("nan"), device="cuda")
        before = rb.clone()
        part = torch.full((nb + 1,), float("nan"), device="cuda")
        ra, ya = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        L.check(_run_fwd(L, yb, ldy, rows, cols, wb, ldw, b2, n_out, tb, ldt, rb, ldr, part, rpb, ra, ya))
        assert U.untouched(rb, before, rows, n_out)
        assert torch.isnan(part[nb]) and torch.isfinite(part[:nb]).all()
        outs.append((rb[:rows, :n_out].clone(), part[:nb].clone(), ra.clone(), ya.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    res, part, ra, ya = outs[0]
    ref, eb = U.fwd_ref(y, w2, b2, tgt)
    r_el = ((res.double() - ref).abs() / eb).max().item()
    got = part.sum().item()  # the caller's fp32 sum over the blocks (counted in loss_terms)
    lb = U.loss_bound(ref, eb, U.loss_terms(rows, n_out, rpb))
    r_loss = abs(got - (ref ** 2).sum().item()) / lb
    print(f"worst error / bound: res {r_el:.3g}, sum res^2 {r_loss:.3g}")
    assert r_el <= 1
    assert r_loss <= 1
    assert ra.item() == res.abs().max().item() and ya.item() == y.abs().max().item()  # the maxima's float bits
    L.check(U.mods()[2]._setup().gm_absmax_finish(ra.data_ptr(), L.stream_ptr()))  # fused._setup: its argtypes
    assert ra.item() == U.expected_scale(res.abs().max().item())


BWD_CASES = [(1, 32, 4, 64, 1, 1.0), (63, 64, 20, 64, 1, 2.0 ** -10), (64, 64, 50, 64, 0, 3.7e-4),
             (65, 256, 20, 64, 1, 3.7e-4), (257, 256, 128, 64, 1, 1.0), (257, 1024, 128, 64, 1, 2.0 ** -10),
             (65, 1024, 4, 8, 0, 1.0), (63, 32, 128, 16, 1, 3.7e-4), (1, 1024, 50, 8, 1, 1.0),
             (64, 96, 20, 24, 1, 2.0 ** -10), (257, 64, 4, 40, 0, 2.0 ** -10), (65, 32, 50, 56, 1, 1.0)]


@pytest.mark.parametrize("rows,cols,n_out,rpb,act,scale", BWD_CASES)
def test_aux_head_mse_bwd_vs_fp64_autograd(rows, cols, n_out, rpb, act, scale):
    """g, the two bias partials' sums and the published scale of gm_aux_head_mse_bwd against fp64 autograd
    (aux_util.bwd_ref), some y exactly 0 and about half negative; the scale split between the host factor and the
    device factor. (W2's gradient on the split-f16 route: test_head_weight_gradients_on_the_wgrad_gemm.)"""
    gm, M, FU, W, T, S, RB, L = U.mods()
    z, w2, b2, tgt = _operands(rows, cols, n_out, rows + cols + n_out + act)
    res = torch.randn(rows, n_out, device="cuda")
    ldr, ldw, ldg = n_out + 1, cols + 8, cols + 4
    rb, _ = U.strided(res, ldr)
    wb, _ = U.strided(w2, ldw)
    bits = U.pack_bits(z > 0)
    nb = (rows + rpb - 1) // rpb
    gb = torch.full((rows + U.GUARD, ldg), float("nan"), device="cuda")
    before = gb.clone()
    pb1, pb2 = torch.empty(nb, cols, device="cuda"), torch.empty(nb, n_out, device="cuda")
    sc = torch.empty(1, device="cuda")
    up = torch.full((1,), 0.5, device="cuda")
    L.check(L.lib().gm_aux_head_mse_bwd(rb.data_ptr(), ldr, n_out, wb.data_ptr(), ldw, bits.data_ptr(), bits.stride(0),
                                        act, rows, cols, 2 * scale, up.data_ptr(), gb.data_ptr(), ldg, pb1.data_ptr(),
                                        pb2.data_ptr(), rpb, sc.data_ptr(), L.stream_ptr()))
    assert U.untouched(gb, before, rows, cols)
    g = gb[:rows, :cols]
    s = float(np.float32(2 * scale) * np.float32(0.5))
    ref_g, ref_b2, ref_w2, bound = U.bwd_ref(res, w2, z, act, s)
    tiny = 1e-45  # a row of zero bound (no such row here) would still compare
    r_g = ((g.double() - ref_g).abs() / (bound + tiny)).max().item()
    # column sums: every element's bound, plus rows additions of up to rows * 2^-24 of the absolute sum
    b1_bound = bound.sum(0) + (rows + 1) * U.U24 * ref_g.abs().sum(0)
    r_b1 = ((pb1.double().sum(0) - ref_g.sum(0)).abs() / (b1_bound + tiny)).max().item()
    b2_bound = (rows + 3) * U.U24 * abs(s) * res.double().abs().sum(0)
    r_b2 = ((pb2.double().sum(0) - ref_b2).abs() / (b2_bound + tiny)).max().item()
    print(f"worst error / bound: g {r_g:.3g}, bias 1 {r_b1:.3g}, bias 2 {r_b2:.3g}")
    assert r_g <= 1 and r_b1 <= 1 and r_b2 <= 1
    assert sc.item() == U.expected_scale(g.abs().max().item())


def test_head_weight_gradients_on_the_wgrad_gemm():
    """Both weight gradients of the head on the route the update ships at training sizes, gm_gemm_x3_wgrad (taken by
    model._wgrad from 4096 batch rows on), with the operand scales the head's own kernels publish, exactly as
    _forward_aux / _backward_aux chain them: rows = 4160 (65 blocks), cols = 256, n_out = 20. Layer 1's GEMM
    publishes max |x|, gm_aux_head_mse max |res| and max |y|, gm_aux_head_mse_bwd the scale of g; then W2's gradient
    s res^T y and W1's g^T x against fp64 of the same fp32 operands within aux_util.wgrad_bound. The test fails if
    either call leaves the GEMM kernel (gm_last_kernel)."""
    gm, M, FU, W, T, S, RB, L = U.mods()
    rows, cols, n_out = 4160, 256, 20
    torch.manual_seed(rows)
    x = torch.randn(rows, cols, device="cuda")
    l1 = M.Linear(cols, cols, act=1).cuda()
    w2 = torch.randn(n_out, cols, device="cuda") / cols ** 0.5
    b2 = torch.randn(n_out, device="cuda")
    tgt = 3 * torch.rand(rows, n_out, device="cuda")
    y, yb = torch.empty(rows, cols, device="cuda"), S._sign_bits(rows, cols, "cuda")
    sx, sr, sy = (torch.zeros(1, device="cuda") for _ in range(3))
    S._gemm_amax(x, cols, cols, S._lin_x3(l1), l1.bias, rows, cols, FU.GM_EPI_BIAS_LEAKY, y, cols, sx, sbits=yb)
    S._finish(sx)
    res = torch.empty(rows, n_out, device="cuda")
    nb = (rows + S.AUX_RPB - 1) // S.AUX_RPB
    part = torch.empty(nb, device="cuda")
    L.check(_run_fwd(L, y, cols, rows, cols, w2, cols, b2, n_out, tgt, n_out, res, n_out, part, S.AUX_RPB, sr, sy))
    assert sr.item() == res.abs().max().item() and sy.item() == y.abs().max().item()
    S._finish(sr)
    S._finish(sy)
    assert sr.item() == U.expected_scale(res.abs().max().item()) and sy.item() == U.expected_scale(y.abs().max().item())
    assert sx.item() == U.expected_scale(x.abs().max().item())
    g = torch.empty(rows, cols, device="cuda")
    pb1, pb2 = torch.empty(nb, cols, device="cuda"), torch.empty(nb, n_out, device="cuda")
    sc = torch.empty(1, device="cuda")
    scale = 2.0 / (rows * n_out)
    L.check(L.lib().gm_aux_head_mse_bwd(res.data_ptr(), n_out, n_out, w2.data_ptr(), cols, yb.data_ptr(), yb.stride(0),
                                        1, rows, cols, scale, None, g.data_ptr(), cols, pb1.data_ptr(), pb2.data_ptr(),
                                        S.AUX_RPB, sc.data_ptr(), L.stream_ptr()))
    assert sc.item() == U.expected_scale(g.abs().max().item())
    s = float(np.float32(scale))
    for name, a, sa, b, sb, mul in (("W2", res, sr, y, sy, s), ("W1", g, sc, x, sx, 1.0)):
        gw = S._wgrad(a, sa, b, cols, sb)
        assert "wgrad" in L.last_kernel(), (name, L.last_kernel())  # the GEMM kernel, not the library fallback
        ref = mul * (a.double().t() @ b.double())
        bound = abs(mul) * U.wgrad_bound(a, b)
        r = ((mul * gw.double() - ref).abs() / bound).max().item()
        fro = (mul * gw.double() - ref).norm().item() / ref.norm().item()
        print(f"{name} gradient on gm_gemm_x3_wgrad: worst error / bound {r:.3g}, Frobenius-relative {fro:.3g}")
        assert r <= 1, name


def test_aux_head_argument_contract():
    """n_out = 129, cols = 1056 and a misaligned y / w2 base each return an error from both entry points and write
    nothing."""
    L = U.mods()[-1]
    rows = 16
    y = torch.randn(rows + 1, 1056 + 4, device="cuda")
    w2 = torch.randn(130, 1056 + 4, device="cuda")
    b2, tgt = torch.randn(130, device="cuda"), torch.randn(rows, 130, device="cuda")
    bits = torch.zeros(rows, 40, dtype=torch.int32, device="cuda")
    ldy = y.stride(0)

    def fwd(n_out, cols, ybase):
        res = torch.full((rows, 130), float("nan"), device="cuda")
        part = torch.full((4,), float("nan"), device="cuda")
        am = torch.zeros(2, device="cuda")
        rc = L.lib().gm_aux_head_mse(ybase, ldy, rows, cols, w2.data_ptr(), ldy, b2.data_ptr(), n_out, tgt.data_ptr(),
                                     130, res.data_ptr(), 130, part.data_ptr(), 64, am.data_ptr(),
                                     am.data_ptr() + 4, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, torch.isnan(res).all().item() and torch.isnan(part).all().item() and (am == 0).all().item()

    def bwd(n_out, cols, wbase, with_scale=True):
        g = torch.full((rows, ldy), float("nan"), device="cuda")
        p1, p2 = torch.full((1, ldy), float("nan"), device="cuda"), torch.full((1, 130), float("nan"), device="cuda")
        sc = torch.full((1,), float("nan"), device="cuda")
        rc = L.lib().gm_aux_head_mse_bwd(tgt.data_ptr(), 130, n_out, wbase, ldy, bits.data_ptr(), 40, 1, rows, cols,
                                         1.0, None, g.data_ptr(), ldy, p1.data_ptr(), p2.data_ptr(), 64,
                                         sc.data_ptr() if with_scale else None, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, all(torch.isnan(t).all().item() for t in (g, p1, p2, sc))

    assert fwd(20, 256, y.data_ptr()) == (0, False)  # the good call writes
    assert bwd(20, 256, w2.data_ptr()) == (0, False)
    for n_out, cols, off in ((129, 256, 0), (20, 1056, 0), (20, 256, 4)):
        rc, clean = fwd(n_out, cols, y.data_ptr() + off)
        assert rc == GM_ERR_INVALID_ARG and clean, ("fwd", n_out, cols, off)
        rc, clean = bwd(n_out, cols, w2.data_ptr() + off)
        assert rc == GM_ERR_INVALID_ARG and clean, ("bwd", n_out, cols, off)
    assert fwd(20, 256, y.data_ptr())[0] == 0  # a refused call leaves the library usable
    assert L.last_kernel() == "k_aux_head_mse"
    assert bwd(20, 256, w2.data_ptr(), with_scale=False)[0] == 0
    assert L.last_kernel() == "k_aux_head_mse_bwd"


def test_seq_update_with_aux_matches_reference_golden():
    """tests/golden/train_aux.npz (--aux-loss-coeff 0.3) through seq_loss: loss_aux at rtol 1e-5 / atol 1e-6, q,
    targets, loss, raw and clipped gradients (the aux head's included), AdamW step and soft update at
    test_train_gpu.check_update's tolerances, the bounds the per-step path meets on this file."""
    gm, M, FU, W, T, S, RB, L = U.mods()
    import golden_update as GU
    from test_train_gpu import check_update
    from test_train_seq_gpu import _golden_seq
    g = np.load(f"{R.GOLDEN}/train_aux.npz")
    dev = torch.device("cuda")
    netmon, model, target, state0 = GU.build(g, M, dev)
    Sz = netmon.get_state_size()
    aux_model = M.MLP(Sz, [Sz, g["node_aux"].shape[-1]], activation_on_output=False).to(dev)
    aux_model.load_state_dict(GU._sd(g, "aux_"))
    assert S.seq_ok(netmon, model, target, 0.0, aux_model)
    Lq = g["actions"].shape[0]
    seq = _golden_seq(g, dev, netmon, RB, state0)._replace(
        node_aux=torch.as_tensor(g["node_aux"][:Lq], device=dev).float().contiguous())
    params = list(model.parameters()) + list(netmon.parameters()) + list(aux_model.parameters())
    names = ([f"model_{k}" for k, _ in model.named_parameters()] + [f"netmon_{k}" for k, _ in netmon.named_parameters()]
             + [f"aux_{k}" for k, _ in aux_model.named_parameters()])
    assert names == list(g["param_names"])
    opt = torch.optim.AdamW(params, lr=float(g["lr"]))
    netmon.train()
    model.train()
    parts = {}
    loss, q, qt = S.seq_loss(netmon, model, target, seq, float(g["gamma"]), params, parts, aux_model,
                             float(g["aux_coeff"]))
    np.testing.assert_allclose(parts["loss_aux"].item(), g["loss_aux"].item(), rtol=1e-5, atol=1e-6)
    for t in range(Lq):
        np.testing.assert_allclose(q[t].detach().cpu().numpy(), g[f"q_{t}"], atol=1e-5, rtol=0, err_msg=f"q_{t}")
        np.testing.assert_allclose(qt[t].cpu().numpy(), g[f"qtarget_{t}"], atol=1e-5, rtol=0, err_msg=f"qt_{t}")
    np.testing.assert_allclose(loss.item(), g["loss"].item(), rtol=1e-5, atol=1e-6)
    opt.zero_grad()
    loss.backward()
    check_update(g, names, params, opt, model, target, T)


def _fro(a, b):
    return (a.double() - b.double()).norm().item() / max(b.double().norm().item(), 1e-30)


def _grads(params, loss):
    for p in params:
        p.grad = None
    loss.backward()
    return [p.grad.clone() for p in params]


# the last case draws 144 sequences (with replacement) from the same ring: L*B*N = 4320 head rows, past the 4096
# rows from which model._wgrad runs gm_gemm_x3_wgrad, so the aux_* (and every other) weight gradient of the batched
# path is judged on the split-f16 weight-gradient GEMM; the other cases draw 16
PARITY = [("lstm", 1, "sum", False, 16), ("gru", 1, "sum", False, 16), ("lnlstm", 1, "sum", False, 16),
          ("lstm", 2, "mean", False, 16), ("gru", 2, "mean", False, 16), ("lnlstm", 2, "mean", False, 16),
          ("lstm", 1, "sum", True, 16), ("lstm", 1, "sum", False, 144)]


@pytest.mark.parametrize("rnn,K,agg,glob,n_seq", PARITY)
def test_seq_aux_matches_per_step_path_on_rollout(rnn, K, agg, glob, n_seq):
    """A replayed rollout (8 envs x 12 steps, episodes of 5 steps, N = A = 10, H = 32, encoder (32,), L = 3): the
    same sampled sequences through train.dqn_loss with the aux model and through seq_loss, both on the common GEMM
    tile. The criterion of test_train_seq_gpu._compare_paths: q and targets within atol 2e-5, loss and loss_aux
    within rtol 1e-5, every gradient's Frobenius error against the exact-fp32 autograd run below max(2e-5, twice
    the per-step path's own)."""
    gm, M, FU, W, T, S, RB, L = U.mods()
    netmon, model, target, aux_model, rb, params = U.replayed_aux(rnn, K, agg, glob)
    assert S.seq_ok(netmon, model, target, 0.0, aux_model)
    batches, seq = U.sample(rb, n_seq, 3)
    assert seq.episode_done[:-1].any()  # an episode end before a sequence's last step
    coeff = 0.3
    lib = FU._setup()
    lib.gm_gemm_set_tile(0)
    try:
        p0, p1 = {}, {}
        netmon.state = None
        l0, q0, t0 = T.dqn_loss(netmon, model, target, batches, 0.98, aux_model=aux_model, aux_coeff=coeff, parts=p0,
                                consecutive=True)
        g0 = _grads(params, l0)
        netmon.state = None
        l1, q1, t1 = S.seq_loss(netmon, model, target, seq, 0.98, params, p1, aux_model, coeff)
        g1 = _grads(params, l1)
        netmon.state = None
        old = L.GEMM_MODE
        L.GEMM_MODE = "f32"  # exact-fp32 reference: the per-step path with every GEMM in fp32
        try:
            lf, _, _ = T.dqn_loss(netmon, model, target, batches, 0.98, aux_model=aux_model, aux_coeff=coeff,
                                  consecutive=True)
            gf = _grads(params, lf)
        finally:
            L.GEMM_MODE = old
    finally:
        lib.gm_gemm_set_tile(-1)
        netmon.state = None
    for t in range(3):
        torch.testing.assert_close(q1[t], q0[t].detach(), rtol=0, atol=2e-5)
        torch.testing.assert_close(t1[t], t0[t], rtol=0, atol=2e-5)
    torch.testing.assert_close(l1, l0.detach(), rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(p1["loss_aux"], p0["loss_aux"].detach(), rtol=1e-5, atol=1e-8)
    torch.testing.assert_close(p1["loss_q"], p0["loss_q"].detach(), rtol=1e-5, atol=1e-8)
    names = [n for m, pre in ((model, "model."), (netmon, "netmon."), (aux_model, "aux."))
             for n in (pre + k for k, _ in m.named_parameters())]
    fails = []
    for n, a, b, c in zip(names, g0, g1, gf):
        e_old, e_new = _fro(a, c), _fro(b, c)
        print(f"{n}: Frobenius-relative error vs exact fp32: per-step {e_old:.3g}, batched {e_new:.3g}")
        if not e_new < max(2e-5, 2 * e_old):
            fails.append((n, e_old, e_new))
    assert not fails, fails


def test_head_weight_gradients_get_their_operands_scales(monkeypatch):
    """The wiring the tolerances cannot see (a neighbouring power of two as scale costs a few bits, not the bound):
    inside _backward_aux every _wgrad call is handed, for each operand, exactly gm_absmax_scale's power of two of
    that operand's own maximum: W2's from the two maxima gm_aux_head_mse published, W1's from gm_aux_head_mse_bwd's
    scale of g and layer 1's forward-GEMM maximum of S[K]."""
    gm, M, FU, W, T, S, RB, L = U.mods()
    netmon, model, target, aux_model, rb, params = U.replayed_aux("lstm", 1)
    _, seq = U.sample(rb, 16, 3)
    calls, inside = [], []
    real_wgrad, real_bwd = S._wgrad, S._backward_aux

    def spy_wgrad(g, sa, x, k, sb):
        if inside:
            calls.append((g.abs().max().item(), sa.item(), x[:, :k].abs().max().item(), sb.item(), g.shape[1]))
        return real_wgrad(g, sa, x, k, sb)

    def spy_bwd(*a, **kw):
        inside.append(1)
        try:
            return real_bwd(*a, **kw)
        finally:
            inside.pop()

    monkeypatch.setattr(S, "_wgrad", spy_wgrad)
    monkeypatch.setattr(S, "_backward_aux", spy_bwd)
    loss, _, _ = S.seq_loss(netmon, model, target, seq, 0.98, params, {}, aux_model, 0.3)
    _grads(params, loss)
    assert sorted(c[4] for c in calls) == [U.N_S, 2 * U.H_S]  # W2's (n_aux columns of res) and W1's (S of g)
    for gmax, sa, xmax, sb, _ in calls:
        assert gmax > 0 and xmax > 0
        assert sa == U.expected_scale(gmax) and sb == U.expected_scale(xmax), (gmax, sa, xmax, sb)


def test_update_with_aux_is_bit_reproducible():
    """Two seq_loss + backward runs on the same sequences give the same loss and gradient bits."""
    gm, M, FU, W, T, S, RB, L = U.mods()
    netmon, model, target, aux_model, rb, params = U.replayed_aux("lstm", 1)
    _, seq = U.sample(rb, 16, 3)
    runs = []
    for _ in range(2):
        netmon.state = None
        parts = {}
        loss, _, _ = S.seq_loss(netmon, model, target, seq, 0.98, params, parts, aux_model, 0.3)
        runs.append([loss.detach().clone(), parts["loss_aux"].clone()] + _grads(params, loss))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_sampler_node_aux():
    """get_sequences after an rng restore draws get_batch's indices (aux_util.sample asserts it) and stacks its
    node_aux bit for bit; None when the ring stores none."""
    netmon, model, target, aux_model, rb, params = U.replayed_aux("lstm", 1)
    batches, seq = U.sample(rb, 16, 3)
    assert seq.node_aux.shape == (3, 16, U.N_S, U.N_S) and seq.node_aux.dtype == torch.float32
    for t, b in enumerate(batches):
        assert torch.equal(seq.node_aux[t], b.node_aux)
    assert (seq.node_aux.sum((-1, -2)) > 0).all()  # shortest-path distances, not an empty field
    rb2 = U.replayed_aux("lstm", 1, aux=False)[4]
    assert rb2.get_sequences(4, 3).node_aux is None


def test_predicates():
    """seq_ok with main.py's head on lstm / gru / lnlstm; not with a three-layer head, a tanh head, a head without
    bias, S = 2048 or GM_GEMM=f32; the DGN and agent predicates keep refusing an aux model."""
    gm, M, FU, W, T, S, RB, L = U.mods()
    DNS = importlib.import_module("graph-marl_amd.dgn_netmon_seq")
    ANS = importlib.import_module("graph-marl_amd.agent_netmon_seq")
    N, H = 20, 128

    def head(Sz, units=None, **kw):
        return M.MLP(Sz, units or [Sz, N], activation_on_output=False, **kw).cuda()

    D = 6 * N + 10 + 4 * H
    model, target = M.DQN(D, [512, 256], 4).cuda(), M.DQN(D, [512, 256], 4).cuda()
    for rnn in ("lstm", "gru", "lnlstm"):
        netmon = M.NetMon(4 * N + 8, H, [512, 256], 1, rnn_type=rnn).cuda()
        Sz = netmon.get_state_size()
        assert Sz == (H if rnn == "gru" else 2 * H)
        assert S.seq_ok(netmon, model, target, 0.0, head(Sz)), rnn
        assert S.seq_ok(netmon, model, target, 0.0, None), rnn
    netmon = M.NetMon(4 * N + 8, H, [512, 256], 1).cuda()
    Sz = 2 * H
    ok = lambda a: S.seq_ok(netmon, model, target, 0.0, a)  # noqa: E731
    assert not ok(head(Sz, [Sz, Sz, N]))  # three layers
    assert not ok(head(Sz, activation="tanh"))
    nb = head(Sz)
    nb.linear_layers[1].bias = None
    assert not ok(nb)
    assert not ok(head(Sz, [Sz // 2, N]))  # first layer not S -> S
    assert not ok(head(Sz, [Sz, 130]))  # n_aux > 128
    big = M.NetMon(4 * N + 8, 1024, [64], 1).cuda()  # S = 2048
    mb = M.DQN(6 * N + 10 + 4096, [64], 4).cuda()
    assert S.seq_ok(big, mb, mb) and not S.seq_ok(big, mb, mb, 0.0, head(2048))
    old = L.GEMM_MODE
    L.GEMM_MODE = "f32"
    try:
        assert not ok(head(Sz))
    finally:
        L.GEMM_MODE = old
    dgn, dgn_t = M.DGN(D, [512, 256], 4).cuda(), M.DGN(D, [512, 256], 4).cuda()
    assert not DNS.dgn_netmon_seq_ok(netmon, dgn, dgn_t, 0.03, head(Sz), N)
    dqnr, dqnr_t = M.DQNR(D, [512, 256], 4).cuda(), M.DQNR(D, [512, 256], 4).cuda()
    assert not ANS.agent_netmon_seq_ok(netmon, dqnr, dqnr_t, 0.0, head(Sz), N)


def test_cli_reaches_batched_update_with_aux(tmp_path, monkeypatch):
    """main.main with --aux-loss-coeff=0.5 --sequence-length=4 reaches dqn_update_seq with the aux model, and
    parts["loss_aux"] is a finite tensor."""
    gm, M, FU, W, T, S, RB, L = U.mods()
    main = importlib.import_module("graph-marl_amd.main")
    seen = []
    real = S.dqn_update_seq

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw.get("aux_model"), kw.get("aux_coeff"), kw["parts"]["loss_aux"].detach().clone(),
                     a[5].node_aux is not None))
        return out

    monkeypatch.setattr(S, "dqn_update_seq", spy)

    def no_per_step(*a, **kw):
        raise AssertionError("the per-step update ran")

    monkeypatch.setattr(T, "dqn_update", no_per_step)
    main.main(["--env-type=routing", "--model=dqn", "--netmon", "--netmon-iterations=1", "--n-env=8",
               "--episode-steps=20", "--total-steps=60", "--step-before-train=40", "--step-between-train=10",
               "--mini-batch-size=8", "--sequence-length=4", "--capacity=4000", "--aux-loss-coeff=0.5",
               "--eval-episodes=8", "--eval-episode-steps=5", "--disable-progressbar", f"--log-dir={tmp_path}"])
    assert len(seen) >= 2
    for aux_model, coeff, la, has in seen:
        assert isinstance(aux_model, M.MLP) and coeff == 0.5 and has
        assert la.dim() == 0 and torch.isfinite(la).item() and la.item() > 0


def test_no_aux_launches_unchanged():
    """With aux_model=None the update launches what tests/golden/train_seq_trace.json recorded. This restates
    test_agent_netmon_seq_gpu.test_dqn_netmon_update_launches_unchanged[lstm] beside the aux tests; it adds no case."""
    import dgn_netmon_util as DU
    with open(os.path.join(R.GOLDEN, "train_seq_trace.json")) as f:
        want = json.load(f)["lstm"]
    got = DU.dqn_update_trace("lstm")
    assert got["tags"] == want["tags"] and got["kernels"] == want["kernels"]
