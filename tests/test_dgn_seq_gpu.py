"""GPU tests of the batched DGN update (graph-marl_amd/dgn_seq.py): gm_agent_attention_bwd and gm_agent_attention_kl
against fp64 torch (the core of AttModel.forward and train.attention_kl), their refusals, the whole update against the
reference's golden DGN update (tests/golden/train_dgn.npz; src/main.py:840-1026), against the per-step autograd path
(train.dqn_loss) on transitions sampled from a replay buffer, and the dispatch predicate."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_replay as R

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED = -1, -5


def mods():
    return (importlib.import_module("graph-marl_amd.model"), importlib.import_module("graph-marl_amd.train"),
            importlib.import_module("graph-marl_amd.dgn_seq"), importlib.import_module("graph-marl_amd.replaybuffer"),
            importlib.import_module("graph-marl_amd._lib"))


# (B, A, heads, dk, dv); the last one runs the runtime-width kernels
CASES = [(2, 1, 8, 16, 16), (3, 3, 2, 16, 16), (5, 20, 8, 16, 16), (1, 64, 8, 16, 16), (2, 7, 3, 8, 24)]


def _adjacency(B, A, gen):
    """Random asymmetric int8 adjacency [B, A, A] with, per env, one all-zero row and one row adjacent only to itself
    (A = 1: the two kinds in different envs)."""
    adj = torch.rand(B, A, A, generator=gen) < 0.4
    if A >= 3:
        adj[:, 0] = False
        adj[:, 1] = False
        adj[:, 1, 1] = True
        assert not torch.equal(adj, adj.transpose(1, 2))
    else:
        adj[::2] = False
        adj[1::2] = True
    return adj.to(torch.int8).cuda()


def _case(B, A, nh, dk, dv, seed):
    """fp32 N(0, 1) q, k, v as the columns [v | k | q] of one padded qkv buffer (forward_rows' layout), the target
    model's buffer (perturbed rows), dout, adj and a row scale with zeros."""
    gen = torch.Generator().manual_seed(seed)
    M = B * A
    n = nh * (dv + 2 * dk)
    qkv = torch.randn(M, n + 4, generator=gen)
    tqkv = qkv + 0.7 * torch.randn(M, n + 4, generator=gen)
    dout = torch.randn(M, nh * dv + 4, generator=gen)
    r = torch.rand(M, generator=gen)
    r[torch.rand(M, generator=gen) < 0.3] = 0.0
    r[0] = 0.0
    return qkv.cuda(), tqkv.cuda(), dout.cuda(), r.cuda(), _adjacency(B, A, gen)


def _cols(buf, nh, dk, dv):
    """(q, k, v) column views of a qkv buffer."""
    return buf[:, nh * (dv + dk):nh * (dv + 2 * dk)], buf[:, nh * dv:nh * (dv + dk)], buf[:, :nh * dv]


def _heads(x, B, A, nh, d):
    return x.reshape(B, A, nh, d).transpose(1, 2)


def _kl_rows(w, wt):
    """train.attention_kl's per-agent KL [B, A] of one layer: F.kl_div(log_softmax(w), softmax(w_tar)) summed over
    heads and destination agents."""
    n = w.shape[-1]
    kl = F.kl_div(F.log_softmax(w, -1).reshape(-1, n), F.softmax(wt, -1).reshape(-1, n), reduction="none").view(w.shape)
    return kl.sum(dim=(1, 3))


def _bwd_ref(qkv, tqkv, dout, r, adj, B, A, nh, dk, dv, reg):
    """fp64 autograd through the core of AttModel.forward on leaf q, k, v (+ sum_i r_i KL_i built as
    train.attention_kl builds it)."""
    q, k, v = (t.double().clone().requires_grad_(True) for t in _cols(qkv, nh, dk, dv))
    qh, kh, vh = _heads(q, B, A, nh, dk), _heads(k, B, A, nh, dk), _heads(v, B, A, nh, dv)
    w = torch.matmul(qh, kh.transpose(2, 3)) * (1 / dk ** 0.5)
    att = F.softmax(w.masked_fill(adj.unsqueeze(1) == 0, -1e9), dim=-1)
    out = (torch.matmul(att, vh) + vh).transpose(1, 2).contiguous().view(B * A, nh * dv)
    obj = (out * dout[:, :nh * dv].double()).sum()
    if reg:
        tq, tk, _ = _cols(tqkv, nh, dk, dv)
        wt = torch.matmul(_heads(tq.double(), B, A, nh, dk), _heads(tk.double(), B, A, nh, dk).transpose(2, 3)) \
            * (1 / dk ** 0.5)
        rr = torch.ones(B * A, dtype=torch.float64, device=q.device) if r is None else r.double()
        obj = obj + (_kl_rows(w, wt).reshape(-1) * rr).sum()
    return torch.autograd.grad(obj, (q, k, v))


def _run_bwd(L, qkv, tqkv, dout, r, adj, B, A, nh, dk, dv, reg):
    n = nh * (dv + 2 * dk)
    d = torch.full((B * A, n + 4), float("nan"), device="cuda")
    q, k, v = _cols(qkv, nh, dk, dv)
    dq, dkk, dvv = _cols(d, nh, dk, dv)
    tq, tk, _ = _cols(tqkv, nh, dk, dv)
    L.check(L.lib().gm_agent_attention_bwd(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), qkv.stride(0), adj.data_ptr(), B, A, nh, dk, dv, dout.data_ptr(),
        dout.stride(0), tq.data_ptr() if reg else None, tk.data_ptr() if reg else None, tqkv.stride(0),
        None if (r is None or not reg) else r.data_ptr(), dq.data_ptr(), dkk.data_ptr(), dvv.data_ptr(), d.stride(0),
        L.stream_ptr()))
    return d


@pytest.mark.parametrize("mode", ["plain", "reg_r", "reg_no_r"])
@pytest.mark.parametrize("B,A,nh,dk,dv", CASES)
def test_agent_attention_bwd_vs_fp64(B, A, nh, dk, dv, mode):
    """dq, dk, dv within the project's 1e-5 absolute contract of fp64 autograd on N(0, 1) inputs: without the
    regulariser, with it and a row scale that holds zeros (done agents), and with it and no row scale (= 1); two runs
    give the same bits; the padding columns of the output rows stay untouched."""
    M_, T, DS, RB, L = mods()
    qkv, tqkv, dout, r, adj = _case(B, A, nh, dk, dv, 100 * A + nh + dk)
    reg = mode != "plain"
    r = r if mode == "reg_r" else None
    d = _run_bwd(L, qkv, tqkv, dout, r, adj, B, A, nh, dk, dv, reg)
    d2 = _run_bwd(L, qkv, tqkv, dout, r, adj, B, A, nh, dk, dv, reg)
    ref = _bwd_ref(qkv, tqkv, dout, r, adj, B, A, nh, dk, dv, reg)
    n = nh * (dv + 2 * dk)
    worst = 0.0
    for name, got, want in zip("qkv", _cols(d, nh, dk, dv), ref):
        err = (got.double() - want).abs().max().item()
        print(f"gm_agent_attention_bwd {mode} B={B} A={A} heads={nh} dk={dk} dv={dv}: d{name} max error {err:.3g} "
              f"(max |ref| {want.abs().max().item():.3g})")
        worst = max(worst, err)
    assert worst <= 1e-5
    assert torch.isnan(d[:, n:]).all()
    assert torch.equal(d[:, :n], d2[:, :n])


@pytest.mark.parametrize("B,A,nh,dk,dv", CASES)
def test_agent_attention_kl_vs_fp64(B, A, nh, dk, dv):
    """kl_row within 1e-5 absolute of fp64 F.kl_div(log_softmax, softmax) row sums, on targets perturbed enough that
    every row's KL is at least 1e-3 (A = 1: both softmaxes are 1 and the KL is exactly 0)."""
    M_, T, DS, RB, L = mods()
    qkv, tqkv, _, _, _ = _case(B, A, nh, dk, dv, 7 * A + nh + dv)
    q, k, _ = _cols(qkv, nh, dk, dv)
    tq, tk, _ = _cols(tqkv, nh, dk, dv)
    out = torch.full((B * A,), float("nan"), device="cuda")
    L.check(L.lib().gm_agent_attention_kl(q.data_ptr(), k.data_ptr(), qkv.stride(0), tq.data_ptr(), tk.data_ptr(),
                                          tqkv.stride(0), B, A, nh, dk, out.data_ptr(), L.stream_ptr()))
    s = 1 / dk ** 0.5
    w = torch.matmul(_heads(q.double(), B, A, nh, dk), _heads(k.double(), B, A, nh, dk).transpose(2, 3)) * s
    wt = torch.matmul(_heads(tq.double(), B, A, nh, dk), _heads(tk.double(), B, A, nh, dk).transpose(2, 3)) * s
    ref = _kl_rows(w, wt).reshape(-1)
    if A > 1:
        assert ref.min().item() >= 1e-3
    err = (out.double() - ref).abs().max().item()
    print(f"gm_agent_attention_kl B={B} A={A} heads={nh} dk={dk}: max error {err:.3g}, KL rows in "
          f"[{ref.min().item():.3g}, {ref.max().item():.3g}]")
    assert err <= 1e-5


@pytest.mark.parametrize("what", ["A65", "dk65", "null", "lds"])
def test_attention_bwd_and_kl_refuse(what):
    """A = 65, dk = 65 and a null pointer: GM_ERR_INVALID_ARG; rows that need more than 160 KB of LDS:
    GM_ERR_UNSUPPORTED; nothing is launched (the outputs keep their NaNs)."""
    M_, T, DS, RB, L = mods()
    B, A, nh, dk, dv = {"A65": (1, 65, 2, 16, 16), "dk65": (1, 4, 2, 65, 16), "null": (1, 4, 2, 16, 16),
                        "lds": (1, 64, 8, 64, 64)}[what]
    n = nh * (dv + 2 * dk)
    qkv = torch.randn(B * A, n, device="cuda")
    dout = torch.randn(B * A, nh * dv, device="cuda")
    adj = torch.ones(B, A, A, dtype=torch.int8, device="cuda")
    d = torch.full((B * A, n), float("nan"), device="cuda")
    kl = torch.full((B * A,), float("nan"), device="cuda")
    q, k, v = _cols(qkv, nh, dk, dv)
    dq, dkk, dvv = _cols(d, nh, dk, dv)
    want = UNSUPPORTED if what == "lds" else INVALID_ARG
    rc = L.lib().gm_agent_attention_bwd(q.data_ptr(), k.data_ptr(), None if what == "null" else v.data_ptr(), n,
                                        adj.data_ptr(), B, A, nh, dk, dv, dout.data_ptr(), nh * dv, q.data_ptr(),
                                        k.data_ptr(), n, None, dq.data_ptr(), dkk.data_ptr(), dvv.data_ptr(), n,
                                        L.stream_ptr())
    assert rc == want
    assert b"gm_agent_attention_bwd" in L.lib().gm_last_error()
    rc = L.lib().gm_agent_attention_kl(q.data_ptr(), k.data_ptr(), n, q.data_ptr(),
                                       None if what == "null" else k.data_ptr(), n, B, A, nh, dk, kl.data_ptr(),
                                       L.stream_ptr())
    assert rc == want
    assert b"gm_agent_attention_kl" in L.lib().gm_last_error()
    if what == "null":  # q_tar without k_tar, r without q_tar
        for tq, tk, r in ((q.data_ptr(), None, None), (None, None, kl.data_ptr())):
            rc = L.lib().gm_agent_attention_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), n, adj.data_ptr(), B, A, nh, dk,
                                                dv, dout.data_ptr(), nh * dv, tq, tk, n, r, dq.data_ptr(),
                                                dkk.data_ptr(), dvv.data_ptr(), n, L.stream_ptr())
            assert rc == INVALID_ARG
    torch.cuda.synchronize()
    assert torch.isnan(d).all() and torch.isnan(kl).all()


def _golden():
    M, T, DS, RB, L = mods()
    g = np.load(os.path.join(R.GOLDEN, "train_dgn.npz"))
    D = g["agent_obs"].shape[-1]
    sd = lambda p: {k[len(p):]: torch.as_tensor(g[k]) for k in g.files  # noqa: E731
                    if k.startswith(p) and not k.startswith(p + "after_")}
    m, tar = M.DGN(D, [64, 48], 4, 4, 2), M.DGN(D, [64, 48], 4, 4, 2)
    m.load_state_dict(sd("model_"))
    tar.load_state_dict(sd("target_"))
    f = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    Lq = g["actions"].shape[0]
    obs = F.pad(f(g["agent_obs"]), (0, (D + 3) // 4 * 4 - D))  # [L + 1, B, A, odp]
    adj = f(g["agent_adj"]).to(torch.int8)
    seq = DS.DGNSeqBatch(obs[:Lq].contiguous(), D, f(g["actions"]).long(), f(g["reward"]), f(g["done"]).bool(),
                         f(g["episode_done"]).bool(), adj[:Lq].contiguous(), obs[1:Lq + 1].contiguous(),
                         adj[1:Lq + 1].contiguous())
    return g, m.cuda(), tar.cuda(), seq


def test_dgn_seq_update_matches_reference_golden():
    """The reference's own DGN update (DGN(D, [64, 48], 4 actions, 4 heads, 2 layers), att coefficient 0.03) through
    dgn_seq_loss at the tolerances of test_models_gpu.test_model_update_matches_reference_golden: q and targets 1e-5,
    loss_q and the loss 1e-5 relative, loss_att 2e-3 relative, the KL's own gradient within 1e-3 of each tensor's
    largest element, then check_update (raw and clipped gradients, AdamW step, target update)."""
    from test_train_gpu import check_update

    M, T, DS, RB, L = mods()
    g, m, tar, seq = _golden()
    coeff = float(g["att_coeff"])
    assert coeff > 0 and DS.dgn_seq_ok(m, tar, None, coeff, None, seq.action.shape[2])
    Lq = seq.action.shape[0]
    params = list(m.parameters())
    names = [f"model_{k}" for k, _ in m.named_parameters()]
    assert names == list(g["param_names"])
    opt = torch.optim.AdamW(params, lr=float(g["lr"]))
    m.train()
    # the KL's own gradient, from a forward of its own (the node frees its saved tensors after one backward)
    parts = {}
    DS.dgn_seq_loss(m, tar, seq, float(g["gamma"]), params, coeff, parts)
    ga = torch.autograd.grad(coeff * parts["loss_att"], params, allow_unused=True)
    worst = 0.0
    for n, p, gr in zip(names, params, ga):
        ref = g["grad_att_" + n]
        if ref.shape != tuple(p.shape):  # the reference's autograd gave None (the KL does not reach this parameter;
            ref = np.zeros(tuple(p.shape), ref.dtype)  # the golden keeps a placeholder): the one node gives zeros
        got = np.zeros_like(ref) if gr is None else gr.detach().cpu().numpy()
        scale = max(np.abs(ref).max(), 1e-12)
        worst = max(worst, np.abs(got - ref).max() / scale)
        assert np.abs(got - ref).max() <= 1e-3 * scale + 1e-10, (n, np.abs(got - ref).max(), scale)
    print(f"dgn_seq: attention-KL gradient worst error / max |g| = {worst:.3g}")
    parts = {}
    loss, q, qt = DS.dgn_seq_loss(m, tar, seq, float(g["gamma"]), params, coeff, parts)
    for t in range(Lq):
        np.testing.assert_allclose(q[t].detach().cpu().numpy(), g[f"q_{t}"], atol=1e-5, rtol=0, err_msg=f"q_{t}")
        np.testing.assert_allclose(qt[t].cpu().numpy(), g[f"qtarget_{t}"], atol=1e-5, rtol=0, err_msg=f"qtarget_{t}")
    print(f"dgn_seq: loss_q {parts['loss_q'].item():.8g} (golden {g['loss_q'].item():.8g}), loss_att "
          f"{parts['loss_att'].item():.8g} (golden {g['loss_att'].item():.8g})")
    np.testing.assert_allclose(parts["loss_q"].item(), g["loss_q"].item(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(loss.item(), g["loss"].item(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(parts["loss_att"].item(), g["loss_att"].item(), rtol=2e-3, atol=1e-7)
    opt.zero_grad()
    loss.backward()
    check_update(g, names, params, opt, m, tar, T)


def _compare_with_per_step(T, DS, m, tar, batches, seq, coeff):
    """loss, q, targets and every gradient of dgn_seq_loss against train.dqn_loss on the same transitions, within
    1e-5 + 1e-4 relative (kink-tolerant, as the existing path comparisons)."""
    params = list(m.parameters())
    m.train()
    for p in params:
        p.grad = None
    p0 = {}
    l0, q0, t0 = T.dqn_loss(None, m, tar, batches, 0.98, att_coeff=coeff, parts=p0)
    l0.backward()
    g0 = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    p1 = {}
    l1, q1, t1 = DS.dgn_seq_loss(m, tar, seq, 0.98, params, coeff, p1)
    l1.backward()
    tol = dict(rtol=1e-4, atol=1e-5)
    for t in range(len(batches)):
        torch.testing.assert_close(q1[t], q0[t].detach(), **tol)
        torch.testing.assert_close(t1[t], t0[t], **tol)
    torch.testing.assert_close(l1, l0.detach(), **tol)
    torch.testing.assert_close(p1["loss_q"], p0["loss_q"].detach(), **tol)
    if coeff > 0:
        torch.testing.assert_close(p1["loss_att"], p0["loss_att"].detach(), **tol)
    else:
        assert p1["loss_att"] is None and p0["loss_att"] is None
    worst = 0.0
    for (n, p), a in zip(m.named_parameters(), g0):
        assert p.grad is not None, n
        worst = max(worst, (p.grad - a).abs().max().item())
        torch.testing.assert_close(p.grad, a, msg=lambda s, n=n: f"{n}: {s}", **tol)
    print(f"dgn_seq vs per-step, coeff {coeff}: loss {l1.item():.8g} / {l0.item():.8g}, worst gradient difference "
          f"{worst:.3g}")


def test_dgn_seq_golden_batches_match_per_step_without_regulariser():
    """The golden batches with coefficient 0: dgn_seq_loss against train.dqn_loss (no regulariser on either path)."""
    M, T, DS, RB, L = mods()
    g, m, tar, seq = _golden()
    f = lambda a: torch.as_tensor(a, device="cuda")  # noqa: E731
    Lq = seq.action.shape[0]
    batches = [RB.TransitionBatch(None, f(g["agent_obs"][t]), f(g["actions"][t]).long(), f(g["reward"][t]),
                                  f(g["agent_obs"][t + 1]), f(g["done"][t]).bool(), f(g["episode_done"][t]).bool(),
                                  None, None, None, None, None, None, f(g["agent_adj"][t]).float(),
                                  f(g["agent_adj"][t + 1]).float(), None) for t in range(Lq)]
    assert DS.dgn_seq_ok(m, tar, None, 0.0, None, seq.action.shape[2])
    _compare_with_per_step(T, DS, m, tar, batches, seq, 0.0)


@pytest.mark.parametrize("Lq", [1, 3])
def test_dgn_seq_matches_per_step_path_on_buffer(Lq):
    """A buffer filled as test_models_gpu.test_training_update_runs_and_reduces_loss fills it (B = 8, A = 6,
    store_adj), the CLI-default DGN (512, 256 encoder, 8 heads, 2 layers), done agents: get_dgn_sequences gathers the
    bits get_batch gathers from the same stream state, and the two paths agree with the regulariser on."""
    M, T, DS, RB, L = mods()
    B, A, D, nseq = 8, 6, 30, 16
    torch.manual_seed(5)
    m, tar = M.DGN(D, [512, 256], 4, 8, 2).cuda(), M.DGN(D, [512, 256], 4, 8, 2).cuda()
    assert DS.dgn_seq_ok(m, tar, None, 0.03, None, A)
    rb = RB.ReplayBuffer(0, 8 * B, B, A, D, 0, 0, 0, torch.device("cuda"), store_adj=True)
    for _ in range(6):
        adj = (torch.rand(B, A, A, device="cuda") < 0.4) | torch.eye(A, dtype=torch.bool, device="cuda")
        nadj = (torch.rand(B, A, A, device="cuda") < 0.4) | torch.eye(A, dtype=torch.bool, device="cuda")
        rb.add_pre(torch.randn(B, A, D, device="cuda"), adj=adj)
        rb.add_post(torch.randint(0, 4, (B, A), device="cuda"), torch.randn(B, A, device="cuda"),
                    torch.randn(B, A, D, device="cuda"), torch.rand(B, A, device="cuda") < 0.2, False, next_adj=nadj)
    rng0 = rb.rng.clone()
    batches = list(rb.get_batch(nseq, sequence_length=Lq))
    rng1 = rb.rng.clone()
    rb.rng.copy_(rng0)
    seq = rb.get_dgn_sequences(nseq, Lq)
    assert torch.equal(rb.rng, rng1)  # the same stream, advanced the same way
    assert len(batches) == Lq and seq.done.any() and not seq.done.all()
    assert seq.adj.dtype == torch.int8 and seq.next_adj.dtype == torch.int8
    for t, b in enumerate(batches):
        assert torch.equal(b.idx[0], seq.idx[0][t]) and torch.equal(b.idx[1], seq.idx[1])
        assert torch.equal(seq.obs[t][..., :D], b.obs) and torch.equal(seq.next_obs[t][..., :D], b.next_obs)
        assert torch.equal(seq.action[t], b.action) and torch.equal(seq.reward[t], b.reward)
        assert torch.equal(seq.done[t], b.done)
        assert torch.equal(seq.episode_done[t].expand(nseq), b.episode_done.expand(nseq))
        assert torch.equal(seq.adj[t], b.adj.to(torch.int8)) and torch.equal(seq.next_adj[t], b.next_adj.to(torch.int8))
    _compare_with_per_step(T, DS, m, tar, batches, seq, 0.03)


def test_dgn_seq_ok_dispatch():
    M, T, DS, RB, L = mods()
    D = 30
    cli = lambda **kw: M.DGN(D, [512, 256], 4, 8, 2, **kw)  # noqa: E731
    m, tar = cli(), cli()
    assert DS.dgn_seq_ok(m, tar, None, 0.03, None, 20)
    assert DS.dgn_seq_ok(m, tar, None, 0.0, None, 64) and DS.dgn_seq_ok(m, tar, None, 0.03, None)
    assert not DS.dgn_seq_ok(m, tar, M.NetMon(8, 32, [32], 1), 0.03, None, 20)
    assert not DS.dgn_seq_ok(m, tar, None, 0.03, M.MLP(8, [8, 4], activation_on_output=False), 20)
    assert not DS.dgn_seq_ok(cli(activation="relu"), cli(activation="relu"), None, 0.03, None, 20)
    assert not DS.dgn_seq_ok(m, tar, None, 0.03, None, 65)
    wide = lambda: M.DGN(D, [512], 4, 8, 2)  # noqa: E731  (head input 512 * 3 = 1536)
    assert not DS.dgn_seq_ok(wide(), wide(), None, 0.03, None, 20)
    assert not DS.dgn_seq_ok(M.DQNR(D, [64, 64], 4), M.DQNR(D, [64, 64], 4), None, 0.0, None, 20)
    assert not DS.dgn_seq_ok(m, M.DQNR(D, [64, 64], 4), None, 0.0, None, 20)
    assert not DS.dgn_seq_ok(m, tar, None, -0.1, None, 20)
    old = L.GEMM_MODE
    L.GEMM_MODE = "f32"
    try:
        assert not DS.dgn_seq_ok(m, tar, None, 0.03, None, 20)
    finally:
        L.GEMM_MODE = old
