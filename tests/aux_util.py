"""Shared helpers of tests/test_aux_seq_gpu.py and tests/test_aux_ref.py: fp64 references and error bounds of the
NetMon aux head kernels (gm_aux_head_mse / gm_aux_head_mse_bwd, include/graph_marl_amd.h), strided operands with
NaN padding and guard rows, and a small replayed rollout whose ring stores the aux targets."""
import importlib
import math

import torch

U24 = 2.0 ** -24  # fp32 unit roundoff
GUARD = 3  # NaN rows after the last row of every strided operand
RPB_MAX = 64


def pack_bits(b):
    """bool [rows][cols] -> int32 words [rows][ceil(cols / 32)], bit c % 32 of word c / 32."""
    rows, cols = b.shape
    W = (cols + 31) // 32
    x = torch.zeros(rows, W * 32, dtype=torch.int64, device=b.device)
    x[:, :cols] = b.long()
    w = (x.view(rows, W, 32) << torch.arange(32, device=b.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def strided(x, ld, guard=GUARD):
    """(buffer [rows + guard][ld] full of NaN with x in its first columns, the view of x's place in it)."""
    rows, cols = x.shape
    buf = torch.full((rows + guard, ld), float("nan"), dtype=x.dtype, device=x.device)
    buf[:rows, :cols] = x
    return buf, buf[:rows, :cols]


def untouched(buf, before, rows, cols):
    """The padding columns and guard rows of buf hold the bits they held in `before` (a clone)."""
    a, b = buf.view(torch.int32).clone(), before.view(torch.int32).clone()
    a[:rows, :cols] = 0
    b[:rows, :cols] = 0
    return torch.equal(a, b)


def fwd_ref(y, w2, b2, tgt):
    """fp64 residual of the head's second layer and the per-element bound of its fp32 evaluation: res = b2 + y w2^T
    - tgt. The kernel rounds cols products into a running sum (one fmaf each: cols roundings), adds the bias and
    subtracts the target (2 more), and one unit covers the inputs' own representation: every rounding is relative
    to a partial result no larger than |b2| + |tgt| + sum |y w2|, so |error| <= (cols + 3) 2^-24 of that."""
    y, w2, b2, tgt = (t.double() for t in (y, w2, b2, tgt))
    res = b2 + y @ w2.t() - tgt
    mag = b2.abs() + tgt.abs() + y.abs() @ w2.abs().t()
    return res, (y.shape[1] + 3) * U24 * mag


def loss_terms(rows, n_out, rpb):
    """Addends on the longest summation path of sum res^2: a lane's own (rpb / 8 rows x ceil(n_out / 32) outputs),
    the 6 levels of the wave's xor tree, 2 levels over the 4 waves, and the caller's sum over the blocks."""
    return (rpb + 7) // 8 * ((n_out + 31) // 32) + 6 + 2 + (rows + rpb - 1) // rpb


def loss_bound(res, elem_bound, terms):
    """Bound of |computed sum res^2 - exact|: each square moves by 2 |res| * (its element's bound), and a sum whose
    longest path has `terms` addends of non-negative numbers is off by at most terms 2^-24 of the sum."""
    return (2 * res.abs() * elem_bound).sum().item() + terms * U24 * (res ** 2).sum().item()


def bwd_ref(res, w2, z, act, s):
    """fp64 autograd of s * sum(res * (act(z) w2^T + b2)) with res held constant: the gradients w.r.t. z (= g of
    gm_aux_head_mse_bwd: s (res w2) times leaky_relu's derivative at z, 0.01 where z <= 0), b2 (s sum_r res) and w2
    (s res^T y), and the per-element bound of g's fp32 evaluation: n_out fmaf roundings, the scale and the mask
    (2 more), one for the inputs, relative to |s| sum |res w2| times the mask."""
    res, w2 = res.double(), w2.double()
    z = z.double().clone().requires_grad_(True)
    w = w2.clone().requires_grad_(True)
    b = torch.zeros(w2.shape[0], dtype=torch.float64, device=w2.device, requires_grad=True)
    y = torch.nn.functional.leaky_relu(z, 0.01) if act else z
    (s * (res * (y @ w.t() + b)).sum()).backward()
    slope = (0.01 + 0.99 * (z.detach() > 0).double()) if act else torch.ones_like(z.detach())
    bound = (w2.shape[0] + 3) * U24 * abs(s) * (res.abs() @ w2.abs()) * slope
    return z.grad, b.grad, w.grad, bound


def wgrad_bound(a, b):
    """Per-element bound of gm_gemm_x3_wgrad's a^T b ([k][m], [k][n] fp32 operands, k batch rows) against fp64 of
    the same operands. Each operand enters as two f16 pieces of its scaled value, 22 significant bits (2^-22
    relative each), and the product drops the low x low term (2^-22 of |a b|): 3 * 2^-22 per product. The three
    piece products accumulate in fp32 on v_mfma 16-deep steps: at most 3 * ceil(k / 16) sequential additions on one
    accumulator's path, plus 8 for the split-K partials' sum, each rounding 2^-24 of a partial sum no larger than
    sum_k |a| |b|."""
    k = a.shape[0]
    mag = a.double().abs().t() @ b.double().abs()
    return (3 * 2.0 ** -22 + (3 * ((k + 15) // 16) + 8) * U24) * mag


def expected_scale(m):
    """gm_absmax_scale's power of two for a maximum m: 2^(14 - e) with m in [2^(e-1), 2^e); 1 for m = 0."""
    if m == 0:
        return 1.0
    return 2.0 ** (14 - math.frexp(m)[1])


def mods():
    names = ("", ".model", ".fused", ".wrapper", ".train", ".train_seq", ".replaybuffer", "._lib")
    return tuple(importlib.import_module("graph-marl_amd" + n) for n in names)


N_S, H_S, ENC_S, DQN_S = 10, 32, [32], [64, 32]


def replayed_aux(rnn="lstm", K=1, agg="sum", glob=False, n_env=8, steps=12, ep_len=5, seed=11, aux=True):
    """n_env routing envs with N = A = 10 under a NetMonWrapper (H = 32, encoder (32,)), `steps` recorded steps with
    random actions, episodes of ep_len steps (the wrapper resets); the ring stores get_node_aux() of every step when
    `aux`. Returns (netmon, model, target, aux_model, rb, params) with the aux head main.py builds (params includes
    its parameters)."""
    gm, M, FU, W, T, S, RB, L = mods()
    N = A = N_S
    H = H_S
    gw = (5 if glob else 4) * H
    env = gm.Routing(gm.Network(N, random_topology=True, excluded_seeds=gm.EVAL_SEEDS), A, n_env=n_env, seed=seed,
                     obs_extra=gw, agent_adjacency=False)
    torch.manual_seed(10 * K + len(rnn) + int(glob))
    netmon = M.NetMon(4 * N + 8, H, list(ENC_S), K, rnn_type=rnn, agg_type=agg, output_global_hidden=glob).cuda()
    D = env.obs_dim + gw
    model, target = M.DQN(D, list(DQN_S), 4).cuda(), M.DQN(D, list(DQN_S), 4).cuda()
    target.load_state_dict(model.state_dict())
    with torch.no_grad():
        for p in target.parameters():
            p.add_(0.01 * torch.randn_like(p))
    Sz = netmon.get_state_size()
    aux_model = M.MLP(Sz, [Sz, N], activation_on_output=False).cuda()
    wenv = W.NetMonWrapper(env, netmon, 1)
    rb = RB.ReplayBuffer(seed, (steps + 1) * n_env, n_env, A, env.obs_dim, N, 4 * N + 8, Sz, "cuda",
                         node_aux_size=N if aux else 0)
    wenv.reset_()
    gen = torch.Generator().manual_seed(seed)
    for t in range(steps):
        rb.add_pre(env.obs, wenv.last_netmon_state, env.node_obs, env.nbr, env.agent_node,
                   node_aux=env.get_node_aux() if aux else None)
        act = torch.randint(0, 4, (n_env, A), generator=gen).to(torch.int32).cuda()
        wenv.step_(act)
        end = (t + 1) % ep_len == 0
        rb.add_post(act, env.reward, env.obs, env.done.bool(), end, env.node_obs, env.agent_node)
        if end:
            wenv.reset_()
    netmon.state = None
    netmon.train()
    model.train()
    params = list(model.parameters()) + list(netmon.parameters()) + list(aux_model.parameters())
    return netmon, model, target, aux_model, rb, params


def sample(rb, n_seq, Lq):
    """The same draw through get_batch and get_sequences (the stream restored in between)."""
    rng0 = rb.rng.clone()
    batches = list(rb.get_batch(n_seq, sequence_length=Lq))
    rng1 = rb.rng.clone()
    rb.rng.copy_(rng0)
    seq = rb.get_sequences(n_seq, Lq)
    assert torch.equal(rb.rng, rng1)
    for t, b in enumerate(batches):
        assert torch.equal(b.idx[0], seq.idx[0][t]) and torch.equal(b.idx[1], seq.idx[1])
    return batches, seq
