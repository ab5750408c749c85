"""GRU NetMon on the sequence-batched training paths (train_seq.py, sl_seq.py): the two cell kernels
gm_gru_cell_fwd / gm_gru_cell_bwd against gm_gru_pointwise and torch fp64, the whole update against the
reference's golden GRU update (train_gru.npz) and against the per-step autograd path on replayed rollout data,
and config 5's unroll against its per-step autograd path. The whole-update tests run the LSTM tests' own bodies
(their setup, assertions and bounds) with the cell type switched to gru."""
import ctypes as C
import importlib

import pytest
import torch

import test_sl_seq_gpu as TSL
import test_train_seq_gpu as TTS
from test_netmon_paths_gpu import sym_table

pytestmark = pytest.mark.gpu

SHAPES = [(777, 32), (130, 64), (197, 128), (65, 256)]


def _lib():
    return importlib.import_module("graph-marl_amd._lib")


@pytest.mark.parametrize("m,H,ldh,ldo", [(777, 32, 32, 32), (130, 64, 72, 68), (197, 128, 128, 128),
                                         (65, 256, 256, 256), (33, 30, 30, 31)])
def test_gru_cell_fwd(m, H, ldh, ldo):
    """h' bit-equal to gm_gru_pointwise on the equivalent gi = [a_r | a_z | a_nx], gh = [0 | 0 | a_nh];
    G = [r | z | n | a_nh] against fp64 sigmoid / tanh of P. (130, 64): h and h' rows strided; (33, 30): the
    scalar form."""
    L = _lib()
    torch.manual_seed(m + H)
    P = torch.randn(m, 4 * H, device="cuda") * 2
    hb = torch.randn(m, ldh, device="cuda")
    ob = torch.full((m, ldo), float("nan"), device="cuda")
    gi = P[:, :3 * H].contiguous()
    gh = torch.cat([torch.zeros(m, 2 * H, device="cuda"), P[:, 3 * H:]], 1).contiguous()
    ref = torch.empty(m, H, device="cuda")
    L.check(L.lib().gm_gru_pointwise(gi.data_ptr(), 3 * H, gh.data_ptr(), 3 * H, hb.data_ptr(), ldh, m, H,
                                     ref.data_ptr(), H, L.stream_ptr()))
    G = P.clone()
    L.check(L.lib().gm_gru_cell_fwd(G.data_ptr(), 4 * H, hb.data_ptr(), ldh, m, H, ob.data_ptr(), ldo,
                                    L.stream_ptr()))
    assert L.last_kernel() == ("k_gru_cell_fwd<4>" if H % 4 == 0 else "k_gru_cell_fwd<1>")
    assert torch.equal(ob[:, :H], ref)
    assert torch.isnan(ob[:, H:]).all()
    P64 = P.double()
    r, z = torch.sigmoid(P64[:, :H]), torch.sigmoid(P64[:, H:2 * H])
    n = torch.tanh(P64[:, 2 * H:3 * H] + r * P64[:, 3 * H:])
    for k, want in enumerate((r, z, n)):
        assert TTS._rel(G[:, k * H:(k + 1) * H], want) < 2e-6, k
    assert torch.equal(G[:, 3 * H:], P[:, 3 * H:])


def _members_mask(nbr):
    """[G, N, N] fp64: 1 where node n is in {r} U nbr(r) (row r's own list, -1 skipped)."""
    G, N, deg = nbr.shape
    mask = torch.eye(N, dtype=torch.float64).repeat(G, 1, 1)
    for k in range(deg):
        col = nbr[:, :, k].long()
        ok = col >= 0
        mask[torch.arange(G)[:, None].expand(G, N)[ok], torch.arange(N)[None, :].expand(G, N)[ok], col[ok]] = 1.0
    return mask


def _gru_bwd_case(m, H, N, mean, pad, full=True):
    """gm_gru_cell_bwd on m rows (the last graph partial when N does not divide m) against fp64 autograd of
    h' = (1 - z) n + z h with r, z, n from fp64 pre-activations; full: every source and output present."""
    L = _lib()
    torch.manual_seed(m + H + N + mean)
    G_ = (m + N - 1) // N
    rows = G_ * N
    nbr = sym_table(G_, N, 3, seed=H + N)
    pre = torch.randn(m, 4 * H, dtype=torch.float64, requires_grad=True)
    h = torch.randn(m, H, dtype=torch.float64, requires_grad=True)
    r, z = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H])
    anh = pre[:, 3 * H:]
    n = torch.tanh(pre[:, 2 * H:3 * H] + r * anh)
    h1 = (1 - z) * n + z * h
    act = torch.cat([r, z, n, anh], 1).detach().float().cuda().contiguous()
    dh0, dh1, dh2, dhe = (torch.randn(m, H).cuda() for _ in range(4))
    dm = torch.randn(rows, H).cuda()
    emask = torch.rand(G_) < 0.4
    emask[0], emask[-1] = True, False
    g = dh0.cpu().double()
    if full:
        cnt = (nbr >= 0).sum(-1).double() + 1  # |{n} U nbr(n)|
        s = (1.0 / cnt if mean else torch.ones_like(cnt)).unsqueeze(-1)
        agg = torch.einsum("grn,gnh->grh", _members_mask(nbr), dm.cpu().double().view(G_, N, H) * s)
        keep = (~emask).double().repeat_interleave(N)[:m].unsqueeze(1)
        g = g + dh1.cpu().double() + dh2.cpu().double() + agg.reshape(rows, H)[:m] + keep * dhe.cpu().double()
    h1.backward(g)
    want = pre.grad  # [da_r | da_z | da_nx | da_nh]: pre's columns are the kernel's gate order
    hd = h.detach().float().cuda().contiguous()
    a = L.GRUBwdArgs()
    a.act, a.ld_act, a.h, a.ld_h = act.data_ptr(), 4 * H, hd.data_ptr(), H
    a.dh0, a.ld_dh0 = dh0.data_ptr(), H
    a.m, a.hidden = m, H
    ld_dg = 4 * H + pad
    dgb = torch.full((m + 1, ld_dg), float("nan"), device="cuda")
    a.dgates, a.ld_dg = dgb.data_ptr(), ld_dg
    nb_ = (m + 63) // 64
    dhd = torch.full((m + 1, H), float("nan"), device="cuda")
    part = torch.empty(nb_, 4 * H, device="cuda")
    sc, mx = torch.empty(1, device="cuda"), torch.zeros(1, device="cuda")
    nbr_d, em = nbr.cuda().contiguous(), emask.to(torch.uint8).cuda()
    if full:
        a.dh1, a.ld_dh1, a.dh2, a.ld_dh2 = dh1.data_ptr(), H, dh2.data_ptr(), H
        a.dm, a.ld_dm, a.nbr, a.n_nodes, a.deg, a.mean = dm.data_ptr(), H, nbr_d.data_ptr(), N, 3, mean
        a.dh_ext, a.ld_ext, a.ext_mask, a.rows_per_sample = dhe.data_ptr(), H, em.data_ptr(), N
        a.dh_dir, a.ld_dhd = dhd.data_ptr(), H
        a.bias_part, a.rows_per_block, a.dg_scale, a.dg_max = part.data_ptr(), 64, sc.data_ptr(), mx.data_ptr()
    assert m % 64, "m must leave a partial last block"
    L.check(L.lib().gm_gru_cell_bwd(C.byref(a), L.stream_ptr()))
    vec = pad % 4 == 0 and H % 4 == 0 and (256 // (H // 4)) * (H // 4) % 64 == 0
    assert L.last_kernel() == ("k_gru_cell_bwd<4>" if vec else "k_gru_cell_bwd<1>")
    dg = dgb[:m, :4 * H]
    assert TTS._rel(dg, want.cuda()) < 2e-6
    assert torch.isnan(dgb[:m, 4 * H:]).all() and torch.isnan(dgb[m]).all()
    if full:
        assert TTS._rel(dhd[:m], (g * z.detach()).cuda()) < 2e-6
        assert torch.isnan(dhd[m]).all()
        assert TTS._rel(part.sum(0), want.sum(0).cuda()) < 1e-5
        assert mx.item() == dg.abs().max().item()
        e = torch.empty(1, device="cuda")
        dgc = dg.contiguous()
        FU = importlib.import_module("graph-marl_amd.fused")
        L.check(FU._setup().gm_absmax_scale(dgc.data_ptr(), dgc.numel(), e.data_ptr(), L.stream_ptr()))
        assert sc.item() == e.item()
    return a, dgb


@pytest.mark.parametrize("pad", [4, 1])
@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("N", [4, 20])
@pytest.mark.parametrize("m,H", SHAPES + [(70, 320)])
def test_gru_cell_bwd_vs_fp64_autograd(m, H, N, mean, pad):
    """Every gradient source (dh0, dh1, dh2, the transposed aggregate of dm on tables with -1 entries in sum and
    mean, dh_ext under an ext_mask that zeroes some graphs) and every output; pad 4 keeps the 16-byte form, pad 1
    (ld_dg = 4H + 1) takes the scalar form; H = 320 is the H % 64 == 0 range on the scalar form."""
    _gru_bwd_case(m, H, N, mean, pad)


def test_gru_cell_bwd_optional_pointers_null():
    """Only the required operands: no source gives zero gate gradients; with dh0 alone (no optional output) the
    gate gradients of that source."""
    L = _lib()
    _gru_bwd_case(197, 128, 20, 0, 4, full=False)
    m, H = 130, 64
    act = torch.rand(m, 4 * H, device="cuda")
    h = torch.randn(m, H, device="cuda")
    dg = torch.full((m, 4 * H), float("nan"), device="cuda")
    a = L.GRUBwdArgs()
    a.act, a.ld_act, a.h, a.ld_h, a.m, a.hidden = act.data_ptr(), 4 * H, h.data_ptr(), H, m, H
    a.dgates, a.ld_dg = dg.data_ptr(), 4 * H
    L.check(L.lib().gm_gru_cell_bwd(C.byref(a), L.stream_ptr()))
    assert torch.equal(dg, torch.zeros_like(dg))


@pytest.mark.parametrize("H", [48, 96, 320 + 32, 1088])
def test_gru_cell_bwd_rejects_other_hidden_sizes(H):
    """H outside {H <= 256, 256 % H == 0} U {H % 64 == 0, H <= 1024}: GM_ERR_UNSUPPORTED, nothing launched."""
    L = _lib()
    m = 8
    act = torch.rand(m, 4 * H, device="cuda")
    h = torch.randn(m, H, device="cuda")
    dg = torch.full((m, 4 * H), float("nan"), device="cuda")
    a = L.GRUBwdArgs()
    a.act, a.ld_act, a.h, a.ld_h, a.m, a.hidden = act.data_ptr(), 4 * H, h.data_ptr(), H, m, H
    a.dgates, a.ld_dg = dg.data_ptr(), 4 * H
    assert L.lib().gm_gru_cell_bwd(C.byref(a), L.stream_ptr()) == -5
    assert b"gm_gru_cell_bwd" in L.lib().gm_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dg).all()


def test_gru_seq_update_matches_reference_golden():
    """train_gru.npz (gru, sum, K = 2, H = 32, L = 3 with episode ends, 4 graphs) through seq_loss + check_update:
    the LSTM golden test's body (seq_ok asserted first, then its assertions and tolerances)."""
    import numpy as np

    import golden_update as GU
    M = TTS.mods()[0]
    g = np.load(f"{TTS.R.GOLDEN}/train_gru.npz")
    assert GU.arch(g)[0] == "gru"
    netmon, model, target, _ = GU.build(g, M, torch.device("cuda"))
    assert TTS.mods()[2].seq_ok(netmon, model, target)
    TTS.test_seq_update_matches_reference_golden("train_gru.npz")


@pytest.mark.parametrize("K,agg,tiles", [(1, "sum", "common"), (2, "mean", "common"), (1, "sum", "default")])
def test_gru_seq_update_matches_autograd_path_on_rollout(K, agg, tiles, monkeypatch):
    """test_seq_update_matches_autograd_path_on_rollout (64 envs x 30 steps, 512 sequences x 8, _compare_paths'
    bounds) with every NetMon it builds a GRU one."""
    M, T, S, FU, L = TTS.mods()
    made = []
    orig = M.NetMon

    def gru_netmon(*a, **kw):
        made.append(orig(*a, rnn_type="gru", **kw))
        return made[-1]

    monkeypatch.setattr(M, "NetMon", gru_netmon)
    TTS.test_seq_update_matches_autograd_path_on_rollout(K, agg, tiles)
    assert len(made) == 1 and made[0].rnn_type == "gru" and made[0].state_size == 128
    model = M.DQN(6 * 20 + 10 + 512, [512, 256], 4).cuda()
    assert S.seq_ok(made[0], model, model)


@pytest.mark.parametrize("K,agg,steps", [(1, "sum", 4), (2, "mean", 3), (1, "sum", 1)])
def test_gru_sl_seq_matches_autograd_path(K, agg, steps, monkeypatch):
    """Config 5's unroll with GRU cells: test_sl_seq_matches_autograd_path (its small case's size and bounds) on
    GRU NetMonSL models; seq_ok accepts them."""
    SL, M = TSL._mods()
    orig = TSL._args

    def gru_args(*a, **kw):
        ns = orig(*a, **kw)
        ns.netmon_rnn_type = "gru"
        return ns

    monkeypatch.setattr(TSL, "_args", gru_args)
    model = SL.NetMonSL(TSL._args(20, 128, "512,256", K, agg), 4 * 20 + 8, 4, 20).cuda()
    assert model.netmon.rnn_type == "gru" and SL.SQ.seq_ok(model.netmon)
    assert SL.SQ.seq_ok(model.netmon, rows=256 * 20, steps=steps)
    TSL.test_sl_seq_matches_autograd_path(K, agg, steps)
