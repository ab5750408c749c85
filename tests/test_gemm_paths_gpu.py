"""Every kernel instantiation the GEMM entry points can launch (csrc/gm_gemm.hip): gm_gemm_f32 / gm_gemm_x3
(dispatch<X3>), gm_gemm_x3_dgrad, gm_gemm_x3_head, gm_encoder_x3 and gm_gemm_x3_wgrad[2] pick one of ~120
instantiations of k_gemm, k_gemm3, k_gemm3g and the weight-gradient kernels from the A source, the epilogue, m, n,
K, amax / scale and the four process-wide knobs (gm_gemm_set_tile / _mfma / _dgrad / _wgrad). CASES maps every
name the library was compiled to launch (gm_gemm_kernel_name) to the cases that run it; every case sets its knobs,
asserts gm_last_kernel() and compares with a plain fp64 torch restatement (gathers by index, no library call), so a
new instantiation without a case fails on any machine and a threshold change cannot silently drop a kernel.

Shapes are the smallest at which a BM x BN tile can still go wrong: m = BM + 37 (two row blocks, the second
ragged; READOUT / AGGREGATE / ROUTING_ENC the nearest G * R), n = BN + 2 (gate epilogues n = 4H, H = 32 or 96),
K = 132 in rows of stride 136 (a 4-wide k tail behind more k steps than any pipeline has stages). Input padding
columns hold 1e6 (they must not reach a product or the published max |A|); outputs, their padding columns and a
guard row hold NaN before the call and padding / guard must still be NaN afterwards.

Tolerances are the project's own: split-f16 forms <= max(1e-6, 2 x the exact-f32 form's error on the same
inputs) of sum |a w| and the exact-f32 forms < 2e-6 (test_gemm_precision_gpu.py, same operand draw); dgrad and
wgrad 4e-6 of sum |g w|; gate epilogues atol 1e-5; head and encoder chain as test_fused_gpu.py. The dgrad bias
partials are sums of at most 128 of the kernel's own fp32 outputs: they are compared with the fp64 sum of those
outputs within the fp32 summation bound 128 * 2^-24 * sum |y|."""
import ctypes as C
import importlib
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

# LDS-DMA tiles of k_gemm3g (gm_gemm_set_tile 8..14): WGM, WGN, TM, TN, stages, blocks / CU
G_TILES = {8: (4, 2, 2, 4, 2, 1), 9: (4, 2, 1, 4, 3, 1), 10: (4, 2, 1, 4, 2, 1), 11: (8, 1, 1, 4, 2, 1),
           12: (4, 1, 1, 4, 2, 2), 13: (2, 2, 2, 2, 2, 2), 14: (2, 2, 2, 4, 2, 1)}
K3_BIAS = {0: (2, 2, 2, 2, 16), 1: (2, 4, 2, 2, 16), 2: (4, 2, 2, 2, 16), 3: (2, 2, 2, 2, 32)}  # k_gemm3, tile 0..3
K3_LSTM = {0: (4, 1, 1, 4, 16), 1: (8, 1, 1, 4, 16), 2: (4, 1, 1, 4, 32)}
K1_BIAS = {0: (2, 2, 2, 2, 32, 2), 1: (2, 2, 2, 4, 16, 2), 2: (2, 2, 4, 2, 16, 2), 3: (2, 2, 2, 2, 16, 2),
           4: (2, 2, 2, 2, 16, 4)}  # k_gemm, tile 0..4 (.., BK, blocks / CU)
K1_LSTM = {0: (4, 1, 1, 4, 32, 2), 2: (4, 1, 2, 4, 16, 2), -1: (4, 1, 1, 4, 16, 4)}


def g3(t, mode, epi, ax, mf):
    wgm, wgn, tm, tn, s, occ = t
    return f"k_gemm3g<{wgm},{wgn},{tm},{tn},S{s},{mode},{epi},occ{occ},AX{ax},MF{mf}>"


def g1(fam, t, mode, epi, occ=2):
    return f"{fam}<{t[0]},{t[1]},{t[2]},{t[3]},BK{t[4]},{mode},{epi},occ{occ}>"


# kernel name (gm_last_kernel) -> (test below, its cases)
#   bias:  (form, A source, tile, mfma, ax, n or None = BN + 2, two sources); ax 1 = amax, 2 = scale
#   gate:  (form, A source, tile, mfma, ax, two sources); each runs the LSTM and the GRU cell
#   dgrad: (gm_gemm_set_dgrad form, mfma, scaled); each runs mask + split + y2 + part + gmax, then bare
#   head:  (mfma, amax, n); chain: (N, k)
#   wgrad: (gm_gemm_set_wgrad form, n, batch rows k, kind); kind "plain", "two" (n1 = 128 + 36) or "map" (period /
#          shift row maps on the two sources); kchunk = 64
CASES = {}


def _add(name, test, *cases):
    t, cs = CASES.setdefault(name, (test, []))
    assert t == test, name
    cs.extend(cases)


for _mf in (0, 1):
    _mfma = 2 if _mf else 0
    for _tile, _t in G_TILES.items():
        for _mode in ("DENSE", "READOUT"):
            _add(g3(_t, _mode, "BIAS", 0, _mf), "bias", ("x3", _mode, _tile, _mfma, 0, None, False))
        # tile 13's 64x64 waves cannot hold a gate group: the gate epilogues run tile 12's kernel there
        _add(g3(G_TILES[12] if _tile == 13 else _t, "DENSE", "LSTM", 0, _mf), "gate",
             ("x3", "DENSE", _tile, _mfma, 0, False))
    for _ax in (1, 2):
        for _tile in (9, 10, 12, 13):  # training operands on forced tiles
            _add(g3(G_TILES[_tile], "DENSE", "BIAS", _ax, _mf), "bias", ("x3", "DENSE", _tile, _mfma, _ax, None, False))
        for _tile in (12, 13):
            _add(g3(G_TILES[12], "DENSE", "LSTM", _ax, _mf), "gate", ("x3", "DENSE", _tile, _mfma, _ax, False))
    for _ax in (0, 2):
        _add(g3(G_TILES[12], "DENSE", "DGRAD", _ax, _mf), "dgrad", (1, _mfma, _ax == 2))
        _add(g3(G_TILES[10], "DENSE", "DGRAD", _ax, _mf), "dgrad", (2, _mfma, _ax == 2))
_add(g3(G_TILES[12], "DENSE", "BIAS", 0, 1), "bias", ("x3", "DENSE", 12, 2, 0, None, True))  # 64 + 36 columns
_add(g3(G_TILES[12], "DENSE", "LSTM", 0, 1), "gate", ("x3", "DENSE", 12, 2, 0, True))
_add(g3(G_TILES[10], "ROUTING_ENC", "BIAS", 0, 1), "bias", ("x3", "ROUTING_ENC", -1, 2, 0, None, False),
     ("x3", "ROUTING_ENC", -1, 0, 0, None, False))  # always on 16x16x32, whatever gm_gemm_set_mfma says
_add(g3(G_TILES[10], "ROUTING_ENC", "CHAIN", 0, 1), "chain", (10, 32))
for _tile, _t in K3_BIAS.items():
    for _mode in ("DENSE", "READOUT", "AGGREGATE"):
        _add(g1("k_gemm3", _t, _mode, "BIAS"), "bias", ("x3", _mode, _tile, 2, 0, None, False))
_add(g1("k_gemm3", K3_BIAS[0], "DENSE", "BIAS"), "bias", ("x3", "DENSE", -1, 2, 0, 33, False),
     ("x3", "DENSE", -1, 2, 0, None, True), ("x3", "DENSE", -1, 2, 1, None, False), ("x3", "DENSE", -1, 2, 2, None, False))
_add(g1("k_gemm3", (1, 1, 1, 1, 16), "DENSE", "BIAS"), "bias", ("x3", "DENSE", -1, 2, 0, 32, False),
     ("x3", "DENSE", 9, 2, 0, 5, False))
for _tile, _t in K3_LSTM.items():
    for _mode in ("DENSE", "AGGREGATE"):
        _add(g1("k_gemm3", _t, _mode, "LSTM"), "gate", ("x3", _mode, _tile, 2, 0, False))
_add(g1("k_gemm3", K3_LSTM[0], "DENSE", "LSTM"), "gate", ("x3", "DENSE", -1, 2, 0, True))
_add(g1("k_gemm3", K3_BIAS[0], "DENSE", "DGRAD"), "dgrad", (0, 2, False), (0, 2, True))
for _tile, _t in K1_BIAS.items():
    for _mode in ("DENSE", "READOUT"):
        _add(g1("k_gemm", _t, _mode, "BIAS", _t[5]), "bias", ("f32", _mode, _tile, 2, 0, None, False))
    _add(g1("k_gemm", K1_BIAS[0], "AGGREGATE", "BIAS"), "bias", ("f32", "AGGREGATE", _tile, 2, 0, None, False))
_add(g1("k_gemm", K1_BIAS[3], "DENSE", "BIAS"), "bias", ("f32", "DENSE", -1, 2, 0, 33, False),
     ("f32", "DENSE", -1, 2, 0, None, True))
_add(g1("k_gemm", (4, 1, 1, 1, 32), "DENSE", "BIAS"), "bias", ("f32", "DENSE", -1, 2, 0, 32, False),
     ("f32", "DENSE", 1, 2, 0, 5, False))
for _tile, _t in K1_LSTM.items():
    for _mode in ("DENSE", "AGGREGATE"):
        _add(g1("k_gemm", _t, _mode, "LSTM", _t[5]), "gate", ("f32", _mode, _tile, 2, 0, False))
_add(g1("k_gemm", K1_LSTM[-1], "DENSE", "LSTM", 4), "gate", ("f32", "DENSE", 1, 2, 0, True))
_add(g3(G_TILES[12], "DENSE", "HEAD", 0, 1), "head", (2, False, 130), (2, False, 256))
_add(g3(G_TILES[10], "DENSE", "HEAD", 0, 1), "head", (2, False, 100))
_add(g3(G_TILES[10], "DENSE", "HEAD", 0, 0), "head", (1, False, 130), (0, False, 100))
_add(g3(G_TILES[10], "DENSE", "HEAD", 1, 1), "head", (2, True, 130), (2, True, 100))
_add(g3(G_TILES[10], "DENSE", "HEAD", 1, 0), "head", (1, True, 130))
# weight gradients: 4 tiles (132 x 132, or 132 x 260 in 256-wide tiles); 84 batch rows = 2 chunks (grid % 8 == 0:
# XCD-grouped unless form + 8), 148 = 3 chunks (grid % 8 != 0: dispatch order)
_add("k_gemm3_kmajor", "wgrad", (0, 132, 148, "plain"), (8, 132, 84, "plain"), (0, 260, 84, "plain"))
for _f, _mfw in ((1, 0), (3, 1)):
    _add(f"k_wgrad_tr<128,{_mfw}>/xcd", "wgrad", (_f, 132, 84, "plain"), (_f, 164, 84, "two"), (_f, 164, 84, "map"))
    _add(f"k_wgrad_tr<128,{_mfw}>", "wgrad", (_f, 132, 148, "plain"), (_f + 8, 132, 84, "plain"), (_f, 164, 148, "map"),
         (_f + 8, 164, 84, "two"))
_add("k_wgrad_tr<128,0>/xcd", "wgrad", (-1, 132, 84, "plain"))
_add("k_wgrad_tr<256,0>/xcd", "wgrad", (2, 260, 84, "plain"))
_add("k_wgrad_tr<256,0>", "wgrad", (2, 260, 148, "plain"), (10, 260, 84, "plain"))

# names the library was compiled to launch that no argument combination selects, with the reason
UNREACHABLE = {
    g3(G_TILES[12], "DENSE", "HEAD", 0, 0):
        "gm_gemm_x3_head takes the 128x128 two-column-block form only when gm_gemm_set_mfma is 2 and passes that as "
        "its MFMA form; launch_g compiles both MFMA forms of every non-ROUTING_ENC tile",
}


def cases(test):
    return [(k,) + p for k, (t, ps) in CASES.items() if t == test for p in ps]


# ---------------------------------------------------------------------------------------------------------
# CPU: the CASES table against the instantiations the library was compiled for
# ---------------------------------------------------------------------------------------------------------
def test_every_compiled_instantiation_has_a_case(gm):
    """gm_gemm_kernel_name lists exactly the instantiations launch / launch_g were compiled for plus the
    weight-gradient forms (no GPU needed); every one is in CASES or in UNREACHABLE with a reason."""
    names = gm._lib.gemm_kernel_names()
    assert len(names) == len(set(names)) and len(names) > 100, len(names)
    names = set(names)
    assert gm._lib.lib().gm_gemm_kernel_name(-1) is None
    assert not set(CASES) & set(UNREACHABLE)
    assert names - set(CASES) - set(UNREACHABLE) == set(), "compiled instantiations without a case"
    assert (set(CASES) | set(UNREACHABLE)) - names == set(), "stale names in CASES / UNREACHABLE"
    assert all(ps for _, ps in CASES.values())
    assert all(isinstance(r, str) and r for r in UNREACHABLE.values())
    assert {t for t, _ in CASES.values()} == {"bias", "gate", "dgrad", "head", "chain", "wgrad"}


# ---------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------
PAD = 1e6  # input padding columns and guard rows: must reach no product and no published max
ROWS = {32: (3, 23), 128: (11, 15), 256: (27, 11)}  # BM -> (graphs, rows per graph): G * R = BM + 37 (256: + 41)


def mods():
    return importlib.import_module("graph-marl_amd.model"), importlib.import_module("graph-marl_amd.fused")


def tile_of(name):
    """(BM, BN) of a k_gemm / k_gemm3 / k_gemm3g name"""
    wgm, wgn, tm, tn = (int(v) for v in re.match(r"k_gemm\w*<(\d+),(\d+),(\d+),(\d+),", name).groups())
    return wgm * tm * 32, wgn * tn * 32


class Knobs:
    """sets the four process-wide knobs, restores all of them on exit"""

    def __init__(self, lib, tile=-1, mfma=2, dgrad=-1, wgrad=-1):
        self.lib, self.v = lib, (tile, mfma, dgrad, wgrad)

    def __enter__(self):
        lib, (tile, mfma, dgrad, wgrad) = self.lib, self.v
        assert lib.gm_gemm_set_tile(tile) == 0 and lib.gm_gemm_set_mfma(mfma) == 0
        assert lib.gm_gemm_set_dgrad(dgrad) == 0 and lib.gm_gemm_set_wgrad(wgrad) == 0

    def __exit__(self, *exc):
        self.lib.gm_gemm_set_tile(-1)
        self.lib.gm_gemm_set_mfma(2)
        self.lib.gm_gemm_set_dgrad(-1)
        self.lib.gm_gemm_set_wgrad(-1)
        return False


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def padded(x, ld, fill=PAD, guard=1):
    """rows of x at the start of a buffer of row stride ld filled with `fill`, one guard row behind"""
    buf = torch.full((x.shape[0] + guard, ld), fill, device="cuda", dtype=x.dtype)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf


def nan_out(rows, cols, pad=3):
    return torch.full((rows + 1, cols + pad), float("nan"), device="cuda")


def check_guard(buf, rows, cols, what):
    """payload written everywhere, padding columns and the guard row untouched"""
    assert not torch.isnan(buf[:rows, :cols]).any(), f"{what}: unwritten payload"
    assert torch.isnan(buf[:rows, cols:]).all() and torch.isnan(buf[rows:]).all(), f"{what}: wrote past its rows"


def draw(m, k, g, kind):
    """activation rows: "wide" one power of two per row in 2^-12 .. 2^3 (test_gemm_precision_gpu._operands),
    "tiny" magnitude 1e-6 with row powers 2^-6 .. 2^0 (test_input_gradient_x3_scaled), "unit" plain randn"""
    x = torch.randn(m, k, device="cuda", generator=g)
    if kind == "wide":
        x *= torch.exp2(torch.randint(-12, 4, (m, 1), device="cuda", generator=g).float())
    elif kind == "tiny":
        x *= 1e-6 * torch.exp2(torch.randint(-6, 1, (m, 1), device="cuda", generator=g).float())
    return x


def draw_w(n, k, g, kind):
    w = torch.randn(n, k, device="cuda", generator=g)
    if kind == "unit":
        return w / k ** 0.5
    return w * torch.exp2(torch.randint(-12, 1, (n, 1), device="cuda", generator=g).float())


def nbr_table(G, N, g, full=False):
    """[G, N, 3] int32 neighbour lists, ascending, no self and no repeats; unless full, some entries -1 (last)"""
    nbr = torch.full((G, N, 3), -1, dtype=torch.int32)
    cg = torch.Generator().manual_seed(int(torch.randint(0, 1 << 30, (1,), device="cuda", generator=g).item()))
    for b in range(G):
        for v in range(N):
            cnt = 3 if full else int(torch.randint(0, 4, (1,), generator=cg).item())
            others = [u for u in range(N) if u != v]
            ids = sorted(others[i] for i in torch.randperm(N - 1, generator=cg)[:cnt].tolist())
            for s, u in enumerate(ids):
                nbr[b, v, s] = u
    assert full or ((nbr < 0).any() and (nbr >= 0).any())
    return nbr.cuda()


class Src:
    """One A operand: the gm_a_src structures, the fp64 matrix the kernel should see, and the buffers"""

    def __init__(self, FU, mode, bm, g, kind, two=False, mean=False):
        self.keep = []
        self.a1 = None
        if mode == "DENSE":
            self.m = m = bm + 37
            ks = (64, 36) if two else (132,)
            xs = [draw(m, k, g, kind) for k in ks]
            bufs = [padded(x, x.shape[1] + 4) for x in xs]
            self.a0 = FU.dense(bufs[0].data_ptr(), bufs[0].stride(0), ks[0])
            if two:
                self.a1 = FU.dense(bufs[1].data_ptr(), bufs[1].stride(0), ks[1])
            self.A = torch.cat(xs, 1).double()
            self.keep += bufs
            self.x0 = bufs[0]
        elif mode == "AGGREGATE":
            G, N = ROWS[bm]
            self.m = m = G * N
            h = draw(m, 132, g, kind)
            buf = padded(h, 136)
            nbr = nbr_table(G, N, g)
            self.a0 = FU.aggregate(buf.data_ptr(), 136, 132, nbr, N, mean=mean)
            hd = h.double().view(G, N, 132)
            A = hd.clone()
            cnt = torch.ones(G, N, 1, device="cuda", dtype=torch.float64)
            bi = torch.arange(G, device="cuda")[:, None].expand(G, N)
            for s in range(3):
                nb = nbr[:, :, s].long()
                ok = (nb >= 0)[:, :, None]
                A += torch.where(ok, hd[bi, nb.clamp_min(0)], torch.zeros_like(hd))
                cnt += ok
            self.A = (A / cnt if mean else A).view(m, 132)
            self.keep += [buf, nbr]
        elif mode == "READOUT":  # [h_final[v] | h_prev[nbr(v, 0..2)]] of v = agent_node[row], then 24 dense columns
            G, R = ROWS[bm]
            N, H = 7, 32
            self.m = m = G * R
            hf, hp = draw(G * N, H, g, kind), draw(G * N, H, g, kind)
            bf, bp = padded(hf, H + 4), padded(hp, H + 8)
            nbr = nbr_table(G, N, g)
            an = torch.randint(0, N - 1, (G, R), device="cuda", generator=g).int()  # node N - 1 is nobody's
            an[:, 1] = an[:, 0]  # a repeated node
            env = draw(m, 24, g, kind)
            be = padded(env, 28)
            self.a0 = FU.readout(bf.data_ptr(), H + 4, bp.data_ptr(), H + 8, nbr, an, N, H)
            self.a1 = FU.dense(be.data_ptr(), 28, 24)
            gi = torch.arange(G, device="cuda").repeat_interleave(R)
            v = an.reshape(-1).long()
            parts = [hf[gi * N + v].double()]
            for s in range(3):
                nb = nbr[gi, v, s].long()
                t = hp[gi * N + nb.clamp_min(0)].double()
                parts.append(torch.where((nb >= 0)[:, None], t, torch.zeros_like(t)))
            self.A = torch.cat(parts + [env.double()], 1)
            self.keep += [bf, bp, nbr, an, be]
        else:  # ROUTING_ENC: A = act0(W0 x + b0) on [onehot(v) | cnt | load | 3 x (onehot(nbr) | len | load)]
            N, k = 10, 32
            G = (bm + 37 + N - 1) // N
            self.m = m = G * N
            nbr = nbr_table(G, N, g, full=True)
            x = torch.zeros(m, 4 * N + 8, device="cuda")
            rows = torch.arange(m, device="cuda")
            x[rows, rows % N] = 1.0
            x[:, N:N + 2] = torch.rand(m, 2, device="cuda", generator=g) * 3
            for s in range(3):
                off = N + 2 + s * (N + 2)
                x[rows, off + nbr.view(m, 3)[:, s].long()] = 1.0
                x[:, off + N:off + N + 2] = torch.rand(m, 2, device="cuda", generator=g) * 3
            bx = padded(x, 4 * N + 12)
            w0 = draw_w(k, 4 * N + 8, g, "unit")
            b0 = torch.randn(k, device="cuda", generator=g) * 0.1
            w0t = w0.t().contiguous()
            s = FU.ASrc()
            s.mode, s.p0, s.ld0, s.p1, s.ld1 = FU.GM_A_ROUTING_ENC, bx.data_ptr(), bx.stride(0), w0t.data_ptr(), k
            s.nbr, s.n_nodes, s.deg, s.k, s.bias0, s.act0 = nbr.data_ptr(), N, 3, k, b0.data_ptr(), 1
            self.a0 = s
            self.A = F.leaky_relu(x.double() @ w0.double().t() + b0.double())
            self.keep += [bx, w0t, b0, nbr]
        self.K = self.A.shape[1]


def rel_err(y, ref, mag):
    return ((y.double() - ref).abs() / mag.clamp_min(1e-300)).max().item()


def report(name, what, err, tol):
    print(f"{name} [{what}]: error {err:.3g}, tolerance {tol:.3g}, error / tolerance {err / tol:.3f}")
    assert err <= tol, (name, what, err, tol)


def pack_bits(b):
    """bool [m, c] -> int32 words [m, ceil(c / 32)], bit c % 32 of word c / 32"""
    m, c = b.shape
    W = (c + 31) // 32
    bb = torch.zeros(m, W * 32, dtype=torch.int64, device=b.device)
    bb[:, :c] = b
    w = (bb.view(m, W, 32) << torch.arange(32, device=b.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).int()


FILL = -559038737  # 0xDEADBEEF as int32: sign words the kernel must not touch


def weights(FU, w, form):
    wp, ldw = FU._pad_cols(w)
    return wp, ldw, (FU.X3(wp, ldw, w.shape[0], w.shape[1]) if form == "x3" else None)


def scale_of(FU, src):
    """gm_absmax_scale of the rows' real columns (the padding holds 1e6)"""
    sc = torch.empty(1, device="cuda")
    FU.L.check(FU._setup().gm_absmax_scale_rows(src.x0.data_ptr(), src.m, src.K, src.x0.stride(0), sc.data_ptr(),
                                                FU.L.stream_ptr()))
    return sc


# ---------------------------------------------------------------------------------------------------------
# forward, bias epilogues
# ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,form,mode,tile,mfma,ax,n,two", cases("bias"))
def test_forward_bias(name, form, mode, tile, mfma, ax, n, two):
    M, FU = mods()
    lib = FU._setup()
    bm, bn = tile_of(name)
    n = bn + 2 if n is None else n
    g = gen(seed_of(name, tile, mfma, ax, n, two))
    renc = mode == "ROUTING_ENC"
    src = Src(FU, mode, bm, g, "unit" if renc else "tiny" if ax == 2 else "wide", two)
    m, K = src.m, src.K
    w = draw_w(n, K, g, "unit" if renc else "wide")
    b = torch.randn(n, device="cuda", generator=g) * (1e-6 if ax == 2 else 2.0 ** -6)
    wp, ldw, x3 = weights(FU, w, form)
    pre = src.A @ w.double().t() + b.double()
    mag = src.A.abs() @ w.abs().double().t() + b.abs().double()
    amax = torch.zeros(1, device="cuda") if ax == 1 else None
    if ax == 1:
        src.a0.amax = amax.data_ptr()
    if ax == 2:
        sc = scale_of(FU, src)
        src.a0.scale = sc.data_ptr()
    # the exact-f32 form's error on the same inputs (default tile), the yardstick of the split forms' bound
    e32 = None
    if form == "x3" and not renc:
        a0 = FU.ASrc.from_buffer_copy(src.a0)
        a0.amax = a0.scale = None
        y32 = nan_out(m, n)
        FU.gemm(a0, src.a1, wp.data_ptr(), ldw, b.data_ptr(), m, n, 0, y32.data_ptr(), y32.stride(0))
        e32 = rel_err(y32[:m, :n], pre, mag)
    W = (n + 31) // 32
    for act, bits in ((0, False), (1, form == "x3")):
        y = nan_out(m, n)
        sb = torch.full((m + 1, W + 1), FILL, dtype=torch.int32, device="cuda") if bits else None
        if amax is not None:
            amax.zero_()
        with Knobs(lib, tile=tile, mfma=mfma):
            FU.gemm(src.a0, src.a1, wp.data_ptr(), ldw, b.data_ptr(), m, n, act, y.data_ptr(), y.stride(0),
                    ldc=W + 1, act_out=None if sb is None else sb.data_ptr(), x3=x3)
            assert FU.L.last_kernel() == name
        torch.cuda.synchronize()
        check_guard(y, m, n, name)
        ref = F.leaky_relu(pre) if act else pre
        if renc:  # absolute, as test_routing_encoder_fold_matches_two_kernels
            report(name, f"act {act}", (y[:m, :n].double() - ref).abs().max().item(), 1e-5)
        elif form == "x3":
            report(name, f"act {act}", rel_err(y[:m, :n], ref, mag), max(1e-6, 2.0 * e32))
        else:
            report(name, f"act {act}", rel_err(y[:m, :n], ref, mag), 2e-6)
        if bits:
            assert torch.equal(sb[:m, :W], pack_bits(y[:m, :n] > 0)), f"{name}: sign bits != (y > 0)"
            assert (sb[:m, W:] == FILL).all() and (sb[m:] == FILL).all(), f"{name}: sign words past ceil(n / 32)"
        if amax is not None:
            assert amax.view(torch.int32).item() == src.A.abs().max().float().view(torch.int32).item(), \
                f"{name}: published max |A|"
    assert FU.L.range_status() == 0


# ---------------------------------------------------------------------------------------------------------
# forward, gate epilogues (LSTM and GRU cells)
# ---------------------------------------------------------------------------------------------------------
def ungate(pre, H):
    """[m, 4H] in the packed order (row 128 t + 32 g + u = gate g of unit 32 t + u) -> four [m, H]"""
    p = pre.view(pre.shape[0], H // 32, 4, 32)
    return [p[:, :, q].reshape(pre.shape[0], H) for q in range(4)]


@gpu
@pytest.mark.parametrize("name,form,mode,tile,mfma,ax,two", cases("gate"))
def test_forward_gates(name, form, mode, tile, mfma, ax, two):
    M, FU = mods()
    lib = FU._setup()
    bm, bn = tile_of(name)
    H = 96 if bn == 256 else 32
    n = 4 * H
    g = gen(seed_of(name, tile, mfma, ax, two))
    src = Src(FU, mode, bm, g, "tiny" if ax == 2 else "unit", two, mean=True)
    m, K = src.m, src.K
    # (tiny operands: weights of magnitude 1e6, so the gates still depend on the products)
    w = draw_w(n, K, g, "unit") * (2.0 ** 20 if ax == 2 else 1.0)
    b = torch.randn(n, device="cuda", generator=g) * 0.1
    wp, ldw, x3 = weights(FU, w, form)
    gates = ungate(src.A @ w.double().t() + b.double(), H)
    c = torch.randn(m, H, device="cuda", generator=g)
    cb = padded(c, H + 4)
    amax = torch.zeros(1, device="cuda") if ax == 1 else None
    if ax == 1:
        src.a0.amax = amax.data_ptr()
    if ax == 2:
        sc = scale_of(FU, src)
        src.a0.scale = sc.data_ptr()
    for cell in ("lstm", "gru"):
        y, y2, ao = nan_out(m, H), nan_out(m, H, pad=5), nan_out(m, 4 * H, pad=0)
        if amax is not None:
            amax.zero_()
        with Knobs(lib, tile=tile, mfma=mfma):
            if cell == "lstm":
                FU.gemm(src.a0, src.a1, wp.data_ptr(), ldw, b.data_ptr(), m, n, FU.GM_EPI_LSTM, y.data_ptr(), y.stride(0),
                        y2.data_ptr(), y2.stride(0), cb.data_ptr(), cb.stride(0), ao.data_ptr(), x3=x3)
            else:
                FU.gemm(src.a0, src.a1, wp.data_ptr(), ldw, b.data_ptr(), m, n, FU.GM_EPI_GRU, y.data_ptr(), y.stride(0),
                        None, 0, cb.data_ptr(), cb.stride(0), None, x3=x3)
            assert FU.L.last_kernel() == name
        torch.cuda.synchronize()
        check_guard(y, m, H, name)
        cd = c.double()
        if cell == "lstm":
            gi, gf, gg, go = gates[0].sigmoid(), gates[1].sigmoid(), gates[2].tanh(), gates[3].sigmoid()
            cn = gf * cd + gi * gg
            check_guard(y2, m, H, name)
            check_guard(ao, m, 4 * H, name)
            report(name, "lstm c'", (y2[:m, :H].double() - cn).abs().max().item(), 1e-5)
            report(name, "lstm h'", (y[:m, :H].double() - go * cn.tanh()).abs().max().item(), 1e-5)
            report(name, "lstm gates", (ao[:m].double() - torch.cat([gi, gf, gg, go], 1)).abs().max().item(), 1e-5)
        else:
            rg, zg = gates[0].sigmoid(), gates[1].sigmoid()
            ng = (gates[2] + rg * gates[3]).tanh()
            report(name, "gru h'", (y[:m, :H].double() - ((1 - zg) * ng + zg * cd)).abs().max().item(), 1e-5)
        if amax is not None:
            assert amax.view(torch.int32).item() == src.A.abs().max().float().view(torch.int32).item(), \
                f"{name}: published max |A|"
    assert FU.L.range_status() == 0


# ---------------------------------------------------------------------------------------------------------
# input gradient
# ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,form,mfma,scaled", cases("dgrad"))
def test_dgrad(name, form, mfma, scaled):
    M, FU = mods()
    lib = FU._setup()
    bm, bn = tile_of(name)
    assert bm == 128  # part rows are 128-row tiles
    n = bn + 2
    split = n - 30
    g = gen(seed_of(name, form, mfma, scaled))
    src = Src(FU, "DENSE", bm, g, "tiny" if scaled else "wide")
    m, K = src.m, src.K
    wt = draw_w(n, K, g, "wide")  # W^T [n][K]
    x3 = weights(FU, wt, "x3")[2]
    if scaled:
        sc = scale_of(FU, src)
        src.a0.scale = sc.data_ptr()
    D = src.A @ wt.double().t()
    mag = src.A.abs() @ wt.abs().double().t()
    mask = torch.rand(m, split, device="cuda", generator=g) > 0.5
    W = (split + 31) // 32
    mb = torch.full((m + 1, W + 1), FILL, dtype=torch.int32, device="cuda")
    mb[:m, :W] = pack_bits(mask)
    nt = (m + 127) // 128
    for full in (True, False):
        sp = split if full else n
        y, y2 = nan_out(m, sp), nan_out(m, n - split, pad=5)
        part = torch.full((nt + 1, sp), float("nan"), device="cuda")
        gmax = torch.zeros(1, device="cuda")
        with Knobs(lib, mfma=mfma, dgrad=form):
            FU.L.check(lib.gm_gemm_x3_dgrad(C.byref(src.a0), x3.wp.data_ptr(), x3.sinv.data_ptr(), m, n, sp,
                                            mb.data_ptr() if full else None, W + 1 if full else 0, y.data_ptr(),
                                            y.stride(0), y2.data_ptr() if full else None, y2.stride(0) if full else 0,
                                            part.data_ptr() if full else None, gmax.data_ptr() if full else None,
                                            FU.L.stream_ptr()))
            assert FU.L.last_kernel() == name
        torch.cuda.synchronize()
        check_guard(y, m, sp, name)
        ref = D[:, :sp] * (mask.double() * 0.99 + 0.01) if full else D
        report(name, "masked" if full else "bare", rel_err(y[:m, :sp], ref, mag[:, :sp]), 4e-6)
        if full:
            check_guard(y2, m, n - split, name)
            report(name, "y2", rel_err(y2[:m, :n - split], D[:, split:], mag[:, split:]), 4e-6)
            assert not torch.isnan(part[:nt]).any() and torch.isnan(part[nt:]).all(), f"{name}: part rows"
            yd = F.pad(y[:m, :sp].double(), (0, 0, 0, nt * 128 - m)).view(nt, 128, sp)
            err = ((part[:nt].double() - yd.sum(1)).abs() / (128 * 2.0 ** -24 * yd.abs().sum(1)).clamp_min(1e-300)).max()
            report(name, "part (of the fp32 summation bound)", err.item(), 1.0)
            assert gmax.view(torch.int32).item() == y[:m, :sp].abs().max().view(torch.int32).item(), f"{name}: gmax"
    assert FU.L.range_status() == 0


# ---------------------------------------------------------------------------------------------------------
# last layer + Q head, encoder chain
# ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,mfma,with_amax,n", cases("head"))
def test_head(name, mfma, with_amax, n):
    M, FU = mods()
    lib = FU._setup()
    bm, _ = tile_of(name)
    nq = 3
    g = gen(seed_of(name, mfma, n))
    src = Src(FU, "DENSE", bm, g, "unit")
    m, K = src.m, src.K
    w, b = draw_w(n, K, g, "unit"), torch.randn(n, device="cuda", generator=g) * 0.1
    wq, bq = padded(draw_w(nq, n, g, "unit"), n + 4, guard=0), torch.randn(nq, device="cuda", generator=g) * 0.1
    x3 = weights(FU, w, "x3")[2]
    amax = torch.zeros(1, device="cuda") if with_amax else None
    if with_amax:
        src.a0.amax = amax.data_ptr()
    tol = 1e-5 * max(1.0, K ** 0.5 / 8)  # test_fused_gpu._head_case
    for act in (0, 1):
        q, y = nan_out(m, nq, pad=1), nan_out(m, n)
        if amax is not None:
            amax.zero_()
        with Knobs(lib, mfma=mfma):
            FU.L.check(lib.gm_gemm_x3_head(C.byref(src.a0), x3.wp.data_ptr(), x3.sinv.data_ptr(), b.data_ptr(), m, n,
                                           act, wq.data_ptr(), wq.stride(0), bq.data_ptr(), nq, q.data_ptr(), q.stride(0),
                                           y.data_ptr(), y.stride(0), FU.L.stream_ptr()))
            assert FU.L.last_kernel() == name
        torch.cuda.synchronize()
        check_guard(y, m, n, name)
        check_guard(q, m, nq, name)
        hid = src.A @ w.double().t() + b.double()
        hid = F.leaky_relu(hid) if act else hid
        qref = hid @ wq[:, :n].double().t() + bq.double()
        report(name, f"hidden, act {act}", (y[:m, :n].double() - hid).abs().max().item(), tol)
        report(name, f"q, act {act}", (q[:m, :nq].double() - qref).abs().max().item(), tol * max(1.0, n ** 0.5 / 8))
        if amax is not None:
            assert amax.view(torch.int32).item() == src.A.abs().max().float().view(torch.int32).item()
    assert FU.L.range_status() == 0


@gpu
@pytest.mark.parametrize("name,N,k", cases("chain"))
def test_encoder_chain(name, N, k):
    M, FU = mods()
    lib = FU._setup()
    bm, _ = tile_of(name)
    g = gen(N + k)
    src = Src(FU, "ROUTING_ENC", bm, g, "unit")
    m = src.m
    w2, b2 = draw_w(256, k, g, "unit"), torch.randn(256, device="cuda", generator=g) * 0.1
    w3, b3 = draw_w(128, 256, g, "unit"), torch.randn(128, device="cuda", generator=g) * 0.1
    x2, x3 = weights(FU, w2, "x3")[2], weights(FU, w3, "x3")[2]
    y = nan_out(m, 128)
    with Knobs(lib):
        FU.L.check(lib.gm_encoder_x3(C.byref(src.a0), x2.wp.data_ptr(), x2.sinv.data_ptr(), b2.data_ptr(), 1,
                                     x3.wp.data_ptr(), x3.sinv.data_ptr(), b3.data_ptr(), 1, m, 256, 128, y.data_ptr(),
                                     y.stride(0), FU.L.stream_ptr()))
        assert FU.L.last_kernel() == name
    torch.cuda.synchronize()
    check_guard(y, m, 128, name)
    ref = F.leaky_relu(F.leaky_relu(src.A @ w2.double().t() + b2.double()) @ w3.double().t() + b3.double())
    report(name, "layer 3", (y[:m, :128].double() - ref).abs().max().item(), 1e-5)  # test_encoder_chain_matches_..
    assert FU.L.range_status() == 0


# ---------------------------------------------------------------------------------------------------------
# weight gradient (through ctypes: model._wgrad2 refuses fewer than 4 096 batch rows)
# ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,form,n,k,kind", cases("wgrad"))
def test_wgrad(name, form, n, k, kind):
    M, FU = mods()
    lib = FU._setup()
    L = FU.L
    m, kchunk = 132, 64
    S = (k + kchunk - 1) // kchunk
    g = gen(seed_of(name, form, n, k, kind))
    gy = draw(k, m, g, "unit") * 1e-5
    ga = padded(gy, m + 4)
    sa = M._gy_scale(gy.contiguous())
    n1 = n if kind == "plain" else 128
    n2 = n - n1
    # B sources: (rows, period, shift); "map": source 1 repeats its 64 rows, source 2 lags by one chunk
    maps = [(64, 64, 0), (k - 64, 0, -64)] if kind == "map" else [(k, 0, 0), (k, 0, 0)]
    specs, refs, mags, keep = [], [], [], []
    r = torch.arange(k, device="cuda")
    for (rows, per, sh), nb, mg in zip(maps, (n1, n2), (1.0, 3e-3)):
        if nb == 0:
            continue
        x = draw(rows, nb, g, "unit") * mg
        bx = padded(x, nb + 4)
        sb = torch.empty(1, device="cuda")
        L.check(lib.gm_absmax_scale_rows(bx.data_ptr(), rows, nb, bx.stride(0), sb.data_ptr(), L.stream_ptr()))
        specs.append(L.WgradSrc(bx.data_ptr(), bx.stride(0), sb.data_ptr(), per, sh, rows))
        sr = (r % per if per else r) + sh  # batch row -> source row, zero outside [0, rows)
        xr = torch.where(((sr >= 0) & (sr < rows))[:, None], x[sr.clamp(0, rows - 1)].double(), 0.0)
        refs.append(gy.double().t() @ xr)
        mags.append(gy.abs().double().t() @ xr.abs())
        keep += [bx, sb]
    c = torch.full((S * m + 1, n + 4), float("nan"), device="cuda")
    with Knobs(lib, wgrad=form):
        L.check(lib.gm_gemm_x3_wgrad2(ga.data_ptr(), ga.stride(0), C.byref(specs[0]), n1,
                                      C.byref(specs[1]) if n2 else None, n2, m, k, kchunk, sa.data_ptr(), c.data_ptr(),
                                      c.stride(0), L.stream_ptr()))
        assert L.last_kernel() == name
    torch.cuda.synchronize()
    check_guard(c, S * m, n, name)
    got = c[:S * m, :n].double().view(S, m, n).sum(0)
    report(name, kind, rel_err(got, torch.cat(refs, 1), torch.cat(mags, 1)), 4e-6)


@gpu
@pytest.mark.parametrize("form", [0, 2])
def test_wgrad_pair_falls_back_when_the_form_takes_one_source(form):
    """model._wgrad2 returns None when the selected kernel form (gm_gemm_set_wgrad 0 / 2) refuses two sources, so
    _wgrad_pair runs one launch per source: the fp64 comparison of test_weight_gradient_two_sources at the
    smallest batch _wgrad2 accepts."""
    M, FU = mods()
    lib = FU._setup()
    L = FU.L
    Mb, o, k1, ld1, k2, ld2 = 4096, 132, 128, 128, 36, 40
    g = gen(form)
    gy = draw(Mb, o, g, "unit") * 1e-5
    x1 = draw(Mb, ld1, g, "unit")
    x2 = draw(Mb, ld2, g, "unit") * 3e-3
    s = [torch.empty(1, device="cuda") for _ in range(3)]
    L.check(lib.gm_absmax_scale(gy.data_ptr(), gy.numel(), s[0].data_ptr(), L.stream_ptr()))
    L.check(lib.gm_absmax_scale_rows(x1.data_ptr(), Mb, k1, ld1, s[1].data_ptr(), L.stream_ptr()))
    L.check(lib.gm_absmax_scale_rows(x2.data_ptr(), Mb, k2, ld2, s[2].data_ptr(), L.stream_ptr()))
    with Knobs(lib, wgrad=form):
        assert M._wgrad2(gy, [(x1, k1, s[1], 0, 0), (x2, k2, s[2], 0, 0)], s[0]) is None
        r = M._wgrad_pair(gy, x1, k1, x2, k2, s[0], s[1], s[2])
        assert L.last_kernel() == ("k_gemm3_kmajor" if form == 0 else "k_wgrad_tr<256,0>")
    for got, x, k in zip(r, (x1, x2), (k1, k2)):
        assert got.shape == (o, k)
        ref = gy.double().t() @ x[:, :k].double()
        mag = gy.abs().double().t() @ x[:, :k].abs().double()
        report(f"_wgrad_pair form {form}", f"k {k}", rel_err(got, ref, mag), 4e-6)
