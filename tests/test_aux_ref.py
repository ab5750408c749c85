"""CPU self-checks of the fp64 references and bounds tests/test_aux_seq_gpu.py judges the aux head kernels by
(tests/aux_util.py): each reference against an independent evaluation, each bound against the fp32 evaluation it
is derived for."""
import numpy as np
import torch

import aux_util as U


def _case(rows, cols, n_out, seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(rows, cols, generator=g)
    w2 = torch.randn(n_out, cols, generator=g) / cols ** 0.5
    b2 = torch.randn(n_out, generator=g)
    tgt = 3 * torch.rand(rows, n_out, generator=g)
    return y, w2, b2, tgt


def test_fwd_ref_matches_loops_and_bounds_fp32_chain():
    y, w2, b2, tgt = _case(7, 64, 5)
    res, eb = U.fwd_ref(y, w2, b2, tgt)
    yn, wn, bn, tn = (t.numpy() for t in (y, w2, b2, tgt))
    worst = 0.0
    for r in range(7):
        for a in range(5):
            exact = float(bn[a]) + sum(float(yn[r, c]) * float(wn[a, c]) for c in range(64)) - float(tn[r, a])
            assert abs(res[r, a].item() - exact) < 1e-12
            acc = np.float32(0)
            for c in range(64):  # ascending c in fp32, a rounded product and a rounded sum: no better than fmaf
                acc = np.float32(acc + np.float32(yn[r, c] * wn[a, c]))
            got = np.float32(np.float32(bn[a] + acc) - tn[r, a])
            worst = max(worst, abs(float(got) - exact) / eb[r, a].item())
    assert 0 < worst < 1


def test_loss_bound_covers_fp32_sum():
    y, w2, b2, tgt = _case(130, 32, 20, seed=1)
    res, eb = U.fwd_ref(y, w2, b2, tgt)
    r32 = (b2 + y @ w2.t() - tgt)  # an fp32 evaluation within eb of res
    assert ((r32.double() - res).abs() <= eb).all()
    got = float((r32 * r32).sum())
    exact = (res ** 2).sum().item()
    assert abs(got - exact) <= U.loss_bound(res, eb, r32.numel())
    assert U.loss_terms(130, 20, 64) == 8 * 1 + 6 + 2 + 3
    assert U.loss_terms(257, 128, 16) == 2 * 4 + 6 + 2 + 17


def test_bwd_ref_against_formula_and_finite_difference():
    y, w2, b2, tgt = _case(9, 32, 6, seed=2)
    z = y.clone()
    z[0, :5] = 0.0
    res = torch.randn(9, 6, generator=torch.Generator().manual_seed(3))
    s = 3.7e-4
    for act in (0, 1):
        g, gb, gw, bound = U.bwd_ref(res, w2, z, act, s)
        m = (0.01 + 0.99 * (z.double() > 0).double()) if act else torch.ones(9, 32, dtype=torch.float64)
        yy = torch.nn.functional.leaky_relu(z.double(), 0.01) if act else z.double()
        assert torch.allclose(g, s * (res.double() @ w2.double()) * m, rtol=1e-12, atol=1e-18)
        assert torch.allclose(gb, s * res.double().sum(0), rtol=1e-12, atol=1e-18)
        assert torch.allclose(gw, s * res.double().t() @ yy, rtol=1e-12, atol=1e-18)
        assert (bound > 0).all()
    # exact zeros of z take the slope, as y <= 0 does in the kernel's mask
    g, _, _, _ = U.bwd_ref(res, w2, z, 1, 1.0)
    assert torch.allclose(g[0, :5], 0.01 * (res.double() @ w2.double())[0, :5])
    # central difference of the scalar at an element away from the kink
    f = lambda zz: (res.double() * (torch.nn.functional.leaky_relu(zz, 0.01) @ w2.double().t())).sum()  # noqa: E731
    zz = z.double()
    e = torch.zeros_like(zz)
    e[3, 4] = 1e-6
    assert abs(((f(zz + e) - f(zz - e)) / 2e-6).item() - g[3, 4].item()) < 1e-6


def test_pack_bits_and_scale():
    b = torch.rand(5, 70, generator=torch.Generator().manual_seed(4)) > 0.5
    w = U.pack_bits(b)
    assert w.shape == (5, 3) and w.dtype == torch.int32
    for r in range(5):
        for c in range(70):
            assert bool((int(w[r, c // 32]) >> (c % 32)) & 1) == bool(b[r, c])
    assert U.expected_scale(0.0) == 1.0
    assert U.expected_scale(1.0) == 2.0 ** 13  # 1 is in [2^0, 2^1)
    assert U.expected_scale(0.75) == 2.0 ** 14
    assert U.expected_scale(3e-5) == 2.0 ** 29  # 3e-5 is in [2^-16, 2^-15)


def test_strided_and_untouched():
    x = torch.arange(6.0).view(2, 3)
    buf, v = U.strided(x, 5)
    assert buf.shape == (2 + U.GUARD, 5) and torch.equal(v, x) and torch.isnan(buf[:, 3:]).all()
    before = buf.clone()
    v.fill_(1.0)
    assert U.untouched(buf, before, 2, 3)
    buf[3, 0] = 0.0
    assert not U.untouched(buf, before, 2, 3)


def test_wgrad_bound_covers_the_split_f16_products():
    """The product term of wgrad_bound: operands scaled by their power of two, split into two f16 pieces, the three
    kept piece products summed exactly (fp64): the error against the exact product is the representation's and the
    dropped low x low term's, below 3 * 2^-22 of sum |a| |b|; the whole bound adds the accumulation term."""
    g = torch.Generator().manual_seed(5)
    a = torch.randn(300, 8, generator=g) * 1e-4
    b = torch.randn(300, 12, generator=g)

    def split(x):
        s = U.expected_scale(x.abs().max().item())
        hi = (x * s).half()
        lo = (x * s - hi.float()).half()
        return hi.double() / s, lo.double() / s

    (ah, al), (bh, bl) = split(a), split(b)
    got = ah.t() @ bh + ah.t() @ bl + al.t() @ bh
    exact = a.double().t() @ b.double()
    mag = a.double().abs().t() @ b.double().abs()
    worst = ((got - exact).abs() / (3 * 2.0 ** -22 * mag)).max().item()
    assert 0 < worst < 1
    assert (U.wgrad_bound(a, b) > 3 * 2.0 ** -22 * mag).all()
