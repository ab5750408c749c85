"""The CPU-side helpers of test_encoder_cells_paths_gpu.py (encoder_cells_util.py) checked without a device: the
synthetic node rows against the documented layout written out row by row, the per-element rounding bound against
an fp32 restatement of the kernel's sum (inside) and against single wrong terms (outside), the share of elements
the sign-bit comparison has to leave out, the bit packing, and the LayerNorm statistics."""
import pytest
import torch

import encoder_cells_util as E


def test_node_rows_follow_the_documented_layout():
    gen = torch.Generator().manual_seed(3)
    G, N = 3, 6
    nbr = E.neighbour_table(G, N, gen)
    scal = torch.rand(G * N, 8, generator=gen) + 0.5
    x = E.node_rows(nbr, scal)
    assert x.shape == (G * N, 4 * N + 8)
    for g in range(G):
        for v in range(N):
            row = [1.0 if j == v else 0.0 for j in range(N)] + scal[g * N + v, :2].tolist()
            for k in range(3):
                u = int(nbr[g, v, k])
                row += [1.0 if j == u else 0.0 for j in range(N)] + scal[g * N + v, 2 + 2 * k:4 + 2 * k].tolist()
            assert x[g * N + v].tolist() == pytest.approx(row, abs=0), (g, v)
    assert torch.equal(E.scalars_of(x, N), scal)
    assert torch.equal(E.node_rows(nbr, E.scalars_of(x, N)), x)


def test_check_table_refuses_what_the_kernel_cannot_compute():
    gen = torch.Generator().manual_seed(4)
    nbr = E.neighbour_table(2, 8, gen)
    for bad, val in (("a missing neighbour", -1), ("an id past N", 8)):
        t = nbr.clone()
        t[1, 3, 2] = val
        with pytest.raises(AssertionError):
            E.check_table(t, 8)
    t = nbr.clone()
    t[0, 0, 1] = t[0, 0, 0]
    with pytest.raises(AssertionError):
        E.check_table(t, 8)


def test_pack_bits():
    m = torch.zeros(2, 64, dtype=torch.bool)
    m[0, 0] = m[0, 33] = m[1, 31] = True
    m[1, 32:] = True
    assert E.pack_bits(m).tolist() == [[1, 2], [-2 ** 31, -1]]


@pytest.mark.parametrize("N,G,n", E.RENC_SHAPES)
def test_bound_admits_fp32_and_rejects_a_wrong_term(N, G, n):
    """An fp32 evaluation of the 13 terms in the kernel's order stays inside the bound at every element; a
    reference with one term wrong (the two weight columns of a neighbour's scalars swapped, or a neighbour's
    one-hot row taken one row early as a -1 entry would) leaves it at most elements."""
    c = E.routing_case(N, G, n)
    for leaky in (True, False):
        y = E.routing_f32_restatement(c, leaky).double()
        ref, tol = E.act_ref(c, E.ACT_LEAKY if leaky else E.ACT_NONE)
        ratio = ((y - ref).abs() / tol).max().item()
        print(f"N={N} n={n} leaky={leaky}: max |fp32 - fp64| / bound = {ratio:.3f}")
        assert ratio <= 1.0
    off = N + 2 + 1 * (N + 2)  # neighbour 1
    w = c.w.double().clone()
    w[:, [off + N, off + N + 1]] = w[:, [off + N + 1, off + N]]
    wrong = c.x.double() @ w.t() + c.b.double()
    assert ((wrong - c.pre).abs() > c.bound).double().mean().item() > 0.99
    x = c.x.double().clone()
    r = torch.arange(G * N)
    u = c.nbr.reshape(-1, 3)[:, 0].long()
    x[r, N + 2 + u] = 0
    x[r, N + 2 + u - 1] += 1
    wrong = x @ c.w.double().t() + c.b.double()
    assert ((wrong - c.pre).abs() > c.bound).double().mean().item() > 0.99


def test_sign_comparison_leaves_out_under_one_percent():
    """Where |ref| is within its tolerance the sign of a correct result is open: those elements are left out of
    the comparison with the reference's sign (never of the comparison with the returned y). Their share, from the
    reference alone, stays far below 1 % for the seeds used."""
    worst = 0.0
    for N, G, n in E.RENC_SHAPES:
        c = E.routing_case(N, G, n)
        for act in (E.RENC_ACTS if N in E.RENC_ALL_ACTS else (E.ACT_LEAKY,)):
            share = E.excluded_share(c, act)
            print(f"N={N} n={n} act={act}: excluded share {share:.2e}")
            worst = max(worst, share)
    assert worst < 0.01


@pytest.mark.parametrize("H", [1, 33, 257])
def test_lnlstm_stats_restate_layer_norm(H):
    """mean and 1 / sqrt(var + eps) reproduce torch's layer_norm on the raw gate rows."""
    leaves = E.lnlstm_leaves(5, H, 7)
    st, mag = E.lnlstm_stats(leaves)
    gi = leaves[0].detach()
    want = torch.nn.functional.layer_norm(gi, (4 * H,), None, None, 1e-5)
    got = (gi - st[:, 0:1]) * st[:, 1:2]
    assert (got - want).abs().max().item() < 1e-12
    assert st.shape == (5, 6) and mag.shape == (5, 3) and bool((mag > 0).all())
    assert all(bool((t.detach().float().double() == t.detach()).all()) for t in leaves), "leaves hold fp32 values"
