"""CPU side of tests/test_edge_change_paths_gpu.py: the expectation code of tests/edge_change_util.py against Floyd,
against oracle/shortest_path_ref.first_hop_table and against the reference's goldens (tests/golden/edge_change.npz),
and the preconditions of the recorded seeds, replayed on the C oracle (no kernel runs here)."""
import importlib
import os

import numpy as np
import pytest

import edge_change_util as U
import test_edge_change_paths_gpu as G
from shortest_path_ref import first_hop_table
from test_edge_change_gpu import _floyd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cubic_graph(n, rs):
    """A random connected 3-regular simple graph (pairing model with rejection) -> (ea, eb), ea < eb, edges in the
    order the pairing made them."""
    while True:
        stubs = np.repeat(np.arange(n), 3)
        rs.shuffle(stubs)
        a, b = np.minimum(stubs[::2], stubs[1::2]), np.maximum(stubs[::2], stubs[1::2])
        if (a == b).any() or len(set(zip(a.tolist(), b.tolist()))) < len(a):
            continue
        if _floyd(n, a, b, np.ones(len(a), np.int64)).max() < n:
            return a, b


@pytest.mark.parametrize("n", [4, 6, 20, 64, 66, 128])
@pytest.mark.parametrize("lengths", [(1, 3), (1, 6), (200, 256), (255, 256)])
def test_solve_matches_floyd_and_first_hop_table(n, lengths):
    """Distances == Floyd, first hops == first_hop_table (lengths of 1 and 2 and all-equal lengths: ties everywhere),
    and the predecessors are those of the paths whose first hops these are."""
    rs = np.random.RandomState(n + lengths[0])
    for _ in range(2 if n > 64 else 4):
        ea, eb = cubic_graph(n, rs)
        ln = rs.randint(*lengths, size=len(ea))
        edges = np.stack([ea, eb, ln], -1)
        dist, first, pred = U.solve(n, edges)
        np.testing.assert_array_equal(dist, _floyd(n, ea, eb, ln))
        np.testing.assert_array_equal(first, first_hop_table(n, edges))
        w = np.full((n, n), -1, np.int64)
        w[ea, eb] = w[eb, ea] = ln
        s, t = np.nonzero(~np.eye(n, dtype=bool))
        p = pred[s, t]
        assert (w[p, t] > 0).all(), "a predecessor that is no neighbour"
        np.testing.assert_array_equal(dist[s, p] + w[p, t], dist[s, t])
        np.testing.assert_array_equal(first[s, t], np.where(p == s, t, first[s, p]))
        assert (pred[np.arange(n), np.arange(n)] == np.arange(n)).all()
        for src, row in enumerate(U.paths(pred)):
            for dst, path in enumerate(row):
                assert path[0] == src and path[-1] == dst and len(set(path)) == len(path)
                assert sum(w[x, y] for x, y in zip(path, path[1:])) == dist[src, dst]
        if lengths[1] - lengths[0] <= 2:
            assert U.has_tied_pair(n, edges, dist) or n == 4


def test_has_tied_pair():
    sq = np.array([[0, 1, 1], [1, 2, 1], [2, 3, 1], [0, 3, 1]])  # a square: two ways to the opposite corner
    assert U.has_tied_pair(4, sq, _floyd(4, sq[:, 0], sq[:, 1], sq[:, 2]))
    sq[0, 2] = 2
    assert not U.has_tied_pair(4, sq, _floyd(4, sq[:, 0], sq[:, 1], sq[:, 2]))  # the way round 0 - 1 is longer
    sq[2, 2] = 2
    assert U.has_tied_pair(4, sq, _floyd(4, sq[:, 0], sq[:, 1], sq[:, 2]))  # 0 -> 2: 2 + 1 == 1 + 2


def test_expectation_reproduces_the_reference():
    """Fed the reference's recorded lengths in place of drawn ones, the expectation gives the reference's proportions
    bit for bit, and its distances and first hops, for every recorded seed."""
    g = np.load(os.path.join(GOLDEN, "edge_change.npz"))
    seen = 0
    for ci, case in enumerate(g["cases"]):
        n = int(str(case).split(":")[0])
        for s in range(len(g[f"c{ci}_seeds"])):
            before, after = g[f"c{ci}_s{s}_edges_before"], g[f"c{ci}_s{s}_edges_after"]
            np.testing.assert_array_equal(before[:, :2], after[:, :2])
            x = U.expect_change(n, before[:, 0], before[:, 1], before[:, 2], after[:, 2])
            tag = f"{case} seed {s}"
            np.testing.assert_array_equal(x["stats"].view(np.uint64), g[f"c{ci}_s{s}_stats"].view(np.uint64), err_msg=tag)
            np.testing.assert_array_equal(x["dist"], g[f"c{ci}_s{s}_apsp"], err_msg=tag)
            np.testing.assert_array_equal(x["first"], g[f"c{ci}_s{s}_first"], err_msg=tag)
            seen += 1
    assert seen == 18


@pytest.mark.parametrize("n", [9, 30, 192])
def test_draw_lengths_and_stream(n):
    """draw_lengths consumes what numpy consumes; words_drawn and assert_same_stream across a block boundary."""
    key, pos = np.random.RandomState(n).get_state()[1:3]
    assert pos == U.MT_N
    a = U.restore_stream(key, pos)
    a.randint(0, 2**32, size=U.MT_N - 3, dtype=np.uint64)
    key, pos = a.get_state()[1:3]
    old = np.arange(1, n + 1)
    for mode, kw in (("shuffle", {}), ("randint", {"low": 1, "high": 256}), ("randint", {"low": 255, "high": 256})):
        new, rs = U.draw_lengths(np.zeros(n), np.ones(n), old, key, pos, mode, **kw)
        words = U.words_drawn(key, pos, rs)
        assert (words == 0) if kw.get("low") == 255 else (words >= n - 1 and pos + words > U.MT_N)
        b = U.restore_stream(key, pos)
        b.randint(0, 2**32, size=words, dtype=np.uint64)
        U.assert_same_stream(*b.get_state()[1:3], rs)
        b.randint(0, 2**32, size=1, dtype=np.uint64)
        with pytest.raises(AssertionError):
            U.assert_same_stream(*b.get_state()[1:3], rs)
    end = U.restore_stream(key, pos)
    end.randint(0, 2**32, size=U.MT_N - pos, dtype=np.uint64)
    k2, p2 = end.get_state()[1:3]
    assert p2 == U.MT_N
    nxt = U.restore_stream(k2, p2)
    nxt.randint(0, 2**32, size=1, dtype=np.uint64)
    k3 = nxt.get_state()[1]
    U.assert_same_stream(k3, 0, end)  # the end of a block == the start of the next one
    new, _ = U.draw_lengths([0, 2, 2], [1, 3, 7], [4, 4, 4], key, pos, "set", edge=(7, 2), length=9)
    assert new.tolist() == [4, 4, 9]


def test_every_triple_has_a_case():
    triples = {(G.INSTANCE[n], m, n) for n in (4, 20, 64, 66, 100, 128) for m in G.MODES}
    assert len(G.MODES) == 6 and len(triples) == 36 and set(G.CASES) == triples and all(G.CASES.values())
    assert {n for n, i in G.INSTANCE.items() if i == 64} == {4, 20, 64}
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "graph-marl_amd", "csrc", "gm_env.hip")).read()
    assert "inline int ncap(int n) { return n <= 64 ? 64 : 128; }" in src
    assert "k_env_reweigh<64>" in src and "k_env_reweigh<128>" in src
    for (inst, m, n), cases in G.CASES.items():
        for test, cid in cases:
            assert callable(getattr(G, test))
            assert (f"{test}[N-{m}]" if test == "test_change" else f"{test}[{cid}]") in G.__doc__


def oracle_dump(O, n, seeds, resets):
    """The GPU cases' set-up replayed on the C oracle -> a get_state()-like dict of the keys the expectation reads."""
    R = importlib.import_module("graph-marl_amd.routing")
    acts = G.tape(n, len(seeds))
    out = {k: [] for k in ("edge_a", "edge_b", "edge_len", "rng_key", "rng_pos")}
    for b, seed in enumerate(seeds):
        cfg = O.make_config(n, G.A, True, False, 0, O.TOPO_RANDOM, 476, excluded=R.EVAL_SEEDS)
        env = O.OracleEnv(cfg, int(seed))
        for _ in range(resets):
            env.reset()
        for t in range(G.STEPS):
            env.step(acts[t, b])
        edges, st = env.topology()["edges"], env.state()
        for k, v in zip(out, (edges[:, 0], edges[:, 1], edges[:, 2], st["rng_key"], st["rng_pos"])):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


@pytest.mark.parametrize("n,m", list(G.CROSSING))
def test_recorded_seeds_cross_a_block(oracle_mod, n, m):
    resets, seeds = G.CROSSING[(n, m)]
    mode, kw = G.MODES[m]
    E = 3 * n // 2
    st = oracle_dump(oracle_mod, n, seeds, resets)
    assert 2 <= len(seeds) <= 16
    for b in np.flatnonzero(G.selected(len(seeds))):
        pos = int(st["rng_pos"][b])
        assert U.MT_N - (E - 1) < pos < U.MT_N, f"env {b} (seed {seeds[b]}): stream position {pos}"
        _, rs = U.draw_lengths(st["edge_a"][b], st["edge_b"][b], st["edge_len"][b], st["rng_key"][b], pos, mode, **kw)
        assert pos + U.words_drawn(st["rng_key"][b], pos, rs) > U.MT_N


@pytest.mark.parametrize("n", list(G.TIES))
def test_recorded_seeds_have_tied_paths(oracle_mod, n):
    seeds = G.TIES[n]
    st = oracle_dump(oracle_mod, n, seeds, 1)
    assert 2 <= len(seeds) <= 16
    tied = []
    for b in np.flatnonzero(G.selected(len(seeds))):
        new, _ = U.draw_lengths(st["edge_a"][b], st["edge_b"][b], st["edge_len"][b], st["rng_key"][b], st["rng_pos"][b],
                                "randint", low=1, high=3)
        edges = np.stack([st["edge_a"][b], st["edge_b"][b], new], -1)
        tied.append(U.has_tied_pair(n, edges, U.solve(n, edges)[0]))
    assert 2 * sum(tied) >= len(tied)
