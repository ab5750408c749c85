"""Edge-weight change during an episode (Routing.randomize_edge_weights, gm_env_randomize_edge_weights) against
the reference's Network.randomize_edge_weights (tests/golden/edge_change.npz, make_golden_edge_change.py), and
its env_mask / re-solve / shortest-path-policy behaviour on the device."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

from shortest_path_ref import first_hop_table, shortest_path_actions

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "edge_change.npz"))


def _first_hops(gm, env):
    L = importlib.import_module("graph-marl_amd._lib")
    out = torch.zeros(env.n_env, env.n_nodes, env.n_nodes, dtype=torch.int32, device=env.device)
    L.check(L.lib().gm_env_first_hops(env._h, L.ptr(out), L.stream_ptr(env.device)))
    return out.cpu().numpy()


def _env(gm, n, a, seeds):
    net = gm.Network(n, random_topology=True, excluded_seeds=gm.EVAL_SEEDS)
    return gm.Routing(net, a, n_env=len(seeds), seeds=[int(s) for s in seeds])


def _change(env, mode, set_args):
    """The case's change in every env -> stats [n_env, 3]. The one-edge cases differ per env: one masked call each."""
    if mode == "shuffle":
        return env.randomize_edge_weights("shuffle")
    if mode == "randint":
        return env.randomize_edge_weights("randint", low=1, high=6)
    out = np.zeros((env.n_env, 3), np.float64)
    for b, (ea, eb, ln) in enumerate(set_args):
        mask = torch.zeros(env.n_env, dtype=torch.bool, device=env.device)
        mask[b] = True
        if (ea, eb, ln) == (2, 7, 10):
            st = env.randomize_edge_weights("bottleneck-971182936", env_mask=mask)
        else:
            st = env.randomize_edge_weights("set", env_mask=mask, edge=(int(eb), int(ea)), length=int(ln))
        assert not st[np.arange(env.n_env) != b].any(), "an env outside the mask reports a change"
        out[b] = st[b]
    return out


@pytest.mark.parametrize("ci", range(6), ids=["6-shuffle", "6-randint", "6-set", "20-shuffle", "20-randint", "20-set"])
def test_edge_change_matches_reference(gm, golden, ci):
    g = golden
    n, mode = str(g["cases"][ci]).split(":")
    n = int(n)
    a, pre, post = (int(x) for x in g["cfg"])
    seeds = g[f"c{ci}_seeds"]
    S = len(seeds)
    assert 5 * len(g[f"c{ci}_skipped_ties"]) <= S + len(g[f"c{ci}_skipped_ties"])
    G = lambda k: np.stack([g[f"c{ci}_s{s}_{k}"] for s in range(S)])  # noqa: E731
    acts = torch.as_tensor(G("actions"), device="cuda")  # [S, pre + post, A]
    env = _env(gm, n, a, seeds)
    env.reset()
    for t in range(pre):
        env.step(acts[:, t])
    st0 = env.get_state()
    np.testing.assert_array_equal(st0["edge_len"], G("edges_before")[..., 2])
    stats = _change(env, mode, G("set_args"))
    assert isinstance(stats, np.ndarray) and stats.dtype == np.float64 and stats.shape == (S, 3)
    st = env.get_state()
    ref_edges = G("edges_after")
    np.testing.assert_array_equal(st["edge_a"], ref_edges[..., 0])
    np.testing.assert_array_equal(st["edge_b"], ref_edges[..., 1])
    np.testing.assert_array_equal(st["edge_len"], ref_edges[..., 2])
    np.testing.assert_array_equal(st["apsp"], G("apsp"))
    np.testing.assert_array_equal(env.get_node_aux().cpu().numpy(), G("apsp").astype(np.float32))
    np.testing.assert_array_equal(_first_hops(gm, env), G("first"))
    np.testing.assert_array_equal(stats.view(np.uint64), G("stats").view(np.uint64))
    # what the reference leaves: packets (a packet on an edge keeps its time), loads, visited sets
    for k in ("now", "target", "edge", "time", "size", "loads", "visited", "spw", "agent_steps"):
        np.testing.assert_array_equal(st[k], st0[k], err_msg=k)
    # the observation buffers already show the new lengths: node observation column N of each neighbour block
    nobs = env.get_node_observation().cpu().numpy()
    for b in range(S):
        for v in range(n):
            for k in range(3):
                e = st["nbr_edge"][b, v, k]
                assert nobs[b, v, n + 2 + k * (n + 2) + n] == ref_edges[b, e, 2]
    for t in range(post):
        obs, _, reward, done, _ = env.step(acts[:, pre + t])
        np.testing.assert_array_equal(reward.cpu().numpy(), G("reward")[:, t], err_msg=f"reward, step {t}")
        np.testing.assert_array_equal(done.cpu().numpy().astype(np.int8), G("done")[:, t], err_msg=f"done, step {t}")
        np.testing.assert_array_equal(obs.cpu().numpy(), G("obs")[:, t], err_msg=f"obs, step {t}")
        np.testing.assert_array_equal(env.get_node_observation().cpu().numpy(), G("node_obs")[:, t])
        s = env.get_state()  # packet resets after the change draw what the reference draws: the stream position
        np.testing.assert_array_equal(s["now"], G("now")[:, t])
        np.testing.assert_array_equal(s["target"], G("target")[:, t])
        np.testing.assert_array_equal(s["size"], G("size")[:, t])
    assert G("done").any(axis=(1, 2)).all(), "every golden run resets a packet after the change"


def test_network_delegates_and_unknown_mode(gm):
    env = _env(gm, 6, 5, [2])
    env.reset()
    with pytest.raises(ValueError, match="Unknown mode"):
        env.randomize_edge_weights("nonsense")
    # an edge the graph does not have, its node outside the graph included: the reference matches no edge,
    # re-solves and returns zeros (its bottleneck mode names the edge (2, 7), which no 6-node graph has)
    before = env.get_state()
    for mode, kw in (("set", {"edge": (0, 9), "length": 3}), ("bottleneck-971182936", {}),
                     ("set", {"edge": (0, 300), "length": 3})):
        assert not env.randomize_edge_weights(mode, **kw).any()
    after = env.get_state()
    for k in ("edge_len", "apsp", "rng_key", "rng_pos"):
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    twin = _env(gm, 6, 5, [2])
    twin.reset()
    out = env.network.randomize_edge_weights("shuffle")
    assert isinstance(out, tuple) and len(out) == 3 and all(isinstance(x, float) for x in out)
    np.testing.assert_array_equal(np.array(out), twin.randomize_edge_weights("shuffle")[0])


def _floyd(n, ea, eb, ln):
    d = np.full((n, n), 1 << 20, np.int64)
    d[np.arange(n), np.arange(n)] = 0
    d[ea, eb] = ln
    d[eb, ea] = ln
    for k in range(n):
        d = np.minimum(d, d[:, k:k + 1] + d[k:k + 1, :])
    return d


@pytest.mark.parametrize("n,mode", [(20, "shuffle"), (20, "randint"), (70, "shuffle")])
def test_env_mask_and_fresh_solve(gm, n, mode):
    """64 envs, every other one selected: the others are bit-identical to a run without the call (state and the
    next 3 steps); the selected ones hold the shortest paths of their new lengths. N = 70 runs the 128-node
    kernel instance (lanes own two sources)."""
    B, A = 64, 5
    seeds = list(range(100, 100 + B))
    x, y = _env(gm, n, A, seeds), _env(gm, n, A, seeds)
    rs = np.random.RandomState(5)
    acts = torch.as_tensor(rs.randint(4, size=(5, B, A)), device="cuda")
    for e in (x, y):
        e.reset()
        for t in range(2):
            e.step(acts[t])
    mask = (torch.arange(B, device="cuda") % 2 == 0)
    kw = {"low": 1, "high": 6} if mode == "randint" else {}
    stats = x.randomize_edge_weights(mode, env_mask=mask, **kw)
    sel = mask.cpu().numpy()
    assert not stats[~sel].any() and stats[sel].any() and (stats >= 0).all() and (stats <= 1).all()
    sx, sy = x.get_state(), y.get_state()
    for k in sx:
        np.testing.assert_array_equal(sx[k][~sel], sy[k][~sel], err_msg=k)
    if mode == "shuffle":  # a permutation of the env's lengths
        np.testing.assert_array_equal(np.sort(sx["edge_len"], -1), np.sort(sy["edge_len"], -1))
        assert (sx["edge_len"][sel] != sy["edge_len"][sel]).any()
    else:
        assert sx["edge_len"][sel].min() >= 1 and sx["edge_len"][sel].max() <= 5
    for b in np.flatnonzero(sel):
        np.testing.assert_array_equal(sx["apsp"][b], _floyd(n, sx["edge_a"][b], sx["edge_b"][b], sx["edge_len"][b]))
        edges = np.stack([sx["edge_a"][b], sx["edge_b"][b], sx["edge_len"][b]], -1)
        if b < 8:
            np.testing.assert_array_equal(_first_hops(gm, x)[b], first_hop_table(n, edges))
    # path weight changed <=> apsp entry changed, over the ordered pairs
    changed = (sx["apsp"] != sy["apsp"]).reshape(B, -1).sum(-1) / (n * (n - 1))
    np.testing.assert_array_equal(stats[:, 2], changed)
    assert (stats[:, 0] <= stats[:, 1]).all(), "a changed first hop is a changed path"
    for t in range(2, 5):
        ox, _, rx, dx, _ = x.step(acts[t])
        oy, _, ry, dy, _ = y.step(acts[t])
        assert torch.equal(ox[~mask], oy[~mask]) and torch.equal(rx[~mask], ry[~mask]) and torch.equal(dx[~mask], dy[~mask])


def test_old_weights_come_from_the_old_lengths(gm):
    """set_state with new edge_len and no apsp leaves apsp stale; the proportions still compare the paths of the
    lengths in force before the call with those after it, weights included."""
    n, B = 20, 4
    env = _env(gm, n, 5, [31, 32, 33, 34])
    env.reset()
    st = env.get_state()
    mid = st["edge_len"].copy()
    mid[:, ::2] += 3
    env.set_state({"edge_len": mid})
    stats = env.randomize_edge_weights("randint", low=1, high=6)
    s2 = env.get_state()
    for b in range(B):
        old = _floyd(n, st["edge_a"][b], st["edge_b"][b], mid[b])
        new = _floyd(n, st["edge_a"][b], st["edge_b"][b], s2["edge_len"][b])
        np.testing.assert_array_equal(s2["apsp"][b], new)
        assert stats[b, 2] == (old != new).sum() / (n * (n - 1))


def test_shortest_path_policy_takes_the_detour(gm, golden):
    """N = 6 fixture graph: the edge (a, b) is the shortest a -> b path until it gets length 40."""
    ci = 2
    g = golden
    assert str(g["cases"][ci]) == "6:set"
    seed = int(g[f"c{ci}_seeds"][0])
    a, b, ln = (int(v) for v in g[f"c{ci}_s0_set_args"])
    before, after = g[f"c{ci}_s0_edges_before"], g[f"c{ci}_s0_edges_after"]
    assert first_hop_table(6, before)[a, b] == b and first_hop_table(6, after)[a, b] != b
    env = _env(gm, 6, 5, [seed])
    env.reset()
    st = env.get_state()
    st["now"][0, :], st["target"][0, :], st["edge"][0, :], st["time"][0, :] = a, b, -1, 0
    env.set_state({k: st[k] for k in ("now", "target", "edge", "time")})
    nbr = env.nbr.cpu().numpy()[0]
    act = torch.zeros(1, 5, dtype=torch.int32, device="cuda")
    direct = env.shortest_path_actions(act).cpu().numpy()[0].copy()
    assert (nbr[a, direct - 1] == b).all()
    env.randomize_edge_weights("set", edge=(a, b), length=ln)
    detour = env.shortest_path_actions(act).cpu().numpy()[0]
    want = shortest_path_actions(np.full(5, a), np.full(5, b), nbr, first_hop_table(6, after))
    np.testing.assert_array_equal(detour, want)
    assert (nbr[a, detour - 1] != b).all()
