"""Both instances of the edge-weight change kernel (k_env_reweigh<64>: N <= 64, one source per lane; <128>: lanes own
two sources) in every mode and at the boundary sizes, against an expectation computed from the env's own dumped
state (tests/edge_change_util.py: numpy's draws from the restored stream, a plain Dijkstra with networkx's tie rule,
the three proportions as quotients of float64). Nothing here has a tolerance: integers and fp64 quotients of integers.

Set-up of every case: A = 5 packets, per-env seeds, `resets` resets, 3 steps of taped random actions, a state dump,
the call with env_mask selecting every other env, a second dump. Selected envs: edge_len, the stream afterwards,
apsp, the first hops of every env, get_node_aux and the three proportions (as uint64) equal the expectation, the
packets and loads are untouched; the other envs' state is untouched and their stats rows are zero.

(instance, mode, N) -> the case that runs it. <64>: N = 4 (E = 6), 20, 64 (every lane busy); <128>: N = 66 (lanes
0-1 own two sources), 100, 128 (path sums up to 127 * 255 in int16).

    mode                 <64>: N = 4, 20, 64              <128>: N = 66, 100, 128
    shuffle              test_change[N-shuffle]           test_change[N-shuffle]
    randint(1, 6)        test_change[N-randint-1-6]       test_change[N-randint-1-6]
    randint(1, 256)      test_change[N-randint-1-256]     test_change[N-randint-1-256]
    randint(255, 256)    test_change[N-randint-255-256]   test_change[N-randint-255-256]   (every edge 255, no draw)
    set 255, edge there  test_change[N-set-255]           test_change[N-set-255]           (the last edge of env 0)
    set, edge absent     test_change[N-set-absent]        test_change[N-set-absent]

    MT block crossed inside the call:  test_block_crossing[128-shuffle] (<128>), test_block_crossing[20-randint] (<64>)
    tied shortest paths, randint(1, 3): test_tied_paths[20] (<64>), test_tied_paths[100] (<128>)
    what step / observe / shortest-path read after randint(200, 256): test_later_kernels[20], [128]
    arguments the host check refuses: test_refused_arguments

CASES holds the same table for tests/test_edge_change_ref.py, which checks on the CPU (with the C oracle's replay of
the set-up) that no triple is without a case and that the recorded seeds of the block-crossing and tie cases meet
their preconditions; the GPU cases assert the same preconditions on the dumped state.
"""
import importlib

import numpy as np
import pytest
import torch

import edge_change_util as U
from shortest_path_ref import first_hop_table, shortest_path_actions
from test_edge_change_gpu import _env, _first_hops

gpu = pytest.mark.gpu
A = 5
STEPS = 3
INVALID_ARG = -1
INSTANCE = {4: 64, 20: 64, 64: 64, 66: 128, 100: 128, 128: 128}
MODES = {  # id -> (mode, arguments; the one-edge cases take their edge from the dump)
    "shuffle": ("shuffle", {}),
    "randint-1-6": ("randint", {"low": 1, "high": 6}),
    "randint-1-256": ("randint", {"low": 1, "high": 256}),
    "randint-255-256": ("randint", {"low": 255, "high": 256}),
    "set-255": ("set", {"length": 255}),
    "set-absent": ("set", {"length": 7}),
}
CASES = {(INSTANCE[n], m, n): [("test_change", f"{n}-{m}")] for n in INSTANCE for m in MODES}
CASES[(128, "shuffle", 128)].append(("test_block_crossing", "128-shuffle"))
CASES[(64, "randint-1-6", 20)].append(("test_block_crossing", "20-randint"))

# Block crossing: (N, mode id) -> (resets, env seeds). After `resets` resets and the 3 steps every env's stream stands
# fewer than E - 1 words before the end of its block, and the call draws at least E - 1 words. Seeds found by
# replaying the set-up on the C oracle (test_edge_change_ref.py repeats that replay).
CROSSING = {
    (128, "shuffle"): (24, [0, 1, 2, 3, 4, 5, 6, 7]),
    (20, "randint-1-6"): (22, [0, 3, 5, 11, 12, 13, 14, 15]),
}
# Ties: N -> env seeds; randint(1, 3). At least half of the selected envs end with a tied pair (two different first
# hops on paths of the shortest distance) by the restatement alone.
TIES = {20: list(range(700, 716)), 100: list(range(800, 808))}


def tape(n, B, steps=STEPS):
    return np.random.RandomState(1000 + n).randint(4, size=(steps, B, A)).astype(np.int32)


def selected(B):
    return np.arange(B) % 2 == 0


def _setup(gm, n, seeds, resets=1):
    env = _env(gm, n, A, seeds)
    for _ in range(resets):
        env.reset()
    acts = torch.as_tensor(tape(n, len(seeds)), device="cuda")
    for t in range(STEPS):
        env.step(acts[t])
    return env


def pick_edge(n, st, sel, present):
    """The last edge of env 0, or a pair of nodes that is an edge of no selected env (N = 4 is complete: a node
    outside the graph)."""
    if present:
        return int(st["edge_a"][0, -1]), int(st["edge_b"][0, -1])
    have = {(int(a), int(b)) for e in np.flatnonzero(sel) for a, b in zip(st["edge_a"][e], st["edge_b"][e])}
    free = [(a, b) for a in range(n) for b in range(a + 1, n) if (a, b) not in have]
    return free[len(free) // 2] if free else (1, n + 1)


def _change_and_check(gm, env, n, mode, kw):
    """The masked call on `env` and every assertion of the module docstring -> (dump before, dump after, expectations
    of the selected envs by env index)."""
    B = env.n_env
    sel = selected(B)
    st0 = env.get_state()
    aux0 = env.get_node_aux().cpu().numpy()
    exp = {int(b): U.expect_env(n, st0, b, mode, **kw) for b in np.flatnonzero(sel)}
    stats = env.randomize_edge_weights(mode, env_mask=torch.as_tensor(sel, device="cuda"), **kw)
    st1 = env.get_state()
    first = _first_hops(gm, env)
    aux1 = env.get_node_aux().cpu().numpy()
    assert stats.dtype == np.float64 and stats.shape == (B, 3)
    for b in range(B):
        tag = f"env {b}"
        if not sel[b]:
            for k in st0:
                np.testing.assert_array_equal(st1[k][b], st0[k][b], err_msg=f"{tag} (not selected): {k}")
            assert not stats[b].view(np.uint64).any(), f"{tag} (not selected): stats {stats[b]}"
            np.testing.assert_array_equal(aux1[b], aux0[b], err_msg=tag)
            edges = np.stack([st0["edge_a"][b], st0["edge_b"][b], st0["edge_len"][b]], -1)
            np.testing.assert_array_equal(first[b], first_hop_table(n, edges), err_msg=tag)
            continue
        x = exp[b]
        np.testing.assert_array_equal(st1["edge_len"][b], x["edge_len"], err_msg=f"{tag}: edge_len")
        U.assert_same_stream(st1["rng_key"][b], st1["rng_pos"][b], x["rs"], tag)
        np.testing.assert_array_equal(st1["apsp"][b], x["dist"], err_msg=f"{tag}: apsp")
        np.testing.assert_array_equal(first[b], x["first"], err_msg=f"{tag}: first hops")
        np.testing.assert_array_equal(aux1[b], x["dist"].astype(np.float32), err_msg=f"{tag}: node aux")
        np.testing.assert_array_equal(stats[b].view(np.uint64), x["stats"].view(np.uint64),
                                      err_msg=f"{tag}: stats {stats[b]} expected {x['stats']}")
        for k in st0:
            if k not in ("edge_len", "apsp", "rng_key", "rng_pos"):
                np.testing.assert_array_equal(st1[k][b], st0[k][b], err_msg=f"{tag}: {k}")
    return st0, st1, exp


@gpu
@pytest.mark.parametrize("n,m", [(n, m) for n in INSTANCE for m in MODES], ids=[f"{n}-{m}" for n in INSTANCE for m in MODES])
def test_change(gm, n, m):
    B = 8
    mode, kw = MODES[m]
    kw = dict(kw)
    env = _setup(gm, n, [500 + 13 * n + b for b in range(B)])
    if mode == "set":
        st = env.get_state()
        kw["edge"] = pick_edge(n, st, selected(B), present=m == "set-255")
    st0, st1, exp = _change_and_check(gm, env, n, mode, kw)
    E = 3 * n // 2
    assert st0["edge_len"].shape == (B, E)
    if m == "set-255":  # env 0 has the edge; 255 on a length of at most 5 changes it
        assert (st1["edge_len"][0] != st0["edge_len"][0]).sum() == 1 and st1["edge_len"][0, -1] == 255
    elif m == "set-absent":
        np.testing.assert_array_equal(st1["edge_len"], st0["edge_len"])
        assert not any(x["stats"].any() for x in exp.values())
    elif m == "randint-255-256":
        assert all((x["edge_len"] == 255).all() and U.words_drawn(st0["rng_key"][b], st0["rng_pos"][b], x["rs"]) == 0
                   for b, x in exp.items())
        if n == 128:  # the longest path sums the int16 tables meet
            assert max(int(x["dist"].max()) for x in exp.values()) > 255 * 8
    elif m == "randint-1-256":
        assert max(int(x["edge_len"].max()) for x in exp.values()) > 200
    else:
        assert any(x["stats"].any() for x in exp.values()), "nothing changed: the case checks nothing"


@gpu
@pytest.mark.parametrize("n,m", list(CROSSING), ids=["128-shuffle", "20-randint"])
def test_block_crossing(gm, n, m):
    """The call starts fewer than E - 1 words before the end of an MT block and draws at least E - 1: it twists
    inside the call in every selected env."""
    resets, seeds = CROSSING[(n, m)]
    mode, kw = MODES[m]
    E = 3 * n // 2
    env = _setup(gm, n, seeds, resets)
    st0, st1, exp = _change_and_check(gm, env, n, mode, kw)
    for b, x in exp.items():
        pos = int(st0["rng_pos"][b])
        assert U.MT_N - (E - 1) < pos < U.MT_N, f"env {b}: stream position {pos} before the call"
        assert pos + U.words_drawn(st0["rng_key"][b], pos, x["rs"]) > U.MT_N
        assert not np.array_equal(x["rs"].get_state()[1], st0["rng_key"][b])


@gpu
@pytest.mark.parametrize("n", list(TIES))
def test_tied_paths(gm, n):
    """randint(1, 3): lengths of 1 and 2 only, so equal-distance paths with different first hops are common and the
    first hops, predecessors and the first two proportions depend on the search's tie rule."""
    env = _setup(gm, n, TIES[n])
    st0, st1, exp = _change_and_check(gm, env, n, "randint", {"low": 1, "high": 3})
    tied = [U.has_tied_pair(n, np.stack([st0["edge_a"][b], st0["edge_b"][b], x["edge_len"]], -1), x["dist"])
            for b, x in exp.items()]
    assert 2 * sum(tied) >= len(tied), f"{sum(tied)} of {len(tied)} selected envs have a tied pair"


@gpu
@pytest.mark.parametrize("n", [20, 128])
def test_later_kernels(gm, n):
    """After randint(200, 256) in every env: the shortest-path policy, the node observation and the step kernel read
    the new lengths from the one-byte topology image."""
    B = 8
    E = 3 * n // 2
    env = _setup(gm, n, [900 + b for b in range(B)])
    st0 = env.get_state()
    env.randomize_edge_weights("randint", low=200, high=256)
    st = env.get_state()
    for b in range(B):
        want, _ = U.draw_lengths(st0["edge_a"][b], st0["edge_b"][b], st0["edge_len"][b], st0["rng_key"][b],
                                 st0["rng_pos"][b], "randint", low=200, high=256)
        np.testing.assert_array_equal(st["edge_len"][b], want)
    ln = st["edge_len"]
    assert ln.min() >= 200 and 250 <= ln.max() <= 255
    # 5 different (now, target) pairs per env, now != target, nobody on an edge, no load
    rs = np.random.RandomState(n)
    pairs = np.stack([rs.choice(n * (n - 1), A, replace=False) for _ in range(B)])
    now, off = pairs // (n - 1), pairs % (n - 1)
    target = off + (off >= now)
    assert (now != target).all()
    env.set_state({"now": now, "target": target, "edge": np.full((B, A), -1), "time": np.zeros((B, A)),
                   "loads": np.zeros((B, E))})
    nbr = env.nbr.cpu().numpy()
    act = env.shortest_path_actions(torch.zeros(B, A, dtype=torch.int32, device="cuda")).cpu().numpy()
    for b in range(B):
        edges = np.stack([st["edge_a"][b], st["edge_b"][b], ln[b]], -1)
        np.testing.assert_array_equal(act[b], shortest_path_actions(now[b], target[b], nbr[b], first_hop_table(n, edges)))
    assert (act > 0).all()
    nobs = env.get_node_observation().cpu().numpy()
    blocks = nobs[:, :, n + 2:].reshape(B, n, 3, n + 2)  # per node: 3 neighbour blocks of onehot | length | load
    np.testing.assert_array_equal(blocks[..., n], ln[np.arange(B)[:, None, None], st["nbr_edge"]].astype(np.float32))
    # one step (routing.py:380-412, 444-453): in packet order a packet is admitted to its edge unless the edge's load
    # plus its size exceeds 1; an admitted packet gets edge = the edge, now = its far end, time = the edge's length,
    # and the same step's second phase takes 1 off: time = length - 1 in the dump (>= 199: still on the edge)
    s0 = env.get_state()
    rows = np.arange(B)[:, None]
    chosen = s0["nbr_edge"][rows, now, act - 1]
    load = np.zeros((B, E))
    entered = np.zeros((B, A), bool)
    for b in range(B):
        for i in range(A):
            c = chosen[b, i]
            if load[b, c] + s0["size"][b, i] > 1.0:
                continue
            load[b, c] = load[b, c] + s0["size"][b, i]
            entered[b, i] = True
    assert entered.any(axis=1).all() and entered.sum() >= 4 * B
    far = st["edge_a"][rows, chosen] ^ st["edge_b"][rows, chosen] ^ now
    np.testing.assert_array_equal(far, nbr[rows, now, act - 1])
    length = ln[rows, chosen]
    env.step(torch.as_tensor(act, device="cuda"))
    s = env.get_state()
    np.testing.assert_array_equal(s["edge"], np.where(entered, chosen, -1))
    np.testing.assert_array_equal(s["time"], np.where(entered, length - 1, 0))
    np.testing.assert_array_equal(s["now"], np.where(entered, far, now))
    np.testing.assert_array_equal(s["loads"], load)
    # a packet leaves its edge at its far end exactly when the counter runs out: `length` steps after it entered
    idle = torch.zeros(B, A, dtype=torch.int32, device="cuda")
    alive = entered.copy()  # still the packet that entered (a packet that arrives at its target is respawned)
    for k in range(1, int(ln.max()) + 1):
        done = env.step(idle)[3].cpu().numpy()
        s = env.get_state()
        on = alive & (k < length - 1)
        out = alive & (k == length - 1)
        assert not done[on].any()
        np.testing.assert_array_equal(s["edge"][on], chosen[on])
        np.testing.assert_array_equal(s["time"][on], (length - 1 - k)[on])
        np.testing.assert_array_equal(s["now"][on], far[on])
        np.testing.assert_array_equal(done[out], (far == target)[out])
        assert (s["edge"][out] == -1).all()
        stay = out & (far != target)
        np.testing.assert_array_equal(s["now"][stay], far[stay])
        assert (s["time"][stay] == 0).all()
        alive &= ~(out & (far == target))
    assert (s["edge"] == -1).all() and (length - 1 < k).all()


@gpu
def test_refused_arguments(gm):
    """Arguments outside the domain of the one-byte lengths: refused by the wrapper and by the C entry point, and the
    state stays as it was (nothing is launched)."""
    L = importlib.import_module("graph-marl_amd._lib")
    env = _setup(gm, 20, [41, 42])
    before = env.get_state()
    stats = torch.zeros(2, 3, dtype=torch.float64, device="cuda")
    bad = [("randint", {"low": 0, "high": 6}, (L.EDGE_RANDINT, 0, 6, 0, 0, 0)),
           ("randint", {"low": 3, "high": 3}, (L.EDGE_RANDINT, 3, 3, 0, 0, 0)),
           ("randint", {"low": 1, "high": 257}, (L.EDGE_RANDINT, 1, 257, 0, 0, 0)),
           ("set", {"edge": (2, 7), "length": 0}, (L.EDGE_SET, 0, 0, 2, 7, 0)),
           ("set", {"edge": (2, 7), "length": 256}, (L.EDGE_SET, 0, 0, 2, 7, 256)),
           ("set", {"edge": (7, 7), "length": 3}, (L.EDGE_SET, 0, 0, 7, 7, 3)),
           (None, None, (L.EDGE_SET, 0, 0, 7, 2, 3))]  # the wrapper sorts the endpoints: only the C call can say this
    for mode, kw, args in bad:
        if mode is not None:
            with pytest.raises(ValueError):
                env.randomize_edge_weights(mode, **kw)
        rc = L.lib().gm_env_randomize_edge_weights(env._h, *args, None, L.ptr(stats), L.stream_ptr(env.device))
        assert rc == INVALID_ARG, (args, rc)
        assert "randomize_edge_weights" in L.lib().gm_last_error().decode()
    torch.cuda.synchronize()
    assert not stats.any()
    after = env.get_state()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
