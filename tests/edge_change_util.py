"""What one edge-weight change (Network.randomize_edge_weights, src/env/network.py:292-351) must leave behind, computed
on the CPU from an env's dumped state by code that shares nothing with the kernel — TEST INFRASTRUCTURE ONLY.

The new lengths are drawn by numpy itself from the env's restored stream. The shortest paths before and after come
from a plain Dijkstra that states networkx's tie rule as oracle/shortest_path_ref.first_hop_table does: a heap of
(distance, push counter, node), a node's path replaced only on a strictly shorter distance, neighbours relaxed in
edge-creation order. It keeps the predecessors; the first hops and the whole paths are read from the predecessor
chains afterwards. tests/test_edge_change_ref.py pins it against Floyd, first_hop_table and the reference's goldens.
"""
import heapq

import numpy as np

MT_N = 624


def solve(n, edges):
    """edges: [(a, b, length)] in creation order -> (dist int64 [n, n], first int32 [n, n], pred int32 [n, n]):
    pred[s, t] is the node before t on networkx's s -> t path, first[s, t] the node after s (s, t on the diagonal)."""
    adj = [[] for _ in range(n)]
    for a, b, ln in edges:
        adj[int(a)].append((int(b), int(ln)))
        adj[int(b)].append((int(a), int(ln)))
    dist = np.zeros((n, n), np.int64)
    first = np.zeros((n, n), np.int32)
    pred = np.zeros((n, n), np.int32)
    for src in range(n):
        final, best, parent = {}, {src: 0}, {src: src}
        pushes = 0
        heap = [(0, pushes, src)]
        while heap:
            d, _, v = heapq.heappop(heap)
            if v in final:
                continue
            final[v] = d
            for u, ln in adj[v]:
                if u in final:
                    continue
                if u not in best or d + ln < best[u]:
                    best[u] = d + ln
                    parent[u] = v
                    pushes += 1
                    heapq.heappush(heap, (d + ln, pushes, u))
        assert len(final) == n, "the graph is not connected"
        for t in range(n):
            dist[src, t] = final[t]
            pred[src, t] = parent[t]
            hop = t
            while parent[hop] != src:
                hop = parent[hop]
            first[src, t] = hop
    return dist, first, pred


def paths(pred):
    """pred [n, n] -> paths[s][t]: the s -> t node tuple, as networkx lists it."""
    n = len(pred)
    out = []
    for s in range(n):
        row = {s: (s,)}

        def walk(t):
            if t not in row:
                row[t] = walk(int(pred[s, t])) + (t,)
            return row[t]

        out.append([walk(t) for t in range(n)])
    return out


def proportions(old, new):
    """(dist, first, pred) before and after -> float64 [3]: the share of the n (n - 1) ordered pairs whose first hop /
    whole path / path weight differs (network.py:331-351)."""
    n = len(old[0])
    off = ~np.eye(n, dtype=bool)
    n_first = int(((old[1] != new[1]) & off).sum())
    po, pn = paths(old[2]), paths(new[2])
    n_path = sum(po[s][t] != pn[s][t] for s in range(n) for t in range(n) if s != t)
    n_weight = int(((old[0] != new[0]) & off).sum())
    return np.array([np.float64(c) / np.float64(n * (n - 1)) for c in (n_first, n_path, n_weight)], np.float64)


def has_tied_pair(n, edges, dist):
    """Some ordered pair (s, t) has two different first hops on paths of the shortest distance."""
    ways = np.zeros((n, n), np.int64)
    for a, b, ln in edges:
        ways[a] += (ln + dist[b] == dist[a])
        ways[b] += (ln + dist[a] == dist[b])
    ways[np.arange(n), np.arange(n)] = 0
    return bool((ways >= 2).any())


def restore_stream(key, pos):
    rs = np.random.RandomState()
    rs.set_state(("MT19937", np.asarray(key, np.uint32), int(pos)))
    return rs


def draw_lengths(ea, eb, old_len, key, pos, mode, low=None, high=None, edge=None, length=None):
    """The call's new lengths, drawn by numpy from the stream (key, pos) -> (int64 [E], the RandomState afterwards)."""
    rs = restore_stream(key, pos)
    new = np.asarray(old_len, np.int64).copy()
    if mode == "shuffle":
        rs.shuffle(new)
    elif mode == "randint":
        for e in range(len(new)):
            new[e] = rs.randint(low, high)
    elif mode == "set":
        a, b = sorted(int(x) for x in edge)
        new[(np.asarray(ea) == a) & (np.asarray(eb) == b)] = length
    else:
        raise ValueError(mode)
    return new, rs


def words_drawn(key, pos, rs):
    """32-bit words between the stream (key, pos) and the later state of rs (less than two blocks apart)."""
    _, key2, pos2 = rs.get_state()[:3]
    return pos2 - pos if np.array_equal(key2, np.asarray(key, np.uint32)) else MT_N - pos + pos2


def assert_same_stream(key, pos, rs, tag=""):
    """The dumped stream (key, pos) stands where rs stands: block and position (a stream at the end of a block equals
    the next block at position 0, so there only the draws can be compared), and the next 700 draws of both."""
    _, key2, pos2 = rs.get_state()[:3]
    if pos2 < MT_N and pos < MT_N:
        assert pos == pos2, f"{tag}: stream position {pos}, numpy stands at {pos2}"
        np.testing.assert_array_equal(np.asarray(key, np.uint32), key2, err_msg=f"{tag}: stream block")
    a, b = restore_stream(key, pos), restore_stream(key2, pos2)
    np.testing.assert_array_equal(a.randint(0, 2**32, size=700, dtype=np.uint64),
                                  b.randint(0, 2**32, size=700, dtype=np.uint64), err_msg=f"{tag}: next draws")


def expect_change(n, ea, eb, old_len, new_len):
    """-> dict: edge_len, dist / first / pred after the change, stats float64 [3], and `old` = the solve before it."""
    old = solve(n, np.stack([ea, eb, old_len], -1))
    new = solve(n, np.stack([ea, eb, new_len], -1))
    return {"edge_len": np.asarray(new_len, np.int64), "dist": new[0], "first": new[1], "pred": new[2],
            "stats": proportions(old, new), "old": old}


def expect_env(n, st, b, mode, **kw):
    """expect_change for env b of a get_state() dump taken before the call; adds `rs`, numpy's stream afterwards."""
    new_len, rs = draw_lengths(st["edge_a"][b], st["edge_b"][b], st["edge_len"][b], st["rng_key"][b], st["rng_pos"][b],
                               mode, **kw)
    out = expect_change(n, st["edge_a"][b], st["edge_b"][b], st["edge_len"][b], new_len)
    out["rs"] = rs
    return out
