"""Evaluation reducer (reference src/eval.py:33-168 evaluate / get_eval_metrics) and the data behind the
reference's evaluation figures (src/eval.py:245-486 create_routing_plots).

Runs `episodes` episodes of `steps_per_episode` steps with the policy in eval mode
(ε = 0) and reduces the per-step env statistics to the reference's metrics:
  reward_mean              mean over every agent reward of every step
  delays/delays_arrived/spr_mean
                           mean over the per-packet lists (delays include the packets still
                           running at the last step, get_final_info)
  looped/throughput/dropped/blocked_mean
                           mean over the per-step counts
  + eval-only statistics (routing.py:414-441) when the env supports set_eval_info.
The n_env envs run ceil(episodes / n_env) rounds of parallel episodes; sums are kept in
fp64 on the device and read back once at the end.

Series (routing envs; `series=True` or an output directory): one gm_eval_series_step launch per step reduces
every env's step to a row of per-episode tables that stay on the device until the end (`Series`):
  series        [E, T, len(SERIES_KEYS)]  per-step values, fields in _lib.SERIES_KEYS order
  feature_diffs [E, T, S]                 per NetMon state column, mean over the nodes of |state_t - state_t-1|
  done_agents   [E, A]                    agents that ever finished in the episode
  distance_map  [E, D, 3]                 count / sum / sum of squares of the steps taken by arrived packets,
                                          keyed by their shortest-path length
Env b of round r is episode r * n_env + b. "state_t" is the NetMon state the policy acts on at step t (after
reset's start-up iterations for t = 0); state_-1 = 0 and a run without NetMon has zero drift, as in the reference.
Files (output_dir): metrics.json, series.npz (the tables, `fields`, `episodes`, `steps`, `detailed`), lzma_d.pk
(the reference's pickle, `pickle_dict`), and node_state_aux.npz with output_node_state_aux. Plots are not drawn.
"""
import math

import numpy as np
import torch

from . import _lib as L

PICKLE_KEYS = ["feature_diffs_mean", "feature_diffs_max", "throughput", "delays_arrived_mean", "looped", "reward",
               "dropped", "episode_done_agents"]
# distance-map slots: shortest-path lengths 0 .. DIST_BOUND - 2, the last slot catches anything longer
DIST_BOUND = 512


def parse_step(text):
    """A step index of an evaluation event (--eval-netmon-freeze STEP): a non-negative integer."""
    try:
        step = int(text)
    except ValueError:
        raise ValueError(f"not a step number: {text!r}") from None
    if step < 0:
        raise ValueError(f"step must be >= 0, not {step}")
    return step


def parse_edge_change(text):
    """STEP:MODE[:ARGS] (--eval-edge-change) -> (step, mode, kwargs of Routing.randomize_edge_weights):
    50:shuffle, 50:randint:LOW:HIGH, 50:set:A:B:LENGTH, 50:bottleneck-971182936. ValueError on anything else."""
    from .routing import edge_change_args

    parts = str(text).split(":")
    if len(parts) < 2:
        raise ValueError(f"expected STEP:MODE[:ARGS], not {text!r}")
    step, mode = parse_step(parts[0]), parts[1]
    want = {"shuffle": 0, "randint": 2, "set": 3, "bottleneck-971182936": 0}
    if mode not in want:
        raise ValueError(f"unknown edge-change mode {mode!r} in {text!r}")
    if len(parts) - 2 != want[mode]:
        raise ValueError(f"mode {mode} takes {want[mode]} arguments, not {len(parts) - 2}: {text!r}")
    try:
        nums = [int(x) for x in parts[2:]]
    except ValueError:
        raise ValueError(f"edge-change arguments must be integers: {text!r}") from None
    kwargs = {}
    if mode == "randint":
        kwargs = {"low": nums[0], "high": nums[1]}
    elif mode == "set":
        kwargs = {"edge": (nums[0], nums[1]), "length": nums[2]}
    edge_change_args(mode, **kwargs)  # range checks
    return step, mode, kwargs


class EdgeChange:
    """Evaluation event: Routing.randomize_edge_weights(mode, **kwargs) in every env; keeps every call's
    proportions (one call per round of parallel episodes) for metrics["edge_change"]."""

    def __init__(self, step, mode, **kwargs):
        self.step, self.mode, self.kwargs = int(step), mode, kwargs
        self.stats = []

    def __call__(self, env):
        base = env.get() if hasattr(env, "get") else env
        self.stats.append(base.randomize_edge_weights(self.mode, **self.kwargs))

    def summary(self, episodes):
        """Env b of call r is episode r * n_env + b: the mean over the first `episodes` rows."""
        p = np.concatenate(self.stats)[:episodes].mean(0) if self.stats else np.full(3, np.nan)
        return {"step": self.step, "mode": self.mode, "args": {k: list(v) if isinstance(v, tuple) else v
                                                               for k, v in self.kwargs.items()},
                "first_hops_changed": float(p[0]), "paths_changed": float(p[1]),
                "path_weights_changed": float(p[2])}


def _need_device_bytes(n, what, dev):
    free = torch.cuda.mem_get_info(dev)[0]
    if n > free:
        raise ValueError(f"evaluate: {what} needs {n} bytes ({n / 2**30:.2f} GiB) of device memory, {free} are free; "
                         "use fewer envs, episodes or steps")


class Series:
    """Device tables of the per-step series and their per-step launch (gm_eval_series_step)."""

    def __init__(self, env, episodes, steps, node_state_aux=False, dist_bound=DIST_BOUND):
        from .wrapper import NetMonWrapper

        self.env = env
        self.base = base = env.get() if hasattr(env, "get") else env
        self.E, self.T, self.D = int(episodes), int(steps), int(dist_bound)
        B, A, N, dev = base.n_env, base.n_data, base.n_nodes, base.device
        self.B, self.A, self.N, self.dev = B, A, N, dev
        netmon = getattr(env, "netmon", None)
        self.has_state = netmon is not None
        self.S = int(netmon.get_state_size()) if self.has_state else 1
        # fused wrapper: the states of step t and t - 1 are its two state buffers between the env step and the
        # NetMon step (NetMonWrapper.step_ before_netmon); anything else keeps one copy of the state per step
        self.inplace = isinstance(env, NetMonWrapper) and bool(env.fused)
        E, T, S, D = self.E, self.T, self.S, self.D
        _need_device_bytes(8 * E * (T * (L.GM_SERIES_FIELDS + S) + 3 * D) + E * A, "the series tables", dev)
        self.series = torch.zeros(E, T, L.GM_SERIES_FIELDS, dtype=torch.float64, device=dev)
        self.feature_diffs = torch.zeros(E, T, S, dtype=torch.float64, device=dev)
        self.done_agents = torch.zeros(E, A, dtype=torch.uint8, device=dev)
        self.distance_map = torch.zeros(E, D, 3, dtype=torch.float64, device=dev)
        self.detail = {"done_steps": torch.zeros(B, A, dtype=torch.int32, device=dev),
                       "done_opt": torch.zeros(B, A, dtype=torch.int32, device=dev),
                       "success": torch.zeros(B, A, dtype=torch.uint8, device=dev)}
        self.cur = self.prev = None
        self.e0 = self.n_active = 0
        self.aux = bool(node_state_aux)
        self.node_state = self.node_aux = None
        if self.aux:
            self.node_state = np.zeros((E, T, N, S), np.float32)
            self.node_aux = np.zeros((E, T, N, N), np.float32)

    def begin_round(self, r):
        self.e0 = r * self.B
        self.n_active = min(self.B, self.E - self.e0)
        self.cur = self.prev = None
        if self.aux:  # one round's states on the device, copied to the host once per round
            n = 4 * self.B * self.T * self.N * (self.S + self.N)
            self._st = self._ax = None
            _need_device_bytes(n, f"one round of node states ([{self.B}, {self.T}, {self.N}, {self.S}] + "
                                  f"[{self.B}, {self.T}, {self.N}, {self.N}] float32)", self.dev)
            self._st = torch.zeros(self.B, self.T, self.N, self.S, device=self.dev)
            self._ax = torch.zeros(self.B, self.T, self.N, self.N, device=self.dev)

    def _state(self):
        st = getattr(self.env, "current_netmon_state", None) if self.has_state else None
        return None if st is None else st.reshape(self.B, self.N, self.S)

    def step(self, actions, t):
        """One env step with the detail buffers filled, and the step's launch -> (reward, done, info) as
        env.step returns them."""
        env, base = self.env, self.base
        if self.aux:
            st = self._state()
            if st is not None:
                self._st[:, t] = st
            self._ax[:, t] = base.get_node_aux()
        if self.inplace:
            # frozen for a step or more: the policy acts on the same state as at the step before (no drift)
            env.step_(actions, self.detail, before_netmon=lambda: self._launch(
                t, env.current_netmon_state, None if t == 0 else
                env.current_netmon_state if env.frozen_steps > 0 else env.last_netmon_state))
        else:
            st = self._state()
            self.prev, self.cur = self.cur, (None if st is None else st.float().contiguous().clone())
            if hasattr(env, "step_"):
                env.step_(actions, self.detail)
            else:  # a wrapper that offers only step(): the env picks the buffers up in Routing._detail
                base.default_detail = self.detail
                try:
                    env.step(actions)
                finally:
                    base.default_detail = None
            self._launch(t, self.cur, self.prev if t > 0 else None)
        info = {k: base.info[:, i] for i, k in enumerate(L.INFO_KEYS)}
        if base.eval_info_enabled:
            info.update({k: base.eval_stats[:, i] for i, k in enumerate(L.EVAL_KEYS)})
        return base.reward, base.done.bool(), info

    def _launch(self, t, cur, prev):
        base, d = self.base, self.detail
        if cur is not None:
            assert cur.is_contiguous() and cur.dtype == torch.float32 and cur.numel() == self.B * self.N * self.S
            assert prev is None or (prev.is_contiguous() and prev.dtype == torch.float32 and
                                    prev.numel() == cur.numel())
        with L.timed("eval_series"):
            L.check(L.lib().gm_eval_series_step(
                L.ptr(cur), L.ptr(prev), self.B, self.N, self.S, L.ptr(base.reward), L.ptr(base.done), self.A,
                L.ptr(base.info), L.ptr(base.eval_stats) if base.eval_info_enabled else None,
                L.ptr(d["done_steps"]), L.ptr(d["done_opt"]), L.ptr(d["success"]), t, self.T, self.e0, self.n_active,
                self.E, L.ptr(self.series), L.ptr(self.feature_diffs), L.ptr(self.done_agents),
                L.ptr(self.distance_map), self.D, L.stream_ptr(self.dev)))

    def end_round(self):
        if self.aux:
            e0, n = self.e0, self.n_active
            self.node_state[e0:e0 + n] = self._st[:n].cpu().numpy()
            self.node_aux[e0:e0 + n] = self._ax[:n].cpu().numpy()
            self._st = self._ax = None

    def tables(self):
        """The host tables (one read-back). The distance map is cut after its longest shortest path: its last
        slot is the first empty one (still the overflow slot check_distance_map looks at)."""
        count = self.distance_map[..., 0].sum(0).cpu().numpy()  # packets per key over all episodes
        check_distance_map(count.reshape(1, -1, 1))
        keep = int(np.flatnonzero(count).max()) + 2 if count.any() else 2
        return {"series": self.series.cpu().numpy(), "feature_diffs": self.feature_diffs.cpu().numpy(),
                "done_agents": self.done_agents.cpu().numpy(),
                "distance_map": self.distance_map[:, :keep].cpu().numpy()}


def check_distance_map(distance_map):
    """Raise when the overflow slot (the last one) of a distance map [E, D, 3] holds a packet: its shortest
    path was D - 1 or longer, so the bound must grow; nothing is dropped silently."""
    if np.any(distance_map[:, -1] != 0):
        D = distance_map.shape[1]
        raise ValueError(f"evaluate: a packet's shortest path is >= {D - 1}: the distance map's bound ({D} slots) "
                         "is too small (evaluate.DIST_BOUND)")


def pickle_dict(series, done_agents):
    """The dict the reference writes to lzma_d.pk (src/eval.py:450-466): seven defaultdict(list) step -> one
    float per episode, in episode order (delays_arrived_mean only for the episodes with an arrival at that step,
    src/eval.py:302-305), and episode_done_agents float64 [E, A]. series [E, T, F] in _lib.SERIES_KEYS order."""
    from collections import defaultdict

    col = {k: i for i, k in enumerate(L.SERIES_KEYS)}
    d = {k: defaultdict(list) for k in PICKLE_KEYS[:-1]}
    E, T = series.shape[:2]
    for e in range(E):
        for t in range(T):
            row = series[e, t]
            for k in ("feature_diffs_mean", "feature_diffs_max", "reward", "dropped", "throughput", "looped"):
                d[k][t].append(float(row[col[k]]))
            if row[col["n_arrived"]] > 0:
                d["delays_arrived_mean"][t].append(float(row[col["sum_delays_arrived"]] / row[col["n_arrived"]]))
    d["episode_done_agents"] = np.asarray(done_agents, dtype=np.float64)
    return {k: d[k] for k in PICKLE_KEYS}


def write_series(output_dir, tables, detailed=False, node_state=None, node_aux=None):
    """series.npz and lzma_d.pk (and node_state_aux.npz when the node tables are given) in output_dir."""
    import lzma
    import os
    import pickle

    check_distance_map(tables["distance_map"])
    os.makedirs(output_dir, exist_ok=True)
    E, T = tables["series"].shape[:2]
    np.savez(os.path.join(output_dir, "series.npz"), fields=np.array(L.SERIES_KEYS), episodes=E, steps=T,
             detailed=bool(detailed), **tables)
    with lzma.open(os.path.join(output_dir, "lzma_d.pk"), "wb") as f:
        pickle.dump(pickle_dict(tables["series"], tables["done_agents"]), f)
    if node_state is not None:
        np.savez_compressed(os.path.join(output_dir, "node_state_aux"), node_state=node_state, node_aux=node_aux)


def evaluate(env, policy, episodes, steps_per_episode, disable_progressbar=True, output_dir=None, *,
             output_detailed=False, output_node_state_aux=False, series=None):
    """-> the metrics dict (and metrics.json in output_dir): `evaluate_events` without events, the reference's
    evaluate as it stands (its manual experiments commented out)."""
    return evaluate_events(env, policy, episodes, steps_per_episode, None, disable_progressbar, output_dir,
                           output_detailed=output_detailed, output_node_state_aux=output_node_state_aux, series=series)


@torch.no_grad()
def evaluate_events(env, policy, episodes, steps_per_episode, events=None, disable_progressbar=True, output_dir=None,
                    *, output_detailed=False, output_node_state_aux=False, series=None):
    """-> the metrics dict (and metrics.json in output_dir).

    events: list of (step, callable(env)), or None; each callable runs before the policy acts at that step of every
    round of parallel episodes (the reference's manual experiments, src/eval.py:92-103: `EdgeChange`, or
    `lambda env: env.freeze()`). An `EdgeChange` adds metrics["edge_change"]. `evaluate` keeps the reference's
    parameter list, so the events have this entry point of their own.

    series / output_dir: collect the per-step series of a routing env (module docstring); output_dir also
    writes series.npz and lzma_d.pk. A dict passed as `series` receives the host tables.
    output_node_state_aux: also write node_state_aux.npz (node_state [E, T, N, S], the NetMon state the policy
    acts on at every step, and node_aux [E, T, N, N] = get_node_aux() before the step); needs output_dir.
    output_detailed: the reference adds per-episode PNGs; no plots are drawn here and the per-episode
    throughput already is series[..., throughput], so the flag is only recorded (`detailed` in series.npz)."""
    base = env.get() if hasattr(env, "get") else env
    n_env = base.n_env
    dev = base.device
    if hasattr(policy, "eval"):
        policy.eval()
    if hasattr(env, "set_eval_info"):
        env.set_eval_info(True)
    routing = hasattr(base, "info")
    acc = {}
    ser = None
    if routing and (series or isinstance(series, dict) or output_dir is not None):
        ser = Series(env, episodes, steps_per_episode, node_state_aux=output_node_state_aux and output_dir is not None)

    def add(key, val):
        acc[key] = acc[key] + val if key in acc else val.clone()

    rounds = math.ceil(episodes / n_env)
    for r in range(rounds):
        active = torch.arange(n_env, device=dev) < (episodes - r * n_env)
        w = active.to(torch.float64)
        env.reset()
        if hasattr(policy, "reset"):  # recurrent agent models start every episode from zeros
            policy.reset(True)
        if hasattr(policy, "reset_episode"):
            policy.reset_episode()
        if ser is not None:
            ser.begin_round(r)
        for step in range(steps_per_episode):
            for at, fn in events or ():
                if at == step:
                    fn(env)
            actions = policy.act(env) if hasattr(policy, "act") else policy(env.obs)
            if ser is not None:
                reward, done, info = ser.step(actions, step)
            else:
                _, _, reward, done, info = env.step(actions)
            if step + 1 == steps_per_episode:
                info = env.get_final_info(info)
            add("reward_sum", (reward.to(torch.float64).sum(-1) * w).sum())
            add("reward_cnt", w.sum() * reward.shape[-1])
            if routing:
                for k in L.INFO_KEYS:
                    add(k, (info[k] * w).sum())
                if "total_edge_load" in info:
                    for k in L.EVAL_KEYS:
                        add(k, (info[k] * w).sum())
            add("steps", w.sum())
            if hasattr(policy, "reset"):  # reset done agents (src/eval.py:111-113)
                policy.reset(done)
        if ser is not None:
            ser.end_round()
    if hasattr(env, "set_eval_info"):
        env.set_eval_info(False)
    h = {k: float(v.item()) for k, v in acc.items()}

    def mean(s, c):
        return s / c if c > 0 else float("inf")

    metrics = {"reward_mean": mean(h["reward_sum"], h["reward_cnt"])}
    if routing:
        A = base.n_data
        metrics.update({
            "delays_mean": mean(h["sum_delays"], h["n_delays"]),
            "delays_arrived_mean": mean(h["sum_delays_arrived"], h["n_arrived"]),
            "spr_mean": mean(h["sum_spr"], h["n_arrived"]),
            "looped_mean": mean(h["looped"], h["steps"]),
            "throughput_mean": mean(h["throughput"], h["steps"]),
            "dropped_mean": mean(h["dropped"], h["steps"]),
            "blocked_mean": mean(h["blocked"], h["steps"]),
        })
        if "total_edge_load" in h:
            metrics.update({
                "total_edge_load_mean": mean(h["total_edge_load"], h["steps"]),
                "occupied_edges_mean": mean(h["occupied_edges"], h["steps"]),
                "packets_on_edges_mean": mean(h["packets_on_edges"], h["steps"]),
                "total_packet_size_mean": mean(h["total_packet_size"], h["steps"]),
                "packet_sizes_mean": mean(h["total_packet_size"], h["steps"] * A),
                "packet_distances_mean": mean(h["sum_packet_distances"], h["steps"] * A),
            })
    for _, fn in events or ():
        if isinstance(fn, EdgeChange):
            metrics["edge_change"] = fn.summary(episodes)
    tables = ser.tables() if ser is not None else None
    if isinstance(series, dict) and tables is not None:
        series.update(tables)
    if output_dir is not None:
        import json
        import os

        os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, "metrics.json"), "w") as f:
            json.dump(metrics, f, indent=4, sort_keys=True)
        if tables is not None:
            write_series(output_dir, tables, output_detailed, ser.node_state, ser.node_aux)
    return metrics
