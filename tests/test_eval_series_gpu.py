"""Evaluation series (graph-marl_amd/evaluate.py, gm_eval_series_step in csrc/gm_eval.hip): the kernel against an
fp64 torch restatement, evaluate's tables against a recording of every step, the files of `main.py --eval`, and
the reference's lzma_d.pk / node_state_aux.npz contents (tests/golden/eval_series.npz)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENT = -7.0  # rows the kernel must not touch keep this value
DIST = 16


def _mods():
    gm = importlib.import_module("graph-marl_amd")
    return gm, gm._lib, importlib.import_module("graph-marl_amd.evaluate")


def _inputs(B, N, S, A, seed, far_key=False):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    dev = "cuda"
    r = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    d = {"cur": torch.randn(B, N, S, device=dev, generator=g), "prev": torch.randn(B, N, S, device=dev, generator=g),
         "reward": torch.randn(B, A, device=dev, generator=g),
         "info": torch.floor(r(B, 9) * 40).double(), "eval": (r(B, 5) * 10).double()}
    succ = r(B, A) < 0.4
    done = succ | (r(B, A) < 0.2)
    d["success"] = succ.to(torch.uint8)
    d["done"] = done.to(torch.uint8)
    d["done_steps"] = (torch.floor(r(B, A) * 30).int() + 1) * done.int()
    d["done_opt"] = torch.floor(r(B, A) * 12).int() + 1
    if far_key:  # one arrived packet whose shortest path is beyond the map
        d["success"][0, 0] = 1
        d["done"][0, 0] = 1
        d["done_steps"][0, 0] = 50
        d["done_opt"][0, 0] = 40
    return d


def _tables(E, T, S, A, B, e0, n_active):
    """Sentinel-filled tables; the accumulated ones start from zero in the rows of the active envs."""
    dev = "cuda"
    t = {"series": torch.full((E, T, 16), SENT, dtype=torch.float64, device=dev),
         "fd": torch.full((E, T, S), SENT, dtype=torch.float64, device=dev),
         "da": torch.full((E, A), 9, dtype=torch.uint8, device=dev),
         "dm": torch.full((E, DIST, 3), SENT, dtype=torch.float64, device=dev)}
    t["da"][e0:e0 + n_active] = 0
    t["dm"][e0:e0 + n_active] = 0
    return t


def _launch(L, d, tb, mode, B, N, S, A, t, T, e0, n_active, E):
    cur = None if mode == "none" else d["cur"]
    prev = d["prev"] if mode == "pair" else None
    L.check(L.lib().gm_eval_series_step(
        L.ptr(cur), L.ptr(prev), B, N, S, L.ptr(d["reward"]), L.ptr(d["done"]), A, L.ptr(d["info"]), L.ptr(d["eval"]),
        L.ptr(d["done_steps"]), L.ptr(d["done_opt"]), L.ptr(d["success"]), t, T, e0, n_active, E, L.ptr(tb["series"]),
        L.ptr(tb["fd"]), L.ptr(tb["da"]), L.ptr(tb["dm"]), DIST, L.stream_ptr()))
    torch.cuda.synchronize()


def _expected_rows(L, d, mode, S):
    """fp64 restatement: fp32 subtract and abs, then double means and max. -> series rows [B, 16], fd rows [B, S]."""
    B, A = d["reward"].shape
    if mode == "none":
        fd = torch.zeros(B, S, dtype=torch.float64, device="cuda")
        fmean = fmax = torch.zeros(B, dtype=torch.float64, device="cuda")
    else:
        diff = (d["cur"] - d["prev"]).abs() if mode == "pair" else d["cur"].abs()
        fd = diff.double().mean(1)
        fmean = diff.double().mean((1, 2))
        fmax = diff.amax((1, 2)).double()
    ok = d["success"].bool()
    spr = torch.where(ok, d["done_steps"].double() / d["done_opt"].double(),
                      torch.full_like(d["reward"], float("inf"), dtype=torch.float64)).amin(1)
    info = {k: d["info"][:, i] for i, k in enumerate(L.INFO_KEYS)}
    info.update({k: d["eval"][:, i] for i, k in enumerate(L.EVAL_KEYS)})
    info.update(reward=d["reward"].double().mean(1), spr_min=spr, feature_diffs_mean=fmean, feature_diffs_max=fmax)
    return torch.stack([info[k] for k in L.SERIES_KEYS], 1), fd


def _expected_dmap(d, b):
    m = np.zeros((DIST, 3))
    succ, steps, opt = (d[k][b].cpu().numpy() for k in ("success", "done_steps", "done_opt"))
    for a in range(len(succ)):
        if succ[a]:
            k = min(int(opt[a]), DIST - 1)
            m[k] += (1.0, float(steps[a]), float(steps[a]) ** 2)
    return m


APPROX = [0, 14]  # reward, feature_diffs_mean: fp64 sums in another order than torch's
SHAPES = [(1, 4, 32, 1), (3, 4, 64, 3), (2, 6, 96, 5), (2, 20, 256, 20), (1, 128, 32, 64)]


@pytest.mark.parametrize("mode", ["pair", "first", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_fp64_restatement(shape, mode):
    """Rows (e0 + b, T - 1) of the active envs against the restatement; every other element keeps its sentinel.
    Sums and means rtol 1e-12 (fp64 summation error <= n 2^-53 ~ 5e-13 at 4096 addends); everything else exact.
    Two runs give the same bits."""
    _, L, _ = _mods()
    B, N, S, A = shape
    T, e0 = 3, 2
    t, E = T - 1, e0 + B
    d = _inputs(B, N, S, A, seed=B * 1000 + S, far_key=(shape == SHAPES[3]))
    rows, fd = _expected_rows(L, d, mode, S)
    for n_active in sorted({B, B - 1}):
        runs = []
        for _ in range(2):
            tb = _tables(E, T, S, A, B, e0, n_active)
            _launch(L, d, tb, mode, B, N, S, A, t, T, e0, n_active, E)
            runs.append(tb)
        for k in runs[0]:
            assert torch.equal(runs[0][k], runs[1][k]), f"{k}: two runs differ"
        tb = runs[0]
        exp = _tables(E, T, S, A, B, e0, n_active)
        exp["series"][e0:e0 + n_active, t] = rows[:n_active]
        exp["fd"][e0:e0 + n_active, t] = fd[:n_active]
        exp["da"][e0:e0 + n_active] = d["done"][:n_active]
        for b in range(n_active):
            exp["dm"][e0 + b] = torch.tensor(_expected_dmap(d, b), device="cuda")
        got, want = tb["series"].cpu().numpy(), exp["series"].cpu().numpy()
        exact = [i for i in range(16) if i not in APPROX]
        print(f"{shape} {mode} n_active={n_active}: max rel err of the sums",
              np.max(np.abs(got[..., APPROX] - want[..., APPROX]) / np.maximum(np.abs(want[..., APPROX]), 1e-300)))
        np.testing.assert_array_equal(got[..., exact], want[..., exact])
        np.testing.assert_allclose(got[..., APPROX], want[..., APPROX], rtol=1e-12, atol=0)
        np.testing.assert_allclose(tb["fd"].cpu().numpy(), exp["fd"].cpu().numpy(), rtol=1e-12, atol=0)
        assert torch.equal(tb["da"], exp["da"])
        assert torch.equal(tb["dm"], exp["dm"])
    if shape == SHAPES[3]:  # the key 40 >= DIST landed in the overflow slot, and the Python side refuses it
        _, _, EV = _mods()
        assert tb["dm"][e0, DIST - 1, 0] >= 1
        with pytest.raises(ValueError, match="shortest path"):
            EV.check_distance_map(tb["dm"][e0:e0 + 1].cpu().numpy())


def test_kernel_accumulates_over_steps_and_rejects_bad_sizes():
    """done_agents is the OR and distance_map the sum over an episode's steps; out-of-range sizes launch nothing."""
    _, L, _ = _mods()
    B, N, S, A, T, E = 2, 6, 96, 5, 2, 2
    tb = _tables(E, T, S, A, B, 0, B)
    d0, d1 = _inputs(B, N, S, A, 1), _inputs(B, N, S, A, 2)
    _launch(L, d0, tb, "first", B, N, S, A, 0, T, 0, B, E)
    _launch(L, d1, tb, "pair", B, N, S, A, 1, T, 0, B, E)
    assert torch.equal(tb["da"], d0["done"] | d1["done"])
    for b in range(B):
        np.testing.assert_array_equal(tb["dm"][b].cpu().numpy(), _expected_dmap(d0, b) + _expected_dmap(d1, b))
    assert not (tb["series"] == SENT).any() and not (tb["fd"] == SENT).any()
    before = {k: v.clone() for k, v in tb.items()}
    args = dict(B=B, N=N, S=S, A=A, t=0, T=T, e0=0, n_active=B, E=E)
    for bad in (dict(t=T), dict(e0=1), dict(n_active=B + 1), dict(A=65), dict(S=98), dict(N=129)):
        with pytest.raises(L.GMError):
            _launch(L, d0, tb, "pair", **{**args, **bad})
    for k in tb:
        assert torch.equal(tb[k], before[k])


# ---------------------------------------------------------------------------------------------------------
# evaluate against a recording of every step
# ---------------------------------------------------------------------------------------------------------
N_NODES, N_AGENTS, H = 20, 20, 32


def _snap(log, base, state, detail):
    log.append({"reward": base.reward.cpu().numpy().copy(), "done": base.done.cpu().numpy().copy(),
                "info": base.info.cpu().numpy().copy(), "eval": base.eval_stats.cpu().numpy().copy(),
                "state": None if state is None else state.cpu().numpy().copy(),
                **{k: v.cpu().numpy().copy() for k, v in (detail or {}).items()}})


def _make_env(kind, n_env, log):
    """kind: 'fused' / 'unfused' NetMonWrapper (a recording subclass), or 'plain': a Routing env behind a wrapper
    that offers only step()."""
    gm = importlib.import_module("graph-marl_amd")
    M = importlib.import_module("graph-marl_amd.model")
    W = importlib.import_module("graph-marl_amd.wrapper")
    net = gm.Network(N_NODES, random_topology=True, excluded_seeds=gm.EVAL_SEEDS)
    base = gm.Routing(net, N_AGENTS, n_env=n_env, seeds=list(range(5, 5 + n_env)),
                      obs_extra=0 if kind == "plain" else 4 * H)

    if kind == "plain":
        class StepOnly:
            def __init__(self, env):
                self._e = env

            def get(self):
                return self._e

            def reset(self):
                return self._e.reset()

            def set_eval_info(self, v):
                self._e.set_eval_info(v)

            def get_final_info(self, info):
                return self._e.get_final_info(info)

            def step(self, actions):
                out = self._e.step(actions)
                _snap(log, self._e, None, self._e.default_detail)
                return out

        return StepOnly(base)

    class Recording(W.NetMonWrapper):
        def step_(self, actions, detail=None, before_netmon=None):
            state = self.current_netmon_state.clone()  # the state the policy acted on
            if before_netmon is None:
                super().step_(actions, detail)
            else:
                super().step_(actions, detail, before_netmon=before_netmon)
            _snap(log, self.env, state, detail)

    torch.manual_seed(3)
    netmon = M.NetMon(4 * N_NODES + 8, H, [64, 48], 1).cuda()
    env = Recording(base, netmon, 1, fused=(kind == "fused"))
    assert env.fused == (kind == "fused")
    return env


@pytest.mark.parametrize("kind", ["fused", "unfused", "plain"])
def test_evaluate_series_match_a_recording(kind, tmp_path):
    """n_env = 2, 3 episodes x 6 steps: the second round has one active env (episode 2 = env 0 of round 1)."""
    gm, L, EV = _mods()
    HEU = importlib.import_module("graph-marl_amd.heuristics")
    n_env, episodes, T = 2, 3, 6
    log = []
    env = _make_env(kind, n_env, log)
    out = {}
    metrics = EV.evaluate(env, HEU.ShortestPath(env), episodes, T, output_dir=str(tmp_path), series=out,
                          output_node_state_aux=True)
    assert len(log) == 2 * T
    env2 = _make_env(kind, n_env, [])
    assert EV.evaluate(env2, HEU.ShortestPath(env2), episodes, T, series=False) == metrics
    assert json.load(open(tmp_path / "metrics.json")) == metrics
    S = 1 if kind == "plain" else 2 * H
    col = {k: i for i, k in enumerate(L.SERIES_KEYS)}
    ser = np.zeros((episodes, T, 16))
    fd = np.zeros((episodes, T, S))
    da = np.zeros((episodes, N_AGENTS), np.uint8)
    dm = {}
    states = np.zeros((episodes, T, N_NODES, S), np.float32)
    for r in range(2):
        for b in range(min(n_env, episodes - r * n_env)):
            e = r * n_env + b
            prev = None
            for t in range(T):
                s = log[r * T + t]
                row = ser[e, t]
                row[col["reward"]] = s["reward"][b].astype(np.float64).mean()
                for i, k in enumerate(L.INFO_KEYS):
                    if k in col:
                        row[col[k]] = s["info"][b, i]
                for i, k in enumerate(L.EVAL_KEYS):
                    row[col[k]] = s["eval"][b, i]
                ok = s["success"][b] != 0
                row[col["spr_min"]] = (s["done_steps"][b][ok] / s["done_opt"][b][ok]).min() if ok.any() else np.inf
                da[e] |= s["done"][b]
                for a in np.nonzero(ok)[0]:
                    v = float(s["done_steps"][b, a])
                    dm.setdefault((e, int(s["done_opt"][b, a])), []).append(v)
                if s["state"] is not None:
                    cur = s["state"][b].reshape(N_NODES, S)
                    states[e, t] = cur
                    diff = np.abs(cur - (0 if prev is None else prev)).astype(np.float32)
                    fd[e, t] = diff.astype(np.float64).mean(0)
                    row[col["feature_diffs_mean"]] = diff.astype(np.float64).mean()
                    row[col["feature_diffs_max"]] = diff.max()
                    prev = cur
    z = np.load(tmp_path / "series.npz")
    assert list(z["fields"]) == L.SERIES_KEYS and int(z["episodes"]) == episodes and int(z["steps"]) == T
    assert not bool(z["detailed"])
    exact = [i for i in range(16) if i not in APPROX]
    np.testing.assert_array_equal(z["series"][..., exact], ser[..., exact])
    np.testing.assert_allclose(z["series"][..., APPROX], ser[..., APPROX], rtol=1e-12, atol=0)
    np.testing.assert_allclose(z["feature_diffs"], fd, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(z["done_agents"], da)
    got_dm = z["distance_map"]
    exp_dm = np.zeros_like(got_dm)
    for (e, k), v in dm.items():
        exp_dm[e, k] = (len(v), sum(v), sum(x * x for x in v))
    np.testing.assert_array_equal(got_dm, exp_dm)
    assert ser[..., col["throughput"]].sum() > 0  # packets did arrive in this short run
    for k in ("series", "feature_diffs", "done_agents", "distance_map"):
        np.testing.assert_array_equal(out[k], z[k])
    nz = np.load(tmp_path / "node_state_aux.npz")
    assert nz["node_state"].shape == (episodes, T, N_NODES, S) and nz["node_aux"].shape == (episodes, T, N_NODES, N_NODES)
    if kind != "plain":
        np.testing.assert_array_equal(nz["node_state"], states)
        assert np.abs(z["feature_diffs"]).max() > 0


def test_node_state_table_too_large_is_refused(tmp_path):
    """A round whose node-state table cannot fit raises a ValueError that names the size, before any step."""
    _, _, EV = _mods()
    HEU = importlib.import_module("graph-marl_amd.heuristics")
    env = _make_env("fused", 2, [])
    steps = 2 ** 31  # 2 envs x 2^31 steps x 20 nodes x 84 floats: far beyond any device
    with pytest.raises(ValueError, match="bytes"):
        ser = EV.Series(env, 2, 4, node_state_aux=False)
        ser.T = steps
        ser.aux = True
        ser.begin_round(0)


# ---------------------------------------------------------------------------------------------------------
# CLI files
# ---------------------------------------------------------------------------------------------------------
def test_cli_eval_writes_the_files(tmp_path):
    main = importlib.import_module("graph-marl_amd.main")
    _, L, _ = _mods()
    out = tmp_path / "ev"
    main.main(["--env-type=routing", "--eval", "--policy=heuristic", "--netmon", "--eval-episodes=2",
               "--eval-episode-steps=5", "--netmon-dim=32", "--netmon-encoder-dim=64,48", "--netmon-iterations=1",
               "--eval-output-dir", str(out), "--eval-output-node-state-aux", "--eval-output-detailed",
               "--random-topology=1", "--disable-progressbar"])
    for f in ("metrics.json", "series.npz", "lzma_d.pk", "node_state_aux.npz"):
        assert (out / f).exists(), f
    nz = np.load(out / "node_state_aux.npz")
    assert nz["node_state"].shape == (2, 5, 20, 64) and nz["node_aux"].shape == (2, 5, 20, 20)
    assert bool(np.load(out / "series.npz")["detailed"])
    # the pickle loads with the standard library and numpy alone, in a process that never saw the GPU or the project
    code = (
        "import sys, lzma, pickle, collections, numpy as np\n"
        "d = pickle.load(lzma.open(sys.argv[1], 'rb'))\n"
        "keys = ['feature_diffs_mean', 'feature_diffs_max', 'throughput', 'delays_arrived_mean', 'looped', 'reward',"
        " 'dropped', 'episode_done_agents']\n"
        "assert list(d) == keys, list(d)\n"
        "for k in keys[:-1]:\n"
        "    v = d[k]\n"
        "    assert type(v) is collections.defaultdict and v.default_factory is list, k\n"
        "    assert all(type(x) is float for l in v.values() for x in l), k\n"
        "    if k != 'delays_arrived_mean':\n"
        "        assert sorted(v) == list(range(5)) and all(len(l) == 2 for l in v.values()), k\n"
        "a = d['episode_done_agents']\n"
        "assert a.dtype == np.float64 and a.shape == (2, 20)\n"
        "assert 'torch' not in sys.modules and not any('graph-marl' in m for m in sys.modules)\n"
        "print('ok')\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", code, str(out / "lzma_d.pk")], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


# ---------------------------------------------------------------------------------------------------------
# the reference's files (tests/golden/make_golden_eval_series.py)
# ---------------------------------------------------------------------------------------------------------
STATE_TOL = 1e-5  # carried lstm states against the reference: test_netmon_gpu.ATOL, test_long_horizon_gpu.TOL


def test_files_match_the_reference(tmp_path):
    """n_env = 1 (the reference's one env draws from one numpy stream over consecutive episodes), set up like
    `main.py --eval --policy=heuristic --netmon`. The heuristic's trajectory does not depend on NetMon, so the
    env-derived series are exact; reward and delays_arrived_mean rtol 1e-6 (test_cli_eval.py); node_state within the
    bound for carried lstm states, the two drift series within twice that bound (a difference of two states).
    Largest deviations seen on MI355X: node_state 1.5e-7, feature_diffs_mean 4.3e-9, feature_diffs_max 1.2e-7."""
    import lzma
    import pickle

    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import detparams

    gm, L, EV = _mods()
    M = importlib.import_module("graph-marl_amd.model")
    W = importlib.import_module("graph-marl_amd.wrapper")
    HEU = importlib.import_module("graph-marl_amd.heuristics")
    g = np.load(os.path.join(GOLDEN, "eval_series.npz"))
    seed, det_seed, E, T, N, A, Hd, e0, e1 = (int(v) for v in g["cfg"])
    net = gm.Network(n_nodes=N, random_topology=True, n_random_seeds=0, topology_init_seed=476,
                     excluded_seeds=gm.EVAL_SEEDS)
    base = gm.Routing(net, A, n_env=1, seeds=[seed], obs_extra=4 * Hd)
    base.reset()
    netmon = M.NetMon(base.node_obs_dim, Hd, [e0, e1], 1).cuda()
    sd = netmon.state_dict()
    vals = detparams.det_state_dict(det_seed, {"netmon." + k: v.shape for k, v in sd.items()})
    netmon.load_state_dict({k: torch.tensor(vals["netmon." + k]) for k in sd})
    env = W.NetMonWrapper(base, netmon, 1)
    env.reset()
    base.set_topology_seeds(gm.EVAL_SEEDS, sequential=True, interleave=False)
    metrics = EV.evaluate(env, HEU.ShortestPath(env), E, T, output_dir=str(tmp_path), output_node_state_aux=True)
    for k, v in zip(g["metric_keys"], g["metric_values"]):
        np.testing.assert_allclose(metrics[str(k)], v, rtol=1e-6, err_msg=str(k))
    p = pickle.load(lzma.open(tmp_path / "lzma_d.pk", "rb"))

    def table(k):
        assert sorted(p[k]) == list(range(T))
        return np.array([p[k][t] for t in range(T)])

    for k in ("throughput", "looped", "dropped"):
        np.testing.assert_array_equal(table(k), g[k], err_msg=k)
    np.testing.assert_array_equal(p["episode_done_agents"], g["episode_done_agents"])
    assert [len(p["delays_arrived_mean"].get(t, [])) for t in range(T)] == list(g["delays_arrived_mean_count"])
    got = [x for t in range(T) for x in p["delays_arrived_mean"].get(t, [])]
    np.testing.assert_allclose(got, g["delays_arrived_mean_values"], rtol=1e-6)
    np.testing.assert_allclose(table("reward"), g["reward"], rtol=1e-6)
    nz = np.load(tmp_path / "node_state_aux.npz")
    assert nz["node_state"].shape == g["node_state"].shape == (E, T, N, 2 * Hd)
    dev = {"node_state": np.abs(nz["node_state"] - g["node_state"]).max()}
    for k in ("feature_diffs_mean", "feature_diffs_max"):
        dev[k] = np.abs(table(k) - g[k]).max()
    print("largest deviations from the reference:", dev)
    np.testing.assert_array_equal(nz["node_aux"], g["node_aux"])
    assert dev["node_state"] <= STATE_TOL
    assert dev["feature_diffs_mean"] <= 2 * STATE_TOL and dev["feature_diffs_max"] <= 2 * STATE_TOL
    assert g["feature_diffs_max"].min() > 100 * STATE_TOL  # the drift is far above the bound: the check has teeth
