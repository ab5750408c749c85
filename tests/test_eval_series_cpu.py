"""Host side of the evaluation series (graph-marl_amd/evaluate.py): the lzma_d.pk layout built from synthetic
tables, the distance-map overflow check, and the C-ABI declaration of gm_eval_series_step. No GPU."""
import collections
import importlib
import lzma
import os
import pickle
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables(L, E=3, T=4, A=5, D=8):
    rng = np.random.RandomState(0)
    col = {k: i for i, k in enumerate(L.SERIES_KEYS)}
    series = rng.rand(E, T, len(L.SERIES_KEYS))
    series[..., col["n_arrived"]] = rng.randint(0, 3, size=(E, T))
    series[1, :, col["n_arrived"]] = 0  # episode 1 never sees an arrival
    series[0, 2, col["n_arrived"]] = 2
    series[..., col["sum_delays_arrived"]] = series[..., col["n_arrived"]] * rng.randint(1, 9, size=(E, T))
    done_agents = (rng.rand(E, A) < 0.5).astype(np.uint8)
    dm = np.zeros((E, D, 3))
    dm[:, 2] = (1.0, 3.0, 9.0)
    return {"series": series, "feature_diffs": rng.rand(E, T, 2), "done_agents": done_agents, "distance_map": dm}, col


def test_pickle_layout_matches_the_reference(gm, tmp_path):
    EV = importlib.import_module("graph-marl_amd.evaluate")
    L = gm._lib
    tb, col = _tables(L)
    E, T = tb["series"].shape[:2]
    EV.write_series(str(tmp_path), tb, detailed=True)
    d = pickle.load(lzma.open(tmp_path / "lzma_d.pk", "rb"))
    assert list(d) == ["feature_diffs_mean", "feature_diffs_max", "throughput", "delays_arrived_mean", "looped",
                       "reward", "dropped", "episode_done_agents"]
    for k in list(d)[:-1]:
        assert type(d[k]) is collections.defaultdict and d[k].default_factory is list
        assert all(type(x) is float for v in d[k].values() for x in v)
    for k in ("feature_diffs_mean", "feature_diffs_max", "throughput", "looped", "reward", "dropped"):
        assert sorted(d[k]) == list(range(T))
        for t in range(T):  # one value per episode, in episode order
            assert d[k][t] == [float(tb["series"][e, t, col[k]]) for e in range(E)]
    n, s = tb["series"][..., col["n_arrived"]], tb["series"][..., col["sum_delays_arrived"]]
    for t in range(T):  # ragged: only the episodes with an arrival at step t, still in episode order
        exp = [float(s[e, t] / n[e, t]) for e in range(E) if n[e, t] > 0]
        assert d["delays_arrived_mean"].get(t, []) == exp
        assert len(exp) < E  # episode 1 is always missing
    assert len(d["delays_arrived_mean"][2]) >= 1
    a = d["episode_done_agents"]
    assert a.dtype == np.float64 and np.array_equal(a, tb["done_agents"])
    z = np.load(tmp_path / "series.npz")
    assert list(z["fields"]) == L.SERIES_KEYS and int(z["episodes"]) == E and int(z["steps"]) == T and bool(z["detailed"])
    for k, v in tb.items():
        assert np.array_equal(z[k], v)
    assert not (tmp_path / "node_state_aux.npz").exists()


def test_distance_map_overflow_raises(gm, tmp_path):
    EV = importlib.import_module("graph-marl_amd.evaluate")
    tb, _ = _tables(gm._lib)
    EV.check_distance_map(tb["distance_map"])
    tb["distance_map"][1, -1] = (1.0, 9.0, 81.0)
    with pytest.raises(ValueError, match="shortest path"):
        EV.check_distance_map(tb["distance_map"])
    with pytest.raises(ValueError):
        EV.write_series(str(tmp_path), tb)
    assert not (tmp_path / "lzma_d.pk").exists()


def test_symbol_is_declared_bound_and_exported(gm):
    L = gm._lib
    hdr = open(os.path.join(ROOT, "include", "graph_marl_amd.h")).read()
    assert re.search(r"\bint gm_eval_series_step\s*\(", hdr)
    assert "gm_eval_series_step" in L.EXPORTS
    m = re.search(r"GM_SERIES_REWARD = 0,(.*?)GM_SERIES_FIELDS", hdr, re.S)
    names = ["reward"] + [n.lower() for n in re.findall(r"GM_SERIES_([A-Z_]+)", re.sub(r"/\*.*?\*/", "", m.group(1)))]
    assert names == L.SERIES_KEYS and len(names) == L.GM_SERIES_FIELDS
    lib = L.lib()
    assert lib.gm_eval_series_step.argtypes is not None and len(lib.gm_eval_series_step.argtypes) == 24
    # argument checks come before any device call
    null = [None, None, 0, 0, 0, None, None, 0, None, None, None, None, None, 0, 0, 0, 0, 0, None, None, None, None,
            0, None]
    assert lib.gm_eval_series_step(*null) == -1 and b"gm_eval_series_step" in lib.gm_last_error()


def test_evaluate_signature(gm):
    import inspect

    EV = importlib.import_module("graph-marl_amd.evaluate")
    p = inspect.signature(EV.evaluate).parameters
    assert list(p) == ["env", "policy", "episodes", "steps_per_episode", "disable_progressbar", "output_dir",
                       "output_detailed", "output_node_state_aux", "series"]
    for k in ("output_detailed", "output_node_state_aux", "series"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["series"].default is None and p["output_detailed"].default is False
