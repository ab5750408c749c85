"""CPU side of the edge-weight change and the NetMon freeze: the legacy np.random.shuffle draws the kernel restates,
the evaluation flags, and the wrapper's flag logic (no kernel runs here)."""
import importlib
import types

import numpy as np
import pytest
import torch


def _raw(rs):
    """One 32-bit word of the legacy stream (a full-range draw takes exactly one)."""
    return int(rs.randint(0, 2**32, dtype=np.uint64))


def _masked_draw(rs, top):
    """random_interval of numpy's legacy stream: a value in [0, top] by masked rejection on 32-bit draws; -> (value,
    number of 32-bit words drawn). top = 0 draws nothing."""
    if top == 0:
        return 0, 0
    mask = top
    for s in (1, 2, 4, 8, 16):
        mask |= mask >> s
    n = 0
    while True:
        v = _raw(rs) & mask
        n += 1
        if v <= top:
            return v, n


def _shuffle(rs, x):
    """np.random.shuffle of a 1-d array, restated: from the top index down, swap with a partner in [0, i]."""
    words = 0
    for i in range(len(x) - 1, 0, -1):
        j, n = _masked_draw(rs, i)
        words += n
        x[i], x[j] = x[j], x[i]
    return words


@pytest.mark.parametrize("n", [1, 2, 9, 30, 192])
@pytest.mark.parametrize("seed", [0, 7, 476])
def test_legacy_shuffle_restated(n, seed):
    """Lengths 1, 2, 9 (= 3N/2 at N = 6), 30 (N = 20) and 192 (N = 128): the same permutation as np.random.shuffle
    and the same number of 32-bit words consumed (the stream position the kernel must leave behind)."""
    a, b = np.random.RandomState(seed), np.random.RandomState(seed)
    x = np.arange(100, 100 + n)
    y = x.copy()
    a.shuffle(x)
    words = _shuffle(b, y)
    np.testing.assert_array_equal(x, y)
    assert words >= n - 1
    # both streams stand at the same word: the next raw draws agree, and a third stream that skips `words` words too
    c = np.random.RandomState(seed)
    for _ in range(words):
        _raw(c)
    nxt = [_raw(a) for _ in range(4)]
    assert nxt == [_raw(b) for _ in range(4)] == [_raw(c) for _ in range(4)]


def test_legacy_randint_restated():
    """np.random.randint(low, high) = low + the masked-rejection draw on high - 1 - low (reset_packet's draw)."""
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    for low, high in [(1, 6), (1, 2), (3, 256), (1, 6), (2, 9)] * 20:
        assert a.randint(low, high) == low + _masked_draw(b, high - 1 - low)[0]
    assert _raw(a) == _raw(b)


def test_edge_change_flags():
    main = importlib.import_module("graph-marl_amd.main")
    p = main.build_parser()
    args = p.parse_args([])
    assert args.eval_edge_change is None and args.eval_netmon_freeze is None
    assert main.eval_events(args, object()) is None
    cases = {"50:shuffle": (50, "shuffle", {}),
             "50:randint:1:6": (50, "randint", {"low": 1, "high": 6}),
             "50:set:2:7:10": (50, "set", {"edge": (2, 7), "length": 10}),
             "0:bottleneck-971182936": (0, "bottleneck-971182936", {})}
    for text, want in cases.items():
        assert p.parse_args(["--eval-edge-change", text]).eval_edge_change == want
    assert p.parse_args(["--eval-netmon-freeze", "25"]).eval_netmon_freeze == 25
    bad = ["shuffle", "50", "x:shuffle", "-1:shuffle", "50:nonsense", "50:shuffle:1", "50:randint", "50:randint:1",
           "50:randint:6:1", "50:randint:0:6", "50:randint:a:b", "50:set:2:7", "50:set:2:2:10", "50:set:2:7:0",
           "50:set:2:7:300", ""]
    for text in bad:
        with pytest.raises(SystemExit):
            p.parse_args(["--eval-edge-change", text])
    for text in ["x", "-3", "2.5"]:
        with pytest.raises(SystemExit):
            p.parse_args(["--eval-netmon-freeze", text])
    # the flags sit in the group of the flags the reference does not have, beside --n-env
    opts = [a.option_strings[0] for a in p._actions if a.option_strings]
    assert opts.index("--eval-edge-change") > opts.index("--n-env") < opts.index("--eval-netmon-freeze")


def test_evaluate_events_signature():
    """evaluate keeps its parameter list; evaluate_events is the same list with `events` after the four positional
    arguments, and evaluate hands everything on to it."""
    import inspect

    EV = importlib.import_module("graph-marl_amd.evaluate")
    p, q = inspect.signature(EV.evaluate).parameters, inspect.signature(EV.evaluate_events).parameters
    assert "events" not in p
    assert list(q) == list(p)[:4] + ["events"] + list(p)[4:] and q["events"].default is None
    for k in p:
        assert q[k].kind is p[k].kind and q[k].default == p[k].default


def test_edge_change_args_and_unknown_mode():
    R = importlib.import_module("graph-marl_amd.routing")
    L = importlib.import_module("graph-marl_amd._lib")
    assert R.edge_change_args("shuffle")[0] == L.EDGE_SHUFFLE
    assert R.edge_change_args("randint", low=1, high=6) == (L.EDGE_RANDINT, 1, 6, 0, 0, 0)
    assert R.edge_change_args("bottleneck-971182936") == (L.EDGE_SET, 0, 0, 2, 7, 10)
    assert R.edge_change_args("set", edge=(7, 2), length=4) == (L.EDGE_SET, 0, 0, 2, 7, 4)
    with pytest.raises(ValueError, match="Unknown mode"):
        R.edge_change_args("swap")
    net = R.Network(6)
    with pytest.raises(RuntimeError):
        net.randomize_edge_weights("shuffle")  # no Routing owns it


def test_freeze_flag_logic(monkeypatch):
    """freeze / frozen / reset on a wrapper around stand-ins: a frozen step launches nothing and leaves the state
    objects alone; reset clears the flag and steps NetMon again."""
    W = importlib.import_module("graph-marl_amd.wrapper")
    calls = []
    env = types.SimpleNamespace(nbr=torch.zeros(2, 6, 3, dtype=torch.int32), obs_dim=46, obs_stride=46 + 128, n_env=2,
                                n_nodes=6, n_data=5, device=torch.device("cpu"), node_obs=None,
                                reset_=lambda: calls.append("reset"),
                                step_=lambda a, d=None: calls.append("step"))
    netmon = types.SimpleNamespace(hidden_features=32, output_neighbor_hidden=True, output_global_hidden=False,
                                   get_state_size=lambda: 64)
    monkeypatch.setattr(W.FU, "netmon_step", lambda nm, x, nbr, st, out=None, last_out=None: (
        calls.append("netmon") or out, last_out))
    w = W.NetMonWrapper(env, netmon, 1, fused=True)
    assert w.frozen is False
    w.reset_()
    assert calls == ["reset", "netmon"] and not w.frozen
    cur, last, hp, parity = w.current_netmon_state, w.last_netmon_state, w.h_prev, w._cur
    w.step_(None)
    assert calls[-2:] == ["step", "netmon"] and w._cur != parity
    cur, last, hp, parity = w.current_netmon_state, w.last_netmon_state, w.h_prev, w._cur
    w.freeze()
    assert w.frozen is True
    w._dirty = False
    for k in range(3):
        w.step_(None)
        assert calls[-1] == "step" and w.frozen_steps == k + 1 and w._dirty
        assert w.current_netmon_state is cur and w.last_netmon_state is last and w.h_prev is hp and w._cur == parity
    w.reset_()
    assert w.frozen is False and w.frozen_steps == 0 and calls[-2:] == ["reset", "netmon"]
