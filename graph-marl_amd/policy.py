"""ε-greedy action selection on the device (reference src/policy.py:7-87 EpsilonGreedy).

Q-values come from the agent model (DQN, DGN, DQNR, CommNet) on the HIP kernels; the random draws
(randint(n_actions, size=A) then rand(A), every call, from each env's numpy-legacy
stream) and the argmax/mix run in the env's egreedy kernel (gm_policy_egreedy /
gm_simple_policy_egreedy).
"""

import torch

# ε-greedy runs as the env step kernel's prologue (gm_env_policy_step); tests compare it with the two launches
FUSED_POLICY_STEP = True
# DGN / DQNR / CommNet take the fused road on a fused NetMonWrapper (forward_fused: no joint observation); False:
# they read `.obs` like the env-only rollout (tests and tools compare the two roads in one process)
FUSED_AGENTS = True


class EpsilonGreedy:
    def __init__(self, env, model, action_space=4, args=None, epsilon=None, epsilon_decay=None,
                 epsilon_update_freq=None, step_before_train=None):
        self._env = env.get() if hasattr(env, "get") else env
        self._model = model
        self._action_space = action_space
        self._epsilon = epsilon if epsilon is not None else getattr(args, "epsilon", 0.6)
        self._decay = epsilon_decay if epsilon_decay is not None else getattr(args, "epsilon_decay", 0.996)
        self._freq = epsilon_update_freq if epsilon_update_freq is not None else getattr(args, "epsilon_update_freq",
                                                                                          100)
        self._before = step_before_train if step_before_train is not None else getattr(args, "step_before_train",
                                                                                        2000)
        self._step = 0
        self._eps_tmp = None
        e = self._env
        self.actions = torch.zeros(e.n_env, e.n_data, dtype=torch.int32, device=e.device)
        self._scratch = {}
        self._state_bufs = None  # recurrent models on the fused road: two fixed state buffers (state_buffer)

    def _buf(self, i, m, n):
        key = (i, m, n)
        b = self._scratch.get(key)
        if b is None:
            b = torch.empty(m, n, device=self._env.device)
            self._scratch[key] = b
        return b

    def q_values(self, obs, adj=None):
        """q [n_env, A, 4] for a joint observation view [n_env, A, D] (strided rows ok); adj:
        agent adjacency [n_env, A, A] for DGN / CommNet (default: the env's)."""
        e = self._env
        with torch.no_grad():
            x2 = obs.reshape(-1, obs.shape[-1])
            if adj is None:
                adj = getattr(e, "agent_adj", None)
            if adj is not None and adj.dtype != torch.int8:
                adj = (adj != 0).to(torch.int8)
            # rows are spaced by the agent-dim stride (reshape may renormalise size-1 dims)
            q = self._model.forward_rows(x2, obs.stride(-2), obs.shape[-1], self._buf, adj=adj, B=e.n_env,
                                         A=e.n_data)
        return q.view(e.n_env, e.n_data, -1)

    def select(self, q):
        """ε-greedy mix of argmax(q) and uniform actions, drawn from each env's stream."""
        return self._env.egreedy(q.contiguous(), self._epsilon, self.actions)

    def _decay_step(self):
        self._step += 1
        if self._epsilon > 0 and self._step > self._before and self._step % self._freq == 0:
            self._epsilon = max(self._epsilon * self._decay, 0.01)

    def __call__(self, obs, adj=None):
        actions = self.select(self.q_values(obs, adj))
        self._decay_step()
        return actions

    def fused_tables(self, wenv):
        """(args, kwargs) of fused.agent_first_layer / fused.dqn_q after the layer or model: a fused NetMonWrapper's
        env rows and NetMon state tables. With the global readout the dense source is the obs buffer's [env obs |
        global mean] columns (NetMonWrapper.global_src)."""
        e = wenv.env
        H = wenv.netmon.hidden_features
        if getattr(wenv, "global_cols", False):
            return ((wenv.global_src(), e.obs_dim, wenv.current_netmon_state, wenv.h_prev, e.nbr, e.agent_node),
                    dict(hidden=H, global_cols=True))
        return ((e.obs_buf, e.obs_dim, wenv.current_netmon_state, wenv.h_prev, e.nbr, e.agent_node),
                dict(hidden=H, obs_gemm=e.obs_gemm))

    def fused_fits(self, wenv):
        """The model has a fused entry for this wrapper: a DQN, or (FUSED_AGENTS) a DGN / DQNR / CommNet with at
        most 64 agents (gm_agent_attention / gm_agent_comm) whose first layer reads the wrapper's joint observation
        (fused.first_layer_ok); DGN and CommNet also need the env's agent adjacency."""
        from . import fused as FU
        from .model import DQN, DQNR

        if not getattr(wenv, "fused", False):
            return False
        m = self._model
        if isinstance(m, DQN):
            return True
        if not (FUSED_AGENTS and hasattr(m, "forward_fused")):
            return False
        e = wenv.env
        needs_adj = not isinstance(m, DQNR) or hasattr(m, "comm_rounds")
        return (e.n_data <= 64 and (not needs_adj or getattr(e, "agent_adjacency", False))
                and FU.first_layer_ok(m.encoder.linear_layers[0], e.obs_dim, e.n_nodes, e.nbr.shape[-1],
                                      wenv.netmon.hidden_features, getattr(wenv, "global_cols", False)))

    def state_buffer(self, wenv, i=None):
        """One of this policy's two fixed agent-state buffers [n_env * A, 2H] (recurrent models). The fused forward
        writes buffer 1 - wenv._cur, so the pair alternates in step with the wrapper's NetMon pair and a captured
        graph reads and writes the same addresses on every replay; i = None: that output buffer, unless the model's
        current state lives in it (then the other one)."""
        e, m = wenv.env, self._model
        if self._state_bufs is None:
            self._state_bufs = [torch.zeros(e.n_env * e.n_data, m.get_state_len(), device=e.device) for _ in range(2)]
        if i is not None:
            return self._state_bufs[i]
        i = 1 - getattr(wenv, "_cur", 0)
        st = m.state
        if st is not None and st.data_ptr() == self._state_bufs[i].data_ptr():
            i = 1 - i
        return self._state_bufs[i]

    def _fused_q(self, wenv):
        """Q rows of the model on a fused NetMonWrapper's state tables: fused.dqn_q for the DQN, forward_fused for
        DGN / DQNR / CommNet (adjacency from the env, the recurrent state into this policy's buffer pair). No joint
        observation row is read or written."""
        from . import fused as FU
        from .model import DQN

        args, kw = self.fused_tables(wenv)
        m = self._model
        if isinstance(m, DQN):
            return FU.dqn_q(m, *args, self._buf, **kw)
        e = wenv.env
        extra = {"state_out": self.state_buffer(wenv)} if hasattr(m, "state") else {}
        with torch.no_grad():
            return m.forward_fused((args, kw), self._buf, e.n_env, e.n_data,
                                   adj=e.agent_adj if getattr(e, "agent_adjacency", False) else None, **extra)

    def act(self, wenv):
        """Fast path for a fused NetMonWrapper: the model's first GEMM gathers the NetMon
        readout from the node state tables instead of reading a materialised joint obs."""
        if not self.fused_fits(wenv):
            return self(wenv.obs)
        e = wenv.env
        q = self._fused_q(wenv)
        actions = self.select(q.view(e.n_env, e.n_data, -1))
        self._decay_step()
        return actions

    def act_step(self, wenv, detail=None):
        """act(wenv) then wenv.step_(actions). On the fused NetMon path the ε-greedy draws run
        as the env step kernel's prologue (gm_env_policy_step: one launch instead of two, the
        same draws and actions)."""
        if not (FUSED_POLICY_STEP and self.fused_fits(wenv)):
            actions = self.act(wenv)
            if detail is None:
                wenv.step_(actions)
            else:
                wenv.step_(actions, detail)
            return actions
        e = wenv.env
        q = self._fused_q(wenv)
        wenv.policy_step_(q.view(e.n_env, e.n_data, -1).contiguous(), self._epsilon, self.actions, detail)
        self._decay_step()
        return self.actions

    def _eps_changes(self):
        """True when ε still decays (its value is a kernel argument)."""
        return self._epsilon > 0.01 and self._decay != 1.0

    def reset(self, agents_to_reset):
        """src/policy.py:72-82: zero the recurrent agent state of the given agents
        ([n_env, A] bool, or True for all)."""
        st = getattr(self._model, "state", None)
        if st is not None:
            m = torch.as_tensor(agents_to_reset, device=st.device).bool()
            self._model.state = st * ~(m.unsqueeze(-1) if m.dim() else m)

    def eval(self):
        self._eps_tmp = self._epsilon
        self._epsilon = 0

    def train(self):
        if self._eps_tmp is not None:
            self._epsilon = self._eps_tmp
            self._eps_tmp = None
