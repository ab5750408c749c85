"""NetMon graph observations for the batched routing env (reference
src/env/wrapper.py:7-109 NetMonWrapper).

After every env step one NetMon step runs on the device over all n_env graphs.
Fused mode (lstm / lnlstm / gru NetMon with carry-over, default): the step is three encoder
GEMMs plus the RNN cells on the HIP kernels (fused.netmon_step: lstm / gru one gate-tile GEMM
with the gate math in its epilogue, lnlstm two GEMMs + the LayerNorm-LSTM pointwise kernel); the graph part of the joint
observation is NOT materialised — the DQN gathers it inside its first GEMM
(policy.EpsilonGreedy.act). Reading `.obs` (the reference API) materialises the joint
observation [env obs | readout] on demand. A stateless NetMon (rnn_type "none") takes the same
road: its step is the encoder plus one gm_mp_iterate that writes h_K and h_{K-1} into the current
buffer pair. Unfused mode runs NetMon.forward_graph and writes the readout into the joint
observation buffer after every step.

Global readout (NetMon output_global_hidden, --netmon-global), fused mode: the joint observation is
[env obs | h | global | nbr x 3] with global = the mean of h over the graph's nodes. After every NetMon step
gm_netmon_global_rows writes that mean into the H columns that directly follow the env observation in the obs
buffer (the columns where a materialised observation holds h), so the DQN's first GEMM reads its dense source
[env obs | global] from the buffer's rows and gathers [h | nbr x 3] from the state tables. The GEMM-ready env copy
has no spare columns, so it is not enabled. Reading `.obs` overwrites the scratch columns with the reference
layout; the next fused Q pass (global_src) writes the mean back first. Both directions are tracked (`_dirty`,
`_gstale`), so `.obs` reads and policy.act calls may alternate freely between env steps.
"""
import torch

from . import _lib as L
from . import fused as FU
from .model import NetMon, netmon_readout


class NetMonWrapper:
    def __init__(self, env, netmon: NetMon, startup_iterations=1, fused=None):
        assert startup_iterations >= 1, "Number of startup iterations must be >= 1"
        # the readout is [h, h_prev of deg neighbours] with deg = the graph's max degree
        # (src/model.py:582-589), so the graph part is (deg + 1) H wide (4H on routing graphs)
        H = netmon.hidden_features
        self.graph_features = H * (1 + (env.nbr.shape[-1] if netmon.output_neighbor_hidden else 0) +
                                   (1 if netmon.output_global_hidden else 0))
        need = env.obs_dim + self.graph_features
        if env.obs_stride < need:
            raise ValueError(f"env obs buffer too narrow: create the env with obs_extra={self.graph_features}")
        self.frozen = False
        self._tables = []  # unfused road: [h, neighbour h] of this wrapper's last NetMon step
        self.frozen_steps = 0  # NetMon steps skipped since freeze() (evaluate: the state drift is 0 from the first)
        self.env = env
        self.netmon = netmon
        self.startup_iterations = startup_iterations
        self.last_netmon_state = None
        self.current_netmon_state = None
        self.h_prev = None
        self.obs_dim = need
        if fused is None:
            fused = FU.fused_ok(netmon)
        self.fused = fused
        # fused global readout: the obs buffer's first H graph columns are the DQN's scratch for the mean
        self.global_cols = bool(fused and netmon.output_global_hidden)
        if fused and hasattr(env, "enable_gemm_obs") and not self.global_cols:
            env.enable_gemm_obs()  # the fused DQN reads the GEMM-ready env obs copy
        self._dirty = False
        self._gstale = False  # global_cols: the scratch columns do not hold the current state's mean
        # fused mode: the state and h_prev alternate between two fixed buffer pairs, so a
        # captured 2-step HIP graph (rollout.StreamedRollout.capture) reads and writes the
        # same addresses on every replay
        self._bufs = None
        self._cur = 0
        self._rd = None  # global_cols: the 4H readout rows of _materialize

    def __getattr__(self, name):
        return getattr(self.env, name)

    def __str__(self):
        return str(self.env) + "\n▲ environment is wrapped with NetMon (graph obs)"

    @property
    def obs(self):
        """joint observation [n_env, A, obs_dim + (deg+1)H] (reference: concat of obs and graph obs)."""
        if self._dirty:
            self._materialize()
        if hasattr(self.env, "sync_obs"):
            self.env.sync_obs()  # env columns rebuilt when the env wrote only its GEMM-ready copy
        return self.env.obs_buf[..., : self.obs_dim]

    def _materialize(self):
        e, H = self.env, self.netmon.hidden_features
        B, N = e.n_env, e.n_nodes
        if self.global_cols:  # [h | global | nbr x 3]: the 4H readout rows, then h and the mean into their columns
            A, deg = e.n_data, e.nbr.shape[-1]
            st = self.current_netmon_state
            ob = e.obs_buf.data_ptr() + 4 * e.obs_dim
            if self._rd is None:
                self._rd = torch.empty(B * A, (deg + 1) * H, device=e.device)
            with torch.no_grad():
                L.check(L.lib().gm_netmon_readout_ld(st.data_ptr(), st.shape[-1], self.h_prev.data_ptr(),
                                                     self.h_prev.stride(0), e.nbr.data_ptr(), e.agent_node.data_ptr(),
                                                     B, N, A, deg, H, self._rd.data_ptr(), self._rd.stride(0),
                                                     L.stream_ptr()))
                g = e.obs_buf.view(B * A, -1)[:, e.obs_dim:e.obs_dim + (deg + 2) * H]
                g[:, :H] = self._rd[:, :H]
                g[:, 2 * H:] = self._rd[:, H:]
                FU.global_rows(st.data_ptr(), st.shape[-1], B, N, H, A, ob + 4 * H, e.obs_stride)
            self._dirty = False
            self._gstale = True
            return
        hf = self.current_netmon_state.reshape(B * N, -1)[:, :H].contiguous()
        hp = self.h_prev[:, :H].contiguous()
        with torch.no_grad():
            netmon_readout(hf, hp, e.nbr, e.agent_node, out=e.obs_buf, col0=e.obs_dim)
        self._dirty = False

    def global_src(self):
        """The obs buffer for fused.dqn_q(global_cols=True): its rows hold [env obs | global mean] for the current
        NetMon state (rewritten here when a `.obs` read has put the reference layout over it)."""
        if self._gstale:
            self._write_global()
        return self.env.obs_buf

    def _write_global(self):
        e, H = self.env, self.netmon.hidden_features
        st = self.current_netmon_state
        FU.global_rows(st.data_ptr(), st.shape[-1], e.n_env, e.n_nodes, H, e.n_data,
                       e.obs_buf.data_ptr() + 4 * e.obs_dim, e.obs_stride)
        self._gstale = False
        self._dirty = True  # the scratch sits where the materialised observation holds h

    def freeze(self):
        """Disable message passing for the rest of this episode (src/env/wrapper.py:53-58): no NetMon launch,
        the state and h_prev tables stay as they are, and agents read them at their current nodes. reset()
        clears it."""
        self.frozen = True

    def _frozen_step(self):
        """src/env/wrapper.py:67-75: only the agent mapping moves. Fused road: the DQN's first GEMM gathers from
        the state tables through agent_node, which the env step refreshed (and `.obs` re-gathers on a read), so
        nothing is launched. Unfused road: the agent rows are gathered again from the last readout's tables."""
        e = self.env
        self.frozen_steps += 1
        if self.fused:
            self._dirty = True
            return
        with torch.no_grad():
            self.netmon.readout_tables(self._tables, e.nbr, e.agent_node, out=e.obs_buf, out_col=e.obs_dim)

    def _netmon_step(self):
        e = self.env
        if self.frozen:
            return self._frozen_step()
        with torch.no_grad():
            self.last_netmon_state = self.current_netmon_state
            if self.fused:
                B, N, H2 = e.n_env, e.n_nodes, self.netmon.get_state_size()
                if self._bufs is None:
                    self._bufs = [(torch.empty(B, N, H2, device=e.device), torch.empty(B * N, H2, device=e.device))
                                  for _ in range(2)]
                nxt = 1 - self._cur
                st, hp = self._bufs[nxt]
                state, self.h_prev = FU.netmon_step(self.netmon, e.node_obs, e.nbr, self.current_netmon_state,
                                                    out=st, last_out=hp)
                self._cur = nxt
                self.current_netmon_state = state
                if self.global_cols:
                    self._write_global()
                self._dirty = True
            else:
                self.netmon.state = self.current_netmon_state
                self.netmon.forward_graph(e.node_obs, e.nbr, e.agent_node, out=e.obs_buf, out_col=e.obs_dim,
                                          tables=self._tables)  # kept for a frozen step's readout
                self.current_netmon_state = self.netmon.state

    def reset_(self):
        """reset() without materialising the joint observation (the rollout driver's form)."""
        self.frozen = False
        self.frozen_steps = 0
        self.current_netmon_state = None
        self.last_netmon_state = None
        self._cur = 1  # the start-up step writes buffer pair 0
        self.env.reset_()
        for _ in range(self.startup_iterations):
            self._netmon_step()

    def reset(self):
        self.reset_()
        return self.obs, self.env.agent_adj

    def step(self, actions):
        _, adj, reward, done, info = self.env.step(actions)
        self._netmon_step()
        return self.obs, adj, reward, done, info

    def step_(self, actions, detail=None, before_netmon=None):
        """before_netmon (optional callable): runs between the env step and the NetMon step, while
        current_netmon_state / last_netmon_state still are the states the policy acted on at this step and at
        the one before (fused mode: the two buffer pairs; the NetMon step then overwrites the older one).
        evaluate's series kernel reads the pair there, in place."""
        self.env.step_(actions, detail)
        if before_netmon is not None:
            before_netmon()
        self._netmon_step()

    def policy_step_(self, q, epsilon, actions, detail=None):
        """ε-greedy on q + env step in one launch (Routing.policy_step_), then the NetMon step."""
        self.env.policy_step_(q, epsilon, actions, detail)
        self._netmon_step()

    def get_netmon_info(self):
        return self.env.node_obs, self.env.nbr, self.env.agent_node

    def get(self):
        return self.env
