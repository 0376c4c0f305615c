"""Rollout collectors of PPO: one class per rollout path behind one interface (class Rollout), chosen once by
make_rollout.  A collector is built from what it needs — env, policy, config, the six rollout buffers it writes, the fused update step
whose weight images it reads, the generator, the episode log and the policy input / episode starts / LSTM state carried over — and
knows nothing of PPO."""
from __future__ import annotations

import ctypes as C
import os
import time
from collections import deque

import torch
import torch.distributed as dist

_p = lambda t: C.c_void_p(t.data_ptr())
_stream = lambda d: C.c_void_p(torch.cuda.current_stream(d).cuda_stream)


def timeout_bootstrap(policy, gamma, rew, term, trunc, state=None, out=None):
    """rew + gamma V(terminal_obs) where truncated (SB3's collect_rollouts; mask, no host sync), for one step ([N] rewards) or a whole
    rollout ([T, N]).  state: the critic's LSTM state AFTER the step, episode_start False (sb3-contrib [3P-RECALL])."""
    tv = policy.predict_values(term.reshape(-1, term.shape[-1]), state, None).view(trunc.shape)
    return torch.add(rew, gamma * tv * trunc.to(rew.dtype), out=out)


def capture_graphs(device, warmup, reset, parts):
    """Run `warmup` eagerly on a side stream (library handles, workspaces, the env's constants), synchronise, `reset` what it counted,
    then capture every callable of `parts` into a graph of its own (own pool: a graph keeps its tensors alive across replays)."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        warmup()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    reset()
    graphs = [torch.cuda.CUDAGraph() for _ in parts]
    for g, part in zip(graphs, parts):
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            part()
    return graphs


class EpisodeLog:
    """Monitor statistics (SB3's ep_info_buffer): the (raw return, length) the kernel reports for every env that finished an episode in
    a step go into row t of a [T, N, 2] log, NaN elsewhere — one small launch per step; stats() reads it."""

    def __init__(self, n_steps, num_envs, device):
        self.T, self.t, self.buffer = n_steps, 0, deque(maxlen=100)
        self.log = torch.full((n_steps, num_envs, 2), float("nan"), device=device)
        self.nan = torch.full((1, 1), float("nan"), device=device)

    def record(self, done, ep) -> None:
        if ep is not None:
            torch.where(done.view(torch.bool).unsqueeze(1), ep, self.nan, out=self.log[self.t % self.T])
            self.t += 1

    def stats(self) -> dict:
        """rollout/ep_rew_mean and rollout/ep_len_mean as SB3 logs them: means over the last 100 finished episodes (Monitor's raw,
        un-normalised returns).  Reads the log once (one host synchronisation per call)."""
        if self.t > 0:
            T = self.T
            rows = min(self.t, T)
            order = [(self.t - rows + k) % T for k in range(rows)]               # oldest step first
            x = self.log[order].reshape(-1, 2)
            fin = x[~torch.isnan(x[:, 0])]
            if fin.shape[0] > 100:
                fin = fin[-100:]
            for r, l in fin.cpu().tolist():
                self.buffer.append((r, l))
            self.log.fill_(float("nan"))
            self.t = 0
        buf = self.buffer
        if not buf:
            return {}
        return {"rollout/ep_rew_mean": float(sum(r for r, _ in buf) / len(buf)), "rollout/ep_len_mean": float(sum(l for _, l in buf) / len(buf))}


class Rollout:
    """What PPO sees of a collector, and the eager loop's share of it.

    obs, starts   policy input and episode starts of the NEXT step (after finish(): of the next rollout)
    state         recurrent policy: the LSTM state that goes with them, (h_pi, c_pi, h_vf, c_vf) float32 [1, N, H]; current after finish()
    state0        recurrent policy: the LSTM state that entered the current rollout
    begin()       per rollout, where parameters or noise may have changed: gSDE matrices, bf16 shadow weights, summed LSTM biases
    step()        one env step of the whole batch, episode log included; the first step of a rollout opens it (env.begin_rollout, state0)
    finish()      env.end_rollout, the deferred timeout bootstrap, V(next obs) -> last_values; leaves obs / starts / state for the next"""
    vn_allreduce_seconds, vn_allreduce_calls, sde_W = 0.0, 0, None

    def __init__(self, env, policy, cfg, bufs, fused, gen, episodes, carry, stacked=False):
        self.env, self.policy, self.cfg, self.fused, self.gen, self.episodes = env, policy, cfg, fused, gen, episodes
        self.bufs = self.obs_buf, self.act_buf, self.rew_buf, self.val_buf, self.logp_buf, self.start_buf = bufs
        self.device = env.device
        self.N, self.A, self.O, self.T = env.num_envs, env.act_dim, env.obs_dim, cfg.n_steps
        last_obs, last_starts, self.state = carry
        self.obs, self.starts = (env.reset_tensor() if last_obs is None else last_obs).clone(), last_starts.clone()
        self.state0, self.t = None, 0            # t: steps into the current rollout
        self.snap_state, self.snap_full, self.snap_spare = None, None, None
        if policy.recurrent and cfg.seq_len is not None and not stacked:
            # four [S, 1, N, H] snapshot buffers shaped after the state, each the first S slots of a buffer with one spare slot (where
            # the captured rollout sends the steps that open no chunk)
            S = self.T // cfg.seq_len
            self.snap_spare = torch.full((1,), S, dtype=torch.long, device=self.device)
            self.snap_full = tuple(torch.zeros((S + 1,) + tuple(x.shape), device=self.device, dtype=x.dtype) for x in self.state)
            self.snap_state = tuple(x[:S] for x in self.snap_full)

    def _autocast(self):      # (a method, not a lambda kept on the instance: a collector must not sit in a reference cycle, or its graphs die
        # whenever the cycle collector runs — inside another capture, for one)
        return torch.autocast(self.device.type, dtype=torch.bfloat16, enabled=self.cfg.bf16 and self.device.type == "cuda")

    def snapshots(self):
        """seq_len: four float32 [S, 1, N, H] tensors, the state that entered step s * seq_len of the last rollout (before the
        episode-start mask); slot 0 is state0.  None without seq_len."""
        return self.snap_state

    def stacked_snapshots(self):
        """The snapshot storage itself where it is the stacked (actor, critic) pair the fused chunk step reads by address: bf16 h,
        float32 c [S, 2, N, H].  None: the update stages copies of snapshots()."""
        return None

    def begin(self) -> None:
        """gSDE: new exploration matrices (SB3: policy.reset_noise(env.num_envs) at the start of a rollout)."""
        if getattr(self.policy, "use_sde", False):
            gen = self.gen if self.gen.device == self.policy.log_std.device else None
            self.policy.reset_noise(self.N, gen, out=self.sde_W)

    def _enter_step(self) -> int:
        """Step counter; at a rollout's first step the normaliser's per-rollout synchronisation and the LSTM state that enters."""
        t = self.t
        if t == 0:
            getattr(self.env, "begin_rollout", lambda: None)()
            if self.policy.recurrent:
                self.state0 = self._state_now()
        self.t = (t + 1) % self.T
        return t

    def _state_now(self):
        return tuple(s.clone() for s in self.state)

    def _deferred_bootstrap(self) -> None:
        pass

    @torch.no_grad()
    def finish(self):
        getattr(self.env, "end_rollout", lambda: None)()
        with self._autocast():
            self._deferred_bootstrap()
            return self.policy.predict_values(self.obs, self.state, self.starts if self.policy.recurrent else None)


class EagerRollout(Rollout):
    @torch.no_grad()
    def step(self) -> None:
        cfg, pol, t = self.cfg, self.policy, self._enter_step()
        obs, starts = self.obs, self.starts
        if self.snap_state is not None and t % cfg.seq_len == 0:      # the state entering a chunk's first step
            for dst, src in zip(self.snap_state, self.state):
                dst[t // cfg.seq_len].copy_(src)
        with self._autocast():
            actions, values, logp, new_state = pol.act(obs, self.state, starts)
        clipped = torch.clamp(actions, -1.0, 1.0)
        nobs, rew, done, trunc, term, comps, ep = self.env.step_tensor(clipped)
        self.episodes.record(done, ep)
        rew = rew.clone()
        if bool(trunc.any()):   # terminal observation, critic state after this step, no episode start
            with self._autocast():
                rew = timeout_bootstrap(pol, cfg.gamma, rew, term, trunc, new_state)
        for buf, x in zip(self.bufs, (obs, actions, rew, values, logp, starts)):
            buf[t] = x
        self.state = new_state
        self.obs = nobs.clone()
        self.starts = done.to(torch.float32)


class GraphRollout(Rollout):
    """Static tensors: obs / starts / state (before the step), state_new (after it), the step's actions, values, log pi and clipped
    actions, and the step index on the device (int64: index_copy_ takes it as it is)."""

    def __init__(self, *args):
        super().__init__(*args)
        env, d, N, A = self.env, self.device, self.N, self.A
        self.vec = env if hasattr(env, "process_step") else None
        self.raw = env.venv if self.vec is not None else env
        self.act_s, self.clip = torch.zeros((N, A), device=d), torch.zeros((N, A), device=d)
        self.val_s, self.logp_s = torch.zeros(N, device=d), torch.zeros(N, device=d)
        self.t_idx = torch.zeros(1, dtype=torch.long, device=d)
        self.state_new = ()
        if self.policy.recurrent:
            self.state = tuple(x.clone() for x in self.state)
            self.state_new = tuple(torch.zeros_like(x) for x in self.state)
        self.gA, self.gB = capture_graphs(d, self._warmup, self.t_idx.zero_, (self._policy_part, lambda: self._post_part(self.raw_static)))

    def _warmup(self):
        for _ in range(2):                      # (also binds the env's constants)
            self._policy_part()
            self.raw_static = self.raw.step_tensor(self.clip)         # the env returns views of its own (static) buffers
            self._post_part(self.raw_static)

    @torch.no_grad()
    def _policy_part(self):
        pol = self.policy
        if self.snap_full is not None:     # the state entering a chunk's first step goes to its slot, any other step's to the spare one
            L = self.cfg.seq_len
            slot = torch.where(self.t_idx % L == 0, torch.div(self.t_idx, L, rounding_mode="floor"), self.snap_spare)
            for dst, src in zip(self.snap_full, self.state):
                dst.index_copy_(0, slot, src.unsqueeze(0))
        with self._autocast():
            actions, values, logp, new_state = pol.act(self.obs, self.state, self.starts)      # (an MLP policy has no state and ignores the starts)
            for dst, src in zip(self.state_new, new_state or ()):
                dst.copy_(src)
        self.act_s.copy_(actions); self.val_s.copy_(values); self.logp_s.copy_(logp)
        self.clip.copy_(torch.clamp(actions, -1.0, 1.0))

    @torch.no_grad()
    def _post_part(self, raw):
        outs = self.vec.process_step(*raw) if self.vec is not None else raw
        nobs, rew, done, trunc, term, comps, ep = outs
        with self._autocast():
            rew = timeout_bootstrap(self.policy, self.cfg.gamma, rew, term, trunc, self.state_new if self.policy.recurrent else None)
        for buf, x in zip(self.bufs, (self.obs, self.act_s, rew, self.val_s, self.logp_s, self.starts)):
            buf.index_copy_(0, self.t_idx, x.unsqueeze(0))
        self.obs.copy_(nobs)
        self.starts.copy_(done.to(torch.float32))
        if self.policy.recurrent:
            for dst, src in zip(self.state, self.state_new):
                dst.copy_(src)
        self.t_idx.add_(1).remainder_(self.T)

    def begin(self) -> None:
        super().begin()
        if self.fused is not None:
            self.fused.refresh_shadow()         # rollout inference runs on the bf16 shadow weights

    def step(self) -> None:
        self._enter_step()
        self.gA.replay()
        raw = self.raw.step_tensor(self.clip)
        self.episodes.record(raw[2], raw[6])
        self.gB.replay()


class KernelRollout(GraphRollout):
    """Per step: graph A (policy input cast, [LSTM step,] stacked trunks, heads, myo_rollout_sample) -> eager myo_batch_step -> graph B
    (myo_vecnorm_step, myo_rollout_advance).  The timeout bootstrap is applied once per rollout in finish() from term_buf / trunc_buf
    (recurrent policy: with the critic's LSTM state after each step, kept in crit_h_buf / crit_c_buf).

    The policy call of a step is ONE launch on the matrix cores (myo_ppo_mlp_rollout) where the architecture fits and
    MYO_ROLLOUT_GEMM=1 does not ask otherwise, else policy-input cast + hipBLASLt trunk / head GEMMs + bias / activation kernels +
    myo_rollout_sample.

    Recurrent policy: hs / cs hold the LSTM state after the previous step, (actor, critic) stacked; hm / cm the masked copies that
    enter the step; the step's pre-activations / gates are scratch.  h is bf16 (the matrix cores' operand, as the update computes it);
    the CELL state is carried in float32 (cs32 / cm32) — what stock nn.LSTM carries, what policy.predict carries in an evaluation, and
    what a bf16 round trip per step would erode over a 300-step episode.  The bf16 copy cs is what the step leaves for the bootstrap
    buffers (and what the cell-kernel fallback computes in).

    N > 1 ranks with a rank-synchronised normaliser: graph B1 (this rank's batch moments) -> eager all-reduce of 2 O + 3 doubles ->
    graph B2 (running statistics from the global moments, normalise, buffer writes)."""

    def __init__(self, *args, world=1):
        Rollout.__init__(self, *args, stacked=True)
        vec, d, cfg, fused = self.env, self.device, self.cfg, self.fused
        N, A, O, T = self.N, self.A, self.O, self.T
        self.raw, self.lib = vec.venv, fused.lib
        self.obs = self.obs.contiguous()
        self.clip = torch.zeros((N, A), device=d)
        self.t_idx = torch.zeros(1, dtype=torch.int32, device=d)      # (int32: the kernels read it)
        self.draw = torch.zeros(2, dtype=torch.int64, device=d)
        self.x2 = torch.empty((2, N, O), device=d, dtype=torch.bfloat16)
        self.term_buf = torch.zeros((T, N, O), device=d)
        self.trunc_buf = torch.zeros((T, N), device=d)
        self.vn_work = torch.zeros(((N + 127) // 128) * 2 * (O + 1), dtype=torch.float64, device=d)
        self.seed = int(self.gen.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self.rdesc = fused.rollout_desc(self.obs, self.seed, self.draw, self.t_idx, self.obs_buf, self.act_buf, self.val_buf,
                                        self.logp_buf, self.clip) if os.environ.get("MYO_ROLLOUT_GEMM") != "1" else None
        self.snap_h, self.snap_c = None, None
        if self.policy.recurrent:
            H, bf = self.policy.hidden, torch.bfloat16
            self.hs, self.cs = torch.zeros((2, N, H), device=d, dtype=bf), torch.zeros((2, N, H), device=d, dtype=bf)
            self.cs32 = torch.zeros((2, N, H), device=d, dtype=torch.float32)
            self.hs[0].copy_(self.state[0][0]); self.hs[1].copy_(self.state[2][0])
            self.cs32[0].copy_(self.state[1][0]); self.cs32[1].copy_(self.state[3][0])
            self.cs.copy_(self.cs32)
            self.hm, self.cm = torch.empty_like(self.hs), torch.empty_like(self.cs)
            self.cm32 = torch.empty_like(self.cs32)
            self.lat, self.cn = torch.empty_like(self.hs), torch.empty_like(self.hs)
            self.ws = torch.empty((2, N, 4 * H), device=d, dtype=bf)
            self.bsum = torch.zeros((2, 1, 4 * H), device=d, dtype=bf)
            self.crit_h_buf, self.crit_c_buf = torch.zeros((T, N, H), device=d, dtype=bf), torch.zeros((T, N, H), device=d, dtype=bf)
            if cfg.seq_len is not None:      # (allocated once: the update's captured graph reads them by address)
                S = T // cfg.seq_len
                self.snap_h, self.snap_c = torch.zeros((S, 2, N, H), device=d, dtype=bf), torch.zeros((S, 2, N, H), device=d)
        if getattr(self.policy, "use_sde", False):
            # gSDE: myo_rollout_sample_sde leaves actions / log pi in step tensors, the rollout buffers take them by index; the
            # exploration matrices live in a buffer of the collector's own, drawn into in place: the captured graph reads it by address,
            # and whatever policy.act did to policy.exploration_mat in between (an evaluation on another batch size) cannot move it
            self.act_s, self.logp_s = torch.zeros((N, A), device=d), torch.zeros(N, device=d)
            self.sde_W = torch.zeros((N,) + tuple(self.policy.log_std.shape), device=d)
        self.vn_sync = world > 1 and getattr(vec, "sync_ranks", False) and vec.training
        self.vn_batch = torch.zeros(2 * O + 3, dtype=torch.float64, device=d)
        self.begin()
        # the warm-up runs WITHOUT stepping the env: part B runs on the env's static output buffers as they are, and everything it
        # touches is put back afterwards, so the recorded rollout starts exactly at the reset
        self.rawout = tuple(getattr(self.raw, k) for k in ("_obs", "_rew", "_done", "_trunc", "_term", "_comps", "_ep"))
        self.restore = (self.obs, self.starts, vec.obs_rms.buf, vec.ret_rms.buf, vec.returns) + ((self.hs, self.cs, self.cs32) if self.policy.recurrent else ())
        self.keep = [t.clone() for t in self.restore]
        parts = (self._part_a, self._part_b1, self._part_b2) if self.vn_sync else (self._part_a, self._part_b)
        self.gA, self.gB, self.gB2 = (capture_graphs(d, lambda: (self._part_a(), self._part_b()), self._after_warmup, parts) + [None])[:3]
        del self.restore, self.keep

    def _after_warmup(self):
        for t, k in zip(self.restore, self.keep):
            t.copy_(k)
        self.env.old_obs, self.env.old_reward = self.rawout[0], self.rawout[1]      # the env's static output buffers
        self.t_idx.zero_()
        self.draw.zero_()

    def begin(self) -> None:
        super().begin()
        if self.policy.recurrent:           # the summed LSTM biases the recurrent step adds to the input projection
            Lw = self.fused.lstm
            torch.add(Lw["bihh"], Lw["bhhh"], out=self.bsum.view(2, -1))

    def _state_now(self):
        """(h_pi, c_pi, h_vf, c_vf) float32 [1, N, H] from the stacked state."""
        f = lambda z, k: z[k:k + 1].float()
        return (f(self.hs, 0), f(self.cs32, 0).clone(), f(self.hs, 1), f(self.cs32, 1).clone())

    def snapshots(self):
        if self.snap_h is None:
            return None
        h, c = self.snap_h, self.snap_c
        return (h[:, 0:1].float(), c[:, 0:1], h[:, 1:2].float(), c[:, 1:2])

    def stacked_snapshots(self):
        return None if self.snap_h is None else (self.snap_h, self.snap_c)

    # ---- graph A
    def _sample(self, saved, mean_h, value_h, st):
        """Actions, log pi, value of this step into the rollout buffers (row t_idx) and the clipped actions for the env."""
        lib, pol, N, A = self.lib, self.policy, self.N, self.A
        if self.sde_W is None:
            lib.check(lib.L.myo_rollout_sample(_p(mean_h), _p(value_h), _p(pol.log_std.data), N, A, self.seed, _p(self.draw),
                                               _p(self.t_idx), _p(self.act_buf), _p(self.val_buf), _p(self.logp_buf), _p(self.clip), 0, st))
            return
        mu, lat = mean_h.float(), saved[-1][0].float().contiguous()      # latent_pi: the actor trunk's output (LSTM output without a trunk)
        lib.check(lib.L.myo_rollout_sample_sde(_p(mu), _p(lat), _p(self.sde_W), _p(pol.log_std.data), N, lat.shape[1], A,
                                               _p(self.act_s), _p(self.clip), _p(self.logp_s), 0, st))
        t64 = self.t_idx.long()
        self.act_buf.index_copy_(0, t64, self.act_s.unsqueeze(0))
        self.logp_buf.index_copy_(0, t64, self.logp_s.unsqueeze(0))
        self.val_buf.index_copy_(0, t64, value_h.float().view(1, N))

    def _lstm_step(self, st):
        """Snapshot (seq_len), episode-start mask and one step of both LSTMs: lat is their output, hs / cs / cs32 the new state."""
        lib, cfg, fused, N, O, H = self.lib, self.cfg, self.fused, self.N, self.O, self.policy.hidden
        Lw = fused.lstm
        if self.snap_h is not None:     # the state entering a chunk's first step, before the mask (the device decides)
            lib.check(lib.L.myo_rollout_state_snapshot(_p(self.hs), _p(self.cs32), 2, N, H, _p(self.t_idx), cfg.seq_len,
                                                       self.T // cfg.seq_len, _p(self.snap_h), _p(self.snap_c), st))
        keep = torch.rsub(self.starts, 1.0).view(1, N, 1)            # state zeroed where an episode starts
        torch.mul(self.hs, keep, out=self.hm)
        torch.mul(self.cs32, keep, out=self.cm32)
        if fused.step_kernels:       # recurrent product + cell in one launch; nothing kept for a backward pass
            # one projection GEMM for both LSTMs with the bias in its epilogue: row n = [actor 4H | critic 4H], read in place
            gx = torch.addmm(self.bsum.view(8 * H), self.x2[0], Lw["wihh"].view(8 * H, O).t())
            # (cell state in and out in float32; the bf16 copy beside it for the bootstrap buffers)
            lib.check(lib.L.myo_lstm_step_fwd(_p(gx), 4 * H, 8 * H, _p(self.hm), None, _p(Lw["whhh"]), None, 2, N, H,
                                              _p(self.lat), N * H, _p(self.hs), _p(self.cs), None, None, _p(self.cm32), _p(self.cs32), st))
        else:                        # (hidden sizes without a fused time-step kernel: GEMM + cell kernel, cell state through bf16)
            self.cm.copy_(self.cm32)
            gx = torch.baddbmm(self.bsum, self.x2, Lw["wihh"].transpose(1, 2))
            gh = torch.bmm(self.hm, Lw["whhh"].transpose(1, 2))
            lib.check(lib.L.myo_lstm_cell_fwd(_p(gx), _p(gh), _p(self.cm), None, 2 * N, N, H, 1, _p(self.lat), _p(self.hs), _p(self.cs),
                                              _p(self.cn), _p(self.ws), st))
            self.cs32.copy_(self.cs)
        t64 = self.t_idx.long()
        self.crit_h_buf.index_copy_(0, t64, self.hs[1:2])
        self.crit_c_buf.index_copy_(0, t64, self.cs[1:2])

    def _part_a(self):
        if self.rdesc is not None and not self.policy.recurrent:
            self.fused.rollout_policy(self.rdesc)
            return
        st = _stream(self.device)
        # (the policy input of this step into row t_idx of obs_buf and, as bf16, into both halves of x2)
        self.lib.check(self.lib.L.myo_rollout_policy_input(_p(self.obs), self.N, self.O, _p(self.obs_buf), _p(self.x2), 2, _p(self.t_idx), st))
        if self.policy.recurrent:
            self._lstm_step(st)
        saved, mean_h, value_h = self.fused.trunk_heads(self.lat if self.policy.recurrent else self.x2)
        self._sample(saved, mean_h, value_h, st)

    # ---- graph B
    def _part_b1(self):
        vec, st = self.env, _stream(self.device)
        self.lib.check(self.lib.L.myo_vecnorm_batch_moments(_p(self.rawout[0]), _p(self.rawout[1]), self.N, self.O, _p(vec.returns), float(vec.gamma),
                                                            int(vec.training), _p(self.vn_work), _p(self.vn_batch), st))

    def _vecnorm(self, entry, gamma, last):
        """myo_vecnorm_step / myo_vecnorm_finish on the env's static outputs, then myo_rollout_advance.  One argument list for both:
        the step form takes gamma after the returns and ends on its block workspace, the finish form (running statistics from the
        all-reduced batch moments) takes no gamma and ends on those moments."""
        vec, st = self.env, _stream(self.device)
        self.lib.check(entry(
            *(_p(x) for x in self.rawout[:5]), self.N, self.O, _p(vec.obs_rms.mean), _p(vec.obs_rms.var), _p(vec.obs_rms.count),
            _p(vec.ret_rms.buf), _p(vec.returns), *gamma, float(vec.epsilon), float(vec.clip_obs), float(vec.clip_reward),
            int(vec.training), int(vec.norm_obs), int(vec.norm_reward), _p(self.obs), _p(self.starts), _p(self.t_idx),
            _p(self.rew_buf), _p(self.start_buf), _p(self.term_buf), _p(self.trunc_buf), _p(last), st))
        self.lib.check(self.lib.L.myo_rollout_advance(_p(self.t_idx), self.T, _p(self.draw), st))

    def _part_b2(self):
        self._vecnorm(self.lib.L.myo_vecnorm_finish, (), self.vn_batch)

    def _part_b(self):
        if self.vn_sync:
            self._part_b1()
            dist.all_reduce(self.vn_batch)
            self._part_b2()
        else:
            self._vecnorm(self.lib.L.myo_vecnorm_step, (float(self.env.gamma),), self.vn_work)

    def step(self) -> None:
        super().step()
        if self.gB2 is not None:
            # (host time of the eager collective between the two graph replays — enqueue + whatever the call blocks on — accumulated for
            #  the bench line of an N > 1 run: `normalizer_allreduce_ms_per_step`)
            t0 = time.perf_counter()
            dist.all_reduce(self.vn_batch)
            self.vn_allreduce_seconds += time.perf_counter() - t0
            self.vn_allreduce_calls += 1
            self.gB2.replay()

    def _deferred_bootstrap(self) -> None:
        pol, (T, N), st = self.policy, self.trunc_buf.shape, None
        if pol.recurrent:
            # time limits are rare events (one step in max_episode_steps), so the pass is skipped when the rollout has none (one host sync)
            self.state = self._state_now()
            if not bool(self.trunc_buf.any()):
                return
            st = (None, None, self.crit_h_buf.view(1, T * N, pol.hidden).float(), self.crit_c_buf.view(1, T * N, pol.hidden).float())
        timeout_bootstrap(pol, self.cfg.gamma, self.rew_buf, self.term_buf.view(T * N, -1), self.trunc_buf, st, out=self.rew_buf)


def make_rollout(env, policy, cfg, bufs, fused, gen, world, episodes, carry) -> Rollout:
    """The one place that chooses a path.  Captured graphs: use_graphs on a GPU env that steps on device tensors; HIP kernels inside
    them: a fused update step with stacked actor / critic trunks (its images are the rollout's weights) and a VecNormalize around the
    env (the kernels normalise).  The first reset and the graph capture happen here."""
    args = (env, policy, cfg, bufs, fused, gen, episodes, carry)
    if not (cfg.use_graphs and env.device.type == "cuda" and hasattr(env, "step_tensor")):
        return EagerRollout(*args)
    if fused is not None and fused.merged is not None and hasattr(env, "process_step") and hasattr(env, "obs_rms"):
        return KernelRollout(*args, world=world)
    return GraphRollout(*args)
