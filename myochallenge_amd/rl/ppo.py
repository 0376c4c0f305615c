"""PPO rollout/update engine on device tensors (SB3 ``OnPolicyAlgorithm`` / sb3-contrib
``RecurrentPPO`` semantics).

What the reference runs (``RecurrentPPO.learn``; /root/reference/src/train/trainer.py:66-71):
  collect_rollouts: policy forward (no_grad) -> clip -> env.step -> timeout bootstrap
                    ``r += gamma * V(terminal_obs)`` -> buffer.add
  compute_returns_and_advantage: GAE(gamma, lambda) backward scan with episode_starts[t+1]
  train: n_epochs x minibatches; per-minibatch advantage normalisation; clipped surrogate +
         vf_coef * MSE + ent_coef * entropy; clip_grad_norm_; Adam(eps=1e-5)
Here the buffer, the normaliser and the policy stay on the GPU; the env step is one HIP kernel
launch (myo_batch_step).  Multi-GPU: one process per GPU, envs sharded by rank, ONE all-reduce
of a flat fp32 gradient bucket per optimizer step over RCCL (torch.distributed backend "nccl").
"""
from __future__ import annotations

import os
import time
import warnings
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import torch
import torch.distributed as dist

from .. import native
from ..native import (HP_APPLIED, HP_CLIP, HP_COUNT, HP_LAST_KL, HP_LAST_PL, HP_LAST_VL, HP_STOP, HP_SUM_ENTLOSS, HP_SUM_KL,
                      HP_WORDS)
from .fused_lstm import FusedRecurrentPPOStep
from .fused_mlp import FlatAdam, FusedPPOStep, activation_code, flatten_parameters, hp_record_torch
from .policy import ActorCriticPolicy
from .rollout import EpisodeLog, make_rollout


@dataclass
class PPOConfig:
    n_steps: int = 128
    batch_size: int = 4096
    n_epochs: int = 10
    learning_rate: float = 3e-4
    clip_range: float = 0.2
    ent_coef: float = 0.0
    vf_coef: float = 0.5
    gamma: float = 0.99
    gae_lambda: float = 0.95
    max_grad_norm: float = 0.5
    normalize_advantage: bool = True
    bf16: bool = True               # autocast the policy GEMMs to bf16 (fp32 master weights)
    sync_adv_moments: bool = False  # all-reduce advantage moments (exact single-process semantics)
    use_graphs: bool = True         # capture one optimizer step in a hipGraph (MLP policy, GPU only)
    # N > 1 ranks: capture the RCCL all-reduce of the flat gradient INSIDE the optimizer hipGraph (forward/backward -> all-reduce ->
    # clip + Adam as ONE replay per minibatch instead of graph / eager collective / graph).  Opt-in (also MYO_GRAPH_ALLREDUCE=1):
    # it saves one launch gap (~10 us of a ~150 us optimizer step) and could only be exercised on a node with >= 2 GPUs, which
    # the build machine does not have — a capture failure there must not cost the scaling run.  Falls back to the eager
    # collective when the capture raises.
    graph_allreduce: bool = False
    # SB3 schedules f(progress_remaining) -> value, evaluated by train() once per update; learning_rate / clip_range above stay
    # plain floats (the schedules' values at progress 1.0, or the constants when there is no schedule)
    lr_schedule: Optional[Callable] = None
    clip_range_schedule: Optional[Callable] = None
    # SB3's KL early stop: a minibatch whose approx_kl exceeds 1.5 * target_kl is not applied and ends the update
    target_kl: Optional[float] = None
    clip_range_vf: Optional[float] = None   # value-function clipping is not implemented: anything but None is refused
    # Recurrent policies: truncated BPTT as sb3-contrib trains (a minibatch = batch_size consecutive transitions, every sequence started
    # from the LSTM state stored with its first transition [3P-RECALL, sb3-contrib 1.6.2 RecurrentRolloutBuffer]).  None: a minibatch is
    # batch_size // n_steps whole rollouts from the state of the rollout start.  L: every env's rollout is cut into n_steps // L aligned
    # chunks of L steps, a minibatch is batch_size // L chunks drawn from one permutation of all of them, each started from the state the
    # rollout stored as it entered the chunk's first step (DESIGN.md §6 lists the differences from sb3-contrib).  The SB3 zip has no such
    # field: a resumed run passes seq_len again.
    seq_len: Optional[int] = None

    def __post_init__(self):
        if self.seq_len is not None:
            if self.seq_len < 1:
                raise ValueError(f"seq_len={self.seq_len}: a chunk has at least one step")
            if self.n_steps % self.seq_len:
                raise ValueError(f"seq_len={self.seq_len} does not divide n_steps={self.n_steps}: chunks are aligned, none is padded")
            if self.batch_size % self.seq_len:
                raise ValueError(f"seq_len={self.seq_len} does not divide batch_size={self.batch_size}: a minibatch is whole chunks")
        if self.clip_range_vf is not None:
            raise NotImplementedError("clip_range_vf (value-function clipping) is not implemented; leave it None")
        if self.lr_schedule is not None:
            self.learning_rate = float(self.lr_schedule(1.0))
        if self.clip_range_schedule is not None:
            self.clip_range = float(self.clip_range_schedule(1.0))


def compute_gae(rewards, values, episode_starts, last_values, last_dones, gamma, lam):
    """rewards/values/episode_starts [T,N]; SB3 buffer semantics: non-terminal mask for step t is
    1 - episode_starts[t+1] (1 - dones for the last step).  On the GPU this is one HIP kernel
    (myo_gae); the torch loop below is the CPU statement of the same scan."""
    T = rewards.shape[0]
    if rewards.is_cuda and rewards.dtype == torch.float32:
        import ctypes as C
        lib = native.load()
        adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
        p = lambda t: C.c_void_p(t.contiguous().data_ptr())
        lv, ld = last_values.float().contiguous(), last_dones.float().contiguous()
        lib.check(lib.L.myo_gae(p(rewards), p(values), p(episode_starts), p(lv), p(ld), T, rewards.shape[1],
                                float(gamma), float(lam), p(adv), p(ret),
                                C.c_void_p(torch.cuda.current_stream(rewards.device).cuda_stream)))
        return adv, ret
    adv = torch.zeros_like(rewards)
    last = torch.zeros_like(last_values)
    for t in reversed(range(T)):
        if t == T - 1:
            nonterm, nextv = 1.0 - last_dones, last_values
        else:
            nonterm, nextv = 1.0 - episode_starts[t + 1], values[t + 1]
        delta = rewards[t] + gamma * nextv * nonterm - values[t]
        last = delta + gamma * lam * nonterm * last
        adv[t] = last
    return adv, adv + values


class PPO:
    def __init__(self, env, policy: ActorCriticPolicy, cfg: PPOConfig = PPOConfig(), seed: int = 0):
        self.env, self.policy, self.cfg = env, policy, cfg
        self.device = env.device
        self.policy.to(self.device)
        on_gpu = self.device.type == "cuda"
        if cfg.target_kl is not None and (cfg.graph_allreduce or os.environ.get("MYO_GRAPH_ALLREDUCE") == "1"):
            raise ValueError("target_kl needs the host between gradient and optimizer step on N > 1 ranks (the all-reduced approx_kl "
                             "decides): it cannot be combined with graph_allreduce")
        if cfg.seq_len is not None:
            if not policy.recurrent:
                raise ValueError("seq_len cuts the sequences of a recurrent policy: this policy has no LSTM")
            if cfg.batch_size // cfg.seq_len > env.num_envs * cfg.n_steps // cfg.seq_len:
                raise ValueError(f"batch_size={cfg.batch_size} asks for {cfg.batch_size // cfg.seq_len} chunks of {cfg.seq_len} steps, the "
                                 f"rollout has {env.num_envs * cfg.n_steps // cfg.seq_len}")
        if not policy.recurrent and (cfg.n_steps * env.num_envs) % min(cfg.batch_size, cfg.n_steps * env.num_envs):
            # SB3 warns here too and then trains on the truncated last minibatch of each epoch; every update path of this
            # class works on fixed-size minibatches (one captured graph) and SKIPS that remainder instead
            warnings.warn(f"rollout of {cfg.n_steps * env.num_envs} samples is not a multiple of batch_size={cfg.batch_size}: the last "
                          f"{(cfg.n_steps * env.num_envs) % cfg.batch_size} samples of every epoch's permutation are not trained on "
                          "(stable-baselines3 would train on them as a truncated minibatch)")
        self._fused = None           # FusedPPOStep: the hand-derived MLP minibatch step
        self._fused_rec = None       # FusedRecurrentPPOStep: the hand-derived recurrent minibatch step
        self._flat_adam = None       # FlatAdam over the flat parameter vector: every captured update path has one
        fused = None
        # (a hidden activation the kernels do not compute — anything but ReLU / Tanh: no fused object and no flat vectors, the update
        # is eager autograd and the rollout goes through the torch module, as for gSDE without stacked views below)
        if cfg.use_graphs and on_gpu and activation_code(self.policy) is not None:
            # flat parameter / gradient vectors (before any graph captures addresses) and the one-kernel optimiser, so that a whole
            # minibatch step (forward, backward, clip + Adam) is ONE hipGraph.  The forward / backward of it is hand-derived
            # (rl/fused_mlp.py, rl/fused_lstm.py) or, for a recurrent policy without such a step, autograd on the flat vectors.
            lib = native.load()
            self._flat_adam = FlatAdam(flatten_parameters(self.policy), lib, cfg.learning_rate, cfg.max_grad_norm)
            if not policy.recurrent:
                self._fused = FusedPPOStep(self.policy, lib, cfg.clip_range, cfg.ent_coef, cfg.vf_coef)
                if getattr(policy, "use_sde", False) and self._fused.merged is None:
                    self._fused = self._flat_adam = None         # gSDE has a loss stage on the stacked-trunk path only: eager autograd
            elif cfg.bf16 and os.environ.get("MYO_RECURRENT_AUTOGRAD") != "1":
                # (None when the layout has no stacked actor/critic views)
                self._fused_rec = FusedRecurrentPPOStep.create(self.policy, lib, cfg.clip_range, cfg.ent_coef, cfg.vf_coef)
            fused = self._fused if self._fused is not None else self._fused_rec
            if fused is not None:        # one bf16 shadow of the flat vector: the Adam kernel keeps it in step
                self._flat_adam.shadow = fused.half[0]
                fused.adam_syncs_shadow = True
                fused.refresh_shadow()
        self.optimizer = torch.optim.Adam(self.policy.parameters(), lr=cfg.learning_rate, eps=1e-5,
                                          capturable=on_gpu, foreach=True if on_gpu else None)
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # the device-resident hyper-parameter block of the fused update paths (layout: include/myobatch.h): lr, clip_range, KL limit,
        # stop flag, applied-step count and the diagnostics' sums.  train() writes it before every update, outside the graphs.
        self._hp = None
        if self._flat_adam is not None:
            self._hp = torch.zeros(HP_WORDS, device=self.device)
            self._flat_adam.hp = self._hp
            if fused is not None:
                fused.hp = self._hp
        self._current_progress_remaining = 1.0
        self._total_timesteps = None
        self._lr_now, self._clip_now = float(cfg.learning_rate), float(cfg.clip_range)
        self._hp_write()                 # (a minibatch step run before the first train(), as the tests do, reads the block too)
        if self._fused is not None and self.world == 1 and os.environ.get("MYO_ADAM_SEPARATE") != "1":
            self._fused.adam = self._flat_adam   # nothing is exchanged between gradient and clip: the fused step also squares the gradient
        if self._fused is not None and os.environ.get("MYO_PPO_RESIDENT") != "0":
            # the fused step's operand images stay resident: rebuilt once per train(), kept current by the Adam kernel (any world size)
            self._fused.resident_adam = self._flat_adam
        self.rank = dist.get_rank() if self.world > 1 else 0
        N, T, O, A = env.num_envs, cfg.n_steps, env.obs_dim, env.act_dim
        d = self.device
        self.obs_buf = torch.zeros((T, N, O), device=d)
        self.act_buf = torch.zeros((T, N, A), device=d)
        self.rew_buf = torch.zeros((T, N), device=d)
        self.val_buf = torch.zeros((T, N), device=d)
        self.logp_buf = torch.zeros((T, N), device=d)
        self.start_buf = torch.zeros((T, N), device=d)
        self._last_obs = None
        self._last_starts = torch.ones(N, device=d)
        self._state = policy.initial_state(N, d)
        self._rollout_state0 = None
        self._last_values = None
        self._rollout = None             # the collector (rl/rollout.py), made at the first rollout step: the ONE rollout attribute here
        self._episodes = EpisodeLog(T, N, d)
        self.num_timesteps = 0
        self.n_updates = 0
        self.gen = torch.Generator(device=self.device if on_gpu else "cpu")   # minibatch permutations on the device
        self.gen.manual_seed(seed + 1000 * self.rank)
        nparam = sum(p.numel() for p in self.policy.parameters())
        self._flat_grad = self.policy._flat["g"] if self._flat_adam is not None else torch.zeros(nparam, device=d)
        # state that the update fills in later: the captured MLP step (_build_graphs) and the captured recurrent step
        # (_build_recurrent_graphs), each with the shape it was captured for, its static tensors and its graphs
        self._graph, self._gs, self._graph_fb, self._graph_ap, self._graph_epoch, self._epoch_chunk = None, None, None, None, None, 0
        self._rgraph, self._rg, self._rgraph_fb, self._rgraph_ap, self._rgraph_L = None, None, None, None, None
        self._allreduce_in_graph = False
        self._early_stopped, self._last_diag = False, None

    def _autocast(self):
        on = self.cfg.bf16 and self.device.type == "cuda"
        return torch.autocast(device_type=self.device.type, dtype=torch.bfloat16, enabled=on)

    # ---------------------------------------------------------------- rollout (rl/rollout.py)
    def _collector(self):
        """The rollout collector, made at the first rollout step: the path is chosen, the env reset and the graphs captured there."""
        if self._rollout is None:
            bufs = (self.obs_buf, self.act_buf, self.rew_buf, self.val_buf, self.logp_buf, self.start_buf)
            fused = self._fused if self._fused is not None else self._fused_rec
            self._rollout = make_rollout(self.env, self.policy, self.cfg, bufs, fused, self.gen, self.world, self._episodes,
                                         (self._last_obs, self._last_starts, self._state))
        return self._rollout

    def rollout_step(self) -> None:
        """One environment step for the whole batch."""
        r = self._collector()
        r.step()
        self._rollout_state0 = r.state0

    def finish_rollout(self) -> None:
        r = self._rollout
        self._last_values = r.finish()
        self._last_obs, self._last_starts, self._state = r.obs, r.starts, r.state

    def collect_rollouts(self) -> None:
        self._collector().begin()
        for _ in range(self.cfg.n_steps):
            self.rollout_step()
        self.finish_rollout()
        self.num_timesteps += self.cfg.n_steps * self.env.num_envs * self.world

    def rollout_snapshots(self):
        """seq_len: (h_pi, c_pi, h_vf, c_vf) float32 [S, 1, N, H], the LSTM state that entered step s * seq_len of the last rollout
        (before the episode-start mask), whichever rollout path stored it.  Slot 0 is _rollout_state0."""
        return self._rollout.snapshots() if self._rollout is not None else None

    def episode_stats(self) -> Dict[str, float]:
        """rollout/ep_rew_mean and rollout/ep_len_mean as SB3 logs them: means over the last 100 finished episodes (Monitor's raw,
        un-normalised returns; /root/reference/src/main_baoding.py runs under SB3's logger)."""
        return self._episodes.stats()

    # (read-only views of the collector for the benchmark: policy input / episode starts of the next step, and the host time of the
    # rank-synchronised normaliser's all-reduce)
    ep_info_buffer = property(lambda self: self._episodes.buffer)
    _obs_s = property(lambda self: self._rollout.obs)
    _starts_s = property(lambda self: self._rollout.starts)
    vn_allreduce_seconds = property(lambda self: self._rollout.vn_allreduce_seconds if self._rollout is not None else 0.0)
    vn_allreduce_calls = property(lambda self: self._rollout.vn_allreduce_calls if self._rollout is not None else 0)

    # ---------------------------------------------------------------- update
    def _allreduce_grads(self) -> None:
        if self.world == 1:
            return
        off = 0
        for p in self.policy.parameters():
            n = p.numel()
            self._flat_grad[off:off + n] = p.grad.reshape(-1) if p.grad is not None else 0
            off += n
        dist.all_reduce(self._flat_grad, op=dist.ReduceOp.SUM)
        self._flat_grad /= self.world
        off = 0
        for p in self.policy.parameters():
            n = p.numel()
            p.grad = self._flat_grad[off:off + n].view_as(p).clone()
            off += n

    def _global_adv_moments(self, a):
        """(mean, unbiased std) of the advantages `a` of this rank's minibatch taken over the minibatches of ALL ranks: one all-reduce of
        (sum, sum of squares, count), in the dtype of `a`."""
        m = torch.stack([a.sum(), (a * a).sum(), torch.tensor(float(a.numel()), dtype=a.dtype, device=a.device)])
        if self.world > 1:
            dist.all_reduce(m)
        mean = m[0] / m[2]
        return mean, torch.sqrt(torch.clamp(m[1] / m[2] - mean * mean, min=0.0) * m[2] / (m[2] - 1))

    def _loss(self, values, logp, entropy, old_logp, adv, returns):
        cfg = self.cfg
        if cfg.normalize_advantage and adv.numel() > 1:
            if cfg.sync_adv_moments and self.world > 1:
                mean, std = self._global_adv_moments(adv)
            else:
                mean, std = adv.mean(), adv.std()
            adv = (adv - mean) / (std + 1e-8)
        ratio = torch.exp(logp - old_logp)
        if self._hp is not None:     # (the autograd recurrent graph: clip_range from the hyper-parameter block, read at replay time)
            clip = self._hp[HP_CLIP]
        else:
            clip = self._clip_now
        pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
        vl = torch.nn.functional.mse_loss(values, returns)
        ent = entropy.mean() if torch.is_tensor(entropy) and entropy.dim() > 0 else entropy      # gSDE: per sample
        with torch.no_grad():        # SB3's diagnostics of the minibatch: approx_kl, clip_fraction, entropy_loss
            log_ratio = logp - old_logp
            kl = ((torch.exp(log_ratio) - 1) - log_ratio).mean()
            cf = (torch.abs(ratio - 1) > clip).float().mean()
            el = -torch.as_tensor(ent, device=kl.device).detach().float()
            self._last_diag = (kl, cf, el)
            if self._hp is not None:
                hp_record_torch(self._hp, pl.detach(), vl.detach(), kl, cf, el)
        return pl + cfg.ent_coef * (-ent) + cfg.vf_coef * vl, pl.detach(), vl.detach()

    # ---------------------------------------------------------------- schedules, KL stop, diagnostics
    def _update_hyper(self):
        """learning_rate / clip_range of this update from the schedules at the current progress_remaining, written everywhere an update
        path reads them: the torch optimiser, FlatAdam, the fused steps' launch scalars and the hyper-parameter block (one small
        asynchronous copy that also clears the stop flag, the applied count and the diagnostics)."""
        cfg = self.cfg
        prog = self._current_progress_remaining
        self._lr_now = float(cfg.lr_schedule(prog)) if cfg.lr_schedule is not None else float(cfg.learning_rate)
        self._clip_now = float(cfg.clip_range_schedule(prog)) if cfg.clip_range_schedule is not None else float(cfg.clip_range)
        for group in self.optimizer.param_groups:
            group["lr"] = self._lr_now
        if self._flat_adam is not None:
            self._flat_adam.lr = self._lr_now
        for fused in (self._fused, self._fused_rec):
            if fused is not None:
                fused.clip = self._clip_now
        self._hp_write()

    def _hp_write(self):
        if self._hp is not None:
            cfg = self.cfg
            # N > 1 ranks decide on the all-reduced approx_kl on the host (between the two graphs): no limit on the device
            limit = 1.5 * cfg.target_kl if (cfg.target_kl is not None and self.world == 1) else 0.0
            self._hp.copy_(torch.tensor([self._lr_now, self._clip_now, limit] + [0.0] * (HP_WORDS - 3)), non_blocking=True)

    def _hp_new_epoch(self):
        """The diagnostics are means over the minibatches of the last epoch run: their sums start again with every epoch."""
        self._hp[HP_COUNT:HP_SUM_ENTLOSS + 1].zero_()

    def _hp_stopped(self) -> bool:
        """The stop flag of the hyper-parameter block: one 4-byte copy to the host (only ever called with target_kl set)."""
        return bool(self._hp[HP_STOP:HP_STOP + 1].view(torch.int32).cpu().item())

    def _kl_exceeded(self, kl) -> bool:
        """SB3's `approx_kl > 1.5 * target_kl` on the host (eager paths; N > 1 ranks: on the rank mean, so every rank stops at the
        same step)."""
        if self.cfg.target_kl is None:
            return False
        if self.world > 1:
            kl = kl.detach().clone().reshape(1)
            dist.all_reduce(kl)
            kl = kl / self.world
        return float(kl) > 1.5 * self.cfg.target_kl

    def _kl_exceeded_ranks(self) -> bool:
        """N > 1 ranks on a fused path: the approx_kl the loss kernel has just recorded, all-reduced (mean), against the limit."""
        return self._kl_exceeded(self._hp[HP_LAST_KL])

    def train(self) -> Dict[str, float]:
        """One PPO update on the current rollout (SB3 PPO.train / sb3-contrib RecurrentPPO.train [3P-RECALL]): learning_rate and
        clip_range from their schedules at the current progress_remaining; with target_kl, a minibatch whose approx_kl =
        mean((ratio - 1) - log ratio) exceeds 1.5 * target_kl is NOT applied and ends the update, its remaining epochs included.

        Returns policy_loss / value_loss (last minibatch processed), n_updates (optimizer steps applied so far), approx_kl,
        clip_fraction and entropy_loss — all three MEANS OVER THE MINIBATCHES PROCESSED IN THE LAST EPOCH RUN, the minibatch that
        stopped the update included (SB3 resets approx_kl per epoch too, but averages the other two over all epochs) —
        explained_variance (1 - Var(returns - values) / Var(returns) over the rollout buffer), the learning_rate and clip_range used,
        and early_stopped.  On the fused paths the three means come from the hyper-parameter block's sums."""
        cfg = self.cfg
        self._update_hyper()
        adv, ret = compute_gae(self.rew_buf, self.val_buf, self.start_buf, self._last_values,
                               self._last_starts, cfg.gamma, cfg.gae_lambda)
        stats = {}
        self._early_stopped, diag = False, []
        if self._fused is not None:
            pl, vl = self._train_graphed(adv, ret)
        elif self._flat_adam is not None:
            pl, vl = self._train_recurrent_graphed(adv, ret)
        else:
            pl, vl, diag = self._train_eager(adv, ret)
        if self._hp is not None:        # fused paths: the block's sums, ONE copy to the host (it also carries pl / vl)
            hp = self._hp.cpu()
            hi = hp.view(torch.int32)
            cnt = max(1, int(hi[HP_COUNT]))
            kl, cf, el = (float(x) / cnt for x in hp[HP_SUM_KL:HP_SUM_KL + 3])
            if cfg.target_kl is not None:
                if self.world == 1:
                    self.n_updates += int(hi[HP_APPLIED])
                    self._early_stopped = bool(hi[HP_STOP])
                pl, vl = hp[HP_LAST_PL], hp[HP_LAST_VL]       # (of the last minibatch processed: later replayed steps changed nothing)
        else:
            kl, cf, el = (float(x) for x in torch.stack(diag).mean(0)) if diag else (float("nan"),) * 3
        y, err = ret.reshape(-1), (ret - self.val_buf).reshape(-1)
        var_y = float(y.var(unbiased=False))
        ev = float("nan") if var_y == 0 else 1.0 - float(err.var(unbiased=False)) / var_y       # SB3 utils.explained_variance
        stats.update(policy_loss=float(pl), value_loss=float(vl), n_updates=self.n_updates, approx_kl=kl, clip_fraction=cf,
                     entropy_loss=el, explained_variance=ev, learning_rate=self._lr_now, clip_range=self._clip_now,
                     early_stopped=self._early_stopped)
        return stats

    # ---------------------------------------------------------------- eager update (CPU, use_graphs=False, gSDE without stacked trunks)
    def _train_eager(self, adv, ret):
        """Autograd + torch Adam.  MLP policy: minibatches are rows of the flattened buffer; recurrent policy: whole rollouts of a
        subset of envs, initial LSTM state = state at rollout start, or with seq_len chunks of the rollouts from the stored state
        that entered them.  Returns the last minibatch's losses and the last epoch's diagnostics."""
        cfg, pol = self.cfg, self.policy
        T, N = cfg.n_steps, self.env.num_envs
        if pol.recurrent and cfg.seq_len is not None:
            L = cfg.seq_len
            n_items, k = N * (T // L), cfg.batch_size // L
            snaps = self.rollout_snapshots()

            def evaluate(items):
                return self._chunk_loss(items, snaps, adv, ret)
        elif pol.recurrent:
            n_items, k = N, max(1, min(N, cfg.batch_size // T))

            def evaluate(idx):
                st0 = tuple(x[:, idx] for x in self._rollout_state0)
                with self._autocast():
                    v, lp, ent = pol.evaluate_actions(self.obs_buf[:, idx], self.act_buf[:, idx], st0, self.start_buf[:, idx])
                return self._loss(v.reshape(-1), lp.reshape(-1), ent, self.logp_buf[:, idx].reshape(-1),
                                  adv[:, idx].reshape(-1), ret[:, idx].reshape(-1))
        else:
            n_items = B = T * N
            k = min(cfg.batch_size, B)
            obs, act = self.obs_buf.view(B, -1), self.act_buf.view(B, -1)
            oldlp, advf, retf = self.logp_buf.view(B), adv.view(B), ret.view(B)

            def evaluate(idx):
                with self._autocast():
                    v, lp, ent = pol.evaluate_actions(obs[idx], act[idx])
                return self._loss(v, lp, ent, oldlp[idx], advf[idx], retf[idx])
        for _ in range(cfg.n_epochs):
            diag = []
            perm = torch.randperm(n_items, generator=self.gen, device=self.device)
            for s in range(0, n_items - k + 1, k):
                loss, pl, vl = evaluate(perm[s:s + k])
                diag.append(torch.stack(self._last_diag))
                if self._kl_exceeded(self._last_diag[0]):
                    self._early_stopped = True
                    break
                self.optimizer.zero_grad(set_to_none=True)
                loss.backward()
                self._allreduce_grads()
                torch.nn.utils.clip_grad_norm_(pol.parameters(), cfg.max_grad_norm)
                self.optimizer.step()
                self.n_updates += 1
            if self._early_stopped:
                break
        return pl, vl, diag

    def _chunk_loss(self, items, snaps, adv, ret):
        """The loss of a minibatch of chunks (seq_len): item c = chunk c // N of env c % N, steps [s L, (s + 1) L), evaluated in one
        call on [L, m, .] tensors from the snapshot states gathered per item (no host synchronisation: capturable)."""
        N, L = self.env.num_envs, self.cfg.seq_len
        s, n = torch.div(items, N, rounding_mode="floor"), items % N
        tt = (s * L).unsqueeze(0) + torch.arange(L, device=items.device).unsqueeze(1)        # [L, m] rollout steps
        sel = lambda buf: buf[tt, n]
        st0 = tuple(x[s, 0, n].unsqueeze(0) for x in snaps)
        with self._autocast():
            v, lp, ent = self.policy.evaluate_actions(sel(self.obs_buf), sel(self.act_buf), st0, sel(self.start_buf))
        return self._loss(v.reshape(-1), lp.reshape(-1), ent, sel(self.logp_buf).reshape(-1), sel(adv).reshape(-1), sel(ret).reshape(-1))

    # ---------------------------------------------------------------- hipGraph-captured minibatch step
    def _mb_forward_backward(self):
        g, cfg = self._gs, self.cfg
        idx = g["idx"]
        pl, vl = self._fused.run_indexed(g["obs"], g["act"], g["oldlp"], g["adv"], g["ret"], idx)
        g["pl"], g["vl"] = pl, vl                 # views of the loss kernel's accumulator: no copies      # gradients land in the flat vector (p.grad are views of it)

    def _mb_apply(self):
        self._flat_adam.step(1.0 / self.world)    # all-reduce SUM ran in place on the flat gradient

    def _capture_step(self, forward_backward, g, graph_allreduce=False, epoch_steps=0, epoch_begin=None, step_begin=None):
        """Capture one minibatch step — forward_backward() on the static tensors `g`, then _mb_apply() — and return
        (fb, ap, epoch, allreduce_inside).  One rank: `fb` is the whole step.  N > 1 ranks: `fb` ends with the gradient, the RCCL
        all-reduce runs eagerly, and `ap` is clip + Adam; or, with graph_allreduce on the nccl backend, `fb` is the whole step with the
        collective inside it (ap None, allreduce_inside True).  epoch_steps = k > 0 also captures `epoch`: k minibatch steps, each
        with its index copy out of g["perm"] (allocated here), in one graph; epoch_begin() is captured ahead of the k steps (work on
        the whole window g["perm"]) and step_begin(j) is called before step j is captured, step_begin(None) after the last.  The
        parameters and the Adam state come out as they went in."""
        d = self.device
        side = torch.cuda.Stream(device=d)
        # warm-up and capture must not move the parameters.  The snapshot is taken BEFORE the side stream is told to wait: its copies run
        # on the current stream, and a warm-up optimizer step on the side stream that overtook them left some ranks restoring a state two
        # Adam steps ahead (replicas of >= 4 ranks sharing a GPU differed; found by the config-D-shape test)
        snap = self._flat_adam.snapshot()
        side.wait_stream(torch.cuda.current_stream(d))
        with torch.cuda.stream(side):       # eager warm-up (library handles, workspaces)
            for _ in range(2):
                forward_backward()
                if self.world > 1:
                    dist.all_reduce(self._flat_grad)
                self._mb_apply()
        torch.cuda.current_stream(d).wait_stream(side)
        torch.cuda.synchronize(d)
        fb, ap, epoch, inside = torch.cuda.CUDAGraph(), None, None, False
        # The gradient all-reduce INSIDE the optimizer hipGraph (forward / backward -> RCCL all-reduce -> clip + Adam, one replay per
        # minibatch): opt-in, nccl (= RCCL) only.  There is no in-process fallback from a failed capture: measured on a one-GPU box with a
        # backend that synchronises inside the capture (gloo), the capture is invalidated, capture_end throws inside torch's graph
        # destructor and the process dies (tests/test_gpu_parity.py).  So a backend that cannot be captured is refused up front
        # (warning, eager collective between two graphs — the tested default), and a capture failure on nccl is raised as an error.
        if graph_allreduce and dist.get_backend() != "nccl":
            warnings.warn(f"graph_allreduce needs the nccl (RCCL) backend, this process group is {dist.get_backend()!r}: "
                          "using the eager all-reduce between the two optimizer graphs")
        elif graph_allreduce:
            try:
                with torch.cuda.graph(fb, capture_error_mode="thread_local"):
                    forward_backward()
                    dist.all_reduce(self._flat_grad, op=dist.ReduceOp.SUM)
                    self._mb_apply()
            except Exception as exc:        # noqa: BLE001
                raise RuntimeError("capturing the RCCL gradient all-reduce inside the optimizer hipGraph failed; run without "
                                   "graph_allreduce / MYO_GRAPH_ALLREDUCE (the eager collective between two graphs)") from exc
            inside = True
        if not inside:
            with torch.cuda.graph(fb, capture_error_mode="thread_local"):
                forward_backward()
                if self.world == 1:             # single GPU: forward, backward and optimiser in ONE graph
                    self._mb_apply()
            if self.world > 1:                  # the RCCL all-reduce runs between the two graphs
                ap = torch.cuda.CUDAGraph()
                with torch.cuda.graph(ap, capture_error_mode="thread_local"):
                    self._mb_apply()
        if epoch_steps:
            bs = g["idx"].numel()
            g["perm"] = torch.zeros(epoch_steps * bs, dtype=torch.long, device=d)
            g["perm"].copy_(torch.arange(epoch_steps * bs, device=d))
            torch.cuda.synchronize(d)
            epoch = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(epoch, capture_error_mode="thread_local"):
                    if epoch_begin is not None:
                        epoch_begin()
                    for s in range(0, epoch_steps * bs, bs):
                        if step_begin is not None:
                            step_begin(s // bs)
                        g["idx"].copy_(g["perm"][s:s + bs])
                        forward_backward()
                        self._mb_apply()
            finally:
                if step_begin is not None:
                    step_begin(None)
        self._flat_adam.restore(snap)
        return fb, ap, epoch, inside

    def _run_captured(self, n_items, k, g, fb, ap, stats=None, epoch=None, adv_of=None):
        """The epochs and minibatches of a captured update: a permutation of n_items per epoch, k of them per minibatch, staged by
        copying their indices into g["idx"] and run by replaying `fb` (one rank, or the all-reduce inside the graph: the whole step;
        else gradient -> eager all-reduce -> `ap`).  stats: where the moments of the GLOBAL minibatch's advantages go when the step
        does not compute them itself (adv_of(items): those advantages, where the items are not columns of g["adv"]).  epoch: the graph of
        _epoch_chunk whole steps, which then runs the epoch (_replay_epoch_chunked)."""
        cfg = self.cfg
        tkl = cfg.target_kl is not None
        # one rank with target_kl: the step itself compares approx_kl with the limit in the hyper-parameter block and, past it, raises
        # the block's stop flag and applies nothing more.  The host reads the flag once per epoch and takes n_updates from the block's
        # applied count (train).  Everywhere else n_updates is counted here.
        device_stop = tkl and self.world == 1
        stopped = False
        for _ in range(cfg.n_epochs):
            self._hp_new_epoch()
            perm = torch.randperm(n_items, generator=self.gen, device=self.device)
            if epoch is not None:
                stopped = self._replay_epoch_chunked(perm, g, k, n_items // k, epoch, fb, device_stop)
                if not device_stop:
                    self.n_updates += n_items // k
            else:
                for s in range(0, n_items - k + 1, k):
                    g["idx"].copy_(perm[s:s + k])
                    if stats is not None:
                        items = perm[s:s + k]
                        mean, std = self._global_adv_moments((adv_of(items) if adv_of is not None else g["adv"][..., items]).double())
                        stats.copy_(torch.stack([mean, std]).float())
                    fb.replay()
                    if ap is not None:
                        dist.all_reduce(self._flat_grad, op=dist.ReduceOp.SUM)
                        if tkl and self._kl_exceeded_ranks():      # the decision between the two graphs: this step is not applied
                            self._early_stopped = stopped = True
                            break
                        if self._dp_check:
                            self._dp_compare("gradient after the all-reduce", self._flat_grad)
                            self._dp_compare("parameters before the optimizer step", self._flat_adam.flat["p"])
                            self._dp_compare("Adam m before the optimizer step", self._flat_adam.m)
                            self._dp_compare("Adam v before the optimizer step", self._flat_adam.v)
                            self._dp_compare("Adam step counter before the optimizer step", self._flat_adam._step)
                        ap.replay()
                        if self._dp_check:
                            self._dp_compare("gradient after the optimizer step", self._flat_grad)
                            self._dp_compare("|g|^2 partial sums", self._flat_adam.sq[:64].contiguous())
                            self._dp_compare("parameters after the optimizer step", self._flat_adam.flat["p"])
                    if not device_stop:
                        self.n_updates += 1
                if device_stop and not stopped:                      # steps after a stop changed nothing: one read per epoch
                    stopped = self._hp_stopped()
            if stopped:
                break

    def _replay_epoch_chunked(self, perm, g, bs, n_mb, epoch, fb, device_stop) -> bool:
        """One epoch (one rank) as replays of the chunk graph `epoch`, each fed _epoch_chunk minibatches of `perm` through g["perm"],
        and what is left of the epoch on the per-step graph.  Returns whether the stop flag is up: read after a chunk that does not
        end the epoch, and once after the tail."""
        k, done, stopped = self._epoch_chunk, 0, False
        while n_mb - done >= k and not stopped:        # whole chunks: one replay each
            g["perm"].copy_(perm[done * bs:(done + k) * bs])
            epoch.replay()
            done += k
            stopped = device_stop and done < n_mb and self._hp_stopped()
        if not stopped:
            for j in range(done, n_mb):                # what is left of the epoch: the per-step graph
                g["idx"].copy_(perm[j * bs:(j + 1) * bs])
                fb.replay()
            stopped = device_stop and self._hp_stopped()
        return stopped

    _dp_check = bool(os.environ.get("MYO_DP_CHECK"))

    def _dp_compare(self, what: str, x: torch.Tensor) -> None:
        """MYO_DP_CHECK=1 (developer diagnostic of the N > 1 path): a bit-level checksum of `x` must be the same on every rank."""
        cs = x.detach().contiguous().view(torch.int32).to(torch.int64).sum().reshape(1)
        lo, hi = cs.clone(), cs.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        if int(lo[0]) != int(hi[0]) and dist.get_rank() == 0:
            print(f"MYO_DP_CHECK: {what} differs across ranks at optimizer step {self.n_updates}", flush=True)

    # ---------------------------------------------------------------- MLP policy: the fused step, captured per step and per epoch chunk
    def _build_graphs(self, B, bs):
        d = self.device
        self._gs = {"idx": torch.zeros(bs, dtype=torch.long, device=d),
                    "obs": self.obs_buf.view(B, -1), "act": self.act_buf.view(B, -1), "oldlp": self.logp_buf.view(B),
                    "adv": torch.zeros(B, device=d), "ret": torch.zeros(B, device=d),
                    "pl": torch.zeros((), device=d), "vl": torch.zeros((), device=d)}
        self._gs["idx"].copy_(torch.arange(bs, device=d))
        # One GPU: a whole EPOCH in one graph — every minibatch's index copy (from a permutation buffer filled before the replay), forward /
        # backward and optimizer step: one replay instead of B / bs, no launch gap between two minibatch steps and none around the index
        # copy (13 us + a 5 us copy kernel per 135 us step at config B).  Same kernels in the same order as the per-step graph
        # (MYO_EPOCH_GRAPH=0), so the parameters come out bit-identical (tests/test_gpu_parity.py).
        # The capture unrolls its minibatch steps, so it is CHUNKED: an SB3-style batch_size of 64 on 4096 x 64 samples is
        # 4,096 steps an epoch — one graph of that would be hundreds of thousands of nodes to capture, instantiate and hold.  A chunk
        # graph holds at most MYO_EPOCH_GRAPH_STEPS (64) steps, reads its minibatches from the first k * bs entries of a chunk-sized
        # window buffer, and is replayed ceil(n / k) times per epoch (the last, shorter chunk: the per-step graph).
        n_mb = B // bs
        self._epoch_chunk = 0
        if self.world == 1 and os.environ.get("MYO_EPOCH_GRAPH") != "0" and n_mb > 1:
            self._epoch_chunk = max(1, min(n_mb, int(os.environ.get("MYO_EPOCH_GRAPH_STEPS", "64"))))
        asked = self.world > 1 and (self.cfg.graph_allreduce or os.environ.get("MYO_GRAPH_ALLREDUCE") == "1")
        fused, hooks = self._fused, {}
        if fused.resident_adam is not None and self._epoch_chunk and not fused.external_adv_stats:
            # resident step: the advantage moments of the chunk's minibatches in two launches ahead of its steps, each step reading its
            # row, instead of one moments pass per step (the per-step graph computes its own minibatch's: _mfma_step)
            k = self._epoch_chunk
            fused.moments_buffers(k)         # (allocated here, not inside the capture)

            def epoch_begin():
                self._chunk_moments = fused.epoch_moments(self._gs["adv"], self._gs["perm"], bs, k)

            def step_begin(j):
                fused.adv_slot = None if j is None else self._chunk_moments[j]
            hooks = dict(epoch_begin=epoch_begin, step_begin=step_begin)
        self._graph_fb, self._graph_ap, self._graph_epoch, self._allreduce_in_graph = self._capture_step(
            self._mb_forward_backward, self._gs, graph_allreduce=asked, epoch_steps=self._epoch_chunk, **hooks)
        self._graph = (B, bs)

    def _train_graphed(self, adv, ret):
        cfg = self.cfg
        B = cfg.n_steps * self.env.num_envs
        bs = min(cfg.batch_size, B)
        # advantage moments of a minibatch: computed by the gather kernel (this rank's rows), or handed to it when they
        # must be the moments of the GLOBAL minibatch (sync_adv_moments, N > 1) or when advantages are not normalised
        ext = (cfg.sync_adv_moments and self.world > 1) or not cfg.normalize_advantage
        if self._fused.external_adv_stats != ext:
            self._fused.external_adv_stats = ext
            self._graph = None
        if self._graph != (B, bs):
            self._build_graphs(B, bs)
            self._hp_write()             # (the capture's warm-up steps have left their marks in the block)
        g = self._gs
        g["adv"].copy_(adv.view(B)); g["ret"].copy_(ret.view(B))
        if self._fused.resident_adam is not None:
            self._fused.refresh_images()      # (parameters may have been loaded or edited since the last update)
        if not cfg.normalize_advantage:
            self._fused.stats.copy_(torch.tensor([0.0, 1.0], device=self.device))
        self._run_captured(B, bs, g, self._graph_fb, self._graph_ap,
                           stats=self._fused.stats if ext and cfg.normalize_advantage else None,
                           epoch=None if ext else self._graph_epoch)
        self._fused.refresh_shadow()     # rollout inference reads the bf16 shadow weights
        return g["pl"], g["vl"]

    # ---------------------------------------------------------------- recurrent policy: one hipGraph per minibatch step
    def _rec_forward_backward(self):
        g = self._rg
        idx = g["idx"]
        L = self._rgraph_L
        if self._fused_rec is not None:
            state = (g["h0"], g["c0"]) if L is None else (g["h_snap"], g["c_snap"])
            pl, vl = self._fused_rec.run_sequences(self.obs_buf, self.act_buf, self.start_buf, self.logp_buf, g["adv"], g["ret"],
                                                   *state, idx, seq_len=L)
            g["pl"], g["vl"] = pl, vl             # views of the loss kernel's accumulator
            return
        self._flat_grad.zero_()
        if L is not None:
            loss, pl, vl = self._chunk_loss(idx, g["state0"], g["adv"], g["ret"])
            loss.backward()
            g["pl"].copy_(pl); g["vl"].copy_(vl)
            return
        st0 = tuple(x.index_select(1, idx) for x in g["state0"])
        sel = lambda buf: buf.index_select(1, idx)
        with self._autocast():
            v, lp, ent = self.policy.evaluate_actions(sel(self.obs_buf), sel(self.act_buf), st0, sel(self.start_buf))
        loss, pl, vl = self._loss(v.reshape(-1), lp.reshape(-1), ent, sel(self.logp_buf).reshape(-1),
                                  sel(g["adv"]).reshape(-1), sel(g["ret"]).reshape(-1))
        loss.backward()                       # p.grad are views of the flat gradient: accumulated in place
        g["pl"].copy_(pl); g["vl"].copy_(vl)

    def _build_recurrent_graphs(self, T, N, m, L=None):
        """The static tensors and the captured step for whole rollouts of m envs, or with L for m chunks of L steps: g["idx"] then
        holds m item ids, and the state inputs are the rollout's snapshots."""
        d = self.device
        state = self._rollout_state0 if L is None else self.rollout_snapshots()
        if L is not None and self._fused_rec is not None:
            state = ()                            # (the fused chunk step reads the stacked snapshots below)
        self._rg = {"idx": torch.arange(m, device=d), "state0": tuple(torch.zeros_like(x) for x in state),
                    "adv": torch.zeros((T, N), device=d), "ret": torch.zeros((T, N), device=d),
                    "pl": torch.zeros((), device=d), "vl": torch.zeros((), device=d)}
        H = self.policy.hidden
        if self._fused_rec is not None and L is None:           # stacked (actor, critic) LSTM state of the rollout start
            self._rg["h0"], self._rg["c0"] = torch.zeros((2, N, H), device=d), torch.zeros((2, N, H), device=d)
        elif self._fused_rec is not None:
            # stacked snapshots, bf16 h / float32 c [S, 2, N, H]: the collector's own storage where it keeps them so (written in
            # place, read by address), else static copies that _rec_stage fills
            self._rg["h_snap"], self._rg["c_snap"] = self._stacked_snapshots() or \
                (torch.zeros((T // L, 2, N, H), device=d, dtype=torch.bfloat16), torch.zeros((T // L, 2, N, H), device=d))
        self._rgraph_L = L
        # (BPTT over n_steps is one graph per minibatch already: no all-reduce inside the graph and no epoch-chunk graph here)
        self._rgraph_fb, self._rgraph_ap, _, _ = self._capture_step(self._rec_forward_backward, self._rg, graph_allreduce=False,
                                                                    epoch_steps=0)
        self._rgraph = (T, N, m, L)

    def _stacked_snapshots(self):
        return self._rollout.stacked_snapshots() if self._rollout is not None else None

    def _rec_stage(self, adv, ret, T, N, m, L=None):
        """Graphs for this shape (built on first use) and the update's inputs copied into their static tensors.  L: m chunks of L steps
        (seq_len) instead of m whole rollouts."""
        cfg = self.cfg
        if self._fused_rec is not None:
            ext = (cfg.sync_adv_moments and self.world > 1) or not cfg.normalize_advantage
            if self._fused_rec.external_adv_stats != ext:
                self._fused_rec.external_adv_stats = ext
                self._rgraph = None
        if self._rgraph != (T, N, m, L):
            self._build_recurrent_graphs(T, N, m, L)
            self._hp_write()             # (the capture's warm-up steps have left their marks in the block)
        g = self._rg
        g["adv"].copy_(adv); g["ret"].copy_(ret)
        fr = self._fused_rec
        state = self._rollout_state0 if L is None else self.rollout_snapshots()
        if fr is None or L is None:
            for dst, src in zip(g["state0"], state):
                dst.copy_(src)
        if fr is not None:
            fr.refresh_shadow()                   # (parameters may have been loaded since the last update)
            hp, cp, hv, cv = state
            if L is None:
                g["h0"][0].copy_(hp[0]); g["h0"][1].copy_(hv[0]); g["c0"][0].copy_(cp[0]); g["c0"][1].copy_(cv[0])
            elif self._stacked_snapshots() is None:
                g["h_snap"][:, 0:1].copy_(hp); g["h_snap"][:, 1:2].copy_(hv); g["c_snap"][:, 0:1].copy_(cp); g["c_snap"][:, 1:2].copy_(cv)
            if not cfg.normalize_advantage:
                fr.stats.copy_(torch.tensor([0.0, 1.0], device=self.device))
        return g

    def _train_recurrent_graphed(self, adv, ret):
        """Same minibatches as the eager recurrent path (whole rollouts of a random subset of envs, LSTM state of
        the rollout start; with seq_len: chunks from their snapshot states), replayed from a graph: BPTT over n_steps is thousands
        of small launches."""
        cfg = self.cfg
        T, N, L = cfg.n_steps, self.env.num_envs, cfg.seq_len
        m = max(1, min(N, cfg.batch_size // T)) if L is None else cfg.batch_size // L
        g, fr = self._rec_stage(adv, ret, T, N, m, L), self._fused_rec
        global_moments = fr is not None and fr.external_adv_stats and cfg.normalize_advantage
        adv_of = None
        if L is not None:        # the advantages of a minibatch of chunks (item c = chunk c // N of env c % N), for the cross-rank moments
            adv_of = lambda items: g["adv"].view(T // L, L, N)[torch.div(items, N, rounding_mode="floor"), :, items % N]
        self._run_captured(N if L is None else N * (T // L), m, g, self._rgraph_fb, self._rgraph_ap,
                           stats=fr.stats if global_moments else None, adv_of=adv_of)
        return g["pl"], g["vl"]

    # ---------------------------------------------------------------- persistence (SB3 zip layout)
    def _optimizer_state_dict(self) -> dict:
        """torch.optim.Adam state_dict layout (what SB3 stores in policy.optimizer.pth), parameter order of
        ``policy.parameters()`` as SB3 builds its optimiser."""
        cfg = self.cfg
        params = list(self.policy.parameters())
        state = {}
        if self._flat_adam is not None:
            fa, flat = self._flat_adam, self.policy._flat
            slot = {id(p): sl for p, sl in zip(flat["params"], flat["slots"])}
            step = float(fa.step_count)
            if step > 0:
                for i, p in enumerate(params):
                    off, k = slot[id(p)]
                    state[i] = {"step": torch.tensor(step), "exp_avg": fa.m[off:off + k].view(p.shape).cpu().clone(),
                                "exp_avg_sq": fa.v[off:off + k].view(p.shape).cpu().clone()}
        else:
            sd = self.optimizer.state_dict()
            state = {i: {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in st.items()}
                     for i, st in sd["state"].items()}
        return {"state": state, "param_groups": [{"lr": cfg.learning_rate, "betas": (0.9, 0.999), "eps": 1e-5, "weight_decay": 0,
                                                  "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                                                  "params": list(range(len(params)))}]}

    def load_optimizer_state(self, opt: Optional[dict]) -> bool:
        """Restore Adam's moments from ``policy.optimizer.pth`` of a stable-baselines3 zip (``RecurrentPPO.load`` does on
        every curriculum resume, /root/reference/src/train/trainer.py:51-56).  State i belongs to the i-th parameter in
        stable-baselines3's order, which is this policy's ``parameters()`` order.  Returns False (and changes nothing)
        when the state is empty or its shapes do not fit."""
        if not opt or not opt.get("state"):
            return False
        params = list(self.policy.parameters())
        st = opt["state"]
        if sorted(st) != list(range(len(params))) or any(tuple(st[i]["exp_avg"].shape) != tuple(p.shape) for i, p in enumerate(params)):
            return False
        step = float(st[0]["step"]) if "step" in st[0] else 0.0
        if self._flat_adam is not None:
            fa, flat = self._flat_adam, self.policy._flat
            slot = {id(p): sl for p, sl in zip(flat["params"], flat["slots"])}
            for i, p in enumerate(params):
                off, k = slot[id(p)]
                fa.m[off:off + k].copy_(st[i]["exp_avg"].reshape(-1).to(fa.m))
                fa.v[off:off + k].copy_(st[i]["exp_avg_sq"].reshape(-1).to(fa.v))
            fa.set_step_count(step)
        else:
            dev = self.device
            for i, p in enumerate(params):
                self.optimizer.state[p] = {"step": torch.tensor(step, dtype=torch.float32, device=dev if self.device.type == "cuda" else "cpu"),
                                           "exp_avg": st[i]["exp_avg"].to(p).clone(), "exp_avg_sq": st[i]["exp_avg_sq"].to(p).clone()}
        return True

    def save(self, path: str) -> None:
        """``model.save(path)`` of the reference's callbacks (src/metrics/custom_callbacks.py:59): a
        stable-baselines3-format zip (rl/sb3_zip.save_sb3_zip)."""
        from .sb3_zip import save_sb3_zip
        cfg = self.cfg
        hyper = {k: getattr(cfg, k) for k in ("n_steps", "batch_size", "n_epochs", "gamma", "gae_lambda", "ent_coef", "vf_coef",
                                              "max_grad_norm", "learning_rate", "clip_range", "normalize_advantage")}
        # schedules are pickled as constant functions of their CURRENT value, next to the progress they were evaluated at
        hyper.update(learning_rate=self._lr_now, clip_range=self._clip_now, target_kl=cfg.target_kl,
                     _current_progress_remaining=float(self._current_progress_remaining))
        last = self._last_obs.detach().cpu().numpy() if self._last_obs is not None else None
        orig = getattr(self.env, "old_obs", None)
        save_sb3_zip(path, self.policy, hyper, n_envs=self.env.num_envs, num_timesteps=self.num_timesteps, n_updates=self.n_updates,
                     last_obs=last, last_original_obs=orig.detach().cpu().numpy() if orig is not None else None,
                     last_episode_starts=self._last_starts.detach().cpu().numpy() > 0.5,
                     optimizer_state=self._optimizer_state_dict(), clip_obs=float(getattr(self.env, "clip_obs", 10.0)))

    def set_parameters(self, path: str) -> None:
        """Load policy weights from a stable-baselines3 zip (``RecurrentPPO.load`` of src/train/trainer.py:51-56)."""
        from .sb3_zip import read_zip
        _, sd, _ = read_zip(path)
        self.policy.load_state_dict(sd, strict=True)        # in place: the flat-vector views stay valid
        if self._fused is not None:
            self._fused.refresh_shadow()

    def learn(self, total_timesteps: int, callback: Optional[Callable[["PPO"], None]] = None, log=None):
        """SB3's loop: collect a rollout (callbacks see every env step of it: `callback(self)` runs at the END of the rollout, BEFORE the
        update, with `self.n_calls` = vec-env steps so far — the policy a mid-rollout `_on_step` would have seen), train, log.
        Logged: time/fps, time/total_timesteps, rollout/ep_rew_mean and rollout/ep_len_mean (last 100 finished episodes, raw returns:
        SB3's Monitor / ep_info_buffer semantics), train/*."""
        t_start = time.time()
        self._total_timesteps = total_timesteps
        while self.num_timesteps < total_timesteps:
            self.collect_rollouts()
            # SB3 1.6.2 _update_current_progress_remaining [3P-RECALL]: after the rollout, before train()
            self._current_progress_remaining = 1.0 - float(self.num_timesteps) / float(total_timesteps)
            if callback is not None:
                callback(self)
            stats = self.train()
            if log is not None and self.rank == 0:
                fps = self.num_timesteps / max(1e-9, time.time() - t_start)
                log({"time/fps": fps, "time/total_timesteps": self.num_timesteps, **self.episode_stats(),
                     **{"train/" + k: v for k, v in stats.items()}})
        return self

    @property
    def n_calls(self) -> int:
        """vec-env steps taken so far (SB3's BaseCallback.n_calls: one per env.step of the vectorised env, whatever its width)"""
        return self.num_timesteps // max(1, self.env.num_envs * self.world)
