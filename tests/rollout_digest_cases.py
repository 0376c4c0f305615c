"""Seeded PPO runs (collect_rollouts, train, collect_rollouts) on every rollout path, reduced to SHA-256 digests: what
tools/rollout_digests.py prints and tests/test_rollout_digests.py compares with tests/golden/rollout_digests.json.  The golden file
was printed by that tool on an MI355X from the commit BEFORE the rollout collectors moved into rl/rollout.py; this file uses only
what exists on both sides of that move, so it ran on that commit unchanged.  A build that keeps every buffer, graph, launch, launch
order and random draw of the rollout reproduces the digests bit for bit.

Shapes: Baoding with a 5-step TimeLimit (truncations, and with them the timeout bootstrap, in every rollout), 160 envs (two 128-row
VecNormalize blocks, the second short), rollouts of 12 steps (three seq_len chunks, two whole episodes) or 32 steps where the fused
MLP update needs minibatches of 1024."""
import hashlib
import os

import torch

BUFFERS = ("obs_buf", "act_buf", "rew_buf", "val_buf", "logp_buf", "start_buf")
ENV, N, HORIZON = "CustomMyoBaodingBallsP1", 160, 5
MLP = dict(arch=(256, 256), n_steps=32, batch_size=1024)
REC = dict(arch=(64, 64), n_steps=12, batch_size=12 * 32, bf16=True)
# name -> (policy / PPO options, wrap in VecNormalize, environment variables, rollout path, what else must hold of the PPO object)
CASES = {
    "A-mlp-one-launch": (dict(MLP), True, {}, "KernelRollout", lambda a: getattr(a._fused, "_rollout", None) is not None),
    "B-mlp-gemm": (dict(MLP), True, {"MYO_ROLLOUT_GEMM": "1"}, "KernelRollout", lambda a: getattr(a._fused, "_rollout", None) is None),
    "C-gsde": (dict(MLP, arch=(64, 64), use_sde=True), True, {}, "KernelRollout", lambda a: a._fused.merged is not None),
    "D-lstm128": (dict(REC, hidden=128), True, {}, "KernelRollout", lambda a: a._fused_rec.step_kernels),
    "E-lstm32-seq4": (dict(REC, hidden=32, seq_len=4, batch_size=4 * 96), True, {}, "KernelRollout", lambda a: a._fused_rec.step_kernels),
    "F-lstm128-two-kernels": (dict(REC, hidden=128), True, {"MYO_LSTM_TWO_KERNELS": "1"}, "KernelRollout",
                              lambda a: not a._fused_rec.step_kernels),
    "G-mlp-bare-env": (dict(MLP), False, {}, "GraphRollout", lambda a: a._fused is not None),
    "H-lstm32-seq4-bare-env": (dict(REC, hidden=32, seq_len=4, batch_size=4 * 96), False, {}, "GraphRollout", lambda a: True),
    "I-mlp-eager": (dict(MLP, n_steps=12, batch_size=960, use_graphs=False), True, {}, "EagerRollout", lambda a: a._fused is None),
}


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def rollout_path(algo) -> str:
    """Which rollout ran: the collector's class name, or what the flags of the single-class PPO said before there were collectors."""
    if hasattr(algo, "_rollout"):
        return type(algo._rollout).__name__
    if not algo._rollout_ready:
        return "EagerRollout"
    return "KernelRollout" if algo._native else "GraphRollout"


def rollout_group(algo) -> dict:
    """Digests of everything a finished rollout leaves behind."""
    t = {name: getattr(algo, name) for name in BUFFERS}
    t.update(last_obs=algo._last_obs, last_starts=algo._last_starts, last_values=algo._last_values)
    if algo._rollout_state0 is not None:
        t.update({"state0.%d" % k: x for k, x in enumerate(algo._rollout_state0)})
    snaps = algo.rollout_snapshots()
    if snaps is not None:
        t.update({"snapshots.%d" % k: x for k, x in enumerate(snaps)})
    if hasattr(algo.env, "obs_rms"):
        t.update(obs_rms=algo.env.obs_rms.buf, ret_rms=algo.env.ret_rms.buf, returns=algo.env.returns)
    torch.cuda.synchronize()
    d = {k: sha(v) for k, v in t.items()}
    d["episode_stats"] = hashlib.sha256(repr(sorted(algo.episode_stats().items())).encode()).hexdigest()
    return d


def run_case(name) -> dict:
    """{"rollout1": {...}, "after_train": {...}, "rollout2": {...}} of one case."""
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    from myochallenge_amd.rl.ppo import PPO, PPOConfig
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    opts, wrap, environ, path, holds = CASES[name]
    opts = dict(opts)
    arch, hidden, use_sde = opts.pop("arch"), opts.pop("hidden", None), opts.pop("use_sde", False)
    old = {k: os.environ.get(k) for k in environ}
    os.environ.update(environ)
    try:
        torch.manual_seed(0)
        env = EnvironmentFactory.create(ENV, num_envs=N, seed=11, max_episode_steps=HORIZON)
        pol = ActorCriticPolicy(env.obs_dim, env.act_dim, arch, arch, lstm_hidden_size=hidden, use_sde=use_sde)
        algo = PPO(VecNormalize(env) if wrap else env, pol, PPOConfig(n_epochs=1, **opts), seed=0)
        out = {}
        algo.collect_rollouts()
        assert rollout_path(algo) == path and holds(algo), (name, rollout_path(algo))
        out["rollout1"] = rollout_group(algo)
        assert float(algo.start_buf[1:].sum()) > 0, "no episode ended inside the rollout"
        algo.train()
        torch.cuda.synchronize()
        flat = torch.cat([p.detach().reshape(-1) for p in pol.parameters()])
        out["after_train"] = {"parameters": sha(flat), "n_updates": int(algo.n_updates)}
        algo.collect_rollouts()
        out["rollout2"] = rollout_group(algo)
        env.close()
        return out
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def rollout_digests(names=None) -> dict:
    return {name: run_case(name) for name in (names or CASES)}
