"""BASELINE config E (die-reorient, 4096 envs on one MI355X, recurrent LSTM policy): env-steps/s of rollout + PPO update.
Not the headline bench; `bench.py --full` records it as `variants.config_E_lstm256`, `tools/bench_reorient.py` prints it.  The env step is
the step kernel's MYO_TASK_REORIENT task (csrc/myo_task.h); the LSTM policy (/root/reference/src/main_reorient.py:53-71: LSTM-256
actor + critic -> [256, 256] ReLU, log_std_init -2) rolls out and trains on the HIP-kernel recurrent path."""
import time


def run(envs: int = 4096, n_steps: int = 32, iters: int = 3, env_only_steps: int = 50, dtype: str = "f64", n_epochs: int = 4,
        reference_settings: bool = False, seq_len=None) -> dict:
    """reference_settings: the PPO settings of /root/reference/src/main_reorient.py:53-71 — n_steps 128, n_epochs 10, learning rate
    2.55673e-5, entropy 3.62109e-6, clip 0.3, lambda 0.9, max_grad_norm 0.7, vf_coef 0.835671, 300-step episodes — on the fp64 stepper
    (the reference's arithmetic).  Its batch_size = 32 belongs to its 16 envs (a rollout of 2,048 samples = 64 minibatches); at 4096 envs
    the minibatch stays an eighth of the rollout's sequences, as in the light setting.
    seq_len: PPOConfig.seq_len — the minibatch, still an eighth of the rollout's transitions, is then made of chunks of seq_len steps
    started from the rollout's stored LSTM states (the reference's truncated BPTT: seq_len = 32) instead of whole rollouts."""
    import torch
    from ..envs.environment_factory import EnvironmentFactory
    from .policy import ActorCriticPolicy
    from .ppo import PPO, PPOConfig
    from .vec_normalize import VecNormalize
    if reference_settings:
        n_steps, n_epochs, dtype = 128, 10, "f64"
    env = EnvironmentFactory.create("CustomMyoReorientP1", num_envs=envs, seed=1, dtype=dtype, **({"max_episode_steps": 300} if reference_settings else {}))
    torch.manual_seed(0)
    pol = ActorCriticPolicy(env.obs_dim, env.act_dim, (256, 256), (256, 256), lstm_hidden_size=256, log_std_init=-2.0)
    cfg = PPOConfig(n_steps=n_steps, batch_size=envs * n_steps // 8, n_epochs=n_epochs, learning_rate=2.5e-5, seq_len=seq_len)
    if reference_settings:
        cfg = PPOConfig(n_steps=128, batch_size=envs * 128 // 8, n_epochs=10, learning_rate=2.55673e-05, ent_coef=3.62109e-06, clip_range=0.3,
                        gamma=0.99, gae_lambda=0.9, max_grad_norm=0.7, vf_coef=0.835671, seq_len=seq_len)
    algo = PPO(VecNormalize(env), pol, cfg)
    algo.collect_rollouts(); algo.train()                       # warm-up (captures the graphs)
    if reference_settings:
        # ... and on past the first time the 300-step limit truncates every env: that rollout's bootstrap GEMMs meet shapes the BLAS
        # library has not seen (+0.05-0.2 s, once per process) — a training run amortises it, a few timed iterations would not
        for _ in range(300 // n_steps + 1):
            algo.collect_rollouts(); algo.train()
    torch.cuda.synchronize()
    t0 = time.time(); tr = 0.0; per_iter = []
    for _ in range(iters):
        t1 = time.time(); algo.collect_rollouts(); torch.cuda.synchronize(); t2 = time.time(); tr += t2 - t1
        algo.train(); torch.cuda.synchronize()
        per_iter.append([round(t2 - t1, 4), round(time.time() - t2, 4)])
    dt = time.time() - t0
    steps = iters * envs * n_steps
    out = {"config": "E: CustomMyoReorientP1, %d envs, LSTM-256 + MLP[256,256]" % envs,
           "env_steps_per_sec_rollout_plus_update": steps / dt, "env_steps_per_sec_rollout_only": steps / tr,
           "n_steps": n_steps, "epochs": n_epochs, "seq_len": seq_len, "dtype": dtype, "settings": "reference (src/main_reorient.py:53-71)" if reference_settings else "light",
           "env_kernel_lds_bytes": env.batch.lds_bytes, "health": env.batch.health(), "recurrent_path": "fused" if algo._fused_rec is not None else "autograd",
           "seconds_per_iteration_rollout_update": per_iter,
           # (the iteration in which the 300-step time limit first truncates every env runs its bootstrap GEMMs on shapes the BLAS library has
           #  not seen yet — a one-off of 0.05-0.2 s that a run of a few iterations does not amortise: the median iteration beside the total)
           "env_steps_per_sec_median_iteration": envs * n_steps / sorted(a + b for a, b in per_iter)[len(per_iter) // 2]}
    if env_only_steps:                                          # physics alone (zero actions)
        act = torch.zeros((envs, env.act_dim), device=env.device)
        t2 = time.time()
        for _ in range(env_only_steps):
            env.step_tensor(act)
        torch.cuda.synchronize()
        out["env_steps_per_sec_env_only"] = env_only_steps * envs / (time.time() - t2)
    env.close()
    return out
