"""Training entry point — the batched counterpart of /root/reference/src/main_pose_hand.py (MyoHand joint pose).

Same flow as main_baoding: env config dict -> ONE batched GPU env (16 SubprocVecEnv workers there) -> ``VecNormalize`` ->
``EvalCallback`` + ``CheckpointCallback`` -> ``MyoTrainer`` (PPO, MLP actor-critic [256, 256] per net) -> ``train`` -> ``save``.

    python -m myochallenge_amd.main_pose_hand --num-envs 4096 --timesteps 10000000
"""
from __future__ import annotations

import argparse
import json
import os
from datetime import datetime

import torch.nn as nn

ENV_NAME = "CustomMyoHandPoseRandom"

# reward structure and task parameters of the reference script (src/main_pose_hand.py:24-40)
config = {
    "weighted_reward_keys": {"pose": 1, "bonus": 0, "penalty": 1, "act_reg": 0, "solved": 1, "done": 0, "sparse": 0},
    "reset_type": "sds",
    "sds_distance": 0,
    "weight_bodyname": None,
    "weight_range": None,
}

# PPO hyper-parameters of the reference script (src/main_pose_hand.py:44-61); batch size and rollout length are per batch here
model_config = dict(
    policy="MlpPolicy",
    learning_rate=2.55673e-05, ent_coef=3.62109e-06, clip_range=0.3, gamma=0.99, gae_lambda=0.9, max_grad_norm=0.7,
    vf_coef=0.835671, n_epochs=10,
    policy_kwargs=dict(log_std_init=-2.0, activation_fn=nn.ReLU, net_arch=[dict(pi=[256, 256], vf=[256, 256])]),
)


def make_parallel_envs(env_config, num_env, start_index=0, env_name=ENV_NAME, **batch_kw):
    """src/main_pose_hand.py:64-74 returns SubprocVecEnv([thunk] * num_env) with TimeLimit(100); here: one batched env."""
    from .envs.environment_factory import EnvironmentFactory
    return EnvironmentFactory.create(env_name, num_envs=num_env, seed=start_index, **batch_kw, **env_config)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--env-name", default=ENV_NAME)
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--timesteps", type=int, default=10_000_000)
    ap.add_argument("--log-dir", default=None)
    ap.add_argument("--load-model", default=None, help="PATH_TO_PRETRAINED_NET (stable-baselines3 zip)")
    ap.add_argument("--load-env", default=None, help="PATH_TO_NORMALIZED_ENV (VecNormalize pickle)")
    ap.add_argument("--config", default=None, help="JSON file with the env kwargs (default: the reference script's)")
    ap.add_argument("--dtype", default="f64", choices=["f64", "mixed"], help="stepper arithmetic")
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--batch-size", type=int, default=16384)
    ap.add_argument("--n-epochs", type=int, default=model_config["n_epochs"])
    ap.add_argument("--eval-freq", type=int, default=2_000_000, help="env TIMESTEPS between evaluations (the callback gets this // num_envs)")
    ap.add_argument("--save-freq", type=int, default=10_000_000, help="env TIMESTEPS between checkpoints (the callback gets this // num_envs)")
    a = ap.parse_args(argv)
    from .metrics import CheckpointCallback, EnvDumpCallback, EvalCallback
    from .rl.vec_normalize import VecNormalize
    from .train.trainer import MyoTrainer
    cfg = json.load(open(a.config)) if a.config else config
    log_dir = a.log_dir or os.path.join("output", "training", datetime.now().strftime("%Y-%m-%d/%H-%M-%S") + "_hand_pose_random_static")
    os.makedirs(log_dir, exist_ok=True)
    envs = make_parallel_envs(cfg, a.num_envs, env_name=a.env_name, dtype=a.dtype)
    envs = VecNormalize.load(a.load_env, envs) if a.load_env else VecNormalize(envs)
    eval_env = make_parallel_envs(cfg, min(256, a.num_envs), start_index=12345, env_name=a.env_name, dtype=a.dtype)
    eval_env = VecNormalize.load(a.load_env, eval_env) if a.load_env else VecNormalize(eval_env)
    eval_callback = EvalCallback(eval_env=eval_env, callback_on_new_best=EnvDumpCallback(log_dir, verbose=0), n_eval_episodes=10,
                                 best_model_save_path=log_dir, log_path=log_dir, eval_freq=max(1, a.eval_freq // a.num_envs), deterministic=True, verbose=1)
    checkpoint_callback = CheckpointCallback(save_freq=max(1, a.save_freq // a.num_envs), save_path=log_dir, save_vecnormalize=True, verbose=1)
    mc = dict(model_config, n_steps=a.n_steps, batch_size=a.batch_size, n_epochs=a.n_epochs)
    trainer = MyoTrainer(envs=envs, env_config=cfg, load_model_path=a.load_model, log_dir=log_dir, model_config=mc,
                         callbacks=[eval_callback, checkpoint_callback], timesteps=a.timesteps)
    trainer.train(total_timesteps=trainer.timesteps)
    trainer.save()


if __name__ == "__main__":
    main()
