"""Train the HOLD policy of the mixture of ensembles — /root/reference/src/train/train_mixture_model.py.

The learner plays ``MixtureModelBaodingEnv``: every episode starts after the frozen *base* policy (the CW / CCW
policy the task classifier is trained with) has acted for its first 20 steps, and the goal never moves
(``goal_time_period`` 1e100), so the learner is taught to hold the balls the base policy handed over.  It starts
from a recurrent zip + VecNormalize pickle with the reference's overrides (lr 3e-5, clip 0.2, n_steps 4096, batch
4096, ent_coef 0, n_epochs 10) and is scored by the reference's callbacks: ``EvaluateLSTM`` on the solved-only
reward, ``EvalCallback`` saving the best model with ``EnvDumpCallback`` (the reference imports it from a module
that is not in its tree), and ``CheckpointCallback``.  The reference's 16 workers x n_steps 4096 = 65,536 samples
per update are kept by default: ``--n-steps`` = 65,536 // ``--num-envs``.

    python -m myochallenge_amd.train.train_mixture_model base.zip base_env.pkl hold.zip hold_env.pkl --num-envs 4096

The result (``<log-dir>/final_model.pkl`` + ``final_env.pkl``) is a hold member for ``eval_mixture_of_ensembles``.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
from datetime import datetime

ENV_NAME = "MixtureModelBaodingEnv"

# reward structure and task parameters (src/train/train_mixture_model.py:37-72)
config = {
    "weighted_reward_keys": {"pos_dist_1": 5, "pos_dist_2": 5, "act_reg": 0, "alive": 0, "solved": 5, "done": 0, "sparse": 0},
    "enable_rsi": False, "rsi_probability": 0, "balls_overlap": False, "overlap_probability": 0, "noise_fingers": 0,
    "goal_time_period": [4, 6], "goal_xrange": (0.020, 0.030), "goal_yrange": (0.022, 0.032),
    "obj_size_range": (0.018, 0.024), "obj_mass_range": (0.030, 0.300), "obj_friction_change": (0.2, 0.001, 0.00002),
    "task_choice": "random",
}

# the reference's custom_objects of RecurrentPPO.load (:185-194)
MODEL_CONFIG = {"lr_schedule": lambda _: 3e-5, "learning_rate": lambda _: 3e-5, "clip_range": 0.2, "n_steps": 4096,
                "batch_size": 4096, "ent_coef": 0.0, "n_epochs": 10}
REFERENCE_ROLLOUT = 16 * 4096           # 16 SubprocVecEnv workers x n_steps


def hold_config(base_model_path: str, base_env_path: str) -> dict:
    """config_hold (:75-84): the goal stands still; the base policy plays the first steps of every episode."""
    cfg = copy.deepcopy(config)
    cfg.update({"goal_time_period": [1e100, 1e100], "base_model_path": base_model_path, "base_env_path": base_env_path,
                "base_env_name": "CustomMyoBaodingBallsP2", "base_env_config": copy.deepcopy(config)})
    return cfg


def score_and_effort_configs(cfg: dict):
    """config_score / config_effort (:112-147): solved-only and effort-only rewards on the final noise distribution."""
    final = {"noise_fingers": 0, "limit_init_angle": False, "beta_init_angle": False, "beta_ball_size": False, "beta_ball_mass": False}
    zero = {"pos_dist_1": 0, "pos_dist_2": 0, "alive": 0, "done": 0, "sparse": 0}
    score, effort = copy.deepcopy(cfg), copy.deepcopy(cfg)
    score.update(final, weighted_reward_keys={**zero, "act_reg": 0, "solved": 5})
    effort.update(final, weighted_reward_keys={**zero, "act_reg": 1, "solved": 0})
    return score, effort


def make_parallel_envs(env_config, num_env, start_index=0, env_name=ENV_NAME, **batch_kw):
    """(:88-98) SubprocVecEnv of Monitor-wrapped envs there; one batched env here."""
    from ..envs.environment_factory import EnvironmentFactory
    return EnvironmentFactory.create(env_name, num_envs=num_env, seed=start_index, **batch_kw, **env_config)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("base_model_path", help="PATH_TO_BASE_NET: the CW + CCW policy (zip) that hands over every episode")
    ap.add_argument("base_env_path", help="PATH_TO_NORMALIZED_BASE_ENV: its VecNormalize pickle")
    ap.add_argument("hold_model_path", help="PATH_TO_HOLD_NET: the recurrent policy (zip) training starts from")
    ap.add_argument("hold_env_path", help="PATH_TO_NORMALIZED_HOLD_ENV: its VecNormalize pickle")
    ap.add_argument("--log-dir", default=None)
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--timesteps", type=int, default=20_000_000)
    ap.add_argument("--n-steps", type=int, default=None, help=f"default: {REFERENCE_ROLLOUT} // num_envs (the reference's samples per update)")
    ap.add_argument("--batch-size", type=int, default=MODEL_CONFIG["batch_size"])
    ap.add_argument("--eval-freq", type=int, default=20_000 * 16, help="env TIMESTEPS between EvalCallback runs (reference: 20,000 vec-env steps x 16)")
    ap.add_argument("--score-freq", type=int, default=1_200_000, help="env TIMESTEPS between EvaluateLSTM scores")
    ap.add_argument("--save-freq", type=int, default=10_000 * 16, help="env TIMESTEPS between checkpoints (reference: 10,000 vec-env steps x 16)")
    ap.add_argument("--n-eval-episodes", type=int, default=5)
    ap.add_argument("--score-episodes", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    from ..metrics import CheckpointCallback, EnvDumpCallback, EvalCallback, EvaluateLSTM
    from ..rl.vec_normalize import VecNormalize
    from .trainer import MyoTrainer
    log_dir = a.log_dir or os.path.join("output", "training", datetime.now().strftime("%Y-%m-%d/%H-%M-%S") + "_mixture-hold")
    os.makedirs(log_dir, exist_ok=True)
    cfg = hold_config(a.base_model_path, a.base_env_path)
    with open(os.path.join(log_dir, "config.json"), "w", encoding="utf8") as fh:
        json.dump(cfg, fh)
    envs = VecNormalize.load(a.hold_env_path, make_parallel_envs(cfg, a.num_envs, start_index=a.seed))
    config_score, _config_effort = score_and_effort_configs(cfg)
    n_eval = min(256, a.num_envs)
    score_env = make_parallel_envs(config_score, n_eval, start_index=a.seed + 12345)
    score_callback = EvaluateLSTM(eval_freq=a.score_freq, eval_env=score_env, name="eval/score", num_episodes=a.score_episodes)
    eval_envs = VecNormalize.load(a.hold_env_path, make_parallel_envs(config_score, n_eval, start_index=a.seed + 23456))
    eval_callback = EvalCallback(eval_envs, callback_on_new_best=EnvDumpCallback(log_dir, verbose=0), best_model_save_path=log_dir,
                                 log_path=log_dir, eval_freq=max(1, a.eval_freq // a.num_envs), deterministic=True, render=False,
                                 n_eval_episodes=a.n_eval_episodes)
    checkpoint_callback = CheckpointCallback(save_freq=max(1, a.save_freq // a.num_envs), save_path=log_dir, save_vecnormalize=True)
    model_config = dict(MODEL_CONFIG, n_steps=a.n_steps or max(1, REFERENCE_ROLLOUT // a.num_envs), batch_size=a.batch_size, seed=a.seed)
    trainer = MyoTrainer(envs=envs, env_config=cfg,
                         load_model_path=a.hold_model_path, log_dir=log_dir, model_config=model_config,
                         callbacks=[eval_callback, score_callback, checkpoint_callback], timesteps=a.timesteps)
    trainer.train(total_timesteps=trainer.timesteps)
    trainer.save()
    for e in (score_env, eval_envs):
        e.close()
    return log_dir


if __name__ == "__main__":
    main()
