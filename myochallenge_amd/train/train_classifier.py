"""Collect classifier trials with a trained policy and train the task classifier — /root/reference/src/train/train_classifier.py.

The reference script runs ``collect_data_for_classifier(model, env, save_path, n_episodes)`` and then
``train_task_classifier(data_path=save_path)``; here both take their paths from the command line and the
collection runs ``--num-envs`` trials at a time on the GPU:

    python -m myochallenge_amd.train.train_classifier best_model.zip training_env.pkl output/classifier --episodes 10000

writes ``<out>/data_for_task_classifier.csv``, ``<out>/task_classifier.pt`` and ``<out>/scaler.pkl`` — the classifier and
scaler that ``eval_mixture_of_ensembles.SuperModel.load`` reads.
"""
from __future__ import annotations

import argparse
import os
import time

from ..models.classifier import collect_data_for_classifier, train_task_classifier

CSV_NAME = "data_for_task_classifier.csv"


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model_path", help="recurrent policy (stable-baselines3 zip) that plays the trials")
    ap.add_argument("env_path", help="its VecNormalize pickle")
    ap.add_argument("output_dir")
    ap.add_argument("--episodes", type=int, default=10_000, help="trials to collect (reference: 10,000)")
    ap.add_argument("--num-envs", type=int, default=4096, help="trials run together on the device")
    ap.add_argument("--seed", type=int, default=0, help="env draws, exploration noise, weight init and batch order")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    os.makedirs(a.output_dir, exist_ok=True)
    save_path = os.path.join(a.output_dir, CSV_NAME)
    t0 = time.time()
    collect_data_for_classifier(a.model_path, a.env_path, save_path, n_episodes=a.episodes, num_envs=a.num_envs, seed=a.seed,
                                device=a.device)
    t1 = time.time()
    res = train_task_classifier(data_path=save_path, save_folder=a.output_dir, seed=a.seed, device=f"cuda:{a.device}")
    print(f"collection + CSV {t1 - t0:.2f} s, training {time.time() - t1:.2f} s")
    return res


if __name__ == "__main__":
    main()
