#!/usr/bin/env python
"""Time the PPO update (PPO.train alone) of three gSDE policies at 4096 envs, through the public Python API only.

  (a) mlp256x2        MLP[256,256], n_steps 32, batch 16384, 4 epochs (32 minibatch steps): the shape of tools/dev/sde_time.py
  (b) lstm256_mlp256  LSTM-256 + [256,256], seq_len 32: the reference's architecture (n_steps 64, batch 65536, 2 epochs: 8 steps)
  (c) lstm128_bare    LSTM-128 with empty trunks, seq_len 32: the winning ensemble's member (same rollout and batch)

all with use_sde=True, log_std_init=-2 on CustomMyoBaodingBallsP1 (mixed stepper: the rollout is not what is timed).  Per policy:
one warm-up round (rollout + update, which also captures the graphs), then `--blocks` rounds whose train() call is timed between
two device synchronisations (host clock); the record is the median over the blocks with their min / max.  Needs a GPU.

    python tools/bench_gsde.py [--blocks 5] [--root OTHER_CHECKOUT] [--label NAME] [--out FILE]
    python tools/bench_gsde.py --combine this=a.json,b.json,c.json parent=d.json,e.json,f.json --out profiles/gsde_update.json

--root puts another checkout first on sys.path, so the same file times another commit (its parent, say) in the same job; --combine
merges alternating runs of two trees into one record: per policy and tree the median of the runs' medians and their spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POLICIES = [
    ("mlp256x2", dict(pi=(256, 256), lstm=None), dict(n_steps=32, batch_size=16384, n_epochs=4)),
    ("lstm256_mlp256", dict(pi=(256, 256), lstm=256), dict(n_steps=64, batch_size=65536, n_epochs=2, seq_len=32)),
    ("lstm128_bare", dict(pi=(), lstm=128), dict(n_steps=64, batch_size=65536, n_epochs=2, seq_len=32)),
]


def combine(groups, out):
    doc = {"what": "PPO.train() seconds per update, gSDE policies at 4096 envs: alternating runs of tools/bench_gsde.py in one job; "
                   "per tree the median of the runs' medians, their min / max, and per minibatch step",
           "trees": {}}
    for spec in groups:
        name, files = spec.split("=", 1)
        runs = [json.load(open(f)) for f in files.split(",")]
        tree = {"build": runs[0]["build"], "device": runs[0]["device"], "runs": len(runs), "policies": {}}
        for pol, _, _ in POLICIES:
            recs = [r for run in runs for r in run["results"] if r["policy"] == pol]
            meds = [r["update_s"] for r in recs]
            tree["policies"][pol] = {"update_s": statistics.median(meds), "update_s_runs": meds,
                                     "update_s_min_max": [min(r["update_s_min_max"][0] for r in recs), max(r["update_s_min_max"][1] for r in recs)],
                                     "minibatch_steps": recs[0]["minibatch_steps"],
                                     "ms_per_minibatch_step": statistics.median(meds) * 1e3 / recs[0]["minibatch_steps"],
                                     "sde_loss_env": recs[0].get("sde_loss_env")}
        doc["trees"][name] = tree
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--only", nargs="+", default=None, help="policy names to time (default: all three)")
    ap.add_argument("--root", default=ROOT, help="the checkout to import myochallenge_amd from")
    ap.add_argument("--label", default=None)
    ap.add_argument("--combine", nargs="+", default=None, metavar="NAME=FILE,FILE,...")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gsde_update.json"))
    args = ap.parse_args()
    if args.combine:
        return combine(args.combine, args.out)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        print("bench_gsde: needs a GPU", file=sys.stderr)
        return 1
    import myochallenge_amd
    from myochallenge_amd import native
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    from myochallenge_amd.rl.ppo import PPO, PPOConfig
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    assert os.path.abspath(os.path.dirname(os.path.dirname(myochallenge_amd.__file__))) == os.path.abspath(args.root), myochallenge_amd.__file__
    results = []
    for name, arch, cfg in POLICIES:
        if args.only and name not in args.only:
            continue
        env = EnvironmentFactory.create("CustomMyoBaodingBallsP1", num_envs=args.envs, seed=1, dtype="mixed")
        torch.manual_seed(0)
        pol = ActorCriticPolicy(env.obs_dim, env.act_dim, arch["pi"], arch["pi"], lstm_hidden_size=arch["lstm"], use_sde=True, log_std_init=-2.0)
        algo = PPO(VecNormalize(env), pol, PPOConfig(use_graphs=True, **cfg))
        algo.collect_rollouts()
        algo.train()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.blocks):
            algo.collect_rollouts()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = algo.train()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        steps = cfg["n_epochs"] * (args.envs * cfg["n_steps"] // cfg["batch_size"])
        rec = {"policy": name, "num_envs": args.envs, **{k: v for k, v in cfg.items()}, "minibatch_steps": steps, "blocks": args.blocks,
               "update_s": statistics.median(times), "update_s_min_max": [min(times), max(times)],
               "ms_per_minibatch_step": statistics.median(times) * 1e3 / steps,
               "sde_loss_env": os.environ.get("MYO_SDE_LOSS"),
               "policy_loss": stats["policy_loss"], "approx_kl": stats["approx_kl"]}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        env.close()
        del algo, pol, env
        torch.cuda.empty_cache()
    doc = {"what": "PPO.train() seconds per update (host time around device syncs, median over blocks), gSDE policies",
           "label": args.label, "device": torch.cuda.get_device_name(0), "build": native.load().build_id, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
