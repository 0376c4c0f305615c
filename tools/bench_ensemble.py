#!/usr/bin/env python
"""Time one SuperModel.predict of the mixture of ensembles, member loop against the fused step.

The workload is the reference's shape (trained_models/winning_ensemble): 6 base + 5 hold members, LSTM-128 with an empty trunk,
O = 86, A = 39, with seeded random weights, statistics and observations, at N = 256 and N = 4096.  Both SuperModels live in one
process and are timed alternately, block by block, after a warm-up of each; every block of `--steps` predict calls is timed
between two device synchronisations (host clock), and the per-call time is the median over the blocks.  Needs a GPU.

    python tools/bench_ensemble.py [--steps 50] [--blocks 9] [--sde] [--out profiles/ensemble_act.json]

--sde builds the members as the reference trains them (use_sde=True, log_std_init=-2: deterministic acting does not read log_std,
so the launch is the same); the default run and profiles/ensemble_act.json are the Gaussian members.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--sde", action="store_true", help="gSDE members (use_sde=True, log_std_init=-2), as the reference's")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_act.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_ensemble: needs a GPU", file=sys.stderr)
        return 1
    from myochallenge_amd import native
    from myochallenge_amd.eval_mixture_of_ensembles import SuperModel
    from myochallenge_amd.models.classifier import TaskClassifier
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    import types
    dev = torch.device("cuda:0")
    O, A, H, M0, M1 = 86, 39, 128, 6, 5
    results = []
    for N in args.envs:
        torch.manual_seed(1)
        kind = dict(use_sde=True, log_std_init=-2.0) if args.sde else {}
        pols = [ActorCriticPolicy(O, A, (), (), lstm_hidden_size=H, **kind) for _ in range(M0 + M1)]
        clf = TaskClassifier()
        venv = types.SimpleNamespace(num_envs=N, device=dev, obs_dim=O, act_dim=A, observation_space=None, action_space=None)

        def norms():
            out = []
            g = torch.Generator().manual_seed(2)
            for _ in range(M0 + M1):
                vn = VecNormalize(venv, training=False, norm_reward=False)
                vn.obs_rms.mean.copy_(0.5 * torch.randn(O, generator=g, dtype=torch.float64))
                vn.obs_rms.var.copy_((0.25 + torch.rand(O, generator=g, dtype=torch.float64)) ** 2)
                out.append(vn)
            return out
        scaler = (torch.zeros(234, dtype=torch.float64).numpy(), torch.ones(234, dtype=torch.float64).numpy())
        models = {}
        for name, fused in (("loop", False), ("fused", True)):
            nr = norms()
            models[name] = SuperModel(pols[:M0], nr[:M0], pols[M0:], nr[M0:], clf, scaler, N, dev, fused=fused)
        if models["fused"].fused is None:
            print("bench_ensemble: the fused step does not apply here", file=sys.stderr)
            return 1
        g = torch.Generator().manual_seed(3)
        obs = [torch.randn(N, O, generator=g).to(dev) for _ in range(8)]
        starts = [(torch.rand(N, generator=g) < 0.02).float().to(dev) for _ in range(8)]

        def block(call, k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(k):
                call(obs[i % 8], starts[i % 8])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / k
        fe, use = models["fused"].fused, models["fused"].use_hold_net
        calls = {"loop": models["loop"].predict, "fused": models["fused"].predict,
                 "kernel": lambda o, s: fe.act(o, s, s, use)}          # the launch alone, without the state machine and the classifier
        for call in calls.values():
            block(call, args.warmup)
        times = {k: [] for k in calls}
        for _ in range(args.blocks):
            for name, call in calls.items():
                times[name].append(block(call, args.steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {"num_envs": N, "members": [M0, M1], **({"use_sde": True} if args.sde else {}), "obs_dim": O, "act_dim": A, "hidden": H, "steps_per_block": args.steps, "blocks": args.blocks,
               "loop_us": med["loop"] * 1e6, "fused_us": med["fused"] * 1e6, "loop_over_fused": med["loop"] / med["fused"],
               "fused_launch_alone_us": med["kernel"] * 1e6,
               "loop_us_min_max": [min(times["loop"]) * 1e6, max(times["loop"]) * 1e6],
               "fused_us_min_max": [min(times["fused"]) * 1e6, max(times["fused"]) * 1e6]}
        results.append(rec)
        print(json.dumps(rec))
    doc = {"what": "SuperModel.predict, member loop (fused=False) vs fused step (fused=True), host time per call around device syncs",
           "device": torch.cuda.get_device_name(0), "build": native.load().build_id, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
