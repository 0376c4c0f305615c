#!/usr/bin/env python
"""Time one static-optimisation call (myo_batch_static_opt) next to one inverse-dynamics call on the same states.

The workload: 4096 Baoding-hand envs (CustomMyoBaodingBallsP1; nu 39, nv 35) after `--env-steps` env steps of seeded random actions,
fp64 and mixed steppers.  The target of the solve is the inverse dynamics of the states' own acceleration — what
`env.static_optimization(qacc=env.data(["qacc"])["qacc"])` passes.  Both calls go through the batch's C ABI binding with
preallocated outputs, in one process, and are timed alternately, block by block, after a warm-up of each; every block of `--steps`
calls is timed between two device synchronisations (host clock), and the per-call time is the median over the blocks.
`inverse()` is the yardstick for "one extra pass": it runs the same position and velocity stages plus the constraint set, no solver.
No threshold is set.  Needs a GPU.

    python tools/bench_static_opt.py [--envs 4096] [--steps 20] [--blocks 7] [--out profiles/static_opt.json]
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
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--env-steps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtypes", nargs="+", default=["f64", "mixed"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_opt.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("bench_static_opt: needs a GPU", file=sys.stderr)
        return 1
    from myochallenge_amd import native
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    results = []
    for dtype in args.dtypes:
        env = EnvironmentFactory.create("CustomMyoBaodingBallsP1", num_envs=args.envs, seed=1, dtype=dtype)
        env.reset()
        rng = np.random.RandomState(1)
        for _ in range(args.env_steps):
            env.step(np.clip(rng.normal(0, 0.5, (args.envs, env.act_dim)), -1, 1).astype(np.float32))
        n, nv, nu, dev = env.num_envs, env._model.size("nv"), env.act_dim, env.device
        qacc = env.data(["qacc"])["qacc"]
        f64 = lambda *shape: torch.empty((n,) + shape, dtype=torch.float64, device=dev)
        i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)
        inv = {"qfrc_inverse": f64(nv), "qfrc_constraint": f64(nv)}
        out = {"u": f64(nu), "force": f64(nu), "qfrc": f64(nv), "residual": f64(nv), "gain": f64(nu), "bias": f64(nu), "kkt": f64(),
               "iters": i32(), "status": i32()}
        gb = {"gain": out["gain"], "bias": out["bias"]}
        calls = {"inverse": lambda: env.batch.inverse(qacc, inv["qfrc_inverse"], inv["qfrc_constraint"], env._stream()),
                 "static_opt": lambda: env.batch.static_opt(inv["qfrc_inverse"], stream=env._stream(), **out),
                 "gain_bias_only": lambda: env.batch.static_opt(None, stream=env._stream(), **gb)}

        def block(call, k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                call()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / k
        for call in calls.values():
            block(call, args.warmup)
        times = {k: [] for k in calls}
        for _ in range(args.blocks):
            for name, call in calls.items():
                times[name].append(block(call, args.steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        it, st = out["iters"].cpu().numpy(), out["status"].cpu().numpy()
        rec = {"dtype": dtype, "num_envs": n, "nu": nu, "nv": nv, "env_steps": args.env_steps, "steps_per_block": args.steps, "blocks": args.blocks,
               "static_opt_ms": med["static_opt"] * 1e3, "inverse_ms": med["inverse"] * 1e3, "gain_bias_only_ms": med["gain_bias_only"] * 1e3,
               "static_opt_over_inverse": med["static_opt"] / med["inverse"],
               "static_opt_ms_min_max": [min(times["static_opt"]) * 1e3, max(times["static_opt"]) * 1e3],
               "inverse_ms_min_max": [min(times["inverse"]) * 1e3, max(times["inverse"]) * 1e3],
               "iters_mean": float(it.mean()), "iters_max": int(it.max()), "converged": int((st == 0).sum()),
               "kkt_max": float(out["kkt"].max()), "active_at_lower_mean": float((out["u"] == 0).sum(1).double().mean()),
               "active_at_upper_mean": float((out["u"] == 1).sum(1).double().mean()),
               "workspace_mib": n * 832 * 8 / 2 ** 20}
        results.append(rec)
        print(json.dumps(rec))
        env.close()
    doc = {"what": "myo_batch_static_opt (all outputs) vs myo_batch_inverse on the same states, host time per call around device syncs; "
                   "inverse() is the yardstick for one extra pass; no threshold is set",
           "device": torch.cuda.get_device_name(0), "build": native.load().build_id, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if os.path.exists(args.out):      # the accuracy figures noted from the tests' output travel with the file
        try:
            doc["tolerance_yardsticks"] = json.load(open(args.out))["tolerance_yardsticks"]
        except (KeyError, ValueError):
            pass
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
