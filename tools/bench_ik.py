#!/usr/bin/env python
"""Time one inverse-kinematics call (myo_batch_ik) next to the loop a user would stitch together on the host without it.

The workload: 4096 Baoding-hand envs (CustomMyoBaodingBallsP1; nv 35, 23 hinge joints) after a reset, fp64 and mixed steppers; five
sites, the last one on each finger's distal body; targets = the sites' positions at a pose U(-0.3, 0.3) rad away from the present
one in joint space, clipped to the joint ranges (reachable).  Both go through the batch's C ABI binding with preallocated outputs, in
one process, and are timed alternately, block by block, after a warm-up of each, between two device synchronisations (host clock);
the per-call time is the median over the blocks.

  kernel     env.batch.ik(...), every output, max_iter 50: one launch.  steps = accepted + rejected Levenberg-Marquardt steps.
  stitched   per step: set_state(q), data(site_xpos), jac("site"), then torch on the device: g = J'e + reg (q - q_ref),
             H = J'J + (reg + mu) I, a batched Cholesky solve, q <- clip(q + d).  A fixed damping and no acceptance test (no second
             position pass per step), so a step of it does LESS than a step of the kernel; run for the kernel's largest step count, with
             the env states saved before and restored after, since it overwrites them.

No threshold is set.  Needs a GPU.

    python tools/bench_ik.py [--envs 4096] [--steps 5] [--blocks 5] [--out profiles/ik.json]
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


def joints_of(compiled):
    """(dof, qpos address, lower, upper) of the hinge / slide joints, numpy arrays"""
    import numpy as np
    f = compiled.fields
    jt = np.asarray(f["jnt_type"])
    hs = np.flatnonzero((jt == 2) | (jt == 3))
    rng, lim = np.asarray(f["jnt_range"], float).reshape(-1, 2)[hs], np.asarray(f["jnt_limited"])[hs] != 0
    return (np.asarray(f["jnt_dofadr"])[hs].astype(int), np.asarray(f["jnt_qposadr"])[hs].astype(int),
            np.where(lim, rng[:, 0], -np.inf), np.where(lim, rng[:, 1], np.inf))


def tip_sites(compiled):
    """the last site on every childless body that no free joint carries"""
    import numpy as np
    f = compiled.fields
    par, sb, jt, jb = (np.asarray(f[k]) for k in ("body_parentid", "site_bodyid", "jnt_type", "jnt_bodyid"))
    free = set(jb[jt == 0].tolist())
    return [int(np.flatnonzero(sb == b)[-1]) for b in range(1, len(par)) if not (par[1:] == b).any() and b not in free and (sb == b).any()]


class Stitched:
    """the host-stitched loop on preallocated device tensors"""

    def __init__(self, env, ids, targets, reg, mu):
        import torch
        t, self.env = torch, env
        n, dev, m = env.num_envs, env.device, env._model
        dofs, qadr, lo, hi = joints_of(env.compiled)
        self.dofs, self.qadr = t.as_tensor(dofs, device=dev), t.as_tensor(qadr, device=dev)
        self.lo, self.hi = t.as_tensor(lo, device=dev), t.as_tensor(hi, device=dev)
        self.ids = t.as_tensor(ids, dtype=t.int32, device=dev)
        self.idl = self.ids.long()
        self.targets, self.reg, self.mu = targets, reg, mu
        f64 = lambda *shape: t.empty((n,) + shape, dtype=t.float64, device=dev)
        self.X, self.J = f64(m.size("nsite"), 3), f64(len(ids), 3, m.size("nv"))
        self.state = [f64(m.size("nq")), f64(m.size("nv")), f64(m.size("na")), f64()]
        self.warm = f64(m.size("nv"))
        self.eye = t.eye(len(dofs), dtype=t.float64, device=dev)

    def run(self, steps):
        t, env, b, st = __import__("torch"), self.env, self.env.batch, self.env._stream()
        b.get_state(*self.state, st)
        b.warmstart(self.warm, None, st)
        q = self.state[0].clone()
        qref = q[:, self.qadr].clone()
        for _ in range(steps):
            b.set_state(q, None, None, None, st)
            b.data(st, None, site_xpos=self.X)
            b.jac("site", self.ids, self.J, None, None, st)
            e = (self.X[:, self.idl] - self.targets).reshape(q.shape[0], -1, 1)
            Ja = self.J[:, :, :, self.dofs].reshape(q.shape[0], -1, len(self.dofs))
            qa = q[:, self.qadr]
            g = (Ja.transpose(1, 2) @ e).squeeze(2) + self.reg * (qa - qref)
            H = Ja.transpose(1, 2) @ Ja + (self.reg + self.mu) * self.eye
            d = t.cholesky_solve(-g.unsqueeze(2), t.linalg.cholesky(H)).squeeze(2)
            q[:, self.qadr] = t.minimum(t.maximum(qa + d, self.lo), self.hi)
        b.set_state(*self.state, st)
        b.warmstart(None, self.warm, st)
        return q, e


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dtypes", nargs="+", default=["f64", "mixed"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ik.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("bench_ik: needs a GPU", file=sys.stderr)
        return 1
    from myochallenge_amd import native
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    results = []
    for dtype in args.dtypes:
        env = EnvironmentFactory.create("CustomMyoBaodingBallsP1", num_envs=args.envs, seed=1, dtype=dtype)
        env.reset()
        rec = measure(env, args, dtype)
        results.append(rec)
        print(json.dumps(rec))
        env.close()
    doc = {"what": "myo_batch_ik (all outputs, one launch) vs the host-stitched loop set_state + data + jac + batched torch solve run for the "
                   "kernel's largest step count, host time per call around device syncs; no threshold is set",
           "device": torch.cuda.get_device_name(0), "build": native.load().build_id, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


def measure(env, args, dtype, sync=None):
    import numpy as np
    import torch
    from myochallenge_amd import native
    sync = sync or torch.cuda.synchronize
    n, dev, m = env.num_envs, env.device, env._model
    ids = tip_sites(env.compiled)
    k = len(ids)
    dofs, qadr, lo, hi = joints_of(env.compiled)
    present = torch.zeros((n, m.size("nq")), dtype=torch.float64, device=dev)
    env.batch.get_state(present, None, None, None)
    q = present.cpu().numpy().copy()
    q[:, qadr] = np.clip(q[:, qadr] + np.random.RandomState(1).uniform(-0.3, 0.3, (n, len(qadr))), lo, hi)
    env.batch.set_state(torch.as_tensor(q, device=dev), None, None, None)
    targets = env.data(["site_xpos"])["site_xpos"][:, ids].contiguous()
    env.batch.set_state(present, None, None, None)
    ids_t = torch.as_tensor(ids, dtype=torch.int32, device=dev)
    shapes = env.batch.ik_shapes(k)
    tdt = {np.int32: torch.int32, np.float64: torch.float64}
    out = {key: torch.empty((n,) + shapes[key][0], dtype=tdt[shapes[key][1]], device=dev) for key in shapes}
    kernel = lambda: env.batch.ik(ids_t, targets, stream=env._stream(), **out)
    kernel()
    sync()
    it, st = out["iters"].cpu().numpy(), out["status"].cpu().numpy()
    steps = int(it.max())
    loop = Stitched(env, ids, targets, 1e-6, 1e-6)
    calls = {"kernel": kernel, "stitched": lambda: loop.run(steps)}

    def block(call, reps):
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        sync()
        return (time.perf_counter() - t0) / reps
    for call in calls.values():
        block(call, args.warmup)
    times = {key: [] for key in calls}
    for _ in range(args.blocks):
        for name, call in calls.items():
            times[name].append(block(call, args.steps))
    med = {key: statistics.median(v) for key, v in times.items()}
    _, e = loop.run(steps)
    sync()
    return {"dtype": dtype, "num_envs": n, "nv": m.size("nv"), "active_joints": len(dofs), "sites": k, "calls_per_block": args.steps, "blocks": args.blocks,
            "kernel_ms": med["kernel"] * 1e3, "kernel_ms_min_max": [min(times["kernel"]) * 1e3, max(times["kernel"]) * 1e3],
            "steps_mean": float(it.mean()), "steps_max": steps, "kernel_ms_per_step": med["kernel"] * 1e3 / max(steps, 1),
            "converged": int((st == 0).sum()), "kkt_max": float(out["kkt"].max()), "residual_max_m": float(out["residual"].abs().max()),
            "stitched_steps": steps, "stitched_ms": med["stitched"] * 1e3, "stitched_ms_min_max": [min(times["stitched"]) * 1e3, max(times["stitched"]) * 1e3],
            "stitched_ms_per_step": med["stitched"] * 1e3 / max(steps, 1), "stitched_residual_max_m": float(e.abs().max()),
            "stitched_over_kernel": med["stitched"] / med["kernel"], "workspace_mib": n * native.IK_WS_DOUBLES * 8 / 2 ** 20}


if __name__ == "__main__":
    sys.exit(main())
