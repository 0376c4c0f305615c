"""Deterministic evaluation of a trained agent — the batched counterpart of /root/reference/src/main_eval.py.

The reference script (src/main_eval.py:52-118) builds one env, loads ``VecNormalize`` statistics and a
``RecurrentPPO`` zip, and plays ``num_episodes`` deterministic episodes one after another, printing the
mean length / return with their standard errors every 10 episodes.  Same inputs and printed quantities
here; the episodes run in parallel on the GPU.

    python -m myochallenge_amd.main_eval --model trained_models/baoding_phase2/final.zip \
        --env-path trained_models/baoding_phase2/normalized_env_final.pkl --env-name CustomMyoBaodingBallsP2
"""
from __future__ import annotations

import argparse
import json

import numpy as np

# evaluation configuration of the reference script (src/main_eval.py:13-45)
DEFAULT_CONFIG = {
    "weighted_reward_keys": {"pos_dist_1": 0, "pos_dist_2": 0, "act_reg": 0, "alive": 0, "solved": 5, "done": 0, "sparse": 0},
    "enable_rsi": False, "rsi_probability": 0, "balls_overlap": False, "overlap_probability": 0,
    "noise_fingers": 0, "limit_init_angle": 3.141592653589793, "goal_time_period": [4, 6],
    "goal_xrange": (0.020, 0.030), "goal_yrange": (0.022, 0.032),
    "obj_size_range": (0.018, 0.024), "obj_mass_range": (0.030, 0.300), "obj_friction_change": (0.2, 0.001, 0.00002),
    "task_choice": "random",
}


def evaluate(model_path: str, env_path: str, env_name: str = "CustomMyoBaodingBallsP2", config: dict = None,
             num_episodes: int = 100, num_envs: int = 256, seed: int = 0, deterministic: bool = True, verbose: bool = True,
             render_dir: str = None, render_envs: int = 1, render_size=(480, 480), render_tendons: bool = False,
             record_dir: str = None, env=None, render_contacts: bool = False, render_geom_alpha: float = None,
             muscle_condition: str = None, fatigue_params: dict = None, record_data=None, record_static_opt: bool = False,
             record_simulate: int = 0):
    """record_simulate: T > 0: record_dir's file also gets ``sim_qpos`` [T_steps, N, nq], the final qpos of ``env.simulate``'s
    T-control-step prediction from the step's state under zero muscle controls (``sim_bad`` [T_steps, N]: the prediction blew up);
    needs record_dir.
    record_static_opt: record_dir's file also gets ``so_u`` [T, N, nu], ``so_residual`` [T, N, nv] and ``so_status`` [T, N]: what a
    static optimiser would have chosen (``env.static_optimization`` for the step's own ``data()["qacc"]``) beside what the policy
    chose; needs record_dir.
    record_data: keys of ``env.data`` (MuJoCo's sim.data names: ``site_xpos``, ``qacc``, ...) that record_dir's file also gets,
    [T, N, ...] each; needs record_dir.
    muscle_condition / fatigue_params: evaluate under MyoSuite's ``muscle_condition`` ("sarcopenia", "fatigue", "reafferentation";
    fatigue_params: a dict with any of F, R, r) — they override the config's; with fatigue, record_dir also gets ``fatigue_MA`` /
    ``fatigue_MR`` / ``fatigue_MF`` [T, N, nu].
    record_dir: write ``batch00000.npz`` there — per env step t and env n: ``qpos``, ``qvel``, ``act`` (the state after the step: the
    reset state where the episode ended), ``actuator_length`` / ``actuator_velocity`` / ``actuator_force`` [T, N, nu], ``ncon`` [T, N] and
    ``object_wrench`` [T, N, nobj, 6] (net contact force and torque on the task's objects, ``object_body_ids``), from ``env.sensors``.
    env: an already built env to evaluate on instead of ``EnvironmentFactory.create(env_name, ...)``.
    render_tendons: draw the tendons, coloured by muscle activation, into the frames.  render_contacts: draw the contact points and
    contact forces into the frames, with the geoms' alpha multiplied by render_geom_alpha if given (``render_tensor``).  render_dir: write a PNG of each of the first ``render_envs`` envs after every step (``env{i}_step{t}.png``; the reference
    script's ``render`` switch, src/main_eval.py:96-97, shows the frames in a window instead)."""
    from .envs.environment_factory import EnvironmentFactory
    from .metrics.evaluation import evaluate_policy, summarize
    from .rl.sb3_zip import load_policy
    from .rl.vec_normalize import VecNormalize
    if config is None:             # the reference script's Baoding config; other envs: their registration defaults
        config = DEFAULT_CONFIG if env_name.startswith("CustomMyoBaoding") or env_name == "MixtureModelBaodingEnv" else {}
    config = dict(config)
    if muscle_condition is not None:
        config["muscle_condition"] = muscle_condition
    if fatigue_params:
        config["fatigue_params"] = dict(config.get("fatigue_params") or {}, **fatigue_params)
    if env is None:
        env = EnvironmentFactory.create(env_name, num_envs=min(num_envs, num_episodes), seed=seed, **config)
    venv = VecNormalize.load(env_path, env)
    venv.training = False          # src/main_eval.py:66-67
    venv.norm_reward = False
    policy, _ = load_policy(model_path)
    policy.to(env.device)
    on_step = None
    import os
    if render_dir:
        from .render_io import write_png
        os.makedirs(render_dir, exist_ok=True)
        k = max(1, min(int(render_envs), env.num_envs))
        style = {"geom_alpha": float(render_geom_alpha)} if render_contacts and render_geom_alpha is not None else None

        def on_step(t):
            rgb = env.render_tensor(list(range(k)), int(render_size[0]), int(render_size[1]), tendons=render_tendons, contacts=render_contacts,
                                    contact_style=style)["rgb"].cpu().numpy()
            for i in range(k):
                write_png(os.path.join(render_dir, f"env{i}_step{t:05d}.png"), rgb[i])
    rec = None
    record_data = list(record_data or [])
    if record_data and not record_dir:
        raise ValueError("record_data needs record_dir")
    if record_static_opt and not record_dir:
        raise ValueError("record_static_opt needs record_dir")
    record_simulate = int(record_simulate or 0)
    if record_simulate < 0:
        raise ValueError("record_simulate must be >= 0")
    if record_simulate and not record_dir:
        raise ValueError("record_simulate needs record_dir")
    if record_dir:
        os.makedirs(record_dir, exist_ok=True)
        rec = {k: [] for k in ("qpos", "qvel", "act", "actuator_length", "actuator_velocity", "actuator_force", "ncon", "object_wrench")}
        obj, draw = env.object_body_ids(), on_step
        fatigue = getattr(env, "muscle_condition", None) == "fatigue"
        if fatigue:
            rec.update(fatigue_MA=[], fatigue_MR=[], fatigue_MF=[])
        from .native import DATA_KEYS
        for k in record_data:
            if k not in DATA_KEYS:
                raise KeyError(f"unknown data key {k!r}; known: {sorted(DATA_KEYS)}")
            rec[k] = []
        if record_static_opt:
            rec.update(so_u=[], so_residual=[], so_status=[])
        if record_simulate:
            rec.update(sim_qpos=[], sim_bad=[])
            zero_ctrl = env.torch.zeros((env.num_envs, record_simulate, env.act_dim), dtype=env.torch.float64, device=env.device)

        def on_step(t):
            if draw is not None:
                draw(t)
            qp, qv, ac, _ = env.get_state()
            s = env.sensors(["act_length", "act_velocity", "act_force", "ncon", "body_wrench"])
            for k, v in (("qpos", qp), ("qvel", qv), ("act", ac), ("actuator_length", s["act_length"]), ("actuator_velocity", s["act_velocity"]),
                         ("actuator_force", s["act_force"]), ("ncon", s["ncon"]), ("object_wrench", s["body_wrench"][:, obj])):
                rec[k].append(v.cpu().numpy())
            if fatigue:
                for k, v in env.fatigue_state().items():
                    rec["fatigue_" + k].append(v.cpu().numpy())
            if record_data:
                for k, v in env.data(record_data).items():
                    rec[k].append(v.cpu().numpy())
            if record_static_opt:
                so = env.static_optimization(qacc=env.data(["qacc"])["qacc"], keys=["u", "residual", "status"])
                for k, v in so.items():
                    rec["so_" + k].append(v.cpu().numpy())
            if record_simulate:
                sm = env.simulate(zero_ctrl, every=record_simulate, keys=["qpos", "bad"])
                rec["sim_qpos"].append(sm["qpos"][:, 0, 0].cpu().numpy())
                rec["sim_bad"].append(sm["bad"][:, 0].cpu().numpy())
    res = evaluate_policy(policy, env, venv, n_eval_episodes=num_episodes, deterministic=deterministic, on_step=on_step)
    if rec is not None:
        np.savez(os.path.join(record_dir, "batch00000.npz"), object_body_ids=np.asarray(obj, np.int64), **{k: np.stack(v) for k, v in rec.items()})
    out = summarize(res)
    if verbose:
        print(f"Average len: {out['mean_len']:.2f} +/- {out['len_err']:.2f}")
        print(f"Average rew: {out['mean_rew']:.2f} +/- {out['rew_err']:.2f}")
        print(f"\nFinished evaluating {model_path}!")
    return res, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True, help="stable-baselines3 model zip (PATH_TO_PRETRAINED_NET)")
    ap.add_argument("--env-path", required=True, help="VecNormalize pickle (PATH_TO_NORMALIZED_ENV)")
    ap.add_argument("--env-name", default="CustomMyoBaodingBallsP2")
    ap.add_argument("--num-episodes", type=int, default=100)
    ap.add_argument("--num-envs", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--config", default=None, help="JSON file with the env kwargs (default: the reference script's config)")
    ap.add_argument("--out", default=None, help="write per-episode returns / lengths to this .npz")
    ap.add_argument("--render-dir", default=None, help="write PNG frames of the first --render-envs envs after every step here")
    ap.add_argument("--render-envs", type=int, default=1)
    ap.add_argument("--render-size", type=int, nargs=2, default=(480, 480), metavar=("W", "H"))
    ap.add_argument("--render-tendons", action="store_true", help="with --render-dir: draw the tendons, coloured by muscle activation")
    ap.add_argument("--render-contacts", action="store_true", help="with --render-dir: draw the contact points and contact forces")
    ap.add_argument("--render-geom-alpha", type=float, default=None, metavar="A",
                    help="with --render-contacts: multiply the geoms' alpha by A in [0, 1] (translucent geoms show the contact points between them)")
    ap.add_argument("--record-dir", default=None, help="write per-step qpos / qvel / act, actuator length / velocity / force, ncon and the "
                                                       "objects' contact wrenches of the evaluated batch to batch00000.npz here")
    ap.add_argument("--record-data", default=None, metavar="KEY[,KEY...]",
                    help="with --record-dir: also write these arrays of env.data (MuJoCo's sim.data names, e.g. site_xpos,qacc), [T, N, ...] each")
    ap.add_argument("--record-static-opt", action="store_true",
                    help="with --record-dir: also write so_u / so_residual / so_status per step: the activations a static optimiser "
                         "(env.static_optimization) would have chosen for the step's own acceleration")
    ap.add_argument("--record-simulate", type=int, default=0, metavar="T",
                    help="with --record-dir: also write sim_qpos / sim_bad per step: the final qpos of the T-step zero-control prediction "
                         "(env.simulate) from the step's state")
    ap.add_argument("--muscle-condition", default=None, choices=("sarcopenia", "fatigue", "reafferentation"),
                    help="evaluate under MyoSuite's muscle_condition (overrides the config's)")
    ap.add_argument("--fatigue-F", type=float, default=None, help="with --muscle-condition fatigue: fatigue rate F (default 0.00912)")
    ap.add_argument("--fatigue-R", type=float, default=None, help="... recovery rate R (default 0.000094)")
    ap.add_argument("--fatigue-r", type=float, default=None, help="... recovery multiplier during rest r (default 150)")
    a = ap.parse_args(argv)
    if a.render_tendons and not a.render_dir:
        ap.error("--render-tendons needs --render-dir")
    if a.render_contacts and not a.render_dir:
        ap.error("--render-contacts needs --render-dir")
    if a.render_geom_alpha is not None and not a.render_contacts:
        ap.error("--render-geom-alpha needs --render-contacts")
    if a.record_data and not a.record_dir:
        ap.error("--record-data needs --record-dir")
    if a.record_static_opt and not a.record_dir:
        ap.error("--record-static-opt needs --record-dir")
    if a.record_simulate < 0:
        ap.error("--record-simulate must be >= 0")
    if a.record_simulate and not a.record_dir:
        ap.error("--record-simulate needs --record-dir")
    fat = {k: v for k, v in (("F", a.fatigue_F), ("R", a.fatigue_R), ("r", a.fatigue_r)) if v is not None}
    if fat and a.muscle_condition != "fatigue":
        ap.error("--fatigue-F / --fatigue-R / --fatigue-r need --muscle-condition fatigue")
    cfg = json.load(open(a.config)) if a.config else None
    res, _ = evaluate(a.model, a.env_path, a.env_name, cfg, a.num_episodes, a.num_envs, a.seed,
                      render_dir=a.render_dir, render_envs=a.render_envs, render_size=a.render_size, render_tendons=a.render_tendons,
                      record_dir=a.record_dir, render_contacts=a.render_contacts, render_geom_alpha=a.render_geom_alpha,
                      muscle_condition=a.muscle_condition, fatigue_params=fat or None,
                      record_data=[k for k in a.record_data.split(",") if k] if a.record_data else None,
                      record_static_opt=a.record_static_opt, record_simulate=a.record_simulate)
    if a.out:
        np.savez(a.out, **res)


if __name__ == "__main__":
    main()
