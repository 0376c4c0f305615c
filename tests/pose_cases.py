"""Joint-pose task (kind MYO_TASK_POSE) checks shared by the emulation (CPU) and HIP (GPU) tests: the device's env steps against
oracle physics twins plus a numpy restatement of the task layer, with every per-episode draw rebuilt from the Philox stream."""
import numpy as np

from helpers import Mem, oracle_for
from myochallenge_amd import native
from oracle.oracle import OracleData

KEYS = ("pose", "bonus", "penalty", "act_reg", "sparse", "solved", "done")
_MASK = 0xFFFFFFFF


def philox_uniform(seed, c0, c1, c2, idx):
    """csrc/myo_task.h philox_uniform: Philox4x32-10 keyed by the batch seed, counter (c0, c1, c2, idx) -> (0, 1), 53 bits."""
    c = [c0 & _MASK, c1 & _MASK, c2 & _MASK, idx & _MASK]
    k0, k1 = seed & _MASK, (seed >> 32) & _MASK
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + 0x9E3779B9) & _MASK, (k1 + 0xBB67AE85) & _MASK
    bits = ((c[0] << 32) | c[1]) >> 11
    return (float(bits) + 0.5) * (1.0 / 9007199254740992.0)


def pose_draws(tcfg, nq, seed, env, episode):
    """CustomPoseEnv.reset's target and start pose of episode `episode` of env `env` (pose.py:55-97,109-113)."""
    u = np.array([philox_uniform(seed, env, episode, 0x504F5345, j) for j in range(2 * nq)])
    init = np.array(tcfg.pose_init_qpos[:nq])
    if tcfg.pose_target_type == native.POSE_TARGET_FIXED:
        full = np.array(tcfg.pose_target_value[:nq])
    else:
        r = np.array([tuple(x) for x in tcfg.pose_target_range[:nq]])
        full = r[:, 0] + (r[:, 1] - r[:, 0]) * u[:nq]
    tgt = init + tcfg.pose_target_distance * (full - init)
    if tcfg.pose_reset_type == native.POSE_RESET_RANDOM:
        r = np.array([tuple(x) for x in tcfg.pose_reset_range[:nq]])
        q0 = r[:, 0] + (r[:, 1] - r[:, 0]) * u[nq:]
    elif tcfg.pose_reset_type == native.POSE_RESET_SDS:
        q0 = (1 - tcfg.pose_sds_distance) * tgt + tcfg.pose_sds_distance * init
    else:
        q0 = init.copy()
    return tgt, q0


def pose_obs_reward(tcfg, qpos, qvel, act, tgt, dt):
    """PoseEnvV0.get_obs_dict / get_reward_dict [3P-RECALL, envs/pose.py MYOSUITE_POSE] -> obs, comps (+ dense), pose_dist."""
    err = tgt - qpos
    obs = np.concatenate([qpos, qvel * dt, err])
    d = np.linalg.norm(err)
    am = np.linalg.norm(act) / len(act) if len(act) else 0.0
    thd, far = tcfg.pose_thd, tcfg.pose_far_th
    r = dict(pose=-d, bonus=float(d < thd) + float(d < 1.5 * thd), penalty=-float(d > far), act_reg=-am, sparse=-d,
             solved=float(d < thd), done=float(d > far))
    comps = np.array([r[k] for k in KEYS] + [sum(tcfg.pose_weights[i] * r[k] for i, k in enumerate(KEYS))])
    return obs, comps, d


def ctrl_of(a):
    """BaseV0.step's muscle map as csrc/myo_task.h computes it: float32 sigmoid(5 (clip(a) - 0.5)), exp correctly rounded."""
    a = np.clip(np.asarray(a, np.float32), np.float32(-1), np.float32(1))
    x = (np.float32(-5.0) * (a - np.float32(0.5))).astype(np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(x.astype(np.float64)).astype(np.float32))).astype(np.float64)


def pose_episodes(lib, dtype, env_name, n=3, nsteps=100, horizon=100, seed=3, act_seed=5, model=None, **kw):
    """`nsteps` env steps of `n` envs on the device against oracle twins that start from the rebuilt draws of every episode.
    Returns the largest errors seen: qpos (relative, fp64 state), obs (absolute, float32), comps; and the episode counts."""
    from myochallenge_amd.envs.pose import make_pose_cfg
    from myochallenge_amd.synth_hand import synthetic_hand_pose
    mem = Mem(lib)
    cm, om, _ = oracle_for(model if model is not None else synthetic_hand_pose())
    tcfg = make_pose_cfg(env_name, cm, max_episode_steps=horizon, **kw)
    b = native.Batch(native.Model(cm, lib), tcfg, n, 0, seed, dtype)
    nq, nv, na, nu = om.nq, om.nv, om.na, om.nu
    assert b.obs_dim == 2 * nq + nv
    dt = tcfg.frame_skip * float(cm.fields["opt_f64"][0])
    obs, rew, done, trunc = mem.zeros((n, b.obs_dim), np.float32), mem.zeros(n, np.float32), mem.zeros(n, np.uint8), mem.zeros(n, np.uint8)
    term, comps, ep = mem.zeros((n, b.obs_dim), np.float32), mem.zeros((n, 8), np.float32), mem.zeros((n, 2), np.float32)
    qp, qv, ac, tm = mem.zeros((n, nq)), mem.zeros((n, nv)), mem.zeros((n, na)), mem.zeros(n)
    ti, td = mem.zeros((n, 2), np.int32), mem.zeros((n, 2 * nq))
    err = dict(qpos=0.0, obs=0.0, comps=0.0, draws=0.0)
    episode, lens, rets = np.ones(n, int), np.zeros(n, int), np.zeros(n)
    twins = [None] * n

    def start(e, dev_obs):
        """a reset just happened on the device: its draws, state and observation against the rebuilt ones; new oracle twin"""
        tgt, q0 = pose_draws(tcfg, nq, seed, e, int(episode[e]))
        b.get_task(ti, td, None)
        b.get_state(qp, qv, ac, tm)
        htd, hq, hv, ha, ht = (mem.host(x)[e] for x in (td, qp, qv, ac, tm))
        err["draws"] = max(err["draws"], np.abs(htd[:nq] - tgt).max(), np.abs(htd[nq:] - q0).max(), np.abs(hq - q0).max())
        assert np.all(hv == 0) and np.all(ha == 0) and ht == 0 and int(mem.host(ti)[e, 1]) == 0
        o, _, _ = pose_obs_reward(tcfg, q0, np.zeros(nv), np.zeros(na), tgt, dt)
        err["obs"] = max(err["obs"], np.abs(dev_obs - o).max())
        d = OracleData(om)
        d.reset()
        d.qpos[:] = q0
        d.qvel[:] = 0
        d.act[:] = 0
        twins[e] = (d, tgt)

    b.reset(None, obs)
    ho = mem.host(obs).copy()
    for e in range(n):
        start(e, ho[e])
    rng = np.random.RandomState(act_seed)
    for t in range(nsteps):
        a = rng.uniform(-1, 1, (n, nu)).astype(np.float32)
        b.step(mem.arr(a, np.float32), obs, rew, done, trunc, term, comps, ep)
        b.get_state(qp, qv, ac, tm)
        ho, hr, hd, ht, hterm, hc, hep, hq = (mem.host(x).copy() for x in (obs, rew, done, trunc, term, comps, ep, qp))
        for e in range(n):
            d, tgt = twins[e]
            d.ctrl[:] = ctrl_of(a[e])
            for _ in range(tcfg.frame_skip):
                d.step()
            o, c, dist = pose_obs_reward(tcfg, d.qpos.copy(), d.qvel.copy(), d.act.copy(), tgt, dt)
            lens[e] += 1
            rets[e] += c[7]
            dev_obs = hterm[e] if hd[e] else ho[e]
            err["obs"] = max(err["obs"], np.abs(dev_obs - o).max())
            if not hd[e]:
                err["qpos"] = max(err["qpos"], np.abs(hq[e] - d.qpos).max() / max(1.0, np.abs(d.qpos).max()))
            near = min(abs(dist - tcfg.pose_thd), abs(dist - 1.5 * tcfg.pose_thd), abs(dist - tcfg.pose_far_th)) < 1e-6
            if not near:                                   # the 0 / 1 terms: identical unless the distance sits on a threshold
                assert np.array_equal(hc[e][[1, 2, 5, 6]], c[[1, 2, 5, 6]].astype(np.float32)), (t, e, hc[e], c)
                err["comps"] = max(err["comps"], np.abs(hc[e] - c).max() / (1 + np.abs(c).max()), abs(hr[e] - c[7]) / (1 + abs(c[7])))
                farr, timeout = bool(c[6]), lens[e] >= horizon
                assert bool(hd[e]) == (farr or timeout) and bool(ht[e]) == (timeout and not farr), (t, e)
            if hd[e]:
                assert int(hep[e, 1]) == lens[e] and abs(hep[e, 0] - rets[e]) < 1e-4 * (1 + abs(rets[e]))
                episode[e] += 1
                lens[e], rets[e] = 0, 0.0
                start(e, ho[e])
    b.close()
    err["episodes"] = int((episode - 1).sum())
    return err, tcfg
