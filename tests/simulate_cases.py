"""Cases of the read-only open-loop simulation (myo_batch_simulate, csrc/myo_simulate.h) shared by the emulation (CPU) and HIP (GPU)
tests of tests/test_simulate.py.  Every case goes through the C ABI.

Shapes unless a case says otherwise: the synthetic Baoding hand (P2's per-env ball parameters), 3 envs a few steps into an episode so
that the balls are in contact, envs listed as [2, 0, 2], S = 3 samples, T = 4 control steps of nsub = 2 substeps, every = 2 (R = 2
recorded rows), seeded controls in [0, 1].

References and bounds.
  composed path    a twin batch of k S envs filled with myo_batch_copy_envs (whole records: state, warm start, task block, per-episode
                   parameters), start states overwritten with set_state where the case overrides them, then T x (physics_step +
                   get_state): the same mj_step of the same library on the same kernel variant, and the record round trip is
                   lossless, so qpos / qvel / act / time are compared BIT FOR BIT.
  oracle           one oracle twin per (env, sample) at the same start state, warm start and per-env object parameters, stepped with
                   the same controls.  The bounds are tests/parity_cases.py's (case_trajectory): rel_err < 1e-9 (fp64 stepper),
                   < 1e-4 (mixed), qvel by the same factor times max(1, |qvel|_inf), time within 1e-9; site_xpos against the oracle's
                   site positions of a forward pass at the new state, under the same relative bound.
"""
import ctypes as C

import numpy as np

import data_cases as dc
import sensor_cases as sc
from helpers import Mem, oracle_for, rel_err
from myochallenge_amd import native
from oracle.oracle import OracleData, make_cfg

TOL = sc.TOL                      # {MYO_F64: 1e-9, MYO_MIXED: 1e-4}: parity_cases' bounds
HEALTHY = sc.HEALTHY
F64 = native.MYO_F64
KEYS = native.SIM_KEYS
IDX, S, T, NSUB, EVERY = [2, 0, 2], 3, 4, 2, 2
_MODELS = {}


# ---------------------------------------------------------------------------------------------------------------- plumbing
def model_of(which, integrator=None):
    """(compiled model, oracle model) of the Baoding stand-in ("hand") or the die stand-in ("die"), compiled once per integrator"""
    key = (which, integrator)
    if key not in _MODELS:
        from myochallenge_amd.synth_hand import synthetic_hand, synthetic_hand_die
        cm, om, _ = oracle_for(synthetic_hand() if which == "hand" else synthetic_hand_die(), integrator=integrator)
        _MODELS[key] = (cm, om)
    return _MODELS[key]


class Setup:
    """a batch a few steps into an episode, what the oracle needs to follow its envs, and the means to build the composed path"""

    def __init__(self, lib, dtype, which="hand", integrator=None, n=3, seed=1, nsteps=3):
        from myochallenge_amd.envs.config import make_task_cfg, task_ids
        self.lib, self.dtype, self.which, self.n = lib, dtype, which, n
        self.mem = mem = Mem(lib)
        self.cm, self.om = cm, om = model_of(which, integrator)
        self.model = native.Model(cm, lib)
        if which == "hand":
            from parity_cases import p2_ball_params
            self.cfg = make_task_cfg("CustomMyoBaodingBallsP2", cm)
            self.ocfg = make_cfg(task_ids(cm))
        else:
            from myochallenge_amd.envs.reorient import make_reorient_cfg
            from parity_cases import reorient_oracle_cfg
            self.cfg = make_reorient_cfg("CustomMyoReorientP2", cm, max_episode_steps=200)
            self.ocfg = reorient_oracle_cfg(cm, self.cfg)
        self.b = b = native.Batch(self.model, self.cfg, n, 0, seed, dtype)
        obs, rew, done = mem.zeros((n, b.obs_dim), np.float32), mem.zeros(n, np.float32), mem.zeros(n, np.uint8)
        b.reset(None, obs)
        if which == "hand":
            b.set_task(None, None, mem.arr(p2_ball_params(n, seed)))
        rng = np.random.RandomState(seed)
        for _ in range(nsteps):
            a = np.clip(rng.normal(0.5 if which == "die" else 0.0, 0.5, (n, om.nu)), -1, 1)
            b.step(mem.arr(a, np.float32), obs, rew, done)
            assert not mem.host(done).any()
        self.obs, self.rew, self.done = obs, rew, done
        self.state = sc.device_state(b, mem, om)          # qpos, qvel, act, time, warm start
        self.task = dc.task_arrays(b, mem)                # task_i, task_d, ball_d
        self.fric = None
        if which == "die":
            assert b.contact_capacity == 48
            fr = mem.zeros((n, self.ocfg.gidn - self.ocfg.gid0, 3))
            b.object_friction(None, fr)
            self.fric = mem.host(fr).copy()

    def snapshot(self):
        """everything of the envs a call could move: state, warm start, task arrays, the die's friction"""
        out = sc.device_state(self.b, self.mem, self.om) + list(dc.task_arrays(self.b, self.mem))
        if self.which == "die":
            fr = self.mem.zeros(self.fric.shape)
            self.b.object_friction(None, fr)
            out.append(self.mem.host(fr).copy())
        return out

    def prepare(self, e):
        """the oracle twin's per-env parameters"""
        if self.which == "hand":
            return dc.baoding_prepare(self.ocfg, self.task[1][e], self.task[2][e])
        from oracle.oracle import reorient_set_die
        return lambda d: reorient_set_die(d, self.ocfg, self.fric[e], self.task[2][e, 8])

    def controls(self, k, s, t, seed=3):
        return np.random.RandomState(seed).uniform(0, 1, (k, s, t, self.om.nu))

    def starts(self, idx, s, seed=4, scale=1e-3):
        """start states [k, S, .]: the listed envs' own, the hand's joint angles / every velocity / the activations moved a little"""
        rng = np.random.RandomState(seed)
        k, f = len(idx), self.cm.fields
        jt, qadr = np.asarray(f["jnt_type"]), np.asarray(f["jnt_qposadr"])
        hinge = qadr[(jt == 2) | (jt == 3)].astype(int)
        q = np.repeat(self.state[0][idx][:, None], s, 1)
        v = np.repeat(self.state[1][idx][:, None], s, 1)
        a = np.repeat(self.state[2][idx][:, None], s, 1)
        q[:, :, hinge] += rng.uniform(-scale, scale, (k, s, len(hinge)))
        v += rng.uniform(-scale, scale, v.shape)
        a = np.clip(a + rng.uniform(-0.05, 0.05, a.shape), 0, 1)
        return q, v, a

    def close(self):
        self.b.close()


def simulate_all(st, idx=IDX, s=S, t=T, nsub=NSUB, every=EVERY, ctrl=None, start=None, sites=None, want=KEYS, b=None):
    """host copies of the outputs of one call; the outputs are pre-filled (a sentinel / -7) and no fill may survive.  ctrl: [k, S, T, nu]
    (per sample), [k, T, nu] (shared) or None; start: (qpos0, qvel0, act0) [k, S, .] or None; idx None: all envs in order"""
    b, mem = b or st.b, st.mem
    k = b.n if idx is None else len(idx)
    ns = 0 if sites is None else len(sites)
    sh = b.simulate_shapes(s, t // every, ns)
    want = [x for x in want if x != "site_xpos" or ns]
    fill = lambda dt: 1.25e300 if dt is np.float64 else -7
    out = {key: mem.arr(np.full((k,) + sh[key][0], fill(sh[key][1])), sh[key][1]) for key in want}
    opt = lambda x, dt=np.float64: None if x is None else mem.arr(x, dt)
    q0, v0, a0 = start if start is not None else (None, None, None)
    b.simulate(k, s, t, opt(ctrl), ctrl is not None and np.ndim(ctrl) == 4, opt(idx, np.int32), nsub, every, opt(q0), opt(v0), opt(a0),
               opt(sites, np.int32), None, **out)
    res = {key: mem.host(v).copy() for key, v in out.items()}
    for key, v in res.items():
        assert not (v == fill(sh[key][1])).any(), key
    return res


def composed(st, idx, s, t, nsub, every, ctrl, start=None):
    """the route a user would stitch together: a twin batch of k S envs, copy_envs, set_state, T x (physics_step + get_state)"""
    mem, om, k = st.mem, st.om, len(idx)
    n2 = k * s
    twin = native.Batch(st.model, st.cfg, n2, 0, 99, st.dtype)
    src = np.repeat(np.asarray(idx, np.int32), s)
    twin.copy_envs_from(st.b, mem.arr(np.arange(n2), np.int32), mem.arr(src, np.int32))
    twin.warmstart(None, mem.arr(st.state[4][src]))
    if start is not None:
        twin.set_state(*(mem.arr(x.reshape(n2, -1)) for x in start), None)
    bufs = [mem.zeros((n2, om.nq)), mem.zeros((n2, om.nv)), mem.zeros((n2, om.na)), mem.zeros(n2)]
    r = t // every
    out = {"qpos": np.zeros((k, s, r, om.nq)), "qvel": np.zeros((k, s, r, om.nv)), "act": np.zeros((k, s, r, om.na)), "time": np.zeros((k, s, r))}
    c = np.broadcast_to(ctrl if np.ndim(ctrl) == 4 else np.asarray(ctrl)[:, None], (k, s, t, om.nu))
    for i in range(t):
        twin.physics_step(mem.arr(np.ascontiguousarray(c[:, :, i]).reshape(n2, om.nu)), nsub)
        if (i + 1) % every == 0:
            twin.get_state(*bufs)
            for key, x in zip(("qpos", "qvel", "act", "time"), bufs):
                out[key][:, :, (i + 1) // every - 1] = mem.host(x).reshape((k, s) + out[key].shape[3:])
    assert twin.health() == HEALTHY
    twin.close()
    return out


def tracked_sites(st):
    """a fingertip-side site, a ball / die site and the task's target sites (placed per env)"""
    names = list(st.cm.names["site"])
    ids = [len(names) - 1, 0]
    for nm in ("ball1_site", "target1_site", "target2_site", "object_o", "target_o"):
        if nm in names:
            ids.append(names.index(nm))
    return ids


# ---------------------------------------------------------------------------------------------------------------- 1. the composed path
def case_composed(lib, dtype, which="hand", integrator=None, override=True, bitwise=True):
    """simulate == copy_envs + set_state + T x (physics_step, get_state), bit for bit (bitwise=False: within parity_cases' bounds)"""
    st = Setup(lib, dtype, which, integrator, n=3 if which == "hand" else 2, nsteps=3 if which == "hand" else 4)
    idx = IDX if which == "hand" else [1, 0, 1]
    ctrl = st.controls(len(idx), S, T)
    start = st.starts(idx, S) if override else None
    got = simulate_all(st, idx, ctrl=ctrl, start=start, sites=tracked_sites(st))
    ref = composed(st, idx, S, T, NSUB, EVERY, ctrl, start)
    assert (got["bad"] == 0).all() and (got["steps"] == T).all()
    worst = {}
    for key in ("qpos", "qvel", "act", "time"):
        worst[key] = float(np.abs(got[key] - ref[key]).max())
        print(f"    {which} dtype {dtype} integrator {integrator}: {key} max |simulate - composed| = {worst[key]:.3e}")
        if bitwise:
            assert np.array_equal(got[key], ref[key]), (key, worst[key])
        else:
            assert worst[key] <= TOL[dtype] * max(1.0, float(np.abs(ref[key]).max())), (key, worst[key])
    # the controls and the start states reach the physics: another sample of the same env ends elsewhere
    assert not np.array_equal(got["qpos"][0, 0], got["qpos"][0, 1])
    assert np.isfinite(got["site_xpos"]).all()
    assert st.b.health() == HEALTHY
    st.close()
    return worst


# ---------------------------------------------------------------------------------------------------------------- 2. the oracle
def case_oracle(lib, dtype, which="hand", integrator=None):
    st = Setup(lib, dtype, which, integrator, n=3 if which == "hand" else 2, nsteps=3 if which == "hand" else 4)
    idx = IDX if which == "hand" else [1, 0, 1]
    om, tol = st.om, TOL[dtype]
    ctrl = st.controls(len(idx), S, T)
    start = st.starts(idx, S)
    sites = tracked_sites(st)
    if which == "die":      # (the twin keeps the `target` body where the model has it, the device at the goal pose: data_cases.case_die_parity)
        goal_b = int(np.asarray(st.cm.fields["site_bodyid"])[st.ocfg.goal_sid])
        sites = [i for i in sites if int(np.asarray(st.cm.fields["site_bodyid"])[i]) != goal_b]
    got = simulate_all(st, idx, ctrl=ctrl, start=start, sites=sites)
    assert (got["bad"] == 0).all() and (got["steps"] == T).all()
    worst = {"qpos": 0.0, "qvel": 0.0, "act": 0.0, "site_xpos": 0.0}
    for a, e in enumerate(idx):
        for j in range(S):
            d = OracleData(om)
            d.reset()
            d.qpos[:], d.qvel[:], d.act[:] = start[0][a, j], start[1][a, j], start[2][a, j]
            d.arr("time")[0] = st.state[3][e]
            d.arr("qacc_warmstart")[:] = st.state[4][e]
            st.prepare(e)(d)
            for t in range(T):
                d.ctrl[:] = ctrl[a, j, t]
                for _ in range(NSUB):
                    d.step()
                if (t + 1) % EVERY:
                    continue
                r = (t + 1) // EVERY - 1
                eq, ev, ea = rel_err(got["qpos"][a, j, r], d.qpos), np.abs(got["qvel"][a, j, r] - d.qvel).max() / max(1.0, np.abs(d.qvel).max()), rel_err(got["act"][a, j, r], d.act)
                d2 = OracleData(om)      # the oracle's site positions at the NEW state
                d2.reset()
                d2.qpos[:], d2.qvel[:], d2.act[:] = d.qpos, d.qvel, d.act
                st.prepare(e)(d2)
                d2.ctrl[:] = 0
                d2.forward()
                es = rel_err(got["site_xpos"][a, j, r], d2.arr("site_xpos").reshape(-1, 3)[sites])
                for key, v in zip(("qpos", "qvel", "act", "site_xpos"), (eq, ev, ea, es)):
                    worst[key] = max(worst[key], float(v))
                assert eq < tol and ev < tol and ea < tol and es < tol, (e, j, t, eq, ev, ea, es)
                assert abs(got["time"][a, j, r] - d.arr("time")[0]) < 1e-9
    print(f"    {which} dtype {dtype} integrator {integrator}: worst errors against the oracle {worst} (bound {tol})")
    st.close()
    return worst


# ---------------------------------------------------------------------------------------------------------------- 3. read-only
def case_read_only(lib, dtype, which="hand"):
    """the envs do not move: state, warm start, task arrays and the die's friction are the same bits after a call with start states
    given, and a following step returns the bits of a batch that never simulated"""
    a, b = (Setup(lib, dtype, which, n=3 if which == "hand" else 2, nsteps=3 if which == "hand" else 4) for _ in range(2))
    idx = IDX if which == "hand" else [1, 0, 1]
    before = a.snapshot()
    for start in (a.starts(idx, S), None):
        got = simulate_all(a, idx, ctrl=a.controls(len(idx), S, T), start=start, sites=tracked_sites(a))
        assert (got["bad"] == 0).all()
        for p, q in zip(before, a.snapshot()):
            assert np.array_equal(p, q)
    act = a.mem.arr(np.clip(np.random.RandomState(8).normal(0, 0.5, (a.n, a.om.nu)), -1, 1), np.float32)
    for x in (a, b):
        x.b.step(act, x.obs, x.rew, x.done)
    for p, q in zip(a.snapshot() + [a.mem.host(v).copy() for v in (a.obs, a.rew, a.done)], b.snapshot() + [b.mem.host(v).copy() for v in (b.obs, b.rew, b.done)]):
        assert np.array_equal(p, q)
    assert a.b.health() == b.b.health() == HEALTHY
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. independence
def case_independence(lib, dtype, integrator=None):
    st = Setup(lib, dtype, "hand", integrator)
    ctrl, start, sites = st.controls(len(IDX), S, T), st.starts(IDX, S), tracked_sites(st)
    a, b = (simulate_all(st, ctrl=ctrl, start=start, sites=sites) for _ in range(2))
    for key in a:                                                   # two calls: the same bits
        assert np.array_equal(a[key], b[key]), key
    for j in range(S):                                              # a sample does not depend on S or on its neighbours
        one = simulate_all(st, s=1, ctrl=ctrl[:, j:j + 1], start=tuple(x[:, j:j + 1] for x in start), sites=sites)
        for key in a:
            assert np.array_equal(one[key][:, 0], a[key][:, j]), (key, j)
    # ... nor on the other listed envs: the list reversed, and one output alone
    rev = simulate_all(st, idx=IDX[::-1], ctrl=ctrl[::-1], start=tuple(x[::-1] for x in start), sites=sites)
    for key in a:
        assert np.array_equal(rev[key][::-1], a[key]), key
    assert np.array_equal(simulate_all(st, ctrl=ctrl, start=start, want=("qvel",))["qvel"], a["qvel"])
    # repeated indices with the same inputs: identical rows (IDX lists env 2 twice)
    c2, s2 = ctrl.copy(), tuple(x.copy() for x in start)
    c2[2] = c2[0]
    for x in s2:
        x[2] = x[0]
    rep = simulate_all(st, ctrl=c2, start=s2, sites=sites)
    for key in rep:
        assert np.array_equal(rep[key][0], rep[key][2]), key
    # shared controls == the same controls repeated per sample; no controls == zeros; idx None == all envs in order
    shared = simulate_all(st, ctrl=ctrl[:, 0], start=start, sites=sites)
    tiled = simulate_all(st, ctrl=np.repeat(ctrl[:, :1], S, 1), start=start, sites=sites)
    for key in shared:
        assert np.array_equal(shared[key], tiled[key]), key
    zero = simulate_all(st, ctrl=None)
    zeros = simulate_all(st, ctrl=np.zeros((len(IDX), T, st.om.nu)))
    every = simulate_all(st, idx=None, ctrl=None)
    listed = simulate_all(st, idx=list(range(st.n)), ctrl=None)
    for key in zero:
        assert np.array_equal(zero[key], zeros[key]) and np.array_equal(every[key], listed[key]), key
    assert np.array_equal(every["qpos"][[2, 0, 2]], zero["qpos"])
    # every = 1 records every step; its odd rows are every = 2's
    fine = simulate_all(st, every=1, ctrl=ctrl, start=start, sites=sites)
    for key in ("qpos", "qvel", "act", "time", "site_xpos"):
        assert fine[key].shape[2] == T and np.array_equal(fine[key][:, :, 1::2], a[key]), key
    # nsub = 0 is the task's frame_skip
    fs = int(st.cfg.frame_skip)
    assert fs >= 1
    auto, named = simulate_all(st, t=2, nsub=0, every=1, ctrl=ctrl[:, :, :2]), simulate_all(st, t=2, nsub=fs, every=1, ctrl=ctrl[:, :, :2])
    for key in auto:
        assert np.array_equal(auto[key], named[key]), key
    assert st.b.health() == HEALTHY
    st.close()


# ---------------------------------------------------------------------------------------------------------------- 5. blow-up
def case_blow_up(lib, dtype):
    """one sample starts with an absurd finger velocity (parity_cases.case_bad_state's), one with a NaN ball velocity: bad = 1, steps = 0,
    NaN rows; a sample that blows up later keeps the rows it completed; the neighbours are the bits of a clean call; the env is unchanged"""
    st = Setup(lib, dtype, "hand")
    ctrl, start, sites = st.controls(len(IDX), S, T), st.starts(IDX, S), tracked_sites(st)
    clean = simulate_all(st, every=1, ctrl=ctrl, start=start, sites=sites)
    bad = tuple(x.copy() for x in start)
    bad[1][1, 1, 3] = 1e12
    bad[1][2, 0, 30] = np.nan
    before = st.snapshot()
    got = simulate_all(st, every=1, ctrl=ctrl, start=bad, sites=sites)
    for p, q in zip(before, st.snapshot()):
        assert np.array_equal(p, q)
    exp = np.zeros((len(IDX), S), np.int32)
    exp[1, 1] = exp[2, 0] = 1
    assert np.array_equal(got["bad"], exp), got["bad"]
    assert np.array_equal(got["steps"], np.where(exp == 1, 0, T)), got["steps"]
    for key in ("qpos", "qvel", "act", "time", "site_xpos"):
        assert np.isnan(got[key][exp == 1]).all(), key
        assert np.isfinite(got[key][exp == 0]).all() and np.array_equal(got[key][exp == 0], clean[key][exp == 0]), key
    # a velocity under the check's 1e10 that the first step turns into a state beyond it: the sample completes no step either, but
    # with every = 2 and a blow-up in the second step the first recorded row would be kept: rows follow steps // every
    late = tuple(x.copy() for x in start)
    late[1][0, 2, 3] = 9e9
    got = simulate_all(st, every=1, ctrl=ctrl, start=late, sites=sites)
    n_ok = int(got["steps"][0, 2])
    assert got["bad"][0, 2] == 1 and 0 <= n_ok < T, (got["bad"], got["steps"])
    assert np.isfinite(got["qpos"][0, 2, :n_ok]).all() and np.isnan(got["qpos"][0, 2, n_ok:]).all()
    assert np.isnan(got["time"][0, 2, n_ok:]).all() and np.isnan(got["site_xpos"][0, 2, n_ok:]).all()
    coarse = simulate_all(st, every=2, ctrl=ctrl, start=late, sites=sites)
    assert coarse["steps"][0, 2] == n_ok and np.isnan(coarse["qpos"][0, 2, n_ok // 2:]).all() and np.isfinite(coarse["qpos"][0, 2, :n_ok // 2]).all()
    others = np.ones((len(IDX), S), bool)
    others[0, 2] = False
    assert (got["bad"][others] == 0).all() and np.array_equal(got["qpos"][others], clean["qpos"][others])
    # an env index outside the batch: its samples are NaN / bad, the others the clean bits
    out = simulate_all(st, idx=[2, 7, -1], every=1, ctrl=ctrl, start=start, sites=sites)
    assert (out["bad"][1:] == 1).all() and (out["steps"][1:] == 0).all() and np.isnan(out["qpos"][1:]).all() and np.isnan(out["site_xpos"][1:]).all()
    assert np.array_equal(out["qpos"][0], clean["qpos"][0]) and (out["bad"][0] == 0).all()
    # a site id outside the model: NaN in its column alone
    odd = simulate_all(st, every=1, ctrl=ctrl, start=start, sites=[sites[0], len(st.cm.names["site"]) + 2, sites[1], -1])
    assert np.isnan(odd["site_xpos"][:, :, :, [1, 3]]).all() and np.array_equal(odd["site_xpos"][:, :, :, [0, 2]], clean["site_xpos"][:, :, :, :2])
    st.close()


# ---------------------------------------------------------------------------------------------------------------- 6. arguments and ABI
def header_struct_fields(name):
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "myobatch.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [x.strip().lstrip("*").strip() for x in re.sub(r"^(const\s+)?[A-Za-z_0-9]+\s*\*?", "", decl, count=1).split(",")]
    return fields


def case_bad_args(lib):
    """the binding mirrors the header's structs; struct sizes of another version, NULLs and bad scalars are refused with their error
    text before any device call (MYO_E_BADARG = MYO_E_ARG = -1): the filled outputs stay untouched; all-NULL outputs launch nothing"""
    si, so = C.sizeof(native.SimIn), C.sizeof(native.SimOut)
    assert si == 96 and so == 64
    assert header_struct_fields("myo_sim_in") == [f[0] for f in native.SimIn._fields_]
    assert header_struct_fields("myo_sim_out") == [f[0] for f in native.SimOut._fields_]
    off = {f[0]: getattr(native.SimIn, f[0]).offset for f in native.SimIn._fields_}
    assert [off[x] for x in ("size", "env_idx", "k", "S", "T", "nsub", "every", "ctrl", "ctrl_per_sample", "qpos0", "qvel0", "act0", "site_ids", "ns")] == \
        [0, 8, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88]
    assert [getattr(native.SimOut, f[0]).offset for f in native.SimOut._fields_] == list(range(0, 64, 8))
    assert "myo_batch_simulate" in native.EXPORTED_SYMBOLS and "myo_batch_simulate" in native.ENV_PATH_SYMBOLS and native.SIM_NS_MAX == 16
    from myochallenge_amd import build
    assert "myo_simulate.h" in build.SOURCES
    mem = Mem(lib)
    b = sc.baoding_batch(lib, mem, native.MYO_MIXED, 2, 0, 0)
    nq, L, P = b.model.size("nq"), lib.L, native._ptr
    q = mem.arr(np.full((2, 1, 2, nq), 7.5))
    ids = mem.arr([0, 1], np.int32)
    sx = mem.arr(np.full((2, 1, 2, 2, 3), 7.5))
    i, o = native.SimIn(), native.SimOut()
    i.size, i.k, i.S, i.T, i.nsub, i.every = si, 2, 1, 2, 1, 1
    o.size, o.qpos = so, P(q)
    call = lambda bb=b.h, ii=i, oo=o: L.myo_batch_simulate(bb, None if ii is None else C.byref(ii), None if oo is None else C.byref(oo), None)
    err = lambda: L.myo_last_error()
    for size in (0, si - 8, si + 8):
        i.size = size
        assert call() == -1 and b"myo_sim_in.size" in err()
    i.size = si
    for size in (0, so - 8, so + 8):
        o.size = size
        assert call() == -1 and b"myo_sim_out.size" in err()
    o.size = so
    assert call(bb=None) == -1 and call(ii=None) == -1 and call(oo=None) == -1 and b"null" in err()
    for field, values, text in (("k", (-1,), b"k must be >= 0"), ("S", (0, -2), b"S and T >= 1"), ("T", (0, -1), b"S and T >= 1"), ("nsub", (-1,), b"nsub must be >= 0"),
                                ("every", (0, -1), b"every must be >= 1 and divide T"), ("ns", (-1, native.SIM_NS_MAX + 1), b"ns must be in [0, 16]")):
        keep = getattr(i, field)
        for v in values:
            setattr(i, field, v)
            assert call() == -1 and text in err(), (field, v, err())
        setattr(i, field, keep)
    i.T, i.every = 5, 2                                        # T % every != 0
    assert call() == -1 and b"every must be >= 1 and divide T, got T = 5, every = 2" in err()
    i.T, i.every = 2, 1
    i.k = 3                                                    # all envs in order: no more than the batch has
    assert call() == -1 and b"env_idx is NULL with k = 3 beyond the batch's 2 envs" in err()
    i.k, i.S = 1 << 20, 1 << 12                                # k S beyond an int
    i.env_idx = P(ids)
    assert call() == -1 and b"exceeds 2^31 - 1" in err()
    i.k, i.S, i.env_idx = 2, 1, None
    o.site_xpos, i.ns = P(sx), 2                               # site outputs without site_ids
    assert call() == -1 and b"site_ids is NULL with ns = 2" in err()
    o.site_xpos, i.ns = None, 0
    assert (mem.host(q) == 7.5).all()
    none = native.SimOut()
    none.size = so
    i.every = 0
    assert call(oo=none) == -1                                 # (the scalars are checked whatever the outputs)
    i.every = 1
    assert call(oo=none) == 0 and (mem.host(q) == 7.5).all()   # all NULL: nothing is launched
    i.k = 0
    assert call() == 0 and (mem.host(q) == 7.5).all()          # k = 0: an empty call
    i.k = 2
    assert call() == 0 and np.isfinite(mem.host(q)).all() and not (mem.host(q) == 7.5).any()
    with np.testing.assert_raises(KeyError):
        b.simulate(2, 1, 2, no_such_key=q)
    assert b.health() == HEALTHY
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 8. the large call (GPU)
def case_large(lib, n=256, s=16, t=8):
    """256 envs x 16 samples x 8 steps on the fp64 stepper: 4096 workgroups, more than one round of the device; finite and healthy, and
    the first envs' first samples are a small call's, bit for bit (what an indexing error would break)"""
    st = Setup(lib, F64, "hand", n=n, nsteps=2)
    ctrl = st.controls(n, s, t)
    got = simulate_all(st, idx=None, s=s, t=t, nsub=1, every=4, ctrl=ctrl, sites=tracked_sites(st))
    assert (got["bad"] == 0).all() and (got["steps"] == t).all()
    for key in ("qpos", "qvel", "act", "time", "site_xpos"):
        assert np.isfinite(got[key]).all(), key
    assert st.b.health() == HEALTHY
    small = simulate_all(st, idx=[0, n - 1], s=2, t=t, nsub=1, every=4, ctrl=ctrl[[0, n - 1], :2], sites=tracked_sites(st))
    for key in small:
        assert np.array_equal(small[key], got[key][[0, n - 1], :2]), key
    st.close()


def case_graph(lib, dtype=F64):
    """one call captured in a graph after a warm-up call has sized the workspace: the replay gives the eager bits; a capture that would
    have to grow the workspace is refused"""
    import torch
    st = Setup(lib, dtype, "hand")
    mem, b, om = st.mem, st.b, st.om
    k, r = len(IDX), T // EVERY
    ctrl, idx = mem.arr(st.controls(k, S, T)), mem.arr(IDX, np.int32)
    sh = b.simulate_shapes(S, r)
    mk = lambda: {key: mem.arr(np.full((k,) + sh[key][0], -7), sh[key][1]) for key in ("qpos", "qvel", "act", "time", "bad", "steps")}
    eager, replay = mk(), mk()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        b.simulate(k, S, T, ctrl, True, idx, NSUB, EVERY, None, None, None, None, stream.cuda_stream, **eager)      # sizes the workspace
    stream.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        b.simulate(k, S, T, ctrl, True, idx, NSUB, EVERY, None, None, None, None, torch.cuda.current_stream().cuda_stream, **replay)
    torch.cuda.synchronize()
    assert (mem.host(replay["qpos"]) == -7).all()      # (captured, not run)
    b.bind_constants()
    g.replay()
    torch.cuda.synchronize()
    for key in eager:
        assert np.array_equal(mem.host(eager[key]), mem.host(replay[key])), key
    assert (mem.host(replay["bad"]) == 0).all()
    # a bigger call inside a capture: refused with its text, and the capture itself survives
    big = {key: mem.arr(np.full((k,) + b.simulate_shapes(4 * S, r)[key][0], -7.0)) for key in ("qpos",)}
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=stream):
        with np.testing.assert_raises(native.MyoError) as cm:
            b.simulate(k, 4 * S, T, None, False, idx, NSUB, EVERY, None, None, None, None, torch.cuda.current_stream().cuda_stream, **big)
        b.simulate(k, S, T, ctrl, True, idx, NSUB, EVERY, None, None, None, None, torch.cuda.current_stream().cuda_stream, **replay)
    assert "capturing" in str(cm.exception)
    torch.cuda.synchronize()
    assert b.health() == HEALTHY
    st.close()
