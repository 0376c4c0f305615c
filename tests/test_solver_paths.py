"""Every linear-solver path of the stepper on a zoo of dof trees (tests/solver_zoo.py) against long-double references
(tests/solver_ref.py: the bounds and the measured ratios are there).

A substep solves M x = f, (M + h B) x = f and (M + J'DJ) x = b with code chosen per model by host tables (csrc/myo_host.h:
build_arrow_tables, build_ldl_tables) and per dtype.  The census below pins which tree takes which path — a change of the table
builders that silently re-routes a model fails it — and the diagnostic switches MYO_DENSE_NEWTON / MYO_DENSE_MSOLVE (read when a model
is created) run every tree down the dense paths as well.  Each case is a function of `lib`: the lane-serial emulation build on the CPU,
the HIP library under -m gpu."""
import os
from unittest import mock

import numpy as np
import pytest

import solver_ref as sr
import solver_zoo as sz
from helpers import Mem, rel_err
from myochallenge_amd import native
from oracle.oracle import OracleData
from sensor_cases import HEALTHY

F64, MIXED = native.MYO_F64, native.MYO_MIXED
DTYPES = [F64, MIXED]
DT_NAME = {F64: "f64", MIXED: "mixed"}
EPS = {F64: sr.EPS64, MIXED: sr.EPS32}
TOL = {F64: 1e-9, MIXED: 1e-4}
SWITCHES = {"none": (), "dense_newton": ("MYO_DENSE_NEWTON",), "dense_msolve": ("MYO_DENSE_MSOLVE",),
            "both": ("MYO_DENSE_NEWTON", "MYO_DENSE_MSOLVE")}
# capacities of the stepper the census speaks of (csrc/myo_model_dev.h, csrc/myo_physics.h)
NV_MAX, ARROW_S, ARROW_B, ARROW_NF, LD_SQ, CHOL_SMALL = 36, 16, 4, 5, 8, 24

_MODELS, _REFS = {}, {}


def model_for(lib, name, switch):
    """native.Model of a zoo member, created once per (library, switch) with the switch's variables in the environment"""
    key = (lib.is_emulation, name, switch)
    if key not in _MODELS:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES["both"]}
        env.update({k: "1" for k in SWITCHES[switch]})
        with mock.patch.dict(os.environ, env, clear=True):
            _MODELS[key] = native.Model(sz.zoo(name)["cm"], lib)
    return _MODELS[key]


def refs(name, warm=None, tag="cold"):
    """the oracle's forward pass at the model's three states (warm: qacc_warmstart [3, nv]), computed once"""
    if (name, tag) not in _REFS:
        z, (qp, qv, act) = sz.zoo(name), sz.states(name)
        _REFS[(name, tag)] = [sr.Ref(z["cm"], z["om"], qp[e], qv[e], act[e], None if warm is None else warm[e]) for e in range(sz.N_ENV)]
    return _REFS[(name, tag)]


def batch_for(lib, mem, name, dtype, switch, warm=None):
    qp, qv, act = sz.states(name)
    b = native.Batch(model_for(lib, name, switch), None, sz.N_ENV, 0, 0, dtype)
    b.set_state(mem.arr(qp), mem.arr(qv), mem.arr(act), mem.zeros(sz.N_ENV))
    b.warmstart(None, mem.arr(np.zeros_like(qv) if warm is None else warm))
    return b


def forward(b, mem):
    """{qacc_smooth, qacc: [N, nv], counts: [N, 4] = ncon, nefc, solver iterations, joint-limit rows} of the envs' present states"""
    out = mem.zeros((b.n, b.dump_size))
    b.forward_dump(None, out)
    res, nv = mem.host(out), b.model.size("nv")
    get = lambda k, n: res[:, b.dump_offset(k):b.dump_offset(k) + n].copy()
    return {"qacc_smooth": get("qacc_smooth", nv), "qacc": get("qacc", nv), "counts": get("counts", 4).astype(int)}


def constraint_force(b, mem, qacc):
    out = mem.arr(np.full(qacc.shape, np.nan))
    b.inverse(mem.arr(qacc), None, out)
    fc = mem.host(out).copy()
    assert not np.isnan(fc).any()
    return fc


def dof_tree(name):
    """subtree sizes of the dofs and the candidate leaf blocks (maximal subtrees of <= ARROW_B dofs), as build_arrow_tables defines them"""
    par = np.asarray(sz.zoo(name)["cm"].fields["dof_parentid"])
    size = np.ones(len(par), int)
    for d in range(len(par) - 1, -1, -1):
        if par[d] >= 0:
            size[par[d]] += size[d]
    blocks = [int(size[d]) for d in range(len(par)) if size[d] <= ARROW_B and (par[d] < 0 or size[par[d]] > ARROW_B)]
    return size, blocks


# ---------------------------------------------------------------------------------------------------------------- 1. census
def case_census(lib):
    S = {n: {k: model_for(lib, n, "none").size(k) for k in ("nv", "nM", "nlead", "arrow_nf", "ld_nfq", "ld_nsq")} for n in sz.NAMES}
    for n, s in S.items():
        print(f"    {n:11s} " + " ".join(f"{k} {v:3d}" for k, v in s.items()))
    # the L'DL tables are host tables of both builds
    assert {n: (s["ld_nfq"], s["ld_nsq"]) for n, s in S.items()} == {
        "full36": (6, 5), "comb6": (6, 5), "ragged": (5, 5), "two_blocks": (4, 4), "deep": (8, 7), "sep16": (8, 7), "sep17": (10, 8),
        "two_hands": (4, 4), "chain18": (0, -1), "chain12": (0, -1), "hand": (8, 6), "die": (8, 6)}
    assert {n: (s["nv"], s["nlead"]) for n, s in S.items()} == {
        "full36": (36, 24), "comb6": (24, 24), "ragged": (16, 16), "two_blocks": (9, 9), "deep": (20, 20), "sep16": (28, 16), "sep17": (29, 17),
        "two_hands": (32, 26), "chain18": (18, 18), "chain12": (12, 12), "hand": (35, 23), "die": (29, 23)}
    assert S["full36"]["nv"] == NV_MAX                                                        # nv == MYO_NV_MAX
    assert S["sep17"]["ld_nsq"] == LD_SQ                                                      # the last substitution chunk in use
    assert S["chain18"]["ld_nsq"] == S["chain12"]["ld_nsq"] == -1 and S["chain18"]["nM"] == 171 < 255      # the tables overflow: dense M solve, no switch
    assert S["full36"]["nlead"] == CHOL_SMALL < S["full36"]["nv"]                             # the 24-wide factorisation plus division rows, at its widest
    assert CHOL_SMALL < S["two_hands"]["nlead"] < S["two_hands"]["nv"]                        # a leading block too wide for it
    if lib.is_emulation:
        assert all(s["arrow_nf"] == 0 for s in S.values())                                    # the emulation factors H densely
    else:
        assert {n: s["arrow_nf"] for n, s in S.items()} == {"full36": 5, "comb6": 5, "ragged": 5, "two_blocks": 2, "deep": 3, "sep16": 3, "sep17": 0,
                                                            "two_hands": 5, "chain18": 0, "chain12": 0, "hand": 5, "die": 5}
    # what the trees are, from their dof tables: the arrow's edges
    blocks = {n: dof_tree(n)[1] for n in sz.TREES}
    assert sorted(blocks["ragged"]) == [1, 2, 3, 4, 4]                                        # kept blocks of fewer than 4 dofs: padded rows
    assert len(blocks["comb6"]) == 6 > ARROW_NF                                               # more candidate blocks than MYO_ARROW_NF
    assert blocks["deep"] == [4, 4, 4] and S["deep"]["nv"] == 20                              # blocks are the ends of longer chains
    # separator rows = dofs outside the kept blocks: the largest MYO_ARROW_NF of the fingers' (the last 4 dofs of a free ball are a
    # candidate too, the last in dof order, but every finger touches the balls: they are never kept)
    nfree = lambda n: int((np.asarray(sz.zoo(n)["cm"].fields["jnt_type"]) == 0).sum())
    hinge_blocks = lambda n: sorted(blocks[n][:len(blocks[n]) - nfree(n)], reverse=True)
    nsep = {n: S[n]["nv"] - sum(hinge_blocks(n)[:ARROW_NF]) for n in ("full36", "sep16", "sep17")}
    assert nsep == {"full36": ARROW_S, "sep16": ARROW_S, "sep17": ARROW_S + 1}, nsep          # exactly 16 separator rows, and one more
    assert 17 <= S["sep17"]["nv"] <= 32                                                       # arrow_nf == 0 with 2 .. 3 MFMA tiles of dense H
    # the switches
    for n in sz.NAMES:
        assert model_for(lib, n, "dense_newton").size("arrow_nf") == 0, n
        assert model_for(lib, n, "dense_newton").size("ld_nsq") == S[n]["ld_nsq"], n
        assert model_for(lib, n, "dense_msolve").size("ld_nsq") == -1 and model_for(lib, n, "dense_msolve").size("ld_nfq") == 0, n
        assert model_for(lib, n, "dense_msolve").size("arrow_nf") == S[n]["arrow_nf"], n
        both = model_for(lib, n, "both")
        assert (both.size("arrow_nf"), both.size("ld_nsq")) == (0, -1), n


def case_states(name):
    """the states are what the module says: limits violated at both ends, an env without and one with >= 2 contacts, and the oracle's
    own solution meets the stop rule everywhere (it did not run into its iteration cap)"""
    z, (qp, qv, act), R = sz.zoo(name), sz.states(name), refs(name)
    f = z["cm"].fields
    hinge = np.asarray(f["jnt_type"]) == 3
    q = qp[:, np.asarray(f["jnt_qposadr"])[hinge]]
    rg = np.asarray(f["jnt_range"], float).reshape(-1, 2)[hinge]
    assert (q < rg[:, 0]).any() and (q > rg[:, 1]).any()
    ncon = [r.ncon for r in R]
    print(f"    {name}: ncon {ncon} limit rows {[r.nl for r in R]} cond2(M) {R[0].cond_M:.2e} cond2(M + hB) {R[0].cond_Mh:.2e} stop {R[0].stop:.2e}")
    assert min(ncon) == 0 and max(ncon) >= 2, ncon
    assert sum(r.nl for r in R) > 0
    for r in R:
        assert r.d.solver_iter < z["om"].iterations


# ---------------------------------------------------------------------------------------------------------------- 2. references
def newton_checks(lib, mem, b, R, fw, dtype, label):
    backend, dt = ("emu" if lib.is_emulation else "gpu"), DT_NAME[dtype]
    kept = 0
    for e, r in enumerate(R):
        assert tuple(fw["counts"][e][[0, 1, 3]]) == (r.ncon, r.nefc, r.nl), (label, e, fw["counts"][e], r.ncon, r.nefc, r.nl)
        err = rel_err(fw["qacc"][e], r.qacc)
        sr.record(backend, dt, "qacc / tol", err / TOL[dtype])
        assert err < TOL[dtype], (label, e, "qacc", err)
    both = np.stack([fw["qacc"], np.stack([r.qacc for r in R])])
    fc = [constraint_force(b, mem, q) for q in both]
    for e, r in enumerate(R):
        k_or, b_or = r.kkt(both[1][e], fc[1][e]), r.kkt_bound(EPS[dtype], both[1][e])
        if k_or > b_or:          # the oracle's own solution does not meet the stop rule here: no test
            continue
        kept += 1
        k, bound = r.kkt(both[0][e], fc[0][e]), r.kkt_bound(EPS[dtype], both[0][e])
        print(f"    {label} env {e}: nefc {r.nefc:3d} |r|_2 {k:.3e} (oracle's qacc {k_or:.3e}) bound {bound:.3e}")
        sr.record(backend, dt, "kkt / bound", k / bound)
        assert k <= bound, (label, e, "kkt", k, bound)
    assert kept == len(R), (label, "states dropped by the oracle's own residual", len(R) - kept)


def case_references(lib, name, dtype, switch):
    mem = Mem(lib)
    backend, dt, eps = ("emu" if lib.is_emulation else "gpu"), DT_NAME[dtype], EPS[dtype]
    R = refs(name)
    label = f"{name} {dt} {switch}"
    b = batch_for(lib, mem, name, dtype, switch)
    fw = forward(b, mem)
    # M solve
    for e, r in enumerate(R):
        err, bound = np.abs(fw["qacc_smooth"][e] - r.ref_smooth).max(), r.msolve_bound(eps)
        unit = eps * r.cond_M * np.abs(r.ref_smooth).max()
        print(f"    {label} env {e}: M solve err {err:.3e} = {err / unit:.3g} eps cond |ref|, bound {bound:.3e}")
        sr.record(backend, dt, "msolve / (eps cond)", err / unit)
        sr.record(backend, dt, "msolve / bound", err / bound)
        assert err <= bound, (label, e, "M solve", err, bound)
        assert rel_err(r.ref_smooth, r.qacc_smooth) < 1e-9                 # the reference and the oracle's own solve agree
    # Newton solve
    newton_checks(lib, mem, b, R, fw, dtype, label)
    # damped solve: one Euler substep
    b.physics_step(None, 1)
    qv = mem.zeros((b.n, b.model.size("nv")))
    b.get_state(None, qv)
    qv = mem.host(qv)
    for e, r in enumerate(R):
        err, bound = np.abs(qv[e] - r.ref_qvel).max(), r.damped_bound(eps)
        unit = r.h * eps * r.cond_Mh * np.abs(r.x_damped).max()
        print(f"    {label} env {e}: damped solve err {err:.3e} = {err / unit:.3g} h eps cond |x|, bound {bound:.3e}")
        sr.record(backend, dt, "damped / (h eps cond)", err / unit)
        sr.record(backend, dt, "damped / bound", err / bound)
        assert err <= bound, (label, e, "damped solve", err, bound)
    assert b.health() == HEALTHY
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 3. cross-path
def case_cross_path(lib, name, dtype):
    mem = Mem(lib)
    backend, dt = ("emu" if lib.is_emulation else "gpu"), DT_NAME[dtype]
    res = {}
    for switch in ("none", "dense_newton", "dense_msolve"):
        b = batch_for(lib, mem, name, dtype, switch)
        res[switch] = forward(b, mem)
        b.close()
    for switch in ("dense_newton", "dense_msolve"):
        assert np.array_equal(res[switch]["counts"][:, [0, 1, 3]], res["none"]["counts"][:, [0, 1, 3]]), (name, switch)
        for k in ("qacc_smooth", "qacc"):
            for e in range(sz.N_ENV):
                err = rel_err(res[switch][k][e], res["none"][k][e])
                sr.record(backend, dt, "cross-path rel_err", err)
                assert err < TOL[dtype], (name, switch, k, e, err)
    print(f"    {name} {dt}: cross-path worst so far {sr.WORST[(backend, dt, 'cross-path rel_err')]:.3e}")


# ---------------------------------------------------------------------------------------------------------------- 4. twenty substeps
def oracle_steps(name, nsteps):
    key = (name, "steps", nsteps)
    if key not in _REFS:
        z, (qp, qv, act) = sz.zoo(name), sz.states(name)
        out = []
        for e in range(sz.N_ENV):
            d = OracleData(z["om"])
            d.reset()
            d.qpos[:], d.qvel[:], d.act[:] = qp[e], qv[e], act[e]
            d.ctrl[:] = 0
            d.step()
            v1 = np.array(d.qvel)
            for _ in range(nsteps - 1):
                d.step()
            assert not d.bad
            out.append((v1, np.array(d.qpos)))
        _REFS[key] = out
    return _REFS[key]


def case_substeps(lib, name, dtype, switch, nsteps=20):
    """fp64: qpos after 20 substeps against the oracle at 1e-8; mixed: the first substep's qvel at 1e-4 (its drift is not pinned here)"""
    mem = Mem(lib)
    ref = oracle_steps(name, nsteps)
    b = batch_for(lib, mem, name, dtype, switch)
    nq, nv = b.model.size("nq"), b.model.size("nv")
    qp, qv = mem.zeros((b.n, nq)), mem.zeros((b.n, nv))
    if dtype == MIXED:
        b.physics_step(None, 1)
        b.get_state(None, qv)
        for e in range(b.n):
            err = rel_err(mem.host(qv)[e], ref[e][0])
            assert err < 1e-4, (name, switch, e, err)
    else:
        for _ in range(nsteps):
            b.physics_step(None, 1)
        b.get_state(qp, None)
        for e in range(b.n):
            err = rel_err(mem.host(qp)[e], ref[e][1])
            print(f"    {name} {switch} env {e}: qpos after {nsteps} substeps rel_err {err:.3e}")
            sr.record("emu" if lib.is_emulation else "gpu", "f64", "20 substeps / 1e-8", err / 1e-8)
            assert err < 1e-8, (name, switch, e, err)
    assert b.health() == HEALTHY
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. warm start
def case_warm_start(lib, name, dtype):
    """the Newton checks with qacc_warmstart = the solved qacc of the state (what the previous substep leaves) and with zeros.  Which
    starting point the solver takes is its own choice (newton_solve: the cheaper of qacc_warmstart and qacc_smooth); solver_ref.Ref.uses_warm
    evaluates the same two costs from the oracle's rows, and the zoo is asserted to contain both outcomes (test_warm_start_branches)."""
    mem = Mem(lib)
    cold = refs(name)
    prev = np.stack([r.qacc for r in cold])
    for tag, warm in (("warm", prev), ("zero", np.zeros_like(prev))):
        R = refs(name, warm, tag)
        b = batch_for(lib, mem, name, dtype, "none", warm)
        newton_checks(lib, mem, b, R, forward(b, mem), dtype, f"{name} {DT_NAME[dtype]} start={tag}")
        b.close()


def test_warm_start_branches():
    took = {}
    for name in sz.NAMES:
        cold = refs(name)
        for r in cold:
            if r.nefc:
                took.setdefault(name, set()).update({("warm", bool(r.uses_warm(r.qacc))), ("zero", bool(r.uses_warm(np.zeros(r.nv))))})
    print("    starting point taken:", {n: sorted(t) for n, t in took.items()})
    for name in sz.NAMES:
        assert ("warm", True) in took[name], name               # the solved qacc is never dearer than qacc_smooth where a row is active
    assert any(("zero", False) in t for t in took.values()) and any(("zero", True) in t for t in took.values())


# ---------------------------------------------------------------------------------------------------------------- tests
def report(lib):
    backend = "emu" if lib.is_emulation else "gpu"
    for (bk, dt, kind), v in sorted(sr.WORST.items()):
        if bk == backend:
            print(f"    worst so far [{bk} {dt}] {kind}: {v:.3e}")


@pytest.mark.parametrize("name", sz.NAMES)
def test_zoo_states(name):
    case_states(name)


def test_conditioning():
    """one synthetic tree at least is as ill-conditioned as the synthetic hand (within a factor 10); cond_2(M) of every member is printed"""
    cond = {n: max(r.cond_M for r in refs(n)) for n in sz.NAMES}
    print("    cond2(M):", {n: f"{c:.2e}" for n, c in cond.items()})
    assert any(cond["hand"] / 10 <= cond[n] <= cond["hand"] * 10 for n in sz.TREES)


def test_census_on_emulation(emu_lib):
    case_census(emu_lib)


@pytest.mark.gpu
def test_census_on_gpu(hip_lib):
    case_census(hip_lib)


@pytest.mark.parametrize("switch", ["none", "dense_newton", "dense_msolve"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("name", sz.NAMES)
def test_references_on_emulation(emu_lib, name, dtype, switch):
    case_references(emu_lib, name, dtype, switch)
    report(emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["none", "dense_newton", "dense_msolve"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("name", sz.NAMES)
def test_references_on_gpu(hip_lib, name, dtype, switch):
    case_references(hip_lib, name, dtype, switch)
    report(hip_lib)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("name", sz.NAMES)
def test_cross_path_on_emulation(emu_lib, name, dtype):
    case_cross_path(emu_lib, name, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("name", sz.NAMES)
def test_cross_path_on_gpu(hip_lib, name, dtype):
    case_cross_path(hip_lib, name, dtype)


@pytest.mark.parametrize("switch", ["none", "both"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("name", sz.NAMES)
def test_substeps_on_emulation(emu_lib, name, dtype, switch):
    case_substeps(emu_lib, name, dtype, switch)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["none", "both"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("name", sz.NAMES)
def test_substeps_on_gpu(hip_lib, name, dtype, switch):
    case_substeps(hip_lib, name, dtype, switch)
    report(hip_lib)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("name", sz.NAMES)
def test_warm_start_on_emulation(emu_lib, name, dtype):
    case_warm_start(emu_lib, name, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_NAME.get)
@pytest.mark.parametrize("name", sz.NAMES)
def test_warm_start_on_gpu(hip_lib, name, dtype):
    case_warm_start(hip_lib, name, dtype)
    report(hip_lib)
