"""Tendon drawing (include/myobatch.h myo_batch_tendon_paths, MYO_RENDER_TENDONS; csrc/myo_render.h): the path items against the
pinned oracle's tendon lengths and against closed forms, the colour rule, the image against the numpy yardstick tests/render_ref.py,
"off means off", and the arguments / Python surface — on the emulation build here, on the MI355X under -m gpu.

Bounds.  Lengths: the project's fp64 parity bound 1e-9 m for fp64 batches; for mixed batches 1e-6 m, the bound tests/test_render.py
applies to pose-pass positions it compares with fp32 data (its Baoding target check).  Geometry: 1e-12 m for positions the pose pass
also writes, 1e-9 for the wrap solver's tangent points (the parity bound).  The 24-double item holds a piece as midpoint, unit axis
and half length, not as its two end points, so "consecutive pieces share an end point" is checked on the end points reconstructed
as mid -/+ half * axis: bit equality is not defined for them, and the bound is the rounding of that reconstruction, 16 eps (|mid| +
half) (four rounded operations on either side), ~1e-16 m here — far below anything a recomputed point would give (the wrap solver's own
rounding is ~1e-13)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as rr  # noqa: E402
from helpers import Mem  # noqa: E402
from test_render import decode_png  # noqa: E402

from myochallenge_amd import native  # noqa: E402

N = native.RENDER_ITEM_N
ACTIVE = np.array([1.00, 0.90, 0.10])                                   # include/myobatch.h: the "active" colour
DERIVED_RGBA, DERIVED_RADIUS = np.array([0.30, 0.35, 0.75, 1.0], np.float32), np.float32(0.002)      # models without visual data
LEN_TOL = {native.MYO_F64: 1e-9, native.MYO_MIXED: 1e-6}
WRAP_SITE, WRAP_SPHERE, WRAP_CYLINDER, WRAP_PULLEY = 3, 4, 5, 2
_MODELS, _RUNS = {}, {}


# ------------------------------------------------------------------------------------------------ models, states, path elements
def _model(name, golden_dir):
    """-> (compiled model, .mjb path or None, mjb model or None), compiled once"""
    if name not in _MODELS:
        from myochallenge_amd.model import compile_model
        if name == "hand":
            from myochallenge_amd.synth_hand import synthetic_hand
            _MODELS[name] = (compile_model(synthetic_hand()), None, None)
        else:
            from myochallenge_amd.mjb import load_mjb
            path = os.path.join(golden_dir, name + ".mjb")
            mj = load_mjb(path)
            _MODELS[name] = (compile_model(mj, unsupported_contacts="drop"), path, mj)
    return _MODELS[name]


def _states(cm, count=4, seed=7):
    """qpos0, then `count` seeded joint states inside jnt_range (hinge / slide joints; free joints stay at qpos0)"""
    rng = np.random.RandomState(seed)
    q0 = np.asarray(cm.qpos0, float).copy()
    rngs = np.asarray(cm.jnt_range, float).reshape(-1, 2)
    out = [q0]
    for _ in range(count):
        q = q0.copy()
        for j, ty in enumerate(cm.jnt_type):
            if ty in (2, 3) and rngs[j, 1] > rngs[j, 0]:
                q[cm.jnt_qposadr[j]] = rng.uniform(rngs[j, 0], rngs[j, 1])
        out.append(q)
    return out


def _elements(cm):
    """the walk along every tendon: (tendon, wrap index of the first site, of the last site, of the wrap geom or -1, divisor, item slot)"""
    els, slot = [], 0
    for t in range(cm.size("ntendon")):
        adr, num, div, j = int(cm.tendon_adr[t]), int(cm.tendon_num[t]), 1.0, 0
        while j < num - 1:
            t0, t1 = int(cm.wrap_type[adr + j]), int(cm.wrap_type[adr + j + 1])
            if t0 == WRAP_PULLEY or t1 == WRAP_PULLEY:
                if t0 == WRAP_PULLEY:
                    div = float(cm.wrap_prm[adr + j])
                j += 1
                continue
            geom = t1 in (WRAP_SPHERE, WRAP_CYLINDER)
            end = j + (2 if geom else 1)
            els.append((t, adr + j, adr + end, adr + j + 1 if geom else -1, div, slot))
            slot += 3 if geom else 1
            j = end
    return els, slot


def _ends(it):
    """the two end points of a capsule item, reconstructed"""
    z = it[3:12].reshape(3, 3)[:, 2]
    return it[0:3] - it[13] * z, it[0:3] + it[13] * z


def _run(lib, name, golden_dir, dtype, route="compiled"):
    """pose-pass items and path items of every state of _states (2 envs per call), computed once per (library, model, dtype, route)"""
    key = (lib.is_emulation, name, dtype, route)
    if key in _RUNS:
        return _RUNS[key]
    cm, path, _ = _model(name, golden_dir)
    mem = Mem(lib)
    m = native.Model.from_mjb(path, lib) if route == "mjb" else native.Model(cm, lib)
    b = native.Batch(m, None, 2, 0, 0, dtype)
    nit, nti = m.size("ngeom") + m.size("nsite"), m.size("ntendon_item")
    assert nti == _elements(cm)[1]
    states = _states(cm)
    idx = mem.arr(np.arange(2), np.int32)
    poses, paths = [], []
    for i in range(0, len(states), 2):
        pair = [states[i], states[(i + 1) % len(states)]]
        b.set_state(mem.arr(pair), mem.zeros((2, cm.size("nv"))), mem.zeros((2, cm.size("na"))), mem.zeros(2))
        po, pa = mem.zeros((2, nit, N)), mem.arr(np.full((2, nti, N), 7.0))
        b.geom_poses(idx, po)
        b.tendon_paths(idx, pa)
        poses += list(mem.host(po).copy())
        paths += list(mem.host(pa).copy())
    b.close()
    _RUNS[key] = (cm, states, poses[:len(states)], paths[:len(states)])
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------ 1. length closure
def _check_lengths(lib, name, golden_dir, dtype):
    from oracle.oracle import OracleData, OracleModel
    cm, states, _, paths = _run(lib, name, golden_dir, dtype)
    d = OracleData(OracleModel(cm.to_blob()))
    nt = cm.size("ntendon")
    els, _ = _elements(cm)
    active = inactive = 0
    for q, it in zip(states, paths):
        d.qpos[:] = q
        d.fwd_position()
        got = np.array([it[it[:, 22] == t + 1, 23].sum() for t in range(nt)])
        err = np.abs(got - d.ten_length).max()
        print(name, dtype, "ten_length closure", err)
        assert err <= LEN_TOL[dtype], (name, dtype, err)
        for (_, _, _, wg, _, slot) in els:
            if wg >= 0:
                used = int((it[slot:slot + 3, 22] > 0).sum())
                assert used in (1, 3)
                active += used == 3
                inactive += used == 1
    if name != "hand":
        _, _, mj = _model(name, golden_dir)
        got0 = np.array([paths[0][paths[0][:, 22] == t + 1, 23].sum() for t in range(nt)])
        assert np.abs(got0 - np.asarray(mj.arrays["tendon_length0"], float)).max() <= LEN_TOL[dtype]      # MuJoCo's own number at qpos0
    assert active >= 1 and inactive >= 1, (name, active, inactive)


@pytest.mark.parametrize("dtype", [native.MYO_F64, native.MYO_MIXED])
@pytest.mark.parametrize("name", ["myo_finger_v0", "hand"])
def test_piece_lengths_sum_to_the_oracles_tendon_lengths(emu_lib, golden_dir, name, dtype):
    _check_lengths(emu_lib, name, golden_dir, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [native.MYO_F64, native.MYO_MIXED])
@pytest.mark.parametrize("name", ["myo_finger_v0", "hand"])
def test_gpu_piece_lengths_sum_to_the_oracles_tendon_lengths(hip_lib, golden_dir, name, dtype):
    _check_lengths(hip_lib, name, golden_dir, dtype)


# ------------------------------------------------------------------------------------------------ 2. geometry, closed forms
def _check_geometry(lib, name, golden_dir):
    cm, states, poses, paths = _run(lib, name, golden_dir, native.MYO_F64)
    ng = cm.size("ngeom")
    els, nslot = _elements(cm)
    eps = np.finfo(float).eps
    nwrapped = 0
    for po, it in zip(poses, paths):
        seen = np.zeros(nslot, bool)
        for (t, w0, we, wg, div, slot) in els:
            x0, x1 = po[ng + int(cm.wrap_objid[w0]), 0:3], po[ng + int(cm.wrap_objid[we]), 0:3]     # the pose pass's site positions
            n_used = 3 if (wg >= 0 and it[slot + 1, 22] > 0) else 1
            pcs = it[slot:slot + n_used]
            seen[slot:slot + (3 if wg >= 0 else 1)] = True
            assert (pcs[:, 22] == t + 1).all() and (pcs[:, 15] == rr.CAPSULE).all() and (pcs[:, 14] == 0).all() and (pcs[:, 21] == 0).all()
            assert np.array_equal(pcs[:, 20], pcs[:, 12] + pcs[:, 13])
            if wg >= 0 and n_used == 1:
                assert not it[slot + 1:slot + 3].any()                                            # an inactive wrap's two unused slots
            ends = [_ends(p) for p in pcs]
            assert np.abs(ends[0][0] - x0).max() <= 1e-12 and np.abs(ends[-1][1] - x1).max() <= 1e-12
            for p, (a, b) in zip(pcs, ends):
                R = p[3:12].reshape(3, 3)
                assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0
            for k in range(n_used - 1):                                                           # consecutive pieces share an end point
                tol = 16 * eps * (np.abs(pcs[k:k + 2, 0:3]).max() + pcs[k:k + 2, 13].max())
                assert np.abs(ends[k][1] - ends[k + 1][0]).max() <= tol, (name, t, k)
            if n_used == 1:                      # half length and axis from the independently known end points (the sites)
                L = np.linalg.norm(x1 - x0)
                assert abs(pcs[0, 13] - 0.5 * L) <= 1e-12 and abs(pcs[0, 23] - L / div) <= 1e-12
                if L > 1e-6:
                    assert np.abs(pcs[0, 3:12].reshape(3, 3)[:, 2] - (x1 - x0) / L).max() <= 2e-12 / L + 4 * eps
                continue
            nwrapped += 1
            g = int(cm.wrap_objid[wg])
            c, Rg, r = po[g, 0:3], po[g, 3:12].reshape(3, 3), po[g, 12]
            p0, p1 = ends[1]                                                                       # the chord's ends: the tangent points
            for p, x, piece, first in ((p0, x0, pcs[0], True), (p1, x1, pcs[2], False)):
                loc = Rg.T @ (p - c)
                if int(cm.wrap_type[wg]) == WRAP_SPHERE:
                    assert abs(np.linalg.norm(loc) - r) <= 1e-9
                    assert abs(np.dot(p - c, p - x)) <= 1e-9 * r * np.linalg.norm(p - x)        # site -> tangent point is tangent
                else:
                    assert abs(np.linalg.norm(loc[:2]) - r) <= 1e-9
                L = np.linalg.norm(p - x)
                assert abs(piece[13] - 0.5 * L) <= 1e-12 and abs(piece[23] - L / div) <= 1e-12
                u = (p - x) / L if first else (x - p) / L
                assert np.abs(piece[3:12].reshape(3, 3)[:, 2] - u).max() <= 2e-12 / L + 4 * eps
            chord = np.linalg.norm(p1 - p0)
            assert abs(pcs[1, 13] - 0.5 * chord) <= 1e-12 and pcs[1, 23] * div >= chord - 1e-12    # the arc is no shorter than its chord
        assert seen.all()
    assert nwrapped >= 1


@pytest.mark.parametrize("name", ["myo_finger_v0", "hand"])
def test_piece_geometry_closed_forms(emu_lib, golden_dir, name):
    _check_geometry(emu_lib, name, golden_dir)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["myo_finger_v0", "hand"])
def test_gpu_piece_geometry_closed_forms(hip_lib, golden_dir, name):
    _check_geometry(hip_lib, name, golden_dir)


def _check_out_of_range_rows(lib, golden_dir):
    cm, _, _, paths = _run(lib, "myo_finger_v0", golden_dir, native.MYO_F64)
    mem = Mem(lib)
    m = native.Model(cm, lib)
    b = native.Batch(m, None, 2, 0, 0, native.MYO_F64)
    out = mem.arr(np.full((4, m.size("ntendon_item"), N), 7.0))
    b.tendon_paths(mem.arr([1, 2, -1, 0], np.int32), out)
    out = mem.host(out)
    assert not out[1].any() and not out[2].any()                      # env 2 of 2 and env -1: all-zero rows
    assert np.array_equal(out[0], paths[0]) and np.array_equal(out[3], paths[0])      # (a fresh batch is at qpos0)
    b.close()


def test_rows_of_an_out_of_range_env_are_zero(emu_lib, golden_dir):
    _check_out_of_range_rows(emu_lib, golden_dir)


@pytest.mark.gpu
def test_gpu_rows_of_an_out_of_range_env_are_zero(hip_lib, golden_dir):
    _check_out_of_range_rows(hip_lib, golden_dir)


# ------------------------------------------------------------------------------------------------ 3. colour rule
def _muscle_of_tendon(cm):
    """tendon -> index of the activation that colours it (the first muscle actuator whose transmission targets it), or -1"""
    nu, na = cm.size("nu"), cm.size("na")
    out = -np.ones(cm.size("ntendon"), int)
    trn = np.asarray(cm.fields["actuator_trnid"]).reshape(nu, 2)
    for i in reversed(range(nu)):
        if i - (nu - na) >= 0 and cm.actuator_dyntype[i] == 3:
            out[trn[i, 0]] = i - (nu - na)
    return out


def _base_colours(name, golden_dir):
    cm, _, mj = _model(name, golden_dir)
    nt = cm.size("ntendon")
    if mj is None:
        return np.tile(DERIVED_RGBA, (nt, 1)).astype(np.float64), np.full(nt, DERIVED_RADIUS, np.float64)
    rgba = np.asarray(mj.arrays["tendon_rgba"], np.float32).reshape(nt, 4).copy()
    mat = np.asarray(mj.arrays["tendon_matid"]).reshape(-1)
    rgba[mat >= 0] = np.asarray(mj.arrays["mat_rgba"], np.float32).reshape(-1, 4)[mat[mat >= 0]]
    rgba[np.asarray(mj.arrays["tendon_group"]).reshape(-1) > 2, 3] = 0
    return rgba.astype(np.float64), np.asarray(mj.arrays["tendon_width"], np.float64)


def _check_colours(lib, name, golden_dir, routes):
    cm, _, _ = _model(name, golden_dir)
    base, width = _base_colours(name, golden_dir)
    mus = _muscle_of_tendon(cm)
    na, nt = cm.size("na"), cm.size("ntendon")
    mem = Mem(lib)
    acts = np.zeros((2, max(na, 1)))
    if na:
        acts[0, :] = np.resize([0.0, 1.0, 0.25], na)
        acts[1, :] = np.resize([1.5, -0.5, 0.25], na)              # beyond [0, 1]: clamped
    results = []
    for route in routes:
        _, path, _ = _model(name, golden_dir)
        m = native.Model.from_mjb(path, lib) if route == "mjb" else native.Model(cm, lib)
        b = native.Batch(m, None, 2, 0, 0, native.MYO_F64)
        b.set_state(mem.arr(np.tile(cm.qpos0, (2, 1))), mem.zeros((2, cm.size("nv"))), mem.arr(acts[:, :na]), mem.zeros(2))
        out = mem.zeros((2, m.size("ntendon_item"), N))
        b.tendon_paths(mem.arr(np.arange(2), np.int32), out)
        out = mem.host(out).copy()
        b.close()
        results.append(out)
        for e in range(2):
            for t in range(nt):
                rows = out[e][out[e][:, 22] == t + 1]
                assert len(rows)
                a = float(np.clip(acts[e, mus[t]], 0, 1)) if mus[t] >= 0 else 0.0
                want = np.append((1 - a) * base[t, :3] + a * ACTIVE, base[t, 3])
                assert np.abs(rows[:, 16:20] - want).max() <= 1e-12, (name, route, e, t)
                assert (rows[:, 12] == np.float32(width[t])).all()
    for r in results[1:]:
        assert np.array_equal(r, results[0])                        # both model routes: the same items to the bit
    return mus


def test_colour_rule_and_visual_data_through_both_model_routes(emu_lib, golden_dir):
    mus = _check_colours(emu_lib, "myo_finger_v0", golden_dir, ("compiled", "mjb"))
    assert (mus >= 0).all() and len(set(mus)) == len(mus)           # five muscles, five tendons: 0, 1, 0.25 all occur
    cm = _model("myo_finger_v0", golden_dir)[0]
    for k in ("tendon_width", "tendon_rgba", "tendon_matid", "tendon_group"):
        assert k in cm.fields
    mus = _check_colours(emu_lib, "motor_finger_v0", golden_dir, ("compiled", "mjb"))
    assert (mus < 0).all()                                           # motors, no muscle: every tendon keeps its base colour
    mus = _check_colours(emu_lib, "hand", golden_dir, ("compiled",))
    assert (mus >= 0).all()
    assert not any(k in _model("hand", golden_dir)[0].fields for k in ("tendon_rgba", "tendon_width"))


@pytest.mark.gpu
def test_gpu_colour_rule(hip_lib, golden_dir):
    _check_colours(hip_lib, "myo_finger_v0", golden_dir, ("compiled", "mjb"))
    _check_colours(hip_lib, "hand", golden_dir, ("compiled",))


# ------------------------------------------------------------------------------------------------ 4. image against the yardstick
# Cameras close enough that the 2 mm tendon radius projects to >= 3 pixels (focal length 0.5 H / tan(fovy / 2) = 116 px at H = 96,
# fovy 45: distance <= 0.077 m), looking at a tendon piece of the state.  EDGE_SHARE: the yardstick's edge mask (silhouettes moved by a
# 0.01 px jitter, depth ties) must leave most of the image to compare — tests/test_render.py states no number; a quarter of the image is
# the bound here, fixed before the library's image was looked at.
W = H = 96
EDGE_SHARE = 0.25
MIN_TENDON_PIXELS = 200


def _close_camera(paths, which, distance, azimuth, elevation):
    rows = paths[paths[:, 22] > 0]
    return {"lookat": tuple(rows[which % len(rows), 0:3]), "distance": distance, "azimuth": azimuth, "elevation": elevation, "fovy": 45.0}


def _check_image(lib, name, golden_dir, cam_args):
    cm, states, poses, paths = _run(lib, name, golden_dir, native.MYO_F64)
    mem = Mem(lib)
    m = native.Model(cm, lib)
    nit = m.size("ngeom") + m.size("nsite")
    b = native.Batch(m, None, 2, 0, 0, native.MYO_F64)
    sel = [1, 2]                                                     # two seeded states
    b.set_state(mem.arr([states[s] for s in sel]), mem.zeros((2, cm.size("nv"))), mem.zeros((2, cm.size("na"))), mem.zeros(2))
    cams = [_close_camera(paths[s], *cam_args) for s in sel]
    rgb, dep, seg = mem.zeros((2, H, W, 3), np.uint8), mem.zeros((2, H, W), np.float32), mem.zeros((2, H, W), np.int32)
    b.render(mem.arr(np.arange(2), np.int32), cams, W, H, 7 | native.RENDER_TENDONS, rgb, dep, seg)
    rgb, dep, seg = mem.host(rgb), mem.host(dep), mem.host(seg)
    b.close()
    for e, s in enumerate(sel):
        items = np.concatenate([poses[s], paths[s]])
        s2, d2, c2, edge = rr.render(items, cams[e], W, H)
        ids = np.where(s2 >= nit, nit + items[np.maximum(s2, 0), 22].astype(int) - 1, s2)       # item index -> tendon id from [22]
        ok = ~edge
        ntp = int((ok & (s2 >= nit)).sum())
        print(name, "env", e, "tendon pixels outside the edge mask", ntp, "edge share", edge.mean())
        assert ntp >= MIN_TENDON_PIXELS and edge.mean() <= EDGE_SHARE
        bad = ok & (ids != seg[e])
        assert not bad.any(), (name, e, int(bad.sum()))
        both = ok & (s2 >= 0)
        d = dep[e].astype(np.float64)
        assert np.all(np.abs(d[both] - d2[both]) <= 1e-5 + 1e-5 * d2[both]), (name, e)
        assert np.isinf(d[ok & (s2 < 0)]).all()
        assert np.abs(rgb[e][ok].astype(int) - c2[ok].astype(int)).max() <= 1, (name, e)


IMAGE_CASES = {"myo_finger_v0": (12, 0.07, 60.0, -20.0), "hand": (60, 0.07, 120.0, -35.0)}


@pytest.mark.parametrize("name", list(IMAGE_CASES))
def test_tendon_image_matches_the_yardstick(emu_lib, golden_dir, name):
    _check_image(emu_lib, name, golden_dir, IMAGE_CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(IMAGE_CASES))
def test_gpu_tendon_image_matches_the_yardstick(hip_lib, golden_dir, name):
    _check_image(hip_lib, name, golden_dir, IMAGE_CASES[name])


# ------------------------------------------------------------------------------------------------ 5. off means off
def test_without_the_flag_the_image_is_what_it_was(emu_lib, golden_dir):
    cm, states, _, _ = _run(emu_lib, "myo_finger_v0", golden_dir, native.MYO_F64)
    m = native.Model(cm, emu_lib)
    b = native.Batch(m, None, 2, 0, 0, native.MYO_F64)
    b.set_state(np.array(states[1:3]), np.zeros((2, cm.size("nv"))), np.full((2, cm.size("na")), 0.5), np.zeros(2))
    idx = np.arange(2, dtype=np.int32)
    cam = [dict(m.default_camera(), distance=0.3)]

    def shot(flags):
        rgb, dep, seg = np.zeros((2, 48, 64, 3), np.uint8), np.zeros((2, 48, 64), np.float32), np.zeros((2, 48, 64), np.int32)
        b.render(idx, cam, 64, 48, flags, rgb, dep, seg)
        return rgb, dep, seg
    before = shot(7)
    out = np.zeros((2, m.size("ntendon_item"), N))
    b.tendon_paths(idx, out)
    with_t = shot(7 | native.RENDER_TENDONS)
    after = shot(7)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    nit = m.size("ngeom") + m.size("nsite")
    assert (with_t[2] >= nit).any() and (with_t[2] < nit + m.size("ntendon")).all() and not (before[2] >= nit).any()
    b.close()


@pytest.mark.gpu
def test_gpu_tendon_paths_and_render_leave_the_steps_bitwise_unchanged(hip_lib):
    """10 steps of 2 envs on the fp64 stepper (the path with owned workspace blocks), with and without the path pass and a tendon
    render between all steps"""
    import torch
    from myochallenge_amd.envs.baoding import BaodingVecEnv
    results = []
    for draw in (False, True):
        env = BaodingVecEnv("CustomMyoBaodingBallsP1", 2, {}, seed=3, dtype="f64")
        env.reset_tensor()
        first = env.render_tensor(None, 48, 48, None, rgb=True, depth=True, segmentation=True)
        g = torch.Generator(device=env.device).manual_seed(0)
        acc = []
        for _ in range(10):
            a = torch.rand((2, env.act_dim), generator=g, device=env.device) * 2 - 1
            out = env.step_tensor(a)
            acc.append(torch.cat([x.reshape(2, -1).to(torch.float64) for x in out], 1).clone())
            if draw:
                p = env.tendon_paths()
                assert tuple(p.shape) == (2, env._model.size("ntendon_item"), N) and bool((p[:, :, 22] > 0).any())
                env.render_tensor(None, 48, 48, None, rgb=True, depth=True, segmentation=True, tendons=True)
        torch.cuda.synchronize()
        last = env.render_tensor(None, 48, 48, None, rgb=True, depth=True, segmentation=True)
        qp, qv, ac, tm = env.get_state()
        results.append((torch.stack(acc), qp.clone(), qv.clone(), ac.clone(), tm.clone(), first, last, env.batch.health()))
        env.close()
    for x, y in zip(results[0][:5], results[1][:5]):
        assert torch.equal(x, y)
    for k in ("rgb", "depth", "segmentation"):                      # without the flag: the same image, before and after any tendon call
        assert torch.equal(results[0][5][k], results[1][5][k]) and torch.equal(results[0][6][k], results[1][6][k])
    assert results[0][7] == results[1][7]


# ------------------------------------------------------------------------------------------------ 6. arguments and surface
def test_tendon_paths_argument_errors_and_symbol(emu_lib, golden_dir):
    assert "myo_batch_tendon_paths" in native.EXPORTED_SYMBOLS and native.RENDER_TENDONS == 16
    cm = _model("myo_finger_v0", golden_dir)[0]
    m = native.Model(cm, emu_lib)
    b = native.Batch(m, None, 2, 0, 0, native.MYO_F64)
    L = emu_lib.L
    idx = np.arange(2, dtype=np.int32)
    out = np.zeros((2, m.size("ntendon_item"), N))
    assert L.myo_batch_tendon_paths(b.h, idx.ctypes.data, 2, out.ctypes.data, None) == 0
    for args in ((b.h, idx.ctypes.data, 2, None, None), (b.h, idx.ctypes.data, -1, out.ctypes.data, None), (b.h, None, 2, out.ctypes.data, None),
                 (None, idx.ctypes.data, 2, out.ctypes.data, None)):
        assert L.myo_batch_tendon_paths(*args) == -1                 # MYO_E_ARG
        assert L.myo_last_error()
    assert m.size("ntendon_item") == 37
    b.close()


def test_a_model_with_more_tendon_items_than_the_renderer_holds_is_refused(emu_lib, golden_dir):
    """The renderer holds 512 tendon items (MYO_RTEN_MAX) and refuses MYO_RENDER_TENDONS beyond with MYO_E_ARG.  The stepper's own
    capacity is smaller — 240 path elements and 96 wrap geoms, at most 432 items (a static_assert in csrc/myo_host.h keeps that
    relation) — so a model with more items is refused, with a message, when it is loaded: a finger model whose last tendon runs on
    through 600 more site -> site pieces."""
    import copy
    cm = copy.deepcopy(_model("myo_finger_v0", golden_dir)[0])
    f = cm.fields
    nw, last = int(f["sizes"][9]), int(f["tendon_adr"][-1]) + int(f["tendon_num"][-1]) - 1
    assert last == nw - 1 and f["wrap_type"][last] == WRAP_SITE and f["wrap_type"][last - 2] == WRAP_SITE
    two = [int(f["wrap_objid"][last - 2]), int(f["wrap_objid"][last])]
    extra = 600
    f["wrap_type"] = np.concatenate([f["wrap_type"], np.full(extra, WRAP_SITE, f["wrap_type"].dtype)])
    f["wrap_objid"] = np.concatenate([f["wrap_objid"], np.resize(two, extra).astype(f["wrap_objid"].dtype)])
    f["wrap_prm"] = np.concatenate([f["wrap_prm"], np.zeros(extra, f["wrap_prm"].dtype)])
    f["tendon_num"] = f["tendon_num"].copy()
    f["tendon_num"][-1] += extra
    f["sizes"] = f["sizes"].copy()
    f["sizes"][9] = nw + extra
    with pytest.raises(Exception, match="tendon path elements"):
        native.Model(cm, emu_lib)
    # ... and one that fits is drawn whole: every used slot of the path pass is a drawn item (nothing truncated)
    m = native.Model(_model("hand", golden_dir)[0], emu_lib)
    assert m.size("ntendon_item") == 243 <= 512


@pytest.mark.gpu
def test_gpu_get_images_render_and_vecnormalize_take_the_keyword(hip_lib):
    from myochallenge_amd.envs.pose import PoseVecEnv
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    env = PoseVecEnv("CustomMyoHandPoseRandom", 3, seed=1)
    env.reset_tensor()
    cam = {"distance": 0.25}
    off, on = env.get_images(width=96, height=96, camera=cam), env.get_images(width=96, height=96, camera=cam, tendons=True)
    assert all(np.array_equal(a, b) for a, b in zip(off, env.get_images(width=96, height=96, camera=cam, tendons=False)))
    seg = env.render_tensor(None, 96, 96, cam, rgb=False, segmentation=True, tendons=True)["segmentation"].cpu().numpy()
    nit = env._model.size("ngeom") + env._model.size("nsite")
    for e in range(3):
        tp = seg[e] >= nit
        assert tp.any() and (off[e][tp] != on[e][tp]).any(axis=-1).mean() > 0.9      # the tendon pixels changed
        assert np.array_equal(off[e][~tp], on[e][~tp])                                 # ... and only they
    vn = VecNormalize(env)
    assert all(np.array_equal(a, b) for a, b in zip(vn.get_images(width=96, height=96, camera=cam, tendons=True), on))
    assert np.array_equal(vn.render("rgb_array", width=96, height=96, camera=cam, tendons=True), env.render("rgb_array", width=96, height=96, camera=cam, tendons=True))
    assert not np.array_equal(vn.render("rgb_array", width=96, height=96, camera=cam, tendons=True), vn.render("rgb_array", width=96, height=96, camera=cam))
    t = vn.render_tensor([2, 0], 32, 32, cam, rgb=False, segmentation=True, tendons=True)
    assert tuple(t["segmentation"].shape) == (2, 32, 32)
    assert tuple(vn.tendon_paths([1]).shape) == (1, env._model.size("ntendon_item"), N)
    env.close()


@pytest.mark.gpu
def test_gpu_main_eval_render_tendons_writes_decodable_pngs(hip_lib, golden_dir, tmp_path):
    out = tmp_path / "frames"
    cmd = [sys.executable, "-m", "myochallenge_amd.main_eval", "--model", os.path.join(golden_dir, "phase1_final.zip"),
           "--env-path", os.path.join(golden_dir, "normalized_env_phase1_final.pkl"), "--env-name", "CustomMyoBaodingBallsP1",
           "--num-episodes", "2", "--num-envs", "2", "--config", str(tmp_path / "cfg.json"),
           "--render-dir", str(out), "--render-tendons", "--render-envs", "2", "--render-size", "40", "30"]
    (tmp_path / "cfg.json").write_text("{}")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(cmd, check=True, cwd=root, timeout=600)
    files = sorted(os.listdir(out))
    assert files and any(f.startswith("env1_") for f in files)
    img = decode_png(open(out / files[0], "rb").read())
    assert img.shape == (30, 40, 3) and img.std() > 0
