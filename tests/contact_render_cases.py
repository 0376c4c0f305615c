"""Cases of the contact overlay (include/myobatch.h myo_batch_contact_items, MYO_RENDER_CONTACTS, myo_render_style;
csrc/myo_render.h) shared by the emulation (CPU) and HIP (GPU) tests of tests/test_render_contacts.py.  Every case takes the native
library and the arithmetic and goes through the env classes, so the same code checks both backends.

Bounds.  Items against ``sensors()`` of the same state: the two passes run the same device functions on the same record, so 1e-12
(absolute, metres / newtons) is far above what they can differ by.  End points of a force shaft are reconstructed as mid -/+ half *
axis: the rounding of that reconstruction, 16 eps (|mid| + half) (tests/test_render_tendons.py), plus the same 16 eps on the numpy
side's own pos + s F, whose size is s |F|.  Force balance: sensor_cases.TOL relative to 1 + |wrench| (the kernel sums the same forces
in fp32 in the mixed stepper).  Image: the per-pixel bounds of tests/test_render_tendons.py (ids equal, depth 1e-5 + 1e-5 d, rgb
+-1 outside the yardstick's edge mask, at most a quarter of the image in the mask)."""
import numpy as np

import render_ref as rr
from helpers import _on_cpu, make_env
from myochallenge_amd import native
from sensor_cases import HEALTHY, TOL, make_frame

N = native.RENDER_ITEM_N
DTYPE_NAME = {native.MYO_F64: "f64", native.MYO_MIXED: "mixed"}
DEFAULT_STYLE = {"disc_radius": 0.003, "disc_half_height": 0.0005, "force_radius": 0.001, "metres_per_newton": 0.02,
                 "point_rgba": (0.9, 0.6, 0.2, 1.0), "force_rgba": (0.7, 0.9, 0.9, 1.0), "geom_alpha": 1.0}
W, H = 64, 48
EDGE_SHARE = 0.25                   # tests/test_render_tendons.py
MIN_CONTACT_PIXELS = 20             # "some pixels": more than a stray one, outside the edge mask
# the style of the image cases: at 64 x 48 (focal length 58 px) and 0.12 m a radius of 5 mm is ~2.4 px, so that items are wider than
# the yardstick's edge mask; 0.1 m/N makes a ball's ~0.4 N support force a 4 cm shaft, longer than a ball's radius
IMAGE_STYLE = {"disc_radius": 0.010, "disc_half_height": 0.001, "force_radius": 0.005, "metres_per_newton": 0.1, "geom_alpha": 0.4}
_ENVS = {}


def _np(x):
    return x.detach().cpu().numpy()


def make_pose_env(lib, num_envs, seed, dtype):
    from myochallenge_amd.envs.pose import PoseVecEnv
    cls = _on_cpu(PoseVecEnv) if lib.is_emulation else PoseVecEnv
    return cls("CustomMyoHandPoseRandom", num_envs, {}, seed=seed, dtype=DTYPE_NAME[dtype], lib=lib)


def stepped_env(lib, dtype, kind, n=None, seed=1, nsteps=None, draw_between=False):
    """a fresh env `nsteps` seeded random-action steps into its episodes: "baoding" (3 envs, the balls rest on the palm), "die" (2 envs,
    the 48-slot stepper, squeezed as in sensor_cases.case_die_parity), "pose" (the hand alone).  draw_between: a contact render and a
    contact item pass between all steps (and before the first)."""
    import torch
    import warnings
    name, n0, steps0, mean = {"baoding": ("CustomMyoBaodingBallsP1", 3, 5, 0.0), "die": ("CustomMyoReorientP1", 2, 25, 0.5),
                              "pose": (None, 2, 3, 0.0)}[kind]
    n, nsteps = n or n0, steps0 if nsteps is None else nsteps
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the die env warns about the mixed stepper's trajectory tolerance: not what is tested here)
        env = make_pose_env(lib, n, seed, dtype) if kind == "pose" else make_env(name, lib, num_envs=n, seed=seed, dtype=DTYPE_NAME[dtype])
    env.reset_tensor()
    rng = np.random.RandomState(seed)

    def draw():
        env.contact_items()
        env.render_tensor(None, 16, 16, None, rgb=True, depth=True, segmentation=True, contacts=True)
    if draw_between:
        draw()
    for _ in range(nsteps):
        a = np.clip(rng.normal(mean, 0.5, (n, env.act_dim)), -1, 1).astype(np.float32)
        env.step_tensor(torch.as_tensor(a, device=env.device))
        if draw_between:
            draw()
    return env


def shared_env(lib, dtype, kind):
    """one stepped env per (library, arithmetic, kind) with its read-out and items, computed once; the cases that use it leave its
    state and style as they found them"""
    key = (lib.is_emulation, dtype, kind)
    if key not in _ENVS:
        env = stepped_env(lib, dtype, kind)
        sens = {k: _np(v) for k, v in env.sensors(["ncon", "con_geom", "con_d", "body_wrench"]).items()}
        _ENVS[key] = (env, sens, _np(env.contact_items()))
    return _ENVS[key]


def ends(it):
    """the two end points of a capsule item, reconstructed (tests/test_render_tendons.py)"""
    z = it[3:12].reshape(3, 3)[:, 2]
    return it[0:3] - it[13] * z, it[0:3] + it[13] * z


def world_force(d):
    """F = n f0 + t1 f1 + t2 f2 of a con_d row (sensor_cases.rebuilt_wrench)"""
    n = d[4:7]
    t1, t2 = make_frame(n)
    return n * d[7] + t1 * d[8] + t2 * d[9]


# ---------------------------------------------------------------------------------------------------------------- 1. items
def case_items_match_sensors(lib, dtype, kind):
    env, sens, items = shared_env(lib, dtype, kind)
    cap = env.batch.contact_capacity
    assert items.shape == (env.num_envs, 2 * cap, N) and cap == (48 if kind == "die" else (22 if dtype == native.MYO_F64 else 24))
    s = DEFAULT_STYLE["metres_per_newton"]
    eps = np.finfo(float).eps
    nforce = 0
    for e in range(env.num_envs):
        nc = int(sens["ncon"][e])
        assert nc >= 2
        disc, arrow = items[e, 0::2], items[e, 1::2]
        assert int((np.abs(disc).sum(1) > 0).sum()) == nc and not disc[nc:].any() and not arrow[nc:].any()
        for c in range(nc):
            d, p, a = sens["con_d"][e, c], disc[c], arrow[c]
            R = p[3:12].reshape(3, 3)
            t1, t2 = make_frame(d[4:7])
            assert np.abs(p[0:3] - d[1:4]).max() <= 1e-12 and np.abs(R[:, 2] - d[4:7]).max() <= 1e-12 and abs(p[23] - d[0]) <= 1e-12
            assert np.abs(R[:, 0] - t1).max() <= 1e-12 and np.abs(R[:, 1] - t2).max() <= 1e-12
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0
            assert p[15] == rr.CYLINDER and p[22] == c + 1 and p[21] == 0 and p[14] == 0
            assert p[12] == DEFAULT_STYLE["disc_radius"] and p[13] == DEFAULT_STYLE["disc_half_height"] and abs(p[20] - np.sqrt(p[12] ** 2 + p[13] ** 2)) <= 4 * eps * p[20]
            assert np.array_equal(p[16:20], np.asarray(DEFAULT_STYLE["point_rgba"], np.float32).astype(np.float64))
            F = world_force(d)
            fn = np.linalg.norm(F)
            if fn == 0:
                assert not a.any()
                continue
            nforce += 1
            p0, p1 = ends(a)
            tol = 16 * eps * (np.abs(a[0:3]).max() + a[13]) + 16 * eps * (np.abs(d[1:4]).max() + s * fn)
            assert np.abs(p0 - d[1:4]).max() <= tol and np.abs(p1 - (d[1:4] + s * F)).max() <= tol, (e, c)
            assert abs(a[23] - fn) <= 1e-12 * max(1.0, fn) and abs(a[13] - 0.5 * s * fn) <= 1e-12
            assert a[15] == rr.CAPSULE and a[22] == c + 1 and a[12] == DEFAULT_STYLE["force_radius"] and a[20] == a[12] + a[13]
            assert np.array_equal(a[16:20], np.asarray(DEFAULT_STYLE["force_rgba"], np.float32).astype(np.float64))
    assert nforce >= 2 * env.num_envs and env.batch.health() == HEALTHY


# ---------------------------------------------------------------------------------------------------------------- 2. force balance
def case_force_balance(lib, dtype, kind):
    env, sens, items = shared_env(lib, dtype, kind)
    gb = np.asarray(env.compiled.fields["geom_bodyid"])
    s = DEFAULT_STYLE["metres_per_newton"]
    objs = env.object_body_ids()
    assert objs
    for e in range(env.num_envs):
        nc = int(sens["ncon"][e])
        for body in objs:
            total, cnt = np.zeros(3), 0
            for c in range(nc):
                a = items[e, 2 * c + 1]
                p0, p1 = ends(a)
                sign = (gb[sens["con_geom"][e, c, 1]] == body) * 1.0 - (gb[sens["con_geom"][e, c, 0]] == body) * 1.0
                total += sign * (p1 - p0) / s
                cnt += sign != 0
            w = sens["body_wrench"][e, body, :3]
            err = np.abs(total - w).max()
            print("force balance", kind, dtype, "env", e, "body", body, "contacts", cnt, "err", err, "|w|", np.linalg.norm(w))
            assert cnt >= 1 and err <= TOL[dtype] * (1 + np.linalg.norm(w)), (e, body, total, w)


# ---------------------------------------------------------------------------------------------------------------- 3. image
def contact_camera(sens, e, distance=0.12, azimuth=90.0, elevation=-45.0):
    nc = int(sens["ncon"][e])
    return {"lookat": tuple(sens["con_d"][e, :nc, 1:4].mean(0)), "distance": distance, "azimuth": azimuth, "elevation": elevation, "fovy": 45.0}


def reference_tables(env, idx, tendons, geom_alpha):
    """the device's item rows of envs idx as the yardstick's table: geoms + sites (the geoms' alpha times geom_alpha, in fp32 as the
    ray caster holds it), tendon items if drawn, contact items; and per table row the segmentation id it stands for"""
    import torch
    m = env._model
    ng, nit, nt = m.size("ngeom"), m.size("ngeom") + m.size("nsite"), m.size("ntendon")
    po = torch.zeros((len(idx), nit, N), dtype=torch.float64, device=env.device)
    env.batch.geom_poses(torch.tensor(idx, dtype=torch.int32, device=env.device), po, env._stream())
    po = _np(po)
    po[:, :ng, 19] = (po[:, :ng, 19].astype(np.float32) * np.float32(geom_alpha)).astype(np.float64)
    tabs, ids = [po], [np.tile(np.arange(nit), (len(idx), 1))]
    if tendons:
        tp = _np(env.tendon_paths(idx))
        tabs.append(tp); ids.append(nit + tp[:, :, 22].astype(int) - 1)
    ci = _np(env.contact_items(idx))
    tabs.append(ci); ids.append(nit + nt + ci[:, :, 22].astype(int) - 1)
    return np.concatenate(tabs, 1), np.concatenate(ids, 1), nit + nt


def case_image(lib, dtype, kind, tendons, elevation):
    env, sens, _ = shared_env(lib, dtype, kind)
    idx = list(range(env.num_envs))
    cams = [contact_camera(sens, e, elevation=elevation) for e in idx]
    try:
        out = env.render_tensor(idx, W, H, cams, rgb=True, depth=True, segmentation=True, tendons=tendons, contacts=True, contact_style=IMAGE_STYLE)
        rgb, dep, seg = _np(out["rgb"]), _np(out["depth"]), _np(out["segmentation"])
        items, ids, seg_c = reference_tables(env, idx, tendons, IMAGE_STYLE["geom_alpha"])
    finally:
        env.batch.set_render_style(**DEFAULT_STYLE)
    total = 0
    for e in idx:
        s2, d2, c2, edge = rr.render(items[e], cams[e], W, H)
        want = np.where(s2 >= 0, ids[e][np.maximum(s2, 0)], -1)
        ok = ~edge
        ncp = int((ok & (want >= seg_c)).sum())
        total += ncp
        print("image", kind, dtype, "env", e, "contact pixels outside the edge mask", ncp, "edge share", edge.mean())
        assert edge.mean() <= EDGE_SHARE
        bad = ok & (want != seg[e])
        assert not bad.any(), (kind, e, int(bad.sum()))
        both = ok & (s2 >= 0)
        d = dep[e].astype(np.float64)
        assert np.all(np.abs(d[both] - d2[both]) <= 1e-5 + 1e-5 * d2[both]), (kind, e)
        assert np.isinf(d[ok & (s2 < 0)]).all()
        assert np.abs(rgb[e][ok].astype(int) - c2[ok].astype(int)).max() <= 1, (kind, e)
        cp = seg[e] >= seg_c
        assert cp.any() and (seg[e][cp] - seg_c < int(sens["ncon"][e])).all()
        assert ncp >= MIN_CONTACT_PIXELS
    return total


def case_many_envs(lib, dtype, k=70):
    """k = 70 rows at 16 x 16 from a 3-env batch (each env listed many times, and two indices outside the batch): more rows than a wave
    has lanes, one tile per env whose last rows / columns ... are all inside; every row equals its env's row of a 3-row call"""
    import torch
    env, sens, items = shared_env(lib, dtype, "baoding")
    idx = [i % 3 for i in range(k)]
    it = _np(env.contact_items(idx))
    assert it.shape == (k, items.shape[1], N)
    for r in range(k):
        assert np.array_equal(it[r], items[idx[r]]), r
    cam = contact_camera(sens, 0)
    small = env.render_tensor(idx, 16, 16, cam, rgb=True, depth=True, segmentation=True, contacts=True)
    three = env.render_tensor([0, 1, 2], 16, 16, cam, rgb=True, depth=True, segmentation=True, contacts=True)
    for key in small:
        a, b = _np(small[key]), _np(three[key])
        assert all(np.array_equal(a[r], b[idx[r]]) for r in range(k)), key
    # a ragged last tile: 20 x 18 is two tiles by two, the last ones 4 / 2 pixels wide
    rag = env.render_tensor([0, 1, 2], 20, 18, cam, rgb=True, depth=True, segmentation=True, contacts=True)
    assert tuple(rag["rgb"].shape) == (3, 18, 20, 3) and np.isfinite(_np(rag["depth"])[_np(rag["segmentation"]) >= 0]).all()
    # out-of-range rows through the C ABI: all zero
    raw = torch.full((4, items.shape[1], N), 7.0, dtype=torch.float64, device=env.device)
    env.batch.contact_items(torch.tensor([1, 3, -1, 0], dtype=torch.int32, device=env.device), raw, env._stream())
    raw = _np(raw)
    assert not raw[1].any() and not raw[2].any() and np.array_equal(raw[0], items[1]) and np.array_equal(raw[3], items[0])


# ---------------------------------------------------------------------------------------------------------------- 4. off, read-only
def case_off_means_off(lib, dtype):
    env, sens, _ = shared_env(lib, dtype, "baoding")
    cam = contact_camera(sens, 0, elevation=45.0)
    shot = lambda **kw: {k: _np(v) for k, v in env.render_tensor(None, W, H, cam, rgb=True, depth=True, segmentation=True, **kw).items()}
    before = shot()
    try:
        with_c = shot(contacts=True, contact_style=IMAGE_STYLE)      # (the default style's 3 mm discs sit inside the opaque geoms)
        after_styled = shot()
    finally:
        env.batch.set_render_style(**DEFAULT_STYLE)
    after = shot()
    for k in before:
        assert np.array_equal(before[k], after[k]) and np.array_equal(before[k], after_styled[k]), k
    seg_c = env._model.size("ngeom") + env._model.size("nsite") + env._model.size("ntendon")
    assert not (before["segmentation"] >= seg_c).any() and (with_c["segmentation"] >= seg_c).any()
    # the pixels that show no contact item are what they are without the flag: opaque items over opaque geoms (geom_alpha back at 1),
    # the one-table cast and the two-layer cast (tendons) against the casts with the contact layer
    try:
        env.batch.set_render_style(**dict(IMAGE_STYLE, geom_alpha=1.0))
        for tendons in (False, True):
            without, with_c = shot(tendons=tendons), shot(tendons=tendons, contacts=True)
            contact = with_c["segmentation"] >= seg_c
            print("other pixels", dtype, "tendons", tendons, "contact pixels", int(contact.sum()), "of", contact.size)
            assert contact.any() and contact.mean() <= 0.5
            for k in without:
                assert np.array_equal(without[k][~contact], with_c[k][~contact]), (tendons, k)
    finally:
        env.batch.set_render_style(**DEFAULT_STYLE)


def case_read_only(lib, dtype, n=3, seed=5, nsteps=10):
    """two envs of one seed, one drawn with contacts (item pass and render) between all steps: the same state bits, the same health"""
    a = stepped_env(lib, dtype, "baoding", n, seed, nsteps, draw_between=True)
    b = stepped_env(lib, dtype, "baoding", n, seed, nsteps, draw_between=False)
    wa, wb = [a.torch.zeros((n, a._model.size("nv")), dtype=a.torch.float64, device=a.device) for _ in range(2)]
    a.batch.warmstart(wa, None, a._stream())
    b.batch.warmstart(wb, None, b._stream())
    for x, y in zip(a.get_state() + (wa,), b.get_state() + (wb,)):
        assert np.array_equal(_np(x), _np(y))
    assert a.batch.health() == HEALTHY and b.batch.health() == HEALTHY
    assert np.array_equal(_np(a.contact_items()), _np(b.contact_items()))
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. style
def case_style(lib, dtype):
    import ctypes as C
    env, sens, items = shared_env(lib, dtype, "baoding")
    b = env.batch
    got = b.get_render_style()
    assert set(got) == set(DEFAULT_STYLE)
    for k, v in DEFAULT_STYLE.items():
        assert np.allclose(got[k], v, rtol=0, atol=1e-7), k          # (the colours are float32)
    try:
        new = {"disc_radius": 0.004, "disc_half_height": 0.001, "force_radius": 0.002, "metres_per_newton": 0.04,
               "point_rgba": (0.25, 0.5, 0.75, 1.0), "force_rgba": (1.0, 0.0, 0.5, 0.5), "geom_alpha": 0.5}
        b.set_render_style(**new)
        assert b.get_render_style() == {k: (tuple(float(x) for x in v) if isinstance(v, tuple) else v) for k, v in new.items()}
        st = native.RenderStyle()
        for size in (0, C.sizeof(native.RenderStyle) - 8, C.sizeof(native.RenderStyle) + 8):
            st.size = size
            assert lib.L.myo_batch_set_render_style(b.h, C.byref(st)) == -1 and b"size" in lib.L.myo_last_error()
            assert lib.L.myo_batch_get_render_style(b.h, C.byref(st)) == -1
        st.size = C.sizeof(native.RenderStyle)
        assert lib.L.myo_batch_set_render_style(None, C.byref(st)) == -1 and lib.L.myo_batch_set_render_style(b.h, None) == -1
        assert lib.L.myo_batch_get_render_style(None, C.byref(st)) == -1 and lib.L.myo_batch_get_render_style(b.h, None) == -1
        for bad in ({"disc_radius": -1.0}, {"metres_per_newton": float("nan")}, {"geom_alpha": 1.5}, {"point_rgba": (0, 0, 0, 2)}):
            try:
                b.set_render_style(**bad)
            except native.MyoError:
                pass
            else:
                raise AssertionError(bad)
        assert b.get_render_style()["metres_per_newton"] == 0.04      # a refused style changes nothing
        # metres_per_newton doubled (0.02 -> 0.04): every shaft's half length doubles, and only that and what follows from it moves
        it2 = _np(env.contact_items())
        arrows = items[:, 1::2, 13] > 0
        # (a half length is half the norm of (pos + s F) - pos: doubled up to the rounding of the two tips, 16 eps (|pos| + 2 half))
        h1, h2 = items[:, 1::2, 13][arrows], it2[:, 1::2, 13][arrows]
        assert arrows.any() and np.all(np.abs(h2 - 2 * h1) <= 16 * np.finfo(float).eps * (np.abs(items[:, :, 0:3]).max() + 2 * h2))
        assert np.array_equal(it2[:, :, 23], items[:, :, 23]) and np.array_equal(it2[:, 0::2, 0:12], items[:, 0::2, 0:12])
        assert (it2[:, 0::2, 12][it2[:, 0::2, 22] > 0] == 0.004).all() and (it2[:, 1::2, 12][arrows] == 0.002).all()
        # geom_alpha < 1 changes the image with the flag, and not without it
        cam = contact_camera(sens, 0)
        shot = lambda **kw: _np(env.render_tensor(None, W, H, cam, **kw)["rgb"])
        half_on, half_off = shot(contacts=True), shot()
        b.set_render_style(geom_alpha=1.0)
        one_on, one_off = shot(contacts=True), shot()
        assert np.array_equal(half_off, one_off) and not np.array_equal(half_on, one_on)
    finally:
        b.set_render_style(**DEFAULT_STYLE)


# ---------------------------------------------------------------------------------------------------------------- 6. pose batch
def case_pose_batch(lib, dtype):
    env = stepped_env(lib, dtype, "pose")
    assert not _np(env.contact_items()).any() and env.object_body_ids() == []
    cam = {"distance": 0.25}
    shot = lambda **kw: {k: _np(v) for k, v in env.render_tensor(None, W, H, cam, rgb=True, depth=True, segmentation=True, **kw).items()}
    off, on = shot(), shot(contacts=True)
    assert (off["segmentation"] >= 0).any()
    for k in off:
        assert np.array_equal(off[k], on[k]), k
    two, three = shot(tendons=True), shot(tendons=True, contacts=True)      # two layers against three with an empty third
    assert not np.array_equal(two["rgb"], off["rgb"])
    for k in two:
        assert np.array_equal(two[k], three[k]), k
    env.close()
