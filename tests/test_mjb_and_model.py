"""MJB reader, model compilation, blob format, host-side constants (CPU only)."""
import json
import os
import struct

import numpy as np
import pytest

from myochallenge_amd.mjb import MjbError, load_mjb, parse_mjb
from myochallenge_amd.model import ModelError, compile_model
from myochallenge_amd.setconst import set_const


@pytest.mark.parametrize("name,short", [("myo_finger_v0", "finger"), ("motor_finger_v0", "motor_finger"), ("myo_load", "load")])
def test_mjb_decodes_to_committed_json(golden_dir, name, short):
    m = load_mjb(os.path.join(golden_dir, name + ".mjb"))
    js = json.load(open(os.path.join(golden_dir, f"mjb_{short}.json")))
    assert m.sizes == js["sizes"]
    assert m.opt["timestep"] == 0.002 and m.opt["integrator"] == 0 and m.opt["cone"] == 0
    for k, v in js["arrays"].items():
        np.testing.assert_array_equal(np.asarray(m.arrays[k]).reshape(-1), np.asarray(v).reshape(-1))


def test_mjb_known_facts(models):
    f = models["finger"]
    assert (f.nq, f.nv, f.nu, f.ntendon, f.nwrap) == (4, 4, 5, 5, 35)
    assert f.names["tendon"] == ["extn", "mflx", "dflx", "adabR", "adabL"]
    assert abs(f.stat["meaninertia"] - np.mean(f.dof_M0)) < 1e-15
    l = models["load"]
    assert (l.nq, l.nu, l.ntendon) == (1, 1, 1) and l.tendon_length0[0] == 0.1


def test_mjb_rejects_garbage(golden_dir):
    blob = open(os.path.join(golden_dir, "myo_load.mjb"), "rb").read()
    with pytest.raises(MjbError):
        parse_mjb(b"\0" * 10)
    with pytest.raises(MjbError):
        parse_mjb(struct.pack("<4i", 1, 8, 57, 266) + blob[16:])
    with pytest.raises(MjbError):
        parse_mjb(blob[:-7])       # truncated buffer


def test_blob_roundtrip(models):
    cm = compile_model(models["finger"], unsupported_contacts="drop")
    blob = cm.to_blob()
    magic, ver, nf, tot = struct.unpack_from("<IIII", blob, 0)
    assert magic == 0x4D4F594D and ver == 1 and tot == len(blob) and nf == len(cm.fields)
    # every field is 8-byte aligned and inside the blob
    for i in range(nf):
        name, dt, cnt, off = struct.unpack_from("<40sIIQ", blob, 16 + 56 * i)
        assert off % 8 == 0 and off + cnt * (4 if dt == 0 else 8) <= len(blob)


def test_collision_pair_filter(models):
    cm = compile_model(models["hand"])
    g1, g2 = cm.x_pair_geom1, cm.x_pair_geom2
    names = cm.names["geom"]
    # only ball-vs-hand and ball-vs-ball pairs (hand geoms have conaffinity 0)
    assert all("ball" in names[a] or "ball" in names[b] for a, b in zip(g1, g2))
    assert sum(1 for a, b in zip(g1, g2) if "ball" in names[a] and "ball" in names[b]) == 1
    assert cm.dropped_pairs == []
    # finger model: its plane / sphere / capsule vs cylinder / ellipsoid pairs have narrow phases (round 3) and are ordered
    # after the primitive pairs; a pair without one (here: the ellipsoid turned into a mesh) makes the model an error unless
    # the caller opts in, and is then listed
    import copy
    import pytest
    from myochallenge_amd.model import UnsupportedContactsError
    fm = compile_model(models["finger"])
    assert fm.dropped_pairs == []
    gt = models["finger"].geom_type
    ext = [(int(gt[a]), int(gt[b])) in ((0, 4), (0, 5), (2, 4), (2, 5), (3, 4), (3, 5)) for a, b in zip(fm.x_pair_geom1, fm.x_pair_geom2)]
    assert any(ext) and ext == sorted(ext)
    mesh = copy.deepcopy(models["finger"])
    mesh.arrays["geom_type"][np.argmax(gt == 4)] = 7
    with pytest.raises(UnsupportedContactsError):
        compile_model(mesh)
    assert len(compile_model(mesh, unsupported_contacts="drop").dropped_pairs) > 0


def test_feature_gates(models):
    """What the stepper does not implement is refused at compile time, never ignored: elliptic cones, equality constraints, condim
    values MuJoCo does not have.  Friction loss and condim 1 / 4 / 6 compile since round 4 (tests/test_narrow_phases.py)."""
    import copy
    m = copy.deepcopy(models["finger"])
    m.arrays["dof_frictionloss"][0] = 0.1
    compile_model(m)                                   # friction loss: rows of their own (mj_instantiateFriction)
    m = copy.deepcopy(models["finger"])
    m.opt["cone"] = 1
    with pytest.raises(ModelError):
        compile_model(m)
    m = copy.deepcopy(models["finger"])
    m.sizes["neq"] = 1
    with pytest.raises(ModelError):
        compile_model(m)
    m = copy.deepcopy(models["hand"])
    m.arrays["geom_condim"][m.names["geom"].index("ball1")] = 5
    with pytest.raises(ModelError):
        compile_model(m)


def test_setconst_reproduces_mujoco_constants(models):
    import copy
    m = copy.deepcopy(models["finger"])
    ref = {k: m.arrays[k].copy() for k in ("dof_M0", "dof_invweight0", "body_invweight0", "tendon_length0")}
    refJ = {k: m.arrays[k].copy() for k in ("tendon_invweight0", "actuator_acc0")}
    set_const(m)
    for k, v in ref.items():
        np.testing.assert_allclose(m.arrays[k], v, rtol=1e-12, atol=1e-15)
    for k, v in refJ.items():   # finite-difference moment arms vs MuJoCo's analytic ones
        np.testing.assert_allclose(m.arrays[k], v, rtol=1e-4)


def test_synthetic_hand_shape(models):
    h = models["hand"]
    assert (h.nq, h.nv, h.nu, h.na) == (37, 35, 39, 39)          # baoding.py:183,187-194,282
    assert h.names["site"][h.name2id("site", "target1_site")] == "target1_site"
    jn = h.names["jnt"]
    assert jn[0] == "pro_sup" and jn[3].startswith("cmc") and jn[8].endswith("abduction") and jn[12].endswith("abduction")
    assert h.opt["timestep"] == 0.002 and h.opt["integrator"] == 0


def test_c_mjb_loader_equals_python_route(emu_lib, golden_dir, tmp_path):
    """myo_model_load_mjb (csrc/myo_mjb.h) against mjb.load_mjb + model.compile_model + myo_model_from_blob on the three
    models the reference ships: same sizes, and bit-identical trajectories of the two myo_model objects."""
    import os
    import numpy as np
    import pytest
    from myochallenge_amd import native
    from myochallenge_amd.mjb import load_mjb
    from myochallenge_amd.model import compile_model
    for name in ("myo_finger_v0.mjb", "motor_finger_v0.mjb", "myo_load.mjb"):
        path = os.path.join(golden_dir, name)
        mc = native.Model.from_mjb(path, emu_lib)                                    # (cylinder / ellipsoid pairs compile since round 3)
        mp = native.Model(compile_model(load_mjb(path), unsupported_contacts="drop"), emu_lib)
        for k in ("nq", "nv", "nu", "na", "nbody", "njnt", "ngeom", "nsite", "ntendon", "nwrap", "npair", "nM", "integrator"):
            assert mc.size(k) == mp.size(k), (name, k)
        nq, nv, na, nu = (mc.size(k) for k in ("nq", "nv", "na", "nu"))
        rng = np.random.RandomState(0)
        outs = []
        for m in (mc, mp):
            b = native.Batch(m, None, 2, 0, 0, native.MYO_F64)
            r = np.random.RandomState(1)
            for _ in range(40):
                b.physics_step(r.uniform(0, 1, (2, nu)), 1)
            qp, qv = np.zeros((2, nq)), np.zeros((2, nv))
            b.get_state(qp, qv)
            outs.append((qp.copy(), qv.copy()))
            b.close()
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.abs(outs[0][1]).max() > 0
    import copy
    from myochallenge_amd.mjb import dump_mjb
    mesh = copy.deepcopy(load_mjb(os.path.join(golden_dir, "myo_finger_v0.mjb")))
    mesh.arrays["geom_type"][np.argmax(mesh.geom_type == 4)] = 7
    (tmp_path / "mesh.mjb").write_bytes(dump_mjb(mesh))
    with pytest.raises(native.MyoError, match="no narrow phase"):
        native.Model.from_mjb(str(tmp_path / "mesh.mjb"), emu_lib)                    # a pair without a narrow phase: refused ...
    assert native.Model.from_mjb(str(tmp_path / "mesh.mjb"), emu_lib, unsupported_contacts="drop").size("npair") < mc.size("npair") + 100   # ... unless the caller opts in
    rk = native.Model.from_mjb(os.path.join(golden_dir, "myo_load.mjb"), emu_lib, integrator=1)
    assert rk.size("integrator") == 1
    bad = tmp_path / "bad.mjb"
    bad.write_bytes(open(os.path.join(golden_dir, "myo_load.mjb"), "rb").read()[:-8])   # truncated
    with pytest.raises(native.MyoError):
        native.Model.from_mjb(str(bad), emu_lib)
    with pytest.raises(native.MyoError, match="cannot open"):
        native.Model.from_mjb(str(tmp_path / "missing.mjb"), emu_lib)


class _nullcontext:
    def __enter__(self): return None
    def __exit__(self, *a): return False


def _with(m, **arrays_and_opts):
    """copy of a decoded model with arrays / sizes / opt entries replaced (test helper)"""
    import copy
    m = copy.deepcopy(m)
    for k, v in arrays_and_opts.items():
        if k.startswith("opt_"):
            m.opt[k[4:]] = v
        elif k.startswith("n") and np.isscalar(v):
            m.sizes[k] = int(v)
        else:
            m.arrays[k] = np.asarray(v)
    return m


def test_exclude_pairs_filterparent_and_refused_options(models, emu_lib, tmp_path):
    """mj_collision's static filters through BOTH model routes (mjb.py + model.py, and the C reader csrc/myo_mjb.h fed by
    mjb.dump_mjb): an <exclude> body pair removes exactly the geom pairs of those two bodies; mjDSBL_FILTERPARENT brings the
    parent-child pairs back; explicit <pair> contacts, opt.collision = predefined, other disable flags and contact override
    are refused (they would change mj_step's contacts and this stepper does not restate them)."""
    from myochallenge_amd import native
    from myochallenge_amd.mjb import dump_mjb
    hand = models["hand"]
    base = compile_model(hand)
    gb = hand.geom_bodyid
    pairs = list(zip(base.x_pair_geom1, base.x_pair_geom2))
    ball1 = hand.names["body"].index("ball1")
    other = int(gb[[a if gb[b] == ball1 else b for a, b in pairs if ball1 in (gb[a], gb[b]) and gb[a] != gb[b]][0]])
    lo, hi = min(ball1, other), max(ball1, other)
    ex = _with(hand, exclude_signature=np.array([((lo + 1) << 16) + hi + 1], np.int32))
    cm = compile_model(ex)
    kept = list(zip(cm.x_pair_geom1, cm.x_pair_geom2))
    gone = [p for p in pairs if p not in kept]
    assert gone and all({int(gb[a]), int(gb[b])} == {lo, hi} for a, b in gone) and all(p in pairs for p in kept)

    def c_route(m, **kw):
        path = tmp_path / "m.mjb"
        path.write_bytes(dump_mjb(m))
        return native.Model.from_mjb(str(path), emu_lib, **kw)

    assert c_route(hand).size("npair") == len(pairs)
    assert c_route(ex).size("npair") == len(kept)
    # parent-child filter: give two finger segments (parent and child) colliding geoms
    fp = _with(hand)
    par = hand.body_parentid
    child = next(b for b in range(2, hand.nbody) if par[b] > 0 and hand.body_weldid[b] == b and hand.body_weldid[par[b]] == par[b]
                 and any(gb == b) and any(gb == par[b]))
    ga, gc = int(np.argmax(gb == par[child])), int(np.argmax(gb == child))
    for g in (ga, gc):
        fp.arrays["geom_contype"][g] = 1; fp.arrays["geom_conaffinity"][g] = 1
    n_filtered = len(compile_model(fp, unsupported_contacts="drop").x_pair_geom1)
    fp2 = _with(fp, opt_disableflags=1 << 9)
    cm2 = compile_model(fp2, unsupported_contacts="drop")
    with_pc = set(zip(cm2.x_pair_geom1, cm2.x_pair_geom2)) | set(cm2.dropped_pairs)
    assert (ga, gc) in with_pc or (gc, ga) in with_pc
    assert len(cm2.x_pair_geom1) + len(cm2.dropped_pairs) > n_filtered
    assert c_route(fp2, unsupported_contacts="drop").size("npair") == len(cm2.x_pair_geom1)
    # refused
    for bad in (_with(hand, npair=1), _with(hand, opt_disableflags=1 << 4), _with(hand, opt_enableflags=1)):        # (npair without its arrays)
        with pytest.raises(ModelError):
            compile_model(bad)
    for bad in (_with(hand, opt_disableflags=1 << 4), _with(hand, opt_enableflags=1),
                _with(hand, pair_dim=np.full(1, 3, np.int32), pair_geom1=np.zeros(1, np.int32), pair_geom2=np.ones(1, np.int32),
                      pair_signature=np.zeros(1, np.int32), pair_solref=np.zeros((1, 2)), pair_solimp=np.zeros((1, 5)), pair_margin=np.zeros(1),
                      pair_gap=np.zeros(1), pair_friction=np.array([[1.0, 0.5, 0.0, 0.0, 0.0]]), name_pairadr=np.zeros(1, np.int32), npair=1)):      # anisotropic friction
        with pytest.raises(native.MyoError, match="not supported|can be disabled"):
            c_route(bad)
    # explicit <contact><pair> entries (round 4): the pair replaces the dynamic pair of its two geoms; opt.collision = predefined keeps only them
    g_ball = hand.names["geom"].index("ball1")
    g_other = next(int(b if a == g_ball else a) for a, b in pairs if g_ball in (a, b))
    xp = _with(hand, pair_dim=np.full(1, 4, np.int32), pair_geom1=np.array([g_ball], np.int32), pair_geom2=np.array([g_other], np.int32),
               pair_signature=np.zeros(1, np.int32), pair_solref=np.array([[0.01, 1.0]]), pair_solimp=np.array([[0.8, 0.9, 0.002, 0.5, 2.0]]),
               pair_margin=np.array([0.003]), pair_gap=np.zeros(1), pair_friction=np.array([[0.7, 0.7, 0.01, 0.002, 0.002]]),
               name_pairadr=np.zeros(1, np.int32), npair=1)
    cmx = compile_model(xp)
    # (the explicit pair replaces EVERY dynamic geom pair between its two bodies: test_explicit_pair_replaces_every_dynamic_pair_of_its_two_bodies)
    same_bodies = sum(1 for a, b in pairs if {int(gb[a]), int(gb[b])} == {int(gb[g_ball]), int(gb[g_other])})
    assert len(cmx.x_pair_geom1) == len(pairs) - same_bodies + 1 and list(cmx.x_pair_explicit).count(0) == 1 and list(cmx.x_xp_dim) == [4]
    assert c_route(xp).size("npair") == len(pairs) - same_bodies + 1
    only = compile_model(_with(xp, opt_collision=1))
    assert len(only.x_pair_geom1) == 1 and c_route(_with(xp, opt_collision=1)).size("npair") == 1


def test_c_loader_rejects_corrupt_files(models, emu_lib, golden_dir, tmp_path):
    """myo_model_load_mjb / myo_model_from_blob are public entry points that must not trust their input: negative sizes, sizes
    whose products overflow, ids out of range and truncated files come back as MYO_E_ARG — no exception crosses the C ABI, no
    out-of-bounds read (the same mutations run under AddressSanitizer in tests/test_sanitizers.py)."""
    from myochallenge_amd import native
    from myochallenge_amd.mjb import dump_mjb
    good = dump_mjb(models["hand"])
    path = tmp_path / "c.mjb"

    def load(raw):
        path.write_bytes(raw)
        return native.Model.from_mjb(str(path), emu_lib)

    assert load(good).size("nv") == 35
    for blob in corrupt_mjb_variants(models["hand"], good):
        with pytest.raises(native.MyoError):
            load(blob)
        with pytest.raises(MjbError):
            parse_mjb(blob)
    # id-level corruption that survives the file parser is caught before any table is built, on both routes
    for m in corrupt_id_variants(models["hand"]):
        with pytest.raises(native.MyoError, match="corrupt model|out of range"):
            load(dump_mjb(m))
        with pytest.raises((native.MyoError, IndexError, ValueError, ModelError)):
            native.Model(compile_model(m), emu_lib)


def corrupt_mjb_variants(m, good):
    """byte-level mutations of a valid file: header sizes negative / huge, truncation"""
    out = []
    for idx, val in ((0, -1), (4, -5), (6, 0x7fffffff), (29, 0x7fffffff), (40, 0x40000000), (56, -1), (56, 0x7fffffff)):
        b = bytearray(good)
        struct.pack_into("<i", b, 16 + 4 * idx, val)
        out.append(bytes(b))
    out += [good[:-9], good[:400], good[:16 + 57 * 4 + 3]]
    return out


def corrupt_id_variants(m):
    v = []
    for name, idx, val in (("body_parentid", 3, 7), ("body_parentid", 2, -4), ("body_weldid", 5, 999), ("geom_bodyid", 0, -1), ("geom_bodyid", 1, 4096),
                           ("site_bodyid", 0, 77), ("wrap_objid", 0, 100000), ("tendon_adr", 1, 1 << 30), ("tendon_num", 0, -3), ("dof_parentid", 4, 9),
                           ("jnt_qposadr", 2, 500), ("jnt_dofadr", 1, -2), ("dof_bodyid", 0, 64), ("dof_jntid", 0, 64), ("jnt_bodyid", 0, -7),
                           ("body_jntadr", 3, 1 << 28), ("body_dofnum", 2, 1 << 28), ("geom_type", 0, 11)):
        mm = _with(m)
        mm.arrays[name] = np.array(mm.arrays[name]).copy()
        mm.arrays[name].reshape(-1)[idx] = val
        v.append(mm)
    return v


def test_every_unsupported_feature_is_reported_at_once_by_both_routes(models, emu_lib, tmp_path, capsys):
    """VERDICT r04 item 3.  (i) Options MuJoCo 2.1 honours and this stepper does not restate are REFUSED by both model routes, one test per
    option: opt.solver other than Newton (PGS / CG would be stepped with another algorithm), noslip_iterations > 0, non-zero density /
    viscosity / wind (fluid forces in mj_passive), actuators with integrator / filter dynamics or user gain / bias.  (ii) A model with
    several unsupported features gets ONE report listing all of them with counts — model.unsupported_features, the message of
    compile_model's ModelError, the C++ route's MyoError, and `python -m myochallenge_amd.model --check file.mjb` agree on the keys."""
    import re
    from myochallenge_amd import native
    from myochallenge_amd.mjb import dump_mjb
    from myochallenge_amd.model import _main, unsupported_features
    hand = models["hand"]

    def c_route(m, **kw):
        path = tmp_path / "m.mjb"
        path.write_bytes(dump_mjb(m))
        return native.Model.from_mjb(str(path), emu_lib, **kw)

    assert unsupported_features(hand) == []
    dyn = hand.arrays["actuator_dyntype"].copy(); dyn[:3] = 2                      # filter
    gain = hand.arrays["actuator_gaintype"].copy(); gain[0] = 2                     # user
    bias = hand.arrays["actuator_biastype"].copy(); bias[:2] = 3                    # user
    single = {"solver": dict(opt_solver=0), "solver ": dict(opt_solver=1), "noslip": dict(opt_noslip_iterations=3), "fluid": dict(opt_density=1.2),
              "fluid ": dict(opt_viscosity=1e-3), "fluid  ": dict(opt_wind=[0.0, 1.0, 0.0]), "cone": dict(opt_cone=1), "integrator": dict(opt_integrator=2),
              "actuator_dyn": dict(actuator_dyntype=dyn), "actuator_gain": dict(actuator_gaintype=gain), "actuator_bias": dict(actuator_biastype=bias)}
    for key, change in single.items():
        bad = _with(hand, **change)
        feats = unsupported_features(bad)
        assert [x["key"] for x in feats] == [key.strip()], (key, feats)
        with pytest.raises(ModelError, match=re.escape(feats[0]["message"][:30])):
            compile_model(bad)
        with pytest.raises(native.MyoError, match=r"\[%s x\d+\]" % key.strip()):
            c_route(bad)
    assert unsupported_features(_with(hand, actuator_dyntype=dyn))[0]["count"] == 3
    # the explicit opt-in of ADVICE r05: a PGS / CG / noslip model may be stepped with this stepper's Newton solver when the caller says so
    # (both routes) — and only those two entries: the same model with an elliptic cone on top is still refused
    other = _with(hand, opt_solver=1, opt_noslip_iterations=2)
    cm_o = compile_model(other, allow_other_solver=True)
    assert cm_o.size("nv") == compile_model(hand).size("nv")
    c_route(other, allow_other_solver=True)
    with pytest.raises(ModelError, match="cone"):
        compile_model(_with(other, opt_cone=1), allow_other_solver=True)
    with pytest.raises(native.MyoError, match=r"\[cone x1\]"):
        c_route(_with(other, opt_cone=1), allow_other_solver=True)
    # several at once: one report, every entry, both routes
    jt = hand.arrays["jnt_type"].copy(); jt[3] = 1                                 # a ball joint
    many = _with(hand, opt_solver=1, opt_noslip_iterations=2, opt_viscosity=0.1, opt_cone=1, actuator_biastype=bias, jnt_type=jt, neq=2)
    keys = sorted(x["key"] for x in unsupported_features(many))
    assert keys == sorted(["solver", "noslip", "fluid", "cone", "actuator_bias", "ball_joints", "equality"])
    with pytest.raises(ModelError) as e_py:
        compile_model(many)
    assert all(x["message"] in str(e_py.value) for x in unsupported_features(many))
    with pytest.raises(native.MyoError) as e_c:
        c_route(many)
    assert sorted(re.findall(r"\[(\w+) x\d+\]", str(e_c.value))) == keys
    counts_c = dict(re.findall(r"\[(\w+) x(\d+)\]", str(e_c.value)))
    assert all(int(counts_c[x["key"]]) == x["count"] for x in unsupported_features(many))
    # the command-line report
    path = tmp_path / "many.mjb"
    path.write_bytes(dump_mjb(many))
    assert _main(["--check", str(path)]) == 1
    text = capsys.readouterr().out
    assert all(("[%s] x%d" % (x["key"], x["count"])) in text for x in unsupported_features(many))
    path.write_bytes(dump_mjb(hand))
    assert _main(["--check", str(path)]) == 0


def test_explicit_pair_replaces_every_dynamic_pair_of_its_two_bodies(models, emu_lib, tmp_path):
    """mj_collision (MuJoCo 2.1) merges predefined pairs into its body-pair sweep by pair_signature = ((body1 + 1) << 16) + body2 + 1: a
    body pair that has explicit pairs gets ONLY those.  A hand body that carries two colliding geoms against a ball:
    one explicit pair between one of the two geoms and the ball removes BOTH dynamic geom pairs of that body pair, through both routes;
    other bodies' pairs with the ball are untouched."""
    from myochallenge_amd import native
    from myochallenge_amd.mjb import dump_mjb
    from host_table_cases import explicit_pair_model
    hand = models["hand"]
    base = compile_model(hand)
    gb = np.asarray(hand.geom_bodyid)
    pairs = list(zip(base.x_pair_geom1.tolist(), base.x_pair_geom2.tolist()))
    xp, body, geoms, g_ball, b_ball = explicit_pair_model(hand)      # a hand body with >= 2 geoms colliding with ball1, one explicit pair
    cm = compile_model(xp)
    kept = list(zip(cm.x_pair_geom1.tolist(), cm.x_pair_geom2.tolist(), cm.x_pair_explicit.tolist()))
    between = [(a, b, x) for a, b, x in kept if {int(gb[a]), int(gb[b])} == {body, b_ball}]
    assert len(between) == 1 and between[0][2] == 0 and {between[0][0], between[0][1]} == {geoms[0], g_ball}      # only the explicit pair is left
    assert len(kept) == len(pairs) - (len(geoms) - 1)                                                             # nothing else changed
    path = tmp_path / "xp.mjb"
    path.write_bytes(dump_mjb(xp))
    assert native.Model.from_mjb(str(path), emu_lib).size("npair") == len(kept)
