"""True-reference hooks: tools/dump_mujoco_trajectory.py writes per-substep MuJoCo trajectories in
a fixed .npz format; every tests/golden/mujoco_traj_*.npz found here is replayed through the oracle (CPU) and the
HIP stepper (-m gpu).  None can be produced in the build image (no MuJoCo), so what runs by default is the unit
test of the FORMAT, with the oracle as the stand-in producer on the finger model the reference ships."""
import glob
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dump_mujoco_trajectory as dmt  # noqa: E402

from helpers import Mem  # noqa: E402
from myochallenge_amd import native  # noqa: E402
from myochallenge_amd.mjb import load_mjb  # noqa: E402
from myochallenge_amd.model import compile_model  # noqa: E402
from oracle.oracle import OracleData, OracleModel  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TRUE_FILES = sorted(glob.glob(os.path.join(GOLDEN, "mujoco_traj_*.npz")))


def load_traj(path):
    z = np.load(path, allow_pickle=False)
    assert set(dmt.FORMAT_KEYS) <= set(z.files), set(dmt.FORMAT_KEYS) - set(z.files)
    meta = json.loads(str(z["meta"]))
    T = z["ctrl"].shape[0]
    assert z["qpos"].shape == (T + 1, meta["nq"]) and z["qvel"].shape == (T + 1, meta["nv"]) and z["act"].shape == (T + 1, meta["na"])
    assert z["qacc_warmstart"].shape == (T + 1, meta["nv"]) and z["ncon"].shape == (T,) and z["solver_iter"].dtype == np.int32
    return meta, z


def model_for(meta, models):
    name = meta["model"]
    if name == "synthetic_hand":
        return models["hand"]
    path = os.path.join(GOLDEN, name)
    if not os.path.exists(path):
        pytest.skip(f"model file {name} of this trajectory is not in tests/golden")
    return load_mjb(path)


def replay_oracle(meta, z, mj, resync_every=None):
    """Step the oracle along the recorded controls from the recorded initial state; returns the per-substep
    relative qpos error.  resync_every: copy the recorded state in every k substeps (local error instead of drift)."""
    cm = compile_model(mj, unsupported_contacts="drop")
    d = OracleData(OracleModel(cm.to_blob()))
    T = z["ctrl"].shape[0]
    err = np.zeros(T)
    for t in range(T):
        if t == 0 or (resync_every and t % resync_every == 0):
            d.qpos[:], d.qvel[:] = z["qpos"][t], z["qvel"][t]
            if meta["na"]:
                d.act[:] = z["act"][t]
            d.qacc_warmstart[:] = z["qacc_warmstart"][t]
        d.ctrl[:] = z["ctrl"][t]
        d.step()
        err[t] = np.abs(np.array(d.qpos) - z["qpos"][t + 1]).max() / max(1e-30, np.abs(z["qpos"][t + 1]).max())
    return err


def replay_stepper(lib, dtype, meta, z, mj):
    mem = Mem(lib)
    cm = compile_model(mj, unsupported_contacts="drop")
    b = native.Batch(native.Model(cm, lib), None, 2, 0, 0, dtype)
    two = lambda a: mem.arr(np.tile(np.asarray(a, float), (2, 1)))
    b.set_state(two(z["qpos"][0]), two(z["qvel"][0]), two(z["act"][0]) if meta["na"] else None, mem.zeros(2))
    b.warmstart(set=two(z["qacc_warmstart"][0]))
    T = z["ctrl"].shape[0]
    qp = mem.zeros((2, meta["nq"]))
    err = np.zeros(T)
    for t in range(T):
        b.physics_step(two(z["ctrl"][t]), 1)
        b.get_state(qp)
        err[t] = np.abs(mem.host(qp)[1] - z["qpos"][t + 1]).max() / max(1e-30, np.abs(z["qpos"][t + 1]).max())
    b.close()
    return err


def test_trajectory_file_format_roundtrip(tmp_path, emu_lib, models):
    """Format unit test: the oracle as stand-in producer on the reference's finger model; the file must load,
    carry every documented field, replay exactly through the oracle, and replay through the stepper."""
    out = str(tmp_path / "traj_finger_oracle.npz")
    meta = dmt.dump("oracle", os.path.join(GOLDEN, "myo_finger_v0.mjb"), out, substeps=300, seed=1, hold=10)
    assert meta["producer"] == "oracle" and meta["is_true_reference"] is False and meta["model"] == "myo_finger_v0.mjb"
    m2, z = load_traj(out)
    assert m2 == meta and z["ctrl"].shape == (300, meta["nu"])
    assert (np.diff(z["ctrl"][:10], axis=0) == 0).all() and (z["ctrl"][10] != z["ctrl"][9]).any()      # held for `hold` substeps
    mj = model_for(meta, models)
    assert replay_oracle(meta, z, mj).max() == 0.0                         # the producer replays itself bit for bit
    assert replay_oracle(meta, z, mj, resync_every=50).max() == 0.0        # and the recorded warm start is the real one
    assert replay_stepper(emu_lib, native.MYO_F64, meta, z, mj).max() < 1e-9
    # the flailing finger is chaotic (the fp64 stepper's 3e-16 of the first substep is 3e-11 after 300): the mixed
    # stepper's 1e-7 stays under north_star's 1e-4 for the first 100 substeps
    assert replay_stepper(emu_lib, native.MYO_MIXED, meta, z, mj)[:100].max() < 1e-4


def test_dump_tool_reports_missing_mujoco():
    for backend in ("mujoco_py", "mujoco"):
        try:
            __import__(backend)
        except Exception:
            with pytest.raises(Exception):
                dmt.dump(backend, os.path.join(GOLDEN, "myo_finger_v0.mjb"), "/dev/null", substeps=1)


@pytest.mark.parametrize("path", TRUE_FILES or [None])
def test_oracle_against_true_mujoco_trajectories(path, models):
    """PINS THE ORACLE'S STEPPING when a user has produced goldens with MuJoCo (none ship: MuJoCo is absent here)."""
    if path is None:
        pytest.skip("no tests/golden/mujoco_traj_*.npz (produce with tools/dump_mujoco_trajectory.py on a machine with MuJoCo 2.1)")
    meta, z = load_traj(path)
    if not meta["is_true_reference"]:
        pytest.skip("stand-in producer")
    mj = model_for(meta, models)
    assert replay_oracle(meta, z, mj, resync_every=100).max() < 1e-6       # local error per 100 substeps
    assert replay_oracle(meta, z, mj).max() < 1e-4                         # north_star's trajectory tolerance


@pytest.mark.gpu
@pytest.mark.parametrize("path", TRUE_FILES or [None])
def test_hip_stepper_against_true_mujoco_trajectories(path, models, hip_lib, tmp_path):
    """PINS THE HIP STEPPER to every true MuJoCo trajectory in tests/golden.  While none ships (`path` None), the same file route runs
    on the device with the oracle as the stand-in producer on the reference's finger model — what test_trajectory_file_format_roundtrip
    does on the emulation build: a written trajectory loads and replays through the HIP steppers, fp64 at the precision of
    test_gpu_parity.py::test_trajectory_small_models over the first 100 substeps and within north_star's 1e-4 over all 300."""
    if path is None:
        out = str(tmp_path / "traj_finger_oracle.npz")
        meta = dmt.dump("oracle", os.path.join(GOLDEN, "myo_finger_v0.mjb"), out, substeps=300, seed=1, hold=10)
        m2, z = load_traj(out)
        assert m2 == meta and meta["is_true_reference"] is False and z["ctrl"].shape == (300, meta["nu"])
        mj = model_for(meta, models)
        err = replay_stepper(hip_lib, native.MYO_F64, meta, z, mj)
        assert err[:100].max() < 1e-8 and err.max() < 1e-4, (err[:100].max(), err.max())
        assert replay_stepper(hip_lib, native.MYO_MIXED, meta, z, mj)[:100].max() < 1e-4
        return
    meta, z = load_traj(path)
    if not meta["is_true_reference"]:
        pytest.skip("stand-in producer")
    mj = model_for(meta, models)
    assert replay_stepper(hip_lib, native.MYO_F64, meta, z, mj).max() < 1e-4
