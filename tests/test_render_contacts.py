"""Contact points and contact forces in the batched renderer (include/myobatch.h myo_batch_contact_items, MYO_RENDER_CONTACTS,
myo_render_style; csrc/myo_render.h): the items against ``sensors()`` of the same state, the force balance on the free objects, the
image against the numpy yardstick tests/render_ref.py, "off means off" and read-only, the style, a batch without contacts, and the
arguments / Python / command-line surface — on the emulation build here, on the MI355X under -m gpu.  The cases and their bounds
are in tests/contact_render_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_render_cases as cc  # noqa: E402
from test_render import decode_png  # noqa: E402

from myochallenge_amd import native  # noqa: E402

DTYPES = [native.MYO_F64, native.MYO_MIXED]
KINDS = ["baoding", "die"]
# (kind, tendons, camera elevation): the Baoding balls press DOWN on the palm, so the shafts of the forces on the palm's geoms leave
# the hand on its back — seen by a camera below the hand looking up; the die's contacts point every way
IMAGE_CASES = [("baoding", False, 45.0), ("baoding", True, 45.0), ("die", False, -45.0)]


# ------------------------------------------------------------------------------------------------ 1. items against sensors()
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_items_match_the_sensors_of_the_same_state(emu_lib, kind, dtype):
    cc.case_items_match_sensors(emu_lib, dtype, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_items_match_the_sensors_of_the_same_state(hip_lib, kind, dtype):
    cc.case_items_match_sensors(hip_lib, dtype, kind)


# ------------------------------------------------------------------------------------------------ 2. force balance
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_force_shafts_sum_to_the_objects_contact_wrench(emu_lib, kind, dtype):
    cc.case_force_balance(emu_lib, dtype, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_force_shafts_sum_to_the_objects_contact_wrench(hip_lib, kind, dtype):
    cc.case_force_balance(hip_lib, dtype, kind)


# ------------------------------------------------------------------------------------------------ 3. image against the yardstick
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,tendons,elevation", IMAGE_CASES)
def test_contact_image_matches_the_yardstick(emu_lib, kind, tendons, elevation, dtype):
    cc.case_image(emu_lib, dtype, kind, tendons, elevation)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,tendons,elevation", IMAGE_CASES)
def test_gpu_contact_image_matches_the_yardstick(hip_lib, kind, tendons, elevation, dtype):
    cc.case_image(hip_lib, dtype, kind, tendons, elevation)


@pytest.mark.parametrize("dtype", DTYPES)
def test_seventy_rows_and_a_ragged_tile(emu_lib, dtype):
    cc.case_many_envs(emu_lib, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_seventy_rows_and_a_ragged_tile(hip_lib, dtype):
    cc.case_many_envs(hip_lib, dtype)


# ------------------------------------------------------------------------------------------------ 4. off means off, read-only
@pytest.mark.parametrize("dtype", DTYPES)
def test_without_the_flag_the_image_is_what_it_was(emu_lib, dtype):
    cc.case_off_means_off(emu_lib, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_without_the_flag_the_image_is_what_it_was(hip_lib, dtype):
    cc.case_off_means_off(hip_lib, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_contact_drawing_leaves_the_steps_bitwise_unchanged(emu_lib, dtype):
    cc.case_read_only(emu_lib, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_contact_drawing_leaves_the_steps_bitwise_unchanged(hip_lib, dtype):
    cc.case_read_only(hip_lib, dtype)


# ------------------------------------------------------------------------------------------------ 5. style
@pytest.mark.parametrize("dtype", DTYPES)
def test_render_style_round_trip_refusals_and_effect(emu_lib, dtype):
    cc.case_style(emu_lib, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_render_style_round_trip_refusals_and_effect(hip_lib, dtype):
    cc.case_style(hip_lib, dtype)


# ------------------------------------------------------------------------------------------------ 6. a pose batch
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_batch_without_contacts_draws_nothing_more(emu_lib, dtype):
    cc.case_pose_batch(emu_lib, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_a_batch_without_contacts_draws_nothing_more(hip_lib, dtype):
    cc.case_pose_batch(hip_lib, dtype)


# ------------------------------------------------------------------------------------------------ 7. arguments and surface
def _check_arguments(lib):
    assert native.RENDER_CONTACTS == 32
    for sym in ("myo_batch_contact_items", "myo_batch_set_render_style", "myo_batch_get_render_style"):
        assert sym in native.EXPORTED_SYMBOLS and sym in native.ENV_PATH_SYMBOLS and hasattr(lib.L, sym)
    env, _, items = cc.shared_env(lib, native.MYO_MIXED, "baoding")
    import torch
    b, L = env.batch, lib.L
    idx = torch.arange(2, dtype=torch.int32, device=env.device)
    out = torch.zeros((2, items.shape[1], cc.N), dtype=torch.float64, device=env.device)
    assert L.myo_batch_contact_items(b.h, idx.data_ptr(), 2, out.data_ptr(), env._stream()) == 0
    assert L.myo_batch_contact_items(b.h, idx.data_ptr(), 0, out.data_ptr(), env._stream()) == 0           # k = 0: an empty result
    for args in ((b.h, idx.data_ptr(), 2, None, None), (b.h, idx.data_ptr(), -1, out.data_ptr(), None), (b.h, None, 2, out.data_ptr(), None),
                 (None, idx.data_ptr(), 2, out.data_ptr(), None)):
        assert L.myo_batch_contact_items(*args) == -1                 # MYO_E_ARG
        assert L.myo_last_error()
    rgb = torch.zeros((2, 16, 16, 3), dtype=torch.uint8, device=env.device)
    with pytest.raises(native.MyoError, match="unknown flag"):
        b.render(idx, [env.default_camera()], 16, 16, native.RENDER_RGB | 64, rgb)
    with pytest.raises(native.MyoError, match="unknown flag"):
        b.render(idx, [env.default_camera()], 16, 16, native.RENDER_RGB | native.RENDER_CONTACTS | 64, rgb)
    b.render(idx, [env.default_camera()], 16, 16, native.RENDER_RGB | native.RENDER_CONTACTS, rgb)


def _check_surface(lib):
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    env, _, items = cc.shared_env(lib, native.MYO_MIXED, "baoding")
    n, cap = env.num_envs, env.batch.contact_capacity
    cam = {"distance": 0.25}
    out = env.render_tensor([2, 0], 32, 24, cam, rgb=True, depth=True, segmentation=True, contacts=True)
    assert tuple(out["rgb"].shape) == (2, 24, 32, 3) and str(out["rgb"].dtype) == "torch.uint8"
    assert tuple(out["depth"].shape) == (2, 24, 32) and str(out["depth"].dtype) == "torch.float32"
    assert tuple(out["segmentation"].shape) == (2, 24, 32) and str(out["segmentation"].dtype) == "torch.int32"
    ci = env.contact_items()
    assert tuple(ci.shape) == (n, 2 * cap, cc.N) and str(ci.dtype) == "torch.float64" and tuple(env.contact_items([1]).shape) == (1, 2 * cap, cc.N)
    with pytest.raises(ValueError):
        env.contact_items([n])
    try:
        on = env.get_images(width=32, height=24, camera=cam, contacts=True, contact_style={"geom_alpha": 0.5})
        assert env.batch.get_render_style()["geom_alpha"] == 0.5                       # the style stays set
        off = env.get_images(width=32, height=24, camera=cam)
        assert len(on) == n and on[0].shape == (24, 32, 3) and on[0].dtype == np.uint8 and any(not np.array_equal(a, b) for a, b in zip(on, off))
        tile = env.render("rgb_array", contacts=True, width=32, height=24, camera=cam)
        assert tile.ndim == 3 and tile.shape[2] == 3 and tile.dtype == np.uint8
        assert not np.array_equal(tile, env.render("rgb_array", width=32, height=24, camera=cam))
        vn = VecNormalize(env)
        assert np.array_equal(cc._np(vn.contact_items([1, 0])), items[[1, 0]])
        assert all(np.array_equal(a, b) for a, b in zip(vn.get_images(width=32, height=24, camera=cam, contacts=True), on))
        assert np.array_equal(vn.render("rgb_array", contacts=True, width=32, height=24, camera=cam), tile)
        t = vn.render_tensor([1], 16, 16, cam, rgb=False, segmentation=True, contacts=True)
        assert tuple(t["segmentation"].shape) == (1, 16, 16)
    finally:
        env.batch.set_render_style(**cc.DEFAULT_STYLE)


def test_contact_items_argument_errors_flags_and_symbols(emu_lib):
    _check_arguments(emu_lib)


@pytest.mark.gpu
def test_gpu_contact_items_argument_errors_flags_and_symbols(hip_lib):
    _check_arguments(hip_lib)


def test_env_and_vecnormalize_surface(emu_lib):
    _check_surface(emu_lib)


@pytest.mark.gpu
def test_gpu_env_and_vecnormalize_surface(hip_lib):
    _check_surface(hip_lib)


def test_render_style_struct_matches_the_header():
    assert C.sizeof(native.RenderStyle) == 8 + 4 * 8 + 2 * 16 + 8
    assert native.RenderStyle.geom_alpha.offset == 72 and native.RenderStyle.point_rgba.offset == 40


def _check_main_eval(lib, golden_dir, tmp_path, capsys):
    from helpers import make_env
    from myochallenge_amd.main_eval import evaluate, main
    model, envp = os.path.join(golden_dir, "phase1_final.zip"), os.path.join(golden_dir, "normalized_env_phase1_final.pkl")
    for extra in (["--render-contacts"], ["--render-contacts", "--render-geom-alpha", "0.5"], ["--render-dir", "x", "--render-geom-alpha", "0.5"]):
        with pytest.raises(SystemExit) as ex:
            main(["--model", model, "--env-path", envp] + extra)
        assert ex.value.code == 2                                      # argparse's usage error
        assert ("--render-contacts needs --render-dir" if extra[0] == "--render-contacts" else "--render-geom-alpha needs --render-contacts") in capsys.readouterr().err
    env = make_env("CustomMyoBaodingBallsP1", lib, num_envs=2, seed=3, max_episode_steps=4)
    frames = tmp_path / "frames"
    plain = tmp_path / "plain"
    res, _ = evaluate(model, envp, "CustomMyoBaodingBallsP1", config={}, num_episodes=2, num_envs=2, seed=3, verbose=False, render_dir=str(frames),
                      render_envs=2, render_size=(40, 30), render_contacts=True, render_geom_alpha=0.5, env=env)
    files = sorted(os.listdir(frames))
    assert len(files) == 2 * int(res["lengths"].max()) and any(f.startswith("env1_") for f in files)
    imgs = [decode_png(open(frames / f, "rb").read()) for f in files]
    assert all(i.shape == (30, 40, 3) for i in imgs) and imgs[0].std() > 0
    assert env.batch.get_render_style()["geom_alpha"] == 0.5
    env.close()
    env = make_env("CustomMyoBaodingBallsP1", lib, num_envs=2, seed=3, max_episode_steps=4)
    evaluate(model, envp, "CustomMyoBaodingBallsP1", config={}, num_episodes=2, num_envs=2, seed=3, verbose=False, render_dir=str(plain),
             render_envs=2, render_size=(40, 30), env=env)
    env.close()
    assert sorted(os.listdir(plain)) == files
    assert any(not np.array_equal(decode_png(open(plain / f, "rb").read()), i) for f, i in zip(files, imgs))      # the switch draws something


def test_main_eval_render_contacts_on_emulation(emu_lib, golden_dir, tmp_path, capsys):
    _check_main_eval(emu_lib, golden_dir, tmp_path, capsys)


@pytest.mark.gpu
def test_gpu_main_eval_render_contacts(hip_lib, golden_dir, tmp_path, capsys):
    _check_main_eval(hip_lib, golden_dir, tmp_path, capsys)
