"""ctypes binding of libmyobatch (C ABI: include/myobatch.h).

The product library is ``myochallenge_amd/libmyobatch.so`` built by ``__graft_entry__.build()``
with hipcc for gfx950.  There is no CPU fallback: if the library is missing, ``load()`` raises.
(``tests/emu`` builds a lane-serial emulation of the same kernel source for debugging; tests
load it by passing its explicit path — nothing in the package ever does.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmyobatch.so")

MYO_F64, MYO_MIXED = 0, 1     # stepper arithmetic: all fp64 | mixed (fp64 state, kinematic chain, contact distances; fp32 dynamics)
MYO_F32 = MYO_MIXED             # the name of round 1, when dtype 1 was a pure fp32 stepper
TASK_NONE, TASK_BAODING_P1, TASK_BAODING_P2, TASK_REORIENT, TASK_POSE = 0, 1, 2, 3, 4
POSE_RESET_INIT, POSE_RESET_RANDOM, POSE_RESET_SDS = 0, 1, 2
POSE_TARGET_GENERATE, POSE_TARGET_FIXED = 0, 1
CHOICE_FIXED, CHOICE_CW, CHOICE_CCW, CHOICE_RANDOM = 0, 1, 2, 3
MUSCLE_NONE, MUSCLE_FATIGUE, MUSCLE_REAFFERENTATION = 0, 1, 2      # myo_task_cfg.muscle_condition
N_RWD = 8
RWD_KEYS = ("pos_dist_1", "pos_dist_2", "act_reg", "alive", "sparse", "solved", "done", "dense")


ROT_CHOICE_MAX, OBJG_MAX, POSE_NQ_MAX = 4, 20, 38      # include/myobatch.h


class TaskCfg(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("frame_skip", C.c_int32), ("max_episode_steps", C.c_int32),
        ("n_hand", C.c_int32),
        ("obj1_sid", C.c_int32), ("obj2_sid", C.c_int32), ("target1_sid", C.c_int32),
        ("target2_sid", C.c_int32), ("obj1_bid", C.c_int32), ("obj2_bid", C.c_int32),
        ("obj1_gid", C.c_int32), ("obj2_gid", C.c_int32),
        ("task_choice", C.c_int32), ("enable_rsi", C.c_int32), ("balls_overlap", C.c_int32),
        ("limit_init_angle_on", C.c_int32), ("beta_init_angle_on", C.c_int32),
        ("beta_ball_size_on", C.c_int32), ("beta_ball_mass_on", C.c_int32),
        ("drop_th", C.c_double), ("proximity_th", C.c_double), ("center_pos", C.c_double * 2),
        ("weights", C.c_double * 7),
        ("goal_time_period", C.c_double * 2), ("goal_xrange", C.c_double * 2),
        ("goal_yrange", C.c_double * 2),
        ("rsi_probability", C.c_double), ("overlap_probability", C.c_double),
        ("noise_palm", C.c_double), ("noise_fingers", C.c_double), ("noise_balls", C.c_double),
        ("limit_init_angle", C.c_double), ("beta_init_angle", C.c_double * 2),
        ("beta_ball_size", C.c_double * 2), ("beta_ball_mass", C.c_double * 2),
        ("obj_size_range", C.c_double * 2), ("obj_mass_range", C.c_double * 2),
        ("obj_friction_change", C.c_double * 3), ("init_qpos0", C.c_double),
        # die reorient (kind TASK_REORIENT)
        ("ro_weights", C.c_double * 9), ("ro_goal_pos", C.c_double * 2), ("ro_goal_rot", C.c_double * 2),
        ("ro_n_rot_choice", C.c_int32 * 3), ("ro_pad_", C.c_int32),
        ("ro_rot_choice", C.c_double * 2 * ROT_CHOICE_MAX * 3),
        ("ro_obj_size_change", C.c_double), ("ro_pos_th", C.c_double), ("ro_rot_th", C.c_double),
        ("ro_goal_init_pos", C.c_double * 3), ("ro_goal_obj_offset", C.c_double * 3),
        ("ro_rsi_distance_pos", C.c_double), ("ro_rsi_distance_rot", C.c_double),
        # joint pose (kind TASK_POSE)
        ("pose_weights", C.c_double * 7),
        ("pose_thd", C.c_double), ("pose_far_th", C.c_double), ("pose_sds_distance", C.c_double),
        ("pose_target_distance", C.c_double),
        ("pose_reset_type", C.c_int32), ("pose_target_type", C.c_int32),
        ("pose_init_qpos", C.c_double * POSE_NQ_MAX), ("pose_target_value", C.c_double * POSE_NQ_MAX),
        ("pose_target_range", C.c_double * 2 * POSE_NQ_MAX), ("pose_reset_range", C.c_double * 2 * POSE_NQ_MAX),
        # muscle condition (every kind): MUSCLE_*; reafferentation's actuators; fatigue's rates
        ("muscle_condition", C.c_int32), ("reaf_src", C.c_int32), ("reaf_dst", C.c_int32),
        ("fatigue_F", C.c_double), ("fatigue_R", C.c_double), ("fatigue_r", C.c_double),
    ]


class MlpLayout(C.Structure):
    """myo_mlp_layout of include/myobatch.h: element offsets of the MLP actor-critic's tensors in the flat vector, [0] actor / [1] critic."""
    _fields_ = [
        ("off_W1", C.c_int64 * 2), ("off_b1", C.c_int64 * 2), ("off_W2", C.c_int64 * 2), ("off_b2", C.c_int64 * 2),
        ("off_Wh", C.c_int64 * 2), ("off_bh", C.c_int64 * 2), ("off_log_std", C.c_int64),
    ]


class PpoMlpDesc(C.Structure):
    """myo_ppo_mlp_desc of include/myobatch.h (one fused PPO minibatch step of the MLP actor-critic)."""
    _fields_ = [
        ("obs", C.c_void_p), ("act", C.c_void_p), ("oldlp", C.c_void_p), ("adv", C.c_void_p), ("ret", C.c_void_p), ("idx", C.c_void_p),
        ("B", C.c_int32), ("O", C.c_int32), ("A", C.c_int32), ("hidden", C.c_int32),
        ("params", C.c_void_p), ("grads", C.c_void_p), ("G", C.c_int64), ("layout", MlpLayout),
        ("clip", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float), ("compute_adv_stats", C.c_int32),
        ("adv_stats", C.c_void_p), ("acc", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
        ("sqnorm_part", C.c_void_p), ("adam_step", C.c_void_p), ("hp", C.c_void_p),
    ]


# word indices of the PPO hyper-parameter block (MYO_HP_* of include/myobatch.h)
HP_LR, HP_CLIP, HP_KL_LIMIT, HP_STOP, HP_APPLIED, HP_COUNT, HP_SUM_KL, HP_SUM_CLIPFRAC, HP_SUM_ENTLOSS, HP_LAST_KL, HP_LAST_PL, HP_LAST_VL = range(12)
HP_WORDS = 16
# activation codes of the hidden MLP layers (MYO_ACT_* of include/myobatch.h)
ACT_RELU, ACT_TANH = 0, 1


class PpoMlpRolloutDesc(C.Structure):
    """myo_ppo_mlp_rollout_desc of include/myobatch.h (one env step's policy call of the rollout, MLP actor-critic)."""
    _fields_ = [
        ("obs", C.c_void_p), ("N", C.c_int32), ("O", C.c_int32), ("A", C.c_int32), ("hidden", C.c_int32), ("params", C.c_void_p),
        ("layout", MlpLayout),
        ("seed", C.c_uint64), ("draw_counter", C.c_void_p), ("t_idx", C.c_void_p),
        ("obs_buf", C.c_void_p), ("act_buf", C.c_void_p), ("val_buf", C.c_void_p), ("logp_buf", C.c_void_p), ("clipped", C.c_void_p),
        ("deterministic", C.c_int32), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64),
    ]


class AdamDesc(C.Structure):
    """myo_adam_desc of include/myobatch.h (clip_grad_norm_ + one Adam step over a flat fp32 vector)."""
    _fields_ = [
        ("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int32),
        ("lr", C.c_float), ("b1", C.c_float), ("b2", C.c_float), ("eps", C.c_float), ("max_norm", C.c_float), ("grad_scale", C.c_float),
        ("step", C.c_void_p), ("scratch", C.c_void_p), ("nparts", C.c_int32),
        ("p_bf16", C.c_void_p), ("hp", C.c_void_p), ("images", C.POINTER(PpoMlpDesc)),
    ]


class EnsembleDesc(C.Structure):
    """myo_ensemble_desc of include/myobatch.h (one acting step of an ensemble of actor-only LSTM policies)."""
    _fields_ = [
        ("N", C.c_int32), ("O", C.c_int32), ("A", C.c_int32), ("H", C.c_int32), ("M0", C.c_int32), ("M1", C.c_int32),
        ("obs", C.c_void_p), ("mean", C.c_void_p), ("var", C.c_void_p), ("eps", C.c_double), ("clip", C.c_double),
        ("w_gates", C.c_void_p), ("w_a", C.c_void_p), ("b_gates", C.c_void_p), ("b_a", C.c_void_p),
        ("h", C.c_void_p), ("c", C.c_void_p), ("start0", C.c_void_p), ("start1", C.c_void_p), ("use_group1", C.c_void_p),
        ("act", C.c_void_p), ("member_act", C.c_void_p),
    ]


class RenderCamera(C.Structure):
    """myo_render_camera of include/myobatch.h: MuJoCo's free camera, angles in degrees."""
    _fields_ = [("lookat", C.c_double * 3), ("distance", C.c_double), ("azimuth", C.c_double), ("elevation", C.c_double),
                ("fovy", C.c_double)]


RENDER_RGB, RENDER_DEPTH, RENDER_SEG, RENDER_SITES, RENDER_TENDONS, RENDER_CONTACTS = 1, 2, 4, 8, 16, 32      # (bit 64 is reserved)
RENDER_ITEM_N = 24      # doubles per item of myo_batch_geom_poses / myo_batch_tendon_paths / myo_batch_contact_items


class RenderStyle(C.Structure):
    """myo_render_style of include/myobatch.h: how contact points and contact forces are drawn (this library's own rule)."""
    _fields_ = [("size", C.c_size_t), ("disc_radius", C.c_double), ("disc_half_height", C.c_double), ("force_radius", C.c_double),
                ("metres_per_newton", C.c_double), ("point_rgba", C.c_float * 4), ("force_rgba", C.c_float * 4), ("geom_alpha", C.c_double)]


RENDER_STYLE_KEYS = tuple(f[0] for f in RenderStyle._fields_[1:])


class SenseOut(C.Structure):
    """myo_sense_out of include/myobatch.h: caller-owned device arrays of myo_batch_sense, any of them NULL."""
    _fields_ = [("size", C.c_size_t), ("ncon", C.c_void_p), ("con_geom", C.c_void_p), ("con_d", C.c_void_p), ("body_wrench", C.c_void_p),
                ("qfrc_constraint", C.c_void_p), ("act_length", C.c_void_p), ("act_velocity", C.c_void_p), ("act_force", C.c_void_p),
                ("activation", C.c_void_p), ("ten_length", C.c_void_p), ("ten_velocity", C.c_void_p)]


SENSE_KEYS = tuple(f[0] for f in SenseOut._fields_[1:])
SENSE_CON_N = 13        # doubles per contact of con_d: dist, pos[3], normal[3], force[6]


class DataOut(C.Structure):
    """myo_data_out of include/myobatch.h: caller-owned device arrays (doubles) of myo_batch_data, any of them NULL."""
    _fields_ = [("size", C.c_size_t)] + [(k, C.c_void_p) for k in (
        "xpos", "xquat", "xmat", "xipos", "subtree_com", "geom_xpos", "geom_xmat", "site_xpos", "cvel", "qM", "ten_J", "actuator_moment",
        "qfrc_bias", "qfrc_passive", "qfrc_actuator", "qacc_smooth", "qacc", "act_dot")]


DATA_KEYS = tuple(f[0] for f in DataOut._fields_[1:])


class JacOut(C.Structure):
    """myo_jac_out of include/myobatch.h: caller-owned device arrays (doubles, [N, k, 3, nv]) of myo_batch_jac, either may be NULL."""
    _fields_ = [("size", C.c_size_t), ("jacp", C.c_void_p), ("jacr", C.c_void_p)]


class InverseOut(C.Structure):
    """myo_inverse_out of include/myobatch.h: caller-owned device arrays (doubles, [N, nv]) of myo_batch_inverse, either may be NULL."""
    _fields_ = [("size", C.c_size_t), ("qfrc_inverse", C.c_void_p), ("qfrc_constraint", C.c_void_p)]


class StaticOptIn(C.Structure):
    """myo_static_opt_in of include/myobatch.h: device arrays (doubles) and scalars of myo_batch_static_opt; every pointer but qfrc may be NULL."""
    _fields_ = [("size", C.c_size_t), ("qfrc", C.c_void_p), ("weight", C.c_void_p), ("u_ref", C.c_void_p), ("lower", C.c_void_p),
                ("upper", C.c_void_p), ("weight_per_env", C.c_int), ("reg", C.c_double), ("max_iter", C.c_int)]


class StaticOptOut(C.Structure):
    """myo_static_opt_out of include/myobatch.h: caller-owned device arrays of myo_batch_static_opt (doubles; iters / status int32), any of them NULL."""
    _fields_ = [("size", C.c_size_t)] + [(k, C.c_void_p) for k in ("u", "force", "qfrc", "residual", "gain", "bias", "kkt", "iters", "status")]


STATIC_OPT_KEYS = tuple(f[0] for f in StaticOptOut._fields_[1:])
STATIC_OPT_CAP, STATIC_OPT_PINNED = 1, 4      # MYO_STATIC_OPT_* of include/myobatch.h: bits of `status`



class IkIn(C.Structure):
    """myo_ik_in of include/myobatch.h: device arrays (site_ids int32, the others doubles) and scalars of myo_batch_ik; every pointer but
    site_ids / targets (k > 0) may be NULL."""
    _fields_ = [("size", C.c_size_t), ("site_ids", C.c_void_p), ("k", C.c_int), ("targets", C.c_void_p), ("weight", C.c_void_p),
                ("weight_per_env", C.c_int), ("q_init", C.c_void_p), ("q_ref", C.c_void_p), ("lower", C.c_void_p), ("upper", C.c_void_p),
                ("active", C.c_uint64), ("reg", C.c_double), ("tol", C.c_double), ("max_iter", C.c_int)]


class IkOut(C.Structure):
    """myo_ik_out of include/myobatch.h: caller-owned device arrays of myo_batch_ik (doubles; iters / status int32), any of them NULL."""
    _fields_ = [("size", C.c_size_t)] + [(k, C.c_void_p) for k in ("qpos", "site_xpos", "residual", "cost", "kkt", "iters", "status")]


IK_KEYS = tuple(f[0] for f in IkOut._fields_[1:])
IK_CAP, IK_STALL, IK_PINNED = 1, 2, 4      # MYO_IK_* of include/myobatch.h: bits of `status`
IK_K_MAX = 16                              # MYO_IK_K_MAX of include/myobatch.h
IK_WS_DOUBLES = 2448                       # MYO_IK_WS_N of csrc/myo_ik.h: doubles per env of the library's own workspace


class SimIn(C.Structure):
    """myo_sim_in of include/myobatch.h: device arrays (env_idx / site_ids int32, the others doubles) and scalars of myo_batch_simulate;
    every pointer may be NULL."""
    _fields_ = [("size", C.c_size_t), ("env_idx", C.c_void_p), ("k", C.c_int), ("S", C.c_int), ("T", C.c_int), ("nsub", C.c_int),
                ("every", C.c_int), ("ctrl", C.c_void_p), ("ctrl_per_sample", C.c_int), ("qpos0", C.c_void_p), ("qvel0", C.c_void_p),
                ("act0", C.c_void_p), ("site_ids", C.c_void_p), ("ns", C.c_int)]


class SimOut(C.Structure):
    """myo_sim_out of include/myobatch.h: caller-owned device arrays of myo_batch_simulate (doubles; bad / steps int32), any of them NULL."""
    _fields_ = [("size", C.c_size_t)] + [(k, C.c_void_p) for k in ("qpos", "qvel", "act", "time", "site_xpos", "bad", "steps")]


SIM_KEYS = tuple(f[0] for f in SimOut._fields_[1:])
SIM_NS_MAX = 16                            # MYO_SIM_NS_MAX of include/myobatch.h

JAC_BODY, JAC_BODYCOM, JAC_SITE, JAC_GEOM, JAC_SUBTREECOM = range(5)      # MYO_JAC_* of include/myobatch.h
JAC_KINDS = {"body": JAC_BODY, "bodycom": JAC_BODYCOM, "site": JAC_SITE, "geom": JAC_GEOM, "subtreecom": JAC_SUBTREECOM}


TABLE_DTYPES = (np.int32, np.uint64, np.float32, np.float64)      # MYO_TABLE_* of include/myobatch.h


class MyoError(RuntimeError):
    pass


class NativeLib:
    def __init__(self, path: str):
        if not os.path.exists(path):
            raise MyoError(
                f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()').  libmyobatch has no CPU fallback.")
        L = C.CDLL(path)
        self.path = path
        self.L = L
        vp, i32, u64, dbl = C.c_void_p, C.c_int, C.c_uint64, C.c_double
        L.myo_last_error.restype = C.c_char_p
        L.myo_version.restype = C.c_char_p
        L.myo_model_from_blob.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.myo_model_load_mjb.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
        L.myo_model_destroy.argtypes = [vp]
        L.myo_model_size.argtypes = [vp, C.c_char_p]
        L.myo_model_table.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(i32)]
        L.myo_batch_create.argtypes = [vp, C.POINTER(TaskCfg), i32, i32, u64, i32, C.POINTER(vp)]
        L.myo_batch_destroy.argtypes = [vp]
        L.myo_batch_num_envs.argtypes = [vp]
        L.myo_batch_set_step_generation.argtypes = [vp, C.c_uint32]
        L.myo_batch_health.argtypes = [vp, C.POINTER(i32)]
        L.myo_debug_wave_slots.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(i32)]
        L.myo_batch_obs_dim.argtypes = [vp]
        L.myo_batch_lds_bytes.argtypes = [vp]
        L.myo_batch_reset.argtypes = [vp, vp, vp, vp]
        L.myo_batch_step.argtypes = [vp] * 10
        L.myo_batch_step_inner.argtypes = [vp] * 6
        L.myo_batch_step_inner_idx.argtypes = [vp, vp, i32, vp, vp, vp, vp]
        L.myo_batch_copy_envs.argtypes = [vp, vp, vp, vp, i32, vp]
        L.myo_batch_physics_step.argtypes = [vp, vp, i32, vp]
        L.myo_batch_get_state.argtypes = [vp] * 6
        L.myo_batch_set_state.argtypes = [vp] * 6
        L.myo_batch_set_task.argtypes = [vp] * 5
        L.myo_batch_warmstart.argtypes = [vp] * 4
        L.myo_batch_set_bad_state_buffer.argtypes = [vp, vp]
        L.myo_batch_get_task.argtypes = [vp] * 5
        L.myo_batch_bind_constants.argtypes = [vp, vp]
        L.myo_batch_tune_wrap_order.argtypes = [vp, vp]
        L.myo_batch_set_object_group.argtypes = [vp, i32, i32]
        L.myo_batch_object_friction.argtypes = [vp, vp, vp, vp]
        L.myo_batch_fatigue.argtypes = [vp, vp, vp, vp]
        L.myo_batch_forward_dump.argtypes = [vp, vp, vp, vp]
        L.myo_batch_dump_size.argtypes = [vp]
        L.myo_batch_dump_offset.argtypes = [vp, C.c_char_p]
        L.myo_batch_kernel_ms.argtypes = [vp]
        L.myo_batch_kernel_ms.restype = dbl
        L.myo_batch_enable_timing.argtypes = [vp, i32]
        L.myo_model_default_camera.argtypes = [vp, C.POINTER(RenderCamera)]
        L.myo_batch_geom_poses.argtypes = [vp, vp, i32, vp, vp]
        L.myo_batch_tendon_paths.argtypes = [vp, vp, i32, vp, vp]
        L.myo_batch_render.argtypes = [vp, vp, i32, C.POINTER(RenderCamera), i32, i32, i32, i32, vp, vp, vp, vp]
        L.myo_batch_contact_items.argtypes = [vp, vp, i32, vp, vp]
        L.myo_batch_set_render_style.argtypes = [vp, C.POINTER(RenderStyle)]
        L.myo_batch_get_render_style.argtypes = [vp, C.POINTER(RenderStyle)]
        L.myo_batch_contact_capacity.argtypes = [vp]
        L.myo_batch_sense.argtypes = [vp, C.POINTER(SenseOut), vp]
        L.myo_batch_data.argtypes = [vp, vp, C.POINTER(DataOut), vp]
        L.myo_batch_jac.argtypes = [vp, i32, vp, i32, vp, C.POINTER(JacOut), vp]
        L.myo_batch_inverse.argtypes = [vp, vp, C.POINTER(InverseOut), vp]
        L.myo_batch_static_opt.argtypes = [vp, C.POINTER(StaticOptIn), C.POINTER(StaticOptOut), vp]
        L.myo_batch_ik.argtypes = [vp, C.POINTER(IkIn), C.POINTER(IkOut), vp]
        L.myo_batch_simulate.argtypes = [vp, C.POINTER(SimIn), C.POINTER(SimOut), vp]
        if b"MYO_EMU" in L.myo_version():
            return      # the emulation build (test tooling, csrc/emu_host.h) implements the env path only: ENV_PATH_SYMBOLS
        L.myo_ppo_loss_grad.argtypes = [vp] * 8 + [i32, i32, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, i32, C.c_float, vp, vp, vp, vp, vp]
        L.myo_ppo_sde_loss_supported.argtypes = [i32, i32]
        L.myo_ppo_sde_loss_work_floats.argtypes = [i32, i32, i32]
        L.myo_ppo_sde_loss_work_floats.restype = C.c_longlong
        L.myo_ppo_sde_loss_grad.argtypes = [vp] * 9 + [i32, i32, i32] + [C.c_float] * 4 + [vp] * 9
        L.myo_ppo_gather.argtypes = [vp] * 6 + [i32, i32, i32, vp, i32] + [vp] * 7
        L.myo_ppo_gather_seq.argtypes = [vp] * 9 + [i32] * 8 + [vp, i32] + [vp] * 11
        L.myo_rollout_state_snapshot.argtypes = [vp, vp, i32, i32, i32, vp, i32, i32, vp, vp, vp]
        L.myo_bias_relu_bf16.argtypes = [vp, vp, i32, i32, i32, vp]
        L.myo_bias_act_bf16.argtypes = [vp, vp, i32, i32, i32, i32, vp]
        L.myo_splitk_reduce.argtypes = [vp, i32, vp, i32, i32, i32, vp]
        L.myo_splitk_reduce2.argtypes = [vp, i32, vp, i32, i32, i32, vp, i32, vp, i32, i32, i32, vp]
        L.myo_relu_bwd_colsum_bf16.argtypes = [vp, vp, i32, i32, vp, vp]
        L.myo_act_bwd_colsum_bf16.argtypes = [vp, vp, i32, i32, vp, i32, vp]
        L.myo_rollout_policy_input.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp]
        L.myo_rollout_sample.argtypes = [vp, vp, vp, i32, i32, u64, vp, vp, vp, vp, vp, vp, i32, vp]
        L.myo_vecnorm_step.argtypes = [vp] * 5 + [i32, i32] + [vp] * 5 + [dbl] * 4 + [i32] * 3 + [vp] * 9
        L.myo_rollout_advance.argtypes = [vp, i32, vp, vp]
        L.myo_rollout_sample_sde.argtypes = [vp] * 4 + [i32] * 3 + [vp] * 3 + [i32, vp]
        L.myo_vecnorm_batch_moments.argtypes = [vp, vp, i32, i32, vp, dbl, i32, vp, vp, vp]
        L.myo_vecnorm_finish.argtypes = [vp] * 5 + [i32, i32] + [vp] * 5 + [dbl] * 3 + [i32] * 3 + [vp] * 9
        L.myo_gae.argtypes = [vp] * 5 + [i32, i32, C.c_float, C.c_float, vp, vp, vp]
        L.myo_lstm_cell_fwd.argtypes = [vp] * 4 + [i32] * 4 + [vp] * 6
        L.myo_lstm_cell_bwd.argtypes = [vp] * 7 + [i32] * 4 + [vp] * 3
        L.myo_lstm_step_supported.argtypes = [i32]
        L.myo_lstm_step_fwd.argtypes = [vp, C.c_longlong, C.c_longlong] + [vp] * 4 + [i32] * 3 + [vp, C.c_longlong] + [vp] * 7
        L.myo_lstm_step_bwd.argtypes = [vp, C.c_longlong] + [vp] * 7 + [i32] * 3 + [vp] * 3
        L.myo_lstm_seq_supported.argtypes = [i32]
        L.myo_lstm_seq_fwd.argtypes = [vp] + [C.c_longlong] * 3 + [vp] * 4 + [i32] * 5 + [vp, C.c_longlong, C.c_longlong] + [vp] * 4
        L.myo_lstm_seq_bwd.argtypes = [vp, C.c_longlong, C.c_longlong] + [vp] * 5 + [i32] * 5 + [vp] * 2
        L.myo_adam_step.argtypes = [C.POINTER(AdamDesc), vp]
        L.myo_ppo_mlp_workspace_bytes.restype = C.c_longlong
        L.myo_ppo_mlp_workspace_bytes.argtypes = [i32, i32, i32, i32, C.c_longlong]
        L.myo_ppo_mlp_step.argtypes = [C.POINTER(PpoMlpDesc), vp]
        L.myo_ppo_mlp_step_act.argtypes = [C.POINTER(PpoMlpDesc), i32, i32, vp]
        L.myo_ppo_mlp_sqnorm_parts.argtypes = [i32]
        L.myo_ppo_mlp_step_resident.argtypes = [C.POINTER(PpoMlpDesc), vp]
        L.myo_ppo_mlp_images.argtypes = [C.POINTER(PpoMlpDesc), vp]
        L.myo_ppo_adv_moments_epoch.argtypes = [vp, vp, i32, i32, vp, vp, vp]
        L.myo_ppo_mlp_rollout_workspace_bytes.restype = C.c_longlong
        L.myo_ppo_mlp_rollout_workspace_bytes.argtypes = [i32, i32, i32]
        L.myo_ppo_mlp_rollout_refresh.argtypes = [C.POINTER(PpoMlpRolloutDesc), vp]
        L.myo_ppo_mlp_rollout.argtypes = [C.POINTER(PpoMlpRolloutDesc), vp]
        L.myo_ppo_mlp_rollout_act.argtypes = [C.POINTER(PpoMlpRolloutDesc), i32, vp]
        L.myo_ensemble_supported.argtypes = [i32, i32, i32]
        L.myo_ensemble_act.argtypes = [C.POINTER(EnsembleDesc), vp]

    def check(self, rc: int):
        if rc != 0:
            raise MyoError(f"libmyobatch error {rc}: {self.L.myo_last_error().decode()}")

    @property
    def version(self) -> str:
        return self.L.myo_version().decode()

    @property
    def build_id(self) -> str:
        """hash of the native sources this library was compiled from (build.py:source_id), "unknown" for ad-hoc builds"""
        v = self.version
        return v.rsplit(" build ", 1)[1] if " build " in v else "unknown"

    @property
    def is_emulation(self) -> bool:
        return "MYO_EMU" in self.version


_LIB: Optional[NativeLib] = None


def load(path: Optional[str] = None) -> NativeLib:
    """Load the HIP library (or an explicitly named one — tests only)."""
    global _LIB
    if path is not None:
        return NativeLib(path)
    if _LIB is None:
        _LIB = NativeLib(LIB_PATH)
    return _LIB


EXPORTED_SYMBOLS = [
    "myo_model_from_blob", "myo_model_load_mjb", "myo_model_destroy", "myo_model_size", "myo_model_table", "myo_batch_create",
    "myo_batch_destroy", "myo_batch_set_step_generation", "myo_batch_health", "myo_debug_wave_slots", "myo_batch_num_envs", "myo_batch_obs_dim", "myo_batch_lds_bytes",
    "myo_batch_reset", "myo_batch_step", "myo_batch_step_inner", "myo_batch_step_inner_idx", "myo_batch_copy_envs", "myo_batch_physics_step", "myo_batch_get_state",
    "myo_batch_set_state", "myo_batch_warmstart", "myo_batch_set_bad_state_buffer", "myo_batch_set_task", "myo_batch_get_task", "myo_batch_set_object_group", "myo_batch_object_friction", "myo_batch_bind_constants", "myo_batch_tune_wrap_order", "myo_batch_forward_dump",
    "myo_batch_dump_size", "myo_batch_dump_offset", "myo_batch_kernel_ms",
    "myo_batch_enable_timing", "myo_ppo_loss_grad", "myo_ppo_gather", "myo_ppo_gather_seq", "myo_rollout_state_snapshot", "myo_bias_relu_bf16", "myo_rollout_policy_input", "myo_rollout_sample",
    "myo_vecnorm_step", "myo_rollout_sample_sde", "myo_vecnorm_batch_moments", "myo_vecnorm_finish", "myo_rollout_advance", "myo_gae", "myo_lstm_cell_fwd", "myo_lstm_cell_bwd", "myo_lstm_step_supported", "myo_lstm_step_fwd", "myo_lstm_step_bwd", "myo_lstm_seq_supported", "myo_lstm_seq_fwd", "myo_lstm_seq_bwd", "myo_splitk_reduce", "myo_splitk_reduce2", "myo_relu_bwd_colsum_bf16", "myo_adam_step", "myo_ppo_mlp_workspace_bytes", "myo_ppo_mlp_step", "myo_ppo_mlp_sqnorm_parts", "myo_ppo_mlp_rollout_workspace_bytes", "myo_ppo_mlp_rollout_refresh", "myo_ppo_mlp_rollout", "myo_last_error", "myo_version",
    "myo_model_default_camera", "myo_batch_geom_poses", "myo_batch_tendon_paths", "myo_batch_render",
    "myo_batch_contact_capacity", "myo_batch_sense", "myo_batch_data", "myo_batch_jac", "myo_batch_inverse", "myo_batch_static_opt", "myo_batch_ik", "myo_batch_simulate",
    "myo_batch_contact_items", "myo_batch_set_render_style", "myo_batch_get_render_style",
    "myo_batch_fatigue",
    "myo_ppo_mlp_step_resident", "myo_ppo_mlp_images", "myo_ppo_adv_moments_epoch",
    "myo_ppo_mlp_step_act", "myo_ppo_mlp_rollout_act", "myo_bias_act_bf16", "myo_act_bwd_colsum_bf16",
    "myo_ensemble_supported", "myo_ensemble_act",
    "myo_ppo_sde_loss_supported", "myo_ppo_sde_loss_work_floats", "myo_ppo_sde_loss_grad",
]

# ... of which the lane-serial emulation build (tests/emu/libmyobatch_emu.so: csrc/myobatch_emu.cpp + csrc/emu_host.h, test tooling) has the env
# path; the PPO-side kernels exist in the product library only
ENV_PATH_SYMBOLS = [
    "myo_batch_bind_constants", "myo_batch_copy_envs", "myo_batch_create", "myo_batch_destroy", "myo_batch_dump_offset", "myo_batch_dump_size",
    "myo_batch_enable_timing", "myo_batch_forward_dump", "myo_batch_get_state", "myo_batch_get_task", "myo_batch_health", "myo_batch_kernel_ms",
    "myo_batch_lds_bytes", "myo_batch_num_envs", "myo_batch_object_friction", "myo_batch_obs_dim", "myo_batch_physics_step", "myo_batch_reset",
    "myo_batch_set_bad_state_buffer", "myo_batch_set_object_group", "myo_batch_set_state", "myo_batch_set_step_generation", "myo_batch_set_task",
    "myo_batch_step", "myo_batch_step_inner", "myo_batch_step_inner_idx", "myo_batch_tune_wrap_order", "myo_batch_warmstart", "myo_debug_wave_slots",
    "myo_last_error", "myo_model_destroy", "myo_model_from_blob", "myo_model_load_mjb", "myo_model_size", "myo_model_table", "myo_version",
    "myo_model_default_camera", "myo_batch_geom_poses", "myo_batch_tendon_paths", "myo_batch_render",
    "myo_batch_contact_capacity", "myo_batch_sense", "myo_batch_data", "myo_batch_jac", "myo_batch_inverse", "myo_batch_static_opt", "myo_batch_ik", "myo_batch_simulate",
    "myo_batch_contact_items", "myo_batch_set_render_style", "myo_batch_get_render_style",
    "myo_batch_fatigue",
]


class Model:
    """Host handle of a compiled model (myo_model*)."""

    def __init__(self, compiled, lib: Optional[NativeLib] = None):
        self.lib = lib or load()
        self.compiled = compiled
        blob = compiled.to_blob()
        self._buf = C.create_string_buffer(blob, len(blob))
        h = C.c_void_p()
        self.lib.check(self.lib.L.myo_model_from_blob(self._buf, len(blob), C.byref(h)))
        self.h = h

    @classmethod
    def from_mjb(cls, path: str, lib: Optional[NativeLib] = None, integrator: Optional[int] = None, unsupported_contacts: str = "error",
                 allow_other_solver: bool = False):
        """The C route: libmyobatch reads the .mjb itself (myo_model_load_mjb)."""
        self = cls.__new__(cls)
        self.lib, self.compiled, self._buf = lib or load(), None, None
        h = C.c_void_p()
        self.lib.check(self.lib.L.myo_model_load_mjb(os.fsencode(path), -1 if integrator is None else int(integrator),
                                                     {"error": 0, "drop": 1}[unsupported_contacts] | (2 if allow_other_solver else 0), C.byref(h)))
        self.h = h
        return self

    def size(self, name: str) -> int:
        return self.lib.L.myo_model_size(self.h, name.encode())

    def table(self, name: str) -> np.ndarray:
        """A copy of one table (or non-int scalar) of the host model, as the loader derived it (myo_model_table)."""
        p, nbytes, dtype = C.c_void_p(), C.c_size_t(), C.c_int()
        self.lib.check(self.lib.L.myo_model_table(self.h, name.encode(), C.byref(p), C.byref(nbytes), C.byref(dtype)))
        raw = C.string_at(p, nbytes.value) if nbytes.value else b""
        return np.frombuffer(raw, dtype=TABLE_DTYPES[dtype.value]).copy()

    def default_camera(self) -> dict:
        """The model's default free camera (myo_model_default_camera): lookat, distance, azimuth, elevation, fovy."""
        c = RenderCamera()
        self.lib.check(self.lib.L.myo_model_default_camera(self.h, C.byref(c)))
        return {"lookat": tuple(c.lookat), "distance": c.distance, "azimuth": c.azimuth, "elevation": c.elevation, "fovy": c.fovy}

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.L.myo_model_destroy(self.h)
            self.h = None


def _ptr(x):
    """Device/host pointer of a torch tensor, numpy array, int or None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data
    return x.data_ptr()  # torch.Tensor


class Batch:
    """Thin handle of myo_batch*; every array argument is a pointer provider (see _ptr)."""

    def __init__(self, model: Model, cfg: Optional[TaskCfg], n_envs: int, device: int = 0, seed: int = 0,
                 dtype: int = MYO_F32):
        self.lib, self.model = model.lib, model
        h = C.c_void_p()
        self.lib.check(self.lib.L.myo_batch_create(model.h, C.byref(cfg) if cfg is not None else None,
                                                   n_envs, device, seed, dtype, C.byref(h)))
        self.h = h
        self.n = n_envs
        self.dtype = dtype
        self.obs_dim = self.lib.L.myo_batch_obs_dim(h)

    def reset(self, mask=None, obs=None, stream=None):
        self.lib.check(self.lib.L.myo_batch_reset(self.h, _ptr(mask), _ptr(obs), stream))

    def step(self, act, obs, rew, done, trunc=None, term_obs=None, comps=None, ep_info=None, stream=None):
        self.lib.check(self.lib.L.myo_batch_step(self.h, _ptr(act), _ptr(obs), _ptr(rew), _ptr(done), _ptr(trunc),
                                                 _ptr(term_obs), _ptr(comps), _ptr(ep_info), stream))

    def step_inner(self, mask, act, obs, done=None, stream=None):
        self.lib.check(self.lib.L.myo_batch_step_inner(self.h, _ptr(mask), _ptr(act), _ptr(obs), _ptr(done), stream))

    def step_inner_idx(self, idx, act, obs, done=None, stream=None):
        """compact form of step_inner: idx int32[n] (-1 = empty slot), act [n, nu], obs [n, obs_dim], done uint8[n] or None"""
        self.lib.check(self.lib.L.myo_batch_step_inner_idx(self.h, _ptr(idx), int(idx.shape[0]), _ptr(act), _ptr(obs), _ptr(done), stream))

    def copy_envs_from(self, src: "Batch", dst_idx, src_idx, stream=None):
        """env records src_idx of `src` -> envs dst_idx of this batch (int32 device arrays of equal length)"""
        self.lib.check(self.lib.L.myo_batch_copy_envs(self.h, _ptr(dst_idx), src.h, _ptr(src_idx), int(dst_idx.shape[0]), stream))

    def physics_step(self, ctrl, nsub, stream=None):
        self.lib.check(self.lib.L.myo_batch_physics_step(self.h, _ptr(ctrl), nsub, stream))

    def get_state(self, qpos=None, qvel=None, act=None, time=None, stream=None):
        self.lib.check(self.lib.L.myo_batch_get_state(self.h, _ptr(qpos), _ptr(qvel), _ptr(act), _ptr(time), stream))

    def set_state(self, qpos=None, qvel=None, act=None, time=None, stream=None):
        self.lib.check(self.lib.L.myo_batch_set_state(self.h, _ptr(qpos), _ptr(qvel), _ptr(act), _ptr(time), stream))

    def health(self) -> dict:
        """{"protocol_errors": k_step workgroups that met a hand-off state of another generation, "contact_overflows": substeps that
        dropped contacts beyond the scratch's capacity, "limit_row_overflows": substeps that dropped limit / friction-loss rows,
        "contact_slots_wanted": the largest number of contact slots such a substep asked for (0 when none overflowed)}; all 0
        in a healthy batch.  Synchronises the device."""
        out = (C.c_int32 * 4)()
        self.lib.check(self.lib.L.myo_batch_health(self.h, out))
        return {"protocol_errors": int(out[0]), "contact_overflows": int(out[1]), "limit_row_overflows": int(out[2]), "contact_slots_wanted": int(out[3])}

    def set_bad_state_buffer(self, buf):
        """uint8[N] device buffer (kept alive by the caller) that every step() fills with 1 for envs reset after a
        numerical blow-up; None to stop reporting."""
        self._bad_buf = buf
        self.lib.check(self.lib.L.myo_batch_set_bad_state_buffer(self.h, _ptr(buf)))

    def warmstart(self, get=None, set=None, stream=None):
        """Read (``get``) and / or overwrite (``set``) qacc_warmstart, double[N, nv]."""
        self.lib.check(self.lib.L.myo_batch_warmstart(self.h, _ptr(get), _ptr(set), stream))

    def set_task(self, task_i=None, task_d=None, ball_d=None, stream=None):
        self.lib.check(self.lib.L.myo_batch_set_task(self.h, _ptr(task_i), _ptr(task_d), _ptr(ball_d), stream))

    def set_object_group(self, gid0: int, gidn: int):
        self.lib.check(self.lib.L.myo_batch_set_object_group(self.h, gid0, gidn))

    def object_friction(self, set_fric=None, get_fric=None, stream=None):
        """friction triples of the object group's geoms, float64 [N, ngeom_group, 3] (set, then get; either may be None)"""
        self.lib.check(self.lib.L.myo_batch_object_friction(self.h, _ptr(set_fric), _ptr(get_fric), stream))

    def fatigue(self, set_state=None, get_state=None, stream=None):
        """fatigue state of a batch made with muscle_condition fatigue, float64 [N, 3, nu] = MA, MR, MF (set, then get; either may be None)"""
        self.lib.check(self.lib.L.myo_batch_fatigue(self.h, _ptr(set_state), _ptr(get_state), stream))

    def bind_constants(self, stream=None):
        """Make this batch the one whose model / task sit in __constant__ memory (needed before replaying a
        captured graph that contains this batch's launches, if other batches may have launched since)."""
        self.lib.check(self.lib.L.myo_batch_bind_constants(self.h, stream))

    def tune_wrap_order(self, stream=None):
        """Re-sort the tendon stage's geom wraps by how often they engage in the envs' present states (runs by itself after a
        reset of all envs; two small kernels on the stream, no result depends on the order: include/myobatch.h)."""
        self.lib.check(self.lib.L.myo_batch_tune_wrap_order(self.h, stream))

    def get_task(self, task_i=None, task_d=None, ball_d=None, stream=None):
        self.lib.check(self.lib.L.myo_batch_get_task(self.h, _ptr(task_i), _ptr(task_d), _ptr(ball_d), stream))

    def forward_dump(self, ctrl, out, stream=None):
        self.lib.check(self.lib.L.myo_batch_forward_dump(self.h, _ptr(ctrl), _ptr(out), stream))

    def geom_poses(self, env_idx, out, stream=None):
        """pose pass of the renderer: env_idx int32[k] -> out float64 [k, ngeom + nsite, RENDER_ITEM_N] (include/myobatch.h)"""
        self.lib.check(self.lib.L.myo_batch_geom_poses(self.h, _ptr(env_idx), int(env_idx.shape[0]), _ptr(out), stream))

    def tendon_paths(self, env_idx, out, stream=None):
        """path pass of the renderer: env_idx int32[k] -> out float64 [k, ntendon_item, RENDER_ITEM_N], the straight pieces of every
        spatial tendon as capsule items (include/myobatch.h)"""
        self.lib.check(self.lib.L.myo_batch_tendon_paths(self.h, _ptr(env_idx), int(env_idx.shape[0]), _ptr(out), stream))

    def contact_items(self, env_idx, out, stream=None):
        """contact item pass of the renderer: env_idx int32[k] -> out float64 [k, 2 * contact_capacity, RENDER_ITEM_N]; slot c's rows
        2c (the contact point, a disc) and 2c + 1 (the contact force, a capsule shaft), zero rows beyond ncon (include/myobatch.h)"""
        self.lib.check(self.lib.L.myo_batch_contact_items(self.h, _ptr(env_idx), int(env_idx.shape[0]), _ptr(out), stream))

    def get_render_style(self) -> dict:
        """the batch's contact drawing style (myo_render_style): a dict of RENDER_STYLE_KEYS"""
        st = RenderStyle()
        st.size = C.sizeof(RenderStyle)
        self.lib.check(self.lib.L.myo_batch_get_render_style(self.h, C.byref(st)))
        return {k: (tuple(getattr(st, k)) if k.endswith("rgba") else float(getattr(st, k))) for k in RENDER_STYLE_KEYS}

    def set_render_style(self, **fields):
        """change fields of the batch's contact drawing style (keys of RENDER_STYLE_KEYS; the others keep their values)"""
        st = RenderStyle()
        st.size = C.sizeof(RenderStyle)
        self.lib.check(self.lib.L.myo_batch_get_render_style(self.h, C.byref(st)))
        for k, v in fields.items():
            if k not in RENDER_STYLE_KEYS:
                raise KeyError(f"unknown render style field {k!r}; known: {RENDER_STYLE_KEYS}")
            if k.endswith("rgba"):
                getattr(st, k)[:] = [float(x) for x in v]
            else:
                setattr(st, k, float(v))
        self.lib.check(self.lib.L.myo_batch_set_render_style(self.h, C.byref(st)))

    def render(self, env_idx, cams, width, height, flags, rgb=None, depth=None, segid=None, stream=None):
        """ray cast of envs env_idx int32[k]; cams: a list of 1 or k camera dicts (lookat, distance, azimuth, elevation, fovy)"""
        arr = (RenderCamera * len(cams))()
        for c, d in zip(arr, cams):
            c.lookat[:] = [float(x) for x in d["lookat"]]
            c.distance, c.azimuth, c.elevation, c.fovy = (float(d[k]) for k in ("distance", "azimuth", "elevation", "fovy"))
        self.lib.check(self.lib.L.myo_batch_render(self.h, _ptr(env_idx), int(env_idx.shape[0]), arr, len(cams), int(width), int(height),
                                                   int(flags), _ptr(rgb), _ptr(depth), _ptr(segid), stream))

    @property
    def contact_capacity(self) -> int:
        """contact slots per env of this batch's stepper (24; 22 in the fp64 stepper; 48 with extended collision pairs or a die)"""
        return self.lib.L.myo_batch_contact_capacity(self.h)

    def sense_shapes(self) -> dict:
        """key -> (per-env shape, numpy dtype) of the arrays of sense()"""
        m, cap = self.model, self.contact_capacity
        nu, na, nt = m.size("nu"), m.size("na"), m.size("ntendon")
        return {"ncon": ((), np.int32), "con_geom": ((cap, 2), np.int32), "con_d": ((cap, SENSE_CON_N), np.float64),
                "body_wrench": ((m.size("nbody"), 6), np.float64), "qfrc_constraint": ((m.size("nv"),), np.float64),
                "act_length": ((nu,), np.float64), "act_velocity": ((nu,), np.float64), "act_force": ((nu,), np.float64),
                "activation": ((na,), np.float64), "ten_length": ((nt,), np.float64), "ten_velocity": ((nt,), np.float64)}

    def sense(self, stream=None, **arrays):
        """contact and muscle read-out of the envs' present states (myo_batch_sense): keyword = a key of SENSE_KEYS, value = the
        device array that receives it ([N, *sense_shapes()[key]]); keys not given are not computed"""
        out = SenseOut()
        out.size = C.sizeof(SenseOut)
        for k, v in arrays.items():
            if k not in SENSE_KEYS:
                raise KeyError(k)
            setattr(out, k, _ptr(v))
        self.lib.check(self.lib.L.myo_batch_sense(self.h, C.byref(out), stream))

    def data_shapes(self) -> dict:
        """key -> per-env shape of the float64 arrays of data()"""
        m = self.model
        nb, nv, nu, ng = m.size("nbody"), m.size("nv"), m.size("nu"), m.size("ngeom")
        return {"xpos": (nb, 3), "xquat": (nb, 4), "xmat": (nb, 9), "xipos": (nb, 3), "subtree_com": (nb, 3), "geom_xpos": (ng, 3),
                "geom_xmat": (ng, 9), "site_xpos": (m.size("nsite"), 3), "cvel": (nb, 6), "qM": (nv, nv), "ten_J": (m.size("ntendon"), nv),
                "actuator_moment": (nu, nv), "qfrc_bias": (nv,), "qfrc_passive": (nv,), "qfrc_actuator": (nv,), "qacc_smooth": (nv,),
                "qacc": (nv,), "act_dot": (m.size("na"),)}

    def data(self, stream=None, ctrl=None, **arrays):
        """kinematics and dynamics read-out of the envs' present states (myo_batch_data): keyword = a key of DATA_KEYS, value = the
        float64 device array that receives it ([N, *data_shapes()[key]]); ctrl: float64 [N, nu] or None (0).  Keys not given are not
        computed, and the pass ends after the last stage a given key needs."""
        out = DataOut()
        out.size = C.sizeof(DataOut)
        for k, v in arrays.items():
            if k not in DATA_KEYS:
                raise KeyError(k)
            setattr(out, k, _ptr(v))
        self.lib.check(self.lib.L.myo_batch_data(self.h, _ptr(ctrl), C.byref(out), stream))

    def jac(self, kind, obj_ids, jacp=None, jacr=None, points=None, stream=None):
        """Jacobians of the envs' present states (myo_batch_jac): kind = a key of JAC_KINDS (or its MYO_JAC_* code), obj_ids int32[k]
        device array, jacp / jacr float64 [N, k, 3, nv] device arrays or None, points float64 [N, k, 3] world points or None ("body"
        only: mj_jac).  Every element of a given output is written; "subtreecom" has no jacr."""
        if isinstance(kind, str):
            if kind not in JAC_KINDS:
                raise KeyError(f"unknown Jacobian kind {kind!r}; known: {sorted(JAC_KINDS)}")
            kind = JAC_KINDS[kind]
        out = JacOut()
        out.size, out.jacp, out.jacr = C.sizeof(JacOut), _ptr(jacp), _ptr(jacr)
        self.lib.check(self.lib.L.myo_batch_jac(self.h, int(kind), _ptr(obj_ids), int(obj_ids.shape[0]), _ptr(points), C.byref(out), stream))

    def inverse(self, qacc, qfrc_inverse=None, qfrc_constraint=None, stream=None):
        """inverse dynamics of the envs' present states (myo_batch_inverse): qacc float64 [N, nv] -> qfrc_inverse / qfrc_constraint
        float64 [N, nv] device arrays (either may be None)"""
        out = InverseOut()
        out.size, out.qfrc_inverse, out.qfrc_constraint = C.sizeof(InverseOut), _ptr(qfrc_inverse), _ptr(qfrc_constraint)
        self.lib.check(self.lib.L.myo_batch_inverse(self.h, _ptr(qacc), C.byref(out), stream))

    def static_opt_shapes(self) -> dict:
        """key -> (per-env shape, dtype) of the arrays of static_opt()"""
        nv, nu = self.model.size("nv"), self.model.size("nu")
        return {"u": ((nu,), np.float64), "force": ((nu,), np.float64), "qfrc": ((nv,), np.float64), "residual": ((nv,), np.float64),
                "gain": ((nu,), np.float64), "bias": ((nu,), np.float64), "kkt": ((), np.float64), "iters": ((), np.int32), "status": ((), np.int32)}

    def static_opt(self, target=None, weight=None, weight_per_env=False, reg=1e-6, u_ref=None, lower=None, upper=None, max_iter=100, stream=None, **arrays):
        """static optimisation at the envs' present states (myo_batch_static_opt): target = the struct's input qfrc, float64 [N, nv] (not needed by gain / bias
        alone), weight float64 [nv] or — weight_per_env — [N, nv], u_ref / lower / upper float64 [N, nu], each a device array or
        None (the library's default); keyword = a key of STATIC_OPT_KEYS, value = the device array that receives it
        ([N, *static_opt_shapes()[key]]).  Keys not given are not computed; gain / bias alone run no solve."""
        inp, out = StaticOptIn(), StaticOptOut()
        inp.size, out.size = C.sizeof(StaticOptIn), C.sizeof(StaticOptOut)
        inp.qfrc, inp.weight, inp.u_ref, inp.lower, inp.upper = _ptr(target), _ptr(weight), _ptr(u_ref), _ptr(lower), _ptr(upper)
        inp.weight_per_env, inp.reg, inp.max_iter = int(bool(weight_per_env)), float(reg), int(max_iter)
        for k, v in arrays.items():
            if k not in STATIC_OPT_KEYS:
                raise KeyError(k)
            setattr(out, k, _ptr(v))
        self.lib.check(self.lib.L.myo_batch_static_opt(self.h, C.byref(inp), C.byref(out), stream))

    def ik_shapes(self, k: int) -> dict:
        """key -> (per-env shape, dtype) of the arrays of ik() for k targets"""
        return {"qpos": ((self.model.size("nq"),), np.float64), "site_xpos": ((k, 3), np.float64), "residual": ((k, 3), np.float64),
                "cost": ((), np.float64), "kkt": ((), np.float64), "iters": ((), np.int32), "status": ((), np.int32)}

    def ik(self, site_ids, targets, weight=None, weight_per_env=False, q_init=None, q_ref=None, lower=None, upper=None, active=0,
           reg=1e-6, tol=1e-10, max_iter=50, stream=None, **arrays):
        """inverse kinematics from the envs' present states or q_init (myo_batch_ik): site_ids int32 [k] device array, targets float64
        [N, k, 3], weight float64 [k] or — weight_per_env — [N, k], q_init / q_ref float64 [N, nq], lower / upper float64 [N, nv] (by dof),
        each a device array or None (the library's default); active: dof mask (0: every hinge / slide dof); keyword = a key of IK_KEYS,
        value = the device array that receives it ([N, *ik_shapes(k)[key]]).  Keys not given are not computed; the envs do not move."""
        inp, out = IkIn(), IkOut()
        inp.size, out.size = C.sizeof(IkIn), C.sizeof(IkOut)
        inp.site_ids, inp.k, inp.targets, inp.weight = _ptr(site_ids), int(site_ids.shape[0]) if site_ids is not None else 0, _ptr(targets), _ptr(weight)
        inp.weight_per_env, inp.q_init, inp.q_ref, inp.lower, inp.upper = int(bool(weight_per_env)), _ptr(q_init), _ptr(q_ref), _ptr(lower), _ptr(upper)
        inp.active, inp.reg, inp.tol, inp.max_iter = int(active), float(reg), float(tol), int(max_iter)
        for k, v in arrays.items():
            if k not in IK_KEYS:
                raise KeyError(k)
            setattr(out, k, _ptr(v))
        self.lib.check(self.lib.L.myo_batch_ik(self.h, C.byref(inp), C.byref(out), stream))

    def simulate_shapes(self, S: int, R: int, ns: int = 0) -> dict:
        """key -> (per-listed-env shape, dtype) of the arrays of simulate() for S samples, R recorded steps and ns sites"""
        m = self.model
        return {"qpos": ((S, R, m.size("nq")), np.float64), "qvel": ((S, R, m.size("nv")), np.float64), "act": ((S, R, m.size("na")), np.float64),
                "time": ((S, R), np.float64), "site_xpos": ((S, R, ns, 3), np.float64), "bad": ((S,), np.int32), "steps": ((S,), np.int32)}

    def simulate(self, k, S, T, ctrl=None, ctrl_per_sample=False, env_idx=None, nsub=0, every=1, qpos0=None, qvel0=None, act0=None,
                 site_ids=None, stream=None, **arrays):
        """read-only open-loop simulation (myo_batch_simulate): S samples of T control steps (nsub substeps each; 0: the task's
        frame_skip) for each of the k envs env_idx (int32 [k] device array; None: envs 0 .. k - 1), from the envs' present states or
        qpos0 / qvel0 / act0 (float64 [k, S, .]); ctrl float64 [k, T, nu] or - ctrl_per_sample - [k, S, T, nu] (None: zeros); site_ids
        int32 [ns] device array; keyword = a key of SIM_KEYS, value = the device array that receives it
        ([k, *simulate_shapes(S, T // every, ns)[key]]).  Keys not given are not written; the envs do not move."""
        inp, out = SimIn(), SimOut()
        inp.size, out.size = C.sizeof(SimIn), C.sizeof(SimOut)
        inp.env_idx, inp.k, inp.S, inp.T, inp.nsub, inp.every = _ptr(env_idx), int(k), int(S), int(T), int(nsub), int(every)
        inp.ctrl, inp.ctrl_per_sample, inp.qpos0, inp.qvel0, inp.act0 = _ptr(ctrl), int(bool(ctrl_per_sample)), _ptr(qpos0), _ptr(qvel0), _ptr(act0)
        inp.site_ids, inp.ns = _ptr(site_ids), int(site_ids.shape[0]) if site_ids is not None else 0
        for key, v in arrays.items():
            if key not in SIM_KEYS:
                raise KeyError(key)
            setattr(out, key, _ptr(v))
        self.lib.check(self.lib.L.myo_batch_simulate(self.h, C.byref(inp), C.byref(out), stream))

    @property
    def dump_size(self) -> int:
        return self.lib.L.myo_batch_dump_size(self.h)

    def dump_offset(self, name: str) -> int:
        return self.lib.L.myo_batch_dump_offset(self.h, name.encode())

    @property
    def lds_bytes(self) -> int:
        return self.lib.L.myo_batch_lds_bytes(self.h)

    def enable_timing(self, on=True):
        self.lib.check(self.lib.L.myo_batch_enable_timing(self.h, int(on)))

    def kernel_ms(self) -> float:
        return self.lib.L.myo_batch_kernel_ms(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.lib.L.myo_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
