/* myobatch.h — C ABI of libmyobatch: batched MyoSuite-class muscle-tendon physics + the
 * Baoding task layer, resident on one MI355X.
 *
 * The reference has no native boundary; the seam this library sits behind is the per-process
 * gym API that stable-baselines3's SubprocVecEnv drives over pipes:
 *     SubprocVecEnv([thunk]*n)            /root/reference/src/main_baoding.py:56-65
 *     env.reset() / env.step(a)           /root/reference/src/main_eval.py:92,104
 *     EnvironmentFactory.create(name,**kw) /root/reference/src/envs/environment_factory.py:8-63
 * Each entry point below names the reference interface it replaces.  All pointers marked
 * "dev" are device (HBM) pointers owned by the caller (torch tensors); `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  Every function returns 0 on success
 * or a negative MYO_E_* code; myo_last_error() gives the thread-local message.  A numerical
 * blow-up of one environment is not an error: the env reports done=1 and is reset
 * (MuJoCo's mj_checkPos/Vel/Acc -> mj_resetData behaviour).
 *
 * There is no CPU execution path in this library.
 */
#ifndef MYOBATCH_H
#define MYOBATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MYO_OK 0
#define MYO_E_ARG -1      /* bad argument / malformed blob */
#define MYO_E_BADARG MYO_E_ARG
#define MYO_E_UNSUPPORTED -2 /* model uses a feature the stepper lacks or exceeds its limits */
#define MYO_E_DEVICE -3   /* HIP runtime error */
#define MYO_E_STATE -4    /* call sequence error */

typedef struct myo_model myo_model;
typedef struct myo_batch myo_batch;

/* arithmetic of the stepper.  MYO_F64: everything in fp64 (the reference's mjtNum).  MYO_MIXED: fp64 for what
 * decides whether a trajectory stays on the fp64 one — the state (qpos, qvel, act, time) and its integration, the
 * kinematic chain, contact / joint-limit distances, the tendon-wrap predicates, the Newton cost, the observation —
 * and fp32 for the rest of the dynamics.  MYO_F32 is round 1's name for value 1. */
enum { MYO_F64 = 0, MYO_MIXED = 1, MYO_F32 = 1 };
enum { MYO_TASK_NONE = 0, MYO_TASK_BAODING_P1 = 1, MYO_TASK_BAODING_P2 = 2, MYO_TASK_REORIENT = 3, MYO_TASK_POSE = 4 };
enum { MYO_POSE_RESET_INIT = 0, MYO_POSE_RESET_RANDOM = 1, MYO_POSE_RESET_SDS = 2 };      /* CustomPoseEnv reset_type ("none" is refused) */
enum { MYO_POSE_TARGET_GENERATE = 0, MYO_POSE_TARGET_FIXED = 1 };                       /* CustomPoseEnv target_type */
enum { MYO_WHICH_HOLD = 0, MYO_WHICH_CW = 1, MYO_WHICH_CCW = 2 }; /* MyoSuite Task enum */
enum { MYO_CHOICE_FIXED = 0, MYO_CHOICE_CW = 1, MYO_CHOICE_CCW = 2, MYO_CHOICE_RANDOM = 3 };

#define MYO_N_RWD 8 /* Baoding: pos_dist_1,pos_dist_2,act_reg,alive,sparse,solved,done,dense; die reorient: pos_dist,rot_dist,... */
#define MYO_ROT_CHOICE_MAX 4 /* entries of a goal_rot_x/y/z range list */
#define MYO_OBJG_MAX 20      /* geoms of the per-env object group (the die) */
#define MYO_POSE_NQ_MAX 38   /* joints of a MYO_TASK_POSE model (the stepper's qpos capacity) */

/* Task configuration = the kwargs of CustomBaodingEnv._setup / CustomBaodingP2Env._setup
 * (/root/reference/src/envs/baoding.py:210-227,300-324) lowered to plain numbers, plus the
 * ids the reference resolves by name (baoding.py:264-269,371-378) and the TimeLimit horizon
 * (/root/reference/src/envs/__init__.py:15,61). */
typedef struct myo_task_cfg {
  int32_t kind;              /* MYO_TASK_* */
  int32_t frame_skip;        /* 10 */
  int32_t max_episode_steps; /* 200 */
  int32_t n_hand;            /* 23: obs hand_pos = qpos[:n_hand] */
  int32_t obj1_sid, obj2_sid, target1_sid, target2_sid;
  int32_t obj1_bid, obj2_bid, obj1_gid, obj2_gid;
  int32_t task_choice;       /* MYO_CHOICE_*: P1 `task` (None->FIXED=CCW,"cw","ccw","random"); P2 `task_choice` */
  int32_t enable_rsi, balls_overlap, limit_init_angle_on, beta_init_angle_on, beta_ball_size_on,
      beta_ball_mass_on;
  double drop_th, proximity_th;
  double center_pos[2];
  double weights[7];         /* pos_dist_1,pos_dist_2,act_reg,alive,sparse,solved,done */
  double goal_time_period[2], goal_xrange[2], goal_yrange[2];
  double rsi_probability, overlap_probability;
  double noise_palm, noise_fingers, noise_balls;
  double limit_init_angle, beta_init_angle[2], beta_ball_size[2], beta_ball_mass[2];
  double obj_size_range[2], obj_mass_range[2], obj_friction_change[3];
  double init_qpos0;         /* -1.57 (baoding.py:283,401); die reorient: -1.5 (reorient.py:121) */
  /* -- kind MYO_TASK_REORIENT: the kwargs of CustomReorientEnv._setup (/root/reference/src/envs/reorient.py:58-122) and what
   * _setup reads from the model.  Ids: obj1_sid = site object_o, target1_sid = site target_o, obj1_bid = body Object,
   * [obj1_gid, obj2_gid) = the die's geoms (body_geomadr .. +body_geomnum); n_hand = nq - 7 (the die's free joint is last).
   * drop_th, obj_friction_change, enable_rsi, frame_skip, max_episode_steps as above.  The other Baoding fields are unused. */
  double ro_weights[9];      /* pos_dist, rot_dist, pos_dist_diff, rot_dist_diff, alive, act_reg, sparse, solved, done */
  double ro_goal_pos[2], ro_goal_rot[2];        /* goal_pos / goal_rot ranges (low, high) */
  int32_t ro_n_rot_choice[3], ro_pad_;          /* lengths of goal_rot_x / _y / _z (0 = None: goal_rot applies) */
  double ro_rot_choice[3][MYO_ROT_CHOICE_MAX][2];
  double ro_obj_size_change, ro_pos_th, ro_rot_th;
  double ro_goal_init_pos[3], ro_goal_obj_offset[3];   /* site_xpos[target_o] and site_xpos[target_o] - site_xpos[object_o] at setup */
  double ro_rsi_distance_pos, ro_rsi_distance_rot;
  /* -- kind MYO_TASK_POSE: the kwargs of CustomPoseEnv._setup (/root/reference/src/envs/pose.py:7-51) for a model of hinge joints only
   * (nq = nv = n_hand; the hand with no object).  frame_skip, max_episode_steps as above; every other field above is unused.
   * Arrays are indexed by joint = qpos index; pose_init_qpos is the env's init_qpos (the model's qpos0). */
  double pose_weights[7];    /* weighted_reward_keys: pose, bonus, penalty, act_reg, sparse, solved, done */
  double pose_thd, pose_far_th, pose_sds_distance, pose_target_distance;
  int32_t pose_reset_type, pose_target_type;                /* MYO_POSE_RESET_*, MYO_POSE_TARGET_* */
  double pose_init_qpos[MYO_POSE_NQ_MAX];
  double pose_target_value[MYO_POSE_NQ_MAX];               /* target_type fixed: target_jnt_value */
  double pose_target_range[MYO_POSE_NQ_MAX][2];            /* target_type generate: target_jnt_range (low, high) per joint */
  double pose_reset_range[MYO_POSE_NQ_MAX][2];             /* reset_type random: the model's jnt_range */
  /* -- every kind: the `muscle_condition` kwarg of MyoSuite's BaseV0._setup [3P-RECALL], MYO_MUSCLE_* below.  0 = none: the step is
   * what it was before the fields existed.  reaf_src / reaf_dst: the actuators EIP / EPL of 'reafferentation' (ctrl[dst] maps
   * action[src], ctrl[src] = 0).  fatigue_F / _R / _r: the rates of the 3CC-r model of 'fatigue' (MyoSuite's defaults: 0.00912,
   * 0.000094, 150).  'sarcopenia' is a model edit made before the model is compiled and has no field here. */
  int32_t muscle_condition, reaf_src, reaf_dst;
  double fatigue_F, fatigue_R, fatigue_r;
} myo_task_cfg;
enum { MYO_MUSCLE_NONE = 0, MYO_MUSCLE_FATIGUE = 1, MYO_MUSCLE_REAFFERENTATION = 2 };

/* -- model ------------------------------------------------------------------------------
 * replaces gym.make(..., model_path=...) -> mj_loadModel (src/envs/__init__.py:17,63).
 * `blob` is the named-array format of include/myo_model_blob.h (host memory). */
int myo_model_from_blob(const void* blob, size_t nbytes, myo_model** out);
/* Load a MuJoCo 2.1 binary model file, what the reference's gym registrations hand to MuJoCo's mj_loadModel
 * (`model_path=…/myo_hand_baoding.mjb`, /root/reference/src/envs/__init__.py:17,63).  The C reader (csrc/myo_mjb.h) decodes the
 * file, applies the feature checks and derives the static tables exactly as the Python route (mjb.load_mjb + model.compile_model
 * + myo_model_from_blob) does.  integrator: -1 keeps the model's, 0 Euler, 1 RK4.  unsupported_contacts: 0 = a model with
 * colliding geom pairs that have no narrow phase here is refused (MYO_E_UNSUPPORTED), 1 = compiled without those pairs; | 2 = a model
 * whose opt.solver is PGS / CG or that asks for noslip iterations is stepped with this stepper's Newton solver (no noslip pass) instead
 * of being refused — an explicit opt-in; every other unsupported feature is refused whatever the flags. */
int myo_model_load_mjb(const char* path, int integrator, int unsupported_contacts, myo_model** out);
void myo_model_destroy(myo_model* m);
int myo_model_size(const myo_model* m, const char* name); /* nq nv nu na nbody ... ; -1 unknown */
/* Read access to what the loader derived (tests pin the host tables through it): *data points INTO the model, host memory, valid until
 * myo_model_destroy; nothing is copied and no device is touched.  `name` is a table of the model (every array of csrc/myo_model_dev.h's
 * MYO_MODEL_*_ARRAYS lists, vis, tvis, titem_adr) or one of its scalars that is no int (timestep, tolerance, impratio, gravity,
 * meaninertia, cam_lookat, cam_distance, arrow_pad); the int scalars are myo_model_size's.  *bytes = size of the table, *dtype = one
 * of MYO_TABLE_* (its element type).  An unknown name: MYO_E_ARG. */
enum { MYO_TABLE_I32 = 0, MYO_TABLE_U64 = 1, MYO_TABLE_F32 = 2, MYO_TABLE_F64 = 3 };
int myo_model_table(const myo_model* m, const char* name, const void** data, size_t* bytes, int* dtype);

/* -- batch ------------------------------------------------------------------------------
 * replaces SubprocVecEnv([thunk]*n) + TimeLimit + Monitor (src/main_baoding.py:56-65).
 * `cfg` may be NULL (kind NONE: physics only).  dtype: MYO_F64 | MYO_MIXED. */
int myo_batch_create(const myo_model* m, const myo_task_cfg* cfg, int n_envs, int device,
                     uint64_t seed, int dtype, myo_batch** out);
void myo_batch_destroy(myo_batch* b);
int myo_batch_num_envs(const myo_batch* b);
int myo_batch_obs_dim(const myo_batch* b);
int myo_batch_lds_bytes(const myo_batch* b); /* LDS footprint of one env's working set */

/* env.reset() for the envs selected by mask (dev uint8[N] or NULL = all); writes obs
 * (dev float[N,obs_dim], may be NULL).  baoding.py:146-208 / :494-647. */
int myo_batch_reset(myo_batch* b, const uint8_t* mask, float* obs, void* stream);

/* env.step(a) for every env with SubprocVecEnv auto-reset semantics: BaodingEnvV1.step ->
 * BaseV0.step -> mj_step x frame_skip -> get_obs/get_reward_dict (baoding.py:24-94,403-467),
 * TimeLimit truncation, reset on done.  act: dev float[N,nu].  Outputs (dev): obs[N,obs_dim]
 * (post-reset obs where done), rew[N], done[N], trunc[N] (info["TimeLimit.truncated"]),
 * term_obs[N,obs_dim] (info["terminal_observation"], valid where done), comps[N,MYO_N_RWD]
 * (rwd_dict of the step), ep_info[N,2] (Monitor's episode r,l; valid where done).
 * Any output pointer except obs/rew/done may be NULL. */
int myo_batch_step(myo_batch* b, const float* act, float* obs, float* rew, uint8_t* done,
                   uint8_t* trunc, float* term_obs, float* comps, float* ep_info, void* stream);

/* Test hook: set the generation counter of the step plan (k_step's part protocol; it wraps after 2^28 steps). */
int myo_batch_set_step_generation(myo_batch* b, unsigned int gen);

/* Health counters of a batch (all 0 in a healthy one; synchronises the device).
 * out[0]: k_step workgroups that found their env's hand-off state in another generation than the launch's (a failed launch,
 *         or one batch stepped from two unsynchronised streams; such a step writes nothing and flags the env in bad_state);
 * out[1]: substeps in which an env had more contacts than its scratch holds (24; 22 in the fp64 stepper; 48 for models with
 *         extended collision pairs or a die) — the surplus was dropped, as MuJoCo drops contacts beyond nconmax with a warning;
 * out[2]: substeps in which an env had more joint-limit / tendon-limit / friction-loss rows than the scratch's row capacity
 *         (MYO_NLIM_MAX = 56) — the surplus was dropped;
 * out[3]: the largest number of contact slots any substep counted in out[1] asked for (what capacity would have been enough). */
int myo_batch_health(myo_batch* b, int out[4]);

/* Device check of the premise of k_step's per-wave-slot workspace (csrc/wave.h: myo_wave_slot): launches n_workgroups one-wave
 * workgroups with lds_bytes of dynamic LDS that each occupy their hardware wave slot's counter for ~20 us.
 * out[0]: workgroups that found their slot occupied by another resident workgroup (0 on a device whose HW_ID layout is the expected one);
 * out[1]: distinct slots seen; out[2]: largest slot index; out[3]: bit mask of the XCC ids seen. */
int myo_debug_wave_slots(int device, int n_workgroups, int lds_bytes, int32_t out[4]);

/* env.step(a) of the UNWRAPPED env for the envs selected by mask (dev uint8[N], NULL = all): no
 * TimeLimit / Monitor accounting, no auto-reset.  This is the `self.step(action)` that
 * MixtureModelBaodingEnv.reset runs with its base policy for the first n_steps_base_model steps
 * (baoding.py:700-711).  obs rows of unselected envs are left untouched; done (may be NULL) receives
 * the env's own done flag (ball dropped) for the selected envs. */
int myo_batch_step_inner(myo_batch* b, const uint8_t* mask, const float* act, float* obs, uint8_t* done, void* stream);

/* The same step for a LIST of envs in compact form: idx = dev int32[n_idx] (env numbers; -1 = empty slot; no env twice), act = dev
 * float[n_idx, nu], obs = dev float[n_idx, obs_dim], done = dev uint8[n_idx] or NULL — row r belongs to env idx[r].  One workgroup
 * per slot instead of one per env of the batch: the base phase of MixtureModelBaodingEnv (baoding.py:700-711) touches the few
 * envs that were just reset. */
int myo_batch_step_inner_idx(myo_batch* b, const int* idx, int n_idx, const float* act, float* obs, uint8_t* done, void* stream);

/* Whole env records from one batch into another of the same model / task kind / device: dst env dst_idx[r] <- src env src_idx[r],
 * r < k (dev int32 arrays; out-of-range entries are skipped).  A record is everything an env is between two steps, so the
 * destination env continues where the source env stood (MixtureModelBaodingEnv: pre-played episodes from a pool batch). */
int myo_batch_copy_envs(myo_batch* dst, const int* dst_idx, const myo_batch* src, const int* src_idx, int k, void* stream);

/* raw physics: apply ctrl (dev double[N,nu]) and run `nsub` mj_step substeps; no task layer.
 * Used by parity tests on arbitrary models. */
int myo_batch_physics_step(myo_batch* b, const double* ctrl, int nsub, void* stream);

/* state access (sim.data.qpos/qvel/act/time; env.set_state; robot.reset).  dev double
 * arrays [N,nq],[N,nv],[N,na],[N]; any may be NULL. */
int myo_batch_get_state(myo_batch* b, double* qpos, double* qvel, double* act, double* time,
                        void* stream);
int myo_batch_set_state(myo_batch* b, const double* qpos, const double* qvel, const double* act,
                        const double* time, void* stream);
/* Numerical blow-up of an env (non-finite / huge qpos, qvel or qacc: MuJoCo's mj_checkPos/Vel/Acc, which warn and
 * reset the data) is NOT an error of myo_batch_step: the env ends its episode (done = 1, trunc = 0, reward 0, reward
 * components 0 except `done`), is reset at once, and its terminal observation is the reset observation, so no NaN
 * leaves the kernel.  Register a caller-owned device buffer uint8[N] here to be told which envs it happened to:
 * every myo_batch_step writes 0 / 1 per env.  NULL (default) = not reported. */
int myo_batch_set_bad_state_buffer(myo_batch* b, uint8_t* bad_state);

/* qacc_warmstart (dev double[N,nv]): the remaining piece of MuJoCo's integration state (mjData.qacc_warmstart
 * seeds the Newton solver, so two steppers only retrace each other when it is copied along with qpos/qvel/act).
 * Either pointer may be NULL. */
int myo_batch_warmstart(myo_batch* b, double* get_qacc_warmstart, const double* set_qacc_warmstart, void* stream);

/* per-env task parameters, explicit injection for parity tests (what reset() samples):
 * task_i  dev int32[N,2]  = which_task, counter
 * task_d  dev double[N,9] = start_angle1, start_angle2, x_radius, y_radius, time_period,
 *                           target1_x, target1_y, target2_x, target2_y (palm-frame site xy)
 * ball_d  dev double[N,10]= mass1, mass2, friction1[3], friction2[3], size1, size2
 * MYO_TASK_REORIENT batches: task_i = 0, episode step counter; task_d = goal_pos[3], goal_quat[4], pos_dist, rot_dist
 * (the shaping state of reorient.py:207-210); ball_d[8] = the die's size delta, the rest unused.
 * MYO_TASK_POSE batches: task_i = 0, episode step counter; task_d = dev double[N, 2 nq] = target_qpos[nq] (the episode's target after
 * the target_distance blend), init_qpos[nq] (the state the episode started from: the reset_type's draw); ball_d unused (may be NULL).
 * Both come from the env's Philox stream keyed by (seed, env, episode): draw j < nq = target joint j (generate), draw nq + j = reset
 * joint j (random), each lo + (hi - lo) u. */
int myo_batch_set_task(myo_batch* b, const int32_t* task_i, const double* task_d,
                       const double* ball_d, void* stream);
int myo_batch_get_task(myo_batch* b, int32_t* task_i, double* task_d, double* ball_d, void* stream);

/* Per-env physical randomisation of an object made of several geoms (the die of CustomReorientEnv.reset,
 * /root/reference/src/envs/reorient.py:136-147): each of the geoms [gid0, gidn) (at most MYO_OBJG_MAX) has its own per-env
 * friction triple (myo_batch_object_friction; the model's values until set) and the group a per-env size delta in
 * ball_d[8] (size1): every geom centre of the group moves outward by the delta along each non-zero local
 * coordinate, capsule half-lengths grow by it.  (-1, -1) clears the group.  A MYO_TASK_REORIENT batch owns its
 * group (the die, from the task cfg) and draws both at every reset; this call is for physics-only batches. */
int myo_batch_set_object_group(myo_batch* b, int gid0, int gidn);
/* friction of the object group's geoms: dev double[N, gidn-gid0, 3]; either pointer may be NULL (set, then get).  The stepper
 * builds condim-3 contacts only, which read the sliding coefficient [.,.,0]; a MYO_TASK_REORIENT reset draws all three
 * per geom in the reference's order and keeps the sliding one (the other two slots stay at the model's values). */
int myo_batch_object_friction(myo_batch* b, const double* set_fric, double* get_fric, void* stream);

/* Muscle fatigue state of a batch made with muscle_condition = MYO_MUSCLE_FATIGUE: dev double[N, 3, nu], per env the active, resting
 * and fatigued fractions MA[nu], MR[nu], MF[nu] of the 3CC-r model (MyoSuite's CumulativeFatigue [3P-RECALL]; the update rule is
 * fatigue_advance in csrc/myo_task.h).  The state is part of the env's record: always fp64, (0, 1, 0) after every reset of the env
 * (myo_batch_reset, the auto-reset of myo_batch_step, the recovery of a blown-up env), advanced once per env step by myo_batch_step /
 * _step_inner / _step_inner_idx from the step's action — ctrl = MA — left alone by myo_batch_physics_step, copied by
 * myo_batch_copy_envs.  Either pointer may be NULL (set, then get).  A batch without fatigue returns MYO_E_ARG with a message. */
int myo_batch_fatigue(myo_batch* b, const double* set_state, double* get_state, void* stream);

/* The model / task parameters of ONE batch per device sit in __constant__ memory; every launching entry point
 * re-uploads them (on its stream) when another batch used the device in between.  A caller that REPLAYS a
 * captured graph containing this batch's launches must call this first whenever other batches of the same
 * process may have launched since (no-op if this batch is still the bound one). */
int myo_batch_bind_constants(myo_batch* b, void* stream);

/* Order of the tendon stage's geom wraps (sphere / cylinder wraps; the solver runs 64 of them per pass and a pass none of whose wraps
 * engages skips its tangent solve): counts which wraps engage in the envs' PRESENT states and sorts the batch's wrap order by it, so
 * that the wraps that rarely engage share the last pass.  Runs by itself: after a myo_batch_reset of all envs (mask = NULL), 16
 * myo_batch_step calls later, then every 256 calls (not while the stream is being captured); a caller may also run it between any
 * two steps — two small kernels on the stream, no host synchronisation, safe beside captured graphs of steps (the tables are
 * rewritten in place).  No result bit depends on the order.  No-op for models with at
 * most 64 geom wraps, and with MYO_NO_WRAP_ORDER set in the environment when the batch is made (A/B switch). */
int myo_batch_tune_wrap_order(myo_batch* b, void* stream);

/* forward dynamics of the current state with intermediates dumped for stage-wise parity
 * tests: out is dev double[N, myo_batch_dump_size()] ; layout by myo_batch_dump_offset(name).
 * names: ten_length ten_J(nt*nv) M(nv*nv) qfrc_bias qfrc_passive qfrc_actuator qacc_smooth
 *        qacc actuator_force act_dot counts(ncon,nefc,iter) efc_aref efc_D site_xpos subtree_com */
int myo_batch_forward_dump(myo_batch* b, const double* ctrl, double* out, void* stream);
int myo_batch_dump_size(const myo_batch* b);
int myo_batch_dump_offset(const myo_batch* b, const char* name);

/* ---- per-env contact and muscle read-out (MuJoCo's data.contact[i], mj_contactForce, data.cfrc_ext, data.qfrc_constraint,
 * data.actuator_length / _velocity / _force, data.act, data.ten_length / ten_velocity — what the reference reads from sim.data).
 * One wave per env runs the stepper's forward pass at the env's PRESENT state — kinematics, tendons, collision, constraint rows and the
 * Newton solve seeded from the env's qacc_warmstart, with the env's own ball / die parameters: what the next substep would compute —
 * and publishes the arrays below.  Controls are not part of an env's state between two steps: the pass runs with ctrl = 0, which
 * enters the activation rates only.  Reads the env records only: no record, warm start, draw counter, step generation or wrap order
 * changes; a pass that has to drop contacts beyond the capacity counts it in myo_batch_health like a substep.
 *
 * myo_sense_out: caller-owned DEVICE arrays, any of them NULL (not wanted); `size` = sizeof(myo_sense_out), first, so that the
 * struct can grow.  N = envs, cap = myo_batch_contact_capacity (contact slots per env: 24, 22 in the fp64 stepper, 48 for models
 * with extended collision pairs or a die):
 *   ncon            int32 [N]             active contacts (the capacity when a surplus was dropped)
 *   con_geom        int32 [N, cap, 2]     geom1, geom2; -1 in unused slots
 *   con_d           double[N, cap, 13]    dist, pos[3] (world), normal[3] (world, from geom1 to geom2), force[6] in the contact frame
 *                                         (normal, tangent 1, tangent 2, torsional, rolling 1, rolling 2 — mj_contactForce: the normal
 *                                         force is the sum of the contact's pyramid edge forces, component i is (f[2i] - f[2i+1]) mu_i;
 *                                         condim 1: the normal force alone); unused components and slots are 0.  The frame's tangents
 *                                         are mju_makeFrame's of the normal; the force acts on geom2's body, its opposite on geom1's
 *   body_wrench     double[N, nbody, 6]   net contact force [0..3) and torque [3..6) on each body, world frame, torque about the body's
 *                                         xpos (cfrc_ext restricted to contacts)
 *   qfrc_constraint double[N, nv]         constraint forces in joint space (contacts, joint / tendon limits, friction loss)
 *   act_length, act_velocity, act_force   double[N, nu]
 *   activation      double[N, na]
 *   ten_length, ten_velocity              double[N, ntendon]
 * Contacts are listed in the stepper's pair order, which is not MuJoCo's.  A NULL batch / struct or another `size` returns
 * MYO_E_BADARG (= MYO_E_ARG) before any device call. */
typedef struct myo_sense_out {
  size_t size;
  int32_t* ncon;
  int32_t* con_geom;
  double* con_d;
  double* body_wrench;
  double* qfrc_constraint;
  double* act_length;
  double* act_velocity;
  double* act_force;
  double* activation;
  double* ten_length;
  double* ten_velocity;
} myo_sense_out;
int myo_batch_contact_capacity(const myo_batch* b);
int myo_batch_sense(myo_batch* b, const myo_sense_out* out, void* stream);

/* ---- per-env kinematics and dynamics read-out (MuJoCo's sim.data by name: data.xpos, data.site_xpos, data.qM, data.actuator_moment,
 * data.qfrc_actuator, data.qacc ... — what custom rewards, fingertip / object tracking and moment-arm curves are made of).
 * One wave per env runs the stepper's forward pass at the env's PRESENT state, seeded like myo_batch_sense (the env's qacc_warmstart,
 * its own ball / die parameters), and publishes the arrays below.  ctrl: dev double[N, nu] or NULL (= 0); it enters act_dot and the
 * forces of actuators without an activation state.  The pass ENDS after the last stage a non-NULL pointer needs — position, inertia,
 * velocity, actuation, smooth acceleration, constrained acceleration, in this order: a call for poses or moment arms runs no
 * composite-inertia pass, no collision and no solver; only qacc runs the collision passes, the constraint rows and the Newton solve.
 * Reads the env records only: no record, warm start, draw counter, step generation or wrap order changes; a qacc pass that has to
 * drop contacts beyond the capacity counts it in myo_batch_health like a substep.
 *
 * myo_data_out: caller-owned DEVICE arrays of doubles, any of them NULL (not wanted); `size` = sizeof(myo_data_out), first, so that
 * the struct can grow.  World frame, MuJoCo's conventions; N = envs; [stage]:
 *   xpos, xipos, subtree_com  [N, nbody, 3]   body frame origin, inertial frame origin, centre of mass of the body's subtree  [position]
 *   xquat                     [N, nbody, 4]   unit quaternion (w, x, y, z)                                                    [position]
 *   xmat                      [N, nbody, 9]   row-major rotation matrix                                                       [position]
 *   geom_xpos, geom_xmat      [N, ngeom, 3 / 9]  with the env's own geometry (the die's size delta moves its geoms)            [position]
 *   site_xpos                 [N, nsite, 3]   the Baoding target sites where the task puts them                              [position]
 *   ten_J                     [N, ntendon, nv]  tendon moment arms, dense                                                     [position]
 *   actuator_moment           [N, nu, nv]     gear times the actuator's tendon's row of ten_J                                 [position]
 *   qM                        [N, nv, nv]     joint-space inertia, dense and symmetric (data.qM expanded by mj_fullM)         [inertia]
 *   cvel                      [N, nbody, 6]   com-based body velocity: rotation [0..3), translation [3..6) at subtree_com of the
 *                                             body's tree root                                                                [velocity]
 *   qfrc_bias, qfrc_passive   [N, nv]                                                                                         [velocity]
 *   qfrc_actuator             [N, nv]                                                                                         [actuation]
 *   act_dot                   [N, na]                                                                                         [actuation]
 *   qacc_smooth               [N, nv]         unconstrained acceleration                                                      [smooth acceleration]
 *   qacc                      [N, nv]                                                                                         [constrained acceleration]
 * The die's `target` body, its geoms and sites are at the episode's goal_pos / goal_quat (the reference writes them into the model).
 * A NULL batch / struct or another `size` returns MYO_E_BADARG (= MYO_E_ARG) before any device call; a struct whose pointers are all
 * NULL launches nothing. */
typedef struct myo_data_out {
  size_t size;
  double *xpos, *xquat, *xmat, *xipos, *subtree_com, *geom_xpos, *geom_xmat, *site_xpos,
      *cvel, *qM, *ten_J, *actuator_moment, *qfrc_bias, *qfrc_passive, *qfrc_actuator, *qacc_smooth, *qacc, *act_dot;
} myo_data_out;
int myo_batch_data(myo_batch* b, const double* ctrl, const myo_data_out* out, void* stream);

/* ---- per-env Jacobians (MuJoCo's mj_jacBody / mj_jacBodyCom / mj_jacSite / mj_jacGeom / mj_jacSubtreeCom / mj_jac) at the envs' PRESENT
 * states: what task-space rewards, operational-space analysis and the mapping of contact forces to joints are made of.  One wave per
 * env runs the position stage alone and writes, for each of the k objects obj_ids[0 .. k) (dev int32, any order, repeats allowed), the
 * dense 3 x nv blocks
 *   jacp [N, k, 3, nv]   jacp[e, o] . qvel = world-frame linear velocity of the object's point
 *   jacr [N, k, 3, nv]   jacr[e, o] . qvel = world-frame angular velocity of the object's body
 * in MuJoCo's conventions: a free joint's three rotational dofs are in the body's local frame, as in qvel; columns of dofs that do not
 * move the object's body are written as 0.0.  EVERY element of a non-NULL output is written: the caller does not pre-zero.  The point
 * is the one myo_batch_data reports for the object, with the env's own geometry:
 *   MYO_JAC_BODY        xpos          (points != NULL: the world point points[e, o], rigidly attached to body obj_ids[o] — mj_jac)
 *   MYO_JAC_BODYCOM     xipos
 *   MYO_JAC_SITE        site_xpos     (the Baoding target sites where the task puts them)
 *   MYO_JAC_GEOM        geom_xpos     (the die's size delta moves its geoms)
 *   MYO_JAC_SUBTREECOM  subtree_com   (jacp only: the mass-weighted sum over the body's subtree, with the env's own ball masses)
 * An object on a body with no dof above it — the world body, the die's `target` goal body — has all-zero blocks.  points: dev
 * double[N, k, 3] or NULL.  The ids live on the device, so the host checks what it can — an unknown objtype, k < 0, a NULL obj_ids
 * with k > 0, points with another type than MYO_JAC_BODY, a jacr with MYO_JAC_SUBTREECOM: MYO_E_ARG — and an id outside the model
 * gets all-zero blocks (as an env index outside the batch does in myo_batch_tendon_paths).  A NULL batch / struct or another `size`
 * returns MYO_E_BADARG (= MYO_E_ARG); all before any device call.  Both outputs NULL, or k = 0, launches nothing.  Read-only exactly
 * as myo_batch_sense is. */
enum { MYO_JAC_BODY = 0, MYO_JAC_BODYCOM, MYO_JAC_SITE, MYO_JAC_GEOM, MYO_JAC_SUBTREECOM };
typedef struct myo_jac_out {
  size_t size;
  double *jacp, *jacr;
} myo_jac_out;
int myo_batch_jac(myo_batch* b, int objtype, const int32_t* obj_ids, int k, const double* points, const myo_jac_out* out, void* stream);

/* ---- per-env inverse dynamics (MuJoCo's mj_inverse) at the envs' PRESENT states (qpos, qvel, act, the env's own ball and die
 * parameters): the generalised force that produces the acceleration qacc (dev double[N, nv], required), constraints included —
 * torque and muscle-load estimation, and the forward / inverse consistency check.  One wave per env runs the position, inertia and
 * velocity stages, builds the constraint set of a substep (limits, friction-loss rows, the collision passes) and its reference
 * accelerations, then jar = J qacc - aref and ONE constraint update:
 *   qfrc_constraint [N, nv]   J' efc_force at that jar
 *   qfrc_inverse    [N, nv]   M qacc + qfrc_bias - qfrc_passive - qfrc_constraint
 * No Newton solve, no actuation stage, no ctrl: with qacc = myo_batch_data's qacc, qfrc_inverse is its qfrc_actuator up to the
 * forward solver's residual.  Read-only exactly as myo_batch_sense is; a pass that has to drop contacts beyond the capacity counts it
 * in myo_batch_health like a substep.  A NULL batch / struct / qacc or another `size` returns MYO_E_BADARG (= MYO_E_ARG) before any
 * device call; a struct whose pointers are both NULL launches nothing. */
typedef struct myo_inverse_out {
  size_t size;
  double *qfrc_inverse, *qfrc_constraint;
} myo_inverse_out;
int myo_batch_inverse(myo_batch* b, const double* qacc, const myo_inverse_out* out, void* stream);

/* ---- per-env static optimisation at the envs' PRESENT states: the actuator inputs that deliver a generalised force — the step after
 * inverse dynamics in a biomechanics tool chain (activations that hold a posture, a reset in muscular equilibrium, supervised
 * activation targets).  The actuation stage is affine in its input: force_i = gain_i u_i + bias_i, u_i = a muscle's activation, or
 * the ctrl of an actuator without an activation state.  With R = actuator_moment [nu, nv], one wave per env solves
 *   minimise  1/2 sum_d w_d (sum_i R[i,d] (gain_i u_i + bias_i) - qfrc_d)^2 + 1/2 reg sum_i (u_i - u_ref_i)^2,   lower_i <= u_i <= upper_i
 * in doubles whatever the batch's dtype, by projected Newton (the scheme of MuJoCo's mju_boxQP), deterministically.  Inputs (dev):
 *   qfrc    [N, nv]            the target, typically myo_batch_inverse's qfrc_inverse; required by any output but gain / bias
 *   weight  [nv] or [N, nv]    (weight_per_env = 0 / 1) w >= 0, negative entries count as 0; NULL: 1 on every dof that some actuator's
 *                              moment row can reach, 0 on the others (a free object's dofs must not pull the fit)
 *   u_ref   [N, nu]            NULL: 0, the classic sum of squared activations; the previous solution gives temporal smoothing
 *   lower, upper [N, nu]       NULL: [0, 1] for muscles, ctrlrange for other actuators with ctrllimited, else unbounded
 *   reg > 0                    (1e-6: activation 1 costs as much as a 1e-3 N m error); max_iter >= 1 (100); else MYO_E_ARG
 * Where an actuator is forcelimited and its gain is not 0, the box is tightened to the interval on which the clamp is inactive; a
 * variable whose interval is empty is pinned at the nearer end of its box, one with lower > upper at lower (both set
 * MYO_STATIC_OPT_PINNED), one with gain 0 at clip(u_ref).  Outputs (dev, any may be NULL):
 *   u, force, gain, bias [N, nu]   the solution, its (clamped) actuator force, and the two curves' values at the present state
 *   qfrc, residual [N, nv]         R' force, and R' force - target (unweighted)
 *   kkt [N]                        max-norm of the projected gradient at u
 *   iters, status [N] int32        Newton steps taken; 0 = converged, bit 0 (MYO_STATIC_OPT_CAP) = stopped at max_iter or without a
 *                                  descent step, bit 2 (MYO_STATIC_OPT_PINNED) = some variable was pinned by an empty interval
 * All outputs NULL launches nothing; a call for gain / bias alone runs no solve and needs no qfrc.  A NULL batch / struct, another
 * `size` or a missing qfrc returns MYO_E_BADARG (= MYO_E_ARG) before any device call.  Read-only exactly as myo_batch_sense is. */
enum { MYO_STATIC_OPT_CAP = 1, MYO_STATIC_OPT_PINNED = 4 };
typedef struct myo_static_opt_in {
  size_t size;
  const double *qfrc, *weight, *u_ref, *lower, *upper;
  int weight_per_env;
  double reg;
  int max_iter;
} myo_static_opt_in;
typedef struct myo_static_opt_out {
  size_t size;
  double *u, *force, *qfrc, *residual, *gain, *bias, *kkt;
  int32_t *iters, *status;
} myo_static_opt_out;
int myo_batch_static_opt(myo_batch* b, const myo_static_opt_in* in, const myo_static_opt_out* out, void* stream);

/* ---- per-env inverse kinematics: the joint pose that puts k sites on k world targets — the first link of the tool chain above
 * (task-space data such as fingertip targets or marker positions -> qpos -> inverse dynamics -> static optimisation).  The ACTIVE
 * joints are the model's hinge and slide joints, or those of them whose dof is set in `active`; every other qpos entry (the balls'
 * and the die's free joints) stays at its start value.  One wave per env solves
 *   minimise  1/2 sum_o w_o |site_xpos_o(q) - t_o|^2 + 1/2 reg sum_a (q_a - q_ref_a)^2,   lower_a <= q_a <= upper_a
 * in doubles whatever the batch's dtype, by projected Levenberg-Marquardt (each step a box QP solved by projected Newton, accepted on
 * the cost of a fresh position pass, so the cost never increases), deterministically.  The env's record is only read: the envs'
 * states do not move.  Inputs (dev):
 *   site_ids [k] int32         the sites to place, k <= MYO_IK_K_MAX; an id outside the model contributes nothing (its output rows are 0)
 *   targets  [N, k, 3]         world positions; required
 *   weight   [k] or [N, k]     (weight_per_env = 0 / 1) w >= 0, negative entries count as 0; NULL: 1
 *   q_init   [N, nq]           the start point (every entry, frozen ones included); NULL: the env's present qpos.  Projected into the box
 *   q_ref    [N, nq]           the regularisation centre; NULL: the start point as given
 *   lower, upper [N, nv]       indexed by dof; NULL: jnt_range where jnt_limited, else unbounded.  lower > upper pins the joint at
 *                              lower (MYO_IK_PINNED)
 *   active                     dof mask, bit i = dof i; 0: every hinge / slide dof; bits of other joints' dofs are ignored
 *   reg > 0 finite (1e-6), tol > 0 (1e-10), max_iter >= 1 (50); else MYO_E_ARG
 * It stops when the projected gradient's max-norm is <= tol (1 + |J'We|_inf at the start), after max_iter steps (MYO_IK_CAP), or
 * when the damping passes its cap without an acceptable step (MYO_IK_STALL).  Outputs (dev, any may be NULL):
 *   qpos [N, nq]                     the solution: an accepted iterate or the projected start; frozen entries bit for bit the start's
 *   site_xpos, residual [N, k, 3]    the sites there, and position - target (unweighted)
 *   cost, kkt [N]                    the cost there and the projected gradient's max-norm
 *   iters, status [N] int32          accepted + rejected steps; 0 = converged, else bits MYO_IK_CAP / MYO_IK_STALL / MYO_IK_PINNED
 * k = 0 is legal (q goes to clip(q_ref)).  All outputs NULL launches nothing.  A NULL batch / struct, another `size` or missing
 * targets (k > 0) returns MYO_E_BADARG (= MYO_E_ARG); k < 0, k > MYO_IK_K_MAX, a NULL site_ids with k > 0, a bad reg / tol / max_iter
 * MYO_E_ARG; all before any device call. */
#define MYO_IK_K_MAX 16
enum { MYO_IK_CAP = 1, MYO_IK_STALL = 2, MYO_IK_PINNED = 4 };
typedef struct myo_ik_in {
  size_t size;
  const int32_t* site_ids;
  int k;
  const double *targets, *weight;
  int weight_per_env;
  const double *q_init, *q_ref, *lower, *upper;
  uint64_t active;
  double reg, tol;
  int max_iter;
} myo_ik_in;
typedef struct myo_ik_out {
  size_t size;
  double *qpos, *site_xpos, *residual, *cost, *kkt;
  int32_t *iters, *status;
} myo_ik_out;
int myo_batch_ik(myo_batch* b, const myo_ik_in* in, const myo_ik_out* out, void* stream);

/* ---- read-only open-loop simulation: what happens from this state under these controls?  S control sequences ("samples") for each
 * of k listed envs, T control steps of nsub substeps each, in ONE launch of k S workgroups — the primitive of sampling-based control
 * (MPPI, predictive sampling), of tracking controllers, of finite-difference linearisation, and the check that static optimisation's
 * activations deliver the motion they were solved for.  Each sample runs on a copy of the env's whole record in a workspace of the
 * library's own (the env's warm start, time, per-episode ball / object parameters and task block go with it): the env's record is
 * only read, the envs do not move, and an env may be listed more than once.  The stepper is the batch's own (dtype, integrator,
 * contact capacity); the controls are muscle controls exactly as myo_batch_physics_step takes them: no action map, no fatigue
 * advance, no task layer, no reset.  Row (e, j) below is sample j of env env_idx[e].  Inputs (dev):
 *   env_idx  [k] int32               the envs; NULL: envs 0 .. k - 1 (k = N: all envs in order).  An index outside [0, N): the rows of
 *                                    its samples are NaN, bad = 1, steps = 0
 *   k >= 0, S >= 1, T >= 1           k S must fit an int
 *   nsub >= 0                        substeps per control step; 0: the task's frame_skip (1 without a task layer)
 *   every >= 1                       the state is recorded after every `every`-th control step: R = T / every rows; T % every must be 0
 *   ctrl                             [k, S, T, nu] (ctrl_per_sample = 1) or [k, T, nu] shared by an env's samples (0); NULL: zeros
 *   qpos0, qvel0, act0               [k, S, nq / nv / na]: the samples' start states; NULL: the env's own
 *   site_ids [ns] int32              sites whose world positions are recorded, ns <= MYO_SIM_NS_MAX; an id outside the model gives NaN
 * Outputs (dev, doubles, any may be NULL):
 *   qpos [k, S, R, nq], qvel [k, S, R, nv], act [k, S, R, na], time [k, S, R]     the state after control step (row + 1) * every
 *   site_xpos [k, S, R, ns, 3]       the listed sites there (one extra position pass per recorded step), as myo_batch_data places them
 *   bad, steps [k, S] int32          a sample whose state blows up (MuJoCo's mj_checkPos / mj_checkVel / mj_checkAcc) stops: bad = 1,
 *                                    steps = the control steps it completed, its remaining rows NaN; else bad = 0, steps = T
 * The same bits on every run, whatever S and whoever a sample's neighbours are.  k = 0 or all outputs NULL launches nothing.  The
 * workspace (k S rows of one record, plus the RK4 stage block where that lives in global memory) grows on demand and is freed with
 * the batch; growing it frees the old block, so a call that has to grow it while `stream` is capturing returns MYO_E_STATE: size it
 * with an eager call of the same k S first.  A NULL batch / struct or another `size` returns MYO_E_BADARG (= MYO_E_ARG); a bad
 * k / S / T / nsub / every / ns, T % every != 0, k S beyond an int, site outputs without site_ids: MYO_E_ARG; all before any device
 * call. */
#define MYO_SIM_NS_MAX 16
typedef struct myo_sim_in {
  size_t size;
  const int32_t* env_idx;
  int k, S, T, nsub, every;
  const double* ctrl;
  int ctrl_per_sample;
  const double *qpos0, *qvel0, *act0;
  const int32_t* site_ids;
  int ns;
} myo_sim_in;
typedef struct myo_sim_out {
  size_t size;
  double *qpos, *qvel, *act, *time, *site_xpos;
  int32_t *bad, *steps;
} myo_sim_out;
int myo_batch_simulate(myo_batch* b, const myo_sim_in* in, const myo_sim_out* out, void* stream);

/* ---- rendering of env states (MuJoCo's mjr_render / mjr_readPixels seam: CustomPenEnv.render -> self.sim.render,
 * /root/reference/src/main_eval.py:96-97).  Draws what the stepper holds: every geom at the pose of the env's present state
 * and with the env's own geometry (Baoding P2 ball radius, die size delta), the Baoding target sites where the task puts
 * them, the die's `target` body at the episode's goal_pos / goal_quat, and — with MYO_RENDER_TENDONS — the spatial tendons
 * as capsules along their paths, coloured by muscle activation (myo_batch_tendon_paths).  Wrap arcs are drawn as chords.
 * No model cameras, no lights or shadows.
 *
 * Render items: the ngeom geoms, then the nsite sites (spheres of site_size[0]).  Visibility and colour: MuJoCo's rule when
 * the model carries geom_rgba (groups 0-2, alpha > 0, mat_rgba where matid >= 0); without visual data (the synthetic models)
 * they are derived — colliding hand geoms one skin colour, free-joint bodies distinct colours, non-colliding geoms of a body
 * welded to the world translucent, wrap-only geoms hidden.  Sites other than the task's targets are drawn only with
 * MYO_RENDER_SITES (MuJoCo would draw every site of groups 0-2). */
typedef struct myo_render_camera {      /* MuJoCo's free camera (mjvCamera, type mjCAMERA_FREE); angles in degrees */
  double lookat[3];
  double distance, azimuth, elevation;
  double fovy;                          /* vertical field of view (mjVisual.global.fovy) */
} myo_render_camera;
#define MYO_RENDER_RGB 1
#define MYO_RENDER_DEPTH 2
#define MYO_RENDER_SEG 4
#define MYO_RENDER_SITES 8              /* draw every site, not only the task's targets */
#define MYO_RENDER_TENDONS 16           /* draw the tendon items of myo_batch_tendon_paths after the geoms and sites */
#define MYO_RENDER_CONTACTS 32          /* draw the contact items of myo_batch_contact_items (points and forces) after them; bit 64 is
                                         * reserved and refused */
#define MYO_RENDER_ITEM_N 24            /* doubles per item of myo_batch_geom_poses / myo_batch_tendon_paths */
#define MYO_RENDER_MAX_PIXELS (1 << 24) /* width * height */

/* the model's default free camera: lookat = stat.center, distance = 1.5 stat.extent (without stat in the model: the bounding
 * sphere of the drawn geoms at qpos0, centre c and radius r, as lookat = c, extent = 2 r); azimuth 90, elevation -45, fovy 45
 * (MuJoCo 2.1's mjVisual.global defaults) */
int myo_model_default_camera(const myo_model* m, myo_render_camera* out);

/* Pose pass: for envs env_idx[0 .. k) (dev int32; an index outside [0, N) gets an all-zero row: nothing drawn), one wave per env loads the env's state and runs the
 * stepper's kinematics; out (dev double[k, ngeom + nsite, MYO_RENDER_ITEM_N]) receives per item: world position [0..3),
 * world rotation matrix, row-major [3..12), size [12..15), type (mjtGeom; sites: sphere) [15], rgba [16..20) (alpha 0:
 * never drawn), bounding radius [20], 1 for a site drawn only with MYO_RENDER_SITES [21], 0 [22..24).  Reads the env
 * records only: no record, draw counter, warm start or health counter changes. */
int myo_batch_geom_poses(myo_batch* b, const int32_t* env_idx, int k, double* out, void* stream);

/* Tendon path pass: for envs env_idx[0 .. k) (dev int32; an index outside [0, N) gets an all-zero row), one wave per env loads
 * the env's state, runs the stepper's kinematics and the stepper's own wrap solver, and writes every straight piece of every
 * spatial tendon as one item of the pose pass's format into out (dev double[k, ntendon_item, MYO_RENDER_ITEM_N];
 * ntendon_item = myo_model_size(m, "ntendon_item"), a model constant: 1 slot per site -> site path element, 3 per element
 * around a sphere / cylinder wrap — an upper bound over all wrap states; unused slots are all-zero rows, alpha 0 = never drawn).
 * Pieces: site -> site; around an active wrap site -> tangent point, the chord between the two tangent points, tangent point ->
 * site; site -> site when the wrap is inactive.  A pulley ends a branch: no piece crosses it.  Per item: position [0..3) = the
 * piece's midpoint, rotation [3..12) with its z axis (third column) along the piece, size [12..15) = radius, half length, 0,
 * type [15] = capsule, rgba [16..20), bounding radius [20] = radius + half length, 0 [21], tendon id + 1 [22], and [23] the
 * piece's contribution to the tendon's length in metres: its length (a chord: the arc length of the wrap it stands for), divided by
 * the divisor of the last pulley before it — the sum of [23] over a tendon's items is ten_length.
 * Radius and base colour: tendon_width and tendon_rgba (mat_rgba where tendon_matid >= 0; groups 0-2 and alpha > 0 are drawn)
 * where the model carries visual data; without it (the synthetic models) radius 0.002 m and rgba (0.30, 0.35, 0.75, 1).
 * Colour rule — this library's own, NOT MuJoCo's (whose tendon colouring is not reproduced or claimed here): a tendon that is the
 * transmission target of a muscle actuator (the first such actuator) has rgb = (1 - a) base + a active, with a that actuator's
 * activation clamped to [0, 1] and active = (1.00, 0.90, 0.10); alpha and every other tendon keep the base colour.
 * Reads the env records only: no record, draw counter, warm start, workspace ownership flag or health counter changes.  A null
 * output or k < 0 returns MYO_E_ARG before any device call. */
int myo_batch_tendon_paths(myo_batch* b, const int32_t* env_idx, int k, double* out, void* stream);

/* Contact item pass (MuJoCo's mjVIS_CONTACTPOINT / mjVIS_CONTACTFORCE): for envs env_idx[0 .. k) (dev int32; an index outside
 * [0, N) gets all-zero rows), one wave per env runs the forward pass of myo_batch_sense at the env's present state — the same device
 * functions, so the contacts are the ones myo_batch_sense reports for that state: same pair order, same slots, same warm-started
 * solve — and one lane per contact slot writes two items of the pose pass's format into out (dev double[k, 2 * cap,
 * MYO_RENDER_ITEM_N], cap = myo_batch_contact_capacity).  Slot c owns rows 2c and 2c + 1; rows of slots >= ncon are all zero
 * (alpha 0 = never drawn).
 *   row 2c, the contact point: a cylinder (a flat disc) centred at the contact's pos; rotation [3..12) with its third column the
 *     contact normal and the first two mju_makeFrame's tangents of it, in that order; size [12..15) = disc_radius, disc_half_height,
 *     0; type [15] = cylinder; rgba [16..20) = point_rgba; bounding radius [20] = sqrt(radius^2 + half height^2); 0 [21];
 *     slot + 1 [22]; the contact's dist [23].
 *   row 2c + 1, the contact force: the world force on geom2's body, F = n f0 + t1 f1 + t2 f2 from the first three components of
 *     con_d's force[6] in that frame (torsional and rolling components are not drawn), as a capsule from pos to pos +
 *     metres_per_newton * F laid out like a tendon piece: midpoint [0..3), rotation with its third column along F, size =
 *     force_radius, half length, 0; rgba = force_rgba; bounding radius = radius + half length; 0 [21]; slot + 1 [22]; |F| in
 *     newtons [23].  |F| == 0 (a contact inside the margin that carries no force): an all-zero row.  No arrow head: a shaft only.
 * Sizes and colours come from the batch's myo_render_style — this library's own drawing rule, NOT MuJoCo's (whose contact
 * colouring and meansize / meanmass scaling are not reproduced or claimed here).  Defaults, for a hand-sized scene: disc radius
 * 0.003 m, half height 0.0005 m; shaft radius 0.001 m; 0.02 m/N; point_rgba (0.9, 0.6, 0.2, 1); force_rgba (0.7, 0.9, 0.9, 1);
 * geom_alpha 1.  geom_alpha multiplies the alpha of GEOM items (not sites, tendons or contact items) in renders with
 * MYO_RENDER_CONTACTS only — mjVIS_TRANSPARENT's job: a disc sits inside the penetration of two surfaces and is hidden otherwise.
 * `size` = sizeof(myo_render_style), first, so that the struct can grow; set / get with another size, a NULL argument, a
 * non-finite or negative length, or a colour component / geom_alpha outside [0, 1] return MYO_E_ARG.
 * The pass is read-only exactly as myo_batch_sense is: no record, warm start, draw counter, step generation or wrap order changes; a
 * pass that has to drop contacts beyond the capacity counts it in myo_batch_health.  A null output or k < 0 returns MYO_E_ARG before
 * any device call. */
typedef struct myo_render_style {
  size_t size;
  double disc_radius, disc_half_height, force_radius, metres_per_newton;
  float point_rgba[4], force_rgba[4];
  double geom_alpha;
} myo_render_style;
int myo_batch_set_render_style(myo_batch* b, const myo_render_style* style);
int myo_batch_get_render_style(const myo_batch* b, myo_render_style* style);
int myo_batch_contact_items(myo_batch* b, const int32_t* env_idx, int k, double* out, void* stream);

/* Pinhole ray casting of the items of envs env_idx[0 .. k): one ray through every pixel centre, row 0 at the top (gym's
 * rgb_array; mjr_readPixels is bottom-up).  cams: HOST array of ncams cameras, ncams = 1 (all envs) or k (one per env).
 * flags: MYO_RENDER_* ; each requested output is a dev buffer owned by the caller:
 *   rgb   uint8 [k, height, width, 3]  headlight Lambert shading rgb * (0.3 + 0.7 |n . d|) over a fixed background; a
 *                                      translucent item (alpha < 1) nearer than the nearest opaque one is blended over it
 *   depth float [k, height, width]     distance along the camera axis, +inf for the background
 *   segid int32 [k, height, width]     geom id, ngeom + site id for sites, ngeom + nsite + tendon id for tendons, ngeom + nsite +
 *                                      ntendon + contact slot for both items of a contact, -1 for the background
 * With MYO_RENDER_TENDONS the tendon items are drawn after the geoms and sites under the same shading, translucency, depth and
 * tile-culling rules (a second pass of the tile over the same pixels; a model with more than 512 tendon items is refused with
 * MYO_E_ARG, never truncated).  Without the flag nothing about the call changes.
 * With MYO_RENDER_CONTACTS the contact items of myo_batch_contact_items are drawn after those, under the same rules (one more pass
 * of the tile over the same pixels), and the geoms' alpha is multiplied by the style's geom_alpha.  Without the flag the call
 * launches exactly what it launched before the flag existed.
 * Depth and segmentation are those of the nearest drawn surface, translucent ones included.  Invalid arguments return
 * MYO_E_ARG before any device call. */
int myo_batch_render(myo_batch* b, const int32_t* env_idx, int k, const myo_render_camera* cams, int ncams, int width, int height,
                     int flags, uint8_t* rgb, float* depth, int32_t* segid, void* stream);

/* average duration (ms) of the step kernel over the launches since the last call, measured
 * with HIP events on the launch stream; resets the accumulator.  Returns <0 if no launch. */
double myo_batch_kernel_ms(myo_batch* b);
int myo_batch_enable_timing(myo_batch* b, int on);

/* Elementwise part of one PPO minibatch step in a single launch (SB3 PPO.train loss terms; the
 * reference runs them as separate torch ops inside sb3_contrib.RecurrentPPO.train,
 * /root/reference/src/train/trainer.py:66-71).  All pointers dev float32: mean[B,A] values[B]
 * actions[B,A] old_logp[B] adv[B] (raw) returns[B] log_std[A] adv_stats[2]={mean,std of adv}.
 * Outputs: dmean[B,A], dvalue[B] = d loss/d(policy mean, value); acc[2A+3] = {sum_i dlogp_i (z^2-1)
 * per action dim (entropy term not included) [A], policy loss, value loss, sum_i dmean[i,:] [A],
 * sum_i dvalue[i]} (the last two are the bias gradients of the action / value heads).
 * dmean_bf16 / dvalue_bf16: optional (NULL) bfloat16 copies of dmean / dvalue for the backward GEMMs.
 * work: dev float32 [ceil(B/64) * (2A+3)] scratch; the sums are formed from per-block partials in
 * block order by a second small launch (deterministic, no float atomics).
 * in_bf16 != 0: `mean` and `values` point to bfloat16 data (the GEMM outputs) instead of float32.
 * Optional direct gradient outputs (NULL to skip): g_log_std[A] = acc[0..A) - ent_coef,
 * g_bias_pi[A] = acc[A+2..2A+2), g_bias_vf[1] = acc[2A+2].
 * hp: the PPO hyper-parameter block (layout below, beside myo_ppo_mlp_desc) or NULL = all of the above.  With it clip_range is
 * hp[MYO_HP_CLIP] (`clip` is ignored), `work` has ceil(B/64) * (2A+6) floats (three more columns: approx_kl, clip fraction,
 * entropy loss) and the second launch records the minibatch in the block and raises its stop flag when approx_kl >
 * hp[MYO_HP_KL_LIMIT]. */
int myo_ppo_loss_grad(const float* mean, const float* values, const float* actions, const float* old_logp,
                      const float* adv, const float* returns, const float* log_std, const float* adv_stats,
                      int B, int A, float clip, float vf_coef, float* dmean, float* dvalue, float* acc,
                      uint16_t* dmean_bf16, uint16_t* dvalue_bf16, float* work, int in_bf16, float ent_coef,
                      float* g_log_std, float* g_bias_pi, float* g_bias_vf, float* hp, void* stream);

/* The same stage for generalised state-dependent exploration (SB3 StateDependentNoiseDistribution, learn_features = False), in
 * two launches (csrc/myo_sde_loss.h), fp32 arithmetic on the bf16 trunk outputs:
 *   var[i,a] = sum_l latent[i,l]^2 exp(2 log_std[l,a]) + sde_eps     (the latent is detached: log_std sees the loss through var only)
 *   logp[i]  = sum_a (-0.5 (action - mean)^2 / var - 0.5 log var) - 0.5 A log 2 pi;  entropy[i] = sum_a 0.5 log var + 0.5 A (1 + log 2 pi)
 * and the clipped surrogate, value loss and diagnostics of the Gaussian stage above.  mean_bf16 [B,A], value_bf16 [B], latent_bf16
 * [B,L] (contiguous) are bfloat16; actions [B,A], old_logp, adv (raw), returns [B], log_std [L,A], adv_stats {mean, std} float32.
 * Outputs: dmean_bf16 [B,A], dvalue_bf16 [B] (bfloat16, round-to-nearest-even), g_log_std [L,A] (entropy term included),
 * g_bias_pi [A] and g_bias_vf [1] (column sums of the unrounded dmean / dvalue), acc[A] = policy loss, acc[A+1] = value loss (no other
 * word of acc is written).  hp: NULL or the hyper-parameter block, as above (clip_range, diagnostics, KL stop).  work: dev float32 of
 * the size the second function gives; no initialisation needed.  Sums over the batch are formed from per-block partials in block
 * order by the second launch (deterministic, no float atomics); a block owns up to ceil(B / 8192) tiles of 64 rows, so the [L,A]
 * partials never exceed 128 per call.  Any B from 1 to 2^24.  A NULL pointer other than hp, or B / L / A < 1, returns MYO_E_ARG
 * before any device call; L > 256 or A > 64 returns MYO_E_UNSUPPORTED (the first function: 1 where the shape is supported). */
int myo_ppo_sde_loss_supported(int L, int A);
long long myo_ppo_sde_loss_work_floats(int B, int L, int A);
int myo_ppo_sde_loss_grad(const uint16_t* mean_bf16, const uint16_t* value_bf16, const uint16_t* latent_bf16, const float* actions,
                          const float* old_logp, const float* adv, const float* returns, const float* log_std, const float* adv_stats,
                          int B, int L, int A, float clip, float vf_coef, float ent_coef, float sde_eps, uint16_t* dmean_bf16,
                          uint16_t* dvalue_bf16, float* g_log_std, float* g_bias_pi, float* g_bias_vf, float* acc, float* work, float* hp,
                          void* stream);

/* Minibatch gather of one optimiser step (SB3 RolloutBuffer.get + the per-minibatch advantage
 * normalisation statistics of PPO.train): rows idx[0..bs) (dev int64) of obs[N,obs_dim] act[N,act_dim]
 * oldlp[N] adv[N] ret[N] (dev float32) -> obs_bf16 [copies, bs, obs_dim] (bfloat16), act_mb, oldlp_mb,
 * adv_mb, ret_mb, adv_stats[2] = {mean, unbiased std} of adv_mb.  work: dev float32
 * [2*ceil(bs/16)] scratch (block moments, merged in block order by a second small launch). */
int myo_ppo_gather(const float* obs, const float* act, const float* oldlp, const float* adv, const float* ret,
                   const int64_t* idx, int bs, int obs_dim, int act_dim, uint16_t* obs_bf16, int copies,
                   float* act_mb, float* oldlp_mb, float* adv_mb, float* ret_mb, float* adv_stats /* NULL: not computed */, float* work,
                   void* stream);

/* The gather for a minibatch of m CHUNKS of L consecutive rollout steps (recurrent PPO with PPOConfig.seq_len; sb3-contrib
 * RecurrentRolloutBuffer._get_samples: a sequence starts from the LSTM state stored with its first transition).  chunk[j] = s*N + n
 * (dev int64) names steps [s*L, (s+1)*L) of env n; output row r = t*m + j (t-major) takes rollout row (s*L + t)*N + n.
 * obs [T,N,obs_dim] act [T,N,act_dim] oldlp / adv / ret / starts [T,N] (dev float32), T % L == 0, S = T / L; h_snap bfloat16 and
 * c_snap float32 [S,G,N,H] (H % 8 == 0): the state that entered step s*L of the rollout, before the episode-start mask.
 * -> obs_bf16 [copies, L*m, obs_dim], act_mb [L*m, act_dim], oldlp_mb / adv_mb / ret_mb [L*m], keep [L,m] = 1 - starts,
 *    hm0 bfloat16 [G,m,H] = h_snap * keep[0], cm0 bfloat16 [G,m,H] and c0_32 float32 [G,m,H] = c_snap * keep[0] (c0_32 unrounded),
 *    adv_stats[2] as above (same partition and merge: bit-identical to the plain gather on the same rows; NULL: not computed).
 * work: dev float32 [2*ceil(L*m/16)].  MYO_E_ARG for NULLs, m < 1, L < 1, T % L != 0. */
int myo_ppo_gather_seq(const float* obs, const float* act, const float* oldlp, const float* adv, const float* ret,
                       const float* starts, const void* h_snap, const float* c_snap, const int64_t* chunk, int T, int N, int L, int m,
                       int G, int H, int obs_dim, int act_dim, uint16_t* obs_bf16, int copies, float* act_mb, float* oldlp_mb,
                       float* adv_mb, float* ret_mb, float* keep, uint16_t* hm0, uint16_t* cm0, float* c0_32,
                       float* adv_stats /* NULL: not computed */, float* work, void* stream);

/* Activation of the hidden MLP layers (torch.nn.ReLU, torch.nn.Tanh: SB3's default) of every fused PPO path.  It is an argument
 * of the *_act entry points below, not a descriptor field (the descriptors keep their size); any other code: MYO_E_ARG.  tanh is
 * ONE formula in every kernel, 1 - 2 / (e^2x + 1), evaluated in double from the fp32 pre-activation (saturates to exactly +-1),
 * rounded to bfloat16 once; its backward is
 * bf16(dy) * (1 - h * h) on the STORED bfloat16 output h, the product rounded once (autograd under bf16 autocast). */
#define MYO_ACT_RELU 0
#define MYO_ACT_TANH 1
/* h <- activation(h + bias) in place: bfloat16 h[groups, rows, cols], bias[groups, cols] (cols even). */
int myo_bias_act_bf16(uint16_t* h, const uint16_t* bias, int groups, int rows, int cols, int activation, void* stream);
/* ... with MYO_ACT_RELU: h <- max(h + bias, 0). */
int myo_bias_relu_bf16(uint16_t* h, const uint16_t* bias, int groups, int rows, int cols, void* stream);

/* Finishes a split-K product: out[g, j] = sum_k part[g, k, j]; part dev [groups, splits, n] of
 * bfloat16 (part_is_bf16 != 0) or float32, n even; out dev float32 [groups, n]. */
int myo_splitk_reduce(const void* part, int part_is_bf16, float* out, int groups, int splits, int n, void* stream);
/* Two such reductions in one launch (a layer's weight-gradient partials and its bias partials; the two head
 * gradients): same arguments and the same arithmetic as two myo_splitk_reduce calls. */
int myo_splitk_reduce2(const void* part_a, int a_is_bf16, float* out_a, int groups_a, int splits_a, int n_a,
                       const void* part_b, int b_is_bf16, float* out_b, int groups_b, int splits_b, int n_b, void* stream);

/* Activation backward in place on bfloat16 dy[rows, cols] from the layer's OUTPUT act (ReLU: dy *= act > 0; tanh: dy <-
 * bf16(dy * (1 - act * act))) plus column sums of the result over blocks of 32 rows: partial dev float32 [rows/32, cols]
 * (finish with myo_splitk_reduce: the bias gradient).  rows % 32 == 0, cols/2 divides 256. */
int myo_act_bwd_colsum_bf16(uint16_t* dy, const uint16_t* act, int rows, int cols, float* partial, int activation, void* stream);
/* ... with MYO_ACT_RELU. */
int myo_relu_bwd_colsum_bf16(uint16_t* dy, const uint16_t* act, int rows, int cols, float* partial, void* stream);

/* ---- per-step rollout plumbing (between two myo_batch_step launches) ------------------------------
 * `t_idx`: dev int32 = rollout-buffer row of the current step; `draw_counter`: dev uint64[2] (Philox
 * stream position, [1] is the pending value).  Buffers are dev float32, row-major [T, N, ...].
 *
 * policy input: obs [N,O] -> obs_buf[t] (may be NULL) and `copies` stacked bfloat16 copies. */
int myo_rollout_policy_input(const float* obs, int N, int O, float* obs_buf, uint16_t* x_bf16, int copies,
                             const int32_t* t_idx, void* stream);
/* SB3 DiagGaussianDistribution sample + log_prob (RecurrentPPO.collect_rollouts ->
 * policy.forward, /root/reference/src/train/trainer.py:66-71): a = mean + exp(log_std) * eps, eps from
 * Philox4x32-10(seed, draw_counter[0]); writes act_buf[t], val_buf[t] (from value_bf16), logp_buf[t]
 * and clipped = clip(a, -1, 1) [N,A] (the env input). */
int myo_rollout_sample(const uint16_t* mean_bf16, const uint16_t* value_bf16, const float* log_std, int N, int A,
                       uint64_t seed, uint64_t* draw_counter, const int32_t* t_idx, float* act_buf, float* val_buf,
                       float* logp_buf, float* clipped, int deterministic, void* stream);
/* stable_baselines3 VecNormalize.step_wait for one batched step (VecNormalize.load / .normalize_obs:
 * /root/reference/src/main_baoding.py:75, src/metrics/custom_callbacks.py:34): running mean/var of obs
 * and of the discounted return (Chan merge, fp64, in place: obs_mean[O] obs_var[O] obs_count[1],
 * ret_stats[3] = mean,var,count, returns[N]), normalised + clipped obs -> nobs [N,O], reward ->
 * rew_buf[t], terminal obs -> term_buf[t] (may be NULL), trunc -> trunc_buf[t] (may be NULL),
 * start_buf[t] <- starts, starts <- done.  work: dev double [ceil(N/128) * 2 * (O+1)]. */
int myo_vecnorm_step(const float* obs, const float* rew, const uint8_t* done, const uint8_t* trunc, const float* term_obs,
                     int N, int O, double* obs_mean, double* obs_var, double* obs_count, double* ret_stats,
                     double* returns, double gamma, double eps, double clip_obs, double clip_rew, int training,
                     int norm_obs, int norm_reward, float* nobs, float* starts, const int32_t* t_idx, float* rew_buf,
                     float* start_buf, float* term_buf, float* trunc_buf, double* work, void* stream);
/* t_idx <- (t_idx + 1) mod T, commit the Philox position. */
/* gSDE action sampling (stable-baselines3 StateDependentNoiseDistribution as the reference's RecurrentPPO(use_sde=True,
 * sde_sample_freq=-1) uses it, /root/reference/docs/summary.md:100): mean f32[N,A], latent f32[N,L] (latent_pi), exploration_mat
 * f32[N,L,A] (one matrix per env, drawn once per rollout), log_std f32[L,A] -> actions (unclipped), clipped, logp f32[N]. */
int myo_rollout_sample_sde(const float* mean, const float* latent, const float* exploration_mat, const float* log_std, int N, int L,
                           int A, float* actions, float* clipped, float* logp, int deterministic, void* stream);

/* myo_vecnorm_step split where N ranks exchange their batch moments (one VecNormalize over the envs of ALL ranks,
 * /root/reference/src/main_baoding.py:75): batch_moments leaves batch[0] = n, batch[1..O+1] = sum x (column O = the
 * discounted returns), batch[O+2..2O+2] = sum x^2 of this rank's step in a caller-owned dev double[2 O + 3]; the
 * caller all-reduces it (SUM); finish then updates the running statistics from it and normalises as myo_vecnorm_step. */
int myo_vecnorm_batch_moments(const float* obs, const float* rew, int N, int O, double* returns, double gamma, int training,
                              double* work, double* batch, void* stream);
int myo_vecnorm_finish(const float* obs, const float* rew, const uint8_t* done, const uint8_t* trunc, const float* term_obs,
                       int N, int O, double* obs_mean, double* obs_var, double* obs_count, double* ret_stats, double* returns,
                       double eps, double clip_obs, double clip_rew, int training, int norm_obs, int norm_reward, float* nobs,
                       float* starts, const int32_t* t_idx, float* rew_buf, float* start_buf, float* term_buf, float* trunc_buf,
                       const double* batch, void* stream);
int myo_rollout_advance(int32_t* t_idx, int T, uint64_t* draw_counter, void* stream);
/* LSTM state entering a chunk of seq_len steps, taken inside the per-step graph (the predicate is read on the device):
 * if (*t_idx % seq_len == 0): h_snap[*t_idx / seq_len] <- h, c_snap[...] <- c32; otherwise nothing, and a slot >= S writes nothing.
 * h bfloat16 [G,N,H], c32 float32 [G,N,H], h_snap bfloat16 [S,G,N,H], c_snap float32 [S,G,N,H]; G*N*H a multiple of 8.
 * MYO_E_ARG for NULLs, seq_len < 1, S < 1. */
int myo_rollout_state_snapshot(const void* h, const float* c32, int G, int N, int H, const int32_t* t_idx, int seq_len, int S,
                               void* h_snap, float* c_snap, void* stream);

/* One time step of G stacked one-layer LSTMs (gate order i, f, g, o) around the recurrent GEMM: the pointwise
 * part of RecurrentActorCriticPolicy's lstm_actor / lstm_critic in collect_rollouts / train
 * (/root/reference/src/train/trainer.py:49-71; sb3-contrib _process_sequence).  Rows r = g * N + n, R = G * N.
 * Storage float32 (is_bf16 = 0) or bfloat16 (1); arithmetic fp32.  keep_next: dev float[N], 0 where the NEXT
 * step starts an episode (NULL = all ones).
 * fwd: gx, gh [R,4H] pre-activations (input and recurrent parts), c_prev [R,H] (already masked) ->
 *      out_h, c_new [R,H] (unmasked), hm_next, cm_next [R,H] (times keep_next: inputs of the next step),
 *      ws [R,4H] (activated gates, for the backward pass).
 * bwd: dout [R,H] (gradient of out_h, may be NULL), dhm_next / dcm_next [R,H] (gradients of hm_next / cm_next
 *      from the later step, NULL at the last step) -> dgates [R,4H] (gradient of gx and of gh), dc_prev [R,H]. */
int myo_lstm_cell_fwd(const void* gx, const void* gh, const void* c_prev, const float* keep_next, int R, int N, int H,
                      int is_bf16, void* out_h, void* hm_next, void* cm_next, void* c_new, void* ws, void* stream);
int myo_lstm_cell_bwd(const void* dout, const void* dhm_next, const void* dcm_next, const float* keep_next,
                      const void* c_prev, const void* c_new, const void* ws, int R, int N, int H, int is_bf16,
                      void* dgates, void* dc_prev, void* stream);

/* The same time step with the recurrent product inside (one launch instead of GEMM + cell kernel): bfloat16 storage, fp32
 * accumulation on the matrix cores; H in {32, 64, 128, 256} (myo_lstm_step_supported).  Arrays are [G, N, .] contiguous except
 *   gx    element (g, n, col) at gx[g*gx_sg + n*gx_sr + col]  (col < 4H; e.g. one [N, G*4H] GEMM output: gx_sg = 4H, gx_sr = G*4H),
 *   out_h element (g, n, u) at out_h[g*out_sg + n*H + u],  dout likewise with dout_sg  (strides in elements, multiples of 4).
 * fwd: h_prev, c_prev [G,N,H] (already masked), w_hh [G,4H,H] (weight_hh_l0 of each LSTM) -> out_h, hm_next, cm_next, c_new, ws
 *      as myo_lstm_cell_fwd; c_new / ws may be NULL (rollout).  The CELL state may travel in float32 beside (or instead of) its
 *      bfloat16 arrays: c_prev32 float32 [G,N,H] (non-NULL: read instead of c_prev), cm_next32 float32 [G,N,H] (non-NULL: written,
 *      unrounded; cm_next may then be NULL) — what an LSTM carries through an episode is c (stock nn.LSTM state is float32,
 *      /root/reference/src/main_reorient.py:53-71); h is the matrix cores' operand and stays bfloat16.
 * bwd: dgates_next [G,N,4H] = the dgates of step t+1 (NULL at the last step), w_hh_t [G,H,4H] = W_hh transposed; the product
 *      dgates_next . W_hh replaces dhm_next of myo_lstm_cell_bwd -> dgates [G,N,4H], dc_prev [G,N,H]. */
int myo_lstm_step_supported(int H);
int myo_lstm_step_fwd(const void* gx, long long gx_sg, long long gx_sr, const void* h_prev, const void* c_prev, const void* w_hh,
                      const float* keep_next, int G, int N, int H, void* out_h, long long out_sg, void* hm_next, void* cm_next,
                      void* c_new, void* ws, const float* c_prev32, float* cm_next32, void* stream);
int myo_lstm_step_bwd(const void* dout, long long dout_sg, const void* dgates_next, const void* dcm_next, const void* w_hh_t,
                      const float* keep_next, const void* c_prev, const void* c_new, const void* ws, int G, int N, int H,
                      void* dgates, void* dc_prev, void* stream);

/* ALL T time steps of the same G stacked LSTMs over N sequences in ONE launch per direction (csrc/myo_lstm_seq.h): what the recurrent
 * PPO minibatch step runs instead of T myo_lstm_step_fwd + T myo_lstm_step_bwd launches (RecurrentPPO.train,
 * /root/reference/src/train/trainer.py:49-71; sb3-contrib _process_sequence).  H in {128, 256} (myo_lstm_seq_supported), N a
 * multiple of 16 (MYO_E_ARG otherwise: the caller keeps the step kernels).  Same roundings as the step kernels.
 * row_split RS in {1, 2} (and 4 at H = 256): a workgroup owns 16 / RS sequences — more, smaller workgroups for small minibatches.
 * The recurrent weights are passed FRAGMENT-MAJOR (one contiguous KB per wave load; permuted from W_hh [G,4H,H] by the caller,
 * once per minibatch step — rl/fused_lstm.py lstm_seq_weights(W_hh, RS)).  With UT = H/128 tiles of 16 units per wave, eight waves,
 * CL = 4*UT/RS, b = i%4 and unit(w, ut, i) = 16*UT*w + 4*UT*(i/4) + CL*(b/(4/RS)) + (4/RS)*ut + b%(4/RS):
 *   w_frag  bf16 [G][8][H/32][4][UT][64][8]:  w_frag[g][w][kk][q][ut][l][j] = W_hh[g][q*H + unit(w, ut, l&15)][32*kk + 8*(l>>4) + j]
 *   wt_frag bf16 [G][8][4H/32][UT][64][8]:   wt_frag[g][w][kk][ut][l][j]   = W_hh[g][32*kk + 8*(l>>4) + j][unit(w, ut, l&15)]
 * The arrays only these two calls exchange — c_new, ws, and cm from slot 1 on — are TILE-MAJOR (same sizes as the row-major
 * shapes below; [(g, r/(16/RS))][wave 8][gate][lane 64][CL], csrc/myo_lstm_seq.h; rl/fused_lstm.py lstm_seq_rows converts).
 * fwd: gx element (t, g, r, col) at gx[t*gx_st + g*gx_sg + r*gx_sr + col]; hm / cm bf16 [T+1,G,N,H]: slot 0 = the masked state
 *      entering step 0 (given, row-major), slots 1..T written (hm row-major, cm tile-major); keep float32 [T,N] (0 where an episode
 *      starts at that step: step t masks its outgoing state with keep[t+1], the last step with 1); out_h element (g, t, r, u) at
 *      out_h[g*out_sg + t*out_st + r*H + u]; c_new [T,G,N,H], ws [T,G,N,4H] (gate activations) kept for the backward pass.
 *      c0_32 float32 [G,N,H] (may be NULL): the masked CELL state entering step 0, unrounded; with it the cell state is carried from
 *      step to step in float32 (the bfloat16 cm slots are still written: the backward pass reads them), without it every step
 *      re-reads its cell state from the bfloat16 slot the previous step wrote (the roundings of T myo_lstm_step_fwd calls on bf16 c).
 * bwd: dout laid out like out_h; keep / cm / c_new / ws as the forward pass left them -> dgates [T,G,N,4H] (row-major). */
int myo_lstm_seq_supported(int H);
int myo_lstm_seq_fwd(const void* gx, long long gx_st, long long gx_sg, long long gx_sr, void* hm, void* cm, const void* w_frag,
                     const float* keep, int G, int N, int H, int T, int row_split, void* out_h, long long out_sg, long long out_st,
                     void* c_new, void* ws, const float* c0_32, void* stream);
int myo_lstm_seq_bwd(const void* dout, long long dout_sg, long long dout_st, const void* wt_frag, const float* keep, const void* cm,
                     const void* c_new, const void* ws, int G, int N, int H, int T, int row_split, void* dgates, void* stream);

/* GAE(gamma, lambda) backward scan = SB3 RolloutBuffer.compute_returns_and_advantage (run by
 * RecurrentPPO.learn, /root/reference/src/train/trainer.py:66-71).  dev float32 [T,N] row-major:
 * rew, val, starts (episode_starts), outputs adv, ret; last_val[N], last_done[N]. */
int myo_gae(const float* rew, const float* val, const float* starts, const float* last_val,
            const float* last_done, int T, int N, float gamma, float lam, float* adv, float* ret,
            void* stream);

/* One PPO minibatch step of the MLP actor-critic (two hidden layers of 256 per net, ReLU or tanh) on the matrix cores: what SB3's
 * PPO.train runs per minibatch through autograd (evaluate_actions -> clipped surrogate + vf_coef * MSE - ent_coef * entropy ->
 * backward; /root/reference/src/train/trainer.py:57-71 hands that loop to sb3-contrib).  Gathers rows
 * idx[0..B) of the rollout arrays, runs forward, loss gradient and backward, and leaves d(loss)/d(param) in `grads` (same flat
 * layout as `params`; offsets in ELEMENTS, [0] actor / [1] critic) and acc[2A+3] = {d log_std[A], policy loss, value loss,
 * action-head bias gradient[A], value-head bias gradient}.  compute_adv_stats != 0: adv_stats <- {mean, unbiased std} of the
 * minibatch advantages (SB3's per-minibatch normalisation); 0: the caller supplies them ({0, 1} = no normalisation).
 * workspace: device memory of myo_ppo_mlp_workspace_bytes() bytes, ZERO-FILLED ONCE by the caller and then owned by these
 * calls (weight images, feature-major activations, split-K slabs).  Deterministic: no float atomics.  Returns
 * MYO_E_UNSUPPORTED for other shapes (hidden != 256, obs > 128, act > 48, B not a multiple of 1024). */
/* The PPO hyper-parameter block: MYO_HP_WORDS 32-bit words of device memory per PPO instance, read by the loss and Adam kernels
 * at RUN time, so a hipGraph captured once follows a learning-rate / clip-range schedule and can stop an update on the device
 * (SB3 PPO.train: learning_rate and clip_range schedules, target_kl).  The host writes it with plain asynchronous copies before
 * an update, outside any graph.  Words (float unless marked int32):
 *   MYO_HP_LR            learning rate of the Adam kernels
 *   MYO_HP_CLIP          clip_range of the loss kernels
 *   MYO_HP_KL_LIMIT      1.5 * target_kl; <= 0: no KL stop (also what N > 1 ranks write: they decide on the all-reduced value)
 *   MYO_HP_STOP          int32, STICKY: raised by the kernel that finishes a minibatch's loss sums when approx_kl > limit.  While
 *                        it is up the gradient-norm / Adam kernels leave p, m, v, the bf16 shadow and the step counter alone and
 *                        nothing below is updated, so the rest of a replayed chunk of steps changes nothing.  Host-cleared.
 *   MYO_HP_APPLIED       int32: optimizer steps applied (advanced by the Adam kernel)
 *   MYO_HP_COUNT         int32: minibatches recorded in the three sums (the one that raised the flag included, as in SB3)
 *   MYO_HP_SUM_KL, MYO_HP_SUM_CLIPFRAC, MYO_HP_SUM_ENTLOSS   sums over the recorded minibatches of approx_kl =
 *                        mean((ratio - 1) - log ratio), mean(|ratio - 1| > clip_range) and -mean(entropy)
 *   MYO_HP_LAST_KL, MYO_HP_LAST_PL, MYO_HP_LAST_VL           approx_kl, policy loss, value loss of the last recorded minibatch */
#define MYO_HP_LR 0
#define MYO_HP_CLIP 1
#define MYO_HP_KL_LIMIT 2
#define MYO_HP_STOP 3
#define MYO_HP_APPLIED 4
#define MYO_HP_COUNT 5
#define MYO_HP_SUM_KL 6
#define MYO_HP_SUM_CLIPFRAC 7
#define MYO_HP_SUM_ENTLOSS 8
#define MYO_HP_LAST_KL 9
#define MYO_HP_LAST_PL 10
#define MYO_HP_LAST_VL 11
#define MYO_HP_WORDS 16
/* Where the MLP actor-critic's tensors lie in its flat fp32 parameter (and gradient) vector: offsets in ELEMENTS, [0] actor /
 * [1] critic; W1 [hidden, obs], W2 [hidden, hidden], Wh [act, hidden] (actor) and [1, hidden] (critic), row-major, their biases,
 * log_std [act]. */
typedef struct myo_mlp_layout {
  int64_t off_W1[2], off_b1[2], off_W2[2], off_b2[2], off_Wh[2], off_bh[2], off_log_std;
} myo_mlp_layout;
typedef struct myo_ppo_mlp_desc {
  const float *obs, *act, *oldlp, *adv, *ret;
  const int64_t* idx;
  int32_t B, O, A, hidden;
  const float* params;
  float* grads;
  int64_t G;
  myo_mlp_layout layout;
  float clip, vf_coef, ent_coef;
  int32_t compute_adv_stats;
  float* adv_stats;
  float* acc;
  void* workspace;
  int64_t workspace_bytes;
  /* single-rank tail (both NULL: off): the squares of the finished gradient, in myo_ppo_mlp_sqnorm_parts(act_dim) partial sums
   * -> sqnorm_part, and Adam's step counter advanced (adam_step: the int32[2] `step` of myo_adam_desc) — then myo_adam_step
   * with nparts = that many.  Not for N > 1 ranks: there the gradient changes (all-reduce) before it is clipped. */
  float* sqnorm_part;
  int32_t* adam_step;
  /* hyper-parameter block (above) or NULL = as without it: clip_range comes from it instead of `clip`, and the launch that
   * finishes the loss sums records the minibatch, takes the KL-stop decision and, stopped, does not advance adam_step. */
  float* hp;
} myo_ppo_mlp_desc;
int myo_ppo_mlp_sqnorm_parts(int act_dim);
long long myo_ppo_mlp_workspace_bytes(int B, int obs_dim, int act_dim, int hidden, long long G);
/* The step for hidden activation `activation` (MYO_ACT_*); resident != 0: with resident operand images (below).  The image pass,
 * the workspace and its size do not depend on the activation.  The tanh step reads each hidden activation back from the
 * feature-major copy in the workspace where the ReLU step keeps one mask bit in a register. */
int myo_ppo_mlp_step_act(const myo_ppo_mlp_desc* d, int resident, int activation, void* stream);
/* ... with MYO_ACT_RELU, resident = 0. */
int myo_ppo_mlp_step(const myo_ppo_mlp_desc* d, void* stream);
/* The same step with RESIDENT operand images, four launches instead of six: the bf16 weight images at the front of `workspace`
 * are taken as current and the advantage moments as the caller's (compute_adv_stats must be 0), so neither the image pass nor
 * the moments pass runs.  The images are current after myo_ppo_mlp_images (once, whenever `params` may have been written from
 * outside: a load, the start of an update) and stay so while every change of `params` is an optimizer step through
 * myo_adam_step with `images` = the same descriptor.  Same results as myo_ppo_mlp_step, bit for bit. */
int myo_ppo_mlp_step_resident(const myo_ppo_mlp_desc* d, void* stream);      /* MYO_ACT_RELU, resident = 1 */
/* The image pass alone: the operand images of `params` into `workspace`, zero padding included (reads B, O, A, hidden, params, G,
 * layout, workspace, workspace_bytes of `d`). */
int myo_ppo_mlp_images(const myo_ppo_mlp_desc* d, void* stream);
/* {mean, unbiased std} of the advantages of n_mb minibatches in two launches: idx int64[n_mb * B] are their rows one minibatch
 * after the other (an epoch's permutation), stats f32[n_mb][2] <- what myo_ppo_mlp_step with compute_adv_stats = 1 leaves in
 * adv_stats for idx[k B .. (k + 1) B), bit for bit.  scratch: f32[192 * n_mb]. */
int myo_ppo_adv_moments_epoch(const float* adv, const int64_t* idx, int B, int n_mb, float* stats, float* scratch, void* stream);

/* One env step's policy call of the rollout for the same MLP actor-critic (collect_rollouts: ActorCriticPolicy.forward,
 * DiagGaussianDistribution.sample / log_prob, RolloutBuffer.add; /root/reference/src/train/trainer.py:66-71 -> agent.learn) in one
 * launch: rows of the policy input obs f32[N,O] -> both trunks and heads on the matrix cores -> actions = mean + exp(log_std) *
 * N(0,1) (Philox, the counters of myo_rollout_sample), log pi, value -> row *t_idx of act_buf [T,N,A], val_buf, logp_buf [T,N]
 * (+ obs_buf [T,N,O] if not NULL), clipped f32[N,A] for the env.  It replaces myo_rollout_policy_input + the trunk / head GEMMs
 * + myo_rollout_sample.  The bf16 weight images it reads live in `workspace` (myo_ppo_mlp_rollout_workspace_bytes, caller-owned);
 * myo_ppo_mlp_rollout_refresh rebuilds them from `params` and has to run after every change of the parameters (once per
 * PPO update).  N must be a multiple of 32; other limits as myo_ppo_mlp_step. */
typedef struct myo_ppo_mlp_rollout_desc {
  const float* obs;
  int32_t N, O, A, hidden;
  const float* params;
  myo_mlp_layout layout;
  uint64_t seed;
  uint64_t* draw_counter;
  const int32_t* t_idx;
  float *obs_buf, *act_buf, *val_buf, *logp_buf, *clipped;
  int32_t deterministic;
  void* workspace;
  int64_t workspace_bytes;
} myo_ppo_mlp_rollout_desc;
long long myo_ppo_mlp_rollout_workspace_bytes(int obs_dim, int act_dim, int hidden);
int myo_ppo_mlp_rollout_refresh(const myo_ppo_mlp_rollout_desc* d, void* stream);
int myo_ppo_mlp_rollout_act(const myo_ppo_mlp_rollout_desc* d, int activation, void* stream);      /* hidden activation MYO_ACT_* */
int myo_ppo_mlp_rollout(const myo_ppo_mlp_rollout_desc* d, void* stream);                           /* ... with MYO_ACT_RELU */

/* clip_grad_norm_(max_norm) followed by one torch.optim.Adam step over a flat fp32 parameter vector
 * (what RecurrentPPO.train does per minibatch; /root/reference/src/train/trainer.py:66-71, SB3 Adam
 * eps 1e-5).  g is multiplied by grad_scale first (1/world after an all-reduce SUM).  step: dev
 * int32[2], zero-initialised ([1] = number of steps taken); scratch: dev float[max(64, nparts)] (partial sums
 * of g^2, added in a fixed order: deterministic).  The descriptor is read at call time; its values go to the kernels by value.
 *   nparts   0: the squares of g are taken here (64 per-block sums -> scratch) and `step` advances.  > 0: |g|^2 = the sum of
 *            scratch[0 .. nparts), left there by myo_ppo_mlp_step with sqnorm_part set, which has also advanced `step`.
 *   p_bf16   NULL, or a bfloat16 copy of p, rewritten with the new parameters in the same pass (the operand the bf16 GEMMs read).
 *   hp       NULL, or the hyper-parameter block: lr is hp[MYO_HP_LR] (`lr` is ignored); with the stop flag up p, m, v, p_bf16,
 *            the images and `step` stay untouched; otherwise hp[MYO_HP_APPLIED] advances by one.
 *   images   NULL, or the descriptor of a fused MLP step (its workspace, shapes and layout; images->G must be n): every parameter
 *            the step updates is also stored into that step's operand images, the weights as bf16 in the layouts of
 *            myo_ppo_mlp_images, the biases as fp32. */
typedef struct myo_adam_desc {
  float* p;
  const float* g;
  float *m, *v;
  int32_t n;
  float lr, b1, b2, eps, max_norm, grad_scale;
  int32_t* step;
  float* scratch;
  int32_t nparts;
  uint16_t* p_bf16;
  float* hp;
  const myo_ppo_mlp_desc* images;
} myo_adam_desc;
int myo_adam_step(const myo_adam_desc* a, void* stream);

/* One deterministic acting step of an ensemble of M = M0 + M1 actor-only LSTM policies (RecurrentActorCriticPolicy with
 * net_arch=[dict(pi=[], vf=[])]: LSTM -> action head) on one observation batch, in one launch: what SuperModel.predict does member by
 * member (/root/reference/src/eval_mixture_of_ensembles.py:250-285).  Member m belongs to group 0 (m < M0, "base") or 1 ("hold").
 * Per member: x = clamp((obs - mean[m]) / sqrt(var[m] + eps), +-clip) in float64 -> float32 -> bf16; gates = [x | keep h] . w_gates[m]^T
 * + b_gates[m] as ONE fp32 accumulation of bf16 operands, keep = 1 - start_g[row]; the cell of myo_lstm_step_fwd; c (float32) and
 * h (bf16) advance in place; a_m = bf16(h_new) . w_a[m]^T + b_a[m] in fp32.  act[row] = the mean of group 1's a_m where
 * use_group1[row] != 0, of group 0's elsewhere: the members summed in member order in fp32, divided by the group size, not clipped.
 * Both groups' states advance on every row.
 *   w_gates  bf16 [M, 4H, OP + H], OP = O rounded up to 32: row k of member m is [W_ih[k, :O] | zeros | W_hh[k, :]]
 *   w_a      bf16 [M, 48, H]: rows of the action head, zero rows beyond A
 *   b_gates  f32 [M, 4H] holding bf16(b_ih + b_hh);  b_a f32 [M, A]
 *   start0 / start1  f32 [N]; start1 and use_group1 (uint8 [N]) may be NULL when M1 = 0
 *   member_act  NULL, or f32 [M, N, A] <- every a_m
 * H in {128, 256}, 1 <= O <= 128, 1 <= A <= 48, any N >= 1, M0 >= 1, M1 >= 0; MYO_E_UNSUPPORTED for other H / O / A, MYO_E_ARG for
 * a NULL or non-positive argument, before any device call. */
typedef struct myo_ensemble_desc {
  int32_t N, O, A, H, M0, M1;
  const float* obs;
  const double *mean, *var;
  double eps, clip;
  const uint16_t *w_gates, *w_a;
  const float *b_gates, *b_a;
  uint16_t* h;
  float* c;
  const float *start0, *start1;
  const uint8_t* use_group1;
  float* act;
  float* member_act;
} myo_ensemble_desc;
int myo_ensemble_supported(int H, int O, int A);
int myo_ensemble_act(const myo_ensemble_desc* d, void* stream);

const char* myo_last_error(void);
const char* myo_version(void);

#ifdef __cplusplus
}
#endif
#endif
