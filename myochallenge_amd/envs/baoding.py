"""GPU-resident batched Baoding environment with the stable-baselines3 ``VecEnv`` surface.

Replaces the reference's ``SubprocVecEnv([thunk]*16)`` of ``Monitor(TimeLimit(CustomBaoding*Env))``
(/root/reference/src/main_baoding.py:56-65; env classes /root/reference/src/envs/baoding.py:15-647)
with ONE object whose ``num_envs`` environments live in HBM and step in one kernel launch.

Two call styles:

* SB3 protocol (numpy in / numpy out, host ``infos`` list with ``terminal_observation``,
  ``TimeLimit.truncated``, ``episode`` and the reward components) — what SB3's algorithms,
  ``VecNormalize`` and the reference's callbacks (src/metrics/custom_callbacks.py:34,60,75) expect;
* tensor-native fast path ``step_tensor`` / ``reset_tensor``: device ``torch.Tensor`` in and
  out, no host synchronisation — what this repo's PPO engine uses.
"""
from __future__ import annotations

from dataclasses import dataclass
import time
from typing import Any, List, Optional, Sequence

import numpy as np

from .. import native
from ..model import CompiledModel, apply_muscle_condition, compile_model
from .config import check_muscle_condition, make_task_cfg, resolve_kwargs


@dataclass
class Box:
    """Stand-in for gym.spaces.Box (gym is not a dependency)."""
    low: np.ndarray
    high: np.ndarray
    shape: tuple
    dtype: Any = np.float32

    @classmethod
    def uniform(cls, lo, hi, n):
        return cls(np.full(n, lo, np.float32), np.full(n, hi, np.float32), (n,), np.float32)

    def sample(self, rng=np.random):
        return rng.uniform(self.low, self.high).astype(self.dtype)


class BaodingVecEnv:
    """``num_envs`` Baoding environments on one GPU (``device`` index)."""

    metadata = {"render.modes": ["rgb_array"]}

    def __init__(self, env_name: str, num_envs: int, config: Optional[dict] = None, *, device: int = 0,
                 seed: int = 0, dtype: str = "mixed", model=None, integrator: Optional[str] = None,
                 lib: Optional[native.NativeLib] = None, unsupported_contacts: str = "error"):
        import torch
        config = dict(config or {})
        self.env_name = env_name
        self.config = config
        self.params = self._resolve(env_name, config)
        self.muscle_condition = check_muscle_condition(self.params.get("muscle_condition"))
        if model is None:
            model = self._default_model()
        if self.muscle_condition == "sarcopenia":       # a model edit (the other conditions are lowered into the task cfg)
            if isinstance(model, CompiledModel):
                raise ValueError(f"{env_name}: muscle_condition='sarcopenia' edits the model and model= is already compiled: apply the "
                                 "condition before compiling (model.apply_muscle_condition), then pass the result without the kwarg")
            model = apply_muscle_condition(model, "sarcopenia")
        if not isinstance(model, CompiledModel):
            integ = None if integrator is None else {"euler": 0, "rk4": 1}[integrator.lower()]
            model = self._compile(model, integ, unsupported_contacts)
            if model.dropped_pairs:            # an explicit opt-in ("drop"): say what the physics now lacks
                import warnings
                warnings.warn(f"{env_name}: {len(model.dropped_pairs)} colliding geom pair(s) have no narrow phase and were dropped: "
                              f"{model.dropped_pairs[:8]}{' ...' if len(model.dropped_pairs) > 8 else ''}")
        self.compiled = model
        self.lib = lib or native.load()
        self.torch = torch
        self.device = self._select_device(device)
        self._model = native.Model(model, self.lib)
        self._cfg = self._make_cfg(env_name, model, config)
        self.max_episode_steps = int(self._cfg.max_episode_steps)
        self.dtype = {"mixed": native.MYO_MIXED, "f32": native.MYO_MIXED, "f64": native.MYO_F64}[dtype]      # "f32": round 1's name of the mixed stepper
        self.batch = native.Batch(self._model, self._cfg, num_envs, device, seed, self.dtype)
        self.num_envs = num_envs
        self.obs_dim = self.batch.obs_dim
        self.act_dim = self._model.size("nu")
        self.observation_space = Box.uniform(-10.0, 10.0, self.obs_dim)   # SB3 zip `data` [ART]
        self.action_space = Box.uniform(-1.0, 1.0, self.act_dim)
        n, o, d = num_envs, self.obs_dim, self.device
        self._obs = torch.zeros((n, o), dtype=torch.float32, device=d)
        self._rew = torch.zeros(n, dtype=torch.float32, device=d)
        self._done = torch.zeros(n, dtype=torch.uint8, device=d)
        self._trunc = torch.zeros(n, dtype=torch.uint8, device=d)
        self._term = torch.zeros((n, o), dtype=torch.float32, device=d)
        self._comps = torch.zeros((n, native.N_RWD), dtype=torch.float32, device=d)
        self._ep = torch.zeros((n, 2), dtype=torch.float32, device=d)
        self._pending = None
        self._closed = False
        self._t_start = time.time()

    def _select_device(self, device: int):
        """The torch device the batch lives on: a GPU, always (libmyobatch has no CPU execution path)."""
        if not self.torch.cuda.is_available():
            raise native.MyoError("BaodingVecEnv needs a GPU: libmyobatch has no CPU execution path")
        return self.torch.device(f"cuda:{device}")

    # ---------------------------------------------------------------- what a task supplies (ReorientVecEnv overrides these)
    rwd_keys = native.RWD_KEYS

    @staticmethod
    def _resolve(env_name, config):
        return resolve_kwargs(env_name, **config)

    @staticmethod
    def _default_model():
        from ..synth_hand import synthetic_hand
        return synthetic_hand()

    @staticmethod
    def _compile(model, integ, unsupported_contacts="error"):
        return compile_model(model, integrator=integ, unsupported_contacts=unsupported_contacts)

    @staticmethod
    def _make_cfg(env_name, compiled, config):
        return make_task_cfg(env_name, compiled, **config)

    # ---------------------------------------------------------------- tensor-native fast path
    def _stream(self):
        if self.device.type != "cuda":
            return None
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def reset_tensor(self):
        self.batch.reset(None, self._obs, self._stream())
        return self._obs

    def step_tensor(self, actions):
        """actions: float32 device tensor [N, 39].  Returns views of internal buffers
        (obs, rew, done, trunc, term_obs, comps, ep_info) — valid until the next call."""
        t = self.torch
        if actions.dtype != t.float32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=t.float32).contiguous()
        if tuple(actions.shape) != (self.num_envs, self.act_dim):
            raise ValueError(f"actions must have shape {(self.num_envs, self.act_dim)}")
        self.batch.step(actions, self._obs, self._rew, self._done, self._trunc, self._term, self._comps,
                        self._ep, self._stream())
        return self._obs, self._rew, self._done, self._trunc, self._term, self._comps, self._ep

    @property
    def rwd_dict(self):
        """The reward dictionary of the last step as device tensors [N] (what the reference's envs put into `info`)."""
        return {k: self._comps[:, j] for j, k in enumerate(self.rwd_keys)}

    # ---------------------------------------------------------------- SB3 VecEnv protocol
    def reset(self) -> np.ndarray:
        return self.reset_tensor().cpu().numpy().copy()

    def step_async(self, actions) -> None:
        self._pending = self.torch.as_tensor(np.asarray(actions, np.float32), device=self.device)

    def step_wait(self):
        obs, rew, done, trunc, term, comps, ep = self.step_tensor(self._pending)
        self._pending = None
        obs_h, rew_h = obs.cpu().numpy().copy(), rew.cpu().numpy().copy()
        done_h, trunc_h = done.cpu().numpy().astype(bool), trunc.cpu().numpy().astype(bool)
        comps_h = comps.cpu().numpy()
        infos: List[dict] = []
        term_h = ep_h = None
        if done_h.any():
            term_h, ep_h = term.cpu().numpy(), ep.cpu().numpy()
        for i in range(self.num_envs):
            rwd = {k: float(comps_h[i, j]) for j, k in enumerate(self.rwd_keys)}
            info = {"rwd_dense": rwd["dense"], "rwd_sparse": rwd["sparse"], "solved": bool(rwd["solved"]),
                    "done": bool(rwd["done"]), "rwd_dict": rwd}
            if done_h[i]:
                info["terminal_observation"] = term_h[i].copy()
                info["TimeLimit.truncated"] = bool(trunc_h[i])
                info["episode"] = {"r": float(ep_h[i, 0]), "l": int(ep_h[i, 1]), "t": round(time.time() - self._t_start, 6)}   # Monitor's keys
            infos.append(info)
        return obs_h, rew_h, done_h, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self) -> None:
        if not self._closed:
            self.batch.close()
            self._closed = True

    def seed(self, seed: Optional[int] = None):
        return [seed] * self.num_envs

    def get_attr(self, attr_name: str, indices: Optional[Sequence[int]] = None):
        idx = range(self.num_envs) if indices is None else indices
        if attr_name == "which_task":
            t = self.torch.zeros((self.num_envs, 2), dtype=self.torch.int32, device=self.device)
            self.batch.get_task(t, None, None, self._stream())
            w = t[:, 0].cpu().numpy()
            return [int(w[i]) for i in idx]
        if attr_name == "muscle_fatigue":              # MyoSuite's env.muscle_fatigue.MF
            v = self.fatigue_state()["MF"].cpu().numpy()
            return [v[i].copy() for i in idx]
        if attr_name in self._SENSOR_ATTRS:
            v = self.sensors([self._SENSOR_ATTRS[attr_name]])[self._SENSOR_ATTRS[attr_name]].cpu().numpy()
            return [v[i].copy() for i in idx]
        if attr_name in native.DATA_KEYS:              # MuJoCo's sim.data.<name> (names sensors() serves keep that route, above)
            v = self.data([attr_name])[attr_name].cpu().numpy()
            return [v[i].copy() for i in idx]
        if attr_name in ("actuator_gain", "actuator_bias"):      # the actuation stage's two curves at the present state (static_optimization)
            key = attr_name[len("actuator_"):]
            v = self.static_optimization(keys=[key])[key].cpu().numpy()
            return [v[i].copy() for i in idx]
        if attr_name in self.params:
            return [self.params[attr_name] for _ in idx]
        raise AttributeError(attr_name)

    # ---------------------------------------------------------------- muscle fatigue (include/myobatch.h myo_batch_fatigue)
    def _fatigue_block(self):
        if self.muscle_condition != "fatigue":
            raise native.MyoError(f"{self.env_name}: made without muscle_condition='fatigue': there is no fatigue state")
        return self.torch.zeros((self.num_envs, 3, self.act_dim), dtype=self.torch.float64, device=self.device)

    def fatigue_state(self) -> dict:
        """The 3CC-r state of every muscle: device tensors ``MA``, ``MR``, ``MF`` (active, resting, fatigued fraction), float64
        [N, nu] each; ``ctrl`` of the last step was ``MA``.  Needs ``muscle_condition="fatigue"``."""
        blk = self._fatigue_block()
        self.batch.fatigue(None, blk, self._stream())
        return {"MA": blk[:, 0], "MR": blk[:, 1], "MF": blk[:, 2]}

    def set_fatigue_state(self, MA, MR, MF) -> None:
        """Overwrite the fatigue state of every env ([N, nu] each, or [nu] for all envs): e.g. start an evaluation fatigued."""
        t, blk = self.torch, self._fatigue_block()
        for k, v in enumerate((MA, MR, MF)):
            blk[:, k] = t.as_tensor(v, dtype=t.float64, device=self.device)
        self.batch.fatigue(blk, None, self._stream())
        if self.device.type == "cuda":
            t.cuda.synchronize(self.device)       # (the block is a temporary: the copy must have read it)

    def set_attr(self, attr_name: str, value, indices=None) -> None:
        raise AttributeError("task parameters are fixed at construction; build a new BaodingVecEnv")

    def env_method(self, method_name: str, *args, indices=None, **kwargs):
        raise AttributeError(method_name)

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * self.num_envs

    # ---------------------------------------------------------------- rendering (include/myobatch.h myo_batch_render)
    def default_camera(self) -> dict:
        """MuJoCo's free camera defaults for this model: lookat = stat.center, distance = 1.5 stat.extent (a model without stat, such as
        the synthetic hands: the bounding sphere of the drawn geoms at qpos0), azimuth 90, elevation -45, fovy 45 [3P-RECALL]."""
        return self._model.default_camera()

    def render_tensor(self, indices=None, width: int = 480, height: int = 480, camera=None, rgb: bool = True, depth: bool = False,
                      segmentation: bool = False, show_sites: bool = False, tendons: bool = False, contacts: bool = False,
                      contact_style=None):
        """Draw the present state of envs ``indices`` (default: all) on the GPU; device tensors, no host copy.

        camera: None (the default camera), a dict of MuJoCo free-camera keys (lookat, distance, azimuth, elevation, fovy; missing
        keys take the defaults) for every env, or a list of such dicts, one per env.  Returns a dict with the requested outputs:
        ``rgb`` uint8 [k, H, W, 3] (row 0 at the top), ``depth`` float32 [k, H, W] (along the camera axis, inf for the background),
        ``segmentation`` int32 [k, H, W] (geom id, ngeom + site id, ngeom + nsite + tendon id, ngeom + nsite + ntendon + contact
        slot, -1 for the background).
        ``tendons``: also draw the spatial tendons (``tendon_paths``), coloured by muscle activation — this library's own colour
        rule, not MuJoCo's (include/myobatch.h).
        ``contacts``: also draw every contact's point (a disc) and force (a shaft of ``metres_per_newton`` metres per newton, no
        arrow head) — ``contact_items``; MuJoCo's mjVIS_CONTACTPOINT / mjVIS_CONTACTFORCE under this library's own sizes and
        colours.  ``contact_style``: a dict of style fields (disc_radius, disc_half_height, force_radius, metres_per_newton,
        point_rgba, force_rgba, geom_alpha) set on the batch before the call; they stay set.  ``geom_alpha`` < 1 makes the geoms
        translucent in renders with ``contacts`` (a disc sits between two touching surfaces and is hidden otherwise).

        Differences from MuJoCo's renderer: primitives ray-cast under a headlight (no model lights, shadows or textures; tendon
        arcs around wrap geoms are drawn as chords); model cameras are not available; sites other than the task's targets are drawn only with ``show_sites`` (the synthetic hand
        has 215 tendon path sites).  Models without visual data (the synthetic ones) get derived colours (include/myobatch.h)."""
        t = self.torch
        idx = list(range(self.num_envs)) if indices is None else [int(i) for i in indices]
        if not idx or min(idx) < 0 or max(idx) >= self.num_envs:
            raise ValueError(f"render indices must be in [0, {self.num_envs})")
        base = self.default_camera()
        cams = camera if isinstance(camera, (list, tuple)) else [camera]
        cams = [dict(base, **(c or {})) for c in cams]
        if len(cams) not in (1, len(idx)):
            raise ValueError("camera: one dict for all envs or one per env")
        k = len(idx)
        flags = (native.RENDER_RGB if rgb else 0) | (native.RENDER_DEPTH if depth else 0) | (native.RENDER_SEG if segmentation else 0)
        flags |= native.RENDER_SITES if show_sites else 0
        flags |= native.RENDER_TENDONS if tendons else 0
        flags |= native.RENDER_CONTACTS if contacts else 0
        if contact_style:
            self.batch.set_render_style(**contact_style)
        out = {}
        if rgb:
            out["rgb"] = t.empty((k, height, width, 3), dtype=t.uint8, device=self.device)
        if depth:
            out["depth"] = t.empty((k, height, width), dtype=t.float32, device=self.device)
        if segmentation:
            out["segmentation"] = t.empty((k, height, width), dtype=t.int32, device=self.device)
        env_idx = t.tensor(idx, dtype=t.int32, device=self.device)
        self.batch.render(env_idx, cams, width, height, flags, out.get("rgb"), out.get("depth"), out.get("segmentation"), self._stream())
        return out

    def tendon_paths(self, indices=None):
        """The tendon path items of envs ``indices`` (default: all): a device tensor float64 [k, ntendon_item, 24], one capsule item
        per straight piece of every spatial tendon (midpoint, rotation with z along the piece, radius and half length, rgba blended
        by muscle activation, tendon id + 1 in [22], the piece's share of the tendon's length in [23]; unused slots are zero rows:
        include/myobatch.h myo_batch_tendon_paths)."""
        t = self.torch
        idx = list(range(self.num_envs)) if indices is None else [int(i) for i in indices]
        if not idx or min(idx) < 0 or max(idx) >= self.num_envs:
            raise ValueError(f"tendon_paths indices must be in [0, {self.num_envs})")
        out = t.zeros((len(idx), self._model.size("ntendon_item"), native.RENDER_ITEM_N), dtype=t.float64, device=self.device)
        if out.numel():
            self.batch.tendon_paths(t.tensor(idx, dtype=t.int32, device=self.device), out, self._stream())
        return out

    def contact_items(self, indices=None):
        """The contact items of envs ``indices`` (default: all): a device tensor float64 [k, 2 * contact_capacity, 24].  Contact slot c
        (the order of ``sensors()``'s contact list) owns row 2c, the contact point (a disc at ``pos`` with its axis along the
        normal, slot + 1 in [22], ``dist`` in [23]), and row 2c + 1, the force on geom2's body (a capsule from ``pos`` to ``pos`` +
        metres_per_newton * F, slot + 1 in [22], |F| in newtons in [23]; a zero row for a contact without force).  Rows of unused
        slots are zero (include/myobatch.h myo_batch_contact_items)."""
        t = self.torch
        idx = list(range(self.num_envs)) if indices is None else [int(i) for i in indices]
        if not idx or min(idx) < 0 or max(idx) >= self.num_envs:
            raise ValueError(f"contact_items indices must be in [0, {self.num_envs})")
        out = t.zeros((len(idx), 2 * self.batch.contact_capacity, native.RENDER_ITEM_N), dtype=t.float64, device=self.device)
        self.batch.contact_items(t.tensor(idx, dtype=t.int32, device=self.device), out, self._stream())
        return out

    def get_images(self, width: int = 480, height: int = 480, camera=None, tendons: bool = False, contacts: bool = False,
                   contact_style=None) -> List[np.ndarray]:
        """SB3 VecEnv.get_images: one [H, W, 3] uint8 array per env."""
        rgb = self.render_tensor(None, width, height, camera, tendons=tendons, contacts=contacts, contact_style=contact_style)["rgb"].cpu().numpy()
        return [rgb[i] for i in range(self.num_envs)]

    def render(self, mode: str = "rgb_array", tendons: bool = False, contacts: bool = False, contact_style=None, **kwargs):
        """SB3 VecEnv.render: "rgb_array" returns the envs' images tiled into one grid (stable_baselines3 tile_images)."""
        if mode in ("human", "window"):
            raise NotImplementedError(f"render mode {mode!r} needs a display; this GPU library renders offscreen only: use 'rgb_array'")
        if mode != "rgb_array":
            raise ValueError(f"unknown render mode {mode!r}; supported: {self.metadata['render.modes']}")
        from ..render_io import tile_images
        return tile_images(self.get_images(tendons=tendons, contacts=contacts, contact_style=contact_style, **kwargs))

    # ---------------------------------------------------------------- contact and muscle read-out (include/myobatch.h myo_batch_sense)
    # get_attr names (MuJoCo's mjData names and the short ones) -> sensors() keys
    _SENSOR_ATTRS = {"contact_forces": "con_d", "contact_geoms": "con_geom", "ncon": "ncon", "cfrc_ext": "body_wrench",
                     "qfrc_constraint": "qfrc_constraint", "actuator_length": "act_length",
                     "actuator_velocity": "act_velocity", "actuator_force": "act_force", "activation": "activation",
                     "ten_length": "ten_length", "ten_velocity": "ten_velocity"}

    def sensors(self, keys=None, indices=None) -> dict:
        """What the hand does to the objects and what the muscles do, for the envs' PRESENT states: one forward pass on the GPU
        (contacts, constraint solve from the env's warm start), nothing about the envs changes.  Device tensors, no host copy.

        keys (default: all): ``ncon`` int32 [k]; ``con_geom`` int32 [k, cap, 2] (geom ids, -1 in unused slots; ``geom_names``);
        ``con_d`` float64 [k, cap, 13] = dist, pos[3], normal[3] (world, geom1 -> geom2), force[6] in the contact frame
        (mj_contactForce); ``body_wrench`` float64 [k, nbody, 6] net contact force and torque about xpos, world frame
        (``body_names``); ``qfrc_constraint`` [k, nv]; ``act_length`` / ``act_velocity`` / ``act_force`` [k, nu]; ``activation``
        [k, na]; ``ten_length`` / ``ten_velocity`` [k, ntendon].  indices: the envs' rows to return (default: all; the pass itself
        always runs the whole batch)."""
        t = self.torch
        shapes = self.batch.sense_shapes()
        keys = list(shapes) if keys is None else list(keys)
        for k in keys:
            if k not in shapes:
                raise KeyError(f"unknown sensor key {k!r}; known: {sorted(shapes)}")
        tdt = {np.int32: t.int32, np.float64: t.float64}
        out = {k: t.zeros((self.num_envs,) + shapes[k][0], dtype=tdt[shapes[k][1]], device=self.device) for k in keys}
        self.batch.sense(self._stream(), **out)
        if indices is not None:
            idx = t.as_tensor([int(i) for i in indices], dtype=t.long, device=self.device)
            out = {k: v[idx] for k, v in out.items()}
        return out

    # ---------------------------------------------------------------- kinematics and dynamics read-out (include/myobatch.h myo_batch_data)
    def data(self, keys=None, indices=None, ctrl=None) -> dict:
        """MuJoCo's ``sim.data`` by name for the envs' PRESENT states: one forward pass on the GPU that ends after the last stage
        the asked keys need, nothing about the envs changes.  Device tensors (float64, world frame), no host copy.

        keys (default: all).  Position stage: ``xpos`` / ``xipos`` / ``subtree_com`` [k, nbody, 3], ``xquat`` [k, nbody, 4] (w, x, y,
        z), ``xmat`` [k, nbody, 9], ``geom_xpos`` / ``geom_xmat`` [k, ngeom, 3 / 9], ``site_xpos`` [k, nsite, 3] (``site_names``),
        ``ten_J`` [k, ntendon, nv], ``actuator_moment`` [k, nu, nv].  Inertia: ``qM`` [k, nv, nv] (dense).  Velocity: ``cvel``
        [k, nbody, 6] (rotation, translation), ``qfrc_bias`` / ``qfrc_passive`` [k, nv].  Actuation: ``qfrc_actuator`` [k, nv],
        ``act_dot`` [k, na].  Acceleration: ``qacc_smooth`` [k, nv]; ``qacc`` [k, nv] — the only key that runs collision and the
        constraint solver.  indices: the envs' rows to return (default: all; the pass itself always runs the whole batch).
        ctrl: [N, nu] tensor or array (default 0): enters ``act_dot`` and the forces of actuators without an activation state."""
        t = self.torch
        shapes = self.batch.data_shapes()
        keys = list(shapes) if keys is None else list(keys)
        for k in keys:
            if k not in shapes:
                raise KeyError(f"unknown data key {k!r}; known: {sorted(shapes)}")
        out = {k: t.zeros((self.num_envs,) + shapes[k], dtype=t.float64, device=self.device) for k in keys}
        if ctrl is not None:
            ctrl = t.as_tensor(ctrl, dtype=t.float64, device=self.device).contiguous()
            if tuple(ctrl.shape) != (self.num_envs, self.act_dim):
                raise ValueError(f"ctrl must have shape {(self.num_envs, self.act_dim)}")
        self.batch.data(self._stream(), ctrl, **out)
        if ctrl is not None and self.device.type == "cuda":
            t.cuda.synchronize(self.device)       # (ctrl may be a temporary: the pass must have read it)
        if indices is not None:
            idx = t.as_tensor([int(i) for i in indices], dtype=t.long, device=self.device)
            out = {k: v[idx] for k, v in out.items()}
        return out

    # ---------------------------------------------------------------- Jacobians and inverse dynamics (include/myobatch.h myo_batch_jac, myo_batch_inverse)
    def _jac_ids(self, kind, objects):
        """int ids of `objects` (names or ids; None: every object of the kind) among the kind's objects"""
        names = {"site": self.site_names(), "geom": self.geom_names}.get(kind, self.body_names)
        count = self._model.size({"site": "nsite", "geom": "ngeom"}.get(kind, "nbody"))
        if objects is None:
            return list(range(count))
        ids = []
        for o in ([objects] if isinstance(objects, (str, int, np.integer)) else objects):
            if isinstance(o, str):
                if not o or o not in names:
                    raise KeyError(f"unknown {kind} name {o!r}")
                o = names.index(o)
            if not 0 <= int(o) < count:
                raise KeyError(f"{kind} id {int(o)} outside [0, {count})")
            ids.append(int(o))
        return ids

    def jac(self, kind, objects=None, points=None, indices=None, jacr=True) -> dict:
        """MuJoCo's ``mj_jacBody`` / ``mj_jacBodyCom`` / ``mj_jacSite`` / ``mj_jacGeom`` / ``mj_jacSubtreeCom`` / ``mj_jac`` for the
        envs' PRESENT states: one position pass on the GPU, nothing about the envs changes.  Device tensors (float64), no host copy.

        kind: ``"body"`` (point: ``xpos``), ``"bodycom"`` (``xipos``), ``"site"`` (``site_xpos``), ``"geom"`` (``geom_xpos``) or
        ``"subtreecom"`` (``subtree_com``; ``jacp`` only).  objects: names or ids (``body_names`` / ``site_names()`` /
        ``geom_names``; default: every object of the kind, in id order); they may repeat.  points: [N, k, 3] world points taken as
        rigidly attached to the bodies (``"body"`` only).  Returns ``jacp`` [k_env, k, 3, nv] with ``jacp @ qvel`` the point's
        world-frame linear velocity and — ``jacr=True``, not for ``"subtreecom"`` — ``jacr`` with ``jacr @ qvel`` the body's angular
        velocity; columns of dofs that do not move the object are 0.  indices: the envs' rows to return (default: all; the pass
        itself always runs the whole batch)."""
        t = self.torch
        if kind not in native.JAC_KINDS:
            raise KeyError(f"unknown Jacobian kind {kind!r}; known: {sorted(native.JAC_KINDS)}")
        ids = self._jac_ids(kind, objects)
        n, k, nv = self.num_envs, len(ids), self._model.size("nv")
        if points is not None:
            if kind != "body":
                raise ValueError("points go with kind 'body' only")
            points = t.as_tensor(points, dtype=t.float64, device=self.device).contiguous()
            if tuple(points.shape) != (n, k, 3):
                raise ValueError(f"points must have shape {(n, k, 3)}")
        ids_t = t.as_tensor(ids, dtype=t.int32, device=self.device)
        out = {"jacp": t.empty((n, k, 3, nv), dtype=t.float64, device=self.device)}
        if jacr and kind != "subtreecom":
            out["jacr"] = t.empty((n, k, 3, nv), dtype=t.float64, device=self.device)
        self.batch.jac(kind, ids_t, out["jacp"], out.get("jacr"), points, self._stream())
        if self.device.type == "cuda":
            t.cuda.synchronize(self.device)       # (ids and points may be temporaries: the pass must have read them)
        if indices is not None:
            idx = t.as_tensor([int(i) for i in indices], dtype=t.long, device=self.device)
            out = {key: v[idx] for key, v in out.items()}
        return out

    def inverse(self, qacc, indices=None) -> dict:
        """MuJoCo's ``mj_inverse`` for the envs' PRESENT states: ``qfrc_inverse`` [k_env, nv], the generalised force that produces
        the acceleration ``qacc`` ([N, nv] tensor or array) with the state's constraints (limits, friction loss, contacts), and the
        ``qfrc_constraint`` [k_env, nv] it was computed with.  One pass on the GPU without a constraint solve, nothing about the
        envs changes; device tensors (float64), no host copy.  indices: the envs' rows to return (default: all)."""
        t = self.torch
        n, nv = self.num_envs, self._model.size("nv")
        qacc = t.as_tensor(qacc, dtype=t.float64, device=self.device).contiguous()
        if tuple(qacc.shape) != (n, nv):
            raise ValueError(f"qacc must have shape {(n, nv)}")
        out = {k: t.empty((n, nv), dtype=t.float64, device=self.device) for k in ("qfrc_inverse", "qfrc_constraint")}
        self.batch.inverse(qacc, out["qfrc_inverse"], out["qfrc_constraint"], self._stream())
        if self.device.type == "cuda":
            t.cuda.synchronize(self.device)       # (qacc may be a temporary: the pass must have read it)
        if indices is not None:
            idx = t.as_tensor([int(i) for i in indices], dtype=t.long, device=self.device)
            out = {k: v[idx] for k, v in out.items()}
        return out

    # ---------------------------------------------------------------- static optimisation (include/myobatch.h myo_batch_static_opt)
    def static_optimization(self, qfrc=None, qacc=None, weight=None, reg=1e-6, u_ref=None, lower=None, upper=None, max_iter=100,
                            indices=None, keys=None) -> dict:
        """The muscle activations that deliver a generalised force at the envs' PRESENT states — the step after inverse dynamics:
        per env, minimise ``1/2 sum_d w_d (R' (gain u + bias) - qfrc)_d^2 + 1/2 reg |u - u_ref|^2`` over ``lower <= u <= upper``
        (``R`` = ``data()``'s ``actuator_moment``; the actuation stage is affine in ``u``, a muscle's activation or another
        actuator's ctrl).  One pass on the GPU (projected Newton, float64 whatever the batch's dtype, deterministic), nothing about
        the envs changes; device tensors, no host copy.

        qfrc: [N, nv] target; ``None``: ``inverse(qacc)["qfrc_inverse"]`` with ``qacc`` [N, nv] (``None``: zeros — the activations
        that hold the present state still).  weight: [nv] or [N, nv], >= 0 (default: 1 on the dofs some actuator reaches, 0 on the
        others, e.g. a free object's).  u_ref: [N, nu] (default 0; the previous solution gives temporal smoothing).  lower / upper:
        [N, nu] (default: [0, 1] for muscles, ctrlrange for other limited actuators, else unbounded; a force limit tightens the box
        to where its clamp is inactive).  Returns (``keys``, default all) ``u`` / ``force`` / ``gain`` / ``bias`` [k_env, nu],
        ``qfrc`` (achieved) / ``residual`` (achieved - target) [k_env, nv], ``kkt`` [k_env], ``iters`` / ``status`` [k_env] int32
        (0: converged; bit 0: iteration cap; bit 2: a variable pinned by an empty interval).  indices: the envs' rows to return
        (default: all; the pass itself always runs the whole batch)."""
        t = self.torch
        n, nv, nu = self.num_envs, self._model.size("nv"), self.act_dim
        shapes = self.batch.static_opt_shapes()
        keys = list(shapes) if keys is None else list(keys)
        for k in keys:
            if k not in shapes:
                raise KeyError(f"unknown static-optimisation key {k!r}; known: {sorted(shapes)}")

        def arr(x, name, shape_ok):
            if x is None:
                return None
            x = t.as_tensor(x, dtype=t.float64, device=self.device).contiguous()
            if tuple(x.shape) not in shape_ok:
                raise ValueError(f"{name} must have shape {' or '.join(str(s) for s in shape_ok)}")
            return x
        if qfrc is not None and qacc is not None:
            raise ValueError("give qfrc or qacc, not both")
        solve = any(k not in ("gain", "bias") for k in keys)
        if qfrc is None and solve:
            qacc = t.zeros((n, nv), dtype=t.float64, device=self.device) if qacc is None else arr(qacc, "qacc", [(n, nv)])
            qfrc = self.inverse(qacc)["qfrc_inverse"]
        qfrc = arr(qfrc, "qfrc", [(n, nv)])
        weight = arr(weight, "weight", [(nv,), (n, nv)])
        on_host = lambda x: not (isinstance(x, t.Tensor) and x.device.type != "cpu")
        check_box = lower is not None and upper is not None and on_host(lower) and on_host(upper)
        u_ref, lower, upper = arr(u_ref, "u_ref", [(n, nu)]), arr(lower, "lower", [(n, nu)]), arr(upper, "upper", [(n, nu)])
        if check_box and bool((lower > upper).any()):      # (host-visible arrays only: no device read-back; the kernel pins such a variable at lower and says so)
            raise ValueError("lower > upper")
        tdt = {np.int32: t.int32, np.float64: t.float64}
        out = {k: t.empty((n,) + shapes[k][0], dtype=tdt[shapes[k][1]], device=self.device) for k in keys}
        self.batch.static_opt(qfrc, weight, weight is not None and weight.dim() == 2, float(reg), u_ref, lower, upper, int(max_iter),
                              self._stream(), **out)
        if self.device.type == "cuda":
            t.cuda.synchronize(self.device)       # (the inputs may be temporaries: the pass must have read them)
        if indices is not None:
            idx = t.as_tensor([int(i) for i in indices], dtype=t.long, device=self.device)
            out = {k: v[idx] for k, v in out.items()}
        return out

    # ---------------------------------------------------------------- inverse kinematics (include/myobatch.h myo_batch_ik)
    def _ik_active(self, joints):
        """dof mask of `joints` (names or ids of hinge / slide joints); None: 0, the library's default (every hinge / slide dof)"""
        if joints is None:
            return 0
        f = self.compiled.fields
        jtype, dofadr = np.asarray(f["jnt_type"]), np.asarray(f["jnt_dofadr"])
        names = list(self.compiled.names.get("jnt", []))
        mask = 0
        for j in ([joints] if isinstance(joints, (str, int, np.integer)) else joints):
            if isinstance(j, str):
                if not j or j not in names:
                    raise KeyError(f"unknown joint name {j!r}")
                j = names.index(j)
            if not 0 <= int(j) < len(jtype):
                raise KeyError(f"joint id {int(j)} outside [0, {len(jtype)})")
            if int(jtype[int(j)]) not in (2, 3):
                raise ValueError(f"joint {int(j)} is neither a hinge nor a slide joint: inverse kinematics does not move it")
            mask |= 1 << int(dofadr[int(j)])
        if mask == 0:
            raise ValueError("joints is empty")
        return mask

    def inverse_kinematics(self, sites, targets, weight=None, q_init=None, q_ref=None, lower=None, upper=None, joints=None, reg=1e-6,
                           tol=1e-10, max_iter=50, indices=None, keys=None) -> dict:
        """The joint pose that puts sites on world targets — the step before inverse dynamics: per env, minimise
        ``1/2 sum_o w_o |site_xpos_o(q) - t_o|^2 + 1/2 reg |q - q_ref|^2`` over ``lower <= q <= upper`` for the hinge and slide joints
        (or ``joints``); every other qpos entry keeps its start value.  One pass on the GPU (projected Levenberg-Marquardt, float64
        whatever the batch's dtype, deterministic), nothing about the envs changes — apply the result with ``set_state`` if wanted;
        device tensors, no host copy.

        sites: names or ids (``site_names()``), at most ``native.IK_K_MAX``.  targets: [N, k, 3].  weight: [k] or [N, k], >= 0
        (default 1).  q_init: [N, nq] start point (default: the envs' present qpos).  q_ref: [N, nq] (default: the start point).
        lower / upper: [N, nv], by dof (default: jnt_range of limited joints, else unbounded).  joints: names or ids of the hinge /
        slide joints to move (default: all of them).  Returns (``keys``, default all) ``qpos`` [k_env, nq], ``site_xpos`` /
        ``residual`` (position - target) [k_env, k, 3], ``cost`` / ``kkt`` [k_env], ``iters`` / ``status`` [k_env] int32 (0: converged;
        ``native.IK_CAP``: max_iter; ``native.IK_STALL``: no acceptable step; ``native.IK_PINNED``: a joint with lower > upper).
        indices: the envs' rows to return (default: all; the pass itself always runs the whole batch)."""
        t = self.torch
        ids = self._jac_ids("site", [] if sites is None else sites)
        n, k, nv, nq = self.num_envs, len(ids), self._model.size("nv"), self._model.size("nq")
        if k > native.IK_K_MAX:
            raise ValueError(f"at most {native.IK_K_MAX} sites per call, got {k}")
        shapes = self.batch.ik_shapes(k)
        keys = list(shapes) if keys is None else list(keys)
        for key in keys:
            if key not in shapes:
                raise KeyError(f"unknown inverse-kinematics key {key!r}; known: {sorted(shapes)}")

        def arr(x, name, shape_ok):
            if x is None:
                return None
            x = t.as_tensor(x, dtype=t.float64, device=self.device).contiguous()
            if tuple(x.shape) not in shape_ok:
                raise ValueError(f"{name} must have shape {' or '.join(str(s) for s in shape_ok)}")
            return x
        active = self._ik_active(joints)
        targets = arr(targets, "targets", [(n, k, 3)])
        if targets is None:
            raise ValueError(f"targets must have shape {(n, k, 3)}")
        weight = arr(weight, "weight", [(k,), (n, k)])
        on_host = lambda x: not (isinstance(x, t.Tensor) and x.device.type != "cpu")
        check_box = lower is not None and upper is not None and on_host(lower) and on_host(upper)
        q_init, q_ref = arr(q_init, "q_init", [(n, nq)]), arr(q_ref, "q_ref", [(n, nq)])
        lower, upper = arr(lower, "lower", [(n, nv)]), arr(upper, "upper", [(n, nv)])
        if check_box and bool((lower > upper).any()):      # (host-visible arrays only, as static_optimization: the kernel pins such a joint at lower and says so)
            raise ValueError("lower > upper")
        tdt = {np.int32: t.int32, np.float64: t.float64}
        out = {key: t.empty((n,) + shapes[key][0], dtype=tdt[shapes[key][1]], device=self.device) for key in keys}
        ids_t = t.as_tensor(ids, dtype=t.int32, device=self.device)
        self.batch.ik(ids_t, targets, weight, weight is not None and weight.dim() == 2, q_init, q_ref,
                      lower, upper, active, float(reg), float(tol), int(max_iter), self._stream(), **out)
        if self.device.type == "cuda":
            t.cuda.synchronize(self.device)       # (the inputs may be temporaries: the pass must have read them)
        if indices is not None:
            idx = t.as_tensor([int(i) for i in indices], dtype=t.long, device=self.device)
            out = {key: v[idx] for key, v in out.items()}
        return out

    # ---------------------------------------------------------------- open-loop simulation (include/myobatch.h myo_batch_simulate)
    def simulate(self, ctrl, samples=None, nsub=None, every=1, qpos=None, qvel=None, act=None, sites=None, indices=None, keys=None) -> dict:
        """What happens from the envs' PRESENT states (or from given start states) under given muscle controls: ``samples`` control
        sequences per env, rolled out for T control steps in ONE launch on copies of the envs' records - nothing about the envs
        changes.  The primitive of sampling-based control (MPPI, predictive sampling), of tracking controllers and of
        ``linearize``; device tensors (float64), no host copy.

        ctrl: [k, T, nu] shared by an env's samples, or [k, S, T, nu] per sample - the actuators' ``ctrl`` as ``data(ctrl=...)`` takes
        it: no action map, no fatigue advance, no task layer, no reset.  samples: S (default: ctrl's, else 1).  nsub: substeps per
        control step (default: the task's frame_skip).  every: record every ``every``-th control step (T % every == 0; R = T / every
        rows).  qpos / qvel / act: [k, S, nq / nv / na] start states (default: the env's own).  sites: names or ids
        (``site_names()``, at most ``native.SIM_NS_MAX``) whose world positions are recorded.  indices: the envs to simulate, in this
        order; they may repeat (default: all, k = N).  Returns (``keys``, default all) ``qpos`` [k, S, R, nq], ``qvel``, ``act``,
        ``time`` [k, S, R], ``site_xpos`` [k, S, R, ns, 3] (with sites), ``bad`` / ``steps`` [k, S] int32: a sample whose state
        blows up stops with bad = 1, steps = the control steps it completed, and NaN in the rows it did not reach."""
        t = self.torch
        n, m = self.num_envs, self._model
        nq, nv, na, nu = m.size("nq"), m.size("nv"), m.size("na"), self.act_dim
        if indices is None:
            idx, k = None, n
        else:
            idx = [int(i) for i in indices]
            for i in idx:
                if not 0 <= i < n:
                    raise IndexError(f"env index {i} outside [0, {n})")
            k = len(idx)
        ids = [] if sites is None else self._jac_ids("site", sites)
        if len(ids) > native.SIM_NS_MAX:
            raise ValueError(f"at most {native.SIM_NS_MAX} sites per call, got {len(ids)}")
        ctrl = t.as_tensor(ctrl, dtype=t.float64, device=self.device).contiguous()
        if ctrl.dim() not in (3, 4) or ctrl.shape[0] != k or ctrl.shape[-1] != nu:
            raise ValueError(f"ctrl must have shape ({k}, T, {nu}) or ({k}, S, T, {nu})")
        per_sample = ctrl.dim() == 4
        S = int(ctrl.shape[1]) if per_sample else (1 if samples is None else int(samples))
        if samples is not None and int(samples) != S:
            raise ValueError(f"samples = {int(samples)} but ctrl holds {S} sequences per env")
        T, every = int(ctrl.shape[-2]), int(every)
        if S < 1 or T < 1:
            raise ValueError("samples and the number of control steps must be >= 1")
        if every < 1 or T % every:
            raise ValueError(f"every must be >= 1 and divide the number of control steps, got T = {T}, every = {every}")
        if nsub is not None and int(nsub) < 1:
            raise ValueError("nsub must be >= 1")

        def start(x, name, w):
            if x is None:
                return None
            x = t.as_tensor(x, dtype=t.float64, device=self.device).contiguous()
            if tuple(x.shape) != (k, S, w):
                raise ValueError(f"{name} must have shape {(k, S, w)}")
            return x
        qpos, qvel, act = start(qpos, "qpos", nq), start(qvel, "qvel", nv), start(act, "act", na)
        shapes = self.batch.simulate_shapes(S, T // every, len(ids))
        if not ids:
            shapes.pop("site_xpos")
        keys = list(shapes) if keys is None else list(keys)
        for key in keys:
            if key not in shapes:
                raise KeyError(f"unknown simulation key {key!r}; known: {sorted(shapes)}")
        tdt = {np.int32: t.int32, np.float64: t.float64}
        out = {key: t.empty((k,) + shapes[key][0], dtype=tdt[shapes[key][1]], device=self.device) for key in keys}
        if k == 0:
            return out
        idx_t = None if idx is None else t.as_tensor(idx, dtype=t.int32, device=self.device)
        ids_t = t.as_tensor(ids, dtype=t.int32, device=self.device) if ids else None
        self.batch.simulate(k, S, T, ctrl, per_sample, idx_t, 0 if nsub is None else int(nsub), every, qpos, qvel, act, ids_t, self._stream(), **out)
        if self.device.type == "cuda" and not t.cuda.is_current_stream_capturing():
            t.cuda.synchronize(self.device)       # (the inputs may be temporaries: the launch must have read them)
        return out

    def _tangent_tables(self):
        f = self.compiled.fields
        return tuple(np.asarray(f[key]).astype(int) for key in ("jnt_type", "jnt_qposadr", "jnt_dofadr"))

    def linearize(self, ctrl=None, eps=1e-6, nsub=None, centered=True, indices=None) -> dict:
        """Finite-difference linearisation of one control step around the envs' PRESENT states - the analogue of MuJoCo's
        ``mjd_transitionFD``, layered on ``simulate`` (one launch, nothing about the envs changes).  The state is
        ``x = (qpos in tangent coordinates [nv], qvel [nv], act [na])``, ``nx = 2 nv + na``; the ``nx + nu`` perturbations of size
        ``eps`` (both signs when ``centered``) and the unperturbed step are the samples of one call.  qpos is perturbed with
        ``mathutil.integrate_pos`` (a free joint's position adds, its quaternion is rotated by the local-frame rotation vector) and
        differenced with ``mathutil.differentiate_pos``; controls are not clamped to their range.

        ctrl: [k, nu] (default zeros).  nsub: substeps of the step (default: the task's frame_skip).  Returns ``A`` [k, nx, nx] and
        ``B`` [k, nx, nu] with ``dx' ~ A dx + B du``, and ``x_next`` [k, nq + nv + na], the unperturbed next state (qpos | qvel | act)."""
        from ..mathutil import differentiate_pos, integrate_pos
        t = self.torch
        n, m = self.num_envs, self._model
        nq, nv, na, nu = m.size("nq"), m.size("nv"), m.size("na"), self.act_dim
        eps = float(eps)
        if not eps > 0:
            raise ValueError("eps must be > 0")
        idx = list(range(n)) if indices is None else [int(i) for i in indices]
        k, nx = len(idx), 2 * nv + na
        sel = t.as_tensor(idx, dtype=t.long, device=self.device)
        q0, v0, a0, _ = (x[sel] for x in self.get_state())
        u0 = t.zeros((k, nu), dtype=t.float64, device=self.device) if ctrl is None else t.as_tensor(ctrl, dtype=t.float64, device=self.device)
        if tuple(u0.shape) != (k, nu):
            raise ValueError(f"ctrl must have shape {(k, nu)}")
        P = nx + nu
        signs = (1.0, -1.0) if centered else (1.0,)
        S = 1 + len(signs) * P
        d = t.zeros((S, P), dtype=t.float64, device=self.device)      # sample 0: the unperturbed step; then +eps e_i (and -eps e_i)
        for g, sg in enumerate(signs):
            d[1 + g * P:1 + (g + 1) * P] = sg * eps * t.eye(P, dtype=t.float64, device=self.device)
        tabs = self._tangent_tables()
        dq, dv, da, du = (d[None, :, a:b] for a, b in ((0, nv), (nv, 2 * nv), (2 * nv, nx), (nx, P)))
        qs = integrate_pos(q0[:, None].expand(k, S, nq), dq.expand(k, S, nv), *tabs)
        out = self.simulate((u0[:, None] + du)[:, :, None], nsub=nsub, qpos=qs, qvel=v0[:, None] + dv, act=a0[:, None] + da if na else None,
                            indices=idx, keys=("qpos", "qvel", "act", "bad"))
        qn, vn, an = out["qpos"][:, :, 0], out["qvel"][:, :, 0], out["act"][:, :, 0]

        def diff(hi, lo, h):      # (x'[hi] - x'[lo]) / h in tangent coordinates: [k, P, nx]
            return t.cat([differentiate_pos(qn[:, hi], qn[:, lo], *tabs), vn[:, hi] - vn[:, lo], an[:, hi] - an[:, lo]], -1) / h
        plus = slice(1, 1 + P)
        J = diff(plus, slice(1 + P, 1 + 2 * P), 2 * eps) if centered else diff(plus, t.zeros(P, dtype=t.long, device=self.device), eps)
        J = J.transpose(1, 2)      # [k, nx, P]: column i = the response to perturbation i
        return {"A": J[:, :, :nx].contiguous(), "B": J[:, :, nx:].contiguous(), "x_next": t.cat([qn[:, 0], vn[:, 0], an[:, 0]], -1), "bad": out["bad"]}

    def site_names(self) -> List[str]:
        """names of the model's sites: rows of ``data()``'s ``site_xpos``"""
        return list(self.compiled.names.get("site", []))

    @property
    def geom_names(self) -> List[str]:
        return list(self.compiled.names.get("geom", []))

    @property
    def body_names(self) -> List[str]:
        return list(self.compiled.names.get("body", []))

    def object_body_ids(self) -> List[int]:
        """ids of the task's free objects (the two balls; the die; none for the pose tasks): rows of ``body_wrench``"""
        kind = int(self._cfg.kind)
        if kind in (native.TASK_BAODING_P1, native.TASK_BAODING_P2):
            return [int(self._cfg.obj1_bid), int(self._cfg.obj2_bid)]
        return [int(self._cfg.obj1_bid)] if kind == native.TASK_REORIENT else []

    def contact_table(self, i: int) -> list:
        """Env i's contacts for humans: a list of (geom1_name, geom2_name, dist, normal_force)."""
        s = self.sensors(["ncon", "con_geom", "con_d"], [i])
        n, g, d = int(s["ncon"][0]), s["con_geom"][0].cpu().numpy(), s["con_d"][0].cpu().numpy()
        names = self.geom_names
        name = lambda k: names[k] if 0 <= k < len(names) and names[k] else f"geom{k}"
        return [(name(int(g[c, 0])), name(int(g[c, 1])), float(d[c, 0]), float(d[c, 7])) for c in range(n)]

    # ---------------------------------------------------------------- state access (parity tests)
    def get_state(self):
        t = self.torch
        n, m = self.num_envs, self._model
        qp = t.zeros((n, m.size("nq")), dtype=t.float64, device=self.device)
        qv = t.zeros((n, m.size("nv")), dtype=t.float64, device=self.device)
        ac = t.zeros((n, m.size("na")), dtype=t.float64, device=self.device)
        tm = t.zeros(n, dtype=t.float64, device=self.device)
        self.batch.get_state(qp, qv, ac, tm, self._stream())
        return qp, qv, ac, tm

    def set_state(self, qpos=None, qvel=None, act=None, time=None):
        c = lambda x: None if x is None else self.torch.as_tensor(x, dtype=self.torch.float64, device=self.device).contiguous()
        args = [c(qpos), c(qvel), c(act), c(time)]
        self.batch.set_state(*args, self._stream())
        if self.device.type == "cuda":
            self.torch.cuda.synchronize(self.device)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
