"""Plain-torch CPU reference of the ensemble acting step (csrc/myo_ensemble.h, rl/ensemble.py), rounding where the kernel rounds.

As tests/lstm_ref.py (whose helpers it uses): every function takes `dt` (float64 = the reference, float32 = its twin, the same
statement with the kernel's accumulation width) and `rnd` (round_bf16, or `identity` for the unrounded mathematics, which is what
SuperModel.predict computes member by member in float32).  Members are stacked: P = {"wih" [M, 4H, O], "whh" [M, 4H, H], "bih",
"bhh" [M, 4H], "wa" [M, A, H], "ba" [M, A] (float32), "mean", "var" [M, O] (float64), "eps", "clip", "M0"}; members [0, M0) are
group 0 (base), the rest group 1 (hold).  Gates in the order i, f, g, o.

Rounding points, read off the kernel:

* x = clamp((obs - mean_m) / sqrt(var_m + eps), +-clip) in float64 whatever `dt` (VecNormalize.normalize_obs and the kernel both do),
  -> float32 -> bf16;
* W_ih, W_hh, W_a -> bf16; the summed gate bias b_ih + b_hh (a float32 add) -> bf16; b_a as stored (float32);
* keep = 1 - start_g[row]; h enters as bf16 values, keep h -> bf16 (exact for starts of 0 and 1);
* pre = x . W_ih^T + (keep h) . W_hh^T + bsum: one accumulation, NOT rounded (it never leaves the chip);
* i, f, o = 1 / (1 + e^-pre), g = tanh(pre), c_new = f (keep c) + i g: c is carried unrounded (float32 in the kernel and the twin,
  float64 in the reference);
* h_new = o tanh(c_new) -> bf16 ONCE: the carried state and the head's operand;
* a_m = h_new . W_a^T + b_a, accumulated unrounded;
* group action = ((a_0 + a_1) + ...) / M_g in member order; output = group 1's where use_group1[row], group 0's elsewhere.
"""
import types

import torch

from lstm_ref import _act, _tanh
from mlp_ref import identity, round_bf16  # noqa: F401  (re-exported for the tests)


def make_norm(mean, var, n_envs=1, act_dim=1, device="cpu", epsilon=1e-8, clip_obs=10.0):
    """A VecNormalize (the project's own class: its normalize_obs is what the members see) holding the given statistics."""
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    venv = types.SimpleNamespace(num_envs=n_envs, device=torch.device(device), obs_dim=int(mean.numel()), act_dim=act_dim,
                                 observation_space=None, action_space=None)
    vn = VecNormalize(venv, training=False, norm_reward=False, clip_obs=clip_obs, epsilon=epsilon)
    vn.obs_rms.mean.copy_(mean.to(torch.float64))
    vn.obs_rms.var.copy_(var.to(torch.float64))
    return vn


def pack_members(pols, norms, m0):
    cp = lambda t: t.detach().float().cpu().clone()
    st = lambda f: torch.stack([cp(f(p)) for p in pols])
    return {"wih": st(lambda p: p.lstm_actor.weight_ih_l0), "whh": st(lambda p: p.lstm_actor.weight_hh_l0),
            "bih": st(lambda p: p.lstm_actor.bias_ih_l0), "bhh": st(lambda p: p.lstm_actor.bias_hh_l0),
            "wa": st(lambda p: p.action_net.weight), "ba": st(lambda p: p.action_net.bias),
            "mean": torch.stack([n.obs_rms.mean.detach().double().cpu().reshape(-1) for n in norms]),
            "var": torch.stack([n.obs_rms.var.detach().double().cpu().reshape(-1) for n in norms]),
            "eps": float(norms[0].epsilon), "clip": float(norms[0].clip_obs), "M0": int(m0)}


def normalize_ref(P, obs, dt=torch.float64, rnd=round_bf16):
    """[M, N, O]: every member's normalised observation as the gates' operand."""
    x = (obs.double()[None] - P["mean"][:, None]) / torch.sqrt(P["var"][:, None] + P["eps"])
    return rnd(torch.clamp(x, -P["clip"], P["clip"]).float()).to(dt)


def _keep(P, start0, start1, dt):
    M, M0 = P["wih"].shape[0], P["M0"]
    s1 = start0 if start1 is None else start1
    return torch.stack([1.0 - (start0 if m < M0 else s1).to(dt) for m in range(M)])[:, :, None]      # [M, N, 1]


def head_ref(P, h_new, dt=torch.float64, rnd=round_bf16):
    """Every member's action from the given h_new [M, N, H] (bf16 values where rnd rounds)."""
    return torch.bmm(h_new.to(dt), rnd(P["wa"]).to(dt).transpose(1, 2)) + P["ba"].to(dt)[:, None]


def group_select(P, member_act, use1):
    """The ensemble action of the member actions [M, N, A], in their dtype: members summed in member order, / M_g, selected."""
    M, M0 = member_act.shape[0], P["M0"]

    def mean(lo, hi):
        s = member_act[lo].clone()
        for m in range(lo + 1, hi):
            s = s + member_act[m]
        return s / (hi - lo)
    a0 = mean(0, M0)
    if M == M0:
        return a0
    return torch.where(use1.bool()[:, None], mean(M0, M), a0)


def ensemble_step_ref(P, obs, h, c, start0, start1, use1, dt=torch.float64, rnd=round_bf16, act="step"):
    """One step from h (bf16 values where rnd rounds) and c [M, N, H].  Returns x, pre, c_new (unrounded, dt), h_new (rounded),
    member_act [M, N, A] and act [N, A]."""
    H = P["whh"].shape[2]
    k = _keep(P, start0, start1, dt)
    x = normalize_ref(P, obs, dt, rnd)
    bsum = rnd(P["bih"] + P["bhh"]).to(dt)
    hk = rnd(h.to(dt) * k)
    pre = torch.bmm(x, rnd(P["wih"]).to(dt).transpose(1, 2)) + torch.bmm(hk, rnd(P["whh"]).to(dt).transpose(1, 2)) + bsum[:, None]
    i, f, g, o = _act(pre, H, act)
    c_new = f * (c.to(dt) * k) + i * g
    h_new = rnd(o * _tanh(c_new, act))
    ma = head_ref(P, h_new, dt, rnd)
    return {"x": x, "pre": pre, "c_new": c_new, "h_new": h_new, "member_act": ma, "act": group_select(P, ma, use1)}


def ensemble_chain_ref(P, obs_seq, start0_seq, start1_seq, use1_seq, h0, c0, dt=torch.float64, rnd=round_bf16, act="step"):
    """T steps; the *_seq arguments are indexed by step.  Returns the actions [T, N, A] and the final h, c."""
    h, c, acts = h0.to(dt), c0.to(dt), []
    for t in range(len(obs_seq)):
        s = ensemble_step_ref(P, obs_seq[t], h, c, start0_seq[t], None if start1_seq is None else start1_seq[t],
                              None if use1_seq is None else use1_seq[t], dt, rnd, act)
        h, c = s["h_new"], s["c_new"]
        acts.append(s["act"])
    return torch.stack(acts), h, c
