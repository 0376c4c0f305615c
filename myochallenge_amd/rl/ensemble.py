"""One launch per env step for an ensemble of actor-only LSTM policies (csrc/myo_ensemble.h, ``myo_ensemble_act``).

The mixture of ensembles (eval_mixture_of_ensembles.py ``SuperModel``) evaluates 6 + 5 LSTM-128 policies with
``net_arch=[dict(pi=[], vf=[])]`` on every observation batch, each behind its own ``VecNormalize`` statistics.  ``FusedEnsemble``
packs their weights and statistics once, owns the LSTM states (h in bf16, c in float32, [M, N, H]) and advances all members of
both groups in one kernel: normalise, gates, cell, action head, group means, selection.  The critic halves are not evaluated.

As rl/fused_mlp.py and rl/fused_lstm.py: ``create`` returns the fused object, or ``None`` where it does not apply.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

APM = 48          # ENS_APM of csrc/myo_ensemble.h


def _member_ok(p) -> bool:
    """(gSDE members included: deterministic acting is action_net(latent), log_std is not read and repack packs action_net only)"""
    return (getattr(p, "recurrent", False) and len(p.mlp_extractor.policy_net) == 0
            and p.lstm_actor.num_layers == 1 and not p.lstm_actor.bidirectional)


def _norm_ok(n) -> bool:
    return getattr(n, "norm_obs", False) is True and hasattr(n, "obs_rms") and hasattr(n, "epsilon") and hasattr(n, "clip_obs")


class FusedEnsemble:
    @classmethod
    def create(cls, policies_base: Sequence, norms_base: Sequence, policies_hold: Sequence, norms_hold: Sequence, num_envs: int,
               device) -> Optional["FusedEnsemble"]:
        """None when the device is not a GPU, a member is not a recurrent policy with an empty actor trunk and a supported hidden
        size, the members differ in shape, or a normaliser does not normalise observations (or the normalisers differ in epsilon /
        clip, which the kernel takes once)."""
        device = torch.device(device)
        pols, norms = list(policies_base) + list(policies_hold), list(norms_base) + list(norms_hold)
        if device.type != "cuda" or not policies_base or len(pols) != len(norms) or len(policies_base) != len(norms_base) or num_envs < 1:
            return None
        if not all(_member_ok(p) for p in pols) or not all(_norm_ok(n) for n in norms):
            return None
        shape = lambda p: (p.obs_dim, p.act_dim, p.lstm_actor.hidden_size)
        if any(shape(p) != shape(pols[0]) for p in pols):
            return None
        if any(float(n.epsilon) != float(norms[0].epsilon) or float(n.clip_obs) != float(norms[0].clip_obs) for n in norms):
            return None
        O, A, H = shape(pols[0])
        if any(n.obs_rms.mean.numel() != O for n in norms):
            return None
        try:
            from .. import native
            lib = native.load()
        except Exception:
            return None
        if lib.is_emulation or not lib.L.myo_ensemble_supported(H, O, A):
            return None
        return cls(lib, pols, norms, len(policies_base), int(num_envs), device)

    def __init__(self, lib, pols, norms, m0, num_envs, device):
        self.lib, self.pols, self.norms, self.device = lib, pols, norms, device
        self.M0, self.M1, self.N = m0, len(pols) - m0, num_envs
        self.O, self.A, self.H = pols[0].obs_dim, pols[0].act_dim, pols[0].lstm_actor.hidden_size
        M, N, H = len(pols), num_envs, self.H
        self.OP = (self.O + 31) // 32 * 32
        self.w_gates = torch.zeros((M, 4 * H, self.OP + H), dtype=torch.bfloat16, device=device)
        self.w_a = torch.zeros((M, APM, H), dtype=torch.bfloat16, device=device)
        self.b_gates = torch.zeros((M, 4 * H), dtype=torch.float32, device=device)
        self.b_a = torch.zeros((M, self.A), dtype=torch.float32, device=device)
        self.mean = torch.zeros((M, self.O), dtype=torch.float64, device=device)
        self.var = torch.ones((M, self.O), dtype=torch.float64, device=device)
        self.h = torch.zeros((M, N, H), dtype=torch.bfloat16, device=device)
        self.c = torch.zeros((M, N, H), dtype=torch.float32, device=device)
        self.eps, self.clip = float(norms[0].epsilon), float(norms[0].clip_obs)
        self.repack()

    @torch.no_grad()
    def repack(self) -> None:
        """The operand images and statistics from the members as they are now (in place: a captured graph keeps reading them)."""
        O, H, A, dev = self.O, self.H, self.A, self.device
        for m, (p, n) in enumerate(zip(self.pols, self.norms)):
            la = p.lstm_actor
            self.w_gates[m, :, :O] = la.weight_ih_l0.detach().to(dev, torch.float32).to(torch.bfloat16)
            self.w_gates[m, :, self.OP:] = la.weight_hh_l0.detach().to(dev, torch.float32).to(torch.bfloat16)
            bsum = la.bias_ih_l0.detach().to(dev, torch.float32) + la.bias_hh_l0.detach().to(dev, torch.float32)
            self.b_gates[m] = bsum.to(torch.bfloat16).to(torch.float32)
            self.w_a[m, :A] = p.action_net.weight.detach().to(dev, torch.float32).to(torch.bfloat16)
            self.b_a[m] = p.action_net.bias.detach().to(dev, torch.float32)
            self.mean[m] = n.obs_rms.mean.detach().to(dev, torch.float64).reshape(-1)
            self.var[m] = n.obs_rms.var.detach().to(dev, torch.float64).reshape(-1)

    def reset_states(self) -> None:
        self.h.zero_()
        self.c.zero_()

    @torch.no_grad()
    def act(self, obs: torch.Tensor, start_base: torch.Tensor, start_hold: torch.Tensor, use_hold: torch.Tensor,
            member_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """obs [N, O]; start_base / start_hold [N] (1 = that group's LSTM states restart on this step); use_hold bool [N] ->
        actions float32 [N, A], not clipped.  member_out: None, or a float32 [M, N, A] tensor that receives every member's action."""
        N = self.N
        if obs.shape != (N, self.O):
            raise ValueError(f"FusedEnsemble.act: obs {tuple(obs.shape)}, packed for {(N, self.O)}")
        f32 = lambda t: t.to(device=self.device, dtype=torch.float32).contiguous()
        obs, s0, s1 = f32(obs), f32(start_base).reshape(N), f32(start_hold).reshape(N)
        ug = use_hold.to(device=self.device, dtype=torch.bool).reshape(N).contiguous()
        out = torch.empty((N, self.A), dtype=torch.float32, device=self.device)
        if member_out is not None and (member_out.shape != (self.M0 + self.M1, N, self.A) or member_out.dtype != torch.float32
                                       or not member_out.is_contiguous()):
            raise ValueError("FusedEnsemble.act: member_out must be a contiguous float32 [M, N, A] tensor")
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        from ..native import EnsembleDesc
        d = EnsembleDesc(N=N, O=self.O, A=self.A, H=self.H, M0=self.M0, M1=self.M1, obs=p(obs), mean=p(self.mean), var=p(self.var),
                         eps=self.eps, clip=self.clip, w_gates=p(self.w_gates), w_a=p(self.w_a), b_gates=p(self.b_gates), b_a=p(self.b_a),
                         h=p(self.h), c=p(self.c), start0=p(s0), start1=p(s1), use_group1=p(ug), act=p(out), member_act=p(member_out))
        self.lib.check(self.lib.L.myo_ensemble_act(C.byref(d), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out
