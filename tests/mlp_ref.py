"""Plain-torch CPU reference of the fused PPO MLP kernels (csrc/myo_ppo_mlp.h) that rounds where the kernels round.

`ppo_mlp_step_ref` states one `myo_ppo_mlp_step`, `ppo_mlp_rollout_ref` the deterministic part of one `myo_ppo_mlp_rollout`
(head mean and value per row).  Rounding points, read off the kernels:

* weights (k_mlp_prep) and gathered observations (k_mlp_fwdbwd's gather) -> bf16, round to nearest even;
* biases, log_std, actions, old log-probs, advantages, returns stay as given (fp32 values);
* hidden layer: (GEMM + bias) -> ReLU -> bf16 (mlp_store_act), both layers; the head output + bias stays unrounded;
* loss phase as k_mlp_fwdbwd writes it: advantage normalised by adv_stats with + 1e-8, clip derivative by `s1 <= s2` / `inside`,
  every per-row term divided by B;
* d(head) -> bf16 before it feeds d hidden 2 and the head's weight gradient; the head-bias and log_std gradients (and the
  `acc` columns) are sums of the UNROUNDED per-row values;
* d hidden 2, d hidden 1: GEMM -> bf16 -> ReLU mask (activation != 0);
* hidden bias gradients = column sums of the bf16 d hidden; weight gradients = sums of products of bf16 values.

Everything else (the sums, the loss arithmetic) is computed in `dt`: float64 is the reference, float32 its twin — the same
statement with the kernels' accumulation width, whose distance from the reference sizes the tests' tolerances.  `rnd` is the
rounding function; the identity turns the reference into the unrounded loss, which the CPU tests compare with autograd.
"""
import math

import torch

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def round_bf16(x: torch.Tensor) -> torch.Tensor:
    """x rounded to the nearest bf16 value (ties to even), returned in x's dtype.  Integer arithmetic on the bit pattern —
    mlp_f2bf's `u += 0x7fff + ((u >> 16) & 1); u >>= 16` — so it does not lean on torch's own bf16 cast, with which the CPU
    tests compare it.  float64 input is rounded ONCE, from its 52-bit mantissa (no intermediate fp32 rounding), except below
    the smallest normal fp32 / bf16 magnitude, where bf16's spacing is fp32's denormal grid and the value goes through fp32."""
    if x.dtype == torch.float32:
        u = x.contiguous().view(torch.int32)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & -65536
        return u.view(torch.float32)
    assert x.dtype == torch.float64
    u = x.contiguous().view(torch.int64)
    u = (u + ((1 << 44) - 1) + ((u >> 45) & 1)) & -(1 << 45)
    big = u.view(torch.float64)
    tiny = x.abs() < 2.0 ** -126
    return torch.where(tiny, round_bf16(x.float()).double(), big)


def identity(x: torch.Tensor) -> torch.Tensor:
    return x


def policy_params(policy):
    """{"pi": (W1, b1, W2, b2, Wh, bh), "vf": (...), "log_std"} — detached fp32 CPU copies of an MLP ActorCriticPolicy."""
    lin = lambda seq: [m for m in seq if isinstance(m, torch.nn.Linear)]
    out = {}
    for name, trunk, head in (("pi", policy.mlp_extractor.policy_net, policy.action_net),
                              ("vf", policy.mlp_extractor.value_net, policy.value_net)):
        l1, l2 = lin(trunk)
        out[name] = tuple(t.detach().float().cpu().clone() for t in (l1.weight, l1.bias, l2.weight, l2.bias, head.weight, head.bias))
    out["log_std"] = policy.log_std.detach().float().cpu().clone()
    return out


def _forward(net, x, dt, rnd):
    W1, b1, W2, b2, Wh, bh = (t.to(dt) for t in net)
    h1 = rnd(torch.relu(x @ rnd(W1).t() + b1))
    h2 = rnd(torch.relu(h1 @ rnd(W2).t() + b2))
    return h1, h2, h2 @ rnd(Wh).t() + bh


def _backward(net, x, h1, h2, d_out, dt, rnd):
    """Gradients of one net from the bf16 d(head output) [B, Ah]: (gW1, gb1, gW2, gb2, gWh) and the hidden gradients."""
    _, _, W2, _, Wh, _ = (t.to(dt) for t in net)
    gWh = d_out.t() @ h2
    dh2 = rnd(d_out @ rnd(Wh)) * (h2 != 0).to(dt)
    gW2, gb2 = dh2.t() @ h1, dh2.sum(0)
    dh1 = rnd(dh2 @ rnd(W2)) * (h1 != 0).to(dt)
    gW1, gb1 = dh1.t() @ x, dh1.sum(0)
    return (gW1, gb1, gW2, gb2, gWh), (dh1, dh2)


def ppo_mlp_step_ref(params, obs, act, oldlp, adv, ret, idx, clip, vf_coef, ent_coef, compute_adv_stats=True,
                     adv_stats=(0.0, 1.0), dt=torch.float64, rnd=round_bf16):
    """One minibatch step on rows `idx` of the rollout arrays.  Returns a dict:
    grads {"pi": (gW1, gb1, gW2, gb2, gWh, gbh), "vf": (...), "log_std"}, acc [2A+3] (the kernel's loss columns: A sums of
    d log_std terms, policy loss, value loss, A head-bias gradients, the value head's bias gradient), adv_stats (mean, unbiased
    std), pl, vl, the diagnostics approx_kl / clip_frac / ent_loss, the clip-fraction row count, and the per-row ratio and
    normalised advantage (what the tests' input conditions are stated on) plus the hidden activations and gradients."""
    idx = idx.long().cpu()
    B, A = idx.numel(), act.shape[1]
    x = rnd(obs[idx].to(dt))
    a, olp, ad, rt = act[idx].to(dt), oldlp[idx].to(dt), adv[idx].to(dt), ret[idx].to(dt)
    ls = params["log_std"].to(dt)
    if compute_adv_stats:
        stats = (ad.mean(), ad.std())               # unbiased, as k_adv_moments / k_mlp_prep (M2 / (B - 1)) and torch.std in SB3
    else:
        stats = (torch.as_tensor(adv_stats[0], dtype=dt), torch.as_tensor(adv_stats[1], dtype=dt))
    # ---- actor
    h1p, h2p, mean = _forward(params["pi"], x, dt, rnd)
    inv = torch.exp(-ls)
    z = (a - mean) * inv
    logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
    an = (ad - stats[0]) / (stats[1] + 1e-8)
    lr = logp - olp
    ratio = torch.exp(lr)
    s1 = an * ratio
    s2 = an * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    pl = -torch.minimum(s1, s2).sum() / B
    inside = (ratio > 1.0 - clip) & (ratio < 1.0 + clip)
    dlogp = -(an * ratio) * ((s1 <= s2) | inside).to(dt) / B
    dm = dlogp[:, None] * z * inv
    dls = dlogp[:, None] * (z * z - 1.0)
    gpi, hid_pi = _backward(params["pi"], x, h1p, h2p, rnd(dm), dt, rnd)
    # ---- critic
    h1v, h2v, val = _forward(params["vf"], x, dt, rnd)
    dv = val[:, 0] - rt
    vl = (dv * dv).sum() / B
    dvi = (vf_coef * 2.0 / B) * dv
    gvf, hid_vf = _backward(params["vf"], x, h1v, h2v, rnd(dvi)[:, None], dt, rnd)
    acc = torch.cat([dls.sum(0), pl[None], vl[None], dm.sum(0), dvi.sum()[None]])
    clipped_rows = int(((ratio - 1.0).abs() > clip).sum())
    return {
        "grads": {"pi": gpi + (dm.sum(0),), "vf": gvf + (dvi.sum()[None],), "log_std": dls.sum(0) - ent_coef},
        "acc": acc, "adv_stats": torch.stack(list(stats)), "pl": pl, "vl": vl,
        "approx_kl": ((ratio - 1.0) - lr).sum() / B, "clip_frac": torch.as_tensor(clipped_rows / B, dtype=dt),
        "ent_loss": -(ls + 0.5 + HALF_LOG_2PI).sum(), "clipped_rows": clipped_rows,
        "ratio": ratio, "adv_norm": an, "hidden": {"pi": (h1p, h2p) + hid_pi, "vf": (h1v, h2v) + hid_vf},
    }


def ppo_mlp_rollout_ref(params, obs, dt=torch.float64, rnd=round_bf16):
    """Head mean [N, A] and value [N] of the rows of `obs` (k_mlp_policy's forward: the forward half of the step)."""
    x = rnd(obs.to(dt))
    return _forward(params["pi"], x, dt, rnd)[2], _forward(params["vf"], x, dt, rnd)[2][:, 0]


def gaussian_logp(act, mean, log_std):
    """log N(act; mean, exp(log_std)) summed over the action dimension, in the dtype of the inputs."""
    z = (act - mean) * torch.exp(-log_std)
    return (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
