"""tests/mlp_ref.py with the hidden activation as an argument: the plain-torch CPU reference of the fused PPO MLP kernels
(csrc/myo_ppo_mlp.h) for MYO_ACT_RELU and MYO_ACT_TANH, and of the two pointwise kernels (k_bias_act, k_act_bwd_colsum).

Rounding points are mlp_ref's.  What the activation changes, read off the kernels:

* hidden layer: (GEMM + bias) -> activation -> bf16.  tanh is the kernels' ONE formula, 1 - 2 / (e^2x + 1) (myo_act_tanh, which
  clamps x to +-10 first: no change to any bf16 result), evaluated in the working dtype `dt` — as lstm_ref._tanh states the
  sequence kernels' — so that float64 is the reference of THAT statement and float32 its twin.  The kernels themselves evaluate
  the formula in double from their fp32 sums; activation="tanh64" states that (sums in `dt`, tanh in float64, one rounding to
  bf16 from the double): with dt = float32 it is the twin that MIRRORS the kernels, and its distance from the reference is
  smaller than the plain twin's, which also counts the roundings a float32 tanh flips;
* d hidden: GEMM -> bf16 -> times the derivative from the STORED bf16 activation h.  ReLU: the mask (h != 0), nothing rounds
  again.  tanh: (1 - h * h), and the product is rounded to bf16 once (mlp_store_grad_tanh) — what autograd under bf16 autocast does.

With activation="relu" every function here returns mlp_ref's result bit for bit (the CPU tests assert it).
"""
import torch

from mlp_ref import HALF_LOG_2PI, gaussian_logp, policy_params, round_bf16  # noqa: F401  (re-exported: one import for the tests)

ACTIVATIONS = ("relu", "tanh")          # (and "tanh64": tanh evaluated in float64 whatever the working dtype)


def act_fwd(x, activation):
    """activation(x) in x's dtype, unrounded."""
    if activation == "relu":
        return torch.relu(x)
    assert activation in ("tanh", "tanh64"), activation
    if activation == "tanh64":
        x = x.double()
    return 1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0)


def act_bwd(g, h, activation, rnd):
    """g (bf16 values) times the derivative taken from the layer's rounded output h."""
    if activation == "relu":
        return g * (h != 0).to(g.dtype)
    assert activation in ("tanh", "tanh64"), activation
    return rnd(g * (1.0 - h * h))


def _forward(net, x, dt, rnd, activation):
    W1, b1, W2, b2, Wh, bh = (t.to(dt) for t in net)
    h1 = rnd(act_fwd(x @ rnd(W1).t() + b1, activation)).to(dt)
    h2 = rnd(act_fwd(h1 @ rnd(W2).t() + b2, activation)).to(dt)
    return h1, h2, h2 @ rnd(Wh).t() + bh


def _backward(net, x, h1, h2, d_out, dt, rnd, activation):
    """Gradients of one net from the bf16 d(head output) [B, Ah]: (gW1, gb1, gW2, gb2, gWh) and the hidden gradients."""
    _, _, W2, _, Wh, _ = (t.to(dt) for t in net)
    gWh = d_out.t() @ h2
    dh2 = act_bwd(rnd(d_out @ rnd(Wh)), h2, activation, rnd)
    gW2, gb2 = dh2.t() @ h1, dh2.sum(0)
    dh1 = act_bwd(rnd(dh2 @ rnd(W2)), h1, activation, rnd)
    gW1, gb1 = dh1.t() @ x, dh1.sum(0)
    return (gW1, gb1, gW2, gb2, gWh), (dh1, dh2)


def ppo_mlp_step_ref(params, obs, act, oldlp, adv, ret, idx, clip, vf_coef, ent_coef, compute_adv_stats=True,
                     adv_stats=(0.0, 1.0), dt=torch.float64, rnd=round_bf16, activation="relu"):
    """mlp_ref.ppo_mlp_step_ref for hidden activation `activation`: same arguments, same result dict."""
    idx = idx.long().cpu()
    B = idx.numel()
    x = rnd(obs[idx].to(dt))
    a, olp, ad, rt = act[idx].to(dt), oldlp[idx].to(dt), adv[idx].to(dt), ret[idx].to(dt)
    ls = params["log_std"].to(dt)
    if compute_adv_stats:
        stats = (ad.mean(), ad.std())
    else:
        stats = (torch.as_tensor(adv_stats[0], dtype=dt), torch.as_tensor(adv_stats[1], dtype=dt))
    # ---- actor
    h1p, h2p, mean = _forward(params["pi"], x, dt, rnd, activation)
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
    gpi, hid_pi = _backward(params["pi"], x, h1p, h2p, rnd(dm), dt, rnd, activation)
    # ---- critic
    h1v, h2v, val = _forward(params["vf"], x, dt, rnd, activation)
    dv = val[:, 0] - rt
    vl = (dv * dv).sum() / B
    dvi = (vf_coef * 2.0 / B) * dv
    gvf, hid_vf = _backward(params["vf"], x, h1v, h2v, rnd(dvi)[:, None], dt, rnd, activation)
    acc = torch.cat([dls.sum(0), pl[None], vl[None], dm.sum(0), dvi.sum()[None]])
    clipped_rows = int(((ratio - 1.0).abs() > clip).sum())
    return {
        "grads": {"pi": gpi + (dm.sum(0),), "vf": gvf + (dvi.sum()[None],), "log_std": dls.sum(0) - ent_coef},
        "acc": acc, "adv_stats": torch.stack(list(stats)), "pl": pl, "vl": vl,
        "approx_kl": ((ratio - 1.0) - lr).sum() / B, "clip_frac": torch.as_tensor(clipped_rows / B, dtype=dt),
        "ent_loss": -(ls + 0.5 + HALF_LOG_2PI).sum(), "clipped_rows": clipped_rows,
        "ratio": ratio, "adv_norm": an, "hidden": {"pi": (h1p, h2p) + hid_pi, "vf": (h1v, h2v) + hid_vf},
    }


def ppo_mlp_rollout_ref(params, obs, dt=torch.float64, rnd=round_bf16, activation="relu"):
    """Head mean [N, A] and value [N] of the rows of `obs` (k_mlp_policy's forward)."""
    x = rnd(obs.to(dt))
    return _forward(params["pi"], x, dt, rnd, activation)[2], _forward(params["vf"], x, dt, rnd, activation)[2][:, 0]


# ---- the pointwise kernels (the GEMM-per-layer path and the recurrent step's trunks): inputs are bf16 VALUES held in `dt`
def bias_act_ref(h, bias, activation, dt=torch.float64, rnd=round_bf16):
    """myo_bias_act_bf16: bf16(activation(h + bias)), h [G, R, C], bias [G, C] — one rounding."""
    return rnd(act_fwd(h.to(dt) + bias.to(dt)[:, None, :], activation))


def act_bwd_ref(dy, out, activation, dt=torch.float64, rnd=round_bf16):
    """myo_act_bwd_colsum_bf16's in-place half: the masked (ReLU: `out > 0`) or scaled and once-rounded (tanh) gradient [rows, C]."""
    dy, out = dy.to(dt), out.to(dt)
    if activation == "relu":
        return dy * (out > 0).to(dt)
    return act_bwd(dy, out, activation, rnd)
