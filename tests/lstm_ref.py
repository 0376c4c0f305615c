"""Plain-torch CPU reference of the LSTM kernels (csrc/myo_lstm_step.h, csrc/myo_lstm_seq.h, the cell kernels of
csrc/myobatch.hip) and of the recurrent PPO minibatch step built on them (rl/fused_lstm.py `_run_rows`), rounding where they round.

As tests/mlp_ref.py: every function takes `dt` (float64 = the reference, float32 = its twin, the same statement with the kernels'
accumulation width) and `rnd` (round_bf16, or `identity` for the unrounded mathematics that the CPU tests compare with autograd).
Arrays are [G, N, .] per step (G stacked LSTMs, N rows), gates in the order i, f, g, o.

Rounding points, read off the kernels:

one step (lstm_fwd_out / k_lstm_step_bwd; k_lstm_seq_fwd / _bwd round at the same places)
* gx, h_prev, W_hh are bf16 values; the recurrent product h_prev . W_hh^T is accumulated in fp32 and NOT rounded (it never leaves
  the chip) — except behind `torch.bmm` + myo_lstm_cell_fwd, where `gh` is a bf16 GEMM output (`gh_round=True`);
* i, f, o = sigmoid(gx + gh), g = tanh(gx + gh), c = f c_prev + i g, h = o tanh(c) in fp32, nothing rounded in between;
  the FORMULAS are the kernels' too (`act`): "step" (step and cell kernels) sigmoid = 1 / (1 + e^-x) with tanhf, "seq" (sequence
  kernels) also tanh = 1 - 2 / (e^2x + 1) — in float64 they equal torch's to 1e-16, in the float32 twin they carry the kernels'
  cancellation (an absolute 6e-8 on a small tanh, where libm keeps a relative one), which decides how often a bf16 rounding flips;
  "exact" is torch.sigmoid / torch.tanh;
* the saved gate activations ws, c_new, out_h, hm_next = h * keep, cm_next = c * keep: each rounded ONCE from the unrounded value;
* c_prev is the bf16 slot, or (c_prev32 / c0_32) the float32 state, which cm_next32 = c * keep continues unrounded;
* backward: reads the SAVED bf16 ws, c_new, c_prev (cm[t], bf16 in float32-state mode too); dh = dout + keep (dgates_next . W_hh)
  with the product unrounded (rounded to bf16 behind torch.bmm + myo_lstm_cell_bwd: `dh_round=True`);
  dc = keep dc_prev_next + dh o (1 - tanh^2 c_new); dgates and dc_prev -> bf16 (the sequence kernel keeps dc_prev in a register,
  bf16-rounded all the same).

the sequence: step t masks with keep[t + 1], the last step with 1; keep[0] is the caller's (it made hm[0] / cm[0]).

the whole step (_run_rows; trunk_heads / _merged_core of rl/fused_mlp.py)
* every parameter is read from the bf16 shadow (biases too); log_std stays float32;
* bsum = bf16(b_ih + b_hh) (a bf16 add); gx = bf16(x . W_ih^T + bsum) (one GEMM output);
* trunk layer: bf16(GEMM) -> bf16(relu(. + b)) (myo_bias_relu_bf16 rounds again); head mean / value: bf16(GEMM + b);
* Gaussian loss as myo_ppo_loss_grad (mlp_ref.py's loss phase on the bf16 mean / value; head-bias and log_std gradients are sums of
  the UNROUNDED per-row terms); gSDE loss as `_sde_loss` (float32 ATen arithmetic on the bf16 mean / value / latent);
  d mean, d value -> bf16;
* head / trunk weight gradients: `s` split-K partial products (s = 64 when B % 64 == 0, else 1), each a bf16 GEMM output, summed
  in fp32; trunk bias gradients: column sums of the masked bf16 d hidden;
* d hidden -> bf16 after every GEMM (dh "between layers"), ReLU mask by activation > 0; the gradient entering the LSTMs is bf16;
* LSTM weight gradients: per-time-step products dG_t^T . [hm_t] and dG_t^T . [x_t | 1], each a bf16 GEMM output, summed over t in
  fp32; the bias gradient is the ones column, written to both b_ih and b_hh.

`off` names rounding points to switch to the identity one at a time (ROUNDING_POINTS), which is how a deviation from the unrounded
gradient is traced to the point that carries it.
"""
import math

import torch

from mlp_ref import HALF_LOG_2PI, identity, round_bf16

ROUNDING_POINTS = ("weights", "bsum", "gx", "lstm_state", "lstm_saved", "lat", "trunk_gemm", "trunk_act", "head_out", "dhead", "dhidden",
                   "wgrad_partials", "lstm_dgates", "lstm_dc", "lstm_wgrad_partials")
SDE_EPS = 1e-6


def _sigmoid(x, act):
    return torch.sigmoid(x) if act == "exact" else 1.0 / (1.0 + torch.exp(-x))


def _tanh(x, act):
    return 1.0 - 2.0 / (torch.exp(2.0 * x) + 1.0) if act == "seq" else torch.tanh(x)


def _act(a, H, act):
    return _sigmoid(a[..., :H], act), _sigmoid(a[..., H:2 * H], act), _tanh(a[..., 2 * H:3 * H], act), _sigmoid(a[..., 3 * H:], act)


def _k(keep, dt):
    return 1.0 if keep is None else keep.to(dt).view(1, -1, 1)


def lstm_step_fwd_ref(gx, h_prev, c_prev, w_hh, keep=None, gh_round=False, dt=torch.float64, rnd=round_bf16, rnd_state=None, rnd_out=None,
                      gh=None, act="step"):
    """One forward step.  gx [G, N, 4H], h_prev / c_prev [G, N, H] (c_prev: the bf16 slot's values, or the float32 state), w_hh
    [G, 4H, H], keep [N] or None (the NULL form: mask 1); gh [G, N, 4H]: the recurrent product handed in as the cell kernel gets it
    (h_prev / w_hh are then not read).  Returns out_h, hm, cm, c_new, ws (bf16 values), cm32 (= c * keep, unrounded: what
    cm_next32 receives) and pre (the gate pre-activations)."""
    rs, ro = rnd_state or rnd, rnd_out or rnd
    H = c_prev.shape[-1]
    if gh is None:
        gh = torch.bmm(h_prev.to(dt), w_hh.to(dt).transpose(1, 2))
        if gh_round:
            gh = rnd(gh)
    gh = gh.to(dt)
    pre = gx.to(dt) + gh
    i, f, g, o = _act(pre, H, act)
    c = f * c_prev.to(dt) + i * g
    h = o * _tanh(c, act)
    k = _k(keep, dt)
    return {"out_h": ro(h), "hm": rs(h * k), "cm": rs(c * k), "cm32": c * k, "c_new": rnd(c), "ws": rnd(torch.cat([i, f, g, o], -1)), "pre": pre}


def lstm_step_bwd_ref(dout, dg_next, dcm_next, w_hh, keep, c_prev, c_new, ws, dh_round=False, dt=torch.float64, rnd=round_bf16, rnd_dc=None,
                      dhm_next=None, act="step"):
    """One backward step from the saved bf16 arrays.  dout [G, N, H] or None, dg_next [G, N, 4H] / dcm_next [G, N, H] or None (the
    last step), keep [N] or None; dhm_next [G, N, H]: the product dgates_next . W_hh handed in as the cell kernel gets it.
    Returns (dgates [G, N, 4H], dc_prev [G, N, H])."""
    H = c_new.shape[-1]
    k = _k(keep, dt)
    dh = torch.zeros_like(c_new, dtype=dt) if dout is None else dout.to(dt)
    if dhm_next is not None:
        dh = dh + k * dhm_next.to(dt)
    elif dg_next is not None:
        prod = torch.bmm(dg_next.to(dt), w_hh.to(dt))
        dh = dh + k * (rnd(prod) if dh_round else prod)
    i, f, g, o = (ws.to(dt)[..., q * H:(q + 1) * H] for q in range(4))
    tc = _tanh(c_new.to(dt), act)
    dct = dh * o * (1 - tc * tc)
    if dcm_next is not None:
        dct = k * dcm_next.to(dt) + dct
    dg = torch.cat([dct * g * i * (1 - i), dct * c_prev.to(dt) * f * (1 - f), dct * i * (1 - g * g), dh * tc * o * (1 - o)], -1)
    return rnd(dg), (rnd_dc or rnd)(dct * f)


def lstm_seq_fwd_ref(gx, h0, c0, w_hh, keep, c32=False, gh_round=False, dt=torch.float64, rnd=round_bf16, rnd_state=None, rnd_out=None,
                     act="seq"):
    """T steps.  gx [T, G, N, 4H]; h0 [G, N, H] = hm[0] (bf16 values); c0 [G, N, H] = the masked cell state entering step 0: bf16
    values, or with c32 the float32 state (cm[0] is then its rounding); keep [T, N].  Returns hm, cm [T + 1, G, N, H], c_new
    [T, G, N, H], ws [T, G, N, 4H], lat [G, T, N, H], c_last (the carried cell state after the last step) and pre."""
    rs = rnd_state or rnd
    T = gx.shape[0]
    hm, cm = [h0.to(dt)], [rs(c0.to(dt))]
    c = c0.to(dt) if c32 else cm[0]
    cn, ws, lat, pre = [], [], [], []
    for t in range(T):
        s = lstm_step_fwd_ref(gx[t], hm[t], c, w_hh, keep[t + 1] if t + 1 < T else None, gh_round, dt, rnd, rnd_state, rnd_out, act=act)
        hm.append(s["hm"]); cm.append(s["cm"]); cn.append(s["c_new"]); ws.append(s["ws"]); lat.append(s["out_h"]); pre.append(s["pre"])
        c = s["cm32"] if c32 else s["cm"]
    return {"hm": torch.stack(hm), "cm": torch.stack(cm), "c_new": torch.stack(cn), "ws": torch.stack(ws), "lat": torch.stack(lat, 1),
            "c_last": c, "pre": torch.stack(pre)}


def lstm_seq_bwd_ref(dlat, w_hh, keep, cm, c_new, ws, dh_round=False, dt=torch.float64, rnd=round_bf16, rnd_dc=None, act="seq"):
    """BPTT over the saved arrays of a forward pass.  dlat [G, T, N, H] -> dgates [T, G, N, 4H]."""
    T = c_new.shape[0]
    dG, dc = [None] * T, None
    for t in range(T - 1, -1, -1):
        last = t == T - 1
        dG[t], dc = lstm_step_bwd_ref(dlat[:, t], None if last else dG[t + 1], None if last else dc, w_hh, None if last else keep[t + 1],
                                      cm[t], c_new[t], ws[t], dh_round, dt, rnd, rnd_dc, act=act)
    return torch.stack(dG)


# ------------------------------------------------------------------------------------------------ the whole minibatch step
def recurrent_policy_params(policy):
    """Detached fp32 CPU copies of a recurrent ActorCriticPolicy, stacked (actor, critic) where the step stacks them."""
    cp = lambda t: t.detach().float().cpu().clone()
    lin = lambda seq: [m for m in seq if isinstance(m, torch.nn.Linear)]
    la, lc = policy.lstm_actor, policy.lstm_critic
    st = lambda key: torch.stack([cp(getattr(la, key)), cp(getattr(lc, key))])
    trunk = [(torch.stack([cp(a.weight), cp(b.weight)]), torch.stack([cp(a.bias), cp(b.bias)]))
             for a, b in zip(lin(policy.mlp_extractor.policy_net), lin(policy.mlp_extractor.value_net))]
    return {"wih": st("weight_ih_l0"), "whh": st("weight_hh_l0"), "bih": st("bias_ih_l0"), "bhh": st("bias_hh_l0"), "trunk": trunk,
            "pi": (cp(policy.action_net.weight), cp(policy.action_net.bias)), "vf": (cp(policy.value_net.weight), cp(policy.value_net.bias)),
            "log_std": cp(policy.log_std), "sde": bool(getattr(policy, "use_sde", False))}


def _splitk(dy, x, s, dt, r):
    """sum over s row slabs of r(dy_slab^T . x_slab): the split-K weight gradient with bf16 partial products."""
    B = dy.shape[-2]
    dy, x = dy.reshape(*dy.shape[:-2], s, B // s, dy.shape[-1]), x.reshape(*x.shape[:-2], s, B // s, x.shape[-1])
    return r(dy.transpose(-1, -2) @ x).sum(-3)


def recurrent_step_ref(P, x, act, oldlp, adv, ret, adv_stats, keep, h0, c0, clip, vf_coef, ent_coef, route="seq", c32=True,
                       dt=torch.float64, rnd=round_bf16, off=()):
    """`_run_rows` on a gathered minibatch: x [T*m, O] (bf16 values), act [T*m, A], oldlp / adv / ret [T*m] (t-major rows), adv_stats
    (mean, std), keep [T, m], h0 [2, m, H] = hm[0], c0 [2, m, H] = the masked float32 cell state entering step 0.  route: "seq" /
    "step" (the same roundings) or "cell" (GEMM + cell kernels: gh and the backward product rounded, bf16 cell state).  Returns
    pl, vl, grads {name: tensor} keyed as the policy's named_parameters, lat, dlat [2, T*m, H], dG [T, 2, m, 4H], pre, ratio, adv_norm."""
    R = lambda name: identity if name in off else rnd
    T, m = keep.shape
    B, G = T * m, 2
    H, O = P["whh"].shape[2], P["wih"].shape[2]
    A = act.shape[1]
    w = lambda t: R("weights")(t.to(dt))
    x, a, olp, ad, rt = x.to(dt), act.to(dt), oldlp.to(dt), adv.to(dt), ret.to(dt)
    wih, whh = w(P["wih"]), w(P["whh"])
    bsum = R("bsum")(w(P["bih"]) + w(P["bhh"]))
    gx = R("gx")(torch.einsum("bo,gko->gbk", x, wih) + bsum[:, None, :]).view(G, T, m, 4 * H).transpose(0, 1)      # [T, G, m, 4H]
    cell = route == "cell"
    use32 = c32 and not cell
    act_ = "seq" if route == "seq" else "step"
    f = lstm_seq_fwd_ref(gx, h0, c0 if use32 else R("lstm_state")(c0.to(dt)), whh, keep, use32, cell, dt, R("lstm_saved"), R("lstm_state"), R("lat"),
                         act_)
    lat = f["lat"].reshape(G, B, H)
    # ---- trunks and heads
    saved, h = [lat], lat
    for W, b in P["trunk"]:
        h = R("trunk_act")(torch.relu(R("trunk_gemm")(torch.bmm(h, w(W).transpose(1, 2))) + w(b)[:, None, :]))
        saved.append(h)
    (Wpi, bpi), (Wvf, bvf) = P["pi"], P["vf"]
    mean = R("head_out")(h[0] @ w(Wpi).t() + w(bpi))
    val = R("head_out")(h[1] @ w(Wvf).t() + w(bvf))[:, 0]
    ls = P["log_std"].to(dt)
    mu, sd = (torch.as_tensor(float(v), dtype=dt) for v in adv_stats)
    an = (ad - mu) / (sd + 1e-8)
    grads = {}
    if P["sde"]:
        lat2 = h[0] ** 2
        e2 = torch.exp(2.0 * ls)
        var = lat2 @ e2 + SDE_EPS
        diff = a - mean
        z2 = diff * diff
        logp = (-0.5 * z2 / var - 0.5 * torch.log(var)).sum(-1) - A * HALF_LOG_2PI
    else:
        inv = torch.exp(-ls)
        z = (a - mean) * inv
        logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
    ratio = torch.exp(logp - olp)
    s1, s2 = an * ratio, an * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    pl = -torch.minimum(s1, s2).sum() / B
    inside = (ratio > 1.0 - clip) & (ratio < 1.0 + clip)
    dlogp = -(an * ratio) * ((s1 <= s2) | inside).to(dt) / B
    if P["sde"]:
        dm = dlogp[:, None] * diff / var
        dvar = dlogp[:, None] * (0.5 * z2 / (var * var) - 0.5 / var) - (ent_coef / B) * 0.5 / var
        grads["log_std"] = 2.0 * e2 * (lat2.t() @ dvar)
    else:
        dm = dlogp[:, None] * z * inv
        grads["log_std"] = (dlogp[:, None] * (z * z - 1.0)).sum(0) - ent_coef
    dv = val - rt
    vl = (dv * dv).sum() / B
    dvi = (vf_coef * 2.0 / B) * dv
    grads["action_net.bias"], grads["value_net.bias"] = dm.sum(0), dvi.sum()[None]
    dmh, dvh = R("dhead")(dm), R("dhead")(dvi)[:, None]
    # ---- heads and trunks backward
    s = 64 if B % 64 == 0 else 1
    rp = R("wgrad_partials")
    grads["action_net.weight"], grads["value_net.weight"] = _splitk(dmh, h[0], s, dt, rp), _splitk(dvh, h[1], s, dt, rp)
    dh = R("dhidden")(torch.stack([dmh @ w(Wpi), dvh @ w(Wvf)]))
    for li in reversed(range(len(P["trunk"]))):
        W = P["trunk"][li][0]
        dh = dh * (saved[li + 1] > 0).to(dt)
        gW, gb = _splitk(dh, saved[li], s, dt, rp), dh.sum(1)
        for g_, net in enumerate(("policy_net", "value_net")):
            grads["mlp_extractor.%s.%d.weight" % (net, 2 * li)], grads["mlp_extractor.%s.%d.bias" % (net, 2 * li)] = gW[g_], gb[g_]
        dh = R("dhidden")(torch.bmm(dh, w(W)))
    dlat = dh
    # ---- BPTT and the LSTM weight gradients
    dG = lstm_seq_bwd_ref(dlat.view(G, T, m, H), whh, keep, f["cm"], f["c_new"], f["ws"], cell, dt, R("lstm_dgates"), R("lstm_dc"), act_)
    rl = R("lstm_wgrad_partials")
    dGt = dG.transpose(2, 3)                                                     # [T, G, 4H, m]
    ghh = rl(dGt @ f["hm"][:T]).sum(0)
    xe = torch.cat([x, torch.ones(B, 1, dtype=dt)], 1).view(T, 1, m, O + 1)
    gih = rl(dGt @ xe).sum(0)
    for g_, net in enumerate(("lstm_actor", "lstm_critic")):
        grads[net + ".weight_ih_l0"], grads[net + ".weight_hh_l0"] = gih[g_, :, :O], ghh[g_]
        grads[net + ".bias_ih_l0"] = grads[net + ".bias_hh_l0"] = gih[g_, :, O]
    return {"pl": pl, "vl": vl, "grads": grads, "lat": lat, "dlat": dlat, "dG": dG, "pre": f["pre"], "ratio": ratio, "adv_norm": an,
            "hm": f["hm"], "mean": mean, "value": val, "logp": logp, "latent_pi": h[0]}
