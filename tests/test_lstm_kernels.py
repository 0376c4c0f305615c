"""The LSTM kernels (csrc/myo_lstm_step.h, csrc/myo_lstm_seq.h, the cell kernels) and the recurrent PPO minibatch step
(rl/fused_lstm.py `_run_rows`) against tests/lstm_ref.py, a float64 CPU reference that rounds to bf16 where the kernels do.

Two tolerance rules, neither a literal fitted to the kernels:

R1, one step from bit-identical inputs (nothing compounds): per element |got - ref| <= ulp_bf16(max(|ref|, 2^-8 max|ref|)), and at
   most 1 element in 256 of an array may differ from the reference at all.  fp32 accumulation over K <= 1024 plus v_exp / v_rcp
   leaves ~2^-19 of the array's scale, 16 times below the floor's ulp; a flip needs that error to cross a bf16 boundary, ~2^-11 per
   O(1) element, 8 times below the cap.  (The float32 twin differs from the reference on 9e-6 .. 4e-5 of the elements.)
R2, chains (a flipped rounding propagates; single near-zero elements may be tens of ulps off): per array the relative L2 distance
   from the float64 reference is <= MARGIN = 4 times the float32 twin's, the convention of test_ppo_mlp_kernels.py.  The twin is
   evaluated on the case's rows plus 2048 more of the same kind (sequence tests: rows are independent), so that the few roundings
   it flips are counted over millions of elements; for the whole step, whose gradients are sums over the minibatch, "more rows" is
   REPLICAS more minibatches of the case's shape (root mean square of the twin's distance over them), and a tensor is bounded by
   the largest twin figure of its net (actor / critic), as in the MLP suite.

The CPU tests pin the reference: against torch.nn.LSTM and float64 autograd with the rounding switched off, and the conditions on
the inputs of every GPU case (both mask values per step, unsaturated gates, a gradient that flows, one clip branch per row).
"""
import ctypes as C
import functools
import math
import zlib

import pytest
import torch

import lstm_ref
from lstm_ref import (lstm_seq_bwd_ref, lstm_seq_fwd_ref, lstm_step_bwd_ref, lstm_step_fwd_ref, recurrent_policy_params,
                      recurrent_step_ref)
from mlp_ref import identity, round_bf16

MARGIN = 4.0
CLIP, VF_COEF, ENT_COEF = 0.2, 0.7, 0.01
RATIO_MARGIN, ADV_MARGIN = 1e-3, 1e-6
EXTRA = 2048                    # rows the twin sees besides the case's
REPLICAS = 24                   # minibatches the whole-step twin is pooled over
SENT = -12345.0
BF = torch.bfloat16
MEASURED = {}                   # name -> largest figure of this process (printed with -s; DESIGN.md quotes them)

p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None


def _note(name, v):
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(v))
    return float(v)


def bfv(x):
    """float32 tensor of bf16 values."""
    return round_bf16(x.float().contiguous())


def ulp_bf16(x):
    """Spacing of bf16 at |x| (float64, normal range)."""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -120))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 8).double())


def r1(name, got, ref, label):
    """Rule R1 on one array; prints and records the share of differing elements and the worst error in ulps."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    tol = ulp_bf16(torch.maximum(ref.abs(), ref.abs().max() * 2.0 ** -8))
    d = (got - ref).abs()
    share, worst = float((d > 0).double().mean()), float((d / tol).max())
    print("R1 %-34s %-8s share %.2e worst %.2f ulp (%d elements)" % (label, name, share, worst, d.numel()))
    _note("R1 share " + name, share); _note("R1 ulp " + name, worst)
    return [] if (worst <= 1.0 and share <= 1.0 / 256) else [(label, name, share, worst)]


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


def r2(name, got, ref, twin, label):
    """Rule R2 on one array: `twin` is the twin's relative L2 distance (a number)."""
    k = rel(got, ref)
    ratio = k / twin if twin > 0 else (0.0 if k == 0 else float("inf"))
    print("R2 %-34s %-10s kernel %.3e twin %.3e ratio %.2f" % (label, name, k, twin, ratio))
    _note("R2 " + name, ratio)
    return [] if k <= MARGIN * twin else [(label, name, k, twin, ratio)]


# ------------------------------------------------------------------------------------------------ inputs (CPU, shared)
def _seed_of(*key):
    return zlib.crc32(repr(key).encode()) % (2 ** 30)


def _gen(*key):
    return torch.Generator().manual_seed(_seed_of(*key))


def _keep_rows(N):
    """Mask over rows with both values wherever N > 1 (row 0 masked, so N = 1 exercises the mask too)."""
    return (torch.arange(N) % 3 != 0).float()


@functools.lru_cache(maxsize=None)
def step_case(H, N, G):
    g = _gen("step", H, N, G)
    rn = lambda *s, sc=1.0: bfv(sc * torch.randn(*s, generator=g))
    c = {"gx": rn(G, N, 4 * H), "hp": rn(G, N, H, sc=0.5), "cp": rn(G, N, H, sc=0.5), "whh": rn(G, 4 * H, H, sc=H ** -0.5), "keep": _keep_rows(N),
         "dout": rn(G, N, H, sc=0.5), "dgn": rn(G, N, 4 * H, sc=0.3), "dcn": rn(G, N, H)}
    c["cp32"] = (c["cp"] + 1e-3 * torch.randn(G, N, H, generator=g)).contiguous()          # not representable in bf16
    c["fwd"] = lstm_step_fwd_ref(c["gx"], c["hp"], c["cp"], c["whh"], c["keep"])
    return c


FWD_CASES = [(H, N, 2) for H in (32, 64, 128, 256) for N in (1, 17, 65)] + [(H, 17, G) for H in (32, 64, 128, 256) for G in (1, 3)]
BWD_CASES = [(H, N, 2) for H in (32, 64, 128, 256) for N in (1, 33)] + [(H, 33, G) for H in (32, 64, 128, 256) for G in (1, 3)]
_sid = lambda c: "H%d-N%d-G%d" % c

# (H, rs, N, T, G, flag): all five instantiations x one / three workgroups x T = 1 (backward: `last` only), 2, 5; G = 1 and 3;
# "restart": every row restarts at one step; "strided": gx / out_h / dout inside wider sentinel-filled buffers
SEQ_CASES = [(H, rs, N, T, 2, "") for H, rs in ((128, 1), (128, 2), (256, 1), (256, 2), (256, 4)) for N in (16, 48) for T in (1, 2, 5)]
SEQ_CASES += [(128, 1, 16, 2, 1, ""), (128, 2, 16, 2, 3, ""), (256, 1, 16, 2, 3, ""), (256, 2, 16, 2, 1, ""), (256, 4, 16, 2, 3, ""),
              (128, 2, 48, 5, 2, "restart"), (256, 4, 48, 5, 2, "restart"), (128, 1, 48, 5, 2, "strided"), (256, 2, 48, 5, 2, "strided"),
              (256, 4, 16, 2, 2, "strided")]
_qid = lambda c: "H%d-rs%d-N%d-T%d-G%d%s" % (c[0], c[1], c[2], c[3], c[4], "-" + c[5] if c[5] else "")
CHAIN_CASES = [(32, 33, 5, 2), (64, 17, 5, 2)]            # (H, N, T, G): the step kernels' T-launch chain where no sequence kernel exists


def _act_of(H):
    """The activation formulas of the kernels that run hidden size H in the chain tests: sequence kernels from 128 on."""
    return "seq" if H >= 128 else "step"


@functools.lru_cache(maxsize=None)
def seq_family(H, T, G, restart):
    """Inputs of every sequence case with this (H, T, G): 48 + EXTRA rows, a case takes the first N (rows never interact).  keep has
    both values among the first 16 rows of every step (but the deliberate all-restart step)."""
    NB = 48 + EXTRA
    g = _gen("seq", H, T, G, restart)
    rn = lambda *s, sc=1.0: bfv(sc * torch.randn(*s, generator=g))
    keep = (torch.rand(T, NB, generator=g) > 0.25).float()
    keep[:, 0:NB:16], keep[:, 1:NB:16] = 0.0, 1.0
    if restart:
        keep[2] = 0.0
    c = {"gx": rn(T, G, NB, 4 * H), "whh": rn(G, 4 * H, H, sc=H ** -0.5), "keep": keep, "dlat": rn(G, T, NB, H, sc=0.5)}
    k0 = keep[0].view(1, NB, 1)
    c["h0"] = rn(G, NB, H, sc=0.5) * k0
    c["c0"] = rn(G, NB, H, sc=0.5) * k0
    c["c0f"] = ((c["c0"] + 1e-3 * torch.randn(G, NB, H, generator=g)) * k0).contiguous()
    return c


@functools.lru_cache(maxsize=None)
def seq_refs(H, T, G, restart, dt):
    """The reference (or twin) on all rows of the family: bf16-c forward, float32-c forward, backward from the float64 reference's
    saved arrays (so that reference and twin read the SAME arrays: the backward pass alone), backward from its own forward pass."""
    c = seq_family(H, T, G, restart)
    act = _act_of(H)
    f16 = lstm_seq_fwd_ref(c["gx"], c["h0"], c["c0"], c["whh"], c["keep"], False, dt=dt, act=act)
    f32 = lstm_seq_fwd_ref(c["gx"], c["h0"], c["c0f"], c["whh"], c["keep"], True, dt=dt, act=act)
    own = lstm_seq_bwd_ref(c["dlat"], c["whh"], c["keep"], f32["cm"], f32["c_new"], f32["ws"], dt=dt, act=act)
    if dt == torch.float64:
        same = own
    else:
        r = seq_refs(H, T, G, restart, torch.float64)["f32"]
        same = lstm_seq_bwd_ref(c["dlat"], c["whh"], c["keep"], r["cm"], r["c_new"], r["ws"], dt=dt, act=act)
    return {"f16": f16, "f32": f32, "bwd_same": same, "bwd_own": own}


FWD_ARRAYS = ("lat", "hm", "cm", "c_new", "ws")


@functools.lru_cache(maxsize=None)
def seq_twin(H, T, G, restart):
    """Relative L2 distance of the twin from the reference per array, over all rows of the family."""
    a, b = seq_refs(H, T, G, restart, torch.float64), seq_refs(H, T, G, restart, torch.float32)
    out = {k: rel(b["f32"][k], a["f32"][k]) for k in FWD_ARRAYS}
    out["dG_same"], out["dG_own"] = rel(b["bwd_same"], a["bwd_same"]), rel(b["bwd_own"], a["bwd_own"])
    return out


# ---- whole step
O_DIM, A_DIM, T_STEP = 22, 6, 4
WHOLE_CASES = [(H, route, m, arch, False) for H, route in ((32, "step"), (48, "cell"), (128, "seq1"), (128, "seq2")) for m in (16, 32)
               for arch in ((), (64,))]
WHOLE_CASES.append((32, "step", 32, (64,), True))          # gSDE
_wid = lambda c: "H%d-%s-m%d-%s%s" % (c[0], c[1], c[2], "trunk" if c[3] else "bare", "-gsde" if c[4] else "")


def build_recurrent_policy(H, arch, sde, seed):
    """ActorCriticPolicy(O, A, arch, arch, lstm_hidden_size=H) with distinct random actor / critic weights and non-zero biases."""
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        pol = ActorCriticPolicy(O_DIM, A_DIM, arch, arch, lstm_hidden_size=H, use_sde=sde)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in pol.modules():
            if isinstance(mod, torch.nn.Linear):
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * mod.weight.std(unbiased=False))
        for lstm in (pol.lstm_actor, pol.lstm_critic):
            for b in (lstm.bias_ih_l0, lstm.bias_hh_l0):
                b.copy_(0.3 * torch.randn(b.shape, generator=g))
        pol.log_std.copy_(-0.5 + 0.1 * torch.randn(pol.log_std.shape, generator=g))
    return pol


def _ref_route(route):
    return "seq" if route.startswith("seq") else route


@functools.lru_cache(maxsize=None)
def whole_inputs(H, route, m, arch, sde, replica):
    """Synthetic gathered rows: bf16 observations, starts inside the sequences, a non-zero masked start state, on-policy actions, old
    log-probs off by N(0, 0.05), advantages and returns that carry signal.  Replica 0 is the GPU case."""
    seed = _seed_of("whole", H, m, arch, sde)
    P = recurrent_policy_params(build_recurrent_policy(H, arch, sde, seed))
    g = torch.Generator().manual_seed(seed + 7 + 1000 * replica)
    T, B = T_STEP, T_STEP * m
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = bfv(rn(B, O_DIM))
    keep = (torch.rand(T, m, generator=g) > 0.25).float()
    keep[:, 0], keep[:, 1] = 0.0, 1.0
    k0 = keep[0].view(1, m, 1)
    h0, c0 = bfv(0.5 * rn(2, m, H)) * k0, (0.5 * rn(2, m, H)).float() * k0
    z = torch.zeros(B)
    fwd = recurrent_step_ref(P, x, torch.zeros(B, A_DIM), z, z, z, (0.0, 1.0), keep, h0, c0, CLIP, VF_COEF, ENT_COEF, _ref_route(route))
    mean = fwd["mean"]
    if sde:
        std = torch.sqrt((fwd["latent_pi"] ** 2) @ torch.exp(2 * P["log_std"].double()) + 1e-6)
    else:
        std = torch.exp(P["log_std"].double())
    act = (mean + std * rn(B, A_DIM)).float()
    probe = recurrent_step_ref(P, x, act, z, z, z, (0.0, 1.0), keep, h0, c0, CLIP, VF_COEF, ENT_COEF, _ref_route(route))
    oldlp = (probe["logp"] + 0.05 * rn(B)).float()                              # log pi(act) of the reference, off by N(0, 0.05)
    wa, wo = rn(A_DIM), rn(O_DIM) / math.sqrt(O_DIM)
    adv = (torch.tanh(((act.double() - mean) / std) @ wa / 3) + 0.3 * rn(B)).float()
    ret = (torch.sin(x.double() @ wo) + 0.1 * rn(B)).float()
    stats = (float(adv.mean()), float(adv.std()))
    return {"P": P, "x": x, "act": act, "oldlp": oldlp, "adv": adv, "ret": ret, "stats": stats, "keep": keep, "h0": h0, "c0": c0, "seed": seed}


@functools.lru_cache(maxsize=None)
def whole_ref(H, route, m, arch, sde, replica, dt, rnd=round_bf16, off=()):
    c = whole_inputs(H, route, m, arch, sde, replica)
    return recurrent_step_ref(c["P"], c["x"], c["act"], c["oldlp"], c["adv"], c["ret"], c["stats"], c["keep"], c["h0"], c["c0"], CLIP, VF_COEF,
                              ENT_COEF, _ref_route(route), dt=dt, rnd=rnd, off=off)


def _net_of(name):
    return "vf" if ("critic" in name or "value_net" in name) else "pi"


@functools.lru_cache(maxsize=None)
def whole_twin(H, route, m, arch, sde):
    """Root mean square over REPLICAS minibatches of the twin's relative L2 distance: per gradient tensor, dG per net, the losses;
    and per net the largest figure over its gradient tensors."""
    acc = {}
    for r in range(REPLICAS):
        a, b = whole_ref(H, route, m, arch, sde, r, torch.float64), whole_ref(H, route, m, arch, sde, r, torch.float32)
        items = {n: rel(b["grads"][n], a["grads"][n]) for n in a["grads"]}
        for g_, net in enumerate(("pi", "vf")):
            items["dG." + net] = rel(b["dG"][:, g_], a["dG"][:, g_])
        items["pl"], items["vl"] = rel(b["pl"], a["pl"]), rel(b["vl"], a["vl"])
        for k, v in items.items():
            acc[k] = acc.get(k, 0.0) + v * v / REPLICAS
    out = {k: math.sqrt(v) for k, v in acc.items()}
    out["D"] = {net: max(v for k, v in out.items() if k not in ("pl", "vl") and not k.startswith("dG") and _net_of(k) == net) for net in ("pi", "vf")}
    return out


# ------------------------------------------------------------------------------------------------ CPU: the reference itself
def _nn_lstms(G, O, H, seed):
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        return [torch.nn.LSTM(O, H).double() for _ in range(G)]


def test_reference_without_rounding_is_nn_lstm_and_its_autograd():
    """rnd = identity, float64: the forward pass is torch.nn.LSTM with the state zeroed at episode starts (starts inside the
    sequence, a non-zero start state); dG[t] is autograd's d(sum(lat * dlat)) / d gx[t]; the W_ih, W_hh and bias gradients formed
    from dG as the step forms them equal autograd's.  All to 1e-10 relative.  H = 32, G = 2, N = 5, T = 4."""
    H, G, N, T, O = 32, 2, 5, 4, 7
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    lstms = _nn_lstms(G, O, H, 3)
    x, h0, c0, dlat = rn(T, N, O), 0.5 * rn(G, N, H), 0.5 * rn(G, N, H), rn(G, T, N, H)
    starts = torch.zeros(T, N, dtype=torch.float64)
    starts[0, 1] = starts[2, 0] = starts[2, 3] = starts[3, 4] = starts[1, 2] = 1.0
    keep = 1.0 - starts
    gx_leaf, lat_nn = [], []
    for gi, l in enumerate(lstms):
        gxl = (x @ l.weight_ih_l0.t() + l.bias_ih_l0 + l.bias_hh_l0).detach().requires_grad_(True)      # [T, N, 4H]
        h, c, outs = h0[gi], c0[gi], []
        for t in range(T):
            # nn.LSTM takes x, not gx: its own step on x[t] gives the forward value, the same arithmetic written out on a gx leaf
            # (asserted equal to it) gives autograd a handle on gx
            k = keep[t].view(N, 1)
            with torch.no_grad():
                o_nn, _ = l(x[t:t + 1], ((h * k).unsqueeze(0), (c * k).unsqueeze(0)))
            a = gxl[t] + (h * k) @ l.weight_hh_l0.detach().t()
            i, f, gg, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            c = f * (c * k) + i * gg
            h = o * torch.tanh(c)
            assert float((h.detach() - o_nn[0]).abs().max()) <= 1e-12
            outs.append(h)
        gx_leaf.append(gxl); lat_nn.append(torch.stack(outs))
    # autograd through nn.LSTM proper for the parameter gradients
    for l in lstms:
        l.zero_grad()
    loss = 0.0
    for gi, l in enumerate(lstms):
        h, c = h0[gi].unsqueeze(0), c0[gi].unsqueeze(0)
        for t in range(T):
            k = keep[t].view(1, N, 1)
            o_nn, (h, c) = l(x[t:t + 1], (h * k, c * k))
            loss = loss + (o_nn[0] * dlat[gi, t]).sum()
    loss.backward()
    sum(((lat_nn[gi] * dlat[gi]).sum() for gi in range(G))).backward()
    # the reference, unrounded
    whh = torch.stack([l.weight_hh_l0.detach() for l in lstms])
    gx = torch.stack([t.detach() for t in gx_leaf], 1)                               # [T, G, N, 4H]
    k0 = keep[0].view(1, N, 1)
    for c32 in (False, True):
        f = lstm_seq_fwd_ref(gx, h0 * k0, c0 * k0, whh, keep, c32, rnd=identity)
        assert rel(f["lat"], torch.stack([t.detach() for t in lat_nn])) <= 1e-10
        dG = lstm_seq_bwd_ref(dlat, whh, keep, f["cm"], f["c_new"], f["ws"], rnd=identity)
        assert rel(dG, torch.stack([t.grad for t in gx_leaf], 1)) <= 1e-10
        dGt = dG.transpose(2, 3)
        ghh = (dGt @ f["hm"][:T]).sum(0)
        gih = (dGt @ x.view(T, 1, N, O)).sum(0)
        gb = dG.sum((0, 2))
        for gi, l in enumerate(lstms):
            assert rel(ghh[gi], l.weight_hh_l0.grad) <= 1e-10 and rel(gih[gi], l.weight_ih_l0.grad) <= 1e-10
            assert rel(gb[gi], l.bias_ih_l0.grad) <= 1e-10 and rel(gb[gi], l.bias_hh_l0.grad) <= 1e-10
    # the masks matter (a reference that ignored them would pass a test without starts)
    f_nomask = lstm_seq_fwd_ref(gx, h0 * k0, c0 * k0, whh, torch.ones_like(keep), False, rnd=identity)
    assert rel(f_nomask["lat"], f["lat"]) > 1e-3


def _policy_loss_autograd(pol, c):
    """SB3's recurrent PPO minibatch loss in float64 through autograd on the policy's OWN modules (nn.LSTM with the state zeroed at
    starts as `_lstm_seq`, mlp_extractor, action_net, value_net) and `evaluate_actions`' formulas (its `.float()` casts would
    truncate float64, so the three lines after the latents are restated; the float32 evaluate_actions itself is compared below)."""
    T, m = c["keep"].shape
    pol = pol.double()
    x = c["x"].double().view(T, m, -1)
    starts = 1.0 - c["keep"].double()
    # the rows' state is already masked by keep[0]; _lstm_seq masks step 0 again with starts[0] (idempotent)
    st = tuple(t.double().unsqueeze(0) for t in (c["h0"][0], c["c0"][0], c["h0"][1], c["c0"][1]))
    lp, lv, _ = pol._latents(x, st, starts)
    mean = pol.action_net(lp).reshape(T * m, -1)
    values = pol.value_net(lv).reshape(T * m)
    a, ls = c["act"].double(), pol.log_std
    if pol.use_sde:
        lat = lp.detach().reshape(T * m, -1)
        std = torch.sqrt((lat ** 2) @ (torch.exp(ls) ** 2) + pol.SDE_EPS)
        logp = pol.log_prob(a, mean, torch.log(std))
        entropy = (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(std)).sum(-1).mean()
    else:
        logp = pol.log_prob(a, mean, ls)
        entropy = (0.5 + 0.5 * math.log(2 * math.pi) + ls).sum()
    an = (c["adv"].double() - c["stats"][0]) / (c["stats"][1] + 1e-8)
    ratio = torch.exp(logp - c["oldlp"].double())
    pl = -torch.min(an * ratio, an * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
    vl = torch.nn.functional.mse_loss(values, c["ret"].double())
    pol.zero_grad()
    (pl - ENT_COEF * entropy + VF_COEF * vl).backward()
    return pl.detach(), vl.detach(), {n: q.grad.clone() for n, q in pol.named_parameters()}, (values.detach(), logp.detach())


@pytest.mark.parametrize("arch,sde", [((), False), ((64,), False), ((), True), ((64,), True)], ids=["bare", "trunk", "bare-gsde", "trunk-gsde"])
def test_step_reference_without_rounding_is_the_policy_loss(arch, sde):
    """recurrent_step_ref(rnd = identity) against float64 autograd through the policy: losses and every parameter's gradient to
    1e-10 relative, Gaussian and gSDE — and the float64 statement used for it is the policy's own evaluate_actions (float32)."""
    H, m = 32, 16
    c = whole_inputs(H, "step", m, arch, sde, 0)
    pol = build_recurrent_policy(H, arch, sde, c["seed"])
    T = T_STEP
    with torch.no_grad():
        st = tuple(t.unsqueeze(0) for t in (c["h0"][0], c["c0"][0], c["h0"][1], c["c0"][1]))
        v32, lp32, _ = pol.evaluate_actions(c["x"].view(T, m, -1), c["act"].view(T, m, -1), st, 1.0 - c["keep"])
    pl, vl, grads, (v64, lp64) = _policy_loss_autograd(pol, c)
    assert float((v32.reshape(-1).double() - v64).abs().max()) <= 1e-4 and float((lp32.reshape(-1).double() - lp64).abs().max()) <= 1e-3 * (1 + float(lp64.abs().max()))
    res = whole_ref(H, "step", m, arch, sde, 0, torch.float64, identity)
    assert set(res["grads"]) == set(grads), set(res["grads"]) ^ set(grads)
    assert abs(float(res["pl"]) - float(pl)) <= 1e-10 * abs(float(pl)) and abs(float(res["vl"]) - float(vl)) <= 1e-10 * abs(float(vl))
    for n, gq in grads.items():
        assert res["grads"][n].shape == gq.shape and rel(res["grads"][n], gq) <= 1e-10, (n, rel(res["grads"][n], gq))
    # each named rounding point is one: switching it off alone changes the result, all of them off is the unrounded statement
    full = whole_ref(H, "step", m, arch, sde, 0, torch.float64)
    alloff = whole_ref(H, "step", m, arch, sde, 0, torch.float64, round_bf16, lstm_ref.ROUNDING_POINTS)
    assert all(torch.equal(alloff["grads"][n], res["grads"][n]) for n in grads)
    for name in lstm_ref.ROUNDING_POINTS:
        if name in ("trunk_gemm", "trunk_act") and not arch:
            continue
        one = whole_ref(H, "step", m, arch, sde, 0, torch.float64, round_bf16, (name,))
        assert any(not torch.equal(one["grads"][n], full["grads"][n]) for n in grads), name


def _saturated(pre):
    return float((pre.abs() > 8).double().mean())


@pytest.mark.parametrize("case", sorted(set(FWD_CASES + BWD_CASES)), ids=_sid)
def test_step_case_inputs(case):
    c = step_case(*case)
    N = case[1]
    assert N == 1 or (float(c["keep"].min()) == 0 and float(c["keep"].max()) == 1)
    assert _saturated(c["fwd"]["pre"]) < 0.01
    f = c["fwd"]
    dg, _ = lstm_step_bwd_ref(c["dout"], c["dgn"], c["dcn"], c["whh"], c["keep"], c["cp"], f["c_new"], f["ws"])
    assert float(dg.abs().max()) > 0.05 and float((dg != 0).double().mean()) > 0.9
    assert not torch.equal(bfv(c["cp32"]), c["cp32"])


@pytest.mark.parametrize("fam", sorted({(c[0], c[3], c[4], c[5] == "restart") for c in SEQ_CASES} | {(H, T, G, False) for H, _, T, G in CHAIN_CASES}),
                         ids=lambda f: "H%d-T%d-G%d%s" % (f[0], f[1], f[2], "-restart" if f[3] else ""))
def test_sequence_case_inputs(fam):
    """Every step of every sequence case masks some rows and keeps others among its first 16 rows (but the all-restart step), the
    gates are not saturated, and a gradient reaches every step."""
    H, T, G, restart = fam
    c = seq_family(*fam)
    for t in range(T):
        k = c["keep"][t, :16]
        if restart and t == 2:
            assert float(c["keep"][t].max()) == 0
        else:
            assert float(k.min()) == 0 and float(k.max()) == 1
    r = seq_refs(H, T, G, restart, torch.float64)
    assert _saturated(r["f16"]["pre"]) < 0.01 and _saturated(r["f32"]["pre"]) < 0.01
    for t in range(T):
        assert float(r["bwd_own"][t, :, :16].abs().max()) > 0.05
    tw = seq_twin(*fam)
    assert all(v > 0 for v in tw.values()), tw         # the twin's estimate rests on roundings it did flip


@pytest.mark.parametrize("case", WHOLE_CASES, ids=_wid)
def test_whole_step_case_inputs(case):
    """No probability ratio within 1e-3 of 1 +- clip and no normalised advantage within 1e-6 of zero (kernel and reference take the
    same clip branch on every row), both clip branches occur, both mask values at every step, unsaturated gates, dG not vanishing."""
    c, r = whole_inputs(*case, 0), whole_ref(*case, 0, torch.float64)
    ratio, an = r["ratio"], r["adv_norm"]
    edge = float(torch.minimum((ratio - (1 - CLIP)).abs(), (ratio - (1 + CLIP)).abs()).min())
    assert edge > RATIO_MARGIN and float(an.abs().min()) > ADV_MARGIN, (edge, float(an.abs().min()))
    assert all(float(c["keep"][t].min()) == 0 and float(c["keep"][t].max()) == 1 for t in range(T_STEP))
    assert _saturated(r["pre"]) < 0.01
    for g_ in range(2):
        assert float(r["dG"][:, g_].abs().max()) > 1e-5 and all(float(r["dG"][t, g_].abs().max()) > 0 for t in range(T_STEP))
    assert float(c["h0"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ GPU plumbing
DEV = "cuda:0"


def dev_bf(x):
    return x.to(DEV).to(BF).contiguous()


def _in_sentinel(shape, strides, offset, size, fill=None):
    """A sentinel-filled bf16 device buffer of `size` elements with a strided window; returns (buffer, window view, mask of the window)."""
    buf = torch.full((size,), SENT, dtype=BF, device=DEV)
    win = torch.as_strided(buf, shape, strides, offset)
    mask = torch.zeros(size, dtype=torch.bool, device=DEV)
    torch.as_strided(mask, shape, strides, offset).fill_(True)
    assert int(mask.sum()) == math.prod(shape)                   # the window does not overlap itself
    if fill is not None:
        win.copy_(fill.to(DEV))
    return buf, win, mask


def _outside_untouched(buf, mask):
    return bool((buf[~mask] == torch.tensor(SENT, dtype=BF)).all()) and int((~mask).sum()) > 0


# ------------------------------------------------------------------------------------------------ GPU 3a: step kernels, R1
@pytest.mark.gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=_sid)
def test_step_forward_matches_reference(hip_lib, case):
    """myo_lstm_step_fwd, rule R1: the bf16-c form with the mask and the saved arrays, the float32-c form (cm_next32 within 2 fp32
    ulps of the scale of the reference's unrounded value, the bf16 slot its rounding), the rollout form (no c_new / ws, no mask).
    gx and out_h are windows of wider sentinel-filled buffers that must come back untouched."""
    H, N, G = case
    L, c, lab = hip_lib.L, step_case(*case), _sid(case)
    H4 = 4 * H
    gx_sr = G * H4 + 16
    gxb, gxw, gxm = _in_sentinel((G, N, H4), (H4, gx_sr, 1), 8, N * gx_sr + 16, c["gx"])
    hp, cp, whh, keep, cp32 = dev_bf(c["hp"]), dev_bf(c["cp"]), dev_bf(c["whh"]), c["keep"].to(DEV), c["cp32"].to(DEV)
    gx_before = gxb.clone()
    fails = []

    def run(c_prev, keep_, save, c32_in, want_cm=True):
        outb, outw, outm = _in_sentinel((G, N, H), (3 * N * H, H, 1), N * H, G * 3 * N * H)
        hm, cm, cn = (torch.full((G, N, H), float("nan"), dtype=BF, device=DEV) for _ in range(3))
        ws = torch.full((G, N, H4), float("nan"), dtype=BF, device=DEV)
        cm32 = torch.full((G, N, H), float("nan"), device=DEV) if c32_in is not None else None
        hip_lib.check(L.myo_lstm_step_fwd(p(gxw), H4, gx_sr, p(hp), p(c_prev), p(whh), p(keep_), G, N, H, p(outw), 3 * N * H, p(hm),
                                          p(cm) if want_cm else None, p(cn) if save else None, p(ws) if save else None, p(c32_in), p(cm32), None))
        torch.cuda.synchronize()
        assert _outside_untouched(outb, outm), "out_h: a neighbour of the window was written"
        return {"out_h": outw, "hm": hm, "cm": cm, "c_new": cn, "ws": ws, "cm32": cm32}
    got, ref = run(cp, keep, True, None), c["fwd"]
    for k in ("out_h", "hm", "cm", "c_new", "ws"):
        fails += r1(k, got[k], ref[k], lab + " bf16-c")
    got, ref = run(None, keep, True, cp32), lstm_step_fwd_ref(c["gx"], c["hp"], c["cp32"], c["whh"], c["keep"])
    for k in ("out_h", "hm", "cm", "c_new", "ws"):
        fails += r1(k, got[k], ref[k], lab + " f32-c")
    scale = float(ref["c_new"].abs().max())                             # (of c itself: with N = 1 the one row is masked and cm32 is zero)
    e32 = float((got["cm32"].double().cpu() - ref["cm32"]).abs().max()) / float(2.0 ** (math.floor(math.log2(scale)) - 23))
    print("   %-34s cm32     worst %.2f fp32 ulps of the scale %.3f" % (lab, e32, scale))
    _note("cm32 fp32 ulps", e32)
    if e32 > 2.0:
        fails.append((lab, "cm32", e32))
    assert torch.equal(got["cm"], got["cm32"].to(BF))
    got2 = run(None, keep, False, cp32, want_cm=False)                    # float32 state alone
    assert torch.equal(got2["cm32"], got["cm32"]) and torch.equal(got2["hm"], got["hm"]) and bool(torch.isnan(got2["cm"].float()).all())
    got, ref = run(cp, None, False, None), lstm_step_fwd_ref(c["gx"], c["hp"], c["cp"], c["whh"], None)
    for k in ("out_h", "hm", "cm"):
        fails += r1(k, got[k], ref[k], lab + " rollout")
    assert torch.equal(got["hm"], got["out_h"]) and bool(torch.isnan(got["c_new"].float()).all()) and bool(torch.isnan(got["ws"].float()).all())
    assert torch.equal(gxb.view(torch.int16), gx_before.view(torch.int16))
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("case", BWD_CASES, ids=_sid)
def test_step_backward_matches_reference(hip_lib, case):
    """myo_lstm_step_bwd, rule R1, from the reference's saved arrays (bit-identical inputs): the full form, no mask, no dout, and
    the last step's NULL form (no later gradient).  dout is a window of a wider buffer."""
    H, N, G = case
    L, c, lab = hip_lib.L, step_case(*case), _sid(case)
    f = c["fwd"]
    H4 = 4 * H
    doutb, doutw, doutm = _in_sentinel((G, N, H), (2 * N * H + 8, H, 1), N * H + 8, G * (2 * N * H + 8) + 8, c["dout"])
    dgn, dcn, cp, cn, ws, keep = dev_bf(c["dgn"]), dev_bf(c["dcn"]), dev_bf(c["cp"]), dev_bf(f["c_new"]), dev_bf(f["ws"]), c["keep"].to(DEV)
    wt = dev_bf(c["whh"].transpose(1, 2))
    before = doutb.clone()
    fails = []
    forms = (("full", True, True, True), ("no-mask", True, True, False), ("no-dout", False, True, True), ("last", True, False, False))
    for name, has_dout, later, mask in forms:
        dg = torch.full((G, N, H4), float("nan"), dtype=BF, device=DEV)
        dcp = torch.full((G, N, H), float("nan"), dtype=BF, device=DEV)
        hip_lib.check(L.myo_lstm_step_bwd(p(doutw) if has_dout else None, 2 * N * H + 8, p(dgn) if later else None, p(dcn) if later else None,
                                          p(wt) if later else None, p(keep) if mask else None, p(cp), p(cn), p(ws), G, N, H, p(dg), p(dcp), None))
        torch.cuda.synchronize()
        rdg, rdc = lstm_step_bwd_ref(c["dout"] if has_dout else None, c["dgn"] if later else None, c["dcn"] if later else None, c["whh"],
                                     c["keep"] if mask else None, c["cp"], f["c_new"], f["ws"])
        fails += r1("dgates", dg, rdg, lab + " " + name) + r1("dc_prev", dcp, rdc, lab + " " + name)
    assert torch.equal(doutb.view(torch.int16), before.view(torch.int16))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ GPU 3b: cell kernels, R1
@pytest.mark.gpu
def test_cell_kernels_match_reference(hip_lib):
    """myo_lstm_cell_fwd / _bwd with bf16 storage (the shapes of test_lstm_cell_kernels_match_formulas), rule R1 against the
    reference handed the same bf16 recurrent products."""
    L = hip_lib.L
    G, N, H = 2, 37, 24
    g = _gen("cell")
    rn = lambda *s: bfv(torch.randn(*s, generator=g))
    gx, gh, cp, dout, dhm, dcm = rn(G, N, 4 * H), rn(G, N, 4 * H), rn(G, N, H), rn(G, N, H), rn(G, N, H), rn(G, N, H)
    keep = (torch.rand(N, generator=g) > 0.4).float()
    assert float(keep.min()) == 0 and float(keep.max()) == 1
    R = G * N
    outs = {k: torch.full((G, N, H), float("nan"), dtype=BF, device=DEV) for k in ("out_h", "hm", "cm", "c_new")}
    ws = torch.full((G, N, 4 * H), float("nan"), dtype=BF, device=DEV)
    d_gx, d_gh, d_cp, d_keep, d_dout, d_dhm, d_dcm = dev_bf(gx), dev_bf(gh), dev_bf(cp), keep.to(DEV), dev_bf(dout), dev_bf(dhm), dev_bf(dcm)
    hip_lib.check(L.myo_lstm_cell_fwd(p(d_gx), p(d_gh), p(d_cp), p(d_keep), R, N, H, 1, p(outs["out_h"]), p(outs["hm"]),
                                      p(outs["cm"]), p(outs["c_new"]), p(ws), None))
    torch.cuda.synchronize()
    ref = lstm_step_fwd_ref(gx, None, cp, None, keep, gh=gh)
    fails = []
    for k in ("out_h", "hm", "cm", "c_new"):
        fails += r1(k, outs[k], ref[k], "cell")
    fails += r1("ws", ws, ref["ws"], "cell")
    d_cn, d_ws = dev_bf(ref["c_new"]), dev_bf(ref["ws"])
    for name, later, mask in (("full", True, True), ("last", False, False)):
        dg = torch.full((G, N, 4 * H), float("nan"), dtype=BF, device=DEV)
        dcp = torch.full((G, N, H), float("nan"), dtype=BF, device=DEV)
        hip_lib.check(L.myo_lstm_cell_bwd(p(d_dout), p(d_dhm) if later else None, p(d_dcm) if later else None, p(d_keep) if mask else None,
                                          p(d_cp), p(d_cn), p(d_ws), R, N, H, 1, p(dg), p(dcp), None))
        torch.cuda.synchronize()
        rdg, rdc = lstm_step_bwd_ref(dout, None, dcm if later else None, None, keep if mask else None, cp, ref["c_new"], ref["ws"],
                                     dhm_next=dhm if later else None)
        fails += r1("dgates", dg, rdg, "cell " + name) + r1("dc_prev", dcp, rdc, "cell " + name)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ GPU 3c / 3d: sequence kernels
class _Seq:
    """Device buffers of one sequence case and the two launches."""

    def __init__(self, lib, case):
        from myochallenge_amd.rl.fused_lstm import lstm_seq_weights
        self.lib = lib
        self.H, self.rs, self.N, self.T, self.G, flag = case
        H, N, T, G = self.H, self.N, self.T, self.G
        self.fam = fam = seq_family(H, T, G, flag == "restart")
        self.strided = flag == "strided"
        H4 = 4 * H
        cut = lambda t, dim: t.narrow(dim, 0, N)
        self.cpu = {"gx": cut(fam["gx"], 2), "keep": cut(fam["keep"], 1).contiguous(), "dlat": cut(fam["dlat"], 2), "h0": cut(fam["h0"], 1),
                    "c0": cut(fam["c0"], 1), "c0f": cut(fam["c0f"], 1).contiguous(), "whh": fam["whh"]}
        if self.strided:
            sg, sr = H4 + 8, G * (H4 + 8) + 8
            self.gx_s = (N * sr + 64, sg, sr)
            self.gxb, self.gx, self.gxm = _in_sentinel((T, G, N, H4), (self.gx_s[0], sg, sr, 1), 8, T * self.gx_s[0] + 16, self.cpu["gx"])
            ost = N * H + 8
            self.out_s = (T * ost + 16, ost)
            self.lat_geom = ((G, T, N, H), (self.out_s[0], ost, H, 1), 8, G * self.out_s[0] + 16)
            self.doutb, self.dlat, self.doutm = _in_sentinel(*self.lat_geom, self.cpu["dlat"])
        else:
            self.gx_s, self.out_s = (G * N * H4, N * H4, H4), (T * N * H, N * H)
            self.gx = dev_bf(self.cpu["gx"])                                     # [T, G, N, 4H] dense
            self.dlat = dev_bf(self.cpu["dlat"])
        self.keep = self.cpu["keep"].to(DEV)
        self.w_frag, self.wt_frag = lstm_seq_weights(dev_bf(fam["whh"]), self.rs)

    def forward(self, prefill, c32, keep=None):
        H, N, T, G = self.H, self.N, self.T, self.G
        mk = lambda *s: torch.full(s, prefill, dtype=BF, device=DEV)
        hm, cm, cn, ws = mk(T + 1, G, N, H), mk(T + 1, G, N, H), mk(T, G, N, H), mk(T, G, N, 4 * H)
        hm[0], cm[0] = dev_bf(self.cpu["h0"]), dev_bf(self.cpu["c0f"] if c32 else self.cpu["c0"])
        if self.strided:
            latb, lat, latm = _in_sentinel(*self.lat_geom)
        else:
            lat = mk(G, T, N, H)
        c0f = self.cpu["c0f"].to(DEV) if c32 else None
        self.lib.check(self.lib.L.myo_lstm_seq_fwd(p(self.gx), *self.gx_s, p(hm), p(cm), p(self.w_frag), p(self.keep if keep is None else keep), G, N, H, T,
                                                   self.rs, p(lat), *self.out_s, p(cn), p(ws), p(c0f), None))
        torch.cuda.synchronize()
        if self.strided:
            assert _outside_untouched(latb, latm), "out_h: written outside its strided window"
        return {"hm": hm, "cm_raw": cm, "cn_raw": cn, "ws_raw": ws, "lat": lat}

    def rows(self, o):
        """Row-major CPU float views of a forward result (cm's slot 0 is row-major already)."""
        from myochallenge_amd.rl.fused_lstm import lstm_seq_rows
        H, N, rs = self.H, self.N, self.rs
        cm = torch.cat([o["cm_raw"][:1], lstm_seq_rows(o["cm_raw"][1:], N, H, 1, rs)]).float().cpu()
        return {"hm": o["hm"].float().cpu(), "cm": cm, "c_new": lstm_seq_rows(o["cn_raw"], N, H, 1, rs).float().cpu(),
                "ws": lstm_seq_rows(o["ws_raw"], N, H, 4, rs).float().cpu(), "lat": o["lat"].float().cpu()}

    def backward(self, o):
        H, N, T, G = self.H, self.N, self.T, self.G
        dG = torch.full((T, G, N, 4 * H), float("nan"), dtype=BF, device=DEV)
        self.lib.check(self.lib.L.myo_lstm_seq_bwd(p(self.dlat), *self.out_s, p(self.wt_frag), p(self.keep), p(o["cm_raw"]), p(o["cn_raw"]), p(o["ws_raw"]),
                                                   G, N, H, T, self.rs, p(dG), None))
        torch.cuda.synchronize()
        return dG


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEQ_CASES, ids=_qid)
def test_sequence_forward_every_step_matches_reference(hip_lib, case):
    """myo_lstm_seq_fwd in the bf16-c mode, rule R1 PER STEP: the state entering step t + 1 is exactly what the kernel stored in
    hm[t + 1] / cm[t + 1], so every step is one step of the reference started from the kernel's own stored state.  Also: slot 0 of
    hm / cm untouched, no dependence on keep[0], NaN-prefilled outputs come back without a NaN (the tile-major stores cover their
    arrays), and a second run into buffers that held something else is bit-identical."""
    s = _Seq(hip_lib, case)
    H, N, T, G = s.H, s.N, s.T, s.G
    lab = _qid(case)
    a = s.forward(float("nan"), False)
    for k in ("hm", "cm_raw", "cn_raw", "ws_raw"):
        assert not bool(torch.isnan(a[k].float()).any()), k + ": an element was not written"
    assert not bool(torch.isnan(a["lat"].float()[..., :H]).any())
    assert torch.equal(a["hm"][0], dev_bf(s.cpu["h0"])) and torch.equal(a["cm_raw"][0], dev_bf(s.cpu["c0"]))
    keep2 = s.keep.clone()
    keep2[0] = 1.0 - keep2[0]
    b = s.forward(3.0, False, keep2)
    for k in ("hm", "cm_raw", "cn_raw", "ws_raw", "lat"):
        assert torch.equal(a[k].view(torch.int16), b[k].view(torch.int16)), k + ": depends on keep[0] or on the buffers' previous contents"
    if s.strided:
        assert _outside_untouched(s.gxb, s.gxm)
    r, fails = s.rows(a), []
    for t in range(T):
        ref = lstm_step_fwd_ref(s.cpu["gx"][t], r["hm"][t], r["cm"][t], s.cpu["whh"], s.cpu["keep"][t + 1] if t + 1 < T else None, act="seq")
        for k, got in (("out_h", r["lat"][:, t]), ("hm", r["hm"][t + 1]), ("cm", r["cm"][t + 1]), ("c_new", r["c_new"][t]), ("ws", r["ws"][t])):
            fails += r1(k, got, ref[k], "%s t=%d" % (lab, t))
    assert not fails, fails


def _seq_chain_checks(lab, fam_key, N, rows32, dG_kernel, cpu):
    """R2 of a float32-c forward pass (rows32: its arrays, row-major, on the CPU) and the two backward comparisons against the
    family's reference, bounded by its twin."""
    ref, tw = seq_refs(*fam_key, torch.float64), seq_twin(*fam_key)
    fails = []
    for k in FWD_ARRAYS:                                # (every array has its rows in dimension 2)
        miss = r2(k, rows32[k], ref["f32"][k].narrow(2, 0, N), tw[k], lab + " f32-c")
        if fam_key[1] == 1:
            # T = 1 is no chain: ONE step from bit-identical inputs, rule R1's case.  Every difference is a first-generation flip, and
            # v_exp / v_rcp (2^-19 of the scale, R1's derivation) flip up to 2^5 times as often as the twin's fp32 libm (2^-24): an L2
            # ratio of up to 2^2.5 = 5.7 from a correct kernel.  Measured on an MI355X: 5.45 (H = 128, N = 48, lat and hm: 3 flipped
            # elements of 12 288, each by one ulp; the twin is 1.8e-5 away over its 2096 rows), every other T = 1 array at 1.4 or
            # below.  R1 bounds these arrays instead; the R2 figure is still printed.
            miss = r1(k, rows32[k], ref["f32"][k].narrow(2, 0, N), lab + " f32-c T=1")
        fails += miss
    # (i) the backward kernel alone: the reference's backward pass on the arrays the KERNEL saved
    want = lstm_seq_bwd_ref(cpu["dlat"], cpu["whh"], cpu["keep"], rows32["cm"], rows32["c_new"], rows32["ws"], act=_act_of(fam_key[0]))
    fails += r2("dG_same", dG_kernel, want, tw["dG_same"], lab + " bwd alone")
    # (ii) end to end: the reference's own forward + backward
    fails += r2("dG_own", dG_kernel, ref["bwd_own"].narrow(2, 0, N), tw["dG_own"], lab + " fwd+bwd")
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEQ_CASES, ids=_qid)
def test_sequence_chain_matches_reference(hip_lib, case):
    """myo_lstm_seq_fwd with the cell state carried in float32 (c0_32), free-running over T steps, and myo_lstm_seq_bwd: rule R2.
    The backward pass twice — from the kernel's saved arrays against the reference's backward pass on those same arrays (the
    backward kernel alone), and end to end against the reference's own forward + backward."""
    s = _Seq(hip_lib, case)
    a = s.forward(float("nan"), True)
    dG = s.backward(a)
    assert not bool(torch.isnan(dG.float()).any()), "dgates: an element was not written"
    if s.strided:
        assert _outside_untouched(s.doutb, s.doutm)
    r = s.rows(a)
    fails = _seq_chain_checks(_qid(case), (s.H, s.T, s.G, case[5] == "restart"), s.N, r, dG, s.cpu)
    assert not fails, fails


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: "H%d-N%d-T%d-G%d" % c)
def test_step_kernel_chain_matches_reference(hip_lib, case):
    """T launches of myo_lstm_step_fwd (float32 cell state, ping-pong) and of myo_lstm_step_bwd, as `_run_rows` chains them at the
    hidden sizes without a sequence kernel, through the comparisons of test_sequence_chain_matches_reference."""
    H, N, T, G = case
    L = hip_lib.L
    fam = seq_family(H, T, G, False)
    cut = lambda t, dim: t.narrow(dim, 0, N).contiguous()
    cpu = {"gx": cut(fam["gx"], 2), "keep": cut(fam["keep"], 1), "dlat": cut(fam["dlat"], 2), "h0": cut(fam["h0"], 1), "c0f": cut(fam["c0f"], 1), "whh": fam["whh"]}
    H4 = 4 * H
    gx, whh, keep, dlat = dev_bf(cpu["gx"]), dev_bf(cpu["whh"]), cpu["keep"].to(DEV), dev_bf(cpu["dlat"])
    mk = lambda *s_: torch.full(s_, float("nan"), dtype=BF, device=DEV)
    hm, cm, cn, ws, lat, dG = mk(T + 1, G, N, H), mk(T + 1, G, N, H), mk(T, G, N, H), mk(T, G, N, H4), mk(G, T, N, H), mk(T, G, N, H4)
    hm[0], cm[0] = dev_bf(cpu["h0"]), dev_bf(cpu["c0f"])
    c32 = [cpu["c0f"].to(DEV), torch.empty((G, N, H), device=DEV)]
    kp = lambda t: p(keep[t + 1]) if t + 1 < T else None
    for t in range(T):
        hip_lib.check(L.myo_lstm_step_fwd(p(gx[t]), N * H4, H4, p(hm[t]), p(cm[t]), p(whh), kp(t), G, N, H, p(lat[:, t]), T * N * H, p(hm[t + 1]),
                                          p(cm[t + 1]), p(cn[t]), p(ws[t]), p(c32[t & 1]), p(c32[(t + 1) & 1]), None))
    wt = dev_bf(cpu["whh"].transpose(1, 2))
    dcm = mk(2, G, N, H)
    for t in range(T - 1, -1, -1):
        last = t == T - 1
        hip_lib.check(L.myo_lstm_step_bwd(p(dlat[:, t]), T * N * H, None if last else p(dG[t + 1]), None if last else p(dcm[(t + 1) & 1]), p(wt), kp(t),
                                          p(cm[t]), p(cn[t]), p(ws[t]), G, N, H, p(dG[t]), p(dcm[t & 1]), None))
    torch.cuda.synchronize()
    r = {"hm": hm.float().cpu(), "cm": cm.float().cpu(), "c_new": cn.float().cpu(), "ws": ws.float().cpu(), "lat": lat.float().cpu()}
    fails = _seq_chain_checks("chain H%d-N%d-T%d-G%d" % case, (H, T, G, False), N, r, dG, cpu)
    # the float32 state the chain ends in: what the bf16 slot cm[T] is the rounding of
    assert torch.equal(c32[T & 1].to(BF), cm[T])
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ GPU 3e: the whole minibatch step
PREFILL, TAIL = 7.0, 4096


class _TorchProbe:
    """Stands in for the `torch` name of rl/fused_lstm.py and remembers the left operands of its batched GEMMs: dG is a local of
    `_run_rows`, and the LSTM weight-gradient GEMM is where it can be seen without touching the code under test."""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def bmm(self, a, b, **kw):
        self.seen.append(a)
        return torch.bmm(a, b, **kw)


class _Step:
    """A flattened recurrent policy on the device, built as PPO builds it, its gradient vector inside a larger allocation (sentinel
    behind the G elements, the G elements pre-filled), and a FusedRecurrentPPOStep on it."""

    def __init__(self, lib, case):
        from myochallenge_amd.rl.fused_lstm import FusedRecurrentPPOStep
        from myochallenge_amd.rl.fused_mlp import flatten_parameters
        H, route, m, arch, sde = case
        self.c = c = whole_inputs(*case, 0)
        self.pol = build_recurrent_policy(H, arch, sde, c["seed"]).to(DEV)
        self.flat = flat = flatten_parameters(self.pol)
        self.G = G = flat["g"].numel()
        self.big = torch.full((G + TAIL,), SENT, device=DEV)
        self.big[:G] = PREFILL
        flat["g"] = self.big[:G]
        for q, (off, k) in zip(flat["params"], flat["slots"]):
            q.grad = flat["g"][off:off + k].view(q.shape)
        self.step = FusedRecurrentPPOStep.create(self.pol, lib, CLIP, ENT_COEF, VF_COEF)
        assert self.step is not None
        assert self.step.step_kernels == (route != "cell") and self.step.seq_kernels == route.startswith("seq") and self.step.c32
        self.step.external_adv_stats = True
        self.step.stats.copy_(torch.tensor(c["stats"], dtype=torch.float32))

    def run(self):
        c = self.c
        T, m = c["keep"].shape
        H = c["h0"].shape[2]
        d = lambda t: t.to(DEV).contiguous()
        hm = torch.full((T + 1, 2, m, H), float("nan"), dtype=BF, device=DEV)
        cm = torch.full_like(hm, float("nan"))
        hm[0], cm[0] = dev_bf(c["h0"]), dev_bf(c["c0"])
        self.step.refresh_shadow()                   # (run_sequences / _gather_chunks do it in front of _run_rows)
        with torch.no_grad():
            pl, vl = self.step._run_rows(dev_bf(c["x"]).unsqueeze(0), d(c["act"]), d(c["oldlp"]), d(c["adv"]), d(c["ret"]), d(c["keep"]), hm, cm, d(c["c0"]))
        torch.cuda.synchronize()
        return float(pl), float(vl), {n: q.grad.detach().cpu().double() for n, q in self.pol.named_parameters()}

    def dG(self, probe):
        T, m = self.c["keep"].shape
        H4 = 4 * self.c["h0"].shape[2]
        got = [a for a in probe.seen if tuple(a.shape) == (2 * T, H4, m)]
        assert len(got) == 2 and got[0].data_ptr() == got[1].data_ptr()          # the W_hh and the W_ih product read the same dG
        return got[0].transpose(1, 2).reshape(T, 2, m, H4).float().cpu()

    def check_slots(self):
        mask = torch.zeros(self.G, dtype=torch.bool, device=DEV)
        for q, (off, k) in zip(self.flat["params"], self.flat["slots"]):
            mask[off:off + k] = True
        assert int((~mask).sum()) > 0
        assert bool((self.big[:self.G][~mask] == PREFILL).all()), "a padding slot of the flat gradient was written"
        assert bool((self.big[:self.G][mask] != PREFILL).all()), "a gradient element was not written"
        assert bool((self.big[self.G:] == SENT).all()), "the step wrote past the gradient vector"


def _whole_step_checks(case, pl, vl, grads, dG):
    ref, tw, lab = whole_ref(*case, 0, torch.float64), whole_twin(*case), _wid(case)
    fails = []
    assert set(grads) == set(ref["grads"])
    for n in sorted(grads):
        assert torch.isfinite(grads[n]).all(), n
        k, D = rel(grads[n], ref["grads"][n]), tw["D"][_net_of(n)]
        print("R2 %-24s %-42s kernel %.3e own twin %.3e net D %.3e kernel/D %.2f" % (lab, n, k, tw[n], D, _note("R2 whole-step gradient", k / D)))
        if k > MARGIN * D:
            fails.append((n, k, D))
    for g_, net in enumerate(("pi", "vf")):
        fails += r2("dG." + net, dG[:, g_], ref["dG"][:, g_], tw["dG." + net], lab)
    for name, got, net in (("pl", pl, "pi"), ("vl", vl, "vf")):
        want = float(ref[name])
        err, size = abs(got - want) / abs(want), max(tw["D"][net], tw[name])
        print("R2 %-24s %-42s kernel %.3e size %.3e ratio %.2f" % (lab, name, err, size, _note("R2 whole-step loss", err / size)))
        if err > MARGIN * size:
            fails.append((name, err, size))
    return fails


@pytest.mark.gpu
@pytest.mark.parametrize("case", WHOLE_CASES, ids=_wid)
def test_whole_recurrent_step_matches_reference(hip_lib, monkeypatch, case):
    """FusedRecurrentPPOStep._run_rows on synthetic gathered rows through its three routes (H = 32: step kernels, 48: GEMM + cell
    kernels, 128: sequence kernels with row split 1 and 2): losses and every parameter's gradient by rule R2 against
    recurrent_step_ref, dG through the weight gradients formed from it; gradient slots outside the parameters untouched."""
    H, route, m, arch, sde = case
    if route.startswith("seq"):
        monkeypatch.setenv("MYO_LSTM_SEQ_RS", route[3:])
    for var in ("MYO_LSTM_TWO_KERNELS", "MYO_LSTM_SEQ", "MYO_LSTM_C32"):
        monkeypatch.delenv(var, raising=False)
    from myochallenge_amd.rl import fused_lstm
    probe = _TorchProbe()
    monkeypatch.setattr(fused_lstm, "torch", probe)
    run = _Step(hip_lib, case)
    pl, vl, grads = run.run()
    run.check_slots()
    fails = _whole_step_checks(case, pl, vl, grads, run.dG(probe))
    assert not fails, fails


@pytest.mark.gpu
def test_gsde_rollout_minibatch_matches_reference(hip_lib, monkeypatch):
    """The lstm+mlp-gsde case of test_reorient.py::test_fused_recurrent_step_matches_autograd (same policy, rollout and minibatch)
    through recurrent_step_ref: the rows `run_sequences` gathered and the fused gradients are taken to the CPU; every gradient is
    within rule R2 of the rounding-matched reference (twin on the same 512 rows), so what separates the fused actor-trunk gradient
    from an unrounded one is rounding (DESIGN.md section 6 names the points), not a mistake.  Printed besides: fused and
    rounding-matched reference against the unrounded float64 gradient."""
    import test_reorient
    N, T, m = 128, 8, 64
    a, _, adv, ret, idx, pol = test_reorient.fused_recurrent_pair(monkeypatch, (64,), 32, True, N, T, m)
    P = recurrent_policy_params(pol)
    fr, rows = a._fused_rec, {}
    g = a._rec_stage(adv, ret, T, N, m)                 # (captures the step's graph: the probe goes in behind it)
    g["idx"].copy_(idx)
    orig = fr._run_rows

    def spy(*args):
        rows["args"] = [t.detach().float().cpu().clone() for t in args]
        return orig(*args)
    monkeypatch.setattr(fr, "_run_rows", spy)
    a._rec_forward_backward()
    torch.cuda.synchronize()
    x, act, oldlp, adv_mb, ret_mb, keep, hm, cm, c0m = rows["args"]
    from myochallenge_amd.native import HP_CLIP
    clip = float(fr.hp[HP_CLIP]) if fr.hp is not None else fr.clip
    stats = tuple(float(v) for v in fr.stats.cpu())
    ref = lambda **kw: recurrent_step_ref(P, x[0], act, oldlp, adv_mb, ret_mb, stats, keep, hm[0], c0m, clip, fr.vf, fr.ent, "step", fr.c32, **kw)
    R, Tw, U = ref(), ref(dt=torch.float32), ref(rnd=identity)
    fused = {n: q.grad.detach().cpu().double() for n, q in pol.named_parameters()}
    assert set(fused) == set(R["grads"])
    D = {net: max(rel(Tw["grads"][n], R["grads"][n]) for n in fused if _net_of(n) == net) for net in ("pi", "vf")}
    edge = float(torch.minimum((R["ratio"] - (1 - clip)).abs(), (R["ratio"] - (1 + clip)).abs()).min())
    print("gsde rollout: smallest distance of a ratio from 1 +- clip %.2e" % edge)
    fails = []
    for n in sorted(fused):
        k = rel(fused[n], R["grads"][n])
        print("R2 gsde-rollout %-36s fused-ref %.3e twin %.3e net D %.3e ratio %.2f | fused-unrounded %.3e ref-unrounded %.3e" % (
            n, k, rel(Tw["grads"][n], R["grads"][n]), D[_net_of(n)], _note("R2 gsde rollout gradient", k / D[_net_of(n)]),
            rel(fused[n], U["grads"][n]), rel(R["grads"][n], U["grads"][n])))
        if k > MARGIN * D[_net_of(n)]:
            fails.append((n, k, D[_net_of(n)]))
    for name, got, net in (("pl", float(g["pl"]), "pi"), ("vl", float(g["vl"]), "vf")):
        want = float(R[name])
        err, size = abs(got - want) / abs(want), max(D[net], rel(Tw[name], R[name]))
        print("R2 gsde-rollout %-36s kernel %.3e size %.3e" % (name, err, size))
        if err > MARGIN * size:
            fails.append((name, err, size))
    assert not fails, fails
