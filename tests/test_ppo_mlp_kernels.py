"""The matrix-core PPO kernels of csrc/myo_ppo_mlp.h (k_mlp_prep, k_mlp_fwdbwd, k_mlp_wgrad, k_mlp_reduce, k_mlp_reduce_finish,
k_mlp_policy) against tests/mlp_ref.py: a float64 CPU reference that rounds to bf16 exactly where the kernels do, so that only
the fp32 summation order (and the few bf16 roundings it flips) separates kernel and reference.

Tolerances are not literals.  Every GPU case also evaluates the reference's float32 TWIN (same statement, fp32 accumulation) on
the same inputs; with d_twin(p) = |g_twin - g_ref| / |g_ref| per parameter tensor and D the largest d_twin over the tensors of
the same net, the kernel has to stay within MARGIN * D in that norm, and within MARGIN * (the net's largest twin value) in the
largest element-wise difference relative to max |g_ref|.  Scalars (losses, diagnostics) use max(D of their net, their own twin
distance).  MARGIN = 4: kernel and twin both add bf16 products in fp32 and differ in order only (32-wide MFMA chunks and 16
split-K slabs against torch's blocking).  The rollout kernel's head mean / value are bounded the same way in the largest
absolute difference, with the twin evaluated on the case's rows plus 2048 more and pooled over both nets (on 32 or 96 rows the
twin flips a bf16 rounding in some cases and none in others: see _check_rollout_mean_value).  The policy loss is compared with
the reference at the advantage moments the kernel stored (see _check_against_reference).  The advantage moments, the Philox noise and the log-probs are bounded from fp32 arithmetic; the
reasoning stands next to each bound.

CPU tests (-m "not gpu") pin the reference itself: against float64 autograd with the rounding switched off, its rounding
function against torch's bf16 cast, and the input condition that makes the clip branch of every GPU case well defined.

Largest kernel / twin ratios measured on an MI355X over all cases of this file (the bound is MARGIN = 4):
  gradients, |.| norm            2.40  (O31-A15-B1024, actor W1: kernel 2.78e-4, the actor's D 1.16e-4)
  gradients, largest element     2.53  (O96-A47-B1024, actor W1: kernel 1.01e-3, the actor's 4.00e-4)
  losses and diagnostics         1.47  (O31-A15-B1024, policy loss: kernel 2.90e-4, twin 1.98e-4)
  rollout head mean / value      0.56  (N96-O128-A31, mean: kernel 1.40e-4, pooled twin 2.51e-4)
  a tensor against its OWN twin figure, where the floor of the net's worst tensor is what keeps it in: up to 12 (critic head
  bias of O96-A47: kernel 2.2e-6, twin 1.8e-7, the critic's D 2.8e-5)
D itself ranges from 1e-5 (critic) to 4e-4 (actor W1); the advantage mean at offset +100 is off by 1.3e-5 (1.7 ulp; bound 4.1e-4),
the partial sums of |g|^2 by 1e-9 relative (bound 7e-7).
"""
import ctypes as C
import functools
import math

import pytest
import torch

import mlp_ref
from mlp_ref import gaussian_logp, identity, policy_params, ppo_mlp_rollout_ref, ppo_mlp_step_ref, round_bf16

MARGIN = 4.0
CLIP, VF_COEF, ENT_COEF = 0.2, 0.7, 0.01
RATIO_MARGIN, ADV_MARGIN = 1e-3, 1e-6          # input conditions: distance of every ratio from 1 +- clip, of every advantage from 0
EPS32 = 2.0 ** -24                               # half an ulp of 1.0f: the relative error of one fp32 rounding

# (O, A, B, advantage offset): every branch of the kernels — OP = 32 / 64 / 96 / 128; the gather's `lane < O`, `lane + 64 < O`,
# `lane + 64 < OP`; one, two and three head tiles with and without padded rows; masked 128-row weight-gradient tiles; B = 2048
# gives a split four k-steps instead of two; the offset loads the moment merge of k_adv_moments / k_mlp_prep.
STEP_CASES = [(1, 1, 1024, 0.0), (31, 15, 1024, 0.0), (32, 16, 1024, 0.0), (33, 17, 1024, 0.0), (64, 32, 1024, 0.0),
              (65, 33, 1024, 0.0), (86, 39, 1024, 0.0), (96, 47, 1024, 0.0), (97, 48, 1024, 0.0), (127, 5, 1024, 0.0),
              (128, 48, 1024, 0.0), (33, 17, 2048, 0.0), (86, 39, 2048, 0.0), (65, 33, 1024, 100.0)]
EXTERNAL_STATS_CASES = [(33, 17, 1024, 0.0), (128, 48, 1024, 0.0)]          # compute_adv_stats = 0
EDGE_CASES = [(1, 1, 1024, 0.0), (97, 48, 1024, 0.0)]                       # hyper-parameter block, both tails, workspace reuse
ROLLOUT_SHAPES = [(1, 1), (33, 3), (64, 4), (65, 5), (128, 31), (33, 32), (64, 33), (128, 48)]     # (O, A)
ROLLOUT_CASES = [(N, O, A) for N in (32, 96) for O, A in ROLLOUT_SHAPES]

# largest kernel / twin ratio of this process, per quantity (what the module docstring quotes; printed by the tests with -s)
RATIOS_MEASURED = {}

_case_id = lambda c: "O%d-A%d-B%d%s" % (c[0], c[1], c[2], "-offset" if c[3] else "")


# ------------------------------------------------------------------------------------------------ inputs, shared by CPU and GPU tests
def build_policy(O, A, seed):
    """A fresh ActorCriticPolicy(O, A, (256, 256), (256, 256)) with every bias random at its weights' scale and
    log_std = -0.5 +- 0.1 per action: no bias fragment and no log_std term of the kernels may drop out unnoticed."""
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        pol = ActorCriticPolicy(O, A, (256, 256), (256, 256), lstm_hidden_size=None)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in pol.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * m.weight.std(unbiased=False))
        pol.log_std.copy_(-0.5 + 0.1 * torch.randn(A, generator=g))
    return pol


def _seed(O, A, B, offset):
    return 100000 * (B // 1024) + 1000 * O + 10 * A + (1 if offset else 0)


@functools.lru_cache(maxsize=None)
def step_case(O, A, B, offset):
    """Rollout arrays with more rows than the minibatch (3000 for B = 1024), a random subset in random order that holds row 0
    and the last row, on-policy actions, old log-probs off by N(0, 0.05), advantages and returns that carry signal."""
    seed = _seed(O, A, B, offset)
    params = policy_params(build_policy(O, A, seed))
    g = torch.Generator().manual_seed(seed + 2)
    R = 2 * B + 952
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    obs = rn(R, O).float()
    inner = 1 + torch.randperm(R - 2, generator=g)[:B - 2]
    idx = torch.cat([torch.tensor([0, R - 1]), inner])[torch.randperm(B, generator=g)]
    obs[idx[7]] = 0.0                                          # one all-zero row
    obs[idx[11], 0], obs[idx[13], O - 1], obs[idx[17], O // 2] = 10.0, -10.0, 10.0      # VecNormalize's clip
    ls = params["log_std"].double()
    mean = ppo_mlp_rollout_ref(params, obs)[0]
    act = (mean + torch.exp(ls) * rn(R, A)).float()
    oldlp = (gaussian_logp(act.double(), mean, ls) + 0.05 * rn(R)).float()
    wa, wo = rn(A), rn(O) / math.sqrt(O)
    adv = (torch.tanh(((act.double() - mean) * torch.exp(-ls)) @ wa / 6) + 0.3 * rn(R) + offset).float()
    ret = (torch.sin(obs.double() @ wo) + 0.1 * rn(R)).float()
    return {"O": O, "A": A, "B": B, "seed": seed, "params": params, "obs": obs, "act": act, "oldlp": oldlp, "adv": adv, "ret": ret, "idx": idx}


@functools.lru_cache(maxsize=None)
def step_ref(case, dt, compute_adv_stats=True):
    c = step_case(*case)
    return ppo_mlp_step_ref(c["params"], c["obs"], c["act"], c["oldlp"], c["adv"], c["ret"], c["idx"], CLIP, VF_COEF, ENT_COEF,
                            compute_adv_stats=compute_adv_stats, adv_stats=(0.0, 1.0), dt=dt)


@functools.lru_cache(maxsize=None)
def step_ref_at_moments(case, dt, mean, std):
    """The reference with the advantage moments handed in (the kernel's own, as read back from the device)."""
    c = step_case(*case)
    return ppo_mlp_step_ref(c["params"], c["obs"], c["act"], c["oldlp"], c["adv"], c["ret"], c["idx"], CLIP, VF_COEF, ENT_COEF,
                            compute_adv_stats=False, adv_stats=(mean, std), dt=dt)


@functools.lru_cache(maxsize=None)
def rollout_case(N, O, A):
    seed = 7000000 + 10000 * N + 100 * O + A
    g = torch.Generator().manual_seed(seed + 2)
    obs = torch.randn(N, O, generator=g)
    obs[5] = 0.0
    obs[3, 0], obs[9, O - 1], obs[N - 1, O // 2] = 10.0, -10.0, 10.0
    return {"N": N, "O": O, "A": A, "seed": seed, "obs": obs}


GRAD_KEYS = ("W1", "b1", "W2", "b2", "Wh", "bh")


def ref_grads(res):
    """{(net, key): float64 tensor} of a reference result, log_std filed under the actor."""
    out = {(net, k): t.double() for net in ("pi", "vf") for k, t in zip(GRAD_KEYS, res["grads"][net])}
    out[("pi", "log_std")] = res["grads"]["log_std"].double()
    return out


def dist(a, b):
    """(|a - b| / |b|, max |a - b| / max |b|) of float64 tensors."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm()), float((a - b).abs().max() / b.abs().max())


def twin_sizes(ref, twin):
    """Per net: the largest twin distance over its gradient tensors, in both norms."""
    gr, gt = ref_grads(ref), ref_grads(twin)
    D = {"pi": [0.0, 0.0], "vf": [0.0, 0.0]}
    for key in gr:
        d = dist(gt[key], gr[key])
        D[key[0]] = [max(D[key[0]][0], d[0]), max(D[key[0]][1], d[1])]
    return D


# ------------------------------------------------------------------------------------------------ CPU: the reference itself
def _autograd_statement(params, obs, act, oldlp, adv, ret, idx, normalize):
    """SB3's PPO minibatch loss in float64 through autograd: evaluate_actions -> clipped surrogate + vf_coef * MSE - ent_coef *
    entropy (the formulas of rl/ppo.py's _loss and rl/fused_mlp.py's ppo_mlp_step_grads).  Without normalisation the advantage
    still passes the loss phase's (adv - 0) / (1 + 1e-8): the kernels have one formula and are handed {0, 1}."""
    import torch.nn.functional as F
    dt = torch.float64
    leaf = lambda t: t.to(dt).clone().requires_grad_(True)
    P = {net: [leaf(t) for t in params[net]] for net in ("pi", "vf")}
    ls = leaf(params["log_std"])
    x, a, olp, ad, rt = (t[idx].to(dt) for t in (obs, act, oldlp, adv, ret))

    def mlp(p):
        h = torch.relu(F.linear(x, p[0], p[1]))
        h = torch.relu(F.linear(h, p[2], p[3]))
        return F.linear(h, p[4], p[5])
    mean, values = mlp(P["pi"]), mlp(P["vf"])[:, 0]
    logp = (-0.5 * ((a - mean) ** 2) / torch.exp(2 * ls) - ls - 0.5 * math.log(2 * math.pi)).sum(-1)
    entropy = (0.5 + 0.5 * math.log(2 * math.pi) + ls).sum()
    m, s = (ad.mean(), ad.std()) if normalize else (0.0, 1.0)
    an = (ad - m) / (s + 1e-8)
    ratio = torch.exp(logp - olp)
    pl = -torch.min(an * ratio, an * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
    vl = F.mse_loss(values, rt)
    ent_loss = -entropy
    (pl + ENT_COEF * ent_loss + VF_COEF * vl).backward()
    with torch.no_grad():
        lr = logp - olp
        diag = {"approx_kl": ((ratio - 1) - lr).mean(), "clip_frac": ((ratio - 1).abs() > CLIP).double().mean(), "ent_loss": ent_loss.detach()}
    grads = {(net, k): p.grad for net in ("pi", "vf") for k, p in zip(GRAD_KEYS, P[net])}
    grads[("pi", "log_std")] = ls.grad
    return grads, pl.detach(), vl.detach(), diag


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("case", [(33, 17, 1024, 0.0), (86, 39, 1024, 0.0)], ids=_case_id)
def test_reference_without_rounding_is_the_autograd_loss(case, normalize):
    """With the rounding function replaced by the identity the reference is SB3's loss: gradients, losses and diagnostics equal
    float64 autograd to 1e-10 relative on every parameter."""
    c = step_case(*case)
    res = ppo_mlp_step_ref(c["params"], c["obs"], c["act"], c["oldlp"], c["adv"], c["ret"], c["idx"], CLIP, VF_COEF, ENT_COEF,
                           compute_adv_stats=normalize, adv_stats=(0.0, 1.0), dt=torch.float64, rnd=identity)
    grads, pl, vl, diag = _autograd_statement(c["params"], c["obs"], c["act"], c["oldlp"], c["adv"], c["ret"], c["idx"], normalize)
    mine = ref_grads(res)
    assert set(mine) == set(grads)
    for key, g in grads.items():
        assert mine[key].shape == g.shape, key
        assert dist(mine[key], g)[0] <= 1e-10, (key, dist(mine[key], g))
    for name, want in (("pl", pl), ("vl", vl), ("approx_kl", diag["approx_kl"]), ("clip_frac", diag["clip_frac"]), ("ent_loss", diag["ent_loss"])):
        assert abs(float(res[name]) - float(want)) <= 1e-10 * abs(float(want)), name
    A = c["A"]
    acc = res["acc"]       # the kernel's loss columns restate the same quantities
    assert torch.equal(acc[:A] - ENT_COEF, res["grads"]["log_std"]) and torch.equal(acc[A + 2:2 * A + 2], res["grads"]["pi"][5])
    assert float(acc[A]) == float(res["pl"]) and float(acc[A + 1]) == float(res["vl"]) and float(acc[2 * A + 2]) == float(res["grads"]["vf"][5])


def test_rounding_function_is_torch_bf16_cast_bit_for_bit():
    """round_bf16 == tensor.bfloat16() on ties (to even, both neighbours), denormals, both signs, zeros, the largest finite
    values that do not overflow, and random bit patterns — from float32 and from float64 holding the same values."""
    bits = [0x3F800000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F80FFFF, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF,
            0x00800000, 0x00808000, 0x7F7F0000, 0x7F7F7FFF, 0x00000000, 0x33800000, 0x3EAAAAAB, 0x40490FDB, 0x0000FFFF, 0x00017FFF]
    bits += [b | 0x80000000 for b in bits]
    g = torch.Generator().manual_seed(0)
    rnd_bits = torch.randint(0, 2 ** 31 - 1, (20000,), generator=g, dtype=torch.int64)
    rnd_bits = rnd_bits[((rnd_bits >> 23) & 0xFF) < 0xFE]                      # finite, below the values that round to infinity
    rnd_bits = torch.cat([rnd_bits, rnd_bits | 0x80000000])
    allb = torch.cat([torch.tensor(bits, dtype=torch.int64), rnd_bits])
    x = torch.where(allb >= 2 ** 31, allb - 2 ** 32, allb).to(torch.int32).view(torch.float32)
    want = x.bfloat16().float()
    assert torch.isfinite(want).all()
    got32, got64 = round_bf16(x), round_bf16(x.double())
    assert got32.dtype == torch.float32 and got64.dtype == torch.float64
    assert torch.equal(got32.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got64.float().view(torch.int32), want.view(torch.int32)) and torch.equal(got64, want.double())
    # float64 is rounded once: a value just above a tie that fp32 would first round ONTO the tie (and then to even, downwards)
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert float(round_bf16(v)) == 1.0 + 2.0 ** -7 and float(v.float().bfloat16()) == 1.0


def _input_condition(res, clip):
    ratio, an = res["ratio"], res["adv_norm"]
    edge = float(torch.minimum((ratio - (1 - clip)).abs(), (ratio - (1 + clip)).abs()).min())
    return edge, float(an.abs().min())


@pytest.mark.parametrize("case", STEP_CASES, ids=_case_id)
def test_gpu_case_inputs_take_one_clip_branch(case):
    """A condition on the inputs, checked on the reference alone: no row's probability ratio within 1e-3 of 1 +- clip, no
    normalised advantage within 1e-6 of zero — kernel and reference then take the same branch of the clip (and count the same
    rows into the clip fraction) on every row, whatever their rounding.  Also what the inputs promise: row 0 and the last row
    are in the minibatch, an all-zero observation row and the +-10 entries too."""
    c = step_case(*case)
    variants = [True] + ([False] if case in EXTERNAL_STATS_CASES else [])
    for compute in variants:
        edge, amin = _input_condition(step_ref(case, torch.float64, compute), CLIP)
        assert edge > RATIO_MARGIN and amin > ADV_MARGIN, (compute, edge, amin)
    idx, x = c["idx"], c["obs"][c["idx"]]
    assert idx.numel() == c["B"] == idx.unique().numel() and c["obs"].shape[0] > c["B"]
    assert int(idx.min()) == 0 and int(idx.max()) == c["obs"].shape[0] - 1 and not torch.equal(idx, idx.sort()[0])
    assert bool((x == 0).all(1).any()) and float(x.max()) == 10.0 and float(x.min()) == -10.0


# ------------------------------------------------------------------------------------------------ GPU plumbing
SENTINEL, PREFILL, TAIL = -12345.0, 7.0, 4096


class _Run:
    """A flattened policy on the device with its gradient vector placed inside a larger allocation (sentinel after the G
    elements, the G elements themselves pre-filled so that 'zero' means 'written'), and a FusedPPOStep on it."""

    def __init__(self, lib, O, A, seed, clip=CLIP, adam=False, hp=None):
        from myochallenge_amd.rl.fused_mlp import FlatAdam, FusedPPOStep, flatten_parameters
        self.lib, self.dev = lib, torch.device("cuda:0")
        self.pol = build_policy(O, A, seed).to(self.dev)
        self.flat = flat = flatten_parameters(self.pol)
        self.G = G = flat["g"].numel()
        self.big = torch.full((G + TAIL,), SENTINEL, device=self.dev)
        self.big[:G] = PREFILL
        flat["g"] = self.big[:G]
        for p, (off, k) in zip(flat["params"], flat["slots"]):
            p.grad = flat["g"][off:off + k].view(p.shape)
        self.step = FusedPPOStep(self.pol, lib, clip, ENT_COEF, VF_COEF)
        assert self.step.merged is not None and len(self.step.merged) == 2
        self.adam = None
        if adam:
            self.adam = self.step.adam = FlatAdam(flat, lib, 3e-4, 0.5)
            self.adam._step.copy_(torch.tensor([3, 7], dtype=torch.int32))
        self.step.hp = hp
        self.O, self.A = O, A

    def run_step(self, c, external_stats=None):
        dev = self.dev
        if not hasattr(self, "data") or self.data[0] is not c:
            self.data = (c, [c[k].to(dev) for k in ("obs", "act", "oldlp", "adv", "ret", "idx")])
        if external_stats is not None:
            self.step.external_adv_stats = True
            self.step.stats.copy_(torch.tensor(external_stats, dtype=torch.float32))
        self.step.run_indexed(*self.data[1])
        torch.cuda.synchronize()
        d = self.step._mfma[(c["B"], self.O, self.A, 256, self.G)][0]
        assert d is not None, "the step fell back to the GEMM path"
        return d

    def grads(self):
        lin = lambda seq: [m for m in seq if isinstance(m, torch.nn.Linear)]
        out = {}
        for net, trunk, head in (("pi", self.pol.mlp_extractor.policy_net, self.pol.action_net), ("vf", self.pol.mlp_extractor.value_net, self.pol.value_net)):
            l1, l2 = lin(trunk)
            for k, p in zip(GRAD_KEYS, (l1.weight, l1.bias, l2.weight, l2.bias, head.weight, head.bias)):
                out[(net, k)] = p.grad.detach().cpu().double()
        out[("pi", "log_std")] = self.pol.log_std.grad.detach().cpu().double()
        return out

    def slot_mask(self, which=None):
        """Boolean mask over the flat vector: True on parameter slots (all, or those of the listed parameters)."""
        m = torch.zeros(self.G, dtype=torch.bool, device=self.dev)
        ids = None if which is None else {id(p) for p in which}
        for p, (off, k) in zip(self.flat["params"], self.flat["slots"]):
            if ids is None or id(p) in ids:
                m[off:off + k] = True
        return m

    def loss_columns(self):
        return (self.pol.log_std, self.pol.action_net.bias, self.pol.value_net.bias)


def _note(name, kernel, twin):
    r = kernel / twin if twin > 0 else (0.0 if kernel == 0 else float("inf"))
    RATIOS_MEASURED[name] = max(RATIOS_MEASURED.get(name, 0.0), r)
    return r


def _check_against_reference(run, case, ref, twin, hp=None, label=""):
    """Gradients, acc, losses (and the hyper-parameter block's diagnostics) of the step `run` has just taken against the
    reference, bounded by the twin.  Prints kernel / twin per quantity before asserting."""
    A = case[1]
    D = twin_sizes(ref, twin)
    gr, gk = ref_grads(ref), run.grads()
    failures = []
    for key in gr:
        dk, dtw = dist(gk[key], gr[key]), dist(ref_grads(twin)[key], gr[key])
        net = key[0]
        print("%s %s %-12s kernel %.3e / %.3e  twin %.3e / %.3e  net D %.3e / %.3e  kernel/D %.2f / %.2f" % (
            label, _case_id(case), "%s.%s" % key, dk[0], dk[1], dtw[0], dtw[1], D[net][0], D[net][1],
            _note("grad norm", dk[0], D[net][0]), _note("grad max", dk[1], D[net][1])))
        if not (dk[0] <= MARGIN * D[net][0] and dk[1] <= MARGIN * D[net][1]):
            failures.append((key, dk, D[net]))
    acc = run.step.acc.detach().cpu().double()
    assert float(acc[2 * A + 3]) == 0.0                      # one spare word after the 2A + 3 columns: untouched
    scal = lambda name, k, r, t, net: (name, float(k), float(r), float(t), net)
    # The policy loss is a mean of B terms adv_i * ratio_i that cancel (normalised advantages): it moves by d(mean) / std when
    # the advantage mean moves by d(mean), and the mean is STORED in fp32 (k_mlp_prep), so kernel, twin and reference each hold
    # their own rounding of it.  With the advantages offset by +100 that one rounding is 19 % of the loss on the kernel and 3 % on
    # the twin — two single draws, whose quotient (6.1 measured) says nothing about the loss arithmetic.  The loss is therefore
    # compared with the reference evaluated AT the moments the kernel stored; those are bounded against the reference's own in
    # test_step_matches_rounding_matched_reference.  Rule and margin are unchanged, and the gradients keep the plain reference.
    km, ks = (float(v) for v in run.step.stats.detach().cpu())
    ref_m, twin_m = step_ref_at_moments(case, torch.float64, km, ks), step_ref_at_moments(case, torch.float32, km, ks)
    items = [scal("pl", acc[A], ref_m["pl"], twin_m["pl"], "pi"), scal("vl", acc[A + 1], ref["vl"], twin["vl"], "vf")]
    if hp is not None:
        from myochallenge_amd.native import HP_LAST_KL, HP_LAST_PL, HP_LAST_VL, HP_SUM_CLIPFRAC, HP_SUM_ENTLOSS, HP_SUM_KL
        h = hp.detach().cpu().double()
        items += [scal("hp.kl", h[HP_LAST_KL], ref["approx_kl"], twin["approx_kl"], "pi"), scal("hp.sum_kl", h[HP_SUM_KL], ref["approx_kl"], twin["approx_kl"], "pi"),
                  scal("hp.pl", h[HP_LAST_PL], ref_m["pl"], twin_m["pl"], "pi"), scal("hp.vl", h[HP_LAST_VL], ref["vl"], twin["vl"], "vf"),
                  scal("hp.entloss", h[HP_SUM_ENTLOSS], ref["ent_loss"], twin["ent_loss"], "pi")]
        assert float(h[HP_SUM_CLIPFRAC]) == ref["clipped_rows"] / case[2] == float(twin["clip_frac"]), (float(h[HP_SUM_CLIPFRAC]), ref["clipped_rows"])
    for name, k, r, t, net in items:
        size = max(D[net][0], abs(t - r) / abs(r))
        err = abs(k - r) / abs(r)
        print("%s %s %-12s kernel %.3e  twin %.3e  bound size %.3e  kernel/size %.2f" % (label, _case_id(case), name, err, abs(t - r) / abs(r), size, _note("scalars", err, size)))
        if not err <= MARGIN * size:
            failures.append((name, err, size))
    # acc's gradient columns: the same numbers as the log_std / head-bias gradients (log_std before the entropy term)
    for name, k, r, t in (("acc.dlogstd", acc[:A], ref["acc"][:A], twin["acc"][:A]), ("acc.dbh_pi", acc[A + 2:2 * A + 2], ref["acc"][A + 2:2 * A + 2], twin["acc"][A + 2:2 * A + 2])):
        dk = dist(k, r)
        print("%s %s %-12s kernel %.3e / %.3e  kernel/D %.2f / %.2f" % (label, _case_id(case), name, dk[0], dk[1], _note("grad norm", dk[0], D["pi"][0]), _note("grad max", dk[1], D["pi"][1])))
        if not (dk[0] <= MARGIN * D["pi"][0] and dk[1] <= MARGIN * D["pi"][1]):
            failures.append((name, dk, D["pi"]))
    assert float(acc[2 * A + 2]) == float(gk[("vf", "bh")])
    assert not failures, failures


def _check_slots_outside_the_gradients(run):
    pad = ~run.slot_mask()
    assert int(pad.sum()) > 0
    assert bool((run.big[:run.G][pad] == 0).all()), "a padding slot of the flat gradient is not zero after the step"
    assert bool((run.big[:run.G][~pad] != PREFILL).all()), "a gradient element was not written"
    assert bool((run.big[run.G:] == SENTINEL).all()), "the step wrote past the G elements of the gradient vector"


# ------------------------------------------------------------------------------------------------ GPU: myo_ppo_mlp_step
@pytest.mark.gpu
@pytest.mark.parametrize("case", STEP_CASES, ids=_case_id)
def test_step_matches_rounding_matched_reference(hip_lib, case):
    """myo_ppo_mlp_step through FusedPPOStep.run_indexed against the float64 reference, every parameter gradient, acc, the
    losses and the advantage moments; padding slots zero, nothing written past G; the same step twice is bit-identical."""
    c, ref, twin = step_case(*case), step_ref(case, torch.float64), step_ref(case, torch.float32)
    run = _Run(hip_lib, c["O"], c["A"], c["seed"])
    run.run_step(c)
    _check_slots_outside_the_gradients(run)
    g1, acc1 = run.big.clone(), run.step.acc.clone()
    _check_against_reference(run, case, ref, twin)
    # advantage moments.  fp32: a slice mean is one 16..32-term tree sum and a division (<= 2 ulp of |mean|), Chan's merge of
    # the 64 slices rounds the running mean once per slice (<= 1/2 ulp each): at most 34 ulp of |mean| however the errors fall;
    # M2 carries the same chain relative to std^2.  One ulp is at most 2^-23 of the magnitude.
    st = run.step.stats.detach().cpu().double()
    m, s = float(ref["adv_stats"][0]), float(ref["adv_stats"][1])
    tol = 34 * 2.0 ** -23 * (abs(m) + s)
    print("%s adv_stats kernel (%.9g, %.9g) ref (%.9g, %.9g) err (%.3e, %.3e) tol %.3e" % (_case_id(case), st[0], st[1], m, s, abs(st[0] - m), abs(st[1] - s), tol))
    assert abs(float(st[0]) - m) <= tol and abs(float(st[1]) - s) <= tol
    run.big[:run.G] = PREFILL
    run.run_step(c)
    assert torch.equal(run.big, g1) and torch.equal(run.step.acc, acc1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES, ids=_case_id)
def test_step_does_not_depend_on_what_the_workspace_held(hip_lib, case):
    """'Deterministic: no float atomics' and no state carried between steps: minibatch X after minibatch Y in the same
    workspace equals, bit for bit, X in a fresh zero-filled workspace."""
    cx = step_case(*case)
    cy = step_case(case[0], case[1], case[2], 100.0 if not case[3] else 0.0)     # other rows, other advantages, same shape and policy size
    a = _Run(hip_lib, cx["O"], cx["A"], cx["seed"])
    a.run_step(cy)
    y = a.big.clone()
    a.run_step(cx)
    b = _Run(hip_lib, cx["O"], cx["A"], cx["seed"])
    b.run_step(cx)
    assert torch.equal(a.flat["p"], b.flat["p"])
    assert not torch.equal(a.big, y)
    assert torch.equal(a.big, b.big) and torch.equal(a.step.acc, b.step.acc) and torch.equal(a.step.stats, b.step.stats)


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES + [(86, 39, 2048, 0.0)], ids=_case_id)
def test_both_gradient_tails_agree(hip_lib, case):
    """k_mlp_reduce_finish (step.adam set) against k_mlp_reduce + k_colmajor_finish on the same inputs: every weight and
    hidden-bias slot bit for bit (same slabs, same split order), the log_std / head-bias slots and acc within the twin-sized
    bound of the reference, the partial sums of |g|^2 equal to the written gradient's, Adam's counter advanced once."""
    c, ref, twin = step_case(*case), step_ref(case, torch.float64), step_ref(case, torch.float32)
    plain, fused = _Run(hip_lib, c["O"], c["A"], c["seed"]), _Run(hip_lib, c["O"], c["A"], c["seed"], adam=True)
    fused.adam.sq.fill_(SENTINEL)
    dp, df = plain.run_step(c), fused.run_step(c)
    assert not dp.sqnorm_part and df.sqnorm_part and df.adam_step
    cols = fused.slot_mask(fused.loss_columns())
    assert torch.equal(plain.big[:plain.G][~cols], fused.big[:fused.G][~cols])
    _check_slots_outside_the_gradients(fused)
    _check_against_reference(fused, case, ref, twin, label="tail=reduce_finish")
    _check_against_reference(plain, case, ref, twin, label="tail=reduce")
    n = hip_lib.L.myo_ppo_mlp_sqnorm_parts(c["A"])
    assert n == 256 + 2 * c["A"] + 3 and fused.adam.presummed == n
    sq = fused.adam.sq.detach().cpu().double()
    assert bool((sq[n:] == SENTINEL).all())
    want = float((fused.big[:fused.G].double() ** 2).sum())
    # a square is rounded once; it then passes at most ceil(G / 65536) serial adds in its thread, 6 shuffle adds and 2 adds
    # over the waves, each rounding a non-negative partial sum by at most 2^-24 of itself
    depth = 1 + math.ceil(fused.G / 65536) + 6 + 2
    print("%s |g|^2 partial sums %.9g, gradient %.9g, rel err %.3e, bound %.3e" % (_case_id(case), float(sq[:n].sum()), want, abs(float(sq[:n].sum()) - want) / want, depth * EPS32))
    assert abs(float(sq[:n].sum()) - want) <= depth * EPS32 * want
    assert fused.adam._step.tolist() == [7, 8]


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXTERNAL_STATS_CASES, ids=_case_id)
def test_step_with_supplied_advantage_moments(hip_lib, case):
    """compute_adv_stats = 0 with {0, 1} supplied: no normalisation happens, the moments are left as supplied."""
    c, ref, twin = step_case(*case), step_ref(case, torch.float64, False), step_ref(case, torch.float32, False)
    run = _Run(hip_lib, c["O"], c["A"], c["seed"])
    d = run.run_step(c, external_stats=(0.0, 1.0))
    assert d.compute_adv_stats == 0 and run.step.stats.tolist() == [0.0, 1.0]
    _check_slots_outside_the_gradients(run)
    _check_against_reference(run, case, ref, twin, label="stats={0,1}")
    normalised = ref_grads(step_ref(case, torch.float64))[("pi", "W2")]
    assert dist(run.grads()[("pi", "W2")], normalised)[0] > 0.1          # (the two statements are far apart on these inputs)


@pytest.mark.gpu
@pytest.mark.parametrize("adam", [False, True], ids=["tail=reduce", "tail=reduce_finish"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=_case_id)
def test_step_with_hyper_parameter_block(hip_lib, case, adam):
    """The clip range comes from the block (the descriptor's own is 0.9, the block's 0.2: bit-identical to a run without a
    block at 0.2); the block's diagnostics match the reference, the clip fraction exactly."""
    from myochallenge_amd.native import HP_CLIP, HP_COUNT, HP_STOP, HP_WORDS
    c, ref, twin = step_case(*case), step_ref(case, torch.float64), step_ref(case, torch.float32)
    hp = torch.zeros(HP_WORDS, device="cuda:0")
    hp[HP_CLIP] = CLIP
    with_block, without = _Run(hip_lib, c["O"], c["A"], c["seed"], clip=0.9, adam=adam, hp=hp), _Run(hip_lib, c["O"], c["A"], c["seed"], adam=adam)
    d = with_block.run_step(c)
    without.run_step(c)
    assert d.hp == hp.data_ptr() and abs(d.clip - 0.9) < 1e-6
    assert torch.equal(with_block.big, without.big) and torch.equal(with_block.step.acc, without.step.acc)
    _check_against_reference(with_block, case, ref, twin, hp=hp, label="hp")
    hi = hp.view(torch.int32)
    assert int(hi[HP_COUNT]) == 1 and int(hi[HP_STOP]) == 0
    if adam:
        assert with_block.adam._step.tolist() == [7, 8]


@pytest.mark.gpu
def test_step_refuses_shapes_outside_its_abi(hip_lib):
    """O in {0, 129}, A in {0, 49}, B in {512, 1000, 1536}, hidden = 128: no workspace size and MYO_E_UNSUPPORTED; a workspace
    one byte short: MYO_E_ARG — all before any launch (the gradient vector keeps what it held)."""
    from myochallenge_amd import native
    E_ARG, E_UNSUPPORTED = -1, -2
    case = (33, 17, 1024, 0.0)
    c = step_case(*case)
    run = _Run(hip_lib, c["O"], c["A"], c["seed"])
    d = run.run_step(c)
    run.big[:run.G] = PREFILL
    run.step.acc.fill_(PREFILL)
    L = hip_lib.L
    good = dict(B=1024, O=33, A=17, hidden=256)
    assert L.myo_ppo_mlp_workspace_bytes(1024, 33, 17, 256, run.G) == d.workspace_bytes > 0
    bad = [dict(O=0), dict(O=129), dict(A=0), dict(A=49), dict(B=512), dict(B=1000), dict(B=1536), dict(hidden=128)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for change in bad:
        s = dict(good, **change)
        assert L.myo_ppo_mlp_workspace_bytes(s["B"], s["O"], s["A"], s["hidden"], run.G) == -1, change
        d2 = native.PpoMlpDesc.from_buffer_copy(d)
        for k, v in change.items():
            setattr(d2, k, v)
        assert L.myo_ppo_mlp_step(C.byref(d2), stream) == E_UNSUPPORTED, change
    d2 = native.PpoMlpDesc.from_buffer_copy(d)
    d2.workspace_bytes = d.workspace_bytes - 1
    assert L.myo_ppo_mlp_step(C.byref(d2), stream) == E_ARG
    torch.cuda.synchronize()
    assert bool((run.big[:run.G] == PREFILL).all()) and bool((run.step.acc == PREFILL).all())
    assert L.myo_ppo_mlp_step(C.byref(d), stream) == 0                       # the unchanged descriptor still runs
    torch.cuda.synchronize()
    assert bool((run.big[:run.G][run.slot_mask()] != PREFILL).all())


# ------------------------------------------------------------------------------------------------ GPU: myo_ppo_mlp_rollout
ROLLOUT_SEED = 0x9E3779B97F4A7C15                # both 32-bit key words in play
DRAW0 = (5 << 32) + 12345                        # both counter words in play
T_ROWS = 3


class _Rollout:
    def __init__(self, lib, c):
        from myochallenge_amd.rl.fused_mlp import FusedPPOStep, flatten_parameters
        self.lib, self.dev, self.c = lib, torch.device("cuda:0"), c
        N, O, A = c["N"], c["O"], c["A"]
        self.pol = build_policy(O, A, c["seed"]).to(self.dev)
        self.flat = flatten_parameters(self.pol)
        self.step = FusedPPOStep(self.pol, lib, CLIP, ENT_COEF, VF_COEF)
        self.obs = c["obs"].to(self.dev)
        self.t_idx = torch.tensor([1], dtype=torch.int32, device=self.dev)
        self.draw = torch.zeros(2, dtype=torch.int64, device=self.dev)
        full = lambda *s: torch.full(s, SENTINEL, device=self.dev)
        self.obs_buf, self.act_buf, self.val_buf, self.logp_buf, self.clipped = full(T_ROWS, N, O), full(T_ROWS, N, A), full(T_ROWS, N), full(T_ROWS, N), full(N, A)
        self.d = self.step.rollout_desc(self.obs, ROLLOUT_SEED, self.draw, self.t_idx, self.obs_buf, self.act_buf, self.val_buf, self.logp_buf, self.clipped)
        assert self.d is not None, "no fused rollout path for this shape"

    def bufs(self):
        return (self.obs_buf, self.act_buf, self.val_buf, self.logp_buf)

    def run(self, deterministic):
        for b in self.bufs() + (self.clipped,):
            b.fill_(SENTINEL)
        self.draw.copy_(torch.tensor([DRAW0, -1], dtype=torch.int64))
        self.d.deterministic = int(deterministic)
        self.step.rollout_policy(self.d)
        torch.cuda.synchronize()
        for b in self.bufs():                                    # rows 0 and 2 of every [T, ...] buffer keep the sentinel
            assert bool((b[0] == SENTINEL).all()) and bool((b[2] == SENTINEL).all())
        assert self.draw.tolist() == [DRAW0, DRAW0 + 1] and self.t_idx.tolist() == [1]
        assert torch.equal(self.obs_buf[1], self.obs)
        assert torch.equal(self.clipped, self.act_buf[1].clamp(-1.0, 1.0))
        return self.act_buf[1].cpu().double(), self.val_buf[1].cpu().double(), self.logp_buf[1].cpu().double()


TWIN_ROWS = 2048


def _check_rollout_mean_value(c, pol, act, val, label=""):
    """Head mean and value against the float64 reference; the bound is MARGIN times the twin's largest absolute difference.
    On the case's 32 or 96 rows alone that figure is one of two things: ~5e-8 (summation order) when no bf16 rounding of a
    hidden activation flips in the twin, 4e-6 .. 2e-4 when one does — measured: 9 of 16 cases without a flip, and one
    (N96-O33-A32) in which the kernel flips one and the twin none, 98 times the twin.  Neither kernel nor twin is wrong there,
    and no margin covers a coin toss, so the twin is evaluated on the case's rows plus TWIN_ROWS rows drawn like them: about
    twenty flips, a stable figure for the size of one, pooled over both nets as the step's tests pool over a net's tensors."""
    params = policy_params(pol)
    g = torch.Generator().manual_seed(c["seed"] + 3)
    pool = torch.cat([c["obs"], torch.randn(TWIN_ROWS, c["O"], generator=g)])
    (mr, vr), (mt, vt) = ppo_mlp_rollout_ref(params, pool, torch.float64), ppo_mlp_rollout_ref(params, pool, torch.float32)
    size = max(float((mt.double() - mr).abs().max()), float((vt.double() - vr).abs().max()))
    mr, vr = mr[:c["N"]], vr[:c["N"]]
    em, ev = float((act - mr).abs().max()), float((val - vr).abs().max())
    print("%s N%d-O%d-A%d mean err %.3e value err %.3e twin %.3e  kernel/twin %.2f %.2f" % (label, c["N"], c["O"], c["A"], em, ev, size, _note("rollout", em, size), _note("rollout", ev, size)))
    assert em <= MARGIN * size and ev <= MARGIN * size, (em, ev, size)
    return params


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROLLOUT_CASES, ids=lambda c: "N%d-O%d-A%d" % c)
def test_rollout_policy_matches_reference_and_sampler(hip_lib, case):
    """myo_ppo_mlp_rollout, one and three workgroups per net, row 1 of three: deterministic = 1 gives the reference's head mean
    and value; deterministic = 0 adds exactly the noise of myo_rollout_sample (same seed, counters, log_std) and stores the
    log-density of that noise."""
    c = rollout_case(*case)
    N, A = c["N"], c["A"]
    r = _Rollout(hip_lib, c)
    mean, val, logp = r.run(True)
    params = _check_rollout_mean_value(c, r.pol, mean, val)
    ls = params["log_std"].double()
    # deterministic log-prob: per action one rounding of (log_std + 1/2 ln 2 pi), then at most 8 serial adds in the lane (two
    # Philox groups of four) and 3 shuffle adds, each rounding a partial sum by at most 2^-24 of sum |term|
    depth = 1 + 8 + 3
    terms = (ls + mlp_ref.HALF_LOG_2PI).abs().sum()
    want = -(ls + mlp_ref.HALF_LOG_2PI).sum()
    assert float((logp - want).abs().max()) <= depth * EPS32 * float(terms)
    # ---- sampled actions on the same inputs
    act, val2, logp2 = r.run(False)
    assert torch.equal(val2, val)
    dev = r.dev
    zeros_h = torch.zeros((N, A), dtype=torch.bfloat16, device=dev)
    draw = torch.tensor([DRAW0, -1], dtype=torch.int64, device=dev)
    noise_buf, vb, lb, cb = (torch.full(s, SENTINEL, device=dev) for s in ((T_ROWS, N, A), (T_ROWS, N), (T_ROWS, N), (N, A)))
    p = lambda t: C.c_void_p(t.data_ptr())
    hip_lib.check(hip_lib.L.myo_rollout_sample(p(zeros_h), p(zeros_h), p(r.pol.log_std.data), N, A, ROLLOUT_SEED, p(draw), p(r.t_idx),
                                               p(noise_buf), p(vb), p(lb), p(cb), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    noise = noise_buf[1].cpu().double()
    assert draw.tolist() == [DRAW0, DRAW0 + 1] and float(noise.abs().max()) > 0 and float(noise.abs().max()) < 10
    z = noise / torch.exp(ls)
    assert abs(float(z.mean())) < 5 / math.sqrt(N * A) and (N * A < 500 or abs(float(z.var()) - 1) < 0.25)      # unit normals, five sigma
    # act = fl(mean + sigma z): one rounding of the sum (<= 2^-24 |act|), and one of the product in the sampler where the
    # policy kernel fuses it into the add (<= 2^-24 |noise|)
    bound = EPS32 * (act.abs() + noise.abs())
    assert bool(((act - mean - noise).abs() <= bound).all()), float(((act - mean - noise).abs() - bound).max())
    # log-prob of the stored action, from that noise in float64.  fp32: z = (act - mean) * exp(-log_std) rounds the difference
    # and the product once each and takes the fast exponential (<= 3 ulp = 6 * 2^-24 for |log_std| < 1): 8 * 2^-24 on z, twice
    # that plus the square's own rounding on the quadratic term; then the sum as above
    zz = (act - mean) * torch.exp(-ls)
    quad, terms = 0.5 * zz * zz, 0.5 * zz * zz + (ls + mlp_ref.HALF_LOG_2PI).abs()
    want = (-quad - ls - mlp_ref.HALF_LOG_2PI).sum(-1)
    tol = 17 * EPS32 * quad.sum(-1) + depth * EPS32 * terms.sum(-1)
    assert bool(((logp2 - want).abs() <= tol).all()), float(((logp2 - want).abs() / tol).max())


@pytest.mark.gpu
def test_rollout_follows_refreshed_parameters(hip_lib):
    """After myo_ppo_mlp_rollout_refresh with changed parameters the output follows the new parameters."""
    c = rollout_case(96, 65, 5)
    r = _Rollout(hip_lib, c)
    mean0, val0, _ = r.run(True)
    g = torch.Generator().manual_seed(3)
    r.flat["p"].add_((0.02 * torch.randn(r.flat["p"].shape, generator=g)).to(r.dev))
    mean1, val1, _ = r.run(True)
    assert torch.equal(mean1, mean0) and torch.equal(val1, val0)            # the images are the kernel's parameters until refreshed
    r.step.refresh_rollout_images()
    mean2, val2, _ = r.run(True)
    assert float((mean2 - mean0).abs().max()) > 1e-2
    _check_rollout_mean_value(c, r.pol, mean2, val2, label="refreshed")


@pytest.mark.gpu
def test_rollout_refuses_shapes_outside_its_abi(hip_lib):
    from myochallenge_amd import native
    c = rollout_case(32, 33, 3)
    r = _Rollout(hip_lib, c)
    r.run(True)
    keep = [b.clone() for b in r.bufs()]
    L = hip_lib.L
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.myo_ppo_mlp_rollout_workspace_bytes(129, 3, 256) == -1 and L.myo_ppo_mlp_rollout_workspace_bytes(33, 49, 256) == -1
    assert L.myo_ppo_mlp_rollout_workspace_bytes(33, 3, 256) == r.d.workspace_bytes
    for change in (dict(N=0), dict(N=48), dict(O=129), dict(A=49)):
        d2 = native.PpoMlpRolloutDesc.from_buffer_copy(r.d)
        for k, v in change.items():
            setattr(d2, k, v)
        assert L.myo_ppo_mlp_rollout(C.byref(d2), stream) == -2, change
        assert L.myo_ppo_mlp_rollout_refresh(C.byref(d2), stream) == -2, change
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, r.bufs())) and r.draw.tolist() == [DRAW0, DRAW0 + 1]
