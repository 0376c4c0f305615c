"""Tanh policies (stable-baselines3's default activation_fn) on every fused PPO path: the matrix-core step and rollout kernels
(k_mlp_fwdbwd / k_mlp_policy, tanh instantiation: myo_ppo_mlp_step_act, myo_ppo_mlp_rollout_act), the two pointwise kernels of the
GEMM-per-layer and recurrent paths (myo_bias_act_bf16, myo_act_bwd_colsum_bf16), PPO's selection of a path from the policy's
activation, and the activation's way through a model zip.

Reference: tests/mlp_act_ref.py — mlp_ref with the activation as an argument, tanh by the kernels' formula in the working dtype,
the tanh backward (1 - h^2) on the rounded output with one more rounding.  Yardstick and margin are test_ppo_mlp_kernels.py's: per
net, D = the largest distance of the reference's float32 twin from the float64 reference over the net's gradient tensors; the
kernel stays within MARGIN = 4 x D in norm and in the largest element; losses likewise; the rollout's head mean / value within 4 x
the pooled twin's largest difference; the diagnostics a step records in the hyper-parameter block (approx_kl, the two losses, the
entropy loss) like the losses, the clip fraction exactly.  Kernel and twin share formula and rounding points; they differ in the
fp32 summation order AND in one more thing: the kernels evaluate tanh in double from their fp32 sums, the twin in float32 as the
reference's statement in its working dtype.  The twin's D therefore also counts the bf16 roundings a float32 tanh flips, which the
kernels do not make, and MARGIN x D is looser on the gradients than the same rule is for ReLU.  So the step's gradients are held
to a second bound as well: MARGIN x the per-net distance of the MIRRORED twin (mlp_act_ref activation "tanh64": float32 sums,
tanh in float64), whose only difference from the kernels is the summation order again.  Its D is 1.4 - 3.4 times smaller (actor)
and up to 12 times smaller (critic) than the plain twin's.  The losses keep the plain twin: the policy loss, a mean of cancelling
terms, is a single draw on either twin.  The pointwise
kernels are held to rule R1 of test_lstm_kernels.py (one bf16 ulp, at most 1 element in 256 off at all).

Largest kernel / twin ratios measured on an MI355X over all cases of this file (the bound is MARGIN = 4):
  gradients, |.| norm / largest element     0.93 / 1.28  (O128-A48-B1024, actor W1: kernel 5.58e-4 / 1.09e-3, the actor's D 5.97e-4 / 8.49e-4)
  the same against the mirrored twin's D    1.49 / 1.68  (O86-A39-B1024, actor W1: kernel 5.64e-4, mirror D 3.78e-4; O86-A39-B2048, actor W1: 6.94e-4, 4.14e-4)
  hyper-parameter block                     approx_kl 0.25 (O1-A1-B1024: kernel 3.11e-5, twin 7.12e-5, the actor's D 1.23e-4), policy loss as below,
                                            value loss 0.01, entropy loss 0.00; clip fraction equal (these inputs clip no row: 0 = 0)
  policy loss                               2.74  (O128-A48-B1024: kernel 1.635e-3, twin 1.329e-4, the actor's D 5.968e-4); 0.08 .. 0.46 in the other five runs
  value loss                                0.02
  rollout head mean / value                 0.15  (N32-O128-A48, mean: kernel 8.15e-5, pooled twin 5.60e-4)
  value through PPO's rollout               0.33  (256 envs x 8 steps: kernel 1.63e-4, pooled twin 4.93e-4); log-prob error / bound 0.022
  pointwise kernels: no element differs from the float64 statement (R1 share 0, both activations, both shapes)
  recurrent step against autograd of the Tanh module: cos >= 0.99997, rel <= 0.0082; against the ReLU copy cos 0.12 .. 0.83 on the trunks

The policy loss is the sensitive quantity: a mean of cancelling terms (-1.5e-3 where the terms are of order 1) whose distance from
the float64 reference comes from the FORWARD pass — bf16 roundings of first-layer activations that flip, each of which moves a
whole row of the second layer.  A float32 evaluation of tanh is good to an ulp of 1.0, not of the result, and flips 30 .. 80 of a
net's 262,144 first-layer activations (the twin's count); with the kernels evaluating it in float32 the O128-A48-B1024 policy loss
was measured at 5.47 (bare v_exp_f32 / v_rcp_f32) and 4.45 (both to about an ulp) times the bound's size.  The kernels now
evaluate it in double (csrc/myobatch.hip: myo_act_tanh), which leaves the flips of the fp32 sums alone.
"""
import ctypes as C
import copy
import functools
import json
import math
import os
import zipfile

import pytest
import torch

import mlp_act_ref as R
import mlp_ref
import test_ppo_mlp_kernels as K
from test_lstm_kernels import r1

MARGIN = K.MARGIN
CLIP, VF_COEF, ENT_COEF = K.CLIP, K.VF_COEF, K.ENT_COEF
EPS32 = K.EPS32
ACT_RELU, ACT_TANH = 0, 1

# (O, A, B): one to three head tiles, padded rows (OP = 32 / 64 / 96 / 128), both split depths (two and four k-steps per split)
TANH_STEP_CASES = [(1, 1, 1024), (33, 17, 1024), (86, 39, 1024), (128, 48, 1024), (86, 39, 2048)]
EXTERNAL_STATS_CASE = (33, 17, 1024)                 # also run with compute_adv_stats = 0
TANH_ROLLOUT_CASES = [(N, O, A) for N in (32, 96) for O, A in ((1, 1), (65, 5), (128, 48))]
RATIOS = {}

_cid = lambda c: "O%d-A%d-B%d" % c


def _note(name, kernel, twin):
    r = kernel / twin if twin > 0 else (0.0 if kernel == 0 else float("inf"))
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


# ------------------------------------------------------------------------------------------------ inputs
def build_policy(O, A, seed, activation_fn=torch.nn.Tanh):
    """test_ppo_mlp_kernels.build_policy with the activation as an argument (same draws: same weights for the same seed)."""
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        pol = ActorCriticPolicy(O, A, (256, 256), (256, 256), lstm_hidden_size=None, activation_fn=activation_fn)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in pol.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * m.weight.std(unbiased=False))
        pol.log_std.copy_(-0.5 + 0.1 * torch.randn(A, generator=g))
    return pol


def _seed(O, A, B):
    return 50000000 + 100000 * (B // 1024) + 1000 * O + 10 * A


@functools.lru_cache(maxsize=None)
def step_case(O, A, B):
    """The inputs of test_ppo_mlp_kernels.step_case, drawn the same way, from a Tanh policy (on-policy actions under the tanh net)."""
    seed = _seed(O, A, B)
    params = R.policy_params(build_policy(O, A, seed))
    g = torch.Generator().manual_seed(seed + 2)
    Rn = 2 * B + 952
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    obs = rn(Rn, O).float()
    inner = 1 + torch.randperm(Rn - 2, generator=g)[:B - 2]
    idx = torch.cat([torch.tensor([0, Rn - 1]), inner])[torch.randperm(B, generator=g)]
    obs[idx[7]] = 0.0
    obs[idx[11], 0], obs[idx[13], O - 1], obs[idx[17], O // 2] = 10.0, -10.0, 10.0
    ls = params["log_std"].double()
    mean = R.ppo_mlp_rollout_ref(params, obs, activation="tanh")[0]
    act = (mean + torch.exp(ls) * rn(Rn, A)).float()
    oldlp = (R.gaussian_logp(act.double(), mean, ls) + 0.05 * rn(Rn)).float()
    wa, wo = rn(A), rn(O) / math.sqrt(O)
    adv = (torch.tanh(((act.double() - mean) * torch.exp(-ls)) @ wa / 6) + 0.3 * rn(Rn)).float()
    ret = (torch.sin(obs.double() @ wo) + 0.1 * rn(Rn)).float()
    return {"O": O, "A": A, "B": B, "seed": seed, "params": params, "obs": obs, "act": act, "oldlp": oldlp, "adv": adv, "ret": ret, "idx": idx}


@functools.lru_cache(maxsize=None)
def step_ref(case, dt, compute_adv_stats=True, moments=(0.0, 1.0), activation="tanh"):
    c = step_case(*case)
    return R.ppo_mlp_step_ref(c["params"], c["obs"], c["act"], c["oldlp"], c["adv"], c["ret"], c["idx"], CLIP, VF_COEF, ENT_COEF,
                              compute_adv_stats=compute_adv_stats, adv_stats=moments, dt=dt, activation=activation)


# ------------------------------------------------------------------------------------------------ CPU: the reference
def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", [(33, 17, 1024, 0.0), (86, 39, 1024, 0.0)], ids=K._case_id)
def test_relu_branch_of_the_reference_is_mlp_ref_bit_for_bit(case, dt):
    c = K.step_case(*case)
    args = (c["params"], c["obs"], c["act"], c["oldlp"], c["adv"], c["ret"], c["idx"], CLIP, VF_COEF, ENT_COEF)
    assert _same(R.ppo_mlp_step_ref(*args, dt=dt, activation="relu"), mlp_ref.ppo_mlp_step_ref(*args, dt=dt))
    assert _same(R.ppo_mlp_step_ref(*args, compute_adv_stats=False, adv_stats=(0.1, 0.9), dt=dt, activation="relu"),
                 mlp_ref.ppo_mlp_step_ref(*args, compute_adv_stats=False, adv_stats=(0.1, 0.9), dt=dt))
    assert _same(R.ppo_mlp_rollout_ref(c["params"], c["obs"][:96], dt, activation="relu"), mlp_ref.ppo_mlp_rollout_ref(c["params"], c["obs"][:96], dt))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("case", [(33, 17, 1024), (86, 39, 1024)], ids=_cid)
def test_tanh_reference_without_rounding_is_float64_autograd_of_the_module(case, normalize):
    """rnd = identity, float64: gradients, losses and diagnostics equal autograd through the layers of an
    ActorCriticPolicy(activation_fn=nn.Tanh) in float64, to the 1e-10 test_ppo_mlp_kernels.py asks of the ReLU reference."""
    import torch.nn.functional as F
    c = step_case(*case)
    res = R.ppo_mlp_step_ref(c["params"], c["obs"], c["act"], c["oldlp"], c["adv"], c["ret"], c["idx"], CLIP, VF_COEF, ENT_COEF,
                             compute_adv_stats=normalize, adv_stats=(0.0, 1.0), dt=torch.float64, rnd=mlp_ref.identity, activation="tanh")
    pol = build_policy(c["O"], c["A"], c["seed"]).double()
    assert pol.activation_fn is torch.nn.Tanh and isinstance(pol.mlp_extractor.policy_net[1], torch.nn.Tanh)
    x, a, olp, ad, rt = (t[c["idx"]].double() for t in (c["obs"], c["act"], c["oldlp"], c["adv"], c["ret"]))
    mean = pol.action_net(pol.mlp_extractor.policy_net(x))
    values = pol.value_net(pol.mlp_extractor.value_net(x))[:, 0]
    ls = pol.log_std
    logp = (-0.5 * ((a - mean) ** 2) / torch.exp(2 * ls) - ls - 0.5 * math.log(2 * math.pi)).sum(-1)
    m, s = (ad.mean(), ad.std()) if normalize else (0.0, 1.0)
    an = (ad - m) / (s + 1e-8)
    ratio = torch.exp(logp - olp)
    pl = -torch.min(an * ratio, an * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
    vl = F.mse_loss(values, rt)
    ent_loss = -(0.5 + 0.5 * math.log(2 * math.pi) + ls).sum()
    (pl + ENT_COEF * ent_loss + VF_COEF * vl).backward()
    lin = lambda seq: [mod for mod in seq if isinstance(mod, torch.nn.Linear)]
    want = {("pi", "log_std"): ls.grad}
    for net, trunk, head in (("pi", pol.mlp_extractor.policy_net, pol.action_net), ("vf", pol.mlp_extractor.value_net, pol.value_net)):
        l1, l2 = lin(trunk)
        for k, p in zip(K.GRAD_KEYS, (l1.weight, l1.bias, l2.weight, l2.bias, head.weight, head.bias)):
            want[(net, k)] = p.grad
    mine = K.ref_grads(res)
    assert set(mine) == set(want)
    for key, g in want.items():
        assert mine[key].shape == g.shape and K.dist(mine[key], g)[0] <= 1e-10, (key, K.dist(mine[key], g))
    lr = (logp - olp).detach()
    for name, w in (("pl", pl), ("vl", vl), ("approx_kl", ((ratio - 1) - lr).mean()), ("ent_loss", ent_loss)):
        assert abs(float(res[name]) - float(w.detach())) <= 1e-10 * abs(float(w.detach())), name


@pytest.mark.parametrize("case", TANH_STEP_CASES, ids=_cid)
def test_tanh_gpu_case_inputs_take_one_clip_branch(case):
    """test_ppo_mlp_kernels.py's input condition on the Tanh cases, asserted on the reference alone: every ratio at least
    RATIO_MARGIN from 1 +- clip, every normalised advantage at least ADV_MARGIN from 0 (the seeds are chosen so)."""
    variants = [True] + ([False] if case == EXTERNAL_STATS_CASE else [])
    for compute in variants:
        edge, amin = K._input_condition(step_ref(case, torch.float64, compute), CLIP)
        assert edge > K.RATIO_MARGIN and amin > K.ADV_MARGIN, (compute, edge, amin)
    c = step_case(*case)
    x = c["obs"][c["idx"]]
    assert bool((x == 0).all(1).any()) and float(x.max()) == 10.0 and float(x.min()) == -10.0
    h = step_ref(case, torch.float64)["hidden"]["pi"]
    assert float(h[0].abs().max()) <= 1.0 and float(h[0].abs().max()) > 0.9          # a tanh net: bounded, and driven towards saturation


# ------------------------------------------------------------------------------------------------ CPU: policy, zip, torch statement
def _small_policy(activation_fn, seed=0, recurrent=False):
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    torch.manual_seed(seed)
    pol = ActorCriticPolicy(11, 3, (16, 12), (8, 8), lstm_hidden_size=8 if recurrent else None, activation_fn=activation_fn)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(0.3 * torch.randn_like(p))
    return pol


def test_activation_code_is_the_one_mapping():
    from myochallenge_amd import native
    from myochallenge_amd.rl.fused_mlp import activation_code
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    assert (native.ACT_RELU, native.ACT_TANH) == (ACT_RELU, ACT_TANH)
    assert ActorCriticPolicy(5, 2).activation_fn is torch.nn.ReLU                       # the default stays ReLU
    assert activation_code(_small_policy(torch.nn.ReLU)) == ACT_RELU and activation_code(_small_policy(torch.nn.Tanh)) == ACT_TANH
    assert activation_code(_small_policy(torch.nn.ELU)) is None
    assert activation_code(ActorCriticPolicy(5, 2, (), (), lstm_hidden_size=8, activation_fn=torch.nn.ELU)) == ACT_RELU      # no hidden MLP layer
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "myobatch.h")).read()
    assert "#define MYO_ACT_RELU 0" in src and "#define MYO_ACT_TANH 1" in src


@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_zip_round_trip_keeps_the_activation(tmp_path, golden_dir, recurrent):
    from myochallenge_amd.rl.sb3_zip import load_policy, read_zip, save_sb3_zip
    pol = _small_policy(torch.nn.Tanh, recurrent=recurrent)
    path = str(tmp_path / "tanh.zip")
    save_sb3_zip(path, pol, {}, n_envs=4)
    back, data = load_policy(path)
    assert back.activation_fn is torch.nn.Tanh and isinstance(back.mlp_extractor.policy_net[1], torch.nn.Tanh)
    assert data["policy_kwargs"]["activation_fn"] == "<class 'torch.nn.modules.activation.Tanh'>"
    obs = torch.randn(6, 11, generator=torch.Generator().manual_seed(1)).numpy()
    a0, a1 = pol.predict(obs, deterministic=True)[0], back.predict(obs, deterministic=True)[0]
    assert (a0 == a1).all() and abs(a0).max() > 0
    relu = _small_policy(torch.nn.ReLU, recurrent=recurrent)
    relu.load_state_dict(pol.state_dict())
    assert not (relu.predict(obs, deterministic=True)[0] == a0).all()                    # (the activation matters on these inputs)
    # no activation_fn entry: what stable-baselines3 builds without one, nn.Tanh
    z = zipfile.ZipFile(path)
    members = {n: z.read(n) for n in z.namelist()}
    d = json.loads(members["data"])
    del d["policy_kwargs"]["activation_fn"]
    members["data"] = json.dumps(d).encode()
    bare = str(tmp_path / "bare.zip")
    with zipfile.ZipFile(bare, "w") as out:
        for n, b in members.items():
            out.writestr(n, b)
    assert "activation_fn" not in read_zip(bare)[0]["policy_kwargs"]
    assert load_policy(bare)[0].activation_fn is torch.nn.Tanh
    # any other torch.nn activation loads as itself; a name torch.nn does not have is an error
    for name, want in (("<class 'torch.nn.modules.activation.ELU'>", torch.nn.ELU), ("<class 'torch.nn.modules.activation.ReLU'>", torch.nn.ReLU)):
        d["policy_kwargs"]["activation_fn"] = name
        members["data"] = json.dumps(d).encode()
        with zipfile.ZipFile(bare, "w") as out:
            for n, b in members.items():
                out.writestr(n, b)
        assert load_policy(bare)[0].activation_fn is want
    for name in ("<class 'somewhere.Swoosh'>", "<class 'torch.nn.modules.linear.Linear'>", "<class 'os.system'>"):
        d["policy_kwargs"]["activation_fn"] = name
        members["data"] = json.dumps(d).encode()
        with zipfile.ZipFile(bare, "w") as out:
            for n, b in members.items():
                out.writestr(n, b)
        with pytest.raises(ValueError):
            load_policy(bare)
    # a ReLU policy still writes the string of the recorded schema
    schema = json.load(open(os.path.join(golden_dir, "sb3_zip_schema.json")))
    rpath = str(tmp_path / "relu.zip")
    save_sb3_zip(rpath, relu, {}, n_envs=4)
    rback, rdata = load_policy(rpath)
    assert rdata["policy_kwargs"]["activation_fn"] == "<class 'torch.nn.modules.activation.ReLU'>" and rback.activation_fn is torch.nn.ReLU
    assert "<class 'torch.nn.modules.activation.ReLU'>" in json.dumps(schema)


def test_policy_from_state_dict_defaults_to_relu():
    from myochallenge_amd.rl.sb3_zip import policy_from_state_dict
    pol = _small_policy(torch.nn.Tanh)
    assert policy_from_state_dict(pol.state_dict()).activation_fn is torch.nn.ReLU
    assert policy_from_state_dict(pol.state_dict(), activation_fn=torch.nn.Tanh).activation_fn is torch.nn.Tanh


@pytest.mark.parametrize("act", [torch.nn.Tanh, torch.nn.ReLU], ids=["tanh", "relu"])
def test_torch_statement_of_the_step_uses_the_policy_activation(act):
    """ppo_mlp_step_grads (CPU, fp32) on the policy's own activation against autograd of the module: test_rl.py's check of the
    ReLU statement, its tolerances (fp32 summation order)."""
    import numpy as np
    from myochallenge_amd.rl.fused_mlp import ppo_mlp_step_grads
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    from myochallenge_amd.rl.ppo import PPO, PPOConfig
    torch.manual_seed(0)
    pol = ActorCriticPolicy(86, 39, (64, 48), (32, 32), lstm_hidden_size=None, activation_fn=act)
    B = 96
    obs, actions = torch.randn(B, 86), torch.randn(B, 39) * 0.3
    with torch.no_grad():
        oldlp = pol.evaluate_actions(obs, actions)[1] + torch.randn(B) * 0.3
    adv, ret = torch.randn(B), torch.randn(B)

    class E:
        num_envs, obs_dim, act_dim, device = 4, 86, 39, torch.device("cpu")
    algo = PPO(E(), pol, PPOConfig(n_steps=2, clip_range=0.2, ent_coef=0.01, vf_coef=0.7, bf16=False))
    v, lp, ent = pol.evaluate_actions(obs, actions)
    loss, pl_ref, vl_ref = algo._loss(v, lp, ent, oldlp, adv, ret)
    pol.zero_grad(); loss.backward()
    ref = [p.grad.clone() for p in pol.parameters()]
    for p in pol.parameters():
        p.grad = None
    pl, vl = ppo_mlp_step_grads(pol, obs, actions, oldlp, adv, ret, 0.2, 0.01, 0.7, True, bf16=False, split_k=4)
    assert abs(float(pl - pl_ref)) < 1e-5 and abs(float(vl - vl_ref)) < 1e-5
    for p, r in zip(pol.parameters(), ref):
        np.testing.assert_allclose(p.grad.numpy(), r.numpy(), rtol=2e-4, atol=5e-5)
    elu = ActorCriticPolicy(86, 39, (64, 48), (32, 32), lstm_hidden_size=None, activation_fn=torch.nn.ELU)
    with pytest.raises(ValueError):
        ppo_mlp_step_grads(elu, obs, actions, oldlp, adv, ret, 0.2, 0.01, 0.7, True, bf16=False, split_k=4)


def test_new_entry_points_check_their_arguments():
    """The four *_act symbols are exported by the product library; NULL pointers and activation code 7 give MYO_E_ARG (-1) with a
    message, before any HIP call (loading needs libamdhip64 only); the descriptors keep their sizes."""
    from myochallenge_amd import native
    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libmyobatch.so not built in this checkout (run __graft_entry__.build())")
    new = ("myo_ppo_mlp_step_act", "myo_ppo_mlp_rollout_act", "myo_bias_act_bf16", "myo_act_bwd_colsum_bf16")
    assert set(new) <= set(native.EXPORTED_SYMBOLS)
    lib = native.NativeLib(native.LIB_PATH)
    L = lib.L
    for sym in new:
        assert hasattr(L, sym), sym
    assert C.sizeof(native.PpoMlpDesc) == 264 and C.sizeof(native.PpoMlpRolloutDesc) == 224
    somewhere = 4096          # stands for a device address: an argument error returns before anything is read through it
    full = native.PpoMlpDesc(B=1024, O=33, A=17, hidden=256, G=1 << 20, workspace_bytes=1 << 40, **{
        k: somewhere for k in ("obs", "act", "oldlp", "adv", "ret", "idx", "params", "grads", "adv_stats", "acc", "workspace")})
    roll = native.PpoMlpRolloutDesc(N=32, O=33, A=17, hidden=256, workspace_bytes=1 << 40, **{
        k: somewhere for k in ("obs", "params", "draw_counter", "t_idx", "act_buf", "val_buf", "logp_buf", "clipped", "workspace")})
    checks = [
        (L.myo_ppo_mlp_step_act, (None, 0, ACT_TANH, None), b"null"),
        (L.myo_ppo_mlp_step_act, (C.byref(native.PpoMlpDesc()), 1, ACT_TANH, None), b"null"),
        (L.myo_ppo_mlp_step_act, (C.byref(full), 0, 7, None), b"activation code 7"),
        (L.myo_ppo_mlp_step_act, (C.byref(full), 1, -1, None), b"activation code -1"),
        (L.myo_ppo_mlp_rollout_act, (None, ACT_TANH, None), b"null"),
        (L.myo_ppo_mlp_rollout_act, (C.byref(native.PpoMlpRolloutDesc()), ACT_RELU, None), b"null"),
        (L.myo_ppo_mlp_rollout_act, (C.byref(roll), 7, None), b"activation code 7"),
        (L.myo_bias_act_bf16, (None, None, 2, 16, 256, ACT_TANH, None), b"bad arguments"),
        (L.myo_bias_act_bf16, (somewhere, somewhere, 2, 16, 255, ACT_TANH, None), b"bad arguments"),
        (L.myo_bias_act_bf16, (somewhere, somewhere, 2, 16, 256, 7, None), b"activation code 7"),
        (L.myo_act_bwd_colsum_bf16, (None, None, 64, 256, None, ACT_TANH, None), b"rows must be"),
        (L.myo_act_bwd_colsum_bf16, (somewhere, somewhere, 48, 256, somewhere, ACT_TANH, None), b"rows must be"),
        (L.myo_act_bwd_colsum_bf16, (somewhere, somewhere, 64, 256, somewhere, 7, None), b"activation code 7"),
    ]
    for fn, args, msg in checks:
        assert fn(*args) == -1, fn.__name__
        assert msg in L.myo_last_error(), (fn.__name__, L.myo_last_error())


# ------------------------------------------------------------------------------------------------ pointwise kernels: inputs, twin
POINTWISE_SHAPES = [(2, 32, 256), (2, 32, 64)]           # (groups, rows, cols)


@functools.lru_cache(maxsize=None)
def pointwise_case(G, Rw, Cc):
    """bf16-valued inputs: pre-activations N(0, 1.5) (tanh from its linear part into saturation), +-40 (exact saturation), exact
    zeros; biases N(0, 0.5); incoming gradients N(0, 1e-3) with zeros."""
    g = torch.Generator().manual_seed(1000 * Cc + Rw + G)
    h = mlp_ref.round_bf16(1.5 * torch.randn(G, Rw, Cc, generator=g))
    h[0, 0, :4] = torch.tensor([40.0, -40.0, 0.0, -0.0])
    bias = mlp_ref.round_bf16(0.5 * torch.randn(G, Cc, generator=g))
    bias[0, :4] = 0.0
    dy = mlp_ref.round_bf16(1e-3 * torch.randn(G * Rw, Cc, generator=g))
    dy[1, :8] = 0.0
    return h, bias, dy


@pytest.mark.parametrize("activation", R.ACTIVATIONS)
@pytest.mark.parametrize("shape", POINTWISE_SHAPES, ids=lambda s: "G%d-R%d-C%d" % s)
def test_pointwise_float32_twin_is_inside_the_cap(shape, activation):
    """On the chosen inputs the float32 statement alone meets rule R1 against the float64 statement (forward and backward), tanh
    saturates to exactly +-1, and tanh(0) = 0."""
    h, bias, dy = pointwise_case(*shape)
    ref, twin = R.bias_act_ref(h, bias, activation), R.bias_act_ref(h, bias, activation, dt=torch.float32)
    assert not r1("act", twin, ref, "twin " + activation)
    if activation == "tanh":
        assert ref[0, 0, :4].tolist() == [1.0, -1.0, 0.0, 0.0] and twin[0, 0, :4].tolist() == [1.0, -1.0, 0.0, 0.0]
        assert float(ref.abs().max()) == 1.0
    out = ref.reshape(dy.shape)
    assert not r1("dact", R.act_bwd_ref(dy, out, activation, dt=torch.float32), R.act_bwd_ref(dy, out, activation), "twin " + activation)


# ------------------------------------------------------------------------------------------------ GPU plumbing
class _Run(K._Run):
    """test_ppo_mlp_kernels._Run on a policy with the given activation; `resident`: the step runs with resident operand images."""

    def __init__(self, lib, O, A, seed, activation_fn=torch.nn.Tanh, resident=False, clip=CLIP, adam=False, hp=None):
        from myochallenge_amd.rl.fused_mlp import FlatAdam, FusedPPOStep, flatten_parameters
        self.lib, self.dev = lib, torch.device("cuda:0")
        self.pol = build_policy(O, A, seed, activation_fn).to(self.dev)
        self.flat = flat = flatten_parameters(self.pol)
        self.G = G = flat["g"].numel()
        self.big = torch.full((G + K.TAIL,), K.SENTINEL, device=self.dev)
        self.big[:G] = K.PREFILL
        flat["g"] = self.big[:G]
        for p, (off, k) in zip(flat["params"], flat["slots"]):
            p.grad = flat["g"][off:off + k].view(p.shape)
        self.step = FusedPPOStep(self.pol, lib, clip, ENT_COEF, VF_COEF)
        assert self.step.merged is not None and len(self.step.merged) == 2
        self.adam = None
        if resident:
            self.adam = self.step.resident_adam = FlatAdam(flat, lib, 3e-4, 0.5)
        elif adam:                                       # (the one-rank tail: k_mlp_reduce_finish records the minibatch)
            self.adam = self.step.adam = FlatAdam(flat, lib, 3e-4, 0.5)
            self.adam._step.copy_(torch.tensor([3, 7], dtype=torch.int32))
        self.step.hp = hp
        self.O, self.A = O, A


def _check_step(run, case, ref, twin, moments_given, label, hp=None, mirror=None):
    """test_ppo_mlp_kernels._check_against_reference for a Tanh case: gradients, acc columns and losses of the step `run` has
    taken — and, with a hyper-parameter block, the diagnostics it recorded there — bounded by the twin (the policy loss against
    the reference at the moments the kernel stored, as there); the clip fraction has to be the reference's exactly.
    mirror: the float32 twin that evaluates tanh in double like the kernels (activation "tanh64") — the gradients have to stay
    within MARGIN times ITS per-net distance as well, which is the smaller of the two: the plain twin's D also counts the bf16
    roundings a float32 tanh flips and the kernels do not."""
    A = case[1]
    D = K.twin_sizes(ref, twin)
    gr, gt, gk = K.ref_grads(ref), K.ref_grads(twin), run.grads()
    failures = []
    for key in gr:
        dk, dtw = K.dist(gk[key], gr[key]), K.dist(gt[key], gr[key])
        net = key[0]
        print("%s %s %-12s kernel %.3e / %.3e  twin %.3e / %.3e  net D %.3e / %.3e  kernel/D %.2f / %.2f" % (
            label, _cid(case), "%s.%s" % key, dk[0], dk[1], dtw[0], dtw[1], D[net][0], D[net][1],
            _note("grad norm", dk[0], D[net][0]), _note("grad max", dk[1], D[net][1])))
        if not (dk[0] <= MARGIN * D[net][0] and dk[1] <= MARGIN * D[net][1]):
            failures.append((key, dk, D[net]))
    if mirror is not None:
        Dm = K.twin_sizes(ref, mirror)
        for key in gr:
            dk, net = K.dist(gk[key], gr[key]), key[0]
            print("%s %s %-12s kernel %.3e / %.3e  mirror D %.3e / %.3e  kernel/mirror D %.2f / %.2f" % (
                label, _cid(case), "%s.%s" % key, dk[0], dk[1], Dm[net][0], Dm[net][1], _note("grad norm, mirror", dk[0], Dm[net][0]), _note("grad max, mirror", dk[1], Dm[net][1])))
            if not (dk[0] <= MARGIN * Dm[net][0] and dk[1] <= MARGIN * Dm[net][1]):
                failures.append(("mirror", key, dk, Dm[net]))
    acc = run.step.acc.detach().cpu().double()
    assert float(acc[2 * A + 3]) == 0.0
    km, ks = (float(v) for v in run.step.stats.detach().cpu())
    if moments_given:
        ref_m, twin_m = ref, twin
    else:
        ref_m, twin_m = step_ref(case, torch.float64, False, (km, ks)), step_ref(case, torch.float32, False, (km, ks))
    items = [("pl", acc[A], ref_m["pl"], twin_m["pl"], "pi"), ("vl", acc[A + 1], ref["vl"], twin["vl"], "vf")]
    if hp is not None:
        from myochallenge_amd.native import HP_LAST_KL, HP_LAST_PL, HP_LAST_VL, HP_SUM_CLIPFRAC, HP_SUM_ENTLOSS, HP_SUM_KL
        h = hp.detach().cpu().double()
        items += [("hp.kl", h[HP_LAST_KL], ref["approx_kl"], twin["approx_kl"], "pi"), ("hp.sum_kl", h[HP_SUM_KL], ref["approx_kl"], twin["approx_kl"], "pi"),
                  ("hp.pl", h[HP_LAST_PL], ref_m["pl"], twin_m["pl"], "pi"), ("hp.vl", h[HP_LAST_VL], ref["vl"], twin["vl"], "vf"),
                  ("hp.entloss", h[HP_SUM_ENTLOSS], ref["ent_loss"], twin["ent_loss"], "pi")]
        assert float(h[HP_SUM_CLIPFRAC]) == ref["clipped_rows"] / case[2] == float(twin["clip_frac"]), (float(h[HP_SUM_CLIPFRAC]), ref["clipped_rows"])
    for name, k, r, t, net in items:
        k, r, t = float(k), float(r), float(t)
        size, err = max(D[net][0], abs(t - r) / abs(r)), abs(k - r) / abs(r)
        print("%s %s %-12s kernel %.3e  twin %.3e  bound size %.3e  kernel/size %.2f" % (label, _cid(case), name, err, abs(t - r) / abs(r), size, _note("scalars", err, size)))
        if not err <= MARGIN * size:
            failures.append((name, err, size))
    for name, k, r in (("acc.dlogstd", acc[:A], ref["acc"][:A]), ("acc.dbh_pi", acc[A + 2:2 * A + 2], ref["acc"][A + 2:2 * A + 2])):
        dk = K.dist(k, r)
        print("%s %s %-12s kernel %.3e / %.3e  kernel/D %.2f / %.2f" % (label, _cid(case), name, dk[0], dk[1], _note("grad norm", dk[0], D["pi"][0]), _note("grad max", dk[1], D["pi"][1])))
        if not (dk[0] <= MARGIN * D["pi"][0] and dk[1] <= MARGIN * D["pi"][1]):
            failures.append((name, dk, D["pi"]))
    assert float(acc[2 * A + 2]) == float(gk[("vf", "bh")])
    assert not failures, failures


# ------------------------------------------------------------------------------------------------ GPU: myo_ppo_mlp_step_act
@pytest.mark.gpu
@pytest.mark.parametrize("case,external", [(c, False) for c in TANH_STEP_CASES] + [(EXTERNAL_STATS_CASE, True)],
                         ids=[_cid(c) for c in TANH_STEP_CASES] + [_cid(EXTERNAL_STATS_CASE) + "-stats={0,1}"])
def test_tanh_step_matches_reference_stateless_and_resident(hip_lib, case, external):
    """myo_ppo_mlp_step_act with MYO_ACT_TANH through FusedPPOStep.run_indexed, stateless and with resident operand images: each
    against the float64 reference, and the two bit for bit (gradient vector, acc, advantage moments).  The ReLU reference on the
    same inputs is far away.  One case also runs with compute_adv_stats = 0 and the moments {0, 1} supplied.
    Measured: gradients within 1.28 x their twin figure, the policy loss within 2.74 x (O128-A48-B1024), see the module docstring."""
    c = step_case(*case)
    ref, twin = step_ref(case, torch.float64, not external), step_ref(case, torch.float32, not external)
    mirror = step_ref(case, torch.float32, not external, activation="tanh64")
    runs = {}
    for resident in (False, True):
        run = runs[resident] = _Run(hip_lib, c["O"], c["A"], c["seed"], resident=resident)
        assert run.step.act == ACT_TANH
        d = run.run_step(c, external_stats=(0.0, 1.0) if external else None)
        assert d.compute_adv_stats == (0 if (external or resident) else 1)
        K._check_slots_outside_the_gradients(run)
        _check_step(run, case, ref, twin, external, "resident" if resident else "stateless", mirror=mirror)
    a, b = runs[False], runs[True]
    assert b.adam.images is not None and torch.equal(a.flat["p"], b.flat["p"])
    assert torch.equal(a.big, b.big) and torch.equal(a.step.acc, b.step.acc) and torch.equal(a.step.stats, b.step.stats)
    if not external:
        st = a.step.stats.detach().cpu().double()
        m, s = float(ref["adv_stats"][0]), float(ref["adv_stats"][1])
        tol = 34 * 2.0 ** -23 * (abs(m) + s)           # (test_ppo_mlp_kernels.py: the fp32 chain of k_adv_moments / k_mlp_prep)
        assert abs(float(st[0]) - m) <= tol and abs(float(st[1]) - s) <= tol
    relu = K.ref_grads(step_ref(case, torch.float64, not external, activation="relu"))[("pi", "W2")]
    assert K.dist(a.grads()[("pi", "W2")], relu)[0] > 0.1


HP_CASES = [(1, 1, 1024), (128, 48, 1024)]              # one and three head tiles; the widest loss phase (A = 48)


@pytest.mark.gpu
@pytest.mark.parametrize("adam", [False, True], ids=["tail=reduce", "tail=reduce_finish"])
@pytest.mark.parametrize("case", HP_CASES, ids=_cid)
def test_tanh_step_with_hyper_parameter_block(hip_lib, case, adam):
    """test_ppo_mlp_kernels.test_step_with_hyper_parameter_block on the Tanh instantiation: the clip range comes from the block
    (the descriptor's own is 0.9, the block's 0.2: bit-identical to a run without a block at 0.2); approx_kl, the policy and value
    loss and the entropy loss the step records in the block are bounded by the twin like the losses, the clip fraction equals the
    Tanh reference's exactly; one minibatch recorded, no stop, Adam's counter advanced once on the one-rank tail."""
    from myochallenge_amd.native import HP_CLIP, HP_COUNT, HP_STOP, HP_WORDS
    c, ref, twin = step_case(*case), step_ref(case, torch.float64), step_ref(case, torch.float32)
    hp = torch.zeros(HP_WORDS, device="cuda:0")
    hp[HP_CLIP] = CLIP
    with_block = _Run(hip_lib, c["O"], c["A"], c["seed"], clip=0.9, adam=adam, hp=hp)
    without = _Run(hip_lib, c["O"], c["A"], c["seed"], adam=adam)
    assert with_block.step.act == ACT_TANH
    d = with_block.run_step(c)
    without.run_step(c)
    assert d.hp == hp.data_ptr() and abs(d.clip - 0.9) < 1e-6
    assert torch.equal(with_block.big, without.big) and torch.equal(with_block.step.acc, without.step.acc)
    _check_step(with_block, case, ref, twin, False, "hp", hp=hp)
    hi = hp.view(torch.int32)
    assert int(hi[HP_COUNT]) == 1 and int(hi[HP_STOP]) == 0
    if adam:
        assert with_block.adam._step.tolist() == [7, 8]


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [False, True], ids=["stateless", "resident"])
def test_step_act_with_relu_is_the_existing_entry_point_bit_for_bit(hip_lib, resident):
    """myo_ppo_mlp_step_act(d, resident, MYO_ACT_RELU) against myo_ppo_mlp_step / myo_ppo_mlp_step_resident on one descriptor:
    the gradient vector, acc and the advantage moments."""
    case = (86, 39, 1024, 0.0)
    c = K.step_case(*case)
    run = _Run(hip_lib, c["O"], c["A"], c["seed"], activation_fn=torch.nn.ReLU, resident=resident)
    assert run.step.act == ACT_RELU
    d = run.run_step(c)                               # (through FusedPPOStep: the _act entry point with the policy's code)
    got = (run.big.clone(), run.step.acc.clone(), run.step.stats.clone())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = hip_lib.L
    for fn, args in ((L.myo_ppo_mlp_step_resident if resident else L.myo_ppo_mlp_step, (C.byref(d), stream)),
                     (L.myo_ppo_mlp_step_act, (C.byref(d), int(resident), ACT_RELU, stream))):
        run.big[:run.G] = K.PREFILL
        run.step.acc.zero_()
        hip_lib.check(fn(*args))
        torch.cuda.synchronize()
        assert torch.equal(run.big, got[0]) and torch.equal(run.step.acc, got[1]) and torch.equal(run.step.stats, got[2]), fn.__name__
    ref = K.ref_grads(K.step_ref(case, torch.float64))[("pi", "W2")]
    assert K.dist(run.grads()[("pi", "W2")], ref)[0] < 1e-2


# ------------------------------------------------------------------------------------------------ GPU: myo_ppo_mlp_rollout_act
class _Rollout(K._Rollout):
    def __init__(self, lib, c, activation_fn=torch.nn.Tanh):
        from myochallenge_amd.rl.fused_mlp import FusedPPOStep, flatten_parameters
        self.lib, self.dev, self.c = lib, torch.device("cuda:0"), c
        N, O, A = c["N"], c["O"], c["A"]
        self.pol = build_policy(O, A, c["seed"], activation_fn).to(self.dev)
        self.flat = flatten_parameters(self.pol)
        self.step = FusedPPOStep(self.pol, lib, CLIP, ENT_COEF, VF_COEF)
        self.obs = c["obs"].to(self.dev)
        self.t_idx = torch.tensor([1], dtype=torch.int32, device=self.dev)
        self.draw = torch.zeros(2, dtype=torch.int64, device=self.dev)
        full = lambda *s: torch.full(s, K.SENTINEL, device=self.dev)
        self.obs_buf, self.act_buf, self.val_buf, self.logp_buf, self.clipped = full(K.T_ROWS, N, O), full(K.T_ROWS, N, A), full(K.T_ROWS, N), full(K.T_ROWS, N), full(N, A)
        self.d = self.step.rollout_desc(self.obs, K.ROLLOUT_SEED, self.draw, self.t_idx, self.obs_buf, self.act_buf, self.val_buf, self.logp_buf, self.clipped)
        assert self.d is not None, "no fused rollout path for this shape"


def rollout_twin_size(params, obs, O, seed, activation):
    """test_ppo_mlp_kernels._check_rollout_mean_value's yardstick: the float32 twin's largest absolute difference from the
    float64 reference in head mean and value, pooled over both nets and over the rows plus TWIN_ROWS more drawn like them."""
    g = torch.Generator().manual_seed(seed + 3)
    pool = torch.cat([obs, torch.randn(K.TWIN_ROWS, O, generator=g)])
    (mr, vr), (mt, vt) = R.ppo_mlp_rollout_ref(params, pool, torch.float64, activation=activation), R.ppo_mlp_rollout_ref(params, pool, torch.float32, activation=activation)
    size = max(float((mt.double() - mr).abs().max()), float((vt.double() - vr).abs().max()))
    return size, mr[:obs.shape[0]], vr[:obs.shape[0]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", TANH_ROLLOUT_CASES, ids=lambda c: "N%d-O%d-A%d" % c)
def test_tanh_rollout_matches_reference(hip_lib, case):
    """myo_ppo_mlp_rollout_act with MYO_ACT_TANH, deterministic: head mean and value against the reference under the pooled-twin
    bound; the ReLU reference is far outside it; MYO_ACT_RELU on the same descriptor is myo_ppo_mlp_rollout bit for bit."""
    c = K.rollout_case(*case)
    r = _Rollout(hip_lib, c)
    assert r.step.act == ACT_TANH
    mean, val, _ = r.run(True)
    params = R.policy_params(r.pol)
    size, mr, vr = rollout_twin_size(params, c["obs"], c["O"], c["seed"], "tanh")
    em, ev = float((mean - mr).abs().max()), float((val - vr).abs().max())
    print("tanh N%d-O%d-A%d mean err %.3e value err %.3e twin %.3e  kernel/twin %.2f %.2f" % (c["N"], c["O"], c["A"], em, ev, size, _note("rollout", em, size), _note("rollout", ev, size)))
    assert em <= MARGIN * size and ev <= MARGIN * size, (em, ev, size)
    m_relu, v_relu = R.ppo_mlp_rollout_ref(params, c["obs"], activation="relu")
    assert float((mean - m_relu).abs().max()) > 10 * MARGIN * size
    # the two ReLU entry points on this descriptor
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for fn, args in ((hip_lib.L.myo_ppo_mlp_rollout, (C.byref(r.d), stream)), (hip_lib.L.myo_ppo_mlp_rollout_act, (C.byref(r.d), ACT_RELU, stream))):
        hip_lib.check(fn(*args))
        torch.cuda.synchronize()
        outs.append((r.act_buf.clone(), r.val_buf.clone(), r.logp_buf.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*outs))
    assert float((outs[0][0][1].cpu().double() - m_relu).abs().max()) <= MARGIN * rollout_twin_size(params, c["obs"], c["O"], c["seed"], "relu")[0]


# ------------------------------------------------------------------------------------------------ GPU: pointwise kernels
@pytest.mark.gpu
@pytest.mark.parametrize("activation", R.ACTIVATIONS)
@pytest.mark.parametrize("shape", POINTWISE_SHAPES, ids=lambda s: "G%d-R%d-C%d" % s)
def test_pointwise_kernels_match_the_float64_statement(hip_lib, shape, activation):
    """myo_bias_act_bf16 and myo_act_bwd_colsum_bf16 for both activations under rule R1; the column sums against the sums of the
    kernel's own bf16 outputs (fp32 order: 32 terms, each add rounding a partial sum of magnitude <= sum |term| by 2^-24);
    with MYO_ACT_RELU both equal the existing entry points bit for bit."""
    G, Rw, Cc = shape
    code = ACT_TANH if activation == "tanh" else ACT_RELU
    h, bias, dy = pointwise_case(*shape)
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    L, p = hip_lib.L, lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hd, bd = h.to(dev).to(bf), bias.to(dev).to(bf)
    assert torch.equal(hd.float().cpu(), h) and torch.equal(bd.float().cpu(), bias)
    out = hd.clone()
    hip_lib.check(L.myo_bias_act_bf16(p(out), p(bd), G, Rw, Cc, code, stream))
    torch.cuda.synchronize()
    failures = r1("act", out.float(), R.bias_act_ref(h, bias, activation), activation)
    if activation == "tanh":
        assert out[0, 0, :4].float().tolist() == [1.0, -1.0, 0.0, 0.0]
    else:
        old = hd.clone()
        hip_lib.check(L.myo_bias_relu_bf16(p(old), p(bd), G, Rw, Cc, stream))
        torch.cuda.synchronize()
        assert torch.equal(old, out)
    # backward on the kernel's own forward output
    act_out = out.reshape(G * Rw, Cc)
    g = dy.to(dev).to(bf)
    part = torch.full((G * Rw // 32, Cc), K.SENTINEL, device=dev)
    hip_lib.check(L.myo_act_bwd_colsum_bf16(p(g), p(act_out), G * Rw, Cc, p(part), code, stream))
    torch.cuda.synchronize()
    failures += r1("dact", g.float(), R.act_bwd_ref(dy, act_out.float().cpu(), activation), activation)
    assert not failures, failures
    gk = g.float().cpu().double().view(G * Rw // 32, 32, Cc)
    want, mag = gk.sum(1), gk.abs().sum(1)
    err = (part.cpu().double() - want).abs()
    assert bool((err <= 32 * EPS32 * mag).all()), float((err - 32 * EPS32 * mag).max())
    if activation == "relu":
        g2, part2 = dy.to(dev).to(bf), torch.zeros_like(part)
        hip_lib.check(L.myo_relu_bwd_colsum_bf16(p(g2), p(act_out), G * Rw, Cc, p(part2), stream))
        torch.cuda.synchronize()
        assert torch.equal(g2, g) and torch.equal(part2, part)


# ------------------------------------------------------------------------------------------------ GPU: through PPO
def _ppo(activation_fn, N=256, T=8, batch=1024, seed=5):
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    from myochallenge_amd.rl.ppo import PPO, PPOConfig
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    torch.manual_seed(0)
    env = EnvironmentFactory.create("CustomMyoBaodingBallsP1", num_envs=N, seed=seed)
    pol = ActorCriticPolicy(env.obs_dim, env.act_dim, (256, 256), (256, 256), lstm_hidden_size=None, log_std_init=-1.0, activation_fn=activation_fn)
    return PPO(VecNormalize(env), pol, PPOConfig(n_steps=T, batch_size=batch, n_epochs=1)), pol


@pytest.mark.gpu
def test_ppo_rolls_out_trains_and_saves_a_tanh_policy(hip_lib, tmp_path):
    """PPO on 256 envs x 8 steps with an MLP[256, 256] Tanh policy: the rollout's stored values and log-probabilities are the
    Tanh network's on the stored observations (reference under the rollout bound; the ReLU reference is not), one train() runs on
    the fused step, and the policy saves and loads as Tanh."""
    from myochallenge_amd.rl.sb3_zip import load_policy
    algo, pol = _ppo(torch.nn.Tanh)
    assert algo._fused is not None and algo._fused.act == ACT_TANH
    algo.collect_rollouts()
    assert type(algo._rollout).__name__ == "KernelRollout" and getattr(algo._fused, "_rollout", None) is not None, "the rollout did not take the fused kernel"
    params = R.policy_params(pol)
    T, N, O = algo.obs_buf.shape
    A = algo.act_buf.shape[2]
    obs = algo.obs_buf.reshape(T * N, O).cpu()
    act = algo.act_buf.reshape(T * N, A).cpu().double()
    val, logp = algo.val_buf.reshape(T * N).cpu().double(), algo.logp_buf.reshape(T * N).cpu().double()
    (mr, vr), (mt, vt) = R.ppo_mlp_rollout_ref(params, obs, torch.float64, activation="tanh"), R.ppo_mlp_rollout_ref(params, obs, torch.float32, activation="tanh")
    size = max(float((mt.double() - mr).abs().max()), float((vt.double() - vr).abs().max()))          # pooled over both nets and 2048 rows
    ev = float((val - vr).abs().max())
    # log pi of the STORED action under the reference mean.  With d = kernel mean - reference mean, |d| <= MARGIN * size, and
    # z = (act - kernel mean) / sigma: log pi_kernel - log pi_ref = sum_a z_a e_a + e_a^2 / 2 with e_a = d_a / sigma_a; |z_a| is
    # at most the reference's |z_a| + |e_a|.  On top, the kernel's own fp32 evaluation (test_ppo_mlp_kernels.py's bound).
    ls = params["log_std"].double()
    e = MARGIN * size * torch.exp(-ls)
    zr = ((act - mr) * torch.exp(-ls)).abs()
    quad, terms = 0.5 * zr * zr, 0.5 * zr * zr + (ls + mlp_ref.HALF_LOG_2PI).abs()
    tol = ((zr + e) * e + 0.5 * e * e).sum(-1) + 17 * EPS32 * quad.sum(-1) + 12 * EPS32 * terms.sum(-1)
    el = (logp - R.gaussian_logp(act, mr, ls)).abs()
    print("ppo tanh rollout: value err %.3e twin %.3e kernel/twin %.2f; log-prob err / bound %.3f" % (ev, size, _note("ppo rollout value", ev, size), float((el / tol).max())))
    assert ev <= MARGIN * size, (ev, size)
    assert bool((el <= tol).all()), float((el / tol).max())
    m_relu, v_relu = R.ppo_mlp_rollout_ref(params, obs, torch.float64, activation="relu")
    assert float((val - v_relu).abs().max()) > 10 * MARGIN * size
    assert float(((logp - R.gaussian_logp(act, m_relu, ls)).abs() / tol).max()) > 10
    before = [p.detach().clone() for p in pol.parameters()]
    st = algo.train()
    assert math.isfinite(st["policy_loss"]) and math.isfinite(st["value_loss"])
    assert any(d is not None for d, _ in algo._fused._mfma.values()), "train() did not take the matrix-core step"
    assert all(torch.isfinite(p).all() for p in pol.parameters()) and all(not torch.equal(x, y) for x, y in zip(before, pol.parameters()))
    path = str(tmp_path / "tanh_ppo.zip")
    algo.save(path)
    back, data = load_policy(path)
    assert back.activation_fn is torch.nn.Tanh and data["policy_kwargs"]["activation_fn"].endswith("Tanh'>")
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    mine = ActorCriticPolicy(O, A, (256, 256), (256, 256), lstm_hidden_size=None, activation_fn=torch.nn.Tanh)
    mine.load_state_dict({k: v.detach().cpu() for k, v in pol.state_dict().items()})
    x = obs[:16].numpy()
    assert (back.predict(x, deterministic=True)[0] == mine.predict(x, deterministic=True)[0]).all()


@pytest.mark.gpu
def test_ppo_keeps_an_unfusable_activation_on_autograd(hip_lib):
    """activation_fn = nn.ELU: no fused object is built and one update trains through autograd."""
    algo, pol = _ppo(torch.nn.ELU, N=64, T=4, batch=128)
    assert algo._fused is None and algo._fused_rec is None and algo._flat_adam is None
    before = [p.detach().clone() for p in pol.parameters()]
    algo.collect_rollouts()
    st = algo.train()
    assert math.isfinite(st["policy_loss"]) and math.isfinite(st["value_loss"])
    assert all(torch.isfinite(p).all() for p in pol.parameters()) and any(not torch.equal(x, y) for x, y in zip(before, pol.parameters()))


# ------------------------------------------------------------------------------------------------ GPU: recurrent step
@pytest.mark.gpu
def test_fused_recurrent_step_with_tanh_trunks_matches_autograd(hip_lib, monkeypatch):
    """tests/test_reorient.py::test_fused_recurrent_step_matches_autograd's smallest case (LSTM 32 -> trunks (64, 64)) with
    activation_fn = nn.Tanh, no gSDE: the fused recurrent step against autograd of the module under bf16 autocast on the same
    minibatch, under that test's own bound (cos > 0.995, rel < 0.1 on every parameter) — and NOT within it against autograd of a
    ReLU copy of the same weights (the trunks' gradients)."""
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    from myochallenge_amd.rl.ppo import PPO, PPOConfig, compute_gae
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    N, T, m, arch, hidden = 128, 8, 64, (64, 64), 32
    torch.manual_seed(0)
    env = EnvironmentFactory.create("CustomMyoReorientP1", num_envs=N, seed=3)
    mk_pol = lambda act: ActorCriticPolicy(env.obs_dim, env.act_dim, arch, arch, lstm_hidden_size=hidden, activation_fn=act)
    pol = mk_pol(torch.nn.Tanh)
    with torch.no_grad():
        pol.log_std.fill_(-0.5)
    pol_b, pol_r = copy.deepcopy(pol), mk_pol(torch.nn.ReLU)
    pol_r.load_state_dict(pol.state_dict())
    mk = lambda p: PPO(VecNormalize(env), p, PPOConfig(n_steps=T, batch_size=T * m, n_epochs=1, ent_coef=0.01))
    a = mk(pol)
    monkeypatch.setenv("MYO_RECURRENT_AUTOGRAD", "1")
    b, r = mk(pol_b), mk(pol_r)
    assert a._fused_rec is not None and a._fused_rec.act == ACT_TANH and b._fused_rec is None and r._fused_rec is None
    a.collect_rollouts(); a.collect_rollouts()
    a.start_buf[3, ::5] = 1.0; a.start_buf[6, 1::7] = 1.0
    for other in (b, r):
        for name in ("obs_buf", "act_buf", "rew_buf", "val_buf", "logp_buf", "start_buf"):
            getattr(other, name).copy_(getattr(a, name))
        other._rollout_state0 = tuple(x.clone() for x in a._rollout_state0)
    adv, ret = compute_gae(a.rew_buf, a.val_buf, a.start_buf, a._last_values, a._last_starts, 0.99, 0.95)
    idx = torch.randperm(N, device=a.device)[:m]
    grads, losses = [], []
    for algo in (a, b, r):
        g = algo._rec_stage(adv, ret, T, N, m)
        g["idx"].copy_(idx)
        algo._rec_forward_backward()
        torch.cuda.synchronize()
        losses.append((float(g["pl"]), float(g["vl"])))
        grads.append({n: p.grad.detach().clone() for n, p in algo.policy.named_parameters()})
    assert abs(losses[0][0] - losses[1][0]) < 2e-3 * (1 + abs(losses[1][0])), losses
    assert abs(losses[0][1] - losses[1][1]) < 2e-2 * (1 + abs(losses[1][1])), losses
    outside = []
    for n, gb in grads[1].items():
        ga, gr = grads[0][n], grads[2][n]
        assert torch.isfinite(ga).all(), n
        cos = float((ga * gb).sum() / (ga.norm() * gb.norm() + 1e-30))
        rel = float((ga - gb).norm() / (gb.norm() + 1e-30))
        cos_r = float((ga * gr).sum() / (ga.norm() * gr.norm() + 1e-30))
        rel_r = float((ga - gr).norm() / (gr.norm() + 1e-30))
        print("recurrent tanh %-40s vs tanh autograd cos %.5f rel %.4f | vs relu autograd cos %.5f rel %.4f" % (n, cos, rel, cos_r, rel_r))
        assert cos > 0.995 and rel < 0.1, (n, cos, rel, float(gb.norm()))
        if not (cos_r > 0.995 and rel_r < 0.1):
            outside.append(n)
    assert any(n.startswith("mlp_extractor.policy_net") for n in outside) and any(n.startswith("mlp_extractor.value_net") for n in outside), outside
