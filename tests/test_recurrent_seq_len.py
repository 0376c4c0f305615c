"""PPOConfig.seq_len: recurrent PPO on truncated-BPTT minibatches — chunks of seq_len consecutive steps, each started from the LSTM state
the rollout stored as it entered the chunk (sb3-contrib's RecurrentRolloutBuffer semantics).  CPU tests on the emulation
env and the eager path; GPU tests of the two HIP entry points (myo_ppo_gather_seq, myo_rollout_state_snapshot), of the fused chunk
step against autograd and of the captured update."""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import make_env
from myochallenge_amd.rl.policy import ActorCriticPolicy
from myochallenge_amd.rl.ppo import PPO, PPOConfig, compute_gae

BUFFERS = ("obs_buf", "act_buf", "rew_buf", "val_buf", "logp_buf", "start_buf")


# ------------------------------------------------------------------------------------------ CPU: the eager path on the emulation env
def _cpu_env(emu_lib):
    return make_env("CustomMyoBaodingBallsP1", emu_lib, num_envs=6, dtype="f64", max_episode_steps=5)


def _cpu_policy():
    torch.manual_seed(0)
    return ActorCriticPolicy(86, 39, (16,), (16,), lstm_hidden_size=8)


def _cpu_cfg(**kw):
    base = dict(n_steps=12, batch_size=72, n_epochs=1, bf16=False, use_graphs=False, max_grad_norm=1e9)
    base.update(kw)
    return PPOConfig(**base)


def _share_rollout(src, dst):
    """dst trains on the rollout src collected."""
    for name in BUFFERS:
        getattr(dst, name).copy_(getattr(src, name))
    dst._last_values, dst._last_starts = src._last_values.clone(), src._last_starts.clone()
    dst._rollout_state0 = tuple(x.clone() for x in src._rollout_state0)


def _train_and_catch_gradient(algo):
    """train() with an optimizer that records the gradient of the (one) minibatch instead of stepping (max_grad_norm = 1e9: unclipped)."""
    got = {}
    algo.optimizer.step = lambda: got.update({n: p.grad.detach().clone() for n, p in algo.policy.named_parameters()})
    return algo.train(), got


def test_seq_len_is_validated(emu_lib, tmp_path):
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    from myochallenge_amd.train.trainer import MyoTrainer
    assert PPOConfig().seq_len is None
    with pytest.raises(ValueError):
        PPOConfig(n_steps=12, batch_size=24, seq_len=0)
    with pytest.raises(ValueError):
        PPOConfig(n_steps=12, batch_size=60, seq_len=5)            # n_steps % seq_len
    with pytest.raises(ValueError):
        PPOConfig(n_steps=12, batch_size=30, seq_len=4)            # batch_size % seq_len
    env = _cpu_env(emu_lib)
    with pytest.raises(ValueError):                                # no LSTM to truncate
        PPO(env, ActorCriticPolicy(86, 39, (16,), (16,), lstm_hidden_size=None), _cpu_cfg(seq_len=4))
    with pytest.raises(ValueError):                                # 19 chunks asked of a rollout of 6 * 3
        PPO(env, _cpu_policy(), _cpu_cfg(seq_len=4, batch_size=76))
    assert PPO(env, _cpu_policy(), _cpu_cfg(seq_len=4, batch_size=72)).cfg.seq_len == 4
    mk = lambda **mc: MyoTrainer(envs=VecNormalize(env), env_config={}, load_model_path=None, log_dir=str(tmp_path / "run"),
                                 model_config={"n_steps": 4, "batch_size": 8, "n_epochs": 1,
                                               "policy_kwargs": {"net_arch": [{"pi": [8], "vf": [8]}], "lstm_hidden_size": 8}, **mc})
    assert mk(seq_len=2).agent.cfg.seq_len == 2 and mk().agent.cfg.seq_len is None
    with pytest.raises(TypeError):
        mk(seq_len=2, sequence_length=2)
    env.close()


def test_snapshots_are_the_states_the_policy_passed_through(emu_lib):
    env, pol = _cpu_env(emu_lib), _cpu_policy()
    algo = PPO(env, pol, _cpu_cfg(seq_len=4))
    algo.collect_rollouts(); algo.collect_rollouts()              # the second rollout starts from a non-zero state
    L, starts = 4, algo.start_buf
    assert float(starts[0::L].sum()) > 0 and float(starts.sum() - starts[0::L].sum()) > 0      # starts on chunk boundaries and inside chunks
    snaps = algo.rollout_snapshots()
    assert all(tuple(x.shape) == (3, 1, 6, 8) for x in snaps)
    assert float(algo._rollout_state0[0].abs().max()) > 0
    for k in range(4):
        assert torch.equal(snaps[k][0], algo._rollout_state0[k])
    for s in (1, 2):
        with torch.no_grad():
            _, _, st = pol._latents(algo.obs_buf[:s * L], algo._rollout_state0, starts[:s * L])
        for k in range(4):
            err = float((st[k] - snaps[k][s]).abs().max())
            assert err <= 1e-6, (s, k, err)
        assert not torch.equal(snaps[0][s], snaps[0][s - 1])
    env.close()


def test_chunk_minibatch_is_what_it_says(emu_lib):
    """Loss and gradient of the eager chunk path == a loop over the permutation's items, each chunk evaluated alone from its snapshot
    (float32 autograd, the same graph up to batching order: 1e-5); and the truncation is really there: the recurrent weights' gradient
    differs from the whole-rollout one."""
    env, pol = _cpu_env(emu_lib), _cpu_policy()
    N, T, L = 6, 12, 4
    algo = PPO(env, pol, _cpu_cfg(seq_len=L), seed=3)
    algo.collect_rollouts(); algo.collect_rollouts()
    with torch.no_grad():        # away from the rollout's policy: ratio != 1, so the policy loss is a number and not the rounding noise around 0
        for p in pol.parameters():
            p.add_(0.05 * torch.randn_like(p))
    whole = PPO(env, copy.deepcopy(pol), _cpu_cfg(seq_len=None), seed=3)
    _share_rollout(algo, whole)
    gen = torch.Generator().set_state(algo.gen.get_state())
    st, grad = _train_and_catch_gradient(algo)
    assert algo.n_updates == 1 and grad
    # the restatement
    perm = torch.randperm(N * (T // L), generator=gen)
    adv, ret = compute_gae(algo.rew_buf, algo.val_buf, algo.start_buf, algo._last_values, algo._last_starts, 0.99, 0.95)
    snaps = algo.rollout_snapshots()
    cols = {k: [] for k in ("v", "lp", "old", "adv", "ret")}
    for c in perm.tolist():
        s, n = c // N, c % N
        t0, t1 = s * L, (s + 1) * L
        st0 = tuple(x[s, :, n:n + 1] for x in snaps)
        v, lp, ent = pol.evaluate_actions(algo.obs_buf[t0:t1, n:n + 1], algo.act_buf[t0:t1, n:n + 1], st0, algo.start_buf[t0:t1, n:n + 1])
        for key, val in (("v", v), ("lp", lp), ("old", algo.logp_buf[t0:t1, n:n + 1]), ("adv", adv[t0:t1, n:n + 1]), ("ret", ret[t0:t1, n:n + 1])):
            cols[key].append(val)
    cat = {k: torch.cat(v, 1).reshape(-1) for k, v in cols.items()}
    loss, pl, vl = algo._loss(cat["v"], cat["lp"], ent, cat["old"], cat["adv"], cat["ret"])
    names = [n for n, _ in pol.named_parameters()]
    want = dict(zip(names, torch.autograd.grad(loss, list(pol.parameters()))))
    print("losses", st["policy_loss"], float(pl), st["value_loss"], float(vl))
    assert abs(st["policy_loss"] - float(pl)) <= 1e-5 * abs(float(pl)), (st["policy_loss"], float(pl))
    assert abs(st["value_loss"] - float(vl)) <= 1e-5 * abs(float(vl)), (st["value_loss"], float(vl))
    for n in names:
        err = float((grad[n] - want[n]).norm())
        print(n, err / float(want[n].norm()))
        assert err <= 1e-5 * float(want[n].norm()), (n, err, float(want[n].norm()))
    # the whole-rollout minibatch of the same transitions (all 6 envs) back-propagates through the chunk boundaries
    _, grad_whole = _train_and_catch_gradient(whole)
    for n in ("lstm_actor.weight_hh_l0", "lstm_critic.weight_hh_l0"):
        diff = float((grad[n] - grad_whole[n]).norm())
        assert diff > 1e-3 * float(grad_whole[n].norm()), (n, diff)
    env.close()


def test_seq_len_equal_to_n_steps_is_none(emu_lib):
    env, pol = _cpu_env(emu_lib), _cpu_policy()
    pol2 = copy.deepcopy(pol)
    a = PPO(env, pol, _cpu_cfg(seq_len=12, batch_size=24, n_epochs=2, max_grad_norm=0.5), seed=7)
    b = PPO(env, pol2, _cpu_cfg(seq_len=None, batch_size=24, n_epochs=2, max_grad_norm=0.5), seed=7)
    a.collect_rollouts(); a.collect_rollouts()
    _share_rollout(a, b)
    before = [p.detach().clone() for p in pol.parameters()]
    sa, sb = a.train(), b.train()
    assert sa["n_updates"] == sb["n_updates"] == 6
    assert sa["policy_loss"] == sb["policy_loss"] and sa["value_loss"] == sb["value_loss"]
    for (n, p), q, p0 in zip(pol.named_parameters(), pol2.parameters(), before):
        assert torch.equal(p, q), n
        assert not torch.equal(p, p0), n
    env.close()


# ------------------------------------------------------------------------------------------ GPU
def _bits(x):
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("m,copies", [(24, 1), (21, 2)], ids=["six-blocks", "ragged-last-block"])
def test_gather_seq_matches_torch(hip_lib, m, copies):
    """myo_ppo_gather_seq against the torch statement of the chunk minibatch: every output bit for bit (copies and products with
    0 / 1 have no rounding of their own), adv_stats bit-equal to myo_ppo_gather on the equivalent rows."""
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    env = EnvironmentFactory.create("CustomMyoReorientP1", num_envs=128, seed=3)
    O, A = env.obs_dim, 39
    assert O % 2 == 1
    d = env.device
    env.close()
    T, L, N, G, H = 8, 4, 128, 2, 32
    S, B = T // L, L * m
    gen = torch.Generator(device=d).manual_seed(11)
    rnd = lambda *shape: torch.randn(shape, device=d, generator=gen)
    obs, act, oldlp, adv, ret = rnd(T, N, O), rnd(T, N, A), rnd(T, N), rnd(T, N), rnd(T, N)
    starts = (torch.rand((T, N), device=d, generator=gen) < 0.3).float()
    h_snap, c_snap = rnd(S, G, N, H).to(torch.bfloat16), rnd(S, G, N, H)
    chunk = torch.randperm(N * S, device=d, generator=gen)[:m]
    s, n = chunk // N, chunk % N
    assert int(s.min()) == 0 and int(s.max()) == 1
    first = starts[s * L, n]
    assert 0 < float(first.sum()) < m and float(starts[s * L + 1, n].sum()) > 0         # starts at step 0 of some chunks, inside others
    ridx = (((s * L).view(1, m) + torch.arange(L, device=d).view(L, 1)) * N + n.view(1, m)).reshape(B)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    L_ = hip_lib.L
    out = dict(x=torch.zeros((copies, B, O), device=d, dtype=torch.bfloat16), act=torch.zeros((B, A), device=d), oldlp=torch.zeros(B, device=d),
               adv=torch.zeros(B, device=d), ret=torch.zeros(B, device=d), keep=torch.zeros((L, m), device=d),
               hm0=torch.zeros((G, m, H), device=d, dtype=torch.bfloat16), cm0=torch.zeros((G, m, H), device=d, dtype=torch.bfloat16),
               c0=torch.zeros((G, m, H), device=d), stats=torch.zeros(2, device=d), work=torch.zeros(2 * ((B + 15) // 16), device=d))

    def call(obs_=obs, m_=m, L_steps=L, T_=T):
        return L_.myo_ppo_gather_seq(p(obs_), p(act), p(oldlp), p(adv), p(ret), p(starts), p(h_snap), p(c_snap), p(chunk), T_, N, L_steps, m_, G, H,
                                     O, A, p(out["x"]), copies, p(out["act"]), p(out["oldlp"]), p(out["adv"]), p(out["ret"]), p(out["keep"]),
                                     p(out["hm0"]), p(out["cm0"]), p(out["c0"]), p(out["stats"]), p(out["work"]), None)
    hip_lib.check(call())
    # the plain gather on the equivalent rows: bf16 rounding of the observations and the advantage moments
    ref = dict(x=torch.zeros_like(out["x"]), act=torch.zeros_like(out["act"]), oldlp=torch.zeros(B, device=d), adv=torch.zeros(B, device=d),
               ret=torch.zeros(B, device=d), stats=torch.zeros(2, device=d), work=torch.zeros_like(out["work"]))
    hip_lib.check(L_.myo_ppo_gather(p(obs), p(act), p(oldlp), p(adv), p(ret), p(ridx), B, O, A, p(ref["x"]), copies, p(ref["act"]), p(ref["oldlp"]),
                                    p(ref["adv"]), p(ref["ret"]), p(ref["stats"]), p(ref["work"]), None))
    torch.cuda.synchronize()
    flat = lambda x: x.reshape(T * N, *x.shape[2:])
    assert torch.equal(_bits(out["x"]), _bits(flat(obs)[ridx].to(torch.bfloat16).unsqueeze(0).expand(copies, B, O)))
    assert torch.equal(_bits(out["x"]), _bits(ref["x"]))
    assert torch.equal(_bits(out["act"]), _bits(flat(act)[ridx]))
    for key, src in (("oldlp", oldlp), ("adv", adv), ("ret", ret)):
        assert torch.equal(_bits(out[key]), _bits(flat(src)[ridx])), key
    keep = (1.0 - flat(starts)[ridx]).view(L, m)
    assert torch.equal(_bits(out["keep"]), _bits(keep))
    k0 = keep[0].view(1, m, 1)
    assert torch.equal(k0.view(m), 1.0 - first)
    hsel, csel = h_snap[s, :, n].permute(1, 0, 2), c_snap[s, :, n].permute(1, 0, 2)                 # [G, m, H]
    assert torch.equal(_bits(out["hm0"]), _bits((hsel.float() * k0).to(torch.bfloat16)))
    assert torch.equal(_bits(out["c0"]), _bits(csel * k0))
    assert torch.equal(_bits(out["cm0"]), _bits((csel * k0).to(torch.bfloat16)))
    assert torch.equal(_bits(out["stats"]), _bits(ref["stats"]))
    assert abs(float(out["stats"][0]) - float(flat(adv)[ridx].mean())) < 1e-5 and abs(float(out["stats"][1]) - float(flat(adv)[ridx].std())) < 1e-5
    from myochallenge_amd import native
    bad = getattr(native, "MYO_E_ARG", -1)
    assert call(obs_=None) == bad and call(m_=0) == bad and call(L_steps=0) == bad and call(L_steps=3) == bad
    assert L_.myo_ppo_gather_seq(p(obs), p(act), p(oldlp), p(adv), p(ret), p(starts), None, p(c_snap), p(chunk), T, N, L, m, G, H, O, A,
                                 p(out["x"]), copies, p(out["act"]), p(out["oldlp"]), p(out["adv"]), p(out["ret"]), p(out["keep"]),
                                 p(out["hm0"]), p(out["cm0"]), p(out["c0"]), p(out["stats"]), p(out["work"]), None) == bad


@pytest.mark.gpu
def test_native_rollout_stores_the_chunk_states(hip_lib):
    """myo_rollout_state_snapshot inside the HIP-kernel rollout's per-step graph: after a rollout stepped by hand the three slots hold
    the (h, c) that entered steps 0, 4 and 8 — read at the END of the rollout, so nothing was written at any other step."""
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    torch.manual_seed(0)
    N, T, L = 128, 12, 4
    env = EnvironmentFactory.create("CustomMyoReorientP1", num_envs=N, seed=5, max_episode_steps=9)
    mkpol = lambda: ActorCriticPolicy(env.obs_dim, env.act_dim, (64, 64), (64, 64), lstm_hidden_size=32)
    plain = PPO(VecNormalize(env), mkpol(), PPOConfig(n_steps=T, batch_size=T * N, n_epochs=1))
    plain.rollout_step()
    assert type(plain._rollout).__name__ == "KernelRollout" and plain._rollout.snap_h is None and plain._rollout.snap_c is None and plain.rollout_snapshots() is None
    algo = PPO(VecNormalize(env), mkpol(), PPOConfig(n_steps=T, batch_size=T * N, n_epochs=1, seq_len=L))
    algo.collect_rollouts()
    assert type(algo._rollout).__name__ == "KernelRollout" and tuple(algo._rollout.snap_h.shape) == (3, 2, N, 32) and algo._rollout.snap_h.dtype == torch.bfloat16
    assert tuple(algo._rollout.snap_c.shape) == (3, 2, N, 32) and algo._rollout.snap_c.dtype == torch.float32
    algo._rollout.begin()
    hs, cs = [], []
    for t in range(T):
        if t % L == 0:
            hs.append(algo._rollout.hs.clone()); cs.append(algo._rollout.cs32.clone())
        algo.rollout_step()
    snap_h, snap_c = algo._rollout.snap_h.clone(), algo._rollout.snap_c.clone()
    state0 = algo._rollout_state0
    algo.finish_rollout()
    torch.cuda.synchronize()
    assert float(hs[0].abs().max()) > 0 and not torch.equal(hs[0], hs[1]) and not torch.equal(hs[1], hs[2])
    assert torch.equal(_bits(snap_h), _bits(torch.stack(hs))) and torch.equal(_bits(snap_c), _bits(torch.stack(cs)))
    for k, x in enumerate(algo.rollout_snapshots()):
        assert tuple(x.shape) == (3, 1, N, 32) and torch.equal(x[0], state0[k]), k
    env.close()


def _twin_chunk_algos(monkeypatch, arch, hidden, **cfg):
    """Two PPOs on copies of one policy and one rollout with seq_len = 4: `a` on the fused recurrent step, `b` on autograd."""
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    torch.manual_seed(0)
    N, T, L, m = 128, 8, 4, 64
    env = EnvironmentFactory.create("CustomMyoReorientP1", num_envs=N, seed=3)
    pol = ActorCriticPolicy(env.obs_dim, env.act_dim, arch, arch, lstm_hidden_size=hidden)
    with torch.no_grad():
        pol.log_std.fill_(-0.5)
    pol2 = copy.deepcopy(pol)
    mk = lambda p, L_: PPO(VecNormalize(env), p, PPOConfig(n_steps=T, batch_size=(L_ or T) * m, n_epochs=1, ent_coef=0.01, seq_len=L_, **cfg))
    a = mk(pol, L)
    monkeypatch.setenv("MYO_RECURRENT_AUTOGRAD", "1")
    b = mk(pol2, L)
    monkeypatch.delenv("MYO_RECURRENT_AUTOGRAD")
    assert a._fused_rec is not None and b._fused_rec is None and b._flat_adam is not None
    a.collect_rollouts(); a.collect_rollouts()                 # second rollout: non-zero states in every slot
    a.start_buf[3, ::5] = 1.0; a.start_buf[6, 1::7] = 1.0
    for name in BUFFERS:
        getattr(b, name).copy_(getattr(a, name))
    b._rollout_state0 = tuple(x.clone() for x in a._rollout_state0)
    snaps = tuple(x.clone() for x in a.rollout_snapshots())
    b._rollout = SimpleNamespace(snapshots=lambda: snaps, stacked_snapshots=lambda: None)     # b never rolls out: a stand-in collector that hands out the planted snapshots
    assert type(a._rollout).__name__ == "KernelRollout" and all(float(x.abs().max()) > 0 for x in b.rollout_snapshots())
    return env, a, b, (N, T, L, m)


def _compare_step(a, b, stage):
    """One minibatch step of each: (|d pl|, |d vl|, pl, vl, {parameter: (cosine, relative error)})."""
    grads, losses = [], []
    for algo in (a, b):
        g = stage(algo)
        algo._rec_forward_backward()
        torch.cuda.synchronize()
        losses.append((float(g["pl"]), float(g["vl"])))
        grads.append({n: p.grad.detach().clone() for n, p in algo.policy.named_parameters()})
    per = {}
    for n, gb in grads[1].items():
        ga = grads[0][n]
        assert torch.isfinite(ga).all(), n
        per[n] = (float((ga * gb).sum() / (ga.norm() * gb.norm() + 1e-30)), float((ga - gb).norm() / (gb.norm() + 1e-30)))
    return losses, per


@pytest.mark.gpu
@pytest.mark.parametrize("arch,hidden", [((64, 64), 32), ((64, 64), 48), ((), 128)], ids=["step-kernels", "gemm+cell-kernels", "seq-kernels"])
def test_fused_chunk_step_matches_autograd(hip_lib, monkeypatch, arch, hidden):
    """The fused recurrent step on a minibatch of 64 chunks of 4 steps (myo_ppo_gather_seq in front of the existing LSTM / trunk / loss
    code) against autograd under bf16 autocast on the same chunks and snapshot states, episode starts inside the chunks; bounds: the
    project's own for this comparison (tests/test_reorient.py::test_fused_recurrent_step_matches_autograd).  Then the captured update."""
    env, a, b, (N, T, L, m) = _twin_chunk_algos(monkeypatch, arch, hidden)
    fr = a._fused_rec
    assert fr.step_kernels == (hidden in (32, 128)) and fr.seq_kernels == (hidden == 128)
    adv, ret = compute_gae(a.rew_buf, a.val_buf, a.start_buf, a._last_values, a._last_starts, 0.99, 0.95)
    items = torch.randperm(N * (T // L), device=a.device)[:m]
    assert int((items // N).min()) == 0 and int((items // N).max()) == 1

    def stage(algo):
        g = algo._rec_stage(adv, ret, T, N, m, L)
        g["idx"].copy_(items)
        return g
    losses, per = _compare_step(a, b, stage)
    print("chunk step", hidden, losses, {n: (round(c, 5), round(r, 4)) for n, (c, r) in per.items()})
    assert a._rgraph == (T, N, m, L)
    assert abs(losses[0][0] - losses[1][0]) < 2e-3 * (1 + abs(losses[1][0])), losses
    assert abs(losses[0][1] - losses[1][1]) < 2e-2 * (1 + abs(losses[1][1])), losses
    for n, (cos, rel) in per.items():
        assert cos > 0.995 and rel < 0.1, (n, cos, rel)
    # the captured graph: two updates, each n_epochs * (N * S // m) = 4 optimizer steps
    for _ in range(2):
        before, n0 = [p.detach().clone() for p in a.policy.parameters()], a.n_updates
        st = a.train()
        assert a.n_updates - n0 == 1 * (N * (T // L) // m) == 4 and not st["early_stopped"]
        assert np.isfinite(st["policy_loss"]) and np.isfinite(st["value_loss"])
        assert all(torch.isfinite(p).all() for p in a.policy.parameters())
        assert all(not torch.equal(x, y) for x, y in zip(before, a.policy.parameters()))
    env.close()


@pytest.mark.gpu
def test_target_kl_stops_the_chunk_update(hip_lib, monkeypatch):
    """target_kl = 1e-9 on the captured chunk update: the first minibatch's approx_kl is over the limit, nothing is applied.
    The policy is moved by one update without a limit first.  Straight after a rollout the first minibatch of a chunk update has
    approx_kl == 0 exactly — the chunks start from the stored states and run the rollout's own step kernels on the same bf16 weights, so
    log pi comes out bit for bit — and SB3's `approx_kl > 1.5 * target_kl` lets that minibatch through (measured: n_updates 1, then
    the stop at the second minibatch)."""
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    torch.manual_seed(0)
    N, T, L, m = 128, 8, 4, 64
    env = EnvironmentFactory.create("CustomMyoReorientP1", num_envs=N, seed=3)
    pol = ActorCriticPolicy(env.obs_dim, env.act_dim, (64, 64), (64, 64), lstm_hidden_size=32)
    a = PPO(VecNormalize(env), pol, PPOConfig(n_steps=T, batch_size=L * m, n_epochs=2, ent_coef=0.01, seq_len=L, target_kl=1e-9))
    assert a._fused_rec is not None
    a.collect_rollouts()
    a.cfg.target_kl = None
    assert not a.train()["early_stopped"] and a.n_updates == 2 * 4
    a.cfg.target_kl = 1e-9
    before, n0 = [p.detach().clone() for p in pol.parameters()], a.n_updates
    st = a.train()
    assert a._rgraph == (T, N, m, L)
    assert st["early_stopped"] and st["n_updates"] == a.n_updates == n0 and st["approx_kl"] > 1.5e-9
    assert all(torch.equal(x, y) for x, y in zip(before, pol.parameters()))
    env.close()
