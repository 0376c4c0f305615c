"""The fused PPO MLP optimizer step with RESIDENT operand images (myo_ppo_mlp_step_resident, myo_ppo_mlp_images,
myo_adam_step with images, myo_ppo_adv_moments_epoch: four launches per step instead of six) against the stateless step it replaces.
Every comparison is torch.equal: the resident path removes passes, it does not reorder a sum.

Shapes (tests/mlp_digest_cases.CASES): B = 1024 with (O, A) = (1, 1), (33, 17), (97, 48) — OP = 32 / 64 / 128, one to three head
tiles, two k-steps per weight-gradient split — and B = 2048 with (86, 39): four k-steps, the benchmark's widths."""
import ctypes as C
import json
import os

import pytest
import torch

import mlp_digest_cases as mdc
from myochallenge_amd import native

pytestmark = pytest.mark.gpu


def _image_bytes(lib, step, case):
    """The operand images of a FusedPPOStep's workspace: its first myo_ppo_mlp_rollout_workspace_bytes bytes (same carve)."""
    O, A, B, _ = case
    (d, ws), = [v for v in step._mfma.values() if v[0] is not None]
    n = lib.L.myo_ppo_mlp_rollout_workspace_bytes(O, A, 256)
    assert 0 < n < ws.numel()
    return d, ws[:n]


def _state(fa, step):
    return {"p": fa.flat["p"], "m": fa.m, "v": fa.v, "g": fa.flat["g"], "acc": step.acc, "adam step": fa._step, "stats": step.stats,
            "shadow": fa.shadow}


def _assert_same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("stop_before_step_two", [False, True], ids=["plain", "stop-flag"])
@pytest.mark.parametrize("case", mdc.CASES, ids=mdc.case_id)
def test_resident_step_equals_stateless_step(hip_lib, case, stop_before_step_two):
    """Two identical policies with a FlatAdam each, three optimizer steps: run_indexed stateless on one, resident on the other.
    After every step p, m, v, the gradient vector, acc, the step counter, the advantage moments, the bf16 shadow and every image
    byte agree (the stateless twin's images are rebuilt from its parameters for the comparison: its own lag one step behind).
    stop-flag: the hyper-parameter block's stop flag is raised before step two — nothing moves from there on, images included.
    At the end the resident images are what the image pass writes for the final parameters, padding included."""
    lib = hip_lib
    _, fa_s, st_s, hp_s, data = mdc.make_run(lib, case)
    _, fa_r, st_r, hp_r, _ = mdc.make_run(lib, case)
    st_r.resident_adam = fa_r
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    frozen = None
    for k in range(3):
        if stop_before_step_two and k == 1:
            for hp in (hp_s, hp_r):
                hp.view(torch.int32)[native.HP_STOP] = 1
            torch.cuda.synchronize()
            frozen = ({n: t.clone() for n, t in _state(fa_r, st_r).items() if n not in ("g", "acc", "stats")}, _image_bytes(lib, st_r, case)[1].clone())
        for fa, st in ((fa_s, st_s), (fa_r, st_r)):
            st.run_indexed(*data)
            assert fa.presummed > 0, "the step fell back to the GEMM path"
            fa.step()
        torch.cuda.synchronize()
        assert fa_r.images is not None and fa_s.images is None
        _assert_same(_state(fa_s, st_s), _state(fa_r, st_r), "after step %d" % k)
        assert torch.equal(hp_s, hp_r)
        d_s, img_s = _image_bytes(lib, st_s, case)
        _, img_r = _image_bytes(lib, st_r, case)
        lib.check(lib.L.myo_ppo_mlp_images(C.byref(d_s), stream()))
        torch.cuda.synchronize()
        assert torch.equal(img_s, img_r), "operand images after step %d" % k
        if frozen is not None:
            now = _state(fa_r, st_r)
            for n, t in frozen[0].items():
                assert torch.equal(t, now[n]), ("moved with the stop flag up", n)
            assert torch.equal(frozen[1], img_r), "images moved with the stop flag up"
    hi = hp_r.view(torch.int32)
    assert int(hi[native.HP_APPLIED]) == (1 if stop_before_step_two else 3) == int(fa_r._step[1])
    # the final images against the image pass on the resident run's own parameters (the block is filled with 0xA5 first: the
    # padding must come out of the pass, not out of what the block held)
    d_r, img_r = _image_bytes(lib, st_r, case)
    kept = img_r.clone()
    img_r.fill_(0xA5)
    lib.check(lib.L.myo_ppo_mlp_images(C.byref(d_r), stream()))
    torch.cuda.synchronize()
    # the six images in the workspace's order, each starting on a 256-byte boundary (the bytes between them belong to no image)
    H, OP, written, o = 256, (case[0] + 31) // 32 * 32, torch.zeros_like(kept, dtype=torch.bool), 0
    for n in (2 * H * OP * 2, 2 * H * H * 2, 2 * H * H * 2, 2 * 48 * H * 2, 2 * H * 64 * 2, (4 * H + 2 * 48) * 4):
        written[o:o + n] = True
        o += (n + 255) // 256 * 256
    assert o == kept.numel()
    assert torch.equal(kept[written], img_r[written]) and bool((img_r[~written] == 0xA5).all())


@pytest.mark.parametrize("case", mdc.CASES, ids=mdc.case_id)
def test_resident_step_with_the_multi_rank_tail(hip_lib, case):
    """The tail N > 1 ranks run — k_mlp_reduce + k_colmajor_finish, then (after the all-reduce) myo_adam_step with nparts = 0 and images, which
    squares the gradient itself — resident against stateless over three steps: same state, same images."""
    lib = hip_lib
    _, fa_s, st_s, hp_s, data = mdc.make_run(lib, case)
    _, fa_r, st_r, hp_r, _ = mdc.make_run(lib, case)
    st_s.adam = st_r.adam = None
    st_r.resident_adam = fa_r
    for k in range(3):
        for fa, st in ((fa_s, st_s), (fa_r, st_r)):
            st.run_indexed(*data)
            assert fa.presummed == 0
            fa.step()
        torch.cuda.synchronize()
        assert fa_r.images is not None and fa_s.images is None
        _assert_same(_state(fa_s, st_s), _state(fa_r, st_r), "after step %d" % k)
        assert torch.equal(hp_s, hp_r)
    d_s, img_s = _image_bytes(lib, st_s, case)
    lib.check(lib.L.myo_ppo_mlp_images(C.byref(d_s), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(img_s, _image_bytes(lib, st_r, case)[1]) and int(fa_r._step[1]) == 3


def test_adam_step_is_one_step_whatever_it_is_handed(hip_lib):
    """One optimizer step through myo_adam_step on the gradient of the smallest digest case with OP != O and two head tiles
    (B = 1024, O = 33, A = 17), from the same state, in the eight combinations nparts in {0, the fused step's partial sums} x
    hp in {NULL, block holding the same lr} x images in {NULL, the fused step's descriptor}.  Within one nparts setting p, m, v
    and the bf16 shadow are bit-equal across hp and images (the two settings add |g|^2 in different orders); where images is set,
    the six images are afterwards what a fresh myo_ppo_mlp_images pass writes for the updated parameters."""
    lib, case = hip_lib, mdc.CASES[1]
    assert case[:3] == (33, 17, 1024)
    _, fa, step, hp, data = mdc.make_run(lib, case)
    before = {k: t.clone() for k, t in (("p", fa.flat["p"]), ("m", fa.m), ("v", fa.v), ("shadow", fa.shadow), ("hp", hp))}
    step.run_indexed(*data)        # leaves the gradient, its partial sums of squares in fa.sq and the step counter advanced
    torch.cuda.synchronize()
    assert fa.presummed == lib.L.myo_ppo_mlp_sqnorm_parts(case[1]) and fa._step.tolist() == [0, 1]
    sq = fa.sq.clone()
    desc, img = _image_bytes(lib, step, case)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = native.AdamDesc(p=fa.flat["p"].data_ptr(), g=fa.flat["g"].data_ptr(), m=fa.m.data_ptr(), v=fa.v.data_ptr(), n=fa.flat["p"].numel(),
                        lr=mdc.LR, b1=0.9, b2=0.999, eps=1e-5, max_norm=mdc.MAX_NORM, grad_scale=1.0, step=fa._step.data_ptr(),
                        scratch=fa.sq.data_ptr(), p_bf16=fa.shadow.data_ptr())
    got = {}
    for nparts in (0, fa.presummed):
        for with_hp in (False, True):
            for with_images in (False, True):
                for k, t in (("p", fa.flat["p"]), ("m", fa.m), ("v", fa.v), ("shadow", fa.shadow), ("hp", hp)):
                    t.copy_(before[k])
                fa.sq.copy_(sq)
                fa._step.copy_(torch.tensor([0, 1 if nparts else 0], dtype=torch.int32))
                lib.check(lib.L.myo_ppo_mlp_images(C.byref(desc), stream()))          # the images of the parameters before the step
                a.nparts, a.hp, a.images = nparts, (hp.data_ptr() if with_hp else None), (C.pointer(desc) if with_images else None)
                lib.check(lib.L.myo_adam_step(C.byref(a), stream()))
                torch.cuda.synchronize()
                assert fa._step.tolist() == [0, 1] and int(hp.view(torch.int32)[native.HP_APPLIED]) == int(with_hp)
                got[nparts, with_hp, with_images] = {k: t.clone() for k, t in (("p", fa.flat["p"]), ("m", fa.m), ("v", fa.v), ("shadow", fa.shadow))}
                if with_images:
                    mirrored = img.clone()
                    lib.check(lib.L.myo_ppo_mlp_images(C.byref(desc), stream()))
                    torch.cuda.synchronize()
                    assert torch.equal(mirrored, img), ("operand images", nparts, with_hp)
        plain = got[nparts, False, False]
        assert not torch.equal(plain["p"], before["p"]), "no step was taken"
        for with_hp, with_images in ((False, True), (True, False), (True, True)):
            _assert_same(plain, got[nparts, with_hp, with_images], "nparts = %d, hp %s, images %s" % (nparts, with_hp, with_images))


@pytest.mark.parametrize("n_mb", [1, 3, 16])
@pytest.mark.parametrize("case", mdc.CASES, ids=mdc.case_id)
def test_epoch_moments_equal_the_steps_own(hip_lib, case, n_mb):
    """myo_ppo_adv_moments_epoch on an index list of n_mb minibatches (advantages offset by +100: the merge's cancellation is
    loaded) — every row is torch.equal to the adv_stats the stateless step leaves for the same slice of the list."""
    lib = hip_lib
    O, A, B, _ = case
    _, fa, step, _, data = mdc.make_run(lib, case)
    obs, act, oldlp, _, ret, _ = data
    R = obs.shape[0]
    g = torch.Generator().manual_seed(1000 * n_mb + B + O)
    adv = (100.0 + torch.randn(R, generator=g)).cuda()
    # (rows may repeat across minibatches when the rollout is shorter than the list: each minibatch is its own permutation slice)
    idx = torch.cat([torch.randperm(R, generator=g)[:B] for _ in range(n_mb)]).cuda()
    got = step.epoch_moments(adv, idx, B, n_mb).clone()
    torch.cuda.synchronize()
    for k in range(n_mb):
        step.run_indexed(obs, act, oldlp, adv, ret, idx[k * B:(k + 1) * B].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(got[k], step.stats), (k, got[k], step.stats)
    assert float(got[:, 0].min()) > 99.0 and float(got[:, 1].min()) > 0.5


def _train_once(monkeypatch, resident, target_kl=None):
    from myochallenge_amd.envs.environment_factory import EnvironmentFactory
    from myochallenge_amd.rl.policy import ActorCriticPolicy
    from myochallenge_amd.rl.ppo import PPO, PPOConfig
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    if resident:
        monkeypatch.delenv("MYO_PPO_RESIDENT", raising=False)
    else:
        monkeypatch.setenv("MYO_PPO_RESIDENT", "0")
    torch.manual_seed(0)
    env = EnvironmentFactory.create("CustomMyoBaodingBallsP1", num_envs=64, seed=5)
    pol = ActorCriticPolicy(86, 39, (256, 256), (256, 256), lstm_hidden_size=None)
    algo = PPO(VecNormalize(env), pol, PPOConfig(n_steps=32, batch_size=1024, n_epochs=2, learning_rate=3e-3, target_kl=target_kl), seed=0)
    assert (algo._fused.resident_adam is not None) == resident
    algo.collect_rollouts()
    stats = algo.train()
    torch.cuda.synchronize()
    fa = algo._flat_adam
    out = {"p": fa.flat["p"].clone(), "m": fa.m.clone(), "v": fa.v.clone(), "adam step": fa._step.clone(), "shadow": fa.shadow.clone()}
    env.close()
    return stats, out


@pytest.mark.parametrize("target_kl", [None, 1e-5], ids=["no-target-kl", "stops-in-first-epoch"])
def test_train_is_bit_equal_with_and_without_resident_images(hip_lib, monkeypatch, target_kl):
    """PPO.train() on 64 envs x 32 steps, minibatches of 1024, 2 epochs: parameters, Adam state and bf16 shadow after the update are
    bit-equal between MYO_PPO_RESIDENT=0 (six launches per step) and the default (four, moments per epoch chunk).  With target_kl =
    1e-5 the update stops in its first epoch (the second minibatch's approx_kl after an lr = 3e-3 step is far above 1.5e-5), on
    the device, in both."""
    s0, a = _train_once(monkeypatch, False, target_kl)
    s1, b = _train_once(monkeypatch, True, target_kl)
    _assert_same(a, b, "after train()")
    assert s0["n_updates"] == s1["n_updates"] and s0["early_stopped"] == s1["early_stopped"]
    for k in ("policy_loss", "value_loss", "approx_kl", "clip_fraction", "entropy_loss"):
        assert s0[k] == s1[k], k
    if target_kl is None:
        assert s1["n_updates"] == 4 and not s1["early_stopped"]
    else:
        assert s1["early_stopped"] and s1["n_updates"] < 2


def test_same_bits_as_the_recorded_build(hip_lib, golden_dir):
    """The stateless step and the Adam step on the seeded cases of tests/mlp_digest_cases.py reproduce the SHA-256 digests that
    tools/mlp_step_digests.py printed on the build of the commit before the resident-image step (tests/golden/mlp_step_digests.json):
    gradients, acc, advantage moments, parameters and Adam moments over two optimizer steps at the four shapes."""
    want = json.load(open(os.path.join(golden_dir, "mlp_step_digests.json")))["digests"]
    got = mdc.step_digests(hip_lib)
    assert sorted(got) == sorted(want)
    diff = [(c, k) for c in want for k in want[c] if got[c].get(k) != want[c][k]]
    assert not diff, diff
