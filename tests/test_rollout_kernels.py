"""The rollout and optimizer plumbing kernels of csrc/myobatch.hip against the float64 references of rollout_ref.py.

CPU tests pin the references to the project's own torch statements (a wrong reference cannot pass for a right kernel); GPU
tests run every kernel through the C ABI at the shapes where its code takes another path.  Every tolerance is a rounding count
(written in rollout_ref.py next to the bound it gives), the reference's own fp32 twin times MARGIN, or exact equality.  Every
output buffer lies between guard words and is pre-filled with a sentinel.

Edges and the test that reaches them:
  k_vecnorm_merge's groups of eight blocks (partial last group, second group)   test_vecnorm_step[N1025-O7] (9 blocks), [N2053-O3] (17)
  k_vecnorm_moments chunks of 1, 2, 7 rows, odd tail, O < 64, O = 65             test_vecnorm_step[N1-O1] [N2-O3] [N7-O5] [N129-O65]
  training / norm_obs / norm_reward = 0, term_buf = trunc_buf = NULL             test_vecnorm_flags_and_null_buffers
  myo_vecnorm_batch_moments + myo_vecnorm_finish, variance from additive sums    test_vecnorm_multi_rank_form
  Philox counter layout (env, action group, draw lo, draw hi)                    test_gaussian_sampler
  u1 = 1.0f (radius 0) and c >> 8 == 0 (radius 5.9)                              test_gaussian_sampler_extreme_uniforms
  k_sample_sde at L = 1, A > 64, a zero latent (sigma at its floor)              test_gsde_sampler
  k_gae at T = 1, N around the 256-thread block, gamma lambda = 1 and gamma = 0  test_gae
  k_moments_finish's strided second and third trip (65 and 129 blocks)           test_gather[B1040-...] [B2049-...]
  k_adam's grid stride (n > 262144), k_grad_sqnorm's stride (n > 16384), bias correction at t = 1 and t = 10000   test_adam
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rollout_ref as rr

U32, U64 = rr.U32, rr.U64
SENTINEL = -12345.0
GUARD = 64
# kernel error allowed in units of the fp32 twin's: the sampler takes the fast __logf and __sincosf, whose error nobody has
# measured here; 64 times the accurate-fp32 figure is still four orders of magnitude below what a counter-layout slip gives (O(1))
MARGIN = 64.0
F32 = np.float32
DEV = "cuda:0"


# ----------------------------------------------------------------------------------------------------------------------- helpers
class Buf:
    """A device buffer between two guard zones, all of it pre-filled with a sentinel."""

    def __init__(self, shape, dtype=torch.float32, dev=None, fill=SENTINEL):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.n = int(np.prod(shape))
        self.fill = fill
        self.whole = torch.full((self.n + 2 * GUARD,), fill, dtype=dtype, device=dev or DEV)
        self.t = self.whole[GUARD:GUARD + self.n].view(shape)

    def refill(self):
        self.whole.fill_(self.fill)

    def check_guards(self, name):
        g = torch.cat([self.whole[:GUARD], self.whole[GUARD + self.n:]])
        assert bool((g == self.fill).all()), "%s: a guard word was overwritten" % name

    def untouched(self, rows):
        return bool((self.t[rows] == self.fill).all())


def ptr(x):
    if x is None:
        return None
    return C.c_void_p((x.t if isinstance(x, Buf) else x).data_ptr())


def host(x):
    return (x.t if isinstance(x, Buf) else x).detach().cpu().numpy()


def dev_of(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def within(name, got, ref, bound):
    got, ref, bound = (np.asarray(x, dtype=np.float64) for x in (got, ref, bound))
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err - bound, -np.inf))), err.shape) if err.shape else ()
        raise AssertionError("%s: |kernel - reference| = %.3e over the bound %.3e at %s (%d of %d elements over)"
                             % (name, err[i], np.broadcast_to(bound, err.shape)[i], i, int(bad.sum()), err.size))
    return float((err / np.where(bound > 0, bound, np.inf)).max()) if err.size else 0.0


BF16_EDGES = np.array([
    0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,     # ties to even (down, up), just above, just below, negative
    0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80000001, 0x80008000,     # subnormals (tie at the lowest bf16 subnormal, largest)
    0x00000000, 0x80000000,                                                     # +0, -0
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,                             # largest finite float -> inf; the last that stays finite; tie -> inf
    0x7F800000, 0xFF800000,                                                     # +inf, -inf
    0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF,                             # quiet and signalling NaN
], dtype=np.uint32).view(np.float32)


# --------------------------------------------------------------------------------------------------------------------- CPU tests
def test_philox_known_answer_vectors():
    """The three Random123 known-answer vectors of philox4x32_10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in rr.philox4x32_10(ctr, key)) == want
    # vectorised: the three at once
    got = rr.philox4x32_10([np.array([k[0][i] for k in kat], dtype=np.uint64) for i in range(4)],
                           [np.array([k[1][i] for k in kat], dtype=np.uint64) for i in range(2)])
    assert [tuple(int(w[j]) for w in got) for j in range(3)] == [k[2] for k in kat]


def test_uniform_of_the_top_word_is_exactly_one():
    """((float)(c >> 8) + 0.5f) * 2^-24 is 1.0f at c >> 8 == 0xFFFFFF, 2^-25 at 0, and the + 0.5 is rounded away from 2^23 on."""
    u = rr.philox_uniform32(np.array([0xFFFFFFFF, 0x000000FF, 0x80000000, 0x7FFFFFFF], dtype=np.uint64))
    assert u.dtype == np.float32 and u[0] == F32(1.0) and u[1] == F32(2.0 ** -25) and u[2] == F32(0.5) and u[3] == F32((2 ** 23 - 0.5) * 2.0 ** -24)


class _Env:
    def __init__(self, N, O):
        self.num_envs, self.obs_dim, self.act_dim, self.device = N, O, 1, "cpu"
        self.observation_space = self.action_space = None


@pytest.mark.parametrize("flags", [(True, True, True), (True, False, False), (False, True, True)], ids=lambda f: "train%d-obs%d-rew%d" % f)
def test_vecnorm_ref_matches_process_step(flags):
    """vecnorm_step_ref against VecNormalize.process_step (the torch statement of SB3's step_wait) on the CPU, six steps with
    episode ends; 300 rows, so three blocks of the bound's block structure."""
    from myochallenge_amd.rl.vec_normalize import VecNormalize
    training, norm_obs, norm_reward = flags
    N, O = 300, 5
    rng = np.random.default_rng(3)
    vn = VecNormalize(_Env(N, O), training=training, norm_obs=norm_obs, norm_reward=norm_reward)
    state = rr.vecnorm_init_state(N, O)
    if not training:                                 # something to normalise with
        vn.obs_rms.load(np.arange(O) * 0.1, 1.0 + np.arange(O), 77.0)
        vn.ret_rms.load(0.3, 2.5, 77.0)
        state.update(obs_mean=np.arange(O) * 0.1, obs_var=1.0 + np.arange(O), obs_count=77.0, ret_mean=0.3, ret_var=2.5, ret_count=77.0)
    for step in range(6):
        obs = (rng.standard_normal((N, O)) * (1 + step) + 0.5 * step).astype(F32)
        obs[:, 1] = 0.75
        obs[0, 2] = 1000.0
        term = (rng.standard_normal((N, O)) * 30).astype(F32)
        rew = (rng.standard_normal(N) * 3).astype(F32)
        done = (rng.random(N) < 0.2).astype(np.uint8)
        t = torch.from_numpy
        nobs, nrew, _, _, nterm, _, _ = vn.process_step(t(obs), t(rew), t(done), t(done), t(term), None, None)
        state, out = rr.vecnorm_step_ref(state, obs, rew, done, term, training=training, norm_obs=norm_obs, norm_reward=norm_reward)
        close = lambda a, b: np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=1e-12, atol=1e-300)
        assert close(state["obs_mean"], vn.obs_rms.mean.numpy()) and close(state["obs_var"], vn.obs_rms.var.numpy())
        assert close(state["ret_mean"], float(vn.ret_rms.mean)) and close(state["ret_var"], float(vn.ret_rms.var))
        assert state["obs_count"] == float(vn.obs_rms.count) and state["ret_count"] == float(vn.ret_rms.count)
        assert close(state["returns"], vn.returns.numpy())
        # torch rounds its own float64 value to fp32: the same value up to float64 noise ahead of the rounding
        for a, b in ((out["nobs"], nobs), (out["nterm"], nterm), (out["nrew"], nrew)):
            assert np.allclose(a, b.numpy().astype(np.float64), rtol=2 * U32, atol=1e-30)
        assert bool((np.abs(out["nterm"]) == 10.0).any()) or not norm_obs
        if training and norm_obs:                      # the counted bound stays a few dozen roundings of the quantity itself
            assert np.all(out["e_obs_var"] <= 1e-13 * state["obs_var"]) and np.all(out["e_obs_mean"] <= 1e-13 * (np.abs(state["obs_mean"]) + np.sqrt(state["obs_var"])))
    assert np.array_equal(state["starts"], done.astype(F32))


def test_gae_ref_matches_compute_gae():
    from myochallenge_amd.rl.ppo import compute_gae
    rng = np.random.default_rng(5)
    T, N = 9, 23
    rew, val = rng.standard_normal((T, N)).astype(F32), (50 + rng.standard_normal((T, N))).astype(F32)
    starts, lv, ld = (rng.random((T, N)) < 0.3).astype(F32), rng.standard_normal(N).astype(F32), (rng.random(N) < 0.5).astype(F32)
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.0, 0.9)):
        adv, ret, e_adv, e_ret = rr.gae_ref(rew, val, starts, lv, ld, gamma, lam)
        t = lambda a: torch.from_numpy(a).double()
        a_t, r_t = compute_gae(t(rew), t(val), t(starts), t(lv), t(ld), float(F32(gamma)), float(F32(lam)))
        assert np.allclose(adv, a_t.numpy(), rtol=1e-13, atol=1e-12) and np.allclose(ret, r_t.numpy(), rtol=1e-13, atol=1e-12)
        # the fp32 torch loop is one admissible rounding of the same scan: it lies inside the carried bound
        a32, r32 = compute_gae(*(torch.from_numpy(x) for x in (rew, val, starts, lv, ld)), float(F32(gamma)), float(F32(lam)))
        assert np.all(np.abs(a32.numpy() - adv) <= e_adv) and np.all(np.abs(r32.numpy() - ret) <= e_ret)
        assert float(e_adv.max()) < 1e-3


def test_adam_ref_matches_torch_clip_and_adam():
    """adam_ref against clip_grad_norm_ + torch.optim.Adam in float64 on the CPU: clipped, unclipped, scaled, max_norm = 0."""
    rng = np.random.default_rng(7)
    n = 1000
    f = lambda x: float(F32(x))
    lr, b1, b2, eps = f(2.5e-4), f(0.9), f(0.999), f(1e-5)
    p = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(F32)).double())
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    pm, m, v = p.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    for t, (scale, max_norm, gs) in enumerate([(10.0, 0.5, 1.0), (1e-3, 0.5, 1.0), (10.0, 0.5, 0.5), (0.1, 0.0, 1.0), (0.0, 0.5, 1.0)], start=1):
        g = (rng.standard_normal(n) * scale).astype(F32)
        p.grad = torch.from_numpy(g).double() * f(gs)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([p], f(max_norm))
        opt.step()
        r = rr.adam_ref(pm, m, v, g, t, lr, b1, b2, eps, max_norm, gs)
        assert (r["clip"] < 1.0) == (scale == 10.0)
        st = opt.state[p]
        assert np.allclose(r["p"], p.detach().numpy(), rtol=1e-12, atol=1e-15)
        assert np.allclose(r["m"], st["exp_avg"].numpy(), rtol=1e-11, atol=1e-300) and np.allclose(r["v"], st["exp_avg_sq"].numpy(), rtol=1e-11, atol=1e-300)
        assert np.all(r["e_p"] < 1e-4) and np.all(r["e_m"] >= 0) and np.all(r["e_v"] >= 0)
        pm, m, v = r["p"], r["m"], r["v"]


def test_sde_ref_and_gaussian_logp_match_torch_normal():
    rng = np.random.default_rng(9)
    N, L, A = 4, 6, 5
    mean, latent = rng.standard_normal((N, A)).astype(F32), np.maximum(rng.standard_normal((N, L)), 0).astype(F32)
    log_std = (-2 + 0.2 * rng.standard_normal((L, A))).astype(F32)
    W = (rng.standard_normal((N, L, A)) * np.exp(log_std)).astype(F32)
    stored = (mean + 0.05 * rng.standard_normal((N, A))).astype(F32)
    act, sigma, logp, e_noise, e_logp = rr.sde_sample_ref(mean, latent, W, log_std, stored)
    t = lambda a: torch.from_numpy(a).double()
    sg = torch.sqrt((t(latent) ** 2) @ (torch.exp(t(log_std)) ** 2) + float(F32(1e-6)))
    assert np.allclose(act, (t(mean) + torch.bmm(t(latent).unsqueeze(1), t(W)).squeeze(1)).numpy(), rtol=1e-14, atol=1e-15)
    assert np.allclose(sigma, sg.numpy(), rtol=1e-14)
    assert np.allclose(logp, torch.distributions.Normal(t(mean), sg).log_prob(t(stored)).sum(-1).numpy(), rtol=1e-13)
    assert np.all(e_logp > 0) and np.all(e_logp < 1e-2 * np.abs(logp))
    ls = (-1 + 0.3 * rng.standard_normal(A)).astype(F32)
    assert np.allclose(rr.gauss_logp(stored, mean, ls), torch.distributions.Normal(t(mean), torch.exp(t(ls))).log_prob(t(stored)).sum(-1).numpy(), rtol=1e-13)


def test_bf16_rne_matches_torch_on_edges():
    """Ties, subnormals, -0, the largest finite float (rounds to inf), +-inf: the bits of torch's .bfloat16(); NaN stays NaN."""
    rng = np.random.default_rng(11)
    x = np.concatenate([BF16_EDGES, rng.standard_normal(1000).astype(F32), rng.integers(0, 2 ** 32, 5000, dtype=np.uint64).astype(np.uint32).view(F32)])
    got = rr.bf16_bits(x)
    want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.all(np.isnan(rr.bf16_rne(x)[nan])) and bool(torch.from_numpy(x).bfloat16().float().isnan()[torch.from_numpy(nan)].all())
    assert int(rr.bf16_bits(np.array([0x7F7FFFFF], dtype=np.uint32).view(F32))[0]) == 0x7F80
    assert rr.bf16_bits(F32(-0.0).reshape(1))[0] == 0x8000 and np.array_equal(rr.bf16_rne(x)[~nan], torch.from_numpy(x).bfloat16().float().numpy()[~nan])


def test_gather_ref_matches_torch_moments():
    rng = np.random.default_rng(13)
    adv = (100 + rng.standard_normal(500)).astype(F32)
    for B in (1, 17, 1040):
        idx = rng.integers(0, 500, B)
        mean, std, e_mean, e_std = rr.gather_ref(adv, idx)
        a = torch.from_numpy(adv).double()[torch.from_numpy(idx)]
        assert abs(mean - float(a.mean())) < 1e-12 and (B == 1 or abs(std - float(a.std())) < 1e-12)
        assert 0 < e_mean < 1e-3 and (std == 0.0 and e_std == 0.0 if B == 1 else 0 < e_std < 1e-3)


# the two blocks of test_gaussian_sampler_extreme_uniforms, found once with the host Philox (env < 32, group < 10, counter varied)
EXTREME_SEED = 20240607
EXTREME_ONE = dict(ctr=170712, env=20, group=5)      # first word 0xFFFFFF1A: c >> 8 == 0xFFFFFF, u1 == 1.0f
EXTREME_ZERO = dict(ctr=76384, env=16, group=1)      # first word 0x00000025: c >> 8 == 0,        u1 == 2^-25


def _extreme_block(b):
    w = rr.philox4x32_10((b["env"], b["group"], b["ctr"] & 0xFFFFFFFF, b["ctr"] >> 32), (EXTREME_SEED & 0xFFFFFFFF, EXTREME_SEED >> 32))
    return [int(x) for x in w]


def test_extreme_blocks_have_the_property():
    w1, w0 = _extreme_block(EXTREME_ONE), _extreme_block(EXTREME_ZERO)
    assert w1[0] >> 8 == 0xFFFFFF and rr.philox_uniform32(np.uint64(w1[0])) == F32(1.0)
    assert w0[0] >> 8 == 0 and rr.philox_uniform32(np.uint64(w0[0])) == F32(2.0 ** -25)
    assert EXTREME_ONE["env"] < 32 and EXTREME_ZERO["env"] < 32 and EXTREME_ONE["group"] < 10 and EXTREME_ZERO["group"] < 10


# ---------------------------------------------------------------------------------------------------------- GPU: VecNormalize
VN_T = 3


def _vn_inputs(N, O, step, rng, ill=False):
    """Inputs of one step: column 1 constant (variance 0), column 2 small values with one outlier (normalised beyond clip_obs from
    128 rows on), terminal observations far outside (clipped at every N), rewards of mean 5 and spread 0.4 (the first step's
    normalised rewards lie around 12.5: beyond clip_reward) and dones / truncations.  ill: column 1 has mean 1e3 and spread 1e-2 instead."""
    obs = (rng.standard_normal((N, O)) * (1 + step) + 0.5 * step).astype(F32)
    if O >= 2:
        obs[:, 1] = (1000.0 + 0.01 * rng.standard_normal(N)).astype(F32) if ill else F32(0.75)
    if O >= 3:
        obs[:, 2] = (0.01 * rng.standard_normal(N)).astype(F32)
        obs[0, 2] = 1000.0
    term = (rng.standard_normal((N, O)) * 3).astype(F32)
    term[:, 0] = 1e6 * np.where(rng.random(N) < 0.5, -1, 1)
    rew = (5.0 + 0.4 * rng.standard_normal(N)).astype(F32)
    done = (rng.random(N) < 0.3).astype(np.uint8)
    done[0] = step % 2
    trunc = ((rng.random(N) < 0.5) & (done > 0)).astype(np.uint8)
    return obs, term, rew, done, trunc


class _VecNorm:
    """Device state of one VecNormalize (SB3's initial state) and the rollout-buffer rows it writes."""

    def __init__(self, N, O):
        self.N, self.O = N, O
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
        self.obs_mean, self.obs_var, self.obs_count, self.ret_stats, self.returns = z(O), z(O) + 1, z(1) + 1e-4, z(3), z(N)
        self.ret_stats[1], self.ret_stats[2] = 1.0, 1e-4
        self.starts = torch.ones(N, device=DEV)
        self.t_idx = torch.zeros(1, dtype=torch.int32, device=DEV)
        nb = (N + rr.VN_ROWS - 1) // rr.VN_ROWS
        self.work = Buf(nb * 2 * (O + 1), torch.float64)
        self.nobs, self.rew_buf, self.start_buf = Buf((N, O)), Buf((VN_T, N)), Buf((VN_T, N))
        self.term_buf, self.trunc_buf = Buf((VN_T, N, O)), Buf((VN_T, N))
        self.bufs = dict(work=self.work, nobs=self.nobs, rew_buf=self.rew_buf, start_buf=self.start_buf, term_buf=self.term_buf, trunc_buf=self.trunc_buf)

    def state(self):
        rs = host(self.ret_stats)
        return {"obs_mean": host(self.obs_mean).copy(), "obs_var": host(self.obs_var).copy(), "obs_count": float(host(self.obs_count)[0]),
                "ret_mean": float(rs[0]), "ret_var": float(rs[1]), "ret_count": float(rs[2]), "returns": host(self.returns).copy(),
                "starts": host(self.starts).copy()}

    def check(self, before, new, out, tt, flags, done, trunc, null_bufs, label):
        """The device state and rows against the reference step taken from `before` (the device state ahead of the launch)."""
        training, norm_obs, norm_reward = flags
        got = self.state()
        if training and norm_obs:
            within(label + " obs mean", got["obs_mean"], new["obs_mean"], out["e_obs_mean"])
            within(label + " obs var", got["obs_var"], new["obs_var"], out["e_obs_var"])
        else:
            assert np.array_equal(got["obs_mean"], before["obs_mean"]) and np.array_equal(got["obs_var"], before["obs_var"])
        if training:
            within(label + " ret mean", got["ret_mean"], new["ret_mean"], out["e_ret_mean"])
            within(label + " ret var", got["ret_var"], new["ret_var"], out["e_ret_var"])
        else:
            assert (got["ret_mean"], got["ret_var"]) == (before["ret_mean"], before["ret_var"])
        assert got["obs_count"] == new["obs_count"] and got["ret_count"] == new["ret_count"]
        dn = done != 0
        assert np.all(got["returns"][dn] == 0.0)
        within(label + " returns", got["returns"], new["returns"], np.where(dn, 0.0, out["e_returns"]))
        if norm_obs:
            within(label + " nobs", host(self.nobs), out["nobs"], out["e_nobs"])
        else:
            assert np.array_equal(host(self.nobs), out["nobs"].astype(F32))
        if norm_reward:
            within(label + " rew row", host(self.rew_buf)[tt], out["nrew"], out["e_nrew"])
        else:
            assert np.array_equal(host(self.rew_buf)[tt], out["nrew"].astype(F32))
        # bookkeeping: exact
        assert np.array_equal(host(self.start_buf)[tt], before["starts"]) and np.array_equal(got["starts"], dn.astype(F32))
        others = [r for r in range(VN_T) if r != tt]
        assert self.rew_buf.untouched(others) and self.start_buf.untouched(others)
        if null_bufs:
            assert self.term_buf.untouched(slice(None)) and self.trunc_buf.untouched(slice(None))
        else:
            if norm_obs:
                within(label + " term row", host(self.term_buf)[tt], out["nterm"], out["e_nterm"])
            else:
                assert np.array_equal(host(self.term_buf)[tt], out["nterm"].astype(F32))
            assert np.array_equal(host(self.trunc_buf)[tt], (trunc != 0).astype(F32))
            assert self.term_buf.untouched(others) and self.trunc_buf.untouched(others)
        for name, b in self.bufs.items():
            b.check_guards(label + " " + name)


def _vn_run(hip_lib, N, O, steps, flags=(1, 1, 1), null_from=None, seed=0):
    """`steps` consecutive myo_vecnorm_step launches; each is checked against the reference step from the device state before it."""
    rng = np.random.default_rng(1000 * N + O + seed)
    vn = _VecNorm(N, O)
    training, norm_obs, norm_reward = flags
    gamma, eps, clip_obs, clip_rew = 0.99, 1e-8, 10.0, 10.0
    hit = dict(obs=False, term=False, rew=False)
    rel = dict(mean=0.0, var=0.0)
    for step in range(steps):
        obs, term, rew, done, trunc = _vn_inputs(N, O, step, rng)
        tt = step % VN_T                                   # rows 0, 1, T - 1, 0
        null_bufs = null_from is not None and step >= null_from
        vn.t_idx.fill_(tt)
        for b in (vn.nobs, vn.rew_buf, vn.start_buf, vn.term_buf, vn.trunc_buf, vn.work):
            b.refill()
        before = vn.state()
        d = [dev_of(x) for x in (obs, rew, done, trunc, term)]
        hip_lib.check(hip_lib.L.myo_vecnorm_step(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), N, O, ptr(vn.obs_mean), ptr(vn.obs_var),
                                                 ptr(vn.obs_count), ptr(vn.ret_stats), ptr(vn.returns), gamma, eps, clip_obs, clip_rew,
                                                 int(training), int(norm_obs), int(norm_reward), ptr(vn.nobs), ptr(vn.starts), ptr(vn.t_idx),
                                                 ptr(vn.rew_buf), ptr(vn.start_buf), None if null_bufs else ptr(vn.term_buf),
                                                 None if null_bufs else ptr(vn.trunc_buf), ptr(vn.work), None))
        torch.cuda.synchronize()
        new, out = rr.vecnorm_step_ref(before, obs, rew, done, term, gamma, eps, clip_obs, clip_rew, bool(training), bool(norm_obs), bool(norm_reward))
        vn.check(before, new, out, tt, flags, done, trunc, null_bufs, "N%d-O%d step %d" % (N, O, step))
        if training:
            # the count must keep the bound under 1e-13: relative to |mean| + sqrt(var) for the mean, to var for the variance
            sd = np.sqrt(new["obs_var"])
            rel["mean"] = max(rel["mean"], float((out["e_obs_mean"] / (np.abs(new["obs_mean"]) + sd)).max()), out["e_ret_mean"] / (abs(new["ret_mean"]) + math.sqrt(new["ret_var"])))
            rel["var"] = max(rel["var"], float((out["e_obs_var"] / new["obs_var"]).max()), out["e_ret_var"] / new["ret_var"])
        hit["obs"] |= bool((np.abs(out["nobs"]) == clip_obs).any())
        hit["term"] |= bool((np.abs(out["nterm"]) == clip_obs).any())
        hit["rew"] |= bool((np.abs(out["nrew"]) == clip_rew).any())
    return hit, rel


VN_SHAPES = [(1, 1), (2, 3), (7, 5), (128, 64), (129, 65), (1025, 7), (2053, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", VN_SHAPES, ids=lambda s: "N%d-O%d" % s)
def test_vecnorm_step(hip_lib, shape):
    """myo_vecnorm_step, four consecutive steps from SB3's initial state (count 1e-4, var 1), rows 0, 1, T - 1, 0 of the rollout
    buffers.  Chunks of 1, 2 and 7 rows (the 8-row unrolled body never runs, one half column is empty at N = 1), the odd tail
    behind a full chunk (129), O < 64 and O = 65 (one live lane pair in the second column pass), 9 blocks (k_vecnorm_merge's
    partial second group) and 17 (two full groups and one block).
    Statistics: fp64 roundings of the kernel's order, counted in rollout_ref._batch_moments and chan_merge — 15 for a block mean
    (4 accumulators of a half column: 8 + 3 adds, the tree 2, the pair shuffle 1, the division 1), 16 for a block M2, 17 + nb and
    21 + nb for the block merge, 5 and 9 for Chan's update: depth * 2^-53 * sum |terms|, 54 roundings at 17 blocks.  That bound
    stays under 1e-13 of |mean| + sqrt(var) and of var on these inputs (asserted).  Normalised outputs: one fp32 rounding of the
    float64 reference plus the propagated statistic error.  Bookkeeping rows and zeroed returns: exact."""
    N, O = shape
    hit, rel = _vn_run(hip_lib, N, O, 4)
    assert rel["mean"] < 1e-13 and rel["var"] < 1e-13, rel
    assert hit["term"] and hit["rew"] and (hit["obs"] or N < 128 or O < 3), hit


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [(t, o, r) for t in (0, 1) for o in (0, 1) for r in (0, 1)], ids=lambda f: "train%d-obs%d-rew%d" % f)
def test_vecnorm_flags_and_null_buffers(hip_lib, flags):
    """(129, 65) under the eight combinations of training, norm_obs, norm_reward: two steps with all buffers, a third with
    term_buf = trunc_buf = NULL (those buffers keep their sentinel).  training = 0 leaves statistics and returns as they are,
    norm_obs = 0 leaves the observation statistics (the returns' are still updated) and passes observations through bit for
    bit, norm_reward = 0 passes the rewards through."""
    _vn_run(hip_lib, 129, 65, 3, flags=flags, null_from=2, seed=7)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cuts", [((1025, 7), (400,)), ((1025, 7), (130, 131)), ((129, 65), (1,)), ((129, 65), (64, 127))],
                         ids=lambda v: "-".join(str(x) for x in v))
def test_vecnorm_multi_rank_form(hip_lib, shape, cuts):
    """myo_vecnorm_batch_moments per row shard, the `batch` vectors added in shard order (float64 torch add, what the all-reduce
    does), myo_vecnorm_finish per shard: two steps, two and three unequal shards.  Every shard ends with the same statistics bit
    for bit, and they meet the reference over ALL rows.  The variance comes from additive sums, sum x^2 / n - mean^2: its bound is
    depth * 2^-53 * (mean^2 + var) (rollout_ref._batch_moments, sums_form: 16 + 4 + nb + shards + 30 + 2 (17 + nb + shards) + 3),
    which for well-conditioned columns is the size of the single-rank bound and for column 1 (mean 1e3, spread 1e-2) allows a
    relative loss of depth * 2^-53 * 1e10 = 1.0e-4 .. 1.4e-4 of the batch variance.  Measured on the MI355X: 7.9e-8 .. 1.3e-6
    (printed per step; recorded in DESIGN.md section 8)."""
    N, O = shape
    edges = [0] + list(cuts) + [N]
    shards = [slice(a, b) for a, b in zip(edges[:-1], edges[1:])]
    P = len(shards)
    rng = np.random.default_rng(N + O + P)
    ranks = [_VecNorm(s.stop - s.start, O) for s in shards]
    batches = [Buf(2 * O + 3, torch.float64) for _ in shards]
    gamma, eps, clip_obs, clip_rew = 0.99, 1e-8, 10.0, 10.0
    L = hip_lib.L
    for step in range(2):
        obs, term, rew, done, trunc = _vn_inputs(N, O, step, rng, ill=True)
        tt = (VN_T - 1) if step else 0
        before = ranks[0].state()
        before["returns"] = np.concatenate([host(r.returns) for r in ranks])
        before["starts"] = np.concatenate([host(r.starts) for r in ranks])
        dev = []
        for r, s, b in zip(ranks, shards, batches):
            r.t_idx.fill_(tt)
            for x in (r.nobs, r.rew_buf, r.start_buf, r.term_buf, r.trunc_buf, r.work, b):
                x.refill()
            d = [dev_of(x[s]) for x in (obs, rew, done, trunc, term)]
            dev.append(d)
            hip_lib.check(L.myo_vecnorm_batch_moments(ptr(d[0]), ptr(d[1]), r.N, O, ptr(r.returns), gamma, 1, ptr(r.work), ptr(b), None))
        torch.cuda.synchronize()
        total = batches[0].t.clone()
        for b in batches[1:]:
            total = total + b.t
        assert float(total[0]) == N
        for r, d in zip(ranks, dev):
            hip_lib.check(L.myo_vecnorm_finish(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), r.N, O, ptr(r.obs_mean), ptr(r.obs_var),
                                               ptr(r.obs_count), ptr(r.ret_stats), ptr(r.returns), eps, clip_obs, clip_rew, 1, 1, 1, ptr(r.nobs),
                                               ptr(r.starts), ptr(r.t_idx), ptr(r.rew_buf), ptr(r.start_buf), ptr(r.term_buf), ptr(r.trunc_buf),
                                               ptr(total), None))
        torch.cuda.synchronize()
        for r in ranks[1:]:
            for a, b in ((r.obs_mean, ranks[0].obs_mean), (r.obs_var, ranks[0].obs_var), (r.obs_count, ranks[0].obs_count), (r.ret_stats, ranks[0].ret_stats)):
                assert torch.equal(a, b)
        for k, (r, s, b) in enumerate(zip(ranks, shards, batches)):
            new, out = rr.vecnorm_step_ref(before, obs, rew, done, term, gamma, eps, clip_obs, clip_rew, sums_form=True, parts=P, rows=s)
            part_before = dict(before, starts=before["starts"][s])
            new_part = dict(new, returns=new["returns"][s], starts=new["starts"][s])
            out_part = dict(out, e_returns=out["e_returns"][s], start_row=out["start_row"][s])
            r.check(part_before, new_part, out_part, tt, (1, 1, 1), done[s], trunc[s], False, "shard %d of %d step %d" % (k, P, step))
            b.check_guards("batch")
        # the batch variance's share of the running variance is bvar * N / tot: the running variance's error, scaled back by
        # tot / N, over the batch variance is what the sums form lost of it
        got, tot = host(ranks[0].obs_var)[1], new["obs_count"]
        loss = abs(got - new["obs_var"][1]) * tot / N / out["batch_obs_var"][1]
        allowed = out["e_batch_obs_var"][1] / out["batch_obs_var"][1]
        print("sums-form variance, column mean 1e3 spread 1e-2, N%d-O%d %d shards step %d: relative loss of the batch variance %.3e (bound %.3e)"
              % (N, O, P, step, loss, allowed))
        assert 1e-6 < allowed < 1e-2            # depth * 2^-53 * 1e10: the column is as ill-conditioned as intended


# ----------------------------------------------------------------------------------------------------- GPU: Gaussian sampler
SAMPLE_T = 3
SAMPLE_SEED = 0x1234ABCD5678EF01
SAMPLE_CASES = [(1, 1), (1, 4), (1, 65), (15, 3), (16, 39), (17, 39), (17, 64), (16, 65), (15, 130), (33, 1), (17, 4), (33, 130)]


class _Sampler:
    def __init__(self, hip_lib, N, A):
        self.lib, self.N, self.A = hip_lib, N, A
        self.act, self.val, self.logp, self.clipped = Buf((SAMPLE_T, N, A)), Buf((SAMPLE_T, N)), Buf((SAMPLE_T, N)), Buf((N, A))
        self.t_idx = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.draw = torch.zeros(2, dtype=torch.int64, device=DEV)

    def run(self, mean_h, value_h, log_std, seed, ctr, tt, det=0):
        for b in (self.act, self.val, self.logp, self.clipped):
            b.refill()
        self.t_idx.fill_(tt)
        self.draw.copy_(torch.tensor([ctr, -1], dtype=torch.int64))
        self.lib.check(self.lib.L.myo_rollout_sample(ptr(mean_h), ptr(value_h), ptr(log_std), self.N, self.A, seed, ptr(self.draw), ptr(self.t_idx),
                                                     ptr(self.act), ptr(self.val), ptr(self.logp), ptr(self.clipped), det, None))
        torch.cuda.synchronize()
        others = [r for r in range(SAMPLE_T) if r != tt]
        assert self.act.untouched(others) and self.val.untouched(others) and self.logp.untouched(others)
        for name, b in (("act", self.act), ("val", self.val), ("logp", self.logp), ("clipped", self.clipped)):
            b.check_guards(name)
        assert self.draw.tolist() == [ctr, ctr + 1] and self.t_idx.tolist() == [tt]          # the pending counter draw[1]
        act = host(self.act)[tt].astype(np.float64)
        assert np.array_equal(host(self.clipped), np.clip(host(self.act)[tt], -1.0, 1.0))
        assert np.array_equal(host(self.val)[tt], value_h.float().cpu().numpy().reshape(-1))
        return act, host(self.logp)[tt].astype(np.float64)


def _logp_bound(act, mean, ls, A):
    """test_rollout_policy_matches_reference_and_sampler's bound on the log-prob of the stored action, at this kernel's depth:
    z = (act - mean) * exp(-log_std) rounds the difference and the product once each and takes the fast exponential (<= 3 ulp =
    6 * 2^-24 for |log_std| < 1): 8 * 2^-24 on z, twice that plus the square's own rounding on the quadratic term (17); per action
    one rounding of (log_std + 1/2 ln 2 pi), 4 serial adds per 64 actions in the lane and the 4 levels of the 16-lane shuffle."""
    depth = 1 + 4 * ((A + 63) // 64) + 4
    zz = (act - mean) * np.exp(-ls)
    quad = 0.5 * zz * zz
    terms = quad + np.abs(ls + rr.HALF_LOG_2PI)
    return 17 * U32 * quad.sum(-1) + depth * U32 * terms.sum(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SAMPLE_CASES, ids=lambda c: "N%d-A%d" % c)
def test_gaussian_sampler(hip_lib, case):
    """myo_rollout_sample against the host Philox4x32-10 + Box-Muller: counter (env, action group, draw lo, draw hi), key (seed
    lo, seed hi with a non-zero high word).  N around the 16 rows of a block, A around the four actions of a Philox block and the
    64 of a lane pass.  With a bf16 zero mean and log_std = 0 the stored action is z itself: draw counter 5 into row 0 and
    2^32 + 5 into row T - 1 (the high word changes the noise), each within MARGIN = 64 times the case's twin, the largest
    |fp32 twin - float64| over every normal of every block both draws touch.  A third draw with a random log_std checks
    exp(log_std) z (the fast exponential and the product add 7 * 2^-24 |action|), the log-prob of the stored action, the clipped
    copy, the value column and the pending counter; deterministic = 1 returns the mean bit for bit.
    Measured kernel / twin on the MI355X: 0.03 .. 1.21 over the twelve cases, largest 1.21 at N15-A130 and N33-A130 (kernel
    1.29e-6, twin 1.07e-6): the fast functions cost no more than the twin's own angle rounding."""
    N, A = case
    s = _Sampler(hip_lib, N, A)
    rng = np.random.default_rng(100 * N + A)
    zeros_h = torch.zeros((N, A), dtype=torch.bfloat16, device=DEV)
    value_h = dev_of(rng.standard_normal(N).astype(F32)).bfloat16()
    ls0 = torch.zeros(A, device=DEV)
    hi = 2 ** 32 + 5
    ref = {c: rr.gauss_noise(SAMPLE_SEED, c, N, A) for c in (5, hi)}
    twin = max(float(np.abs(r[2]["z32"].astype(np.float64) - r[2]["z64"]).max()) for r in ref.values())
    assert 0 < twin < 1e-5
    z5, _ = s.run(zeros_h, value_h, ls0, SAMPLE_SEED, 5, 0)
    zhi, _ = s.run(zeros_h, value_h, ls0, SAMPLE_SEED, hi, SAMPLE_T - 1)
    assert not np.array_equal(z5, zhi)
    err = max(float(np.abs(z5 - ref[5][0]).max()), float(np.abs(zhi - ref[hi][0]).max()))
    print("sampler N%d-A%d: kernel err %.3e twin %.3e kernel/twin %.2f" % (N, A, err, twin, err / twin))
    assert np.all(np.isfinite(z5)) and np.all(np.isfinite(zhi))
    assert err <= MARGIN * twin, (err, twin)
    # ---- a random log_std, row 1
    ls = (-0.25 + 0.7 * (rng.random(A) - 0.5)).astype(F32)                                   # |log_std| < 1
    act, logp = s.run(zeros_h, value_h, dev_of(ls), SAMPLE_SEED, 5, 1)
    sd = np.exp(ls.astype(np.float64))
    within("exp(log_std) z", act, sd * ref[5][0], MARGIN * twin * sd + (rr.FASTEXP32 + 1) * U32 * np.abs(sd * ref[5][0]))
    within("log-prob", logp, rr.gauss_logp(act, 0.0, ls), _logp_bound(act, 0.0, ls.astype(np.float64), A))
    # ---- deterministic: the mean, bit for bit
    mean_h = dev_of((0.3 * rng.standard_normal((N, A))).astype(F32)).bfloat16()
    act, logp = s.run(mean_h, value_h, dev_of(ls), SAMPLE_SEED, 5, SAMPLE_T - 1, det=1)
    mean = mean_h.float().cpu().numpy()
    assert np.array_equal(act.astype(F32), mean)
    within("deterministic log-prob", logp, rr.gauss_logp(mean, mean, ls), _logp_bound(mean.astype(np.float64), mean.astype(np.float64), ls.astype(np.float64), A))


@pytest.mark.gpu
def test_gaussian_sampler_extreme_uniforms(hip_lib):
    """The two ends of ((float)(c >> 8) + 0.5f) * 2^-24: a block whose first word has c >> 8 == 0xFFFFFF (u1 == 1.0f exactly,
    since 16777215.5f rounds to 2^24: Box-Muller radius 0, the first pair of normals are exact zeros) and one with c >> 8 == 0
    (u1 = 2^-25, radius sqrt(50 ln 2) = 5.887).  Both blocks were found once with the host Philox and are re-derived here; the
    kernel's four normals of each must be finite and within MARGIN times the twin of the 32 x 40 draw they lie in.
    Measured kernel / twin over those draws on the MI355X: 1.36 and 2.26; every value finite, so the sampler's bits stay."""
    N, A = 32, 40
    s = _Sampler(hip_lib, N, A)
    zeros_h = torch.zeros((N, A), dtype=torch.bfloat16, device=DEV)
    value_h = torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    ls0 = torch.zeros(A, device=DEV)
    for blk, top in ((EXTREME_ONE, 0xFFFFFF), (EXTREME_ZERO, 0)):
        w = _extreme_block(blk)
        assert w[0] >> 8 == top
        z64, _, b = rr.gauss_noise(EXTREME_SEED, blk["ctr"], N, A)
        assert [int(x) for x in b["words"][blk["env"], blk["group"]]] == w
        twin = float(np.abs(b["z32"].astype(np.float64) - b["z64"]).max())
        z, _ = s.run(zeros_h, value_h, ls0, EXTREME_SEED, blk["ctr"], 0)
        assert np.all(np.isfinite(z))
        cols = slice(4 * blk["group"], 4 * blk["group"] + 4)
        four, want = z[blk["env"], cols], z64[blk["env"], cols]
        print("extreme block c >> 8 == %#x: kernel %s reference %s, kernel/twin over the draw %.2f"
              % (top, four.tolist(), want.tolist(), float(np.abs(z - z64).max()) / twin))
        assert float(np.abs(z - z64).max()) <= MARGIN * twin
        if top:
            assert b["u"][blk["env"], blk["group"], 0] == F32(1.0) and four[0] == 0.0 and four[1] == 0.0 and want[0] == 0.0 and want[1] == 0.0
        else:
            assert abs(math.hypot(want[0], want[1]) - math.sqrt(50 * math.log(2))) < 1e-12
            assert abs(math.hypot(four[0], four[1]) - math.sqrt(50 * math.log(2))) <= 2 * MARGIN * twin


# ------------------------------------------------------------------------------------------------------------- GPU: gSDE sampler
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 7, 39), (5, 256, 65), (2, 64, 130)], ids=lambda s: "N%d-L%d-A%d" % s)
def test_gsde_sampler(hip_lib, shape):
    """myo_rollout_sample_sde: one latent (L = 1), A below, above and twice the 64 lanes; from N = 2 on the last env has an all-zero
    latent (sigma at its 1e-6 floor, noise 0, the action is the mean).  With a zero mean the stored action is the noise and the
    bound is L * 2^-24 * sum |latent W| alone (L fused multiply-adds); with a non-zero mean action = fl(mean + noise) rounds once more
    (2^-24 |action|).  The log-prob is that of the action the kernel stored, under the float64 mean and sigma, within the counted
    roundings of rollout_ref.sde_sample_ref.  The clipped copy is exact; deterministic = 1 returns the mean."""
    N, L, A = shape
    rng = np.random.default_rng(N + 10 * L + A)
    latent = np.maximum(rng.standard_normal((N, L)), 0.05).astype(F32)
    if N > 1:
        latent[-1] = 0.0
    log_std = (-2.0 + 0.2 * rng.standard_normal((L, A))).astype(F32)
    W = (rng.standard_normal((N, L, A)) * np.exp(log_std)).astype(F32)
    act, clip, lp = Buf((N, A)), Buf((N, A)), Buf(N)
    d_lat, d_W, d_ls = dev_of(latent), dev_of(W), dev_of(log_std)
    for zero_mean in (True, False):
        mean = np.zeros((N, A), dtype=F32) if zero_mean else (0.3 * rng.standard_normal((N, A))).astype(F32)
        d_mean = dev_of(mean)
        for det in (0, 1):
            for b in (act, clip, lp):
                b.refill()
            hip_lib.check(hip_lib.L.myo_rollout_sample_sde(ptr(d_mean), ptr(d_lat), ptr(d_W), ptr(d_ls), N, L, A, ptr(act), ptr(clip), ptr(lp), det, None))
            torch.cuda.synchronize()
            for name, b in (("act", act), ("clip", clip), ("logp", lp)):
                b.check_guards(name)
            a = host(act)
            assert np.array_equal(host(clip), np.clip(a, -1.0, 1.0))
            a_ref, sigma, logp, e_noise, e_logp = rr.sde_sample_ref(mean, latent, W, log_std, a)
            if det:
                assert np.array_equal(a, mean)
            else:
                within("action", a, a_ref, e_noise + (0.0 if zero_mean else U32) * np.abs(a_ref))
                if N > 1:
                    assert np.array_equal(a[-1], mean[-1]) and np.allclose(sigma[-1], math.sqrt(float(F32(1e-6))), rtol=1e-15)
            within("log-prob", host(lp), logp, e_logp)


# ----------------------------------------------------------------------------------------------------------------------- GPU: GAE
@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 17])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_gae(hip_lib, T, N):
    """myo_gae: T = 1 (only the bootstrap value), N below, at and above the 256-thread block; (gamma, lambda) = (0.99, 0.95),
    (1, 1) (nothing decays: the bound grows linearly) and (0, 0.9) (the advantage is the one-step delta); episode starts all 0,
    all 1 and random; last_done mixed; values offset by + 50 so that the deltas cancel.  Every element lies within the bound
    E_t carried through the scan (rollout_ref.gae_ref: k = 6 fp32 roundings per trip)."""
    rng = np.random.default_rng(100 * T + N)
    rew = rng.standard_normal((T, N)).astype(F32)
    val, lv = (50 + rng.standard_normal((T, N))).astype(F32), (50 + rng.standard_normal(N)).astype(F32)
    ld = (rng.random(N) < 0.5).astype(F32)
    adv, ret = Buf((T, N)), Buf((T, N))
    d = [dev_of(x) for x in (rew, val, lv, ld)]
    for mode in ("zeros", "ones", "random"):
        starts = {"zeros": np.zeros((T, N)), "ones": np.ones((T, N)), "random": rng.random((T, N)) < 0.3}[mode].astype(F32)
        d_st = dev_of(starts)
        for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.0, 0.9)):
            adv.refill(); ret.refill()
            hip_lib.check(hip_lib.L.myo_gae(ptr(d[0]), ptr(d[1]), ptr(d_st), ptr(d[2]), ptr(d[3]), T, N, gamma, lam, ptr(adv), ptr(ret), None))
            torch.cuda.synchronize()
            a_ref, r_ref, e_adv, e_ret = rr.gae_ref(rew, val, starts, lv, ld, gamma, lam)
            label = "starts %s gamma %g lambda %g" % (mode, gamma, lam)
            within(label + " adv", host(adv), a_ref, e_adv)
            within(label + " ret", host(ret), r_ref, e_ret)
            adv.check_guards("adv"); ret.check_guards("ret")


# -------------------------------------------------------------------------------------------------------------------- GPU: gather
GATHER_CASES = [(1, 1, 1, 1), (15, 3, 39, 2), (16, 86, 1, 3), (17, 1, 39, 1), (1040, 3, 1, 2), (1040, 86, 39, 1), (2049, 86, 39, 3), (2049, 1, 1, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GATHER_CASES, ids=lambda c: "B%d-O%d-A%d-copies%d" % c)
def test_gather(hip_lib, case):
    """myo_ppo_gather: B around the 16 rows of a block; 65 and 129 blocks (B = 1040, 2049) run the second and third strided trip
    of k_moments_finish.  Indices with repeats, the bf16 edge values of the CPU test among the gathered observations, advantages
    offset by + 100.  Copies are exact, bf16 observations equal bf16_rne in every stacked copy, mean and unbiased std against
    exact summation within the counted fp32 bound of rollout_ref.gather_ref; at B = 1 the std is 0."""
    B, O, A, copies = case
    R = 300
    rng = np.random.default_rng(B + O + A)
    obs = rng.standard_normal((R, O)).astype(F32)
    obs.reshape(-1)[:min(BF16_EDGES.size, R * O)] = BF16_EDGES[:min(BF16_EDGES.size, R * O)]
    act, lp, ret = rng.standard_normal((R, A)).astype(F32), rng.standard_normal(R).astype(F32), rng.standard_normal(R).astype(F32)
    adv = (100 + rng.standard_normal(R)).astype(F32)
    idx = rng.integers(0, R, B).astype(np.int64)
    edge_rows = (BF16_EDGES.size + O - 1) // O
    idx[:min(B, edge_rows)] = np.arange(min(B, edge_rows))
    if B > 40:
        idx[20:24] = idx[19]                                       # repeats inside a block and across two
    nb = (B + rr.GATHER_ROWS - 1) // rr.GATHER_ROWS
    x_h = Buf((copies, B, O), torch.int16, fill=0x5A5A)
    a_mb, lp_mb, adv_mb, ret_mb, st, work = Buf((B, A)), Buf(B), Buf(B), Buf(B), Buf(2), Buf(2 * nb)
    d = [dev_of(x) for x in (obs, act, lp, adv, ret, idx)]
    hip_lib.check(hip_lib.L.myo_ppo_gather(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(d[4]), ptr(d[5]), B, O, A, ptr(x_h), copies,
                                           ptr(a_mb), ptr(lp_mb), ptr(adv_mb), ptr(ret_mb), ptr(st), ptr(work), None))
    torch.cuda.synchronize()
    for name, b in (("x_h", x_h), ("act", a_mb), ("logp", lp_mb), ("adv", adv_mb), ("ret", ret_mb), ("stats", st), ("work", work)):
        b.check_guards(name)
    bits = host(x_h).view(np.uint16)
    want = rr.bf16_bits(obs[idx])
    for k in range(copies):
        assert np.array_equal(bits[k], want), "copy %d" % k
    same = lambda got, ref: np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert same(host(a_mb), act[idx]) and same(host(lp_mb), lp[idx]) and same(host(adv_mb), adv[idx]) and same(host(ret_mb), ret[idx])
    mean, std, e_mean, e_std = rr.gather_ref(adv, idx)
    got = host(st).astype(np.float64)
    within("advantage mean", got[0], mean, e_mean)
    within("advantage std", got[1], std, e_std)
    if B == 1:
        assert got[1] == 0.0


@pytest.mark.gpu
def test_policy_input_on_bf16_edges(hip_lib):
    """myo_rollout_policy_input on the edge values: row t_idx of obs_buf takes the fp32 bits, every stacked bf16 copy equals
    bf16_rne (ties, subnormals, -0, the largest finite float -> inf, +-inf, NaN with its quiet bit); other rows keep the sentinel."""
    N, O, T, copies = 5, 7, 3, 2
    obs = np.resize(BF16_EDGES, N * O).reshape(N, O)
    obs_buf, x_h = Buf((T, N, O)), Buf((copies, N, O), torch.int16, fill=0x5A5A)
    t_idx = torch.tensor([1], dtype=torch.int32, device=DEV)
    d_obs = dev_of(obs)
    hip_lib.check(hip_lib.L.myo_rollout_policy_input(ptr(d_obs), N, O, ptr(obs_buf), ptr(x_h), copies, ptr(t_idx), None))
    torch.cuda.synchronize()
    obs_buf.check_guards("obs_buf"); x_h.check_guards("x_h")
    assert np.array_equal(host(obs_buf)[1].view(np.uint32), obs.view(np.uint32)) and obs_buf.untouched([0, 2])
    bits = host(x_h).view(np.uint16)
    assert np.array_equal(bits[0], rr.bf16_bits(obs)) and np.array_equal(bits[1], bits[0])
    x_h.refill()
    hip_lib.check(hip_lib.L.myo_rollout_policy_input(ptr(d_obs), N, O, None, ptr(x_h), 1, ptr(t_idx), None))      # no rollout buffer, one copy
    torch.cuda.synchronize()
    bits = host(x_h).view(np.uint16)
    assert np.array_equal(bits[0], rr.bf16_bits(obs)) and bool((x_h.t[1] == 0x5A5A).all())


# ---------------------------------------------------------------------------------------------------------------------- GPU: Adam
class _Adam:
    def __init__(self, hip_lib, n, rng):
        from myochallenge_amd import native
        self.lib, self.n = hip_lib, n
        self.p, self.m, self.v = Buf(n), Buf(n), Buf(n)
        self.p.t.copy_(dev_of(rng.standard_normal(n).astype(F32)))
        self.m.t.zero_(); self.v.t.zero_()
        self.shadow = Buf(n, torch.int16, fill=0x5A5A)
        self.scratch = Buf(rr.SQN_BLOCKS)
        self.step = Buf(2, torch.int32, fill=0)
        self.g = torch.zeros(n, device=DEV)
        self.hyper = dict(lr=2.5e-4, b1=0.9, b2=0.999, eps=1e-5)
        self.desc = native.AdamDesc(p=self.p.t.data_ptr(), g=self.g.data_ptr(), m=self.m.t.data_ptr(), v=self.v.t.data_ptr(), n=n,
                                    step=self.step.t.data_ptr(), scratch=self.scratch.t.data_ptr(), nparts=0, p_bf16=self.shadow.t.data_ptr(),
                                    hp=None, **self.hyper)

    def run(self, g, t, max_norm, gs, label):
        before = [host(x).copy() for x in (self.p, self.m, self.v)]
        self.g.copy_(dev_of(g))
        self.desc.max_norm, self.desc.grad_scale = max_norm, gs
        self.lib.check(self.lib.L.myo_adam_step(C.byref(self.desc), None))
        torch.cuda.synchronize()
        for name, b in (("p", self.p), ("m", self.m), ("v", self.v), ("shadow", self.shadow), ("scratch", self.scratch), ("step", self.step)):
            b.check_guards(label + " " + name)
        assert host(self.step).tolist() == [t - 1, t], label                                  # (committed, pending)
        r = rr.adam_ref(*before, g, t, max_norm=max_norm, grad_scale=gs, **self.hyper)
        assert not 0.999 < r["ratio"] < 1.001, "the case sits on the clip threshold"
        ratios = [within(label + " " + k, host(b), r[k], r["e_" + k]) for k, b in (("p", self.p), ("m", self.m), ("v", self.v))]
        assert np.array_equal(host(self.shadow).view(np.uint16), rr.bf16_bits(host(self.p))), label + ": bf16 shadow"
        return r, ratios


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, 16385, 262147])
def test_adam(hip_lib, n):
    """myo_adam_step with nparts = 0 (k_grad_sqnorm + k_adam), no images, no hyper-parameter block: one element, both sides of a
    256-thread block, n > 16384 (k_grad_sqnorm's stride) and n > 262144 (k_adam's 1024-block grid stride).  Three steps from zero
    moments — clipped, unclipped, grad_scale = 0.5 — then the device step counter is set so that the next step is t = 10000
    (b1^t underflows, b2^t = 4.5e-5), then max_norm = 0 and an all-zero gradient.  p, m, v lie within rollout_ref.adam_ref's counted
    fp32 bound from the device state before the step (powf, sqrtf, rsqrtf at 2 ulp, powf's amplified by b^t / (1 - b^t); the norm
    from 64 block partials of a 256-lane tree); the bf16 shadow equals bf16_rne(p); the step pair reads (t - 1, t).  A zero gradient
    on zero moments leaves p as it is."""
    rng = np.random.default_rng(n)
    ad = _Adam(hip_lib, n, rng)
    randn = lambda s: (rng.standard_normal(n) * s).astype(F32)
    r, _ = ad.run(randn(10.0), 1, 0.5, 1.0, "t=1 clipped")
    assert r["clip"] < 1.0
    r, _ = ad.run(randn(0.01 / math.sqrt(n)), 2, 0.5, 1.0, "t=2 unclipped")
    assert r["clip"] == 1.0
    r, _ = ad.run(randn(10.0), 3, 0.5, 0.5, "t=3 grad_scale 0.5")
    assert r["clip"] < 1.0
    ad.step.t.copy_(torch.tensor([9998, 9999], dtype=torch.int32))
    r, _ = ad.run(randn(10.0), 10000, 0.5, 1.0, "t=10000")
    assert r["clip"] < 1.0
    r, _ = ad.run(randn(0.1), 10001, 0.0, 1.0, "t=10001 max_norm 0")
    assert r["clip"] == 1.0
    ad.run(np.zeros(n, dtype=F32), 10002, 0.5, 1.0, "t=10002 zero gradient")
    fresh = _Adam(hip_lib, n, rng)
    p0 = host(fresh.p).copy()
    fresh.run(np.zeros(n, dtype=F32), 1, 0.5, 1.0, "zero gradient on zero moments")
    assert np.array_equal(host(fresh.p), p0) and not host(fresh.m).any() and not host(fresh.v).any()
