"""Float64 / exact references of the rollout and optimizer plumbing kernels of csrc/myobatch.hip, in numpy and python only.

No GPU and no native library in here.  Inputs are the fp32 arrays the kernels get, widened exactly; every reference returns
the value in float64 and, where the kernel rounds, a BOUND on |kernel - reference| counted from the kernel's own order of
operations (u32 = 2^-24 and u64 = 2^-53 are the relative errors of one rounding).  A sum rounded `depth` times in any order
errs by at most depth * u * sum |terms| (first order); products and quotients add their relative errors.

* philox4x32_10 / gauss_noise      k_sample_actions (and its copy in k_mlp_policy)
* vecnorm_step_ref                 k_vecnorm_moments + k_vecnorm_merge (or k_vecnorm_batch + k_vecnorm_merge_batch) + k_vecnorm_apply
* gae_ref                          k_gae
* adam_ref                         k_grad_sqnorm + k_adam
* sde_sample_ref                   k_sample_sde
* gather_ref                       k_ppo_gather + k_moments_finish
* bf16_rne / bf16_bits             myo_f2bf
"""
import math

import mpmath
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
VN_ROWS = 128            # MYO_VN_ROWS
GATHER_ROWS = 16         # MYO_GATHER_ROWS
SQN_BLOCKS = 64          # MYO_SQN_BLOCKS
# fp32 function errors in units of u32 (1 ulp <= 2 u32).  The build passes -fno-hip-fp32-correctly-rounded-divide-sqrt: an fp32
# `/` is then OpenCL's 2.5 ulp division.  powf, sqrtf, rsqrtf: 2 ulp each (no document in the ROCm tree states a figure).
DIV32, SQRT32, RSQRT32, POW32, LOG32, FASTEXP32 = 5.0, 4.0, 4.0, 4.0, 6.0, 6.0

mpmath.mp.dps = 50


# ------------------------------------------------------------------------------------------------------------------ bf16
def bf16_bits(x):
    """bf16 bit pattern (uint16) of fp32 values, round to nearest even on the fp32 bit pattern; a NaN keeps its upper 16 bits and
    gets the quiet bit (myo_f2bf)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return np.where(nan, (u >> np.uint64(16)) | np.uint64(0x40), r).astype(np.uint16)


def bf16_rne(x):
    """x (fp32) rounded to the nearest bf16 value, as fp32."""
    return (bf16_bits(x).astype(np.uint32) << np.uint32(16)).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------- Philox
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32 with ten rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).  counter: four words,
    key: two words, each an integer or an array of uint64 holding 32-bit values (broadcast against each other).  Per round:
    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the key words are bumped by
    0x9E3779B9 and 0xBB67AE85.  Returns the four output words as uint64 arrays."""
    c = [np.asarray(w, dtype=np.uint64) & _MASK for w in counter]
    k0, k1 = (np.asarray(w, dtype=np.uint64) & _MASK for w in key)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def philox_uniform32(w):
    """The kernel's uniform of one output word, formed in fp32 exactly as it forms it: ((float)(w >> 8) + 0.5f) * 2^-24."""
    return (((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float32)


def gauss_noise(seed, ctr, N, A):
    """The standard normals of k_sample_actions for N envs and A actions at draw counter `ctr`: Philox block
    (env, a >> 2, ctr lo, ctr hi) under key (seed lo, seed hi) gives the normals of actions 4 (a >> 2) .. + 3 by Box-Muller,
    words (0, 1) -> z0 = r cos, z1 = r sin, words (2, 3) -> z2, z3, with r = sqrt(-2 ln u1) and angle 2 pi u2.
    Returns (z64, z32, blocks): z64 [N, A] from the fp32 uniforms with ln, sqrt, sin and cos in float64; z32 [N, A] the fp32 twin
    (every operation in numpy.float32 with numpy's accurate functions, the angle formed as the kernel forms it, 6.2831855f * u2);
    blocks = dict(words [N, G, 4] uint64, u [N, G, 4] float32, z64 / z32 [N, 4 G]: all four normals of every block drawn)."""
    G = (A + 3) // 4
    env, grp = np.meshgrid(np.arange(N, dtype=np.uint64), np.arange(G, dtype=np.uint64), indexing="ij")
    w = philox4x32_10((env, grp, np.uint64(ctr & 0xFFFFFFFF), np.uint64((ctr >> 32) & 0xFFFFFFFF)),
                      (np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)))
    words = np.stack(w, axis=-1)                                  # [N, G, 4]
    u = philox_uniform32(words)
    u1, u2 = u[..., 0::2], u[..., 1::2]                           # [N, G, 2]: pair h uses words 2h, 2h + 1
    r64 = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    ang64 = 2.0 * math.pi * u2.astype(np.float64)
    z64 = np.stack([r64 * np.cos(ang64), r64 * np.sin(ang64)], axis=-1).reshape(N, 4 * G)
    f = np.float32
    r32 = np.sqrt(f(-2.0) * np.log(u1)).astype(f)
    ang32 = (f(6.283185307179586) * u2).astype(f)
    z32 = np.stack([(r32 * np.cos(ang32)).astype(f), (r32 * np.sin(ang32)).astype(f)], axis=-1).reshape(N, 4 * G)
    return z64[:, :A], z32[:, :A], {"words": words, "u": u, "z64": z64, "z32": z32}


def gauss_logp(act, mean, log_std):
    """log N(act; mean, exp(log_std)) summed over the last axis, float64."""
    act, mean, log_std = (np.asarray(x, dtype=np.float64) for x in (act, mean, log_std))
    z = (act - mean) * np.exp(-log_std)
    return (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)


# ---------------------------------------------------------------------------------------------------------- VecNormalize
def vecnorm_init_state(N, O):
    """SB3's initial state: mean 0, var 1, count 1e-4 (obs and returns), returns 0, episode_starts 1."""
    return {"obs_mean": np.zeros(O), "obs_var": np.ones(O), "obs_count": 1e-4, "ret_mean": 0.0, "ret_var": 1.0, "ret_count": 1e-4,
            "returns": np.zeros(N), "starts": np.ones(N, dtype=np.float32)}


def _fsum_moments(col):
    """(mean, biased variance, mean |x|) of a list of floats by exact summation."""
    n = len(col)
    mean = math.fsum(col) / n
    return mean, math.fsum([(x - mean) * (x - mean) for x in col]) / n, math.fsum([abs(x) for x in col]) / n


def _batch_moments(x, extra_in=None, sums_form=False, parts=1):
    """Batch mean / variance of the columns of x [N, C] (float64 holding the kernel's inputs) with the bound of the kernel's
    order.  Roundings (fp64), k_vecnorm_moments per 128-row block and column: a half column is at most 64 rows in 4 accumulators
    (8 adds each in the unrolled body, at most 3 in the tail), the accumulator tree (2), the pair shuffle (1), the division (1):
    15 for the block mean; the deviations add one subtraction and one square: 16 for the block M2.
    k_vecnorm_merge: n_b * mean_b (1), nb adds, / N (1)                      -> mean depth 17 + nb
                     dm (1), n_b dm dm (2), + M2_b (1), nb adds, / N (1)       -> variance depth 21 + nb on top of the block's 16
    and the block means' own error e_b enters M2 through 2 n_b |mean_b - mean| e_b (the cross term of the shifted sum of squares).
    sums_form (k_vecnorm_batch + a host add over `parts` + k_vecnorm_merge_batch): s1 = sum n_b mean_b, s2 = sum M2_b + n_b mean_b^2,
    var = s2 / n - mean^2, which loses depth * u64 * (mean^2 + var): block M2 16, n_b m m (2), + (1), nb + parts adds, / n (1),
    the cross term 2 n_b |mean_b| e_b <= 30 u64 sum x^2, mean^2 (1 + twice the mean's depth), the subtraction (1).
    extra_in [N, C]: bound on an error of the inputs themselves (the returns column, which the kernel updates in fp64 first).
    Returns mean, var, e_mean, e_var (arrays of C)."""
    N, C = x.shape
    nb = (N + VN_ROWS - 1) // VN_ROWS
    mean, var, e_mean, e_var = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C)
    for c in range(C):
        col = x[:, c].tolist()
        m, v, mabs = _fsum_moments(col)
        d_mean = (15 + 1 + nb + parts + 1) if sums_form else (17 + nb)
        em = d_mean * U64 * mabs
        if sums_form:
            depth = (16 + 2 + 1 + nb + parts + 1) + 30 + (1 + 2 * d_mean) + 1
            ev = depth * U64 * (m * m + v)
        else:
            cross = 0.0
            for b in range(nb):
                blk = col[b * VN_ROWS:(b + 1) * VN_ROWS]
                mb, _, mb_abs = _fsum_moments(blk)
                cross += 2.0 * len(blk) * abs(mb - m) * (15 * U64 * mb_abs + em)
            ev = (16 + 21 + nb) * U64 * v + cross / N
        if extra_in is not None:
            ein = extra_in[:, c].tolist()
            em += math.fsum(ein) / N
            ev += 2.0 * math.fsum([abs(xi - m) * e for xi, e in zip(col, ein)]) / N
        mean[c], var[c], e_mean[c], e_var[c] = m, v, em, ev
    return mean, var, e_mean, e_var


def chan_merge(mean, var, count, bmean, bvar, n, e_bmean=0.0, e_bvar=0.0):
    """RunningMeanStd.update_from_moments in mpmath (50 digits), with the bound of the fp64 statement
        delta = bmean - mean; tot = count + n; new_mean = mean + delta * n / tot
        M2 = var * count + bvar * n + delta * delta * count * n / tot; new_var = M2 / tot
    Roundings: new_mean: the final add (|new_mean|) and delta, tot, the product, the quotient (4 |delta n / tot|).
    M2: T1 = var count (1 + 2 adds after it), T2 = bvar n (1 + 2), T3 = delta^2 count n / tot (delta twice: 2, three products and
    a quotient: 4, tot: 1, 2 adds: 9); new_var: the division and tot (2).  The batch moments' own errors pass through linearly."""
    mp = mpmath.mpf
    mean_, var_, cnt, bm, bv, n_ = mp(float(mean)), mp(float(var)), mp(float(count)), mp(float(bmean)), mp(float(bvar)), mp(float(n))
    delta, tot = bm - mean_, cnt + n_
    new_mean = mean_ + delta * n_ / tot
    T1, T2, T3 = var_ * cnt, bv * n_, delta * delta * cnt * n_ / tot
    new_var = (T1 + T2 + T3) / tot
    d, t = abs(float(delta)), float(tot)
    e_mean = e_bmean + U64 * (abs(float(new_mean)) + 4.0 * d * float(n) / t)
    e_delta = e_bmean + U64 * d
    e_m2 = U64 * (3.0 * float(T1) + 3.0 * float(T2) + 9.0 * float(T3)) + float(n) * e_bvar + 2.0 * d * e_delta * float(count) * float(n) / t
    e_var = e_m2 / t + 2.0 * U64 * float(new_var)
    return float(new_mean), float(new_var), float(tot), e_mean, e_var


def vecnorm_step_ref(state, obs, rew, done, term_obs=None, gamma=0.99, eps=1e-8, clip_obs=10.0, clip_reward=10.0,
                     training=True, norm_obs=True, norm_reward=True, sums_form=False, parts=1, rows=None):
    """One VecNormalize.step_wait (SB3 1.6.2) from `state` (vecnorm_init_state's keys; float64 statistics as the kernel holds
    them): returns = returns * gamma + rew; Chan's merge of the batch moments of obs and of the returns (training; obs only with
    norm_obs); normalisation with the UPDATED statistics and clipping; returns of finished envs zeroed; episode_starts <- done.
    Batch moments by math.fsum, the merge in mpmath.  sums_form / parts: the bound of the multi-rank form (see _batch_moments).
    rows: slice of the envs whose outputs are wanted (a rank's shard in the multi-rank form; statistics are over all rows).
    Returns (new_state, out): out has nobs, nterm, nrew (float64, before the kernel's fp32 store), start_row (= the old
    episode_starts) and the bounds e_obs_mean, e_obs_var, e_ret_mean, e_ret_var, e_returns, e_nobs, e_nterm, e_nrew, in which one
    fp32 rounding of the output is included."""
    obs64, rew64 = np.asarray(obs, dtype=np.float64), np.asarray(rew, dtype=np.float64)
    N, O = obs64.shape
    new = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    out = {"e_obs_mean": np.zeros(O), "e_obs_var": np.zeros(O), "e_ret_mean": 0.0, "e_ret_var": 0.0, "e_returns": np.zeros(N)}
    if training:
        old = state["returns"]
        new["returns"] = old * gamma + rew64
        out["e_returns"] = 2.0 * U64 * (np.abs(old * gamma) + np.abs(rew64))          # product and sum (one rounding if fused)
        if norm_obs:
            bm, bv, ebm, ebv = _batch_moments(obs64, sums_form=sums_form, parts=parts)
            out["batch_obs_var"], out["e_batch_obs_var"] = bv, ebv
            for c in range(O):
                m, v, _, em, ev = chan_merge(state["obs_mean"][c], state["obs_var"][c], state["obs_count"], bm[c], bv[c], N, ebm[c], ebv[c])
                new["obs_mean"][c], new["obs_var"][c], out["e_obs_mean"][c], out["e_obs_var"][c] = m, v, em, ev
            new["obs_count"] = float(mpmath.mpf(float(state["obs_count"])) + N)
        bm, bv, ebm, ebv = _batch_moments(new["returns"][:, None], extra_in=out["e_returns"][:, None], sums_form=sums_form, parts=parts)
        new["ret_mean"], new["ret_var"], new["ret_count"], out["e_ret_mean"], out["e_ret_var"] = chan_merge(
            state["ret_mean"], state["ret_var"], state["ret_count"], bm[0], bv[0], N, ebm[0], ebv[0])
    sl = slice(None) if rows is None else rows

    def normalise(x):
        x = np.asarray(x, dtype=np.float64)[sl]
        if not norm_obs:
            return x, np.zeros_like(x)
        sd = np.sqrt(new["obs_var"] + eps)
        raw = (x - new["obs_mean"]) / sd
        val = np.clip(raw, -clip_obs, clip_obs)
        # the statistics' error through (x - mean) / sqrt(var + eps), four fp64 roundings of the expression, the fp32 store
        # (a value beyond the clip by more than its error is the clip value exactly)
        e = (out["e_obs_mean"] + np.abs(x - new["obs_mean"]) * out["e_obs_var"] / (2.0 * (new["obs_var"] + eps))) / sd + 4.0 * U64 * np.abs(raw)
        return val, np.where(np.abs(raw) - e > clip_obs, 0.0, np.minimum(e, 2.0 * clip_obs) + U32 * np.abs(val))
    out["nobs"], out["e_nobs"] = normalise(obs64)
    if term_obs is not None:
        out["nterm"], out["e_nterm"] = normalise(term_obs)
    r = rew64[sl]
    if norm_reward:
        sd = math.sqrt(new["ret_var"] + eps)
        raw = r / sd
        out["nrew"] = np.clip(raw, -clip_reward, clip_reward)
        e = np.abs(raw) * (out["e_ret_var"] / (2.0 * (new["ret_var"] + eps)) + 3.0 * U64)
        out["e_nrew"] = np.where(np.abs(raw) - e > clip_reward, 0.0, np.minimum(e, 2.0 * clip_reward) + U32 * np.abs(out["nrew"]))
    else:
        out["nrew"], out["e_nrew"] = r, np.zeros_like(r)
    out["start_row"] = state["starts"].copy()
    dn = np.asarray(done) != 0
    new["returns"] = np.where(dn, 0.0, new["returns"])
    new["starts"] = dn.astype(np.float32)
    return new, out


# ------------------------------------------------------------------------------------------------------------------- GAE
GAE_ROUNDINGS = 6


def gae_ref(rew, val, starts, last_val, last_done, gamma, lam):
    """SB3's compute_returns_and_advantage, backward scan in float64 over [T, N] arrays; gamma and lambda first rounded to fp32
    (the ABI passes floats).  One trip of k_gae rounds k = 6 times on the way to the advantage:
        delta = rew + gamma * nextv * nonterm - v        gamma * nextv (1), + rew (1), - v (1); nonterm is 0 or 1: exact
        last  = delta + gamma * lam * nonterm * last     gamma * lam (1), * last (1), + delta (1)
    (fewer where the compiler fuses a product into the add).  Each rounds a value no larger than the sum of the absolute terms,
    so E_t = k 2^-24 (|r| + g |v'| + |v| + g l |last|) + g l E_(t+1), with |last| the reference's plus E_(t+1), masked by
    nonterm.  ret = last + v rounds once more.  Returns adv, ret, e_adv, e_ret."""
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    rew, val, starts = (np.asarray(x, dtype=np.float64) for x in (rew, val, starts))
    T, N = rew.shape
    adv, e_adv = np.zeros((T, N)), np.zeros((T, N))
    last, E = np.zeros(N), np.zeros(N)
    nextv, nonterm = np.asarray(last_val, dtype=np.float64), 1.0 - np.asarray(last_done, dtype=np.float64)
    for t in range(T - 1, -1, -1):
        v = val[t]
        terms = np.abs(rew[t]) + g * np.abs(nextv) * nonterm + np.abs(v) + g * l * nonterm * (np.abs(last) + E)
        E = GAE_ROUNDINGS * U32 * terms + g * l * nonterm * E
        last = (rew[t] + g * nextv * nonterm - v) + g * l * nonterm * last
        adv[t], e_adv[t] = last, E
        nextv, nonterm = v, 1.0 - starts[t]
    ret = adv + val
    return adv, ret, e_adv, e_adv + U32 * (np.abs(adv) + e_adv + np.abs(val))


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam_ref(p, m, v, g, t, lr, b1, b2, eps, max_norm, grad_scale):
    """clip_grad_norm_(max_norm) + one torch.optim.Adam step (no weight decay, no amsgrad) at step ordinal t over flat fp32
    vectors, in float64; the hyper-parameters are rounded to fp32 first (the ABI passes floats).  Returns a dict with p, m, v
    (float64), their per-element bounds e_p, e_m, e_v, and norm, clip.  fp32 roundings, in units of u = 2^-24:
      |g|^2   x = g gs (1), x x (1), per-thread strided adds ceil(n / 16384), 6 wave shuffles, 2 LDS adds (k_grad_sqnorm), then
              the 64 block partials through k_adam's 256-lane tree (one partial per lane: 6 levels add non-zeros).  All terms are
              positive: relative error D u.
      clip    sqrtf (D / 2 + 4), + 1e-6f (1), max_norm / . (5); exact 1 when the norm is below max_norm
      gi      g gs (1), . clip (1)
      m       b1 m (1), (1 - b1) gi (1; 1 - b is exact for b in [0.5, 1]), the add (1)
      v       b2 v (1), (1 - b2) gi (1), . gi (1), the add (1)
      bc      1 - powf(b, t): 4 b^t / (1 - b^t) from powf, the subtraction (1)
      p       lr / bc1 (5), rsqrtf(bc2) (4), sqrtf(v) (4), their product (1), + eps (1), step m (1), / (5), p - . (1)"""
    f32 = lambda x: float(np.float32(x))
    lr, b1, b2, eps, max_norm, gs = (f32(x) for x in (lr, b1, b2, eps, max_norm, grad_scale))
    p, m, v, g = (np.asarray(x, dtype=np.float64) for x in (p, m, v, g))
    n, u = p.size, U32
    x = g * gs
    sq = math.fsum((x * x).tolist())
    norm = math.sqrt(sq)
    D = 2 + (n + SQN_BLOCKS * 256 - 1) // (SQN_BLOCKS * 256) + 6 + 2 + 6
    clip, e_clip = 1.0, 0.0
    if max_norm > 0.0:
        ratio = max_norm / (norm + f32(1e-6))
        if ratio < 1.0:
            clip, e_clip = ratio, (D / 2.0 + SQRT32 + 1.0 + DIV32) * u
    gi = x * clip
    e_g = 2.0 * u + e_clip                                                     # relative
    t1, t2 = b1 * m, (1.0 - b1) * gi
    mi = t1 + t2
    e_m = u * np.abs(t1) + (u + e_g) * np.abs(t2) + u * np.abs(mi)
    s1, s2 = b2 * v, (1.0 - b2) * gi * gi
    vi = s1 + s2
    e_v = u * s1 + (2.0 * u + 2.0 * e_g) * s2 + u * vi
    pw1, pw2 = b1 ** t, b2 ** t
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    e_bc1, e_bc2 = POW32 * u * pw1 / bc1 + u, POW32 * u * pw2 / bc2 + u        # relative
    step, e_step = lr / bc1, e_bc1 + DIV32 * u
    inv, e_inv = 1.0 / math.sqrt(bc2), e_bc2 / 2.0 + RSQRT32 * u
    rel_v = np.divide(e_v, vi, out=np.zeros_like(vi), where=vi > 0)
    root = np.sqrt(vi) * inv
    den = root + eps
    e_den = root * (rel_v / 2.0 + SQRT32 * u + e_inv + u) + u * den
    upd = step * mi / den
    e_upd = (step / den) * e_m + np.abs(upd) * (e_step + e_den / den + u + DIV32 * u)
    pn = p - upd
    e_p = e_upd + u * (np.abs(pn) + e_upd)
    return {"p": pn, "m": mi, "v": vi, "e_p": e_p, "e_m": e_m, "e_v": e_v, "norm": norm, "clip": clip, "ratio": (max_norm / (norm + f32(1e-6))) if max_norm > 0 else math.inf}


# ------------------------------------------------------------------------------------------------------------------ gSDE
def sde_sample_ref(mean, latent, W, log_std, stored_action):
    """SB3's StateDependentNoiseDistribution sample in float64: noise[n, j] = sum_l latent[n, l] W[n, l, j],
    sigma[n, j] = sqrt(sum_l latent^2 exp(log_std[l, j])^2 + 1e-6f), action = mean + noise, and the log-prob OF THE ACTION THE
    KERNEL STORED (stored_action) under the float64 mean and sigma.  Bounds of k_sample_sde (u = 2^-24):
      noise    L fused multiply-adds: L u sum_l |latent W|; action = fl(mean + noise): one more rounding, u |action|
      sigma    per term: latent^2 (1), __expf (<= 3 ulp = 6 for |log_std| <= 3) twice through sd sd (12 + 1), L fused adds: relative
               (14 + L) u on the variance (positive terms), + 1e-6f (1), sqrtf (4): e_s = ((15 + L) / 2 + 4) u relative
      z        a - mu (1), / sigma (5), e_s: e_z = 6 u + e_s;  z^2 / 2: (2 e_z + u);  logf(sigma): 3 ulp = 6 u |log sigma| + e_s
      sum      three adds of the expression, ceil(A / 64) adds in the lane, 6 shuffles: (9 + ceil(A / 64)) u sum_j |terms|
    Returns action, sigma, logp, e_noise (bound on action - mean, without the last rounding), e_logp."""
    mean, latent, W, log_std, a = (np.asarray(x, dtype=np.float64) for x in (mean, latent, W, log_std, stored_action))
    N, L = latent.shape
    A = mean.shape[1]
    prod = latent[:, :, None] * W
    noise = prod.sum(1)
    e_noise = L * U32 * np.abs(prod).sum(1)
    var = (latent ** 2) @ (np.exp(log_std) ** 2)
    sigma = np.sqrt(var + float(np.float32(1e-6)))
    z = (a - mean) / sigma
    quad, lg = 0.5 * z * z, np.log(sigma)
    logp = (-quad - lg - HALF_LOG_2PI).sum(-1)
    e_s = ((15 + L) / 2.0 + SQRT32) * U32
    e_z = (1 + DIV32) * U32 + e_s
    per = (2.0 * e_z + U32) * quad + LOG32 * U32 * np.abs(lg) + e_s
    e_logp = per.sum(-1) + (9 + (A + 63) // 64) * U32 * (quad + np.abs(lg) + HALF_LOG_2PI).sum(-1)
    return mean + noise, sigma, logp, e_noise, e_logp


# ---------------------------------------------------------------------------------------------------------------- gather
def gather_ref(adv, idx):
    """Mean and unbiased std of adv[idx] by exact summation, with the fp32 bound of k_ppo_gather + k_moments_finish (u = 2^-24).
    Block of 16 rows: the 16-lane part of the shuffle sum (4 levels add non-zeros), / rows (5): e_b = 9 u mean|a_b|; deviations
    (1), squares (1), 4 shuffle levels.  Finish: n_b mean_b (1), ceil(nb / 64) strided adds, 6 shuffles, / bs (5) on top of the
    block's 9; M2: dm (1), n_b dm dm (2), + M2_b (1), the strided adds and 6 shuffles, / (bs - 1) (5, halved by the root),
    sqrtf (4), and the block means' errors through 2 n_b |dm_b| (e_b + e_mean) + n_b e_b^2.
    Returns mean, std, e_mean, e_std."""
    a = np.asarray(adv, dtype=np.float64)[np.asarray(idx)]
    B, u = a.size, U32
    nb = (B + GATHER_ROWS - 1) // GATHER_ROWS
    trips = (nb + 63) // 64
    col = a.tolist()
    mean = math.fsum(col) / B
    m2 = math.fsum([(x - mean) ** 2 for x in col])
    mabs = math.fsum([abs(x) for x in col]) / B
    e_mean = (9 + 1 + trips + 6 + DIV32) * u * mabs
    e_m2 = 0.0
    for b in range(nb):
        blk = col[b * GATHER_ROWS:(b + 1) * GATHER_ROWS]
        nbk = len(blk)
        mb = math.fsum(blk) / nbk
        m2b = math.fsum([(x - mb) ** 2 for x in blk])
        e_b = 9 * u * math.fsum([abs(x) for x in blk]) / nbk
        dm = abs(mb - mean)
        e_dm = e_b + e_mean + u * dm
        e_m2 += (2 + 4) * u * m2b + nbk * e_b * e_b + 2 * nbk * dm * e_dm + nbk * e_dm * e_dm + 3 * u * nbk * dm * dm
    e_m2 += (1 + trips + 6) * u * m2
    std = math.sqrt(m2 / (B - 1)) if B > 1 else 0.0
    e_std = 0.0
    if m2 > 0:
        e_std = std * (e_m2 / (2 * m2) + (DIV32 / 2 + SQRT32) * u)
    return mean, std, e_mean, e_std
