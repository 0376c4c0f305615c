"""Plain-torch CPU references of the PPO loss stage and the split-K reducers of csrc/myobatch.hip.

* ppo_loss_ref   myo_ppo_loss_grad (k_ppo_loss<false|true> + k_colmajor_finish): everything the call writes
* hp_block_ref   myo_hp_record: the hyper-parameter block over a sequence of minibatches
* splitk_ref     myo_splitk_reduce / myo_splitk_reduce2 (k_splitk_reduce<true|false>, k_colsum_finish, k_reduce_pair)

No GPU and no native library in here.  Inputs are the tensors the kernels get (fp32, or bf16 for `mean` / `values` with
in_bf16), widened exactly to the working dtype `dt`; the launch scalars are taken as the C floats the entry point receives.
float64 is the reference, float32 its twin: the same statement at the kernel's width, whose distance from the reference sizes
the tests' tolerance.  `mut` names one deliberate mistake of the twin (MUTATIONS): the CPU tests show that the tolerance
rejects each of them.
"""
import numpy as np
import torch

from mlp_ref import HALF_LOG_2PI, gaussian_logp, round_bf16

U32 = 2.0 ** -24                     # relative error of one fp32 rounding
BLOCK_ROWS = 64                      # rows per k_ppo_loss block
FINISH_LANES = 64                    # lanes of myo_col_sum: block b is read by lane b % 64
EPS_STD = float(np.float32(1e-8))    # the kernel's 1e-8f

HP_LR, HP_CLIP, HP_KL_LIMIT, HP_STOP, HP_APPLIED, HP_COUNT, HP_SUM_KL, HP_SUM_CLIPFRAC, HP_SUM_ENTLOSS, HP_LAST_KL, HP_LAST_PL, HP_LAST_VL = range(12)
HP_WORDS = 16

MUTATIONS = {
    "a": "`inside` taken with <= instead of <",
    "b": "clip taken from the launch scalar while a block is given",
    "c": "one /B missing in dvalue",
    "d": "the entropy constant 1.4189385 replaced by 0.9189385",
    "e": "the last row of a ragged block dropped from the column sums",
    "f": "the block partials summed only over the first 64 blocks",
    "g": "the bf16 copies truncated instead of rounded to nearest even",
    "h": "approx_kl computed as lr^2 / 2",
}


def f32(x) -> float:
    """The value a C float argument holds."""
    return float(np.float32(x))


def trunc_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> the bf16 value below it in magnitude (mutation g)."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def work_floats(B, A, with_hp):
    """Size of `work` as include/myobatch.h documents it."""
    return ((B + BLOCK_ROWS - 1) // BLOCK_ROWS) * (2 * A + (6 if with_hp else 3))


def ppo_loss_ref(mean, values, actions, old_logp, adv, returns, log_std, adv_stats, clip, vf_coef, ent_coef, in_bf16=False,
                 dt=torch.float64, mut=None, clip_launch=None):
    """One myo_ppo_loss_grad call.  mean [B,A], values [B] (bf16 tensors with in_bf16: the values are widened exactly), actions
    [B,A], old_logp / adv / returns [B], log_std [A], adv_stats {mean, std}; `clip` is the clip range in force (the block's when a
    block is given, else the launch scalar).  Returns a dict:
      dmean [B,A], dvalue [B], acc [2A+3] = {sum_i dlogp_i (z^2 - 1) [A], policy loss, value loss, sum_i dmean[i,:] [A],
      sum_i dvalue[i]}, g_log_std = acc[:A] - ent_coef, g_bias_pi = acc[A+2:2A+2], g_bias_vf = acc[2A+2:],
      approx_kl = sum((ratio - 1) - lr) / B, clip_frac = #(|ratio - 1| > clip) / B with its row count clipped_rows,
      ent_loss = -sum_a (log_std_a + 1/2 + 1/2 log 2 pi), dmean_bf16 / dvalue_bf16 = RNE of the fp32 outputs (as fp32 values),
      and per row ratio, adv_norm, log_ratio (what the tests' input conditions are stated on)."""
    if in_bf16:
        assert mean.dtype == torch.bfloat16 and values.dtype == torch.bfloat16
    mean, values, actions, old_logp, adv, returns, log_std = (t.detach().cpu().to(dt) for t in (mean, values, actions, old_logp, adv, returns, log_std))
    stats = torch.as_tensor(adv_stats).detach().cpu().to(dt)
    clip, vf_coef, ent_coef = f32(clip), f32(vf_coef), f32(ent_coef)
    if mut == "b" and clip_launch is not None:
        clip = f32(clip_launch)
    B, A = mean.shape
    inv = torch.exp(-log_std)
    z = (actions - mean) * inv
    logp = gaussian_logp(actions, mean, log_std)
    an = (adv - stats[0]) / (stats[1] + EPS_STD)
    lr = logp - old_logp
    ratio = torch.exp(lr)
    s1 = an * ratio
    s2 = an * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    pl = -torch.minimum(s1, s2).sum() / B
    if mut == "a":
        inside = (ratio >= 1.0 - clip) & (ratio <= 1.0 + clip)
    else:
        inside = (ratio > 1.0 - clip) & (ratio < 1.0 + clip)
    dlogp = -(an * ratio) * ((s1 <= s2) | inside).to(dt) / B
    dm = dlogp[:, None] * z * inv
    dls = dlogp[:, None] * (z * z - 1.0)
    dv = values - returns
    vl = (dv * dv).sum() / B
    dvi = (vf_coef * 2.0) * dv if mut == "c" else (vf_coef * 2.0 / B) * dv
    kl_rows = 0.5 * lr * lr if mut == "h" else (ratio - 1.0) - lr
    clipped = (ratio - 1.0).abs() > clip
    ent_const = HALF_LOG_2PI if mut == "d" else 0.5 + HALF_LOG_2PI
    keep_col = torch.ones(B, dtype=torch.bool)           # rows entering the column sums acc[:A], acc[A+2:2A+2]
    keep_all = torch.ones(B, dtype=torch.bool)           # rows entering every sum
    if mut == "e" and B % BLOCK_ROWS:
        keep_col[B - 1] = False
    if mut == "f":
        keep_all[FINISH_LANES * BLOCK_ROWS:] = False
        keep_col &= keep_all
        pl = -torch.minimum(s1, s2)[keep_all].sum() / B
        vl = (dv * dv)[keep_all].sum() / B
    acc = torch.cat([dls[keep_col].sum(0), pl[None], vl[None], dm[keep_col].sum(0), dvi[keep_all].sum()[None]])
    rnd = trunc_bf16 if mut == "g" else round_bf16
    return {
        "dmean": dm, "dvalue": dvi, "acc": acc, "pl": pl, "vl": vl,
        "g_log_std": acc[:A] - ent_coef, "g_bias_pi": acc[A + 2:2 * A + 2], "g_bias_vf": acc[2 * A + 2:],
        "approx_kl": kl_rows[keep_all].sum() / B, "clipped_rows": int(clipped[keep_all].sum()),
        "clip_frac": torch.as_tensor(int(clipped[keep_all].sum()), dtype=dt) / B, "ent_loss": -(log_std + ent_const).sum(),
        "dmean_bf16": rnd(dm.float()), "dvalue_bf16": rnd(dvi.float()),
        "ratio": ratio, "adv_norm": an, "log_ratio": lr,
    }


# --------------------------------------------------------------------------------------------------- hyper-parameter block
HP_NEVER_WRITTEN = (HP_LR, HP_APPLIED, 12, 13, 14, 15)      # by the loss stage (CLIP and KL_LIMIT are its inputs)


def hp_block_new(clip, kl_limit, sentinel=0.0):
    """A block at the start of an epoch as uint32[HP_WORDS] bit patterns: clip range and KL limit set, flag, count, sums and
    last values zero, and `sentinel` in the words the loss stage never writes."""
    b = np.zeros(HP_WORDS, dtype=np.float32)
    b[HP_CLIP], b[HP_KL_LIMIT] = clip, kl_limit
    b[list(HP_NEVER_WRITTEN)] = sentinel
    return b.view(np.uint32).copy()


def hp_block_ref(block, pl, vl, kl, cf, el):
    """myo_hp_record over a sequence of minibatches.  block: uint32[HP_WORDS] bit patterns (not modified); pl, vl, kl, cf, el:
    one fp32 value each or equally long sequences, in minibatch order.  Returns the block after the last minibatch.
      STOP up: nothing is written (sticky);
      else COUNT += 1, SUM_KL / SUM_CLIPFRAC / SUM_ENTLOSS += kl / cf / el (one fp32 add each), LAST_KL / LAST_PL / LAST_VL = kl / pl /
      vl, and then, with KL_LIMIT > 0 and kl > KL_LIMIT, STOP = 1 — the minibatch that raises the flag is recorded;
      LR, CLIP, KL_LIMIT, APPLIED and words 12-15 are never written."""
    u = np.array(block, dtype=np.uint32, copy=True)
    assert u.shape == (HP_WORDS,)
    fl = u.view(np.float32)
    it = u.view(np.int32)
    seq = [np.atleast_1d(np.asarray(x, dtype=np.float32)) for x in (pl, vl, kl, cf, el)]
    assert len({len(s) for s in seq}) == 1
    for p, v, k, c, e in zip(*seq):
        if it[HP_STOP]:
            continue
        fl[HP_SUM_KL] = np.float32(fl[HP_SUM_KL] + k)
        fl[HP_SUM_CLIPFRAC] = np.float32(fl[HP_SUM_CLIPFRAC] + c)
        fl[HP_SUM_ENTLOSS] = np.float32(fl[HP_SUM_ENTLOSS] + e)
        it[HP_COUNT] += 1
        fl[HP_LAST_KL], fl[HP_LAST_PL], fl[HP_LAST_VL] = k, p, v
        if fl[HP_KL_LIMIT] > 0 and k > fl[HP_KL_LIMIT]:
            it[HP_STOP] = 1
    return u


# ------------------------------------------------------------------------------------------------------------ split-K
def splitk_ref(part, groups, splits, n):
    """out[g, j] = sum_k part[g, k, j] in float64 of the values given (bf16 or fp32, widened exactly), and the bound on
    |kernel - out|.  Every kernel path adds the `splits` fp32 terms of one output element one after the other in SOME order,
    starting from 0 (the first add is exact): splits - 1 roundings, each at most 2^-24 of a partial sum that is itself at most
    sum_k |part_k| (first order), so in any order
        |err| <= (splits - 1) * 2^-24 * sum_k |part_k|
    — derived, not measured; times 2 for the second-order terms.  Returns (out [groups, n], bound [groups, n]) as float64."""
    p = part.detach().cpu().to(torch.float64).reshape(groups, splits, n)
    return p.sum(1), 2.0 * (splits - 1) * U32 * p.abs().sum(1)


def reduce_mode(is_bf16, splits, n):
    """The code path of one reduction job: 0 bf16 partials, 1 tall fp32 through LDS, 2 plain fp32 (make_reduce_job)."""
    if is_bf16:
        return 0
    return 1 if ((n // 2) % 32 == 0 and splits >= 64) else 2


def reduce_blocks(is_bf16, groups, splits, n):
    total2 = groups * (n // 2)
    return total2 // 32 if reduce_mode(is_bf16, splits, n) == 1 else (total2 + 255) // 256
