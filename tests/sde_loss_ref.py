"""The gSDE loss stage of the fused PPO steps (csrc/myo_sde_loss.h, FusedPPOStep._sde_loss) stated once for any float type.

* ``sde_loss(case, torch.float64)`` is THE REFERENCE: the loss stage on the bf16 inputs in float64, with dmean / dvalue rounded to
  bf16 (round-to-nearest-even, straight from float64: ``bf16_rne``) at the end, where the kernel rounds.
* ``sde_loss(case, torch.float32)`` is ITS TWIN: the same statements in float32, a transcription of ``_sde_loss`` (fp32 GEMMs, the
  batch sums as ones-row GEMMs, ``.to(bfloat16)`` at the end).  What the twin misses the reference by is the error any correct fp32
  implementation may have; the GPU tests scale their bounds from it (``twin_errors``).
* ``make_case(B, L, A, seed)`` is the seeded case generator; it refuses a case with a row whose float64 ratio lies within 1e-4 of
  1 +- clip (such a row may legitimately flip its whole gradient), so CASES lists seeds that have none.

No GPU and no native library is needed here.  The cases and their results are cached: compute once, share, leave unchanged.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

SDE_EPS = 1e-6
CLIP, ENT_COEF, VF_COEF = 0.2, 1e-3, 0.5
LOG_2PI = math.log(2.0 * math.pi)

# (B, L, A, seed): a partial last block, L not a multiple of 32, the hand's odd A = 39, both real latent sizes
CASES = [(64, 32, 3, 1), (37, 256, 5, 2), (200, 24, 39, 2), (1000, 128, 39, 2), (4096, 256, 39, 2)]
CASE_IDS = ["%dx%dx%d" % c[:3] for c in CASES]


def bf16_rne(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest bfloat16 value (ties to even), returned as float64.  Not through float32: that would round twice."""
    a = np.asarray(x.detach().cpu().numpy(), dtype=np.float64)
    mag = np.abs(a)
    u = mag.astype(np.float32).view(np.uint32)
    lo_u = u & np.uint32(0xFFFF0000)
    hi_u = lo_u + np.uint32(0x10000)
    lo, hi = lo_u.view(np.float32).astype(np.float64), hi_u.view(np.float32).astype(np.float64)
    d_lo, d_hi = np.abs(mag - lo), np.abs(hi - mag)
    even_lo = (lo_u >> np.uint32(16)) & np.uint32(1) == 0
    pick_lo = (d_lo < d_hi) | ((d_lo == d_hi) & even_lo)
    return torch.from_numpy(np.copysign(np.where(pick_lo, lo, hi), a))


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """Spacing of bfloat16 at |x| (float64; normal range)."""
    e = torch.floor(torch.log2(torch.clamp(x.abs().double(), min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def _logp64(mean, lat, log_std, actions):
    var = (lat.double() ** 2) @ torch.exp(2.0 * log_std.double()) + SDE_EPS
    diff = actions.double() - mean.double()
    return (-0.5 * diff * diff / var - 0.5 * torch.log(var)).sum(-1) - 0.5 * mean.shape[1] * LOG_2PI


@functools.lru_cache(maxsize=None)
def make_case(B: int, L: int, A: int, seed: int) -> dict:
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    lat = torch.relu(n(B, L)).to(torch.bfloat16)
    mean = (0.3 * n(B, A)).to(torch.bfloat16)
    log_std = -2.0 + 0.2 * n(L, A)
    std = torch.sqrt((lat.float() ** 2) @ torch.exp(2.0 * log_std) + SDE_EPS)
    actions = mean.float() + std * n(B, A)                       # drawn from the policy's own distribution
    old_logp = (_logp64(mean, lat, log_std, actions) + 0.15 * n(B).double()).float()
    adv, ret, value = n(B), n(B), n(B).to(torch.bfloat16)
    var_a, mu_a = torch.var_mean(adv)                            # unbiased, as PPO's minibatch normalisation
    case = dict(B=B, L=L, A=A, seed=seed, lat=lat, mean=mean, value=value, log_std=log_std, actions=actions, old_logp=old_logp, adv=adv,
                ret=ret, adv_stats=torch.stack([mu_a, var_a.sqrt()]), clip=CLIP, ent_coef=ENT_COEF, vf_coef=VF_COEF)
    ratio = torch.exp(_logp64(mean, lat, log_std, actions) - old_logp.double())
    edge = torch.minimum((ratio - (1 - CLIP)).abs(), (ratio - (1 + CLIP)).abs()).min().item()
    assert edge > 1e-4, f"case {(B, L, A, seed)}: a row's ratio lies {edge:.2e} from a clip boundary; choose another seed"
    clipped = ((ratio - 1).abs() > CLIP).double().mean().item()
    assert 0.10 <= clipped <= 0.20 or B < 100, f"case {(B, L, A, seed)}: {clipped:.3f} of the rows clipped"
    return case


def sde_loss(case: dict, dtype, clip=None) -> dict:
    """The loss stage in `dtype` (float64: the reference, float32: the twin), line by line as FusedPPOStep._sde_loss."""
    f = lambda t: t.to(dtype)
    B, A = case["B"], case["A"]
    clip = case["clip"] if clip is None else clip
    ent_coef, vf_coef = case["ent_coef"], case["vf_coef"]
    ones = torch.ones((1, B), dtype=dtype)
    colsum = lambda x: (ones @ x).squeeze(0)
    lat2 = f(case["lat"]) ** 2
    e2 = torch.exp(2.0 * f(case["log_std"]))
    var = lat2 @ e2 + SDE_EPS
    diff = f(case["actions"]) - f(case["mean"])
    z2 = diff * diff
    logp = (-0.5 * z2 / var - 0.5 * torch.log(var)).sum(-1) - 0.5 * A * LOG_2PI
    st = f(case["adv_stats"])
    advn = (f(case["adv"]) - st[0]) / (st[1] + 1e-8)
    lr = logp - f(case["old_logp"])
    ratio = torch.exp(lr)
    s1, s2 = advn * ratio, advn * torch.clamp(ratio, 1 - clip, 1 + clip)
    inside = (ratio > 1 - clip) & (ratio < 1 + clip)
    dlogp = -(advn * ratio) * torch.where(s1 <= s2, torch.ones_like(ratio), inside.to(dtype)) / B
    dmean = dlogp.unsqueeze(-1) * diff / var
    dvar = dlogp.unsqueeze(-1) * (0.5 * z2 / (var * var) - 0.5 / var) - (ent_coef / B) * 0.5 / var
    g_log_std = 2.0 * e2 * (lat2.t() @ dvar)
    err = f(case["value"]) - f(case["ret"])
    dvalue = (vf_coef * 2.0 / B) * err
    sums = colsum(torch.stack([torch.min(s1, s2), err * err], -1))
    ent = (0.5 * torch.log(var)).sum(-1) + 0.5 * A * (1.0 + LOG_2PI)
    d3 = colsum(torch.stack([(ratio - 1) - lr, ((ratio - 1).abs() > clip).to(dtype), -ent], -1)) / B
    out = dict(g_log_std=g_log_std, g_bias_pi=colsum(dmean), g_bias_vf=colsum(dvalue.unsqueeze(-1)), pl=-sums[0] / B, vl=sums[1] / B,
               kl=d3[0], cf=d3[1], el=d3[2], ratio=ratio, dmean_raw=dmean, dvalue_raw=dvalue)
    if dtype == torch.float64:
        out["dmean"], out["dvalue"] = bf16_rne(dmean), bf16_rne(dvalue)
    else:
        out["dmean"], out["dvalue"] = dmean.to(torch.bfloat16).double(), dvalue.to(torch.bfloat16).double()
    return out


@functools.lru_cache(maxsize=None)
def reference(B: int, L: int, A: int, seed: int) -> dict:
    return sde_loss(make_case(B, L, A, seed), torch.float64)


@functools.lru_cache(maxsize=None)
def twin(B: int, L: int, A: int, seed: int) -> dict:
    return sde_loss(make_case(B, L, A, seed), torch.float32)


FLOAT_KEYS = ("g_log_std", "g_bias_pi", "g_bias_vf", "pl", "vl", "kl", "cf", "el")


def rel_err(x, ref) -> float:
    """max |x - ref| / max |ref| (a scalar: |x - ref| / |ref|)."""
    x, ref = torch.as_tensor(x).double().cpu(), torch.as_tensor(ref).double().cpu()
    den = ref.abs().max().item()
    return (x - ref).abs().max().item() / (den if den > 0 else 1.0)


def bf16_mismatch(x, ref):
    """(fraction of elements where the bf16 arrays differ, the largest difference in ulps of the reference value)."""
    x, ref = torch.as_tensor(x).double().cpu(), torch.as_tensor(ref).double().cpu()
    d = (x - ref).abs()
    bad = d > 0
    if not bad.any():
        return 0.0, 0.0
    return bad.double().mean().item(), (d[bad] / bf16_ulp(ref[bad])).max().item()


BF16_FRACTION_CAP = 1.0 / 256       # the project's single-step cap (tests/test_lstm_kernels.py): at most 1 element in 256, by one ulp


def assert_bf16_cap(x, ref, what):
    frac, ulps = bf16_mismatch(x, ref)
    assert frac <= BF16_FRACTION_CAP and ulps <= 1.0 + 1e-9, f"{what}: {frac:.2e} of the elements differ, by up to {ulps:.2f} ulp"
    return frac, ulps


@functools.lru_cache(maxsize=None)
def twin_errors(B: int, L: int, A: int, seed: int) -> dict:
    """The twin's own error per float output on this case: the unit of the GPU test's bounds."""
    ref, tw = reference(B, L, A, seed), twin(B, L, A, seed)
    return {k: rel_err(tw[k], ref[k]) for k in FLOAT_KEYS}
