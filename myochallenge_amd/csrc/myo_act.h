// myo_act.h — the hidden activations of the MLP actor-critic paths (MYO_ACT_* of include/myobatch.h): what k_mlp_fwdbwd, k_mlp_policy
// (myo_ppo_mlp.h) and the pointwise kernels k_bias_act / k_act_bwd_colsum (myobatch.hip) share.
#pragma once
#ifndef MYO_EMU

// tanh of the hidden layers (MYO_ACT_TANH), the ONE statement every kernel of the MLP paths uses (k_mlp_fwdbwd, k_mlp_policy, k_bias_act):
// 1 - 2 / (e^2x + 1), branch-free, evaluated in DOUBLE from the fp32 pre-activation and handed back as the nearest float.  The
// result is rounded to bf16 next, and a hidden unit's rounding flips wherever the evaluated value lands on the other side of a bf16
// boundary than the exact one.  Any fp32 evaluation of this formula is good to an ulp of 1.0 (the subtraction), not of the result:
// it flipped 30 - 80 of a net's 262,144 first-layer activations, each flip then moves its whole row of the second layer, and the
// fused step's policy loss (a mean of cancelling terms) sat at 4.5 - 5.5 times its float32 reference twin's distance from the
// float64 statement in one test case.  In double the evaluation adds no flips of its own (3 - 28 remain, from the fp32 sums).
// x is clamped to +-10 first (tanh(10) is 1 - 4e-9: 1.0f; the clamp would turn a NaN into a number, so a NaN input is handed
// back as it came, by a select); e^2x = 2^n 2^f with n = rint(2 x log2 e), 2^f = exp(f ln 2) by its
// Taylor series to degree 9 (|f ln 2| <= 0.347: 7e-12), the reciprocal by v_rcp_f64 and two Newton steps.  About 25 fp64
// operations, which the matrix-core kernels' epilogues absorb beside their MFMA phases (DESIGN.md section 9 has the times).
__device__ __forceinline__ float myo_act_tanh(float x) {
  const double xc = (double)__builtin_amdgcn_fmed3f(x, -10.f, 10.f);
  const double y = xc * 2.8853900817779268;                 // 2 x log2(e)
  const double n = __builtin_rint(y);
  const double g = (y - n) * 0.6931471805599453;            // e^2x = 2^n e^g
  double p = 1.0 / 362880.0;
  p = __builtin_fma(p, g, 1.0 / 40320.0);
  p = __builtin_fma(p, g, 1.0 / 5040.0);
  p = __builtin_fma(p, g, 1.0 / 720.0);
  p = __builtin_fma(p, g, 1.0 / 120.0);
  p = __builtin_fma(p, g, 1.0 / 24.0);
  p = __builtin_fma(p, g, 1.0 / 6.0);
  p = __builtin_fma(p, g, 0.5);
  p = __builtin_fma(p, g, 1.0);
  p = __builtin_fma(p, g, 1.0);
  const double d = __builtin_ldexp(p, (int)n) + 1.0;
  double r = __builtin_amdgcn_rcp(d);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  const float t = (float)__builtin_fma(-2.0, r, 1.0);
  return x != x ? x : t;
}
#endif
