// myo_ensemble.h — one deterministic acting step of an ENSEMBLE of actor-only LSTM policies in ONE launch: what
// SuperModel.predict (eval_mixture_of_ensembles.py) does member by member in eager torch — per member a float64 normalize_obs, the
// input projection, the recurrent product, the cell, the action head, and the critic half for nothing; then stack + mean per
// group and a `where` — for M = M0 (group 0, "base") + M1 (group 1, "hold") members on one observation batch.
//
// Work split: a workgroup of four waves owns a 32-row tile (two MFMA row tiles) and walks the members serially.  Per member
//   1. all 256 threads write the operand rows [x | keep h] of the tile into LDS as bf16: x = clamp((obs - mean_m) / sqrt(var_m + eps),
//      +-clip) in float64 -> float32 -> bf16 (VecNormalize.normalize_obs, then the operand cast), h from the carried bf16 state;
//   2. (barrier) wave w computes the four gates of units [w H/4, (w+1) H/4) for the whole K = OP + H: ONE fp32 accumulation over
//      the concatenated reduction, weight fragments straight from L2 (the image [M, 4H, K] is K-contiguous: 16 bytes per lane and
//      fragment, the next k-step's fragments in flight while this one's MFMAs run), the operand rows from LDS.  The product is
//      transposed, D[unit][row], so a lane ends with four consecutive units of one row and all four gates of them: the cell
//      (the formulas of lstm_fwd_out) runs in registers, c (fp32) and h (bf16) are updated in place, h_new also goes to LDS;
//   3. (barrier) the head a_m = bf16(h_new) . W_a^T + b_a: six 16x16 tiles (3 action tiles x 2 row tiles) over the four waves,
//      again transposed.  The lane that owns (row, 4 actions) keeps the two groups' running sums in registers, in member order.
// After the last member the group means are taken (sum / M_g, correctly rounded) and use_group1[row] picks the output.  No atomics,
// a fixed summation order, two barriers per member.
//
// v_mfma_f32_16x16x32_bf16 fragment maps as in myo_lstm_step.h.
#pragma once
#ifndef MYO_EMU

#define ENS_ROWS 32          // rows of a workgroup's tile
#define ENS_APM 48           // padded action width (three MFMA tiles), as MLP_APM
#define ENS_OPMAX 128        // padded observation width, as MLP_OPMAX

struct EnsArgs {
  const float* obs;                  // [N, O]
  const double *mean, *var;          // [M, O]
  double eps, clip;
  const unsigned short* w_gates;     // bf16 [M, 4H, K], K = OP + H: rows of [W_ih | 0 | W_hh]
  const unsigned short* w_a;         // bf16 [M, ENS_APM, H]: rows of W_a, zero rows beyond A
  const float* b_gates;              // [M, 4H]: bf16(b_ih + b_hh) as float32
  const float* b_a;                  // [M, A]
  unsigned short* h;                 // bf16 [M, N, H]
  float* c;                          // [M, N, H]
  const float *start0, *start1;      // [N] each (start1 unused when M1 = 0)
  const unsigned char* use_group1;   // [N] (unused when M1 = 0)
  float* act;                        // [N, A]
  float* member_act;                 // [M, N, A] or NULL
  int N, O, OP, A, M0, M1;
};

template <int H>
__global__ void __launch_bounds__(256) k_ensemble_act(const EnsArgs a) {
  constexpr int UT = H / 64;                          // unit tiles of 16 per wave (a quarter of H)
  constexpr int HS = H + 8;                           // LDS row stride of h_new (bf16 elements; +8: rows 16 bytes apart in the banks)
  __shared__ __attribute__((aligned(16))) unsigned short xs[ENS_ROWS * (ENS_OPMAX + H + 8)];
  __shared__ __attribute__((aligned(16))) unsigned short hn[ENS_ROWS * HS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int N = a.N, O = a.O, OP = a.OP, A = a.A;
  const int K = OP + H, XS = K + 8, KS = K / 32;
  const int row0 = blockIdx.x * ENS_ROWS;
  const int M = a.M0 + a.M1;

  // head tiles of this wave: t = wave + 4 s < 6 -> (action tile t % 3, row tile t / 3); running group sums in registers
  myo_f32x4 gsum[2][2];
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int s = 0; s < 2; ++s) gsum[g][s] = myo_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int m = 0; m < M; ++m) {
    const int grp = m >= a.M0;
    const float* start = grp ? a.start1 : a.start0;
    // ---- 1. operand rows [x | keep h] -> LDS
    {
      const int c = tid & 127, rg = tid >> 7;         // column c, rows rg*16 .. rg*16 + 15
      if (c < OP) {
        double mu = 0.0, sd = 1.0;
        if (c < O) { mu = a.mean[(size_t)m * O + c]; sd = sqrt(a.var[(size_t)m * O + c] + a.eps); }
        for (int i = 0; i < 16; ++i) {
          const int rl = rg * 16 + i, r = row0 + rl;
          unsigned short v = 0;
          if (c < O && r < N) {
            double x = ((double)a.obs[(size_t)r * O + c] - mu) / sd;
            x = x < -a.clip ? -a.clip : (x > a.clip ? a.clip : x);        // (a NaN passes through, as torch.clamp)
            v = myo_f2bf((float)x);
          }
          xs[rl * XS + c] = v;
        }
      }
      for (int idx = tid; idx < ENS_ROWS * (H / 8); idx += 256) {
        const int rl = idx / (H / 8), cc = idx % (H / 8), r = row0 + rl;
        myo_u16x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (r < N) {
          const float keep = 1.f - start[r];
          const unsigned short* hp = a.h + ((size_t)m * N + r) * H + cc * 8;
          lo = lstm_ld4(hp); hi = lstm_ld4(hp + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { lo[j] = myo_f2bf(lstm_bf(lo[j]) * keep); hi[j] = myo_f2bf(lstm_bf(hi[j]) * keep); }
        }
        unsigned short* xp = xs + rl * XS + OP + cc * 8;
        *reinterpret_cast<myo_u16x4*>(xp) = lo;
        *reinterpret_cast<myo_u16x4*>(xp + 4) = hi;
      }
    }
    __syncthreads();
    // ---- 2. gates of units [wave H/4, (wave+1) H/4), all of K; cell in registers
    {
      const int ub = wave * (H / 4);
      const unsigned short* W = a.w_gates + ((size_t)m * 4 * H + ub + lr) * K + lk * 8;      // + (q H + ut 16) K + kk 32
      myo_f32x4 acc[UT][4][2];
#pragma unroll
      for (int ut = 0; ut < UT; ++ut)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[ut][q][0] = acc[ut][q][1] = myo_f32x4{0.f, 0.f, 0.f, 0.f};
      myo_bf16x8 wa[UT][4], wb[UT][4];
#pragma unroll
      for (int ut = 0; ut < UT; ++ut)
#pragma unroll
        for (int q = 0; q < 4; ++q) wa[ut][q] = lstm_ld8(W + (size_t)(q * H + ut * 16) * K);
      const unsigned short* xb = xs + lr * XS + lk * 8;
      for (int kk = 0; kk < KS; ++kk) {
        const int kn = kk + 1 < KS ? kk + 1 : kk;     // (the last step loads its own fragments again: no branch, no read out of bounds)
#pragma unroll
        for (int ut = 0; ut < UT; ++ut)
#pragma unroll
          for (int q = 0; q < 4; ++q) wb[ut][q] = lstm_ld8(W + (size_t)(q * H + ut * 16) * K + kn * 32);
        const myo_bf16x8 b0 = lstm_ld8(xb + kk * 32), b1 = lstm_ld8(xb + 16 * XS + kk * 32);
#pragma unroll
        for (int ut = 0; ut < UT; ++ut)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            acc[ut][q][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ut][q], b0, acc[ut][q][0], 0, 0, 0);
            acc[ut][q][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ut][q], b1, acc[ut][q][1], 0, 0, 0);
          }
#pragma unroll
        for (int ut = 0; ut < UT; ++ut)
#pragma unroll
          for (int q = 0; q < 4; ++q) wa[ut][q] = wb[ut][q];
      }
      const float* bg = a.b_gates + (size_t)m * 4 * H;
#pragma unroll
      for (int ut = 0; ut < UT; ++ut) {
        const int u0 = ub + ut * 16 + 4 * lk;
        myo_f32x4 bq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bq[q] = *reinterpret_cast<const myo_f32x4*>(bg + q * H + u0);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int rl = n * 16 + lr, r = row0 + rl;
          float hv[4] = {0.f, 0.f, 0.f, 0.f};
          if (r < N) {
            const float keep = 1.f - start[r];
            float* cp = a.c + ((size_t)m * N + r) * H + u0;
            const myo_f32x4 c0 = *reinterpret_cast<const myo_f32x4*>(cp);
            myo_f32x4 cv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float iv = myo_sigmoid(acc[ut][0][n][j] + bq[0][j]);
              const float fv = myo_sigmoid(acc[ut][1][n][j] + bq[1][j]);
              const float gv = tanhf(acc[ut][2][n][j] + bq[2][j]);
              const float ov = myo_sigmoid(acc[ut][3][n][j] + bq[3][j]);
              cv[j] = fv * (c0[j] * keep) + iv * gv;
              hv[j] = ov * tanhf(cv[j]);
            }
            *reinterpret_cast<myo_f32x4*>(cp) = cv;
            lstm_st4(a.h + ((size_t)m * N + r) * H + u0, hv[0], hv[1], hv[2], hv[3]);
          }
          lstm_st4(hn + rl * HS + u0, hv[0], hv[1], hv[2], hv[3]);
        }
      }
    }
    __syncthreads();
    // ---- 3. head tiles, member sums
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int t = wave + 4 * s;
      if (t < 6) {                                     // (uniform per wave)
        const int at = t % 3, n = t / 3;
        const unsigned short* Wa = a.w_a + ((size_t)m * ENS_APM + at * 16 + lr) * H + lk * 8;
        const unsigned short* hb = hn + (n * 16 + lr) * HS + lk * 8;
        myo_f32x4 o = myo_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < H / 32; ++kk) o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lstm_ld8(Wa + kk * 32), lstm_ld8(hb + kk * 32), o, 0, 0, 0);
        const int a0 = at * 16 + 4 * lk, r = row0 + n * 16 + lr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = o[j] + (a0 + j < A ? a.b_a[(size_t)m * A + a0 + j] : 0.f);
          if (grp) gsum[1][s][j] = (m == a.M0) ? v : gsum[1][s][j] + v;
          else gsum[0][s][j] = (m == 0) ? v : gsum[0][s][j] + v;
          if (a.member_act && r < N && a0 + j < A) a.member_act[((size_t)m * N + r) * A + a0 + j] = v;
        }
      }
    }
  }
  // ---- group means, selection
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int t = wave + 4 * s;
    if (t < 6) {
      const int at = t % 3, n = t / 3;
      const int a0 = at * 16 + 4 * lk, r = row0 + n * 16 + lr;
      if (r < N) {
        const bool g1 = a.M1 > 0 && a.use_group1[r] != 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (a0 + j < A)      // (the quotient of two floats through float64 rounds once: 53 >= 2 * 24 + 2 bits)
            a.act[(size_t)r * A + a0 + j] = g1 ? (float)((double)gsum[1][s][j] / (double)a.M1) : (float)((double)gsum[0][s][j] / (double)a.M0);
      }
    }
  }
}

template <int H>
static void ensemble_launch(const EnsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((k_ensemble_act<H>), dim3((a.N + ENS_ROWS - 1) / ENS_ROWS), dim3(256), 0, s, a);
}
#endif
