// The PPO loss stage for generalised state-dependent exploration (gSDE), as two launches: the arithmetic of FusedPPOStep._sde_loss
// (rl/fused_mlp.py), statement by statement, in fp32 on the bf16 trunk outputs.  Included by myobatch.hip after the Gaussian loss
// stage, whose helpers it uses (myo_f2bf, myo_col_sum, myo_hp_record).
//
//   var[i,a]  = sum_l lat[i,l]^2 exp(2 log_std[l,a]) + eps               (latent detached: log_std sees the loss through var only)
//   logp[i]   = sum_a (-0.5 diff^2 / var - 0.5 log var) - 0.5 A log 2pi,   diff = action - mean
//   dmean     = dlogp diff / var,   dvar = dlogp (0.5 diff^2 / var^2 - 0.5 / var) - (ent_coef / B) 0.5 / var
//   g_log_std = 2 exp(2 log_std) o (lat^2^T dvar)
//
// k_sde_loss: 256 threads own SDE_TILE-row tiles of a contiguous row range.  exp(2 log_std) [L, A] and the tile's latent (bf16, squared
// on use: the square of a bf16 is exact in fp32) sit in LDS.  Thread (row, column group) accumulates var for its CPT columns over l with
// fp32 FMAs (VALU: every operand keeps its fp32 value), the four column groups of a row exchange their partial log-probabilities
// through LDS and add them in a fixed order, each writes its dmean (bf16, the stage's one rounding of an output) and leaves dvar in
// LDS; then thread l accumulates row l of lat^2^T dvar in registers ACROSS the block's tiles, so that a block leaves one [L, A] partial
// however many rows it owns: sde_blocks() caps the grid at SDE_MAXBLK, 5 MB of partials at B = 65536, L = 256, A = 39.
// k_sde_finish: adds the partials block by block in a fixed order (deterministic, no float atomics; a kernel boundary instead of an
// in-kernel release fence, as k_colmajor_finish), scales by 2 exp(2 log_std), writes the head-bias gradients and the two losses and
// enters the diagnostics into the hyper-parameter block.
//
// Rounding points: expf / logf / fp32 division (the build's 2.5-ulp division) where _sde_loss has torch.exp / torch.log / a division;
// sums over l, over the rows of a tile and over blocks are sequential fp32.
#pragma once

#define SDE_TILE 64
#define SDE_MAXBLK 128
#define SDE_LMAX 256
#define SDE_AMAX 64

static inline int sde_tiles_per_block(int B) {
  const int tiles = (B + SDE_TILE - 1) / SDE_TILE;
  return (tiles + SDE_MAXBLK - 1) / SDE_MAXBLK;
}
static inline int sde_blocks(int B) {
  const int tiles = (B + SDE_TILE - 1) / SDE_TILE, tpb = sde_tiles_per_block(B);
  return (tiles + tpb - 1) / tpb;
}
// columns of the per-block scalar partials (column-major [SDE_COLS(A), blocks]): bias gradient of the action head [A], then
#define SDE_C_PL(A) (A)            /* sum of min(s1, s2) */
#define SDE_C_VL(A) ((A) + 1)      /* sum of squared value errors */
#define SDE_C_DV(A) ((A) + 2)      /* sum of dvalue: bias gradient of the value head */
#define SDE_C_KL(A) ((A) + 3)      /* sums of (ratio - 1) - log ratio, of [|ratio - 1| > clip], of -entropy */
#define SDE_COLS(A) ((A) + 6)
// latent row stride in LDS (bf16 elements): even, and an odd number of 32-bit words, so that the rows of a wave fall into distinct banks
static inline int sde_lat_stride(int L) {
  int ls = (L + 1) & ~1;
  if (((ls >> 1) & 1) == 0) ls += 2;
  return ls;
}
static inline size_t sde_lds_bytes(int L, int AP) {
  const int Le = (L + 1) & ~1;
  return ((size_t)Le * AP + 2 * SDE_TILE * AP + 8 * SDE_TILE) * sizeof(float) + (size_t)SDE_TILE * sde_lat_stride(L) * sizeof(unsigned short);
}

struct SdeArgs {
  const unsigned short *mean, *value, *lat;
  const float *actions, *old_logp, *adv, *returns, *log_std, *adv_stats, *hp;
  unsigned short *dmean, *dvalue;
  float *gpart, *part;
  int B, L, A, LS, tpb;
  float clip, vf_coef, ent_coef, eps;
};

__device__ __forceinline__ float sde_bf(unsigned short u) { return __uint_as_float(((unsigned)u) << 16); }

template <int CPT>
__global__ void __launch_bounds__(256) k_sde_loss(const SdeArgs p) {
  constexpr int AP = 4 * CPT;
  extern __shared__ float sde_lds[];
  const int B = p.B, L = p.L, A = p.A, LS = p.LS, Le = (L + 1) & ~1;
  float* s_e2 = sde_lds;                              // [Le, AP]: exp(2 log_std), zero beyond A and in the pad row
  float* s_dvar = s_e2 + (size_t)Le * AP;             // [SDE_TILE, AP]
  float* s_dmean = s_dvar + SDE_TILE * AP;            // [SDE_TILE, AP]
  float* s_red = s_dmean + SDE_TILE * AP;             // [2, 4, SDE_TILE]: the column groups' partial sums of a row
  unsigned short* s_lat = reinterpret_cast<unsigned short*>(s_red + 8 * SDE_TILE);   // [SDE_TILE, LS] bf16
  const int t = threadIdx.x, r = t & 63, cg = t >> 6, a0 = cg * CPT;
  const float clip = p.hp ? p.hp[MYO_HP_CLIP] : p.clip;
  const float adv_mean = p.adv_stats[0], adv_den = p.adv_stats[1] + 1e-8f;
  for (int k = t; k < Le * AP; k += 256) {
    const int l = k / AP, a = k - l * AP;
    s_e2[k] = (l < L && a < A) ? expf(2.0f * p.log_std[(size_t)l * A + a]) : 0.f;
  }
  float g[AP];                                        // thread l: row l of lat^2^T dvar over all the block's rows
#pragma unroll
  for (int c = 0; c < AP; ++c) g[c] = 0.f;
  float bsum = 0.f;                                   // thread a < A: column a of dmean over all the block's rows
  float pl_s = 0.f, vl_s = 0.f, dv_s = 0.f, kl_s = 0.f, cf_s = 0.f, el_s = 0.f;    // column group 0: this row's share
  const int tile0 = blockIdx.x * p.tpb;
  for (int ti = 0; ti < p.tpb; ++ti) {
    const int r0 = (tile0 + ti) * SDE_TILE;
    if (r0 >= B) break;
    __syncthreads();                                  // (the previous tile's readers of s_lat / s_dvar / s_dmean, and s_e2's writers)
    for (int k = t; k < SDE_TILE * Le; k += 256) {
      const int rr = k / Le, l = k - rr * Le;
      s_lat[rr * LS + l] = (r0 + rr < B && l < L) ? p.lat[(size_t)(r0 + rr) * L + l] : (unsigned short)0;
    }
    const int row = r0 + r;
    const bool on = row < B;
    float diff[CPT], var[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int a = a0 + c;
      diff[c] = (on && a < A) ? p.actions[(size_t)row * A + a] - sde_bf(p.mean[(size_t)row * A + a]) : 0.f;
      var[c] = 0.f;
    }
    __syncthreads();
    {   // var over l: the row's latent pair by pair, exp(2 log_std) broadcast to the wave
      const unsigned* lat2w = reinterpret_cast<const unsigned*>(s_lat + r * LS);
      for (int lp = 0; lp < Le / 2; ++lp) {
        const unsigned w = lat2w[lp];
        const float x0 = __uint_as_float(w << 16), x1 = __uint_as_float(w & 0xffff0000u);
        const float q0 = x0 * x0, q1 = x1 * x1;
        const float4* e0 = reinterpret_cast<const float4*>(s_e2 + (size_t)(2 * lp) * AP + a0);
        const float4* e1 = reinterpret_cast<const float4*>(s_e2 + (size_t)(2 * lp + 1) * AP + a0);
#pragma unroll
        for (int c4 = 0; c4 < CPT / 4; ++c4) {
          const float4 u = e0[c4];
          var[4 * c4 + 0] = fmaf(q0, u.x, var[4 * c4 + 0]); var[4 * c4 + 1] = fmaf(q0, u.y, var[4 * c4 + 1]);
          var[4 * c4 + 2] = fmaf(q0, u.z, var[4 * c4 + 2]); var[4 * c4 + 3] = fmaf(q0, u.w, var[4 * c4 + 3]);
        }
#pragma unroll
        for (int c4 = 0; c4 < CPT / 4; ++c4) {
          const float4 u = e1[c4];
          var[4 * c4 + 0] = fmaf(q1, u.x, var[4 * c4 + 0]); var[4 * c4 + 1] = fmaf(q1, u.y, var[4 * c4 + 1]);
          var[4 * c4 + 2] = fmaf(q1, u.z, var[4 * c4 + 2]); var[4 * c4 + 3] = fmaf(q1, u.w, var[4 * c4 + 3]);
        }
      }
    }
    float lq = 0.f, lh = 0.f;                         // this column group's share of the log-probability and of sum_a 0.5 log var
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      var[c] += p.eps;
      if (a0 + c < A) {
        const float hl = 0.5f * logf(var[c]);
        lq += -0.5f * (diff[c] * diff[c]) / var[c] - hl;
        lh += hl;
      }
    }
    s_red[cg * SDE_TILE + r] = lq;
    s_red[(4 + cg) * SDE_TILE + r] = lh;
    __syncthreads();
    float dlogp = 0.f;
    if (on) {
      const float logp = (((s_red[r] + s_red[SDE_TILE + r]) + s_red[2 * SDE_TILE + r]) + s_red[3 * SDE_TILE + r]) - 0.5f * A * 1.8378770664093453f;
      const float an = (p.adv[row] - adv_mean) / adv_den;
      const float lr = logp - p.old_logp[row];
      const float ratio = expf(lr);
      const float s1 = an * ratio, s2 = an * fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
      const bool inside = (ratio > 1.f - clip) && (ratio < 1.f + clip);
      dlogp = -(an * ratio) * ((s1 <= s2) ? 1.f : (inside ? 1.f : 0.f)) / B;
      if (cg == 0) {
        const float hsum = ((s_red[4 * SDE_TILE + r] + s_red[5 * SDE_TILE + r]) + s_red[6 * SDE_TILE + r]) + s_red[7 * SDE_TILE + r];
        const float err = sde_bf(p.value[row]) - p.returns[row];
        const float dv = (p.vf_coef * 2.0f / B) * err;
        p.dvalue[row] = myo_f2bf(dv);
        pl_s += fminf(s1, s2); vl_s += err * err; dv_s += dv;
        kl_s += (ratio - 1.f) - lr; cf_s += (fabsf(ratio - 1.f) > clip) ? 1.f : 0.f;
        el_s -= hsum + 0.5f * A * (1.0f + 1.8378770664093453f);
      }
    }
    const float ec = (p.ent_coef / B) * 0.5f;
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int a = a0 + c;
      float dm = 0.f, dvr = 0.f;
      if (on && a < A) {
        const float z2 = diff[c] * diff[c], v = var[c];
        dm = dlogp * diff[c] / v;
        dvr = dlogp * (0.5f * z2 / (v * v) - 0.5f / v) - ec / v;
        p.dmean[(size_t)row * A + a] = myo_f2bf(dm);
      }
      s_dmean[r * AP + a] = dm;
      s_dvar[r * AP + a] = dvr;
    }
    __syncthreads();
    if (t < A)
      for (int rr = 0; rr < SDE_TILE; ++rr) bsum += s_dmean[rr * AP + t];
    if (t < L) {
      for (int rr = 0; rr < SDE_TILE; ++rr) {
        const float x = sde_bf(s_lat[rr * LS + t]);
        const float q = x * x;
        const float4* dv4 = reinterpret_cast<const float4*>(s_dvar + rr * AP);
#pragma unroll
        for (int c4 = 0; c4 < CPT; ++c4) {
          const float4 u = dv4[c4];
          g[4 * c4 + 0] = fmaf(q, u.x, g[4 * c4 + 0]); g[4 * c4 + 1] = fmaf(q, u.y, g[4 * c4 + 1]);
          g[4 * c4 + 2] = fmaf(q, u.z, g[4 * c4 + 2]); g[4 * c4 + 3] = fmaf(q, u.w, g[4 * c4 + 3]);
        }
      }
    }
  }
  // the block's partials, plain stores: k_sde_finish adds them up
  const int NB = gridDim.x, blk = blockIdx.x;
  if (t < L) {
    float* out = p.gpart + ((size_t)blk * L + t) * A;
#pragma unroll
    for (int c = 0; c < AP; ++c)
      if (c < A) out[c] = g[c];
  }
  if (t < A) p.part[(size_t)t * NB + blk] = bsum;
  if (cg == 0) {
    for (int off = 32; off >= 1; off >>= 1) {
      pl_s += __shfl_xor(pl_s, off, 64); vl_s += __shfl_xor(vl_s, off, 64); dv_s += __shfl_xor(dv_s, off, 64);
      kl_s += __shfl_xor(kl_s, off, 64); cf_s += __shfl_xor(cf_s, off, 64); el_s += __shfl_xor(el_s, off, 64);
    }
    if (t == 0) {
      p.part[(size_t)SDE_C_PL(A) * NB + blk] = pl_s; p.part[(size_t)SDE_C_VL(A) * NB + blk] = vl_s;
      p.part[(size_t)SDE_C_DV(A) * NB + blk] = dv_s; p.part[(size_t)SDE_C_KL(A) * NB + blk] = kl_s;
      p.part[(size_t)(SDE_C_KL(A) + 1) * NB + blk] = cf_s; p.part[(size_t)(SDE_C_KL(A) + 2) * NB + blk] = el_s;
    }
  }
}

// Blocks 0 .. ceil(L A / 256) - 1: g_log_std[l,a] = 2 exp(2 log_std[l,a]) * sum over blocks (in block order) of the partials.
// The last block: wave 0 the two losses, the value head's bias gradient and the record in the hyper-parameter block; waves 1-3 the
// action head's bias gradient, one column per wave at a time.
__global__ void __launch_bounds__(256) k_sde_finish(const float* __restrict__ gpart, const float* __restrict__ part,
                                                    const float* __restrict__ log_std, int NB, int B, int L, int A,
                                                    float* __restrict__ g_log_std, float* __restrict__ g_bias_pi,
                                                    float* __restrict__ g_bias_vf, float* __restrict__ acc, float* __restrict__ hp) {
  const int t = threadIdx.x, LA = L * A;
  if ((int)blockIdx.x + 1 < (int)gridDim.x) {
    const int k = blockIdx.x * 256 + t;
    if (k >= LA) return;
    float s = 0.f;
    for (int b = 0; b < NB; ++b) s += gpart[(size_t)b * LA + k];
    g_log_std[k] = 2.0f * expf(2.0f * log_std[k]) * s;
    return;
  }
  const int wave = t >> 6, lane = t & 63;
  if (wave == 0) {
    const float pl = -myo_col_sum(part, SDE_C_PL(A), NB, lane) / B, vl = myo_col_sum(part, SDE_C_VL(A), NB, lane) / B;
    const float dv = myo_col_sum(part, SDE_C_DV(A), NB, lane);
    const float kl = myo_col_sum(part, SDE_C_KL(A), NB, lane) / B, cf = myo_col_sum(part, SDE_C_KL(A) + 1, NB, lane) / B;
    const float el = myo_col_sum(part, SDE_C_KL(A) + 2, NB, lane) / B;
    if (lane == 0) {
      acc[A] = pl; acc[A + 1] = vl;
      g_bias_vf[0] = dv;
      if (hp) (void)myo_hp_record(hp, pl, vl, kl, cf, el);
    }
    return;
  }
  for (int c = wave - 1; c < A; c += 3) {
    const float s = myo_col_sum(part, c, NB, lane);
    if (lane == 0) g_bias_pi[c] = s;
  }
}

template <int CPT>
static int sde_launch(const SdeArgs& a, int NB, hipStream_t st) {
  const size_t lds = sde_lds_bytes(a.L, 4 * CPT);
  if (lds > 64 * 1024) {               // beyond the default limit (a host-side attribute of the current device: not a stream operation)
    const hipError_t e = hipFuncSetAttribute((const void*)k_sde_loss<CPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(MYO_E_DEVICE, "myo_ppo_sde_loss_grad: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(k_sde_loss<CPT>, dim3(NB), dim3(256), (unsigned)lds, st, a);
  return MYO_OK;
}
