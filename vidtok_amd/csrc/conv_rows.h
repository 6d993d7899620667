// The row phase of the LDS-transposed convolution epilogues: conv_epilogue_lds128_at, conv_epilogue_lds256, conv_epilogue_lds256_pair
// (conv_igemm_kernel.h) and conv_epilogue_in8 (conv_in8.hip).  Each of them moves a finished accumulator tile (+ bias) through the LDS so that a lane
// ends up with 8 consecutive channels of a pixel row, and then does the same work on that row: residual add / alpha-mix, activation, store
// of y, LayerNorm(+SiLU) of the unrounded row, store of n.  Every piece of that is stated once, here.
//
// A row is held in one of two forms, and the arithmetic of a form is part of the results (the two sum in different orders):
//   * scalar-8, float[8]:  C = 128, 16 lanes a row (the 128-wide tile and conv_in8_kernel) -- one-pass LayerNorm = ln_row8<16> (common.h);
//   * pairs, f32x2[4]:     C = 256, 32 lanes a row (the 256-wide tile, plain and paired)  -- the same one-pass form on channel pairs
//                          (v_pk_add / mul / fma_f32: no MFMA runs on the CU during an epilogue, so packed fp32 costs what it says).
// 16-bit storage takes the one-pass LayerNorm, fp32 storage (fp32 / split-bf16 modes, held to 1e-3 of the oracle with FSQ codes bit-exact) the
// two-pass one.  Nothing here depends on FMA contraction: fused operations are spelled out, the rest are single operations (contract(off)).
#pragma once
#include <type_traits>

#include "conv_common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// ReLU of the ACT = VT_ACT_RELU epilogues (vt_conv_act): a select, so that -0 and negative results both become +0 (max-pooling the
// features afterwards is then bit-equal to torch's max_pool2d of them)
__device__ __forceinline__ float act_relu(float v) { return v > 0.0f ? v : 0.0f; }
__device__ __forceinline__ f32x2 act_relu(f32x2 v) { return f32x2{act_relu(v[0]), act_relu(v[1])}; }

__device__ __forceinline__ float ew_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ f32x2 ew_exp2(f32x2 x) { return f32x2{__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1])}; }
__device__ __forceinline__ float ew_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ f32x2 ew_rcp(f32x2 x) { return f32x2{__builtin_amdgcn_rcpf(x[0]), __builtin_amdgcn_rcpf(x[1])}; }

// ---- the tile in the LDS: T[row][W floats] (W = 128 or 256) as chunks of 4 floats, chunk index XOR (row & (W / 4 - 1)).  The 8 lanes a
// ds_write_b128 services together hold 8 different rows of one chunk -> 8 different columns; a lane's two chunks (2j, 2j + 1) stay adjacent.
template <int W>
__device__ __forceinline__ float* rows_chunk(float* T, int row, int chunk) {
  return T + row * W + ((chunk ^ (row & (W / 4 - 1))) << 2);
}
// 4 bias values from channel n, or zeros
__device__ __forceinline__ f32x4 rows_bias(const float* bias, int n) {
  if (bias) return *reinterpret_cast<const f32x4*>(bias + n);
  return f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}
// quad g of a 32 x 32 accumulator (one pixel, 4 consecutive channels) + bias -> channels [c, c + 4) of T row `row`
template <int W>
__device__ __forceinline__ void rows_scatter(float* T, int row, int c, const f32x16& acc, int g, const f32x4& bq) {
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = acc[4 * g + e] + bq[e];
  *reinterpret_cast<f32x4*>(rows_chunk<W>(T, row, c >> 2)) = v;
}
// lane j reads channels [8j, 8j + 8) of T row `row`
template <int W, typename E, int N>
__device__ __forceinline__ void rows_read(float* T, int row, int j, E (&v)[N]) {
  const f32x4 t0 = *reinterpret_cast<const f32x4*>(rows_chunk<W>(T, row, 2 * j));
  const f32x4 t1 = *reinterpret_cast<const f32x4*>(rows_chunk<W>(T, row, 2 * j + 1));
  if constexpr (std::is_same<E, float>::value) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e < 4 ? t0[e] : t1[e - 4];
  } else {
    v[0] = f32x2{t0[0], t0[1]}; v[1] = f32x2{t0[2], t0[3]}; v[2] = f32x2{t1[0], t1[1]}; v[3] = f32x2{t1[2], t1[3]};
  }
}

// ---- the LayerNorm affine of lane j's 8 channels; fold: scaled by -log2(e) for the one-pass SiLU form (ln_fold, common.h)
__device__ __forceinline__ void rows_affine(const ConvArgs& p, int j, bool fold, float (&g)[8], float (&b)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    g[e] = ln_fold(p.ln_gamma[8 * j + e], fold);
    b[e] = ln_fold(p.ln_beta[8 * j + e], fold);
  }
}
__device__ __forceinline__ void rows_affine(const ConvArgs& p, int j, bool fold, f32x2 (&g)[4], f32x2 (&b)[4]) {
  float gs[8], bs[8];
  rows_affine(p, j, fold, gs, bs);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    g[q] = f32x2{gs[2 * q], gs[2 * q + 1]};
    b[q] = f32x2{bs[2 * q], bs[2 * q + 1]};
  }
}

// ---- alpha r + (1 - alpha) v.  Scalar rows: one product rounded, the other fused into the sum -- channel 1 of a lane's eight rounds
// alpha r, the others (1 - alpha) v.  The channel index means nothing: it is an inherited artefact, what the optimiser made of the
// expression while contraction was left to it (the same in every instantiation: profiles/epilogue_rows_ab.txt, section 1), and the
// results are held to those bits.  Do not read a rule into it, and do not copy it.  Pair rows: both products rounded.
__device__ __forceinline__ float rows_mix(float r, float v, float alpha, int e) {
#pragma clang fp contract(off)
  const float beta = 1.0f - alpha;
  return e == 1 ? __builtin_fmaf(beta, v, alpha * r) : __builtin_fmaf(alpha, r, beta * v);
}
__device__ __forceinline__ f32x2 rows_mix(f32x2 r, f32x2 v, float alpha, int) {
#pragma clang fp contract(off)
  return r * alpha + v * (1.0f - alpha);
}

// ---- one-pass LayerNorm(+SiLU) of a row, 16-bit storage; g / b folded for SiLU.  Scalar rows: ln_row8.  Pair rows: the same form on
// channel pairs -- both moments together, t = x rstd - mean rstd, and for SiLU a = t g' + b': u sigmoid(u) = a * rcp(fma(2^a, -log2e, -log2e))
template <int G>
__device__ __forceinline__ void ln_row_one_pass(const float (&v)[8], const float (&g)[8], const float (&b)[8], float eps, bool silu, float (&o)[8]) {
  if (silu) ln_row8<G, true>(v, g, b, eps, o);
  else ln_row8<G, false>(v, g, b, eps, o);
}
template <int G>
__device__ __forceinline__ void ln_row_one_pass(const f32x2 (&v)[4], const f32x2 (&g)[4], const f32x2 (&b)[4], float eps, bool silu, float (&o)[8]) {
#pragma clang fp contract(off)
  const f32x2 s = (v[0] + v[1]) + (v[2] + v[3]);
  f32x2 qq = v[0] * v[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) qq = __builtin_elementwise_fma(v[q], v[q], qq);
  float nm;
  const float rstd = ln_row_stats<G>(s[0] + s[1], qq[0] + qq[1], eps, &nm);
  const f32x2 rstd2 = {rstd, rstd}, nm2 = {nm, nm}, c2 = {kNegLog2e, kNegLog2e};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x2 u = __builtin_elementwise_fma(__builtin_elementwise_fma(v[q], rstd2, nm2), g[q], b[q]);
    if (silu) u = u * ew_rcp(__builtin_elementwise_fma(ew_exp2(u), c2, c2));
    o[2 * q] = u[0];
    o[2 * q + 1] = u[1];
  }
}

// ---- two-pass LayerNorm(+SiLU) of a row, fp32 storage (statistics like layernorm_act_kernel); g / b as they are.  The forms differ in
// the order of the two sums only: scalar rows add the eight values, then the eight rounded squares, one after the other; pair rows add
// (v0 + v1) + (v2 + v3) and accumulate the squares by fma, per pair lane, then add the two lanes.
template <int G, typename E, int N>
__device__ __forceinline__ void ln_row_two_pass(const E (&v)[N], const E (&g)[N], const E (&b)[N], float eps, bool silu, float (&o)[8]) {
#pragma clang fp contract(off)
  constexpr bool kScalar = std::is_same<E, float>::value;
  constexpr float kInvC = 1.0f / (8.0f * G);
  float s;
  if constexpr (kScalar) {
    s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
  } else {
    const f32x2 s2 = (v[0] + v[1]) + (v[2] + v[3]);
    s = s2[0] + s2[1];
  }
  const float mean = group_sum_dpp<G>(s) * kInvC;
  E d[N];
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = v[i] - mean;
  float q;
  if constexpr (kScalar) {
    q = d[0] * d[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) {
      const float sq = d[e] * d[e];
      q += sq;
    }
  } else {
    f32x2 qq = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < N; ++i) qq = __builtin_elementwise_fma(d[i], d[i], qq);
    q = qq[0] + qq[1];
  }
  const float rstd = __builtin_amdgcn_rsqf(__builtin_fmaf(group_sum_dpp<G>(q), kInvC, eps));
#pragma unroll
  for (int i = 0; i < N; ++i) {
    E u = __builtin_elementwise_fma(d[i] * rstd, g[i], b[i]);
    if (silu) u = u * ew_rcp(ew_exp2(u * kNegLog2e) + 1.0f);       // u * sigmoid(u), the arithmetic of silu_fast
    if constexpr (kScalar) {
      o[i] = u;
    } else {
      o[2 * i] = u[0];
      o[2 * i + 1] = u[1];
    }
  }
}

// ---- one finished row: residual add / alpha-mix against rq (res_mode: a vt_res_mode; rq is read only with a residual), ACT, y, then the
// LayerNorm of the unrounded row as p.ln_mode says (1 plain, 2 + SiLU) into n.  G lanes hold the row; y / n: the lane's 8 channels there.
template <int G, typename TOut, int ACT, typename E, int N>
__device__ __forceinline__ void rows_finish(const ConvArgs& p, int res_mode, E (&v)[N], const Oct<TOut>& rq, float alpha, const E (&lg)[N],
                                            const E (&lb)[N], TOut* y, TOut* n) {
  constexpr bool kScalar = std::is_same<E, float>::value;
  static_assert(N * sizeof(E) == 32 && G == (kScalar ? 16 : 32), "scalar-8 rows on 16 lanes, pair rows on 32");
  auto res = [&](int i) -> E {
    if constexpr (kScalar) return rq.get(i);
    else return f32x2{rq.get(2 * i), rq.get(2 * i + 1)};
  };
  if (res_mode == VT_RES_ADD) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = res(i) + v[i];
  } else if (res_mode == VT_RES_MIX) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = rows_mix(res(i), v[i], alpha, i);
  }
  if constexpr (ACT == VT_ACT_RELU) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = act_relu(v[i]);
  }
  if (!p.ln_mode || p.ln_keep_y) {
    float yv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (kScalar) yv[e] = v[e];
      else yv[e] = v[e >> 1][e & 1];
    }
    Oct<TOut>::store(y, yv, p.nt_store != 0);
  }
  if (!p.ln_mode) return;   // uniform; statistics of the fp32 row, taken before the rounding to TOut
  float o[8];
  if constexpr (sizeof(TOut) == 2) ln_row_one_pass<G>(v, lg, lb, p.ln_eps, p.ln_mode == 2, o);
  else ln_row_two_pass<G>(v, lg, lb, p.ln_eps, p.ln_mode == 2, o);
  Oct<TOut>::store(n, o, p.nt_store != 0);
}

}  // namespace
