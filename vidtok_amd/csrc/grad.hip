// Backward-pass kernels of the decoder convolutions and LayerNorm sites (the first layer of decoder fine-tuning).
//
// vt_conv_wgrad: dW[co][k] = sum over output pixels m of dY[m][co] * im2col(X)[m][k], db[co] = sum_m dY[m][co], for the
// geometry of a forward vt_conv (taps, strides, pads, causal time mode, nearest x2 folded into the gather).  An MFMA
// implicit GEMM whose reduction runs over M: a workgroup of four waves owns a 64 (Cout) x 64 (K = taps x stored Cin) tile of
// dW and one contiguous range of M; every range writes its own fp32 partial tile into the workspace and a second kernel
// adds the ranges in index order, dropping pad channels into the reference layout [Cout][Cin][KT][KH][KW].  No float
// atomics: the result is bit-reproducible and capture-safe.
//
// vt_layernorm_act_backward: per-row LayerNorm(+SiLU) backward over channels-last rows, mean / rstd recomputed from the
// saved pre-norm rows; gamma / beta gradients as per-workgroup partials plus a fixed-order reduce.
#include "launch.h"

namespace {

// ---- convolution weight gradient --------------------------------------------------------------------------------------
constexpr int kWgBlock = 256;       // four waves
constexpr int kWgTile = 64;         // dW tile: 64 output channels x 64 reduction columns
constexpr int kWgMK = 32;           // pixels per LDS stage
constexpr int kWgLd = kWgMK + 1;    // LDS row (one tile row = one channel / column, pixels contiguous); +1 against bank conflicts

struct WgradArgs {
  const void* x;
  const void* dy;
  float* part;        // [nsplit][Cout][K]
  float* bpart;       // [nsplit][Cout] or null
  int64_t M;          // B * To * Ho * Wo
  int64_t chunk;      // pixels per split (multiple of kWgMK)
  int32_t K;          // KT * KH * KW * ldx
  int32_t B, Ti, Hi, Wi, ldx, To, Ho, Wo, lddy, Cout;
  int32_t KH, KW, st, sh, sw, pt, ph, pw, tmode, ups_t, ups_s;
};

template <typename T>
__global__ __launch_bounds__(kWgBlock) void conv_wgrad_kernel(const WgradArgs a) {
  __shared__ float sA[kWgTile * kWgLd];   // dY^T tile: [co][m]
  __shared__ float sB[kWgTile * kWgLd];   // im2col(X)^T tile: [k][m]
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const T* __restrict__ dy = static_cast<const T*>(a.dy);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = blockIdx.x * kWgTile, c0 = blockIdx.y * kWgTile, split = blockIdx.z;
  const int64_t mbeg = (int64_t)split * a.chunk, mend = std::min<int64_t>(a.M, mbeg + a.chunk);

  // this thread's load column: one output channel of dY and one reduction column of im2col(X), fixed for the whole range
  const int col = tid & 63, row0 = tid >> 6;
  const int co_ld = c0 + col, kk = k0 + col;
  const bool co_ok = co_ld < a.Cout, k_ok = kk < a.K;
  int ci = 0, tq = 0, tp = 0, ta = 0;
  if (k_ok) {
    ci = kk % a.ldx;
    const int tap = kk / a.ldx;
    tq = tap % a.KW;
    tp = (tap / a.KW) % a.KH;
    ta = tap / (a.KW * a.KH);
  }
  const int Tv = a.Ti << a.ups_t, Hv = a.Hi << a.ups_s, Wv = a.Wi << a.ups_s;

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const int wr = wave >> 1, wc = wave & 1;     // this wave's 32 x 32 quadrant of the tile

  __shared__ int sPix[kWgMK][4];      // per pixel of the stage: batch (-1 past the range), its window's first t / h / w
  for (int64_t m0 = mbeg; m0 < mend; m0 += kWgMK) {
    if (tid < kWgMK) {                 // the stage's pixels are decoded once, not once per column
      const int64_t m = m0 + tid;
      int b = -1, t0 = 0, h0 = 0, w0 = 0;
      if (m < mend) {
        const int wo = (int)(m % a.Wo);
        const int64_t m1 = m / a.Wo;
        const int ho = (int)(m1 % a.Ho);
        const int64_t m2 = m1 / a.Ho;
        b = (int)(m2 / a.To);
        t0 = (int)(m2 % a.To) * a.st - a.pt;
        h0 = ho * a.sh - a.ph;
        w0 = wo * a.sw - a.pw;
      }
      sPix[tid][0] = b;
      sPix[tid][1] = t0;
      sPix[tid][2] = h0;
      sPix[tid][3] = w0;
    }
    __syncthreads();
#pragma unroll
    for (int r = row0; r < kWgMK; r += kWgBlock / 64) {
      const int64_t m = m0 + r;
      const int b = sPix[r][0];
      float va = 0.f, vb = 0.f;
      if (b >= 0) {
        if (co_ok) va = to_f32<T>(dy[m * a.lddy + co_ld]);
        if (k_ok) {
          int tv = sPix[r][1] + ta;
          const int hv = sPix[r][2] + tp, wv = sPix[r][3] + tq;
          if (tv < 0 && a.tmode == VT_TPAD_REPLICATE) tv = 0;
          if (tv >= 0 && tv < Tv && hv >= 0 && hv < Hv && wv >= 0 && wv < Wv) {
            const int ti = tv >> a.ups_t, hi = hv >> a.ups_s, wi = wv >> a.ups_s;
            vb = to_f32<T>(x[((((int64_t)b * a.Ti + ti) * a.Hi + hi) * a.Wi + wi) * a.ldx + ci]);
          }
        }
      }
      sA[col * kWgLd + r] = va;
      sB[col * kWgLd + r] = vb;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < kWgTile) {      // db: the tile's column sums, in pixel order
#pragma unroll 8
      for (int r = 0; r < kWgMK; ++r) bsum += sA[tid * kWgLd + r];
    }
    const int li = lane & 15, lk = lane >> 4;
    if constexpr (is_h16<T>::value) {
      // v_mfma_f32_16x16x32: lane holds A[i = lane % 16][k = 8 (lane / 16) + 0..7] and B[k][j = lane % 16]
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        const float* pa = &sA[(wr * 32 + ib * 16 + li) * kWgLd + 8 * lk];
        u32x4 av;
#pragma unroll
        for (int v = 0; v < 4; ++v) av[v] = h16<T>::pack(pa[2 * v], pa[2 * v + 1]);     // exact: the values came from T
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
          const float* pb = &sB[(wc * 32 + jb * 16 + li) * kWgLd + 8 * lk];
          u32x4 bv;
#pragma unroll
          for (int v = 0; v < 4; ++v) bv[v] = h16<T>::pack(pb[2 * v], pb[2 * v + 1]);
          acc[ib][jb] = h16<T>::mfma16(av, bv, acc[ib][jb]);
        }
      }
    } else {
      // v_mfma_f32_16x16x4f32: lane holds A[i = lane % 16][k = lane / 16] and B[k][j = lane % 16]
#pragma unroll
      for (int ks = 0; ks < kWgMK; ks += 4) {
        float av[2], bv[2];
#pragma unroll
        for (int ib = 0; ib < 2; ++ib) av[ib] = sA[(wr * 32 + ib * 16 + li) * kWgLd + ks + lk];
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) bv[jb] = sB[(wc * 32 + jb * 16 + li) * kWgLd + ks + lk];
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
          for (int jb = 0; jb < 2; ++jb) acc[ib][jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ib], bv[jb], acc[ib][jb], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // D[i][j] of a 16 x 16 block: lane holds rows 4 (lane / 16) + 0..3 of column lane % 16
  float* part = a.part + (int64_t)split * a.Cout * a.K;
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) {
      const int kc = k0 + wc * 32 + jb * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = c0 + wr * 32 + ib * 16 + 4 * (lane >> 4) + r;
        if (co < a.Cout && kc < a.K) part[(int64_t)co * a.K + kc] = acc[ib][jb][r];
      }
    }
  if (a.bpart != nullptr && blockIdx.x == 0 && tid < kWgTile && c0 + tid < a.Cout) a.bpart[(int64_t)split * a.Cout + c0 + tid] = bsum;
}

// dW[co][ci][kt][kh][kw] = sum over splits (in index order) of part[s][co][tap * ldx + ci]; then db likewise.  Threads run
// over (co, tap, ci) with ci fastest, so the partial rows (read once per split) are read contiguously
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ bpart,
                                                                float* __restrict__ dw, float* __restrict__ db, int nsplit, int Cout,
                                                                int Cin, int taps, int ldx, int K) {
  const int64_t nw = (int64_t)Cout * Cin * taps;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nw) {
    const int ci = (int)(i % Cin);
    const int64_t r = i / Cin;
    const int tap = (int)(r % taps), co = (int)(r / taps);
    const int64_t off = (int64_t)co * K + (int64_t)tap * ldx + ci, stride = (int64_t)Cout * K;
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += part[k * stride + off];
    dw[((int64_t)co * Cin + ci) * taps + tap] = s;
  } else if (db != nullptr && i < nw + Cout) {
    const int co = (int)(i - nw);
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += bpart[(int64_t)k * Cout + co];
    db[co] = s;
  }
}

struct WgradPlan {
  int32_t nsplit;
  int64_t chunk, M, K, part_floats, bpart_floats;
};

int wgrad_plan(const vt_wgrad_desc* d, WgradPlan* p) {
  VT_CHECK_ARG(d != nullptr, "vt_conv_wgrad: null descriptor");
  VT_CHECK_ARG(d->dtype == VT_F32 || d->dtype == VT_BF16, "vt_conv_wgrad: dtype %d (F32 or BF16 operands)", d->dtype);
  VT_CHECK_ARG(d->B > 0 && d->Ti > 0 && d->Hi > 0 && d->Wi > 0 && d->To > 0 && d->Ho > 0 && d->Wo > 0, "vt_conv_wgrad: empty tensor");
  VT_CHECK_ARG(d->Cin > 0 && d->Cout > 0 && d->ldx >= d->Cin && d->lddy >= d->Cout, "vt_conv_wgrad: bad channel counts / strides");
  VT_CHECK_ARG(d->KT > 0 && d->KH > 0 && d->KW > 0 && d->st > 0 && d->sh > 0 && d->sw > 0, "vt_conv_wgrad: bad kernel / stride");
  VT_CHECK_ARG(d->pt >= 0 && d->ph >= 0 && d->pw >= 0, "vt_conv_wgrad: negative pad");
  VT_CHECK_ARG(d->tmode == VT_TPAD_ZERO || d->tmode == VT_TPAD_REPLICATE, "vt_conv_wgrad: tmode %d (ZERO or REPLICATE)", d->tmode);
  VT_CHECK_ARG((d->ups_t == 0 || d->ups_t == 1) && (d->ups_s == 0 || d->ups_s == 1), "vt_conv_wgrad: ups_t / ups_s must be 0 or 1");
  const int64_t K = (int64_t)d->KT * d->KH * d->KW * d->ldx;
  VT_CHECK_ARG(K < (int64_t)1 << 30, "vt_conv_wgrad: reduction width too large");
  const int64_t M = (int64_t)d->B * d->To * d->Ho * d->Wo;
  VT_CHECK_ARG(M < (int64_t)1 << 31, "vt_conv_wgrad: more than 2^31 output pixels");
  VT_CHECK_ARG(d->pt_hi >= 0 && d->ph_hi >= 0 && d->pw_hi >= 0, "vt_conv_wgrad: negative pad");
  const int64_t tiles = ((K + kWgTile - 1) / kWgTile) * ((d->Cout + kWgTile - 1) / kWgTile);
  const int64_t stages = (M + kWgMK - 1) / kWgMK;
  // enough workgroups to fill the chip twice over, each range at least 8 stages long; the split depends on the shape only
  int64_t ns = std::max<int64_t>(1, std::min<int64_t>((2048 + tiles - 1) / tiles, std::min<int64_t>(stages / 8, 64)));
  const int64_t per = (stages + ns - 1) / ns;
  ns = (stages + per - 1) / per;
  p->nsplit = (int32_t)std::max<int64_t>(ns, 1);
  p->chunk = per * kWgMK;
  p->M = M;
  p->K = K;
  p->part_floats = (int64_t)p->nsplit * d->Cout * K;
  p->bpart_floats = (int64_t)p->nsplit * d->Cout;
  return VT_OK;
}

// ---- LayerNorm(+SiLU) backward -------------------------------------------------------------------------------------------
constexpr int kLnBlock = 256;
constexpr int kLnMaxJ = 8;         // channels per lane: C <= 512, every LayerNorm site of the models (instantiated for 1, 2, 4, 8)
constexpr int kLnRowsPerWave = 8;  // rows a wave walks before the next workgroup takes over (sets the partial count)

template <typename T, typename TO, int NJ>
__global__ __launch_bounds__(kLnBlock) void layernorm_act_bwd_kernel(const T* __restrict__ y, const T* __restrict__ dn, int64_t ld,
                                                                     TO* __restrict__ dx, int64_t ldo, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float* __restrict__ gpart,
                                                                     float* __restrict__ bpart, int64_t M, int C, int64_t rows_per_wg,
                                                                     float eps, int silu) {
  __shared__ float sg[4][64 * NJ], sb[4][64 * NJ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nj = (C + 63) / 64;
  float g[NJ], bt[NJ], ag[NJ], ab[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    const bool ok = j < nj && c < C;
    g[j] = ok ? gamma[c] : 0.f;
    bt[j] = ok ? beta[c] : 0.f;
    ag[j] = ab[j] = 0.f;
  }
  const float invC = 1.0f / (float)C;
  const int64_t rbeg = (int64_t)blockIdx.x * rows_per_wg, rend = std::min<int64_t>(M, rbeg + rows_per_wg);
  for (int64_t row = rbeg + wave; row < rend; row += 4) {
    float v[NJ], d[NJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      const bool ok = j < nj && c < C;
      v[j] = ok ? to_f32<T>(y[row * ld + c]) : 0.f;
      d[j] = ok ? to_f32<T>(dn[row * ld + c]) : 0.f;
      s += v[j];
    }
    // a true division: C * fl(1 / C) is not 1 for most C, and the mean of a constant row has to be that constant -- one ulp of it,
    // times rstd = eps^-1/2 on such a row, is an x-hat of 1e-3 where it is 0
    const float mean = group_sum_dpp<64>(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      const float t = (j < nj && c < C) ? v[j] - mean : 0.f;
      q += t * t;
    }
    const float rstd = rsqrtf(group_sum_dpp<64>(q) * invC + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      const bool ok = j < nj && c < C;
      const float xh = ok ? (v[j] - mean) * rstd : 0.f;
      float du = d[j];
      if (silu) {
        const float u = g[j] * xh + bt[j];
        const float sg1 = 1.0f / (1.0f + __expf(-u));
        du *= sg1 * (1.0f + u * (1.0f - sg1));
      }
      if (!ok) du = 0.f;
      ag[j] += du * xh;
      ab[j] += du;
      const float dh = du * g[j];
      v[j] = xh;       // keep x-hat, d = dL/dx-hat
      d[j] = dh;
      s1 += dh;
      s2 += dh * xh;
    }
    s1 = group_sum_dpp<64>(s1) * invC;
    s2 = group_sum_dpp<64>(s2) * invC;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = lane + 64 * j;
      if (j < nj && c < ldo) dx[row * ldo + c] = from_f32<TO>(c < C ? rstd * (d[j] - s1 - v[j] * s2) : 0.f);
    }
  }
  // gamma / beta partials of this workgroup: the four waves added in wave order
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (j < nj && c < C) {
      sg[wave][c] = ag[j];
      sb[wave][c] = ab[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kLnBlock) {
    gpart[(int64_t)blockIdx.x * C + c] = ((sg[0][c] + sg[1][c]) + sg[2][c]) + sg[3][c];
    bpart[(int64_t)blockIdx.x * C + c] = ((sb[0][c] + sb[1][c]) + sb[2][c]) + sb[3][c];
  }
}

__global__ __launch_bounds__(256) void partial_rows_reduce_kernel(const float* __restrict__ gpart, const float* __restrict__ bpart,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta, int nparts, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float sg = 0.f, sb = 0.f;
  for (int k = 0; k < nparts; ++k) {
    sg += gpart[(int64_t)k * C + c];
    sb += bpart[(int64_t)k * C + c];
  }
  if (dgamma != nullptr) dgamma[c] = sg;
  if (dbeta != nullptr) dbeta[c] = sb;
}

int64_t ln_bwd_groups(int64_t M) { return grid_for(M, 4 * kLnRowsPerWave, 4096); }

}  // namespace

extern "C" int vt_wgrad_desc_size(void) { return (int)sizeof(vt_wgrad_desc); }

extern "C" int64_t vt_conv_wgrad_work_bytes(const vt_wgrad_desc* d) {
  WgradPlan p;
  if (wgrad_plan(d, &p) != VT_OK) return -1;
  return align256(p.part_floats * 4) + align256(p.bpart_floats * 4);
}

extern "C" int vt_conv_wgrad(const vt_wgrad_desc* d, vt_stream stream_) {
  hipStream_t stream = as_stream(stream_);
  WgradPlan p;
  const int rc = wgrad_plan(d, &p);
  if (rc != VT_OK) return rc;
  VT_CHECK_ARG(d->x && d->dy && d->dw && d->work, "vt_conv_wgrad: null pointer");
  const int64_t need = align256(p.part_floats * 4) + align256(p.bpart_floats * 4);
  VT_CHECK_ARG(d->work_bytes >= need, "vt_conv_wgrad: workspace of %lld bytes, need %lld (vt_conv_wgrad_work_bytes)",
               (long long)d->work_bytes, (long long)need);
  // the forward's output extent must lie inside the (virtually up-sampled, padded) input, or the descriptor is inconsistent
  const int Tv = d->Ti << d->ups_t, Hv = d->Hi << d->ups_s, Wv = d->Wi << d->ups_s;
  VT_CHECK_ARG((int64_t)(d->To - 1) * d->st + d->KT <= (int64_t)Tv + d->pt + d->pt_hi &&
                   (int64_t)(d->Ho - 1) * d->sh + d->KH <= (int64_t)Hv + d->ph + d->ph_hi &&
                   (int64_t)(d->Wo - 1) * d->sw + d->KW <= (int64_t)Wv + d->pw + d->pw_hi,
               "vt_conv_wgrad: output extent does not match the input and geometry");
  WgradArgs a;
  a.x = d->x;
  a.dy = d->dy;
  a.part = static_cast<float*>(d->work);
  a.bpart = d->db != nullptr ? reinterpret_cast<float*>(static_cast<char*>(d->work) + align256(p.part_floats * 4)) : nullptr;
  a.M = p.M;
  a.chunk = p.chunk;
  a.K = (int32_t)p.K;
  a.B = d->B; a.Ti = d->Ti; a.Hi = d->Hi; a.Wi = d->Wi; a.ldx = d->ldx;
  a.To = d->To; a.Ho = d->Ho; a.Wo = d->Wo; a.lddy = d->lddy; a.Cout = d->Cout;
  a.KH = d->KH; a.KW = d->KW; a.st = d->st; a.sh = d->sh; a.sw = d->sw;
  a.pt = d->pt; a.ph = d->ph; a.pw = d->pw; a.tmode = d->tmode; a.ups_t = d->ups_t; a.ups_s = d->ups_s;
  const dim3 grid((unsigned)((p.K + kWgTile - 1) / kWgTile), (unsigned)((d->Cout + kWgTile - 1) / kWgTile), (unsigned)p.nsplit);
  const int rc2 = vt_dispatch<float, bf16_t>(d->dtype, [&](auto t) { return launch(conv_wgrad_kernel<vt_t<decltype(t)>>, grid, dim3(kWgBlock), 0, stream, a); });
  if (rc2 != VT_OK) return rc2;
  const int taps = d->KT * d->KH * d->KW;
  const int64_t n = (int64_t)d->Cout * d->Cin * taps + (d->db != nullptr ? d->Cout : 0);
  return launch(conv_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.part, a.bpart, d->dw, d->db,
                p.nsplit, d->Cout, d->Cin, taps, d->ldx, a.K);
}

extern "C" int64_t vt_layernorm_act_backward_work_bytes(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0 || C > 64 * kLnMaxJ) return -1;
  return 2 * align256(ln_bwd_groups(M) * C * 4);
}

extern "C" int vt_layernorm_act_backward(const void* y, const void* dn, int32_t dtype, int64_t ld, void* dx, int32_t dx_dtype, int64_t ldo,
                                         const float* gamma, const float* beta, float* dgamma, float* dbeta, int64_t M, int32_t C, float eps,
                                         int32_t silu, void* work, int64_t work_bytes, vt_stream stream_) {
  hipStream_t stream = as_stream(stream_);
  VT_CHECK_ARG(y && dn && dx && gamma && beta && work, "vt_layernorm_act_backward: null pointer");
  VT_CHECK_ARG(M > 0 && C > 0 && C <= 64 * kLnMaxJ && ld >= C && ldo >= C && ldo <= 64 * ((C + 63) / 64),
               "vt_layernorm_act_backward: bad dims (M=%lld C=%d ld=%lld ldo=%lld; C <= 512, pad lanes of dx within the last 64)",
               (long long)M, C, (long long)ld, (long long)ldo);
  VT_CHECK_ARG(dtype == VT_F32 || dtype == VT_BF16, "vt_layernorm_act_backward: dtype %d (F32 or BF16)", dtype);
  VT_CHECK_ARG(dx_dtype == dtype || dx_dtype == VT_F32, "vt_layernorm_act_backward: dx dtype %d (the input's or F32)", dx_dtype);
  const int64_t groups = ln_bwd_groups(M);
  const int64_t pbytes = align256(groups * C * 4);
  VT_CHECK_ARG(work_bytes >= 2 * pbytes, "vt_layernorm_act_backward: workspace of %lld bytes, need %lld", (long long)work_bytes,
               (long long)(2 * pbytes));
  float* gpart = static_cast<float*>(work);
  float* bpart = reinterpret_cast<float*>(static_cast<char*>(work) + pbytes);
  const int64_t rows_per_wg = (M + groups - 1) / groups;
  const int nj = (C + 63) / 64;
  const int rc = vt_dispatch_grad(dtype, dx_dtype, [&](auto t, auto to) {
    using T = vt_t<decltype(t)>;
    using TO = vt_t<decltype(to)>;
    return vt_dispatch_int<1, 2, 4, kLnMaxJ>(nj <= 1 ? 1 : nj <= 2 ? 2 : nj <= 4 ? 4 : kLnMaxJ, [&](auto j) {
      return launch(layernorm_act_bwd_kernel<T, TO, decltype(j)::value>, dim3((unsigned)groups), dim3(kLnBlock), 0, stream, static_cast<const T*>(y),
                    static_cast<const T*>(dn), ld, static_cast<TO*>(dx), ldo, gamma, beta, gpart, bpart, M, C, rows_per_wg, eps, silu);
    });
  });
  if (rc != VT_OK) return rc;
  return launch(partial_rows_reduce_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, gpart, bpart, dgamma, dbeta, (int)groups, C);
}
