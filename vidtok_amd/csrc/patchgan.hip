// The kernels of the 2-D PatchGAN discriminator (include/vidtok_amd.h, "PatchGAN discriminator"): batch-statistics BatchNorm with
// LeakyReLU forward and backward, the LeakyReLU backward of the un-normalised first layer, and the data gradient of a convolution with
// row / column stride 2.
//
// Rows are NDHWC pixels [M][ld]; a lane owns 8 consecutive channels of a row (row8.h), a workgroup walks a fixed range of rows.  Every
// sum over rows is a per-workgroup partial in the caller's `work`, added in index order by a second launch (fp64 in that launch): no
// atomics, two runs give the same bits, nothing allocates or synchronises.
//
// vt_conv_dgrad_strided: an input pixel of parity class (rh, rw) = (h mod sh, w mod sw) receives only the taps with (r + p - k) mod s = 0,
// so each class is a stride-1 convolution of dy with a flipped, transposed sub-kernel (vt_pack_conv_weight_dgrad_strided).  The classes run
// on vt_conv unchanged, fp32 into `work`; strided_finish_kernel interleaves them, adds acc and rounds once.  No zero-dilated dy.
#include <algorithm>

#include "row8.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxC = 512;              // a lane per 8 channels, up to 64 lanes a row
constexpr int kMaxGroups = 1024;        // per-workgroup partials of one reduction

inline bool pg_dtype_ok(int dt) { return dt == VT_F32 || dt == VT_BF16; }
inline int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

// rows walked side by side by one workgroup (nq lanes a row), and the workgroups of a reduction over M rows
inline int rows_par(int nq) { return kBlock / nq; }
inline int64_t reduce_groups(int64_t M, int nq) {
  const int64_t per = (int64_t)rows_par(nq) * 8;
  return std::max<int64_t>(1, std::min<int64_t>((M + per - 1) / per, kMaxGroups));
}

// the pre-activation of a normalised channel: ONE expression for the forward and the backward's sign mask
__device__ __forceinline__ float bn_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float bn_pre(float xh, float g, float b) { return __builtin_fmaf(xh, g, b); }
__device__ __forceinline__ float leaky_slope(float pre, float slope) { return pre > 0.0f ? 1.0f : slope; }

struct Chan8 {
  float mean[8], rstd[8], g[8], b[8];
};
__device__ __forceinline__ void load_chan8(Chan8& p, const float* mean, const float* rstd, const float* gamma, const float* beta, int c0, int C) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const bool ok = c0 + e < C;
    p.mean[e] = ok ? mean[c0 + e] : 0.f;
    p.rstd[e] = ok ? rstd[c0 + e] : 0.f;
    p.g[e] = ok ? gamma[c0 + e] : 0.f;
    p.b[e] = ok ? beta[c0 + e] : 0.f;
  }
}

// ---- statistics: fp64 partial sums of x and x^2 per workgroup ------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void bn_stats_kernel(const T* __restrict__ x, int64_t ld, int64_t M, int C, int nq, int64_t rows_per_wg,
                                                          double* __restrict__ part) {
  extern __shared__ double sm[];                  // [rows_par][2][nq * 8]
  const int rp = kBlock / nq;
  const int q = threadIdx.x % nq, rs = threadIdx.x / nq;
  double s[8], ss[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = ss[e] = 0.0;
  const int64_t rbeg = (int64_t)blockIdx.x * rows_per_wg, rend = std::min<int64_t>(M, rbeg + rows_per_wg);
  if (rs < rp)
    for (int64_t row = rbeg + rs; row < rend; row += rp) {
      float v[8];
      Row8<T>::load(x + row * ld + q * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double d = (double)v[e];
        s[e] += d;
        ss[e] += d * d;
      }
    }
  const int w8 = nq * 8;
  if (rs < rp) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sm[(rs * 2 + 0) * w8 + q * 8 + e] = s[e];
      sm[(rs * 2 + 1) * w8 + q * 8 + e] = ss[e];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kBlock) {
    double a = 0.0, b = 0.0;
    for (int r = 0; r < rp; ++r) {
      a += sm[(r * 2 + 0) * w8 + c];
      b += sm[(r * 2 + 1) * w8 + c];
    }
    part[((int64_t)blockIdx.x * 2 + 0) * C + c] = a;
    part[((int64_t)blockIdx.x * 2 + 1) * C + c] = b;
  }
}

__global__ __launch_bounds__(kBlock) void bn_stats_finish_kernel(const double* __restrict__ part, int nparts, int64_t M, int C, float eps,
                                                                 float* __restrict__ mean, float* __restrict__ var, float* __restrict__ rstd) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int k = 0; k < nparts; ++k) {
    a += part[((int64_t)k * 2 + 0) * C + c];
    b += part[((int64_t)k * 2 + 1) * C + c];
  }
  const double m = a / (double)M;
  const double v = std::max(b / (double)M - m * m, 0.0);
  mean[c] = (float)m;
  var[c] = (float)v;
  if (rstd != nullptr) rstd[c] = (float)(1.0 / sqrt(v + (double)eps));
}

// ---- y = leaky(gamma (x - mean) rstd + beta) -------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void bn_act_kernel(const T* __restrict__ x, int64_t ld, T* __restrict__ y, int64_t ldy, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float slope, int64_t M, int C) {
  // a lane keeps its 8 channels for the whole walk (the grid's threads are dealt out nq to a row), so the channel vectors load once
  const int nq = (int)(ldy / 8);
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock / nq;
  const int c0 = (int)(tid % nq) * 8;
  if (tid / nq >= step) return;
  Chan8 p;
  load_chan8(p, mean, rstd, gamma, beta, c0, C);
  for (int64_t row = tid / nq; row < M; row += step) {
    float o[8];
    if (c0 < C) {
      float v[8];
      Row8<T>::load(x + row * ld + c0, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float pre = bn_pre(bn_xhat(v[e], p.mean[e], p.rstd[e]), p.g[e], p.b[e]);
        o[e] = c0 + e < C ? pre * leaky_slope(pre, slope) : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
    }
    Row8<T>::store(y + row * ldy + c0, o);
  }
}

// ---- backward, pass 1: per-workgroup partials of sum g and sum g x-hat, g = dy * (pre > 0 ? 1 : slope) ---------------------------------------
template <typename T, typename TD>
__global__ __launch_bounds__(kBlock) void bn_bwd_sums_kernel(const T* __restrict__ x, const TD* __restrict__ dy, int64_t ld, int64_t lddy,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float slope, int64_t M, int C, int nq, int64_t rows_per_wg,
                                                             float* __restrict__ part) {
  extern __shared__ float smf[];                  // [rows_par][2][nq * 8]
  const int rp = kBlock / nq;
  const int q = threadIdx.x % nq, rs = threadIdx.x / nq;
  const int c0 = q * 8;
  Chan8 p;
  load_chan8(p, mean, rstd, gamma, beta, c0, C);
  float sb[8], sg[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sb[e] = sg[e] = 0.f;
  const int64_t rbeg = (int64_t)blockIdx.x * rows_per_wg, rend = std::min<int64_t>(M, rbeg + rows_per_wg);
  if (rs < rp)
    for (int64_t row = rbeg + rs; row < rend; row += rp) {
      float v[8], d[8];
      Row8<T>::load(x + row * ld + c0, v);
      Row8<TD>::load(dy + row * lddy + c0, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = bn_xhat(v[e], p.mean[e], p.rstd[e]);
        const float g = c0 + e < C ? d[e] * leaky_slope(bn_pre(xh, p.g[e], p.b[e]), slope) : 0.f;
        sb[e] += g;
        sg[e] = __builtin_fmaf(g, xh, sg[e]);
      }
    }
  const int w8 = nq * 8;
  if (rs < rp) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      smf[(rs * 2 + 0) * w8 + c0 + e] = sb[e];
      smf[(rs * 2 + 1) * w8 + c0 + e] = sg[e];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kBlock) {
    float a = 0.f, b = 0.f;
    for (int r = 0; r < rp; ++r) {
      a += smf[(r * 2 + 0) * w8 + c];
      b += smf[(r * 2 + 1) * w8 + c];
    }
    part[((int64_t)blockIdx.x * 2 + 0) * C + c] = a;
    part[((int64_t)blockIdx.x * 2 + 1) * C + c] = b;
  }
}

// the partials in index order (fp64) -> sums [2][C] fp32 (sum g, sum g x-hat), and dbeta / dgamma where asked for
__global__ __launch_bounds__(kBlock) void bn_bwd_reduce_kernel(const float* __restrict__ part, int nparts, int C, float* __restrict__ sums,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int k = 0; k < nparts; ++k) {
    a += (double)part[((int64_t)k * 2 + 0) * C + c];
    b += (double)part[((int64_t)k * 2 + 1) * C + c];
  }
  sums[c] = (float)a;
  sums[C + c] = (float)b;
  if (dbeta != nullptr) dbeta[c] = (float)a;
  if (dgamma != nullptr) dgamma[c] = (float)b;
}

// pass 2: dx = gamma rstd (g - sum g / M - x-hat sum(g x-hat) / M) (batch) or gamma rstd g (running)
template <typename T, typename TD>
__global__ __launch_bounds__(kBlock) void bn_bwd_dx_kernel(const T* __restrict__ x, const TD* __restrict__ dy, int64_t ld, int64_t lddy, T* __restrict__ dx,
                                                           int64_t ldo, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                                           const float* __restrict__ sums, int64_t M, int C, int batch) {
  const int nq = (int)(ldo / 8);
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x, step = (int64_t)gridDim.x * kBlock / nq;
  const int c0 = (int)(tid % nq) * 8;
  if (tid / nq >= step) return;
  const float invM = 1.0f / (float)M;
  Chan8 p;
  load_chan8(p, mean, rstd, gamma, beta, c0, C);
  float sb[8], sg[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const bool ok = batch && c0 + e < C;
    sb[e] = ok ? sums[c0 + e] * invM : 0.f;
    sg[e] = ok ? sums[C + c0 + e] * invM : 0.f;
  }
  for (int64_t row = tid / nq; row < M; row += step) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
    if (c0 < C) {
      float v[8], d[8];
      Row8<T>::load(x + row * ld + c0, v);
      Row8<TD>::load(dy + row * lddy + c0, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (c0 + e < C) {
          const float xh = bn_xhat(v[e], p.mean[e], p.rstd[e]);
          float g = d[e] * leaky_slope(bn_pre(xh, p.g[e], p.b[e]), slope);
          if (batch) g = g - sb[e] - xh * sg[e];
          o[e] = p.g[e] * p.rstd[e] * g;
        }
      }
    }
    Row8<T>::store(dx + row * ldo + c0, o);
  }
}

// ---- dx = dy * (y > 0 ? 1 : slope), y the saved post-activation --------------------------------------------------------------------------
template <typename T, typename TD>
__global__ __launch_bounds__(kBlock) void leaky_bwd_kernel(const TD* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, float slope, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kBlock) {
    float d[8], v[8], o[8];
    Row8<TD>::load(dy + i * 8, d);
    Row8<T>::load(y + i * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = d[e] * leaky_slope(v[e], slope);
    Row8<T>::store(dx + i * 8, o);
  }
}

inline unsigned grid_for(int64_t n, int64_t cap = 16384) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, cap)); }

// ---- strided data gradient ---------------------------------------------------------------------------------------------------------------
// one axis of a parity class r: the taps k0, k0 + s, ... (nk of them), the front pad of the class convolution over dy, its output extent
struct AxisClass {
  int k0, nk, pad, n;
};
inline AxisClass axis_class(int K, int s, int p, int r, int extent) {
  AxisClass a;
  a.k0 = (r + p) % s;
  a.nk = K > a.k0 ? (K - a.k0 + s - 1) / s : 0;
  a.pad = a.nk - 1 - (r + p) / s;
  a.n = extent > r ? (extent - r + s - 1) / s : 0;
  return a;
}

// out[cls][ci][k], k = ((a' nkh + p') nkw + q') cout_p + co  <-  w[co][ci][KT-1-a'][kh0 + sh (nkh-1-p')][kw0 + sw (nkw-1-q')]; the rest zero
template <typename TO>
__global__ __launch_bounds__(kBlock) void pack_dgrad_strided_kernel(const float* __restrict__ w, TO* __restrict__ out, int Cout, int Cin, int cout_p, int KT,
                                                                    int KH, int KW, int sh, int sw, int ph, int pw, long long ldw) {
  const long long per = (long long)Cin * ldw;
  const long long n = per * sh * sw;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const int cls = (int)(i / per);
    const long long j = i - cls * per;
    const long long ci = j / ldw;
    const int k = (int)(j - ci * ldw);
    const int rh = cls / sw, rw = cls - rh * sw;
    const int kh0 = (rh + ph) % sh, kw0 = (rw + pw) % sw;
    const int nkh = KH > kh0 ? (KH - kh0 + sh - 1) / sh : 0, nkw = KW > kw0 ? (KW - kw0 + sw - 1) / sw : 0;
    const int tap = k / cout_p, co = k - tap * cout_p;
    float v = 0.0f;
    if (tap < KT * nkh * nkw && co < Cout) {
      const int q = tap % nkw, pp = (tap / nkw) % nkh, a = tap / (nkw * nkh);
      const int kt = KT - 1 - a, kh = kh0 + sh * (nkh - 1 - pp), kw = kw0 + sw * (nkw - 1 - q);
      v = w[((((long long)co * Cin + ci) * KT + kt) * KH + kh) * KW + kw];
    }
    out[i] = from_f32<TO>(v);
  }
}

struct FinishArgs {
  const float* work;
  const void* acc;
  void* dx;
  long long off[4];      // class (rh, rw) at off[rh * sw + rw] floats into work, or -1: no tap reaches the class (zeros)
  int nh[4], nw[4];
  int B, T, H, W, C, ld, lda, sh, sw;
};

template <typename TO>
__global__ __launch_bounds__(kBlock) void strided_finish_kernel(const FinishArgs a) {
  const TO* __restrict__ acc = static_cast<const TO*>(a.acc);
  TO* __restrict__ dx = static_cast<TO*>(a.dx);
  const int q = a.ld / 4;
  const long long n = (long long)a.B * a.T * a.H * a.W * q;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const int c0 = (int)(i % q) * 4;
    long long r = i / q;
    const int w = (int)(r % a.W);
    r /= a.W;
    const int h = (int)(r % a.H);
    const long long bt = r / a.H;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (c0 < a.C) {
      const int cls = (h % a.sh) * a.sw + (w % a.sw);
      if (a.off[cls] >= 0) {
        const float* p = a.work + a.off[cls] + ((bt * a.nh[cls] + h / a.sh) * a.nw[cls] + w / a.sw) * a.ld + c0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c0 + e < a.C) s[e] = p[e];
      }
      if (acc) {
        const TO* p = acc + ((bt * a.H + h) * a.W + w) * a.lda + c0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c0 + e < a.C) s[e] += to_f32<TO>(p[e]);
      }
    }
    TO* o = dx + ((bt * a.H + h) * a.W + w) * a.ld + c0;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = from_f32<TO>(s[e]);
  }
}

struct StridedPlan {
  AxisClass ah[2], aw[2];
  int64_t off[4];        // bytes into work
  int64_t bytes;
};

int strided_prepare(const vt_dgrad_desc* d, StridedPlan* p) {
  VT_CHECK_ARG(d != nullptr, "vt_conv_dgrad_strided: null descriptor");
  VT_CHECK_ARG(pg_dtype_ok(d->dtype) && (d->dx_dtype == d->dtype || d->dx_dtype == VT_F32),
               "vt_conv_dgrad_strided: dtype %d -> dx_dtype %d (fp32 or bf16 operands; dx in the operand type or fp32)", d->dtype, d->dx_dtype);
  VT_CHECK_ARG(d->st == 1 && (d->sh == 1 || d->sh == 2) && (d->sw == 1 || d->sw == 2) && d->sh + d->sw > 2,
               "vt_conv_dgrad_strided: strides (%d, %d, %d): st = 1 and sh, sw in {1, 2} with at least one 2 (vt_conv_dgrad serves stride 1)", d->st, d->sh, d->sw);
  VT_CHECK_ARG(d->tmode == VT_TPAD_ZERO && d->ups_t == 0 && d->ups_s == 0, "vt_conv_dgrad_strided: tmode %d, ups (%d, %d): zero time pad, no folded up-sampling",
               d->tmode, d->ups_t, d->ups_s);
  VT_CHECK_ARG(d->B > 0 && d->Ti > 0 && d->Hi > 0 && d->Wi > 0 && d->Cin > 0 && d->Cout > 0 && d->To > 0 && d->Ho > 0 && d->Wo > 0, "vt_conv_dgrad_strided: bad dims");
  VT_CHECK_ARG(d->KT > 0 && d->KT <= 4 && d->KH > 0 && d->KH <= 4 && d->KW > 0 && d->KW <= 4, "vt_conv_dgrad_strided: taps (%d, %d, %d): 1 .. 4 an axis", d->KT, d->KH, d->KW);
  VT_CHECK_ARG(d->pt >= 0 && d->pt < d->KT && d->pt_hi >= 0 && d->pt_hi < d->KT && d->ph >= 0 && d->ph < d->KH && d->ph_hi >= 0 && d->ph_hi < d->KH && d->pw >= 0 &&
                   d->pw < d->KW && d->pw_hi >= 0 && d->pw_hi < d->KW, "vt_conv_dgrad_strided: a pad must be smaller than its kernel extent");
  VT_CHECK_ARG(d->To == d->Ti + d->pt + d->pt_hi - d->KT + 1 && d->Ho == (d->Hi + d->ph + d->ph_hi - d->KH) / d->sh + 1 && d->Hi + d->ph + d->ph_hi >= d->KH &&
                   d->Wo == (d->Wi + d->pw + d->pw_hi - d->KW) / d->sw + 1 && d->Wi + d->pw + d->pw_hi >= d->KW,
               "vt_conv_dgrad_strided: dy extents (%d, %d, %d) are not the forward convolution's", d->To, d->Ho, d->Wo);
  const int vec = d->dtype == VT_BF16 ? 8 : 4;
  VT_CHECK_ARG(d->lddy >= d->Cout && d->lddy % vec == 0 && d->lddx >= d->Cin && d->lddx % 4 == 0, "vt_conv_dgrad_strided: lddy %d / lddx %d", d->lddy, d->lddx);
  const int nkh = (d->KH + d->sh - 1) / d->sh, nkw = (d->KW + d->sw - 1) / d->sw;
  VT_CHECK_ARG(d->ldw >= (int64_t)d->KT * nkh * nkw * d->lddy && d->ldw % vec == 0, "vt_conv_dgrad_strided: ldw %d (vt_pack_conv_weight_dgrad_strided: KT ceil(KH/sh) ceil(KW/sw) lddy)",
               d->ldw);
  VT_CHECK_ARG(d->acc == nullptr || d->ldacc >= d->Cin, "vt_conv_dgrad_strided: ldacc %d", d->ldacc);
  int64_t at = 0;
  for (int rh = 0; rh < d->sh; ++rh) p->ah[rh] = axis_class(d->KH, d->sh, d->ph, rh, d->Hi);
  for (int rw = 0; rw < d->sw; ++rw) p->aw[rw] = axis_class(d->KW, d->sw, d->pw, rw, d->Wi);
  for (int rh = 0; rh < d->sh; ++rh)
    for (int rw = 0; rw < d->sw; ++rw) {
      const AxisClass &h = p->ah[rh], &w = p->aw[rw];
      VT_CHECK_ARG(h.pad >= 0 && w.pad >= 0, "vt_conv_dgrad_strided: pads (%d, %d) put a class convolution in front of dy's first pixel", d->ph, d->pw);
      const int cls = rh * d->sw + rw;
      if (h.nk == 0 || w.nk == 0 || h.n == 0 || w.n == 0) {
        p->off[cls] = -1;
        continue;
      }
      p->off[cls] = at;
      at += align256((int64_t)d->B * d->Ti * h.n * w.n * d->lddx * 4);
    }
  p->bytes = at;
  return VT_OK;
}

}  // namespace

extern "C" int64_t vt_batchnorm_stats_work_bytes(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0 || C > kMaxC) return -1;
  return align256(reduce_groups(M, (C + 7) / 8) * 2 * C * 8);
}

extern "C" int vt_batchnorm_stats(const void* x, int32_t dtype, int64_t ld, int64_t M, int32_t C, float eps, float* mean, float* var, float* rstd, void* work,
                                  int64_t work_bytes, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(x && mean && var && work, "vt_batchnorm_stats: null pointer");
  VT_CHECK_ARG(pg_dtype_ok(dtype), "vt_batchnorm_stats: dtype %d (F32 or BF16)", dtype);
  VT_CHECK_ARG(M > 0 && C > 0 && C <= kMaxC && ld % 8 == 0 && ld >= (C + 7) / 8 * 8, "vt_batchnorm_stats: bad dims (M=%lld C=%d ld=%lld; C <= 512, ld a multiple of 8)",
               (long long)M, C, (long long)ld);
  VT_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(work) & 15) == 0, "vt_batchnorm_stats: tensors must be 16-byte aligned");
  const int nq = (C + 7) / 8;
  const int64_t groups = reduce_groups(M, nq);
  VT_CHECK_ARG(work_bytes >= align256(groups * 2 * C * 8), "vt_batchnorm_stats: workspace of %lld bytes, need %lld (vt_batchnorm_stats_work_bytes)",
               (long long)work_bytes, (long long)align256(groups * 2 * C * 8));
  const int64_t rows_per_wg = (M + groups - 1) / groups;
  const size_t lds = (size_t)rows_par(nq) * 2 * nq * 8 * sizeof(double);
  double* part = static_cast<double*>(work);
  if (dtype == VT_F32)
    hipLaunchKernelGGL(bn_stats_kernel<float>, dim3((unsigned)groups), dim3(kBlock), lds, stream, static_cast<const float*>(x), ld, M, C, nq, rows_per_wg, part);
  else
    hipLaunchKernelGGL(bn_stats_kernel<bf16_t>, dim3((unsigned)groups), dim3(kBlock), lds, stream, static_cast<const bf16_t*>(x), ld, M, C, nq, rows_per_wg, part);
  VT_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((unsigned)((C + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, part, (int)groups, M, C, eps, mean, var, rstd);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int vt_batchnorm_act(const void* x, int32_t dtype, int64_t ld, void* y, int64_t ldy, const float* mean, const float* rstd, const float* gamma,
                                const float* beta, float slope, int64_t M, int32_t C, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(x && y && mean && rstd && gamma && beta, "vt_batchnorm_act: null pointer");
  VT_CHECK_ARG(pg_dtype_ok(dtype), "vt_batchnorm_act: dtype %d (F32 or BF16)", dtype);
  VT_CHECK_ARG(M > 0 && C > 0 && ld % 8 == 0 && ldy % 8 == 0 && ld >= (C + 7) / 8 * 8 && ldy >= C, "vt_batchnorm_act: bad dims (M=%lld C=%d ld=%lld ldy=%lld; strides multiples of 8)",
               (long long)M, C, (long long)ld, (long long)ldy);
  VT_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0, "vt_batchnorm_act: tensors must be 16-byte aligned");
  const unsigned grid = grid_for(M * (ldy / 8));
  if (dtype == VT_F32)
    hipLaunchKernelGGL(bn_act_kernel<float>, dim3(grid), dim3(kBlock), 0, stream, static_cast<const float*>(x), ld, static_cast<float*>(y), ldy, mean, rstd, gamma, beta,
                       slope, M, C);
  else
    hipLaunchKernelGGL(bn_act_kernel<bf16_t>, dim3(grid), dim3(kBlock), 0, stream, static_cast<const bf16_t*>(x), ld, static_cast<bf16_t*>(y), ldy, mean, rstd, gamma,
                       beta, slope, M, C);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int64_t vt_batchnorm_act_backward_work_bytes(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0 || C > kMaxC) return -1;
  return align256(reduce_groups(M, (C + 7) / 8) * 2 * C * 4) + align256(2 * C * 4);
}

extern "C" int vt_batchnorm_act_backward(const void* x, const void* dy, int32_t dtype, int32_t dy_dtype, int64_t ld, int64_t lddy, void* dx, int64_t ldo,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta, float slope, float* dgamma, float* dbeta,
                                         int64_t M, int32_t C, int32_t mode, void* work, int64_t work_bytes, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(x && dy && dx && mean && rstd && gamma && beta && work, "vt_batchnorm_act_backward: null pointer");
  VT_CHECK_ARG(pg_dtype_ok(dtype) && (dy_dtype == dtype || dy_dtype == VT_F32), "vt_batchnorm_act_backward: dtype %d (F32 or BF16), dy_dtype %d (dtype or F32)", dtype,
               dy_dtype);
  VT_CHECK_ARG(mode == VT_BN_BATCH || mode == VT_BN_RUNNING, "vt_batchnorm_act_backward: mode %d (VT_BN_BATCH or VT_BN_RUNNING)", mode);
  const int64_t c8 = (C + 7) / 8 * 8;
  VT_CHECK_ARG(M > 0 && C > 0 && C <= kMaxC && ld % 8 == 0 && lddy % 8 == 0 && ldo % 8 == 0 && ld >= c8 && lddy >= c8 && ldo >= C,
               "vt_batchnorm_act_backward: bad dims (M=%lld C=%d ld=%lld lddy=%lld ldo=%lld; C <= 512, strides multiples of 8)", (long long)M, C, (long long)ld,
               (long long)lddy, (long long)ldo);
  VT_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(dy) & 15) == 0 && (reinterpret_cast<uintptr_t>(dx) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(work) & 15) == 0, "vt_batchnorm_act_backward: tensors must be 16-byte aligned");
  const int nq = (C + 7) / 8;
  const int64_t groups = reduce_groups(M, nq);
  const int64_t pbytes = align256(groups * 2 * C * 4);
  VT_CHECK_ARG(work_bytes >= pbytes + align256(2 * C * 4), "vt_batchnorm_act_backward: workspace of %lld bytes, need %lld (vt_batchnorm_act_backward_work_bytes)",
               (long long)work_bytes, (long long)(pbytes + align256(2 * C * 4)));
  float* part = static_cast<float*>(work);
  float* sums = reinterpret_cast<float*>(static_cast<char*>(work) + pbytes);
  const int64_t rows_per_wg = (M + groups - 1) / groups;
  const size_t lds = (size_t)rows_par(nq) * 2 * nq * 8 * sizeof(float);
  const bool need_sums = mode == VT_BN_BATCH || dgamma != nullptr || dbeta != nullptr;
  const unsigned grid = grid_for(M * (ldo / 8));
  const int batch = mode == VT_BN_BATCH;
#define VT_BN_BWD(T, TD)                                                                                                                                     \
  do {                                                                                                                                                       \
    if (need_sums) {                                                                                                                                         \
      hipLaunchKernelGGL((bn_bwd_sums_kernel<T, TD>), dim3((unsigned)groups), dim3(kBlock), lds, stream, static_cast<const T*>(x), static_cast<const TD*>(dy), ld, \
                         lddy, mean, rstd, gamma, beta, slope, M, C, nq, rows_per_wg, part);                                                                 \
      hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((unsigned)((C + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, part, (int)groups, C, sums, dgamma, dbeta); \
    }                                                                                                                                                        \
    hipLaunchKernelGGL((bn_bwd_dx_kernel<T, TD>), dim3(grid), dim3(kBlock), 0, stream, static_cast<const T*>(x), static_cast<const TD*>(dy), ld, lddy,         \
                       static_cast<T*>(dx), ldo, mean, rstd, gamma, beta, slope, sums, M, C, batch);                                                         \
  } while (0)
  if (dtype == VT_F32)
    VT_BN_BWD(float, float);
  else if (dy_dtype == VT_F32)
    VT_BN_BWD(bf16_t, float);
  else
    VT_BN_BWD(bf16_t, bf16_t);
#undef VT_BN_BWD
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int vt_leaky_relu_backward(const void* dy, int32_t dy_dtype, const void* y, void* dx, int32_t dtype, int64_t n, float slope, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(dy && y && dx && n > 0 && n % 8 == 0, "vt_leaky_relu_backward: null pointer or n = %lld not a positive multiple of 8", (long long)n);
  VT_CHECK_ARG(pg_dtype_ok(dtype) && (dy_dtype == dtype || dy_dtype == VT_F32), "vt_leaky_relu_backward: dtype %d (F32 or BF16), dy_dtype %d (dtype or F32)", dtype,
               dy_dtype);
  VT_CHECK_ARG(slope > 0.0f, "vt_leaky_relu_backward: slope %g: the sign of y is the sign of the pre-activation only for a positive slope", (double)slope);
  VT_CHECK_ARG((reinterpret_cast<uintptr_t>(dy) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (reinterpret_cast<uintptr_t>(dx) & 15) == 0,
               "vt_leaky_relu_backward: tensors must be 16-byte aligned");
  const unsigned grid = grid_for(n / 8);
  if (dtype == VT_F32)
    hipLaunchKernelGGL((leaky_bwd_kernel<float, float>), dim3(grid), dim3(kBlock), 0, stream, static_cast<const float*>(dy), static_cast<const float*>(y),
                       static_cast<float*>(dx), slope, n / 8);
  else if (dy_dtype == VT_F32)
    hipLaunchKernelGGL((leaky_bwd_kernel<bf16_t, float>), dim3(grid), dim3(kBlock), 0, stream, static_cast<const float*>(dy), static_cast<const bf16_t*>(y),
                       static_cast<bf16_t*>(dx), slope, n / 8);
  else
    hipLaunchKernelGGL((leaky_bwd_kernel<bf16_t, bf16_t>), dim3(grid), dim3(kBlock), 0, stream, static_cast<const bf16_t*>(dy), static_cast<const bf16_t*>(y),
                       static_cast<bf16_t*>(dx), slope, n / 8);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int vt_pack_conv_weight_dgrad_strided(const float* w, void* out, int32_t out_dtype, int32_t Cout, int32_t Cin, int32_t cout_p, int32_t KT, int32_t KH,
                                                 int32_t KW, int32_t sh, int32_t sw, int32_t ph, int32_t pw, int64_t ldw, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(w && out && Cout > 0 && Cin > 0 && cout_p >= Cout && KT > 0 && KH > 0 && KW > 0 && KT <= 4 && KH <= 4 && KW <= 4, "vt_pack_conv_weight_dgrad_strided: bad arguments");
  VT_CHECK_ARG(pg_dtype_ok(out_dtype), "vt_pack_conv_weight_dgrad_strided: out_dtype %d (fp32 or bf16)", out_dtype);
  VT_CHECK_ARG((sh == 1 || sh == 2) && (sw == 1 || sw == 2) && ph >= 0 && ph < KH && pw >= 0 && pw < KW, "vt_pack_conv_weight_dgrad_strided: strides (%d, %d) in {1, 2}, pads (%d, %d) below the taps",
               sh, sw, ph, pw);
  VT_CHECK_ARG(ldw >= (int64_t)KT * ((KH + sh - 1) / sh) * ((KW + sw - 1) / sw) * cout_p, "vt_pack_conv_weight_dgrad_strided: ldw %lld", (long long)ldw);
  const unsigned grid = grid_for((int64_t)sh * sw * Cin * ldw, 8192);
  if (out_dtype == VT_F32)
    hipLaunchKernelGGL(pack_dgrad_strided_kernel<float>, dim3(grid), dim3(kBlock), 0, stream, w, static_cast<float*>(out), Cout, Cin, cout_p, KT, KH, KW, sh, sw, ph, pw,
                       (long long)ldw);
  else
    hipLaunchKernelGGL(pack_dgrad_strided_kernel<bf16_t>, dim3(grid), dim3(kBlock), 0, stream, w, static_cast<bf16_t*>(out), Cout, Cin, cout_p, KT, KH, KW, sh, sw, ph, pw,
                       (long long)ldw);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int64_t vt_conv_dgrad_strided_work_bytes(const vt_dgrad_desc* d) {
  StridedPlan p;
  if (strided_prepare(d, &p) != VT_OK) return -1;
  return p.bytes;
}

extern "C" int vt_conv_dgrad_strided(const vt_dgrad_desc* d, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  StridedPlan p;
  const int rc = strided_prepare(d, &p);
  if (rc != VT_OK) return rc;
  VT_CHECK_ARG(d->dy && d->wt && d->dx, "vt_conv_dgrad_strided: null tensor pointer");
  VT_CHECK_ARG(p.bytes == 0 || (d->work != nullptr && d->work_bytes >= p.bytes && (reinterpret_cast<uintptr_t>(d->work) & 15) == 0),
               "vt_conv_dgrad_strided: workspace of %lld bytes needed (vt_conv_dgrad_strided_work_bytes)", (long long)p.bytes);
  const int es = d->dtype == VT_BF16 ? 2 : 4;
  FinishArgs f;
  memset(&f, 0, sizeof(f));
  for (int rh = 0; rh < d->sh; ++rh)
    for (int rw = 0; rw < d->sw; ++rw) {
      const int cls = rh * d->sw + rw;
      const AxisClass &h = p.ah[rh], &w = p.aw[rw];
      f.off[cls] = p.off[cls] < 0 ? -1 : p.off[cls] / 4;
      f.nh[cls] = h.n;
      f.nw[cls] = w.n;
      if (p.off[cls] < 0) continue;
      vt_conv_desc c;
      memset(&c, 0, sizeof(c));
      c.x = d->dy;
      c.w = static_cast<const char*>(d->wt) + (int64_t)cls * d->Cin * d->ldw * es;
      c.y = static_cast<char*>(d->work) + p.off[cls];
      c.B = d->B; c.Ti = d->To; c.Hi = d->Ho; c.Wi = d->Wo; c.Cin = d->lddy;
      c.To = d->Ti; c.Ho = h.n; c.Wo = w.n; c.Cout = d->Cin;
      c.ldw = d->ldw; c.ldy = d->lddx;
      c.KT = d->KT; c.KH = h.nk; c.KW = w.nk;
      c.st = c.sh = c.sw = 1;
      c.pt = d->KT - 1 - d->pt; c.ph = h.pad; c.pw = w.pad;
      c.tmode = VT_TPAD_ZERO;
      c.out_layout = VT_NDHWC;
      c.dtype = d->dtype; c.out_dtype = VT_F32;
      c.nbatch = 1;
      const int rc2 = vt_conv(&c, stream_);
      if (rc2 != VT_OK) return rc2;
    }
  f.work = static_cast<const float*>(d->work);
  f.acc = d->acc;
  f.dx = d->dx;
  f.B = d->B; f.T = d->Ti; f.H = d->Hi; f.W = d->Wi; f.C = d->Cin; f.ld = d->lddx; f.lda = d->ldacc; f.sh = d->sh; f.sw = d->sw;
  const unsigned grid = grid_for((int64_t)d->B * d->Ti * d->Hi * d->Wi * (d->lddx / 4));
  if (d->dx_dtype == VT_F32)
    hipLaunchKernelGGL(strided_finish_kernel<float>, dim3(grid), dim3(kBlock), 0, stream, f);
  else
    hipLaunchKernelGGL(strided_finish_kernel<bf16_t>, dim3(grid), dim3(kBlock), 0, stream, f);
  VT_CHECK_LAUNCH();
  return VT_OK;
}
