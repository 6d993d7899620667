// The kernels of the 2-D PatchGAN discriminator (include/vidtok_amd.h, "PatchGAN discriminator"): batch-statistics BatchNorm with
// LeakyReLU forward and backward, and the LeakyReLU backward of the un-normalised first layer.
//
// Rows are NDHWC pixels [M][ld]; a lane owns 8 consecutive channels of a row (row8.h), a workgroup walks a fixed range of rows.  Every
// sum over rows is a per-workgroup partial in the caller's `work`, added in index order by a second launch (fp64 in that launch): no
// atomics, two runs give the same bits, nothing allocates or synchronises.
#include "launch.h"
#include "row8.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxC = 512;              // a lane per 8 channels, up to 64 lanes a row
constexpr int kMaxGroups = 1024;        // per-workgroup partials of one reduction

// rows walked side by side by one workgroup (nq lanes a row), and the workgroups of a reduction over M rows
inline int rows_par(int nq) { return kBlock / nq; }
inline int64_t reduce_groups(int64_t M, int nq) {
  return grid_for(M, rows_par(nq) * 8, kMaxGroups);
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

}  // namespace

extern "C" int64_t vt_batchnorm_stats_work_bytes(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0 || C > kMaxC) return -1;
  return align256(reduce_groups(M, (C + 7) / 8) * 2 * C * 8);
}

extern "C" int vt_batchnorm_stats(const void* x, int32_t dtype, int64_t ld, int64_t M, int32_t C, float eps, float* mean, float* var, float* rstd, void* work,
                                  int64_t work_bytes, vt_stream stream_) {
  hipStream_t stream = as_stream(stream_);
  VT_CHECK_ARG(x && mean && var && work, "vt_batchnorm_stats: null pointer");
  VT_CHECK_ARG(grad_dtype_ok(dtype), "vt_batchnorm_stats: dtype %d (F32 or BF16)", dtype);
  VT_CHECK_ARG(M > 0 && C > 0 && C <= kMaxC && ld % 8 == 0 && ld >= (C + 7) / 8 * 8, "vt_batchnorm_stats: bad dims (M=%lld C=%d ld=%lld; C <= 512, ld a multiple of 8)",
               (long long)M, C, (long long)ld);
  VT_CHECK_ARG(aligned16(x, work), "vt_batchnorm_stats: tensors must be 16-byte aligned");
  const int nq = (C + 7) / 8;
  const int64_t groups = reduce_groups(M, nq);
  VT_CHECK_ARG(work_bytes >= align256(groups * 2 * C * 8), "vt_batchnorm_stats: workspace of %lld bytes, need %lld (vt_batchnorm_stats_work_bytes)",
               (long long)work_bytes, (long long)align256(groups * 2 * C * 8));
  const int64_t rows_per_wg = (M + groups - 1) / groups;
  const size_t lds = (size_t)rows_par(nq) * 2 * nq * 8 * sizeof(double);
  double* part = static_cast<double*>(work);
  const int rc = vt_dispatch<float, bf16_t>(dtype, [&](auto t) {
    using T = vt_t<decltype(t)>;
    return launch(bn_stats_kernel<T>, dim3((unsigned)groups), dim3(kBlock), lds, stream, static_cast<const T*>(x), ld, M, C, nq, rows_per_wg, part);
  });
  if (rc != VT_OK) return rc;
  return launch(bn_stats_finish_kernel, dim3((unsigned)((C + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, part, (int)groups, M, C, eps, mean, var, rstd);
}

extern "C" int vt_batchnorm_act(const void* x, int32_t dtype, int64_t ld, void* y, int64_t ldy, const float* mean, const float* rstd, const float* gamma,
                                const float* beta, float slope, int64_t M, int32_t C, vt_stream stream_) {
  VT_CHECK_ARG(x && y && mean && rstd && gamma && beta, "vt_batchnorm_act: null pointer");
  VT_CHECK_ARG(grad_dtype_ok(dtype), "vt_batchnorm_act: dtype %d (F32 or BF16)", dtype);
  VT_CHECK_ARG(M > 0 && C > 0 && ld % 8 == 0 && ldy % 8 == 0 && ld >= (C + 7) / 8 * 8 && ldy >= C, "vt_batchnorm_act: bad dims (M=%lld C=%d ld=%lld ldy=%lld; strides multiples of 8)",
               (long long)M, C, (long long)ld, (long long)ldy);
  VT_CHECK_ARG(aligned16(x, y), "vt_batchnorm_act: tensors must be 16-byte aligned");
  return vt_dispatch<float, bf16_t>(dtype, [&](auto t) {
    using T = vt_t<decltype(t)>;
    return launch(bn_act_kernel<T>, dim3(grid_for(M * (ldy / 8), kBlock, 16384)), dim3(kBlock), 0, as_stream(stream_), static_cast<const T*>(x), ld, static_cast<T*>(y), ldy,
                  mean, rstd, gamma, beta, slope, M, C);
  });
}

extern "C" int64_t vt_batchnorm_act_backward_work_bytes(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0 || C > kMaxC) return -1;
  return align256(reduce_groups(M, (C + 7) / 8) * 2 * C * 4) + align256(2 * C * 4);
}

extern "C" int vt_batchnorm_act_backward(const void* x, const void* dy, int32_t dtype, int32_t dy_dtype, int64_t ld, int64_t lddy, void* dx, int64_t ldo,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta, float slope, float* dgamma, float* dbeta,
                                         int64_t M, int32_t C, int32_t mode, void* work, int64_t work_bytes, vt_stream stream_) {
  hipStream_t stream = as_stream(stream_);
  VT_CHECK_ARG(x && dy && dx && mean && rstd && gamma && beta && work, "vt_batchnorm_act_backward: null pointer");
  VT_CHECK_ARG(grad_dtype_ok(dtype) && (dy_dtype == dtype || dy_dtype == VT_F32), "vt_batchnorm_act_backward: dtype %d (F32 or BF16), dy_dtype %d (dtype or F32)", dtype,
               dy_dtype);
  VT_CHECK_ARG(mode == VT_BN_BATCH || mode == VT_BN_RUNNING, "vt_batchnorm_act_backward: mode %d (VT_BN_BATCH or VT_BN_RUNNING)", mode);
  const int64_t c8 = (C + 7) / 8 * 8;
  VT_CHECK_ARG(M > 0 && C > 0 && C <= kMaxC && ld % 8 == 0 && lddy % 8 == 0 && ldo % 8 == 0 && ld >= c8 && lddy >= c8 && ldo >= C,
               "vt_batchnorm_act_backward: bad dims (M=%lld C=%d ld=%lld lddy=%lld ldo=%lld; C <= 512, strides multiples of 8)", (long long)M, C, (long long)ld,
               (long long)lddy, (long long)ldo);
  VT_CHECK_ARG(aligned16(x, dy, dx, work), "vt_batchnorm_act_backward: tensors must be 16-byte aligned");
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
  const int batch = mode == VT_BN_BATCH;
  return vt_dispatch_grad(dtype, dy_dtype, [&](auto t, auto td) {
    using T = vt_t<decltype(t)>;
    using TD = vt_t<decltype(td)>;
    if (need_sums) {
      int rc = launch(bn_bwd_sums_kernel<T, TD>, dim3((unsigned)groups), dim3(kBlock), lds, stream, static_cast<const T*>(x), static_cast<const TD*>(dy), ld, lddy, mean,
                      rstd, gamma, beta, slope, M, C, nq, rows_per_wg, part);
      if (rc != VT_OK) return rc;
      rc = launch(bn_bwd_reduce_kernel, dim3((unsigned)((C + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, part, (int)groups, C, sums, dgamma, dbeta);
      if (rc != VT_OK) return rc;
    }
    return launch(bn_bwd_dx_kernel<T, TD>, dim3(grid_for(M * (ldo / 8), kBlock, 16384)), dim3(kBlock), 0, stream, static_cast<const T*>(x), static_cast<const TD*>(dy), ld,
                  lddy, static_cast<T*>(dx), ldo, mean, rstd, gamma, beta, slope, sums, M, C, batch);
  });
}

extern "C" int vt_leaky_relu_backward(const void* dy, int32_t dy_dtype, const void* y, void* dx, int32_t dtype, int64_t n, float slope, vt_stream stream_) {
  VT_CHECK_ARG(dy && y && dx && n > 0 && n % 8 == 0, "vt_leaky_relu_backward: null pointer or n = %lld not a positive multiple of 8", (long long)n);
  VT_CHECK_ARG(grad_dtype_ok(dtype) && (dy_dtype == dtype || dy_dtype == VT_F32), "vt_leaky_relu_backward: dtype %d (F32 or BF16), dy_dtype %d (dtype or F32)", dtype,
               dy_dtype);
  VT_CHECK_ARG(slope > 0.0f, "vt_leaky_relu_backward: slope %g: the sign of y is the sign of the pre-activation only for a positive slope", (double)slope);
  VT_CHECK_ARG(aligned16(dy, y, dx), "vt_leaky_relu_backward: tensors must be 16-byte aligned");
  return vt_dispatch_grad(dtype, dy_dtype, [&](auto t, auto td) {
    using T = vt_t<decltype(t)>;
    using TD = vt_t<decltype(td)>;
    return launch(leaky_bwd_kernel<T, TD>, dim3(grid_for(n / 8, kBlock, 16384)), dim3(kBlock), 0, as_stream(stream_), static_cast<const TD*>(dy), static_cast<const T*>(y),
                  static_cast<T*>(dx), slope, n / 8);
  });
}
