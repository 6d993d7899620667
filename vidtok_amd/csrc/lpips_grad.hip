// Backward of LPIPS with respect to the reconstruction (include/vidtok_amd.h, "differentiable LPIPS"): the memory-bound pieces around
// vt_conv_dgrad.  Only the N reconstruction frames (the second half of the 2N stack) get a gradient.
//   lpips_tap_backward_kernel   adjoint of the head of one tap + routing of the next slice's gradient through the 2 x 2 max-pool + the
//                               ReLU mask of the tap's own convolution: ONE pass over relu_k, one rounding
//   relu_backward_kernel        dx = dy * (y > 0) on 8 channels a lane
//   lpips_prep_backward_kernel  adjoint of the ScalingLayer + layout change: [N][H][W][8] -> fp32 [N][3][H][W]
// No atomics, no cross-workgroup sums: every output element is written once by one lane, the channel sums of a pixel are DPP sums in
// a fixed order, so two runs give the same bits.  Nothing allocates or synchronises.
#include "launch.h"
#include "row8.h"

namespace {

// The layout of lpips_tap_kernel: L = C / 8 lanes share a pixel (8 consecutive channels a lane, 16-byte accesses), a group of L lanes
// takes a 2 x 2 quad of pixels of frame n (f0, the input) and frame n + N (f1, the reconstruction).  Per pixel, in fp32:
//   s_i = |f_i|, u_i = f_i / (s_i + 1e-10)                                    (the forward's true divisions)
//   e_c = 2 gout[n] w_c (u1_c - u0_c) / (H W)
//   g_c = e_c / (s1 + eps) - f1_c (sum_j e_j f1_j) / (s1 (s1 + eps)^2)        (second term 0 at s1 = 0)
// then dpool of the quad's window is added at the FIRST maximum of f1 over (0,0), (0,1), (1,0), (1,1) per channel, and the sum is
// masked by f1 > 0.  Odd last rows / columns belong to no window: head term only.
template <typename T, typename TP, int C>
__global__ __launch_bounds__(256) void lpips_tap_backward_kernel(const T* __restrict__ feat, const float* __restrict__ lin_w,
                                                                 const float* __restrict__ gout, const TP* __restrict__ dpool,
                                                                 T* __restrict__ dfeat, int N, int H, int W) {
  constexpr int L = C / 8;
  constexpr int G = 256 / L;
  const int tid = threadIdx.x, g = tid / L, j = tid % L;
  const int n = blockIdx.y;
  const int QW = (W + 1) >> 1, nq = ((H + 1) >> 1) * QW;
  const int Hp = H >> 1, Wp = W >> 1;
  const long long HW = (long long)H * W;
  const T* f0 = feat + (long long)n * HW * C + 8 * j;
  const T* f1 = feat + (long long)(n + N) * HW * C + 8 * j;
  T* out = dfeat + (long long)n * HW * C + 8 * j;
  float w8[8];
  {
    const f32x4 a = *reinterpret_cast<const f32x4*>(lin_w + 8 * j), b = *reinterpret_cast<const f32x4*>(lin_w + 8 * j + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { w8[e] = a[e]; w8[4 + e] = b[e]; }
  }
  const float k = 2.0f * gout[n] / (float)HW;
  for (int q = blockIdx.x * G + g; q < nq; q += gridDim.x * G) {      // uniform over the L lanes of a group (groups are aligned inside a wave)
    const int qy = q / QW, qx = q - qy * QW;
    float a[4][8], b[4][8];
    bool ok[4];
    long long off[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int yy = 2 * qy + (p >> 1), xx = 2 * qx + (p & 1);
      ok[p] = yy < H && xx < W;
      off[p] = ok[p] ? ((long long)yy * W + xx) * C : 0;              // odd edges: a valid address, the pixel is not written below
      Row8<T>::load(f0 + off[p], a[p]);
      Row8<T>::load(f1 + off[p], b[p]);
    }
    const bool window = dpool != nullptr && qy < Hp && qx < Wp;
    float dp[8];
    if (window) {
      Row8<TP>::load(dpool + (((long long)n * Hp + qy) * Wp + qx) * C + 8 * j, dp);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) dp[e] = 0.0f;
    }
    float sa[4], sb[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      sa[p] = a[p][0] * a[p][0];
      sb[p] = b[p][0] * b[p][0];
#pragma unroll
      for (int e = 1; e < 8; ++e) {
        sa[p] = __builtin_fmaf(a[p][e], a[p][e], sa[p]);
        sb[p] = __builtin_fmaf(b[p][e], b[p][e], sb[p]);
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      sa[p] = group_sum_dpp<L>(sa[p]);
      sb[p] = group_sum_dpp<L>(sb[p]);
    }
    float ev[4][8], dot[4], s1[4], n1[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float na = sqrtf(sa[p]) + 1e-10f;
      s1[p] = sqrtf(sb[p]);
      n1[p] = s1[p] + 1e-10f;
      float d = 0.0f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        ev[p][e] = k * w8[e] * (b[p][e] / n1[p] - a[p][e] / na);
        d = __builtin_fmaf(ev[p][e], b[p][e], d);
      }
      dot[p] = d;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) dot[p] = group_sum_dpp<L>(dot[p]);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float r = s1[p] > 0.0f ? dot[p] / (s1[p] * (n1[p] * n1[p])) : 0.0f;
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float gr = ev[p][e] / n1[p] - b[p][e] * r;
        // the first maximum of the window in row-major order takes the pooled gradient (F.max_pool2d's backward)
        const float m = fmaxf(fmaxf(b[0][e], b[1][e]), fmaxf(b[2][e], b[3][e]));
        const int first = b[0][e] == m ? 0 : (b[1][e] == m ? 1 : (b[2][e] == m ? 2 : 3));
        if (first == p) gr += dp[e];
        o[e] = b[p][e] > 0.0f ? gr : 0.0f;
      }
      if (ok[p]) Row8<T>::store(out + off[p], o);
    }
  }
}

template <typename TS, typename T>
__global__ __launch_bounds__(256) void relu_backward_kernel(const TS* __restrict__ dy, const T* __restrict__ y, T* __restrict__ dx, long long n8) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    float d[8], v[8], o[8];
    Row8<TS>::load(dy + i * 8, d);
    Row8<T>::load(y + i * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = v[e] > 0.0f ? d[e] : 0.0f;
    Row8<T>::store(dx + i * 8, o);
  }
}

// one thread = one pixel of one frame: a 16- / 32-byte row in, three coalesced planar stores out
template <typename TS>
__global__ __launch_bounds__(256) void lpips_prep_backward_kernel(const TS* __restrict__ d, const float* __restrict__ scale, float* __restrict__ out,
                                                                  int N, long long HW) {
#pragma clang fp contract(off)
  const long long total = (long long)N * HW;
  const float sc[3] = {scale[0], scale[1], scale[2]};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / HW, pix = i - n * HW;
    float v[8];
    Row8<TS>::load(d + i * 8, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(n * 3 + c) * HW + pix] = v[c] / sc[c];
  }
}

template <typename T, typename TP>
int launch_tap_backward(const void* feat, const float* lin_w, const float* gout, const void* dpool, void* dfeat, int N, int H, int W, int C,
                        hipStream_t s) {
  const int nq = ((H + 1) / 2) * ((W + 1) / 2);
  const dim3 grid(grid_for(nq, 256 / (C / 8), 2048), N);
  return vt_dispatch_int<64, 128, 256, 512>(C, [&](auto c) {
    return launch(lpips_tap_backward_kernel<T, TP, decltype(c)::value>, grid, dim3(256), 0, s, reinterpret_cast<const T*>(feat), lin_w, gout,
                  reinterpret_cast<const TP*>(dpool), reinterpret_cast<T*>(dfeat), N, H, W);
  });
}

}  // namespace

extern "C" int vt_lpips_tap_backward(const void* feat, const float* lin_w, const float* gout, const void* dpool, int32_t dpool_dtype, void* dfeat,
                                     int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, vt_stream stream) {
  VT_CHECK_ARG(grad_dtype_ok(dtype), "vt_lpips_tap_backward: dtype %d (VT_F32 or VT_BF16: the backward kernels take fp32 or bf16)", dtype);
  VT_CHECK_ARG(C == 64 || C == 128 || C == 256 || C == 512, "vt_lpips_tap_backward: C=%d (64, 128, 256 or 512)", C);
  VT_CHECK_ARG(feat && lin_w && gout && dfeat, "vt_lpips_tap_backward: null pointer");
  VT_CHECK_ARG(dpool == nullptr || dpool_dtype == dtype || dpool_dtype == VT_F32, "vt_lpips_tap_backward: dpool_dtype %d (dtype or VT_F32)", dpool_dtype);
  VT_CHECK_ARG(aligned16(feat, lin_w, dfeat, dpool),
               "vt_lpips_tap_backward: feat, lin_w, dpool and dfeat must be 16-byte aligned");
  VT_CHECK_ARG(N > 0 && H > 0 && W > 0 && N <= 65535 && (long long)H * W < (1ll << 30), "vt_lpips_tap_backward: N=%d H=%d W=%d", N, H, W);
  return vt_dispatch_grad(dtype, dpool != nullptr ? dpool_dtype : dtype, [&](auto t, auto tp) {
    return launch_tap_backward<vt_t<decltype(t)>, vt_t<decltype(tp)>>(feat, lin_w, gout, dpool, dfeat, N, H, W, C, as_stream(stream));
  });
}

extern "C" int vt_relu_backward(const void* dy, int32_t dy_dtype, const void* y, void* dx, int32_t dtype, int64_t n, vt_stream stream) {
  VT_CHECK_ARG(grad_dtype_ok(dtype) && (dy_dtype == dtype || dy_dtype == VT_F32), "vt_relu_backward: dy_dtype %d, dtype %d (fp32 or bf16; dy in dtype or fp32)",
               dy_dtype, dtype);
  VT_CHECK_ARG(dy && y && dx && n > 0 && n % 8 == 0, "vt_relu_backward: null pointer or n=%lld (a positive multiple of 8)", (long long)n);
  VT_CHECK_ARG(aligned16(dy, y, dx), "vt_relu_backward: dy, y and dx must be 16-byte aligned");
  const long long n8 = n / 8;
  return vt_dispatch_grad(dtype, dy_dtype, [&](auto t, auto ts) {
    using T = vt_t<decltype(t)>;
    using TS = vt_t<decltype(ts)>;
    return launch(relu_backward_kernel<TS, T>, dim3(grid_for(n8, 256, 16384)), dim3(256), 0, as_stream(stream), static_cast<const TS*>(dy), static_cast<const T*>(y),
                  static_cast<T*>(dx), n8);
  });
}

extern "C" int vt_lpips_prep_backward(const void* d, int32_t dtype, const float* scale, float* dtarget, int32_t N, int32_t H, int32_t W, vt_stream stream) {
  VT_CHECK_ARG(grad_dtype_ok(dtype), "vt_lpips_prep_backward: dtype %d (VT_F32 or VT_BF16)", dtype);
  VT_CHECK_ARG(d && scale && dtarget, "vt_lpips_prep_backward: null pointer");
  VT_CHECK_ARG(aligned16(d), "vt_lpips_prep_backward: d must be 16-byte aligned");
  VT_CHECK_ARG(N > 0 && H > 0 && W > 0, "vt_lpips_prep_backward: N=%d H=%d W=%d", N, H, W);
  const long long HW = (long long)H * W;
  return vt_dispatch<float, bf16_t>(dtype, [&](auto t) {
    using TS = vt_t<decltype(t)>;
    return launch(lpips_prep_backward_kernel<TS>, dim3(grid_for((long long)N * HW, 256, 16384)), dim3(256), 0, as_stream(stream), static_cast<const TS*>(d), scale, dtarget,
                  N, HW);
  });
}
