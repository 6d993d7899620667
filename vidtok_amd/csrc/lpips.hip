// LPIPS on VGG16 features (include/vidtok_amd.h, vt_lpips_*): the memory-bound pieces around the convolutions (vt_conv_act).
//   lpips_prep_kernel    the eval loop's post-processing + ScalingLayer, NCTHW fp32 pair -> one NHWC stack of 2N frames (8 channels)
//   lpips_tap_kernel     the head of one tap, fused with the 2 x 2 max-pool that feeds the next VGG slice: ONE pass over relu_k
//   lpips_finish_kernel  the spatial means and their sum over the taps, fixed order
// Deterministic by construction: the pixels of a (tap, pair) are cut into a fixed number of ranges that depends on the shape only,
// every range is summed in a fixed order by one workgroup into its own workspace slot, and the finish adds the slots in order.
#include "launch.h"
#include "row8.h"

namespace {

constexpr int kTaps = 5;
constexpr int kSlots = 64;                  // workspace floats per (tap, pair): at most this many pixel ranges
constexpr int kQuadsPerSlot = 32;           // ... of at least this many 2 x 2 quads each

// workgroups (= pixel ranges) of a tap over an H x W feature map: a function of the shape alone
inline int tap_slots(int H, int W) {
  const long long nq = (long long)((H + 1) / 2) * ((W + 1) / 2);
  return (int)std::min<long long>((nq + kQuadsPerSlot - 1) / kQuadsPerSlot, kSlots);
}

// one thread = one pixel of one of the 2N output frames; the three input channels are strided by T*H*W in NCTHW
template <typename T>
__global__ __launch_bounds__(256) void lpips_prep_kernel(const float* __restrict__ x, const float* __restrict__ y, T* __restrict__ out,
                                                         const float* __restrict__ shift, const float* __restrict__ scale, int N, int Tn,
                                                         long long HW, int flags) {
#pragma clang fp contract(off)
  const long long total = 2ll * N * HW;
  const float sh[3] = {shift[0], shift[1], shift[2]}, sc[3] = {scale[0], scale[1], scale[2]};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long f = i / HW, pix = i - f * HW;
    const bool second = f >= N;
    const int n = (int)(second ? f - N : f);
    const int b = n / Tn, t = n - b * Tn;
    const float* src = second ? y : x;
    const long long cs = (long long)Tn * HW;
    const long long base = (long long)b * 3 * cs + (long long)t * HW + pix;
    float o[8];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = src[base + c * cs];
      if (second && (flags & VT_LPIPS_CLAMP_Y)) v = fminf(fmaxf(v, -1.0f), 1.0f);
      if (flags & VT_LPIPS_ROUNDTRIP) {
        const float u = (v + 1.0f) / 2.0f;
        v = u * 2.0f - 1.0f;
      }
      if (flags & VT_LPIPS_UNIT) v = v * 2.0f - 1.0f;
      o[c] = (v - sh[c]) / sc[c];
    }
#pragma unroll
    for (int c = 3; c < 8; ++c) o[c] = 0.0f;
    Row8<T>::store(out + i * 8, o);
  }
}

// The head of one tap.  L = C / 8 lanes share a pixel (8 consecutive channels a lane, 16-byte loads), a group of L lanes takes a
// 2 x 2 quad of pixels of frame n and frame n + N: 8 row loads a lane, issued together, then
//   both channel norms of the four pixels (DPP sums over the L lanes), the normalised squared difference weighted by lin_w,
//   its channel sum (one DPP sum of the four pixels' partials), and
//   the 2 x 2 max of both frames' quads -- the pooled rows written straight from the registers (no second read of relu_k).
// A workgroup walks its fixed range of quads (G in flight); the group sums meet in the LDS and are added in group order.
template <typename T, int C>
__global__ __launch_bounds__(256) void lpips_tap_kernel(const T* __restrict__ feat, T* __restrict__ pooled, const float* __restrict__ lin_w,
                                                        float* __restrict__ part, int N, int H, int W, int chunk) {
  constexpr int L = C / 8;
  constexpr int G = 256 / L;
  __shared__ float red[G];
  const int tid = threadIdx.x, g = tid / L, j = tid % L;
  const int n = blockIdx.y;
  const int QW = (W + 1) >> 1, nq = ((H + 1) >> 1) * QW;
  const int Hp = H >> 1, Wp = W >> 1;
  const long long HW = (long long)H * W;
  const T* f0 = feat + (long long)n * HW * C + 8 * j;
  const T* f1 = feat + (long long)(n + N) * HW * C + 8 * j;
  float w8[8];
  {
    const f32x4 a = *reinterpret_cast<const f32x4*>(lin_w + 8 * j), b = *reinterpret_cast<const f32x4*>(lin_w + 8 * j + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { w8[e] = a[e]; w8[4 + e] = b[e]; }
  }
  const int q0 = blockIdx.x * chunk, q1 = min(q0 + chunk, nq);
  float acc = 0.0f;
  for (int q = q0 + g; q < q1; q += G) {          // uniform over the L lanes of a group (groups are aligned inside a wave)
    const int qy = q / QW, qx = q - qy * QW;
    float a[4][8], b[4][8];
    bool ok[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int yy = 2 * qy + (p >> 1), xx = 2 * qx + (p & 1);
      ok[p] = yy < H && xx < W;
      const long long off = ok[p] ? ((long long)yy * W + xx) * C : 0;    // odd edges: a valid address, the pixel is left out below
      Row8<T>::load(f0 + off, a[p]);
      Row8<T>::load(f1 + off, b[p]);
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
    float v = 0.0f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float na = sqrtf(sa[p]) + 1e-10f, nb = sqrtf(sb[p]) + 1e-10f;
      float s = 0.0f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = a[p][e] / na - b[p][e] / nb;      // true divisions, as normalize_tensor's x / (norm + eps)
        s = __builtin_fmaf(w8[e], d * d, s);
      }
      if (ok[p]) v += s;
    }
    v = group_sum_dpp<L>(v);
    acc += v;
    if (pooled != nullptr && qy < Hp && qx < Wp) {
      float m0[8], m1[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        m0[e] = fmaxf(fmaxf(a[0][e], a[1][e]), fmaxf(a[2][e], a[3][e]));
        m1[e] = fmaxf(fmaxf(b[0][e], b[1][e]), fmaxf(b[2][e], b[3][e]));
      }
      const long long po = ((long long)qy * Wp + qx) * C + 8 * j;
      const long long HWp = (long long)Hp * Wp * C;
      Row8<T>::store(pooled + (long long)n * HWp + po, m0);
      Row8<T>::store(pooled + (long long)(n + N) * HWp + po, m1);
    }
  }
  if (j == 0) red[g] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = red[0];
    for (int i = 1; i < G; ++i) s += red[i];
    part[(long long)n * kSlots + blockIdx.x] = s;
  }
}

struct FinishGeom {
  int slots[kTaps];
  float hw[kTaps];
};

__global__ __launch_bounds__(256) void lpips_finish_kernel(const float* __restrict__ part, float* __restrict__ out, float* __restrict__ taps,
                                                           int N, FinishGeom geo) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float val = 0.0f;
#pragma unroll
  for (int k = 0; k < kTaps; ++k) {
    const float* p = part + ((long long)k * N + n) * kSlots;
    float s = p[0];
    for (int i = 1; i < geo.slots[k]; ++i) s += p[i];
    const float m = s / geo.hw[k];
    if (taps) taps[(long long)k * N + n] = m;
    val = k == 0 ? m : val + m;
  }
  out[n] = val;
}

template <typename T>
int launch_tap(const void* feat, void* pooled, const float* lin_w, float* part, int N, int H, int W, int C, hipStream_t s) {
  const int slots = tap_slots(H, W);
  const int nq = ((H + 1) / 2) * ((W + 1) / 2);
  const int chunk = (nq + slots - 1) / slots;
  return vt_dispatch_int<64, 128, 256, 512>(C, [&](auto c) {
    return launch(lpips_tap_kernel<T, decltype(c)::value>, dim3(slots, N), dim3(256), 0, s, reinterpret_cast<const T*>(feat), reinterpret_cast<T*>(pooled), lin_w, part,
                  N, H, W, chunk);
  });
}

}  // namespace

extern "C" int64_t vt_lpips_work_bytes(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || H < 16 || W < 16) return 0;
  return (int64_t)kTaps * N * kSlots * (int64_t)sizeof(float);
}

extern "C" int vt_lpips_prep(const float* x, const float* y, void* out, const float* shift, const float* scale, int32_t dtype, int32_t B,
                             int32_t T, int32_t H, int32_t W, int32_t flags, vt_stream stream) {
  VT_CHECK_ARG(dtype == VT_F32 || dtype == VT_BF16 || dtype == VT_F16, "vt_lpips_prep: dtype %d (VT_F32, VT_BF16 or VT_F16)", dtype);
  VT_CHECK_ARG(x && y && out && shift && scale, "vt_lpips_prep: null pointer");
  VT_CHECK_ARG(aligned16(out), "vt_lpips_prep: out must be 16-byte aligned");
  VT_CHECK_ARG(B > 0 && T > 0, "vt_lpips_prep: B=%d T=%d", B, T);
  VT_CHECK_ARG(H >= 16 && W >= 16, "vt_lpips_prep: %d x %d input: LPIPS needs H, W >= 16 (relu5_3 is H/16 x W/16)", H, W);
  VT_CHECK_ARG((flags & ~(VT_LPIPS_CLAMP_Y | VT_LPIPS_ROUNDTRIP | VT_LPIPS_UNIT)) == 0, "vt_lpips_prep: flags %d", flags);
  const int N = B * T;
  const long long HW = (long long)H * W;
  const long long total = 2ll * N * HW;
  return vt_dispatch<float, bf16_t, f16_t>(dtype, [&](auto t) {
    using TO = vt_t<decltype(t)>;
    return launch(lpips_prep_kernel<TO>, dim3(grid_for(total, 256, 65536)), dim3(256), 0, as_stream(stream), x, y, reinterpret_cast<TO*>(out), shift, scale, N, T, HW, flags);
  });
}

extern "C" int vt_lpips_tap(const void* feat, void* pooled, const float* lin_w, void* work, int64_t work_bytes, int32_t dtype, int32_t N,
                            int32_t H, int32_t W, int32_t C, int32_t tap, vt_stream stream) {
  VT_CHECK_ARG(dtype == VT_F32 || dtype == VT_BF16 || dtype == VT_F16, "vt_lpips_tap: dtype %d (VT_F32, VT_BF16 or VT_F16)", dtype);
  VT_CHECK_ARG(C == 64 || C == 128 || C == 256 || C == 512, "vt_lpips_tap: C=%d (64, 128, 256 or 512)", C);
  VT_CHECK_ARG(feat && lin_w && work, "vt_lpips_tap: null pointer");
  VT_CHECK_ARG(aligned16(feat, lin_w, work, pooled),
               "vt_lpips_tap: feat, pooled, lin_w and work must be 16-byte aligned");
  VT_CHECK_ARG(tap >= 0 && tap < kTaps, "vt_lpips_tap: tap %d (0..4)", tap);
  VT_CHECK_ARG(N > 0 && H > 0 && W > 0 && N <= 65535, "vt_lpips_tap: N=%d H=%d W=%d", N, H, W);
  VT_CHECK_ARG(work_bytes >= (int64_t)kTaps * N * kSlots * (int64_t)sizeof(float), "vt_lpips_tap: workspace %lld B < %lld B",
               (long long)work_bytes, (long long)kTaps * N * kSlots * (long long)sizeof(float));
  float* part = reinterpret_cast<float*>(work) + (long long)tap * N * kSlots;
  return vt_dispatch<float, bf16_t, f16_t>(dtype, [&](auto t) {
    return launch_tap<vt_t<decltype(t)>>(feat, pooled, lin_w, part, N, H, W, C, as_stream(stream));
  });
}

extern "C" int vt_lpips_finish(const void* work, int64_t work_bytes, float* lpips, float* tap_means, int32_t N, int32_t H, int32_t W,
                               vt_stream stream) {
  VT_CHECK_ARG(work && lpips, "vt_lpips_finish: null pointer");
  VT_CHECK_ARG(N > 0 && N <= (1 << 24), "vt_lpips_finish: N=%d", N);
  VT_CHECK_ARG(H >= 16 && W >= 16, "vt_lpips_finish: %d x %d input: LPIPS needs H, W >= 16 (relu5_3 is H/16 x W/16)", H, W);
  VT_CHECK_ARG(work_bytes >= vt_lpips_work_bytes(N, H, W), "vt_lpips_finish: workspace %lld B < %lld B", (long long)work_bytes,
               (long long)vt_lpips_work_bytes(N, H, W));
  FinishGeom geo;
  int h = H, w = W;
  for (int k = 0; k < kTaps; ++k) {             // relu1_2 at H x W, then a floor-halving max-pool in front of every further slice
    geo.slots[k] = tap_slots(h, w);
    geo.hw[k] = (float)((long long)h * w);
    h >>= 1;
    w >>= 1;
  }
  return launch(lpips_finish_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), reinterpret_cast<const float*>(work), lpips, tap_means, N, geo);
}
