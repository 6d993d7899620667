// Data-gradient path of the decoder backward (include/vidtok_amd.h, "differentiable decode").
//
// vt_conv_dgrad: the gradient of a stride-1 vt_conv with respect to its stored input.  The MACs run on the FORWARD implicit-GEMM
// tiles: dx is itself a convolution of dy with the tap-flipped, Cin/Cout-transposed weight (vt_pack_conv_weight_dgrad) and mirrored
// pads, so vt_conv does the work at forward rates.  What a plain convolution cannot express is finished by grad_fold_kernel: the
// KT - 1 virtual front frames of a replicate time pad add into frame 0, and the 2 / 2 x 2 positions of a folded nearest x2
// up-sampling add into their source pixel -- fp32 sums in a fixed order, rounded once.
//
// The rest are the small kernels a decoder backward needs around the convolutions and LayerNorms: softmax backward, a batched
// transpose (the attention GEMMs want K-contiguous operands), the alpha-mix of the time up-samplers forward and backward (with the
// mix_factor gradient as fixed-order partials + a second launch), the adjoint of the x2 time interpolation, the cotangent's layout
// change and a gradient add.  No float atomics anywhere: every result is bit-reproducible and every call is capture-safe.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kBlock = 256;

inline unsigned grid_for(long long n, int per_block = kBlock, long long cap = 16384) {
  return (unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, cap));
}

// ---- transposed, tap-flipped weight pack ------------------------------------------------------------------------------------
// out[ci][k], k = ((a' KH + p') KW + q') cout_p + co  <-  w[co][ci][KT-1-a'][KH-1-p'][KW-1-q'];  co >= Cout and k past the taps: 0
template <typename TO>
__global__ __launch_bounds__(kBlock) void pack_dgrad_kernel(const float* __restrict__ w, TO* __restrict__ out, int Cout, int Cin, int cout_p,
                                                            int KT, int KH, int KW, long long ldw) {
  const int taps = KT * KH * KW;
  const long long n = (long long)Cin * ldw;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const long long ci = i / ldw;
    const int k = (int)(i - ci * ldw);
    const int j = k / cout_p, co = k - j * cout_p;
    float v = 0.0f;
    if (j < taps && co < Cout) v = w[((long long)co * Cin + ci) * taps + (taps - 1 - j)];     // flipping all three axes = reversing the row-major tap index
    out[i] = from_f32<TO>(v);
  }
}

// ---- fold: virtual front frames and up-sampled positions into their source pixel (+ acc), one rounding -------------------------
struct FoldArgs {
  const void* src;      // [B][rep + (T << ups_t)][H << ups_s][W << ups_s][lds], fp32 or the output type
  const void* acc;      // [B][T][H][W][lda] in the output type, or null
  void* dx;             // [B][T][H][W][ldo]
  int B, T, H, W, C, lds, lda, ldo, rep, ups_t, ups_s;
};

template <typename TS, typename TO>
__global__ __launch_bounds__(kBlock) void grad_fold_kernel(const FoldArgs a) {
  const TS* __restrict__ src = static_cast<const TS*>(a.src);
  const TO* __restrict__ acc = static_cast<const TO*>(a.acc);
  TO* __restrict__ dx = static_cast<TO*>(a.dx);
  const int q = a.ldo / 4;                       // quads per output pixel
  const long long n = (long long)a.B * a.T * a.H * a.W * q;
  const int ft = 1 << a.ups_t, fs = 1 << a.ups_s;
  const int Tv = a.rep + a.T * ft, Hv = a.H * fs, Wv = a.W * fs;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const int c0 = (int)(i % q) * 4;
    long long r = i / q;
    const int w = (int)(r % a.W);
    r /= a.W;
    const int h = (int)(r % a.H);
    r /= a.H;
    const int t = (int)(r % a.T);
    const int b = (int)(r / a.T);
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (c0 < a.C) {
      // frames of the virtual tensor that read this source frame, in ascending order: the replicate pad frames belong to frame 0
      const int tv0 = t == 0 ? 0 : a.rep + t * ft, tv1 = a.rep + (t + 1) * ft;
      for (int tv = tv0; tv < tv1; ++tv)
        for (int dh = 0; dh < fs; ++dh)
          for (int dw = 0; dw < fs; ++dw) {
            const TS* p = src + ((((long long)b * Tv + tv) * Hv + (h * fs + dh)) * Wv + (w * fs + dw)) * a.lds + c0;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (c0 + e < a.C) s[e] += to_f32<TS>(p[e]);
          }
      if (acc) {
        const TO* p = acc + ((((long long)b * a.T + t) * a.H + h) * a.W + w) * a.lda + c0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c0 + e < a.C) s[e] += to_f32<TO>(p[e]);
      }
    }
    TO* o = dx + ((((long long)b * a.T + t) * a.H + h) * a.W + w) * a.ldo + c0;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = from_f32<TO>(c0 + e < a.C ? s[e] : 0.f);
  }
}

// ---- softmax backward: dS = scale * P * (dP - rowsum(dP * P)), one wave per row, fp32 --------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void softmax_rows_backward_kernel(const T* __restrict__ p, long long ldp, const float* __restrict__ dp,
                                                                       T* __restrict__ ds, long long ldo, long long rows, int cols, float scale) {
  const int lane = threadIdx.x & 63;
  const long long wave0 = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const long long nwaves = (long long)gridDim.x * (kBlock / 64);
  for (long long r = wave0; r < rows; r += nwaves) {
    const T* pr = p + r * ldp;
    const float* dr = dp + r * (long long)cols;
    float dot = 0.f;
    for (int c = lane; c < cols; c += 64) dot += dr[c] * to_f32<T>(pr[c]);
    dot = wave_sum(dot, 64);
    T* o = ds + r * ldo;
    for (int c = lane; c < ldo; c += 64) o[c] = from_f32<T>(c < cols ? scale * (to_f32<T>(pr[c]) * (dr[c] - dot)) : 0.f);
  }
}

// ---- batched transpose: out[z][c][r] = in[z][r][c] (r < R, c < C), columns R..ldo-1 of out zero ------------------------------------
template <typename E>
__global__ __launch_bounds__(kBlock) void transpose_kernel(const E* __restrict__ in, E* __restrict__ out, int R, int C, long long ldi, long long ldo) {
  __shared__ E tile[32][33];
  const int z = blockIdx.z, r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
  const E* src = in + (long long)z * R * ldi;
  E* dst = out + (long long)z * C * ldo;
  for (int j = ty; j < 32; j += 8) {
    const int r = r0 + j, c = c0 + tx;
    tile[j][tx] = (r < R && c < C) ? src[(long long)r * ldi + c] : E(0);
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, r = r0 + tx;
    if (c < C && r < ldo) dst[(long long)c * ldo + r] = tile[tx][j];     // r >= R: the tile holds zeros there
  }
}

// ---- alpha-mix of the time up-samplers: y = a u + (1 - a) c, a = sigmoid(mix_factor) ---------------------------------------------
__device__ __forceinline__ float sigmoid_f32(float v) { return 1.0f / (1.0f + __expf(-v)); }

template <typename T>
__global__ __launch_bounds__(kBlock) void mix_forward_kernel(const T* __restrict__ u, const T* __restrict__ c, const float* __restrict__ mf,
                                                             T* __restrict__ y, long long M, int C, int ld) {
  const float a = sigmoid_f32(mf[0]), na = 1.0f - a;
  const long long n = M * ld;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const int ch = (int)(i % ld);
    y[i] = from_f32<T>(ch < C ? a * to_f32<T>(u[i]) + na * to_f32<T>(c[i]) : 0.f);
  }
}

// d_u = a dy, d_c = (1 - a) dy, partial[block] = sum over the block's elements of dy (u - c): the elements are dealt to the threads
// by index, a thread adds its own in index order, the block adds its threads through a fixed LDS tree
template <typename T>
__global__ __launch_bounds__(kBlock) void mix_backward_kernel(const T* __restrict__ dy, const T* __restrict__ u, const T* __restrict__ c,
                                                              const float* __restrict__ mf, T* __restrict__ du, T* __restrict__ dc,
                                                              float* __restrict__ partial, long long M, int C, int ld) {
  __shared__ float red[kBlock];
  const float a = sigmoid_f32(mf[0]), na = 1.0f - a;
  const long long n = M * ld;
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const int ch = (int)(i % ld);
    float g = 0.f;
    if (ch < C) {
      g = to_f32<T>(dy[i]);
      s += g * (to_f32<T>(u[i]) - to_f32<T>(c[i]));
    }
    du[i] = from_f32<T>(a * g);
    dc[i] = from_f32<T>(na * g);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// d_mix_factor = a (1 - a) * (partials added in index order by one thread)
__global__ void mix_finish_kernel(const float* __restrict__ partial, int n, const float* __restrict__ mf, float* __restrict__ dmf) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += partial[i];
  const float a = sigmoid_f32(mf[0]);
  dmf[0] = a * (1.0f - a) * s;
}

inline int mix_blocks(long long n) { return (int)grid_for(n, kBlock * 8, 1024); }

// ---- adjoint of vt_time_lerp2x: dx[i] = sum over the output frames j that read frame i of their weight * dy[j] -------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void time_lerp2x_backward_kernel(const T* __restrict__ dy, T* __restrict__ dx, int B, int Ti, long long F) {
  const int r = blockIdx.y;            // source frame (b, i)
  const int b = r / Ti, i = r - b * Ti;
  // output frames 2i-1 .. 2i+2 can read frame i (align_corners=False, scale 1/2, clamped at both ends); same arithmetic as the forward
  float wgt[4];
  int jj[4];
  for (int k = 0; k < 4; ++k) {
    const int j = 2 * i - 1 + k;
    float w = 0.f;
    if (j >= 0 && j < 2 * Ti) {
      float src = ((float)j + 0.5f) * 0.5f - 0.5f;
      if (src < 0.f) src = 0.f;
      const int t0 = (int)src;
      const int t1 = t0 + (t0 < Ti - 1 ? 1 : 0);
      const float l1 = src - (float)t0, l0 = 1.0f - l1;
      if (t0 == i) w += l0;
      if (t1 == i) w += l1;
    }
    wgt[k] = w;
    jj[k] = j >= 0 && j < 2 * Ti ? j : 0;
  }
  const T* base = dy + (long long)b * 2 * Ti * F;
  T* o = dx + (long long)r * F;
  for (long long f = (long long)blockIdx.x * kBlock + threadIdx.x; f < F; f += (long long)gridDim.x * kBlock) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (wgt[k] != 0.f) s += wgt[k] * to_f32<T>(base[(long long)jj[k] * F + f]);
    o[f] = from_f32<T>(s);
  }
}

// ---- cotangent NCTHW fp32 -> NDHWC, `tpad` zero frames in front (the frames the v1.0 decoder trims), pad lanes zero ----------------
template <typename TO>
__global__ __launch_bounds__(kBlock) void grad_ncthw_to_ndhwc_kernel(const float* __restrict__ x, TO* __restrict__ y, int B, int C, int T, int H, int W,
                                                                     int ldy, int tpad) {
  const long long HW = (long long)H * W;
  const long long npix = (long long)B * (T + tpad) * HW;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < npix; i += (long long)gridDim.x * kBlock) {
    const long long hw = i % HW;
    const long long r = i / HW;
    const int tp = (int)(r % (T + tpad));
    const int b = (int)(r / (T + tpad));
    TO* yp = y + i * ldy;
    for (int c = 0; c < ldy; ++c) {
      float v = 0.f;
      if (c < C && tp >= tpad) v = x[(((long long)b * C + c) * T + (tp - tpad)) * HW + hw];
      yp[c] = from_f32<TO>(v);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void grad_add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ o, long long n) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
    o[i] = from_f32<T>(to_f32<T>(a[i]) + to_f32<T>(b[i]));
}

inline bool grad_dtype_ok(int dt) { return dt == VT_F32 || dt == VT_BF16; }

// checks of a vt_dgrad_desc; fills the geometry of the convolution over dy.  rep = virtual front frames kept for the fold
int dgrad_prepare(const vt_dgrad_desc* d, int* rep, bool* folded) {
  VT_CHECK_ARG(d != nullptr, "vt_conv_dgrad: null descriptor");
  VT_CHECK_ARG(grad_dtype_ok(d->dtype) && (d->dx_dtype == d->dtype || d->dx_dtype == VT_F32), "vt_conv_dgrad: dtype %d -> dx_dtype %d (fp32 or bf16 operands; dx in the operand type or fp32)",
               d->dtype, d->dx_dtype);
  VT_CHECK_ARG(d->st == 1 && d->sh == 1 && d->sw == 1,
               "vt_conv_dgrad: strides (%d, %d, %d): only stride-1 convolutions have a data gradient here (the decoder has no strided one)", d->st, d->sh, d->sw);
  VT_CHECK_ARG(d->B > 0 && d->Ti > 0 && d->Hi > 0 && d->Wi > 0 && d->Cin > 0 && d->Cout > 0 && d->To > 0 && d->Ho > 0 && d->Wo > 0, "vt_conv_dgrad: bad dims");
  VT_CHECK_ARG(d->KT > 0 && d->KH > 0 && d->KW > 0 && d->KT * d->KH * d->KW <= 64, "vt_conv_dgrad: bad taps");
  VT_CHECK_ARG((d->ups_t | d->ups_s | 1) == 1, "vt_conv_dgrad: ups_t / ups_s are 0 or 1");
  VT_CHECK_ARG(d->tmode == VT_TPAD_ZERO || d->tmode == VT_TPAD_REPLICATE, "vt_conv_dgrad: tmode %d (zero or replicate: a whole clip, no chunk cache)", d->tmode);
  VT_CHECK_ARG(d->pt >= 0 && d->pt < d->KT && d->pt_hi >= 0 && d->pt_hi < d->KT && d->ph >= 0 && d->ph < d->KH && d->ph_hi >= 0 && d->ph_hi < d->KH &&
                   d->pw >= 0 && d->pw < d->KW && d->pw_hi >= 0 && d->pw_hi < d->KW, "vt_conv_dgrad: a pad must be smaller than its kernel extent");
  const int Tv = d->Ti << d->ups_t, Hv = d->Hi << d->ups_s, Wv = d->Wi << d->ups_s;
  VT_CHECK_ARG(d->To == Tv + d->pt + d->pt_hi - d->KT + 1 && d->Ho == Hv + d->ph + d->ph_hi - d->KH + 1 && d->Wo == Wv + d->pw + d->pw_hi - d->KW + 1,
               "vt_conv_dgrad: dy extents (%d, %d, %d) are not the forward convolution's", d->To, d->Ho, d->Wo);
  const int vec = d->dtype == VT_BF16 ? 8 : 4;
  VT_CHECK_ARG(d->lddy >= d->Cout && d->lddy % vec == 0 && d->lddx >= d->Cin && d->lddx % 4 == 0, "vt_conv_dgrad: lddy %d / lddx %d", d->lddy, d->lddx);
  VT_CHECK_ARG(d->ldw >= (int64_t)d->KT * d->KH * d->KW * d->lddy && d->ldw % vec == 0, "vt_conv_dgrad: ldw %d (taps x lddy of vt_pack_conv_weight_dgrad)", d->ldw);
  VT_CHECK_ARG(d->acc == nullptr || d->ldacc >= d->Cin, "vt_conv_dgrad: ldacc %d", d->ldacc);
  *rep = (d->tmode == VT_TPAD_REPLICATE) ? d->pt : 0;
  // straight from the convolution's epilogue only where that is the single rounding: fp32 results of a plain geometry
  *folded = *rep > 0 || d->ups_t || d->ups_s || d->dx_dtype != VT_F32;
  return VT_OK;
}

}  // namespace

extern "C" int vt_dgrad_desc_size(void) { return (int)sizeof(vt_dgrad_desc); }

extern "C" int vt_pack_conv_weight_dgrad(const float* w, void* out, int32_t out_dtype, int32_t Cout, int32_t Cin, int32_t cout_p, int32_t KT, int32_t KH,
                                         int32_t KW, int64_t ldw, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(w && out && Cout > 0 && Cin > 0 && cout_p >= Cout && KT > 0 && KH > 0 && KW > 0, "vt_pack_conv_weight_dgrad: bad arguments");
  VT_CHECK_ARG(grad_dtype_ok(out_dtype), "vt_pack_conv_weight_dgrad: out_dtype %d (fp32 or bf16)", out_dtype);
  VT_CHECK_ARG(ldw >= (int64_t)KT * KH * KW * cout_p, "vt_pack_conv_weight_dgrad: ldw %lld", (long long)ldw);
  const unsigned grid = grid_for((long long)Cin * ldw, kBlock, 8192);
  if (out_dtype == VT_F32)
    hipLaunchKernelGGL(pack_dgrad_kernel<float>, dim3(grid), dim3(kBlock), 0, stream, w, static_cast<float*>(out), Cout, Cin, cout_p, KT, KH, KW, (long long)ldw);
  else
    hipLaunchKernelGGL(pack_dgrad_kernel<bf16_t>, dim3(grid), dim3(kBlock), 0, stream, w, static_cast<bf16_t*>(out), Cout, Cin, cout_p, KT, KH, KW, (long long)ldw);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int64_t vt_conv_dgrad_work_bytes(const vt_dgrad_desc* d) {
  int rep = 0;
  bool folded = false;
  if (dgrad_prepare(d, &rep, &folded) != VT_OK) return -1;
  if (!folded) return 0;
  return (int64_t)d->B * (rep + (d->Ti << d->ups_t)) * (d->Hi << d->ups_s) * (d->Wi << d->ups_s) * d->lddx * 4;
}

extern "C" int vt_grad_fold(const void* src, int32_t src_dtype, const void* acc, void* dx, int32_t dx_dtype, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t lds,
                            int32_t lda, int32_t ldo, int32_t rep, int32_t ups_t, int32_t ups_s, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(src && dx && B > 0 && T > 0 && H > 0 && W > 0 && C > 0 && lds >= C && ldo >= C && ldo % 4 == 0 && (acc == nullptr || lda >= C),
               "vt_grad_fold: bad arguments");
  VT_CHECK_ARG(grad_dtype_ok(dx_dtype) && (src_dtype == VT_F32 || src_dtype == dx_dtype) && rep >= 0 && (ups_t | ups_s | 1) == 1,
               "vt_grad_fold: src_dtype %d (fp32 or dx's), dx_dtype %d, rep %d, ups (%d, %d)", src_dtype, dx_dtype, rep, ups_t, ups_s);
  FoldArgs a{src, acc, dx, B, T, H, W, C, lds, lda, ldo, rep, ups_t, ups_s};
  const unsigned grid = grid_for((long long)B * T * H * W * (ldo / 4));
  if (dx_dtype == VT_F32) hipLaunchKernelGGL((grad_fold_kernel<float, float>), dim3(grid), dim3(kBlock), 0, stream, a);
  else if (src_dtype == VT_F32) hipLaunchKernelGGL((grad_fold_kernel<float, bf16_t>), dim3(grid), dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL((grad_fold_kernel<bf16_t, bf16_t>), dim3(grid), dim3(kBlock), 0, stream, a);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int vt_conv_dgrad(const vt_dgrad_desc* d, vt_stream stream) {
  int rep = 0;
  bool folded = false;
  const int rc = dgrad_prepare(d, &rep, &folded);
  if (rc != VT_OK) return rc;
  VT_CHECK_ARG(d->dy && d->wt && d->dx, "vt_conv_dgrad: null tensor pointer");
  const int Tv = d->Ti << d->ups_t, Hv = d->Hi << d->ups_s, Wv = d->Wi << d->ups_s;
  vt_conv_desc c;
  memset(&c, 0, sizeof(c));
  c.x = d->dy; c.w = d->wt;
  c.B = d->B; c.Ti = d->To; c.Hi = d->Ho; c.Wi = d->Wo; c.Cin = d->lddy;
  c.To = rep + Tv; c.Ho = Hv; c.Wo = Wv; c.Cout = d->Cin;
  c.ldw = d->ldw; c.ldy = d->lddx;
  c.KT = d->KT; c.KH = d->KH; c.KW = d->KW;
  c.st = c.sh = c.sw = 1;
  // mirrored pads: virtual-input position i receives dy[i - (K-1) + a'] through flipped tap a'; the output starts at the first REAL
  // position (zero pad: i = pt) or at the first virtual one (replicate: i = 0, the front frames are folded afterwards)
  c.pt = rep > 0 ? d->KT - 1 : d->KT - 1 - d->pt;
  c.ph = d->KH - 1 - d->ph; c.pw = d->KW - 1 - d->pw;
  c.tmode = VT_TPAD_ZERO;
  c.out_layout = VT_NDHWC;
  c.dtype = d->dtype; c.out_dtype = VT_F32;
  c.nbatch = 1;
  if (!folded) {
    c.y = d->dx;
    if (d->acc) { c.res_mode = VT_RES_ADD; c.res = d->acc; c.Tr = d->Ti; c.ldr = d->ldacc; }
    return vt_conv(&c, stream);
  }
  const int64_t need = (int64_t)d->B * (rep + Tv) * Hv * Wv * d->lddx * 4;
  VT_CHECK_ARG(d->work != nullptr && d->work_bytes >= need && (reinterpret_cast<uintptr_t>(d->work) & 15) == 0, "vt_conv_dgrad: workspace of %lld bytes needed (vt_conv_dgrad_work_bytes)",
               (long long)need);
  c.y = d->work;
  const int rc2 = vt_conv(&c, stream);
  if (rc2 != VT_OK) return rc2;
  return vt_grad_fold(d->work, VT_F32, d->acc, d->dx, d->dx_dtype, d->B, d->Ti, d->Hi, d->Wi, d->Cin, d->lddx, d->ldacc, d->lddx, rep, d->ups_t,
                      d->ups_s, stream);
}

extern "C" int vt_softmax_rows_backward(const void* p, int64_t ldp, const float* dp, void* ds, int64_t ldo, int32_t dtype, int64_t rows, int32_t cols, float scale,
                                        vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(p && dp && ds && rows > 0 && cols > 0 && ldp >= cols && ldo >= cols && grad_dtype_ok(dtype), "vt_softmax_rows_backward: bad arguments");
  const unsigned grid = grid_for(rows, kBlock / 64, 8192);
  if (dtype == VT_F32)
    hipLaunchKernelGGL(softmax_rows_backward_kernel<float>, dim3(grid), dim3(kBlock), 0, stream, static_cast<const float*>(p), (long long)ldp, dp, static_cast<float*>(ds),
                       (long long)ldo, (long long)rows, cols, scale);
  else
    hipLaunchKernelGGL(softmax_rows_backward_kernel<bf16_t>, dim3(grid), dim3(kBlock), 0, stream, static_cast<const bf16_t*>(p), (long long)ldp, dp, static_cast<bf16_t*>(ds),
                       (long long)ldo, (long long)rows, cols, scale);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int vt_transpose_batched(const void* in, void* out, int32_t dtype, int32_t Z, int32_t R, int32_t C, int64_t ldi, int64_t ldo, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(in && out && Z > 0 && Z < 65536 && R > 0 && C > 0 && ldi >= C && ldo >= R && grad_dtype_ok(dtype), "vt_transpose_batched: bad arguments");
  const dim3 grid((unsigned)((ldo + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)Z);
  if (dtype == VT_F32)
    hipLaunchKernelGGL(transpose_kernel<uint32_t>, grid, dim3(kBlock), 0, stream, static_cast<const uint32_t*>(in), static_cast<uint32_t*>(out), R, C, (long long)ldi, (long long)ldo);
  else
    hipLaunchKernelGGL(transpose_kernel<uint16_t>, grid, dim3(kBlock), 0, stream, static_cast<const uint16_t*>(in), static_cast<uint16_t*>(out), R, C, (long long)ldi, (long long)ldo);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int vt_upsample_mix(const void* u, const void* c, const float* mix_factor, void* y, int32_t dtype, int64_t M, int32_t C, int32_t ld, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(u && c && mix_factor && y && M > 0 && C > 0 && ld >= C && grad_dtype_ok(dtype), "vt_upsample_mix: bad arguments");
  const unsigned grid = grid_for(M * ld);
  if (dtype == VT_F32)
    hipLaunchKernelGGL(mix_forward_kernel<float>, dim3(grid), dim3(kBlock), 0, stream, static_cast<const float*>(u), static_cast<const float*>(c), mix_factor, static_cast<float*>(y), (long long)M, C, ld);
  else
    hipLaunchKernelGGL(mix_forward_kernel<bf16_t>, dim3(grid), dim3(kBlock), 0, stream, static_cast<const bf16_t*>(u), static_cast<const bf16_t*>(c), mix_factor, static_cast<bf16_t*>(y), (long long)M, C, ld);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int64_t vt_upsample_mix_backward_work_bytes(int64_t M, int32_t ld) {
  if (M <= 0 || ld <= 0) return -1;
  return (int64_t)mix_blocks(M * ld) * 4;
}

extern "C" int vt_upsample_mix_backward(const void* dy, const void* u, const void* c, const float* mix_factor, void* du, void* dc, float* dmix, int32_t dtype, int64_t M,
                                        int32_t C, int32_t ld, void* work, int64_t work_bytes, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(dy && u && c && mix_factor && du && dc && dmix && M > 0 && C > 0 && ld >= C && grad_dtype_ok(dtype), "vt_upsample_mix_backward: bad arguments");
  const int blocks = mix_blocks(M * ld);
  VT_CHECK_ARG(work != nullptr && work_bytes >= (int64_t)blocks * 4, "vt_upsample_mix_backward: workspace of %d bytes needed", blocks * 4);
  float* part = static_cast<float*>(work);
  if (dtype == VT_F32)
    hipLaunchKernelGGL(mix_backward_kernel<float>, dim3(blocks), dim3(kBlock), 0, stream, static_cast<const float*>(dy), static_cast<const float*>(u), static_cast<const float*>(c), mix_factor,
                       static_cast<float*>(du), static_cast<float*>(dc), part, (long long)M, C, ld);
  else
    hipLaunchKernelGGL(mix_backward_kernel<bf16_t>, dim3(blocks), dim3(kBlock), 0, stream, static_cast<const bf16_t*>(dy), static_cast<const bf16_t*>(u), static_cast<const bf16_t*>(c), mix_factor,
                       static_cast<bf16_t*>(du), static_cast<bf16_t*>(dc), part, (long long)M, C, ld);
  VT_CHECK_LAUNCH();
  hipLaunchKernelGGL(mix_finish_kernel, dim3(1), dim3(64), 0, stream, part, blocks, mix_factor, dmix);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int vt_time_lerp2x_backward(const void* dy, void* dx, int32_t dtype, int32_t B, int32_t Ti, int64_t HWC, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(dy && dx && B > 0 && Ti > 0 && HWC > 0 && (int64_t)B * Ti < 65536 && grad_dtype_ok(dtype), "vt_time_lerp2x_backward: bad arguments");
  const dim3 grid(grid_for(HWC, kBlock, 1024), (unsigned)(B * Ti));
  if (dtype == VT_F32)
    hipLaunchKernelGGL(time_lerp2x_backward_kernel<float>, grid, dim3(kBlock), 0, stream, static_cast<const float*>(dy), static_cast<float*>(dx), B, Ti, (long long)HWC);
  else
    hipLaunchKernelGGL(time_lerp2x_backward_kernel<bf16_t>, grid, dim3(kBlock), 0, stream, static_cast<const bf16_t*>(dy), static_cast<bf16_t*>(dx), B, Ti, (long long)HWC);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int vt_grad_ncthw_to_ndhwc(const float* x, void* y, int32_t out_dtype, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t ldy, int32_t tpad,
                                      vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(x && y && B > 0 && C > 0 && T > 0 && H > 0 && W > 0 && ldy >= C && tpad >= 0 && grad_dtype_ok(out_dtype), "vt_grad_ncthw_to_ndhwc: bad arguments");
  const unsigned grid = grid_for((long long)B * (T + tpad) * H * W);
  if (out_dtype == VT_F32) hipLaunchKernelGGL(grad_ncthw_to_ndhwc_kernel<float>, dim3(grid), dim3(kBlock), 0, stream, x, static_cast<float*>(y), B, C, T, H, W, ldy, tpad);
  else hipLaunchKernelGGL(grad_ncthw_to_ndhwc_kernel<bf16_t>, dim3(grid), dim3(kBlock), 0, stream, x, static_cast<bf16_t*>(y), B, C, T, H, W, ldy, tpad);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

extern "C" int vt_grad_add(const void* a, const void* b, void* out, int32_t dtype, int64_t n, vt_stream stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  VT_CHECK_ARG(a && b && out && n > 0 && grad_dtype_ok(dtype), "vt_grad_add: bad arguments");
  const unsigned grid = grid_for(n);
  if (dtype == VT_F32) hipLaunchKernelGGL(grad_add_kernel<float>, dim3(grid), dim3(kBlock), 0, stream, static_cast<const float*>(a), static_cast<const float*>(b), static_cast<float*>(out), (long long)n);
  else hipLaunchKernelGGL(grad_add_kernel<bf16_t>, dim3(grid), dim3(kBlock), 0, stream, static_cast<const bf16_t*>(a), static_cast<const bf16_t*>(b), static_cast<bf16_t*>(out), (long long)n);
  VT_CHECK_LAUNCH();
  return VT_OK;
}
