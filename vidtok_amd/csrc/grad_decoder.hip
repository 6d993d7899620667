// Data-gradient path of the decoder backward (include/vidtok_amd.h, "differentiable decode").
//
// vt_conv_dgrad: the gradient of a vt_conv (row / column stride 1 or 2) with respect to its stored input.  The MACs run on the FORWARD
// implicit-GEMM tiles: an input pixel of parity class (h mod sh, w mod sw) receives only the taps with (r + p - k) mod s = 0, so each
// class is a stride-1 convolution of dy with a tap-flipped, Cin/Cout-transposed sub-kernel (vt_pack_conv_weight_dgrad) under mirrored
// pads, and vt_conv does the work at forward rates; stride 1 is the one class that holds every tap.  What a plain convolution cannot
// express is finished by one more launch.  One class (grad_fold_kernel): the KT - 1 virtual front frames of a replicate time pad add
// into frame 0, and the 2 / 2 x 2 positions of a folded nearest x2 up-sampling add into their source pixel -- fp32 sums in a fixed
// order, rounded once.  Several classes (strided_finish_kernel): they interleave, acc is added, one rounding.  The two stay apart
// because one body for both was measurably slower on either side.
//
// The rest are the small kernels a decoder backward needs around the convolutions and LayerNorms: softmax backward, a batched
// transpose (the attention GEMMs want K-contiguous operands), the alpha-mix of the time up-samplers forward and backward (with the
// mix_factor gradient as fixed-order partials + a second launch), the adjoint of the x2 time interpolation, the cotangent's layout
// change and a gradient add.  No float atomics anywhere: every result is bit-reproducible and every call is capture-safe.
#include "launch.h"

namespace {

constexpr int kBlock = 256;

// ---- parity classes of the input, per axis -----------------------------------------------------------------------------------
// input positions i = s j + r receive only the taps k0, k0 + s, ... (nk of them): as a stride-1 convolution over dy that is the flipped
// tap list under the front pad `pad`, n outputs.  s = 1: the one class r = 0 holds every tap under the mirrored pad K - 1 - p
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

// ---- transposed, tap-flipped weight pack, one block [Cin][ldw] per class ---------------------------------------------------------
// out[cls][ci][k], k = ((a' nkh + p') nkw + q') cout_p + co  <-  w[co][ci][KT-1-a'][kh0 + sh (nkh-1-p')][kw0 + sw (nkw-1-q')]; the rest zero
template <typename TO>
__global__ __launch_bounds__(kBlock) void pack_dgrad_kernel(const float* __restrict__ w, TO* __restrict__ out, int Cout, int Cin, int cout_p, int KT, int KH,
                                                            int KW, int sh, int sw, int ph, int pw, long long ldw) {
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

// ---- the classes of a strided data gradient interleaved (+ acc), one rounding ----------------------------------------------------------
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

// what vt_conv_dgrad launches: the classes of the virtual (up-sampled) rows and columns and where each class convolution writes
struct DgradPlan {
  AxisClass ah[2], aw[2];
  int64_t off[4];        // class rh * sw + rw at off[] bytes into work; -1: no tap or no pixel (zeros)
  int64_t bytes;         // of work; 0: the one class is written into dx by its own launch
  int rep;               // virtual front frames kept for the fold
};

// checks of a vt_dgrad_desc; fills the plan
int dgrad_prepare(const vt_dgrad_desc* d, DgradPlan* p) {
  VT_CHECK_ARG(d != nullptr, "vt_conv_dgrad: null descriptor");
  VT_CHECK_ARG(grad_dtype_ok(d->dtype) && (d->dx_dtype == d->dtype || d->dx_dtype == VT_F32), "vt_conv_dgrad: dtype %d -> dx_dtype %d (fp32 or bf16 operands; dx in the operand type or fp32)",
               d->dtype, d->dx_dtype);
  VT_CHECK_ARG(d->st == 1 && (d->sh == 1 || d->sh == 2) && (d->sw == 1 || d->sw == 2), "vt_conv_dgrad: strides (%d, %d, %d): st = 1 and sh, sw in {1, 2}", d->st, d->sh, d->sw);
  const bool strided = d->sh + d->sw > 2;
  VT_CHECK_ARG(d->B > 0 && d->Ti > 0 && d->Hi > 0 && d->Wi > 0 && d->Cin > 0 && d->Cout > 0 && d->To > 0 && d->Ho > 0 && d->Wo > 0, "vt_conv_dgrad: bad dims");
  VT_CHECK_ARG(d->KT > 0 && d->KH > 0 && d->KW > 0 && d->KT * d->KH * d->KW <= 64, "vt_conv_dgrad: bad taps");
  VT_CHECK_ARG((d->ups_t | d->ups_s | 1) == 1, "vt_conv_dgrad: ups_t / ups_s are 0 or 1");
  VT_CHECK_ARG(d->tmode == VT_TPAD_ZERO || d->tmode == VT_TPAD_REPLICATE, "vt_conv_dgrad: tmode %d (zero or replicate: a whole clip, no chunk cache)", d->tmode);
  VT_CHECK_ARG(!strided || (d->tmode == VT_TPAD_ZERO && d->ups_t == 0 && d->ups_s == 0 && d->KT <= 4 && d->KH <= 4 && d->KW <= 4),
               "vt_conv_dgrad: strides (%d, %d) with tmode %d, ups (%d, %d), taps (%d, %d, %d): a strided geometry has a zero time pad, no folded up-sampling and 1 .. 4 taps an axis",
               d->sh, d->sw, d->tmode, d->ups_t, d->ups_s, d->KT, d->KH, d->KW);
  VT_CHECK_ARG(d->pt >= 0 && d->pt < d->KT && d->pt_hi >= 0 && d->pt_hi < d->KT && d->ph >= 0 && d->ph < d->KH && d->ph_hi >= 0 && d->ph_hi < d->KH &&
                   d->pw >= 0 && d->pw < d->KW && d->pw_hi >= 0 && d->pw_hi < d->KW, "vt_conv_dgrad: a pad must be smaller than its kernel extent");
  const int Tv = d->Ti << d->ups_t, Hv = d->Hi << d->ups_s, Wv = d->Wi << d->ups_s;
  VT_CHECK_ARG(d->To == Tv + d->pt + d->pt_hi - d->KT + 1 && Hv + d->ph + d->ph_hi >= d->KH && d->Ho == (Hv + d->ph + d->ph_hi - d->KH) / d->sh + 1 &&
                   Wv + d->pw + d->pw_hi >= d->KW && d->Wo == (Wv + d->pw + d->pw_hi - d->KW) / d->sw + 1,
               "vt_conv_dgrad: dy extents (%d, %d, %d) are not the forward convolution's", d->To, d->Ho, d->Wo);
  const int vec = d->dtype == VT_BF16 ? 8 : 4;
  VT_CHECK_ARG(d->lddy >= d->Cout && d->lddy % vec == 0 && d->lddx >= d->Cin && d->lddx % 4 == 0, "vt_conv_dgrad: lddy %d / lddx %d", d->lddy, d->lddx);
  const int nkh = (d->KH + d->sh - 1) / d->sh, nkw = (d->KW + d->sw - 1) / d->sw;
  VT_CHECK_ARG(d->ldw >= (int64_t)d->KT * nkh * nkw * d->lddy && d->ldw % vec == 0, "vt_conv_dgrad: ldw %d (vt_pack_conv_weight_dgrad: KT ceil(KH/sh) ceil(KW/sw) lddy)", d->ldw);
  VT_CHECK_ARG(d->acc == nullptr || d->ldacc >= d->Cin, "vt_conv_dgrad: ldacc %d", d->ldacc);
  p->rep = (d->tmode == VT_TPAD_REPLICATE) ? d->pt : 0;
  // straight from the convolution's epilogue only where that is the single rounding: fp32 results of a plain stride-1 geometry
  const bool folded = strided || p->rep > 0 || d->ups_t || d->ups_s || d->dx_dtype != VT_F32;
  int64_t at = 0;
  for (int rh = 0; rh < d->sh; ++rh) p->ah[rh] = axis_class(d->KH, d->sh, d->ph, rh, Hv);
  for (int rw = 0; rw < d->sw; ++rw) p->aw[rw] = axis_class(d->KW, d->sw, d->pw, rw, Wv);
  for (int rh = 0; rh < d->sh; ++rh)
    for (int rw = 0; rw < d->sw; ++rw) {
      const AxisClass &h = p->ah[rh], &w = p->aw[rw];
      VT_CHECK_ARG(h.pad >= 0 && w.pad >= 0, "vt_conv_dgrad: pads (%d, %d) put a class convolution in front of dy's first pixel", d->ph, d->pw);
      const bool empty = h.nk == 0 || w.nk == 0 || h.n == 0 || w.n == 0;
      p->off[rh * d->sw + rw] = empty ? -1 : at;
      // several classes start on 256-byte boundaries; a lone class takes exactly its size
      const int64_t sz = (int64_t)d->B * (p->rep + Tv) * h.n * w.n * d->lddx * 4;
      if (folded && !empty) at += strided ? (sz + 255) / 256 * 256 : sz;
    }
  p->bytes = at;
  return VT_OK;
}

// the stride-1 convolution over dy that computes class (rh, rw): flipped sub-kernel, mirrored pads, fp32 out
vt_conv_desc class_conv(const vt_dgrad_desc* d, const DgradPlan& p, int rh, int rw) {
  const AxisClass &h = p.ah[rh], &w = p.aw[rw];
  const int cls = rh * d->sw + rw;
  vt_conv_desc c;
  memset(&c, 0, sizeof(c));
  c.x = d->dy;
  c.w = static_cast<const char*>(d->wt) + (int64_t)cls * d->Cin * d->ldw * (d->dtype == VT_BF16 ? 2 : 4);
  c.B = d->B; c.Ti = d->To; c.Hi = d->Ho; c.Wi = d->Wo; c.Cin = d->lddy;
  c.To = p.rep + (d->Ti << d->ups_t); c.Ho = h.n; c.Wo = w.n; c.Cout = d->Cin;
  c.ldw = d->ldw; c.ldy = d->lddx;
  c.KT = d->KT; c.KH = h.nk; c.KW = w.nk;
  c.st = c.sh = c.sw = 1;
  // mirrored pads: virtual-input position i receives dy[i - (K-1) + a'] through flipped tap a'; the output starts at the first REAL
  // position (zero pad: i = pt) or at the first virtual one (replicate: i = 0, the front frames are folded afterwards)
  c.pt = p.rep > 0 ? d->KT - 1 : d->KT - 1 - d->pt;
  c.ph = h.pad; c.pw = w.pad;
  c.tmode = VT_TPAD_ZERO;
  c.out_layout = VT_NDHWC;
  c.dtype = d->dtype; c.out_dtype = VT_F32;
  c.nbatch = 1;
  if (p.bytes > 0) {
    c.y = static_cast<char*>(d->work) + p.off[cls];
  } else {
    c.y = d->dx;
    if (d->acc) { c.res_mode = VT_RES_ADD; c.res = d->acc; c.Tr = d->Ti; c.ldr = d->ldacc; }
  }
  return c;
}

}  // namespace

extern "C" int vt_dgrad_desc_size(void) { return (int)sizeof(vt_dgrad_desc); }

extern "C" int vt_pack_conv_weight_dgrad(const float* w, void* out, int32_t out_dtype, int32_t Cout, int32_t Cin, int32_t cout_p, int32_t KT, int32_t KH,
                                         int32_t KW, int32_t sh, int32_t sw, int32_t ph, int32_t pw, int64_t ldw, vt_stream stream_) {
  VT_CHECK_ARG(w && out && Cout > 0 && Cin > 0 && cout_p >= Cout && KT > 0 && KH > 0 && KW > 0, "vt_pack_conv_weight_dgrad: bad arguments");
  VT_CHECK_ARG(grad_dtype_ok(out_dtype), "vt_pack_conv_weight_dgrad: out_dtype %d (fp32 or bf16)", out_dtype);
  VT_CHECK_ARG((sh == 1 || sh == 2) && (sw == 1 || sw == 2) && ph >= 0 && ph < KH && pw >= 0 && pw < KW, "vt_pack_conv_weight_dgrad: strides (%d, %d) in {1, 2}, pads (%d, %d) below the taps",
               sh, sw, ph, pw);
  VT_CHECK_ARG(sh + sw == 2 || (KT <= 4 && KH <= 4 && KW <= 4), "vt_pack_conv_weight_dgrad: taps (%d, %d, %d): 1 .. 4 an axis under a stride", KT, KH, KW);
  VT_CHECK_ARG(ldw >= (int64_t)KT * ((KH + sh - 1) / sh) * ((KW + sw - 1) / sw) * cout_p, "vt_pack_conv_weight_dgrad: ldw %lld", (long long)ldw);
  return vt_dispatch<float, bf16_t>(out_dtype, [&](auto t) {
    using TO = vt_t<decltype(t)>;
    return launch(pack_dgrad_kernel<TO>, dim3(grid_for((long long)sh * sw * Cin * ldw, kBlock, 8192)), dim3(kBlock), 0, as_stream(stream_), w, static_cast<TO*>(out), Cout, Cin,
                  cout_p, KT, KH, KW, sh, sw, ph, pw, (long long)ldw);
  });
}

extern "C" int64_t vt_conv_dgrad_work_bytes(const vt_dgrad_desc* d) {
  DgradPlan p;
  return dgrad_prepare(d, &p) == VT_OK ? p.bytes : -1;
}

extern "C" int vt_grad_fold(const void* src, int32_t src_dtype, const void* acc, void* dx, int32_t dx_dtype, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t lds,
                            int32_t lda, int32_t ldo, int32_t rep, int32_t ups_t, int32_t ups_s, vt_stream stream_) {
  VT_CHECK_ARG(src && dx && B > 0 && T > 0 && H > 0 && W > 0 && C > 0 && lds >= C && ldo >= C && ldo % 4 == 0 && (acc == nullptr || lda >= C),
               "vt_grad_fold: bad arguments");
  VT_CHECK_ARG(grad_dtype_ok(dx_dtype) && (src_dtype == VT_F32 || src_dtype == dx_dtype) && rep >= 0 && (ups_t | ups_s | 1) == 1,
               "vt_grad_fold: src_dtype %d (fp32 or dx's), dx_dtype %d, rep %d, ups (%d, %d)", src_dtype, dx_dtype, rep, ups_t, ups_s);
  FoldArgs a{src, acc, dx, B, T, H, W, C, lds, lda, ldo, rep, ups_t, ups_s};
  return vt_dispatch_grad(dx_dtype, src_dtype, [&](auto to, auto ts) {
    return launch(grad_fold_kernel<vt_t<decltype(ts)>, vt_t<decltype(to)>>, dim3(grid_for((long long)B * T * H * W * (ldo / 4), kBlock, 16384)), dim3(kBlock), 0,
                  as_stream(stream_), a);
  });
}

extern "C" int vt_conv_dgrad(const vt_dgrad_desc* d, vt_stream stream_) {
  DgradPlan p;
  const int rc = dgrad_prepare(d, &p);
  if (rc != VT_OK) return rc;
  VT_CHECK_ARG(d->dy && d->wt && d->dx, "vt_conv_dgrad: null tensor pointer");
  VT_CHECK_ARG(p.bytes == 0 || (d->work != nullptr && d->work_bytes >= p.bytes && (reinterpret_cast<uintptr_t>(d->work) & 15) == 0),
               "vt_conv_dgrad: workspace of %lld bytes needed (vt_conv_dgrad_work_bytes)", (long long)p.bytes);
  FinishArgs f;
  memset(&f, 0, sizeof(f));
  for (int rh = 0; rh < d->sh; ++rh)
    for (int rw = 0; rw < d->sw; ++rw) {
      const int cls = rh * d->sw + rw;
      f.off[cls] = p.off[cls] < 0 ? -1 : p.off[cls] / 4;
      f.nh[cls] = p.ah[rh].n;
      f.nw[cls] = p.aw[rw].n;
      if (p.off[cls] < 0) continue;
      const vt_conv_desc c = class_conv(d, p, rh, rw);
      const int rc2 = vt_conv(&c, stream_);
      if (rc2 != VT_OK) return rc2;
    }
  if (p.bytes == 0) return VT_OK;                     // the one class went straight into dx
  if (d->sh + d->sw == 2)                             // one class: replicate front frames, folded up-sampling, acc, one rounding
    return vt_grad_fold(d->work, VT_F32, d->acc, d->dx, d->dx_dtype, d->B, d->Ti, d->Hi, d->Wi, d->Cin, d->lddx, d->ldacc, d->lddx, p.rep, d->ups_t, d->ups_s, stream_);
  f.work = static_cast<const float*>(d->work);
  f.acc = d->acc;
  f.dx = d->dx;
  f.B = d->B; f.T = d->Ti; f.H = d->Hi; f.W = d->Wi; f.C = d->Cin; f.ld = d->lddx; f.lda = d->ldacc; f.sh = d->sh; f.sw = d->sw;
  return vt_dispatch<float, bf16_t>(d->dx_dtype, [&](auto t) {
    return launch(strided_finish_kernel<vt_t<decltype(t)>>, dim3(grid_for((long long)d->B * d->Ti * d->Hi * d->Wi * (d->lddx / 4), kBlock, 16384)), dim3(kBlock), 0,
                  as_stream(stream_), f);
  });
}

extern "C" int vt_softmax_rows_backward(const void* p, int64_t ldp, const float* dp, void* ds, int64_t ldo, int32_t dtype, int64_t rows, int32_t cols, float scale,
                                        vt_stream stream_) {
  VT_CHECK_ARG(p && dp && ds && rows > 0 && cols > 0 && ldp >= cols && ldo >= cols && grad_dtype_ok(dtype), "vt_softmax_rows_backward: bad arguments");
  return vt_dispatch<float, bf16_t>(dtype, [&](auto t) {
    using T = vt_t<decltype(t)>;
    return launch(softmax_rows_backward_kernel<T>, dim3(grid_for(rows, kBlock / 64, 8192)), dim3(kBlock), 0, as_stream(stream_), static_cast<const T*>(p), (long long)ldp, dp,
                  static_cast<T*>(ds), (long long)ldo, (long long)rows, cols, scale);
  });
}

extern "C" int vt_transpose_batched(const void* in, void* out, int32_t dtype, int32_t Z, int32_t R, int32_t C, int64_t ldi, int64_t ldo, vt_stream stream_) {
  VT_CHECK_ARG(in && out && Z > 0 && Z < 65536 && R > 0 && C > 0 && ldi >= C && ldo >= R && grad_dtype_ok(dtype), "vt_transpose_batched: bad arguments");
  const dim3 grid((unsigned)((ldo + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)Z);
  return vt_dispatch_size<uint32_t, uint16_t>(dtype == VT_F32 ? 4 : 2, [&](auto t) {
    using E = vt_t<decltype(t)>;
    return launch(transpose_kernel<E>, grid, dim3(kBlock), 0, as_stream(stream_), static_cast<const E*>(in), static_cast<E*>(out), R, C, (long long)ldi, (long long)ldo);
  });
}

extern "C" int vt_upsample_mix(const void* u, const void* c, const float* mix_factor, void* y, int32_t dtype, int64_t M, int32_t C, int32_t ld, vt_stream stream_) {
  VT_CHECK_ARG(u && c && mix_factor && y && M > 0 && C > 0 && ld >= C && grad_dtype_ok(dtype), "vt_upsample_mix: bad arguments");
  return vt_dispatch<float, bf16_t>(dtype, [&](auto t) {
    using T = vt_t<decltype(t)>;
    return launch(mix_forward_kernel<T>, dim3(grid_for(M * ld, kBlock, 16384)), dim3(kBlock), 0, as_stream(stream_), static_cast<const T*>(u), static_cast<const T*>(c), mix_factor,
                  static_cast<T*>(y), (long long)M, C, ld);
  });
}

extern "C" int64_t vt_upsample_mix_backward_work_bytes(int64_t M, int32_t ld) {
  if (M <= 0 || ld <= 0) return -1;
  return (int64_t)mix_blocks(M * ld) * 4;
}

extern "C" int vt_upsample_mix_backward(const void* dy, const void* u, const void* c, const float* mix_factor, void* du, void* dc, float* dmix, int32_t dtype, int64_t M,
                                        int32_t C, int32_t ld, void* work, int64_t work_bytes, vt_stream stream_) {
  hipStream_t stream = as_stream(stream_);
  VT_CHECK_ARG(dy && u && c && mix_factor && du && dc && dmix && M > 0 && C > 0 && ld >= C && grad_dtype_ok(dtype), "vt_upsample_mix_backward: bad arguments");
  const int blocks = mix_blocks(M * ld);
  VT_CHECK_ARG(work != nullptr && work_bytes >= (int64_t)blocks * 4, "vt_upsample_mix_backward: workspace of %d bytes needed", blocks * 4);
  float* part = static_cast<float*>(work);
  const int rc = vt_dispatch<float, bf16_t>(dtype, [&](auto t) {
    using T = vt_t<decltype(t)>;
    return launch(mix_backward_kernel<T>, dim3(blocks), dim3(kBlock), 0, stream, static_cast<const T*>(dy), static_cast<const T*>(u), static_cast<const T*>(c), mix_factor,
                  static_cast<T*>(du), static_cast<T*>(dc), part, (long long)M, C, ld);
  });
  if (rc != VT_OK) return rc;
  return launch(mix_finish_kernel, dim3(1), dim3(64), 0, stream, part, blocks, mix_factor, dmix);
}

extern "C" int vt_time_lerp2x_backward(const void* dy, void* dx, int32_t dtype, int32_t B, int32_t Ti, int64_t HWC, vt_stream stream_) {
  VT_CHECK_ARG(dy && dx && B > 0 && Ti > 0 && HWC > 0 && (int64_t)B * Ti < 65536 && grad_dtype_ok(dtype), "vt_time_lerp2x_backward: bad arguments");
  const dim3 grid(grid_for(HWC, kBlock, 1024), (unsigned)(B * Ti));
  return vt_dispatch<float, bf16_t>(dtype, [&](auto t) {
    using T = vt_t<decltype(t)>;
    return launch(time_lerp2x_backward_kernel<T>, grid, dim3(kBlock), 0, as_stream(stream_), static_cast<const T*>(dy), static_cast<T*>(dx), B, Ti, (long long)HWC);
  });
}

extern "C" int vt_grad_ncthw_to_ndhwc(const float* x, void* y, int32_t out_dtype, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t ldy, int32_t tpad,
                                      vt_stream stream_) {
  VT_CHECK_ARG(x && y && B > 0 && C > 0 && T > 0 && H > 0 && W > 0 && ldy >= C && tpad >= 0 && grad_dtype_ok(out_dtype), "vt_grad_ncthw_to_ndhwc: bad arguments");
  return vt_dispatch<float, bf16_t>(out_dtype, [&](auto t) {
    using TO = vt_t<decltype(t)>;
    return launch(grad_ncthw_to_ndhwc_kernel<TO>, dim3(grid_for((long long)B * (T + tpad) * H * W, kBlock, 16384)), dim3(kBlock), 0, as_stream(stream_), x, static_cast<TO*>(y), B,
                  C, T, H, W, ldy, tpad);
  });
}

extern "C" int vt_grad_add(const void* a, const void* b, void* out, int32_t dtype, int64_t n, vt_stream stream_) {
  VT_CHECK_ARG(a && b && out && n > 0 && grad_dtype_ok(dtype), "vt_grad_add: bad arguments");
  return vt_dispatch<float, bf16_t>(dtype, [&](auto t) {
    using T = vt_t<decltype(t)>;
    return launch(grad_add_kernel<T>, dim3(grid_for(n, kBlock, 16384)), dim3(kBlock), 0, as_stream(stream_), static_cast<const T*>(a), static_cast<const T*>(b), static_cast<T*>(out),
                  (long long)n);
  });
}
