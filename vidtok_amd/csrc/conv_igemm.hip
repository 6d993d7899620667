// vt_conv and the calls around it (include/vidtok_amd.h): each asks conv_decide (conv_select.h) for the plan once, then runs or reports it;
// the split-K path of the implicit-GEMM convolution.
// The kernel itself is conv_igemm_kernel.h, instantiated per arithmetic in conv_igemm_{f32,bf16,f16,x3}.hip; the special-shape kernels
// it hands over to live in conv_ws2.hip (3 x 3, 128 -> 128), conv_in8.hip (the encoder's conv_in) and conv_narrow.hip (Cout <= 4).
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "conv_select.h"

namespace {

// ---- split-K over the time taps (include/vidtok_amd.h, vt_conv_work_bytes) ------------------------------------------------------------
// y[m][n] = H(((p0 + p1) + p2) + bias[n]  [+ res[m][n]]) (H = bf16 / fp16) from the KT fp32 partials [KT][M][Cout]; a thread = 8 channels of a pixel
template <typename H>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, int planes, long long M, int Cout, const float* __restrict__ bias,
                                                            const H* __restrict__ res, H* __restrict__ y) {
  const long long n8 = M * (Cout / 8);
  const long long plane = M * (long long)Cout;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i * 8;
    const int c = (int)(e % Cout);
    float v[8];
    {
      const f32x4 a = *reinterpret_cast<const f32x4*>(part + e), b = *reinterpret_cast<const f32x4*>(part + e + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) { v[k] = a[k]; v[4 + k] = b[k]; }
    }
    for (int pz = 1; pz < planes; ++pz) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(part + pz * plane + e), b = *reinterpret_cast<const f32x4*>(part + pz * plane + e + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) { v[k] += a[k]; v[4 + k] += b[k]; }
    }
    if (bias) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(bias + c), b = *reinterpret_cast<const f32x4*>(bias + c + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) { v[k] += a[k]; v[4 + k] += b[k]; }
    }
    if (res) {
      Oct<H> r;
      r.load(res + e);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = r.get(k) + v[k];
    }
    Oct<H>::store(y + e, v);
  }
}

// the per-arithmetic translation unit of an implicit-GEMM launch
int launch_igemm(int dtype, bool out_f32, const IgemmLaunch& l, void* stream) {
  switch (dtype) {
    case VT_F32: return vt_igemm_dispatch_f32(&l, stream);
    case VT_BF16X3: return vt_igemm_dispatch_x3(&l, stream);
    case VT_F16: return vt_igemm_dispatch_f16(&l, out_f32 ? 1 : 0, stream);
    default: return vt_igemm_dispatch_bf16(&l, out_f32 ? 1 : 0, stream);
  }
}

// The scratch side of split-K, for the launch and for the report: the plan holds the geometry rule, the call has to bring the scratch.
// vt_conv (`sized`) also wants it large enough and 16-byte aligned and runs unsplit otherwise; vt_conv_plan counts the split launch for
// any scratch pointer, as it always has -- hosts size the scratch with vt_conv_work_bytes, so the two agree on every call they make.
bool splitk_runs(const ConvPlan& p, const ConvArgs& a, const vt_conv_desc* d, bool sized) {
  if (p.kernel != CONV_IGEMM || p.splitk_planes == 0 || d->work == nullptr) return false;
  return !sized || (d->work_bytes >= (int64_t)p.splitk_planes * a.M * a.Cout * 4 && (reinterpret_cast<uintptr_t>(d->work) & 15) == 0);
}

// the plan's partial launch (p.part: conv_decide built its arguments), then the reduction over the planes into a's y
int launch_splitk(const vt_conv_desc* d, const ConvArgs& a, const ConvPlan& p, hipStream_t stream) {
  const int planes = p.splitk_planes;
  if (p.part_rc != VT_OK) return p.part_rc;       // conv_decide found no form for the partial launch, and said why
  int rc = launch_igemm(d->dtype, true, p.part, stream);
  if (rc != VT_OK) return rc;
  const long long n8 = (long long)a.M * (a.Cout / 8);
  const unsigned grid = (unsigned)std::min<long long>((n8 + 255) / 256, 4096);
  const void* res = a.res_mode == VT_RES_ADD ? a.res : nullptr;
  if (d->dtype == VT_F16)
    hipLaunchKernelGGL(splitk_reduce_kernel<f16_t>, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const float*>(d->work), planes, (long long)a.M, a.Cout, a.bias,
                       reinterpret_cast<const f16_t*>(res), reinterpret_cast<f16_t*>(a.y));
  else
    hipLaunchKernelGGL(splitk_reduce_kernel<bf16_t>, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const float*>(d->work), planes, (long long)a.M, a.Cout, a.bias,
                       reinterpret_cast<const bf16_t*>(res), reinterpret_cast<bf16_t*>(a.y));
  VT_CHECK_LAUNCH();
  return VT_OK;
}

// vt_time_upsample3's decision: the parity descriptor's plan, the serving rule, the form of the paired launch (l.a still without V)
int tup3_decide(const vt_conv_desc* u, IgemmLaunch& l) {
  ConvArgs a;
  ConvPlan p;
  const int rc = conv_decide(u, a, p);
  if (rc != VT_OK) return rc;
  VT_CHECK_ARG(tup3_eligible(u, a, p), "vt_time_upsample3: descriptor not covered (ask vt_time_upsample3_supported; the parity launches of vt_conv serve it)");
  const IgemmVariant pair = {TILE_256x256, true, 2, 2, kRowBytes};
  return igemm_launch_form(l, a, pair, 1, u->dtype, u->out_dtype);
}

// vt_conv_act's decision: vt_conv's descriptor checks with the activation's tile rule, then what the ReLU instantiations cover
int conv_act_decide(const vt_conv_desc* d, int32_t act, ConvArgs& a, ConvPlan& p) {
  VT_CHECK_ARG(act == VT_ACT_RELU, "vt_conv_act: act %d (VT_ACT_RELU = %d is the one activation)", act, VT_ACT_RELU);
  const int rc = conv_decide(d, a, p, nullptr, act);
  if (rc != VT_OK) return rc;
  VT_CHECK_ARG(d->dtype != VT_BF16X3 && d->out_dtype == d->dtype, "vt_conv_act: fp32, bf16 or fp16 arithmetic with results in the same type");
  VT_CHECK_ARG(d->out_layout == VT_NDHWC && d->res_mode == VT_RES_NONE && d->ln_mode == 0 && p.nbatch == 1 && a.yt_mul == 1 && a.ys_mul == 1,
               "vt_conv_act: NDHWC output without residual, LayerNorm, batching or interleave");
  VT_CHECK_ARG(p.whole.v.tile == TILE_256x64 || p.whole.v.fast, "vt_conv_act: Cout=%d needs Cin a multiple of %d (got %d)", a.Cout,
               kRowBytes / (vt_is_h16(d->dtype) ? 2 : 4), a.Cin);
  return VT_OK;
}

}  // namespace

extern "C" int vt_conv_max_lds_bytes(void) { return 163840; }   // the persistent kernels take nearly all of a CU's LDS

// the plan of vt_conv(d) as numbers (out8: include/vidtok_amd.h)
extern "C" int vt_conv_plan(const vt_conv_desc* d, int32_t* out8) {
  VT_CHECK_ARG(out8 != nullptr, "vt_conv_plan: null output");
  ConvArgs a;
  ConvPlan p;
  const int rc = conv_decide(d, a, p);
  if (rc != VT_OK) return rc;
  out8[4] = p.ln_fused ? 1 : 0;
  out8[5] = 1;
  out8[6] = p.kernel;
  out8[7] = 0;
  switch (p.kernel) {
    case CONV_NARROW:   // independent waves: 8 x 14 output pixels x all frames of a time segment; split-bf16 in two passes (hi / lo weight plane)
      vt_conv_narrow_plan(&a, out8);
      out8[5] = p.narrow_mode == 2 ? 2 : 1;
      break;
    case CONV_WS2:      // persistent, at most one workgroup per CU, all 128 channels per tile: 4 x 16-pixel tiles on 8 waves
      out8[0] = 64; out8[1] = 128; out8[2] = 8;
      out8[3] = (a.Wo / 16) * (a.Ho / 4) * a.B * a.To;
      break;
    case CONV_IN8:      // the 128 x 128 tile from a halo patch, register-stationary weights, epilogue through the LDS
      out8[0] = 128; out8[1] = 128; out8[2] = 4;
      out8[3] = a.M / 128;
      out8[7] = 1;
      break;
    case CONV_IGEMM: {
      const IgemmVariant& v = p.whole.v;
      const TileShape& t = kTileShapes[v.tile];
      out8[0] = t.bm(); out8[1] = t.bn(); out8[2] = t.waves();
      out8[3] = (int32_t)((long long)((a.M + t.bm() - 1) / t.bm()) * ((a.Cout + t.bn() - 1) / t.bn()) * p.nbatch);
      if (d->ln_mode != 0 && !p.ln_fused) out8[5] += 1;     // vt_layernorm_act behind the convolution
      if (splitk_runs(p, a, d, false)) out8[5] += 1;        // partial launch + reduction
      out8[7] = v.tile == TILE_256x256 ? (v.ln256 ? 1 : 0) : (v.stages == 4 ? 2 : 0);
      break;
    }
  }
  return VT_OK;
}

// Measurement aid (scripts/conv_profile.py): vt_conv on the 8-wave 256 x 256 bf16 tile with shader-clock stamps at the
// phase boundaries of K steps 8..11 of workgroup 0; stamps_out (device, 8 waves x 4 steps x 8 uint64).
extern "C" int vt_conv_profile(const vt_conv_desc* d, uint64_t* stamps_out, vt_stream stream_) {
  VT_CHECK_ARG(stamps_out != nullptr, "vt_conv_profile: null output");
  ConvArgs a;
  ConvPlan p;
  const int rc = conv_decide(d, a, p, reinterpret_cast<unsigned long long*>(stamps_out));
  if (rc != VT_OK) return rc;
  if (p.kernel == CONV_WS2) return vt_ws2_launch(&a, d->dtype, stream_);       // stamps [wave][16]: conv_ws2.hip iterations 8, 9 of workgroup 0 (8 waves; bf16 only)
  VT_CHECK_ARG(p.kernel == CONV_IGEMM && ((d->dtype == VT_BF16 && d->out_dtype == VT_BF16) || d->dtype == VT_BF16X3) && d->ln_mode == 0 &&
                   p.whole.v.tile == TILE_256x256,
               "vt_conv_profile: bf16 / split-bf16 launches on the 256 x 256 tile without LayerNorm, or on the weight-stationary kernel");
  return launch_igemm(d->dtype, false, p.whole, stream_);
}

extern "C" int64_t vt_conv_work_bytes(const vt_conv_desc* d) {
  ConvArgs a;
  ConvPlan p;
  if (conv_decide(d, a, p) != VT_OK || p.kernel != CONV_IGEMM) return 0;
  return (int64_t)p.splitk_planes * a.M * a.Cout * 4;
}

extern "C" int vt_conv(const vt_conv_desc* d, vt_stream stream_) {
  ConvArgs a;
  ConvPlan p;
  int rc = conv_decide(d, a, p);
  if (rc != VT_OK) return rc;
  switch (p.kernel) {
    case CONV_WS2: return vt_ws2_launch(&a, d->dtype, stream_);
    case CONV_NARROW: return vt_conv_narrow_launch(&a, stream_, p.narrow_mode);
    case CONV_IN8: return vt_conv_in8_launch(&a, d->dtype, stream_);
    case CONV_IGEMM: break;
  }
  rc = splitk_runs(p, a, d, true) ? launch_splitk(d, a, p, reinterpret_cast<hipStream_t>(stream_))
                                  : launch_igemm(d->dtype, d->out_dtype == VT_F32, p.whole, stream_);
  if (rc != VT_OK || d->ln_mode == 0 || p.ln_fused) return rc;
  // not fusable here: the same contract in two launches
  return vt_layernorm_act(d->y, d->out_dtype, d->ldy, d->ln_out, d->out_dtype, d->ldn, d->ln_gamma, d->ln_beta, a.M, d->Cout,
                          d->ln_eps, d->ln_mode == 2 ? 1 : 0, stream_);
}

// The three-product time up-sampler (include/vidtok_amd.h): the parity descriptor's launch on the 8-wave tile with the paired epilogue
// (LN256 = 2 of conv_igemm_glds_kernel), which forms both frames of a pair from one accumulator row and V = W1 x.  The serving rule is
// tup3_eligible (conv_select.h); the K loop, the tile walk, the skipped zero taps and the streaming stores are vt_conv's.
extern "C" int vt_time_upsample3_supported(const vt_conv_desc* u) {
  ConvArgs a;
  ConvPlan p;
  if (conv_decide(u, a, p) != VT_OK) return 0;
  return tup3_eligible(u, a, p) ? 1 : 0;
}

extern "C" int vt_time_upsample3(const vt_conv_desc* u, const void* v, int32_t ldv, vt_stream stream_) {
  IgemmLaunch l;
  const int rc = tup3_decide(u, l);
  if (rc != VT_OK) return rc;
  VT_CHECK_ARG(v != nullptr && (reinterpret_cast<uintptr_t>(v) & 15) == 0 && ldv >= u->Cout && ldv % 8 == 0,
               "vt_time_upsample3: v must be 16-byte aligned with ldv = %d >= Cout and a multiple of 8", ldv);
  l.a.pair_v = reinterpret_cast<const char*>(v);
  l.a.ldv = ldv;
  return launch_igemm(u->dtype, false, l, stream_);
}

// vt_conv with a ReLU epilogue (VGG16's conv + ReLU pairs, LPIPS): the same descriptor checks, then the ACT = VT_ACT_RELU instantiations of
// conv_igemm_act.hip -- never the weight-stationary, conv_in8, narrow or split-K kernels, whose epilogues have no activation
extern "C" int vt_conv_act(const vt_conv_desc* d, int32_t act, vt_stream stream_) {
  ConvArgs a;
  ConvPlan p;
  const int rc = conv_act_decide(d, act, a, p);
  if (rc != VT_OK) return rc;
  return vt_igemm_dispatch_relu(&p.whole, d->dtype, stream_);
}

// the form of the implicit-GEMM launch behind vt_conv (call 0), vt_time_upsample3 (1) or vt_conv_act with ReLU (2), as numbers
// (out16: include/vidtok_amd.h); the other kernels report themselves and zeros
extern "C" int vt_conv_launch_form(const vt_conv_desc* d, int32_t call, int64_t* out16) {
  VT_CHECK_ARG(out16 != nullptr && call >= 0 && call <= 2, "vt_conv_launch_form: null output, or call %d outside 0 .. 2", call);
  ConvArgs a;
  ConvPlan p;
  IgemmLaunch pair;
  const IgemmLaunch* l = &p.whole;
  int rc;
  if (call == 1) {
    rc = tup3_decide(d, pair);
    l = &pair;
  } else if (call == 2) {
    rc = conv_act_decide(d, VT_ACT_RELU, a, p);
  } else {
    rc = conv_decide(d, a, p);
    if (rc == VT_OK && splitk_runs(p, a, d, true)) {
      l = &p.part;
      rc = p.part_rc;
    }
  }
  if (rc != VT_OK) return rc;
  std::fill(out16, out16 + 16, (int64_t)0);
  if (call != 1 && p.kernel != CONV_IGEMM) {
    out16[0] = p.kernel;
    return VT_OK;
  }
  const ConvArgs& f = l->a;
  const IgemmVariant& v = l->v;
  const int64_t out[16] = {CONV_IGEMM, l->buf ? 1 : 0, f.x_bytes, f.w_bytes, f.c_bytes, f.tskip, f.hw_tiles, f.lds_epi, f.nsteps, f.m_tiles, f.n_tiles,
                           l->grid_z, f.ksplit, l->sched, l->lds_bytes, (int)v.tile | ((v.fast ? 1 : 0) << 4) | (v.ln256 << 8) | (v.stages << 12) | (v.rowb << 16)};
  std::copy(out, out + 16, out16);
  return VT_OK;
}
