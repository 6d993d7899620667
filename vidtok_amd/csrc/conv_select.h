// Which kernel / tile / epilogue / ring a vt_conv call gets, and the form of its implicit-GEMM launches.  conv_decide makes the decision ONCE
// per call, as a ConvPlan: vt_conv runs the plan, vt_conv_plan and vt_conv_launch_form report it, vt_conv_work_bytes / vt_conv_profile /
// vt_conv_act read it (conv_igemm.hip), and the per-type translation units that hold the kernel instantiations
// (conv_igemm_{f32,bf16,f16,x3,act}.hip) switch on an IgemmLaunch's variant and launch it as it stands.  The *_eligible predicates are pure
// functions of the descriptor (ConvArgs) and of the option table; conv_decide is their only caller -- but for tup3_eligible, the rule of the
// paired time up-sampler launch, which vt_time_upsample3 / vt_time_upsample3_supported apply to conv_decide's result.  igemm_launch_form is
// the one place that fills in the rest of a launch: gather form, tile walk, skipped taps, K steps, schedule, LDS.
#pragma once
#include "conv_common.h"

namespace {

// Test / A-B switches of the option table (options.h; vt_set_option, seeded once from VT_<NAME> -- no launch path reads the environment):
//   conv_buf = 0      gather through 64-bit pointers (global_load_lds) instead of buffer descriptors
//   conv_tinner = 0   plain pixel order for temporal convs
//   conv_tile = 256   force the 8-wave 256x256 tile wherever it is legal (Cout % 256 == 0, vector epilogue), however
//                     few tiles that gives; = 128 forbids it -- lets small parity cases reach either instantiation
inline bool conv_buf() { return vt_opt(OPT_CONV_BUF) != 0; }
inline bool conv_tinner() { return vt_opt(OPT_CONV_TINNER) != 0; }

// Bytes of the tensors a launch gathers from, as a buffer descriptor would have to hold them: x [B][Ti][Hi][Wi][Cin], the weight rows
// [Cout][ldw], the cache [B][ncache][Hi][Wi][Cin] (cache mode; else 0).  A descriptor takes an extent below 4 GiB minus the out-of-range
// marker (the kernels' kOob offset, which the hardware answers with zeros).
struct GatherExtents {
  unsigned long long x, w, c;
};
inline GatherExtents gather_extents(const ConvArgs& a, int elem_bytes) {
  const unsigned long long pix = (unsigned long long)a.Hi * a.Wi * a.Cin * elem_bytes;
  return {(unsigned long long)a.B * a.Ti * pix, (unsigned long long)a.Cout * a.ldw * elem_bytes,
          a.tmode == VT_TPAD_CACHE ? (unsigned long long)a.B * a.ncache * pix : 0ull};
}
inline bool desc_holds(unsigned long long bytes) { return bytes < 0xFFFF0000ull; }

// conv_in8_kernel (conv_in8.hip): the encoder's conv_in in a 16-bit type
inline bool in8_eligible(const ConvArgs& a, int nbatch, int dtype, int out_dtype, bool ln_fused, int ln_mode_asked) {
  if (vt_opt(OPT_CONV_IN8) == 0 || !conv_buf() || nbatch != 1 || a.prof != nullptr) return false;
  if (!vt_is_h16(dtype) || out_dtype != dtype || a.Cin != 8 || a.Cout != 128 || a.ldw != 216) return false;
  if (a.KT != 3 || a.KH != 3 || a.KW != 3 || a.st != 1 || a.sh != 1 || a.sw != 1 || a.pt != 2 || a.ph != 1 || a.pw != 1) return false;
  if (a.To != a.Ti || a.Ho != a.Hi || a.Wo != a.Wi || a.ups_t || a.ups_s || a.tmode == VT_TPAD_CACHE) return false;
  if (a.out_layout != VT_NDHWC || a.res_mode != VT_RES_NONE || a.yt_mul != 1 || a.ys_mul == 2) return false;
  // a tile = a 128-pixel segment of one row, or 128 / Wo whole rows, inside one frame
  if (a.Wo < 8 || !((a.Wo % 128 == 0) || (128 % a.Wo == 0)) || ((long long)a.Ho * a.Wo) % 128 != 0) return false;
  if (ln_mode_asked != 0 && !ln_fused) return false;                                            // the LayerNorm belongs to the epilogue or to nobody
  if (a.ldy % 8 != 0 || (a.ln_mode != 0 && a.ldn % 8 != 0) || vt_opt(OPT_CONV_LDSEPI) == 0) return false;   // the epilogue's 16-byte rows
  return desc_holds(gather_extents(a, 2).x);
}

// 128 x 128 tile on a 4-slot ring (128 KB of LDS, three K steps of DMA in flight instead of one).  Two workgroups per CU
// cover each other's DMA latency; a launch with no more tiles than CUs leaves every workgroup alone on its CU, and with
// one step of look-ahead its K step then lasts one fabric round trip (the deep layers of a v1.1 chunk, M = 4 096 / 5 120
// at 512 channels and K = 13 824: ~1 600 cycles per step against 512 of MFMA work).  Alone on the CU it can have the LDS.
inline bool deep_ring_eligible(const ConvArgs& a, int nbatch, int elem_bytes) {
  if (vt_opt(OPT_CONV_DEEP) == 0 || a.prof != nullptr) return false;
  const int bk = kRowBytes / elem_bytes;
  if (a.Cin % bk != 0 || a.ntaps * (a.Cin / bk) < 8) return false;              // descriptor-walk form only; a K worth the ring
  const long long tiles = (long long)((a.M + 127) / 128) * ((a.Cout + 127) / 128) * nbatch;
  return tiles <= device_cus();
}

// Tile selection.  Bytes staged per FLOP fall with the tile area (128x128: 15.6 KB/MFLOP bf16, 256x256: 7.8),
// so Cout % 256 == 0 layers with enough pixels take the 8-wave 256x256 tile (measured 988 vs 814 TFLOP/s on
// the 27-tap 256->256 conv when introduced); everything else keeps 128x128 with two independent workgroups
// per CU, which cover each other's prologue / epilogue / DMA stalls (256x128 tiles measured slower).
enum TileKind { TILE_256x32 = 0, TILE_256x64, TILE_256x256, TILE_128x128 };
// waves along pixels / channels and 32 x 32 MFMA blocks per wave of each tile: the template arguments of its instantiations (launch_tile,
// conv_igemm_kernel.h) and the tile dimensions vt_conv_plan reports are both read from here
struct TileShape {
  int wm, wn, tm, tn;
  constexpr int bm() const { return wm * tm * 32; }
  constexpr int bn() const { return wn * tn * 32; }
  constexpr int waves() const { return wm * wn; }
};
constexpr TileShape kTileShapes[4] = {{4, 1, 2, 1}, {4, 1, 2, 2}, {4, 2, 2, 4}, {2, 2, 2, 2}};

// Weight-stationary persistent kernel (conv_ws2.hip): 3x3 stride-1 pad-1 convolutions in a 16-bit type with Cin = Cout = 128 on
// frames that tile by 8 x 16 pixels -- the nine ResnetBlock convolutions of the widest level.  Option conv_ws = 0 keeps them
// on the tile-per-workgroup kernel (A/B runs, and the parity tests run both).
inline bool ws_eligible(const ConvArgs& a, int nbatch, bool h16_io) {
  if (!h16_io || vt_opt(OPT_CONV_WS) == 0) return false;
  if (a.Cin != 128 || a.Cout != 128 || a.ldw != 1152 || a.ldy != 128) return false;
  if (a.KT != 1 || a.KH != 3 || a.KW != 3 || a.st != 1 || a.sh != 1 || a.sw != 1 || a.ph != 1 || a.pw != 1) return false;
  if (a.ups_t || a.ups_s || a.Ho != a.Hi || a.Wo != a.Wi || a.To != a.Ti) return false;
  if (a.Ho % 8 != 0 || a.Wo % 16 != 0 || (long long)a.Ho * a.Wo * 256 > (1ll << 30)) return false;
  if (a.out_layout != VT_NDHWC || a.yt_mul != 1 || a.ys_mul == 2 || nbatch != 1) return false;
  if (a.res_mode == VT_RES_MIX) return false;
  if (a.res_mode == VT_RES_ADD && (a.ldr != 128 || a.Tr != a.To || a.res_tshift != 0 || (reinterpret_cast<uintptr_t>(a.res) & 15))) return false;
  if ((reinterpret_cast<uintptr_t>(a.y) & 15) || (a.bias && (reinterpret_cast<uintptr_t>(a.bias) & 15))) return false;
  return true;
}

// Narrow-output 3x3x3 convolution (conv_narrow.hip): 16-bit (or split-bf16) in, fp32 NCTHW out, Cin = 128, Cout <= 4 -- the decoder's
// conv_out (reference model_3dcausal.py:862-870).  Option conv_narrow = 0 keeps it on the 256 x 32 implicit-GEMM tile.
inline bool narrow_eligible(const ConvArgs& a, int nbatch, int dtype, int out_dtype, int ln_mode) {
  if ((!vt_is_h16(dtype) && dtype != VT_BF16X3) || out_dtype != VT_F32 || a.out_layout != VT_NCTHW || vt_opt(OPT_CONV_NARROW) == 0) return false;
  if (a.Cin != 128 || a.Cout > 4 || a.KT != 3 || a.KH != 3 || a.KW != 3) return false;
  if (a.st != 1 || a.sh != 1 || a.sw != 1 || a.ph != 1 || a.pw != 1 || a.pt < 1 || a.pt > 2) return false;
  if (a.ups_t || a.ups_s || a.Ho != a.Hi || a.Wo != a.Wi || a.To != a.Ti) return false;
  if (a.res_mode != VT_RES_NONE || ln_mode != 0 || nbatch != 1 || a.yt_mul != 1 || a.ys_mul == 2) return false;
  if ((long long)a.Ho * a.Wo * 256 > (1ll << 30)) return false;
  if (a.tmode == VT_TPAD_CACHE && a.ncache < a.pt) return false;
  if (dtype == VT_BF16X3 && a.ldw != 27 * 128) return false;      // the planes are addressed as [K / 16][hi 16 | lo 16], K = 3 456
  return true;
}

// the 8-wave 256 x 256 tile for a layer of `tiles` such tiles: at least conv_tile_min (default 128), or forced / forbidden by conv_tile
inline bool tile256_wanted(long long tiles) {
  const int force = vt_opt(OPT_CONV_TILE);
  return force != 128 && (tiles >= vt_opt(OPT_CONV_TILE_MIN) || force == 256);
}

// the gather through buffer descriptors (option conv_buf): both operands below 4 GiB minus the out-of-range marker
inline bool desc_gather_fits(const ConvArgs& a, int elem_bytes) {
  const GatherExtents e = gather_extents(a, elem_bytes);
  return conv_buf() && desc_holds(e.x) && desc_holds(e.w);
}

inline TileKind select_tile(const ConvArgs& a, int nbatch) {
  auto blocks = [&](int bm, int bn) {
    return (long long)((a.M + bm - 1) / bm) * ((a.Cout + bn - 1) / bn) * nbatch;
  };
  const bool vec_epi = a.out_layout == VT_NDHWC && (a.ldy & 3) == 0 && (a.res_mode == VT_RES_NONE || (a.ldr & 3) == 0);
  if (a.Cout <= 32) return TILE_256x32;
  if (a.Cout <= 64) return TILE_256x64;
  // at least conv_tile_min (default 128) tiles: with the scheduled K loops even half-filled single rounds of the 8-wave
  // tile beat 1.25 rounds of 128 x 128 tiles (M = 20 480, Cout = 512: 0.143 -> 0.121 ms at K = 4 608, 0.38 -> 0.29 at 13 824)
  if (a.Cout % 256 == 0 && vec_epi && tile256_wanted(blocks(256, 256))) return TILE_256x256;
  return TILE_128x128;
}

// 8-wave tile, no LayerNorm, but everything the LDS-transposed epilogue needs (conv_epilogue_lds256 with ln_mode = 0):
// a 16-bit type, full tiles, plain NDHWC rows, a residual / mix operand indexed like the output
inline bool lds256_plain_eligible(const ConvArgs& a, int nbatch, bool h16_io) {
  return h16_io && a.ln_mode == 0 && a.prof == nullptr && vt_opt(OPT_CONV_LDSEPI) != 0 &&
         a.M % 256 == 0 && a.Cout % 256 == 0 && nbatch == 1 && a.Cin % (kRowBytes / 2) == 0 && a.out_layout == VT_NDHWC &&
         (a.ldy & 7) == 0 && (a.res_mode == VT_RES_NONE || ((a.ldr & 7) == 0 && a.Tr == a.To && a.res_tshift == 0));
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
// Which instantiation of conv_igemm_glds_kernel a launch gets (launch_variant's template arguments beyond the types)
struct IgemmVariant {
  TileKind tile;
  bool fast;    // tap-walk form (Cin a multiple of the K step); false: the general gather
  int ln256;    // 8-wave tile: the LDS-transposed epilogue conv_epilogue_lds256 (fused LayerNorm, or plain rows with ln_mode = 0)
  int stages;   // ring slots: 2, or 4 (the deep ring of the 128 x 128 tile; split-bf16 on the 8-wave tile)
  int rowb;     // bytes of K per tile row per step: kRowBytes, or 64 (split-bf16 on the 8-wave tile)
};

enum ConvKernel { CONV_IGEMM = 0, CONV_NARROW = 2, CONV_WS2 = 3, CONV_IN8 = 4 };   // out8[6] of vt_conv_plan; 1 (conv_ws128, gone) stays reserved

// K-step schedule of an instantiation on descriptors (see the kernel): the 8-wave tile's tap-walk form runs 16-bit operands on 2 (two-group
// ping-pong), fp32 operands on 1 (software-pipelined single body), split-bf16 on its 64-byte-row ring on 5; everything else -- the 4-wave
// tiles, the general (non tap-walk) form, and every pointer-form launch -- runs the plain loop 0.  (Earlier rounds kept every schedule
// selectable: their measurements are in DESIGN section 6, the instantiations are gone.)  launch_variant instantiates by this function.
constexpr int igemm_sched(TileKind tile, bool fast, int dtype, int rowb, int stages) {
  if (tile != TILE_256x256 || !fast) return 0;
  if (dtype == VT_BF16X3) return (rowb == 64 && stages == 4) ? 5 : 0;
  if (rowb != kRowBytes || stages != 2) return 0;
  return (dtype == VT_BF16 || dtype == VT_F16) ? 2 : 1;
}

// One implicit-GEMM launch, complete: launch_variant (conv_igemm_kernel.h) picks the kernel pointer of `v` and launches `a` as it stands.
// `a` is a COPY of the ConvArgs conv_decide returns, taken when the form is computed: what a caller writes into its own ConvArgs afterwards
// never reaches the launch.  Whatever the kernel has to see is set before igemm_launch_form runs (conv_decide's parameters), or written
// into the launch's own `a` (vt_time_upsample3's V operand).
struct IgemmLaunch {
  ConvArgs a;      // the kernel's arguments, launch-form fields included (m_tiles, n_tiles, nsteps, lds_epi, hw_tiles, tskip, *_bytes)
  IgemmVariant v;
  int grid_z;      // nbatch, or the tap planes of split-K
  bool buf;        // gather through buffer descriptors (a.x_bytes / w_bytes / c_bytes are their extents); false: 64-bit pointers
  int sched;       // K-step schedule the launch runs
  int lds_bytes;   // dynamic LDS: the ring (+ the stamp area of vt_conv_profile)
};

// The form of the launch of `a_in` in instantiation `v` on grid z `grid_z`: everything about it that is not the choice of kernel, tile and
// epilogue -- a pure function of its arguments and the option table.  dtype / out_dtype: arithmetic and result type (vt_dtype).
inline int igemm_launch_form(IgemmLaunch& l, const ConvArgs& a_in, const IgemmVariant& v, int grid_z, int dtype, int out_dtype) {
  const TileShape& t = kTileShapes[v.tile];
  const int BM = t.bm(), BN = t.bn(), elem = vt_is_h16(dtype) ? 2 : 4, BK = v.rowb / elem;   // split-bf16 steps over fp32 storage
  l.a = a_in;
  l.v = v;
  l.grid_z = grid_z;
  ConvArgs& a = l.a;
  a.m_tiles = (a.M + BM - 1) / BM;
  a.n_tiles = (a.Cout + BN - 1) / BN;
  a.nsteps = v.fast ? a.ntaps * (a.Cin / BK) : (a.K + BK - 1) / BK;
  if (a.ksplit) {
    VT_CHECK_ARG(v.fast, "vt_conv: split-K needs the tap-walk form");
    a.nsteps = (a.ksplit == 1 ? a.KH * a.KW : a.KW) * (a.Cin / BK);
  }
  const int oct_align = vt_is_h16(out_dtype) ? 8 : 4;   // elements per 16 bytes of the result type, at least a quad
  a.lds_epi = (vt_opt(OPT_CONV_LDSEPI) != 0 && a.out_layout == VT_NDHWC && a.ldy % oct_align == 0 &&
               (a.res_mode == VT_RES_NONE || a.ldr % oct_align == 0) && (a.ln_mode == 0 || a.ldn % oct_align == 0)) ? 1 : 0;
  // Temporal taps: in pixel order (b,t,h,w) the frames t-1, t-2 a tile reads were last touched one whole frame of
  // tiles earlier -- far beyond the 4 MiB L2 of its XCD -- so every kt tap came from the fabric again (the k3
  // temporal conv of the widest level moved 3x its input).  Walking the tiles as (b, hw tile, t) puts the
  // producers of those lines right before their consumer on the same XCD (xcd_remap keeps the sequence
  // contiguous): 298 -> 340 TFLOP/s on that layer, +3 % on the 27-tap up-sampler conv (same-run A/B).
  const long long hw = (long long)a.Ho * a.Wo;
  const bool tile_in_frame = hw % BM == 0;
  a.hw_tiles = (conv_tinner() && a.KT > 1 && a.To > 1 && tile_in_frame) ? (int)(hw / BM) : 0;
  // cache mode (v1.1 chunks after the first): descriptors only where a tile lies in one output frame, so that a time tap reads
  // the cache or x for the whole tile (the kernel switches the descriptor per tap); other shapes gather through pointers
  const GatherExtents e = gather_extents(a, elem);
  const bool alone = grid_z == 1 || a.ksplit;          // the tile index is a pixel index of the one tensor the descriptors hold
  const bool cache_ok = a.tmode != VT_TPAD_CACHE || (v.fast && alone && a.prof == nullptr && desc_holds(e.c) && tile_in_frame && a.ups_t == 0);
  l.buf = desc_gather_fits(a, elem) && cache_ok && a.KH <= 8 && a.KW <= 8;   // the per-row padding mask of the tap walk holds 8 bits per axis
  VT_CHECK_ARG(!a.ksplit || l.buf, "vt_conv: split-K needs the descriptor gather");
  // the paired launch exists on descriptors only (tup3_eligible asks for them); no pointer-form instantiation
  VT_CHECK_ARG(v.ln256 != 2 || l.buf, "vt_time_upsample3: the descriptor gather is required (option conv_buf, tensors below 4 GiB)");
  a.x_bytes = l.buf ? (unsigned)e.x : 0u;
  a.w_bytes = l.buf ? (unsigned)e.w : 0u;
  a.c_bytes = l.buf ? (unsigned)e.c : 0u;
  // zero-padded time taps skipped per tile: the tap-walk form on descriptors, a tile inside one output frame
  a.tskip = (v.fast && l.buf && vt_opt(OPT_CONV_TSKIP) != 0 && a.tmode == VT_TPAD_ZERO && a.KT > 1 && a.pt > 0 && a.ups_t == 0 && !a.ksplit &&
             grid_z == 1 && a.prof == nullptr && tile_in_frame) ? 1 : 0;
  l.sched = l.buf ? igemm_sched(v.tile, v.fast, dtype, v.rowb, v.stages) : 0;
  l.lds_bytes = v.stages * (BM + BN) * v.rowb + (a.prof != nullptr ? 4096 : 0);
  return VT_OK;
}

// the ConvArgs of split-K's partial launch: grid z = tap plane, each plane's walk into its fp32 plane of the scratch `work`; bias, residual
// and rounding belong to the reduction (launch_splitk, conv_igemm.hip)
inline ConvArgs splitk_partial_args(const ConvArgs& a, void* work) {
  ConvArgs s = a;
  s.ksplit = a.KT == 3 ? 1 : 2;
  s.plane_bytes = (unsigned)((a.KT == 3 ? a.KH * a.KW : a.KW) * a.Cin * 2);
  s.y = reinterpret_cast<char*>(work);
  s.bias = nullptr;
  s.res = nullptr; s.res_mode = VT_RES_NONE;
  s.ln_mode = 0;
  s.xs_z = 0; s.ws_z = 0; s.rs_z = 0;
  s.ys_z = (long long)a.M * a.ldy;
  return s;
}

struct ConvPlan {
  ConvKernel kernel;
  IgemmLaunch whole;    // CONV_IGEMM: the whole launch ...
  IgemmLaunch part;     // ... and the tap-plane launch of split-K (splitk_planes > 0): its grid z counts as nbatch in the rules
  int part_rc;          //     VT_ERR_ARG where that launch has no form (its error text is set): returned only by a call that would run it
  int splitk_planes;    // the geometry rule only (0 = none); whether the call HAS the scratch is splitk_runs (conv_igemm.hip)
  bool ln_fused;        // the LayerNorm the descriptor asks for comes from the conv kernel's epilogue
  int nbatch;
  int narrow_mode;      // CONV_NARROW: 0 bf16, 1 fp16, 2 split-bf16 (fp32 x, two passes)
};

// how many tap planes vt_conv would split `a` into (0 = no split): a 16-bit type, 3 taps in time at stride 1 or the 3 rows of a 3 x 3,
// K long, few pixels PER CLIP, plain NDHWC rows, residual add at most; `tile` = what the unsplit launch selects
inline int splitk_planes(const vt_conv_desc* d, const ConvArgs& a, const ConvPlan& p, TileKind tile) {
  if (vt_opt(OPT_CONV_SPLITK) == 0 || !conv_buf()) return 0;
  if (!vt_is_h16(d->dtype) || d->out_dtype != d->dtype || p.nbatch != 1 || p.ln_fused || a.prof != nullptr) return 0;
  const bool by_kt = a.KT == 3 && a.st == 1, by_kh = a.KT == 1 && a.KH == 3;      // three planes: the time taps, or the rows of a 3 x 3
  if (!(by_kt || by_kh) || a.ups_t || a.ups_s || a.out_layout != VT_NDHWC || a.yt_mul != 1 || a.ys_mul == 2) return 0;
  if (a.Cin % 64 != 0 || a.Cout % 128 != 0 || a.ldy != a.Cout || a.KT * a.KH * a.KW * a.Cin < 4608) return 0;
  if (a.res_mode == VT_RES_MIX || (a.res_mode == VT_RES_ADD && (a.ldr != a.Cout || a.Tr != a.To || a.res_tshift != 0))) return 0;
  if (a.tmode == VT_TPAD_CACHE && ((long long)a.Ho * a.Wo) % 256 != 0) return 0;     // the descriptor form of the cache gather: a tile inside one frame
  const GatherExtents e = gather_extents(a, 2);
  if (!desc_holds(e.x) || !desc_holds(e.w)) return 0;
  if (tile != TILE_256x256 && tile != TILE_128x128) return 0;
  // The decision is a function of ONE CLIP's geometry (To, Ho, Wo, Cout, K) and never of B: a split launch sums its tap planes in
  // another order than a whole one, so a rule that looked at the launch's pixel count (round 4: "no more tiles than CUs") tied a
  // clip's bits to the batch it was part of.  A clip whose pixels make no more 128 x 128 tiles than the device has CUs splits --
  // alone it would leave every workgroup by itself on a CU walking the whole K -- whatever the batch around it.
  const long long clip_tiles = (((long long)a.To * a.Ho * a.Wo + 127) / 128) * ((a.Cout + 127) / 128);
  return clip_tiles <= device_cus() ? 3 : 0;
}

// Paired launch of the three-product time up-sampler (vt_time_upsample3; conv_epilogue_lds256_pair): is the parity descriptor `d` --
// already validated by conv_decide into (a, p) -- served?  Like splitk_planes a function of ONE CLIP's geometry, the type and the
// options, never of B: the paired launch rounds V = W1 x once more than the two parity launches, so a rule that counted the launch's
// tiles would tie a clip's bits to its batch.  16-bit storage = arithmetic type; the even-frame parity descriptor (k = 2 in time over
// 3 x 3, causal zero padding, alpha-mix against x, frames interleaved by 2); the 256 x 256 tile in the tap-walk form on buffer
// descriptors with the LDS epilogue's 16-byte rows; a tile inside one frame (the epilogue reads V[j-1] / V[j] and "first frame of the
// clip" per tile).  A LayerNorm is taken exactly where conv_decide fuses it into an alpha-mix launch (Cout = 256, option conv_tup_ln);
// one it does not fuse never gets here (conv_decide rejects the LayerNorm of an interleaved output outside an epilogue).
inline bool tup3_eligible(const vt_conv_desc* d, const ConvArgs& a, const ConvPlan& p) {
  if (vt_opt(OPT_CONV_TUP3) == 0 || a.prof != nullptr) return false;
  const bool h16_io = vt_is_h16(d->dtype) && d->out_dtype == d->dtype;
  if (a.KT != 2 || a.KH != 3 || a.KW != 3 || a.st != 1 || a.sh != 1 || a.sw != 1 || a.pt != 1 || a.ph != 1 || a.pw != 1) return false;
  if (a.tmode != VT_TPAD_ZERO || a.ups_t || a.ups_s || a.To != a.Ti || a.Ho != a.Hi || a.Wo != a.Wi) return false;
  if (a.yt_mul != 2 || a.yt_base != 0 || a.ys_mul == 2 || a.res_mode != VT_RES_MIX) return false;
  if (d->ln_mode != 0 && (!p.ln_fused || (a.ldn & 7) != 0)) return false;
  // the LDS epilogue's own conditions (16-bit rows of 16 bytes, full tiles, the tap walk, the mix operand indexed like the result) ...
  ConvArgs e = a;
  e.ln_mode = 0;
  if (!lds256_plain_eligible(e, p.nbatch, h16_io)) return false;
  // ... on descriptors (igemm_launch_form refuses the paired instantiation otherwise), a tile inside one frame, and the 8-wave tile by
  // select_tile's rule applied to one clip's pixels
  const long long hw = (long long)a.Ho * a.Wo;
  if (!desc_gather_fits(a, 2) || hw % 256 != 0) return false;
  return tile256_wanted((a.To * hw / 256) * (a.Cout / 256));
}

// vt_conv's decision, made once: argument validation, the kernel's view of the descriptor (`a`) and the plan, in the order vt_conv applies
// it -- ws2, narrow, in8, then the implicit GEMM with its tile, variant and split-K geometry.  `prof`: vt_conv_profile's stamp buffer (the
// rules that read a.prof see it); `act`: vt_conv_act's activation, which has its own tile rule and only the implicit GEMM (conv_igemm_act.hip)
inline int conv_decide(const vt_conv_desc* d, ConvArgs& a, ConvPlan& p, unsigned long long* prof = nullptr, int act = 0) {
  VT_CHECK_ARG(d != nullptr, "vt_conv: null descriptor");
  VT_CHECK_ARG(d->x && d->w && d->y, "vt_conv: null tensor pointer");
  VT_CHECK_ARG(d->dtype == VT_F32 || d->dtype == VT_BF16 || d->dtype == VT_F16 || d->dtype == VT_BF16X3, "vt_conv: dtype %d", d->dtype);
  VT_CHECK_ARG((d->out_dtype == d->dtype && d->dtype != VT_BF16X3) || d->out_dtype == VT_F32, "vt_conv: out_dtype %d with dtype %d",
               d->out_dtype, d->dtype);
  const int vec = vt_is_h16(d->dtype) ? 8 : 4;
  if (d->dtype == VT_BF16X3)    // split weight planes: [hi 16 x bf16 | lo 16 x bf16] per 16 k-values, K padded to the block
    VT_CHECK_ARG(d->ldw % 32 == 0 && d->ldw >= (d->KT * d->KH * d->KW * d->Cin + 31) / 32 * 32 && d->nbatch <= 1,
                 "vt_conv: VT_BF16X3 needs ldw = K rounded up to 32 (got %d) and nbatch 1", d->ldw);
  VT_CHECK_ARG(d->B > 0 && d->Ti > 0 && d->Hi > 0 && d->Wi > 0 && d->Cin > 0, "vt_conv: bad input dims");
  VT_CHECK_ARG(d->To > 0 && d->Ho > 0 && d->Wo > 0 && d->Cout > 0, "vt_conv: bad output dims");
  VT_CHECK_ARG(d->Cin % vec == 0, "vt_conv: Cin=%d must be a multiple of %d (pad the channel dim)", d->Cin, vec);
  VT_CHECK_ARG(d->KT > 0 && d->KH > 0 && d->KW > 0 && d->KT * d->KH * d->KW <= 64, "vt_conv: bad taps");
  VT_CHECK_ARG(d->st > 0 && d->sh > 0 && d->sw > 0, "vt_conv: bad strides");
  VT_CHECK_ARG(d->ldw >= d->KT * d->KH * d->KW * d->Cin && d->ldw % vec == 0, "vt_conv: ldw=%d", d->ldw);
  VT_CHECK_ARG((reinterpret_cast<uintptr_t>(d->x) & 15) == 0 && (reinterpret_cast<uintptr_t>(d->w) & 15) == 0,
               "vt_conv: x / w must be 16-byte aligned");
  VT_CHECK_ARG(d->ups_t == 0 || d->ups_t == 1, "vt_conv: ups_t");
  VT_CHECK_ARG(d->ups_s == 0 || d->ups_s == 1, "vt_conv: ups_s");
  VT_CHECK_ARG(d->tmode >= VT_TPAD_ZERO && d->tmode <= VT_TPAD_CACHE, "vt_conv: tmode %d", d->tmode);
  if (d->tmode == VT_TPAD_CACHE && d->pt > 0) {
    VT_CHECK_ARG(d->cache != nullptr && d->ncache >= d->pt, "vt_conv: cache mode needs cache with >= pt frames");
    VT_CHECK_ARG(d->ups_t == 0, "vt_conv: cache mode with ups_t");
    VT_CHECK_ARG((reinterpret_cast<uintptr_t>(d->cache) & 15) == 0, "vt_conv: cache must be 16-byte aligned");
  }
  VT_CHECK_ARG(d->res_mode >= VT_RES_NONE && d->res_mode <= VT_RES_MIX, "vt_conv: res_mode %d", d->res_mode);
  if (d->res_mode != VT_RES_NONE) {
    VT_CHECK_ARG(d->res != nullptr && d->Tr > 0 && d->ldr >= d->Cout, "vt_conv: residual operand");
    VT_CHECK_ARG(((d->To - 1) >> d->res_tshift) < d->Tr, "vt_conv: residual time extent");
  }
  if (d->res_mode == VT_RES_MIX) VT_CHECK_ARG(d->mix_factor != nullptr, "vt_conv: mix_factor is null");
  if (d->out_layout == VT_NCTHW) {
    VT_CHECK_ARG(d->out_dtype == VT_F32, "vt_conv: NCTHW output is fp32 only");
    VT_CHECK_ARG(d->t_trim >= 0 && d->t_trim < d->To, "vt_conv: t_trim");
  } else {
    VT_CHECK_ARG(d->out_layout == VT_NDHWC && d->ldy >= d->Cout, "vt_conv: ldy=%d < Cout=%d", d->ldy, d->Cout);
  }
  const long long M = (long long)d->B * d->To * d->Ho * d->Wo;
  VT_CHECK_ARG(M < (1ll << 31), "vt_conv: M too large");
  const int nbatch = d->nbatch > 0 ? d->nbatch : 1;
  const int yt_mul = d->yt_mul > 0 ? d->yt_mul : 1;
  if (yt_mul != 1)
    VT_CHECK_ARG(d->out_layout == VT_NDHWC && nbatch == 1 && d->yt_off >= 0 && d->yt_off < yt_mul,
                 "vt_conv: output frame interleave needs NDHWC, nbatch 1 and 0 <= yt_off < yt_mul");
  const int ys_mul = d->ys_mul == 2 ? 2 : 1;
  VT_CHECK_ARG(d->ys_mul == 0 || d->ys_mul == 1 || d->ys_mul == 2, "vt_conv: ys_mul %d", d->ys_mul);
  if (ys_mul == 2)
    VT_CHECK_ARG(d->out_layout == VT_NDHWC && nbatch == 1 && yt_mul == 1 && (d->ys_oh | d->ys_ow | 1) == 1,
                 "vt_conv: output pixel interleave needs NDHWC, nbatch 1, no frame interleave, offsets in {0,1}");
  if (d->ln_mode != 0) {
    VT_CHECK_ARG(d->ln_mode == 1 || d->ln_mode == 2, "vt_conv: ln_mode %d", d->ln_mode);
    VT_CHECK_ARG(d->ln_gamma && d->ln_beta && d->ln_out, "vt_conv: fused LayerNorm needs gamma, beta and ln_out");
    VT_CHECK_ARG(d->out_layout == VT_NDHWC && nbatch == 1 && d->ldn >= d->Cout, "vt_conv: fused LayerNorm: NDHWC, nbatch 1, ldn >= Cout");
  }

  memset(&a, 0, sizeof(a));
  a.x = (const char*)d->x; a.w = (const char*)d->w; a.bias = d->bias; a.y = (char*)d->y;
  a.res = (const char*)d->res; a.cache = (const char*)d->cache; a.mix_factor = d->mix_factor;
  a.B = d->B; a.Ti = d->Ti; a.Hi = d->Hi; a.Wi = d->Wi; a.Cin = d->Cin;
  a.To = d->To; a.Ho = d->Ho; a.Wo = d->Wo; a.Cout = d->Cout;
  a.ldw = d->ldw; a.ldy = d->ldy;
  a.KT = d->KT; a.KH = d->KH; a.KW = d->KW;
  a.st = d->st; a.sh = d->sh; a.sw = d->sw;
  a.pt = d->pt; a.ph = d->ph; a.pw = d->pw;
  a.tmode = d->tmode; a.ncache = d->ncache;
  a.ups_t = d->ups_t; a.ups_s = d->ups_s;
  a.res_mode = d->res_mode; a.res_tshift = d->res_tshift;
  a.Tr = d->res_mode != VT_RES_NONE ? d->Tr : d->To;
  a.ldr = d->ldr;
  // streaming (nt) stores of the LDS epilogues' rows for outputs far larger than the caches (option conv_nt_mb, MiB; 0 = never)
  a.nt_store = (vt_opt(OPT_CONV_NT_MB) > 0 && M * d->Cout * (vt_is_h16(d->out_dtype) ? 2 : 4) >= ((long long)vt_opt(OPT_CONV_NT_MB) << 20)) ? 1 : 0;
  a.out_layout = d->out_layout; a.t_trim = d->t_trim;
  a.M = (int)M; a.ntaps = d->KT * d->KH * d->KW; a.K = a.ntaps * d->Cin;
  a.ys_mul = ys_mul; a.ys_oh = d->ys_oh; a.ys_ow = d->ys_ow;
  a.yt_mul = yt_mul;
  a.yt_step = (long long)(yt_mul - 1) * d->Ho * d->Wo;
  a.yt_base = (long long)(yt_mul != 1 ? d->yt_off : 0) * d->Ho * d->Wo;
  a.fd_hw = make_fastdiv((unsigned)(d->Ho * d->Wo));
  a.fd_wo = make_fastdiv((unsigned)d->Wo); a.fd_ho = make_fastdiv((unsigned)d->Ho); a.fd_to = make_fastdiv((unsigned)d->To);
  a.xs_z = d->xs_z; a.ws_z = d->ws_z; a.ys_z = d->ys_z; a.rs_z = d->rs_z;

  a.prof = prof;
  a.prof_mode = prof != nullptr ? vt_opt(OPT_WS_PROF_MODE) : 0;
  p = ConvPlan{};        // CONV_IGEMM, no split, nothing fused
  p.nbatch = nbatch;

  const bool h16 = vt_is_h16(d->dtype), h16_io = h16 && d->out_dtype == d->dtype;
  const int elem = h16 ? 2 : 4;
  // vt_conv_act has its own tile rule (conv_igemm_act.hip holds the 256 x 64, 256 x 256 and 128 x 128 tiles only)
  auto tile_for = [&](const ConvArgs& c, int nb) {
    if (act == 0) return select_tile(c, nb);
    return c.Cout <= 64 ? TILE_256x64 : (c.Cout % 256 == 0 && (c.ldy & 3) == 0) ? TILE_256x256 : TILE_128x128;
  };
  // the instantiation of tile `t` the implicit-GEMM kernel runs `c` in; same_type: results stored in the arithmetic's own storage type
  auto variant = [&](const ConvArgs& c, int nb, TileKind t, bool same_type) {
    IgemmVariant v = {t, c.Cin % (kRowBytes / elem) == 0, 0, 2, kRowBytes};
    if (t == TILE_256x256 && d->dtype == VT_BF16X3) {
      // split-bf16: 64-byte rows (one group of 16 k-values per K step) on a 4-slot ring
      if (c.Cin % 16 == 0) v = {t, true, c.ln_mode != 0 ? 1 : 0, 4, 64};
    } else if (t == TILE_256x256 && same_type) {
      // the LayerNorm rule below checked Cin; without LayerNorm the same epilogue gives coalesced stores and residual reads (-8 % on
      // the time up-sampler's parity convolutions, -10 % on the K = 1 024 / 1 536 layers)
      if (c.ln_mode != 0 || (h16 && lds256_plain_eligible(c, nb, true))) v = {t, true, 1, 2, kRowBytes};
    } else if (t == TILE_128x128 && act == 0 && deep_ring_eligible(c, nb, elem)) {
      v = {t, true, 0, 4, kRowBytes};
    }
    return v;
  };
  const TileKind tile = tile_for(a, nbatch);

  // LayerNorm inside the epilogue: the weight-stationary kernel, or the 128 x 128 tile with the LDS epilogue on full tiles spanning the channel row
  const bool ws_ln_ok = d->ln_mode == 0 || (d->ldn == 128 && (reinterpret_cast<uintptr_t>(d->ln_out) & 15) == 0);
  const bool use_ws = act == 0 && ws_ln_ok && ws_eligible(a, nbatch, h16_io);
  p.ln_fused = d->ln_mode != 0 && (use_ws || (d->Cout == 128 && M % 128 == 0 && (d->ldy & 7) == 0 && (d->ldn & 7) == 0 &&
                                              (d->res_mode == VT_RES_NONE || (d->ldr & 7) == 0) && vt_opt(OPT_CONV_LDSEPI) != 0 &&
                                              vt_opt(OPT_CONV_FUSE_LN) != 0));
  // ... or inside the 8-wave 256 x 256 tile's epilogue for Cout = 256 (conv_epilogue_lds256): full tiles, plain rows
  if (d->ln_mode != 0 && !p.ln_fused && d->Cout == 256 && M % 256 == 0 && (d->dtype == VT_BF16X3 ? VT_F32 : d->dtype) == d->out_dtype && nbatch == 1 &&
      d->Cin % (kRowBytes / elem) == 0 && (d->ldy & 7) == 0 && (d->ldn & 7) == 0 &&
      (d->res_mode == VT_RES_NONE || (d->res_mode == VT_RES_ADD && (d->ldr & 7) == 0 && d->Tr == d->To && d->res_tshift == 0) ||
       // alpha-mix + LayerNorm (the consumer's norm behind a time up-sampler's parity launches; option conv_tup_ln)
       (d->res_mode == VT_RES_MIX && (d->ldr & 7) == 0 && d->Tr == d->To && d->res_tshift == 0 && vt_opt(OPT_CONV_TUP_LN) != 0)) &&
      vt_opt(OPT_CONV_FUSE_LN256) != 0 && tile == TILE_256x256)
    p.ln_fused = true;
  if (p.ln_fused) {
    a.ln_gamma = d->ln_gamma; a.ln_beta = d->ln_beta; a.ln_out = (char*)d->ln_out;
    a.ln_mode = d->ln_mode; a.ln_keep_y = d->ln_keep_y; a.ldn = d->ldn; a.ln_eps = d->ln_eps;
  }
  if (d->ln_mode != 0 && !p.ln_fused)
    VT_CHECK_ARG(yt_mul == 1 && ys_mul == 1,
                 "vt_conv: LayerNorm of an interleaved output is only available fused (Cout = 128, full tiles)");

  if (use_ws) {
    p.kernel = CONV_WS2;
  } else if (act == 0 && narrow_eligible(a, nbatch, d->dtype, d->out_dtype, d->ln_mode)) {
    p.kernel = CONV_NARROW;
    p.narrow_mode = d->dtype == VT_BF16X3 ? 2 : (d->dtype == VT_F16 ? 1 : 0);
  } else if (act == 0 && in8_eligible(a, nbatch, d->dtype, d->out_dtype, p.ln_fused, d->ln_mode)) {
    p.kernel = CONV_IN8;
  } else {
    int rc = igemm_launch_form(p.whole, a, variant(a, nbatch, tile, (d->dtype == VT_BF16X3 ? VT_F32 : d->dtype) == d->out_dtype), nbatch,
                               d->dtype, d->out_dtype);
    if (rc != VT_OK) return rc;
    p.splitk_planes = act == 0 ? splitk_planes(d, a, p, tile) : 0;
    if (p.splitk_planes > 0) {   // the partial launch: fp32 planes, no residual, no LayerNorm
      // splitk_planes does not restate every condition of the descriptor gather (a tap axis above 8, a cache of 4 GiB): a partial launch
      // without a form is refused where it would run (launch_splitk) -- a call without the scratch runs the whole launch all the same
      const ConvArgs s = splitk_partial_args(a, d->work);
      p.part_rc = igemm_launch_form(p.part, s, variant(s, p.splitk_planes, tile_for(s, p.splitk_planes), false), p.splitk_planes, d->dtype, VT_F32);
    }
    return VT_OK;
  }
  return VT_OK;
}
}  // namespace

// the per-type translation units (conv_igemm_*.hip): launch of `launch` (an IgemmLaunch) in the instantiation its variant names
// (an instantiation the unit does not hold is VT_ERR_ARG)
extern "C" int vt_igemm_dispatch_f32(const void* launch, void* stream);                  // fp32 -> fp32
extern "C" int vt_igemm_dispatch_x3(const void* launch, void* stream);                   // split-bf16 arithmetic, fp32 storage
extern "C" int vt_igemm_dispatch_bf16(const void* launch, int out_f32, void* stream);    // bf16 -> bf16 | fp32
extern "C" int vt_igemm_dispatch_f16(const void* launch, int out_f32, void* stream);     // fp16 -> fp16 | fp32
extern "C" int vt_igemm_dispatch_relu(const void* launch, int dtype, void* stream);      // conv_igemm_act.hip: + ReLU, in the arithmetic type
extern "C" int vt_ws2_launch(const void* conv_args, int dtype, void* stream);                         // conv_ws2.hip
extern "C" int vt_conv_in8_launch(const void* conv_args, int dtype, void* stream);                    // conv_in8.hip
extern "C" int vt_conv_narrow_launch(const void* conv_args, void* stream, int mode);                  // conv_narrow.hip (mode: 0 bf16, 1 fp16, 2 split-bf16: fp32 x, two passes)
extern "C" void vt_conv_narrow_plan(const void* conv_args, int32_t* plan4);
