/*
 * vidtok_amd.h -- C-ABI of libvidtok_amd.so: the MI355X (gfx950) kernels behind the VidTok
 * causal tokenizer's encode / decode path.
 *
 * The reference (microsoft/VidTok) has no FFI of its own: every operator on the hot path is a
 * torch.nn call.  Each entry point below replaces the ATen operator(s)
 * the reference reaches from the cited file:line, so a maintainer binds them with ctypes
 * (INTEGRATION.md shows the stub) from the Python modules that mirror the reference classes.
 *
 * Conventions
 *   - plain C: pointers are DEVICE pointers unless said otherwise, sizes are element counts;
 *   - every function returns 0 on success, a negative vt_status otherwise; vt_last_error()
 *     returns a thread-local message; nothing throws across the boundary;
 *   - the library never allocates or frees activation memory, never synchronises the stream
 *     and is hipGraph-capture safe (all launches go to the stream argument);
 *   - activation layout is NDHWC ([B][T][H][W][C], C innermost, C stored padded to `ld*`
 *     elements); the public tensors of the reference API are NCTHW fp32 and are converted at
 *     the two ends by vt_ncthw_to_ndhwc / the NCTHW epilogue of vt_conv;
 *   - `dtype` selects the arithmetic: VT_F32 = fp32 storage + fp32-input MFMA
 *     (v_mfma_f32_32x32x2_f32, bit-wise an fmaf chain), VT_BF16 = bf16 storage + bf16 MFMA
 *     (v_mfma_f32_32x32x16_bf16) with fp32 accumulation, VT_F16 = fp16 storage + fp16 MFMA
 *     (v_mfma_f32_32x32x16_f16, the same rate) with fp32 accumulation: what the reference's
 *     README computes in under torch.autocast(device_type="cuda", dtype=torch.float16)
 *     (README.md:336-340,375-385; scripts/inference_*.py --precision autocast).  Results beyond
 *     fp16's range (|v| > 65 504) become +-inf when a tensor is stored, as they do in the
 *     reference's fp16 convolutions.  Every operator that takes VT_BF16 takes VT_F16.
 *     Statistics, softmax, the regularizers and all epilogue arithmetic are fp32 in every mode.
 *     vt_conv additionally takes
 *     VT_BF16X3 ("split-bf16"): fp32 storage (x, cache, y, res, ln_out exactly as for VT_F32,
 *     out_dtype = VT_F32) with the products taken on the bf16 matrix cores from bf16 hi / lo
 *     planes of both operands (x_hi w_hi + x_hi w_lo + x_lo w_hi, fp32 accumulation: ~2^-17
 *     relative per product against 2^-9 for VT_BF16, at 3/16 of the matrix-pipe time of
 *     VT_F32).  Activations are split inside the kernel; the WEIGHTS are handed over already
 *     split: row n of `w` holds, per group of 16 consecutive k, 16 bf16 hi values followed by
 *     16 bf16 lo values (hi = bf16_rne(w), lo = bf16_rne(w - hi)) -- 64 bytes, the size of the
 *     16 fp32 values they replace; rows are zero-padded to whole 128-byte K steps, so ldw (in
 *     4-byte units) = K rounded up to 32
 *     (vidtok_amd/packing.py::pack_split3).  Every other operator of a split-bf16 pass is the
 *     VT_F32 one.
 */
#ifndef VIDTOK_AMD_H
#define VIDTOK_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vt_stream;          /* hipStream_t */

typedef enum vt_status {
  VT_OK = 0,
  VT_ERR_ARG = -1,                /* bad / unsupported argument (message in vt_last_error) */
  VT_ERR_HIP = -2,                /* a HIP runtime call failed */
  VT_ERR_UNSUPPORTED = -3
} vt_status;

typedef enum vt_dtype { VT_F32 = 0, VT_BF16 = 1, VT_I32 = 2, VT_BF16X3 = 3 /* vt_conv arithmetic only, see above */, VT_F16 = 4 } vt_dtype;

/* time-axis treatment of taps that fall before the first frame of the input */
typedef enum vt_tmode {
  VT_TPAD_ZERO = 0,       /* v1.0 CausalConv{1,3}d, pad_mode "constant"  (model_3dcausal.py:156-159,193-197) */
  VT_TPAD_REPLICATE = 1,  /* v1.1 first chunk: first frame repeated        (model_3dcausal_v1_1.py:160-163,217-220) */
  VT_TPAD_CACHE = 2,      /* v1.1 later chunks: last frames of the cache   (model_3dcausal_v1_1.py:164-171,221-228) */
  VT_TPAD_ZERO_BACK = 3   /* vt_time_avgpool3s2 only: one zero frame AFTER the sequence, non-causal TimeDownsampleRes2x (model_3dnoncausal.py:86-89) */
} vt_tmode;

typedef enum vt_resmode {
  VT_RES_NONE = 0,
  VT_RES_ADD = 1,         /* y = conv + bias + res          (ResnetBlock x + h, model_3dcausal.py:337,424,499,118) */
  VT_RES_MIX = 2          /* y = a*res + (1-a)*(conv+bias), a = sigmoid(*mix_factor)
                             (TimeDown/UpsampleResCausal2x, model_3dcausal.py:248-252,268-273) */
} vt_resmode;

typedef enum vt_layout { VT_NDHWC = 0, VT_NCTHW = 1 } vt_layout;

const char* vt_last_error(void);
/* returns a version integer; also a cheap "is the library loadable" probe */
int vt_version(void);
/* hipGraphLaunch of an instantiated graph (hipGraphExec_t) on `stream`, nothing else: how the Python host replays the encoder /
 * decoder launch sequences it captured (vidtok_amd/graphs.py) -- a framework's own replay also launches bookkeeping kernels */
int vt_graph_launch(void* graph_exec, vt_stream stream);
/* number of bytes of dynamic LDS the biggest conv variant asks for (diagnostic) */
int vt_conv_max_lds_bytes(void);

/* ------------------------------------------------------------------------------------------
 * Process-wide tuning / test switches.  Which kernel a call runs is a function of its descriptor and of this
 * table only -- no launch path reads the environment.  The table is filled once, on first use, from the
 * environment (variable VT_<NAME>, e.g. VT_CONV_WS=0, so shell A/B runs work) and changes afterwards only
 * through vt_set_option; vt_reset_options() re-reads the environment defaults.  Every option selects between
 * implementations of the SAME operator contract (the parity tests run both sides of each switch), so none of them
 * is part of the reference's interface.  Names (default):
 *   conv_buf (1)        gather through buffer descriptors; 0 = 64-bit pointers (always used for > 4 GiB tensors, and in cache mode when a tile spans frames)
 *   conv_tinner (1)     temporal convolutions walk their tiles frames-innermost (L2 reuse of the kt taps)
 *   conv_ldsepi (1)     128 x 128 tile: epilogue transposed through the LDS (whole-line stores, carries the fused LayerNorm)
 *   conv_ws (2)         weight-stationary persistent kernel (conv_ws2.hip: two waves per SIMD splitting K) for the 3x3 128 -> 128
 *                       convolutions in a 16-bit type; 0 = off (the tile-per-workgroup kernel)
 *   conv_narrow (1)     conv3d_narrow_kernel for Cout <= 4 (the decoder's conv_out)
 *   conv_tile (0)       128 / 256: force that tile wherever it is legal; 0 = choose by size
 *   conv_tile_min (128) fewest 256 x 256 tiles for which the 8-wave tile is chosen
 *   conv_fuse_ln (1), conv_fuse_ln256 (1)   LayerNorm of the result inside the epilogue for Cout = 128 / 256
 *   conv_deep (1)       128 x 128 tile on a 4-slot ring (three K steps of DMA in flight) for launches with no more tiles than CUs
 *   conv_splitk (1)     split-K over the tap planes for launches with few pixels PER CLIP when the caller provides scratch
 *                       (vt_conv_work_bytes).  A split launch sums in another order than a whole one, so the decision is a function
 *                       of one clip's geometry (To, Ho, Wo, Cout, K) and never of B: a clip's bits do not depend on its batch.
 *                       + 2-3 % on a v1.1 tiled pass, neutral on the B = 4 benchmark step (profiles/r05_tskip_splitk_ab.txt)
 *   conv_tskip (1)      causal zero padding in time (tmode VT_TPAD_ZERO): a tile that lies inside one output frame starts its K walk
 *                       behind the tap planes that read only the zero frames in front of the clip (frames 0 / 1 of a 3-tap convolution
 *                       run a third / two thirds of the K steps); the skipped products are exact zeros: same bits as the full walk
 *   conv_in8 (1)        conv_in8_kernel for the encoder's conv_in (bf16, 3 x 3 x 3, 8 stored input channels -> 128, zero / replicate time
 *                       padding, frames whose width divides or is a multiple of 128): the tile's halo patch arrives by LDS-DMA once, a
 *                       fragment is one ds_read, the weights are register-stationary, the epilogue transposes through a 64-row buffer.
 *                       The same bits as the general path of the implicit-GEMM kernel (0), 16 % faster on the launch
 *   conv_tup_ln (1)     the LayerNorm the consumer of a v1.0 time up-sampler starts with is emitted by the up-sampler's two parity launches
 *                       (alpha-mix + interleaved output frames + LayerNorm together in the bf16 LDS epilogue of the 8-wave tile) instead of
 *                       running as its own pass (- 0.2 ... 0.3 ms of the benchmark step); hosts ask vt_conv_plan whether a launch fuses it; 0 = the separate pass.
 *                       (Gates the Cout = 256 epilogue only: the Cout = 128 LayerNorm epilogue takes an alpha-mix / interleaved output under conv_fuse_ln alone.)
 *   conv_nt_mb (64)     outputs (y and the fused LayerNorm) of at least this many MiB are written by the LDS epilogues with streaming (nt)
 *                       stores: rows nobody reads before they have left every cache do not displace the weight slabs and halo rows the next tiles
 *                       read again (whole benchmark step - 0.7 %; the fused temporal block and conv3x3_ws2 always store this way); 0 = plain stores
 *   conv_tup3 (1)       a causal v1.0 time up-sampler runs as vt_conv (V = W1 x) + vt_time_upsample3 (three frame products for two output
 *                       frames) where vt_time_upsample3_supported says so; 0: it answers no, the hosts run the two parity launches (four products)
 *   attn_flash (1)      the attention block as one vt_flash_attention launch where it applies; 0: GEMM -> softmax -> GEMM operators
 *   tblock_prof_mode (0), ws_prof_mode (0)   measurement aids
 * (Rounds 1-5 also kept the superseded forms selectable -- K-step schedules 0 / 1 / 3 / 4, the first LayerNorm epilogue of the 8-wave
 * tile, the first-generation weight-stationary kernel, 128 x 256 half tiles: their measurements are in DESIGN.md section 6, the code is
 * in the history.)
 *   tblock_fused (1)   0: vt_temporal_block_supported answers no (blocks stay on the unfused operators)
 * Returns VT_ERR_ARG for an unknown name.
 * ---------------------------------------------------------------------------------------- */
int vt_set_option(const char* name, int32_t value);
int vt_get_option(const char* name, int32_t* value);
int vt_reset_options(void);
int vt_option_count(void);
const char* vt_option_name(int32_t i);    /* i < vt_option_count(), else NULL */

/* ------------------------------------------------------------------------------------------
 * vt_conv -- implicit-GEMM convolution on NDHWC, M = B*To*Ho*Wo pixels x N = Cout x K = taps*Cin.
 * One entry point covers every convolution of the path:
 *   nn.Conv2d 3x3 s1 p1      ResnetBlock.conv1/conv2            model_3dcausal.py:296,301
 *   nn.Conv2d 3x3 s1 p1 after nearest x2   Upsample               model_3dcausal.py:208-212  (ups_s=1)
 *   nn.Conv2d 3x3 s2 p0 after F.pad(0,1,0,1)  Downsample          model_3dcausal.py:223-227
 *   nn.Conv2d 1x1            nin_shortcut                       model_3dcausal.py:306
 *   nn.Conv1d k3 causal      CausalConv1d                       model_3dcausal.py:144-159
 *   nn.Conv3d 3x3x3 causal   CausalConv3d (stride 1 or (2,1,1)) model_3dcausal.py:162-197
 *   nn.Conv3d 1x1x1          AttnBlockWrapper q/k/v/proj_out    model_3dcausal.py:124-127
 *   nearest x2 in T folded   TimeUpsampleResCausal2x            model_3dcausal.py:267-273  (ups_t=1)
 * and, with KT=KH=KW=1 and nbatch>1, the batched GEMMs of the attention block
 * (F.scaled_dot_product_attention, model_3dcausal.py:140).
 *
 * Tap (kt,kh,kw) of output (b,to,ho,wo) reads the *virtual* input position
 *   tv = to*st + kt - pt,  hv = ho*sh + kh - ph,  wv = wo*sw + kw - pw
 * in a virtual input of size (Ti<<ups_t, Hi<<ups_s, Wi<<ups_s); the stored element is
 * (tv>>ups_t, hv>>ups_s, wv>>ups_s).  Spatial positions outside the virtual extent read 0;
 * tv<0 follows `tmode` (cache: frame ncache+tv of `cache`, shape [B][ncache][Hi][Wi][Cin]);
 * tv beyond the end reads 0.
 * Weights are pre-packed row-major [Cout][ldw], k = ((kt*KH+kh)*KW+kw)*Cin + c (see
 * vidtok_amd/packing.py), in the arithmetic dtype.
 * yt_mul = 2 serves the convolutions over a nearest-x2 frame-repeated input (TimeUpsampleRes*2x): with u[t] = x[t>>1]
 * the three temporal taps of an output frame hit only two input frames, so even and odd output frames are two 2-tap
 * convolutions over x with pre-summed weights -- 2/3 of the MACs of the folded ups_t form, no up-sampled tensor
 * either way (vidtok_amd/packing.py::time_upsample_parity_weights).
 * ys_mul = 2 is the same identity in space (Upsample: nearest x2 then 3x3): each of the four output parities (py, px)
 * is a 2x2 convolution over the stored frame with pre-summed taps, 4/9 of the MACs
 * (vidtok_amd/packing.py::space_upsample_parity_weights).
 * ln_mode != 0 additionally emits ln_out = [SiLU](LayerNorm_Cout(result) * gamma + beta), the norm that follows the
 * convolution inside the residual blocks (norm2 + nonlinearity after conv1, model_3dcausal.py:321-323,405-407,
 * 482-484).  When the tile spans the channel row (Cout = 128) the statistics are taken from the fp32 result inside
 * the epilogue and, with ln_keep_y = 0, y is never written: one activation write instead of write + read + write.
 * Otherwise the library runs the convolution into y and vt_layernorm_act on it -- same contract, y must always be
 * a full-size buffer.  NDHWC output, nbatch = 1 only.
 * ---------------------------------------------------------------------------------------- */
typedef struct vt_conv_desc {
  const void* x;            /* input  [B][Ti][Hi][Wi][Cin]     (dtype)                        */
  const void* w;            /* packed weights [Cout][ldw]       (dtype)                        */
  const float* bias;        /* [Cout] fp32 or NULL                                             */
  void* y;                  /* output, out_dtype; NDHWC [M][ldy] or NCTHW (see out_layout)     */
  const void* res;          /* residual / mix operand, out_dtype, [B][Tr][Ho][Wo][ldr] or NULL */
  const void* cache;        /* time cache [B][ncache][Hi][Wi][Cin] (dtype) or NULL             */
  const float* mix_factor;  /* device scalar; alpha = sigmoid(*mix_factor) for VT_RES_MIX      */
  const float* ln_gamma;    /* fused LayerNorm of the result (ln_mode != 0): affine, fp32 [Cout]  */
  const float* ln_beta;
  void* ln_out;             /* normalised (+SiLU) result, out_dtype, NDHWC [M][ldn]            */
  int32_t B, Ti, Hi, Wi, Cin;
  int32_t To, Ho, Wo, Cout;
  int32_t ldw;              /* row stride of w in elements (>= KT*KH*KW*Cin, multiple of 16 B) */
  int32_t ldy;              /* channel stride of y for NDHWC                                   */
                            /* (lanes Cout .. ldy-1 of a row, and Cout .. ldn-1 of ln_out, are left unchanged or zero-filled:
                             *  a caller that zeroes them once may rely on zeros -- tests/test_gpu_arena.py holds every kernel to it) */
  int32_t KT, KH, KW;
  int32_t st, sh, sw;
  int32_t pt, ph, pw;
  int32_t tmode, ncache;
  int32_t ups_t, ups_s;
  int32_t res_mode;         /* vt_resmode                                                      */
  int32_t res_tshift;       /* res time index = to >> res_tshift                               */
  int32_t Tr, ldr;
  int32_t out_layout;       /* vt_layout; VT_NCTHW needs out_dtype == VT_F32                   */
  int32_t t_trim;           /* NCTHW only: drop the first t_trim output frames                 */
  int32_t dtype;            /* arithmetic / input / weight dtype                               */
  int32_t out_dtype;        /* dtype or VT_F32                                                 */
  int32_t nbatch;           /* >=1: independent problems along grid.z                          */
  int32_t ln_mode;          /* 0 none, 1 LayerNorm over Cout, 2 LayerNorm + SiLU -> ln_out     */
  int32_t ln_keep_y;        /* 0: only ln_out is needed; y is then scratch (may stay unwritten) */
  int32_t ldn;              /* channel stride of ln_out                                        */
  int32_t yt_mul, yt_off;   /* output frame interleave: computed frame f (b*To + to) is stored as frame
                               f*yt_mul + yt_off of a y (and ln_out) holding To*yt_mul frames; 0/1 = off  */
  int32_t ys_mul, ys_oh, ys_ow; /* ys_mul = 2: computed pixel (ho, wo) is stored as pixel (2ho+ys_oh, 2wo+ys_ow) of
                               a y whose frames are 2Ho x 2Wo (spatial parity classes, see below); 0/1 = off     */
  float ln_eps;
  int64_t xs_z, ws_z, ys_z, rs_z;   /* element strides between problems                       */
  void* work;                  /* optional scratch for split-K launches (see vt_conv_work_bytes); NULL = never split */
  int64_t work_bytes;
} vt_conv_desc;

int vt_conv(const vt_conv_desc* d, vt_stream stream);
/* Split-K over tap planes (the three time taps; the three rows of a 3 x 3 without time taps).  A long-K convolution on few pixels (the 512-channel 3x3x3 layers on a chunk of a v1.1 tiled
 * pass: M = 4 096 pixels x N = 512 x K = 13 824 = 128 tiles of 128 x 128 with 216 K steps each on 256 CUs) is latency-bound: one tile per
 * CU walking a long K.  Given scratch, vt_conv runs it as three launches-in-one (grid.z = tap plane: each workgroup walks the KH x KW x Cin
 * -- or KW x Cin -- of ONE plane into an fp32 partial) and a reduction that owns bias / residual / rounding: 3 x the workgroups, a third of the steps.
 * vt_conv_work_bytes(d) = the scratch vt_conv(d) would use (0: this call does not split; decided from ONE clip's geometry in the
 * descriptor -- never from B -- and option conv_splitk, ignoring d->work); with d->work = NULL or d->work_bytes too small the call runs unsplit.  The fp32 sum of an output
 * is then taken in another order (per tap, then over the taps): results differ from the unsplit launch by fp32 rounding. */
int64_t vt_conv_work_bytes(const vt_conv_desc* d);
/* What vt_conv(d) will do, without launching (no GPU needed; validates `d` exactly like vt_conv).  vt_conv runs the plan this reports --
 * both come from one decision -- so hosts may rely on it: whether a LayerNorm is fused (before allocating its output), which
 * instantiation a parity case exercises, which kernel serves a layer.
 *   out8[0..1]  pixel x channel tile         out8[2]  waves per workgroup      out8[3]  workgroups (tiles for the persistent kernel)
 *   out8[4]     1 if the LayerNorm asked for comes from the conv kernel's epilogue (0: second launch of vt_layernorm_act, or none asked)
 *   out8[5]     kernel launches the call performs (+ 1 for an un-fused LayerNorm, + 1 for a split-K launch's reduction when d->work is given,
 *               2 for the split-bf16 narrow kernel's two passes)
 *   out8[6]     kernel: 0 = tile-per-workgroup implicit GEMM (conv_igemm_glds_kernel); 2 = the narrow-output kernel (conv3d_narrow_kernel);
 *               3 = weight-stationary persistent 3x3 for Cin = Cout = 128 in a 16-bit type (conv3x3_ws2_kernel, 4 x 16-pixel tiles on 8 waves);
 *               4 = conv_in8_kernel, the encoder's conv_in from an LDS halo patch; 1 is reserved (a kernel that is gone)
 *   out8[7]     1 if the epilogue goes through the LDS (coalesced rows: conv_in8; the 8-wave tile always with a fused LayerNorm, without one
 *               for full tiles in a 16-bit type), 2 if the 128 x 128 tile runs on its 4-slot ring (option conv_deep: launches with no more
 *               tiles than the device has CUs), else 0 */
int vt_conv_plan(const vt_conv_desc* d, int32_t* out8);
/* The form of the implicit-GEMM launch behind a call, without launching (no GPU needed; validates exactly like the call it describes).
 * The plan above names kernel, tile, epilogue and ring; this is the rest of the same decision -- every choice in it leaves the result
 * bit-equal, so only this report shows whether a layer keeps its descriptor gather, its skipped taps or its tile order.
 *   call  0 = vt_conv(d): the partial launch where d->work / d->work_bytes make the split run, else the whole launch
 *         1 = vt_time_upsample3(d, ..): the paired launch (VT_ERR_ARG where vt_time_upsample3_supported(d) is 0)
 *         2 = vt_conv_act(d, VT_ACT_RELU)
 *   out16[0]      kernel, as out8[6] of vt_conv_plan; the launches of kernels 2, 3, 4 report it and zeros
 *   out16[1]      gather form: 1 = buffer descriptors, 0 = 64-bit pointers (option conv_buf = 0, a tensor of 4 GiB, a cache-mode tile that
 *                 spans frames)
 *   out16[2..4]   descriptor extents in bytes of x, the weights and the cache (0 on pointers)
 *   out16[5]      1 if zero-padded time taps in front of the clip are skipped per tile (option conv_tskip)
 *   out16[6]      > 0: pixel tiles per frame, tiles walked frames-innermost (option conv_tinner); 0 = pixel order
 *   out16[7]      1 if full 128 x 128 tiles go through the LDS-transposed epilogue (meaningful on that tile only)
 *   out16[8]      K steps per tile      out16[9..10]  pixel x channel tiles      out16[11]  grid z (nbatch, or the split planes)
 *   out16[12]     0 whole launch; split-K partial launch over 1 = the time taps, 2 = the rows of a 3 x 3
 *   out16[13]     K-step schedule of the instantiation (0 plain loop, 1 / 2 / 5 the scheduled loops of the 8-wave tile)
 *   out16[14]     dynamic LDS bytes
 *   out16[15]     the instantiation: tile index (0 = 256 x 32, 1 = 256 x 64, 2 = 256 x 256, 3 = 128 x 128) | tap-walk form << 4 |
 *                 LDS epilogue of the 8-wave tile (0 none, 1 plain / LayerNorm, 2 paired) << 8 | ring slots << 12 | K bytes per row and step << 16 */
int vt_conv_launch_form(const vt_conv_desc* d, int32_t call, int64_t* out16);
/* Measurement aid (scripts/conv_profile.py): vt_conv(d) on the bf16 8-wave 256 x 256 tile (no LayerNorm) with shader-clock
 * stamps at the phase boundaries of K steps 8..11 of workgroup 0: stamps_out (device, 8*4*8 uint64) = [wave][step][stamp] */
int vt_conv_profile(const vt_conv_desc* d, uint64_t* stamps_out, vt_stream stream);
/* sizeof(vt_conv_desc) as compiled: lets a binding verify its struct mirror */
int vt_conv_desc_size(void);

/* ------------------------------------------------------------------------------------------
 * vt_time_upsample3 -- the causal v1.0 time up-sampler (TimeUpsampleResCausal2x: every frame twice, causal 3 x 3 x 3 convolution,
 * alpha-mix against the repeated input) as three frame products for two output frames.  With x[-1] = 0 the two parity launches of
 * vt_conv (yt_mul = 2) compute o[2j] = (W0+W1) x[j-1] + W2 x[j] and o[2j+1] = W0 x[j-1] + (W1+W2) x[j]: four 3 x 3 products.
 * Both frames share U[j] = W0 x[j-1] + W2 x[j], and W1 x[j-1] is the previous pair's W1 x[j]; with V[j] = W1 x[j], V[-1] = 0:
 *     o[2j] = U[j] + V[j-1]        o[2j+1] = U[j] + V[j]
 * `u` is the parity descriptor of the even frames with the weights [W0 | W2]: KT = 2, 3 x 3, pt = 1, tmode VT_TPAD_ZERO,
 * res_mode VT_RES_MIX against x, yt_mul = 2, yt_off = 0, optionally ln_*.  `v` = V, [B][Ti][Ho][Wo][ldv] in the storage type (a
 * plain vt_conv of x with W1, no bias).  One launch writes, for every pixel of frame j, both frames of the pair:
 *     y[2j+q] = alpha x[j] + (1 - alpha) (acc + bias + V[j-1+q])        q = 0, 1;   V[-1] = 0 at the start of every clip
 * and, where vt_conv_plan(u) fuses the LayerNorm (its rule for an alpha-mix launch: Cout = 256, option conv_tup_ln), also
 * ln_out[2j+q] = [SiLU](LN(y[2j+q])) from the unrounded row.
 * Covered (a function of one clip's geometry, the type and the options, never of B): bf16 / fp16 with results in the same type,
 * Cout % 256 == 0 on the 256 x 256 tile, Cin % 64 == 0 and tensors below 4 GiB (the tap walk on buffer descriptors),
 * Ho * Wo % 256 == 0, ldy / ldr / ldn (and ldv) % 8 == 0, option conv_tup3.  vt_time_upsample3_supported(u) says so without
 * launching (1 / 0); anything else returns VT_ERR_ARG, and the host runs the two parity launches.
 * ------------------------------------------------------------------------------------------ */
int vt_time_upsample3_supported(const vt_conv_desc* u);
int vt_time_upsample3(const vt_conv_desc* u, const void* v, int32_t ldv, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * vt_temporal_block -- one fused launch for the temporal residual block of the reference,
 * ResnetCausalBlock1D._forward (vidtok/modules/model_3dcausal.py:473-499 with CausalConv1d :144-159 and, for the
 * first-frame-replicate padding of v1.1, model_3dcausal_v1_1.py:159-178):
 *     y = x + conv2( SiLU(LN2( conv1( SiLU(LN1(x)) ) )) )       conv = causal Conv1d over T, k = 3, C -> C
 * on an NDHWC activation x [B][T][HW][ld]; optionally also n_out = [SiLU](LayerNorm_next(y)), the norm the consumer
 * of y starts with (same contract as vt_conv's ln_mode / ln_keep_y).  LayerNorms are per position over C, eps as
 * given, statistics in fp32.  w1 / w2 are packed like vt_conv weights: [C][3*C], k = kt*C + c.
 * tmode: VT_TPAD_ZERO (frames before the clip are zeros), VT_TPAD_REPLICATE (first frame repeated) or VT_TPAD_CACHE
 * (the two frames a previous chunk left: v1.1 tiling, CausalConv1d.causal_cache of model_3dcausal_v1_1.py:159-178).
 * The cached tensors are the INPUTS of the two convolutions -- SiLU(LN1(x)) and SiLU(LN2(conv1)), which a fused launch
 * never writes out -- so the launch keeps them itself: cache1 / cache2 [B][2][HW][ld] are read in cache mode and, when
 * given (any tmode), rewritten in place with frames T - cache_offset - 2, T - cache_offset - 1 of this clip (the
 * reference's padded[:len - cache_offset][-2:]); T - cache_offset >= 3 is required.
 * Covered shapes: bf16, C = ld = 128, HW % 64 == 0 (the widest level of every 488 / 41616 / 288 config);
 * vt_temporal_block_supported(d) says so without launching (1 / 0); anything else returns VT_ERR_ARG.
 * ------------------------------------------------------------------------------------------ */
typedef struct vt_tblock_desc {
  const void* x;                 /* [B][T][HW][ld]                                            */
  void* y;                       /* same shape; may be NULL when keep_y == 0                   */
  void* n_out;                   /* same shape; LayerNorm_next(y) (+SiLU), or NULL             */
  const void* w1; const float* b1;   /* conv1: [C][3C] packed, bias [C] fp32 or NULL           */
  const void* w2; const float* b2;   /* conv2                                                   */
  const float* norm1_gamma; const float* norm1_beta;   /* [C] fp32                              */
  const float* norm2_gamma; const float* norm2_beta;
  const float* next_gamma; const float* next_beta;     /* used when ln_next_mode != 0           */
  int32_t dtype;                 /* VT_BF16 or VT_F16                                          */
  int32_t C, ld;
  int32_t B, T;
  int64_t HW;
  int32_t tmode;                 /* VT_TPAD_ZERO | VT_TPAD_REPLICATE | VT_TPAD_CACHE           */
  int32_t keep_y;                /* 0: only n_out is needed (y is never written)               */
  int32_t ln_next_mode;          /* 0 none, 1 LayerNorm, 2 LayerNorm + SiLU                    */
  float eps;
  int32_t cache_offset;          /* frames at the end of the clip that the kept chunk state skips */
  void* cache1;                  /* [B][2][HW][ld] chunk state of conv1 (see above), or NULL    */
  void* cache2;                  /* ... of conv2                                               */
} vt_tblock_desc;

/* sizeof(vt_tblock_desc) as compiled: lets a binding verify its struct mirror */
int vt_tblock_desc_size(void);
int vt_temporal_block_supported(const vt_tblock_desc* d);
int vt_temporal_block(const vt_tblock_desc* d, vt_stream stream);
/* Measurement aid (scripts/tblock_profile.py): the same launch (ln_next_mode 2, keep_y 1 only) with shader-clock
 * stamps at the phase boundaries of four steps of workgroup 0: stamps_out (device, 8*4*8 uint64) = [wave][step][stamp] */
int vt_temporal_block_profile(const vt_tblock_desc* d, uint64_t* stamps_out, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * vt_layernorm_act -- per-position LayerNorm over C (eps inside the sqrt, biased variance,
 * affine) optionally followed by SiLU x*sigmoid(x).
 * Replaces LayerNorm wrapper + nonlinearity: model_3dcausal.py:62-80, 26-27 (every norm site of
 * ResnetBlock / ResnetCausalBlock / ResnetCausalBlock1D / AttnBlock / norm_out).
 * x: [M][ldx] in `in_dtype`, y: [M][ldy] in `out_dtype`; gamma, beta fp32 [C].
 * ---------------------------------------------------------------------------------------- */
int vt_layernorm_act(const void* x, int in_dtype, int64_t ldx, void* y, int out_dtype, int64_t ldy,
                     const float* gamma, const float* beta, int64_t M, int32_t C, float eps,
                     int32_t silu, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * vt_groupnorm_act -- torch.nn.GroupNorm(32, C, eps, affine) optionally followed by SiLU: the `norm_type: groupnorm`
 * branch of Normalize() (model_3dcausal.py:30-34; no shipped config selects it).  GroupNorm normalises over
 * (C/groups, *spatial) of the view its call site passes, so the reduction domain is a parameter:
 *   VT_GN_FRAME  spatial ResnetBlock on "(b t) c h w"  (model_3dcausal.py:14-19, 317-337)  per (b,t,g) over (C/G,H,W)
 *   VT_GN_PIXEL  temporal blocks on "(b h w) c t"       (model_3dcausal.py:20-23, 473-499)  per (b,h,w,g) over (C/G,T)
 *   VT_GN_CLIP   3-D blocks, attention norm, norm_out on "b c t h w"                          per (b,g) over (C/G,T,H,W)
 * x [B][T][HW][ldx], y [B][T][HW][ldy]; gamma, beta fp32 [C]; work: vt_groupnorm_work_bytes() bytes (fp64 sums).
 * ---------------------------------------------------------------------------------------- */
typedef enum { VT_GN_FRAME = 0, VT_GN_PIXEL = 1, VT_GN_CLIP = 2 } vt_gn_scope;
int64_t vt_groupnorm_work_bytes(int32_t B, int32_t T, int32_t groups, int32_t scope);
int vt_groupnorm_act(const void* x, int in_dtype, int64_t ldx, void* y, int out_dtype, int64_t ldy,
                     const float* gamma, const float* beta, int32_t B, int32_t T, int64_t HW, int32_t C,
                     int32_t groups, int32_t scope, float eps, int32_t silu, void* work, vt_stream stream);

/* Single-head self-attention of the pixels of a frame in ONE launch, nothing S x S in memory (F.scaled_dot_product_attention
 * of AttnBlock, model_3dcausal.py:129-141): o[z][q][:] = sum_k softmax_k(scale * q[z][q] . k[z][k]) v[z][k][:] + bias_v.
 * q, k, o: [Z][S][C]; vt: V TRANSPOSED, [Z][C][ldv] with the keys contiguous (the v projection with its operands swapped, as the
 * hosts already compute it; its bias goes in as bias_v, fp32 [C] or NULL).  bf16, C = 512, S a multiple of 64
 * (vt_flash_attention_supported says whether a shape is covered and option attn_flash is on; otherwise the same contract is
 * vt_conv as batched GEMM -> vt_softmax_rows -> vt_conv).  Online softmax in fp32; P is rounded to bf16 before the second
 * product, un-normalised, and the division by the row sum comes last. */
int vt_flash_attention_supported(int32_t dtype, int32_t S, int32_t C, int32_t ldv);
int vt_flash_attention(const void* q, const void* k, const void* vt, const float* bias_v, void* o, int32_t dtype, int32_t Z, int32_t S,
                       int32_t C, int32_t ldv, float scale, vt_stream stream);

/* row softmax(scale * s) over the last dim; s fp32 [rows][cols] -> p (out_dtype) [rows][ldp].
 * The softmax inside F.scaled_dot_product_attention (model_3dcausal.py:140), scale = C^-0.5. */
/* x = tanh(x) in place on n fp32 elements: the decoders' `tanh_out` option (model_3dcausal.py:866-869) */
int vt_tanh_inplace(float* x, int64_t n, vt_stream stream);
int vt_softmax_rows(const float* s, void* p, int out_dtype, int64_t rows, int32_t cols,
                    int64_t ldp, float scale, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * layout conversion at the two ends of the path
 * vt_ncthw_to_ndhwc: x fp32 NCTHW [B][C][T][H][W] -> y (out_dtype) [B][tpad+T][H][W][ldy],
 *   channels C..ldy-1 zero-filled, the first `tpad` frames replicate frame 0
 *   (EncoderCausal3DPadding.forward pad_at_dim(..., "replicate"), model_3dcausal.py:685-689,
 *   v1.1 model_3dcausal_v1_1.py:755-760).
 * vt_ndhwc_to_ncthw: x (in_dtype) [B][T][H][W][ldx] -> y fp32 [B][C][T-ttrim][H][W]
 *   (DecoderCausal3DPadding.forward trim, model_3dcausal.py:883-885).
 * ---------------------------------------------------------------------------------------- */
int vt_ncthw_to_ndhwc(const float* x, void* y, int out_dtype, int32_t B, int32_t C, int32_t T,
                      int32_t H, int32_t W, int32_t ldy, int32_t tpad, vt_stream stream);
int vt_ndhwc_to_ncthw(const void* x, int in_dtype, float* y, int32_t B, int32_t C, int32_t T,
                      int32_t H, int32_t W, int32_t ldx, int32_t ttrim, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * time resamplers (the non-conv branches)
 * vt_time_avgpool3s2: y[to] = (xp[2to]+xp[2to+1]+xp[2to+2])/3 over the front-padded sequence
 *   xp = [pad, x]; pad frame = 0 (tmode ZERO, v1.0 model_3dcausal.py:249-250), x[0]
 *   (REPLICATE, v1.1 first chunk) or `cache` (one frame [B][1][H][W][C], v1.1 later chunks,
 *   model_3dcausal_v1_1.py:293-300); VT_TPAD_ZERO_BACK: xp = [x, 0] instead (non-causal family,
 *   model_3dnoncausal.py:86-89).  x [B][Ti][HW][C] -> y [B][Ti/2][HW][C] (floor: an odd Ti loses its
 *   last frame, as avg_pool3d does), same dtype.
 * vt_time_lerp2x: F.interpolate(scale (2,1,1), "trilinear", align_corners=False) along T of a
 *   sequence of Ti frames -> 2*Ti frames (model_3dcausal_v1_1.py:327-341); fp32 arithmetic.
 * vt_time_lerp2x_cat: the same of the sequence [head (nh frames, [B][nh][HWC]) | x ([B][Tx][HWC])] per clip without
 *   assembling it, leaving out the first `skip` output frames: y [B][2 (nh + Tx) - skip][HWC].  The chunks after the
 *   first of a v1.1 tiled pass: head = the frames cached from the previous chunk, skip = 2 * num_temp_upsample
 *   (torch.cat + interpolate + slice, model_3dcausal_v1_1.py:331-341).  nh = 0, skip = 0 is vt_time_lerp2x.
 * ---------------------------------------------------------------------------------------- */
int vt_time_avgpool3s2(const void* x, const void* cache, void* y, int dtype, int32_t B, int32_t Ti,
                       int64_t HW, int32_t C, int32_t tmode, vt_stream stream);
int vt_time_lerp2x(const void* x, void* y, int dtype, int32_t B, int32_t Ti, int64_t HWC,
                   vt_stream stream);
int vt_time_lerp2x_cat(const void* head, int32_t nh, const void* x, void* y, int dtype, int32_t B, int32_t Tx, int32_t skip,
                       int64_t HWC, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * vt_pack_conv_weight -- a convolution parameter in the reference's layout, w fp32 [Cout][Cin][taps_in] (nn.Conv3d / Conv2d /
 * Conv1d weight, taps = kT*kH*kW row-major), to the rows vt_conv reads: out [Cout][ldw], k = tap * cin_p + c,
 * channels zero-padded to cin_p (the activation's stored count), the row tail zero.  out_dtype VT_F32 / VT_BF16 / VT_F16 = plain rows
 * (round to nearest even); VT_BF16X3 = the split-bf16 container: per 16 k [hi 16 x bf16 | lo 16 x bf16], hi = bf16(w),
 * lo = bf16(w - hi), 4 bytes per k, ldw a multiple of 32.  mix_host (host, [taps_out][4], -1 = absent; NULL = identity): output
 * tap j = (w[m0] + w[m1]) + (w[m2] + w[m3]) in fp32 -- the pre-summed taps of the up-samplers' parity classes (a 3-tap window
 * over a nearest-x2 repeated input touches two inputs: [W0 + W1, W2] / [W0, W1 + W2] per axis).  One-time work per weight. */
int vt_pack_conv_weight(const float* w, void* out, int32_t out_dtype, int32_t Cout, int32_t Cin, int32_t cin_p, int32_t taps_in,
                        int32_t taps_out, const int32_t* mix_host, int64_t ldw, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * regularizers; all tensors NCTHW fp32 as in the reference API
 * vt_kl_sample: h [B][2*zc][S] (S = T*H*W); mean,logvar = chunk(h,2,dim=1); logvar clamped to
 *   [-30,20]; z = mean + exp(0.5*logvar)*noise (noise [B][zc][S] or NULL -> mode());
 *   *kl_out = 0.5*sum(mean^2 + var - 1 - logvar) / B     (distributions.py:8-28,
 *   regularizers.py:82-92; the reference draws `noise` on the host with torch.randn).
 * vt_fsq_quantize: h [B][D][S], levels[D]; bound -> round-half-even -> codes z [B][D][S]
 *   (values q/(L//2)) and int32 indices [B][S] (regularizers.py:153-178, 225-230).
 * vt_fsq_indices_to_codes: indices [B][S] -> z [B][D][S] (regularizers.py:180-198).
 * vt_fsq_aux_stats: the two entropies and the commitment term of FSQRegularizer.forward
 *   (regularizers.py:231-246) for h [B][D][S]: out[0] = per-sample entropy (mean), out[1] =
 *   codebook entropy of the batch-mean distribution, out[2] = commit loss.  `work` is a device
 *   scratch of vt_fsq_aux_work_floats(...) floats.
 * vt_fsq_aux_stats_avg: the same, and (avg_out != NULL) the batch-mean code distribution avg_prob[prod(levels)] the
 *   codebook entropy is taken of -- the tensor the reference averages across ranks when torch.distributed runs
 *   with world > 1 (maybe_distributed_mean, regularizers.py:49-59,240); vt_entropy(avg, J, out) then recomputes
 *   out[0] = sum_j -avg_j * log(max(avg_j, 1e-5)) (regularizers.py:40-45) of the all-reduced distribution.
 * ---------------------------------------------------------------------------------------- */
/* host-only helper: writes half_l[D], offset[D], shift[D], basis[D] (as floats) exactly as the
 * FSQ kernels use them (FSQRegularizer.bound constants, regularizers.py:153-158) -- no GPU needed. */
int vt_fsq_consts(const int32_t* levels_host, int32_t D, float* out_host);
int vt_kl_sample(const float* h, const float* noise, float* z, float* kl_out, int32_t B,
                 int32_t zc, int64_t S, vt_stream stream);
int vt_fsq_quantize(const float* h, float* z, int32_t* indices, const int32_t* levels_host,
                    int32_t D, int32_t B, int64_t S, vt_stream stream);
int vt_fsq_indices_to_codes(const int32_t* indices, float* z, const int32_t* levels_host,
                            int32_t D, int32_t B, int64_t S, vt_stream stream);
/* The same with `ncb` codebooks (FSQRegularizer num_codebooks, "b n (c d) -> b n c d", regularizers.py:131-133,227): h, z
 * [B][ncb * D][S] -- the D channels of codebook c of a clip are contiguous --, each codebook quantised on its own, and the
 * codebook axis LAST on the indices as the reference keeps it: indices [B][S][ncb].  ncb = 1 is the plain form. */
int vt_fsq_quantize_cb(const float* h, float* z, int32_t* indices, const int32_t* levels_host,
                       int32_t D, int32_t B, int32_t ncb, int64_t S, vt_stream stream);
int vt_fsq_indices_to_codes_cb(const int32_t* indices, float* z, const int32_t* levels_host,
                               int32_t D, int32_t B, int32_t ncb, int64_t S, vt_stream stream);
int64_t vt_fsq_aux_work_floats(const int32_t* levels_host, int32_t D, int32_t B, int64_t S);
int vt_fsq_aux_stats(const float* h, const int32_t* levels_host, int32_t D, int32_t B, int64_t S,
                     float inv_temperature, float* work, float* out3, vt_stream stream);
int vt_fsq_aux_stats_avg(const float* h, const int32_t* levels_host, int32_t D, int32_t B, int64_t S,
                         float inv_temperature, float* work, float* out3, float* avg_out, vt_stream stream);
/* out[0] = (stats3[0] - diversity_gamma * ce) * entropy_weight + stats3[2] * commitment_weight, ce = codebook_entropy[0] or
 * (NULL) stats3[1]: the auxiliary loss FSQRegularizer.forward returns (regularizers.py:241,264-266), every product / sum
 * rounded on its own like the reference's separate tensor operations */
int vt_fsq_aux_loss(const float* stats3, const float* codebook_entropy, float diversity_gamma, float entropy_weight,
                    float commitment_weight, float* out, vt_stream stream);
int vt_entropy(const float* avg, int64_t J, float* out, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * Model handle: AutoencodingEngine.encode / decode of the causal (v1.0, v1.1) and non-causal tokenizers driven from C++ over the operators above
 * (reference vidtok/models/autoencoder.py:197-229: encode = encoder -> regularization, decode = decoder, forward = both;
 * the module tree of vidtok/modules/model_3dcausal.py:502-885 with `norm_type: layernorm`, `resamp_with_conv: true`).
 * Same stage graph, descriptors and fusion decisions as the Python host (vidtok_amd/modules.py), hence the same bits.
 *   vt_create(cfg, VT_BF16 | VT_F16 | VT_F32 | VT_BF16X3, &h)   the fields of cfg are the constructor arguments of the reference's YAML;
 *                                            VT_BF16X3 = fp32 storage with every convolution in split-bf16 arithmetic
 *   vt_load_weight(h, key, data, shape, n)   key = the reference state_dict key ("encoder.down.0.block.0.conv1.weight",
 *                                            ...), data = fp32 on the HOST in the reference's parameter layout; weights
 *                                            are re-packed when first used.  vt_weight_count / vt_weight_name /
 *                                            vt_weight_shape list the parameters; unknown keys and wrong shapes are refused.
 *   vt_workspace_bytes(h, B, T, H, W)        device bytes vt_encode of a [B][in_channels][T][H][W] clip and vt_decode of
 *                                            its latent need (activations; the handle owns its packed weights)
 *   vt_latent_dims(h, T, H, W, out4)         {channels of the encoder output, T', H', W'}
 *   vt_encode(h, x, B, T, H, W, h_out, ws, ws_bytes, stream)     x fp32 NCTHW -> h_out fp32 [B][C'][T'][H'][W'] (the
 *                                            Gaussian moments for KL, the pre-quantisation latent for FSQ)
 *   vt_regularize_kl(h, moments, noise | NULL, z, kl_out, B, T', H', W', stream)     = vt_kl_sample
 *   vt_regularize_fsq(h, pre, z, indices, B, T', H', W', stream)                     = [project_in ->] vt_fsq_quantize_cb [-> project_out]
 *   vt_indices_to_latent(h, indices, z, B, T', H', W', stream)                       = vt_fsq_indices_to_codes_cb [-> project_out]
 *                                            (indices int32 [B][T'][H'][W'], with fsq_num_codebooks = c > 1: [B][T'][H'][W'][c]; with
 *                                            projections the handle keeps a scratch of the projected latent, grown on first use)
 *   vt_decode(h, z, B, T', H', W', x_out, ws, ws_bytes, stream)  z fp32 NCTHW -> x_out fp32 [B][out_ch][T][H][W]
 *   vt_regularize_fsq_aux(h, pre, B, T', H', W', inv_temperature, work, out3, stream)   the three statistics of FSQ's auxiliary
 *                                            loss = vt_fsq_aux_stats with the handle's levels
 *   v1.1 (version 1): the encoder pads T up to a multiple of time_downsample_factor in front and vt_decode returns all
 *   T' * factor frames -- the caller keeps the last T, as AutoencodingEngine.forward does (autoencoder_v1_1.py:339-341).
 * Temporal tiling of the v1.1 models (AutoencodingEngine.tile_encode / tile_decode, autoencoder_v1_1.py:218-331): the clip
 * runs as chunks [0,1), [1,1+c), [1+c,1+2c) ... through the same graph, every causal convolution and time resampler
 * keeping its last frames in device buffers owned by the handle (the reference's `causal_cache` attributes):
 *   vt_tile_latent_frames(h, T, t_chunk_enc)      T' of a tiled encode = sum over the chunks of ceil(frames / factor)
 *   vt_tile_workspace_bytes(h, B, T, H, W, t_chunk_enc, use_overlap)   workspace of vt_tile_encode + vt_tile_decode
 *   vt_tile_encode(h, x, B, T, H, W, t_chunk_enc, h_out, ws, ws_bytes, stream)     h_out fp32 [B][C'][T'][H'][W']; the
 *                                            regularizer then runs on the whole latent (it is per position)
 *   vt_tile_decode(h, z, B, T', H', W', t_chunk_dec, use_overlap, x_out, ws, ws_bytes, stream)   t_chunk_dec = t_chunk_enc /
 *                                            factor; use_overlap = one look-ahead latent frame per chunk whose output frames
 *                                            are dropped, with the doubling cache offsets of the reference (:307-320);
 *                                            x_out fp32 [B][out_ch][T' * factor][H][W]
 *   vt_reset_cache(h)                        drops the chunk state and frees its buffers (synchronises the device); the
 *                                            tiled calls reset the state themselves at the start of a clip
 *   vt_prepare(h)                            packs and uploads every weight now instead of at its first use
 * All device pointers; the calls are asynchronous on `stream` except that (a) the FIRST use of a weight packs it on the host
 * and uploads it with a blocking copy (vt_prepare does all of them up front) and (b) a chunk cache is hipMalloc'ed the first time a chunk kind needs it -- run one
 * warm-up call before capturing a stream.  A handle keeps per-call state (arenas, caches): one call at a time per handle.
 * The workspace must outlive the work queued on it.
 * ---------------------------------------------------------------------------------------- */
typedef struct vt_model_config {
  int32_t version;               /* 0 = v1.0 causal, 1 = v1.1 causal (replicate padding; one pass or temporal tiling), 2 = non-causal */
  int32_t ch, num_res_blocks, in_channels, out_ch, z_channels, double_z;
  int32_t num_resolutions;       /* len(ch_mult)                                                                */
  int32_t ch_mult[8];
  int32_t n_spatial_ds, spatial_ds[8], n_tempo_ds, tempo_ds[8];     /* encoder levels that end in a down-sampler */
  int32_t n_spatial_us, spatial_us[8], n_tempo_us, tempo_us[8];     /* decoder levels that end in an up-sampler  */
  int32_t time_downsample_factor;
  int32_t regularizer;           /* 0 DiagonalGaussianRegularizer, 1 FSQRegularizer                              */
  int32_t n_levels, levels[8];
  int32_t interpolation_mode;    /* v1.1 time up-samplers: 0 nearest, 1 trilinear                                 */
  /* the constructor arguments no shipped YAML sets (zero = the reference's default):                             */
  int32_t norm_type;             /* 0 "layernorm", 1 "groupnorm": torch.nn.GroupNorm(32, C, eps=1e-6) at every norm site, its
                                    statistics over the view the reference's call site passes (model_3dcausal.py:30-34;
                                    parameters at "<norm>.weight" / ".bias", no ".norm" level); never fused into an epilogue */
  int32_t fsq_num_codebooks;     /* FSQRegularizer num_codebooks (0 or 1 = one): indices carry the codebook axis last,
                                    [B][T'][H'][W'][c] (regularizers.py:131-133)                                  */
  int32_t fsq_dim;               /* FSQRegularizer dim (0 = len(levels) * num_codebooks): when it differs, z_channels = dim and the
                                    quantiser sits between project_in / project_out (nn.Linear along the channel axis,
                                    "regularization.project_in.weight" ..., regularizers.py:137-139,225,255)       */
} vt_model_config;
typedef struct vt_model vt_model;
int vt_model_config_size(void);    /* sizeof(vt_model_config) as compiled: lets a binding verify its struct mirror */
int vt_create(const vt_model_config* cfg, int32_t compute_dtype, vt_model** out);
int vt_destroy(vt_model* h);
int vt_load_weight(vt_model* h, const char* ref_key, const float* data_host, const int64_t* shape, int32_t ndim);
int vt_weight_count(vt_model* h);
const char* vt_weight_name(vt_model* h, int32_t i);
int vt_weight_shape(vt_model* h, int32_t i, int64_t* shape5, int32_t* ndim);   /* the shape vt_load_weight expects for key i */
int64_t vt_workspace_bytes(vt_model* h, int32_t B, int32_t T, int32_t H, int32_t W);
int vt_latent_dims(const vt_model* h, int32_t T, int32_t H, int32_t W, int32_t* out4);
int vt_encode(vt_model* h, const float* x, int32_t B, int32_t T, int32_t H, int32_t W, float* h_out, void* workspace,
              int64_t workspace_bytes, vt_stream stream);
int vt_regularize_kl(vt_model* h, const float* moments, const float* noise, float* z, float* kl_out, int32_t B, int32_t Tz,
                     int32_t Hz, int32_t Wz, vt_stream stream);
int vt_regularize_fsq(vt_model* h, const float* pre, float* z, int32_t* indices, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz,
                      vt_stream stream);
int vt_indices_to_latent(vt_model* h, const int32_t* indices, float* z, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz,
                         vt_stream stream);    /* FSQ: decode(indices, decode_from_indices=True) = this, then vt_decode */
int vt_decode(vt_model* h, const float* z, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz, float* x_out, void* workspace,
              int64_t workspace_bytes, vt_stream stream);
int vt_reset_cache(vt_model* h);
int vt_prepare(vt_model* h);       /* pack + upload every weight now (blocking) instead of at first use */
int vt_regularize_fsq_aux(vt_model* h, const float* pre, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz, float inv_temperature,
                          float* work, float* out3, vt_stream stream);
int32_t vt_tile_latent_frames(const vt_model* h, int32_t T, int32_t t_chunk_enc);
int64_t vt_tile_workspace_bytes(vt_model* h, int32_t B, int32_t T, int32_t H, int32_t W, int32_t t_chunk_enc, int32_t use_overlap);
int vt_tile_encode(vt_model* h, const float* x, int32_t B, int32_t T, int32_t H, int32_t W, int32_t t_chunk_enc, float* h_out,
                   void* workspace, int64_t workspace_bytes, vt_stream stream);
int vt_tile_decode(vt_model* h, const float* z, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz, int32_t t_chunk_dec, int32_t use_overlap,
                   float* x_out, void* workspace, int64_t workspace_bytes, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * Sessions of the v1.1 models (version 1): the temporal tiling above, fed as the frames arrive -- a live feed, a camera, the
 * tokens of an autoregressive model -- instead of from one whole clip.  Same chunk schedule ([0,1), [1,1+c), [1+c,1+2c) ...),
 * same kernels: the concatenated outputs of push* + finish equal vt_tile_encode / vt_tile_decode byte for byte, however the
 * input is split into pushes.  A session owns its causal state (one buffer per module cache) and the frames of its incomplete
 * chunk, both sized at create by a dry walk, so a push runs no hipMalloc and no device synchronisation, and device memory is
 * bounded by the chunk, not by the length of the video.  Several sessions may be open on one handle: each push swaps the
 * session's state in for its duration (one call at a time per handle, as for every other call).
 *   vt_session_create(h, kind, B, H, W, t_chunk, use_overlap, &s)
 *       kind VT_SESSION_ENCODE: frames [B][in_channels][n][H][W] in, pre-regularizer moments [B][C'][n'][H'][W'] out (the caller
 *         runs vt_regularize_* on each emitted slice, as after vt_tile_encode); t_chunk = t_chunk_enc, a multiple of the
 *         temporal factor f.  Chunk 0 is the first frame alone: its latent comes back from the first push.
 *       kind VT_SESSION_DECODE: latents [B][z_channels][n][H'][W'] in (H, W = H', W'), frames [B][out_ch][n][H'*s][W'*s] out;
 *         t_chunk = t_chunk_dec.  Without overlap a chunk is decoded when it is complete; with use_overlap, once the latent
 *         after it has arrived (one latent frame of latency) or at finish.
 *   vt_session_workspace_bytes(s)          workspace of every push / finish of the session (-1: bad session)
 *   vt_session_push(s, in, n, out, out_cap_frames, &n_out, ws, ws_bytes, stream)   n >= 1 frames; writes the n_out frames of
 *                                          every chunk the push completed to out[:, :, 0:n_out] (out has out_cap_frames frames;
 *                                          at most (n + t_chunk) / f + 1 latent frames for an encode, (n + t_chunk + 1) * f
 *                                          frames for a decode; a push that would not fit is refused before anything runs)
 *   vt_session_finish(s, out, out_cap_frames, &n_out, ws, ws_bytes, stream)   runs the incomplete last chunk, if any; the
 *                                          session takes no frames afterwards
 *   vt_session_destroy(s)                  frees the session's buffers (synchronises the device: work may still be queued on them)
 * ---------------------------------------------------------------------------------------- */
#define VT_SESSION_ENCODE 0
#define VT_SESSION_DECODE 1
typedef struct vt_session vt_session;
int vt_session_create(vt_model* h, int32_t kind, int32_t B, int32_t H, int32_t W, int32_t t_chunk, int32_t use_overlap, vt_session** out);
int64_t vt_session_workspace_bytes(const vt_session* s);
int vt_session_push(vt_session* s, const float* in, int32_t n, float* out, int32_t out_cap_frames, int32_t* n_out, void* workspace,
                    int64_t workspace_bytes, vt_stream stream);
int vt_session_finish(vt_session* s, float* out, int32_t out_cap_frames, int32_t* n_out, void* workspace, int64_t workspace_bytes,
                      vt_stream stream);
int vt_session_destroy(vt_session* s);

/* ------------------------------------------------------------------------------------------
 * Video front / back end around model(x): the device halves of scripts/inference_reconstruct.py (the codec --
 * decord / torchvision.io.write_video -- stays with the caller).  B = 1 like the reference's DataLoader.
 * vt_frames_u8_to_ncthw: decoded frames uint8 [T][H0][W0][3] -> x fp32 [3][Tdst][H][W], frames t_off .. t_off+T:
 *   v/255, torchvision Resize(size, antialias=True) to (Hr, Wr) (= ATen's separable anti-aliased bilinear filter,
 *   horizontal pass then vertical pass in fp32; Hr == H0 and Wr == W0 is the identity), CenterCrop window
 *   [top, top+H) x [left, left+W) of the resized frame, Normalize(0.5, 0.5) = (v-0.5)/0.5
 *   (inference_reconstruct.py:39-45,70-73; vidtok/data/vidtok.py:180-188).  `work`: vt_frames_work_floats(T, H0, W) floats.
 * vt_ncthw_to_frames_u8: x fp32 [3][Tsrc][H][W] frames t0 .. t0+n -> out uint8 [n][H][Wtot][3] at column w_off:
 *   clamp(-1,1), (x+1)/2, *255, truncation (tensor_to_uint8, inference_reconstruct.py:76-80; w_off / Wtot place the
 *   input next to the reconstruction for --concate_input, :228-235).
 * vt_ncthw_copy_frames: dst[c][td0+k] = (clamp ? clamp(src[c][ts0+k], -1, 1) : src[c][ts0+k]), k < n, for C channels of
 *   [C][T*][HW] tensors: the --pad_gen_frames chaining (last f-1 generated frames prepended to the next clip, :213-221).
 * ------------------------------------------------------------------------------------------ */
int64_t vt_frames_work_floats(int32_t T, int32_t H0, int32_t W);
int vt_frames_u8_to_ncthw(const uint8_t* frames, int32_t T, int32_t H0, int32_t W0, int32_t Hr, int32_t Wr, int32_t top,
                          int32_t left, float* x, int32_t Tdst, int32_t t_off, int32_t H, int32_t W, float* work,
                          vt_stream stream);
int vt_ncthw_to_frames_u8(const float* x, int32_t Tsrc, int32_t t0, int32_t n, int32_t H, int32_t W, uint8_t* out,
                          int32_t Wtot, int32_t w_off, vt_stream stream);
int vt_ncthw_copy_frames(const float* src, float* dst, int32_t C, int32_t Ts, int32_t Td, int32_t ts0, int32_t td0,
                         int32_t n, int64_t HW, int32_t clamp, vt_stream stream);

/* copy `n` frames of `frame_elems` elements each: dst frame j <- src frame idx_host[j]
 * (cache maintenance of the v1.1 chunked path, model_3dcausal_v1_1.py:172-176,230-234);
 * src/dst are [B][Ts|Td][frame_elems] with the given batch strides, element size `esize`. */
int vt_gather_frames(const void* src, void* dst, int32_t esize, int32_t B, int64_t frame_elems,
                     int64_t src_bstride, int64_t dst_bstride, const int32_t* idx_host, int32_t n,
                     vt_stream stream);

/* many small device-to-device copies in one launch: entry i of `table` (a DEVICE array of n entries) copies bytes_i bytes from
 * src_i to dst_i (ranges must not overlap).  16-byte vector accesses where both ends are 16-byte aligned, narrower otherwise; any
 * size.  The table is read on the device, so the launch may be captured into a graph.  `max_bytes` (the largest entry, or any
 * estimate) only sizes the grid.  A session switch of a v1.1 model (its dozens of chunk caches in / out) is two such launches. */
typedef struct vt_copy_segment {
  const void* src;
  void* dst;
  int64_t bytes;
} vt_copy_segment;
int vt_copy_segments(const vt_copy_segment* table, int32_t n, int64_t max_bytes, vt_stream stream);

/* nn.Linear along the channel axis of an NCTHW fp32 tensor viewed as [B][Cin][S] -> [B][Cout][S]:
 * FSQRegularizer.project_in / project_out when dim != len(levels) (vidtok/modules/regularizers.py:137-139,225,255).
 * w [Cout][Cin] row-major, bias [Cout] or NULL. */
int vt_channel_linear(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t Cin,
                      int32_t Cout, int64_t S, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * evaluation metrics of the reference's eval loop: per frame
 *   out = clamp(y,-1,1); x,out -> (.+1)/2                          scripts/inference_evaluate.py:175-176
 *   psnr = -10 log10(mean_{c,h,w}(x-out)^2 + 1e-8)                  vidtok/modules/util.py:146-154
 *   ssim = mean_c mean_{h,w} SSIM map, 11x11 Gaussian sigma 1.5      vidtok/modules/util.py:157-222
 * x, y NCTHW fp32 [B][C][T][H][W]; psnr, ssim [B][T]; work: vt_eval_work_floats() floats of scratch.
 * raw = 1: x, y are the model's input / output in [-1,1], the post-processing above is applied inside;
 * raw = 0: x, y are already [0,1] images (the argument convention of compute_psnr / compute_ssim).
 * (The reference averages these per-frame values over 16-frame splits: a mean of means of equal size.)
 * ---------------------------------------------------------------------------------------- */
int64_t vt_eval_work_floats(int32_t B, int32_t T);
int vt_eval_psnr_ssim(const float* x, const float* y, float* psnr, float* ssim, float* work, int32_t B, int32_t C,
                      int32_t T, int32_t H, int32_t W, int32_t raw, vt_stream stream);

/* ------------------------------------------------------------------------------------------
 * LPIPS, the third metric of the reference's eval loop (scripts/inference_evaluate.py:164-186), on VGG16 features
 * (vidtok/modules/lpips.py).  Per image pair n of N:
 *   ScalingLayer  (v - shift) / scale, shift = [-0.030, -0.088, -0.188], scale = [0.458, 0.448, 0.450]   lpips.py:98-105
 *   vgg16         features[0:30]: 3x3 conv s1 p1 + bias + ReLU, MaxPool2d(2, 2) (floor) at 4, 9, 16, 23;
 *                 taps relu1_2 (64 ch), relu2_2 (128, /2), relu3_3 (256, /4), relu4_3 (512, /8), relu5_3 (512, /16)   lpips.py:126-163
 *   per tap k     f / (sqrt(sum_c f^2) + 1e-10) for both images, (a - b)^2, 1x1 conv C -> 1 without bias (linK),
 *                 spatial mean                                                                      lpips.py:82-95,166-172
 *   lpips[n]      = sum over the 5 taps of the means (the reference's [N,1,1,1])
 * The host drives it as: vt_lpips_prep -> 13 x vt_conv_act (a VGG slice at a time, the input frames and the reconstruction frames
 * of all pairs in one launch) -> vt_lpips_tap after each slice (its pooled output feeds the next slice) -> vt_lpips_finish.
 * Deterministic (no floating-point atomics; a fixed partition of the pixels per shape, fixed-order sums), no allocation, no host
 * synchronisation: graph-capture safe.  Arithmetic of the convolutions: dtype (VT_F32 / VT_BF16 / VT_F16); the head runs in fp32.
 *
 * vt_conv_act: vt_conv (same descriptor, same contract) followed by an activation of the fp32 result before the rounding to
 *   out_dtype; act = VT_ACT_RELU (torch.nn.ReLU after each VGG16 conv, lpips.py:130 via torchvision features).  Supported: dtype
 *   VT_F32 / VT_BF16 / VT_F16 with out_dtype == dtype, NDHWC output, no residual, no LayerNorm, nbatch 1, no interleave; Cout > 64
 *   needs Cin a multiple of 16 bytes' worth of K step (32 fp32 / 64 16-bit values).  VGG's first layer: Cin 3 stored as 8.
 * vt_lpips_prep: x, y fp32 NCTHW [B][3][T][H][W] (T = 1: NCHW) -> out [2N][H][W][8] in dtype, N = B*T, frame n = b*T + t: frames
 *   0..N-1 from x, N..2N-1 from y, channels 3..7 zero.  Per value, in fp32 and in the reference's statement order:
 *     flags & VT_LPIPS_CLAMP_Y    y only: clamp(v, -1, 1)                    (output.clamp(-1, 1), inference_evaluate.py:175)
 *     flags & VT_LPIPS_ROUNDTRIP  u = (v + 1) / 2; v = u * 2 - 1             ((x+1)/2 then inp*2-1, :176,186)
 *     flags & VT_LPIPS_UNIT       v = v * 2 - 1                              ([0,1] images, the compute_psnr convention)
 *     (v - shift[c]) / scale[c]                                             (a true division; shift, scale: fp32 [3] on the device)
 * vt_lpips_tap: feat = relu_k [2N][H][W][C] (dtype, C in 64 / 128 / 256 / 512) of tap k = `tap` (0..4), lin_w fp32 [C]: writes the
 *   pixel sums of sum_c lin_w[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2 (a = frame n, b = frame n + N) into the
 *   workspace, and, if pooled != NULL, pooled [2N][H/2][W/2][C] = MaxPool2d(2, 2) of feat (bit-exact; odd sizes floor).
 * vt_lpips_finish: lpips[n] (fp32 [N]) = sum over taps of the means; tap_means (fp32 [5][N]) or NULL.  H, W: the input size.
 * work: vt_lpips_work_bytes(N, H, W) bytes (16-byte aligned), shared by the taps and the finish of one LPIPS pass.
 * Arguments are checked before any device work: VT_ERR_ARG for a dtype other than F32 / BF16 / F16, C outside 64 / 128 / 256 / 512,
 * null tensors, a workspace below vt_lpips_work_bytes, or an input H or W below 16 (relu5_3 would be empty).
 * ---------------------------------------------------------------------------------------- */
#define VT_ACT_RELU 1
#define VT_LPIPS_CLAMP_Y 1
#define VT_LPIPS_ROUNDTRIP 2
#define VT_LPIPS_UNIT 4
int vt_conv_act(const vt_conv_desc* d, int32_t act, vt_stream stream);
int64_t vt_lpips_work_bytes(int32_t N, int32_t H, int32_t W);     /* 0 for invalid sizes */
int vt_lpips_prep(const float* x, const float* y, void* out, const float* shift, const float* scale, int32_t dtype, int32_t B,
                  int32_t T, int32_t H, int32_t W, int32_t flags, vt_stream stream);
int vt_lpips_tap(const void* feat, void* pooled, const float* lin_w, void* work, int64_t work_bytes, int32_t dtype, int32_t N,
                 int32_t H, int32_t W, int32_t C, int32_t tap, vt_stream stream);
int vt_lpips_finish(const void* work, int64_t work_bytes, float* lpips, float* tap_means, int32_t N, int32_t H, int32_t W,
                    vt_stream stream);

/* ---- differentiable LPIPS: the gradient with respect to the reconstruction (the second image of every pair) ---------------------
 * VGG16 and the lin layers are frozen and the first image is the ground truth, so the backward runs over the N reconstruction frames
 * (frames N..2N-1 of the forward's stack) only, from relu5_3 down: vt_lpips_tap_backward at each tap, vt_conv_dgrad (weights packed
 * by vt_pack_conv_weight_dgrad) through each of the 13 convolutions, vt_relu_backward on the dx of a convolution whose input is a
 * non-tap ReLU output, vt_lpips_prep_backward at the bottom.  dtype VT_F32 or VT_BF16 (VT_ERR_ARG otherwise).  No atomics, every sum
 * in a fixed order (two runs give the same bits), no allocation, no synchronisation.
 *
 * vt_lpips_tap_backward: feat = relu_k [2N][H][W][C] (dtype, C in 64 / 128 / 256 / 512: f0 = frame n, f1 = frame n + N), lin_w fp32
 *   [C], gout fp32 [N] = dL/dlpips[n], dpool [N][H/2][W/2][C] (dpool_dtype: dtype or VT_F32) = the data gradient of the next slice's
 *   first convolution, or NULL (relu5_3).  Writes dfeat [N][H][W][C] (dtype) = dL/d(pre-activation of the tap's convolution) in one
 *   pass: per element the fp32 sum of two terms, masked by f1 > 0 (the ReLU of the tap's own convolution), rounded once.
 *     head term, per pixel, all fp32 (eps = 1e-10):
 *       s_i = ||f_i||_2, u_i = f_i / (s_i + eps)
 *       e_c = 2 gout[n] lin_w[c] (u1_c - u0_c) / (H W)
 *       d/df1_c = e_c / (s1 + eps) - f1_c (sum_j e_j f1_j) / (s1 (s1 + eps)^2)
 *       At s1 = 0 the second term is DEFINED as 0.  This is the one divergence from torch autograd, which returns NaN there (0/0
 *       in the backward of sqrt); with the mask f1 > 0 the whole pixel's gradient is then 0.
 *     pool term: dpool[n][h/2][w/2][c] goes to the FIRST maximum of f1 over the 2 x 2 window in row-major order (0,0), (0,1), (1,0),
 *       (1,1), as F.max_pool2d's backward routes it (equal positive bf16 values do occur).  A last row or column no window covers
 *       (odd H or W) gets the head term only.
 * vt_relu_backward: dx[i] = y[i] > 0 ? dy[i] : 0 for i < n (n a multiple of 8): y the saved post-ReLU output (dtype), dy in dy_dtype
 *   (dtype or VT_F32: the fp32 dx of vt_conv_dgrad, rounded here once), dx in dtype.  Bit-exact.
 * vt_lpips_prep_backward: d [N][H][W][8] (dtype; channels 0..2 real) -> dtarget fp32 [N][3][H][W] = d[..][c] / scale[c] (a true
 *   division): the adjoint of vt_lpips_prep with flags = 0.
 * All tensors 16-byte aligned. */
int vt_lpips_tap_backward(const void* feat, const float* lin_w, const float* gout, const void* dpool, int32_t dpool_dtype, void* dfeat,
                          int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, vt_stream stream);
int vt_relu_backward(const void* dy, int32_t dy_dtype, const void* y, void* dx, int32_t dtype, int64_t n, vt_stream stream);
int vt_lpips_prep_backward(const void* d, int32_t dtype, const float* scale, float* dtarget, int32_t N, int32_t H, int32_t W,
                           vt_stream stream);

/* ---- backward reductions (decoder fine-tuning) ---------------------------------------------------------------------------
 * vt_conv_wgrad: the weight / bias gradient of one forward convolution (vt_conv geometry):
 *   dw[co][ci][a][p][q] = sum over output pixels (b, to, ho, wo) of dy[b][to][ho][wo][co] * x[b][ti][hi][wi][ci]
 *     with ti = to*st - pt + a, hi = ho*sh - ph + p, wi = wo*sw - pw + q in the (ups_t / ups_s: nearest x2) up-sampled input,
 *     zero outside it, and ti < 0 read as frame 0 under tmode VT_TPAD_REPLICATE;
 *   db[co] = sum over output pixels of dy[..][co] (db may be NULL).
 * x: NDHWC [B][Ti][Hi][Wi][ldx] (the stored channels; only the first Cin reach dw), dy: NDHWC [B][To][Ho][Wo][lddy], both of
 * `dtype` (VT_F32 or VT_BF16; MFMA products, fp32 accumulation).  dw: fp32 [Cout][Cin][KT][KH][KW] (the reference's layout), db:
 * fp32 [Cout]; both are overwritten.  The reduction over pixels is split into ranges that each write an fp32 partial tile into
 * `work` (vt_conv_wgrad_work_bytes(d) bytes, -1 for an invalid descriptor) and a second launch adds the ranges in index order:
 * no atomics, results are bit-reproducible and the pair is graph-capture safe.  The split depends on the shape only.
 * Checked before any device work: VT_ERR_ARG for another dtype, tmode other than ZERO / REPLICATE, ups other than 0 / 1, an
 * output extent the geometry cannot produce from the input ((To-1)*st + KT <= (Ti << ups_t) + pt + pt_hi, likewise H, W),
 * more than 2^31 output pixels, or a workspace below the size asked for.
 * ---------------------------------------------------------------------------------------------------------------------- */
typedef struct vt_wgrad_desc {
  const void* x;
  const void* dy;
  float* dw;
  float* db;
  void* work;
  int64_t work_bytes;
  int32_t B, Ti, Hi, Wi, ldx, Cin;
  int32_t To, Ho, Wo, lddy, Cout;
  int32_t KT, KH, KW, st, sh, sw;
  int32_t pt, ph, pw, pt_hi, ph_hi, pw_hi;
  int32_t tmode, ups_t, ups_s, dtype;
} vt_wgrad_desc;
int vt_wgrad_desc_size(void);
int64_t vt_conv_wgrad_work_bytes(const vt_wgrad_desc* d);
int vt_conv_wgrad(const vt_wgrad_desc* d, vt_stream stream);

/* vt_layernorm_act_backward: backward of vt_layernorm_act (n = [SiLU](gamma * (y - mean) * rstd + beta) over the first C of ld
 * channels of each of M rows).  y: the saved pre-norm rows, dn: dL/dn, both `dtype` (VT_F32 / VT_BF16) with row stride ld;
 * mean / rstd are recomputed from y in fp32.  Writes dx = dL/dy (dx_dtype: dtype or VT_F32, row stride ldo; lanes C..ldo-1 get
 * zeros, ldo within the 64-multiple above C), dgamma and dbeta (fp32 [C], overwritten; either may be NULL) as per-workgroup
 * partials in `work` (vt_layernorm_act_backward_work_bytes(M, C) bytes, -1 if C > 512) added in index order by a second launch.
 * -------------------------------------------------------------------------------------------------------------------------- */
int64_t vt_layernorm_act_backward_work_bytes(int64_t M, int32_t C);
int vt_layernorm_act_backward(const void* y, const void* dn, int32_t dtype, int64_t ld, void* dx, int32_t dx_dtype, int64_t ldo,
                              const float* gamma, const float* beta, float* dgamma, float* dbeta, int64_t M, int32_t C, float eps,
                              int32_t silu, void* work, int64_t work_bytes, vt_stream stream);

/* ---- differentiable decode: the data-gradient path (decoder fine-tuning) ------------------------------------------------------
 * vt_conv_dgrad: dx = the gradient of a vt_conv with respect to its stored input x [B][Ti][Hi][Wi][lddx] (before a folded nearest x2
 * up-sampling), from dy [B][To][Ho][Wo][lddy] (dtype VT_F32 / VT_BF16; pad lanes of dy may hold any finite value).  The MACs run on
 * vt_conv itself.  An input pixel of parity class (rh, rw) = (h mod sh, w mod sw) receives only the taps k with (r + p - k) mod s = 0:
 * per class, dx is a stride-1 convolution of dy with the flipped, transposed sub-kernel of those taps (vt_pack_conv_weight_dgrad)
 * under the front pad nk - 1 - (r + p) / s.  Stride 1 is one class with every tap under the mirrored pads K-1-p; k4 s2 p1 is four
 * 2 x 2 kernels, 16 tap products per 4 pixels, no zero-dilated dy; a class without a pixel (extent <= r) takes no launch.  A stride-1 geometry
 * without replicate pad or ups and with fp32 dx is written by that one launch (acc rides its residual epilogue; lanes Cin..lddx-1 of
 * dx are NOT written then: hand in a zeroed dx where they matter).  Otherwise the class convolutions write fp32 into `work`
 * (vt_conv_dgrad_work_bytes(d) bytes; 0 = none needed, -1 = invalid descriptor; a lone class takes exactly its size, several classes
 * a multiple of 256 bytes each) and one finishing launch reads them: an output pixel sums its virtual positions -- under
 * VT_TPAD_REPLICATE the pt virtual front frames add into frame 0, under ups_t / ups_s the 2 / 2 x 2 up-sampled positions add into
 * their source pixel; under a stride it is the one position of the pixel's class -- then acc (dx_dtype, row stride ldacc) is added
 * and the fp32 sum is rounded ONCE to dx_dtype (dtype or VT_F32), pad lanes zero.  A bf16 dx is therefore the rounded fp32 dx bit for bit.  No atomics; sums in a fixed
 * order; capture-safe.
 * Served: strides (1, 1, 1) with a zero or replicate time pad, ups_t / ups_s, up to 64 taps; st = 1 with sh, sw in {1, 2} and at
 * least one 2 under VT_TPAD_ZERO without ups, KT, KH, KW <= 4, dy extents the forward's ((Hi + ph + ph_hi - KH) / sh + 1).  Everything
 * else returns VT_ERR_ARG with a message: st != 1, stride 3, a stride with ups or a replicate pad, tmode VT_TPAD_CACHE, pads >= the
 * kernel extent, pads that would put a class convolution in front of dy's first pixel (nk - 1 < (r + p) / s), dy extents that are
 * not the forward convolution's.
 * vt_pack_conv_weight_dgrad: weight fp32 [Cout][Cin][KT][KH][KW] -> sh * sw blocks [Cin][ldw], block rh * sw + rw holding the class's
 * taps flipped (k = ((a' nkh + p') nkw + q') cout_p + co <- w[co][ci][KT-1-a'][kh0 + sh (nkh-1-p')][kw0 + sw (nkw-1-q')]), zeros
 * elsewhere; ldw >= KT ceil(KH / sh) ceil(KW / sw) cout_p, the same for every block.  sh = sw = 1: one block, all taps flipped.
 * vt_grad_fold: the finishing kernel of one class on its own (src [B][rep + (T << ups_t)][H << ups_s][W << ups_s][lds], fp32 or dx_dtype) -- with
 * rep = 0, ups_t = 1 it is the backward of a nearest x2 time up-sampling.
 * ---------------------------------------------------------------------------------------------------------------------- */
typedef struct vt_dgrad_desc {
  const void* dy;
  const void* wt;        /* vt_pack_conv_weight_dgrad blocks [sh * sw][Cin][ldw] in `dtype` */
  void* dx;
  const void* acc;       /* optional: a gradient already held for x, added (dx_dtype) */
  void* work;
  int64_t work_bytes;
  int32_t B, Ti, Hi, Wi, lddx, Cin;
  int32_t To, Ho, Wo, lddy, Cout;
  int32_t KT, KH, KW, st, sh, sw;
  int32_t pt, ph, pw, pt_hi, ph_hi, pw_hi;
  int32_t tmode, ups_t, ups_s, dtype, dx_dtype;
  int32_t ldw, ldacc;
} vt_dgrad_desc;
int vt_dgrad_desc_size(void);
int vt_pack_conv_weight_dgrad(const float* w, void* out, int32_t out_dtype, int32_t Cout, int32_t Cin, int32_t cout_p, int32_t KT,
                              int32_t KH, int32_t KW, int32_t sh, int32_t sw, int32_t ph, int32_t pw, int64_t ldw, vt_stream stream);
int64_t vt_conv_dgrad_work_bytes(const vt_dgrad_desc* d);
int vt_conv_dgrad(const vt_dgrad_desc* d, vt_stream stream);
int vt_grad_fold(const void* src, int32_t src_dtype, const void* acc, void* dx, int32_t dx_dtype, int32_t B, int32_t T, int32_t H, int32_t W, int32_t C,
                 int32_t lds, int32_t lda, int32_t ldo, int32_t rep, int32_t ups_t, int32_t ups_s, vt_stream stream);

/* vt_softmax_rows_backward: ds = scale * p * (dp - rowsum(dp * p)) for p = softmax(scale * s): p [rows][ldp] (dtype VT_F32 / VT_BF16),
 *   dp fp32 [rows][cols], ds [rows][ldo] in dtype with columns cols..ldo-1 zero; a row's arithmetic is fp32.
 * vt_transpose_batched: out[z][c][r] = in[z][r][c] (in [Z][R][ldi], first C columns; out [Z][C][ldo], columns R..ldo-1 zero): the
 *   K-contiguous operands of the attention backward's GEMMs (dV = P^T dO, dQ = dS K, dK = dS^T Q on vt_conv's batched GEMM form).
 * vt_upsample_mix: y = a u + (1 - a) c, a = sigmoid(*mix_factor), over the first C of ld channels of M rows (pad lanes zero): the
 *   alpha-mix of TimeUpsampleResCausal2x as a pass of its own, so that the training forward keeps both operands.
 * vt_upsample_mix_backward: du = a dy, dc = (1 - a) dy (pad lanes zero) and dmix[0] = a (1 - a) sum(dy (u - c)): per-workgroup fp32
 *   partials in `work` (vt_upsample_mix_backward_work_bytes(M, ld) bytes), added in index order by a second launch.
 * vt_time_lerp2x_backward: the adjoint of vt_time_lerp2x: dy [B][2 Ti][HWC] -> dx [B][Ti][HWC].
 * vt_grad_ncthw_to_ndhwc: the cotangent fp32 [B][C][T][H][W] -> [B][tpad + T][H][W][ldy] with the tpad front frames (the ones a
 *   v1.0 decode trims) and the pad lanes zero.
 * vt_grad_add: out = a + b (fp32 sum, one rounding), the junction of a residual path with a LayerNorm's gradient.
 * All: dtype VT_F32 or VT_BF16, no atomics, fixed summation order, capture-safe on the caller's stream. */
int vt_softmax_rows_backward(const void* p, int64_t ldp, const float* dp, void* ds, int64_t ldo, int32_t dtype, int64_t rows,
                             int32_t cols, float scale, vt_stream stream);
int vt_transpose_batched(const void* in, void* out, int32_t dtype, int32_t Z, int32_t R, int32_t C, int64_t ldi, int64_t ldo,
                         vt_stream stream);
int vt_upsample_mix(const void* u, const void* c, const float* mix_factor, void* y, int32_t dtype, int64_t M, int32_t C, int32_t ld,
                    vt_stream stream);
int64_t vt_upsample_mix_backward_work_bytes(int64_t M, int32_t ld);
int vt_upsample_mix_backward(const void* dy, const void* u, const void* c, const float* mix_factor, void* du, void* dc, float* dmix,
                             int32_t dtype, int64_t M, int32_t C, int32_t ld, void* work, int64_t work_bytes, vt_stream stream);
int vt_time_lerp2x_backward(const void* dy, void* dx, int32_t dtype, int32_t B, int32_t Ti, int64_t HWC, vt_stream stream);
int vt_grad_ncthw_to_ndhwc(const float* x, void* y, int32_t out_dtype, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W,
                           int32_t ldy, int32_t tpad, vt_stream stream);
int vt_grad_add(const void* a, const void* b, void* out, int32_t dtype, int64_t n, vt_stream stream);

/* ---- PatchGAN discriminator (reference vidtok/modules/discriminator.py:88-137, the adversarial term of losses.py:187-249) -----------
 * NLayerDiscriminator is Conv2d k4 (s2, s2, s2, s1, s1) with BatchNorm2d + LeakyReLU(0.2) between; its convolutions are vt_conv, its
 * weight gradients vt_conv_wgrad, its data gradients vt_conv_dgrad.  The entry points below are the rest.  All take VT_F32 /
 * VT_BF16 (VT_ERR_ARG otherwise, fp16 included: there is no loss scaling here), compute in fp32, use no float atomics, reduce over rows
 * through per-workgroup partials in the caller's `work` added in index order by a second launch (bit-reproducible), neither allocate
 * nor synchronise (capture-safe on `stream`), and write zeros into the pad lanes C..ld-1 of every row they own.  Rows are the M pixels
 * of an NDHWC tensor, row strides multiples of 8, C <= 512, tensors 16-byte aligned.
 *
 * vt_batchnorm_stats: mean[c] and the BIASED variance var[c] over the M rows of x [M][ld], fp32 [C]; rstd[c] = 1 / sqrt(var[c] + eps)
 *   as well where rstd != NULL.  The partial sums of x and x^2 are fp64 (work: vt_batchnorm_stats_work_bytes(M, C) bytes, -1 for
 *   C > 512), so a mean far from zero costs no digits of the variance.
 * vt_batchnorm_act: y = leaky(gamma[c] (x - mean[c]) rstd[c] + beta[c]), leaky(v) = v > 0 ? v : slope v.  The batch statistics of
 *   vt_batchnorm_stats (train mode), the running statistics (eval mode), or mean 0 / rstd 1 / gamma 1 / beta 0: a plain LeakyReLU,
 *   bit-exact (the discriminator's first layer).
 * vt_batchnorm_act_backward: x the saved convolution output, dy dL/dy (dy_dtype: dtype or VT_F32).  With pre the forward's
 *   pre-activation, recomputed by the same device expression (so the mask is the forward's bit for bit; pre == 0 takes `slope`, as
 *   torch), g = dy (pre > 0 ? 1 : slope) and x^ = (x - mean) rstd:
 *     dbeta[c] = sum g, dgamma[c] = sum g x^      (fp32 [C]; either may be NULL)
 *     mode VT_BN_BATCH:   dx = gamma rstd (g - sum g / M - x^ sum(g x^) / M)
 *     mode VT_BN_RUNNING: dx = gamma rstd g       (mean / rstd are constants of the call)
 *   dx in dtype, rounded once.  work: vt_batchnorm_act_backward_work_bytes(M, C) bytes.
 * vt_leaky_relu_backward: dx[i] = dy[i] (y[i] > 0 ? 1 : slope) for i < n (n a multiple of 8) from the saved POST-activation y -- the
 *   sign of y is the sign of the pre-activation because slope > 0 (slope <= 0 is refused); dy in dy_dtype (dtype or VT_F32), dx in
 *   dtype.  Bit-exact.
 * ---------------------------------------------------------------------------------------------------------------------- */
#define VT_BN_BATCH 0
#define VT_BN_RUNNING 1
int64_t vt_batchnorm_stats_work_bytes(int64_t M, int32_t C);
int vt_batchnorm_stats(const void* x, int32_t dtype, int64_t ld, int64_t M, int32_t C, float eps, float* mean, float* var, float* rstd,
                       void* work, int64_t work_bytes, vt_stream stream);
int vt_batchnorm_act(const void* x, int32_t dtype, int64_t ld, void* y, int64_t ldy, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, float slope, int64_t M, int32_t C, vt_stream stream);
int64_t vt_batchnorm_act_backward_work_bytes(int64_t M, int32_t C);
int vt_batchnorm_act_backward(const void* x, const void* dy, int32_t dtype, int32_t dy_dtype, int64_t ld, int64_t lddy, void* dx,
                              int64_t ldo, const float* mean, const float* rstd, const float* gamma, const float* beta, float slope,
                              float* dgamma, float* dbeta, int64_t M, int32_t C, int32_t mode, void* work, int64_t work_bytes,
                              vt_stream stream);
int vt_leaky_relu_backward(const void* dy, int32_t dy_dtype, const void* y, void* dx, int32_t dtype, int64_t n, float slope,
                           vt_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDTOK_AMD_H */
