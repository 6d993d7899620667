/* Sessions of libvidtok_amd.so from plain C: vidtok_kl_causal_488_16chn_v1_1 (pseudo-random weights, as in roundtrip.c) encodes
 * a synthetic clip pushed in ragged pieces through an encode session and decodes its latents through a decode session with the
 * look-ahead frame; both results are compared byte for byte with vt_tile_encode / vt_tile_decode of the whole clip.  Prints OK.
 *   cc -O2 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include examples/session_encode.c -o examples/session_encode \
 *      -L vidtok_amd -lvidtok_amd -L /opt/rocm/lib -lamdhip64 -lm -Wl,-rpath,$PWD/vidtok_amd -Wl,-rpath,/opt/rocm/lib
 *   ./examples/session_encode            (needs an MI355X) */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vidtok_amd.h"

#define CHECK(expr)                                                        \
  do {                                                                     \
    if ((expr) != 0) {                                                     \
      fprintf(stderr, "%s failed: %s\n", #expr, vt_last_error());          \
      return 1;                                                            \
    }                                                                      \
  } while (0)
#define HIP(expr)                                                          \
  do {                                                                     \
    hipError_t e_ = (expr);                                                \
    if (e_ != hipSuccess) {                                                \
      fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));           \
      return 1;                                                            \
    }                                                                      \
  } while (0)

static unsigned long long rng = 0x9E3779B97F4A7C15ull;
static float uniform(void) {                       /* [-1, 1) */
  rng = rng * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((rng >> 40) & 0xFFFFFF) / 8388608.0f - 1.0f;
}

/* device [B][C][T][HW] -> host, `n` frames of each (b, c) plane from frame t0 */
static int fetch(const float* dev, int planes, int T, int t0, int n, size_t hw, float* host) {
  for (int p = 0; p < planes; ++p)
    if (hipMemcpy(host + (size_t)p * n * hw, dev + ((size_t)p * T + t0) * hw, (size_t)n * hw * 4, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  return 0;
}

int main(void) {
  const int B = 1, T = 39, H = 64, W = 64, c = 16, f = 4;
  const int pushes[] = {1, 5, 16, 2, 15};          /* 39 frames in ragged pieces: chunks [0,1) [1,17) [17,33) and the partial [33,39) */
  vt_model_config cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.version = 1; cfg.interpolation_mode = 1;
  cfg.ch = 128; cfg.num_res_blocks = 2; cfg.in_channels = 3; cfg.out_ch = 3; cfg.z_channels = 16; cfg.double_z = 1;
  cfg.num_resolutions = 4;
  const int mult[4] = {1, 2, 4, 4};
  memcpy(cfg.ch_mult, mult, sizeof mult);
  cfg.n_spatial_ds = 3; cfg.spatial_ds[0] = 0; cfg.spatial_ds[1] = 1; cfg.spatial_ds[2] = 2;
  cfg.n_tempo_ds = 2; cfg.tempo_ds[0] = 2; cfg.tempo_ds[1] = 1;
  cfg.n_spatial_us = 3; cfg.spatial_us[0] = 1; cfg.spatial_us[1] = 2; cfg.spatial_us[2] = 3;
  cfg.n_tempo_us = 2; cfg.tempo_us[0] = 1; cfg.tempo_us[1] = 2;
  cfg.time_downsample_factor = f;
  vt_model* m = NULL;
  CHECK(vt_create(&cfg, VT_BF16, &m));
  for (int i = 0; i < vt_weight_count(m); ++i) {
    int64_t shape[5];
    int32_t nd;
    CHECK(vt_weight_shape(m, i, shape, &nd));
    long long n = 1, fan = 1;
    for (int k = 0; k < nd; ++k) n *= shape[k];
    for (int k = 1; k < nd; ++k) fan *= shape[k];
    float* w = (float*)malloc((size_t)n * sizeof(float));
    const char* key = vt_weight_name(m, i);
    const int is_norm_w = strstr(key, ".norm.weight") != NULL, is_vec = nd == 1;
    for (long long j = 0; j < n; ++j) w[j] = is_norm_w ? 1.0f + 0.1f * uniform() : (is_vec ? 0.05f * uniform() : uniform() * sqrtf(3.0f / (float)fan));
    CHECK(vt_load_weight(m, key, w, shape, nd));
    free(w);
  }
  CHECK(vt_prepare(m));
  int32_t ld[4];
  CHECK(vt_latent_dims(m, T, H, W, ld));
  const int tz = vt_tile_latent_frames(m, T, c), Hz = ld[2], Wz = ld[3], cm = ld[0];
  const size_t hw = (size_t)H * W, hwz = (size_t)Hz * Wz, nx = (size_t)B * 3 * T * hw;
  const size_t nm = (size_t)B * cm * tz * hwz, nz = (size_t)B * cfg.z_channels * tz * hwz, nd = (size_t)B * 3 * tz * f * hw;
  hipStream_t stream;
  HIP(hipStreamCreate(&stream));
  float *x, *mom, *z, *kl, *dec, *smom, *sdec;
  HIP(hipMalloc((void**)&x, nx * 4)); HIP(hipMalloc((void**)&mom, nm * 4)); HIP(hipMalloc((void**)&z, nz * 4));
  HIP(hipMalloc((void**)&kl, 4)); HIP(hipMalloc((void**)&dec, nd * 4));
  float* xh = (float*)malloc(nx * 4);
  for (size_t i = 0; i < nx; ++i) xh[i] = uniform();
  HIP(hipMemcpy(x, xh, nx * 4, hipMemcpyHostToDevice));
  /* the whole clip through the tiled calls */
  const int64_t wsb = vt_tile_workspace_bytes(m, B, T, H, W, c, 1);
  if (wsb < 0) { fprintf(stderr, "vt_tile_workspace_bytes: %s\n", vt_last_error()); return 1; }
  void* ws;
  HIP(hipMalloc(&ws, (size_t)wsb));
  CHECK(vt_tile_encode(m, x, B, T, H, W, c, mom, ws, wsb, stream));
  CHECK(vt_regularize_kl(m, mom, NULL, z, kl, B, tz, Hz, Wz, stream));
  CHECK(vt_tile_decode(m, z, B, tz, Hz, Wz, c / f, 1, dec, ws, wsb, stream));
  /* the same clip through an encode session, frame pieces as they might arrive from a camera.  The input of a push is a tensor
   * of its own ([B][3][n][H][W]): the clip's frames are gathered into a staging buffer first */
  vt_session *se, *sd;
  CHECK(vt_session_create(m, VT_SESSION_ENCODE, B, H, W, c, 0, &se));
  CHECK(vt_session_create(m, VT_SESSION_DECODE, B, Hz, Wz, c / f, 1, &sd));
  const int64_t wse = vt_session_workspace_bytes(se), wsd = vt_session_workspace_bytes(sd);
  void *ws_e, *ws_d;
  float* piece;
  HIP(hipMalloc(&ws_e, (size_t)wse)); HIP(hipMalloc(&ws_d, (size_t)wsd));
  HIP(hipMalloc((void**)&piece, (size_t)B * 3 * c * hw * 4));
  HIP(hipMalloc((void**)&smom, nm * 4)); HIP(hipMalloc((void**)&sdec, nd * 4));
  const int cap_e = c / f + 2, cap_d = (c / f + 4) * f;
  float *oe, *od;
  HIP(hipMalloc((void**)&oe, (size_t)B * cm * cap_e * hwz * 4)); HIP(hipMalloc((void**)&od, (size_t)B * 3 * cap_d * hw * 4));
  int t = 0, te = 0;
  for (size_t p = 0; p <= sizeof pushes / sizeof pushes[0]; ++p) {
    int32_t n_out = 0;
    if (p < sizeof pushes / sizeof pushes[0]) {
      const int n = pushes[p];
      CHECK(vt_ncthw_copy_frames(x, piece, B * 3, T, n, t, 0, n, (int64_t)hw, 0, stream));
      CHECK(vt_session_push(se, piece, n, oe, cap_e, &n_out, ws_e, wse, stream));
      t += n;
    } else {
      CHECK(vt_session_finish(se, oe, cap_e, &n_out, ws_e, wse, stream));
    }
    if (n_out > 0) CHECK(vt_ncthw_copy_frames(oe, smom, B * cm, cap_e, tz, 0, te, n_out, (int64_t)hwz, 0, stream));
    te += n_out;
  }
  /* ... and the tiled latents through a decode session, three latent frames per push */
  int td = 0;
  for (int a = 0; a <= tz; a += 3) {
    int32_t n_out = 0;
    if (a < tz) {
      const int n = tz - a < 3 ? tz - a : 3;
      float* zp = (float*)piece;
      CHECK(vt_ncthw_copy_frames(z, zp, B * cfg.z_channels, tz, n, a, 0, n, (int64_t)hwz, 0, stream));
      CHECK(vt_session_push(sd, zp, n, od, cap_d, &n_out, ws_d, wsd, stream));
    }
    if (n_out > 0) CHECK(vt_ncthw_copy_frames(od, sdec, B * 3, cap_d, tz * f, 0, td, n_out, (int64_t)hw, 0, stream));
    td += n_out;
  }
  {
    int32_t n_out = 0;
    CHECK(vt_session_finish(sd, od, cap_d, &n_out, ws_d, wsd, stream));
    if (n_out > 0) CHECK(vt_ncthw_copy_frames(od, sdec, B * 3, cap_d, tz * f, 0, td, n_out, (int64_t)hw, 0, stream));
    td += n_out;
  }
  HIP(hipStreamSynchronize(stream));
  if (te != tz || td != tz * f) {
    fprintf(stderr, "sessions emitted %d latent / %d output frames, the tiled calls %d / %d\n", te, td, tz, tz * f);
    return 2;
  }
  float *a = (float*)malloc(nd * 4), *b = (float*)malloc(nd * 4);
  if (fetch(mom, B * cm, tz, 0, tz, hwz, a) || fetch(smom, B * cm, tz, 0, tz, hwz, b)) return 1;
  const int enc_same = memcmp(a, b, nm * 4) == 0;
  if (fetch(dec, B * 3, tz * f, 0, tz * f, hw, a) || fetch(sdec, B * 3, tz * f, 0, tz * f, hw, b)) return 1;
  const int dec_same = memcmp(a, b, nd * 4) == 0;
  printf("encode session (pushes 1 5 16 2 15) vs vt_tile_encode: %s; decode session (3 latents per push, look-ahead) vs vt_tile_decode: %s\n",
         enc_same ? "identical" : "DIFFERENT", dec_same ? "identical" : "DIFFERENT");
  CHECK(vt_session_destroy(se));
  CHECK(vt_session_destroy(sd));
  CHECK(vt_destroy(m));
  if (!(enc_same && dec_same)) return 3;
  printf("OK\n");
  return 0;
}
