// Handle-level C-ABI (include/vidtok_amd.h, "model handle"): the stage graph of the causal v1.0 tokenizers -- what
// AutoencodingEngine.encode / decode run (reference vidtok/models/autoencoder.py:197-229 over EncoderCausal3DPadding /
// DecoderCausal3DPadding, vidtok/modules/model_3dcausal.py:502-885) -- driven from C++ over the operator entry points of
// this library, so that a host without Python runs the model:  vt_create(config) -> vt_load_weight(reference state_dict
// key, fp32 data) x N -> vt_encode / vt_regularize_* / vt_decode.
//
// It is the same graph as vidtok_amd/modules.py builds (same operators, same descriptors, same fusion decisions: which
// convolution emits which LayerNorm, the fused temporal block, the parity classes of the up-samplers), so its results
// equal the Python engine's bit for bit (tests/test_gpu_e2e.py::test_model_handle_matches_engine drives it through ctypes
// only).  Scope: `norm_type: layernorm`, `resamp_with_conv: true` -- every shipped causal config, v1.0 and v1.1 (first-frame
// replicate padding, nearest or trilinear time up-sampling, model_3dcausal_v1_1.py) as ONE pass over the clip, and the
// temporal TILING of v1.1 (vt_tile_encode / vt_tile_decode: the chunk schedule, the per-module causal caches, the decoder's
// look-ahead frame with its cache offsets -- AutoencodingEngine.tile_encode / tile_decode, autoencoder_v1_1.py:202-331); and
// (version 2) the non-causal family, Encoder3D / Decoder3D of model_3dnoncausal.py:314-651: the same stages with centred temporal
// windows and plain nn.Conv parameter keys.
//
// The vocabulary is the Python host's: a `Site` is one convolution as the kernels see it (packing.ConvSite: key, window, weight
// transform, chunk state; built once by the graph builders, which is where the parameter list comes from), `residual_block` the one
// body of the residual stages, `keep_frames` the one way a module keeps frames as its chunk cache, `guarded` the one exception
// boundary of the extern "C" entries.
//
// Memory: weights are packed on the host when first used and live in device allocations owned by the handle;
// activations come from a caller-provided workspace, cut into two arenas that alternate between stages (a stage reads the
// previous stage's output from one arena and builds its own output and temporaries in the other);
// vt_workspace_bytes() runs the graph dry to size it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "../../include/vidtok_amd.h"

void vt_set_error(const char* fmt, ...);

namespace {

struct Fail {
  int code;
};
#define M_CHECK(cond, ...)        \
  do {                            \
    if (!(cond)) {                \
      vt_set_error(__VA_ARGS__);  \
      throw Fail{VT_ERR_ARG};     \
    }                             \
  } while (0)
#define M_CALL(expr)                 \
  do {                               \
    const int rc_ = (expr);          \
    if (rc_ != VT_OK) throw Fail{rc_}; \
  } while (0)
#define M_HIP(expr)                                                        \
  do {                                                                     \
    const hipError_t e_ = (expr);                                          \
    if (e_ != hipSuccess) {                                                \
      vt_set_error("%s: %s", #expr, hipGetErrorString(e_));                \
      throw Fail{VT_ERR_HIP};                                              \
    }                                                                      \
  } while (0)

// the body of an extern "C" entry: a Fail becomes its code, any other exception "<name>: what()" + VT_ERR_ARG; the int64_t flavour
// (the *_bytes entries) answers -1 for both
template <class F>
auto guarded(const char* name, F&& body) -> decltype(body()) {
  const bool bytes = sizeof(decltype(body())) == sizeof(int64_t);
  try {
    return body();
  } catch (const Fail& f) {
    return bytes ? -1 : f.code;
  } catch (const std::exception& e) {
    vt_set_error("%s: %s", name, e.what());
    return bytes ? -1 : VT_ERR_ARG;
  }
}

int pad8(int c) { return (c + 7) / 8 * 8; }
size_t esize(int dt) { return dt == VT_F32 ? 4 : 2; }

// fp32 -> bf16, round to nearest even (what torch's .to(bfloat16) does)
uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0, peak = 0;
  void reset() { off = 0; }
  char* alloc(size_t n, bool dry) {
    off = (off + 255) & ~(size_t)255;
    char* p = base + off;        // dry: base = nullptr, pointers are never dereferenced
    off += n;
    if (off > peak) peak = off;
    if (!dry) M_CHECK(off <= cap, "vt_model: workspace too small (%zu of %zu bytes in one arena; ask vt_workspace_bytes)", off, cap);
    return p;
  }
};

struct Tens {                      // NDHWC activation
  char* p = nullptr;
  int B = 0, T = 0, H = 0, W = 0, ld = 0, dt = VT_BF16;
  size_t bytes() const { return (size_t)B * T * H * W * ld * esize(dt); }
};

struct Norm;
struct Act {                       // an activation, optionally with the LayerNorm(+SiLU) its consumer starts with
  Tens y, n;
  const Norm* norm = nullptr;
  bool silu = false;
  bool has_n() const { return norm != nullptr; }
  bool tup3 = false;               // answer of a ConvOpts::tup3_probe call: vt_time_upsample3 serves the descriptor
};
struct NormRef {
  const Norm* norm = nullptr;
  bool silu = false;
};

struct Param {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

struct Model;
struct Ctx {
  Model* m;
  hipStream_t stream;
  bool dry;
  Arena* cur;                      // arena the running stage allocates from
  Tens alloc(int B, int T, int H, int W, int ld, int dt, int c_real) {
    Tens t;
    t.B = B; t.T = T; t.H = H; t.W = W; t.ld = ld; t.dt = dt;
    t.p = cur->alloc(t.bytes(), dry);
    if (ld != c_real && !dry) M_HIP(hipMemsetAsync(t.p, 0, t.bytes(), stream));   // keep the pad lanes defined (they meet zero weights)
    return t;
  }
};

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// Chunk-to-chunk state of one module of a v1.1 tiled pass: the last frames of a causal convolution's input
// (CausalConv*.causal_cache, model_3dcausal_v1_1.py:155-178) or the frames a time resampler keeps (:286-300, 323-343).  The
// buffer is owned by the handle and rewritten in place; `offset` = the module's cache_offset of an overlapped decode.
struct CState {
  std::unique_ptr<DevBuf> buf;
  size_t cap = 0;
  int frames = 0;                  // frames held (0 = nothing cached yet)
  int offset = 0;
  size_t need = 0;                 // the most a dry walk asked of the buffer (sizes a session's state at vt_session_create)
};

struct Model {
  vt_model_config cfg;
  bool tiled = false;              // a chunk of a tiled pass is running: causal convolutions read / leave caches
  bool first_chunk = true;
  std::vector<CState*> states;     // every CState of both graphs (vt_reset_cache)
  std::vector<std::unique_ptr<DevBuf>> retired;   // outgrown cache buffers: work queued on them may still run; freed at reset / destroy
  // the cache buffer of `st` with room for `bytes` (grown by a synchronous hipMalloc the first time a chunk kind needs it)
  char* persistent(CState& st, size_t bytes, bool dry) {
    if (dry) {
      st.need = std::max(st.need, bytes);
      return nullptr;
    }
    if (st.cap < bytes) {
      auto b = std::make_unique<DevBuf>();
      if (hipMalloc(&b->p, bytes) != hipSuccess) {
        vt_set_error("vt_model: hipMalloc of a %zu-byte chunk cache failed", bytes);
        throw Fail{VT_ERR_HIP};
      }
      if (st.buf) retired.push_back(std::move(st.buf));
      st.buf = std::move(b);
      st.cap = bytes;
    }
    return (char*)st.buf->p;
  }
  int dt;                          // storage type of the activations (VT_BF16 | VT_F16 | VT_F32)
  bool x3 = false;                 // VT_BF16X3: fp32 storage, convolutions on split-bf16 weight planes (three bf16 MFMAs per product)
  bool v11() const { return cfg.version == 1; }
  bool noncausal() const { return cfg.version == 2; }          // Encoder3D / Decoder3D of model_3dnoncausal.py: centred temporal windows
  // time padding of a convolution with taps before the clip: zeros (v1.0) or the first frame repeated (v1.1, one pass)
  int tpad() const { return v11() ? VT_TPAD_REPLICATE : VT_TPAD_ZERO; }
  std::map<std::string, Param> params;
  std::map<std::string, std::unique_ptr<DevBuf>> packed;      // cache key -> the packed tensor on the device (owned)
  std::unique_ptr<DevBuf> reg_buf; // FSQ with projections: the projected latent and its codes (grown on first use, like the chunk caches)
  size_t reg_cap = 0;
  float* reg_scratch(size_t floats) {
    if (reg_cap < floats * 4) {
      auto b = std::make_unique<DevBuf>();
      if (hipMalloc(&b->p, floats * 4) != hipSuccess) {
        vt_set_error("vt_model: hipMalloc of the %zu-byte FSQ projection scratch failed", floats * 4);
        throw Fail{VT_ERR_HIP};
      }
      if (reg_buf) retired.push_back(std::move(reg_buf));
      reg_buf = std::move(b);
      reg_cap = floats * 4;
    }
    return (float*)reg_buf->p;
  }
  int fsq_ncb() const { return cfg.fsq_num_codebooks > 1 ? cfg.fsq_num_codebooks : 1; }
  int fsq_eff() const { return cfg.n_levels * fsq_ncb(); }                     // effective_codebook_dim
  bool fsq_proj() const { return cfg.regularizer == 1 && cfg.fsq_dim > 0 && cfg.fsq_dim != fsq_eff(); }
  bool prepare = false;            // vt_prepare: a dry walk of the graphs that packs and uploads every weight it meets
  Arena arena[2];
  std::vector<std::string> expected;        // state_dict keys the graph reads (filled by a dry run)

  const Param& param(const std::string& key) {
    auto it = params.find(key);
    M_CHECK(it != params.end(), "vt_model: weight '%s' was not loaded (vt_load_weight)", key.c_str());
    return it->second;
  }
  void* upload(const std::string& ckey, const void* host, size_t bytes) {
    auto b = std::make_unique<DevBuf>();
    M_HIP(hipMalloc(&b->p, bytes));
    M_HIP(hipMemcpy(b->p, host, bytes, hipMemcpyHostToDevice));
    void* p = b->p;
    packed[ckey] = std::move(b);
    return p;
  }
  // fp32 vector on the device as it is (biases, LayerNorm affines, mix factors)
  static std::string f32_ckey(const std::string& key) { return "f32:" + key; }
  const float* f32(const std::string& key, bool dry) { return f32(key, f32_ckey(key), dry); }
  const float* f32(const std::string& key, const std::string& ckey, bool dry) {
    if (dry && !prepare) {
      expected.push_back(key);
      return nullptr;
    }
    auto it = packed.find(ckey);
    if (it != packed.end()) return (const float*)it->second->p;
    const Param& p = param(key);
    return (const float*)upload(ckey, p.data.data(), p.data.size() * 4);
  }
  // convolution weight [Cout][Cin][k...] -> [Cout][taps * cin_p] in the arithmetic dtype (vidtok_amd/packing.py); `xf`
  // optionally rewrites the fp32 weight first (parity classes of the up-samplers: pre-summed taps)
  typedef std::vector<float> (*Xform)(const Param&, std::vector<int64_t>& shape, int a, int b);
  // `rows` = plain rows in the storage type even under VT_BF16X3 (the row operand of a GEMM against activations).  `ckey` names
  // the packed form in `packed` (w_ckey: a Site builds it once; vt_load_weight drops every "w:<key>:..." of the tensor it replaces)
  std::string w_ckey(const std::string& key, int cin_p, Xform xf, int xa, int xb, bool rows) const {
    return "w:" + key + ":" + std::to_string(cin_p) + ":" + std::to_string(dt) + (x3 && !rows ? "x3" : "") + ":" + std::to_string((xf ? 1 : 0) * 100 + xa * 10 + xb);
  }
  const void* conv_w(const std::string& key, const std::string& ckey, int cin_p, bool dry, Xform xf, int xa, int xb, bool rows) {
    if (dry && !prepare) {
      expected.push_back(key);
      return nullptr;
    }
    const bool split = x3 && !rows;
    auto it = packed.find(ckey);
    if (it != packed.end()) return it->second->p;
    const Param& p = param(key);
    std::vector<int64_t> shape = p.shape;
    std::vector<float> tmp;
    const float* src = p.data.data();
    if (xf) {
      tmp = xf(p, shape, xa, xb);
      src = tmp.data();
    }
    M_CHECK(shape.size() >= 3, "vt_model: '%s' is not a convolution weight", key.c_str());
    const int64_t cout = shape[0], cin = shape[1];
    int64_t taps = 1;
    for (size_t i = 2; i < shape.size(); ++i) taps *= shape[i];
    M_CHECK(cin <= cin_p, "vt_model: '%s' has %lld input channels, the activation stores %d", key.c_str(), (long long)cin, cin_p);
    std::vector<float> w((size_t)cout * taps * cin_p, 0.0f);
    for (int64_t o = 0; o < cout; ++o)
      for (int64_t c = 0; c < cin; ++c)
        for (int64_t t = 0; t < taps; ++t) w[((size_t)o * taps + t) * cin_p + c] = src[((size_t)o * cin + c) * taps + t];
    if (split) {
      // vidtok_amd/packing.py::pack_split3: per group of 16 k, [hi 16 x bf16 | lo 16 x bf16], hi = bf16(w), lo = bf16(w - hi);
      // rows zero-padded to whole 128-byte K steps (ldw = K rounded up to 32, in 4-byte units)
      const size_t K = (size_t)taps * cin_p, Kp = (K + 31) / 32 * 32;
      std::vector<uint16_t> pl((size_t)cout * Kp * 2, 0);
      for (int64_t o = 0; o < cout; ++o)
        for (size_t k = 0; k < K; ++k) {
          const float v = w[(size_t)o * K + k];
          const uint16_t hi = bf16_rne(v);
          uint32_t hb = (uint32_t)hi << 16;
          float hf;
          memcpy(&hf, &hb, 4);
          uint16_t* blk = &pl[((size_t)o * Kp + (k / 16) * 16) * 2];
          blk[k % 16] = hi;
          blk[16 + k % 16] = bf16_rne(v - hf);
        }
      return upload(ckey, pl.data(), pl.size() * 2);
    }
    if (dt == VT_F32) return upload(ckey, w.data(), w.size() * 4);
    std::vector<uint16_t> h(w.size());
    if (dt == VT_F16) {
      for (size_t i = 0; i < w.size(); ++i) {          // round to nearest even (the compiler's float -> _Float16 conversion)
        const _Float16 f = (_Float16)w[i];
        memcpy(&h[i], &f, 2);
      }
    } else {
      for (size_t i = 0; i < w.size(); ++i) h[i] = bf16_rne(w[i]);
    }
    return upload(ckey, h.data(), h.size() * 2);
  }
};

// ---- pre-summed taps of the up-samplers (vidtok_amd/packing.py) ------------------------------------------------------------
// time: [Co][Ci][3][kh][kw] -> [Co][Ci][2][kh][kw]; early: [W0 + W1, W2], else [W0, W1 + W2]
std::vector<float> xf_time_parity(const Param& p, std::vector<int64_t>& shape, int early, int) {
  const int64_t co = shape[0], ci = shape[1], hw = shape[3] * shape[4];
  std::vector<float> o((size_t)co * ci * 2 * hw);
  for (int64_t a = 0; a < co * ci; ++a)
    for (int64_t s = 0; s < hw; ++s) {
      const float w0 = p.data[(a * 3 + 0) * hw + s], w1 = p.data[(a * 3 + 1) * hw + s], w2 = p.data[(a * 3 + 2) * hw + s];
      o[(a * 2 + 0) * hw + s] = early ? w0 + w1 : w0;
      o[(a * 2 + 1) * hw + s] = early ? w2 : w1 + w2;
    }
  shape[2] = 2;
  return o;
}
// the three-product form of the causal time up-sampler (packing.py::time_upsample3_weights): part 2 = [W0, W2] (the k = 2 window of U),
// part 3 = W1 alone (V, a per-frame convolution); single taps, nothing summed.  (The part numbers continue xf_time_parity's 0 / 1:
// Model::w_ckey names a packed weight by the transform's arguments.)
std::vector<float> xf_time_up3(const Param& p, std::vector<int64_t>& shape, int part, int) {
  const int64_t co = shape[0], ci = shape[1], hw = shape[3] * shape[4];
  const int kt = part == 2 ? 2 : 1;
  std::vector<float> o((size_t)co * ci * kt * hw);
  for (int64_t a = 0; a < co * ci; ++a)
    for (int64_t s = 0; s < hw; ++s) {
      if (part == 2) {
        o[(a * 2 + 0) * hw + s] = p.data[(a * 3 + 0) * hw + s];
        o[(a * 2 + 1) * hw + s] = p.data[(a * 3 + 2) * hw + s];
      } else {
        o[a * hw + s] = p.data[(a * 3 + 1) * hw + s];
      }
    }
  shape[2] = kt;
  return o;
}
// space: [Co][Ci][3][3] -> [Co][Ci][2][2]; rows [W0, W1+W2] for py = 0, [W0+W1, W2] for py = 1, likewise columns
std::vector<float> xf_space_parity(const Param& p, std::vector<int64_t>& shape, int py, int px) {
  const int64_t n = shape[0] * shape[1];
  std::vector<float> o((size_t)n * 4);
  for (int64_t a = 0; a < n; ++a) {
    const float* w = &p.data[a * 9];
    float rows[2][3];
    for (int c = 0; c < 3; ++c) {
      rows[0][c] = py == 0 ? w[0 * 3 + c] : w[0 * 3 + c] + w[1 * 3 + c];
      rows[1][c] = py == 0 ? w[1 * 3 + c] + w[2 * 3 + c] : w[2 * 3 + c];
    }
    for (int r = 0; r < 2; ++r) {
      o[a * 4 + r * 2 + 0] = px == 0 ? rows[r][0] : rows[r][0] + rows[r][1];
      o[a * 4 + r * 2 + 1] = px == 0 ? rows[r][1] + rows[r][2] : rows[r][2];
    }
  }
  shape[2] = 2;
  shape[3] = 2;
  return o;
}

// ---- operators ---------------------------------------------------------------------------------------------------------
struct Geom {
  int kt = 1, kh = 1, kw = 1, st = 1, sh = 1, sw = 1, pt = 0, ph = 0, pw = 0, ph_hi = 0, pw_hi = 0;
  int pt_hi = 0;                   // zero frames after the clip (non-causal windows; the kernel reads 0 beyond the end)
  void out_dims(int Ti, int Hi, int Wi, int& To, int& Ho, int& Wo) const {
    To = (Ti + pt + pt_hi - kt) / st + 1;
    Ho = (Hi + ph + ph_hi - kh) / sh + 1;
    Wo = (Wi + pw + pw_hi - kw) / sw + 1;
  }
};
Geom causal3d(int kt, int kh, int kw, int st = 1, int sh = 1, int sw = 1) {
  Geom g;
  g.kt = kt; g.kh = kh; g.kw = kw; g.st = st; g.sh = sh; g.sw = sw;
  g.pt = (kt - 1) + (1 - st);
  const int hp = (kh - 1) + (1 - sh), wp = (kw - 1) + (1 - sw);
  g.ph = hp / 2; g.pw = wp / 2; g.ph_hi = hp - hp / 2; g.pw_hi = wp - wp / 2;
  return g;
}
// the same window centred in time (nn.Conv3d / Conv1d with padding k / 2 of the non-causal family): `before` frames in front,
// the rest of the k - 1 behind
Geom centred(Geom g, int before) {
  g.pt_hi = g.pt - before;
  g.pt = before;
  return g;
}

struct Norm {
  std::string key;                 // "...norm1": LayerNorm wrapper, parameters at key + ".norm.weight" / ".norm.bias"; GroupNorm: key + ".weight" / ".bias"
  float eps = 1e-6f;
  bool group = false;              // norm_type "groupnorm": torch.nn.GroupNorm(32, C, eps 1e-6) (model_3dcausal.py:30-32)
  int site = VT_GN_FRAME;          // GroupNorm only: the view the reference's call site normalises; -1 = single positions (the causal temporal blocks)
  std::string wkey() const { return key + (group ? ".weight" : ".norm.weight"); }
  std::string bkey() const { return key + (group ? ".bias" : ".norm.bias"); }
  // the norm of a plain tensor (LayerNorm: vt_layernorm_act; GroupNorm: vt_groupnorm_act over the site's domain, as
  // vidtok_amd/ops.py::groupnorm_act drives it)
  Tens of(Ctx& c, const Tens& t, bool silu, int c_real) const {
    Tens o = c.alloc(t.B, t.T, t.H, t.W, t.ld, c.m->dt, c_real);
    const float* g = c.m->f32(wkey(), c.dry);
    const float* b = c.m->f32(bkey(), c.dry);
    if (!group) {
      if (!c.dry)
        M_CALL(vt_layernorm_act(t.p, t.dt, t.ld, o.p, o.dt, o.ld, g, b, (int64_t)t.B * t.T * t.H * t.W, c_real, eps, silu ? 1 : 0, c.stream));
      return o;
    }
    // single positions ("(b t) c s" with s = 1, model_3dcausal.py:476-487) = the PIXEL domain of a one-frame view of all positions
    const int scope = site < 0 ? VT_GN_PIXEL : site;
    const int B = site < 0 ? 1 : t.B, T = site < 0 ? 1 : t.T;
    const int64_t HW = site < 0 ? (int64_t)t.B * t.T * t.H * t.W : (int64_t)t.H * t.W;
    const int64_t wb = std::max<int64_t>(vt_groupnorm_work_bytes(B, T, 32, scope), 8);
    void* work = c.cur->alloc((size_t)wb, c.dry);
    if (!c.dry) M_CALL(vt_groupnorm_act(t.p, t.dt, t.ld, o.p, o.dt, o.ld, g, b, B, T, HW, c_real, 32, scope, eps, silu ? 1 : 0, work, c.stream));
    return o;
  }
  // LayerNorm(+SiLU) of x, unless x already carries exactly that
  Tens apply(Ctx& c, const Act& x, bool silu, int c_real) const {
    if (x.has_n() && x.norm == this && x.silu == silu) return x.n;
    return of(c, x.y, silu, c_real);
  }
  // what a stage asks its producer to emit: nothing for GroupNorm (its statistics span more than a position: never fused)
  NormRef ref(bool silu) const { return group ? NormRef() : NormRef{this, silu}; }
};

struct ConvOpts {
  const Tens* res = nullptr;
  int res_mode = VT_RES_NONE;
  const float* mix = nullptr;
  NormRef ln;                      // emit this norm of the result
  bool keep_y = true;
  Tens* out = nullptr;             // preallocated interleaved output (parity classes)
  Tens* ln_out = nullptr;          // ... and its normalised twin (the emitted LayerNorm of an interleaved output)
  bool ln_optional = false;        // emit `ln` only if this launch's epilogue takes it (vt_conv_plan), else run without (ops.conv ln_optional)
  bool plan_only = false;          // with ln_optional: launch nothing, only answer (Act::has_n) whether the epilogue would take the LayerNorm
  bool tup3_probe = false;         // with plan_only: also answer (Act::tup3) whether vt_time_upsample3 serves this parity descriptor
  const Tens* tup3_v = nullptr;    // run as the paired launch vt_time_upsample3 with this V = W1 x (the descriptor was probed before)
  int yt_mul = 1, yt_off = 0, ys = 0, ys_oh = 0, ys_ow = 0;
  float* ncthw = nullptr;          // write fp32 NCTHW here instead
  int t_trim = 0;
  int tmode = VT_TPAD_ZERO;
  const void* cache = nullptr;     // tmode VT_TPAD_CACHE: [B][ncache][H][W][ld]
  int ncache = 0;
};

// mirror of vidtok_amd/ops.py::conv
Act conv(Ctx& c, const Tens& x, const void* w, int ldw, const float* bias, const Geom& g, int cout, const ConvOpts& o) {
  int To, Ho, Wo;
  g.out_dims(x.T, x.H, x.W, To, Ho, Wo);
  M_CHECK(To > 0 && Ho > 0 && Wo > 0, "vt_model: convolution output is empty (%d x %d x %d)", To, Ho, Wo);
  Act r;
  vt_conv_desc d;
  memset(&d, 0, sizeof(d));
  int ldy;
  if (o.out) {
    r.y = *o.out;
    ldy = o.out->ld;
  } else if (o.ncthw) {
    ldy = cout;
  } else {
    ldy = pad8(cout);
    r.y = c.alloc(x.B, To, Ho, Wo, ldy, c.m->dt, cout);
  }
  d.x = x.p; d.w = w; d.bias = bias; d.y = o.ncthw ? (void*)o.ncthw : (void*)r.y.p;
  d.B = x.B; d.Ti = x.T; d.Hi = x.H; d.Wi = x.W; d.Cin = x.ld;
  d.To = To; d.Ho = Ho; d.Wo = Wo; d.Cout = cout;
  d.ldw = c.m->x3 ? (ldw + 31) / 32 * 32 : ldw; d.ldy = ldy;
  d.KT = g.kt; d.KH = g.kh; d.KW = g.kw; d.st = g.st; d.sh = g.sh; d.sw = g.sw; d.pt = g.pt; d.ph = g.ph; d.pw = g.pw;
  d.tmode = g.pt > 0 ? o.tmode : VT_TPAD_ZERO;
  if (d.tmode == VT_TPAD_CACHE) { d.cache = o.cache; d.ncache = o.ncache; }
  d.res_mode = o.res_mode;
  if (o.res_mode != VT_RES_NONE) {
    d.res = o.res->p; d.res_tshift = 0; d.Tr = o.res->T; d.ldr = o.res->ld;
    d.mix_factor = o.mix;
  }
  d.out_layout = o.ncthw ? VT_NCTHW : VT_NDHWC;
  d.t_trim = o.t_trim;
  d.dtype = c.m->x3 ? VT_BF16X3 : x.dt; d.out_dtype = o.ncthw ? VT_F32 : c.m->dt;
  d.nbatch = 1;
  d.yt_mul = o.yt_mul; d.yt_off = o.yt_off;
  if (o.ys) { d.ys_mul = 2; d.ys_oh = o.ys_oh; d.ys_ow = o.ys_ow; }
  const bool ln_after = o.ln.norm && o.ln.norm->group;      // GroupNorm of the result: its own pass behind the convolution (GroupNorm32.after)
  if (o.ln.norm && !ln_after) {
    r.n = o.ln_out ? *o.ln_out : c.alloc(x.B, To, Ho, Wo, ldy, c.m->dt, cout);
    d.ln_gamma = c.m->f32(o.ln.norm->wkey(), c.dry);
    d.ln_beta = c.m->f32(o.ln.norm->bkey(), c.dry);
    d.ln_out = r.n.p;
    d.ln_mode = o.ln.silu ? 2 : 1; d.ln_keep_y = o.keep_y ? 1 : 0; d.ldn = ldy; d.ln_eps = o.ln.norm->eps;
    r.norm = o.ln.norm; r.silu = o.ln.silu;
  }
  // (a dry run has no pointers to validate: the library is asked with stand-ins, its decisions depend on the geometry only)
  auto standins = [&](vt_conv_desc& q) {
    if (!c.dry) return;
    q.x = q.w = q.y = (void*)16;
    if (q.res_mode != VT_RES_NONE) q.res = (void*)16;
    if (q.res_mode == VT_RES_MIX) q.mix_factor = (const float*)16;
    if (q.tmode == VT_TPAD_CACHE) q.cache = (void*)16;
    if (q.ln_mode != 0) { q.ln_gamma = q.ln_beta = (const float*)16; q.ln_out = (void*)16; }
  };
  // the LayerNorm of an interleaved output exists only inside an epilogue: where this launch's does not take it, run without and let
  // the consumer normalise y itself (vidtok_amd/ops.py::conv ln_optional; option conv_tup_ln)
  if (o.ln_optional && d.ln_mode != 0) {
    vt_conv_desc q = d;
    standins(q);
    int32_t plan[8];
    if (q.ln_out == nullptr) q.ln_out = (void*)16;             // (plan_only: the twin tensor is not allocated yet)
    if (!(vt_conv_plan(&q, plan) == VT_OK && plan[4] == 1)) {
      d.ln_gamma = d.ln_beta = nullptr; d.ln_out = nullptr; d.ln_mode = 0;
      r.n = Tens(); r.norm = nullptr;
    }
  }
  if (o.tup3_probe) {
    vt_conv_desc q = d;
    standins(q);
    if (q.ln_mode != 0 && q.ln_out == nullptr) q.ln_out = (void*)16;
    r.tup3 = vt_time_upsample3_supported(&q) == 1;
  }
  if (o.plan_only) return r;
  if (o.tup3_v) {
    if (!c.dry) M_CALL(vt_time_upsample3(&d, o.tup3_v->p, o.tup3_v->ld, c.stream));
    return r;
  }
  // split-K over the time taps (small-M launches): the library says how much scratch; it comes from the stage's arena.
  {
    vt_conv_desc q = d;
    standins(q);
    const int64_t wb = ((x.dt == VT_BF16 || x.dt == VT_F16) && (g.kt == 3 || g.kh == 3)) ? vt_conv_work_bytes(&q) : 0;
    if (wb > 0) {
      d.work = c.cur->alloc((size_t)wb, c.dry);
      d.work_bytes = wb;
    }
  }
  if (!c.dry) M_CALL(vt_conv(&d, c.stream));
  if (ln_after) {
    M_CHECK(!o.out && !o.ncthw, "vt_model: GroupNorm of an interleaved / NCTHW result");
    r.n = o.ln.norm->of(c, r.y, o.ln.silu, cout);
    r.norm = o.ln.norm; r.silu = o.ln.silu;
  }
  return r;
}

std::vector<int> range(int a, int b) {                 // a, a + 1, ..., b - 1
  std::vector<int> v;
  for (int t = a; t < b; ++t) v.push_back(t);
  return v;
}
Tens frames_at(const Tens& like, const void* p, int T) {          // T frames shaped like `like`'s at p
  Tens t = like;
  t.p = (char*)p;
  t.T = T;
  return t;
}

// frames idx[0..n) of src -> dst frames [t0, t0 + n) of [B][Td][frame] (vidtok_amd/ops.py::gather_frames)
void gather(Ctx& c, const Tens& src, char* dst, int Td, int t0, const std::vector<int>& idx) {
  const int64_t fr = (int64_t)src.H * src.W * src.ld;
  const int es = (int)esize(src.dt);
  for (size_t j0 = 0; j0 < idx.size(); j0 += 128) {
    int32_t part[128];
    const int n = (int)std::min<size_t>(128, idx.size() - j0);
    for (int j = 0; j < n; ++j) part[j] = idx[j0 + j];
    if (!c.dry) M_CALL(vt_gather_frames(src.p, dst + (size_t)(t0 + (int)j0) * fr * es, es, src.B, fr, (int64_t)src.T * fr, (int64_t)Td * fr, part, n, c.stream));
  }
}

// keep frames idx of src as st's chunk cache: frames [t0, t0 + n) of the `total` (default: n) the cache then holds
void keep_frames(Ctx& c, CState& st, const Tens& src, const std::vector<int>& idx, int t0 = 0, int total = 0) {
  if (total == 0) total = (int)idx.size();
  char* buf = c.m->persistent(st, frames_at(src, nullptr, total).bytes(), c.dry);
  gather(c, src, buf, total, t0, idx);
  if (!c.dry) st.frames = total;
}

// _CausalState._update_cache (vidtok_amd/modules.py; reference model_3dcausal_v1_1.py:172-176): keep the last P frames of
// padded[: len - offset], padded = [P pad frames (x[0] repeated on the first chunk | the previous cache), x]
void update_cache(Ctx& c, CState& st, const Tens& x, int P) {
  if (P == 0) return;
  const int T = x.T, off = st.offset;
  std::vector<int> sx, sc;                           // the frames taken from x, and in front of them those that stay from the old cache
  for (int j = 0; j < P; ++j) {
    const int q = T - off + j;                      // index into the padded sequence
    M_CHECK(q >= 0, "vt_model: chunk of %d frames is shorter than its cache offset %d", T, off);
    if (q >= P) sx.push_back(q - P);
    else if (c.m->first_chunk) sx.push_back(0);
    else sc.push_back(q);
  }
  // frames kept from the old cache move inside the buffer they are read from: through a temporary (stream order)
  if (!sc.empty()) {
    M_CHECK(c.dry || st.frames >= P, "vt_model: causal cache missing (the first chunk must come first)");
    const Tens kept = c.alloc(x.B, (int)sc.size(), x.H, x.W, x.ld, x.dt, x.ld);
    gather(c, frames_at(x, c.dry ? nullptr : st.buf->p, P), kept.p, kept.T, 0, sc);
    keep_frames(c, st, kept, range(0, kept.T), 0, P);
  }
  if (!sx.empty()) keep_frames(c, st, x, sx, (int)sc.size(), P);
}

typedef std::map<std::string, std::vector<int64_t>> Shapes;     // reference state_dict key -> parameter shape
struct Build {                     // what the graph builders pass around: the handle being built and its parameter list
  Model& m;
  Shapes& sh;
  const vt_model_config& cf() const { return m.cfg; }
  bool wrap() const { return !m.noncausal(); }                   // the causal families keep their 3-D / 1-D convolutions under a Causal* wrapper
  int gn_site() const { return wrap() ? VT_GN_FRAME : VT_GN_CLIP; }      // the view the 3-D sites hand to GroupNorm (vidtok_amd/modules.py SITE_*)
  // a norm of the graph under `key` over `ch` channels; `site` = the view its call site hands to GroupNorm
  void norm(Norm& n, const std::string& key, int ch, int site) {
    n.key = key;
    n.group = cf().norm_type == 1;
    n.site = site;
    sh[n.wkey()] = {ch};
    sh[n.bkey()] = {ch};
  }
};

// One convolution as the kernels see it (packing.ConvSite of the Python host): its parameters' state_dict key, its window, the
// transform that turns the stored weight into this launch's operand, and -- causal sites -- its chunk state.  Built once by the
// graph builders, which is also where its parameters enter the handle's list; several sites may read one key (the parity classes
// of the up-samplers, the U and V forms of the three-product time up-sampler).
struct Site {
  std::string wkey, bkey;          // "<key>.weight" / "<key>.bias"
  std::string wckey, bckey;        // their packed forms in Model::packed
  int cin = 0, cout = 0;
  Geom g;
  Model::Xform xf = nullptr;       // parity classes: pre-summed taps (xf_* above) with arguments xa, xb
  int xa = 0, xb = 0;
  bool rows = false;               // plain rows even under VT_BF16X3 (attention's W_v)
  bool causal = false;             // keeps `st` in a tiled pass (CausalConv3d.run / CausalConv1d.run of vidtok_amd/modules.py)
  CState st;
  // `k`: the kernel dims of the stored tensor.  THE key rule: a convolution with a time axis sits under a Causal* wrapper, which
  // adds a ".conv" level ("...conv1.conv.weight"), in the causal families; nn.Conv2d and the non-causal family's nn.Conv3d / Conv1d have none
  void init(Build& b, const std::string& key, int cout_, int cin_, std::vector<int64_t> k, const Geom& g_, bool causal_ = false,
            Model::Xform xf_ = nullptr, int xa_ = 0, int xb_ = 0, bool rows_ = false) {
    const std::string full = key + (b.wrap() && k.size() != 2 ? ".conv" : "");
    cin = cin_; cout = cout_; g = g_; causal = causal_; xf = xf_; xa = xa_; xb = xb_; rows = rows_;
    wkey = full + ".weight"; bkey = full + ".bias";
    wckey = b.m.w_ckey(wkey, pad8(cin), xf, xa, xb, rows); bckey = Model::f32_ckey(bkey);
    std::vector<int64_t> w = {cout, cin};
    w.insert(w.end(), k.begin(), k.end());
    b.sh[wkey] = w;
    b.sh[bkey] = {cout};
  }
  const void* w(Ctx& c) const { return c.m->conv_w(wkey, wckey, pad8(cin), c.dry, xf, xa, xb, rows); }
  const float* bias(Ctx& c) const { return c.m->f32(bkey, bckey, c.dry); }
  int ldw(const Tens& x) const { return g.kt * g.kh * g.kw * x.ld; }
  Act run(Ctx& c, const Tens& x, ConvOpts o, bool with_bias = true) {
    const int P = g.pt;
    const bool cached = causal && c.m->tiled;
    if (cached && P > 0) {
      if (c.m->first_chunk) o.tmode = VT_TPAD_REPLICATE;
      else {
        M_CHECK(c.dry || st.frames >= P, "vt_model: causal cache missing (the first chunk must come first)");
        o.tmode = VT_TPAD_CACHE;
        o.cache = c.dry ? (const void*)16 : st.buf->p;
        o.ncache = c.dry ? P : st.frames;
      }
    }
    const Act r = conv(c, x, w(c), ldw(x), with_bias ? bias(c) : nullptr, g, cout, o);
    if (cached) update_cache(c, st, x, P);
    return r;
  }
  // launch nothing; answer whether the epilogue would take o.ln (Act::has_n; o.ln_optional) and, `tup3` (asked before any weight is
  // packed: stand-in operands), whether vt_time_upsample3 serves the descriptor (Act::tup3)
  Act probe(Ctx& c, const Tens& x, ConvOpts o, bool tup3 = false) {
    o.plan_only = true;
    o.tup3_probe = tup3;
    return conv(c, x, tup3 ? (const void*)16 : w(c), ldw(x), tup3 ? nullptr : bias(c), g, cout, o);
  }
};

// batched C[z] = A[z] B[z]^T on the convolution kernel (vidtok_amd/ops.py::gemm_nt)
char* gemm_nt(Ctx& c, const void* a, bool a_batched, const void* b, int Z, int M, int N, int K, int in_dt, int out_dt, int ldo, const float* bias) {
  const size_t bytes = (size_t)Z * M * ldo * esize(out_dt);
  char* y = c.cur->alloc(bytes, c.dry);
  if (ldo != N && !c.dry) M_HIP(hipMemsetAsync(y, 0, bytes, c.stream));
  vt_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.x = a; d.w = b; d.y = y; d.bias = bias;
  d.B = 1; d.Ti = 1; d.Hi = 1; d.Wi = M; d.Cin = K;
  d.To = 1; d.Ho = 1; d.Wo = M; d.Cout = N;
  d.ldw = K; d.ldy = ldo;
  d.KT = d.KH = d.KW = 1; d.st = d.sh = d.sw = 1;
  d.dtype = in_dt; d.out_dtype = out_dt;
  d.nbatch = Z;
  d.xs_z = a_batched ? (int64_t)M * K : 0; d.ws_z = (int64_t)N * K; d.ys_z = (int64_t)M * ldo;
  if (!c.dry) M_CALL(vt_conv(&d, c.stream));
  return y;
}

// ---- stages ------------------------------------------------------------------------------------------------------------
struct Stage {
  virtual ~Stage() {}
  virtual NormRef first_norm(Ctx&) const { return NormRef(); }      // the norm this stage wants from its producer
  virtual Act run(Ctx& c, const Act& x, NormRef next) = 0;
  virtual void states(std::vector<CState*>&) {}                     // the chunk state this stage keeps in a tiled pass
  virtual bool time_up() const { return false; }                    // a temporal up-sampler: cache offsets double from here on
};

ConvOpts emit(NormRef next, int tmode = VT_TPAD_ZERO) {
  ConvOpts o;
  o.ln = next;                     // keep_y = true
  o.tmode = tmode;
  return o;
}

// the body of every residual block (residual_block of the Python host): norm1 + SiLU -> conv1, seen only through norm2 + SiLU ->
// [1x1 shortcut of x] -> conv2 + residual, emitting the consumer's norm
Act residual_block(Ctx& c, const Norm& n1, const Norm& n2, Site& c1, Site& c2, Site* shortcut, const Act& x, NormRef next) {
  const Tens h = n1.apply(c, x, true, c1.cin);
  ConvOpts o1;
  o1.ln = NormRef{&n2, true};
  o1.keep_y = false;
  o1.tmode = c.m->tpad();
  const Act h2 = c1.run(c, h, o1);
  const Tens xs = shortcut ? shortcut->run(c, x.y, ConvOpts()).y : x.y;
  ConvOpts o2 = emit(next, c.m->tpad());
  o2.res = &xs;
  o2.res_mode = VT_RES_ADD;
  return c2.run(c, h2.n, o2);
}

struct ResBlock : Stage {          // ResnetBlock (2-D per frame) or ResnetCausalBlock (3-D causal), model_3dcausal.py:276-424
  Norm n1, n2;
  Site c1, c2, sc;                 // the 3-D causal block's convolutions keep two frames each in a tiled pass; sc: nin_shortcut, where cin != cout
  ResBlock(Build& b, const std::string& key, int cin, int cout, bool causal, int site = VT_GN_FRAME) {
    Geom g3 = causal ? causal3d(3, 3, 3) : causal3d(1, 3, 3);
    if (causal && b.m.noncausal()) g3 = centred(g3, 1);             // ResnetNoncausalBlock: Conv3d padding 1
    const std::vector<int64_t> k3 = causal ? std::vector<int64_t>{3, 3, 3} : std::vector<int64_t>{3, 3};
    b.norm(n1, key + ".norm1", cin, site);
    b.norm(n2, key + ".norm2", cout, site);
    c1.init(b, key + ".conv1", cout, cin, k3, g3, causal);
    c2.init(b, key + ".conv2", cout, cout, k3, g3, causal);
    if (cin != cout) sc.init(b, key + ".nin_shortcut", cout, cin, std::vector<int64_t>(k3.size(), 1), Geom());
  }
  void states(std::vector<CState*>& v) override {
    if (c1.causal) { v.push_back(&c1.st); v.push_back(&c2.st); }
  }
  NormRef first_norm(Ctx&) const override { return n1.ref(true); }
  Act run(Ctx& c, const Act& x, NormRef next) override { return residual_block(c, n1, n2, c1, c2, c1.cin != c1.cout ? &sc : nullptr, x, next); }
};

struct TBlock : Stage {            // ResnetCausalBlock1D, model_3dcausal.py:427-499
  int ch;
  Norm n1, n2;
  Site c1, c2;                     // CausalConv1d; chunk state of the two convolutions: [B][2][H][W][C] each
  TBlock(Build& b, const std::string& key, int ch_) : ch(ch_) {
    Geom g;
    g.kt = 3; g.pt = 2;
    if (b.m.noncausal()) g = centred(g, 1);            // ResnetBlock1D: Conv1d padding 1
    // causal temporal blocks normalise single positions (model_3dcausal.py:476-487), the non-causal ones pixels over time (model_3dnoncausal.py:228-236)
    b.norm(n1, key + ".norm1", ch, b.wrap() ? -1 : VT_GN_PIXEL);
    b.norm(n2, key + ".norm2", ch, b.wrap() ? -1 : VT_GN_PIXEL);
    c1.init(b, key + ".conv1", ch, ch, {3}, g, true);
    c2.init(b, key + ".conv2", ch, ch, {3}, g, true);
  }
  void states(std::vector<CState*>& v) override { v.push_back(&c1.st); v.push_back(&c2.st); }
  // ResnetCausalBlock1D._fusable (vidtok_amd/modules.py): one launch for bf16, C = 128; in a tiled pass both convolutions must
  // stand at the same point of the chunk schedule and, past the first chunk, both caches must be there
  bool fusable(const Ctx& c) const {
    if (c.m->noncausal()) return false;                // the fused launch is the causal block
    if (!((c.m->dt == VT_BF16 || c.m->dt == VT_F16) && ch == 128 && n1.eps == n2.eps) || n1.group) return false;
    if (!c.m->tiled) return true;
    if (c1.st.offset != c2.st.offset) return false;
    return c.m->first_chunk || c.dry || (c1.st.frames >= 2 && c2.st.frames >= 2);
  }
  NormRef first_norm(Ctx& c) const override { return fusable(c) ? NormRef() : n1.ref(true); }
  Act run(Ctx& c, const Act& x, NormRef next) override {
    Model* m = c.m;
    const Tens& xp = x.y;
    vt_tblock_desc d;
    memset(&d, 0, sizeof(d));
    d.dtype = xp.dt; d.C = ch; d.ld = xp.ld; d.B = xp.B; d.T = xp.T; d.HW = (int64_t)xp.H * xp.W; d.tmode = m->tpad();
    const bool fus = fusable(c);
    if (fus && m->tiled) {           // the launch keeps the chunk state itself: both caches rewritten in place
      const size_t cb = (size_t)xp.B * 2 * xp.H * xp.W * xp.ld * esize(xp.dt);
      d.tmode = m->first_chunk ? VT_TPAD_REPLICATE : VT_TPAD_CACHE;
      d.cache1 = m->persistent(c1.st, cb, c.dry);
      d.cache2 = m->persistent(c2.st, cb, c.dry);
      if (c.dry) d.cache1 = d.cache2 = (void*)16;
      d.cache_offset = c1.st.offset;
    }
    if (fus && vt_temporal_block_supported(&d)) {
      if (m->tiled && !c.dry) c1.st.frames = c2.st.frames = 2;
      Act r;
      r.y = c.alloc(xp.B, xp.T, xp.H, xp.W, xp.ld, xp.dt, ch);
      const bool nx = next.norm != nullptr && next.norm->eps == n1.eps;
      if (nx) r.n = c.alloc(xp.B, xp.T, xp.H, xp.W, xp.ld, xp.dt, ch);
      d.x = xp.p; d.y = r.y.p; d.n_out = nx ? r.n.p : nullptr;
      d.w1 = c1.w(c); d.b1 = c1.bias(c);
      d.w2 = c2.w(c); d.b2 = c2.bias(c);
      d.norm1_gamma = m->f32(n1.wkey(), c.dry); d.norm1_beta = m->f32(n1.bkey(), c.dry);         // (LayerNorm: fusable() refuses GroupNorm)
      d.norm2_gamma = m->f32(n2.wkey(), c.dry); d.norm2_beta = m->f32(n2.bkey(), c.dry);
      if (nx) {
        d.next_gamma = m->f32(next.norm->wkey(), c.dry); d.next_beta = m->f32(next.norm->bkey(), c.dry);
        d.ln_next_mode = next.silu ? 2 : 1;
        r.norm = next.norm; r.silu = next.silu;
      }
      d.keep_y = 1; d.eps = n1.eps;
      if (!c.dry) M_CALL(vt_temporal_block(&d, c.stream));
      return r;
    }
    return residual_block(c, n1, n2, c1, c2, nullptr, x, next);
  }
};

struct Attn : Stage {              // AttnBlockWrapper, model_3dcausal.py:83-141 ("heads" = frames)
  int ch;
  Norm n;
  Site q_, k_, v_, proj;           // CausalConv3d 1x1x1; W_v is the row operand of a GEMM: plain rows
  Attn(Build& b, const std::string& key, int ch_) : ch(ch_) {
    b.norm(n, key + ".norm", ch, b.gn_site());
    q_.init(b, key + ".q", ch, ch, {1, 1, 1}, Geom());
    k_.init(b, key + ".k", ch, ch, {1, 1, 1}, Geom());
    v_.init(b, key + ".v", ch, ch, {1, 1, 1}, Geom(), false, nullptr, 0, 0, true);
    proj.init(b, key + ".proj_out", ch, ch, {1, 1, 1}, Geom());
  }
  NormRef first_norm(Ctx&) const override { return n.ref(false); }
  Act run(Ctx& c, const Act& x, NormRef next) override {
    Model* m = c.m;
    const Tens hn = n.apply(c, x, false, ch);
    const Tens& xp = x.y;
    const int S = xp.H * xp.W, Z = xp.B * xp.T, Cc = xp.ld, Sp = pad8(S), dt = m->dt;
    M_CHECK(Cc == ch, "vt_model: attention over %d channels stored as %d (channel counts must be multiples of 8)", ch, Cc);
    const Tens q = q_.run(c, hn, ConvOpts()).y;
    const Tens k = k_.run(c, hn, ConvOpts()).y;
    const void* wv = v_.w(c);
    const float* bv = v_.bias(c);
    // V^T directly: the weight is the row operand; v's bias is added after P V (rows of P sum to 1)
    char* vT = gemm_nt(c, wv, false, hn.p, Z, Cc, S, Cc, dt, dt, Sp, nullptr);                // [Z][C][Sp]
    // scale = C^-0.5 as the Python host passes it: computed in double, rounded once to float
    const float scale = (float)std::pow((double)Cc, -0.5);
    Tens o = xp;
    if (vt_flash_attention_supported(dt, S, Cc, Sp)) {
      // one launch with the online softmax: no [Z][S][S] scores in memory (vidtok_amd/modules.py takes the same decision)
      o.p = c.cur->alloc((size_t)Z * S * Cc * esize(dt), c.dry);
      if (!c.dry) M_CALL(vt_flash_attention(q.p, k.p, vT, bv, o.p, dt, Z, S, Cc, Sp, scale, c.stream));
    } else {
      char* s = gemm_nt(c, q.p, true, k.p, Z, S, S, Cc, dt, VT_F32, S, nullptr);               // [Z][S][S] fp32
      const size_t pbytes = (size_t)Z * S * Sp * esize(dt);
      char* p = c.cur->alloc(pbytes, c.dry);
      if (!c.dry) {
        if (Sp != S) M_HIP(hipMemsetAsync(p, 0, pbytes, c.stream));
        M_CALL(vt_softmax_rows((const float*)s, p, dt, (int64_t)Z * S, S, Sp, scale, c.stream));
      }
      o.p = gemm_nt(c, p, true, vT, Z, S, Cc, Sp, dt, dt, Cc, bv);                             // [Z][S][C] = [B][T][H][W][C]
    }
    ConvOpts op = emit(next);
    op.res = &xp;
    op.res_mode = VT_RES_ADD;
    return proj.run(c, o, op);
  }
};

struct Down : Stage {              // Downsample: F.pad(0,1,0,1) + conv3x3 stride 2, model_3dcausal.py:215-230
  Site cv;                         // nn.Conv2d at key + ".conv"
  Down(Build& b, const std::string& key, int ch) {
    Geom g;
    g.kh = 3; g.kw = 3; g.sh = 2; g.sw = 2; g.ph_hi = 1; g.pw_hi = 1;
    cv.init(b, key + ".conv", ch, ch, {3, 3}, g);
  }
  Act run(Ctx& c, const Act& x, NormRef next) override { return cv.run(c, x.y, emit(next)); }
};

struct TimeDown : Stage {          // TimeDownsampleResCausal2x, model_3dcausal.py:233-252
  std::string mix_key;             // key + ".mix_factor"
  Site cv;                         // CausalConv3d at key + ".conv"; its cache holds one frame
  CState sp;                       // the pooling branch's cache (the chunk's last frame)
  TimeDown(Build& b, const std::string& key, int ch) : mix_key(key + ".mix_factor") {
    Geom g = causal3d(3, 3, 3, 2, 1, 1);
    if (b.m.noncausal()) g = centred(g, 0);                           // stride-2 Conv3d with padding (0,1,1) over [x, 0]
    cv.init(b, key + ".conv", ch, ch, {3, 3, 3}, g, true);
    b.sh[mix_key] = {1};
  }
  void states(std::vector<CState*>& v) override { v.push_back(&cv.st); v.push_back(&sp); }
  Act run(Ctx& c, const Act& x, NormRef next) override {
    Model* m = c.m;
    const Tens& xp = x.y;
    Tens x1 = c.alloc(xp.B, xp.T / 2, xp.H, xp.W, xp.ld, xp.dt, xp.ld);
    int tm = m->noncausal() ? VT_TPAD_ZERO_BACK : m->tpad();        // non-causal: both branches see [x, 0] (model_3dnoncausal.py:86-89)
    const void* pc = nullptr;
    if (m->tiled) {                // TimeDownsampleResCausal2x.run of the Python host (model_3dcausal_v1_1.py:286-300)
      tm = m->first_chunk ? VT_TPAD_REPLICATE : VT_TPAD_CACHE;
      if (!m->first_chunk) {
        M_CHECK(c.dry || sp.frames >= 1, "vt_model: time down-sampler cache missing (the first chunk must come first)");
        pc = c.dry ? nullptr : sp.buf->p;
      }
    }
    if (!c.dry) M_CALL(vt_time_avgpool3s2(xp.p, pc, x1.p, xp.dt, xp.B, xp.T, (int64_t)xp.H * xp.W, xp.ld, tm, c.stream));
    if (m->tiled) keep_frames(c, sp, xp, {xp.T - 1});
    ConvOpts o = emit(next, m->tpad());
    o.res = &x1;
    o.res_mode = VT_RES_MIX;
    o.mix = m->f32(mix_key, c.dry);
    return cv.run(c, xp, o);
  }
};

struct Up : Stage {                // Upsample: nearest x2 + conv3x3 as four parity classes, model_3dcausal.py:200-212
  int ch;
  Site par[2][2];                  // nn.Conv2d at key + ".conv", the 2x2 window of output rows / columns of parity py / px
  Up(Build& b, const std::string& key, int ch_) : ch(ch_) {
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        Geom g;
        g.kh = 2; g.kw = 2; g.ph = 1 - py; g.pw = 1 - px; g.ph_hi = py; g.pw_hi = px;
        par[py][px].init(b, key + ".conv", ch, ch, {3, 3}, g, false, xf_space_parity, py, px);
      }
  }
  Act run(Ctx& c, const Act& x, NormRef) override {
    const Tens& xp = x.y;
    Act r;
    r.y = c.alloc(xp.B, xp.T, 2 * xp.H, 2 * xp.W, pad8(ch), c.m->dt, ch);
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        ConvOpts o;
        o.out = &r.y; o.ys = 1; o.ys_oh = py; o.ys_ow = px;
        par[py][px].run(c, xp, o);
      }
    return r;
  }
};

struct TimeUp : Stage {            // TimeUpsampleResCausal2x: v1.0 nearest as two parity classes (model_3dcausal.py:255-273);
  int ch;                          // v1.1 nearest / trilinear up-sampling, then the 27-tap convolution (model_3dcausal_v1_1.py:305-343)
  int n_up = 1;                    // num_temp_upsample: 1, 2, 4 ... along the decoder (how many frames the trilinear head covers)
  std::string mix_key;             // key + ".mix_factor"
  // the sites of the one Conv3d at key + ".conv".  v1.1: the 27-tap convolution itself, whose cache holds two frames.  v1.0 and
  // non-causal: the parity classes par[0 / 1] of the even / odd output frames over pre-summed taps; v1.0 also the three-product form,
  // U = [W0, W2] over a frame pair and V = W1 per frame (no bias: U's launch adds it)
  Site full, par[2], u3, v3;
  CState su;                       // the trilinear interpolation's cache (num_temp_upsample frames)
  TimeUp(Build& b, const std::string& key, int ch_, int n_up_) : ch(ch_), n_up(n_up_), mix_key(key + ".mix_factor") {
    const std::vector<int64_t> k = {3, 3, 3};
    b.sh[mix_key] = {1};
    if (b.m.v11()) {
      full.init(b, key + ".conv", ch, ch, k, causal3d(3, 3, 3), true);
      return;
    }
    const bool nc = b.m.noncausal();
    Geom g, gv;
    g.kt = 2; g.kh = 3; g.kw = 3; g.pt = 1; g.ph = 1; g.pw = 1; g.ph_hi = 1; g.pw_hi = 1;
    gv.kh = 3; gv.kw = 3; gv.ph = 1; gv.pw = 1; gv.ph_hi = 1; gv.pw_hi = 1;
    // causal (window ends at the output frame):  o[2j] = (W0+W1) x[j-1] + W2 x[j],  o[2j+1] = W0 x[j-1] + (W1+W2) x[j]
    // centred (TimeUpsampleRes2x, model_3dnoncausal.py:93-115):  o[2j] = W0 x[j-1] + (W1+W2) x[j],  o[2j+1] = (W0+W1) x[j] + W2 x[j+1]
    for (int p = 0; p < 2; ++p) par[p].init(b, key + ".conv", ch, ch, k, nc ? centred(g, 1 - p) : g, false, xf_time_parity, nc ? p : 1 - p, 0);
    if (nc) return;
    u3.init(b, key + ".conv", ch, ch, k, g, false, xf_time_up3, 2, 0);
    v3.init(b, key + ".conv", ch, ch, k, gv, false, xf_time_up3, 3, 0);
  }
  void states(std::vector<CState*>& v) override { v.push_back(&full.st); v.push_back(&su); }
  bool time_up() const override { return true; }
  // later chunks of a tiled pass with trilinear up-sampling: [cache | x] interpolated, the frames the previous chunk already
  // delivered left out (TimeUpsampleResCausal2x._interp_v11 of the Python host; model_3dcausal_v1_1.py:325-343)
  Tens interp_cached(Ctx& c, const Tens& xp) {
    const int n = n_up, T = xp.T;
    const int64_t fr = (int64_t)xp.H * xp.W * xp.ld;
    const int nc = c.dry ? n : su.frames;
    M_CHECK(nc >= 1, "vt_model: time up-sampler cache missing (the first chunk must come first)");
    const int Tc = nc + T;
    const Tens head = frames_at(xp, c.dry ? nullptr : su.buf->p, nc);
    if (Tc - 2 * n >= nc) {
      Tens up = c.alloc(xp.B, 2 * Tc - 2 * n, xp.H, xp.W, xp.ld, xp.dt, xp.ld);
      if (!c.dry) M_CALL(vt_time_lerp2x_cat(head.p, nc, xp.p, up.p, xp.dt, xp.B, T, 2 * n, fr, c.stream));
      keep_frames(c, su, xp, range(Tc - 2 * n - nc, Tc - n - nc));
      return up;
    }
    Tens xc = c.alloc(xp.B, Tc, xp.H, xp.W, xp.ld, xp.dt, xp.ld);     // [cache | x]
    gather(c, head, xc.p, Tc, 0, range(0, nc));
    gather(c, xp, xc.p, Tc, nc, range(0, T));
    keep_frames(c, su, xc, range(std::max(0, Tc - 2 * n), Tc - n));    // (xc is a copy: the cache buffer is free to be rewritten)
    Tens all = c.alloc(xp.B, 2 * Tc, xp.H, xp.W, xp.ld, xp.dt, xp.ld);
    if (!c.dry) M_CALL(vt_time_lerp2x(xc.p, all.p, xp.dt, xp.B, Tc, fr, c.stream));
    Tens up = c.alloc(xp.B, 2 * Tc - 2 * n, xp.H, xp.W, xp.ld, xp.dt, xp.ld);
    gather(c, all, up.p, up.T, 0, range(2 * n, 2 * Tc));
    return up;
  }
  Act conv_of(Ctx& c, const Tens& up, NormRef next) {
    ConvOpts o = emit(next, VT_TPAD_REPLICATE);
    o.res = &up;
    o.res_mode = VT_RES_MIX;
    o.mix = c.m->f32(mix_key, c.dry);
    return full.run(c, up, o);
  }
  Act run_v11(Ctx& c, const Act& x, NormRef next) {
    const Tens& xp = x.y;
    const int T = xp.T;
    const int64_t fr = (int64_t)xp.H * xp.W * xp.ld;
    if (c.m->tiled && !c.m->first_chunk && c.m->cfg.interpolation_mode == 1) return conv_of(c, interp_cached(c, xp), next);
    Tens up = c.alloc(xp.B, 2 * T, xp.H, xp.W, xp.ld, xp.dt, xp.ld);
    if (c.m->cfg.interpolation_mode == 0) {                            // nearest: up[t] = x[t / 2]
      std::vector<int> half = range(0, 2 * T);
      for (int& t : half) t /= 2;
      gather(c, xp, up.p, 2 * T, 0, half);
    } else {
      // trilinear, first chunk (the only one here): the first n_up frames are interpolated on their own, the rest likewise
      // (F.interpolate on x[:, :n] and x[:, n:] separately, model_3dcausal_v1_1.py:327-341); one launch per clip and part
      const int hn = std::min(n_up, T);
      auto lerp_part = [&](int t0, int n, int out_t0) {
        Tens part = c.alloc(xp.B, n, xp.H, xp.W, xp.ld, xp.dt, xp.ld);
        gather(c, xp, part.p, n, 0, range(t0, t0 + n));
        for (int b = 0; b < xp.B; ++b)
          if (!c.dry)
            M_CALL(vt_time_lerp2x(part.p + (size_t)b * n * fr * esize(xp.dt), up.p + ((size_t)b * 2 * T + out_t0) * fr * esize(xp.dt), xp.dt, 1, n, fr, c.stream));
      };
      // first chunk of a tiled pass: keep the last n_up frames for the next chunk's interpolation
      if (c.m->tiled) keep_frames(c, su, xp, range(std::max(0, T - n_up), T));
      lerp_part(0, hn, 0);
      if (T > n_up) lerp_part(n_up, T - n_up, 2 * hn);
    }
    return conv_of(c, up, next);
  }
  Act run(Ctx& c, const Act& x, NormRef next) override {
    if (c.m->v11()) return run_v11(c, x, next);
    const Tens& xp = x.y;
    Act r;
    r.y = c.alloc(xp.B, 2 * xp.T, xp.H, xp.W, pad8(ch), c.m->dt, ch);
    // the consumer's LayerNorm from the two launches' epilogues where they can take it (TimeUpsampleResCausal2x.run of the Python host)
    bool emit_ln = next.norm != nullptr;
    Tens nbuf;
    const float* mf = c.m->f32(mix_key, c.dry);
    if (!c.m->noncausal()) {
      // three frame products instead of four (vt_time_upsample3; time_parity_upsample of the Python host): U[j] = W0 x[j-1] + W2 x[j] is
      // shared by the two frames of a pair, V[j] = W1 x[j] by neighbouring pairs -- o[2j] = U[j] + V[j-1], o[2j+1] = U[j] + V[j].
      // Asked with the LayerNorm the launch would really carry, before anything is allocated or packed.
      ConvOpts o;
      Tens probe = r.y;
      probe.p = nullptr;
      o.out = &r.y; o.yt_mul = 2; o.yt_off = 0;
      if (emit_ln) { o.ln = next; o.ln_out = &probe; o.ln_optional = true; }
      o.res = &xp; o.res_mode = VT_RES_MIX; o.mix = mf;
      const Act q = u3.probe(c, xp, o, true);
      if (q.tup3) {
        const Act v = v3.run(c, xp, ConvOpts(), false);
        ConvOpts u;
        u.out = &r.y; u.yt_mul = 2; u.yt_off = 0; u.tup3_v = &v.y;
        u.res = &xp; u.res_mode = VT_RES_MIX; u.mix = mf;
        if (q.has_n()) {
          nbuf = c.alloc(xp.B, 2 * xp.T, xp.H, xp.W, pad8(ch), c.m->dt, ch);
          u.ln = next; u.ln_out = &nbuf;
        }
        u3.run(c, xp, u);
        if (q.has_n()) { r.n = nbuf; r.norm = next.norm; r.silu = next.silu; }
        return r;
      }
    }
    if (emit_ln) {
      // ask before allocating the twin (a launch that refuses -- the 512-channel up-sampler always does -- left a full-size
      // buffer in the arena's peak): the decision depends on the geometry only, the same for both parity launches
      ConvOpts o;
      Tens probe = r.y;
      probe.p = nullptr;
      o.out = &r.y; o.yt_mul = 2; o.yt_off = 0; o.ln = next; o.ln_out = &probe; o.ln_optional = true;
      o.res = &xp; o.res_mode = VT_RES_MIX; o.mix = mf;
      emit_ln = par[0].probe(c, xp, o).has_n();
      if (emit_ln) nbuf = c.alloc(xp.B, 2 * xp.T, xp.H, xp.W, pad8(ch), c.m->dt, ch);
    }
    for (int p = 0; p < 2; ++p) {
      ConvOpts o;
      o.out = &r.y; o.yt_mul = 2; o.yt_off = p;
      if (emit_ln) { o.ln = next; o.ln_out = &nbuf; o.ln_optional = true; }
      o.res = &xp; o.res_mode = VT_RES_MIX; o.mix = mf;
      if (!par[p].run(c, xp, o).has_n()) emit_ln = false;
    }
    if (emit_ln) { r.n = nbuf; r.norm = next.norm; r.silu = next.silu; }
    return r;
  }
};

bool in_list(const int32_t* v, int n, int x) {
  for (int i = 0; i < n; ++i)
    if (v[i] == x) return true;
  return false;
}

struct Graph {
  std::vector<std::unique_ptr<Stage>> stages;
  Site conv_in, conv_out;          // causal, or Conv3d padding 1; two frames of chunk state each
  Norm norm_out;
  // the order sessions index their state by (vt_session::st) and set_offsets walks
  void states(std::vector<CState*>& v) {
    v.push_back(&conv_in.st);
    for (auto& st : stages) st->states(v);
    v.push_back(&conv_out.st);
  }
  // cache offsets of an overlapped decode (AutoencodingEngineV11._overlap_offsets, autoencoder_v1_1.py:307-320): 1 at latent
  // rate, doubling at each temporal up-sampler (the up-sampler itself already works at the doubled rate); 0 = no look-ahead
  void set_offsets(bool overlap) {
    int off = overlap ? 1 : 0;
    conv_in.st.offset = off;
    for (auto& st : stages) {
      if (st->time_up()) off *= 2;
      std::vector<CState*> v;
      st->states(v);
      for (CState* s : v) s->offset = off;
    }
    conv_out.st.offset = off;
  }
};

void build_encoder(Build& b, Graph& g) {
  const vt_model_config& cf = b.cf();
  const int L = cf.num_resolutions;
  const Geom g333 = b.wrap() ? causal3d(3, 3, 3) : centred(causal3d(3, 3, 3), 1);
  int block_in = cf.ch;
  for (int i = 0; i < L; ++i) {
    block_in = cf.ch * (i == 0 ? 1 : cf.ch_mult[i - 1]);
    const int block_out = cf.ch * cf.ch_mult[i];
    const std::string d = "encoder.down." + std::to_string(i), dt = "encoder.down_temporal." + std::to_string(i);
    for (int j = 0; j < cf.num_res_blocks; ++j) {
      g.stages.emplace_back(new ResBlock(b, d + ".block." + std::to_string(j), block_in, block_out, false));
      g.stages.emplace_back(new TBlock(b, dt + ".block." + std::to_string(j), block_out));
      block_in = block_out;
    }
    if (in_list(cf.spatial_ds, cf.n_spatial_ds, i)) {
      g.stages.emplace_back(new Down(b, d + ".downsample", block_in));
      if (in_list(cf.tempo_ds, cf.n_tempo_ds, i)) g.stages.emplace_back(new TimeDown(b, dt + ".downsample", block_in));
    }
  }
  g.stages.emplace_back(new ResBlock(b, "encoder.mid.block_1", block_in, block_in, true, b.gn_site()));
  g.stages.emplace_back(new Attn(b, "encoder.mid.attn_1", block_in));
  g.stages.emplace_back(new ResBlock(b, "encoder.mid.block_2", block_in, block_in, true, b.gn_site()));
  g.conv_in.init(b, "encoder.conv_in", cf.ch, cf.in_channels, {3, 3, 3}, g333, true);
  g.conv_out.init(b, "encoder.conv_out", cf.double_z ? 2 * cf.z_channels : cf.z_channels, block_in, {3, 3, 3}, g333, true);
  b.norm(g.norm_out, "encoder.norm_out", block_in, b.gn_site());
}

void build_decoder(Build& b, Graph& g) {
  const vt_model_config& cf = b.cf();
  const int L = cf.num_resolutions;
  const Geom g333 = b.wrap() ? causal3d(3, 3, 3) : centred(causal3d(3, 3, 3), 1);
  int block_in = cf.ch * cf.ch_mult[L - 1];
  int n_up = 1;
  g.conv_in.init(b, "decoder.conv_in", block_in, cf.z_channels, {3, 3, 3}, g333, true);
  g.stages.emplace_back(new ResBlock(b, "decoder.mid.block_1", block_in, block_in, true, b.gn_site()));
  g.stages.emplace_back(new Attn(b, "decoder.mid.attn_1", block_in));
  g.stages.emplace_back(new ResBlock(b, "decoder.mid.block_2", block_in, block_in, true, b.gn_site()));
  for (int i = L - 1; i >= 0; --i) {
    const int block_out = cf.ch * cf.ch_mult[i];
    const std::string u = "decoder.up." + std::to_string(i), ut = "decoder.up_temporal." + std::to_string(i);
    for (int j = 0; j < cf.num_res_blocks + 1; ++j) {
      g.stages.emplace_back(new ResBlock(b, u + ".block." + std::to_string(j), block_in, block_out, false));
      g.stages.emplace_back(new TBlock(b, ut + ".block." + std::to_string(j), block_out));
      block_in = block_out;
    }
    if (in_list(cf.spatial_us, cf.n_spatial_us, i)) {
      g.stages.emplace_back(new Up(b, u + ".upsample", block_in));
      if (in_list(cf.tempo_us, cf.n_tempo_us, i)) {
        g.stages.emplace_back(new TimeUp(b, ut + ".upsample", block_in, n_up));
        n_up *= 2;
      }
    }
  }
  g.conv_out.init(b, "decoder.conv_out", cf.out_ch, block_in, {3, 3, 3}, g333, true);
  b.norm(g.norm_out, "decoder.norm_out", block_in, b.gn_site());
}

// conv_in -> stages -> norm_out + SiLU -> conv_out (fp32 NCTHW); each stage is told which norm its consumer starts with
void run_graph(Ctx& c, Graph& g, const Tens& x_in, float* out_ncthw, int t_trim) {
  Model* m = c.m;
  int which = 1;                   // x_in lives in arena 0
  c.cur = &m->arena[which];
  c.cur->reset();
  const NormRef first = g.stages[0]->first_norm(c);
  Act h = g.conv_in.run(c, x_in, emit(first, m->tpad()));
  for (size_t i = 0; i < g.stages.size(); ++i) {
    which ^= 1;
    c.cur = &m->arena[which];
    c.cur->reset();                // holds the input of the previous stage: no longer needed
    const NormRef next = i + 1 < g.stages.size() ? g.stages[i + 1]->first_norm(c) : g.norm_out.ref(true);
    h = g.stages[i]->run(c, h, next);
  }
  which ^= 1;
  c.cur = &m->arena[which];
  c.cur->reset();
  const Tens hn = g.norm_out.apply(c, h, true, g.conv_out.cin);
  ConvOpts o;
  o.ncthw = out_ncthw ? out_ncthw : (float*)16;      // dry runs pass no buffer
  o.t_trim = t_trim;
  o.tmode = m->tpad();
  g.conv_out.run(c, hn, o);
}

int front_pad(const vt_model_config& cf, int T) {      // EncoderCausal3DPadding.forward: v1.0 pads f - 1 frames, v1.1 up to a multiple of f
  const int f = cf.time_downsample_factor;
  if (T % f == 0 || cf.version == 2) return 0;         // Encoder3D pads nothing (T must be a multiple of f: vt_encode checks)
  return cf.version == 1 ? f - T % f : f - 1;
}

void encode_impl(Model* m, Graph& g, const float* x, int B, int T, int H, int W, float* h_out, hipStream_t stream, bool dry) {
  Ctx c{m, stream, dry, &m->arena[0]};
  m->arena[0].reset();
  const int npad = front_pad(m->cfg, T);
  Tens xin = c.alloc(B, T + npad, H, W, pad8(m->cfg.in_channels), m->dt, pad8(m->cfg.in_channels));   // the kernel zero-fills the pad channels itself
  if (!dry) M_CALL(vt_ncthw_to_ndhwc(x, xin.p, m->dt, B, m->cfg.in_channels, T, H, W, xin.ld, npad, stream));
  run_graph(c, g, xin, h_out, 0);
}

void decode_impl(Model* m, Graph& g, const float* z, int B, int T, int H, int W, float* x_out, hipStream_t stream, bool dry) {
  Ctx c{m, stream, dry, &m->arena[0]};
  m->arena[0].reset();
  Tens zin = c.alloc(B, T, H, W, pad8(m->cfg.z_channels), m->dt, pad8(m->cfg.z_channels));
  if (!dry) M_CALL(vt_ncthw_to_ndhwc(z, zin.p, m->dt, B, m->cfg.z_channels, T, H, W, zin.ld, 0, stream));
  run_graph(c, g, zin, x_out, m->cfg.version != 0 ? 0 : m->cfg.time_downsample_factor - 1);   // v1.1 keeps every frame (the caller drops the padding's), the non-causal decoder drops nothing
}

// ---- temporal tiling of the v1.1 tokenizers (AutoencodingEngineV11.tile_encode / tile_decode, autoencoder_v1_1.py:218-331) -----------
// [[0, 1], [1, 1 + c], [1 + c, 1 + 2 c], ...]: the first chunk is the single leading frame (build_chunk_start_end, :218-228)
std::vector<std::pair<int, int>> chunk_list(int t, int step) {
  std::vector<std::pair<int, int>> v{{0, 1}};
  for (int start = 1; start < t;) {
    const int end = std::min(t, start + step);
    v.emplace_back(start, end);
    start = end;
  }
  return v;
}
int ceil_div(int a, int b) { return (a + b - 1) / b; }

struct ChunkBufs {                 // staging of one chunk in front of the arenas: its input frames and its result, contiguous NCTHW
  float* in = nullptr;
  float* out = nullptr;
  size_t bytes = 0;
};
ChunkBufs chunk_bufs(void* ws, size_t in_elems, size_t out_elems) {
  ChunkBufs b;
  const size_t ib = (in_elems * 4 + 255) & ~(size_t)255, ob = (out_elems * 4 + 255) & ~(size_t)255;
  b.in = (float*)ws;
  b.out = (float*)((char*)ws + ib);
  b.bytes = ib + ob;
  return b;
}
void reset_states(Model& m) {
  for (CState* st : m.states) st->frames = 0;
}

// The handle's tiled-pass state (tiled / first_chunk flags, the decoder's doubling cache offsets), restored on EVERY exit path of a
// tiled walk -- a walk that throws half way (an M_CHECK in Attn, update_cache, interp_cached, a workspace that is too small) must
// not leave a handle on which the next plain vt_encode / vt_decode runs as "a chunk" (extra allocations, cache reads, "causal cache
// missing")
struct TileScope {
  Model* m;
  Graph* g;
  TileScope(Model* m_, Graph& g_, bool overlap) : m(m_), g(&g_) {
    g->set_offsets(overlap);
    m->tiled = true;
  }
  ~TileScope() {
    m->tiled = false;
    m->first_chunk = true;
    g->set_offsets(false);
  }
  TileScope(const TileScope&) = delete;
  TileScope& operator=(const TileScope&) = delete;
};

// dry walks (workspace sizing, vt_prepare) run on empty arenas: the caller's arenas come back on every exit path
struct ArenaScope {
  Model* m;
  Arena save[2];
  explicit ArenaScope(Model* m_) : m(m_), save{m_->arena[0], m_->arena[1]} {
    m->arena[0] = Arena();
    m->arena[1] = Arena();
  }
  ~ArenaScope() {
    m->arena[0] = save[0];
    m->arena[1] = save[1];
  }
  ArenaScope(const ArenaScope&) = delete;
  ArenaScope& operator=(const ArenaScope&) = delete;
};

// every chunk through the encoder in order (the module caches carry the causal state); a chunk of n frames is front-padded
// to a multiple of f by the encoder and yields ceil(n / f) latent frames, written to h_out at their place
void tile_encode_impl(Model* m, Graph& g, const float* x, int B, int T, int H, int W, int t_chunk, float* h_out, char* ws, hipStream_t stream, bool dry) {
  const vt_model_config& cf = m->cfg;
  const int f = cf.time_downsample_factor, cin = cf.in_channels, cz = cf.double_z ? 2 * cf.z_channels : cf.z_channels;
  const int Hz = H >> cf.n_spatial_ds, Wz = W >> cf.n_spatial_ds;
  const auto chunks = chunk_list(T, t_chunk);
  int tz = 0, nmax = 1;
  for (auto& ch : chunks) {
    tz += ceil_div(ch.second - ch.first, f);
    nmax = std::max(nmax, ch.second - ch.first);
  }
  const ChunkBufs cb = chunk_bufs(ws, (size_t)B * cin * nmax * H * W, (size_t)B * cz * ceil_div(nmax, f) * Hz * Wz);
  TileScope scope(m, g, false);
  if (!dry) reset_states(*m);
  int done = 0;
  std::set<int> sized;                                     // sizing: the first chunk and one chunk of every other length (a short trailing
  for (size_t i = 0; i < chunks.size(); ++i) {             // chunk takes branches the largest one never sees)
    const int n = chunks[i].second - chunks[i].first, nz = ceil_div(n, f);
    if (dry && i != 0 && !sized.insert(n).second) continue;
    m->first_chunk = i == 0;
    if (!dry) M_CALL(vt_ncthw_copy_frames(x, cb.in, B * cin, T, n, chunks[i].first, 0, n, (int64_t)H * W, 0, stream));
    encode_impl(m, g, cb.in, B, n, H, W, cb.out, stream, dry);
    if (!dry) M_CALL(vt_ncthw_copy_frames(cb.out, h_out, B * cz, nz, tz, 0, done, nz, (int64_t)Hz * Wz, 0, stream));
    done += nz;
  }
}

// chunks of t_chunk_dec latent frames decoded in order, each with one look-ahead latent frame when `overlap` (its f trailing
// output frames are dropped, the module caches stop `cache_offset` frames early); f * Tz output frames in all
void tile_decode_impl(Model* m, Graph& g, const float* z, int B, int Tz, int Hz, int Wz, int t_chunk_dec, bool overlap, float* x_out, char* ws, hipStream_t stream, bool dry) {
  const vt_model_config& cf = m->cfg;
  const int f = cf.time_downsample_factor, zc = cf.z_channels, oc = cf.out_ch;
  const int H = Hz << cf.n_spatial_us, W = Wz << cf.n_spatial_us;
  const auto chunks = chunk_list(Tz, t_chunk_dec);
  int nmax = 1;
  for (auto& ch : chunks) nmax = std::max(nmax, ch.second - ch.first + ((overlap && ch.second + 1 <= Tz) ? 1 : 0));
  const ChunkBufs cb = chunk_bufs(ws, (size_t)B * zc * nmax * Hz * Wz, (size_t)B * oc * nmax * f * H * W);
  TileScope scope(m, g, overlap);
  if (!dry) reset_states(*m);
  int done = 0;
  std::set<int> sized;                                     // as in tile_encode_impl: every distinct chunk length is walked once
  for (size_t i = 0; i < chunks.size(); ++i) {
    const bool look = overlap && chunks[i].second + 1 <= Tz;
    const int nl = chunks[i].second - chunks[i].first + (look ? 1 : 0), n = nl * f - (look ? f : 0);
    if (dry && i != 0 && !sized.insert(nl).second) continue;
    m->first_chunk = i == 0;
    if (!dry) M_CALL(vt_ncthw_copy_frames(z, cb.in, B * zc, Tz, nl, chunks[i].first, 0, nl, (int64_t)Hz * Wz, 0, stream));
    decode_impl(m, g, cb.in, B, nl, Hz, Wz, cb.out, stream, dry);
    if (!dry) M_CALL(vt_ncthw_copy_frames(cb.out, x_out, B * oc, nl * f, Tz * f, 0, done, n, (int64_t)H * W, 0, stream));
    done += n;
  }
}

}  // namespace

struct vt_model {
  Model m;
  Graph enc, dec;
  Shapes shapes;                  // every parameter of the graph: the keys vt_weight_name lists, with their shapes
  std::vector<std::string> names;
};

extern "C" int vt_create(const vt_model_config* cfg, int32_t compute_dtype, vt_model** out) {
  return guarded("vt_create", [&]() -> int {
    M_CHECK(cfg != nullptr && out != nullptr, "vt_create: null argument");
    M_CHECK(compute_dtype == VT_BF16 || compute_dtype == VT_F16 || compute_dtype == VT_F32 || compute_dtype == VT_BF16X3,
            "vt_create: compute dtype must be VT_BF16, VT_F16, VT_F32 or VT_BF16X3");
    M_CHECK(cfg->version >= 0 && cfg->version <= 2, "vt_create: version 0 (v1.0 causal), 1 (v1.1 causal) or 2 (non-causal Encoder3D / Decoder3D)");
    M_CHECK(cfg->interpolation_mode == 0 || (cfg->interpolation_mode == 1 && cfg->version == 1), "vt_create: interpolation_mode 0 (nearest) or, for v1.1, 1 (trilinear)");
    M_CHECK(cfg->num_resolutions >= 1 && cfg->num_resolutions <= 8 && cfg->num_res_blocks >= 1 && cfg->ch > 0, "vt_create: bad level / block counts");
    M_CHECK(cfg->n_spatial_ds <= 8 && cfg->n_tempo_ds <= 8 && cfg->n_spatial_us <= 8 && cfg->n_tempo_us <= 8 && cfg->n_levels <= 8, "vt_create: list too long");
    M_CHECK(cfg->time_downsample_factor == 2 || cfg->time_downsample_factor == 4 || cfg->time_downsample_factor == 8, "vt_create: time_downsample_factor must be 2, 4 or 8");
    M_CHECK(cfg->norm_type == 0 || cfg->norm_type == 1, "vt_create: norm_type 0 (layernorm) or 1 (groupnorm)");
    M_CHECK(cfg->regularizer == 0 || cfg->regularizer == 1, "vt_create: regularizer 0 (KL) or 1 (FSQ)");
    if (cfg->regularizer == 1) {
      const int ncb = cfg->fsq_num_codebooks > 1 ? cfg->fsq_num_codebooks : 1, eff = cfg->n_levels * ncb;
      const int dim = cfg->fsq_dim > 0 ? cfg->fsq_dim : eff;
      M_CHECK(cfg->n_levels >= 1 && !cfg->double_z && cfg->z_channels == dim && cfg->fsq_num_codebooks >= 0 && cfg->fsq_dim >= 0 && eff <= 1024 && dim <= 1024,
              "vt_create: FSQ needs double_z = 0 and z_channels = dim (%d; len(levels) * num_codebooks = %d unless fsq_dim says otherwise)", dim, eff);
    }
    for (int i = 0; i < cfg->n_tempo_ds; ++i) M_CHECK(in_list(cfg->spatial_ds, cfg->n_spatial_ds, cfg->tempo_ds[i]), "vt_create: a temporal down-sampler sits behind a spatial one (tempo_ds must be a subset of spatial_ds)");
    for (int i = 0; i < cfg->n_tempo_us; ++i) M_CHECK(in_list(cfg->spatial_us, cfg->n_spatial_us, cfg->tempo_us[i]), "vt_create: tempo_us must be a subset of spatial_us");
    auto* h = new vt_model();
    h->m.cfg = *cfg;
    h->m.x3 = compute_dtype == VT_BF16X3;              // fp32 storage, split-bf16 convolutions (set_compute_dtype("bf16x3") of the Python host)
    h->m.dt = h->m.x3 ? VT_F32 : compute_dtype;
    Build b{h->m, h->shapes};
    build_encoder(b, h->enc);
    build_decoder(b, h->dec);
    h->enc.states(h->m.states);
    h->dec.states(h->m.states);
    if (h->m.fsq_proj()) {         // nn.Linear(dim, effective_codebook_dim) / back (regularizers.py:137-139)
      const int64_t eff = h->m.fsq_eff(), dim = cfg->fsq_dim;
      h->shapes["regularization.project_in.weight"] = {eff, dim};
      h->shapes["regularization.project_in.bias"] = {eff};
      h->shapes["regularization.project_out.weight"] = {dim, eff};
      h->shapes["regularization.project_out.bias"] = {dim};
    }
    for (const auto& kv : h->shapes) h->names.push_back(kv.first);
    *out = h;
    return VT_OK;
  });
}

extern "C" int vt_model_config_size(void) { return (int)sizeof(vt_model_config); }

extern "C" int vt_destroy(vt_model* h) {
  delete h;
  return VT_OK;
}

extern "C" int vt_load_weight(vt_model* h, const char* ref_key, const float* data_host, const int64_t* shape, int32_t ndim) {
  return guarded("vt_load_weight", [&]() -> int {
    M_CHECK(h && ref_key && data_host && shape && ndim >= 1 && ndim <= 5, "vt_load_weight: bad argument");
    const auto want = h->shapes.find(ref_key);
    M_CHECK(want != h->shapes.end(), "vt_load_weight: '%s' is not a parameter of this model (vt_weight_name lists them)", ref_key);
    bool same = (int)want->second.size() == ndim;
    for (int i = 0; same && i < ndim; ++i) same = want->second[(size_t)i] == shape[i];
    M_CHECK(same, "vt_load_weight: '%s' has the wrong shape (%d dims, first %lld; expected %zu dims, first %lld)", ref_key, ndim,
            (long long)shape[0], want->second.size(), (long long)want->second[0]);
    Param p;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
      M_CHECK(shape[i] > 0, "vt_load_weight: '%s' has an empty dimension", ref_key);
      p.shape.push_back(shape[i]);
      n *= shape[i];
    }
    p.data.assign(data_host, data_host + n);
    h->m.params[ref_key] = std::move(p);
    // packed copies of an earlier version of THIS tensor are stale ("f32:<key>", "w:<key>:..."): freed here, after the
    // device has finished whatever was queued on them
    const std::string fk = "f32:" + std::string(ref_key), wk = "w:" + std::string(ref_key) + ":";
    bool synced = false;
    for (auto it = h->m.packed.begin(); it != h->m.packed.end();) {
      if (it->first == fk || it->first.compare(0, wk.size(), wk) == 0) {
        if (!synced) {
          M_HIP(hipDeviceSynchronize());
          synced = true;
        }
        it = h->m.packed.erase(it);
      } else {
        ++it;
      }
    }
    return VT_OK;
  });
}

namespace {
void check_loaded_all(vt_model* h) {
  for (const std::string& k : h->names) (void)h->m.param(k);
}
}  // namespace

extern "C" int vt_latent_dims(const vt_model* h, int32_t T, int32_t H, int32_t W, int32_t* out4) {
  if (!h || !out4) {
    vt_set_error("vt_latent_dims: null argument");
    return VT_ERR_ARG;
  }
  const vt_model_config& cf = h->m.cfg;
  const int Tp = T + front_pad(cf, T);
  out4[0] = cf.double_z ? 2 * cf.z_channels : cf.z_channels;
  out4[1] = Tp >> cf.n_tempo_ds;
  out4[2] = H >> cf.n_spatial_ds;
  out4[3] = W >> cf.n_spatial_ds;
  return VT_OK;
}

extern "C" int64_t vt_workspace_bytes(vt_model* h, int32_t B, int32_t T, int32_t H, int32_t W) {
  return guarded("vt_workspace_bytes", [&]() -> int64_t {
    M_CHECK(h && B > 0 && T > 0 && H > 0 && W > 0, "vt_workspace_bytes: bad argument");
    Model& m = h->m;
    ArenaScope arenas(&m);
    m.expected.clear();
    encode_impl(&m, h->enc, nullptr, B, T, H, W, nullptr, nullptr, true);
    int32_t ld[4];
    vt_latent_dims(h, T, H, W, ld);
    decode_impl(&m, h->dec, nullptr, B, ld[1], ld[2], ld[3], nullptr, nullptr, true);
    const size_t peak = std::max(m.arena[0].peak, m.arena[1].peak);
    return (int64_t)(2 * ((peak + 255) & ~(size_t)255) + 512);
  });
}

// Pack and upload every weight now (host-side repacking + blocking copies), so that the first vt_encode / vt_decode is as
// asynchronous as the later ones -- e.g. before capturing a stream.  Walks both graphs dry on a minimal clip.
extern "C" int vt_prepare(vt_model* h) {
  return guarded("vt_prepare", [&]() -> int {
    M_CHECK(h != nullptr, "vt_prepare: null handle");
    check_loaded_all(h);
    Model& m = h->m;
    const int s = 1 << m.cfg.n_spatial_ds, T = m.cfg.time_downsample_factor;
    int32_t ld[4];
    vt_latent_dims(h, T, 8 * s, 8 * s, ld);
    {
      struct PrepareScope {        // Model::prepare for the length of the walk, off again on every exit path
        Model& m;
        explicit PrepareScope(Model& m_) : m(m_) { m.prepare = true; }
        ~PrepareScope() { m.prepare = false; }
      } preparing(m);
      ArenaScope arenas(&m);
      encode_impl(&m, h->enc, nullptr, 1, T, 8 * s, 8 * s, nullptr, nullptr, true);
      decode_impl(&m, h->dec, nullptr, 1, ld[1], ld[2], ld[3], nullptr, nullptr, true);
    }
    if (m.fsq_proj())              // FSQ projections: uploaded with the rest
      for (const char* k : {"regularization.project_in.weight", "regularization.project_in.bias", "regularization.project_out.weight", "regularization.project_out.bias"})
        (void)m.f32(k, false);
    return VT_OK;
  });
}

// the reference state_dict keys of the model's parameters (sorted) with their shapes: a loader walks them
extern "C" int vt_weight_count(vt_model* h) { return h ? (int)h->names.size() : 0; }
extern "C" const char* vt_weight_name(vt_model* h, int32_t i) {
  if (!h || i < 0 || i >= (int)h->names.size()) return nullptr;
  return h->names[(size_t)i].c_str();
}
extern "C" int vt_weight_shape(vt_model* h, int32_t i, int64_t* shape5, int32_t* ndim) {
  if (!h || !shape5 || !ndim || i < 0 || i >= (int)h->names.size()) {
    vt_set_error("vt_weight_shape: bad argument");
    return VT_ERR_ARG;
  }
  const std::vector<int64_t>& sh = h->shapes[h->names[(size_t)i]];
  *ndim = (int32_t)sh.size();
  for (size_t k = 0; k < sh.size(); ++k) shape5[k] = sh[k];
  return VT_OK;
}

namespace {
// every tensor the graph reads is there before anything is launched (prefix: "encoder." / "decoder.")
void check_loaded(vt_model* h, const char* prefix) {
  for (const std::string& k : h->names)
    if (k.compare(0, strlen(prefix), prefix) == 0) (void)h->m.param(k);
}
void bind_workspace(Model& m, void* ws, int64_t bytes, size_t skip = 0) {
  M_CHECK(ws != nullptr && bytes >= 1024 && (reinterpret_cast<uintptr_t>(ws) & 255) == 0, "vt_model: workspace must be a 256-byte aligned device buffer");
  M_CHECK((size_t)bytes > skip + 1024, "vt_model: workspace too small (%lld bytes; ask vt_workspace_bytes / vt_tile_workspace_bytes)", (long long)bytes);
  const size_t half = (((size_t)bytes - skip) / 2) & ~(size_t)255;
  m.arena[0].base = (char*)ws + skip; m.arena[0].cap = half; m.arena[0].peak = 0;
  m.arena[1].base = (char*)ws + skip + half; m.arena[1].cap = half; m.arena[1].peak = 0;
}
// bytes the chunk staging buffers of a tiled pass take at the front of the workspace
// (sized for the largest chunk the schedule can hold, whatever the clip length: t_chunk_enc frames in, t_chunk_dec + 1 latent frames)
size_t tile_staging_bytes(const vt_model_config& cf, int B, int H, int W, int t_chunk_enc) {
  const int f = cf.time_downsample_factor, cz = cf.double_z ? 2 * cf.z_channels : cf.z_channels;
  const int Hz = H >> cf.n_spatial_ds, Wz = W >> cf.n_spatial_ds;
  const int ne = std::max(1, t_chunk_enc);
  const size_t enc = chunk_bufs(nullptr, (size_t)B * cf.in_channels * ne * H * W, (size_t)B * cz * ceil_div(ne, f) * Hz * Wz).bytes;
  const int nd = std::max(1, t_chunk_enc / f) + 1;
  const size_t dec = chunk_bufs(nullptr, (size_t)B * cf.z_channels * nd * Hz * Wz, (size_t)B * cf.out_ch * nd * f * H * W).bytes;
  return std::max(enc, dec);
}
}  // namespace

extern "C" int vt_encode(vt_model* h, const float* x, int32_t B, int32_t T, int32_t H, int32_t W, float* h_out, void* workspace,
                         int64_t workspace_bytes, vt_stream stream) {
  return guarded("vt_encode", [&]() -> int {
    M_CHECK(h && x && h_out && B > 0 && T > 0 && H > 0 && W > 0, "vt_encode: bad argument");
    const int ds = 1 << h->m.cfg.n_spatial_ds;
    M_CHECK(H % ds == 0 && W % ds == 0, "vt_encode: H and W must be multiples of %d", ds);
    M_CHECK(!h->m.noncausal() || T % h->m.cfg.time_downsample_factor == 0, "vt_encode: the non-causal encoder takes clips whose length is a multiple of %d",
            h->m.cfg.time_downsample_factor);
    check_loaded(h, "encoder.");
    bind_workspace(h->m, workspace, workspace_bytes);
    encode_impl(&h->m, h->enc, x, B, T, H, W, h_out, reinterpret_cast<hipStream_t>(stream), false);
    return VT_OK;
  });
}

extern "C" int vt_decode(vt_model* h, const float* z, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz, float* x_out, void* workspace,
                         int64_t workspace_bytes, vt_stream stream) {
  return guarded("vt_decode", [&]() -> int {
    M_CHECK(h && z && x_out && B > 0 && Tz > 0 && Hz > 0 && Wz > 0, "vt_decode: bad argument");
    M_CHECK(h->m.cfg.version != 0 || (Tz << h->m.cfg.n_tempo_us) > h->m.cfg.time_downsample_factor - 1, "vt_decode: too few latent frames");
    check_loaded(h, "decoder.");
    bind_workspace(h->m, workspace, workspace_bytes);
    decode_impl(&h->m, h->dec, z, B, Tz, Hz, Wz, x_out, reinterpret_cast<hipStream_t>(stream), false);
    return VT_OK;
  });
}

extern "C" int vt_regularize_kl(vt_model* h, const float* moments, const float* noise, float* z, float* kl_out, int32_t B, int32_t Tz,
                                int32_t Hz, int32_t Wz, vt_stream stream) {
  if (!h || h->m.cfg.regularizer != 0) {
    vt_set_error("vt_regularize_kl: the handle's regularizer is not the diagonal Gaussian");
    return VT_ERR_ARG;
  }
  return vt_kl_sample(moments, noise, z, kl_out, B, h->m.cfg.z_channels, (int64_t)Tz * Hz * Wz, stream);
}

// FSQRegularizer.forward without the auxiliary loss (regularizers.py:206-230,247-268): [project_in ->] bound / round / pack per
// codebook [-> project_out]; indices [B][T'][H'][W'] (num_codebooks c > 1: [B][T'][H'][W'][c])
extern "C" int vt_regularize_fsq(vt_model* h, const float* pre, float* z, int32_t* indices, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz,
                                 vt_stream stream) {
  if (!h || h->m.cfg.regularizer != 1) {
    vt_set_error("vt_regularize_fsq: the handle's regularizer is not FSQ");
    return VT_ERR_ARG;
  }
  return guarded("vt_regularize_fsq", [&]() -> int {
    Model& m = h->m;
    const int64_t S = (int64_t)Tz * Hz * Wz;
    const int ncb = m.fsq_ncb();
    if (!m.fsq_proj()) return vt_fsq_quantize_cb(pre, z, indices, m.cfg.levels, m.cfg.n_levels, B, ncb, S, stream);
    const int eff = m.fsq_eff(), dim = m.cfg.fsq_dim;
    float* hp = m.reg_scratch((size_t)2 * B * eff * S);
    float* codes = hp + (size_t)B * eff * S;
    M_CALL(vt_channel_linear(pre, m.f32("regularization.project_in.weight", false), m.f32("regularization.project_in.bias", false), hp, B, dim, eff, S, stream));
    M_CALL(vt_fsq_quantize_cb(hp, codes, indices, m.cfg.levels, m.cfg.n_levels, B, ncb, S, stream));
    M_CALL(vt_channel_linear(codes, m.f32("regularization.project_out.weight", false), m.f32("regularization.project_out.bias", false), z, B, eff, dim, S, stream));
    return VT_OK;
  });
}

// FSQ: token indices -> latent codes (AutoencodingEngine.indices_to_latent / decode(..., decode_from_indices=True),
// reference autoencoder.py:205-229; FSQRegularizer.indices_to_codes with project_out, regularizers.py:180-198): z then goes to vt_decode
extern "C" int vt_indices_to_latent(vt_model* h, const int32_t* indices, float* z, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz, vt_stream stream) {
  if (!h || h->m.cfg.regularizer != 1) {
    vt_set_error("vt_indices_to_latent: the handle's regularizer is not FSQ");
    return VT_ERR_ARG;
  }
  return guarded("vt_indices_to_latent", [&]() -> int {
    Model& m = h->m;
    const int64_t S = (int64_t)Tz * Hz * Wz;
    const int ncb = m.fsq_ncb();
    if (!m.fsq_proj()) return vt_fsq_indices_to_codes_cb(indices, z, m.cfg.levels, m.cfg.n_levels, B, ncb, S, stream);
    const int eff = m.fsq_eff(), dim = m.cfg.fsq_dim;
    float* codes = m.reg_scratch((size_t)2 * B * eff * S);
    M_CALL(vt_fsq_indices_to_codes_cb(indices, codes, m.cfg.levels, m.cfg.n_levels, B, ncb, S, stream));
    M_CALL(vt_channel_linear(codes, m.f32("regularization.project_out.weight", false), m.f32("regularization.project_out.bias", false), z, B, eff, dim, S, stream));
    return VT_OK;
  });
}

// forget the chunk state of a tiled pass (vt_tile_encode / vt_tile_decode do it themselves at the start of a clip) and give the
// cache buffers back: SYNCHRONISES the device first -- work queued on them may still be running
extern "C" int vt_reset_cache(vt_model* h) {
  if (!h) {
    vt_set_error("vt_reset_cache: null handle");
    return VT_ERR_ARG;
  }
  if (hipDeviceSynchronize() != hipSuccess) {
    vt_set_error("vt_reset_cache: hipDeviceSynchronize failed");
    return VT_ERR_HIP;
  }
  for (CState* st : h->m.states) {
    st->frames = 0;
    st->cap = 0;
    st->buf.reset();
  }
  h->m.retired.clear();
  return VT_OK;
}

extern "C" int32_t vt_tile_latent_frames(const vt_model* h, int32_t T, int32_t t_chunk_enc) {
  if (!h || T <= 0 || t_chunk_enc <= 0) return -1;
  int tz = 0;
  for (auto& ch : chunk_list(T, t_chunk_enc)) tz += ceil_div(ch.second - ch.first, h->m.cfg.time_downsample_factor);
  return tz;
}

extern "C" int64_t vt_tile_workspace_bytes(vt_model* h, int32_t B, int32_t T, int32_t H, int32_t W, int32_t t_chunk_enc, int32_t use_overlap) {
  return guarded("vt_tile_workspace_bytes", [&]() -> int64_t {
    M_CHECK(h && B > 0 && T > 0 && H > 0 && W > 0 && t_chunk_enc > 0, "vt_tile_workspace_bytes: bad argument");
    M_CHECK(h->m.v11(), "vt_tile_workspace_bytes: temporal tiling exists only in the v1.1 models (version 1)");
    Model& m = h->m;
    const int f = m.cfg.time_downsample_factor;
    M_CHECK(t_chunk_enc >= f, "vt_tile_workspace_bytes: t_chunk_enc must be at least the temporal factor %d", f);
    ArenaScope arenas(&m);
    const int Hz = H >> m.cfg.n_spatial_ds, Wz = W >> m.cfg.n_spatial_ds;
    const int tz = vt_tile_latent_frames(h, T, t_chunk_enc);
    tile_encode_impl(&m, h->enc, nullptr, B, T, H, W, t_chunk_enc, nullptr, nullptr, nullptr, true);
    tile_decode_impl(&m, h->dec, nullptr, B, tz, Hz, Wz, t_chunk_enc / f, use_overlap != 0, nullptr, nullptr, nullptr, true);
    const size_t peak = std::max(m.arena[0].peak, m.arena[1].peak);
    return (int64_t)(tile_staging_bytes(m.cfg, B, H, W, t_chunk_enc) + 2 * ((peak + 255) & ~(size_t)255) + 1024);
  });
}

extern "C" int vt_tile_encode(vt_model* h, const float* x, int32_t B, int32_t T, int32_t H, int32_t W, int32_t t_chunk_enc, float* h_out,
                              void* workspace, int64_t workspace_bytes, vt_stream stream) {
  return guarded("vt_tile_encode", [&]() -> int {
    M_CHECK(h && x && h_out && B > 0 && T > 0 && H > 0 && W > 0, "vt_tile_encode: bad argument");
    M_CHECK(h->m.v11(), "vt_tile_encode: temporal tiling exists only in the v1.1 models (version 1)");
    M_CHECK(t_chunk_enc >= h->m.cfg.time_downsample_factor, "vt_tile_encode: t_chunk_enc must be at least the temporal factor");
    const int ds = 1 << h->m.cfg.n_spatial_ds;
    M_CHECK(H % ds == 0 && W % ds == 0, "vt_tile_encode: H and W must be multiples of %d", ds);
    check_loaded(h, "encoder.");
    const size_t skip = tile_staging_bytes(h->m.cfg, B, H, W, t_chunk_enc);
    bind_workspace(h->m, workspace, workspace_bytes, skip);
    tile_encode_impl(&h->m, h->enc, x, B, T, H, W, t_chunk_enc, h_out, (char*)workspace, reinterpret_cast<hipStream_t>(stream), false);
    return VT_OK;
  });
}

extern "C" int vt_tile_decode(vt_model* h, const float* z, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz, int32_t t_chunk_dec, int32_t use_overlap,
                              float* x_out, void* workspace, int64_t workspace_bytes, vt_stream stream) {
  return guarded("vt_tile_decode", [&]() -> int {
    M_CHECK(h && z && x_out && B > 0 && Tz > 0 && Hz > 0 && Wz > 0 && t_chunk_dec > 0, "vt_tile_decode: bad argument");
    M_CHECK(h->m.v11(), "vt_tile_decode: temporal tiling exists only in the v1.1 models (version 1)");
    check_loaded(h, "decoder.");
    const vt_model_config& cf = h->m.cfg;
    const int f = cf.time_downsample_factor;
    const size_t skip = tile_staging_bytes(cf, B, Hz << cf.n_spatial_us, Wz << cf.n_spatial_us, t_chunk_dec * f);
    bind_workspace(h->m, workspace, workspace_bytes, skip);
    tile_decode_impl(&h->m, h->dec, z, B, Tz, Hz, Wz, t_chunk_dec, use_overlap != 0, x_out, (char*)workspace, reinterpret_cast<hipStream_t>(stream), false);
    return VT_OK;
  });
}

// FSQ: the three statistics of the auxiliary loss on the pre-quantisation latent (FSQRegularizer.forward, regularizers.py:229-262):
// out3 = {per-sample entropy, codebook entropy, commitment}; the caller forms (out3[0] - diversity_gamma * out3[1]) *
// entropy_loss_weight + out3[2] * commitment_loss_weight with its YAML's weights.  work: vt_fsq_aux_work_floats(levels, D, B, S) floats
extern "C" int vt_regularize_fsq_aux(vt_model* h, const float* pre, int32_t B, int32_t Tz, int32_t Hz, int32_t Wz, float inv_temperature,
                                     float* work, float* out3, vt_stream stream) {
  if (!h || h->m.cfg.regularizer != 1) {
    vt_set_error("vt_regularize_fsq_aux: the handle's regularizer is not FSQ");
    return VT_ERR_ARG;
  }
  return guarded("vt_regularize_fsq_aux", [&]() -> int {
    Model& m = h->m;
    const int64_t S = (int64_t)Tz * Hz * Wz;
    // with the codebook axis kept the reference's own forward raises (its implicit codebook is one-dimensional, regularizers.py:143-146,234)
    M_CHECK(m.fsq_ncb() == 1, "vt_regularize_fsq_aux: the reference cannot compute the FSQ auxiliary loss with num_codebooks > 1 either");
    const float* hq = pre;
    if (m.fsq_proj()) {            // the statistics are those of the PROJECTED latent (regularizers.py:225-246)
      const int eff = m.fsq_eff();
      float* hp = m.reg_scratch((size_t)2 * B * eff * S);
      M_CALL(vt_channel_linear(pre, m.f32("regularization.project_in.weight", false), m.f32("regularization.project_in.bias", false), hp, B, m.cfg.fsq_dim, eff, S, stream));
      hq = hp;
    }
    return vt_fsq_aux_stats_avg(hq, m.cfg.levels, m.cfg.n_levels, B, S, inv_temperature, work, out3, nullptr, stream);
  });
}

// ---- sessions: the v1.1 tiling fed as the frames arrive (include/vidtok_amd.h, "Sessions") ----------------------------------------
// A session is the loop of tile_encode_impl / tile_decode_impl turned inside out: the chunk schedule advances with every push, the
// frames of the incomplete chunk wait in a buffer of the session's own, and the per-module causal state lives in CStates owned by the
// session -- swapped into the graph for the length of a push (SessionSwap), so that any number of sessions, and the handle's own
// vt_tile_* / vt_encode calls, can take turns on one handle.  Swapping moves pointers, not bytes: the C host captures no graphs.
struct vt_session {
  vt_model* h = nullptr;
  int kind = VT_SESSION_ENCODE;
  int B = 0, H = 0, W = 0, c = 0;  // H, W: of the input (frames of an encode, latents of a decode); c: chunk length in input frames
  bool overlap = false;            // decode: one look-ahead latent frame per chunk
  int cin = 0, cout = 0, Ho = 0, Wo = 0, f = 1;
  std::vector<CState> st;          // the session's causal state, in the order of Graph::states
  DevBuf pend;                     // frames of the incomplete chunk, fp32 [B][cin][cap][H][W]
  int cap = 0, npend = 0;
  int chunks = 0;                  // chunks run so far
  bool finished = false, broken = false;
  size_t staging = 0;              // chunk staging at the front of the workspace
  int64_t ws_bytes = 0;
  Graph& graph() { return kind == VT_SESSION_ENCODE ? h->enc : h->dec; }
};

namespace {

struct SessionSwap {               // the session's causal state in the graph for the length of a push; the handle's own back on every exit
  vt_session* s;
  std::vector<CState*> g;
  explicit SessionSwap(vt_session* s_) : s(s_) {
    s->graph().states(g);
    swap();
  }
  ~SessionSwap() { swap(); }
  void swap() {
    for (size_t i = 0; i < g.size(); ++i) {
      std::swap(g[i]->buf, s->st[i].buf);
      std::swap(g[i]->cap, s->st[i].cap);
      std::swap(g[i]->frames, s->st[i].frames);
    }
  }
  SessionSwap(const SessionSwap&) = delete;
  SessionSwap& operator=(const SessionSwap&) = delete;
};

// one step of a push: copy `k` input frames from `in_t0` into the pending buffer, or run the pending frames [0, nl) as chunk `idx`
struct SessionOp {
  bool run;
  int in_t0, k;                    // copy
  int nl, idx, n_out;              // run: input frames, chunk index, output frames kept
  bool look;
};

int session_chunk_len(const vt_session* s, int idx) { return idx == 0 ? 1 : s->c; }

// the host side of a push / finish, before anything runs: which frames go where, which chunks complete, how many frames come out
std::vector<SessionOp> session_plan(const vt_session* s, int n, bool fin, int* npend_after, int* chunks_after, int* frames_out) {
  std::vector<SessionOp> ops;
  int np = s->npend, ch = s->chunks, t = 0, outf = 0;
  const bool dec = s->kind == VT_SESSION_DECODE;
  auto run = [&](int nl, bool look) {
    const int n_out = dec ? nl * s->f - (look ? s->f : 0) : ceil_div(nl, s->f);
    ops.push_back(SessionOp{true, 0, 0, nl, ch, n_out, look});
    outf += n_out;
    ++ch;
  };
  while (t < n) {
    const int len = session_chunk_len(s, ch), want = len + (dec && s->overlap ? 1 : 0);
    const int k = std::min(want - np, n - t);
    ops.push_back(SessionOp{false, t, k, 0, 0, 0, false});
    np += k;
    t += k;
    if (np == want) {
      run(want, dec && s->overlap);
      np = want - len;             // the look-ahead latent stays: it opens the next chunk
    }
  }
  if (fin && np > 0) {
    run(np, false);
    np = 0;
  }
  *npend_after = np;
  *chunks_after = ch;
  *frames_out = outf;
  return ops;
}

int session_step(vt_session* s, const float* in, int n, float* out, int out_cap, int* n_out, void* ws, int64_t ws_bytes, hipStream_t stream, bool fin,
                 const char* what) {
  M_CHECK(s != nullptr && s->h != nullptr && n_out != nullptr, "%s: null argument", what);
  M_CHECK(!s->broken, "%s: an earlier call on this session failed half way; its state is undefined (destroy it)", what);
  M_CHECK(!s->finished, "%s: the session is finished (vt_session_finish ran): it takes no more frames", what);
  int np, ch, outf;
  const std::vector<SessionOp> plan = session_plan(s, n, fin, &np, &ch, &outf);
  M_CHECK(outf == 0 || out != nullptr, "%s: null output", what);
  M_CHECK(outf <= out_cap, "%s: %d output frames do not fit into out_cap_frames = %d", what, outf, out_cap);
  M_CHECK(ws_bytes >= s->ws_bytes, "%s: workspace too small (%lld bytes; ask vt_session_workspace_bytes: %lld)", what, (long long)ws_bytes,
          (long long)s->ws_bytes);
  Model& m = s->h->m;
  const int64_t hw = (int64_t)s->H * s->W, hwo = (int64_t)s->Ho * s->Wo;
  const bool dec = s->kind == VT_SESSION_DECODE;
  s->broken = true;
  {
    bind_workspace(m, ws, ws_bytes, s->staging);
    const ChunkBufs cb = chunk_bufs(ws, (size_t)s->B * s->cin * s->cap * hw, 0);     // inside the staging vt_session_create sized
    SessionSwap swap(s);
    TileScope scope(&m, s->graph(), dec && s->overlap);
    int npend = s->npend, done = 0;
    for (const SessionOp& op : plan) {
      if (!op.run) {
        M_CALL(vt_ncthw_copy_frames(in, (float*)s->pend.p, s->B * s->cin, n, s->cap, op.in_t0, npend, op.k, hw, 0, stream));
        npend += op.k;
        continue;
      }
      const float* x = (const float*)s->pend.p;
      if (op.nl != s->cap) {       // the chunk as a tensor of its own length (the pending buffer is laid out for `cap` frames)
        M_CALL(vt_ncthw_copy_frames(x, cb.in, s->B * s->cin, s->cap, op.nl, 0, 0, op.nl, hw, 0, stream));
        x = cb.in;
      }
      m.first_chunk = op.idx == 0;
      const int nres = dec ? op.nl * s->f : ceil_div(op.nl, s->f);
      if (dec) decode_impl(&m, s->graph(), x, s->B, op.nl, s->H, s->W, cb.out, stream, false);
      else encode_impl(&m, s->graph(), x, s->B, op.nl, s->H, s->W, cb.out, stream, false);
      M_CALL(vt_ncthw_copy_frames(cb.out, out, s->B * s->cout, nres, out_cap, 0, done, op.n_out, hwo, 0, stream));
      done += op.n_out;
      if (op.look)                 // the look-ahead latent opens the next chunk
        M_CALL(vt_ncthw_copy_frames((const float*)s->pend.p, (float*)s->pend.p, s->B * s->cin, s->cap, s->cap, op.nl - 1, 0, 1, hw, 0, stream));
      npend = op.look ? 1 : 0;
    }
  }
  s->npend = np;
  s->chunks = ch;
  s->finished = fin;
  s->broken = false;
  *n_out = outf;
  return VT_OK;
}

}  // namespace

extern "C" int vt_session_create(vt_model* h, int32_t kind, int32_t B, int32_t H, int32_t W, int32_t t_chunk, int32_t use_overlap, vt_session** out) {
  return guarded("vt_session_create", [&]() -> int {
    M_CHECK(out != nullptr, "vt_session_create: null argument");
    *out = nullptr;
    M_CHECK(h != nullptr, "vt_session_create: null handle");
    M_CHECK(h->m.v11(), "vt_session_create: sessions exist only for the v1.1 models (version 1): the v1.0 and non-causal models have no chunk protocol");
    M_CHECK(kind == VT_SESSION_ENCODE || kind == VT_SESSION_DECODE, "vt_session_create: kind must be VT_SESSION_ENCODE or VT_SESSION_DECODE");
    M_CHECK(B > 0 && H > 0 && W > 0 && t_chunk > 0, "vt_session_create: bad argument");
    Model& m = h->m;
    const vt_model_config& cf = m.cfg;
    const int f = cf.time_downsample_factor;
    auto s = std::make_unique<vt_session>();
    s->h = h;
    s->kind = kind;
    s->B = B; s->H = H; s->W = W; s->c = t_chunk; s->f = f;
    s->overlap = kind == VT_SESSION_DECODE && use_overlap != 0;
    if (kind == VT_SESSION_ENCODE) {
      M_CHECK(t_chunk % f == 0, "vt_session_create: t_chunk_enc (%d) must be a multiple of the temporal factor %d", t_chunk, f);
      const int ds = 1 << cf.n_spatial_ds;
      M_CHECK(H % ds == 0 && W % ds == 0, "vt_session_create: H and W must be multiples of %d", ds);
      check_loaded(h, "encoder.");
      s->cin = cf.in_channels;
      s->cout = cf.double_z ? 2 * cf.z_channels : cf.z_channels;
      s->Ho = H >> cf.n_spatial_ds; s->Wo = W >> cf.n_spatial_ds;
      s->cap = t_chunk;
      s->staging = tile_staging_bytes(cf, B, H, W, t_chunk);
    } else {
      check_loaded(h, "decoder.");
      s->cin = cf.z_channels;
      s->cout = cf.out_ch;
      s->Ho = H << cf.n_spatial_us; s->Wo = W << cf.n_spatial_us;
      s->cap = t_chunk + (s->overlap ? 1 : 0);
      s->staging = tile_staging_bytes(cf, B, s->Ho, s->Wo, t_chunk * f);
    }
    // dry walks over every chunk kind the schedule can meet (each chunk length after the first, with and without the look-ahead
    // frame): the arenas' peak sizes the workspace, the caches' sizes the session's state
    std::vector<CState*> gs;
    s->graph().states(gs);
    for (CState* g : gs) g->need = 0;
    size_t peak = 0;
    {
      ArenaScope arenas(&m);
      if (kind == VT_SESSION_ENCODE)
        for (int n = 1; n <= t_chunk; ++n) tile_encode_impl(&m, h->enc, nullptr, B, 1 + n, H, W, t_chunk, nullptr, nullptr, nullptr, true);
      else
        for (int n = 1; n <= t_chunk + 2; ++n) tile_decode_impl(&m, h->dec, nullptr, B, n, H, W, t_chunk, s->overlap, nullptr, nullptr, nullptr, true);
      peak = std::max(m.arena[0].peak, m.arena[1].peak);
    }
    s->ws_bytes = (int64_t)(s->staging + 2 * ((peak + 255) & ~(size_t)255) + 1024);
    s->st.resize(gs.size());
    for (size_t i = 0; i < gs.size(); ++i) {
      if (gs[i]->need == 0) continue;
      s->st[i].buf = std::make_unique<DevBuf>();
      M_HIP(hipMalloc(&s->st[i].buf->p, gs[i]->need));
      s->st[i].cap = gs[i]->need;
    }
    M_HIP(hipMalloc(&s->pend.p, (size_t)B * s->cin * s->cap * H * W * sizeof(float)));
    *out = s.release();
    return VT_OK;
  });
}

extern "C" int64_t vt_session_workspace_bytes(const vt_session* s) {
  if (!s) {
    vt_set_error("vt_session_workspace_bytes: null session");
    return -1;
  }
  return s->ws_bytes;
}

extern "C" int vt_session_push(vt_session* s, const float* in, int32_t n, float* out, int32_t out_cap_frames, int32_t* n_out, void* workspace,
                               int64_t workspace_bytes, vt_stream stream) {
  return guarded("vt_session_push", [&]() -> int {
    M_CHECK(s != nullptr && in != nullptr && n >= 1, "vt_session_push: bad argument (a session, and n >= 1 frames)");
    return session_step(s, in, n, out, out_cap_frames, n_out, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), false, "vt_session_push");
  });
}

extern "C" int vt_session_finish(vt_session* s, float* out, int32_t out_cap_frames, int32_t* n_out, void* workspace, int64_t workspace_bytes,
                                 vt_stream stream) {
  return guarded("vt_session_finish", [&]() -> int {
    return session_step(s, nullptr, 0, out, out_cap_frames, n_out, workspace, workspace_bytes, reinterpret_cast<hipStream_t>(stream), true,
                        "vt_session_finish");
  });
}

extern "C" int vt_session_destroy(vt_session* s) {
  delete s;                        // hipFree of its buffers waits for the work queued on them
  return VT_OK;
}
