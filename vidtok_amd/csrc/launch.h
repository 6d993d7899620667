// Host-side launch helpers of the pointwise and backward entry points (not the convolution launchers, which decide in conv_select.h).
// An entry point validates with VT_CHECK_ARG, picks its kernel instantiation with one of the vt_dispatch forms over the types it
// SERVES -- the list is written at the call, so nothing outside it is instantiated -- and hands the kernel to launch().
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.h"

inline hipStream_t as_stream(vt_stream s) { return reinterpret_cast<hipStream_t>(s); }

// workgroups for n items at per_block items a workgroup, 1 .. cap: the span and the cap are the call site's and differ on purpose
// (a grid-stride kernel's cap is its resident-wave budget; kernels with per-workgroup partials fix the partial count with it)
inline unsigned grid_for(long long n, long long per_block, long long cap) {
  return (unsigned)std::max<long long>(1, std::min<long long>((n + per_block - 1) / per_block, cap));
}

template <typename... P>
inline bool aligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t(0)) & 15) == 0; }

inline int64_t align256(int64_t n) { return (n + 255) / 256 * 256; }

// the storage types of the backward entry points
inline bool grad_dtype_ok(int dt) { return dt == VT_F32 || dt == VT_BF16; }

// launch + the launch check; returns the entry point's status
template <typename... KArgs, typename... Args>
int launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, std::forward<Args>(args)...);
  VT_CHECK_LAUNCH();
  return VT_OK;
}

// ---- dispatch: fn is a generic lambda, called once with a tag (or integral constant) of the match; its status is returned --------
template <typename T>
struct vt_tag {
  using type = T;
};
template <typename Tag>
using vt_t = typename Tag::type;    // using T = vt_t<decltype(tag)>;

// nothing in the list matched: no vt_status has this value, and the caller raises its own message
// (VT_CHECK_ARG(st != kNoMatch, ...)); a caller that validated the value beforehand returns the status as it is
constexpr int kNoMatch = 1;

// over storage types by vt_dtype code: vt_dispatch<float, bf16_t, f16_t>(dtype, [&](auto t) { ... })
template <typename... Ts, typename F>
int vt_dispatch(int dtype, F&& fn) {
  int st = kNoMatch;
  (void)((dtype == dtype_code<Ts>::value && ((st = fn(vt_tag<Ts>{})), true)) || ...);
  return st;
}

// over unit types by size in bytes (kernels that only move data)
template <typename... Ts, typename F>
int vt_dispatch_size(int bytes, F&& fn) {
  int st = kNoMatch;
  (void)((bytes == (int)sizeof(Ts) && ((st = fn(vt_tag<Ts>{})), true)) || ...);
  return st;
}

// over a small set of integers that are template arguments: fn gets std::integral_constant<int, N>
template <int... Ns, typename F>
int vt_dispatch_int(int v, F&& fn) {
  int st = kNoMatch;
  (void)((v == Ns && ((st = fn(std::integral_constant<int, Ns>{})), true)) || ...);
  return st;
}

// the backward entry points' (T, TD): operands in T = fp32 or bf16, the second tensor (a cotangent, or dx) in T or in fp32
template <typename F>
int vt_dispatch_grad(int dtype, int d_dtype, F&& fn) {
  if (dtype == VT_F32 && d_dtype == VT_F32) return fn(vt_tag<float>{}, vt_tag<float>{});
  if (dtype == VT_BF16 && d_dtype == VT_F32) return fn(vt_tag<bf16_t>{}, vt_tag<float>{});
  if (dtype == VT_BF16 && d_dtype == VT_BF16) return fn(vt_tag<bf16_t>{}, vt_tag<bf16_t>{});
  return kNoMatch;
}

// the normalisations' (TI, TO): both of one storage type, or one of the two fp32
template <typename F>
int vt_dispatch_io(int in_dtype, int out_dtype, F&& fn) {
  return vt_dispatch<float, bf16_t, f16_t>(in_dtype, [&](auto ti) {
    return vt_dispatch<float, bf16_t, f16_t>(out_dtype, [&](auto to) {
      using TI = vt_t<decltype(ti)>;
      using TO = vt_t<decltype(to)>;
      if constexpr (std::is_same_v<TI, TO> || std::is_same_v<TI, float> || std::is_same_v<TO, float>) return fn(ti, to);
      else return kNoMatch;
    });
  });
}
