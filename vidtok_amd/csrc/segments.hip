// vt_copy_segments: many small device-to-device copies in ONE launch, from a table on the device.
//
// A v1.1 tokenizer keeps dozens of small chunk-cache tensors (one or two frames of one layer each).  A streaming session
// (vidtok_amd/streaming.py, the vt_session_* calls of model.cpp) parks its causal state in buffers of its own between pushes
// and moves it in and out of the buffers the model's kernels (and captured graphs) read; as separate copies that is ~2 x N
// launches per push, here it is two.  The table is read on the device, so the launch is graph-capture safe: a captured
// switch replays against whatever the table holds at replay time.
//
// Layout: blockIdx.y = segment, blockIdx.x strides over the segment's bytes.  16-byte loads and stores where both ends are
// 16-byte aligned, 4-byte where they are 4-byte aligned, bytes otherwise; the tail past the last whole vector is copied by
// the threads of the segment's first block.
#include "launch.h"

namespace {

constexpr int kBlock = 256;
constexpr int kUnroll = 4;                 // loads in flight per thread before their stores
constexpr int kMaxBlocksPerSeg = 1024;     // a cache of a 256 x 256 clip is tens of MB: enough waves to keep HBM busy

template <typename V>
__device__ __forceinline__ void copy_vec(const char* src, char* dst, int64_t nvec, int64_t t0, int64_t stride) {
  const V* s = reinterpret_cast<const V*>(src);
  V* d = reinterpret_cast<V*>(dst);
  int64_t i = t0;
  for (; i + (kUnroll - 1) * stride < nvec; i += kUnroll * stride) {
    V v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) v[u] = s[i + u * stride];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) d[i + u * stride] = v[u];
  }
  for (; i < nvec; i += stride) d[i] = s[i];
}

__global__ void __launch_bounds__(kBlock) copy_segments_kernel(const vt_copy_segment* __restrict__ table) {
  const vt_copy_segment sg = table[blockIdx.y];
  const char* src = static_cast<const char*>(sg.src);
  char* dst = static_cast<char*>(sg.dst);
  const int64_t bytes = sg.bytes;
  if (bytes <= 0) return;
  const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
  const uintptr_t al = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst);
  int64_t body;
  if ((al & 15) == 0) {
    body = bytes & ~(int64_t)15;
    copy_vec<u32x4>(src, dst, body >> 4, t0, stride);
  } else if ((al & 3) == 0) {
    body = bytes & ~(int64_t)3;
    copy_vec<uint32_t>(src, dst, body >> 2, t0, stride);
  } else {
    body = 0;
  }
  if (body == 0) {
    for (int64_t i = t0; i < bytes; i += stride) dst[i] = src[i];
  } else if (blockIdx.x == 0) {
    for (int64_t i = body + threadIdx.x; i < bytes; i += kBlock) dst[i] = src[i];
  }
}

}  // namespace

extern "C" int vt_copy_segments(const vt_copy_segment* table, int32_t n, int64_t max_bytes, vt_stream stream_) {
  VT_CHECK_ARG(n >= 0 && max_bytes >= 0, "vt_copy_segments: bad arguments");
  if (n == 0) return VT_OK;
  VT_CHECK_ARG(table != nullptr && n <= 65535, "vt_copy_segments: table must be a device array of 1 .. 65535 entries");
  // max_bytes only sizes the grid (each block strides over its segment, whatever its length)
  const dim3 grid(grid_for(max_bytes, (long long)kBlock * 16 * kUnroll, kMaxBlocksPerSeg), n);
  return launch(copy_segments_kernel, grid, dim3(kBlock), 0, as_stream(stream_), table);
}
