// Implicit-GEMM convolution kernel (conv_igemm_kernel.h) with a ReLU in the epilogue: the instantiations behind vt_conv_act
// (conv_igemm.hip validates the descriptor).  Only the tiles the VGG16 feature stack of LPIPS selects are instantiated, in fp32, bf16
// and fp16 arithmetic with results in the same type:
//   Cout <= 64          the 256 x 64 tile (4 waves), the tap-walk form or -- Cin = 8, the 3-channel image stored as 8 -- the general one
//   Cout % 256 == 0     the 8-wave 256 x 256 tile; in a 16-bit type with the LDS-transposed epilogue where it applies (full tiles)
//   otherwise           the 128 x 128 tile (4 waves), two workgroups per CU
// The K loops are the ones vt_conv runs; ACT = VT_ACT_RELU changes the epilogues only (max(v, 0) on the fp32 result, then the rounding).
#include "conv_igemm_kernel.h"

namespace {

template <typename MT>
int dispatch_relu(const IgemmLaunch& l, hipStream_t stream) {
  const IgemmVariant& v = l.v;
  constexpr int R = VT_ACT_RELU;
  VT_CHECK_VARIANT(v.stages == 2 && v.rowb == kRowBytes);
  if (v.tile == TILE_256x64 && v.ln256 == 0) {
    if (v.fast) return launch_variant<MT, MT, TILE_256x64, true, 0, 2, kRowBytes, R>(l, stream);
    return launch_variant<MT, MT, TILE_256x64, false, 0, 2, kRowBytes, R>(l, stream);
  }
  VT_CHECK_VARIANT(v.fast);        // vt_conv_act refuses the general gather beyond Cout = 64 (conv_act_decide, conv_igemm.hip)
  if (v.tile == TILE_256x256) {
    if constexpr (is_h16<MT>::value) {
      if (v.ln256) return launch_variant<MT, MT, TILE_256x256, true, 1, 2, kRowBytes, R>(l, stream);
    }
    VT_CHECK_VARIANT(v.ln256 == 0);
    return launch_variant<MT, MT, TILE_256x256, true, 0, 2, kRowBytes, R>(l, stream);
  }
  VT_CHECK_VARIANT(v.tile == TILE_128x128 && v.ln256 == 0);
  return launch_variant<MT, MT, TILE_128x128, true, 0, 2, kRowBytes, R>(l, stream);
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) int vt_igemm_dispatch_relu(const void* launch, int dtype, void* stream) {
  const IgemmLaunch& l = *reinterpret_cast<const IgemmLaunch*>(launch);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VT_F32) return dispatch_relu<float>(l, s);
  if (dtype == VT_F16) return dispatch_relu<f16_t>(l, s);
  return dispatch_relu<bf16_t>(l, s);
}
