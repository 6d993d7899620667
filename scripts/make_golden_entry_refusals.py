"""Record what the pointwise and backward entry points answer to arguments they refuse -> tests/golden/entry_refusal_table.json
(tests/test_entry_refusal_table.py replays it against the built library, code for code and byte for byte; no GPU needed).

    python scripts/make_golden_entry_refusals.py [--lib PATH] [--out PATH]     record (default: the in-tree library, the committed table)

Every call of CALLS is refused by a VT_CHECK_ARG before anything is launched or dereferenced: pointers are small integers (P: 16-byte
aligned, Q: not), never read.  The table pins the order of the checks and the text of their messages in pointwise.hip, groupnorm.hip,
regularizers.hip, metrics.hip, lpips.hip, lpips_grad.hip, video_io.hip, segments.hip, packing.hip, grad.hip, grad_decoder.hip and
patchgan.hip, so it is recorded with the library of the commit BEFORE a change of their host code.  Per entry point with a dtype
argument: dtype 99, VT_F16 where only fp32 / bf16 are served, a (dtype, second dtype) pair outside the served three, and where the
entry checks them a null pointer, a misaligned pointer and a bad extent or stride.  A row that is NOT refused (any status but
VT_ERR_ARG) stops the recording: such a call would reach a launch.  A row that differs later is a finding about the change at hand,
never a reason to record again."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from util import GOLDEN_DIR  # noqa: E402

VT_ERR_ARG = -1
F32, BF16, F16, BAD = 0, 1, 4, 99          # vt_dtype codes (vidtok_amd.lib.VT_*) and one that is none
P, Q = 16, 8                               # "pointers": aligned / not 16-byte aligned; never dereferenced

# entry points of the twelve files whose storage type comes in through a descriptor, not a parameter: (descriptor class, fields)
WGRAD_OK = dict(B=1, Ti=1, Hi=4, Wi=4, ldx=8, Cin=8, To=1, Ho=4, Wo=4, lddy=8, Cout=8, KT=1, KH=3, KW=3, st=1, sh=1, sw=1, ph=1, pw=1,
                ph_hi=1, pw_hi=1)
DGRAD_OK = dict(B=1, Ti=1, Hi=4, Wi=4, lddx=8, Cin=8, To=1, Ho=4, Wo=4, lddy=8, Cout=8, KT=1, KH=3, KW=3, st=1, sh=1, sw=1, ph=1, pw=1,
                ph_hi=1, pw_hi=1, ldw=72)

LN = lambda **k: _args([P, F32, 64, P, F32, 64, P, P, 4, 64, 1e-6, 1, None], k)                                     # noqa: E731
GN = lambda **k: _args([P, F32, 64, P, F32, 64, P, P, 1, 1, 16, 64, 32, 0, 1e-6, 1, None, None], k)                 # noqa: E731
LNB = lambda **k: _args([P, P, F32, 64, P, F32, 64, P, P, None, None, 4, 64, 1e-6, 1, P, 1 << 20, None], k)         # noqa: E731
BNS = lambda **k: _args([P, F32, 64, 4, 64, 1e-5, P, P, P, P, 1 << 20, None], k)                                    # noqa: E731
BNA = lambda **k: _args([P, F32, 64, P, 64, P, P, P, P, 0.2, 4, 64, None], k)                                       # noqa: E731
BNB = lambda **k: _args([P, P, F32, F32, 64, 64, P, 64, P, P, P, P, 0.2, None, None, 4, 64, 0, P, 1 << 20, None], k)  # noqa: E731


def _args(base, changes):
    """`base` with positions replaced: a0=..., a7=..."""
    out = list(base)
    for k, v in changes.items():
        out[int(k[1:])] = v
    return out


CALLS = [
    # ---- pointwise.hip
    ("vt_layernorm_act", LN(a1=BAD)), ("vt_layernorm_act", LN(a1=BF16, a4=F16)), ("vt_layernorm_act", LN(a4=BAD)),
    ("vt_layernorm_act", LN(a0=None)), ("vt_layernorm_act", LN(a2=32)), ("vt_layernorm_act", LN(a2=68)), ("vt_layernorm_act", LN(a9=24)),
    ("vt_tanh_inplace", [None, 4, None]), ("vt_tanh_inplace", [P, -1, None]),
    ("vt_softmax_rows", [P, P, BAD, 4, 8, 8, 1.0, None]), ("vt_softmax_rows", [P, P, 2, 4, 8, 8, 1.0, None]),
    ("vt_softmax_rows", [P, P, F32, 4, 8, 4, 1.0, None]), ("vt_softmax_rows", [None, P, F32, 4, 8, 8, 1.0, None]),
    ("vt_ncthw_to_ndhwc", [P, P, BAD, 1, 3, 1, 4, 4, 8, 0, None]), ("vt_ncthw_to_ndhwc", [P, P, 3, 1, 3, 1, 4, 4, 8, 0, None]),
    ("vt_ncthw_to_ndhwc", [P, P, F32, 1, 3, 1, 4, 4, 2, 0, None]), ("vt_ncthw_to_ndhwc", [P, None, F32, 1, 3, 1, 4, 4, 8, 0, None]),
    ("vt_ndhwc_to_ncthw", [P, BAD, P, 1, 3, 2, 4, 4, 8, 0, None]), ("vt_ndhwc_to_ncthw", [P, 2, P, 1, 3, 2, 4, 4, 8, 0, None]),
    ("vt_ndhwc_to_ncthw", [P, F32, P, 1, 3, 2, 4, 4, 8, 2, None]), ("vt_ndhwc_to_ncthw", [None, F32, P, 1, 3, 2, 4, 4, 8, 0, None]),
    ("vt_time_avgpool3s2", [P, None, P, BAD, 1, 2, 16, 8, 0, None]), ("vt_time_avgpool3s2", [P, None, P, 2, 1, 2, 16, 8, 0, None]),
    ("vt_time_avgpool3s2", [P, None, P, F32, 1, 1, 16, 8, 0, None]), ("vt_time_avgpool3s2", [P, None, P, F32, 1, 2, 3, 3, 0, None]),
    ("vt_time_avgpool3s2", [P, None, P, F32, 1, 2, 16, 8, 7, None]), ("vt_time_avgpool3s2", [P, None, P, F32, 1, 2, 16, 8, 2, None]),
    ("vt_time_lerp2x", [P, P, BAD, 1, 2, 64, None]), ("vt_time_lerp2x", [P, P, 3, 1, 2, 64, None]), ("vt_time_lerp2x", [P, P, F32, 1, 2, 6, None]),
    ("vt_time_lerp2x", [P, P, F32, 40000, 2, 64, None]),
    ("vt_time_lerp2x_cat", [None, 0, P, P, BAD, 1, 2, 0, 64, None]), ("vt_time_lerp2x_cat", [None, 0, P, P, 2, 1, 2, 0, 64, None]),
    ("vt_time_lerp2x_cat", [None, 1, P, P, F32, 1, 2, 0, 64, None]), ("vt_time_lerp2x_cat", [None, 0, P, P, F32, 1, 2, 4, 64, None]),
    ("vt_gather_frames", [P, P, 3, 1, 64, 64, 64, None, 1, None]), ("vt_gather_frames", [P, P, 4, 1, 64, 64, 64, None, 1, None]),
    # ---- groupnorm.hip
    ("vt_groupnorm_act", GN(a1=BAD)), ("vt_groupnorm_act", GN(a1=F16, a4=BF16)), ("vt_groupnorm_act", GN(a4=BAD)),
    ("vt_groupnorm_act", GN(a3=None)), ("vt_groupnorm_act", GN(a2=32)), ("vt_groupnorm_act", GN(a12=16)), ("vt_groupnorm_act", GN(a13=3)),
    # ---- regularizers.hip, metrics.hip, video_io.hip, segments.hip (no dtype argument: one refusal each)
    ("vt_kl_sample", [None, P, P, P, 1, 4, 16, None]), ("vt_fsq_quantize", [None, P, P, None, 3, 1, 16, None]),
    ("vt_fsq_indices_to_codes_cb", [P, P, None, 3, 1, 0, 16, None]), ("vt_channel_linear", [P, P, None, P, 1, 2048, 4, 16, None]),
    ("vt_fsq_aux_loss", [None, None, 1.0, 0.1, 0.25, P, None]), ("vt_entropy", [P, 0, P, None]),
    ("vt_fsq_aux_stats", [P, None, 3, 1, 0, 100.0, P, P, None]),
    ("vt_eval_psnr_ssim", [P, P, P, P, None, 1, 3, 1, 32, 32, 0, None]), ("vt_eval_psnr_ssim", [P, P, P, P, P, 1, 3, 1, 8, 8, 0, None]),
    ("vt_frames_u8_to_ncthw", [None, 1, 8, 8, 8, 8, 0, 0, P, 1, 0, 8, 8, P, None]),
    ("vt_frames_u8_to_ncthw", [P, 1, 8, 8, 8, 8, 1, 0, P, 1, 0, 8, 8, P, None]),
    ("vt_ncthw_to_frames_u8", [P, 2, 1, 2, 8, 8, P, 8, 0, None]), ("vt_ncthw_copy_frames", [P, P, 3, 2, 2, 1, 0, 2, 64, 0, None]),
    ("vt_copy_segments", [P, -1, 0, None]), ("vt_copy_segments", [None, 2, 64, None]),
    # ---- packing.hip
    ("vt_pack_conv_weight", [P, P, BAD, 8, 8, 8, 9, 9, None, 72, None]), ("vt_pack_conv_weight", [P, P, 2, 8, 8, 8, 9, 9, None, 72, None]),
    ("vt_pack_conv_weight", [P, None, F32, 8, 8, 8, 9, 9, None, 72, None]), ("vt_pack_conv_weight", [P, P, F32, 8, 8, 8, 9, 9, None, 64, None]),
    ("vt_pack_conv_weight", [P, P, 3, 8, 8, 8, 9, 9, None, 72, None]), ("vt_pack_conv_weight", [P, P, F32, 8, 8, 8, 9, 4, None, 72, None]),
    # ---- lpips.hip
    ("vt_lpips_prep", [P, P, P, P, P, BAD, 1, 1, 16, 16, 0, None]), ("vt_lpips_prep", [P, P, P, P, P, 2, 1, 1, 16, 16, 0, None]),
    ("vt_lpips_prep", [P, None, P, P, P, F32, 1, 1, 16, 16, 0, None]), ("vt_lpips_prep", [P, P, Q, P, P, F32, 1, 1, 16, 16, 0, None]),
    ("vt_lpips_prep", [P, P, P, P, P, F32, 1, 1, 8, 16, 0, None]), ("vt_lpips_prep", [P, P, P, P, P, F32, 1, 1, 16, 16, 8, None]),
    ("vt_lpips_tap", [P, P, P, P, 1 << 20, BAD, 1, 4, 4, 64, 0, None]), ("vt_lpips_tap", [P, P, P, P, 1 << 20, 3, 1, 4, 4, 64, 0, None]),
    ("vt_lpips_tap", [P, P, P, P, 1 << 20, F16, 1, 4, 4, 96, 0, None]), ("vt_lpips_tap", [P, P, None, P, 1 << 20, F32, 1, 4, 4, 64, 0, None]),
    ("vt_lpips_tap", [P, Q, P, P, 1 << 20, F32, 1, 4, 4, 64, 0, None]), ("vt_lpips_tap", [P, P, P, P, 1 << 20, F32, 1, 4, 4, 64, 5, None]),
    ("vt_lpips_tap", [P, P, P, P, 16, F32, 1, 4, 4, 64, 0, None]),
    ("vt_lpips_finish", [None, 1 << 20, P, None, 1, 16, 16, None]), ("vt_lpips_finish", [P, 16, P, None, 1, 16, 16, None]),
    # ---- lpips_grad.hip
    ("vt_lpips_tap_backward", [P, P, P, None, -1, P, BAD, 1, 4, 4, 64, None]), ("vt_lpips_tap_backward", [P, P, P, None, -1, P, F16, 1, 4, 4, 64, None]),
    ("vt_lpips_tap_backward", [P, P, P, P, F16, P, BF16, 1, 4, 4, 64, None]), ("vt_lpips_tap_backward", [P, P, P, P, BF16, P, F32, 1, 4, 4, 64, None]),
    ("vt_lpips_tap_backward", [P, P, P, None, -1, P, BF16, 1, 4, 4, 96, None]), ("vt_lpips_tap_backward", [P, P, None, None, -1, P, BF16, 1, 4, 4, 64, None]),
    ("vt_lpips_tap_backward", [P, P, P, Q, BF16, P, BF16, 1, 4, 4, 64, None]), ("vt_lpips_tap_backward", [P, P, P, None, -1, P, F32, 70000, 4, 4, 64, None]),
    ("vt_relu_backward", [P, F32, P, P, BAD, 16, None]), ("vt_relu_backward", [P, F32, P, P, F16, 16, None]),
    ("vt_relu_backward", [P, BF16, P, P, F32, 16, None]), ("vt_relu_backward", [P, F32, None, P, BF16, 16, None]),
    ("vt_relu_backward", [P, F32, P, P, BF16, 12, None]), ("vt_relu_backward", [P, F32, P, Q, BF16, 16, None]),
    ("vt_lpips_prep_backward", [P, BAD, P, P, 1, 16, 16, None]), ("vt_lpips_prep_backward", [P, F16, P, P, 1, 16, 16, None]),
    ("vt_lpips_prep_backward", [None, F32, P, P, 1, 16, 16, None]), ("vt_lpips_prep_backward", [Q, F32, P, P, 1, 16, 16, None]),
    ("vt_lpips_prep_backward", [P, F32, P, P, 0, 16, 16, None]),
    # ---- grad.hip
    ("vt_conv_wgrad", dict(WGRAD_OK, dtype=BAD)), ("vt_conv_wgrad", dict(WGRAD_OK, dtype=F16)), ("vt_conv_wgrad", dict(WGRAD_OK, dtype=BF16, lddy=4)),
    ("vt_conv_wgrad", dict(WGRAD_OK, dtype=F32)), ("vt_conv_wgrad", dict(WGRAD_OK, dtype=F32, x=P, dy=P, dw=P, work=P, work_bytes=16)),
    ("vt_layernorm_act_backward", LNB(a2=BAD)), ("vt_layernorm_act_backward", LNB(a2=F16, a5=F16)), ("vt_layernorm_act_backward", LNB(a2=F32, a5=BF16)),
    ("vt_layernorm_act_backward", LNB(a2=BF16, a5=F16)), ("vt_layernorm_act_backward", LNB(a1=None)), ("vt_layernorm_act_backward", LNB(a3=32)),
    ("vt_layernorm_act_backward", LNB(a12=520, a3=520, a6=520)), ("vt_layernorm_act_backward", LNB(a16=64)),
    # ---- grad_decoder.hip
    ("vt_pack_conv_weight_dgrad", [P, P, BAD, 8, 8, 8, 1, 3, 3, 1, 1, 1, 1, 72, None]), ("vt_pack_conv_weight_dgrad", [P, P, F16, 8, 8, 8, 1, 3, 3, 1, 1, 1, 1, 72, None]),
    ("vt_pack_conv_weight_dgrad", [None, P, F32, 8, 8, 8, 1, 3, 3, 1, 1, 1, 1, 72, None]), ("vt_pack_conv_weight_dgrad", [P, P, F32, 8, 8, 8, 1, 3, 3, 3, 1, 1, 1, 72, None]),
    ("vt_pack_conv_weight_dgrad", [P, P, F32, 8, 8, 8, 1, 3, 3, 1, 1, 1, 1, 64, None]),
    ("vt_conv_dgrad", dict(DGRAD_OK, dtype=BAD, dx_dtype=F32)), ("vt_conv_dgrad", dict(DGRAD_OK, dtype=F16, dx_dtype=F16)),
    ("vt_conv_dgrad", dict(DGRAD_OK, dtype=F32, dx_dtype=BF16)), ("vt_conv_dgrad", dict(DGRAD_OK, dtype=BF16, dx_dtype=BF16, lddy=4)),
    ("vt_conv_dgrad", dict(DGRAD_OK, dtype=F32, dx_dtype=F32)), ("vt_conv_dgrad", dict(DGRAD_OK, dtype=F32, dx_dtype=F32, st=2)),
    ("vt_grad_fold", [P, F32, None, P, BAD, 1, 1, 4, 4, 8, 8, 0, 8, 0, 0, 0, None]), ("vt_grad_fold", [P, F32, None, P, F16, 1, 1, 4, 4, 8, 8, 0, 8, 0, 0, 0, None]),
    ("vt_grad_fold", [P, BF16, None, P, F32, 1, 1, 4, 4, 8, 8, 0, 8, 0, 0, 0, None]), ("vt_grad_fold", [P, F32, None, P, F32, 1, 1, 4, 4, 8, 8, 0, 10, 0, 0, 0, None]),
    ("vt_grad_fold", [None, F32, None, P, F32, 1, 1, 4, 4, 8, 8, 0, 8, 0, 0, 0, None]),
    ("vt_softmax_rows_backward", [P, 8, P, P, 8, BAD, 4, 8, 1.0, None]), ("vt_softmax_rows_backward", [P, 8, P, P, 8, F16, 4, 8, 1.0, None]),
    ("vt_softmax_rows_backward", [P, 8, None, P, 8, F32, 4, 8, 1.0, None]), ("vt_softmax_rows_backward", [P, 4, P, P, 8, F32, 4, 8, 1.0, None]),
    ("vt_transpose_batched", [P, P, BAD, 1, 4, 8, 8, 4, None]), ("vt_transpose_batched", [P, P, F16, 1, 4, 8, 8, 4, None]),
    ("vt_transpose_batched", [P, P, F32, 1, 4, 8, 8, 2, None]), ("vt_transpose_batched", [P, None, F32, 1, 4, 8, 8, 4, None]),
    ("vt_upsample_mix", [P, P, P, P, BAD, 4, 8, 8, None]), ("vt_upsample_mix", [P, P, P, P, F16, 4, 8, 8, None]),
    ("vt_upsample_mix", [P, P, None, P, F32, 4, 8, 8, None]), ("vt_upsample_mix", [P, P, P, P, F32, 4, 8, 4, None]),
    ("vt_upsample_mix_backward", [P, P, P, P, P, P, P, BAD, 4, 8, 8, P, 1 << 20, None]), ("vt_upsample_mix_backward", [P, P, P, P, P, P, P, F16, 4, 8, 8, P, 1 << 20, None]),
    ("vt_upsample_mix_backward", [P, P, P, P, P, P, None, F32, 4, 8, 8, P, 1 << 20, None]), ("vt_upsample_mix_backward", [P, P, P, P, P, P, P, F32, 4, 8, 8, P, 2, None]),
    ("vt_time_lerp2x_backward", [P, P, BAD, 1, 2, 64, None]), ("vt_time_lerp2x_backward", [P, P, F16, 1, 2, 64, None]),
    ("vt_time_lerp2x_backward", [P, P, F32, 40000, 2, 64, None]), ("vt_time_lerp2x_backward", [None, P, F32, 1, 2, 64, None]),
    ("vt_grad_ncthw_to_ndhwc", [P, P, BAD, 1, 3, 1, 4, 4, 8, 0, None]), ("vt_grad_ncthw_to_ndhwc", [P, P, F16, 1, 3, 1, 4, 4, 8, 0, None]),
    ("vt_grad_ncthw_to_ndhwc", [P, P, F32, 1, 3, 1, 4, 4, 2, 0, None]), ("vt_grad_ncthw_to_ndhwc", [None, P, F32, 1, 3, 1, 4, 4, 8, 0, None]),
    ("vt_grad_add", [P, P, P, BAD, 64, None]), ("vt_grad_add", [P, P, P, F16, 64, None]), ("vt_grad_add", [P, P, P, F32, 0, None]),
    ("vt_grad_add", [P, None, P, F32, 64, None]),
    # ---- patchgan.hip
    ("vt_batchnorm_stats", BNS(a1=BAD)), ("vt_batchnorm_stats", BNS(a1=F16)), ("vt_batchnorm_stats", BNS(a0=None)), ("vt_batchnorm_stats", BNS(a0=Q)),
    ("vt_batchnorm_stats", BNS(a2=60)), ("vt_batchnorm_stats", BNS(a4=520, a2=520)), ("vt_batchnorm_stats", BNS(a10=64)),
    ("vt_batchnorm_act", BNA(a1=BAD)), ("vt_batchnorm_act", BNA(a1=F16)), ("vt_batchnorm_act", BNA(a5=None)), ("vt_batchnorm_act", BNA(a3=Q)),
    ("vt_batchnorm_act", BNA(a4=60)),
    ("vt_batchnorm_act_backward", BNB(a2=BAD)), ("vt_batchnorm_act_backward", BNB(a2=F16, a3=F16)), ("vt_batchnorm_act_backward", BNB(a2=F32, a3=BF16)),
    ("vt_batchnorm_act_backward", BNB(a2=BF16, a3=F16)), ("vt_batchnorm_act_backward", BNB(a18=None)), ("vt_batchnorm_act_backward", BNB(a17=2)),
    ("vt_batchnorm_act_backward", BNB(a5=60)), ("vt_batchnorm_act_backward", BNB(a1=Q)), ("vt_batchnorm_act_backward", BNB(a19=64)),
    ("vt_leaky_relu_backward", [P, F32, P, P, BAD, 16, 0.2, None]), ("vt_leaky_relu_backward", [P, F16, P, P, F16, 16, 0.2, None]),
    ("vt_leaky_relu_backward", [P, BF16, P, P, F32, 16, 0.2, None]), ("vt_leaky_relu_backward", [P, F32, None, P, BF16, 16, 0.2, None]),
    ("vt_leaky_relu_backward", [P, F32, P, P, BF16, 12, 0.2, None]), ("vt_leaky_relu_backward", [P, F32, P, P, BF16, 16, 0.0, None]),
    ("vt_leaky_relu_backward", [Q, F32, P, P, BF16, 16, 0.2, None]),
]

DESCRIPTORS = {"vt_conv_wgrad": "WgradDesc", "vt_conv_dgrad": "DgradDesc"}
# what the table need not hold two rows of: the exported names of the other translation units (the convolution launchers, the
# attention, the model handle, options and errors), and the entry points of the twelve files that take no storage type
OUT_OF_SCOPE_PREFIXES = ("vt_conv_act", "vt_conv_plan", "vt_conv_launch_form", "vt_conv_profile", "vt_conv_work_bytes", "vt_conv_desc_size", "vt_conv_max_lds_bytes",
                         "vt_time_upsample3", "vt_temporal_block", "vt_tblock", "vt_flash_attention", "vt_session", "vt_tile", "vt_regularize")


def key(name, args):
    if isinstance(args, dict):
        return name + "{" + ",".join(f"{k}={v}" for k, v in sorted(args.items())) + "}"
    return name + "(" + ",".join("null" if a is None else repr(a) for a in args) + ")"


def call(lib, name, args):
    """(status, message) of one call of the table"""
    from vidtok_amd import lib as L

    if isinstance(args, dict):
        d = getattr(L, DESCRIPTORS[name])(**args)
        rc = getattr(lib, name)(C.byref(d), None)
    else:
        rc = getattr(lib, name)(*args)
    return rc, (lib.vt_last_error() or b"").decode()


def dtype_entries():
    """in-scope names of lib.SIGNATURES that take a storage type: a parameter named *dtype in include/vidtok_amd.h, or a descriptor"""
    import re

    from vidtok_amd import lib as L

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vidtok_amd.h")).read(), flags=re.S)
    out = set(DESCRIPTORS)
    for name in L.SIGNATURES:
        m = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", hdr)
        if m and re.search(r"\b\w*dtype\b", m.group(1)) and name != "vt_conv" and not name.startswith(OUT_OF_SCOPE_PREFIXES) and name != "vt_create":
            out.add(name)
    return sorted(out)


def main(argv):
    from vidtok_amd import lib as L

    lib = L.load(argv[argv.index("--lib") + 1] if "--lib" in argv else None)
    rows = {}
    for name, args in CALLS:
        k = key(name, args)
        assert k not in rows, f"{k} twice"
        rc, msg = call(lib, name, args)
        if rc != VT_ERR_ARG:
            print(f"{k}: status {rc} ({msg!r}): not refused -- not a row of this table; nothing written")
            return 1
        rows[k] = [rc, msg]
    out = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(GOLDEN_DIR, "entry_refusal_table.json")
    with open(out, "w") as f:
        json.dump(rows, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(rows)} rows, {len({v[1] for v in rows.values()})} distinct messages, {os.path.getsize(out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
