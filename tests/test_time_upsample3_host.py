"""The three-product form of the causal v1.0 time up-sampler (vt_time_upsample3), the parts that need no GPU: the packed weights, the
identity itself against the oracle, and the serving rule vt_time_upsample3_supported (a function of the descriptor and the option table)."""
import pytest
import torch
import torch.nn.functional as F

from conv_plan_cases import PTR, g
from vidtok_amd import lib as L
from vidtok_amd.packing import pack_conv_weight, time_upsample3_mix, time_upsample3_weights


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_packed_rows_are_the_reference_taps_rounded_once(dtype):
    """[W0 | W2] and W1 as vt_conv rows: k = tap * Cin_stored + c, every element the fp32 weight's tap rounded once -- nothing summed"""
    gen = torch.Generator().manual_seed(3)
    co, ci, cs = 16, 12, 16
    w = torch.randn((co, ci, 3, 3, 3), generator=gen)
    u = pack_conv_weight(time_upsample3_weights(w, "u"), dtype, cin_stored=cs)
    v = pack_conv_weight(time_upsample3_weights(w, "v"), dtype, cin_stored=cs)
    assert u.shape == (co, 18 * cs) and v.shape == (co, 9 * cs) and u.dtype == dtype and v.dtype == dtype
    u, v = u.view(co, 2, 3, 3, cs), v.view(co, 3, 3, cs)
    taps = w.permute(0, 2, 3, 4, 1).to(dtype)                      # [co, kt, kh, kw, ci]
    assert torch.equal(u[:, 0, ..., :ci], taps[:, 0]) and torch.equal(u[:, 1, ..., :ci], taps[:, 2]) and torch.equal(v[..., :ci], taps[:, 1])
    assert not u[..., ci:].any() and not v[..., ci:].any()         # the channel pad meets zeros
    # the device packer's tap tables name the same taps
    assert time_upsample3_mix((3, 3, 3), "u") == [[i] for i in range(9)] + [[18 + i] for i in range(9)]
    assert time_upsample3_mix((3, 3, 3), "v") == [[9 + i] for i in range(9)]


def test_three_products_equal_the_oracle_upsampler():
    """o[2j] = U[j] + V[j-1], o[2j+1] = U[j] + V[j] with U[j] = W0 x[j-1] + W2 x[j], V[j] = W1 x[j], x[-1] = V[-1] = 0 per clip, then the
    alpha-mix against x[j]: the oracle's TimeUpsampleResCausal2x (nearest x2, causal 3 x 3 x 3 convolution) in fp32 to 1e-5"""
    import oracle.vidtok_oracle as O

    gen = torch.Generator().manual_seed(11)
    B, T, H, W, C = 2, 3, 8, 8, 16
    x = torch.randn((B, C, T, H, W), generator=gen)
    sd = {"up.conv.conv.weight": torch.randn((C, C, 3, 3, 3), generator=gen) / (27 * C) ** 0.5, "up.conv.conv.bias": torch.randn((C,), generator=gen) * 0.1,
          "up.mix_factor": torch.tensor([0.2])}
    ref = O.time_upsample(sd, "up", x, "v1_0", None, "nearest", 1)
    wu, wv = time_upsample3_weights(sd["up.conv.conv.weight"], "u"), time_upsample3_weights(sd["up.conv.conv.weight"], "v")
    U = F.conv3d(F.pad(x, (1, 1, 1, 1, 1, 0)), wu, sd["up.conv.conv.bias"])
    V = F.conv3d(F.pad(x, (1, 1, 1, 1)), wv, None)
    Vprev = torch.cat([torch.zeros_like(V[:, :, :1]), V[:, :, :-1]], dim=2)         # per clip: the batch dimension is not shifted
    a = torch.sigmoid(sd["up.mix_factor"])
    out = torch.stack([a * x + (1 - a) * (U + Vprev), a * x + (1 - a) * (U + V)], dim=3).reshape(B, C, 2 * T, H, W)
    assert out.shape == ref.shape
    assert ((out - ref).abs().max() / ref.abs().max()).item() < 1e-5


def _desc(base, dtype, **kw):
    f = dict(base, res_mode=L.VT_RES_MIX, res=PTR, mix_factor=PTR, dtype=dtype, out_dtype=L.VT_F32 if dtype == L.VT_BF16X3 else dtype)
    f.setdefault("ldr", f["ldy"])
    f.setdefault("Tr", f["To"])
    f.update(kw)
    if "ln_mode" in f:
        f.update(ln_gamma=PTR, ln_beta=PTR, ln_out=PTR)
        f.setdefault("ldn", f["ldy"])
    d = L.ConvDesc()
    for k, v in f.items():
        setattr(d, k, v)
    return d


def test_supported_accepts_and_rejects(built_lib, vt_opts):
    sup = lambda d: built_lib.vt_time_upsample3_supported(d)        # noqa: E731
    big256 = g(4, 10, 256, 256, 256, 256, (2, 3, 3), yt_mul=2, yt_off=0)     # the benchmark's two up-samplers
    big512 = g(4, 5, 128, 128, 512, 512, (2, 3, 3), yt_mul=2, yt_off=0)
    for dt in (L.VT_BF16, L.VT_F16):
        assert sup(_desc(big256, dt)) == 1 and sup(_desc(big512, dt)) == 1
        assert sup(_desc(big256, dt, ln_mode=2, ln_keep_y=1)) == 1            # Cout = 256: the LayerNorm rides along (option conv_tup_ln)
        assert sup(_desc(big512, dt, ln_mode=2, ln_keep_y=1)) == 0            # Cout = 512: nobody fuses it; the hosts ask without
    assert sup(_desc(big256, L.VT_F32)) == 0 and sup(_desc(dict(big256, ldw=18 * 256), L.VT_BF16X3)) == 0
    bf = L.VT_BF16
    assert sup(_desc(dict(big256, yt_off=1), bf)) == 0                        # the odd parity launch is not the paired launch
    assert sup(_desc(dict(big256, yt_mul=1), bf)) == 0
    assert sup(_desc(big256, bf, res_mode=L.VT_RES_ADD)) == 0 and sup(_desc(big256, bf, res_mode=L.VT_RES_NONE)) == 0
    assert sup(_desc(dict(big256, tmode=L.VT_TPAD_REPLICATE), bf)) == 0       # zero time padding only
    assert sup(_desc(g(4, 10, 256, 256, 256, 256, (3, 3, 3), yt_mul=2), bf)) == 0 and sup(_desc(g(4, 10, 256, 256, 256, 256, (2, 1, 1), yt_mul=2), bf)) == 0
    assert sup(_desc(g(4, 10, 256, 256, 256, 128, (2, 3, 3), yt_mul=2), bf)) == 0       # Cout % 256
    assert sup(_desc(g(4, 10, 256, 256, 32, 256, (2, 3, 3), yt_mul=2), bf)) == 0        # Cin % 64: no tap walk
    assert sup(_desc(dict(big256, ldy=260), bf)) == 0 and sup(_desc(big256, bf, ldr=260)) == 0      # 16-byte rows
    assert sup(_desc(dict(big256, x=0), bf)) == 0                             # what vt_conv's validation rejects
    # one clip's geometry, never B: 3 frames of 16 x 16 make 3 tiles -- below conv_tile_min whatever the batch; forced, served whatever the batch
    small = [g(B, 3, 16, 16, 256, 256, (2, 3, 3), yt_mul=2) for B in (1, 2, 64)]
    assert [sup(_desc(s, bf)) for s in small] == [0, 0, 0]
    assert sup(_desc(g(64, 3, 16, 16, 256, 256, (2, 3, 3), yt_mul=2), bf, ln_mode=1, ln_keep_y=1)) == 0
    vt_opts(conv_tile=256)
    assert [sup(_desc(s, bf)) for s in small] == [1, 1, 1]
    assert sup(_desc(small[1], bf, ln_mode=1, ln_keep_y=1)) == 1
    assert sup(_desc(g(2, 3, 8, 8, 256, 256, (2, 3, 3), yt_mul=2), bf)) == 0  # 64 pixels per frame: a tile would span frames
    assert sup(_desc(g(2, 3, 16, 24, 256, 256, (2, 3, 3), yt_mul=2), bf)) == 0
    vt_opts(conv_tile=128)
    assert sup(_desc(big256, bf)) == 0
    vt_opts(conv_tile=0, conv_tup3=0)
    assert sup(_desc(big256, bf)) == 0 and sup(_desc(big512, L.VT_F16)) == 0
    vt_opts(conv_tup3=1, conv_tup_ln=0)
    assert sup(_desc(big256, bf)) == 1 and sup(_desc(big256, bf, ln_mode=2, ln_keep_y=1)) == 0
    vt_opts(conv_tup_ln=1, conv_buf=0)
    assert sup(_desc(big256, bf)) == 0                                        # the paired launch gathers through buffer descriptors


def test_launch_refuses_what_supported_refuses(built_lib):
    """vt_time_upsample3 validates before it launches: VT_ERR_ARG for an uncovered descriptor and for a bad V operand (no GPU touched)"""
    big = g(4, 10, 256, 256, 256, 256, (2, 3, 3), yt_mul=2, yt_off=0)
    assert built_lib.vt_time_upsample3(_desc(big, L.VT_F32), PTR, 256, None) != 0 and b"vt_time_upsample3" in built_lib.vt_last_error()
    d = _desc(big, L.VT_BF16)
    for v, ldv in ((None, 256), (PTR + 8, 256), (PTR, 128), (PTR, 260)):
        assert built_lib.vt_time_upsample3(d, v, ldv, None) != 0 and b"ldv" in built_lib.vt_last_error()
