"""Pure-torch restatement of the reference LPIPS (vidtok/modules/lpips.py) and of its eval-loop use (scripts/inference_evaluate.py:
175-186) on a state_dict with the reference's keys (TEST INFRASTRUCTURE: no torchvision, runs on the CPU or the GPU).  `dtype` runs the
VGG16 convolutions in bf16 / fp16 (the torch-statement baseline of scripts/lpips_bench.py); the head stays fp32 like the kernels'."""
import torch
import torch.nn.functional as F

CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
POOLS = (4, 9, 16, 23)
TAPS = (3, 8, 15, 22, 29)            # the ReLU of relu1_2 ... relu5_3 in features[0:30]
SLICE = {i: k + 1 for k, (a, b) in enumerate(((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))) for i in range(a, b)}


def _lin(sd, k):
    w = sd.get(f"lin{k}.model.1.weight")
    return sd[f"lin{k}.model.0.weight"] if w is None else w


def vgg_taps(sd, h, dtype=torch.float32):
    """the five ReLU taps of vgg16 slices 1..5 on scaled images h (NCHW)"""
    h = h.to(dtype)
    outs = []
    for i in range(30):
        if i in CONVS:
            p = f"net.slice{SLICE[i]}.{i}."
            h = F.conv2d(h, sd[p + "weight"].to(h), sd[p + "bias"].to(h), padding=1)
        elif i in POOLS:
            h = F.max_pool2d(h, 2, 2)
        else:
            h = F.relu(h)
        if i in TAPS:
            outs.append(h)
    return outs


def normalize_tensor(x, eps=1e-10):
    norm_factor = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True))
    return x / (norm_factor + eps)


def lpips(sd, x, y, dtype=torch.float32, with_taps=False):
    """LPIPS(x, y) of NCHW images in [-1, 1] -> [N] (and the per-tap means [5, N])"""
    shift, scale = sd["scaling_layer.shift"].to(x), sd["scaling_layer.scale"].to(x)
    a, b = (x - shift) / scale, (y - shift) / scale
    fa, fb = vgg_taps(sd, a, dtype), vgg_taps(sd, b, dtype)
    res = []
    for k in range(5):
        d = (normalize_tensor(fa[k].float()) - normalize_tensor(fb[k].float())) ** 2
        res.append(F.conv2d(d, _lin(sd, k).to(d)).mean([2, 3], keepdim=True))
    val = res[0]
    for r in res[1:]:
        val = val + r
    val = val.reshape(-1)
    return (val, torch.stack([r.reshape(-1) for r in res])) if with_taps else val


def eval_frames(sd, x, xrec, dtype=torch.float32, with_taps=False):
    """the eval loop's per-frame LPIPS of NCTHW clips: clamp only the reconstruction, (v+1)/2, LPIPS on v*2-1 -> [B, T]"""
    out = xrec.clamp(-1, 1)
    inp, out = (x + 1) / 2, (out + 1) / 2
    B, C, T, H, W = x.shape
    inp = inp.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
    out = out.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
    r = lpips(sd, inp * 2 - 1, out * 2 - 1, dtype, with_taps)
    return (r[0].reshape(B, T), r[1]) if with_taps else r.reshape(B, T)
