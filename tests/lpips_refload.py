"""TEST INFRASTRUCTURE ONLY (build container): the *unmodified* reference vidtok/modules/lpips.py, importable without torchvision and
without any way to reach the network.

Before the import, sys.modules gets stand-ins for
  torchvision.models.vgg16(pretrained=...)  -> an object whose .features is the 31-layer VGG16 nn.Sequential in torchvision's index order
                                                (uninitialised weights: the tests load a state_dict);
  requests                                   -> a module whose get() raises at once;
and afterwards LPIPS.load_from_pretrained, download and get_ckpt_path of the loaded module are replaced by stand-ins (the first a no-op,
the other two raise), so the reference's download path is unreachable.  The previous sys.modules entries are restored after the import.
"""
import sys
import types

import torch.nn as nn

_MOD = None


def vgg16_features():
    layers, c = [], 3
    for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"):
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(c, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            c = v
    return nn.Sequential(*layers)


def _no_network(*a, **k):
    raise RuntimeError("the tests never reach the network")


def reference_lpips_module():
    global _MOD
    if _MOD is not None:
        return _MOD
    from oracle.refload import _install_stubs

    _install_stubs()
    tv, tvm, rq = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("requests")
    tvm.vgg16 = lambda pretrained=False, **kw: types.SimpleNamespace(features=vgg16_features())
    tv.models = tvm
    rq.get = _no_network
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.models", "requests")}
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "requests": rq})
    try:
        import importlib

        mod = importlib.import_module("vidtok.modules.lpips")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    mod.LPIPS.load_from_pretrained = lambda self, name="vgg_lpips": None
    mod.download = _no_network
    mod.get_ckpt_path = _no_network
    _MOD = mod
    return mod


def reference_lpips(use_dropout=True):
    return reference_lpips_module().LPIPS(use_dropout=use_dropout).eval()


def reference_taps(ref, x, y):
    """per-tap spatial means [5, N] from the reference module's own pieces (the steps of LPIPS.forward, lpips.py:82-95)"""
    mod = reference_lpips_module()
    outs0, outs1 = ref.net(ref.scaling_layer(x)), ref.net(ref.scaling_layer(y))
    lins = [ref.lin0, ref.lin1, ref.lin2, ref.lin3, ref.lin4]
    res = []
    for kk in range(5):
        d = (mod.normalize_tensor(outs0[kk]) - mod.normalize_tensor(outs1[kk])) ** 2
        res.append(mod.spatial_average(lins[kk].model(d), keepdim=True).reshape(-1))
    import torch

    return torch.stack(res)
