"""The PatchGAN discriminator restated in torch.nn, in our own words, as the reference of the HIP path (tests only).

`RefPatchGan` has the state_dict keys of vidtok.modules.discriminator.NLayerDiscriminator (main.0 ... main.11); `seeded` fills it with
seeded weights large enough that every layer matters and with non-trivial running statistics; `run64` is the fp64 CPU autograd pass that
every gate is measured against: logits, dx, every parameter gradient and the running statistics after the call.
"""
import copy

import torch
import torch.nn as nn

SLOPE = 0.2
SHAPES = ((3, 3, 27, 36), (5, 3, 24, 24))        # the shapes of the recorded golden (tests/golden/patchgan.safetensors)
GOLDEN = "patchgan.safetensors"


class RefPatchGan(nn.Module):
    def __init__(self, input_nc=3, ndf=64, n_layers=3):
        super().__init__()
        chans = [ndf * min(2 ** n, 8) for n in range(n_layers + 1)]
        seq = [nn.Conv2d(input_nc, chans[0], 4, 2, 1), nn.LeakyReLU(SLOPE)]
        for n in range(1, n_layers + 1):
            stride = 2 if n < n_layers else 1
            seq += [nn.Conv2d(chans[n - 1], chans[n], 4, stride, 1, bias=False), nn.BatchNorm2d(chans[n]), nn.LeakyReLU(SLOPE)]
        seq += [nn.Conv2d(chans[-1], 1, 4, 1, 1)]
        self.main = nn.Sequential(*seq)

    def forward(self, x):
        return self.main(x)


def seeded(seed=0, ndf=64, n_layers=3, cls=RefPatchGan):
    """a network with seeded parameters (He-scaled convolutions, so activations keep their size through the depth) and seeded running
    statistics; `cls` may be the reference's class: it is filled through its state_dict"""
    g = torch.Generator().manual_seed(seed)
    net = cls(ndf=ndf, n_layers=n_layers)
    sd = net.state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            v.fill_(3)
        elif k.endswith("running_mean"):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif v.dim() == 4:
            v.copy_(torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * 16)) ** 0.5)
        elif isinstance(net.main[int(k.split(".")[1])], nn.BatchNorm2d):
            v.copy_((1.0 if k.endswith("weight") else 0.0) + 0.2 * torch.randn(v.shape, generator=g))
        else:
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
    net.load_state_dict(sd)
    return net


def make_inputs(shape, seed):
    """(frames in [-1, 1]-like range, cotangent of the logits' shape is made by the caller from the logits)"""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(shape, generator=g).clamp_(-2.5, 2.5) * 0.5


def cotangent(logits_shape, seed):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(logits_shape, generator=g)


def run(net, x, train, dtype=torch.float64, cot=None, seed=0):
    """one forward + backward of a COPY of `net` on the CPU in `dtype` -> dict(logits, dx, grads {key: tensor}, stats {buffer key: tensor}),
    everything returned in fp64; the loss is sum(cot * logits)"""
    net = copy.deepcopy(net).to(dtype)
    net.train(train)
    xx = x.detach().to(dtype).requires_grad_(True)
    y = net(xx)
    if cot is None:
        cot = cotangent(y.shape, seed)
    (y * cot.to(dtype)).sum().backward()
    return dict(logits=y.detach().double(), dx=xx.grad.double(), cot=cot,
                grads={k: p.grad.double() for k, p in net.named_parameters()},
                stats={k: v.detach().double().clone() for k, v in net.named_buffers()})


def run64(net, x, train, cot=None, seed=0):
    return run(net, x, train, torch.float64, cot, seed)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def rel_max(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
