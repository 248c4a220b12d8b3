"""Float64 yardstick of the PatchGAN discriminator tests, written from the definitions with torch on the CPU: ``nn.Conv2d(.., 4, s, 1)``,
``nn.BatchNorm2d``, ``nn.LeakyReLU(0.2)`` (Isola et al. 2017: C64-C128-C256-C512 with 4x4 convs, BatchNorm from the second layer on,
one logit per patch).  Everything here is NCHW and double precision; a case is computed once and shared by the tests that need it.

Measured on the CPU: torch's own fp32 run of the network (ndf 16, 64^2, B 4) is within 1.3e-6 relative of this float64 run on the
logits, the input gradient and every parameter gradient; a single 64 -> 64 stride-2 conv is at 5.5e-7 of max in fp32 and 3.8e-3 in
bf16."""
import torch
from torch import nn

SLOPE = 0.2
# the project's conv bounds, relative to max |result|; every K here (<= 16 * 64) is below the 9 * 512 they were set at
CONV_BOUND = {'fp32': 2e-5, 'bf16': 1e-2}
BN_BOUND_FP32 = 5e-6            # the GroupNorm bound of DESIGN section 5
BN_PARAM_BOUND_FP32 = 7e-6      # dgamma / dbeta
BF16_EPS = 2.0 ** -8            # one rounding to nearest of a stored bf16 element, relative to the element


class NLayerDiscriminatorRef(nn.Module):
    def __init__(self, input_nc=3, ndf=64, n_layers=3):
        super().__init__()
        seq = [nn.Conv2d(input_nc, ndf, 4, 2, 1), nn.LeakyReLU(SLOPE)]
        mult = 1
        for n in range(1, n_layers + 1):
            prev, mult = mult, min(2 ** n, 8)
            seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 2 if n < n_layers else 1, 1, bias=False), nn.BatchNorm2d(ndf * mult),
                    nn.LeakyReLU(SLOPE)]
        seq.append(nn.Conv2d(ndf * mult, 1, 4, 1, 1))
        self.main = nn.Sequential(*seq)
        for m in self.modules():                    # the usual initialisation: conv N(0, 0.02), BatchNorm N(1, 0.02) / 0
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0.0, 0.02)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.normal_(m.weight, 1.0, 0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.main(x)


def expected_keys(n_layers=3):
    keys = ['main.0.weight', 'main.0.bias']
    for n in range(1, n_layers + 1):
        i = 3 * n - 1
        keys.append(f'main.{i}.weight')
        keys += [f'main.{i + 1}.{k}' for k in ('weight', 'bias', 'running_mean', 'running_var', 'num_batches_tracked')]
    last = 3 * n_layers + 2
    return keys + [f'main.{last}.weight', f'main.{last}.bias']


def out_size(size, stride):
    return (size + 2 - 4) // stride + 1


def rel(got, want):
    """max |got - want| / max |want| (the metric of every bound in this family)"""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


_CONV: dict = {}


def conv_case(n, h, w, cin, cout, stride, bias, lrelu, dtype, seed=0):
    """inputs (rounded to ``dtype`` where the kernels store them: x and dy; the weights stay fp32 masters, rounded inside the bf16
    kernels, so the float64 reference rounds them the same way) and float64 y, dx, dw, db of one conv layer"""
    key = (n, h, w, cin, cout, stride, bias, lrelu, dtype, seed)
    if key in _CONV:
        return _CONV[key]
    g = torch.Generator().manual_seed(1000 + seed)
    tdt = torch.float32 if dtype == 'fp32' else torch.bfloat16
    x = torch.randn(n, cin, h, w, generator=g).to(tdt)
    wgt = (torch.randn(cout, cin, 4, 4, generator=g) * (1.0 / (16 * cin) ** 0.5)).float()
    b = torch.randn(cout, generator=g).float() if bias else None
    ho, wo = out_size(h, stride), out_size(w, stride)
    dy = torch.randn(n, cout, ho, wo, generator=g).to(tdt)
    xd = x.double().requires_grad_(True)
    wd = wgt.to(tdt).double().requires_grad_(True)
    bd = b.double().requires_grad_(True) if bias else None
    y = torch.nn.functional.conv2d(xd, wd, bd, stride=stride, padding=1)
    if lrelu:
        y = torch.nn.functional.leaky_relu(y, SLOPE)
    grads = torch.autograd.grad(y, [xd, wd] + ([bd] if bias else []), dy.double())
    _CONV[key] = dict(x=x, w=wgt, b=b, dy=dy, y=y.detach(), dx=grads[0], dw=grads[1], db=grads[2] if bias else None)
    return _CONV[key]


def dgrad_phases(dy, w, h, wd):
    """stride-2 data gradient of the 4x4 / padding-1 conv as four input-parity phases of 2x2 taps each: input row 2 j + p reads
    dy rows j + p - a through kernel rows (1 - p) + 2 a, a in {0, 1} (columns alike); rows / columns no output reads stay zero"""
    n, co, ho, wo = dy.shape
    ci = w.shape[1]
    dx = torch.zeros(n, ci, h, wd, dtype=dy.dtype)
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for b in (0, 1):
                    kh, kw = (1 - py) + 2 * a, (1 - px) + 2 * b
                    for j in range((h - py + 1) // 2):
                        oy = j + py - a
                        if not 0 <= oy < ho:
                            continue
                        for i in range((wd - px + 1) // 2):
                            ox = i + px - b
                            if 0 <= ox < wo:
                                dx[:, :, 2 * j + py, 2 * i + px] += dy[:, :, oy, ox] @ w[:, :, kh, kw]
    return dx


_BN: dict = {}


def bn_case(n, c, h, w, lrelu, dtype, mean=0.0, seed=0, calls=1):
    """float64 BatchNorm2d (+ LeakyReLU) in training mode: y, batch mean / rstd, running buffers after ``calls`` calls on the same
    input, dx / dgamma / dbeta, and the eval-mode output with those running statistics"""
    key = (n, c, h, w, lrelu, dtype, mean, seed, calls)
    if key in _BN:
        return _BN[key]
    g = torch.Generator().manual_seed(2000 + seed)
    tdt = torch.float32 if dtype == 'fp32' else torch.bfloat16
    x = (torch.randn(n, c, h, w, generator=g) + mean).to(tdt)
    gamma = (1.0 + 0.3 * torch.randn(c, generator=g)).float()
    beta = (0.2 * torch.randn(c, generator=g)).float()
    dy = torch.randn(n, c, h, w, generator=g).to(tdt)
    bn = nn.BatchNorm2d(c).double()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    xd = x.double().requires_grad_(True)
    for _ in range(calls):
        z = bn(xd)
    y = torch.nn.functional.leaky_relu(z, SLOPE) if lrelu else z
    dx, dg, db = torch.autograd.grad(y, [xd, bn.weight, bn.bias], dy.double())
    mu = x.double().mean((0, 2, 3))
    var = x.double().var((0, 2, 3), unbiased=False)
    bn.eval()
    with torch.no_grad():
        ze = bn(x.double())
        ye = torch.nn.functional.leaky_relu(ze, SLOPE) if lrelu else ze
    _BN[key] = dict(x=x, gamma=gamma, beta=beta, dy=dy, y=y.detach(), mean=mu, rstd=(var + bn.eps).rsqrt(), dx=dx, dgamma=dg, dbeta=db,
                    running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                    num_batches_tracked=int(bn.num_batches_tracked), y_eval=ye)
    return _BN[key]


_NET: dict = {}


def net_case(ndf=16, n_layers=3, batch=4, size=64, seed=0):
    """the whole discriminator in float64, training mode: state dict (before the pass), input, logits, the input gradient and every
    parameter gradient of sum(logits * dlogits), buffers after the pass"""
    key = (ndf, n_layers, batch, size, seed)
    if key in _NET:
        return _NET[key]
    torch.manual_seed(3000 + seed)
    net = NLayerDiscriminatorRef(3, ndf, n_layers)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(3100 + seed)
    img = torch.randn(batch, 3, size, size, generator=g)
    net64 = NLayerDiscriminatorRef(3, ndf, n_layers).double()
    net64.load_state_dict(state)
    net64.train()
    xd = img.double().requires_grad_(True)
    logits = net64(xd)
    dlog = torch.randn(logits.shape, generator=g)
    params = dict(net64.named_parameters())
    grads = torch.autograd.grad(logits, [xd] + list(params.values()), dlog.double())
    _NET[key] = dict(state=state, img=img, dlogits=dlog, logits=logits.detach(), dimg=grads[0],
                     grads={k: v for k, v in zip(params, grads[1:])},
                     buffers={k: v.clone() for k, v in net64.state_dict().items() if k not in params})
    return _NET[key]
