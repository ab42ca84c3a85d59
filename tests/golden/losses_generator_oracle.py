"""Oracle of the generator step's gradient through the discriminators (pure torch on the CPU).

Builds on losses_backward_oracle.forward: the module's own nn.Conv1d stacks on the CPU in a given
dtype, every LeakyReLU a product with a constant slope mask that can be prescribed for both sides,
and the feature-matching term either as mean |d| or, with prescribed signs, as mean (d * sgn), whose
gradient is sgn / count whatever side of 0 the difference d = f_fake - f_real fell on.

    objective = w_adv * (1/3) sum_s mean (D_s(fake) - 1)^2
              + w_fm * (1/18) sum_{s,j} mean |f_{s,j}(fake) - f_{s,j}(real)|

Only the fake audio is differentiated: the real maps are constants and the parameters get nothing.
"""
import torch
import torch.nn.functional as F

import losses_backward_oracle as orc


def objective(stacks, scales, real, fake, w_adv, w_fm, positive_real=None, positive_fake=None, signs=None):
    """(objective, real maps or None, fake maps).  real may be None when w_fm == 0.  signs[s][j]
    (the stacks' dtype, values -1, 0, 1; None: the difference's own sign) prescribes sign(f_fake - f_real)."""
    fo, fm = orc.forward(stacks, scales, fake, positive_fake)
    total = w_adv * sum(((f - 1) ** 2).mean() for f in fo) / len(scales)
    rm = None
    if real is not None:
        with torch.no_grad():
            _, rm = orc.forward(stacks, scales, real, positive_real)
    if w_fm != 0:
        terms = 0
        for s in range(len(scales)):
            for j in range(len(fm[s])):
                d = fm[s][j] - rm[s][j]
                terms = terms + (d.abs().mean() if signs is None else (d * signs[s][j]).mean())
        total = total + w_fm * terms / (len(scales) * len(fm[0]))
    return total, rm, fm


def gradient(stacks, scales, real, fake, w_adv, w_fm, positive_real=None, positive_fake=None, signs=None):
    """(objective, d objective / d fake, real maps or None, fake maps), all detached."""
    x = fake.detach().clone().requires_grad_(True)
    total, rm, fm = objective(stacks, scales, real, x, w_adv, w_fm, positive_real, positive_fake, signs)
    (g,) = torch.autograd.grad(total, x)
    return total.detach(), g, rm, [[m.detach() for m in row] for row in fm]


def masks(maps):
    """Where each LeakyReLU passes its input unscaled."""
    return [[m > 0 for m in row] for row in maps]


def signs_of(fake_maps, real_maps, dtype):
    """sign(f_fake - f_real) per map, in `dtype`."""
    return [[torch.sign(f - r).to(dtype) for f, r in zip(fr, rr)] for fr, rr in zip(fake_maps, real_maps)]


def plain_gradient(stacks, scales, real, fake, w_adv, w_fm):
    """The reference's formulas (F.mse_loss, F.l1_loss, F.leaky_relu) differentiated by autograd alone."""
    x = fake.detach().clone().requires_grad_(True)

    def run(a):
        outs, feats = [], []
        for scale, convs in zip(scales, stacks):
            h = a if scale == 1 else F.avg_pool1d(a, scale, scale)
            row = []
            for l, conv in enumerate(convs):
                h = conv(h)
                if l < len(convs) - 1:
                    row.append(h)
                    h = F.leaky_relu(h, orc.SLOPE)
            outs.append(h)
            feats.append(row)
        return outs, feats

    fo, ff = run(x)
    gen = sum(F.mse_loss(o, torch.ones_like(o)) for o in fo) / len(fo)
    total = w_adv * gen
    if w_fm != 0:
        with torch.no_grad():
            _, rf = run(real)
        fmv = sum(F.l1_loss(a, b) for ra, rb in zip(ff, rf) for a, b in zip(ra, rb)) / (len(ff) * len(ff[0]))
        total = total + w_fm * fmv
    (g,) = torch.autograd.grad(total, x)
    return total.detach(), g
