"""Float64 oracle of the discriminator step's gradients (pure torch on the CPU).

Shared by test_gpu_losses_backward.py and test_losses_backward_host.py.  The
module's own nn.Conv1d stacks are deep-copied to the CPU and differentiated by
torch autograd, with every LeakyReLU applied as a multiplication by a constant
slope mask, so that the side of each kink can be prescribed: a pre-activation
within float32 rounding of 0 may take the other slope on the GPU, and one such
element moves every gradient upstream of it by far more than rounding.
"""
import copy

import torch
import torch.nn.functional as F

SLOPE = 0.2


def cpu_stacks(disc, dtype):
    """The nn.Conv1d layers of every scale of a MultiScaleDiscriminator, copied to the CPU in `dtype`."""
    stacks = []
    for seq in disc.discriminators:
        convs = [copy.deepcopy(m).to("cpu", dtype) for m in seq if isinstance(m, torch.nn.Conv1d)]
        for c in convs:
            for p in c.parameters():
                p.requires_grad_(True)
                p.grad = None
        stacks.append(convs)
    return stacks


def parameters(stacks):
    """state_dict order: weight, bias per layer, scale after scale."""
    return [p for convs in stacks for c in convs for p in (c.weight, c.bias)]


def forward(stacks, scales, x, positive=None):
    """One side through every scale.  positive[s][l] (bool, or None: the stack's own sign) says where
    LeakyReLU after layer l of scale s passes its input unscaled.  Returns (logits per scale, the
    six pre-activation maps per scale)."""
    outs, maps = [], []
    for s, (scale, convs) in enumerate(zip(scales, stacks)):
        h = x if scale == 1 else F.avg_pool1d(x, scale, scale)
        pre = []
        for l, conv in enumerate(convs):
            h = conv(h)
            if l < len(convs) - 1:
                pre.append(h)
                pos = (h.detach() > 0) if positive is None else positive[s][l]
                h = h * torch.where(pos, torch.ones((), dtype=h.dtype), torch.full((), SLOPE, dtype=h.dtype))
        outs.append(h)
        maps.append(pre)
    return outs, maps


def discriminator_loss(stacks, scales, real, fake, positive_real=None, positive_fake=None):
    """L_D = mean over scales of [mean (D(real) - 1)^2 + mean D(fake)^2] and the maps of both sides."""
    ro, rm = forward(stacks, scales, real, positive_real)
    fo, fm = forward(stacks, scales, fake, positive_fake)
    loss = sum(((r - 1) ** 2).mean() + (f ** 2).mean() for r, f in zip(ro, fo)) / len(scales)
    return loss, rm, fm


def gradients(stacks, scales, real, fake, positive_real=None, positive_fake=None):
    """(loss, the 42 gradients in state_dict order, real maps, fake maps); the stacks' .grad are left unset."""
    loss, rm, fm = discriminator_loss(stacks, scales, real, fake, positive_real, positive_fake)
    grads = torch.autograd.grad(loss, parameters(stacks))
    detach = lambda maps: [[m.detach() for m in row] for row in maps]  # noqa: E731
    return loss.detach(), list(grads), detach(rm), detach(fm)


def plain_gradients(stacks, scales, real, fake):
    """The same loss through F.leaky_relu, differentiated by autograd alone."""
    total = 0
    for x, target in ((real, 1.0), (fake, 0.0)):
        for scale, convs in zip(scales, stacks):
            h = x if scale == 1 else F.avg_pool1d(x, scale, scale)
            for l, conv in enumerate(convs):
                h = conv(h)
                if l < len(convs) - 1:
                    h = F.leaky_relu(h, SLOPE)
            total = total + ((h - target) ** 2).mean()
    loss = total / len(scales)
    return loss.detach(), list(torch.autograd.grad(loss, parameters(stacks)))
