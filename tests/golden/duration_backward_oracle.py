"""Float64 oracle of DurationPredictor's gradients (pure torch on the CPU).

Shared by test_duration_backward_host.py, test_gpu_duration_backward.py and
test_gpu_model_backward.py.  As encoder_backward_oracle.py: the module's own
nn.Conv1d layers and BatchNorm parameters and buffers are deep-copied to the
CPU and differentiated by torch autograd; BatchNorm is
F.batch_norm(training=False), the running statistics as constants, and every
ReLU is a product with a constant 0/1 mask, so that the side of each kink can
be prescribed.  Nothing reads the reference.

The function, for enc [B, S, H]: x = enc^T; per ConvBlock u = conv(x),
a = batch_norm(u), y = a [a > 0]; z = projection(y2); dur = softplus(z).  The
ReLU's pre-activation is a.

The cases (H, B, S, modifiers): enc and d_dur are N(0, 1).  The conv weights
and biases are the module's own init under torch.manual_seed(seed); BatchNorm
weights are set N(1, 0.2), biases N(0, 0.2), running means N(0, 0.5) and
running variances uniform in [0.3, 2], so nothing is tested against a
degenerate statistic.  Modifiers:
  gamma    in each block norm.weight[1] = 0 (with norm.bias[1] = 0.3, so the
           channel is alive and d gamma there is not zero) and
           norm.weight[2] = -0.7 (with norm.bias[2] = 0.3, running_mean[2] = 0);
  eps      BatchNorm eps 1e-3 instead of 1e-5;
  extreme  projection.weight x 400 and projection.bias 50, which puts some z
           above 20 (softplus's threshold branch) and some below -30.
"""
import copy

import torch
import torch.nn.functional as F

CASES = {
    "s1": (64, 2, 100, ("gamma",)),             # the stage1 width: two 64-position chunks, the last partial
    "one": (32, 1, 1, ()),                      # one row
    "edge63": (32, 3, 63, ("eps",)),            # one short of a chunk
    "tile": (96, 2, 64, ("extreme",)),          # exactly one chunk; six 16-wide n-blocks
    "wide": (128, 2, 65, ("gamma", "extreme")),  # the widest; one past a chunk
    "long": (64, 1, 130, ()),                   # three chunks, five 32-position transpose tiles
    "thin": (16, 2, 7, ("gamma", "eps")),       # the narrowest
    "h24": (24, 2, 33, ()),                     # H % 16 != 0
}
# Seeds at which CPU float32 and float64 agree on the side of every ReLU kink
# (test_duration_backward_host.py asserts it).
SEEDS = {"s1": 0, "one": 1, "edge63": 2, "tile": 3, "wide": 4, "long": 5, "thin": 6, "h24": 7}
GAMMA_ZERO, GAMMA_NEG = 1, 2  # the channels the `gamma` modifier sets
N_PARAMS = 10


def randomize_norms(pred, seed, mods=()):
    """Non-degenerate BatchNorm parameters and running statistics, then the modifiers (in place)."""
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for blk in pred.predictor.conv_layers:
            n = blk.norm
            n.weight.copy_(torch.randn(n.weight.shape, generator=g) * 0.2 + 1.0)
            n.bias.copy_(torch.randn(n.bias.shape, generator=g) * 0.2)
            n.running_mean.copy_(torch.randn(n.running_mean.shape, generator=g) * 0.5)
            n.running_var.copy_(torch.rand(n.running_var.shape, generator=g) * 1.7 + 0.3)
            if "gamma" in mods:
                n.weight[GAMMA_ZERO] = 0.0
                n.bias[GAMMA_ZERO] = 0.3
                n.weight[GAMMA_NEG] = -0.7
                n.bias[GAMMA_NEG] = 0.3
                n.running_mean[GAMMA_NEG] = 0.0
            if "eps" in mods:
                n.eps = 1e-3
        if "extreme" in mods:
            pred.predictor.projection.weight.mul_(400.0)
            pred.predictor.projection.bias.fill_(50.0)
    return pred


def make_predictor(case):
    """The stand-alone DurationPredictor of a case (on the CPU, float32, eval mode)."""
    from models.tts_model import DurationPredictor
    H, _, _, mods = CASES[case]
    seed = SEEDS[case]
    torch.manual_seed(seed)
    return randomize_norms(DurationPredictor(hidden_dim=H).eval(), seed, mods)


def make_inputs(case):
    """(enc [B,S,H], d_dur [B,S]) float32."""
    H, B, S, _ = CASES[case]
    g = torch.Generator().manual_seed(2000 + SEEDS[case])
    return torch.randn(B, S, H, generator=g), torch.randn(B, S, generator=g)


def cpu_copy(pred, dtype):
    """`pred` deep-copied to the CPU in `dtype` (the running statistics too), every parameter a leaf that
    requires grad."""
    c = copy.deepcopy(pred).to("cpu", dtype)
    for p in c.parameters():
        p.requires_grad_(True)
        p.grad = None
    return c


def parameters(pred):
    """parameters() order: (conv.weight, conv.bias, norm.weight, norm.bias) x 2, projection.weight, .bias."""
    return [p for _, p in pred.named_parameters()]


def forward(pred, enc, positive=None):
    """(dur [B,S], the ReLU pre-activations a1, a2 [B,H,S], the conv outputs u1, u2, z [B,S]).  positive[i]
    (bool [B,H,S], or None: the copy's own sign) says where block i's ReLU passes its input."""
    x = enc.transpose(1, 2)
    pre, convs = [], []
    for i, blk in enumerate(pred.predictor.conv_layers):
        n = blk.norm
        u = blk.conv(x)
        a = F.batch_norm(u, n.running_mean, n.running_var, n.weight, n.bias, False, 0.0, n.eps)
        pos = (a.detach() > 0) if positive is None else positive[i]
        x = a * pos.to(a.dtype)
        pre.append(a)
        convs.append(u)
    z = pred.predictor.projection(x).squeeze(1)
    return F.softplus(z), pre, convs, z


def gradients(pred, enc, d_dur, positive=None):
    """(the 10 gradients in parameters() order, d_enc, dur, pre-activations) of sum(dur * d_dur)."""
    enc = enc.detach().clone().requires_grad_(True)
    dur, pre, _, _ = forward(pred, enc, positive)
    grads = torch.autograd.grad(dur, parameters(pred) + [enc], d_dur)
    return list(grads[:-1]), grads[-1], dur.detach(), [a.detach() for a in pre]


def plain_gradients(pred, enc, d_dur):
    """The same through the nn modules in eval mode, torch.relu and F.softplus alone."""
    assert not pred.training
    enc = enc.detach().clone().requires_grad_(True)
    x = enc.transpose(1, 2)
    for blk in pred.predictor.conv_layers:
        x = torch.relu(blk.norm(blk.conv(x)))
    dur = F.softplus(pred.predictor.projection(x)).squeeze(1)
    grads = torch.autograd.grad(dur, parameters(pred) + [enc], d_dur)
    return list(grads[:-1]), grads[-1], dur.detach()
