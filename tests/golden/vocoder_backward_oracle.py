"""Float64 oracle of SimpleVocoder's gradients (pure torch on the CPU).

Shared by test_vocoder_backward_host.py and test_gpu_vocoder_backward.py.  The
module's own nn.Conv1d / nn.ConvTranspose1d layers are deep-copied to the CPU
and differentiated by torch autograd, with every LeakyReLU applied as a
multiplication by a constant slope mask, so that the side of each kink can be
prescribed (as losses_backward_oracle.py does): a pre-activation within
float32 rounding of 0 may take the other slope on the GPU, and one such
element moves every gradient upstream of it by far more than rounding.

The cases (M, C, B, T, seed): mel and d_audio are N(0, 1); the weights are the
module's own init under torch.manual_seed(seed), the biases N(0, 0.05), so no
bias gradient is tested against a zero bias.
"""
import copy

import torch
import torch.nn.functional as F

SLOPE = 0.1
RATES = (4, 4, 2, 2)
CASES = {
    "s1": (64, 128, 2, 5, 0),      # the stage1 shape at a few frames
    "s2": (80, 256, 1, 3, 1),      # the stage2 shape
    "thin": (5, 32, 3, 1, 2),      # every layer narrow; T = 1 is shorter than every halo; odd M
    "tiles": (64, 128, 2, 70, 3),  # several position tiles and split-K chunks at every stage
    "odd": (64, 128, 1, 17, 4),    # no length a multiple of a tile
}
PRE = tuple(f"{n}{k}" for k in range(4) for n in ("u", "v"))  # the eight pre-activation maps


def make_vocoder(case):
    """The stand-alone SimpleVocoder of a case (on the CPU, float32)."""
    from models.tts_model import SimpleVocoder
    M, C, _, _, seed = CASES[case]
    torch.manual_seed(seed)
    voc = SimpleVocoder(mel_channels=M, hidden_channels=C)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in voc.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return voc


def make_inputs(case):
    """(mel [B,M,T], d_audio [B,1,64T]) float32."""
    M, _, B, T, seed = CASES[case]
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(B, M, T, generator=g), torch.randn(B, 1, 64 * T, generator=g)


def cpu_copy(voc, dtype):
    """`voc` deep-copied to the CPU in `dtype`, every parameter a leaf that requires grad."""
    c = copy.deepcopy(voc).to("cpu", dtype)
    for p in c.parameters():
        p.requires_grad_(True)
        p.grad = None
    return c


def parameters(voc):
    """state_dict order."""
    return [p for _, p in voc.named_parameters()]


def _leaky(h, positive, name):
    pos = (h.detach() > 0) if positive is None else positive[name]
    return h * torch.where(pos, torch.ones((), dtype=h.dtype), torch.full((), SLOPE, dtype=h.dtype))


def forward(voc, mel, positive=None):
    """(audio, the eight pre-activation maps u_k = ConvT_k(x_k), v_k = conv1_k(a_k)).  positive[name]
    (bool, or None: the copy's own sign) says where that LeakyReLU passes its input unscaled."""
    pre = {}
    x = voc.input_conv(mel)
    for k in range(4):
        u = voc.upsamples[k](x)
        a = _leaky(u, positive, f"u{k}")
        v = voc.resblocks[k].conv1(a)
        x = voc.resblocks[k].conv2(_leaky(v, positive, f"v{k}")) + a
        pre[f"u{k}"], pre[f"v{k}"] = u, v
    return torch.tanh(voc.output_conv(x)), pre


def gradients(voc, mel, d_audio, positive=None):
    """(the 28 gradients in state_dict order, d_mel, audio, pre-activation maps) of sum(audio * d_audio)."""
    mel = mel.detach().clone().requires_grad_(True)
    audio, pre = forward(voc, mel, positive)
    grads = torch.autograd.grad(audio, parameters(voc) + [mel], d_audio)
    return list(grads[:-1]), grads[-1], audio.detach(), {k: v.detach() for k, v in pre.items()}


def plain_gradients(voc, mel, d_audio):
    """The same through F.leaky_relu and the nn modules alone."""
    mel = mel.detach().clone().requires_grad_(True)
    x = voc.input_conv(mel)
    for k in range(4):
        a = F.leaky_relu(voc.upsamples[k](x), SLOPE)
        x = voc.resblocks[k].conv2(F.leaky_relu(voc.resblocks[k].conv1(a), SLOPE)) + a
    audio = torch.tanh(voc.output_conv(x))
    grads = torch.autograd.grad(audio, parameters(voc) + [mel], d_audio)
    return list(grads[:-1]), grads[-1], audio.detach()
