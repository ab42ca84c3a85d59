"""Float64 oracle of MelDecoder's gradients (pure torch on the CPU).

Shared by test_decoder_backward_host.py and test_gpu_decoder_backward.py.  The
module's own nn.Linear / nn.LayerNorm layers are deep-copied to the CPU and
differentiated by torch autograd; attention is computed as the reference
writes it (scores * scale, masked_fill(-1e9), softmax, @ v), and every ReLU is
applied as a product with a constant 0/1 mask, so that the side of each kink
can be prescribed: a pre-activation within float32 rounding of 0 may take the
other side on the GPU, and one such element moves every gradient upstream of
it by far more than rounding.

The cases (H, M, layers, heads, B, T): x and d_mel are N(0, 1); the linear
weights are the module's own init under torch.manual_seed(seed).
initialize_weights leaves LayerNorm at 1 / 0 and every bias at 0, so LayerNorm
weights are set N(1, 0.2), LayerNorm biases N(0, 0.2) and linear biases
N(0, 0.1): no gradient is tested against a degenerate parameter.
"""
import copy

import torch

CASES = {
    "s1": (64, 64, 2, 2, 2, 5),        # the stage1 decoder at a few frames
    "s2": (96, 80, 3, 2, 1, 3),        # the stage2 decoder: head_dim 48
    "thin": (32, 5, 1, 2, 3, 1),       # head_dim 16, T = 1, odd M
    "tiles": (64, 64, 2, 2, 2, 130),   # 260 rows: five 64-row tiles, the last partial; three key chunks
    "odd": (96, 80, 1, 2, 1, 67),      # no length a multiple of a tile
    "wide": (128, 80, 1, 2, 1, 65),    # head_dim 64, ffn 256 (the limit)
    "heads4": (64, 64, 1, 4, 2, 33),   # four heads
}
LAYER_PARAMS = 11


def make_decoder(case):
    """The stand-alone MelDecoder of a case (on the CPU, float32)."""
    from models.tts_model import MelDecoder
    H, M, layers, heads, _, _ = CASES[case]
    seed = list(CASES).index(case)
    torch.manual_seed(seed)
    dec = MelDecoder(hidden_dim=H, mel_channels=M, num_layers=layers, num_heads=heads)
    g = torch.Generator().manual_seed(1000 + seed)
    norms = {id(m) for m in dec.modules() if isinstance(m, torch.nn.LayerNorm)}
    with torch.no_grad():
        for mod in dec.modules():
            for name, p in mod.named_parameters(recurse=False):
                if id(mod) in norms:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.2 + (1.0 if name == "weight" else 0.0))
                elif name == "bias":
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return dec


def make_inputs(case):
    """(x [B,T,H], d_mel [B,T,M]) float32."""
    H, M, _, _, B, T = CASES[case]
    g = torch.Generator().manual_seed(2000 + list(CASES).index(case))
    return torch.randn(B, T, H, generator=g), torch.randn(B, T, M, generator=g)


def cpu_copy(dec, dtype):
    """`dec` deep-copied to the CPU in `dtype`, every parameter a leaf that requires grad."""
    c = copy.deepcopy(dec).to("cpu", dtype)
    for p in c.parameters():
        p.requires_grad_(True)
        p.grad = None
    return c


def parameters(dec):
    """state_dict order."""
    return [p for _, p in dec.named_parameters()]


def attention(qkv, heads, key_mask=None):
    """softmax(Q K^T * scale with masked_fill(mask == 0, -1e9)) V as the reference writes it: qkv [B,N,3H],
    key_mask [B,N] (True / non-zero = attend) -> [B,N,H]."""
    B, N, H3 = qkv.shape
    H = H3 // 3
    hd = H // heads
    q, k, v = (t.reshape(B, N, heads, hd).transpose(1, 2) for t in qkv.split(H, dim=-1))
    scores = torch.matmul(q, k.transpose(-2, -1)) * (1.0 / hd ** 0.5)
    if key_mask is not None:
        scores = scores.masked_fill(key_mask.reshape(B, 1, 1, N) == 0, -1e9)
    out = torch.matmul(torch.softmax(scores, dim=-1), v)
    return out.transpose(1, 2).reshape(B, N, H)


def forward(dec, x, positive=None):
    """(mel, the ReLU pre-activations per layer).  positive[l] (bool [B,T,2H], or None: the copy's own
    sign) says where layer l's ReLU passes its input."""
    pre = []
    for l, layer in enumerate(dec.layers):
        a = layer.self_attn
        att = attention(a.qkv(layer.norm1(x)), a.num_heads)
        x = x + a.out_proj(att)
        u = layer.ffn.linear1(layer.norm2(x))
        pos = (u.detach() > 0) if positive is None else positive[l]
        x = x + layer.ffn.linear2(u * pos.to(u.dtype))
        pre.append(u)
    return dec.mel_projection(dec.norm(x)), pre


def gradients(dec, x, d_mel, positive=None):
    """(the 11 layers + 4 gradients in state_dict order, d_x, mel, pre-activations) of sum(mel * d_mel)."""
    x = x.detach().clone().requires_grad_(True)
    mel, pre = forward(dec, x, positive)
    grads = torch.autograd.grad(mel, parameters(dec) + [x], d_mel)
    return list(grads[:-1]), grads[-1], mel.detach(), [u.detach() for u in pre]


def plain_gradients(dec, x, d_mel):
    """The same through torch.relu and the nn modules alone."""
    x = x.detach().clone().requires_grad_(True)
    h = x
    for layer in dec.layers:
        a = layer.self_attn
        h = h + a.out_proj(attention(a.qkv(layer.norm1(h)), a.num_heads))
        h = h + layer.ffn.linear2(torch.relu(layer.ffn.linear1(layer.norm2(h))))
    mel = dec.mel_projection(dec.norm(h))
    grads = torch.autograd.grad(mel, parameters(dec) + [x], d_mel)
    return list(grads[:-1]), grads[-1], mel.detach()
