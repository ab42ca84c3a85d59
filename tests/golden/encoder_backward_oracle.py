"""Float64 oracle of TextEncoder's gradients and of the length regulator's
adjoint (pure torch on the CPU).

Shared by test_encoder_backward_host.py and test_gpu_encoder_backward.py.  As
decoder_backward_oracle.py, whose attention it imports: the module's own
nn.Embedding / nn.Linear / nn.LayerNorm layers are deep-copied to the CPU and
differentiated by torch autograd, and every ReLU is a product with a constant
0/1 mask, so that the side of each kink can be prescribed.  The regulator is
index arithmetic: frame t of utterance b reads phoneme
searchsorted(cum[b, 1:], t, right=True) and is zero at or past cum[b, S].

The cases (V, H, layers, heads, B, S, lengths): ids are uniform in [0, V) and
d_out is N(0, 1) on every row, padded rows included: padded query rows do
carry gradient.  The linear and embedding weights are the module's own init
under torch.manual_seed(seed); LayerNorm weights are set N(1, 0.2), LayerNorm
biases N(0, 0.2) and linear biases N(0, 0.1), so no gradient is tested against
a degenerate parameter.
"""
import copy

import torch

from decoder_backward_oracle import attention  # noqa: F401  (the tests use it too)

CASES = {
    "s1": (256, 64, 2, 2, 2, 7, (7, 4)),          # the stage1 encoder at a few phonemes
    "s2": (256, 96, 3, 2, 1, 5, None),            # the stage2 encoder: head_dim 48, no mask
    "thin": (5, 32, 1, 2, 3, 1, (1, 1, 0)),       # head_dim 16, S = 1, a small phoneme set
    "tiles": (40, 64, 2, 2, 2, 130, (130, 67)),   # 260 rows: five 64-row tiles; every id repeated
    "odd": (300, 96, 1, 2, 1, 67, (33,)),         # most rows of the table never occur
    "wide": (256, 128, 1, 2, 1, 65, None),        # head_dim 64, ffn 256 (the limit)
    "heads4": (256, 64, 1, 4, 3, 33, (33, 16, 0)),  # four heads, one fully masked utterance
}
# Seeds at which CPU float32 and float64 agree on the side of every ReLU kink
# (test_encoder_backward_host.py asserts it).
SEEDS = {"s1": 0, "s2": 1, "thin": 2, "tiles": 66, "odd": 4, "wide": 5, "heads4": 6}
LAYER_PARAMS = 11


def make_encoder(case):
    """The stand-alone TextEncoder of a case (on the CPU, float32)."""
    from models.tts_model import TextEncoder
    V, H, layers, heads = CASES[case][:4]
    seed = SEEDS[case]
    torch.manual_seed(seed)
    enc = TextEncoder(vocab_size=V, hidden_dim=H, num_layers=layers, num_heads=heads)
    g = torch.Generator().manual_seed(1000 + seed)
    norms = {id(m) for m in enc.modules() if isinstance(m, torch.nn.LayerNorm)}
    with torch.no_grad():
        for mod in enc.modules():
            for name, p in mod.named_parameters(recurse=False):
                if id(mod) in norms:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.2 + (1.0 if name == "weight" else 0.0))
                elif name == "bias":
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return enc


def make_inputs(case):
    """(ids int64 [B,S], lengths int64 [B] or None, d_out [B,S,H] float32)."""
    V, H, _, _, B, S, lengths = CASES[case]
    g = torch.Generator().manual_seed(2000 + SEEDS[case])
    ids = torch.randint(0, V, (B, S), generator=g)
    d_out = torch.randn(B, S, H, generator=g)
    return ids, (None if lengths is None else torch.tensor(lengths, dtype=torch.int64)), d_out


def key_mask(lengths, S):
    """mask[b, s] = s < lengths[b] (create_padding_mask), or None."""
    return None if lengths is None else torch.arange(S)[None, :] < lengths[:, None]


def cpu_copy(enc, dtype):
    """`enc` deep-copied to the CPU in `dtype`, every parameter a leaf that requires grad."""
    c = copy.deepcopy(enc).to("cpu", dtype)
    for p in c.parameters():
        p.requires_grad_(True)
        p.grad = None
    return c


def parameters(enc):
    """parameters() order: embedding.weight, 11 per layer, norm.weight, norm.bias."""
    return [p for _, p in enc.named_parameters()]


def forward(enc, ids, lengths, positive=None):
    """(out, the ReLU pre-activations per layer, x0).  positive[l] (bool [B,S,2H], or None: the copy's own
    sign) says where layer l's ReLU passes its input."""
    S = ids.shape[1]
    mask = key_mask(lengths, S)
    x0 = enc.embedding(ids) * enc.hidden_dim ** 0.5 + enc.pos_encoding.pe[:, :S]
    x, pre = x0, []
    for l, layer in enumerate(enc.layers):
        a = layer.self_attn
        x = x + a.out_proj(attention(a.qkv(layer.norm1(x)), a.num_heads, mask))
        u = layer.ffn.linear1(layer.norm2(x))
        pos = (u.detach() > 0) if positive is None else positive[l]
        x = x + layer.ffn.linear2(u * pos.to(u.dtype))
        pre.append(u)
    return enc.norm(x), pre, x0


def gradients(enc, ids, lengths, d_out, positive=None):
    """(the 1 + 11 layers + 2 gradients in parameters() order, out, pre-activations) of sum(out * d_out)."""
    out, pre, _ = forward(enc, ids, lengths, positive)
    grads = torch.autograd.grad(out, parameters(enc), d_out)
    return list(grads), out.detach(), [u.detach() for u in pre]


def plain_gradients(enc, ids, lengths, d_out):
    """The same through torch.relu and the nn modules alone."""
    S = ids.shape[1]
    mask = key_mask(lengths, S)
    h = enc.embedding(ids) * enc.hidden_dim ** 0.5 + enc.pos_encoding.pe[:, :S]
    for layer in enc.layers:
        a = layer.self_attn
        h = h + a.out_proj(attention(a.qkv(layer.norm1(h)), a.num_heads, mask))
        h = h + layer.ffn.linear2(torch.relu(layer.ffn.linear1(layer.norm2(h))))
    out = enc.norm(h)
    return list(torch.autograd.grad(out, parameters(enc), d_out)), out.detach()


# ---- the length regulator ----------------------------------------------------------

def frame_counts(durations):
    """cum int64 [B, S + 1]: the exclusive prefix sums of int(d) per phoneme, as the reference counts frames:
    truncation toward zero, nothing below one frame."""
    if durations.is_floating_point():
        frames = torch.where(durations >= 1, torch.trunc(durations), torch.zeros((), dtype=durations.dtype))
        frames = frames.to(torch.int64)
    else:
        frames = durations.to(torch.int64).clamp(min=0)
    B = durations.shape[0]
    return torch.cat([torch.zeros(B, 1, dtype=torch.int64), torch.cumsum(frames, dim=1)], dim=1)


def frame_sources(cum, T_out):
    """(src int64 [B, T_out], live bool [B, T_out]): frame t of utterance b reads phoneme
    searchsorted(cum[b, 1:], t, right=True) and is zero (not live) at or past cum[b, S]."""
    B, S1 = cum.shape
    t = torch.arange(T_out, dtype=torch.int64)[None, :].expand(B, T_out).contiguous()
    src = torch.searchsorted(cum[:, 1:].contiguous(), t, right=True)
    live = t < cum[:, -1:]
    return src.clamp(max=max(S1 - 2, 0)), live


def output_length(cum, max_length=None):
    """max_length, or the batch's longest utterance (an utterance without frames is one zero frame)."""
    return int(max_length) if max_length is not None else max(1, int(cum[:, -1].max()))


def regulate(enc, cum, T_out):
    """[B,S,H] -> [B,T_out,H] by that index arithmetic (differentiable in enc)."""
    src, live = frame_sources(cum, T_out)
    H = enc.shape[2]
    if enc.shape[1] == 0:
        return enc.new_zeros(enc.shape[0], T_out, H)
    out = torch.gather(enc, 1, src[:, :, None].expand(-1, -1, H))
    return out * live[:, :, None].to(enc.dtype)


def regulate_adjoint(d_reg, cum, S):
    """d_enc [B,S,H] as a segment sum: phoneme s receives the frames cum[b,s] <= t < min(cum[b,s+1], T_out)."""
    B, T_out, H = d_reg.shape
    d_enc = d_reg.new_zeros(B, S, H)
    for b in range(B):
        for s in range(S):
            lo, hi = int(cum[b, s]), min(int(cum[b, s + 1]), T_out)
            if hi > lo:
                d_enc[b, s] = d_reg[b, lo:hi].sum(0)
    return d_enc
