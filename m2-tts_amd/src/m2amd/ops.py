"""Tensor-level wrappers of the C-ABI kernels (one function per entry point).

Every function takes torch tensors that live on a ROCm device, allocates its
outputs with torch (caching allocator), and launches on the current torch
stream.  Nothing here computes on the CPU: a CPU tensor is an error.
"""
from __future__ import annotations

import ctypes
import math
import weakref
from typing import Optional

import torch

from . import _lib
from ._lib import ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SOFTPLUS, ACT_TANH, M2Error  # noqa: F401

Tensor = torch.Tensor


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def require_device(*tensors: Optional[Tensor], what: str = "m2-tts_amd"):
    """Fail loudly on CPU tensors: the product path has no CPU fallback."""
    for t in tensors:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError(
                f"{what}: tensors must be on a ROCm GPU device (got {t.device}); move the module "
                f"and its inputs with .to('cuda').  m2-tts_amd has no CPU execution path.")


def f32c(t: Tensor) -> Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"m2-tts_amd computes in fp32; got {t.dtype}")
    return t.contiguous()


def _shape(t: Tensor) -> tuple:
    return tuple(t.shape)


def _vec(t: Optional[Tensor], n: int, what: str) -> Optional[Tensor]:
    """A per-channel vector as contiguous float32 [n] (None stays None)."""
    if t is None:
        return None
    t = f32c(t)
    if _shape(t) != (n,):
        raise RuntimeError(f"{what} must be [{n}], got {_shape(t)}")
    return t


def _like(t: Optional[Tensor], shape: tuple, what: str) -> Optional[Tensor]:
    """A tensor of the output's shape as contiguous float32 (None stays None)."""
    if t is None:
        return None
    t = f32c(t)
    if _shape(t) != tuple(shape):
        raise RuntimeError(f"{what} must be {tuple(shape)}, got {_shape(t)}")
    return t


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, *, ln: Optional[tuple] = None,
           act: int = ACT_NONE, residual: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """y = act(LN?(x) @ W^T + b) (+ residual) over the last dim (nn.Linear layout W [N, K])."""
    g, b_ = (ln if ln is not None else (None, None))
    require_device(x, weight, bias, g, b_, residual, out, what="linear")
    x, weight = f32c(x), f32c(weight)
    K = x.shape[-1]
    if weight.dim() != 2 or weight.shape[1] != K:
        raise RuntimeError(f"linear: weight {_shape(weight)} does not fit x {_shape(x)}: it must be [N, {K}]")
    N = weight.shape[0]
    R = x.numel() // K if K else 0
    shape = (*x.shape[:-1], N)
    bias = _vec(bias, N, "linear: bias")
    g, b_ = _vec(g, K, "linear: the LayerNorm weight"), _vec(b_, K, "linear: the LayerNorm bias")
    res = _like(residual, shape, "linear: residual")
    if out is not None and (_like(out, shape, "linear: out") is not out):
        raise RuntimeError(f"linear: out {_shape(out)} must be contiguous, got strides {out.stride()}")
    y = out if out is not None else torch.empty(shape, device=x.device, dtype=torch.float32)
    if y.numel() == 0:
        return y
    _lib.call("m2_linear", _ptr(x), _ptr(g), _ptr(b_), _ptr(weight), _ptr(bias), _ptr(res), act,
              R, K, N, _ptr(y), stream_handle(x.device))
    return y


def layer_norm(x: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    require_device(x, weight, bias, what="layer_norm")
    x = f32c(x)
    K = x.shape[-1]
    weight, bias = _vec(weight, K, "layer_norm: weight"), _vec(bias, K, "layer_norm: bias")
    y = torch.empty_like(x)
    if y.numel() == 0:
        return y
    _lib.call("m2_layer_norm", _ptr(x), _ptr(weight), _ptr(bias), x.numel() // K if K else 0, K, _ptr(y),
              stream_handle(x.device))
    return y


def attention_core(qkv: Tensor, heads: int, key_mask: Optional[Tensor]) -> Tensor:
    """softmax(QK^T/sqrt(hd) with -1e9 key mask) V for qkv [B,N,3H] -> [B,N,H]."""
    require_device(qkv, key_mask, what="attention")
    qkv = f32c(qkv)
    if qkv.dim() != 3 or qkv.shape[-1] % 3 != 0:
        raise RuntimeError(f"attention: qkv must be [B, N, 3H], got {_shape(qkv)}")
    B, N, H3 = qkv.shape
    H = H3 // 3
    m = None
    if key_mask is not None:
        if _shape(key_mask) != (B, N):
            raise RuntimeError(f"attention: the key mask must be {(B, N)}, got {_shape(key_mask)}")
        m = key_mask.to(torch.uint8).contiguous() if key_mask.dtype != torch.bool else key_mask.contiguous()
    out = torch.empty(B, N, H, device=qkv.device, dtype=torch.float32)
    if out.numel() == 0:
        return out
    _lib.call("m2_attention", _ptr(qkv), _ptr(m), B, N, H, heads, _ptr(out), stream_handle(qkv.device))
    return out


def conv1d(x: Tensor, weight: Tensor, bias: Tensor, *, act: int = ACT_NONE,
           affine: Optional[tuple] = None, residual: Optional[Tensor] = None, dilation: int = 1,
           padding: Optional[int] = None) -> Tensor:
    """Conv1d(k, dilation, zero padding (default k//2)) [+ per-channel affine]
    [+ act] [+ residual], x [B,Cin,L] -> [B,Cout,L + 2 pad - dil (k - 1)].
    Order: affine, then act, then the residual add.
    k = 1 | 3 with dilation 1 and padding k//2 run the tiled kernel
    (m2_conv1d); every other geometry the general one (m2_conv1d_ex)."""
    al, be = affine if affine is not None else (None, None)
    require_device(x, weight, bias, al, be, residual, what="conv1d")
    x, weight = f32c(x), f32c(weight)
    if x.dim() != 3 or weight.dim() != 3 or weight.shape[1] != x.shape[1]:
        raise RuntimeError(f"conv1d: weight {_shape(weight)} does not fit x {_shape(x)}: x must be [B, Cin, L] "
                           f"and weight [Cout, Cin, k]")
    B, Cin, L = x.shape
    Cout, _, K = weight.shape
    pad = K // 2 if padding is None else int(padding)
    Lo = L + 2 * pad - dilation * (K - 1)
    if residual is not None and Lo != L:
        raise RuntimeError(f"conv1d: output length {Lo} != input length {L}: the residual add has mismatched shapes")
    if Lo < 0:
        raise RuntimeError(f"conv1d: x {_shape(x)} is shorter than the kernel (k {K}, dilation {dilation}, "
                           f"padding {pad}): output length {Lo}")
    bias = _vec(bias, Cout, "conv1d: bias")
    al, be = _vec(al, Cout, "conv1d: the affine scale"), _vec(be, Cout, "conv1d: the affine shift")
    res = _like(residual, (B, Cout, Lo), "conv1d: residual")
    y = torch.empty(B, Cout, Lo, device=x.device, dtype=torch.float32)
    if y.numel() == 0:
        return y
    if K in (1, 3) and dilation == 1 and pad == K // 2:
        _lib.call("m2_conv1d", _ptr(x), _ptr(weight), _ptr(bias), _ptr(al), _ptr(be), _ptr(res), K, act,
                  B, Cin, Cout, L, _ptr(y), stream_handle(x.device))
    else:
        _lib.call("m2_conv1d_ex", _ptr(x), _ptr(weight), _ptr(bias), _ptr(al), _ptr(be), _ptr(res), K,
                  int(dilation), pad, act, B, Cin, Cout, L, _ptr(y), stream_handle(x.device))
    return y


def conv_transpose1d(x: Tensor, weight: Tensor, bias: Tensor, rate: int, *, act: int = ACT_NONE) -> Tensor:
    """ConvTranspose1d(k=2r, stride=r, padding=r/2) [+ act]; weight [Cin, Cout, 2r]."""
    require_device(x, weight, bias, what="conv_transpose1d")
    x, weight = f32c(x), f32c(weight)
    rate = int(rate)
    if x.dim() != 3 or weight.dim() != 3 or weight.shape[0] != x.shape[1] or weight.shape[2] != 2 * rate:
        raise RuntimeError(f"conv_transpose1d: weight {_shape(weight)} does not fit x {_shape(x)} at rate {rate}: "
                           f"x must be [B, Cin, L] and weight [Cin, Cout, {2 * rate}]")
    B, Cin, L = x.shape
    Cout = weight.shape[1]
    bias = _vec(bias, Cout, "conv_transpose1d: bias")
    y = torch.empty(B, Cout, L * rate, device=x.device, dtype=torch.float32)
    if y.numel() == 0:
        return y
    _lib.call("m2_conv_transpose1d", _ptr(x), _ptr(weight), _ptr(bias), rate, act, B, Cin, Cout, L,
              _ptr(y), stream_handle(x.device))
    return y


def conv1d_strided(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, *, stride: int = 1, padding: int = 0,
                   groups: int = 1, leaky_slope: float = 1.0) -> Tensor:
    """leaky(F.conv1d(x, weight [Cout, Cin/groups, k], bias, stride, padding, groups=groups), slope)
    (m2_conv1d_strided; slope 1.0: no activation), x [B,Cin,L] -> [B,Cout,(L + 2 padding - k)//stride + 1]."""
    require_device(x, weight, bias, what="conv1d_strided")
    x = f32c(x)
    B, Cin, L = x.shape
    Cout, Cg, K = weight.shape
    if groups < 1 or Cin % groups or Cout % groups or Cg * groups != Cin:
        raise ValueError(f"conv1d_strided: weight {tuple(weight.shape)} and groups {groups} do not fit x {tuple(x.shape)}")
    Lo = (L + 2 * padding - K) // stride + 1
    y = torch.empty(B, Cout, max(Lo, 0), device=x.device, dtype=torch.float32)
    _lib.call("m2_conv1d_strided", _ptr(x), _ptr(f32c(weight)), None if bias is None else _ptr(f32c(bias)), K,
              int(stride), int(padding), int(groups), float(leaky_slope), B, Cin, Cout, L, _ptr(y),
              stream_handle(x.device))
    return y


def conv1d_strided_backward(x_pre: Tensor, weight: Tensor, dy: Tensor, *, stride: int = 1, padding: int = 0,
                            groups: int = 1, in_slope: float = 1.0, need_dx: bool = True, need_db: bool = True):
    """The gradients of y = F.conv1d(F.leaky_relu(x_pre, in_slope), weight, bias, stride, padding, groups=groups)
    given dy, the cotangent of y (m2_conv1d_strided_backward): (dx [B,Cin,L] or None, dw like weight, db [Cout]
    or None), dw and db summed over the batch."""
    require_device(x_pre, weight, dy, what="conv1d_strided_backward")
    x_pre, dy, weight = f32c(x_pre), f32c(dy), f32c(weight)
    B, Cin, L = x_pre.shape
    Cout, Cg, K = weight.shape
    if groups < 1 or Cin % groups or Cout % groups or Cg * groups != Cin:
        raise ValueError(f"conv1d_strided_backward: weight {tuple(weight.shape)} and groups {groups} do not fit "
                         f"x_pre {tuple(x_pre.shape)}")
    Lo = (L + 2 * padding - K) // stride + 1
    if tuple(dy.shape) != (B, Cout, Lo):
        raise ValueError(f"conv1d_strided_backward: dy {tuple(dy.shape)} must be {(B, Cout, Lo)}")
    dev = x_pre.device
    dx = torch.empty_like(x_pre) if need_dx else None
    dw = torch.empty_like(weight)
    db = torch.empty(Cout, device=dev, dtype=torch.float32) if need_db else None
    geo = (K, int(stride), int(padding), int(groups))
    need = int(_lib.load().m2_conv1d_strided_backward_workspace_bytes(*geo, B, Cin, Cout, L))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    _lib.call("m2_conv1d_strided_backward", _ptr(x_pre), _ptr(weight), _ptr(dy), *geo, float(in_slope), B, Cin, Cout, L,
              _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws), ws.numel(), stream_handle(dev))
    return dx, dw, db


def conv1d_audio_backward(dy: Tensor, weight: Tensor, L: int, *, padding: int = 0, pool: int = 1,
                          out: Optional[Tensor] = None) -> Tensor:
    """The gradient of y = F.conv1d(F.avg_pool1d(x, pool), weight [Cout,1,k], padding=padding) with respect to
    x [B,1,L], given dy [B,Cout,L//pool + 2 padding - k + 1] (m2_conv1d_audio_backward).  Without ``out`` a new
    [B,1,L] tensor is written, the samples floor pooling dropped with 0; with ``out`` the gradient is added to
    it and those samples are left alone."""
    require_device(dy, weight, out, what="conv1d_audio_backward")
    dy, weight = f32c(dy), f32c(weight)
    B, Cout, Lo = dy.shape
    K, L, pool, padding = weight.shape[2], int(L), int(pool), int(padding)
    if tuple(weight.shape) != (Cout, 1, K) or pool < 1 or Lo != L // pool + 2 * padding - K + 1:
        raise ValueError(f"conv1d_audio_backward: dy {tuple(dy.shape)} and weight {tuple(weight.shape)} do not fit "
                         f"{L} samples, pool {pool}, padding {padding}")
    if out is None:
        dx = torch.empty(B, 1, L, device=dy.device, dtype=torch.float32)
    else:
        dx = out
        if tuple(dx.shape) != (B, 1, L) or dx.dtype != torch.float32 or not dx.is_contiguous():
            raise ValueError(f"conv1d_audio_backward: out must be contiguous float32 {(B, 1, L)}")
    _lib.call("m2_conv1d_audio_backward", _ptr(dy), _ptr(weight), K, padding, pool, B, Cout, L,
              0 if out is None else 1, _ptr(dx), stream_handle(dy.device))
    return dx


def avg_pool1d(x: Tensor, kernel_size: int) -> Tensor:
    """F.avg_pool1d(x [B,C,L], k, stride=k) -> [B,C,L//k] (m2_avg_pool1d)."""
    require_device(x, what="avg_pool1d")
    x = f32c(x)
    B, C, L = x.shape
    y = torch.empty(B, C, L // kernel_size, device=x.device, dtype=torch.float32)
    _lib.call("m2_avg_pool1d", _ptr(x), int(kernel_size), B, C, L, _ptr(y), stream_handle(x.device))
    return y


class Discriminators:
    """The packed discriminators of one MultiScaleDiscriminator on one device
    (m2_disc_*): ``tensors`` are its state_dict values in order (weight, bias
    of the seven convs of every scale)."""

    LAYERS = 7
    # Cin, Cout, k, stride, padding, groups (losses.py:69-91)
    LAYER_TABLE = ((1, 64, 15, 1, 7, 1), (64, 128, 41, 4, 20, 4), (128, 256, 41, 4, 20, 16), (256, 512, 41, 4, 20, 64),
                   (512, 1024, 41, 4, 20, 256), (1024, 1024, 5, 1, 2, 1), (1024, 1, 3, 1, 1, 1))

    def __init__(self, tensors, scales, device: torch.device):
        lib = _lib.load()
        self.device = torch.device(device)
        self.scales = [int(s) for s in scales]
        keep = []
        for t in tensors:
            require_device(t, what="discriminator weight")
            keep.append(f32c(t.detach()))
        ptrs = (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
        sc = (ctypes.c_int32 * len(self.scales))(*self.scales)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.m2_disc_create(ptrs, len(keep), sc, len(self.scales), stream_handle(self.device),
                                          ctypes.byref(h)), "m2_disc_create")
        self.handle = h
        self._finalizer = weakref.finalize(self, lib.m2_disc_destroy, h)

    def set_slice_bytes(self, nbytes: int):
        """Bound the activations one batch slice of forward / losses may take (0: the default, 1 GiB)."""
        _lib.call("m2_disc_set_slice_bytes", self.handle, int(nbytes))

    def shapes(self, L: int):
        """[(channels, length)] of the seven layers of every scale for audio of L samples."""
        lib = _lib.load()
        c, n = ctypes.c_int32(), ctypes.c_int32()
        out = []
        for s in range(len(self.scales)):
            row = []
            for layer in range(self.LAYERS):
                _lib.check(lib.m2_disc_layer_shape(self.handle, L, s, layer, ctypes.byref(c), ctypes.byref(n)),
                           "m2_disc_layer_shape")
                row.append((c.value, n.value))
            out.append(row)
        return out

    def layer(self, scale_index: int, layer: int, x: Tensor) -> Tensor:
        """One packed layer (m2_disc_layer): x [B,Cin,L], the previous layer's output (the
        LeakyReLU(0.2) between them is applied here) or the pooled audio -> [B,Cout,len]."""
        require_device(x, what="discriminator")
        x = f32c(x)
        B, _, L = x.shape
        c = self.LAYER_TABLE[layer]
        if x.shape[1] != c[0]:
            raise ValueError(f"discriminator layer {layer}: {c[0]} input channels, got {x.shape[1]}")
        n = (L + 2 * c[4] - c[2]) // c[3] + 1
        y = torch.empty(B, c[1], n, device=x.device, dtype=torch.float32)
        _lib.call("m2_disc_layer", self.handle, int(scale_index), int(layer), _ptr(x), B, L, _ptr(y),
                  stream_handle(x.device))
        return y

    def _audio(self, x: Tensor) -> Tensor:
        require_device(x, what="discriminator")
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError(f"discriminator: audio must be [B, 1, L], got {tuple(x.shape)}")
        return f32c(x.detach().float())

    def forward(self, x: Tensor, features: bool = True):
        """x [B,1,L] -> (logits per scale, the six feature maps per scale or None)."""
        x = self._audio(x)
        B, _, L = x.shape
        shapes = self.shapes(L)
        logits = torch.empty(B * sum(row[-1][1] for row in shapes), device=x.device, dtype=torch.float32)
        feats = None
        if features:
            feats = torch.empty(B * sum(c * n for row in shapes for c, n in row[:-1]), device=x.device,
                                dtype=torch.float32)
        need = int(_lib.load().m2_disc_forward_workspace_bytes(self.handle, B, L))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
        _lib.call("m2_disc_forward", self.handle, _ptr(x), B, L, _ptr(logits), _ptr(feats), _ptr(ws), ws.numel(),
                  stream_handle(x.device))
        outs, maps, lo, fo = [], [], 0, 0
        for row in shapes:
            n = row[-1][1]
            outs.append(logits[lo:lo + B * n].view(B, 1, n))
            lo += B * n
            if features:
                m = []
                for c, n in row[:-1]:
                    m.append(feats[fo:fo + B * c * n].view(B, c, n))
                    fo += B * c * n
                maps.append(m)
        return outs, (maps if features else None)

    def _pair(self, real: Optional[Tensor], fake: Optional[Tensor], need_real=False, need_fake=False):
        """real and fake as [B,1,L] float32 of one shape; one that is not needed may be None."""
        real = self._audio(real) if need_real or real is not None else None
        fake = self._audio(fake) if need_fake or fake is not None else None
        if real is not None and fake is not None and real.shape != fake.shape:
            raise ValueError(f"discriminator: real {tuple(real.shape)} and fake {tuple(fake.shape)} differ")
        return real, fake

    def _rows_call(self, name: str, real: Optional[Tensor], fake: Optional[Tensor], before=(), after=()) -> Tensor:
        """m2_disc_<name>(handle, real, fake, B, L, *before, rows, *after, workspace, bytes, stream) with zeroed
        float64 rows [B, K] and the workspace the call asks for; returns the rows."""
        ref = fake if fake is not None else real
        B, _, L = ref.shape
        lib = _lib.load()
        out = torch.zeros(B, lib.m2_loss_column_count(1), device=ref.device, dtype=torch.float64)
        need = int(getattr(lib, f"m2_disc_{name}_workspace_bytes")(self.handle, B, L))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=ref.device)
        _lib.call(f"m2_disc_{name}", self.handle, _ptr(real), _ptr(fake), B, L, *before, _ptr(out), *after, _ptr(ws),
                  ws.numel(), stream_handle(ref.device))
        return out

    def losses(self, real: Optional[Tensor], fake: Optional[Tensor]) -> Tensor:
        """The logit and feature-matching sums of real and/or fake [B,1,L] ->
        float64 [B, K] on the device, columns ``dsp.loss_columns("disc")``."""
        real, fake = self._pair(real, fake)
        return self._rows_call("losses", real, fake)

    def step(self, real: Tensor, fake: Tensor):
        """The discriminator step (m2_disc_step): ``losses(real, fake)``'s rows, bit for bit, and the
        gradient of L_D = mean over scales of [mean (D(real) - 1)^2 + mean D(fake)^2] with respect to
        every weight and bias: new float32 tensors in state_dict order, shaped like the parameters."""
        real, fake = self._pair(real, fake, need_real=True, need_fake=True)
        dev = real.device
        grads = []
        for _ in self.scales:
            for cin, cout, k, _, _, groups in self.LAYER_TABLE:
                grads.append(torch.zeros(cout, cin // groups, k, device=dev, dtype=torch.float32))
                grads.append(torch.zeros(cout, device=dev, dtype=torch.float32))
        ptrs = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
        return self._rows_call("step", real, fake, after=(ptrs,)), grads

    def gen_step(self, real: Optional[Tensor], fake: Tensor, w_adv: float, w_fm: float):
        """The generator step through the discriminators (m2_disc_gen_step): ``losses(real, fake)``'s rows,
        bit for bit, and d_fake [B,1,L] float32, the gradient of w_adv * generator loss + w_fm *
        feature-matching loss with respect to ``fake``.  ``real`` may be None only when ``w_fm == 0``: the
        rows are ``losses(None, fake)``'s then."""
        w_adv, w_fm = float(w_adv), float(w_fm)
        if real is None and w_fm != 0.0:
            raise ValueError("discriminator: gen_step needs real for the feature-matching term")
        real, fake = self._pair(real, fake, need_fake=True)
        d_fake = torch.empty_like(fake)
        return self._rows_call("gen_step", real, fake, (w_adv, w_fm), (_ptr(d_fake),)), d_fake


VOCODER_PARAMS = 28
VOCODER_TAPE_NAMES = ("h",) + tuple(f"{n}{k + (n == 'x')}" for k in range(4) for n in ("a", "lv", "x")) + ("y",)


def _vocoder_params(params):
    """The 28 SimpleVocoder parameters (state_dict order) as contiguous float32 device tensors, their
    pointer array, and (M, C)."""
    keep = [f32c(p.detach()) for p in params]
    if len(keep) != VOCODER_PARAMS:
        raise ValueError(f"vocoder: {VOCODER_PARAMS} parameters in state_dict order, got {len(keep)}")
    require_device(*keep, what="vocoder parameter")
    C, M, K = keep[0].shape
    if K != 3:
        raise NotImplementedError(f"vocoder backward: kernel size 3 only, got {K}")
    return keep, (ctypes.c_void_p * VOCODER_PARAMS)(*[t.data_ptr() for t in keep]), int(M), int(C)


def _vocoder_mel(mel: Tensor, M: int) -> Tensor:
    require_device(mel, what="vocoder")
    if mel.dim() != 3 or mel.shape[1] != M:
        raise ValueError(f"vocoder: mel must be [B, {M}, T], got {tuple(mel.shape)}")
    return f32c(mel.detach())


def vocoder_train_forward(params, mel: Tensor):
    """SimpleVocoder's forward from its 28 raw parameters, keeping a tape (m2_vocoder_train_forward):
    (audio [B,1,64T], bit-equal to the stand-alone module's forward, and the tape, a uint8 tensor that
    ``vocoder_tape_maps`` names and ``vocoder_backward`` reads)."""
    keep, ptrs, M, C = _vocoder_params(params)
    mel = _vocoder_mel(mel, M)
    B, _, T = mel.shape
    dev = mel.device
    lib = _lib.load()
    need = int(lib.m2_vocoder_tape_bytes(M, C, B, T))
    if need == 0:
        raise M2Error(f"vocoder_train_forward: unsupported shape M={M} C={C} B={B} T={T}")
    tape = torch.empty(need, dtype=torch.uint8, device=dev)
    audio = torch.empty(B, 1, 64 * T, device=dev, dtype=torch.float32)
    _lib.call("m2_vocoder_train_forward", ptrs, M, C, _ptr(mel), B, T, _ptr(audio), _ptr(tape), tape.numel(),
              stream_handle(dev))
    return audio, tape


def vocoder_tape_maps(tape: Tensor, M: int, C: int, B: int, T: int) -> dict:
    """The maps of a tape as named float32 views [B, channels, length] (m2_vocoder_tape_map): h, then per
    stage k a<k> = leaky(ConvT_k(x_k)), lv<k> = leaky(conv1_k(a_k)), x<k+1> = conv2_k(lv_k) + a_k, and y."""
    lib = _lib.load()
    flat = tape.view(torch.float32) if tape.numel() % 4 == 0 else tape[:tape.numel() // 4 * 4].view(torch.float32)
    off, ch, n = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
    out = {}
    for i, name in enumerate(VOCODER_TAPE_NAMES):
        _lib.check(lib.m2_vocoder_tape_map(M, C, B, T, i, ctypes.byref(off), ctypes.byref(ch), ctypes.byref(n)),
                   "m2_vocoder_tape_map")
        out[name] = flat[off.value:off.value + B * ch.value * n.value].view(B, ch.value, n.value)
    return out


def vocoder_backward(params, mel: Tensor, tape: Tensor, d_audio: Tensor, need_mel: bool = True, need=None,
                     out=None):
    """The gradients of SimpleVocoder given d_audio [B,1,64T] (m2_vocoder_backward): (d_mel [B,M,T] or None,
    the 28 gradients in state_dict order, None where ``need[i]`` is false).  ``out`` (28 tensors or None
    entries): gradients to add to instead of new tensors."""
    keep, ptrs, M, C = _vocoder_params(params)
    mel = _vocoder_mel(mel, M)
    B, _, T = mel.shape
    dev = mel.device
    require_device(tape, d_audio, what="vocoder_backward")
    d_audio = f32c(d_audio.detach().to(torch.float32))
    if d_audio.numel() != B * 64 * T:
        raise ValueError(f"vocoder_backward: d_audio must be {(B, 1, 64 * T)}, got {tuple(d_audio.shape)}")
    lib = _lib.load()
    if tape.numel() < int(lib.m2_vocoder_tape_bytes(M, C, B, T)):
        raise ValueError("vocoder_backward: the tape is not that of this shape")
    want = [True] * VOCODER_PARAMS if need is None else [bool(n) for n in need]
    grads = []
    for i, (p, w) in enumerate(zip(keep, want)):
        if not w:
            grads.append(None)
        elif out is not None and out[i] is not None:
            grads.append(out[i])
        else:
            grads.append(torch.empty_like(p) if out is None else torch.zeros_like(p))
    gp =(ctypes.c_void_p * VOCODER_PARAMS)(*[_ptr(g) for g in grads])
    d_mel = torch.empty_like(mel) if need_mel else None
    nbytes = int(lib.m2_vocoder_backward_workspace_bytes(M, C, B, T))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.call("m2_vocoder_backward", ptrs, M, C, _ptr(mel), B, T, _ptr(tape), _ptr(d_audio), _ptr(d_mel), gp,
              0 if out is None else 1, _ptr(ws), ws.numel(), stream_handle(dev))
    return d_mel, grads


def vocoder_out_backward(gy: Tensor, y: Tensor, x: Tensor, w: Tensor):
    """(gx, dw, db) of y = tanh(conv1d(x [B,c,L], w [1,c,3], b, padding=1)) given gy (m2_vocoder_out_backward)."""
    require_device(gy, y, x, w, what="vocoder_out_backward")
    gy, y, x, w = f32c(gy), f32c(y), f32c(x), f32c(w)
    B, c, L = x.shape
    gx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty(1, device=x.device, dtype=torch.float32)
    ws = torch.empty(max(int(_lib.load().m2_vocoder_out_backward_workspace_bytes(B, c, L)), 1), dtype=torch.uint8,
                     device=x.device)
    _lib.call("m2_vocoder_out_backward", _ptr(gy), _ptr(y), _ptr(x), _ptr(w), B, c, L, _ptr(gx), _ptr(dw), _ptr(db),
              _ptr(ws), ws.numel(), stream_handle(x.device))
    return gx, dw, db


def resblock_backward(g_r: Tensor, lv: Tensor, a: Tensor, w1: Tensor, w2: Tensor):
    """(g_v, g_u) of x_out = conv2(lv) + a, lv = leaky(conv1(a), 0.1), a = leaky(u, 0.1) given g_r, the
    cotangent of x_out (m2_resblock_backward): the cotangents of conv1's output and of u."""
    require_device(g_r, lv, a, w1, w2, what="resblock_backward")
    g_r, lv, a, w1, w2 = f32c(g_r), f32c(lv), f32c(a), f32c(w1), f32c(w2)
    B, c, L = g_r.shape
    g_v, g_u = torch.empty_like(g_r), torch.empty_like(g_r)
    _lib.call("m2_resblock_backward", _ptr(g_r), _ptr(lv), _ptr(a), _ptr(w1), _ptr(w2), B, c, L, _ptr(g_v), _ptr(g_u),
              stream_handle(g_r.device))
    return g_v, g_u


def conv1d_narrow_dw(x: Tensor, dy: Tensor, ksize: int, *, stride: int = 1, padding: int = 0):
    """(dw [Cout,Cin,k], db [Cout]) of y = conv1d(x, w, b, stride, padding) given dy, for Cout < 16
    (m2_conv1d_narrow_dw)."""
    require_device(x, dy, what="conv1d_narrow_dw")
    x, dy = f32c(x), f32c(dy)
    B, Cin, L = x.shape
    Cout = dy.shape[1]
    geo = (int(ksize), int(stride), int(padding))
    dw = torch.empty(Cout, Cin, ksize, device=x.device, dtype=torch.float32)
    db = torch.empty(Cout, device=x.device, dtype=torch.float32)
    ws = torch.empty(max(int(_lib.load().m2_conv1d_narrow_dw_workspace_bytes(*geo, B, Cin, Cout, L)), 1),
                     dtype=torch.uint8, device=x.device)
    _lib.call("m2_conv1d_narrow_dw", _ptr(x), _ptr(dy), *geo, B, Cin, Cout, L, _ptr(dw), _ptr(db), _ptr(ws),
              ws.numel(), stream_handle(x.device))
    return dw, db


DECODER_LAYER_PARAMS = 11
DECODER_TAIL_PARAMS = 4
DECODER_TAPE_NAMES = ("qkv", "att", "x_mid", "h", "x_out")


def _decoder_params(params, heads: int):
    """MelDecoder's 11 layers + 4 parameters (state_dict order) as contiguous float32 device tensors, their
    pointer array, and the dimensions (H, M, layers, heads)."""
    keep = [f32c(p.detach()) for p in params]
    layers, tail = divmod(len(keep) - DECODER_TAIL_PARAMS, DECODER_LAYER_PARAMS)
    if layers < 1 or tail != 0:
        raise ValueError(f"decoder: 11 layers + 4 parameters in state_dict order, got {len(keep)}")
    require_device(*keep, what="decoder parameter")
    M, H = keep[-2].shape
    return keep, (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep]), (int(H), int(M), layers, int(heads))


def _decoder_x(x: Tensor, H: int) -> Tensor:
    require_device(x, what="decoder")
    if x.dim() != 3 or x.shape[2] != H:
        raise ValueError(f"decoder: x must be [B, T, {H}], got {tuple(x.shape)}")
    return f32c(x.detach())


def decoder_supported(H: int, M: int, layers: int, heads: int) -> bool:
    """Whether m2_decoder_backward takes a MelDecoder of these dimensions (host arithmetic only)."""
    return int(_lib.load().m2_decoder_tape_bytes(H, M, layers, heads, 1, 1)) != 0


def decoder_train_forward(params, x: Tensor, heads: int):
    """MelDecoder's forward from its raw parameters, keeping a tape (m2_decoder_train_forward): (mel [B,T,M],
    bit-equal to the stand-alone module's forward, and the tape, a uint8 tensor that ``decoder_tape_maps``
    names and ``decoder_backward`` reads)."""
    keep, ptrs, dims = _decoder_params(params, heads)
    x = _decoder_x(x, dims[0])
    B, T, _ = x.shape
    dev = x.device
    need = int(_lib.load().m2_decoder_tape_bytes(*dims, B, T))
    if need == 0:
        raise M2Error(f"decoder_train_forward: unsupported shape (H, M, layers, heads) = {dims}, B={B} T={T}")
    tape = torch.empty(need, dtype=torch.uint8, device=dev)
    mel = torch.empty(B, T, dims[1], device=dev, dtype=torch.float32)
    _lib.call("m2_decoder_train_forward", ptrs, *dims, _ptr(x), B, T, _ptr(mel), _ptr(tape), tape.numel(),
              stream_handle(dev))
    return mel, tape


def decoder_tape_maps(tape: Tensor, H: int, M: int, layers: int, heads: int, B: int, T: int) -> list:
    """The maps of a tape as float32 views (m2_decoder_tape_map): one dict per layer with qkv [B,T,3H],
    att [B,T,H], x_mid [B,T,H], h [B,T,2H] (post-ReLU) and x_out [B,T,H]."""
    lib = _lib.load()
    flat = tape[:tape.numel() // 4 * 4].view(torch.float32)
    off, width = ctypes.c_size_t(), ctypes.c_int32()
    out = []
    for layer in range(layers):
        maps = {}
        for i, name in enumerate(DECODER_TAPE_NAMES):
            _lib.check(lib.m2_decoder_tape_map(H, M, layers, heads, B, T, len(DECODER_TAPE_NAMES) * layer + i,
                                               ctypes.byref(off), ctypes.byref(width)), "m2_decoder_tape_map")
            maps[name] = flat[off.value:off.value + B * T * width.value].view(B, T, width.value)
        out.append(maps)
    return out


def decoder_backward(params, x: Tensor, tape: Tensor, d_mel: Tensor, heads: int, need_x: bool = True, need=None,
                     accumulate=False):
    """The gradients of MelDecoder given d_mel [B,T,M] (m2_decoder_backward): (d_x [B,T,H] or None, the
    11 layers + 4 gradients in state_dict order, None where ``need[i]`` is false).  ``accumulate``: a list of
    that many tensors (or None entries) to add the gradients to instead of new tensors."""
    keep, ptrs, dims = _decoder_params(params, heads)
    x = _decoder_x(x, dims[0])
    B, T, _ = x.shape
    dev = x.device
    require_device(tape, d_mel, what="decoder_backward")
    d_mel = f32c(d_mel.detach().to(torch.float32))
    if tuple(d_mel.shape) != (B, T, dims[1]):
        raise ValueError(f"decoder_backward: d_mel must be {(B, T, dims[1])}, got {tuple(d_mel.shape)}")
    lib = _lib.load()
    tape_bytes = int(lib.m2_decoder_tape_bytes(*dims, B, T))
    if tape_bytes == 0:
        raise M2Error(f"decoder_backward: unsupported shape (H, M, layers, heads) = {dims}, B={B} T={T}")
    if tape.numel() < tape_bytes:
        raise ValueError("decoder_backward: the tape is not that of this shape")
    onto = accumulate if accumulate else None
    want = [True] * len(keep) if need is None else [bool(n) for n in need]
    grads = []
    for i, (p, w) in enumerate(zip(keep, want)):
        if not w:
            grads.append(None)
        elif onto is not None and onto[i] is not None:
            grads.append(onto[i])
        else:
            grads.append(torch.empty_like(p) if onto is None else torch.zeros_like(p))
    gp = (ctypes.c_void_p * len(keep))(*[_ptr(g) for g in grads])
    d_x = torch.empty_like(x) if need_x else None
    ws = torch.empty(max(int(lib.m2_decoder_backward_workspace_bytes(*dims, B, T)), 1), dtype=torch.uint8, device=dev)
    _lib.call("m2_decoder_backward", ptrs, *dims, _ptr(x), B, T, _ptr(tape), _ptr(d_mel), _ptr(d_x), gp,
              0 if onto is None else 1, _ptr(ws), ws.numel(), stream_handle(dev))
    return d_x, grads


def _key_mask(key_mask: Optional[Tensor]) -> Optional[Tensor]:
    if key_mask is None:
        return None
    return key_mask.contiguous() if key_mask.dtype == torch.bool else key_mask.to(torch.uint8).contiguous()


def attention_backward(qkv: Tensor, key_mask: Optional[Tensor], att: Tensor, d_att: Tensor, heads: int) -> Tensor:
    """d_qkv [B,N,3H] of att = attention_core(qkv, heads, key_mask) given d_att [B,N,H]
    (m2_attention_backward).  A masked key's dS is 0 by definition."""
    require_device(qkv, att, d_att, key_mask, what="attention_backward")
    qkv, att, d_att = f32c(qkv), f32c(att), f32c(d_att)
    B, N, H3 = qkv.shape
    m = _key_mask(key_mask)
    d_qkv = torch.empty_like(qkv)
    ws = torch.empty(max(int(_lib.load().m2_attention_backward_workspace_bytes(B, N, heads)), 1), dtype=torch.uint8,
                     device=qkv.device)
    _lib.call("m2_attention_backward", _ptr(qkv), _ptr(m), _ptr(att), _ptr(d_att), B, N, H3 // 3, heads, _ptr(d_qkv),
              _ptr(ws), ws.numel(), stream_handle(qkv.device))
    return d_qkv


def linear_backward_input(g_y: Tensor, weight: Tensor, *, relu_of: Optional[Tensor] = None, ln_x: Optional[Tensor] = None,
                          gamma: Optional[Tensor] = None, g_res: Optional[Tensor] = None):
    """g_x = g_y @ W of y = x @ W^T (m2_linear_backward_input), W [N,K] as stored.  ``relu_of``: times
    (relu_of > 0).  ``ln_x`` with ``gamma``: the linear consumed LayerNorm(ln_x) and the result is
    (g_x, dgamma, dbeta), g_x the LayerNorm's input cotangent plus ``g_res``."""
    require_device(g_y, weight, relu_of, ln_x, gamma, g_res, what="linear_backward_input")
    g_y, weight = f32c(g_y), f32c(weight)
    N, K = weight.shape
    R = g_y.numel() // N
    dev = g_y.device
    relu_of, ln_x, gamma, g_res = (None if t is None else f32c(t) for t in (relu_of, ln_x, gamma, g_res))
    g_x = torch.empty(*g_y.shape[:-1], K, device=dev, dtype=torch.float32)
    dg = db = None
    if ln_x is not None:
        dg, db = torch.empty(K, device=dev, dtype=torch.float32), torch.empty(K, device=dev, dtype=torch.float32)
    ws = torch.empty(max(int(_lib.load().m2_linear_backward_input_workspace_bytes(R, K)), 1), dtype=torch.uint8,
                     device=dev)
    _lib.call("m2_linear_backward_input", _ptr(g_y), _ptr(weight), _ptr(relu_of), _ptr(ln_x), _ptr(gamma), _ptr(g_res),
              R, K, N, _ptr(g_x), _ptr(dg), _ptr(db), _ptr(ws), ws.numel(), stream_handle(dev))
    return g_x if ln_x is None else (g_x, dg, db)


def linear_backward_weight(g_y: Tensor, x: Tensor, *, ln: Optional[tuple] = None):
    """(dw [N,K], db [N]) of y = X @ W^T + b given g_y [.., N] (m2_linear_backward_weight); X = x [.., K], or
    LayerNorm(x; *ln) re-formed on the fly."""
    require_device(g_y, x, what="linear_backward_weight")
    g_y, x = f32c(g_y), f32c(x)
    N, K = g_y.shape[-1], x.shape[-1]
    R = x.numel() // K
    dev = x.device
    g, b_ = (None, None) if ln is None else (f32c(ln[0]), f32c(ln[1]))
    dw = torch.empty(N, K, device=dev, dtype=torch.float32)
    db = torch.empty(N, device=dev, dtype=torch.float32)
    ws = torch.empty(max(int(_lib.load().m2_linear_backward_weight_workspace_bytes(R, K, N)), 1), dtype=torch.uint8,
                     device=dev)
    _lib.call("m2_linear_backward_weight", _ptr(g_y), _ptr(x), _ptr(g), _ptr(b_), R, K, N, _ptr(dw), _ptr(db), _ptr(ws),
              ws.numel(), stream_handle(dev))
    return dw, db


ENCODER_LAYER_PARAMS = DECODER_LAYER_PARAMS
ENCODER_TAIL_PARAMS = 2
ENCODER_TAPE_NAMES = DECODER_TAPE_NAMES


def _encoder_params(params, heads: int):
    """TextEncoder's 1 + 11 layers + 2 parameters (parameters() order) as contiguous float32 device tensors,
    their pointer array, and the dimensions (V, H, layers, heads)."""
    keep = [f32c(p.detach()) for p in params]
    layers, tail = divmod(len(keep) - 1 - ENCODER_TAIL_PARAMS, ENCODER_LAYER_PARAMS)
    if layers < 1 or tail != 0:
        raise ValueError(f"encoder: 1 + 11 layers + 2 parameters in parameters() order, got {len(keep)}")
    require_device(*keep, what="encoder parameter")
    V, H = keep[0].shape
    return keep, (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep]), (int(V), int(H), layers, int(heads))


def _encoder_inputs(ids: Tensor, key_mask: Optional[Tensor]):
    require_device(ids, key_mask, what="encoder")
    if ids.dim() != 2:
        raise ValueError(f"encoder: ids must be [B, S], got {tuple(ids.shape)}")
    if key_mask is not None and tuple(key_mask.shape) != tuple(ids.shape):
        raise ValueError(f"encoder: the key mask must be {tuple(ids.shape)}, got {tuple(key_mask.shape)}")
    return ids.to(torch.int64).contiguous(), _key_mask(key_mask)


def encoder_supported(V: int, H: int, layers: int, heads: int) -> bool:
    """Whether m2_encoder_backward takes a TextEncoder of these dimensions (host arithmetic only)."""
    return int(_lib.load().m2_encoder_tape_bytes(V, H, layers, heads, 1, 1)) != 0


def encoder_train_forward(params, ids: Tensor, pe: Tensor, key_mask: Optional[Tensor], heads: int):
    """TextEncoder's forward from its raw parameters, keeping a tape (m2_encoder_train_forward): (out [B,S,H],
    bit-equal to the stand-alone module's forward, and the tape, a uint8 tensor that ``encoder_tape_maps``
    names and ``encoder_backward`` reads).  ``pe``: the positional table's rows [>= S, H]; ``key_mask``
    [B,S] (True / non-zero = attend) or None."""
    keep, ptrs, dims = _encoder_params(params, heads)
    ids, mask = _encoder_inputs(ids, key_mask)
    B, S = ids.shape
    dev = ids.device
    require_device(pe, what="encoder")
    pe = f32c(pe)
    if pe.dim() != 2 or pe.shape[0] < S or pe.shape[1] != dims[1]:
        raise ValueError(f"encoder: the positional table must be [>= {S}, {dims[1]}], got {tuple(pe.shape)}")
    need = int(_lib.load().m2_encoder_tape_bytes(*dims, B, S))
    if need == 0:
        raise M2Error(f"encoder_train_forward: unsupported shape (V, H, layers, heads) = {dims}, B={B} S={S}")
    tape = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(B, S, dims[1], device=dev, dtype=torch.float32)
    _lib.call("m2_encoder_train_forward", ptrs, *dims, _ptr(ids), _ptr(pe), _ptr(mask), B, S, _ptr(out), _ptr(tape),
              tape.numel(), stream_handle(dev))
    return out, tape


def encoder_tape_maps(tape: Tensor, V: int, H: int, layers: int, heads: int, B: int, S: int):
    """The maps of a tape as float32 views (m2_encoder_tape_map): (x0 [B,S,H], the embedding's output, and
    one dict per layer as ``decoder_tape_maps``)."""
    lib = _lib.load()
    flat = tape[:tape.numel() // 4 * 4].view(torch.float32)
    off, width = ctypes.c_size_t(), ctypes.c_int32()

    def view(index):
        _lib.check(lib.m2_encoder_tape_map(V, H, layers, heads, B, S, index, ctypes.byref(off), ctypes.byref(width)),
                   "m2_encoder_tape_map")
        return flat[off.value:off.value + B * S * width.value].view(B, S, width.value)

    n = len(ENCODER_TAPE_NAMES)
    return view(0), [{name: view(1 + n * layer + i) for i, name in enumerate(ENCODER_TAPE_NAMES)}
                     for layer in range(layers)]


def encoder_backward(params, ids: Tensor, key_mask: Optional[Tensor], tape: Tensor, d_out: Tensor, heads: int,
                     need=None, accumulate=False):
    """The gradients of TextEncoder given d_out [B,S,H] (m2_encoder_backward): the 1 + 11 layers + 2
    gradients in parameters() order, None where ``need[i]`` is false.  ``accumulate``: a list of that many
    tensors (or None entries) to add the gradients to instead of new tensors."""
    keep, ptrs, dims = _encoder_params(params, heads)
    ids, mask = _encoder_inputs(ids, key_mask)
    B, S = ids.shape
    dev = ids.device
    require_device(tape, d_out, what="encoder_backward")
    d_out = f32c(d_out.detach().to(torch.float32))
    if tuple(d_out.shape) != (B, S, dims[1]):
        raise ValueError(f"encoder_backward: d_out must be {(B, S, dims[1])}, got {tuple(d_out.shape)}")
    lib = _lib.load()
    tape_bytes = int(lib.m2_encoder_tape_bytes(*dims, B, S))
    if tape_bytes == 0:
        raise M2Error(f"encoder_backward: unsupported shape (V, H, layers, heads) = {dims}, B={B} S={S}")
    if tape.numel() < tape_bytes:
        raise ValueError("encoder_backward: the tape is not that of this shape")
    onto = accumulate if accumulate else None
    want = [True] * len(keep) if need is None else [bool(n) for n in need]
    grads = []
    for i, (p, w) in enumerate(zip(keep, want)):
        if not w:
            grads.append(None)
        elif onto is not None and onto[i] is not None:
            grads.append(onto[i])
        else:
            grads.append(torch.empty_like(p) if onto is None else torch.zeros_like(p))
    gp = (ctypes.c_void_p * len(keep))(*[_ptr(g) for g in grads])
    ws = torch.empty(max(int(lib.m2_encoder_backward_workspace_bytes(*dims, B, S)), 1), dtype=torch.uint8, device=dev)
    _lib.call("m2_encoder_backward", ptrs, *dims, _ptr(ids), _ptr(mask), B, S, _ptr(tape), _ptr(d_out), gp,
              0 if onto is None else 1, _ptr(ws), ws.numel(), stream_handle(dev))
    return grads


def embedding_backward(ids: Tensor, d_x: Tensor, vocab: int, scale: float = 1.0, accumulate: Optional[Tensor] = None):
    """d_emb [vocab, H] = scale * the sum of d_x [.., H] over the positions whose id is the row
    (m2_embedding_backward); ids outside [0, vocab) contribute nothing.  ``accumulate``: a [vocab, H] tensor
    to add to instead of a new one."""
    require_device(ids, d_x, accumulate, what="embedding_backward")
    ids, d_x = ids.to(torch.int64).contiguous(), f32c(d_x)
    H = d_x.shape[-1]
    R = ids.numel()
    if d_x.numel() != R * H:
        raise ValueError(f"embedding_backward: d_x {tuple(d_x.shape)} does not fit ids {tuple(ids.shape)}")
    dev = d_x.device
    vocab = int(vocab)
    if accumulate is not None and _like(accumulate, (vocab, H), "embedding_backward: accumulate") is not accumulate:
        raise ValueError("embedding_backward: accumulate must be contiguous float32")
    d_emb = accumulate if accumulate is not None else torch.empty(vocab, H, device=dev, dtype=torch.float32)
    ws = torch.empty(max(int(_lib.load().m2_embedding_backward_workspace_bytes(R, vocab, H)), 1), dtype=torch.uint8,
                     device=dev)
    _lib.call("m2_embedding_backward", _ptr(ids), _ptr(d_x), R, vocab, H, float(scale), _ptr(d_emb),
              0 if accumulate is None else 1, _ptr(ws), ws.numel(), stream_handle(dev))
    return d_emb


def layer_norm_backward(g_y: Tensor, x: Tensor, gamma: Tensor, g_res: Optional[Tensor] = None):
    """(g_x, dgamma, dbeta) of y = LayerNorm(x; gamma, beta) over the last dim given g_y
    (m2_layer_norm_backward); g_x is the input's cotangent plus ``g_res``."""
    require_device(g_y, x, gamma, g_res, what="layer_norm_backward")
    g_y, x = f32c(g_y), f32c(x)
    K = x.shape[-1]
    R = x.numel() // K if K else 0
    gamma = _vec(gamma, K, "layer_norm_backward: gamma")
    g_y = _like(g_y, x.shape, "layer_norm_backward: g_y")
    g_res = _like(g_res, x.shape, "layer_norm_backward: g_res")
    dev = x.device
    g_x = torch.empty_like(x)
    dg, db = torch.empty(K, device=dev, dtype=torch.float32), torch.empty(K, device=dev, dtype=torch.float32)
    ws = torch.empty(max(int(_lib.load().m2_layer_norm_backward_workspace_bytes(R, K)), 1), dtype=torch.uint8,
                     device=dev)
    _lib.call("m2_layer_norm_backward", _ptr(g_y), _ptr(x), _ptr(gamma), _ptr(g_res), R, K, _ptr(g_x), _ptr(dg),
              _ptr(db), _ptr(ws), ws.numel(), stream_handle(dev))
    return g_x, dg, db


def regulate_backward(d_reg: Tensor, cum: Tensor, S: int) -> Tensor:
    """The adjoint of ``expand_frames`` (m2_length_regulator_backward): d_enc [B,S,H] given d_reg [B,T_out,H]
    and the prefix sums cum [B,S+1] the forward expanded with.  Durations get no gradient."""
    require_device(d_reg, cum, what="length_regulator")
    d_reg = f32c(d_reg)
    B, T_out, H = d_reg.shape
    S = int(S)
    if tuple(cum.shape) != (B, S + 1) or cum.dtype != torch.int32:
        raise ValueError(f"regulate_backward: cum must be int32 {(B, S + 1)}, got {cum.dtype} {tuple(cum.shape)}")
    d_enc = torch.empty(B, S, H, device=d_reg.device, dtype=torch.float32)
    if d_enc.numel() == 0:
        return d_enc
    _lib.call("m2_length_regulator_backward", _ptr(d_reg), _ptr(cum.contiguous()), B, S, H, T_out, _ptr(d_enc),
              stream_handle(d_reg.device))
    return d_enc


DURATION_PARAMS = 10
DURATION_TAPE_NAMES = ("y1", "y2")


def batchnorm_eval_stats(weight: Tensor, bias: Tensor, mean: Tensor, var: Tensor, eps: float) -> Tensor:
    """One block's four vectors of ``duration_train_forward``'s ``bn_stats`` as a [4, H] tensor: alpha and
    beta' exactly as ``batchnorm_eval_affine`` returns them, the running mean, and invstd = 1 / sqrt(var + eps)."""
    alpha, beta = batchnorm_eval_affine(weight.detach(), bias.detach(), mean, var, eps)
    invstd = 1.0 / torch.sqrt(var + eps)
    return torch.stack([alpha, beta, mean.to(torch.float32), invstd])


def _duration_params(params, bn_stats):
    """DurationPredictor's 10 parameters (parameters() order) as contiguous float32 device tensors, their
    pointer array, bn_stats as one contiguous [8, H] tensor (eight [H] vectors, or two [4, H] blocks), and H."""
    keep = [f32c(p.detach()) for p in params]
    if len(keep) != DURATION_PARAMS:
        raise ValueError(f"duration: (conv.weight, conv.bias, norm.weight, norm.bias) x 2, projection.weight, "
                         f"projection.bias in parameters() order, got {len(keep)}")
    require_device(*keep, what="duration parameter")
    H = int(keep[0].shape[0])
    shapes = [(H, H, 3), (H,), (H,), (H,)] * 2 + [(1, H, 1), (1,)]
    for i, (t, want) in enumerate(zip(keep, shapes)):
        if tuple(t.shape) != want:
            raise ValueError(f"duration: parameter {i} must be {want} (kernel size 3), got {tuple(t.shape)}")
    bn = bn_stats if isinstance(bn_stats, Tensor) else torch.cat([b.detach().reshape(-1, H) for b in bn_stats])
    require_device(bn, what="duration bn_stats")
    bn = f32c(bn.detach().reshape(-1, H))
    if tuple(bn.shape) != (8, H):
        raise ValueError(f"duration: bn_stats must be 8 vectors [{H}] (alpha, beta', mean, invstd per block), got "
                         f"{tuple(bn.shape)}")
    return keep, (ctypes.c_void_p * len(keep))(*[t.data_ptr() for t in keep]), bn, H


def _duration_enc(enc: Tensor, H: int) -> Tensor:
    require_device(enc, what="duration")
    if enc.dim() != 3 or enc.shape[2] != H:
        raise ValueError(f"duration: enc must be [B, S, {H}], got {tuple(enc.shape)}")
    return f32c(enc.detach())


def duration_supported(H: int) -> bool:
    """Whether m2_duration_backward takes a DurationPredictor of this width (host arithmetic only)."""
    return int(_lib.load().m2_duration_tape_bytes(H, 1, 1)) != 0


def duration_train_forward(params, bn_stats, enc: Tensor):
    """DurationPredictor's forward from its raw parameters and the eval-mode BatchNorm constants, keeping a
    tape (m2_duration_train_forward): (dur [B,S], bit-equal to the stand-alone module's forward, and the tape,
    a uint8 tensor that ``duration_tape_maps`` names and ``duration_backward`` reads).  ``bn_stats``: alpha,
    beta', running mean and invstd of block 1, then of block 2 (``batchnorm_eval_stats`` per block)."""
    keep, ptrs, bn, H = _duration_params(params, bn_stats)
    enc = _duration_enc(enc, H)
    B, S, _ = enc.shape
    dev = enc.device
    need = int(_lib.load().m2_duration_tape_bytes(H, B, S))
    if need == 0:
        raise M2Error(f"duration_train_forward: unsupported shape H = {H}, B={B} S={S}")
    tape = torch.empty(need, dtype=torch.uint8, device=dev)
    dur = torch.empty(B, S, device=dev, dtype=torch.float32)
    _lib.call("m2_duration_train_forward", ptrs, _ptr(bn), H, _ptr(enc), B, S, _ptr(dur), _ptr(tape), tape.numel(),
              stream_handle(dev))
    return dur, tape


def duration_tape_maps(tape: Tensor, H: int, B: int, S: int) -> dict:
    """The maps of a tape as float32 views (m2_duration_tape_map): y1 and y2 [B,H,S], the two ConvBlocks'
    outputs (post-ReLU)."""
    lib = _lib.load()
    flat = tape[:tape.numel() // 4 * 4].view(torch.float32)
    off, width = ctypes.c_size_t(), ctypes.c_int32()
    maps = {}
    for i, name in enumerate(DURATION_TAPE_NAMES):
        _lib.check(lib.m2_duration_tape_map(H, B, S, i, ctypes.byref(off), ctypes.byref(width)), "m2_duration_tape_map")
        maps[name] = flat[off.value:off.value + B * S * width.value].view(B, width.value, S)
    return maps


def duration_backward(params, bn_stats, enc: Tensor, tape: Tensor, d_dur: Tensor, need_enc: bool = True, need=None,
                      accumulate=False):
    """The gradients of DurationPredictor given d_dur [B,S] (m2_duration_backward): (d_enc [B,S,H] or None,
    the 10 gradients in parameters() order, None where ``need[i]`` is false).  ``accumulate``: a list of that
    many tensors (or None entries) to add the gradients to instead of new tensors."""
    keep, ptrs, bn, H = _duration_params(params, bn_stats)
    enc = _duration_enc(enc, H)
    B, S, _ = enc.shape
    dev = enc.device
    require_device(tape, d_dur, what="duration_backward")
    d_dur = f32c(d_dur.detach().to(torch.float32))
    if tuple(d_dur.shape) != (B, S):
        raise ValueError(f"duration_backward: d_dur must be {(B, S)}, got {tuple(d_dur.shape)}")
    lib = _lib.load()
    tape_bytes = int(lib.m2_duration_tape_bytes(H, B, S))
    if tape_bytes == 0:
        raise M2Error(f"duration_backward: unsupported shape H = {H}, B={B} S={S}")
    if tape.numel() < tape_bytes:
        raise ValueError("duration_backward: the tape is not that of this shape")
    onto = accumulate if accumulate else None
    want = [True] * len(keep) if need is None else [bool(n) for n in need]
    grads = []
    for i, (p, w) in enumerate(zip(keep, want)):
        if not w:
            grads.append(None)
        elif onto is not None and onto[i] is not None:
            grads.append(onto[i])
        else:
            grads.append(torch.empty_like(p) if onto is None else torch.zeros_like(p))
    gp = (ctypes.c_void_p * len(keep))(*[_ptr(g) for g in grads])
    d_enc = torch.empty_like(enc) if need_enc else None
    ws = torch.empty(max(int(lib.m2_duration_backward_workspace_bytes(H, B, S)), 1), dtype=torch.uint8, device=dev)
    _lib.call("m2_duration_backward", ptrs, _ptr(bn), H, _ptr(enc), B, S, _ptr(tape), _ptr(d_dur), _ptr(d_enc), gp,
              0 if onto is None else 1, _ptr(ws), ws.numel(), stream_handle(dev))
    return d_enc, grads


def embed_positional(ids: Tensor, emb: Tensor, pe: Tensor, scale: float) -> Tensor:
    """y[b,s,:] = emb[ids[b,s],:] * scale + pe[s,:]; ids outside [0, vocab) read a zero row."""
    require_device(ids, emb, pe, what="embedding")
    ids = ids.to(torch.int64).contiguous()
    emb, pe = f32c(emb), f32c(pe)
    if ids.dim() != 2 or emb.dim() != 2:
        raise RuntimeError(f"embedding: ids must be [B, S] and emb [vocab, H], got {_shape(ids)} and {_shape(emb)}")
    B, S = ids.shape
    H = emb.shape[1]
    if pe.dim() != 2 or pe.shape[0] < S or pe.shape[1] != H:
        raise RuntimeError(f"embedding: the positional table must be [>= {S}, {H}], got {_shape(pe)}")
    y = torch.empty(B, S, H, device=emb.device, dtype=torch.float32)
    if y.numel() == 0:
        return y
    _lib.call("m2_embed_positional", _ptr(ids), _ptr(emb), _ptr(pe), B, S, H, emb.shape[0],
              float(scale), _ptr(y), stream_handle(emb.device))
    return y


def add_positional(x: Tensor, pe: Tensor) -> Tensor:
    """y = x + pe[:S] for x [B,S,H]; pe [rows >= S, H] (leading dimensions of size 1 allowed)."""
    require_device(x, pe, what="positional encoding")
    x, pe = f32c(x), f32c(pe)
    if x.dim() != 3:
        raise RuntimeError(f"positional encoding: x must be [B, S, H], got {_shape(x)}")
    B, S, H = x.shape
    if pe.dim() < 2 or pe.shape[-1] != H or pe.numel() != pe.shape[-2] * H:
        raise RuntimeError(f"positional encoding: the table must be [rows, {H}], got {_shape(pe)}")
    if S > pe.shape[-2]:
        raise RuntimeError(f"sequence length {S} exceeds the positional table ({pe.shape[-2]})")
    y = torch.empty_like(x)
    if y.numel() == 0:
        return y
    _lib.call("m2_add_positional", _ptr(x), _ptr(pe), B, S, H, _ptr(y), stream_handle(x.device))
    return y


def durations_for_regulator(durations: Tensor):
    """Return (tensor, is_int) in the form m2_length_regulator_count reads.

    fp32 durations are passed as-is (int() truncation happens in the kernel);
    integer durations become int32; other float dtypes are truncated toward
    zero in their own precision first (what int(d.item()) does)."""
    if durations.dtype == torch.float32:
        return durations.contiguous(), 0
    if durations.is_floating_point():
        return torch.trunc(durations).clamp(-2**30, 2**30).to(torch.int32).contiguous(), 1
    return durations.clamp(-2**30, 2**30).to(torch.int32).contiguous(), 1


def frame_counts(durations: Tensor, scale: float = 1.0):
    """Counting half of the length regulator (m2_length_regulator_count):
    returns (cum [B,S+1] int32 exclusive prefix sums, T [B] int32, Tmax [1] int32)."""
    require_device(durations, what="length_regulator")
    B, S = durations.shape
    d, is_int = durations_for_regulator(durations)
    dev = durations.device
    cum = torch.empty(B, S + 1, device=dev, dtype=torch.int32)
    tot = torch.empty(B, device=dev, dtype=torch.int32)
    tmax = torch.empty(1, device=dev, dtype=torch.int32)
    _lib.call("m2_length_regulator_count", _ptr(d), is_int, float(scale), B, S, _ptr(cum), _ptr(tot), _ptr(tmax),
              stream_handle(dev))
    return cum, tot, tmax


def frame_counts_sync(durations: Tensor, scale: float = 1.0):
    """frame_counts plus the host read of T_max (m2_length_regulator_count_sync:
    a host-mapped mailbox the count kernel posts to, polled in C with the GIL
    released): returns (cum, T, Tmax device tensors, Tmax as an int)."""
    require_device(durations, what="length_regulator")
    B, S = durations.shape
    d, is_int = durations_for_regulator(durations)
    dev = durations.device
    cum = torch.empty(B, S + 1, device=dev, dtype=torch.int32)
    tot = torch.empty(B, device=dev, dtype=torch.int32)
    tmax = torch.empty(1, device=dev, dtype=torch.int32)
    host = ctypes.c_int32(0)
    _lib.call("m2_length_regulator_count_sync", _ptr(d), is_int, float(scale), B, S, _ptr(cum), _ptr(tot), _ptr(tmax),
              ctypes.addressof(host), stream_handle(dev))
    return cum, tot, tmax, int(host.value)


def expand_frames(enc: Tensor, cum: Tensor, T_out: int) -> Tensor:
    """Expanding half (m2_length_regulator_expand): [B,S,H] -> [B,T_out,H]."""
    enc = f32c(enc)
    B, S, H = enc.shape
    out = torch.empty(B, T_out, H, device=enc.device, dtype=torch.float32)
    _lib.call("m2_length_regulator_expand", _ptr(enc), _ptr(cum), B, S, H, T_out, _ptr(out), stream_handle(enc.device))
    return out


def regulate(enc: Tensor, durations: Tensor, max_length: Optional[int] = None, scale: float = 1.0) -> Tensor:
    """LengthRegulator.forward (tts_model.py:126-178) on the GPU: scan + gather.

    One device->host read of the batch maximum frame count, only when
    max_length is not given (it sizes the output)."""
    return regulate_with_counts(enc, durations, max_length, scale)[0]


def regulate_with_counts(enc: Tensor, durations: Tensor, max_length: Optional[int] = None, scale: float = 1.0):
    """``regulate`` and the prefix sums it expanded with: (out [B,T_out,H], cum [B,S+1] int32), what
    ``regulate_backward`` reads."""
    require_device(enc, durations, what="length_regulator")
    if max_length is not None:
        cum, _, _ = frame_counts(durations, scale)
        return expand_frames(enc, cum, max_length), cum
    cum, _, _, t_max = frame_counts_sync(durations, scale)
    # an utterance with no frames becomes one zero frame (tts_model.py:158-160)
    return expand_frames(enc, cum, max(1, t_max)), cum


def batchnorm_eval_affine(weight: Tensor, bias: Tensor, mean: Tensor, var: Tensor, eps: float):
    """alpha = w / sqrt(var + eps), beta = b - mean * alpha (ATen's eval-mode form).

    Parameter preprocessing on the device (a few elementwise ops on H-sized
    vectors), not part of the per-frame work."""
    invstd = 1.0 / torch.sqrt(var + eps)
    alpha = invstd * weight
    return alpha.contiguous(), (bias - mean * alpha).contiguous()


def sqrt_hidden(h: int) -> float:
    return h ** 0.5


def inv_sqrt(hd: int) -> float:
    return 1.0 / math.sqrt(hd)
