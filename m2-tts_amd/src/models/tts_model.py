"""Drop-in ``models.tts_model`` for MI355X.

Same classes, constructor signatures, submodule/parameter names (so
reference checkpoints load unchanged), return types and shapes as the
reference ``src/models/tts_model.py``; the forward path runs on gfx950 HIP
kernels through the C ABI in ``include/m2tts_hip.h``:

* ``M2TTSModel.forward`` / ``inference`` use one packed model handle
  (``m2amd.runtime.HipModel``): one C call per stage, the length regulator as
  a GPU scan + gather with a single device->host read of the frame count.
* The stage modules (``text_encoder``, ``duration_predictor``,
  ``length_regulator``, ``decoder``, ``vocoder``) may be called directly, as
  the reference's callers do; inside an M2TTSModel they use the owner's
  handle, standalone they compose the per-op kernels of ``m2amd.ops``.

Differences from the reference that do not change results:
* ``inference`` runs the vocoder once (the reference runs it inside
  ``forward`` and again afterwards, tts_model.py:388-391 vs 435-436, on the
  same mel) and skips the unscaled decoder pass when duration_scale != 1.
* Eval-mode math only; see models/components.py.
"""
from __future__ import annotations

import logging
import weakref
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from m2amd import _lib, ops, runtime
from m2amd.runtime import HandleCache, make_config

from .components import (LightweightResBlock, PositionalEncoding, TransformerEncoderLayer, VariancePredictor,
                         _eval_only, count_parameters, create_padding_mask, initialize_weights)

logger = logging.getLogger(__name__)
Tensor = torch.Tensor

UPSAMPLE_RATES = (4, 4, 2, 2)   # reference tts_model.py:244
VOCODER_HALO = 3                # receptive field of one audio sample, mel frames per side (m2_vocoder_halo_frames)
_HANDLES: "weakref.WeakKeyDictionary[nn.Module, HandleCache]" = weakref.WeakKeyDictionary()


def unpad(mel: Tensor, audio: Tensor, frames: Tensor) -> List[Tuple[Tensor, Tensor]]:
    """The utterances of an ``inference_ragged`` result without their padding:
    a list of (mel_b [T_b, M], audio_b [64 T_b]) views, T_b = frames[b].  Pure
    indexing (one host read of ``frames``), on any device."""
    if mel.dim() != 3 or audio.dim() != 3 or audio.shape[1] != 1 or audio.shape[2] != 64 * mel.shape[1]:
        raise ValueError(f"unpad: expected mel [B,T,M] and audio [B,1,64T], got {tuple(mel.shape)} and "
                         f"{tuple(audio.shape)}")
    counts = [int(t) for t in frames.tolist()]
    if len(counts) != mel.shape[0] or audio.shape[0] != mel.shape[0]:
        raise ValueError(f"unpad: {len(counts)} frame counts for a batch of {mel.shape[0]}")
    if any(t < 0 or t > mel.shape[1] for t in counts):
        raise ValueError(f"unpad: frame counts {counts} outside [0, {mel.shape[1]}]")
    return [(mel[b, :t], audio[b, 0, :64 * t]) for b, t in enumerate(counts)]


def _owner_handle(stage: nn.Module, attr: str, device: torch.device):
    """The owning M2TTSModel's packed handle if `stage` is still its `attr`."""
    ref = getattr(stage, "_m2_owner", None)
    owner = ref() if ref is not None else None
    if owner is None or getattr(owner, attr, None) is not stage:
        return None
    return owner._hip(device)


class _EncoderGrad(torch.autograd.Function):
    """TextEncoder.forward with a graph: ops.encoder_train_forward on the
    module's own parameters, and ops.encoder_backward on grad_output (once
    differentiable).  Arguments: ids, the positional rows, the key mask or
    None, the head count, then the 1 + 11 layers + 2 parameters in
    parameters() order."""

    @staticmethod
    def forward(ctx, ids, pe, mask, heads, *params):
        out, tape = ops.encoder_train_forward(params, ids, pe, mask, heads)
        ctx.save_for_backward(ids, *params)
        ctx.tape, ctx.heads, ctx.mask = tape, heads, mask
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        ids, *params = ctx.saved_tensors
        grads = ops.encoder_backward(params, ids, ctx.mask, ctx.tape, grad_output, ctx.heads,
                                     need=ctx.needs_input_grad[4:])
        return (None, None, None, None, *grads)


class TextEncoder(nn.Module):
    """Embedding*sqrt(H) + positional table, pre-LN transformer layers with a
    key-padding mask, final LayerNorm (reference tts_model.py:19-89).

    ``enable_backward()`` gives ``forward`` a graph: when gradients are enabled
    and a parameter requires grad, the output comes from the per-op path on
    the module's own parameters (inside an M2TTSModel too: no handle, the
    stand-alone module's bits) and carries a ``grad_fn`` whose backward fills
    the 1 + 11 layers + 2 ``.grad`` on the GPU; the mask is returned as without
    it.  The gradient is that of the function this module computes: no dropout
    (models/components.py).  Off by default; with it off, under ``no_grad`` or
    with nothing requiring grad, ``forward`` is unchanged."""

    backward_enabled = False

    def __init__(self, vocab_size: int = 256, hidden_dim: int = 64, num_layers: int = 2, num_heads: int = 2,
                 dropout: float = 0.1, max_seq_len: int = 1000):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.embedding = nn.Embedding(vocab_size, hidden_dim)
        self.pos_encoding = PositionalEncoding(hidden_dim, max_seq_len)
        self.layers = nn.ModuleList(
            [TransformerEncoderLayer(hidden_dim=hidden_dim, num_heads=num_heads, ffn_dim=hidden_dim * 2, dropout=dropout)
             for _ in range(num_layers)])
        self.norm = nn.LayerNorm(hidden_dim)
        self.dropout = nn.Dropout(dropout)
        self.apply(initialize_weights)

    def _dims(self) -> Tuple[int, int, int, int]:
        """(V, H, layers, heads)."""
        v, h = self.embedding.weight.shape
        heads = self.layers[0].self_attn.num_heads if len(self.layers) else 0
        return int(v), int(h), len(self.layers), int(heads)

    def enable_backward(self, enabled: bool = True) -> "TextEncoder":
        """Switch the graph of ``forward`` on or off (a plain attribute, no
        state_dict entry).  Supported: a vocabulary of 1 to 65536, H a multiple
        of 8 with 2 H <= 256, head_dim in {16, 32, 48, 64}, at least one
        layer."""
        if enabled:
            v, h, layers, heads = self._dims()
            ok = (layers >= 1 and 1 <= v <= 65536 and h % 8 == 0 and 2 * h <= 256 and heads >= 1 and h % heads == 0
                  and h // heads in (16, 32, 48, 64) and self.embedding.padding_idx is None
                  and all(la.ffn.linear1.out_features == 2 * h for la in self.layers))
            if not ok:
                raise NotImplementedError(f"TextEncoder.enable_backward: a vocabulary of 1 to 65536, hidden_dim a "
                                          f"multiple of 8 up to 128, head_dim 16, 32, 48 or 64 and at least one layer; "
                                          f"got vocabulary {v}, hidden_dim {h}, {heads} heads, {layers} layers")
        self.backward_enabled = bool(enabled)
        return self

    def forward(self, phoneme_ids: Tensor, lengths: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
        if self.backward_enabled and torch.is_grad_enabled():
            params = list(self.parameters())
            if any(p.requires_grad for p in params):
                ops.require_device(phoneme_ids, lengths, *params, what="TextEncoder")
                s = phoneme_ids.shape[1]
                if s > self.pos_encoding.pe.shape[1]:
                    raise RuntimeError(f"sequence length {s} exceeds the positional table "
                                       f"({self.pos_encoding.pe.shape[1]})")
                mask = create_padding_mask(lengths, s) if lengths is not None else None
                out = _EncoderGrad.apply(phoneme_ids, self.pos_encoding.pe[0, :s], mask, self._dims()[3], *params)
                return out, mask
        hm = _owner_handle(self, "text_encoder", phoneme_ids.device)
        if hm is not None:
            return hm.text_encoder(phoneme_ids, lengths)
        ops.require_device(phoneme_ids, self.embedding.weight, what="TextEncoder")
        _, s = phoneme_ids.shape
        mask = create_padding_mask(lengths, s) if lengths is not None else None
        x = ops.embed_positional(phoneme_ids, self.embedding.weight, self.pos_encoding.pe[0, :s],
                                 ops.sqrt_hidden(self.hidden_dim))
        for layer in self.layers:
            x = layer(x, mask)
        return ops.layer_norm(x, self.norm.weight, self.norm.bias), mask


class _DurationGrad(torch.autograd.Function):
    """DurationPredictor.forward with a graph: ops.duration_train_forward on the
    module's own parameters and the eval-mode BatchNorm constants, and
    ops.duration_backward on grad_output (once differentiable).  Arguments:
    encoder_output, the constants [8, H] (ops.batchnorm_eval_stats per block),
    then the 10 parameters in parameters() order."""

    @staticmethod
    def forward(ctx, enc, bn, *params):
        dur, tape = ops.duration_train_forward(params, bn, enc)
        ctx.save_for_backward(enc, bn, *params)
        ctx.tape = tape
        return dur

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        enc, bn, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_enc, grads = ops.duration_backward(params, bn, enc, ctx.tape, grad_output, need_enc=need[0], need=need[2:])
        return (d_enc, None, *grads)


class DurationPredictor(nn.Module):
    """softplus(VariancePredictor(enc^T)) -> [B, S] (reference tts_model.py:92-117).

    ``enable_backward()`` gives ``forward`` a graph: when gradients are enabled
    and ``encoder_output`` or a parameter requires grad, the durations come
    from the per-op path on the module's own parameters (inside an M2TTSModel
    too: no handle, the stand-alone module's bits) and carry a ``grad_fn``
    whose backward fills the 10 ``.grad`` and ``encoder_output.grad`` on the
    GPU.  The gradient is that of the function this module computes: BatchNorm
    with its running statistics as constants (the buffers get no gradient and
    are not written), no dropout (models/components.py).  Off by default; with
    it off, under ``no_grad`` or with nothing requiring grad, ``forward`` is
    unchanged."""

    backward_enabled = False

    def __init__(self, hidden_dim: int = 64, kernel_size: int = 3, dropout: float = 0.1):
        super().__init__()
        self.predictor = VariancePredictor(hidden_dim, kernel_size, dropout)

    def enable_backward(self, enabled: bool = True) -> "DurationPredictor":
        """Switch the graph of ``forward`` on or off (a plain attribute, no
        state_dict entry).  Supported: kernel size 3, H a multiple of 8 from 16
        to 128."""
        if enabled:
            conv = self.predictor.conv_layers[0].conv
            k, h = int(conv.kernel_size[0]), int(conv.out_channels)
            if k != 3 or h % 8 != 0 or not 16 <= h <= 128:
                raise NotImplementedError(f"DurationPredictor.enable_backward: kernel size 3 and hidden_dim a multiple "
                                          f"of 8 from 16 to 128; got kernel size {k}, hidden_dim {h}")
        self.backward_enabled = bool(enabled)
        return self

    def forward(self, encoder_output: Tensor) -> Tensor:
        if self.backward_enabled and torch.is_grad_enabled():
            params = list(self.parameters())
            if encoder_output.requires_grad or any(p.requires_grad for p in params):
                ops.require_device(encoder_output, *params, what="DurationPredictor")
                stats = []
                for blk in self.predictor.conv_layers:
                    _eval_only(blk)
                    n = blk.norm
                    stats.append(ops.batchnorm_eval_stats(n.weight, n.bias, n.running_mean, n.running_var, n.eps))
                return _DurationGrad.apply(encoder_output, torch.cat(stats), *params)
        hm = _owner_handle(self, "duration_predictor", encoder_output.device)
        if hm is not None:
            return hm.duration(encoder_output)
        x = encoder_output.transpose(1, 2).contiguous()
        return self.predictor(x, _act=ops.ACT_SOFTPLUS).squeeze(1)


class _RegulateGrad(torch.autograd.Function):
    """LengthRegulator.forward with a graph: ops.regulate's own launches
    (with its one host read when max_length is None), keeping the prefix sums;
    the backward is the expansion's adjoint, ops.regulate_backward (once
    differentiable).  Durations get no gradient: the reference takes
    int(duration.item())."""

    @staticmethod
    def forward(ctx, encoder_output, durations, max_length):
        out, cum = ops.regulate_with_counts(encoder_output, durations, max_length)
        ctx.cum, ctx.phonemes = cum, encoder_output.shape[1]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        return ops.regulate_backward(grad_output, ctx.cum, ctx.phonemes), None, None


class LengthRegulator(nn.Module):
    """Repeat each phoneme row int(duration) times, pad/truncate to the batch
    maximum or ``max_length`` (reference tts_model.py:120-178).  GPU scan +
    gather; truncation toward zero and the all-zero-durations case (one zero
    frame) follow the reference.

    ``enable_backward()`` gives ``forward`` a graph: when gradients are enabled
    and ``encoder_output`` requires grad, the result carries a ``grad_fn``
    whose backward sums each phoneme's frames back into ``encoder_output.grad``
    on the GPU; durations get no gradient.  Off by default; with it off, under
    ``no_grad`` or with ``encoder_output`` not requiring grad, ``forward`` is
    unchanged."""

    backward_enabled = False

    def enable_backward(self, enabled: bool = True) -> "LengthRegulator":
        """Switch the graph of ``forward`` on or off (a plain attribute, no
        state_dict entry)."""
        self.backward_enabled = bool(enabled)
        return self

    def forward(self, encoder_output: Tensor, durations: Tensor, max_length: Optional[int] = None) -> Tensor:
        if self.backward_enabled and torch.is_grad_enabled() and encoder_output.requires_grad:
            return _RegulateGrad.apply(encoder_output, durations.detach(), max_length)
        return ops.regulate(encoder_output, durations, max_length)


class _DecoderGrad(torch.autograd.Function):
    """MelDecoder.forward with a graph: ops.decoder_train_forward on the
    module's own parameters, and ops.decoder_backward on grad_output (once
    differentiable).  Arguments: x, the head count, then the 11 layers + 4
    parameters in state_dict order."""

    @staticmethod
    def forward(ctx, x, heads, *params):
        mel, tape = ops.decoder_train_forward(params, x, heads)
        ctx.save_for_backward(x, *params)
        ctx.tape, ctx.heads = tape, heads
        return mel

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        x, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_x, grads = ops.decoder_backward(params, x, ctx.tape, grad_output, ctx.heads, need_x=need[0], need=need[2:])
        return (d_x, None, *grads)


class MelDecoder(nn.Module):
    """Unmasked pre-LN transformer over frames -> LayerNorm -> Linear(H, M)
    (reference tts_model.py:181-228).

    ``enable_backward()`` gives ``forward`` a graph: when gradients are enabled
    and x or a parameter requires grad, the mel comes from the per-op path on
    the module's own parameters (inside an M2TTSModel too: no handle, the
    stand-alone module's bits) and carries a ``grad_fn`` whose backward fills
    the 11 layers + 4 ``.grad`` and ``x.grad`` on the GPU.  The gradient is that
    of the function this module computes: no dropout (models/components.py).
    Off by default; with it off, under ``no_grad`` or with nothing requiring
    grad, ``forward`` is unchanged."""

    backward_enabled = False

    def __init__(self, hidden_dim: int = 64, mel_channels: int = 64, num_layers: int = 2, num_heads: int = 2,
                 dropout: float = 0.1):
        super().__init__()
        self.layers = nn.ModuleList(
            [TransformerEncoderLayer(hidden_dim=hidden_dim, num_heads=num_heads, ffn_dim=hidden_dim * 2, dropout=dropout)
             for _ in range(num_layers)])
        self.norm = nn.LayerNorm(hidden_dim)
        self.mel_projection = nn.Linear(hidden_dim, mel_channels)
        self.apply(initialize_weights)

    def _dims(self) -> Tuple[int, int, int, int]:
        """(H, M, layers, heads)."""
        m, h = self.mel_projection.weight.shape
        heads = self.layers[0].self_attn.num_heads if len(self.layers) else 0
        return int(h), int(m), len(self.layers), int(heads)

    def enable_backward(self, enabled: bool = True) -> "MelDecoder":
        """Switch the graph of ``forward`` on or off (a plain attribute, no
        state_dict entry).  Supported: H a multiple of 8 with 2 H <= 256,
        head_dim in {16, 32, 48, 64}, at least one layer."""
        if enabled:
            h, m, layers, heads = self._dims()
            ok = (layers >= 1 and h % 8 == 0 and 2 * h <= 256 and heads >= 1 and h % heads == 0
                  and h // heads in (16, 32, 48, 64) and m >= 1
                  and all(la.ffn.linear1.out_features == 2 * h for la in self.layers))
            if not ok:
                raise NotImplementedError(f"MelDecoder.enable_backward: hidden_dim a multiple of 8 up to 128, head_dim "
                                          f"16, 32, 48 or 64 and at least one layer; got hidden_dim {h}, "
                                          f"{heads} heads, {layers} layers")
        self.backward_enabled = bool(enabled)
        return self

    def forward(self, x: Tensor) -> Tensor:
        if self.backward_enabled and torch.is_grad_enabled():
            params = list(self.parameters())
            if x.requires_grad or any(p.requires_grad for p in params):
                ops.require_device(x, *params, what="MelDecoder")
                return _DecoderGrad.apply(x, self._dims()[3], *params)
        hm = _owner_handle(self, "decoder", x.device)
        if hm is not None:
            return hm.decoder(x)
        for layer in self.layers:
            x = layer(x)
        return ops.linear(x, self.mel_projection.weight, self.mel_projection.bias,
                          ln=(self.norm.weight, self.norm.bias))


class _VocoderGrad(torch.autograd.Function):
    """SimpleVocoder.forward with a graph: ops.vocoder_train_forward on the
    module's own parameters, and ops.vocoder_backward on grad_output (once
    differentiable).  Arguments: mel, then the 28 parameters in state_dict
    order."""

    @staticmethod
    def forward(ctx, mel, *params):
        audio, tape = ops.vocoder_train_forward(params, mel)
        ctx.save_for_backward(mel, *params)
        ctx.tape = tape
        return audio

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        mel, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_mel, grads = ops.vocoder_backward(params, mel, ctx.tape, grad_output, need_mel=need[0], need=need[1:])
        return (d_mel, *grads)


class SimpleVocoder(nn.Module):
    """input_conv -> 4 x [ConvT(k=2r, s=r, p=r/2) -> leaky(0.1) -> resblock]
    -> output_conv -> tanh; 64 samples per mel frame (reference
    tts_model.py:231-297).  ``kernel_size``/``n_layers`` are accepted and, as
    in the reference, do not change the upsampling schedule.

    ``enable_backward()`` gives ``forward`` a graph: when gradients are enabled
    and mel or a parameter requires grad, the audio comes from the exact-fp32
    per-op path on the module's own parameters (inside an M2TTSModel too: no
    handle, the stand-alone module's bits) and carries a ``grad_fn`` whose
    backward fills the 28 ``.grad`` and ``mel.grad`` on the GPU.  Off by
    default; with it off, under ``no_grad`` or with nothing requiring grad,
    ``forward`` is unchanged."""

    backward_enabled = False

    def __init__(self, mel_channels: int = 64, hidden_channels: int = 128, kernel_size: int = 3, n_layers: int = 4):
        super().__init__()
        self.input_conv = nn.Conv1d(mel_channels, hidden_channels, kernel_size, padding=kernel_size // 2)
        self.upsamples = nn.ModuleList()
        self.resblocks = nn.ModuleList()
        ch = hidden_channels
        for r in UPSAMPLE_RATES:
            self.upsamples.append(nn.ConvTranspose1d(ch, ch // 2, kernel_size=2 * r, stride=r, padding=r // 2))
            ch //= 2
            self.resblocks.append(LightweightResBlock(ch, kernel_size))
        self.output_conv = nn.Conv1d(ch, 1, kernel_size, padding=kernel_size // 2)
        self.apply(initialize_weights)

    def enable_backward(self, enabled: bool = True) -> "SimpleVocoder":
        """Switch the graph of ``forward`` on or off (a plain attribute, no
        state_dict entry); kernel size 3 only."""
        if enabled and self.input_conv.kernel_size[0] != 3:
            raise NotImplementedError(f"SimpleVocoder.enable_backward: kernel_size 3 only, got "
                                      f"{self.input_conv.kernel_size[0]}")
        self.backward_enabled = bool(enabled)
        return self

    def forward(self, mel: Tensor) -> Tensor:
        if self.backward_enabled and torch.is_grad_enabled():
            params = list(self.parameters())
            if mel.requires_grad or any(p.requires_grad for p in params):
                ops.require_device(mel, *params, what="SimpleVocoder")
                return _VocoderGrad.apply(mel, *params)
        hm = _owner_handle(self, "vocoder", mel.device)
        if hm is not None:
            return hm.vocoder(mel, layout_btm=False)
        # any kernel_size: input / output convs with padding k//2 and the
        # resblocks' general form (an even k changes lengths and the resblock
        # residual fails, as in the reference)
        x = ops.conv1d(mel, self.input_conv.weight, self.input_conv.bias, padding=self.input_conv.padding[0])
        for r, up, rb in zip(UPSAMPLE_RATES, self.upsamples, self.resblocks):
            x = ops.conv_transpose1d(x, up.weight, up.bias, r, act=ops.ACT_LEAKY)
            x = rb(x)
        return ops.conv1d(x, self.output_conv.weight, self.output_conv.bias, act=ops.ACT_TANH,
                          padding=self.output_conv.padding[0])

    def stream(self, mel: Tensor, chunk_frames: int = 256):
        """Yield the audio of mel [B, M, T] chunk by chunk ([B, 1, 64 n] for
        n <= chunk_frames frames each), for playback while later chunks are
        still being computed.  Each chunk is computed over its window widened
        by the vocoder's receptive field (VOCODER_HALO frames per side): the
        chunks concatenate to exactly forward(mel) (the reference's one-shot
        output, tts_model.py:279-297)."""
        if chunk_frames <= 0:
            raise ValueError("chunk_frames must be positive")
        hm = _owner_handle(self, "vocoder", mel.device)
        if hm is not None:
            yield from hm.vocoder_stream(mel, chunk_frames)
            return
        T = mel.shape[2]
        for f0 in range(0, T, chunk_frames):
            f1 = min(T, f0 + chunk_frames)
            w0, w1 = max(0, f0 - VOCODER_HALO), min(T, f1 + VOCODER_HALO)
            yield self.forward(mel[:, :, w0:w1])[:, :, 64 * (f0 - w0):64 * (f1 - w0)].contiguous()


class M2TTSModel(nn.Module):
    """Text encoder -> duration predictor -> length regulator -> mel decoder ->
    vocoder (reference tts_model.py:300-459).

    ``enable_backward()`` gives ``forward`` a graph: when gradients are enabled
    and a parameter requires grad, ``forward`` composes the stage modules with
    their switches on (no handle: an optimizer step changes every weight) and
    returns the same six keys, ``mel_output`` and ``duration_pred`` carrying
    ``grad_fn``s, so the reference's training step (a mel loss plus a duration
    loss, ``backward()``, an optimizer step) runs on the GPU.  The length
    regulator gives durations no gradient, as in the reference.  The vocoder's
    switch stays the caller's (``model.vocoder.enable_backward()``).  Off by
    default; with it off, under ``no_grad`` or with nothing requiring grad,
    ``forward`` is unchanged."""

    backward_enabled = False

    def __init__(self, vocab_size: int = 256, hidden_dim: int = 64, mel_channels: int = 64,
                 text_encoder_layers: int = 2, decoder_layers: int = 2, num_heads: int = 2, dropout: float = 0.1,
                 vocoder_channels: int = 128):
        super().__init__()
        self.text_encoder = TextEncoder(vocab_size=vocab_size, hidden_dim=hidden_dim, num_layers=text_encoder_layers,
                                        num_heads=num_heads, dropout=dropout)
        self.duration_predictor = DurationPredictor(hidden_dim=hidden_dim, dropout=dropout)
        self.length_regulator = LengthRegulator()
        self.decoder = MelDecoder(hidden_dim=hidden_dim, mel_channels=mel_channels, num_layers=decoder_layers,
                                  num_heads=num_heads, dropout=dropout)
        self.vocoder = SimpleVocoder(mel_channels=mel_channels, hidden_channels=vocoder_channels)
        self._m2_cfg = make_config(vocab_size, hidden_dim, mel_channels, text_encoder_layers, decoder_layers,
                                   num_heads, vocoder_channels, self.text_encoder.pos_encoding.pe.shape[1])
        me = weakref.ref(self)
        for stage in (self.text_encoder, self.duration_predictor, self.decoder, self.vocoder):
            object.__setattr__(stage, "_m2_owner", me)
        total, trainable = count_parameters(self)
        logger.info(f"M2TTSModel: {total:,} parameters ({trainable:,} trainable), "
                    f"{total * 4 / (1024 * 1024):.1f} MB fp32")

    def enable_backward(self, enabled: bool = True) -> "M2TTSModel":
        """Switch the graph of ``forward`` on or off (a plain attribute, no
        state_dict entry), together with the switches of ``text_encoder``,
        ``duration_predictor``, ``length_regulator`` and ``decoder``.  A stage
        that refuses its shape raises NotImplementedError, and then nothing is
        switched.  The vocoder's switch is not touched."""
        stages = (self.text_encoder, self.duration_predictor, self.length_regulator, self.decoder)
        before = [st.backward_enabled for st in stages]
        try:
            for st in stages:
                st.enable_backward(enabled)
        except NotImplementedError:
            for st, was in zip(stages, before):
                st.backward_enabled = was
            raise
        self.backward_enabled = bool(enabled)
        return self

    # -------------------------------------------------------------- handle
    def _eval_if_training(self):
        """self.eval() (tts_model.py:404) without the recursive train(False)
        walk when every module is already in eval mode (~35 us of host time per
        call at stage1, more than the length regulator's GPU time)."""
        mods = self.__dict__.get("_m2_modules")
        if mods is None or mods[0] != runtime._GEN[0]:
            mods = (runtime._GEN[0], list(self.modules()))
            self.__dict__["_m2_modules"] = mods
        for mod in mods[1]:
            if mod.training:
                self.eval()
                return

    def _hip(self, device: torch.device, lane: int = 0):
        cache = _HANDLES.get(self)
        if cache is None:
            cache = HandleCache()
            _HANDLES[self] = cache
        return cache.get(self, self._m2_cfg, device, lane)

    def set_vocoder_chunking(self, chunk_frames: int = 256):
        """Stream the vocoder in chunks of ``chunk_frames`` mel frames inside
        forward/inference/vocoder (0 = whole utterance).  Each chunk is
        computed over a window widened by the vocoder's 3-frame receptive
        field, so the audio is bit-identical to the unchunked call; the
        workspace holds one window instead of the whole utterance."""
        self.__dict__["_m2_chunk_frames"] = int(chunk_frames)
        cache = _HANDLES.get(self)
        for hm in (cache.handles() if cache is not None else []):
            hm.set_chunking(chunk_frames)

    def set_range_policy(self, policy: str = "fallback"):
        """The split-f16 vocoder carries fp32 values as f16 hi/lo pairs; an
        input or activation of magnitude >= 65520 turns its audio non-finite
        (never silently wrong).  "fallback" (the default, also without this
        call; M2_RANGE_POLICY overrides it for new handles): the non-finite
        part of a vocoder call is recomputed in fp32 on the device before
        anything behind it on the stream runs, so a call never returns
        non-finite audio for an input the reference's fp32 path handles.  On
        the pipelined tails (the defaults) each strip whose split audio is not
        finite is recomputed inside the tail launch by direct fp32 convolution
        in the reference's layer order (within the reference-conditioned
        tolerance, not bit-equal to the exact-f32 kernels); M2_REDO_LAUNCH=1
        and the windowed tails use the guarded exact-f32 launch behind the
        split kernels instead (bit-equal to those kernels).  The per-call cost
        is bench.py's ``vocoder_report_policy`` difference.
        "report" (opt-in): asynchronous - the next call raises,
        check_numerics() reports it at once."""
        if policy not in runtime.RANGE_POLICIES:
            raise ValueError(f"range policy {policy!r}: expected one of {sorted(runtime.RANGE_POLICIES)}")
        self.__dict__["_m2_range_policy"] = policy
        cache = _HANDLES.get(self)
        for hm in (cache.handles() if cache is not None else []):
            hm.set_range_policy(policy)

    def check_numerics(self, device: Optional[torch.device] = None):
        """Synchronise and raise if a split-path vocoder call since the last
        check produced non-finite audio (M2_E_RANGE semantics)."""
        cache = _HANDLES.get(self)
        want = None
        if device is not None:
            want = torch.device(device)
            if want.type == "cuda" and want.index is None:
                want = torch.device("cuda", torch.cuda.current_device())
        for hm in (cache.handles() if cache is not None else []):
            if (want is None or hm.device == want) and hm.check():
                raise ops.M2Error(
                    "m2-tts_amd: a split-f16 vocoder call produced non-finite audio (an input or activation "
                    "of magnitude >= 65520); re-run with set_vocoder_precision('f32') or set_range_policy('fallback')")

    def set_vocoder_precision(self, precision: str = "split"):
        """"split" = split-f16 MFMA kernels (fp32 operands as f16 hi/lo pairs,
        the default), "f32" = exact-f32 MFMA kernels."""
        path = {"split": 2, "f32": 1}[precision]
        self.__dict__["_m2_voc_path"] = path
        cache = _HANDLES.get(self)
        for hm in (cache.handles() if cache is not None else []):
            hm.vocoder_select(path)

    # -------------------------------------------------------------- forward
    def forward(self, phoneme_ids: Tensor, phoneme_lengths: Optional[Tensor] = None,
                target_durations: Optional[Tensor] = None,
                max_target_length: Optional[int] = None) -> Dict[str, Optional[Tensor]]:
        """Reference tts_model.py:350-400: audio only when not training."""
        ops.require_device(phoneme_ids, what="M2TTSModel")
        if self.backward_enabled and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            enc, mask = self.text_encoder(phoneme_ids, phoneme_lengths)
            dur = self.duration_predictor(enc)
            durations = target_durations if target_durations is not None else dur.detach()
            reg = self.length_regulator(enc, durations, max_target_length)
            mel = self.decoder(reg)
            audio = None if self.training else self.vocoder(mel.transpose(1, 2))
            return {"encoder_output": enc, "duration_pred": dur, "regulated_output": reg,
                    "mel_output": mel, "audio_output": audio, "padding_mask": mask}
        with torch.no_grad():
            hm = self._hip(phoneme_ids.device)
            enc, mask = hm.text_encoder(phoneme_ids, phoneme_lengths)
            dur = hm.duration(enc)
            durations = target_durations if target_durations is not None else dur
            reg = ops.regulate(enc, durations, max_target_length)
            mel = hm.decoder(reg)
            audio = None if self.training else hm.vocoder(mel, layout_btm=True)
        return {"encoder_output": enc, "duration_pred": dur, "regulated_output": reg,
                "mel_output": mel, "audio_output": audio, "padding_mask": mask}

    def inference(self, phoneme_ids: Tensor, phoneme_lengths: Optional[Tensor] = None,
                  duration_scale: float = 1.0) -> Tuple[Tensor, Tensor]:
        """(mel [B,T,M], audio [B,1,64T]) - reference tts_model.py:402-438."""
        self._eval_if_training()
        ops.require_device(phoneme_ids, what="M2TTSModel")
        with torch.no_grad():
            mel, audio = self._hip(phoneme_ids.device).inference(phoneme_ids, phoneme_lengths, duration_scale)
        return mel, audio

    def inference_ragged(self, phoneme_ids: Tensor, phoneme_lengths: Optional[Tensor] = None,
                         duration_scale: float = 1.0,
                         durations: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        """A batch of independent requests: (mel [B,T_max,M], audio
        [B,1,64 T_max], frames int64 [B]).  frames[b] = T_b is utterance b's own
        frame count, max(1, sum_s int(d[b,s])) with d = ``durations`` ([B,S],
        used as forward's target_durations) or duration_pred * duration_scale;
        mel[b, :T_b] and audio[b, 0, :64 T_b] are what the single-utterance
        call on the same S columns returns (within the parity tolerance: tile
        forms differ between a batch and a single call), everything behind is
        exactly 0.  With equal T_b the result is inference()'s, bit for bit.
        ``unpad`` splits the result.  inference() and forward() keep the
        reference's batch-coupled semantics (every utterance decoded over
        T_max rows)."""
        self._eval_if_training()
        ops.require_device(phoneme_ids, phoneme_lengths, durations, what="M2TTSModel")
        with torch.no_grad():
            hm = self._hip(phoneme_ids.device)
            try:
                mel, audio, frames = hm.inference_ragged(phoneme_ids, phoneme_lengths, duration_scale, durations)
            except ops.M2Error as e:
                if e.status != _lib.M2_E_SHAPE:
                    raise
                if not self.__dict__.get("_m2_ragged_warned"):
                    self.__dict__["_m2_ragged_warned"] = True
                    logger.warning(f"inference_ragged: running the utterances one by one ({e})")
                mel, audio, frames = self._ragged_one_by_one(phoneme_ids, phoneme_lengths, duration_scale, durations)
        return mel, audio, frames.to(torch.int64)

    def _ragged_one_by_one(self, ids: Tensor, lengths: Optional[Tensor], scale: float, durations: Optional[Tensor]):
        """inference_ragged by its definition: B single-utterance calls,
        assembled into the zero-padded outputs."""
        outs = []
        for b in range(ids.shape[0]):
            lb = lengths[b:b + 1] if lengths is not None else None
            if durations is None:
                outs.append(self.inference(ids[b:b + 1], lb, scale))
            else:
                r = self(ids[b:b + 1], lb, target_durations=durations[b:b + 1])
                outs.append((r["mel_output"], r["audio_output"]))
        dev = ids.device
        frames = torch.tensor([m.shape[1] for m, _ in outs], dtype=torch.int64, device=dev)
        T = max([m.shape[1] for m, _ in outs], default=1)
        mel = torch.zeros(len(outs), T, self._m2_cfg.mel_channels, device=dev, dtype=torch.float32)
        audio = torch.zeros(len(outs), 1, 64 * T, device=dev, dtype=torch.float32)
        for b, (m, a) in enumerate(outs):
            mel[b, :m.shape[1]] = m[0]
            audio[b, 0, :a.shape[2]] = a[0, 0]
        return mel, audio, frames

    def get_model_size(self) -> Dict[str, Any]:
        """Parameter counts per component (reference tts_model.py:440-459)."""
        comps = {}
        for name, module in self.named_children():
            total, trainable = count_parameters(module)
            comps[name] = {"total": total, "trainable": trainable, "size_mb": total * 4 / (1024 * 1024)}
        total, trainable = count_parameters(self)
        return {"total_params": total, "trainable_params": trainable,
                "total_size_mb": total * 4 / (1024 * 1024), "components": comps}
