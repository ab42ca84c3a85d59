"""Loss functions of M2 TTS training, stage 2 (reference src/training/losses.py).

Same class names, constructor signatures, defaults, attribute names,
state_dict keys and returned dict keys as the reference, computed on the GPU:
the discriminators' convolutions, the STFTs and every reduction run in the
m2_disc_* / m2_loss_spectral / m2_eval_pair_stats kernels (m2amd.ops,
m2amd.dsp), which write per-utterance rows of double sums; a few torch ops on
the device turn those rows into the reference's means, so a call needs no host
synchronisation.

**Values, and three gradients.**  By default every returned value is a 0-dim
float32 tensor on the inputs' device with ``requires_grad=False``: the values
carry no autograd graph, the same contract M2TTSModel.forward has in this
tree, and score a checkpoint with the objective it was trained on.

The discriminator step of the reference's stage-2 trainer is available on
request: after ``CombinedTTSLoss.enable_backward()`` (or
``AdversarialLoss.enable_backward()``), with gradients enabled and at least
one discriminator parameter requiring grad,
``AdversarialLoss.discriminator_loss(real, fake)`` and the
``discriminator_loss`` and ``total_loss`` entries of
``CombinedTTSLoss.forward(..., optimize_discriminator=True)`` carry a
``grad_fn``: one ``torch.autograd.Function`` whose forward runs m2_disc_step
(the same values, bit for bit, and the gradients of all 42 parameters) and
whose backward hands those gradients out scaled by ``grad_output``, on the
device.  So ``optimizer_d.zero_grad(); loss(...)['total_loss'].backward();
clip_grad_norm_(...); optimizer_d.step()`` works as in the reference.  The
backward is once-differentiable, the audio inputs get no gradient (the
reference detaches the fake audio there), and parameters with
``requires_grad=False`` get ``None``.

The same switch governs the generator side.  A generator-side graph exists
only when the switch is on, gradients are enabled and the prediction tensor in
question has ``requires_grad=True``; with plain input tensors everything stays
graph-free.  Values are computed as without the switch and are bit-equal; an
``_AttachGradients`` function returns the value unchanged and, in its
once-differentiable backward, hands each prediction its kept gradient scaled
by ``grad_output``, on the device.

* ``AdversarialLoss.generator_loss(fake)``, ``feature_matching_loss(real,
  fake)`` and ``generator_terms(real, fake, adversarial_weight,
  feature_matching_weight)`` (the weighted sum as one tensor from one pass)
  run m2_disc_gen_step: the gradient through the three discriminators into the
  fake audio.  ``real`` never gets a gradient.
* ``CombinedTTSLoss.forward`` in generator mode runs one m2_disc_gen_step with
  its two weights in place of the forward-only sums when ``audio_pred``
  requires grad (same rows, same values, no second forward).  Its ``mel_loss``
  and ``duration_loss`` entries carry a ``grad_fn`` when ``mel_pred`` /
  ``duration_pred`` require grad (sign(pred - target) over the counted frames,
  and 2 (p - t) / n, a few device-side torch ops); ``generator_loss`` and
  ``feature_matching_loss`` stay plain values.  ``total_loss`` carries a graph
  only when every term of it with a non-zero weight has a gradient, i.e. with
  ``spectral_loss_weight == perceptual_loss_weight == 0``, without audio, or
  with the spectral switch below; otherwise it stays graph-free and a one-time
  warning names the terms without a gradient, because a ``backward()`` that
  silently omitted two terms would be worse than none.

**The spectral and perceptual gradient** has a switch of its own, default off
and not in the state_dict: ``CombinedTTSLoss.enable_backward(spectral=True)``,
or ``SpectralLoss.enable_backward()`` / ``PerceptualLoss.enable_backward()`` on
either module alone.  ``enable_backward()`` and ``enable_backward(False)`` leave
it off, and everything above is then exactly as described.  With it on,
gradients enabled and a predicted audio that requires grad,
``SpectralLoss.forward`` / ``stft_loss``, ``PerceptualLoss.forward`` and the
``spectral_loss`` and ``perceptual_loss`` entries of generator mode carry a
once-differentiable ``grad_fn`` that reaches the predicted audio (the target
gets nothing), and generator mode's ``total_loss`` follows its rule: at the
default weights every term now has a gradient, so ``total_loss.backward()``
fills ``mel_pred``, ``duration_pred`` and ``audio_pred`` gradients.  Values are
computed as without the switch and are bit-equal.  The gradient is computed in
``backward``, from the saved audio pair, by m2_loss_spectral_backward: the
forward's framing and FFT, the cotangent of every bin in double, an inverse FFT
per frame and a fixed-order gather into each sample (the STFT's adjoint).  Its
coefficients are host numbers from the shapes (``spectral_backward_calls``);
the total runs three calls, n_fft 512, 1024 and 2048, the 1024 one carrying the
perceptual term with its weight, each accumulating onto a copy of the generator
step's gradient, and ``grad_output`` multiplies on the device: no host
synchronisation, and a forward that is never backpropagated costs nothing
extra.  In a frame that reflect padding makes symmetric (frame 0; the last when
L = 1 mod hop) the imaginary parts are rounding residue and so is the sign of
the phase term in every bin, in any float32 evaluation including the
reference's; the kernel differentiates on its own spectrum.

One difference from the reference: there a generator ``backward()`` also fills
the discriminators' ``.grad``, which its trainer zeroes before the next
discriminator step, so nothing reads them; here the generator step leaves the
42 parameters' ``.grad`` alone.

Nothing goes through ``MultiScaleDiscriminator.forward`` or into
``M2TTSModel`` yet, and the trainers are not part of this package.

The discriminators' parameters live in plain ``nn.Conv1d`` modules built in the
reference's order, so ``torch.manual_seed(s); CombinedTTSLoss()`` gives the
reference's weights bit for bit and the reference's checkpoints load.  Packed
copies are cached per device and rebuilt when a parameter changes
(``load_state_dict``, ``.to``, an optimizer step).

Like the rest of the product path there is no CPU fallback: CPU tensors raise
RuntimeError (the module itself imports and constructs anywhere).
"""
from __future__ import annotations

import logging
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

logger = logging.getLogger(__name__)

Tensor = torch.Tensor
SAMPLE_RATE = 22050  # names the m2_dsp tables; no loss depends on it
# PerceptualLoss's framing and feature count (the reference's _mel_features): its forward and its
# gradient both read them from here
PERCEPTUAL_N_FFT, PERCEPTUAL_HOP, PERCEPTUAL_MELS = 1024, 256, 80


def _require(*tensors, what: str):
    from m2amd.ops import require_device
    require_device(*tensors, what=what)


def _audio_pair(pred: Tensor, target: Tensor, what: str) -> Tuple[Tensor, Tensor]:
    """pred, target [B, 1, L] (or [B, L]) -> float32 [B, L] each."""
    _require(pred, target, what=what)
    p = pred.detach().float().reshape(pred.shape[0], -1)
    t = target.detach().float().reshape(target.shape[0], -1)
    if p.shape != t.shape:
        raise RuntimeError(f"{what}: pred audio {tuple(pred.shape)} and target audio {tuple(target.shape)} differ")
    return p, t


def _spectral_rows(p: Tensor, t: Tensor, n_fft: int, hop: int, cache: Optional[dict]) -> Dict[str, Tensor]:
    """Batch sums (0-dim float64) of Dsp.loss_spectral's columns; ``cache`` shares a
    framing between SpectralLoss and PerceptualLoss within one call."""
    key = (n_fft, hop)
    if cache is not None and key in cache:
        return cache[key]
    from m2amd.dsp import get_dsp, loss_columns
    d = get_dsp(SAMPLE_RATE, n_fft, hop, n_fft, device=p.device)
    sums = d.loss_spectral(p, t, PerceptualLoss.mel_weights(p.device, n_fft // 2 + 1)).sum(0)
    rows = {name: sums[i] for i, name in enumerate(loss_columns("spectral"))}
    if cache is not None:
        cache[key] = rows
    return rows


def spectral_backward_calls(B: int, L: int, n_fft_list=(512, 1024, 2048), hop_length_factor: float = 0.25,
                            spectral_weight: float = 1.0, perceptual_weight: float = 0.0):
    """The Dsp.loss_spectral_backward calls behind the gradient of spectral_weight * SpectralLoss +
    perceptual_weight * PerceptualLoss for audio [B, L]: [(n_fft, hop, c_mag, c_phase, c_perc)], host
    numbers from the shapes.  Per n_fft the means over B F frames bins, averaged over the sizes:
    c_mag = spectral_weight / (len(n_fft_list) B F frames), c_phase = 0.1 c_mag; the perceptual mean
    over B PERCEPTUAL_MELS frames joins the call at PerceptualLoss's framing (1024, 256):
    c_perc = perceptual_weight / (B PERCEPTUAL_MELS frames).
    Terms of weight 0 make no call."""
    calls: Dict[Tuple[int, int], list] = {}
    if B <= 0:
        return []
    if spectral_weight:
        for n_fft in n_fft_list:
            hop = int(n_fft * hop_length_factor)
            c = float(spectral_weight) / (len(n_fft_list) * B * (n_fft // 2 + 1) * (1 + L // hop))
            e = calls.setdefault((n_fft, hop), [0.0, 0.0, 0.0])
            e[0] += c
            e[1] += 0.1 * c
    if perceptual_weight:
        e = calls.setdefault((PERCEPTUAL_N_FFT, PERCEPTUAL_HOP), [0.0, 0.0, 0.0])
        e[2] += float(perceptual_weight) / (B * PERCEPTUAL_MELS * (1 + L // PERCEPTUAL_HOP))
    return [(n_fft, hop, c[0], c[1], c[2]) for (n_fft, hop), c in calls.items()]


def _spectral_gradient(pred: Tensor, target: Tensor, calls, base: Optional[Tensor] = None) -> Tensor:
    """float32 [B, L]: a copy of ``base`` (or nothing) plus the gradients of ``calls`` with respect to
    pred, each call accumulating onto the one before in stream order."""
    from m2amd.dsp import get_dsp
    with torch.no_grad():
        p, t = _audio_pair(pred, target, "SpectralLoss")
        out = None if base is None else base.detach().float().reshape(p.shape).clone(
            memory_format=torch.contiguous_format)
        for n_fft, hop, c_mag, c_phase, c_perc in calls:
            d = get_dsp(SAMPLE_RATE, n_fft, hop, n_fft, device=p.device)
            out = d.loss_spectral_backward(p, t, PerceptualLoss.mel_weights(p.device, n_fft // 2 + 1), c_mag, c_phase,
                                           c_perc, out=out, accumulate=out is not None)
        return torch.zeros_like(p) if out is None else out


class _AttachSpectral(torch.autograd.Function):
    """_AttachGradients whose last input, the predicted audio, gets the spectral and perceptual
    gradient of ``calls`` as well: computed in backward from the saved audio pair, so a forward that
    is never backpropagated launches nothing, and accumulated onto a copy of ``base`` (the audio's
    kept gradient, or None)."""

    @staticmethod
    def forward(ctx, value, grads, base, calls, target, *inputs):
        ctx.grads = [g.to(x.dtype).reshape(x.shape) for g, x in zip(grads, inputs[:-1])]
        ctx.base, ctx.calls = base, calls
        ctx.save_for_backward(inputs[-1], target)
        return value.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        pred, target = ctx.saved_tensors
        need = ctx.needs_input_grad[5:]
        audio = None
        if need[-1]:
            g = _spectral_gradient(pred, target, ctx.calls, ctx.base)
            audio = (grad_output.to(g.dtype) * g).to(pred.dtype).reshape(pred.shape)
        return (None,) * 5 + tuple(grad_output.to(g.dtype) * g if n else None
                                   for g, n in zip(ctx.grads, need[:-1])) + (audio,)


def _attach_spectral(value: Tensor, pairs, audio_pred: Tensor, audio_target: Tensor, calls, base=None) -> Tensor:
    """``value`` (no graph) with a grad_fn that reaches the inputs of ``pairs`` as _attach does and
    audio_pred through ``calls`` (spectral_backward_calls) on top of ``base``."""
    with torch.enable_grad():
        return _AttachSpectral.apply(value, [g for _, g in pairs], base, calls, audio_target.detach(),
                                     *[x for x, _ in pairs], audio_pred)


def _switched(module, pred: Optional[Tensor]) -> bool:
    """Whether ``module``'s own switch gives a term of ``pred`` a graph: the switch, grad mode, and pred itself."""
    return module.backward_enabled and torch.is_grad_enabled() and pred is not None and pred.requires_grad


class SpectralLoss(nn.Module):
    """Multi-scale spectral loss: per n_fft, mean | |P| - |T| | + 0.1 mean |angle P - angle T|
    over torch.stft(hop n_fft * factor, Hann, centre, reflect padding), averaged over the sizes.
    After enable_backward() the value carries the gradient with respect to pred_audio."""

    backward_enabled = False  # set by enable_backward(); a plain attribute, not in the state_dict

    def __init__(self, n_fft_list=[512, 1024, 2048], hop_length_factor=0.25):
        super().__init__()
        self.n_fft_list = n_fft_list
        self.hop_length_factor = hop_length_factor

    def enable_backward(self, enabled: bool = True):
        """Let the loss carry its gradient with respect to the predicted audio (module docstring)."""
        self.backward_enabled = bool(enabled)
        return self

    def _calls(self, shape, weight: float = 1.0, n_fft_list=None):
        return spectral_backward_calls(shape[0], shape[1], self.n_fft_list if n_fft_list is None else n_fft_list,
                                       self.hop_length_factor, weight, 0.0)

    def _stft_loss(self, p: Tensor, t: Tensor, n_fft: int, cache: Optional[dict]) -> Tensor:
        r = _spectral_rows(p, t, n_fft, int(n_fft * self.hop_length_factor), cache)
        return r["mag_abs"] / r["bins"] + r["phase_abs"] / r["bins"] * 0.1

    def stft_loss(self, pred_audio, target_audio, n_fft):
        """The loss of one STFT size."""
        with torch.no_grad():
            p, t = _audio_pair(pred_audio, target_audio, "SpectralLoss")
            value = self._stft_loss(p, t, n_fft, None).float()
        if _switched(self, pred_audio):
            return _attach_spectral(value, [], pred_audio, target_audio, self._calls(p.shape, 1.0, [n_fft]))
        return value

    def _value(self, p: Tensor, t: Tensor, cache: Optional[dict]) -> Tensor:
        total = 0
        for n_fft in self.n_fft_list:
            total = total + self._stft_loss(p, t, n_fft, cache)
        return total / len(self.n_fft_list)

    def forward(self, pred_audio, target_audio):
        with torch.no_grad():
            p, t = _audio_pair(pred_audio, target_audio, "SpectralLoss")
            value = self._value(p, t, None).float()
        if _switched(self, pred_audio):
            return _attach_spectral(value, [], pred_audio, target_audio, self._calls(p.shape))
        return value


class _DiscriminatorStep(torch.autograd.Function):
    """The discriminator loss with the gradients of the discriminators' parameters, both from one
    m2_disc_step call in forward; backward scales the kept gradients by grad_output."""

    @staticmethod
    def forward(ctx, disc, real, fake, *params):
        rows, grads = disc._handle(real.device).step(real, fake)
        ctx.grads = grads
        return disc._discriminator_value(disc._columns(rows.sum(0))).float()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        return (None, None, None) + tuple(grad_output * g if need else None
                                          for g, need in zip(ctx.grads, ctx.needs_input_grad[3:]))


class _AttachGradients(torch.autograd.Function):
    """A value computed outside autograd together with its gradients: forward returns ``value``
    unchanged, backward hands each input its kept gradient (cast and reshaped to the input's dtype
    and shape) scaled by grad_output, on the device."""

    @staticmethod
    def forward(ctx, value, grads, *inputs):
        ctx.grads = [g.to(x.dtype).reshape(x.shape) for g, x in zip(grads, inputs)]
        return value.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        return (None, None) + tuple(grad_output.to(g.dtype) * g if need else None
                                    for g, need in zip(ctx.grads, ctx.needs_input_grad[2:]))


def _attach(value: Tensor, pairs) -> Tensor:
    """``value`` (no graph) with a grad_fn that reaches the inputs of ``pairs`` [(input, gradient)]."""
    with torch.enable_grad():
        return _AttachGradients.apply(value, [g for _, g in pairs], *[x for x, _ in pairs])


class MultiScaleDiscriminator(nn.Module):
    """Multi-scale discriminator: seven Conv1d per scale, scale i on avg_pool1d(x, scales[i])."""

    backward_enabled = False  # set by enable_backward(); a plain attribute, not in the state_dict

    def __init__(self, scales=[1, 2, 4]):
        super().__init__()
        self.scales = scales
        self.discriminators = nn.ModuleList([
            self._make_discriminator() for _ in scales
        ])

    def _make_discriminator(self):
        return nn.Sequential(
            nn.Conv1d(1, 64, 15, 1, padding=7),
            nn.LeakyReLU(0.2),
            nn.Conv1d(64, 128, 41, 4, padding=20, groups=4),
            nn.LeakyReLU(0.2),
            nn.Conv1d(128, 256, 41, 4, padding=20, groups=16),
            nn.LeakyReLU(0.2),
            nn.Conv1d(256, 512, 41, 4, padding=20, groups=64),
            nn.LeakyReLU(0.2),
            nn.Conv1d(512, 1024, 41, 4, padding=20, groups=256),
            nn.LeakyReLU(0.2),
            nn.Conv1d(1024, 1024, 5, 1, padding=2),
            nn.LeakyReLU(0.2),
            nn.Conv1d(1024, 1, 3, 1, padding=1),
        )

    def _handle(self, device: torch.device):
        """The packed discriminators on ``device``, rebuilt when a parameter changed."""
        from m2amd.ops import Discriminators
        from m2amd.runtime import state_key
        key = state_key(self)
        handles = self.__dict__.setdefault("_m2_handles", {})
        ent = handles.get(device)
        if ent is not None and ent[0] == key:
            return ent[1]
        tensors = list(self.state_dict(keep_vars=True).values())
        _require(*tensors, what="MultiScaleDiscriminator")
        if any(t.device != device for t in tensors):
            raise RuntimeError(f"MultiScaleDiscriminator: parameters on {tensors[0].device}, audio on {device}")
        h = Discriminators(tensors, self.scales, device)
        handles[device] = (key, h)
        return h

    def forward(self, x):
        """x [B, 1, L] -> (logits per scale, the six pre-activation feature maps per scale)."""
        _require(x, what="MultiScaleDiscriminator")
        with torch.no_grad():
            return self._handle(x.device).forward(x, features=True)

    @staticmethod
    def _columns(sums: Tensor) -> Dict[str, Tensor]:
        from m2amd.dsp import loss_columns
        return {name: sums[i] for i, name in enumerate(loss_columns("disc"))}

    def _sums(self, real: Optional[Tensor], fake: Optional[Tensor]) -> Dict[str, Tensor]:
        """Batch sums (0-dim float64) of the m2_disc_losses columns."""
        ref = real if real is not None else fake
        _require(real, fake, what="AdversarialLoss")
        return self._columns(self._handle(ref.device).losses(real, fake).sum(0))

    def _discriminator_value(self, c: Dict[str, Tensor]) -> Tensor:
        """mean over scales of [mean (D(real) - 1)^2 + mean D(fake)^2], float64."""
        n = len(self.scales)
        real = sum(c[f"s{s}_real_err_sq"] / c[f"s{s}_logits"] for s in range(n))
        fake = sum(c[f"s{s}_fake_sq"] / c[f"s{s}_logits"] for s in range(n))
        return (real + fake) / n

    def enable_backward(self, enabled: bool = True):
        """Let the discriminator loss carry the gradients of this module's parameters (module docstring)."""
        self.backward_enabled = bool(enabled)
        return self

    def _wants_backward(self) -> bool:
        return self.backward_enabled and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def _wants_gradient(self, pred: Optional[Tensor]) -> bool:
        """Whether a generator-side term of ``pred`` carries a graph: the switch, grad mode, and pred itself."""
        return self.backward_enabled and torch.is_grad_enabled() and pred is not None and pred.requires_grad

    def _gen_step(self, real: Optional[Tensor], fake: Tensor, w_adv: float, w_fm: float):
        """``_sums(real, fake)`` (the same rows, from m2_disc_gen_step) and the gradient of w_adv *
        generator loss + w_fm * feature-matching loss with respect to fake, float32 [B, 1, L]."""
        _require(real, fake, what="AdversarialLoss")
        with torch.no_grad():
            rows, d_fake = self._handle(fake.device).gen_step(real, fake, w_adv, w_fm)
            return self._columns(rows.sum(0)), d_fake

    def _step_loss(self, real: Tensor, fake: Tensor) -> Tensor:
        """The discriminator loss (0-dim float32) with a grad_fn that reaches the parameters."""
        _require(real, fake, what="AdversarialLoss")
        with torch.enable_grad():
            return _DiscriminatorStep.apply(self, real.detach(), fake.detach(),
                                            *self.state_dict(keep_vars=True).values())


class AdversarialLoss(nn.Module):
    """GAN-based adversarial loss (least squares); values, and after enable_backward() the
    discriminator loss's gradient with respect to the discriminators' parameters."""

    def __init__(self):
        super().__init__()
        self.discriminator = MultiScaleDiscriminator()

    def _mse(self, c: Dict[str, Tensor], col: str) -> Tensor:
        n = len(self.discriminator.scales)
        return sum(c[f"s{s}_{col}"] / c[f"s{s}_logits"] for s in range(n))

    def _generator(self, c) -> Tensor:
        return self._mse(c, "fake_err_sq") / len(self.discriminator.scales)

    def _feature_matching(self, c) -> Tensor:
        n, layers = len(self.discriminator.scales), 6  # len(real_features) * len(real_features[0])
        total = sum(c[f"s{s}_l{j}_abs_diff"] / c[f"s{s}_l{j}_count"] for s in range(n) for j in range(layers))
        return total / (n * layers)

    def enable_backward(self, enabled: bool = True):
        """Switch the gradient of discriminator_loss on or off (module docstring)."""
        self.discriminator.enable_backward(enabled)
        return self

    def discriminator_loss(self, real_audio, fake_audio):
        if self.discriminator._wants_backward():
            return self.discriminator._step_loss(real_audio, fake_audio)
        with torch.no_grad():
            return self.discriminator._discriminator_value(self.discriminator._sums(real_audio, fake_audio)).float()

    def generator_loss(self, fake_audio):
        if self.discriminator._wants_gradient(fake_audio):
            c, d_fake = self.discriminator._gen_step(None, fake_audio, 1.0, 0.0)
            return _attach(self._generator(c).float(), [(fake_audio, d_fake)])
        with torch.no_grad():
            return self._generator(self.discriminator._sums(None, fake_audio)).float()

    def feature_matching_loss(self, real_audio, fake_audio):
        if self.discriminator._wants_gradient(fake_audio):
            c, d_fake = self.discriminator._gen_step(real_audio, fake_audio, 0.0, 1.0)
            return _attach(self._feature_matching(c).float(), [(fake_audio, d_fake)])
        with torch.no_grad():
            return self._feature_matching(self.discriminator._sums(real_audio, fake_audio)).float()

    def generator_terms(self, real_audio, fake_audio, adversarial_weight: float = 1.0,
                        feature_matching_weight: float = 1.0):
        """adversarial_weight * generator_loss + feature_matching_weight * feature_matching_loss as one
        0-dim tensor from one pass over each signal; with a gradient (module docstring) one chain
        through the discriminators serves both terms."""
        aw, fw = float(adversarial_weight), float(feature_matching_weight)
        grad = self.discriminator._wants_gradient(fake_audio)
        if grad:
            c, d_fake = self.discriminator._gen_step(real_audio, fake_audio, aw, fw)
        with torch.no_grad():
            if not grad:
                c = self.discriminator._sums(real_audio, fake_audio)
            value = (aw * self._generator(c) + fw * self._feature_matching(c)).float()
        return _attach(value, [(fake_audio, d_fake)]) if grad else value


class PerceptualLoss(nn.Module):
    """Perceptual loss on the reference's "mel" features: its filter rows are
    constant (row j holds w_j in every bin, w_0 = 0), so a feature is
    ln(w_j sum_f |X| + 1e-8) of a frame's magnitude sum."""

    _WEIGHTS: Dict[Tuple, Tensor] = {}
    backward_enabled = False  # set by enable_backward(); a plain attribute, not in the state_dict

    def __init__(self, model_type="mel"):
        super().__init__()
        self.model_type = model_type
        self.feature_extractor = self._mel_features

    def enable_backward(self, enabled: bool = True):
        """Let the loss carry its gradient with respect to the predicted audio (module docstring)."""
        self.backward_enabled = bool(enabled)
        return self

    @staticmethod
    def _calls(shape, weight: float = 1.0):
        return spectral_backward_calls(shape[0], shape[1], (), 0.25, 0.0, weight)

    @classmethod
    def mel_weights(cls, device, freq_bins: int = PERCEPTUAL_N_FFT // 2 + 1, n_mels: int = PERCEPTUAL_MELS) -> Tensor:
        """The filter rows' values, by the reference's float32 expressions."""
        key = (torch.device(device), freq_bins, n_mels)
        w = cls._WEIGHTS.get(key)
        if w is None:
            f = torch.linspace(0, 1, n_mels, dtype=torch.float32).unsqueeze(1).expand(n_mels, freq_bins)
            f = f / (f.sum(dim=1, keepdim=True) + 1e-8)
            w = cls._WEIGHTS[key] = f[:, 0].contiguous().to(device)
        return w

    def _mel_features(self, audio, n_mels=PERCEPTUAL_MELS):
        """ln(mel + 1e-8) [B, n_mels, T] of audio [B, 1, L]: torch.stft(1024, 256) magnitudes, summed per frame."""
        _require(audio, what="PerceptualLoss")
        from m2amd.dsp import get_dsp
        with torch.no_grad():
            y = audio.detach().float().reshape(audio.shape[0], -1)
            _, spec, _ = get_dsp(SAMPLE_RATE, PERCEPTUAL_N_FFT, PERCEPTUAL_HOP, PERCEPTUAL_N_FFT,
                                  device=y.device).loss_spectral(y, y, spectra=True)
            mag = spec.abs().sum(dim=1, keepdim=True)
            return torch.log(self.mel_weights(y.device, PERCEPTUAL_N_FFT // 2 + 1, n_mels).view(1, -1, 1) * mag + 1e-8)

    def _value(self, p: Tensor, t: Tensor, cache: Optional[dict]) -> Tensor:
        r = _spectral_rows(p, t, PERCEPTUAL_N_FFT, PERCEPTUAL_HOP, cache)
        return r["mel_log_abs"] / (r["frames"] * PERCEPTUAL_MELS)

    def forward(self, pred_audio, target_audio):
        with torch.no_grad():
            p, t = _audio_pair(pred_audio, target_audio, "PerceptualLoss")
            value = self._value(p, t, None).float()
        if _switched(self, pred_audio):
            return _attach_spectral(value, [], pred_audio, target_audio, self._calls(p.shape))
        return value


class CombinedTTSLoss(nn.Module):
    """Combined loss of stage 2 TTS training: values, and after enable_backward() the gradient of
    the discriminator step (see the module docstring)."""

    def __init__(
        self,
        mel_loss_weight: float = 1.0,
        duration_loss_weight: float = 0.1,
        adversarial_loss_weight: float = 0.25,
        feature_matching_weight: float = 2.0,
        spectral_loss_weight: float = 1.0,
        perceptual_loss_weight: float = 0.5,
        use_discriminator: bool = True
    ):
        super().__init__()
        self.mel_loss_weight = mel_loss_weight
        self.duration_loss_weight = duration_loss_weight
        self.adversarial_loss_weight = adversarial_loss_weight
        self.feature_matching_weight = feature_matching_weight
        self.spectral_loss_weight = spectral_loss_weight
        self.perceptual_loss_weight = perceptual_loss_weight

        self.spectral_loss = SpectralLoss()
        self.perceptual_loss = PerceptualLoss()
        if use_discriminator:
            self.adversarial_loss = AdversarialLoss()
        else:
            self.adversarial_loss = None
        self.training_step = 0

    backward_enabled = False  # set by enable_backward(); a plain attribute, not in the state_dict
    _warned_partial_total = False

    def enable_backward(self, enabled: bool = True, spectral: bool = False):
        """Switch the gradients of the discriminator step and of the generator step on or off;
        ``spectral`` also switches on those of spectral_loss and perceptual_loss, which
        enable_backward() and enable_backward(False) leave off (module docstring)."""
        self.backward_enabled = bool(enabled)
        if self.adversarial_loss is not None:
            self.adversarial_loss.enable_backward(enabled)
        self.spectral_loss.enable_backward(bool(enabled) and bool(spectral))
        self.perceptual_loss.enable_backward(bool(enabled) and bool(spectral))
        return self

    def _wants_gradient(self, pred: Optional[Tensor]) -> bool:
        on = self.backward_enabled or (self.adversarial_loss is not None and
                                       self.adversarial_loss.discriminator.backward_enabled)
        return on and torch.is_grad_enabled() and pred is not None and pred.requires_grad

    @staticmethod
    def _mel_gradient(mel_pred: Tensor, mel_target: Tensor, mel_lengths) -> Tensor:
        """d _mel_loss / d mel_pred, float32 like mel_pred [B, Tp, M]: sign(pred - target) / (B M len_b)
        on the first len_b of T = min(Tp, Tt) frames with lengths, sign(pred - target) / (B T M) without."""
        B, Tp, M = mel_pred.shape
        T = min(Tp, mel_target.shape[2])
        sgn = torch.sign(mel_pred.detach()[:, :T].float() - mel_target.detach()[:, :, :T].transpose(1, 2).float())
        g = torch.zeros(B, Tp, M, device=mel_pred.device, dtype=torch.float32)
        if mel_lengths is None:
            g[:, :T] = sgn / float(B * T * M)
            return g
        n = torch.as_tensor(mel_lengths).to(mel_pred.device).reshape(-1).clamp(min=0, max=T)
        live = torch.arange(T, device=mel_pred.device)[None, :] < n[:, None]
        g[:, :T] = torch.where(live[:, :, None], sgn / (float(B * M) * n.float())[:, None, None], torch.zeros_like(sgn))
        return g

    @staticmethod
    def _duration_gradient(pred: Tensor, target: Tensor) -> Tensor:
        """d _duration_loss / d pred: 2 (p - t) / n over the broadcast pair, summed back to pred's shape."""
        p, t = torch.broadcast_tensors(pred.detach().float(), target.detach().float().to(pred.device))
        return ((p - t) * (2.0 / max(p.numel(), 1))).sum_to_size(pred.shape)

    @staticmethod
    def _mel_loss(mel_pred: Tensor, mel_target: Tensor, mel_lengths) -> Tensor:
        """mel_pred [B, Tp, M] against mel_target [B, M, Tt]: with lengths the mean over
        utterances of the L1 mean of the first min(len, Tp, Tt) frames; else the L1 mean."""
        from m2amd.dsp import eval_columns, pair_stats
        if mel_pred.dim() != 3 or mel_target.dim() != 3 or mel_pred.shape[0] != mel_target.shape[0] or \
                mel_pred.shape[2] != mel_target.shape[1]:
            raise RuntimeError(f"CombinedTTSLoss: mel_pred {tuple(mel_pred.shape)} must be [B, T, M] for mel_target "
                               f"{tuple(mel_target.shape)} [B, M, T]")
        Tp, Tt = mel_pred.shape[1], mel_target.shape[2]
        cols = None
        if mel_lengths is not None:
            T = min(Tp, Tt)
            mel_pred, mel_target = mel_pred[:, :T], mel_target[:, :, :T]
            cols = torch.as_tensor(mel_lengths).to(mel_pred.device).reshape(-1).clamp(min=0, max=T).to(torch.int32)
        elif Tp != Tt:
            raise RuntimeError(f"CombinedTTSLoss: {Tp} predicted and {Tt} target frames, and no mel_lengths")
        rows = pair_stats(mel_pred.detach(), mel_target.detach(), transposed=True, cols=cols)
        names = eval_columns("pair")
        s, n = rows[:, names.index("abs_diff")], rows[:, names.index("count")]
        return (s / n).mean() if cols is not None else s.sum() / n.sum()

    @staticmethod
    def _duration_loss(pred: Tensor, target: Tensor) -> Tensor:
        from m2amd.dsp import eval_columns, pair_stats
        p, t = torch.broadcast_tensors(pred.detach().float(), target.detach().float().to(pred.device))
        rows = pair_stats(p.reshape(1, 1, -1), t.reshape(1, 1, -1))
        names = eval_columns("pair")
        return rows[0, names.index("sq_diff")] / rows[0, names.index("count")]

    def forward(
        self,
        mel_pred: torch.Tensor,
        mel_target: torch.Tensor,
        duration_pred: torch.Tensor,
        duration_target: torch.Tensor,
        audio_pred: Optional[torch.Tensor] = None,
        audio_target: Optional[torch.Tensor] = None,
        mel_lengths: Optional[torch.Tensor] = None,
        optimize_discriminator: bool = False
    ) -> Dict[str, torch.Tensor]:
        """
        Args:
            mel_pred: predicted mel spectrogram [batch, time, mel_dim]
            mel_target: target mel spectrogram [batch, mel_dim, time]
            duration_pred, duration_target: durations [batch, text_len]
            audio_pred, audio_target: waveforms [batch, 1, audio_len]
            mel_lengths: actual mel lengths [batch]
            optimize_discriminator: compute the discriminator loss instead of the generator's

        Returns:
            the loss components by name, 0-dim float32 tensors; without a graph, except after
            enable_backward() the discriminator_loss and total_loss of a discriminator step and,
            for predictions that require grad, the generator side (module docstring)
        """
        _require(mel_pred, mel_target, duration_pred, duration_target, audio_pred, audio_target,
                 what="CombinedTTSLoss")
        step = optimize_discriminator and self.adversarial_loss is not None and \
            self.adversarial_loss.discriminator._wants_backward()
        # the gradient of each generator-side term, by name (filled below for the terms that get one)
        gen = not optimize_discriminator  # the discriminator step's other entries stay plain values
        wants = {"mel_loss": gen and self._wants_gradient(mel_pred),
                 "duration_loss": gen and self._wants_gradient(duration_pred),
                 "adversarial": gen and self._wants_gradient(audio_pred)}
        grads: Dict[str, Tuple[Tensor, Tensor]] = {}
        # the terms whose gradient is computed in backward, by name: the module behind each
        lazy = {k: m for k, m in (("spectral_loss", self.spectral_loss), ("perceptual_loss", self.perceptual_loss))
                if gen and audio_target is not None and _switched(m, audio_pred)}
        with torch.no_grad():
            v: Dict[str, Tensor] = {}  # float64 on the device
            v["mel_loss"] = self._mel_loss(mel_pred, mel_target, mel_lengths)
            v["duration_loss"] = self._duration_loss(duration_pred, duration_target)
            if wants["mel_loss"]:
                grads["mel_loss"] = (mel_pred, self._mel_gradient(mel_pred, mel_target, mel_lengths))
            if wants["duration_loss"]:
                grads["duration_loss"] = (duration_pred, self._duration_gradient(duration_pred, duration_target))
            if audio_pred is not None and audio_target is not None:
                p, t = _audio_pair(audio_pred, audio_target, "CombinedTTSLoss")
                cache: dict = {}
                v["spectral_loss"] = self.spectral_loss._value(p, t, cache)
                v["perceptual_loss"] = self.perceptual_loss._value(p, t, cache)
                if self.adversarial_loss is not None:
                    adv = self.adversarial_loss
                    real, fake = t.unsqueeze(1), p.unsqueeze(1)
                    if step:
                        v["discriminator_loss"] = adv.discriminator._step_loss(real, fake)  # float32, with a grad_fn
                    elif optimize_discriminator:
                        v["discriminator_loss"] = adv.discriminator._discriminator_value(
                            adv.discriminator._sums(real, fake))
                    else:
                        # one pass over each signal serves both terms (the reference runs fake twice)
                        if wants["adversarial"]:  # the same rows, and the weighted pair's gradient
                            c, d_fake = adv.discriminator._gen_step(real, fake, self.adversarial_loss_weight,
                                                                    self.feature_matching_weight)
                            grads["adversarial"] = (audio_pred, d_fake)
                        else:
                            c = adv.discriminator._sums(real, fake)
                        v["generator_loss"] = adv._generator(c)
                        v["feature_matching_loss"] = adv._feature_matching(c)

            weights = {"mel_loss": self.mel_loss_weight, "duration_loss": self.duration_loss_weight}
            if optimize_discriminator and "discriminator_loss" in v:
                total = v["discriminator_loss"]
            else:
                total = self.mel_loss_weight * v["mel_loss"] + self.duration_loss_weight * v["duration_loss"]
                for name, weight in (("spectral_loss", self.spectral_loss_weight),
                                     ("perceptual_loss", self.perceptual_loss_weight),
                                     ("generator_loss", self.adversarial_loss_weight),
                                     ("feature_matching_loss", self.feature_matching_weight)):
                    if name in v:
                        total = total + weight * v[name]
                        weights[name] = weight
            v["total_loss"] = total
            losses = {k: x.float() for k, x in v.items()}
            pairs = [(x, weights[k] * g) for k, (x, g) in grads.items() if k in weights and weights[k] != 0]
            if "adversarial" in grads:
                pairs.append(grads["adversarial"])
        if grads or lazy:
            for k in ("mel_loss", "duration_loss"):
                if k in grads:
                    losses[k] = _attach(losses[k], [grads[k]])
            for k, m in lazy.items():
                losses[k] = _attach_spectral(losses[k], [], audio_pred, audio_target, m._calls(p.shape))
            have = {"mel_loss": "mel_loss", "duration_loss": "duration_loss", "generator_loss": "adversarial",
                    "feature_matching_loss": "adversarial", "spectral_loss": "spectral_loss",
                    "perceptual_loss": "perceptual_loss"}
            missing = [k for k, w in weights.items() if w != 0 and have.get(k) not in grads and have.get(k) not in lazy]
            calls = spectral_backward_calls(
                p.shape[0], p.shape[1], self.spectral_loss.n_fft_list, self.spectral_loss.hop_length_factor,
                self.spectral_loss_weight if "spectral_loss" in lazy else 0.0,
                self.perceptual_loss_weight if "perceptual_loss" in lazy else 0.0) if lazy else []
            if not missing and calls:
                # the audio's kept gradient (the generator step's d_fake) is the base the calls add to
                base = grads["adversarial"][1] if "adversarial" in grads else None
                others = [pair for pair in pairs if pair[0] is not audio_pred]
                losses["total_loss"] = _attach_spectral(losses["total_loss"], others, audio_pred, audio_target, calls,
                                                        base)
            elif not missing:
                losses["total_loss"] = _attach(losses["total_loss"], pairs)
            elif not self._warned_partial_total:
                self._warned_partial_total = True
                logger.warning("CombinedTTSLoss: total_loss carries no graph: %s has no gradient here "
                               "(backward() through the other entries is available)", ", ".join(missing))
        self.training_step += 1
        return losses

    def get_discriminator_parameters(self):
        """Discriminator parameters, for a separate optimizer."""
        if self.adversarial_loss is not None:
            return self.adversarial_loss.discriminator.parameters()
        return []


class EarlyStopping:
    """Early stopping utility for training (host Python)."""

    def __init__(self, patience: int = 10000, min_delta: float = 0.001):
        self.patience = patience
        self.min_delta = min_delta
        self.best_loss = float('inf')
        self.wait = 0

    def __call__(self, val_loss: float) -> bool:
        """True if training should stop: ``patience`` calls in a row without an
        improvement of more than ``min_delta`` on the best loss."""
        if val_loss < self.best_loss - self.min_delta:
            self.best_loss = val_loss
            self.wait = 0
        else:
            self.wait += 1
        return self.wait >= self.patience
