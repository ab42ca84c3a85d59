"""Mel features and Griffin-Lim on the GPU (C ABI m2_dsp_*, csrc/audio_dsp.hip).

The reference's src/utils/audio.py:45-151 runs librosa on the CPU;
``Dsp`` runs the same algorithms on a ROCm device, batched over utterances
(tensors [B, L] of audio, [B, n_mels, T] of mel).  Like the rest of the
product path there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
import weakref
from typing import Dict, Optional, Tuple

import torch

from . import _lib
from .ops import require_device, stream_handle

Tensor = torch.Tensor


def _rows(t: Tensor, *tail: int) -> Tensor:
    """t as [B, *tail]; B may be 0, which reshape(-1, ...) cannot infer."""
    n = math.prod(tail)
    return t.reshape(t.numel() // n if n else 0, *tail)


class Dsp:
    """Tables for one (sample_rate, n_fft, hop, win_length, n_mels, fmin, fmax) on one device."""

    def __init__(self, sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=64, fmin=0.0,
                 fmax=None, device=None):
        lib = _lib.load()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        fmax = sample_rate / 2.0 if fmax is None else float(fmax)
        self.sample_rate, self.n_fft, self.hop, self.win_length, self.n_mels = (sample_rate, n_fft, hop_length,
                                                                               win_length, n_mels)
        self.F = n_fft // 2 + 1
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.m2_dsp_create(sample_rate, n_fft, hop_length, win_length, n_mels, float(fmin), fmax,
                                         stream_handle(self.device), ctypes.byref(h)), "m2_dsp_create")
        self.handle = h
        self._ws: Optional[Tensor] = None
        self._finalizer = weakref.finalize(self, lib.m2_dsp_destroy, h)

    def frames(self, L: int) -> int:
        return 1 + L // self.hop

    def _audio(self, audio: Tensor) -> Tensor:
        require_device(audio, what="m2 dsp")
        if audio.dtype != torch.float32:
            audio = audio.float()
        return _rows(audio, audio.shape[-1]).contiguous()

    def stft(self, audio: Tensor) -> Tensor:
        """librosa.stft(center=True, pad_mode='constant', window='hann') -> complex64 [B, F, T]."""
        y = self._audio(audio)
        B, L = y.shape
        out = torch.empty(B, self.frames(L), self.F, 2, device=y.device, dtype=torch.float32)
        _lib.call("m2_stft", self.handle, y.data_ptr(), B, L, out.data_ptr(), stream_handle(y.device))
        return torch.view_as_complex(out).transpose(1, 2)

    def mel_spectrogram(self, audio: Tensor) -> Tensor:
        """compute_mel_spectrogram (audio.py:45-98) per utterance -> [B, n_mels, T] in [-1, 1]."""
        y = self._audio(audio)
        B, L = y.shape
        out = torch.empty(B, self.n_mels, self.frames(L), device=y.device, dtype=torch.float32)
        _lib.call("m2_mel_spectrogram", self.handle, y.data_ptr(), B, L, out.data_ptr(), stream_handle(y.device))
        return out

    def mel_features_ragged(self, samples: Tensor, offsets=None, lengths=None, normalize: bool = True,
                            max_frames: int = 0, out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """compute_mel_spectrogram of B utterances of unequal length in one call
        (m2_mel_features_ragged), each as if featurized alone.

        ``samples``: the utterances packed back to back, a 1-D device tensor,
        float32 or int16 (PCM16, read as s / 32768).  ``offsets`` [B + 1] from 0
        or ``lengths`` [B]: host integers (a list, numpy array or CPU tensor) -
        the shapes come from them, so nothing is counted on the device.
        ``normalize``: x / max|x| per utterance when the peak is > 0
        (load_audio(normalize=True)).  ``max_frames`` > 0 stores only each
        utterance's first ``max_frames`` frames; the dB reference, the top_db
        floor and the min/max still cover all of its frames.

        -> (mel [B, n_mels, T_out] float32, frames [B] int32) on the device:
        utterance b's first frames[b] columns equal ``mel_spectrogram`` of it
        alone bit for bit, every column behind them is exactly 0.  ``out``
        ([B, n_mels, T_out], T_out at least the largest stored count) is
        written in full when given."""
        require_device(samples, what="m2 mel_features_ragged")
        if samples.dtype not in (torch.float32, torch.int16):
            raise TypeError(f"mel_features_ragged: samples must be float32 or int16, got {samples.dtype}")
        if (offsets is None) == (lengths is None):
            raise ValueError("mel_features_ragged: give offsets or lengths")
        if offsets is not None:
            off = torch.as_tensor(offsets, dtype=torch.int64).cpu().reshape(-1)
            if off.numel() < 1 or int(off[0]) != 0:
                raise ValueError("mel_features_ragged: offsets must be [B + 1], from 0")
        else:
            ln = torch.as_tensor(lengths, dtype=torch.int64).cpu().reshape(-1)
            off = torch.zeros(ln.numel() + 1, dtype=torch.int64)
            torch.cumsum(ln, 0, out=off[1:])
        off = off.contiguous()
        B = off.numel() - 1
        s = samples.reshape(-1).contiguous()
        if int(off[-1]) != s.numel():
            raise ValueError(f"mel_features_ragged: offsets end at {int(off[-1])}, {s.numel()} samples given")
        dev = s.device
        frames = torch.empty(B, dtype=torch.int32, device=dev)
        T = 1 + (off[1:] - off[:-1]) // self.hop
        keep = int((T.clamp(max=max_frames) if max_frames > 0 else T).max()) if B else 0
        if out is None:
            out = torch.empty(B, self.n_mels, keep, device=dev, dtype=torch.float32)
        else:
            require_device(out, what="m2 mel_features_ragged")
            if (out.dtype != torch.float32 or out.dim() != 3 or out.shape[:2] != (B, self.n_mels)
                    or not out.is_contiguous() or out.device != dev):
                raise ValueError(f"mel_features_ragged: out must be contiguous float32 [{B}, {self.n_mels}, T_out] "
                                 f"on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        if B == 0:
            return out, frames
        off_dev = off.to(dev)
        need = int(_lib.load().m2_mel_features_ragged_workspace_bytes(self.handle, B, s.numel()))
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.call("m2_mel_features_ragged", self.handle, s.data_ptr(), 1 if s.dtype == torch.int16 else 0,
                  off_dev.data_ptr(), ctypes.cast(off.data_ptr(), ctypes.POINTER(ctypes.c_int64)), B, int(bool(normalize)),
                  int(max_frames), out.data_ptr(), out.shape[2], frames.data_ptr(), self._ws.data_ptr(),
                  self._ws.numel(), stream_handle(dev))
        return out, frames

    def mel_to_magnitude(self, mel: Tensor, nnls_iters: int = 200) -> Tensor:
        """librosa.feature.inverse.mel_to_stft of (mel + 1) / 2 in dB (audio.py:128-132)
        -> magnitudes [B, F, T]: librosa.util.nnls's result, its L-BFGS-B's
        start max(0, pinv(W) M) where its convergence test passes there (every
        mel in the normalised range); ``nnls_iters`` projected-gradient steps
        per frame for a block that would iterate (m2_mel_to_magnitude)."""
        require_device(mel, what="m2 mel_to_magnitude")
        m = _rows(mel.float(), self.n_mels, mel.shape[-1]).contiguous()
        B, T = m.shape[0], m.shape[2]
        out = torch.empty(B, T, self.F, device=m.device, dtype=torch.float32)
        n = int(_lib.load().m2_mel_to_magnitude_workspace_bytes(self.handle, B, T))
        ws = torch.empty(max(n, 1), dtype=torch.uint8, device=m.device)
        _lib.call("m2_mel_to_magnitude", self.handle, m.data_ptr(), B, T, int(nnls_iters), out.data_ptr(),
                  ws.data_ptr(), ws.numel(), stream_handle(m.device))
        return out.transpose(1, 2)

    def random_angles(self, B: int, T: int, seed: Optional[int] = None) -> Tensor:
        """librosa griffinlim(init='random'): unit phases exp(2 pi i U[0, 1)), [B, T, F] complex64."""
        g = torch.Generator(device=self.device)
        if seed is not None:
            g.manual_seed(seed)
        else:
            g.seed()
        ph = torch.rand(B, T, self.F, generator=g, device=self.device, dtype=torch.float64) * (2 * math.pi)
        return torch.polar(torch.ones_like(ph), ph).to(torch.complex64)

    def griffin_lim(self, mel: Optional[Tensor] = None, mag: Optional[Tensor] = None,
                    init_angles: Optional[Tensor] = None, n_iter: int = 32, momentum: float = 0.99,
                    nnls_iters: int = 200, seed: Optional[int] = None) -> Tensor:
        """mel_to_audio (audio.py:101-151) from mel [B, n_mels, T] (normalised dB), or
        the bare griffinlim from magnitudes mag [B, F, T]; -> audio [B, hop (T - 1)]."""
        src = mel if mel is not None else mag
        require_device(src, what="m2 griffin_lim")
        if mel is not None:
            m = _rows(mel.float(), self.n_mels, mel.shape[-1]).contiguous()
            B, T = m.shape[0], m.shape[2]
            mg = None
        else:
            mg = _rows(mag.float(), self.F, mag.shape[-1]).transpose(1, 2).contiguous()
            B, T = mg.shape[0], mg.shape[1]
            m = None
        if init_angles is None:
            init_angles = self.random_angles(B, T, seed)
        ang = torch.view_as_real(init_angles.to(torch.complex64).reshape(B, T, self.F).contiguous()).contiguous()
        out = torch.empty(B, self.hop * (T - 1), device=src.device, dtype=torch.float32)
        need = int(_lib.load().m2_griffin_lim_workspace_bytes(self.handle, B, T))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=src.device)
        _lib.call("m2_griffin_lim", self.handle, None if m is None else m.data_ptr(),
                  None if mg is None else mg.data_ptr(), ang.data_ptr(), B, T, int(n_iter), float(momentum),
                  int(nnls_iters), out.data_ptr(), self._ws.data_ptr(), self._ws.numel(), stream_handle(src.device))
        return out

    def eval_audio(self, pred: Tensor, target: Optional[Tensor] = None) -> Tensor:
        """The sums behind estimate_mos_score (metrics.py:79-148) for pred [B, Lp]
        and target [B, Lt] (None: reference-free) -> float64 [B, K] on the
        device, columns ``eval_columns("audio")`` (m2_eval_audio)."""
        y = self._audio(pred)
        B, Lp = y.shape
        q = None
        if target is not None:
            q = self._audio(target)
            if q.shape[0] != B:
                raise ValueError(f"eval_audio: {B} predictions, {q.shape[0]} targets")
        out = torch.empty(B, len(eval_columns("audio")), device=y.device, dtype=torch.float64)
        need = int(_lib.load().m2_eval_audio_workspace_bytes(self.handle, B, Lp))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=y.device)
        _lib.call("m2_eval_audio", self.handle, y.data_ptr(), None if q is None else q.data_ptr(), B, Lp,
                  0 if q is None else q.shape[1], out.data_ptr(), ws.data_ptr(), ws.numel(), stream_handle(y.device))
        return out

    def loss_spectral(self, pred: Tensor, target: Tensor, mel_weights: Optional[Tensor] = None,
                      spectra: bool = False):
        """The sums behind SpectralLoss.stft_loss and PerceptualLoss (losses.py:21-47,
        180-205) for pred, target [B, L] under torch.stft's framing (centre,
        reflect padding) at this handle's n_fft and hop -> float64 [B, K] on the
        device, columns ``loss_columns("spectral")`` (m2_loss_spectral).  With
        ``spectra`` also the complex64 spectra [B, F, T] of pred and of target
        the sums were taken from."""
        y, q = self._audio(pred), self._audio(target)
        if y.shape != q.shape:
            raise ValueError(f"loss_spectral: pred {tuple(y.shape)} and target {tuple(q.shape)} differ")
        B, L = y.shape
        if L <= self.n_fft // 2:
            raise RuntimeError(f"loss_spectral: reflect padding of n_fft {self.n_fft} needs more than "
                               f"{self.n_fft // 2} samples, got {L}")
        w = None
        if mel_weights is not None:
            require_device(mel_weights, what="m2 dsp")
            w = mel_weights.float().contiguous()
        out = torch.empty(B, len(loss_columns("spectral")), device=y.device, dtype=torch.float64)
        sp = st = None
        if spectra:
            sp = torch.empty(B, self.frames(L), self.F, 2, device=y.device, dtype=torch.float32)
            st = torch.empty_like(sp)
        need = int(_lib.load().m2_loss_spectral_workspace_bytes(self.handle, B, L))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=y.device)
        _lib.call("m2_loss_spectral", self.handle, y.data_ptr(), q.data_ptr(), B, L,
                  None if w is None else w.data_ptr(), 0 if w is None else w.numel(), out.data_ptr(),
                  None if sp is None else sp.data_ptr(), None if st is None else st.data_ptr(), ws.data_ptr(),
                  ws.numel(), stream_handle(y.device))
        if spectra:
            return out, torch.view_as_complex(sp).transpose(1, 2), torch.view_as_complex(st).transpose(1, 2)
        return out

    def loss_spectral_backward(self, pred: Tensor, target: Tensor, mel_weights: Optional[Tensor], c_mag: float,
                               c_phase: float, c_perc: float, out: Optional[Tensor] = None,
                               accumulate: bool = False, cotangent: bool = False):
        """The gradient with respect to pred [B, L] of c_mag * mag_abs + c_phase * phase_abs +
        c_perc * mel_log_abs summed over the batch: ``loss_spectral``'s columns at this handle's
        n_fft and hop, differentiated on the spectra that call forms (m2_loss_spectral_backward).
        -> float32 [B, L] on the device; ``out`` (contiguous float32, B * L elements) is written
        and returned when given, overwritten or, with ``accumulate``, added to.  With ``cotangent``
        also the complex64 cotangent [B, F, T] of pred's spectrum, d/dRe + i d/dIm per bin.  The
        coefficients are host numbers; target gets no gradient."""
        y, q = self._audio(pred), self._audio(target)
        if y.shape != q.shape:
            raise ValueError(f"loss_spectral_backward: pred {tuple(y.shape)} and target {tuple(q.shape)} differ")
        B, L = y.shape
        if L <= self.n_fft // 2:
            raise RuntimeError(f"loss_spectral_backward: reflect padding of n_fft {self.n_fft} needs more than "
                               f"{self.n_fft // 2} samples, got {L}")
        w = None
        if mel_weights is not None:
            require_device(mel_weights, what="m2 dsp")
            w = mel_weights.float().contiguous()
        if out is None:
            if accumulate:
                raise ValueError("loss_spectral_backward: accumulate needs out")
            out = torch.empty(B, L, device=y.device, dtype=torch.float32)
        else:
            require_device(out, what="m2 dsp")
            if out.dtype != torch.float32 or out.numel() != B * L or not out.is_contiguous() or out.device != y.device:
                raise ValueError(f"loss_spectral_backward: out must be contiguous float32 of {B * L} elements on "
                                 f"{y.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        cot = torch.empty(B, self.frames(L), self.F, 2, device=y.device, dtype=torch.float32) if cotangent else None
        need = int(_lib.load().m2_loss_spectral_backward_workspace_bytes(self.handle, B, L))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=y.device)
        _lib.call("m2_loss_spectral_backward", self.handle, y.data_ptr(), q.data_ptr(), B, L,
                  None if w is None else w.data_ptr(), 0 if w is None else w.numel(), float(c_mag), float(c_phase),
                  float(c_perc), int(bool(accumulate)), out.data_ptr(), None if cot is None else cot.data_ptr(),
                  ws.data_ptr(), ws.numel(), stream_handle(y.device))
        if cotangent:
            return out, torch.view_as_complex(cot).transpose(1, 2)
        return out



_CACHE: Dict[Tuple, Dsp] = {}


def get_dsp(sample_rate=22050, n_fft=1024, hop_length=256, win_length=1024, n_mels=64, fmin=0.0, fmax=None,
            device=None) -> Dsp:
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    key = (sample_rate, n_fft, hop_length, win_length, n_mels, float(fmin), fmax, dev)
    d = _CACHE.get(key)
    if d is None:
        d = _CACHE[key] = Dsp(sample_rate, n_fft, hop_length, win_length, n_mels, fmin, fmax, dev)
    return d


_EVAL_KINDS = {"audio": 0, "pair": 1, "mcd": 2}
_EVAL_COLUMNS: Dict[str, Tuple[str, ...]] = {}
_DCT_TABLES: Dict[Tuple, Tensor] = {}


def eval_columns(kind: str) -> Tuple[str, ...]:
    """Column names of the rows of eval_audio ("audio"), pair_stats ("pair") and mcd ("mcd")."""
    cols = _EVAL_COLUMNS.get(kind)
    if cols is None:
        lib, k = _lib.load(), _EVAL_KINDS[kind]
        cols = _EVAL_COLUMNS[kind] = tuple(lib.m2_eval_column_name(k, i).decode()
                                           for i in range(lib.m2_eval_column_count(k)))
    return cols


_LOSS_KINDS = {"spectral": 0, "disc": 1}
_LOSS_COLUMNS: Dict[str, Tuple[str, ...]] = {}


def loss_columns(kind: str) -> Tuple[str, ...]:
    """Column names of the rows of Dsp.loss_spectral ("spectral") and ops.Discriminators.losses ("disc")."""
    cols = _LOSS_COLUMNS.get(kind)
    if cols is None:
        lib, k = _lib.load(), _LOSS_KINDS[kind]
        cols = _LOSS_COLUMNS[kind] = tuple(lib.m2_loss_column_name(k, i).decode()
                                           for i in range(lib.m2_loss_column_count(k)))
    return cols


def _pair(pred: Tensor, target: Tensor, cols: Optional[Tensor], what: str):
    require_device(pred, target, cols, what=what)
    t = target.float().contiguous()
    p = pred.float().contiguous()
    if t.dim() != 3 or p.dim() != 3 or p.shape[0] != t.shape[0]:
        raise ValueError(f"{what}: pred {tuple(pred.shape)} and target {tuple(target.shape)} must be [B, ., .]")
    if cols is not None:
        cols = cols.to(torch.int32).contiguous()
        if cols.numel() != t.shape[0]:
            raise ValueError(f"{what}: {cols.numel()} lengths for {t.shape[0]} utterances")
    return p, t, cols


def pair_stats(pred: Tensor, target: Tensor, transposed: bool = False, cols: Optional[Tensor] = None) -> Tensor:
    """Sums of p - t, p, t and their products per utterance (m2_eval_pair_stats):
    target [B, R, C]; pred [B, R, C], or [B, C, R] with ``transposed``; ``cols``
    [B] keeps each utterance's first columns -> float64 [B, K], ``eval_columns("pair")``."""
    p, t, cols = _pair(pred, target, cols, "m2 pair_stats")
    B, R, C = t.shape
    if tuple(p.shape) != ((B, C, R) if transposed else (B, R, C)):
        raise ValueError(f"m2 pair_stats: pred {tuple(p.shape)} does not match target {tuple(t.shape)}"
                         f"{' transposed' if transposed else ''}")
    out = torch.empty(B, len(eval_columns("pair")), device=t.device, dtype=torch.float64)
    _lib.call("m2_eval_pair_stats", p.data_ptr(), t.data_ptr(), None if cols is None else cols.data_ptr(), B, R, C,
              int(transposed), out.data_ptr(), stream_handle(t.device))
    return out


def mcd(pred: Tensor, target: Tensor, transposed: bool = False, cols: Optional[Tensor] = None) -> Tensor:
    """compute_mcd's sums (metrics.py:61-76, m2_eval_mcd): target [B, M, Tt]; pred
    [B, M, Tp], or [B, Tp, M] with ``transposed`` -> float64 [B, 2]: the sum over
    the first min(Tp, Tt, cols[b]) frames of the 13-coefficient distance, and that count."""
    p, t, cols = _pair(pred, target, cols, "m2 mcd")
    B, M, Tt = t.shape
    Tp = p.shape[1] if transposed else p.shape[2]
    if (p.shape[2] if transposed else p.shape[1]) != M:
        raise ValueError(f"m2 mcd: pred {tuple(p.shape)} does not have the target's {M} mel bands")
    key = (M, t.device)
    table = _DCT_TABLES.get(key)
    if table is None:
        lib = _lib.load()
        host = (ctypes.c_double * (lib.m2_eval_mcd_coefficients() * M))()
        _lib.check(lib.m2_eval_dct_table(M, host), "m2_eval_dct_table")
        table = _DCT_TABLES[key] = torch.tensor(list(host), dtype=torch.float64).to(t.device)
    out = torch.empty(B, len(eval_columns("mcd")), device=t.device, dtype=torch.float64)
    _lib.call("m2_eval_mcd", p.data_ptr(), t.data_ptr(), None if cols is None else cols.data_ptr(), table.data_ptr(),
              B, M, Tp, Tt, int(transposed), out.data_ptr(), stream_handle(t.device))
    return out
