"""Oracle of the gradient of the spectral and perceptual losses (numpy / torch on the CPU).

For one n_fft = N and hop, P and T the one-sided spectra [B, F, frames] of pred and target under
torch.stft(center=True, pad_mode='reflect', periodic Hann), S_X(t) = sum_f |X_f(t)|:

    objective = c_mag  sum | |P| - |T| |  +  c_ph sum |angle P - angle T|
              + c_perc sum_t sum_j |ln(w_j S_P(t) + 1e-8) - ln(w_j S_T(t) + 1e-8)|

Three things, each on its own:

  cotangent   the closed form of g = d/dRe P + i d/dIm P on given spectra, float64;
  adjoint     the adjoint of the framing: the unnormalised one-sided inverse transform, the window,
              overlap-add and the adjoint of reflect padding, float64;
  objective   the formula over torch.stft in a chosen dtype, with every |.| either itself or, with
              prescribed signs s, s * (.), whose gradient is s times the inner derivative whatever
              side of 0 the argument fell on; `gradient` differentiates it by autograd.

Only pred is differentiated; sign(0) = 0, and every term is 0 where |P| = 0 (torch's abs and angle
backward).
"""
import numpy as np
import torch

N_MELS = 80


def mel_weights(freq_bins, n_mels=N_MELS):
    """PerceptualLoss's constant filter rows, float32, by the reference's expressions; w_0 = 0."""
    f = torch.linspace(0, 1, n_mels, dtype=torch.float32).unsqueeze(1).expand(n_mels, freq_bins)
    f = f / (f.sum(dim=1, keepdim=True) + 1e-8)
    return f[:, 0].contiguous()


def coefficients(B, L, n_fft, hop, n_sizes=3, n_mels=N_MELS):
    """(c_mag, c_phase, c_perc) that make the objective SpectralLoss's share of one size (the mean over
    B F frames bins, averaged over n_sizes) and PerceptualLoss's mean over B n_mels frames."""
    frames = 1 + L // hop
    c_mag = 1.0 / (n_sizes * B * (n_fft // 2 + 1) * frames)
    return c_mag, 0.1 * c_mag, 1.0 / (B * n_mels * frames)


def stft(x, n_fft, hop):
    """x [B, L] (torch, float32 or float64) -> complex [B, F, frames] in x's precision."""
    win = torch.hann_window(n_fft, periodic=True, dtype=x.dtype)
    return torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=win, center=True, pad_mode="reflect",
                      return_complex=True)


def _abs(X):
    """sqrt(re^2 + im^2): exact products of float32 values in float64, two roundings."""
    return np.sqrt(X.real * X.real + X.imag * X.imag)


def signs_of(P, T, w):
    """The three sign arrays of the objective on spectra P, T (numpy complex [B, F, frames], taken to
    float64): sign(|P| - |T|) and sign(angle P - angle T) [B, F, frames], and
    sign(ln(w_j S_P + 1e-8) - ln(w_j S_T + 1e-8)) [B, len(w), frames]."""
    P, T = np.asarray(P).astype(np.complex128), np.asarray(T).astype(np.complex128)
    w = np.asarray(w, dtype=np.float64).reshape(1, -1, 1)
    mp, mt = _abs(P), _abs(T)
    sP, sT = mp.sum(axis=1, keepdims=True), mt.sum(axis=1, keepdims=True)
    return (np.sign(mp - mt), np.sign(np.arctan2(P.imag, P.real) - np.arctan2(T.imag, T.real)),
            np.sign(np.log(w * sP + 1e-8) - np.log(w * sT + 1e-8)))


def cotangent(P, T, w, c_mag, c_ph, c_perc, signs=None):
    """g [B, F, frames] complex128, the closed form on spectra P, T; `signs` as signs_of returns
    them (None: the spectra's own)."""
    P, T = np.asarray(P).astype(np.complex128), np.asarray(T).astype(np.complex128)
    sm, sa, sp = signs_of(P, T, w) if signs is None else signs
    w = np.asarray(w, dtype=np.float64).reshape(1, -1, 1)
    mp = _abs(P)
    sP = mp.sum(axis=1, keepdims=True)
    kappa = c_perc * (sp * w / (w * sP + 1e-8)).sum(axis=1, keepdims=True)  # [B, 1, frames]
    live = mp > 0
    safe = np.where(live, mp, 1.0)
    radial = (c_mag * sm + kappa) / safe
    turn = c_ph * sa / (safe * safe)
    g = radial * P + turn * (-P.imag + 1j * P.real)
    return np.where(live, g, 0.0)


def adjoint(g, n_fft, hop, L):
    """d_pred [B, L] float64 from the cotangent g [B, F, frames] of the spectrum: frame t's samples are
    win[n] Re sum_{f <= N/2} g_f e^(+2 pi i f n / N), added at offset t hop - N/2; then the adjoint of
    reflect padding: sample i receives padded positions i, -i and 2 (L - 1) - i."""
    g = np.asarray(g).astype(np.complex128)
    B, F, frames = g.shape
    N = n_fft
    assert F == N // 2 + 1 and frames == 1 + L // hop and L > N // 2
    full = np.zeros((B, N, frames), dtype=np.complex128)
    full[:, :F] = g
    win = torch.hann_window(N, periodic=True, dtype=torch.float64).numpy()
    y = (np.fft.ifft(full, axis=1) * N).real * win[None, :, None]  # [B, N, frames]
    padded = np.zeros((B, L + N), dtype=np.float64)  # padded position p at index p + N/2
    for t in range(frames):
        padded[:, t * hop:t * hop + N] += y[:, :, t]
    h = N // 2
    out = padded[:, h:h + L].copy()
    i = np.arange(1, h + 1)
    out[:, i] += padded[:, h - i]
    i = np.arange(L - 1 - h, L - 1)
    out[:, i] += padded[:, h + 2 * (L - 1) - i]
    return out


def objective(pred, target, n_fft, hop, w, c_mag, c_ph, c_perc, signs=None):
    """The objective over torch.stft in pred's dtype (torch tensors [B, L]; target a constant).
    `signs` (numpy arrays as signs_of returns them, or None: plain abs) are cast to that dtype."""
    P = stft(pred, n_fft, hop)
    with torch.no_grad():
        T = stft(target.to(pred.dtype), n_fft, hop)
    w = torch.as_tensor(np.asarray(w, dtype=np.float64)).to(pred.dtype).reshape(1, -1, 1)
    mp, mt = P.abs(), T.abs()
    d_mag, d_ang = mp - mt, P.angle() - T.angle()
    d_log = torch.log(w * mp.sum(dim=1, keepdim=True) + 1e-8) - torch.log(w * mt.sum(dim=1, keepdim=True) + 1e-8)
    if signs is None:
        terms = (d_mag.abs(), d_ang.abs(), d_log.abs())
    else:
        terms = tuple(d * torch.as_tensor(s).to(pred.dtype) for d, s in zip((d_mag, d_ang, d_log), signs))
    return c_mag * terms[0].sum() + c_ph * terms[1].sum() + c_perc * terms[2].sum()


def gradient(pred, target, n_fft, hop, w, c_mag, c_ph, c_perc, signs=None):
    """d objective / d pred by autograd, detached, in pred's dtype."""
    x = pred.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(objective(x, target, n_fft, hop, w, c_mag, c_ph, c_perc, signs), x)
    return g
