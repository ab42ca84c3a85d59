"""GPU: mel features and Griffin-Lim (reference src/utils/audio.py:45-151, SURVEY
8f row f4) against the CPU restatement of librosa 0.10 in oracle/audio_oracle.py.
librosa itself is not installed here, so parity with the reference's library is
UNPINNED; these tests pin the GPU kernels to the restatement, at ONE handle
(22050 Hz, n_fft 1024, hop 256, win 1024, 64 mels, fmin 0), on batches of one
or two rows and signals several frames long whose noise floor keeps the
dynamic range under 80 dB.  The other FFT sizes, a window shorter than the
FFT, hops that do not divide n_fft, 80 and 40 bands, fmin / fmax / another
sample rate, power_to_db's clamps, signals of one frame or one sample, batched
NNLS and Griffin-Lim and the two-frame minimum are test_gpu_dsp_edges.py's,
against a float64 reference.
  STFT                fp32 rounding: within 2e-6 * 32 of the largest magnitude
  mel features        normalised log-mel within 1e-3 (max-abs, in [-1, 1] units)
  griffinlim          same magnitudes and start phases -> same audio within 1e-3
  mel_to_stft (NNLS)  librosa.util.nnls's minimiser itself (scipy L-BFGS-B on the
                      block-normalised objective stops at its start
                      max(0, pinv(W) M) for every mel in the normalised range;
                      the GPU makes that convergence test and returns the start):
                      within 1e-3 relative of the oracle, over one and two
                      1024-column blocks; outside that range (blocks L-BFGS-B
                      iterates) the objective within 2 % of L-BFGS-B's."""
import numpy as np
import pytest
import torch

import audio_oracle as ao
from conftest import golden

pytestmark = pytest.mark.gpu


def _signal(n=22050, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    s = 0.5 * np.sin(2 * np.pi * 220 * t) + 0.25 * np.sin(2 * np.pi * 3100 * t) + 0.05 * rng.standard_normal(n)
    return s.astype(np.float32)


def test_stft_matches_oracle(gpu):
    from m2amd.dsp import get_dsp
    d = get_dsp(device=gpu)
    y = np.stack([_signal(22050, 0), _signal(22050, 1)])
    S = d.stft(torch.from_numpy(y).to(gpu)).cpu().numpy()
    for b in range(2):
        ref = ao.stft(y[b], 1024, 256, 1024)
        assert S[b].shape == ref.shape == (513, 87)
        assert np.abs(S[b] - ref).max() <= 2e-6 * np.abs(ref).max() * 32


@pytest.mark.parametrize("n", [22050, 5000, 1024 * 3 + 7])
def test_mel_spectrogram_matches_oracle(gpu, n):
    from utils.audio import compute_mel_spectrogram
    y = _signal(n, 2)
    got = compute_mel_spectrogram(y)
    ref = ao.compute_mel_spectrogram(y)
    assert got.shape == ref.shape == (64, 1 + n // 256)
    assert np.abs(got - ref).max() <= 1e-3
    assert got.min() == -1.0 and abs(got.max() - 1.0) < 1e-6


def test_mel_spectrogram_of_vocoder_audio_batched(gpu):
    """The features of the reference's own audio (s1_small fixture), batched."""
    from m2amd.dsp import get_dsp
    a = golden("s1_small")["audio"][:, 0].astype(np.float32)  # [2, 64 T]
    got = get_dsp(device=gpu).mel_spectrogram(torch.from_numpy(a).to(gpu)).cpu().numpy()
    for b in range(a.shape[0]):
        assert np.abs(got[b] - ao.compute_mel_spectrogram(a[b])).max() <= 1e-3


def test_griffin_lim_same_start_matches_oracle(gpu):
    from m2amd.dsp import get_dsp
    d = get_dsp(device=gpu)
    y = _signal(8192, 3)
    S = np.abs(ao.stft(y, 1024, 256, 1024)).astype(np.float32)
    rng = np.random.default_rng(5)
    ang = np.exp(2j * np.pi * rng.random(S.shape)).astype(np.complex64)
    for n_iter in (0, 1, 8):
        ref = ao.griffin_lim(S, ang, n_iter, 1024, 256, 1024)
        got = d.griffin_lim(mag=torch.from_numpy(S)[None].to(gpu),
                            init_angles=torch.from_numpy(ang.T.copy())[None].to(gpu), n_iter=n_iter).cpu().numpy()[0]
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-3 * np.abs(ref).max(), n_iter


@pytest.mark.parametrize("case", ["features", "normal3", "two_blocks"])
def test_mel_to_magnitude_is_librosa_minimiser(gpu, case):
    """GPU mel_to_stft = sqrt(librosa.util.nnls(W, M)) within 1e-3 relative:
    the oracle's scipy L-BFGS-B returns its start (nit 0) on these blocks."""
    from m2amd.dsp import get_dsp
    rng = np.random.default_rng(3)
    if case == "features":
        mel = ao.compute_mel_spectrogram(_signal(22050, 4))
    elif case == "normal3":  # far wider than the normalised range, still nit 0
        mel = (rng.standard_normal((64, 300)) * 3).astype(np.float32)
    else:  # 1500 frames: blocks [0, 1024) and [1024, 1500), each its own L-BFGS-B problem
        mel = rng.uniform(-1, 1, (64, 1500)).astype(np.float32)
    d = get_dsp(device=gpu)
    mag = d.mel_to_magnitude(torch.from_numpy(mel).to(gpu)).cpu().numpy()[0]
    W = ao.mel_filterbank(22050, 1024, 64, 0, 11025.0)
    M = np.power(10.0, 0.1 * (mel + 1) / 2).astype(np.float32)
    X_ref, info = ao.nnls_lbfgs(W, M, return_info=True)
    assert all(nit == 0 for nit, _ in info), info
    S_ref = np.sqrt(X_ref)
    assert mag.shape == S_ref.shape
    assert np.abs(mag - S_ref).max() <= 1e-3 * np.abs(S_ref).max(), np.abs(mag - S_ref).max() / np.abs(S_ref).max()


def test_mel_to_magnitude_iterating_block(gpu):
    """A mel far outside the normalised range (std 20): L-BFGS-B iterates from
    its start; the GPU's per-frame projected gradient reaches an NNLS
    objective within 2 % of L-BFGS-B's (a different minimiser of the
    under-determined system: 64 equations, 513 unknowns per frame)."""
    from m2amd.dsp import get_dsp
    mel = (np.random.default_rng(8).standard_normal((64, 100)) * 20).astype(np.float32)
    d = get_dsp(device=gpu)
    mag = d.mel_to_magnitude(torch.from_numpy(mel).to(gpu), nnls_iters=400).cpu().numpy()[0]
    W = ao.mel_filterbank(22050, 1024, 64, 0, 11025.0)
    M = np.power(10.0, 0.1 * (mel + 1) / 2).astype(np.float32)
    X_ref, info = ao.nnls_lbfgs(W, M, return_info=True)
    assert info[0][0] > 0
    obj_gpu, obj_ref = ao.nnls_objective(W, mag.astype(np.float64) ** 2, M), ao.nnls_objective(W, X_ref, M)
    assert (mag >= 0).all()
    assert obj_gpu <= 1.02 * obj_ref + 1e-9 * float(np.sum(M.astype(np.float64) ** 2)), (obj_gpu, obj_ref)


def test_mel_to_audio_pipeline(gpu):
    """mel_to_audio (audio.py:101-151) from the same start phases as the
    oracle's full chain (its NNLS included), peak-normalised: within 2e-3."""
    from utils.audio import mel_to_audio
    mel = ao.compute_mel_spectrogram(_signal(22050, 4))
    rng = np.random.default_rng(9)
    T = mel.shape[1]
    ang = np.exp(2j * np.pi * rng.random((513, T))).astype(np.complex64)
    got = mel_to_audio(mel, init_angles=torch.from_numpy(ang.T.copy())[None].to(gpu))
    ref, _ = ao.mel_to_audio(mel, ang)
    assert got.shape == ref.shape == (256 * 86,)
    assert abs(np.abs(got).max() - 1.0) < 1e-6
    assert np.abs(got - ref).max() <= 2e-3, np.abs(got - ref).max()
    # seeded random start: reproducible
    a1 = mel_to_audio(mel, seed=7)
    a2 = mel_to_audio(mel, seed=7)
    assert np.array_equal(a1, a2)
