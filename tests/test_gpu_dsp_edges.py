"""GPU: the audio DSP kernels (csrc/audio_dsp.hip) away from the default handle
and the single utterance of test_gpu_audio_features.py, against the float64
counterparts of the oracle (oracle/audio_oracle.py, dtype=np.float64; pinned to
the float32 restatement in test_audio_oracle.py).  Configurations 1..6 are
audio_cases.CONFIGS (sr, n_fft, hop, win, n_mels, fmin, fmax):
  1  22050 1024 256 1024 80  0 11025     4  22050 1024 200  800 64 50  8000
  2  22050  512 128  512 40  0 11025     5  16000  512 160  400 40 20  7600
  3  22050 2048 512 2048 80  0 11025     6  22050 2048 300 1200 80  0 11025
and audio_cases.GAP_CONFIG (22050 512 256 200 40 0 11025) is one more for
Griffin-Lim: its hop exceeds its window, so output samples have a
window-sum-square of 0 and ola_kernel leaves them undivided.

No bound is looser than test_gpu_audio_features.py's for the same quantity:
  STFT           2e-6 * 32 of the largest reference magnitude
  mel features   1e-3 max-abs; where the float32 restatement is itself further
                 than 1e-4 from float64, ten times that distance: one_sample at
                 configuration 3 (distance 1.2e-4, bound 1.2e-3) and at
                 configuration 6 (1.5e-4, 1.5e-3), nowhere else
  NNLS           1e-3 of the largest sqrt of the oracle's minimiser (nit 0)
  Griffin-Lim    1e-3 of the reference's peak
  mel_to_audio   2e-3
  batch rows     bit for bit the single-utterance calls

Each test prints its largest error as "DSPEDGE <quantity> <configuration>
<value>" before it asserts (pytest -s shows them; DESIGN 4.6 has one run's)."""
import numpy as np
import pytest
import torch

import audio_cases as ac
import audio_oracle as ao

pytestmark = pytest.mark.gpu

CFG = ac.CONFIGS


def _cfgs(*numbers):
    return pytest.mark.parametrize("cfg", [CFG[i - 1] for i in numbers], ids=ac.config_id)


def _dsp(cfg, gpu):
    from m2amd.dsp import get_dsp
    sr, n_fft, hop, win, n_mels, fmin, fmax = cfg
    return get_dsp(sr, n_fft, hop, win, n_mels, fmin, fmax, gpu)


def _report(quantity, cfg, value):
    print(f"DSPEDGE {quantity} {ac.config_id(cfg)} {value:.3e}")


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _angles(ang, gpu):
    """[B, F, T] complex64 -> the [B, T, F] device tensor griffin_lim takes."""
    return _dev(np.ascontiguousarray(np.swapaxes(ang, 1, 2)), gpu)


# ------------------------------------------------------------------ a. STFT
@_cfgs(1, 2, 3, 4, 5, 6)
def test_stft_matches_float64(gpu, cfg):
    """Three distinct signals per call at one sample, around hop, n_fft / 2
    and n_fft, and several frames: shape (F, 1 + L // hop), error within the
    existing test's 2e-6 * 32 of the largest reference magnitude."""
    _, n_fft, hop, win = cfg[:4]
    d = _dsp(cfg, gpu)
    worst = 0.0
    for L in ac.stft_lengths(cfg):
        y = np.stack([ac.tone_noise(L, 10 + b, 1.0 + b) for b in range(3)])
        S = d.stft(_dev(y, gpu)).cpu().numpy()
        assert S.shape == (3, n_fft // 2 + 1, 1 + L // hop), L
        for b in range(3):
            ref = ao.stft(y[b], n_fft, hop, win, dtype=np.float64)
            assert S[b].shape == ref.shape
            err, top = np.abs(S[b] - ref).max(), np.abs(ref).max()
            assert top > 0
            worst = max(worst, err / top)
            assert err <= 2e-6 * top * 32, (L, b, err / top)
    _report("stft", cfg, worst)


# ---------------------------------------------------------- b. mel features
@pytest.mark.parametrize("name", list(ac.MEL_SIGNALS))
@_cfgs(1, 2, 3, 4, 5, 6)
def test_mel_features_match_float64(gpu, cfg, name):
    """AudioProcessor.compute_mel_spectrogram against the float64 reference:
    1e-3 max-abs, or ten times the float32 restatement's own distance where
    that exceeds 1e-4 (audio_cases.mel_bound; one_sample at configurations 3
    and 6, see the module docstring).  The clamp cases first show on the
    reference that their clamp binds."""
    from utils.audio import AudioProcessor
    sr, n_fft, hop, win, n_mels, fmin, fmax = cfg
    y = ac.mel_signal(name, cfg)
    P, db, ref = ac.mel_reference(y, cfg)
    floor_hits = int((db == db.max() - ao.TOP_DB).sum())
    amin_hits = int((P < ao.AMIN).sum())
    if ac.MEL_SIGNALS[name] == "floor":  # top_db binds
        assert floor_hits > 0
    if ac.MEL_SIGNALS[name] == "amin":   # amin binds on powers, not on ref, and its level is above the floor
        level = 10.0 * np.log10(ao.AMIN) - 10.0 * np.log10(P.max())
        assert amin_hits > 0 and P.max() > ao.AMIN and level > db.max() - ao.TOP_DB
        assert int((db == level).sum()) == amin_hits and floor_hits == 0
    bound, d32 = ac.mel_bound(y, cfg)
    assert bound == 1e-3 or (name == "one_sample" and n_fft == 2048 and bound == 10.0 * d32 <= 1.6e-3)
    got = AudioProcessor(sr, n_fft, hop, win, n_mels, fmin, fmax).compute_mel_spectrogram(y)
    assert got.dtype == np.float32 and got.shape == ref.shape == (n_mels, 1 + len(y) // hop)
    err = np.abs(got - ref).max()
    _report("mel:" + name, cfg, err)
    assert err <= bound, (err, bound, d32)
    assert got.min() == -1.0 and abs(got.max() - 1.0) < 1e-6


# ----------------------------------------------------- c. degenerate inputs
@_cfgs(1, 2, 3, 4, 5, 6)
def test_degenerate_mel_is_nan_like_the_reference(gpu, cfg):
    """Silence, and (at n_fft 512) two tones scaled by 1e-6 so that every mel
    power is below amin: the reference's normalisation divides 0 by 0 and
    returns NaN throughout; so does the float64 oracle, and so must the GPU."""
    from utils.audio import compute_mel_spectrogram
    sr, n_fft, hop, win, n_mels, fmin, fmax = cfg
    signals = [np.zeros(3 * n_fft, np.float32)]
    if n_fft == 512:
        signals.append(ac.two_tone(3 * n_fft, 1e-6))
    for y in signals:
        P, _, ref = ac.mel_reference(y, cfg)
        assert P.max() < ao.AMIN and np.isnan(ref).all()
        got = compute_mel_spectrogram(y, sr, n_fft, hop, win, n_mels, fmin, fmax)
        assert got.shape == ref.shape
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(got, ref.astype(np.float32), equal_nan=True)


# ------------------------------------------------------ d. row independence
def _assert_rows_equal(batched, singles, what):
    assert batched.shape[0] == len(singles)
    for b, one in enumerate(singles):
        assert one.shape[0] == 1 and torch.equal(batched[b], one[0]), (what, b)


@_cfgs(1, 2, 4)
def test_batch_rows_equal_single_calls_bit_for_bit(gpu, cfg):
    """B = 4 distinct rows at four scales (so db_norm_kernel and
    peak_norm_kernel cannot borrow a neighbour's extremum) equal the four
    B = 1 calls exactly: every workgroup handles one (frame, utterance) pair
    or one utterance in a fixed order.  The NNLS rows span a block edge of
    librosa's column blocking (819 / 1638 / 1024 columns)."""
    sr, n_fft, hop, win, n_mels, fmin, fmax = cfg
    d = _dsp(cfg, gpu)
    scales = (1.0, 0.03, 7.0, 1e-3)
    y = _dev(np.stack([ac.tone_noise(3 * n_fft + 7, 20 + b, s) for b, s in enumerate(scales)]), gpu)
    S = d.stft(y)
    _assert_rows_equal(torch.view_as_real(S.contiguous()),
                       [torch.view_as_real(d.stft(y[b:b + 1]).contiguous()) for b in range(4)], "stft")
    _assert_rows_equal(d.mel_spectrogram(y), [d.mel_spectrogram(y[b:b + 1]) for b in range(4)], "mel_spectrogram")

    rng = np.random.default_rng(21)
    T = (256 * 1024) // (4 * n_mels) + 12
    mel = _dev((rng.uniform(-1, 1, (4, n_mels, T)) * np.array([1.0, 0.5, 0.25, 0.8])[:, None, None]).astype(np.float32),
               gpu)
    _assert_rows_equal(d.mel_to_magnitude(mel), [d.mel_to_magnitude(mel[b:b + 1]) for b in range(4)],
                       "mel_to_magnitude")

    mag, ang = ac.griffin_inputs(cfg, 4096, 22, B=4)
    mag, ang = _dev(mag, gpu), _angles(ang, gpu)
    got = d.griffin_lim(mag=mag, init_angles=ang, n_iter=3)
    _assert_rows_equal(got, [d.griffin_lim(mag=mag[b:b + 1], init_angles=ang[b:b + 1], n_iter=3) for b in range(4)],
                       "griffin_lim(mag)")
    assert float(got.abs().max()) > 0
    Tm = mag.shape[2]
    got = d.griffin_lim(mel=mel[:, :, :Tm], init_angles=ang, n_iter=3)
    _assert_rows_equal(got, [d.griffin_lim(mel=mel[b:b + 1, :, :Tm], init_angles=ang[b:b + 1], n_iter=3)
                             for b in range(4)], "griffin_lim(mel)")
    assert torch.equal(got.abs().amax(1), torch.ones(4, device=gpu))  # each row normalised by its own peak


# ---------------------------------------------------------------- e. NNLS
@pytest.mark.parametrize("number,B,T", [(1, 2, 830), (2, 1, 1650), (3, 1, 40), (5, 1, 40)],
                         ids=lambda v: str(v))
def test_mel_to_magnitude_is_librosa_minimiser(gpu, number, B, T):
    """sqrt(librosa.util.nnls(W, M)) at 80 and 40 bands within 1e-3 relative:
    across the 819-column block edge at configuration 1 (two rows) and the
    1638-column edge at configuration 2; the oracle's L-BFGS-B returns its
    start (nit 0) on every block."""
    cfg = CFG[number - 1]
    sr, n_fft, hop, win, n_mels, fmin, fmax = cfg
    rng = np.random.default_rng(30 + number)
    mel = rng.uniform(-1, 1, (B, n_mels, T)).astype(np.float32)
    W = ao.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    mag = _dsp(cfg, gpu).mel_to_magnitude(_dev(mel, gpu)).cpu().numpy()
    assert mag.shape == (B, n_fft // 2 + 1, T)
    worst = 0.0
    for b in range(B):
        M = np.power(10.0, 0.1 * (mel[b] + 1) / 2).astype(np.float32)
        X_ref, info = ao.nnls_lbfgs(W, M, return_info=True)
        assert len(info) == -(-T // ao.nnls_block_columns(W, M)) and all(nit == 0 for nit, _ in info), info
        S_ref = np.sqrt(X_ref)
        err = np.abs(mag[b] - S_ref).max() / np.abs(S_ref).max()
        worst = max(worst, err)
        assert err <= 1e-3, (b, err)
    _report("nnls", cfg, worst)


# ---------------------------------------------------------- f. Griffin-Lim
@pytest.mark.parametrize("cfg", [CFG[1], CFG[2], CFG[3], CFG[5], ac.GAP_CONFIG], ids=ac.config_id)
def test_griffin_lim_matches_float64(gpu, cfg):
    """Given magnitudes and start phases, B = 2, T from 4096 samples and the
    minimum T = 2, n_iter 0, 1 and 8, against the float64 griffin_lim within
    1e-3 of its peak.  Configuration 4's window (800 of 1024) has zero flanks:
    the reference's overlap-add has samples with a window-sum-square at or
    below tiny, but with hop 200 < 800 all of them lie in the trimmed centre
    padding, so ola_kernel, which computes the kept samples only, never meets
    one there; at the gap configuration (hop 256 > win 200) kept samples have
    one, and the undivided overlap-add there is exactly 0."""
    _, n_fft, hop, win = cfg[:4]
    d = _dsp(cfg, gpu)
    tiny = np.finfo(np.float32).tiny
    worst = 0.0
    for T_from in (4096, hop):
        S, ang = ac.griffin_inputs(cfg, T_from, 3)
        T = S.shape[2]
        assert T == (2 if T_from == hop else 1 + 4096 // hop)
        wss = ao.window_sumsquare(T, n_fft, hop, win, np.float64)
        kept = wss[n_fft // 2:n_fft // 2 + hop * (T - 1)]
        if win < n_fft:
            assert (wss <= tiny).any()
        if cfg == ac.GAP_CONFIG:
            assert (kept <= tiny).any()
        for n_iter in (0, 1, 8):
            got = d.griffin_lim(mag=_dev(S, gpu), init_angles=_angles(ang, gpu), n_iter=n_iter).cpu().numpy()
            assert got.shape == (2, hop * (T - 1))
            for b in range(2):
                ref = ao.griffin_lim(S[b], ang[b], n_iter, n_fft, hop, win, dtype=np.float64)
                err = np.abs(got[b] - ref).max() / np.abs(ref).max()
                worst = max(worst, err)
                assert err <= 1e-3, (T, n_iter, b, err)
                assert (got[b][kept <= tiny] == 0).all() and (ref[kept <= tiny] == 0).all()
    _report("griffin_lim", cfg, worst)


# --------------------------------------------------------- g. mel_to_audio
def test_mel_to_audio_80_mels_batched(gpu):
    """utils.audio.mel_to_audio on a [2, 80, T] mel from given phases: each
    row within 2e-3 of the oracle's chain (its NNLS included), and bit for
    bit its single-mel call."""
    from utils.audio import mel_to_audio
    mel = np.stack([ao.compute_mel_spectrogram(ac.tone_noise(8192, 40 + b, 1.0 + 3 * b), n_mels=80) for b in range(2)])
    T = mel.shape[2]
    assert mel.shape == (2, 80, 33)
    ang = np.exp(2j * np.pi * np.random.default_rng(41).random((2, 513, T))).astype(np.complex64)
    dev_ang = _angles(ang, gpu)
    got = mel_to_audio(mel, init_angles=dev_ang)
    assert got.shape == (2, 256 * (T - 1))
    for b in range(2):
        ref, _ = ao.mel_to_audio(mel[b], ang[b], n_mels=80)
        assert abs(np.abs(got[b]).max() - 1.0) < 1e-6
        err = np.abs(got[b] - ref).max()
        _report("mel_to_audio", CFG[0], err)
        assert err <= 2e-3, (b, err)
        one = mel_to_audio(mel[b], init_angles=dev_ang[b:b + 1])
        assert one.shape == got[b].shape and np.array_equal(one, got[b]), b


# --------------------------------------------------------------- h. contract
def test_contract_errors_and_empty_batch(gpu):
    """Bad configurations and shapes are refused by the host checks (status
    and message of the library, or require_device) before any launch; B = 0
    returns empty results."""
    from m2amd._lib import M2_E_SHAPE, M2Error
    from m2amd.dsp import Dsp
    with pytest.raises(M2Error, match="n_fft must be 512, 1024 or 2048") as e:
        Dsp(n_fft=4096, hop_length=1024, win_length=4096, device=gpu)
    assert e.value.status == M2_E_SHAPE
    with pytest.raises(M2Error, match="m2_dsp_create: bad argument"):
        Dsp(n_fft=1024, win_length=1025, device=gpu)
    d = _dsp(CFG[1], gpu)
    F, n_mels = d.F, d.n_mels
    with pytest.raises(M2Error, match="m2_stft: bad argument"):
        d.stft(torch.zeros(2, 0, device=gpu))
    with pytest.raises(M2Error, match="m2_mel_spectrogram: bad argument"):
        d.mel_spectrogram(torch.zeros(2, 0, device=gpu))
    ang1 = torch.ones(1, 1, F, dtype=torch.complex64, device=gpu)
    with pytest.raises(M2Error, match="at least 2 frames") as e:
        d.griffin_lim(mag=torch.ones(1, F, 1, device=gpu), init_angles=ang1)
    assert e.value.status == M2_E_SHAPE
    with pytest.raises(M2Error, match="at least 2 frames"):
        d.griffin_lim(mel=torch.zeros(1, n_mels, 1, device=gpu), init_angles=ang1)
    for call in (lambda: d.stft(torch.zeros(1, 100)), lambda: d.mel_spectrogram(torch.zeros(1, 100)),
                 lambda: d.mel_to_magnitude(torch.zeros(1, n_mels, 4)),
                 lambda: d.griffin_lim(mag=torch.ones(1, F, 4), init_angles=torch.ones(1, 4, F, dtype=torch.complex64))):
        with pytest.raises(RuntimeError, match="must be on a ROCm GPU"):
            call()
    assert tuple(d.stft(torch.zeros(0, 300, device=gpu)).shape) == (0, F, 1 + 300 // d.hop)
    assert tuple(d.mel_spectrogram(torch.zeros(0, 300, device=gpu)).shape) == (0, n_mels, 1 + 300 // d.hop)
    assert tuple(d.mel_to_magnitude(torch.zeros(0, n_mels, 5, device=gpu)).shape) == (0, F, 5)
    assert tuple(d.griffin_lim(mag=torch.zeros(0, F, 5, device=gpu)).shape) == (0, d.hop * 4)
    assert tuple(d.griffin_lim(mel=torch.zeros(0, n_mels, 5, device=gpu), seed=1).shape) == (0, d.hop * 4)
