"""CPU checks of the librosa-0.10 restatement used as the f4 checker
(oracle/audio_oracle.py).  librosa is not installed, so these pin the
restatement to the published algorithm's known properties instead:
perfect reconstruction of the Hann/hop-256 STFT (COLA), the Slaney mel
scale's anchor points and the area normalisation of the filters, a pure tone
landing in the band that contains it, power_to_db's floor."""
import numpy as np
import pytest

import audio_cases as ac
import audio_oracle as ao


def test_stft_istft_roundtrip():
    x = np.random.default_rng(0).standard_normal(10000).astype(np.float32)
    S = ao.stft(x, 1024, 256, 1024)
    assert S.shape == (513, 1 + 10000 // 256)
    y = ao.istft(S, 1024, 256, 1024)
    assert len(y) == 256 * (S.shape[1] - 1)
    assert np.abs(y - x[:len(y)]).max() < 2e-6


def test_stft_matches_direct_dft():
    x = np.random.default_rng(1).standard_normal(3000).astype(np.float32)
    S = ao.stft(x, 512, 128, 512)
    w = ao.hann_periodic(512).astype(np.float64)
    xp = np.pad(x, 256).astype(np.float64)
    t = 5
    frame = xp[t * 128:t * 128 + 512] * w
    k = np.arange(257)[:, None]
    n = np.arange(512)[None, :]
    ref = (frame[None, :] * np.exp(-2j * np.pi * k * n / 512)).sum(1)
    assert np.abs(S[:, t] - ref).max() < 1e-4


def test_slaney_mel_scale_and_filters():
    assert abs(ao.hz_to_mel(1000.0) - 15.0) < 1e-12           # linear part: 1000 / (200/3)
    assert abs(ao.mel_to_hz(ao.hz_to_mel(4321.0)) - 4321.0) < 1e-9
    W = ao.mel_filterbank(22050, 1024, 64, 0, 11025)
    assert W.shape == (64, 513) and (W >= 0).all()
    # slaney norm: each triangle has area 1 in Hz (weights * bin spacing summed ~ 1)
    df = 22050 / 1024
    areas = W.sum(1) * df
    assert np.all(np.abs(areas[8:] - 1) < 0.05)


def test_tone_lands_in_its_band_and_db_floor():
    t = np.arange(22050) / 22050
    for f in (300.0, 2500.0):
        y = np.sin(2 * np.pi * f * t).astype(np.float32)
        mel = ao.compute_mel_spectrogram(y)
        band = int(np.argmax(mel[:, 40]))
        edges = ao.mel_to_hz(np.linspace(ao.hz_to_mel(0), ao.hz_to_mel(11025), 66))
        assert edges[band] <= f <= edges[band + 2]
    db = ao.power_to_db(np.array([[1.0, 1e-12, 1e-3]], dtype=np.float32))
    assert db.max() == 0.0 and db.min() == -80.0 and abs(db[0, 2] + 30.0) < 1e-4


def test_nnls_restatement_blocks_and_start():
    """librosa.util.nnls restated: 1024-column blocks for 64 float32 bands,
    each an L-BFGS-B problem on the block-normalised objective; in the
    normalised mel range its convergence test passes at the clipped-pinv
    start, so the result IS that start (what the GPU reproduces)."""
    A = ao.mel_filterbank(22050, 1024, 64, 0, 11025.0)
    rng = np.random.default_rng(2)
    mel = rng.uniform(-1, 1, (64, 1100)).astype(np.float32)
    M = np.power(10.0, 0.1 * (mel + 1) / 2).astype(np.float32)
    assert ao.nnls_block_columns(A, M) == 1024
    X, info = ao.nnls_lbfgs(A, M, return_info=True)
    assert len(info) == 2 and all(nit == 0 for nit, _ in info)
    X0 = np.clip(np.linalg.pinv(A) @ M, 0, None)
    assert np.array_equal(X, X0.astype(np.float32))
    assert ao.nnls_projected_gradient_norm(A, X0[:, :1024], M[:, :1024]) <= 1e-5
    # far outside the range the start is not stationary and L-BFGS-B iterates
    big = (rng.standard_normal((64, 40)) * 20).astype(np.float32)
    Mb = np.power(10.0, 0.1 * (big + 1) / 2).astype(np.float32)
    Xb, ib = ao.nnls_lbfgs(A, Mb, return_info=True)
    assert ib[0][0] > 0
    assert ao.nnls_objective(A, Xb, Mb) < ao.nnls_objective(A, np.clip(np.linalg.pinv(A) @ Mb, 0, None), Mb)


# ---------------------------------------------------------------------------
# The float32 restatement against its float64 counterpart (dtype=np.float64:
# the same operations, nothing rounded below double) at the configurations
# and signals of tests/test_gpu_dsp_edges.py, which holds the kernels to the
# float64 one.  Each pin is one tenth of the bound the GPU test sets for the
# quantity, so that bound leaves a factor of ten over an implementation of
# the arithmetic the kernel is allowed.
ALL_CONFIGS = ac.CONFIGS + [ac.GAP_CONFIG]
# normalised features further than 1e-4 from float64: a single sample has a
# flat spectrum, so the bands differ by their filter sums alone and the
# [-1, 1] normalisation stretches a dB range of well under 1 dB
MEL_PIN_EXCEPTIONS = {(ac.CONFIGS[2], "one_sample"): 1.2e-4, (ac.CONFIGS[5], "one_sample"): 1.5e-4}


@pytest.mark.parametrize("cfg", ALL_CONFIGS, ids=ac.config_id)
def test_float32_stft_and_istft_pinned_to_float64(cfg):
    """Largest distances over the seven configurations, relative to the
    float64 result's largest magnitude: stft 5.5e-8 (pin 6.4e-6, a tenth of
    the GPU test's 2e-6 * 32); istft of the float64 spectrum 2.1e-7 at
    configurations 1 to 6 and 5.1e-5 at the gap configuration, whose samples
    next to a gap are divided by a window-sum-square of 6e-8 (pin 1e-4, a
    tenth of the Griffin-Lim bound)."""
    _, n_fft, hop, win = cfg[:4]
    for L in ac.stft_lengths(cfg):
        for b in range(3):
            y = ac.tone_noise(L, 10 + b, 1.0 + b)
            ref = ao.stft(y, n_fft, hop, win, dtype=np.float64)
            got = ao.stft(y, n_fft, hop, win)
            assert ref.dtype == np.complex128 and got.dtype == np.complex64
            assert got.shape == ref.shape == (n_fft // 2 + 1, 1 + L // hop)
            assert np.abs(got - ref).max() <= 6.4e-6 * np.abs(ref).max(), (L, b)
            if ref.shape[1] >= 2:
                r64 = ao.istft(ref, n_fft, hop, win, dtype=np.float64)
                r32 = ao.istft(ref.astype(np.complex64), n_fft, hop, win)
                assert r64.dtype == np.float64 and r32.dtype == np.float32 and r32.shape == r64.shape
                assert np.abs(r32 - r64).max() <= 1e-4 * np.abs(r64).max(), (L, b)


@pytest.mark.parametrize("name", list(ac.MEL_SIGNALS))
@pytest.mark.parametrize("cfg", ALL_CONFIGS, ids=ac.config_id)
def test_float32_mel_features_pinned_to_float64(cfg, name):
    """Largest distances per signal over the seven configurations (mel power
    relative to its maximum / dB / normalised features):
      tone_noise               2.1e-7 / 1.8e-5 / 1.1e-6
      silence_then_tones       1.6e-7 / 1.8e-4 / 4.5e-6
      silence_then_tones_1e-4  2.1e-7 / 1.6e-5 / 8.2e-7
      quiet_then_loud          2.0e-7 / 2.6e-4 / 6.5e-6
      one_frame                8.0e-8 / 6.9e-6 / 2.9e-7
      one_sample               1.5e-7 / 7.0e-6 / 1.5e-4
    The normalised features are pinned to 1e-4, a tenth of the project's
    1e-3; one_sample exceeds it at n_fft 2048 (1.2e-4 at hop 512, 1.5e-4 at
    hop 300 / win 1200; 2.0e-5 to 5.1e-5 elsewhere), where the GPU test's
    bound is ten times the distance instead.  The power and the dB carry no
    GPU bound of their own; they are held to 1e-5 of the maximum and 1e-3
    dB."""
    y = ac.mel_signal(name, cfg)
    P, db, mel = ac.mel_reference(y, cfg, np.float64)
    P32, db32, mel32 = ac.mel_reference(y, cfg, np.float32)
    assert mel.dtype == np.float64 and mel32.dtype == np.float32
    assert mel.shape == mel32.shape == (cfg[4], 1 + len(y) // cfg[2])
    assert np.abs(P32 - P).max() <= 1e-5 * P.max()
    assert np.abs(db32 - db).max() <= 1e-3
    d = np.abs(mel32 - mel).max()
    bound, d_again = ac.mel_bound(y, cfg)
    assert d_again == d
    if (cfg, name) in MEL_PIN_EXCEPTIONS:
        assert 1e-4 < d <= 1.1 * MEL_PIN_EXCEPTIONS[(cfg, name)] and bound == 10.0 * d
    else:
        assert d <= 1e-4 and bound == 1e-3
    assert mel.min() == -1.0 and abs(mel.max() - 1.0) < 1e-12
    # the clamp the signal is there for binds on the float64 reference
    floor_hits = int((db == db.max() - ao.TOP_DB).sum())
    amin_hits = int((P < ao.AMIN).sum())
    if ac.MEL_SIGNALS[name] == "floor":
        assert floor_hits > 0
    if ac.MEL_SIGNALS[name] == "amin":
        amin_level = 10.0 * np.log10(ao.AMIN) - 10.0 * np.log10(P.max())
        assert amin_hits > 0 and P.max() > ao.AMIN and amin_level > db.max() - ao.TOP_DB and floor_hits == 0
        assert int((db == amin_level).sum()) == amin_hits


def test_float64_degenerate_mel_is_nan_like_float32():
    """0 / 0 in the normalisation: silence, and tones every mel power of
    which is below amin, give NaN throughout at either precision."""
    for cfg in ALL_CONFIGS:
        for y in (np.zeros(3 * cfg[1], np.float32), ac.two_tone(3 * cfg[1], 1e-6)):
            P, db, mel = ac.mel_reference(y, cfg, np.float64)
            if P.max() >= ao.AMIN:
                assert cfg[1] != 512  # the 1e-6 tones stay below amin at n_fft 512
                continue
            assert (db == 0).all() and np.isnan(mel).all()
            assert np.isnan(ac.mel_reference(y, cfg, np.float32)[2]).all()


@pytest.mark.parametrize("cfg", [ac.CONFIGS[i] for i in (1, 2, 3, 5)] + [ac.GAP_CONFIG], ids=ac.config_id)
def test_float32_griffin_lim_pinned_to_float64(cfg):
    """Largest distance relative to the float64 peak, over B = 2, T from 4096
    samples and T = 2: n_iter 0 1.8e-7, n_iter 1 3.2e-7, n_iter 8 7.8e-6
    (pin 1e-4, a tenth of the GPU bound).  Configuration 5 (16 kHz, hop 160,
    win 400), which the GPU Griffin-Lim cases do not use, reaches 1.6e-4 after
    8 iterations."""
    _, n_fft, hop, win = cfg[:4]
    for T_from in (4096, hop):
        S, ang = ac.griffin_inputs(cfg, T_from, 3)
        assert S.shape[2] == 1 + T_from // hop
        for n_iter in (0, 1, 8):
            for b in range(2):
                ref = ao.griffin_lim(S[b], ang[b], n_iter, n_fft, hop, win, dtype=np.float64)
                got = ao.griffin_lim(S[b], ang[b], n_iter, n_fft, hop, win)
                assert ref.dtype == np.float64 and got.shape == ref.shape == (hop * (S.shape[2] - 1),)
                assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), (T_from, n_iter, b)


def test_window_sumsquare_zero_flanks():
    """A window shorter than the FFT has zero flanks.  At configurations 4
    and 6 (hop < win_length) every sample with a window-sum-square at or
    below tiny(float32) lies in the n_fft / 2 centre padding istft trims; at
    the gap configuration (hop > win_length) such samples are inside the
    signal, where istft leaves the overlap-add undivided."""
    tiny = np.finfo(np.float32).tiny
    for cfg, inside in ((ac.CONFIGS[3], False), (ac.CONFIGS[5], False), (ac.GAP_CONFIG, True)):
        _, n_fft, hop, win = cfg[:4]
        for T in (2, 1 + 4096 // hop):
            wss = ao.window_sumsquare(T, n_fft, hop, win, np.float64)
            assert (wss <= tiny).any()
            kept = wss[n_fft // 2:n_fft // 2 + hop * (T - 1)]
            assert bool((kept <= tiny).any()) == inside
            if inside:  # 1 / wss would be inf there: the undivided samples are the overlap-add's own (0)
                S, ang = ac.griffin_inputs(cfg, hop * (T - 1), 3, B=1)
                y = ao.griffin_lim(S[0], ang[0], 0, n_fft, hop, win, dtype=np.float64)
                assert np.isfinite(y).all() and (y[kept <= tiny] == 0).all()


def test_nnls_block_columns_at_80_and_40_bands():
    """librosa's L-BFGS-B blocks: 819 columns at 80 float32 bands, 1638 at 40."""
    W80, W40 = np.zeros((80, 513), np.float32), np.zeros((40, 257), np.float32)
    assert ao.nnls_block_columns(W80, np.zeros((80, 830), np.float32)) == 819
    assert ao.nnls_block_columns(W40, np.zeros((40, 1650), np.float32)) == 1638
