"""GPU: Dsp.mel_features_ragged (m2_mel_features_ragged, csrc/audio_dsp.hip):
compute_mel_spectrogram of a packed batch of utterances of unequal length, each
as if featurized alone.

The invariant every case leans on: utterance b of a ragged call equals, bit for
bit, the leading columns of Dsp.mel_spectrogram of that utterance alone, taken
from the float32 signal (PCM16: s / 32768, then / peak as numpy divides).  The
plain call in turn is held to the float64 oracle by test_gpu_dsp_edges.py; the
edge-length case repeats that bound (audio_cases.mel_bound, 1e-3 for each of
its inputs) on the ragged result itself.

Three handles, so that the 512-, 1024- and 2048-point FFT instantiations all
run: the default (22050, 1024, 256, 1024, 64, 0, 11025), audio_cases.CONFIGS[1]
(n_fft 512, hop 128) and audio_cases.CONFIGS[5] (n_fft 2048, hop 300, win 1200).
Each test prints its figures as "RAGGEDMEL <quantity> <handle> <value>" before
it asserts."""
import sys

import numpy as np
import pytest
import torch

import audio_cases as ac

from conftest import GOLDEN

if str(GOLDEN) not in sys.path:
    sys.path.insert(0, str(GOLDEN))

import dataset_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

HANDLES = [(22050, 1024, 256, 1024, 64, 0, 11025), ac.CONFIGS[1], ac.CONFIGS[5]]
handles = pytest.mark.parametrize("cfg", HANDLES, ids=ac.config_id)


def _dsp(cfg, gpu):
    from m2amd.dsp import get_dsp
    sr, n_fft, hop, win, n_mels, fmin, fmax = cfg
    return get_dsp(sr, n_fft, hop, win, n_mels, fmin, fmax, gpu)


def _report(quantity, cfg, value):
    print(f"RAGGEDMEL {quantity} {ac.config_id(cfg)} {value:.3e}")


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _peak_normalised(y):
    y = np.asarray(y, dtype=np.float32)
    m = np.max(np.abs(y))
    return y / m if m > 0 else y


def _from_pcm(pcm):
    return pcm.astype(np.float32) / np.float32(32768.0)


def _alone(d, y, gpu):
    """Dsp.mel_spectrogram of one float32 signal -> [n_mels, T] on the device."""
    return d.mel_spectrogram(_dev(np.asarray(y, dtype=np.float32), gpu))[0]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32),
                                                                    b.contiguous().view(torch.int32))


def _pack(signals, gpu):
    return _dev(np.concatenate(signals), gpu), [len(s) for s in signals]


def _ragged(d, gpu, signals, **kw):
    samples, lens = _pack(signals, gpu)
    return d.mel_features_ragged(samples, lengths=lens, **kw)


def _check_rows(mel, frames, want, n_mels):
    """Every utterance's leading columns equal ``want`` bit for bit, zeros behind."""
    frames = frames.cpu().tolist()
    assert frames == [w.shape[1] for w in want]
    assert mel.shape[:2] == (len(want), n_mels) and mel.shape[2] >= max(frames, default=0)
    for b, w in enumerate(want):
        assert _same_bits(mel[b, :, :frames[b]], w), b
        pad = mel[b, :, frames[b]:]
        assert bool((pad == 0).all()), b


# -------------------------------------------------------------- 1. edge lengths
@handles
def test_edge_lengths_in_one_batch(gpu, cfg):
    """Every length of audio_cases.stft_lengths in one shuffled batch, PCM16:
    each utterance equals its own plain call, is within mel_bound (1e-3 here)
    of the float64 oracle, and int16 and float32 samples give the same bits."""
    n_mels, hop = cfg[4], cfg[2]
    d = _dsp(cfg, gpu)
    lengths = ac.stft_lengths(cfg)
    lengths = [lengths[i] for i in np.random.default_rng(5).permutation(len(lengths))]
    assert len(set(lengths)) == len(lengths) == 9
    pcm = [dc.to_pcm16(ac.tone_noise(L, L % 7)) for L in lengths]
    samples, lens = _pack(pcm, gpu)
    assert samples.dtype == torch.int16
    mel, frames = d.mel_features_ragged(samples, lengths=lens)
    assert mel.dtype == torch.float32 and frames.dtype == torch.int32 and mel.is_contiguous()
    assert mel.shape == (9, n_mels, 1 + max(lengths) // hop)
    ys = [_peak_normalised(_from_pcm(p)) for p in pcm]
    _check_rows(mel, frames, [_alone(d, y, gpu) for y in ys], n_mels)
    worst = 0.0
    host = mel.cpu().numpy()
    for b, y in enumerate(ys):
        bound, d32 = ac.mel_bound(y, cfg)
        assert bound == 1e-3, (lengths[b], d32)
        ref = ac.mel_reference(y, cfg)[2]
        err = float(np.abs(host[b, :, :ref.shape[1]] - ref).max())
        worst = max(worst, err)
        assert err <= bound, (lengths[b], err)
    _report("edge_lengths_vs_float64", cfg, worst)
    as_float, _ = _pack([_from_pcm(p) for p in pcm], gpu)
    mel_f, frames_f = d.mel_features_ragged(as_float, offsets=np.concatenate([[0], np.cumsum(lens)]))
    assert _same_bits(mel_f, mel) and torch.equal(frames_f, frames)


# --------------------------------------------------------- 2. batch composition
@handles
def test_position_in_the_batch_does_not_matter(gpu, cfg):
    n_fft, hop, n_mels = cfg[1], cfg[2], cfg[4]
    d = _dsp(cfg, gpu)
    u = dc.to_pcm16(ac.tone_noise(2 * n_fft + 3, 4))
    others = [dc.to_pcm16(ac.tone_noise(L, s, sc)) for L, s, sc in ((5 * n_fft, 1, 0.2), (hop + 1, 2, 1.0), (7, 3, 0.6))]
    alone, fa = _ragged(d, gpu, [u])
    assert alone.shape == (1, n_mels, 1 + len(u) // hop) and fa.tolist() == [alone.shape[2]]
    assert _same_bits(alone[0], _alone(d, _peak_normalised(_from_pcm(u)), gpu))
    first, ff = _ragged(d, gpu, [u] + others)
    last, fl = _ragged(d, gpu, others + [u])
    T = alone.shape[2]
    assert ff[0].item() == fl[-1].item() == T
    assert _same_bits(first[0, :, :T], alone[0]) and _same_bits(last[-1, :, :T], alone[0])
    assert bool((first[0, :, T:] == 0).all()) and bool((last[-1, :, T:] == 0).all())
    for k in range(len(others)):
        assert _same_bits(first[1 + k], last[k])


@handles
def test_empty_batch(gpu, cfg):
    d = _dsp(cfg, gpu)
    mel, frames = d.mel_features_ragged(torch.empty(0, dtype=torch.int16, device=gpu), lengths=[])
    assert mel.shape == (0, cfg[4], 0) and frames.shape == (0,) and frames.dtype == torch.int32


# ----------------------------------------------------------------- 3. truncation
@handles
def test_truncation_cuts_the_store_not_the_statistics(gpu, cfg):
    """max_frames keeps the first columns of the untruncated features.  On the
    oracle, the features of the cut audio differ from those columns by far
    more than the bound (the loud second half sets the dB reference and the
    floor), so computing from truncated audio would be caught."""
    n_fft, hop, n_mels = cfg[1], cfg[2], cfg[4]
    d = _dsp(cfg, gpu)
    y = ac.two_tone(6 * n_fft)
    y[:3 * n_fft] *= np.float32(1e-2)
    keep = 1 + 2 * n_fft // hop
    T = 1 + len(y) // hop
    assert keep < T
    yn = _peak_normalised(y)
    full_ref = ac.mel_reference(yn, cfg)[2]
    cut_ref = ac.mel_reference(_peak_normalised(y[:(keep - 1) * hop]), cfg)[2]
    assert cut_ref.shape == (n_mels, keep)
    teeth = float(np.abs(cut_ref - full_ref[:, :keep]).max())
    _report("truncation_teeth", cfg, teeth)
    assert teeth > 100 * ac.mel_bound(yn, cfg)[0]
    short = ac.tone_noise(hop * (keep - 1) + 1, 3)  # exactly `keep` frames
    samples, lens = _pack([y, short], gpu)
    full, f_full = d.mel_features_ragged(samples, lengths=lens)
    assert f_full.tolist() == [T, keep] and full.shape[2] == T
    cut, f_cut = d.mel_features_ragged(samples, lengths=lens, max_frames=keep)
    assert f_cut.tolist() == [keep, keep] and cut.shape == (2, n_mels, keep)
    assert _same_bits(cut, full[:, :, :keep])
    assert _same_bits(full[0], _alone(d, yn, gpu))
    err = float(np.abs(cut[0].cpu().numpy() - full_ref[:, :keep]).max())
    _report("truncated_vs_float64", cfg, err)
    assert err <= ac.mel_bound(yn, cfg)[0]
    for limit in (T, T + 5):  # equal to and above the longest count: nothing is cut
        same, f_same = d.mel_features_ragged(samples, lengths=lens, max_frames=limit)
        assert f_same.tolist() == [T, keep] and _same_bits(same, full)
    mid, f_mid = d.mel_features_ragged(samples, lengths=lens, max_frames=keep + 2)  # binds for one of the two
    assert f_mid.tolist() == [keep + 2, keep] and _same_bits(mid[0], full[0, :, :keep + 2])
    assert _same_bits(mid[1, :, :keep], full[1, :, :keep]) and bool((mid[1, :, keep:] == 0).all())


# -------------------------------------------------------------------- 4. padding
@handles
def test_padding_is_written_as_zeros(gpu, cfg):
    n_fft, hop, n_mels = cfg[1], cfg[2], cfg[4]
    d = _dsp(cfg, gpu)
    pcm = [dc.to_pcm16(ac.tone_noise(L, s)) for L, s in ((3, 1), (2 * n_fft, 2), (hop, 3), (n_fft + 1, 4))]
    samples, lens = _pack(pcm, gpu)
    T_out = 1 + max(lens) // hop + 3
    for limit in (0, 2):
        out = torch.full((len(pcm), n_mels, T_out), float("nan"), device=gpu)
        mel, frames = d.mel_features_ragged(samples, lengths=lens, max_frames=limit, out=out)
        assert mel.data_ptr() == out.data_ptr()
        want = [1 + L // hop for L in lens]
        assert frames.tolist() == [min(t, limit) if limit else t for t in want]
        for b, t in enumerate(frames.tolist()):
            assert bool(torch.isfinite(out[b, :, :t]).all()), b
            assert bool((out[b, :, t:] == 0).all()), b  # a NaN left behind compares unequal


# -------------------------------------------------------------------- 5. silence
@handles
def test_silent_utterance_between_two_others(gpu, cfg):
    """All-zero audio: 0 / 0 in the [-1, 1] step, NaN in every frame, as the
    reference gives and test_gpu_dsp_edges pins for the plain call; its
    padding is still 0, its neighbours are untouched, and a peak of 0 leaves
    the samples as they are."""
    n_fft, hop, n_mels = cfg[1], cfg[2], cfg[4]
    d = _dsp(cfg, gpu)
    a, c = dc.to_pcm16(ac.tone_noise(n_fft + 5, 1)), dc.to_pcm16(ac.tone_noise(3 * n_fft, 2, 0.5))
    z = np.zeros(2 * hop + 1, "<i2")
    mel, frames = _ragged(d, gpu, [a, z, c])
    Tz = 1 + len(z) // hop
    assert frames.tolist() == [1 + len(a) // hop, Tz, 1 + len(c) // hop]
    assert bool(torch.isnan(mel[1, :, :Tz]).all()) and bool((mel[1, :, Tz:] == 0).all())
    assert _same_bits(mel[1, :, :Tz], _alone(d, np.zeros(len(z), np.float32), gpu))
    pair, _ = _ragged(d, gpu, [a, c])
    assert _same_bits(mel[0], pair[0]) and _same_bits(mel[2], pair[1])
    assert _same_bits(mel[0, :, :frames[0]], _alone(d, _peak_normalised(_from_pcm(a)), gpu))
    raw, _ = _ragged(d, gpu, [a, z, c], normalize=False)
    assert _same_bits(raw[1], mel[1])


# ------------------------------------------------------------ 6. normalize=False
@handles
def test_without_normalisation(gpu, cfg):
    n_fft, hop, n_mels = cfg[1], cfg[2], cfg[4]
    d = _dsp(cfg, gpu)
    ys = [ac.tone_noise(L, s, 0.37) for L, s in ((2 * n_fft + 1, 1), (hop - 1, 2), (4 * n_fft, 3))]
    mel, frames = _ragged(d, gpu, ys, normalize=False)
    _check_rows(mel, frames, [_alone(d, y, gpu) for y in ys], n_mels)
    normed, _ = _ragged(d, gpu, ys, normalize=True)
    _check_rows(normed, frames, [_alone(d, _peak_normalised(y), gpu) for y in ys], n_mels)
    pcm = [dc.to_pcm16(y) for y in ys]
    mel_i, frames_i = _ragged(d, gpu, pcm, normalize=False)
    _check_rows(mel_i, frames_i, [_alone(d, _from_pcm(p), gpu) for p in pcm], n_mels)


# --------------------------------------------------------------- 7. reproducible
@handles
def test_two_runs_are_bit_identical(gpu, cfg):
    n_fft, hop = cfg[1], cfg[2]
    d = _dsp(cfg, gpu)
    rng = np.random.default_rng(9)
    pcm = [dc.to_pcm16(ac.tone_noise(int(L), b, 0.1 + 0.1 * b)) for b, L in enumerate(rng.integers(1, 6 * n_fft, 12))]
    samples, lens = _pack(pcm, gpu)
    one, f1 = d.mel_features_ragged(samples, lengths=lens, max_frames=9)
    one, f1 = one.clone(), f1.clone()
    two, f2 = d.mel_features_ragged(samples, lengths=lens, max_frames=9)
    assert _same_bits(one, two) and torch.equal(f1, f2)


# --------------------------------------------------------------------- 8. errors
@handles
def test_shape_errors(gpu, cfg):
    from m2amd._lib import M2_E_SHAPE, M2Error
    n_mels, hop = cfg[4], cfg[2]
    d = _dsp(cfg, gpu)
    samples = _dev(dc.to_pcm16(ac.tone_noise(12, 1)), gpu)
    with pytest.raises(M2Error) as e:
        d.mel_features_ragged(samples, lengths=[5, 0, 7])
    assert e.value.status == M2_E_SHAPE
    long = _dev(dc.to_pcm16(ac.tone_noise(3 * hop, 1)), gpu)  # 4 frames
    with pytest.raises(M2Error) as e:
        d.mel_features_ragged(long, lengths=[3 * hop], out=torch.zeros(1, n_mels, 3, device=gpu))
    assert e.value.status == M2_E_SHAPE
    mel, frames = d.mel_features_ragged(long, lengths=[3 * hop], max_frames=3, out=torch.zeros(1, n_mels, 3, device=gpu))
    assert frames.tolist() == [3]  # the stored count is what T_out has to hold
