"""The three-file corpus of the dataset tests, by seed (pure numpy + wave).

Shared by make_dataset_golden.py, which runs the reference's own
src/data/dataset.py on it and records the results in dataset_reference.json /
dataset_reference.npz, and by the tests that run data.dataset on the same
files.  Nothing here is stored as an array: the signals are
oracle/audio_cases.py's, written as mono PCM16 by ``write_pcm16``.

  utt_a  tone_noise, 9000 samples (36 frames at hop 256); plain text;
  utt_b  two_tone over 6 n_fft samples, the first half 40 dB down (25 frames):
         truncating it changes which frames set the dB reference; its text has
         no lexicon word, so every phoneme comes from the letter-to-sound rules;
  utt_c  tone_noise at 0.3, 5000 samples (20 frames: exactly the binding
         max_mel_length); its metadata line has 3 fields (raw | normalised).
"""
import wave
from pathlib import Path

import numpy as np

import audio_cases as ac

SR = 22050
N_FFT, HOP, N_MELS = 1024, 256, 64  # TTSDataset's AudioProcessor(sample_rate, n_mels) defaults
CFG = (SR, N_FFT, HOP, N_FFT, N_MELS, 0, SR // 2)
MAX_TEXT_LENGTH = 32
CUT = 20  # a max_mel_length that binds for utt_a and utt_b and equals utt_c's count

# name -> metadata fields after the id
TEXTS = {
    "utt_a": ("Hello world, this is a test.",),
    "utt_b": ("zxqv brrk plomf",),
    "utt_c": ("Dr. Smith has 3 cats", "doctor smith has three cats"),
}
NAMES = tuple(TEXTS)

# name -> (layout, TTSDataset keyword arguments)
VARIANTS = {
    "lj": ("ljspeech", {}),
    "lj_cut": ("ljspeech", {"max_mel_length": CUT}),
    "lj_subset": ("ljspeech", {"subset_size": 2}),
    "paired": ("paired", {}),
    "paired_cut": ("paired", {"max_mel_length": CUT}),
}

DUMMY_SEED = 7
DUMMY_ARGS = (4, 12, 60, 8, 50)  # size, max_text_length, max_mel_length, mel_dim, vocab_size


def signal(name: str) -> np.ndarray:
    if name == "utt_a":
        return ac.tone_noise(9000, 11)
    if name == "utt_b":
        y = ac.two_tone(6 * N_FFT)
        y[:3 * N_FFT] *= np.float32(1e-2)
        return y
    if name == "utt_c":
        return ac.tone_noise(5000, 2, 0.3)
    raise KeyError(name)


def to_pcm16(y: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(np.asarray(y, dtype=np.float32) * np.float32(32767.0)), -32768, 32767).astype("<i2")


def write_pcm16(path, pcm: np.ndarray, sample_rate: int = SR) -> None:
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sample_rate))
        w.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


def text_of(name: str) -> str:
    """What the dataset takes as the sample's text: the last metadata field."""
    return TEXTS[name][-1]


def write_corpus(root, layout: str) -> Path:
    """The corpus under ``root``: "ljspeech" (metadata.csv and wavs/) or
    "paired" (NAME.wav with NAME.txt beside it, holding text_of(NAME))."""
    root = Path(root)
    if layout == "ljspeech":
        (root / "wavs").mkdir(parents=True, exist_ok=True)
        for n in NAMES:
            write_pcm16(root / "wavs" / f"{n}.wav", to_pcm16(signal(n)))
        (root / "metadata.csv").write_text("".join("|".join((n,) + TEXTS[n]) + "\n" for n in NAMES), encoding="utf-8")
    elif layout == "paired":
        root.mkdir(parents=True, exist_ok=True)
        for n in NAMES:
            write_pcm16(root / f"{n}.wav", to_pcm16(signal(n)))
            (root / f"{n}.txt").write_text(text_of(n) + "\n", encoding="utf-8")
    else:
        raise KeyError(layout)
    return root


def normalised(name: str) -> np.ndarray:
    """The float32 signal the features are taken from: PCM16 / 32768, / peak."""
    y = to_pcm16(signal(name)).astype(np.float32) / np.float32(32768.0)
    m = np.max(np.abs(y))
    return y / m if m > 0 else y
