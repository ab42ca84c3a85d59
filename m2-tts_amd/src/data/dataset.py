"""Datasets for M2 TTS training (drop-in for the reference's src/data/dataset.py).

``TTSDataset``, ``collate_fn``, ``create_dataloader`` and ``DummyDataset`` keep
the reference's names, signatures, defaults, dictionary keys, dtypes and
behaviour, its quirks included:

- LJSpeech ``metadata.csv``: the text is field 1 of a 2-field line, else
  field 2; without a metadata file, every audio file with a ``.txt`` beside it;
- ``process_text(text, max_text_length)`` pads the ids with SIL, so
  ``text_length`` is the padded length, while the uniform alignment spreads
  the mel frames over ``text_info['length']``, the non-SIL phonemes
  (``uniform_durations``);
- ``subset_size`` keeps the first N samples that could be processed; a file
  that fails is logged and dropped;
- ``processed_samples.pkl`` in ``cache_dir`` holds the same list of
  dictionaries, so caches interchange with the reference's.

What differs is how the features are made.  The reference runs librosa on
one file at a time; here ``TTSDataset`` hands all its files to
``AudioProcessor.process_files``, which featurizes them on the GPU as a few
ragged batches (every utterance peak-normalised, scaled to dB and truncated
as if processed alone).  Only mono PCM16 ``.wav`` at the dataset's sample
rate can be read: there is no resampler, and ``.mp3`` / ``.flac`` files are
found and skipped with a warning because there is no decoder.  Dataset items
are CPU tensors and ``__getitem__`` never touches the GPU.

One deliberate difference: ``create_dataloader`` passes ``prefetch_factor``
only with ``num_workers > 0``; current torch refuses the reference's
``num_workers=0`` call ("prefetch_factor option could only be specified in
multiprocessing").
"""
from __future__ import annotations

import logging
import pickle
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch.utils.data import DataLoader, Dataset

from utils.audio import AudioProcessor
from utils.text import TextProcessor

logger = logging.getLogger(__name__)

_AUDIO_EXTENSIONS = [".wav", ".mp3", ".flac"]
_READABLE = {".wav"}


def uniform_durations(mel_length: int, length: int, n_ids: int) -> List[float]:
    """The reference's simplified alignment (dataset.py:182-196): ``mel_length /
    length`` frames for each of the ``length`` non-SIL phonemes, then zeros up
    to the ``n_ids`` (padded) ids, cut to ``n_ids`` if longer; all zeros for a
    ``length`` of 0."""
    if length <= 0:
        return [0.0] * n_ids
    durations = [mel_length / length] * length
    if len(durations) < n_ids:
        durations.extend([0.0] * (n_ids - len(durations)))
    return durations[:n_ids]


class TTSDataset(Dataset):
    """Dataset for TTS training: (text, mel) samples of a corpus directory."""

    def __init__(self, data_dir: Path, subset_size: Optional[int] = None, max_text_length: int = 256,
                 max_mel_length: int = 1000, sample_rate: int = 22050, n_mels: int = 64,
                 cache_dir: Optional[Path] = None):
        self.data_dir = Path(data_dir)
        self.subset_size = subset_size
        self.max_text_length = max_text_length
        self.max_mel_length = max_mel_length
        self.audio_processor = AudioProcessor(sample_rate=sample_rate, n_mels=n_mels)
        self.text_processor = TextProcessor()
        self.cache_dir = cache_dir
        if self.cache_dir:
            self.cache_dir.mkdir(parents=True, exist_ok=True)
        self.samples = self._load_samples()
        logger.info(f"TTSDataset initialized with {len(self.samples)} samples")

    def _load_samples(self) -> List[Dict[str, Any]]:
        cache_file = self.cache_dir / "processed_samples.pkl" if self.cache_dir else None
        if cache_file and cache_file.exists():
            logger.info(f"Loading cached samples from {cache_file}")
            with open(cache_file, "rb") as f:
                samples = pickle.load(f)
            return samples[:self.subset_size] if self.subset_size else samples
        if (self.data_dir / "metadata.csv").exists():
            pairs = self._list_ljspeech_format()
        else:
            pairs = self._list_paired_files()
        samples = self._process_samples(pairs)
        if self.subset_size:
            samples = samples[:self.subset_size]
            logger.info(f"Limited to {len(samples)} samples for subset training")
        if cache_file:
            logger.info(f"Caching processed samples to {cache_file}")
            with open(cache_file, "wb") as f:
                pickle.dump(samples, f)
        return samples

    def _list_ljspeech_format(self) -> List[Tuple[Path, str]]:
        """(audio path, text) of every metadata line whose wav exists."""
        metadata_file = self.data_dir / "metadata.csv"
        wavs_dir = self.data_dir / "wavs"
        logger.info(f"Loading LJSpeech format from {metadata_file}")
        with open(metadata_file, "r", encoding="utf-8") as f:
            lines = f.readlines()
        pairs = []
        for line in lines:
            parts = line.strip().split("|")
            if len(parts) < 2:
                continue
            text = parts[1] if len(parts) == 2 else parts[2]  # the normalised text when there is one
            audio_path = wavs_dir / f"{parts[0]}.wav"
            if audio_path.exists():
                pairs.append((audio_path, text))
        return pairs

    def _list_paired_files(self) -> List[Tuple[Path, str]]:
        """(audio path, text) of every audio file with a .txt beside it."""
        audio_files: List[Path] = []
        for ext in _AUDIO_EXTENSIONS:
            audio_files.extend(self.data_dir.glob(f"**/*{ext}"))
        logger.info(f"Found {len(audio_files)} audio files")
        pairs = []
        for audio_path in audio_files:
            text_path = audio_path.with_suffix(".txt")
            if not text_path.exists():
                continue
            if audio_path.suffix not in _READABLE:
                logger.warning(f"Skipping {audio_path}: no {audio_path.suffix} decoder in this build")
                continue
            try:
                with open(text_path, "r", encoding="utf-8") as f:
                    pairs.append((audio_path, f.read().strip()))
            except Exception as e:
                logger.warning(f"Failed to process {audio_path}: {e}")
        return pairs

    def _process_samples(self, pairs: List[Tuple[Path, str]]) -> List[Dict[str, Any]]:
        """All files through the ragged GPU featurization, then the text side
        per sample; a sample that fails either is logged and dropped."""
        limit = self.max_mel_length if self.max_mel_length > 0 else None
        features = self.audio_processor.process_files([p for p, _ in pairs], max_mel_length=limit,
                                                      return_audio=False)
        samples = []
        for (audio_path, text), feat in zip(pairs, features):
            if feat is None:
                logger.error(f"Error processing {audio_path}: no features")
                continue
            try:
                sample = self._make_sample(audio_path, text, feat[1])
            except Exception as e:
                logger.error(f"Error processing {audio_path}: {e}")
                continue
            samples.append(sample)
        return samples

    def _make_sample(self, audio_path: Path, text: str, mel_spec) -> Dict[str, Any]:
        if mel_spec.shape[1] > self.max_mel_length:
            mel_spec = mel_spec[:, :self.max_mel_length]
        text_info = self.text_processor.process_text(text, self.max_text_length)
        mel_length = mel_spec.shape[1]
        ids = text_info["phoneme_ids"]
        return {
            "audio_path": str(audio_path),
            "text": text,
            "phoneme_ids": ids,
            "phonemes": text_info["phonemes"],
            "text_length": len(ids),
            "mel_spec": mel_spec,
            "mel_length": mel_length,
            "durations": uniform_durations(mel_length, text_info["length"], len(ids)),
        }

    def __len__(self) -> int:
        return len(self.samples)

    def __getitem__(self, idx: int) -> Dict[str, torch.Tensor]:
        sample = self.samples[idx]
        return {
            "phoneme_ids": torch.LongTensor(sample["phoneme_ids"]),
            "text_length": torch.LongTensor([sample["text_length"]]),
            "mel_spec": torch.FloatTensor(sample["mel_spec"]),
            "mel_length": torch.LongTensor([sample["mel_length"]]),
            "durations": torch.FloatTensor(sample["durations"]),
            "text": sample["text"],
        }


def collate_fn(batch: List[Dict[str, Any]]) -> Dict[str, torch.Tensor]:
    """Zero-pad a list of items to the batch's longest text and longest mel."""
    n = len(batch)
    max_text_len = max(item["phoneme_ids"].size(0) for item in batch)
    max_mel_len = max(item["mel_spec"].size(1) for item in batch)
    mel_dim = batch[0]["mel_spec"].size(0)
    phoneme_ids = torch.zeros(n, max_text_len, dtype=torch.long)
    text_lengths = torch.zeros(n, dtype=torch.long)
    mel_specs = torch.zeros(n, mel_dim, max_mel_len, dtype=torch.float)
    mel_lengths = torch.zeros(n, dtype=torch.long)
    durations = torch.zeros(n, max_text_len, dtype=torch.float)
    texts = []
    for i, item in enumerate(batch):
        text_len = item["phoneme_ids"].size(0)
        mel_len = item["mel_spec"].size(1)
        phoneme_ids[i, :text_len] = item["phoneme_ids"]
        text_lengths[i] = item["text_length"]
        mel_specs[i, :, :mel_len] = item["mel_spec"]
        mel_lengths[i] = item["mel_length"]
        durations[i, :text_len] = item["durations"]
        texts.append(item["text"])
    return {
        "phoneme_ids": phoneme_ids,
        "text_lengths": text_lengths,
        "mel_specs": mel_specs,
        "mel_lengths": mel_lengths,
        "durations": durations,
        "texts": texts,
    }


def create_dataloader(dataset: TTSDataset, batch_size: int = 2, shuffle: bool = True, num_workers: int = 2,
                      pin_memory: bool = False, drop_last: bool = True) -> DataLoader:
    """DataLoader over ``collate_fn``; persistent workers and a prefetch factor
    of 1 when there are workers."""
    workers = {"persistent_workers": True, "prefetch_factor": 1} if num_workers > 0 else {}
    return DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                      pin_memory=pin_memory, drop_last=drop_last, collate_fn=collate_fn, **workers)


class DummyDataset(Dataset):
    """Random samples for testing without data; the ``torch`` RNG calls are the
    reference's, in its order, so a seed gives the same items."""

    def __init__(self, size: int = 100, max_text_length: int = 50, max_mel_length: int = 200, mel_dim: int = 64,
                 vocab_size: int = 256):
        self.size = size
        self.max_text_length = max_text_length
        self.max_mel_length = max_mel_length
        self.mel_dim = mel_dim
        self.vocab_size = vocab_size
        logger.info(f"Created DummyDataset with {size} samples")

    def __len__(self) -> int:
        return self.size

    def __getitem__(self, idx: int) -> Dict[str, torch.Tensor]:
        text_len = torch.randint(10, self.max_text_length, (1,)).item()
        mel_len = torch.randint(50, self.max_mel_length, (1,)).item()
        phoneme_ids = torch.randint(0, self.vocab_size, (text_len,))
        mel_spec = torch.randn(self.mel_dim, mel_len)
        durations = torch.rand(text_len)
        durations = durations / durations.sum() * mel_len
        return {
            "phoneme_ids": phoneme_ids,
            "text_length": torch.LongTensor([text_len]),
            "mel_spec": mel_spec,
            "mel_length": torch.LongTensor([mel_len]),
            "durations": durations,
            "text": f"dummy_text_{idx}",
        }
