"""Ragged batches, the parts that need no GPU: the entry points are
exported and bound with the header's signatures, unpad is pure indexing, CPU
tensors are refused, and the CLI's --text-file mode parses."""
import ctypes
import re
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, str(ROOT / "m2-tts_amd" / "scripts"))

RAGGED = ["m2_mel_decoder_ragged", "m2_vocoder_ragged", "m2_inference_back_ragged", "m2_ragged_workspace_bytes"]
CTYPES = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}


def header_signature(name):
    """(return ctype, argument ctypes) of a function as include/m2tts_hip.h declares it."""
    text = (ROOT / "include" / "m2tts_hip.h").read_text()
    m = re.search(r"^(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text, re.M | re.S)
    assert m, f"{name} is not declared in include/m2tts_hip.h"
    args = []
    for a in m.group(2).split(","):
        a = " ".join(a.split())
        args.append(ctypes.c_void_p if "*" in a else CTYPES[a.replace("const ", "").split(" ")[0]])
    return CTYPES[m.group(1)], args


@pytest.mark.parametrize("name", RAGGED)
def test_entry_points_exported_and_bound(name):
    from m2amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by the library"
    assert name in _lib._SIGNATURES
    res, args = header_signature(name)
    assert _lib._SIGNATURES[name] == (res, args)
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args
    assert lib.m2_abi_version() == 1


def test_bad_arguments_are_reported():
    from m2amd import _lib
    lib = _lib.load()
    assert lib.m2_mel_decoder_ragged(None, None, None, 1, 1, None, None, 0, None) == -1
    assert b"m2_mel_decoder_ragged" in lib.m2_last_error()
    assert lib.m2_vocoder_ragged(None, None, 1, None, 1, 1, None, None, 0, None) == -1
    assert lib.m2_inference_back_ragged(None, 1, 1, 1, None, 0, None, None, None, None, 0, None) == -1
    assert lib.m2_ragged_workspace_bytes(None, 1) == 0


def test_unpad_views_on_cpu():
    from models.tts_model import unpad
    mel = torch.arange(2 * 5 * 3, dtype=torch.float32).reshape(2, 5, 3)
    audio = torch.arange(2 * 320, dtype=torch.float32).reshape(2, 1, 320)
    parts = unpad(mel, audio, torch.tensor([5, 2]))
    assert [tuple(m.shape) for m, _ in parts] == [(5, 3), (2, 3)]
    assert [tuple(a.shape) for _, a in parts] == [(320,), (128,)]
    assert torch.equal(parts[1][0], mel[1, :2]) and torch.equal(parts[1][1], audio[1, 0, :128])
    parts[1][0].zero_()  # views, not copies
    assert torch.count_nonzero(mel[1, :2]) == 0 and torch.count_nonzero(mel[1, 2:]) == 9
    assert parts[1][1].data_ptr() == audio[1].data_ptr()
    with pytest.raises(ValueError):
        unpad(mel, audio, torch.tensor([5, 6]))
    with pytest.raises(ValueError):
        unpad(mel, audio, torch.tensor([5]))
    with pytest.raises(ValueError):
        unpad(mel, audio[:, :, :100], torch.tensor([5, 2]))


def test_inference_ragged_refuses_cpu_tensors():
    from models.tts_model import M2TTSModel
    m = M2TTSModel()
    ids = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU execution path") as e_plain:
        m.inference(ids)
    with pytest.raises(RuntimeError, match="no CPU execution path") as e_ragged:
        m.inference_ragged(ids)
    assert type(e_ragged.value) is type(e_plain.value)
    with pytest.raises(RuntimeError, match="no CPU execution path"):
        m.inference_ragged(ids, torch.tensor([4, 4]), durations=torch.ones(2, 4))


def test_cli_text_file_flags():
    import synthesize
    p = synthesize.build_parser()
    a = p.parse_args(["--text-file", "t.txt", "--output-dir", "out", "--checkpoint", "c.pt"])
    assert (a.text_file, a.output_dir, a.batch_size, a.text) == ("t.txt", "out", 32, None)
    a = p.parse_args(["--text", "hi", "--checkpoint", "c.pt"])
    assert (a.text, a.text_file, a.output, a.duration_scale, a.sample_rate) == ("hi", None, "output.wav", 1.0, 22050)
    with pytest.raises(SystemExit):
        p.parse_args(["--text", "hi", "--text-file", "t.txt", "--output-dir", "out", "--checkpoint", "c.pt"])
    with pytest.raises(SystemExit):
        p.parse_args(["--checkpoint", "c.pt"])  # one of --text / --text-file is required
    with pytest.raises(SystemExit):
        synthesize.main(["--text-file", "t.txt", "--checkpoint", "c.pt"])  # needs --output-dir


def test_cli_reads_one_text_per_line(tmp_path):
    import synthesize
    f = tmp_path / "t.txt"
    f.write_text("one\n\n  two words \n   \nthree\n")
    assert synthesize.read_texts(f) == ["one", "two words", "three"]
