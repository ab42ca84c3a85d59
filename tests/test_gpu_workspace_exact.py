"""GPU: the loss and DSP calls' *_workspace_bytes are exact up to their 256 bytes of slack.

Every such call writes its workspace layout once and runs it over a byte counter and over
the caller's buffer.  So, with need = *_workspace_bytes(...):
  need - 256 bytes  the call succeeds, and its outputs equal, bit for bit, those of the
                    call with 2 need bytes;
  need - 257 bytes  M2_E_WORKSPACE with the function's name in m2_last_error(), before
                    any launch: after a stream synchronisation the outputs still hold
                    the sentinel they were filled with.
The buffer behind the pointer is 2 need bytes in every call, whatever size is stated.
"""
import ctypes
import sys

import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import losses_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7
M2_OK, M2_E_WORKSPACE = 0, -3


@pytest.fixture(scope="module")
def loss(gpu):
    from training.losses import CombinedTTSLoss
    torch.manual_seed(lc.WEIGHT_SEED)
    return CombinedTTSLoss().eval().to(gpu)


@pytest.fixture(scope="module")
def dsp(gpu):
    from m2amd.dsp import get_dsp
    return get_dsp(lc.SR, 1024, 256, 1024, device=gpu)


def _audio(gpu, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tanh(0.5 * torch.randn(B, L, generator=g)).to(gpu)


def _exact(gpu, name, need, outputs, call):
    """call(workspace pointer, stated bytes) -> status, writing `outputs`."""
    from m2amd import _lib
    lib = _lib.load()
    assert need > 257, (name, need)
    ws = torch.empty(2 * need, dtype=torch.uint8, device=gpu)

    def run(stated):
        for o in outputs:
            o.fill_(SENTINEL)
        rc = call(ws.data_ptr(), stated)
        err = lib.m2_last_error()
        torch.cuda.synchronize()
        return rc, err, [o.clone() for o in outputs]

    rc, err, left = run(need - 257)
    assert rc == M2_E_WORKSPACE, (name, rc)
    assert name.encode() in err and b"workspace" in err, (name, err)
    assert all(bool((o == SENTINEL).all()) for o in left), name  # refused before any launch
    rc, _, tight = run(need - 256)
    assert rc == M2_OK, (name, rc, lib.m2_last_error())
    rc, _, roomy = run(2 * need)
    assert rc == M2_OK, (name, rc, lib.m2_last_error())
    for a, b in zip(tight, roomy):
        assert not bool((a == SENTINEL).all()), name  # the call wrote it
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name


# ---- the discriminators ----------------------------------------------------------

def _disc_calls(gpu, h, B, L):
    """name -> (need, outputs, call) of the four discriminator calls on B utterances of L samples."""
    from m2amd import _lib
    lib = _lib.load()
    hd = h.handle
    real, fake = _audio(gpu, B, L, 11), _audio(gpu, B, L, 12)
    shapes = h.shapes(L)
    K = lib.m2_loss_column_count(1)

    def rows():
        return torch.empty(B, K, device=gpu, dtype=torch.float64)

    calls = {}
    logits = torch.empty(B * sum(row[-1][1] for row in shapes), device=gpu)
    feats = torch.empty(B * sum(c * n for row in shapes for c, n in row[:-1]), device=gpu)
    need = lib.m2_disc_forward_workspace_bytes(hd, B, L)
    calls["m2_disc_forward"] = (need, [logits], lambda ws, n: lib.m2_disc_forward(
        hd, real.data_ptr(), B, L, logits.data_ptr(), None, ws, n, None))
    calls["m2_disc_forward+features"] = (need, [logits, feats], lambda ws, n: lib.m2_disc_forward(
        hd, real.data_ptr(), B, L, logits.data_ptr(), feats.data_ptr(), ws, n, None))
    out_l = rows()
    need = lib.m2_disc_losses_workspace_bytes(hd, B, L)
    calls["m2_disc_losses"] = (need, [out_l], lambda ws, n: lib.m2_disc_losses(
        hd, real.data_ptr(), fake.data_ptr(), B, L, out_l.data_ptr(), ws, n, None))
    out_s = rows()
    grads = []
    for _ in h.scales:
        for cin, cout, k, _, _, groups in h.LAYER_TABLE:
            grads += [torch.empty(cout, cin // groups, k, device=gpu), torch.empty(cout, device=gpu)]
    ptrs = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    need = lib.m2_disc_step_workspace_bytes(hd, B, L)
    calls["m2_disc_step"] = (need, [out_s] + grads, lambda ws, n: lib.m2_disc_step(
        hd, real.data_ptr(), fake.data_ptr(), B, L, out_s.data_ptr(), ptrs, ws, n, None))
    out_g, d_fake = rows(), torch.empty(B, 1, L, device=gpu)
    need = lib.m2_disc_gen_step_workspace_bytes(hd, B, L)
    calls["m2_disc_gen_step"] = (need, [out_g, d_fake], lambda ws, n: lib.m2_disc_gen_step(
        hd, real.data_ptr(), fake.data_ptr(), B, L, 1.0, 2.0, out_g.data_ptr(), d_fake.data_ptr(), ws, n, None))
    return calls


DISC_CALLS = ("m2_disc_forward", "m2_disc_forward+features", "m2_disc_losses", "m2_disc_step", "m2_disc_gen_step")


@pytest.mark.parametrize("name", DISC_CALLS)
def test_discriminator_calls(gpu, loss, name):
    """B = 2, L = 3000: one slice, three scales, so the step's pooled buffer exists."""
    h = loss.adversarial_loss.discriminator._handle(gpu)
    need, outputs, call = _disc_calls(gpu, h, 2, 3000)[name]
    _exact(gpu, name.split("+")[0], need, outputs, call)


@pytest.mark.parametrize("name", DISC_CALLS)
def test_discriminator_calls_with_a_short_last_slice(gpu, loss, name):
    """B = 3 under a slice bound that admits two utterances: slices of 2 and 1.  The sizes are
    those of a full slice, and the bound counts one set of maps in forward, two in the others."""
    from m2amd import _lib
    lib = _lib.load()
    h = loss.adversarial_loss.discriminator._handle(gpu)
    L = 3000
    per_utterance = 4 * sum(-(-c * n // 64) * 64 for c, n in h.shapes(L)[0])
    sides = 1 if name.startswith("m2_disc_forward") else 2
    whole = _disc_calls(gpu, h, 3, L)[name][0]
    h.set_slice_bytes(2 * sides * per_utterance + 4)
    try:
        need, outputs, call = _disc_calls(gpu, h, 3, L)[name]
        assert need < whole and need == getattr(lib, name.split("+")[0] + "_workspace_bytes")(h.handle, 2, L)
        _exact(gpu, name.split("+")[0], need, outputs, call)
    finally:
        h.set_slice_bytes(0)


# ---- the spectral loss, the evaluation sums, the DSP calls -----------------------

def test_loss_spectral(gpu, dsp):
    from m2amd import _lib
    lib = _lib.load()
    B, L = 2, 3000
    pred, target = _audio(gpu, B, L, 21), _audio(gpu, B, L, 22)
    out = torch.empty(B, lib.m2_loss_column_count(0), device=gpu, dtype=torch.float64)
    need = lib.m2_loss_spectral_workspace_bytes(dsp.handle, B, L)
    _exact(gpu, "m2_loss_spectral", need, [out], lambda ws, n: lib.m2_loss_spectral(
        dsp.handle, pred.data_ptr(), target.data_ptr(), B, L, None, 0, out.data_ptr(), None, None, ws, n, None))


def test_eval_audio(gpu, dsp):
    from m2amd import _lib
    lib = _lib.load()
    B, L = 2, 3000
    pred, target = _audio(gpu, B, L, 31), _audio(gpu, B, L, 32)
    out = torch.empty(B, lib.m2_eval_column_count(0), device=gpu, dtype=torch.float64)
    need = lib.m2_eval_audio_workspace_bytes(dsp.handle, B, L)
    _exact(gpu, "m2_eval_audio", need, [out], lambda ws, n: lib.m2_eval_audio(
        dsp.handle, pred.data_ptr(), target.data_ptr(), B, L, L, out.data_ptr(), ws, n, None))


def _mel(gpu, dsp, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, dsp.n_mels, T, generator=g) * 2 - 1).to(gpu)  # normalised dB


def test_mel_to_magnitude(gpu, dsp):
    from m2amd import _lib
    lib = _lib.load()
    B, T = 1, 4
    mel = _mel(gpu, dsp, B, T, 41)
    out = torch.empty(B, T, dsp.F, device=gpu)
    need = lib.m2_mel_to_magnitude_workspace_bytes(dsp.handle, B, T)
    _exact(gpu, "m2_mel_to_magnitude", need, [out], lambda ws, n: lib.m2_mel_to_magnitude(
        dsp.handle, mel.data_ptr(), B, T, 20, out.data_ptr(), ws, n, None))


@pytest.mark.parametrize("source", ["mel", "mag"])
def test_griffin_lim(gpu, dsp, source):
    """One size serves both inputs: the NNLS scratch is counted and carved also when the
    magnitudes are given."""
    from m2amd import _lib
    lib = _lib.load()
    B, T = 1, 4
    mel = _mel(gpu, dsp, B, T, 51)
    mag = dsp.mel_to_magnitude(mel, nnls_iters=20).transpose(1, 2).contiguous()  # [B, T, F]
    ang = torch.view_as_real(dsp.random_angles(B, T, seed=5)).contiguous()
    out = torch.empty(B, dsp.hop * (T - 1), device=gpu)
    need = lib.m2_griffin_lim_workspace_bytes(dsp.handle, B, T)
    src = (mel.data_ptr(), None) if source == "mel" else (None, mag.data_ptr())
    _exact(gpu, "m2_griffin_lim", need, [out], lambda ws, n: lib.m2_griffin_lim(
        dsp.handle, *src, ang.data_ptr(), B, T, 2, 0.99, 20, out.data_ptr(), ws, n, None))


def test_mel_features_ragged(gpu, dsp):
    """700 and 1500 samples: 3 + 6 frames, one fewer than the B + total / hop the size counts."""
    from m2amd import _lib
    lib = _lib.load()
    lengths = (700, 1500)
    B, total = len(lengths), sum(lengths)
    samples = _audio(gpu, 1, total, 61).reshape(-1)
    off = torch.tensor([0, lengths[0], total], dtype=torch.int64)
    off_dev = off.to(gpu)
    off_host = ctypes.cast(off.data_ptr(), ctypes.POINTER(ctypes.c_int64))
    T_out = 1 + max(lengths) // dsp.hop
    assert sum(1 + n // dsp.hop for n in lengths) == B + total // dsp.hop - 1
    mel = torch.empty(B, dsp.n_mels, T_out, device=gpu)
    frames = torch.empty(B, dtype=torch.int32, device=gpu)
    need = lib.m2_mel_features_ragged_workspace_bytes(dsp.handle, B, total)
    _exact(gpu, "m2_mel_features_ragged", need, [mel, frames], lambda ws, n: lib.m2_mel_features_ragged(
        dsp.handle, samples.data_ptr(), 0, off_dev.data_ptr(), off_host, B, 1, 0, mel.data_ptr(), T_out,
        frames.data_ptr(), ws, n, None))
