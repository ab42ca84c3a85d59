"""Host-side checks of the vocoder's backward (no GPU): the masked float64
oracle the GPU tests compare against equals plain torch autograd when its masks
come from itself; the ConvTranspose1d gradients are the strided Conv1d forms
with the roles swapped, exactly; the cases' inputs sit on the same side of
every LeakyReLU kink in float32 and float64; the plan (tape, workspace, launch
rows) agrees with a restatement of its formulas; the switch is a plain
attribute; the entry points are exported and bound with the header's
signatures."""
import ctypes
import re
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from test_ragged_host import header_signature

sys.path.insert(0, str(GOLDEN))
import vocoder_backward_oracle as orc  # noqa: E402

ENTRIES = {"m2_vocoder_tape_bytes": 4, "m2_vocoder_tape_map": 8, "m2_vocoder_train_forward": 10,
           "m2_vocoder_backward_workspace_bytes": 4, "m2_vocoder_backward": 14, "m2_debug_vocoder_grad_plan": 6,
           "m2_vocoder_out_backward_workspace_bytes": 3, "m2_vocoder_out_backward": 13, "m2_resblock_backward": 11,
           "m2_conv1d_narrow_dw_workspace_bytes": 7, "m2_conv1d_narrow_dw": 14}
RATES = (4, 4, 2, 2)


@pytest.mark.parametrize("case", list(orc.CASES))
def test_masked_oracle_equals_plain_autograd_with_its_own_masks(case):
    voc = orc.cpu_copy(orc.make_vocoder(case), torch.float64)
    assert len(orc.parameters(voc)) == 28
    assert [tuple(p.shape) for p in orc.parameters(voc)] == [tuple(v.shape) for v in voc.state_dict().values()]
    mel, dy = (t.double() for t in orc.make_inputs(case))
    grads, d_mel, audio, pre = orc.gradients(voc, mel, dy)
    plain, plain_mel, plain_audio = orc.plain_gradients(voc, mel, dy)
    assert float((audio - plain_audio).abs().max()) <= 1e-12
    for g, p in zip(grads + [d_mel], plain + [plain_mel]):
        assert float((g - p).abs().max()) <= 1e-12 * float(p.abs().max())
        assert float(p.abs().max()) > 0
    # masks given explicitly reproduce it bit for bit, and a flipped mask element changes the result
    positive = {k: v > 0 for k, v in pre.items()}
    again, again_mel, _, _ = orc.gradients(voc, mel, dy, positive)
    assert all(torch.equal(a, b) for a, b in zip(again + [again_mel], grads + [d_mel]))
    positive["v3"] = ~positive["v3"]
    flipped, _, _, _ = orc.gradients(voc, mel, dy, positive)
    assert not torch.equal(flipped[0], grads[0])
    assert all(p.grad is None for p in orc.parameters(voc))


@pytest.mark.parametrize("r,cin,cout,L", [(4, 6, 3, 5), (2, 4, 2, 7), (4, 3, 5, 1)])
def test_conv_transpose_gradients_are_the_strided_conv_forms(r, cin, cout, L):
    """g_x = conv1d(g_u, WT read as [Cout' = Cin_T, Cin' = Cout_T, 2r], stride r, padding r/2), and dWT is
    that Conv1d's weight gradient with input g_u and dy x: to 0.0 in float64."""
    g = torch.Generator().manual_seed(r * 100 + cin)
    x = torch.randn(2, cin, L, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cin, cout, 2 * r, generator=g, dtype=torch.float64, requires_grad=True)
    g_u = torch.randn(2, cout, L * r, generator=g, dtype=torch.float64)
    u = F.conv_transpose1d(x, w, None, stride=r, padding=r // 2)
    assert u.shape == g_u.shape
    gx, gw = torch.autograd.grad(u, (x, w), g_u)
    w2 = w.detach().clone().requires_grad_(True)
    y = F.conv1d(g_u, w2, None, stride=r, padding=r // 2)
    assert y.shape == x.shape  # the output length is exactly L
    assert float((y.detach() - gx).abs().max()) == 0.0
    (gw2,) = torch.autograd.grad(y, (w2,), x.detach())
    assert gw2.shape == w.shape  # it comes out in ConvT layout
    assert float((gw2 - gw).abs().max()) == 0.0


@pytest.mark.parametrize("case", list(orc.CASES))
def test_inputs_take_one_side_of_every_kink_in_both_precisions(case):
    """The condition on the inputs: CPU float32 and float64 forwards take the same LeakyReLU side at
    every element, and tanh is nowhere saturated."""
    voc = orc.make_vocoder(case)
    mel, dy = orc.make_inputs(case)
    with torch.no_grad():
        y32, pre32 = orc.forward(orc.cpu_copy(voc, torch.float32), mel)
        y64, pre64 = orc.forward(orc.cpu_copy(voc, torch.float64), mel.double())
    total = sum(v.numel() for v in pre64.values())
    differ = sum(int(((pre32[k] > 0) != (pre64[k] > 0)).sum()) for k in orc.PRE)
    s_fwd = max(float((pre32[k].double() - pre64[k]).abs().max()) / float(pre64[k].abs().max()) for k in orc.PRE)
    print(f"{case}: {differ} of {total} pre-activations differ in sign; forward s {s_fwd:.2e}; "
          f"max|y| {float(y64.abs().max()):.3f}")
    M, C, B, T, _ = orc.CASES[case]
    assert total == 2 * B * sum((C >> (k + 1)) * T * n for k, n in enumerate((4, 16, 32, 64)))
    assert differ == 0
    assert float(y64.abs().max()) <= 0.9 and float((y32.double() - y64).abs().max()) <= 1e-5


# ---- the plan ----------------------------------------------------------------------

def _cdiv(a, b):
    return -(-a // b)


def _up(n, a=256):
    return _cdiv(n, a) * a


def _maps(M, C, B, T):
    out = [(C, T)]
    L = T
    for k, r in enumerate(RATES):
        L *= r
        out += [(C >> (k + 1), L)] * 3
    return out + [(1, 64 * T)]


def _tape_layout(M, C, B, T):
    off, at = 0, []
    for c, n in _maps(M, C, B, T):
        off = _up(off)
        at.append(off // 4)
        off += 4 * B * c * n
    return at, off + 256


def _dw_part(cin, cout, k, stride, pad, B, L):
    """Floats of partials of one weight gradient: split-K copies on the MFMA, (dw, db) per split below 16 rows."""
    Lo = (L + 2 * pad - k) // stride + 1
    n = cout * cin * k
    if cout < 16:
        chunks = B * _cdiv(Lo, 256)
        cps = _cdiv(chunks, min(chunks, 512))
        return _cdiv(chunks, cps) * (n + cout)
    return max(1, min(B * _cdiv(Lo, 64), 64, 1 + (8 << 20) // n)) * n


def _res_width(c):
    return next(W for W in (256, 128, 64, 32) if c * (2 * W + 2) * 4 <= 48 * 1024)


def _workspace(M, C, B, T):
    widest = max(c * n for c, n in _maps(M, C, B, T))
    part = B * _cdiv(64 * T, 1024) * (3 * (C >> 4) + 1)
    L = T
    for k, r in enumerate(RATES):
        L *= r
        c = C >> (k + 1)
        part = max(part, _dw_part(c, c, 3, 1, 1, B, L), _dw_part(c, C >> k, 2 * r, r, r // 2, B, L))
    part = max(part, _dw_part(M, C, 3, 1, 1, B, T))
    off = 0
    weight = max(3 * C * M, 4 * C * C)  # the input conv, or ConvT_0 [C, C/2, 8]
    for n in (B * widest,) * 3 + (part, weight, C):
        off = _up(off) + 4 * n
    return off + 256, B * widest, part


def _plan_line(lib, M, C, B, T):
    buf = ctypes.create_string_buffer(1 << 15)
    n = lib.m2_debug_vocoder_grad_plan(M, C, B, T, buf, len(buf))
    assert 0 < n < len(buf)
    return buf.value.decode()


def _rows(line):
    return [(m.group(1), m.group(2), tuple(int(v) for v in m.group(3, 4, 5)), int(m.group(6)), int(m.group(7)))
            for m in re.finditer(r"(\w+):(\w+)\[grid=(\d+)x(\d+)x(\d+) thr=(\d+) lds=(\d+)\]", line)]


SWEEP = [(M, C, B, T) for (M, C) in ((64, 16), (5, 32), (64, 128), (80, 256)) for B in (1, 3, 32) for T in (1, 17, 70, 500)]


def test_plan_agrees_with_a_restatement():
    from m2amd import _lib
    lib = _lib.load()
    off, ch, n = ctypes.c_size_t(), ctypes.c_int32(), ctypes.c_int32()
    for M, C, B, T in SWEEP + [c[:4] for c in orc.CASES.values()]:
        at, tape_bytes = _tape_layout(M, C, B, T)
        assert lib.m2_vocoder_tape_bytes(M, C, B, T) == tape_bytes
        for i, (c, length) in enumerate(_maps(M, C, B, T)):
            assert lib.m2_vocoder_tape_map(M, C, B, T, i, ctypes.byref(off), ctypes.byref(ch), ctypes.byref(n)) == 0
            assert (off.value, ch.value, n.value) == (at[i], c, length), (M, C, B, T, i)
        assert lib.m2_vocoder_tape_map(M, C, B, T, 14, ctypes.byref(off), ctypes.byref(ch), ctypes.byref(n)) == -1
        ws_bytes, cot, part = _workspace(M, C, B, T)
        assert lib.m2_vocoder_backward_workspace_bytes(M, C, B, T) == ws_bytes, (M, C, B, T)
        line = _plan_line(lib, M, C, B, T)
        assert line.startswith(f"M={M} C={C} B={B} T={T} tape={tape_bytes} ws={ws_bytes} cot={cot} part={part} out:")
        rows = _rows(line)
        assert len(line.split(" ")) == 8 + 3 * len(rows)  # every item after the header is a row
        assert all(lds <= 48 * 1024 and thr in (256, 1024) for *_, thr, lds in rows)
        assert all(0 < g[0] and 0 < g[1] <= 65535 and 0 < g[2] <= 65535 for _, _, g, _, _ in rows)
        by_step = {}
        for step, kernel, grid, thr, lds in rows:
            by_step.setdefault(step, []).append((kernel, grid, thr, lds))
        assert list(by_step) == ["out"] + [f"{s}{k}" for k in (3, 2, 1, 0)
                                           for s in ("res", "c2w", "c1w", "upb", "upw", "updx")] + ["in"]
        assert by_step["out"][0] == ("voc_out_bwd_kernel", (_cdiv(64 * T, 1024), B, 1), 256, 1026 * 4)
        L = T
        for k, r in enumerate(RATES):
            L *= r
            c = C >> (k + 1)
            W = _res_width(c)
            assert by_step[f"res{k}"] == [("voc_res_dx_kernel", (_cdiv(L, W - 2), B, 1), 256, c * (2 * W + 2) * 4)]
            for s in ("c2w", "c1w"):
                first = by_step[f"{s}{k}"][0][0]
                assert first == ("voc_dw_narrow_kernel" if c < 16 else "conv_dw_mfma_kernel"), (C, k)
                assert len(by_step[f"{s}{k}"]) == 3  # partials, the weight's finish, the bias
            assert by_step[f"upw{k}"][0][0] == ("voc_dw_narrow_kernel" if (C >> k) < 16 else "conv_dw_mfma_kernel")
            assert by_step[f"upb{k}"] == [("conv_db_kernel", (c, 1, 1), 1024, 0)]
    assert lib.m2_vocoder_tape_bytes(64, 120, 1, 4) == 0 and lib.m2_vocoder_tape_bytes(64, 8, 1, 4) == 0
    assert lib.m2_vocoder_tape_bytes(0, 128, 1, 4) == 0 and lib.m2_vocoder_backward_workspace_bytes(64, 100, 1, 4) == 0
    assert lib.m2_vocoder_tape_bytes(64, 128, 0, 4) == 256 == lib.m2_vocoder_backward_workspace_bytes(64, 128, 2, 0)
    # about 10.7 MB of tape per utterance at stage1, T = 500, twice that at stage2
    assert 10.5e6 < lib.m2_vocoder_tape_bytes(64, 128, 1, 500) < 11.2e6
    assert 21e6 < lib.m2_vocoder_tape_bytes(80, 256, 1, 500) < 22.4e6


@pytest.mark.parametrize("dims", [(64, 128, 32, 500), (80, 256, 8, 500)])
def test_training_shapes_take_no_direct_kernel(dims):
    from m2amd import _lib
    line = _plan_line(_lib.load(), *dims)
    assert "conv_dw_direct_kernel" not in line and "conv_dx_direct_kernel" not in line
    kernels = {k for _, k, *_ in _rows(line)}
    assert {"voc_out_bwd_kernel", "voc_res_dx_kernel", "conv_dw_mfma_kernel", "conv_mfma_kernel", "conv_dx_mfma_kernel",
            "dw_finish_kernel", "conv_db_kernel"} <= kernels
    assert ("voc_dw_narrow_kernel" in kernels) == (dims[1] == 128)  # stage1's 8-channel stage


def test_bad_arguments_are_reported():
    from m2amd import _lib
    lib = _lib.load()
    assert lib.m2_vocoder_train_forward(None, 64, 128, None, 1, 4, None, None, 0, None) == -1
    assert b"m2_vocoder_train_forward" in lib.m2_last_error()
    assert lib.m2_vocoder_backward(None, 64, 128, None, 1, 4, None, None, None, None, 0, None, 0, None) == -1
    assert b"m2_vocoder_backward" in lib.m2_last_error()
    assert lib.m2_vocoder_backward(None, 64, 120, None, 1, 4, None, None, None, None, 0, None, 0, None) == -2
    assert lib.m2_vocoder_train_forward(None, 64, 128, None, 0, 4, None, None, 0, None) == 0  # nothing to do
    assert lib.m2_vocoder_backward(None, 64, 128, None, 3, 0, None, None, None, None, 0, None, 0, None) == 0
    assert lib.m2_debug_vocoder_grad_plan(64, 128, 1, 4, None, 0) == -1
    assert lib.m2_conv1d_narrow_dw_workspace_bytes(3, 1, 1, 2, 16, 16, 100) == 0  # 16 rows go to the MFMA
    assert lib.m2_conv1d_narrow_dw_workspace_bytes(3, 1, 1, 2, 8, 8, 100) == 2 * (8 * 8 * 3 + 8) * 4 + 256


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entry_points_exported_and_bound(name):
    from m2amd import _lib
    lib = _lib.load()
    assert hasattr(lib, name), f"{name} is not exported by the library"
    assert name in _lib.exported_symbols()
    res, args = header_signature(name)
    assert _lib._SIGNATURES[name] == (res, args) and len(args) == ENTRIES[name]
    fn = getattr(lib, name)
    assert fn.restype is res and list(fn.argtypes) == args
    assert lib.m2_abi_version() == 1


def test_switch_is_a_plain_attribute():
    from models.tts_model import M2TTSModel, SimpleVocoder
    voc = SimpleVocoder()
    keys = list(voc.state_dict())
    assert voc.backward_enabled is False and SimpleVocoder.backward_enabled is False
    assert voc.enable_backward() is voc and voc.backward_enabled is True
    assert list(voc.state_dict()) == keys and len(keys) == 28
    assert keys[:4] == ["input_conv.weight", "input_conv.bias", "upsamples.0.weight", "upsamples.0.bias"]
    assert keys[10:14] == ["resblocks.0.conv1.weight", "resblocks.0.conv1.bias", "resblocks.0.conv2.weight",
                           "resblocks.0.conv2.bias"] and keys[26:] == ["output_conv.weight", "output_conv.bias"]
    assert "backward_enabled" not in dict(voc.named_buffers()) and "backward_enabled" not in dict(voc.named_parameters())
    assert voc.enable_backward(False) is voc and voc.backward_enabled is False
    assert voc.enable_backward(enabled=True).backward_enabled is True
    assert SimpleVocoder.backward_enabled is False  # the switch follows the instance
    with pytest.raises(NotImplementedError):
        SimpleVocoder(kernel_size=5).enable_backward()
    assert SimpleVocoder(kernel_size=5).enable_backward(False).backward_enabled is False
    model = M2TTSModel()
    assert model.vocoder.backward_enabled is False and model.vocoder.enable_backward() is model.vocoder
    assert len(model.vocoder.state_dict()) == 28
    # with the switch on, CPU tensors are refused: there is no CPU path
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        voc(torch.zeros(1, 64, 4))
