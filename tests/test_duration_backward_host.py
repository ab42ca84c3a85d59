"""Host-side checks of the duration predictor's backward and of
M2TTSModel.enable_backward (no GPU): the masked float64 oracle the GPU tests
compare against equals plain torch autograd of the module's layers in eval
mode; the formulas the kernels implement (softplus' with its threshold branch,
the head's sums, BatchNorm's and ReLU's backward with d gamma formed per
element from u, right where gamma is 0 or negative) reproduce float64 autograd
to 1e-12 relative; the cases' inputs sit on the same side of every ReLU kink in
float32 and float64; the plan (tape, workspace, launch rows, the printed line)
agrees with a restatement of its formulas; the switches are plain attributes
and refuse what the kernels do not take; the entry points are exported and
bound with the header's signatures."""
import ctypes
import re
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from test_ragged_host import header_signature

sys.path.insert(0, str(GOLDEN))
import duration_backward_oracle as orc  # noqa: E402

ENTRIES = {"m2_duration_tape_bytes": 3, "m2_duration_tape_map": 6, "m2_duration_train_forward": 10,
           "m2_duration_backward_workspace_bytes": 3, "m2_duration_backward": 14, "m2_debug_duration_grad_plan": 5}
TOL = 1e-12


def _close(a, b):
    return float((a - b).abs().max()) <= TOL * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("case", list(orc.CASES))
def test_masked_oracle_equals_plain_autograd_with_its_own_masks(case):
    H, B, S, mods = orc.CASES[case]
    pred = orc.cpu_copy(orc.make_predictor(case), torch.float64)
    params = orc.parameters(pred)
    assert len(params) == orc.N_PARAMS and all(a is b for a, b in zip(params, pred.parameters()))
    assert [tuple(p.shape) for p in params] == [(H, H, 3), (H,), (H,), (H,)] * 2 + [(1, H, 1), (1,)]
    enc, d_dur = orc.make_inputs(case)
    enc, d_dur = enc.double(), d_dur.double()
    grads, d_enc, dur, pre = orc.gradients(pred, enc, d_dur)
    plain, plain_d_enc, plain_dur = orc.plain_gradients(pred, enc, d_dur)
    assert dur.shape == (B, S) and _close(dur, plain_dur) and d_enc.shape == (B, S, H) and _close(d_enc, plain_d_enc)
    for g, p in zip(grads, plain):
        assert _close(g, p) and float(p.abs().max()) > 0
    positive = [a > 0 for a in pre]
    again, d_again, _, _ = orc.gradients(pred, enc, d_dur, positive)
    assert all(torch.equal(a, b) for a, b in zip(again, grads)) and torch.equal(d_again, d_enc)
    positive[-1] = ~positive[-1]
    flipped, _, _, _ = orc.gradients(pred, enc, d_dur, positive)
    assert not torch.equal(flipped[0], grads[0])
    assert all(p.grad is None for p in params)
    # the running statistics are constants of the function
    norms = [blk.norm for blk in pred.predictor.conv_layers]
    assert all(not n.running_mean.requires_grad and int(n.num_batches_tracked) == 0 for n in norms)
    assert all(0.3 <= float(n.running_var.min()) and float(n.running_var.max()) <= 2.0 for n in norms)
    assert all(n.eps == (1e-3 if "eps" in mods else 1e-5) for n in norms)
    if "gamma" in mods:
        for i, n in enumerate(norms):
            assert float(n.weight.detach()[orc.GAMMA_ZERO]) == 0.0 and float(n.weight.detach()[orc.GAMMA_NEG]) < 0
            # the dead-gamma channel is alive through its bias: d gamma there is not zero
            assert float(grads[4 * i + 2][orc.GAMMA_ZERO].abs()) > 0 and float(grads[4 * i + 2][orc.GAMMA_NEG].abs()) > 0
            assert bool((pre[i][:, orc.GAMMA_ZERO] > 0).all())
    if "extreme" in mods:
        _, _, _, z = orc.forward(pred, enc)
        assert int((z > 20).sum()) > 0 and int((z < -30).sum()) > 0 and int(((z > -30) & (z < 20)).sum()) > 0


def test_modifiers_cover_the_cases():
    mods = [m for c in orc.CASES.values() for m in c[3]]
    assert {"gamma", "eps", "extreme"} <= set(mods)
    assert [c[:3] for c in orc.CASES.values()] == [(64, 2, 100), (32, 1, 1), (32, 3, 63), (96, 2, 64), (128, 2, 65),
                                                   (64, 1, 130), (16, 2, 7), (24, 2, 33)]


@pytest.mark.parametrize("case", list(orc.CASES))
def test_inputs_take_one_side_of_every_kink_in_both_precisions(case):
    H, B, S, _ = orc.CASES[case]
    pred = orc.make_predictor(case)
    enc, _ = orc.make_inputs(case)
    with torch.no_grad():
        d32, pre32, _, _ = orc.forward(orc.cpu_copy(pred, torch.float32), enc)
        d64, pre64, _, _ = orc.forward(orc.cpu_copy(pred, torch.float64), enc.double())
    differ = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(pre32, pre64))
    total = sum(b.numel() for b in pre64)
    print(f"{case}: {differ} of {total} pre-activations differ in sign")
    assert total == 2 * B * H * S and differ == 0
    assert float((d32.double() - d64).abs().max()) <= 1e-4 * float(d64.abs().max())
    # both sides of the ReLU occur in both blocks
    assert all(0 < int((a > 0).sum()) < a.numel() for a in pre64) or B * S == 1


# ---- the formulas of the kernels ---------------------------------------------------

@pytest.mark.parametrize("case", ["s1", "wide", "thin", "tile"])
def test_formulas_reproduce_autograd(case):
    """g_z = g_dur (z > 20 ? 1 : sigmoid(z)); g_y2 = pw g_z, d pw = sum g_z y2, d pb = sum g_z; per block
    g_a = g_y [y > 0], g_u = g_a alpha, d gamma = sum g_a (u - mean) invstd, d beta = sum g_a; then the conv's
    gradients from g_u; d_enc is conv1's data gradient transposed back."""
    H, B, S, mods = orc.CASES[case]
    pred = orc.cpu_copy(orc.make_predictor(case), torch.float64)
    enc, d_dur = orc.make_inputs(case)
    enc, d_dur = enc.double(), d_dur.double()
    want, want_d_enc, _, _ = orc.gradients(pred, enc, d_dur)
    with torch.no_grad():
        dur, pre, convs, z = orc.forward(pred, enc)
        blocks = pred.predictor.conv_layers
        pw = pred.predictor.projection.weight
        g_z = d_dur * torch.where(z > 20, torch.ones_like(z), torch.sigmoid(z))
        if "extreme" in mods:  # the threshold branch is taken, and softplus there is the identity
            assert int((z > 20).sum()) > 0 and torch.equal(dur[z > 20], z[z > 20])
        y = [a * (a > 0) for a in pre]
        x = [enc.transpose(1, 2), y[0]]
        got = [None] * 10
        got[8] = (g_z[:, None, :] * y[1]).sum((0, 2)).reshape(1, H, 1)
        got[9] = g_z.sum().reshape(1)
        g_y = pw.reshape(1, H, 1) * g_z[:, None, :]
        for i in (1, 0):
            n = blocks[i].norm
            invstd = 1.0 / torch.sqrt(n.running_var + n.eps)
            alpha = n.weight * invstd
            g_a = g_y * (y[i] > 0)
            got[4 * i + 2] = (g_a * (convs[i] - n.running_mean[None, :, None]) * invstd[None, :, None]).sum((0, 2))
            got[4 * i + 3] = g_a.sum((0, 2))
            g_u = g_a * alpha[None, :, None]
            got[4 * i] = torch.nn.grad.conv1d_weight(x[i], (H, H, 3), g_u, padding=1)
            got[4 * i + 1] = g_u.sum((0, 2))
            g_y = torch.nn.grad.conv1d_input((B, H, S), blocks[i].conv.weight, g_u, padding=1)
        d_enc = g_y.transpose(1, 2)
        # alpha and beta' are the affine the forward applies
        n = blocks[0].norm
        a1 = convs[0] * (n.weight / torch.sqrt(n.running_var + n.eps))[None, :, None] + \
            (n.bias - n.running_mean * n.weight / torch.sqrt(n.running_var + n.eps))[None, :, None]
        assert _close(a1, pre[0])
    assert _close(d_enc, want_d_enc)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and _close(g, w), (case, i)
    if "gamma" in mods:  # recovering u from y by dividing by gamma is impossible here, and sum g_a u - mean sum g_a cancels
        assert float(want[2][orc.GAMMA_ZERO].abs()) > 0 and float(want[6][orc.GAMMA_ZERO].abs()) > 0


def test_softplus_derivative_at_the_threshold():
    z = torch.tensor([-100.0, -30.5, -1.0, 0.0, 19.999, 20.0, 20.001, 50.0], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.softplus(z), z, torch.ones_like(z))
    ours = torch.where(z > 20, torch.ones_like(z), torch.sigmoid(z)).detach()
    assert _close(ours, g) and float(ours[-1]) == 1.0 and float(ours[-3]) < 1.0 and 0 < float(ours[0]) < 1e-40


# ---- the plan ----------------------------------------------------------------------

def _cdiv(a, b):
    return -(-a // b)


def _up(n, a=256):
    return _cdiv(n, a) * a


def _conv_dw(H, B, S):
    """losses_plan.h's dw_plan for the geometry {H, H, 3, 1, 1, 1}: (input-channel blocks, splits, LDS bytes,
    floats of partials)."""
    chunks, n = B * _cdiv(S, 64), 3 * H * H
    spanp, dys = (63 + 3) | 1, 16 * 65
    fit = (48 * 1024 // 4 - dys) // spanp
    nci = min(704 // 3, 64, H, fit)
    splits = max(1, min(chunks, 64, 1 + (8 << 20) // n))
    part = splits * n
    cps = _cdiv(chunks, splits)
    return _cdiv(H, nci), _cdiv(chunks, cps), 4 * (nci * spanp + dys), part


def _workspace(H, B, S):
    n = B * H * S
    part = max(B * _cdiv(S, 64) * (3 * H + 1), _conv_dw(H, B, S)[3])
    off = 0
    for f in (n, n, n, n, part, 3 * H * H, H):
        off = _up(off) + 4 * f
    return off + 256, part


def _plan_line(lib, *dims):
    buf = ctypes.create_string_buffer(1 << 14)
    n = lib.m2_debug_duration_grad_plan(*dims, buf, len(buf))
    assert 0 < n < len(buf)
    return buf.value.decode()


def _rows(line):
    return [(m.group(1), m.group(2), tuple(int(v) for v in m.group(3, 4, 5)), int(m.group(6)), int(m.group(7)))
            for m in re.finditer(r"(\w+):(\w+)\[grid=(\d+)x(\d+)x(\d+) thr=(\d+) lds=(\d+)\]", line)]


SWEEP = [(H, B, S) for H in (16, 24, 64, 96, 128) for B in (1, 3, 32) for S in (1, 17, 64, 100, 130, 1025)]


def test_plan_agrees_with_a_restatement():
    from m2amd import _lib
    lib = _lib.load()
    off, width = ctypes.c_size_t(), ctypes.c_int32()
    for dims in SWEEP + [c[:3] for c in orc.CASES.values()] + [(64, 32, 100)]:
        H, B, S = dims
        n = B * H * S
        tape_bytes = _up(4 * n) + 4 * n + 256
        assert lib.m2_duration_tape_bytes(*dims) == tape_bytes
        for i, at in enumerate((0, _up(4 * n) // 4)):
            assert lib.m2_duration_tape_map(*dims, i, ctypes.byref(off), ctypes.byref(width)) == 0
            assert (off.value, width.value) == (at, H) and off.value % 64 == 0
        assert lib.m2_duration_tape_map(*dims, 2, ctypes.byref(off), ctypes.byref(width)) == -1
        ws_bytes, part = _workspace(*dims)
        assert lib.m2_duration_backward_workspace_bytes(*dims) == ws_bytes, dims
        line = _plan_line(lib, *dims)
        assert line.startswith(f"H={H} B={B} S={S} tape={tape_bytes} ws={ws_bytes} part={part} u=recomputed xt:")
        rows = _rows(line)
        assert len(line.split(" ")) == 7 + 3 * len(rows)  # every item after the header is a row
        assert all(lds <= 48 * 1024 for *_, lds in rows)
        assert all(0 < g[0] and 0 < g[1] <= 65535 and 0 < g[2] <= 65535 for _, _, g, _, _ in rows)
        by_step = {}
        for step, kernel, grid, thr, lds in rows:
            by_step.setdefault(step, []).append((kernel, grid, thr, lds))
        assert list(by_step) == ["xt", "u2", "hd", "c2", "u1", "b1", "c1", "dt"]
        fin = lambda k: ("dec_finish_kernel", (_cdiv(k, 32), 1, 1), 256, 0)  # noqa: E731
        chunks = _cdiv(S, 64)
        blocks, splits, dw_lds, _ = _conv_dw(*dims)
        conv = [("conv_dx_mfma_kernel", (_cdiv(S + 1, 64), _cdiv(H, 64), B), 256, 4 * 16 * ((64 + 3 - 1) | 1)),
                ("conv_dw_mfma_kernel", (blocks, _cdiv(H, 16), splits), 256, dw_lds),
                ("dw_finish_kernel", (_cdiv(3 * H * H, 256), 1, 1), 256, 0), ("conv_db_kernel", (H, 1, 1), 1024, 0)]
        fwd = [("conv_kernel", (_cdiv(S, 1024), H // 8, B), 256, 0)]
        assert by_step["xt"] == [("dur_transpose_kernel", (_cdiv(H, 32), _cdiv(S, 32), B), 256, 0)]
        assert by_step["dt"] == [("dur_transpose_kernel", (_cdiv(S, 32), _cdiv(H, 32), B), 256, 0)]
        assert by_step["u2"] == fwd and by_step["u1"] == fwd
        assert by_step["hd"] == [("dur_bn_bwd_kernel", (chunks, B, 1), 256, 4 * 64 * H), fin(H), fin(H), fin(H), fin(1)]
        assert by_step["b1"] == [("dur_bn_bwd_kernel", (chunks, B, 1), 256, 0), fin(H), fin(H)]
        assert by_step["c2"] == conv and by_step["c1"] == conv
    for H in (8, 12, 60, 136, 256, 0, -8):
        assert lib.m2_duration_tape_bytes(H, 1, 4) == 0 and lib.m2_duration_backward_workspace_bytes(H, 1, 4) == 0, H
    assert lib.m2_duration_tape_bytes(64, 1, (1 << 20) + 1) == 0 and lib.m2_duration_tape_bytes(64, 1 << 16, 1) == 0
    assert lib.m2_duration_tape_bytes(128, 8, 1 << 20) > 0 and lib.m2_duration_tape_bytes(128, 16, 1 << 20) == 0  # 2^30 floats a map
    assert lib.m2_duration_tape_bytes(64, 0, 4) == 256 == lib.m2_duration_backward_workspace_bytes(64, 2, 0)


def test_bad_arguments_are_reported():
    from m2amd import _lib
    lib = _lib.load()
    assert lib.m2_duration_train_forward(None, None, 64, None, 1, 4, None, None, 0, None) == -1
    assert b"m2_duration_train_forward" in lib.m2_last_error()
    assert lib.m2_duration_backward(None, None, 64, None, 1, 4, None, None, None, None, 0, None, 0, None) == -1
    assert b"m2_duration_backward" in lib.m2_last_error()
    assert lib.m2_duration_backward(None, None, 60, None, 1, 4, None, None, None, None, 0, None, 0, None) == -2
    assert lib.m2_duration_train_forward(None, None, 136, None, 1, 4, None, None, 0, None) == -2
    assert lib.m2_duration_train_forward(None, None, 64, None, 0, 4, None, None, 0, None) == 0  # nothing to do
    assert lib.m2_duration_backward(None, None, 64, None, 3, 0, None, None, None, None, 0, None, 0, None) == 0
    assert lib.m2_debug_duration_grad_plan(64, 1, 4, None, 0) == -1
    off, width = ctypes.c_size_t(), ctypes.c_int32()
    assert lib.m2_duration_tape_map(60, 1, 4, 0, ctypes.byref(off), ctypes.byref(width)) == -2


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


# ---- the switches ------------------------------------------------------------------

def test_switches_are_plain_attributes():
    from models.tts_model import DurationPredictor, M2TTSModel
    pred = DurationPredictor()
    keys = list(pred.state_dict())
    assert pred.backward_enabled is False and DurationPredictor.backward_enabled is False
    assert pred.enable_backward() is pred and pred.backward_enabled is True
    assert list(pred.state_dict()) == keys and len(keys) == 10 + 2 * 3  # each BatchNorm has three buffers
    names = [n for n, _ in pred.named_parameters()]
    assert names == [f"predictor.conv_layers.{i}.{n}" for i in (0, 1)
                     for n in ("conv.weight", "conv.bias", "norm.weight", "norm.bias")] + \
        ["predictor.projection.weight", "predictor.projection.bias"]
    assert "backward_enabled" not in dict(pred.named_buffers()) and "backward_enabled" not in dict(pred.named_parameters())
    assert pred.enable_backward(False) is pred and pred.backward_enabled is False
    assert pred.enable_backward(enabled=True).backward_enabled is True
    assert DurationPredictor.backward_enabled is False  # the switch follows the instance
    with pytest.raises(RuntimeError, match="ROCm GPU"):  # with the switch on, CPU tensors are refused
        pred(torch.zeros(1, 4, 64))

    model = M2TTSModel()
    keys = list(model.state_dict())
    stages = (model.text_encoder, model.duration_predictor, model.length_regulator, model.decoder)
    assert model.backward_enabled is False and M2TTSModel.backward_enabled is False
    assert not any(s.backward_enabled for s in stages) and model.vocoder.backward_enabled is False
    assert model.enable_backward() is model and model.backward_enabled is True
    assert all(s.backward_enabled for s in stages) and model.vocoder.backward_enabled is False  # the caller's
    assert list(model.state_dict()) == keys
    assert model.enable_backward(False) is model and model.backward_enabled is False
    assert not any(s.backward_enabled for s in stages)
    assert M2TTSModel.backward_enabled is False
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        model.enable_backward()(torch.zeros(1, 4, dtype=torch.int64))


def test_enable_backward_raises_on_an_unsupported_shape():
    from models.tts_model import DurationPredictor, M2TTSModel
    for bad in (dict(hidden_dim=8), dict(hidden_dim=60), dict(hidden_dim=136), dict(hidden_dim=64, kernel_size=5),
                dict(hidden_dim=64, kernel_size=1)):
        pred = DurationPredictor(**bad)
        with pytest.raises(NotImplementedError, match="kernel size 3 and hidden_dim a multiple of 8 from 16 to 128"):
            pred.enable_backward()
        assert pred.backward_enabled is False and pred.enable_backward(False).backward_enabled is False
    for h in (16, 24, 128):
        assert DurationPredictor(hidden_dim=h).enable_backward().backward_enabled
    # a refusal from any stage propagates, and then nothing is switched
    model = M2TTSModel(hidden_dim=160, num_heads=4)  # the stacks take H <= 128
    with pytest.raises(NotImplementedError):
        model.enable_backward()
    stages = (model.text_encoder, model.duration_predictor, model.length_regulator, model.decoder)
    assert model.backward_enabled is False and not any(s.backward_enabled for s in stages)
    model = M2TTSModel(hidden_dim=64, num_heads=8)  # the encoder refuses head_dim 8 first
    model.length_regulator.enable_backward()
    with pytest.raises(NotImplementedError):
        model.enable_backward()
    assert model.length_regulator.backward_enabled is True and not model.text_encoder.backward_enabled
    assert not model.duration_predictor.backward_enabled and not model.decoder.backward_enabled
