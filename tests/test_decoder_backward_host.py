"""Host-side checks of the mel decoder's backward (no GPU): the masked float64
oracle the GPU tests compare against equals plain torch autograd when its masks
come from itself; the hand-written backward formulas the kernels implement
(the LayerNorm-backward epilogue, the dS rule of the attention including a
fully masked row, the weight gradient over a re-formed LayerNorm) reproduce
float64 autograd to 1e-12 relative; the cases' inputs sit on the same side of
every ReLU kink in float32 and float64; the plan (tape, workspace, launch rows)
agrees with a restatement of its formulas; the switch is a plain attribute; the
entry points are exported and bound with the header's signatures."""
import ctypes
import re
import sys

import pytest
import torch

from conftest import GOLDEN
from test_ragged_host import header_signature

sys.path.insert(0, str(GOLDEN))
import decoder_backward_oracle as orc  # noqa: E402

ENTRIES = {"m2_decoder_tape_bytes": 6, "m2_decoder_tape_map": 9, "m2_decoder_train_forward": 12,
           "m2_decoder_backward_workspace_bytes": 6, "m2_decoder_backward": 16, "m2_debug_decoder_grad_plan": 8,
           "m2_attention_backward_workspace_bytes": 3, "m2_attention_backward": 12,
           "m2_linear_backward_input_workspace_bytes": 2, "m2_linear_backward_input": 15,
           "m2_linear_backward_weight_workspace_bytes": 3, "m2_linear_backward_weight": 12}
TOL = 1e-12
EPS = 1e-5


def _close(a, b):
    return float((a - b).abs().max()) <= TOL * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("case", list(orc.CASES))
def test_masked_oracle_equals_plain_autograd_with_its_own_masks(case):
    H, M, layers, heads, B, T = orc.CASES[case]
    dec = orc.cpu_copy(orc.make_decoder(case), torch.float64)
    assert len(orc.parameters(dec)) == 11 * layers + 4
    assert [tuple(p.shape) for p in orc.parameters(dec)] == [tuple(v.shape) for v in dec.state_dict().values()]
    x, dy = (t.double() for t in orc.make_inputs(case))
    grads, d_x, mel, pre = orc.gradients(dec, x, dy)
    plain, plain_x, plain_mel = orc.plain_gradients(dec, x, dy)
    assert mel.shape == (B, T, M) and _close(mel, plain_mel)
    for g, p in zip(grads + [d_x], plain + [plain_x]):
        assert _close(g, p) and float(p.abs().max()) > 0
    positive = [u > 0 for u in pre]
    again, again_x, _, _ = orc.gradients(dec, x, dy, positive)
    assert all(torch.equal(a, b) for a, b in zip(again + [again_x], grads + [d_x]))
    positive[-1] = ~positive[-1]
    flipped, _, _, _ = orc.gradients(dec, x, dy, positive)
    assert not torch.equal(flipped[0], grads[0])
    assert all(p.grad is None for p in orc.parameters(dec))


@pytest.mark.parametrize("case", list(orc.CASES))
def test_inputs_take_one_side_of_every_kink_in_both_precisions(case):
    dec = orc.make_decoder(case)
    x, _ = orc.make_inputs(case)
    with torch.no_grad():
        y32, pre32 = orc.forward(orc.cpu_copy(dec, torch.float32), x)
        y64, pre64 = orc.forward(orc.cpu_copy(dec, torch.float64), x.double())
    differ = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(pre32, pre64))
    total = sum(b.numel() for b in pre64)
    print(f"{case}: {differ} of {total} pre-activations differ in sign")
    H, M, layers, heads, B, T = orc.CASES[case]
    assert total == layers * B * T * 2 * H and differ == 0
    assert float((y32.double() - y64).abs().max()) <= 1e-4 * float(y64.abs().max())
    # no parameter is at its degenerate initial value
    sd = dec.state_dict()
    assert float((sd["norm.weight"] - 1).abs().min()) > 0 and float(sd["mel_projection.bias"].abs().min()) > 0


# ---- the formulas of the kernels ---------------------------------------------------

@pytest.mark.parametrize("R,K,N,res", [(7, 64, 192, True), (5, 96, 80, False), (3, 32, 5, True)])
def test_layer_norm_backward_epilogue(R, K, N, res):
    """g_x = g_res + rstd (a - mean_k(a) - x^ mean_k(a x^)), a = g_n gamma; dgamma = sum_r g_n x^,
    dbeta = sum_r g_n, for y = LN(x) W^T + (x as the residual branch)."""
    g = torch.Generator().manual_seed(R * K + N)
    x = torch.randn(R, K, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (torch.randn(K, generator=g, dtype=torch.float64) * 0.2 + 1).requires_grad_()
    beta = (torch.randn(K, generator=g, dtype=torch.float64) * 0.2).requires_grad_()
    w = torch.randn(N, K, generator=g, dtype=torch.float64)
    g_y = torch.randn(R, N, generator=g, dtype=torch.float64)
    g_res = torch.randn(R, K, generator=g, dtype=torch.float64) if res else None
    y = torch.nn.functional.layer_norm(x, (K,), gamma, beta, EPS) @ w.t()
    outs, cots = ([y, x], [g_y, g_res]) if res else ([y], [g_y])
    want = torch.autograd.grad(outs, (x, gamma, beta), cots)
    with torch.no_grad():
        mean = x.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + EPS)
        xh = (x - mean) * rstd
        g_n = g_y @ w
        a = g_n * gamma
        g_x = rstd * (a - a.mean(1, keepdim=True) - xh * (a * xh).mean(1, keepdim=True))
        if res:
            g_x = g_res + g_x
        got = (g_x, (g_n * xh).sum(0), g_n.sum(0))
    assert all(_close(p, q) for p, q in zip(got, want))


@pytest.mark.parametrize("R,K,N", [(9, 64, 192), (4, 96, 80), (70, 32, 5)])
def test_weight_gradient_over_a_reformed_layer_norm(R, K, N):
    g = torch.Generator().manual_seed(R + K + N)
    x = torch.randn(R, K, generator=g, dtype=torch.float64)
    gamma = torch.randn(K, generator=g, dtype=torch.float64) * 0.2 + 1
    beta = torch.randn(K, generator=g, dtype=torch.float64) * 0.2
    w = torch.randn(N, K, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    g_y = torch.randn(R, N, generator=g, dtype=torch.float64)
    y = torch.nn.functional.layer_norm(x, (K,), gamma, beta, EPS) @ w.t() + b
    want = torch.autograd.grad(y, (w, b), g_y)
    mean = x.mean(1, keepdim=True)
    xn = (x - mean) / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + EPS) * gamma + beta
    assert _close(g_y.t() @ xn, want[0]) and _close(g_y.sum(0), want[1])


def attention_backward_by_hand(qkv, heads, key_mask, d_att):
    """The kernels' formulas in the tensor's own dtype: P from the replaced scores, dP = dO V^T,
    D = sum_d dO o, dS = P (dP - D) with dS of a masked key 0 by definition, dQ = scale dS K,
    dK = scale dS^T Q, dV = P^T dO."""
    B, N, H3 = qkv.shape
    H = H3 // 3
    hd = H // heads
    scale = 1.0 / hd ** 0.5
    q, k, v = (t.reshape(B, N, heads, hd).transpose(1, 2) for t in qkv.split(H, dim=-1))
    dO = d_att.reshape(B, N, heads, hd).transpose(1, 2)
    s = q @ k.transpose(-2, -1) * scale
    live = torch.ones(B, 1, 1, N, dtype=torch.bool) if key_mask is None else (key_mask.reshape(B, 1, 1, N) != 0)
    s = torch.where(live, s, torch.full((), -1e9, dtype=s.dtype))
    P = torch.softmax(s, dim=-1)
    dP = dO @ v.transpose(-2, -1)
    D = (dO * (P @ v)).sum(-1, keepdim=True)
    dS = torch.where(live, P * (dP - D), torch.zeros((), dtype=s.dtype))
    parts = (scale * dS @ k, scale * dS.transpose(-2, -1) @ q, P.transpose(-2, -1) @ dO)
    return torch.cat([t.transpose(1, 2).reshape(B, N, H) for t in parts], dim=-1)


@pytest.mark.parametrize("hd,N", [(16, 5), (48, 9), (64, 2), (32, 1)])
def test_attention_ds_rule_including_a_fully_masked_row(hd, N):
    heads, B = 2, 3
    H = heads * hd
    g = torch.Generator().manual_seed(hd + N)
    qkv = torch.randn(B, N, 3 * H, generator=g, dtype=torch.float64)
    d_att = torch.randn(B, N, H, generator=g, dtype=torch.float64)
    lengths = torch.tensor([N, max(1, N // 2), 0])
    mask = torch.arange(N)[None, :] < lengths[:, None]
    for m in (None, mask):
        leaf = qkv.clone().requires_grad_()
        (want,) = torch.autograd.grad(orc.attention(leaf, heads, m), leaf, d_att)
        got = attention_backward_by_hand(qkv, heads, m, d_att)
        assert _close(got, want)
    # utterance 2 is fully masked: P = 1 / N, so dQ and dK are exactly 0 and dV is not
    assert float(got[2, :, :2 * H].abs().max()) == 0.0 and float(want[2, :, :2 * H].abs().max()) == 0.0
    assert float(got[2, :, 2 * H:].abs().max()) > 0


# ---- the plan ----------------------------------------------------------------------

def _cdiv(a, b):
    return -(-a // b)


def _up(n, a=256):
    return _cdiv(n, a) * a


def _widths(H, layers):
    return [3 * H, H, H, 2 * H, H] * layers


def _tape_layout(H, layers, B, T):
    off, at = 0, []
    for w in _widths(H, layers):
        off = _up(off)
        at.append(off // 4)
        off += 4 * B * T * w
    return at, off + 256


def _dw_split(R, N):
    """(64-row tiles of N, workgroups over R): enough of them to cover 256 compute units, 32-row chunks."""
    tiles, chunks = _cdiv(N, 64), _cdiv(R, 32)
    want = max(1, min(chunks, _cdiv(256, tiles)))
    rps = _cdiv(chunks, want) * 32
    return tiles, _cdiv(R, rps)


def _b_stride(K):
    kt = _cdiv(K, 16)
    return 16 * kt + (16 if kt % 2 == 0 else 0)


def _workspace(H, M, layers, heads, B, T):
    R = B * T
    part = _cdiv(R, 64) * 2 * H  # the LayerNorm slots
    for K, N in ((H, M), (2 * H, H), (H, 2 * H), (H, H), (H, 3 * H)):
        part = max(part, _dw_split(R, N)[1] * (N * K + N))
    off = 0
    for n in (R * H, R * H, R * 3 * H, B * heads * T * 3, part):
        off = _up(off) + 4 * n
    return off + 256, part


def _plan_line(lib, *dims):
    buf = ctypes.create_string_buffer(1 << 16)
    n = lib.m2_debug_decoder_grad_plan(*dims, buf, len(buf))
    assert 0 < n < len(buf)
    return buf.value.decode()


def _rows(line):
    return [(m.group(1), m.group(2), tuple(int(v) for v in m.group(3, 4, 5)), int(m.group(6)), int(m.group(7)))
            for m in re.finditer(r"(\w+):(\w+)\[grid=(\d+)x(\d+)x(\d+) thr=(\d+) lds=(\d+)\]", line)]


SWEEP = [(H, M, layers, heads, B, T) for (H, M, layers, heads) in ((64, 64, 2, 2), (96, 80, 3, 2), (32, 5, 1, 2),
                                                                   (128, 80, 1, 2), (64, 64, 1, 4))
         for B in (1, 3, 32) for T in (1, 17, 130, 500)]


def test_plan_agrees_with_a_restatement():
    from m2amd import _lib
    lib = _lib.load()
    off, width = ctypes.c_size_t(), ctypes.c_int32()
    for dims in SWEEP + list(orc.CASES.values()):
        H, M, layers, heads, B, T = dims
        R = B * T
        at, tape_bytes = _tape_layout(H, layers, B, T)
        assert lib.m2_decoder_tape_bytes(*dims) == tape_bytes
        for i, w in enumerate(_widths(H, layers)):
            assert lib.m2_decoder_tape_map(*dims, i, ctypes.byref(off), ctypes.byref(width)) == 0
            assert (off.value, width.value) == (at[i], w) and off.value % 64 == 0, (dims, i)
        assert lib.m2_decoder_tape_map(*dims, 5 * layers, ctypes.byref(off), ctypes.byref(width)) == -1
        ws_bytes, part = _workspace(*dims)
        assert lib.m2_decoder_backward_workspace_bytes(*dims) == ws_bytes, dims
        line = _plan_line(lib, *dims)
        assert line.startswith(f"H={H} M={M} layers={layers} heads={heads} B={B} T={T} tape={tape_bytes} "
                               f"ws={ws_bytes} part={part} mw:")
        rows = _rows(line)
        assert len(line.split(" ")) == 9 + 3 * len(rows)  # every item after the header is a row
        assert all(lds <= 48 * 1024 and thr == 256 for *_, thr, lds in rows)
        assert all(0 < g[0] and 0 < g[1] <= 65535 and 0 < g[2] <= 65535 for _, _, g, _, _ in rows)
        by_step = {}
        for step, kernel, grid, thr, lds in rows:
            by_step.setdefault(step, []).append((kernel, grid))
        assert list(by_step) == ["mw", "mx"] + [f"{s}{l}" for l in reversed(range(layers))
                                                for s in ("l2w", "l2x", "l1w", "l1x", "ow", "ox", "att", "qw", "qx")]
        fin = lambda n: ("dec_finish_kernel", (_cdiv(n, 32), 1, 1))  # noqa: E731
        dw = lambda K, N, bias: ([("lin_dw_kernel", _dw_split(R, N) + (1,)), fin(N * K)]  # noqa: E731
                                 + ([fin(N)] if bias else []))
        dx = lambda ln: [("lin_dx_kernel", (_cdiv(R, 64), 1, 1))] + ([fin(H), fin(H)] if ln else [])  # noqa: E731
        att = [(k, (_cdiv(T, 64), heads, B)) for k in ("att_bwd_q_kernel", "att_bwd_kv_kernel")]
        assert by_step["mw"] == dw(H, M, True) and by_step["mx"] == dx(True)
        for l in range(layers):
            assert by_step[f"l2w{l}"] == dw(2 * H, H, True) and by_step[f"l2x{l}"] == dx(False)
            assert by_step[f"l1w{l}"] == dw(H, 2 * H, True) and by_step[f"l1x{l}"] == dx(True)
            assert by_step[f"ow{l}"] == dw(H, H, True) and by_step[f"ox{l}"] == dx(False)
            assert by_step[f"att{l}"] == att
            assert by_step[f"qw{l}"] == dw(H, 3 * H, False) and by_step[f"qx{l}"] == dx(True)
        lds = {k: v for _, k, _, _, v in rows}
        assert lds["lin_dw_kernel"] in {4 * 32 * (65 + _b_stride(K)) for K in (H, 2 * H)}
        assert lds["att_bwd_q_kernel"] == lds["att_bwd_kv_kernel"] == 4 * (2 * (H // heads) * 68 + 192)
    bad = [(60, 64, 2, 2), (160, 64, 2, 2), (64, 64, 2, 8), (64, 0, 2, 2), (64, 64, 0, 2), (64, 64, 2, 3)]
    for d in bad:
        assert lib.m2_decoder_tape_bytes(*d, 1, 4) == 0 and lib.m2_decoder_backward_workspace_bytes(*d, 1, 4) == 0, d
    assert lib.m2_decoder_tape_bytes(64, 64, 2, 2, 0, 4) == 256 == lib.m2_decoder_backward_workspace_bytes(64, 64, 2, 2, 2, 0)


@pytest.mark.parametrize("dims", [(64, 64, 2, 2, 32, 500), (96, 80, 3, 2, 32, 500)])
def test_training_shapes_cover_the_part(dims):
    """Every weight gradient's grid covers the part's 256 compute units at R = 16000, whatever the
    layer's width: a workgroup takes whole 32-row chunks, and that rounding (500 chunks over 256 workgroups
    are 2 each, 250 workgroups) leaves fewer than a sixteenth of them idle."""
    from m2amd import _lib
    rows = _rows(_plan_line(_lib.load(), *dims))
    grids = [g for _, k, g, _, _ in rows if k == "lin_dw_kernel"]
    assert len(grids) == 1 + 4 * dims[2] and all(g[0] * g[1] >= 240 for g in grids)
    assert {k for _, k, *_ in rows} == {"lin_dw_kernel", "lin_dx_kernel", "att_bwd_q_kernel", "att_bwd_kv_kernel",
                                        "dec_finish_kernel"}


def test_bad_arguments_are_reported():
    from m2amd import _lib
    lib = _lib.load()
    d = (64, 64, 2, 2)
    assert lib.m2_decoder_train_forward(None, *d, None, 1, 4, None, None, 0, None) == -1
    assert b"m2_decoder_train_forward" in lib.m2_last_error()
    assert lib.m2_decoder_backward(None, *d, None, 1, 4, None, None, None, None, 0, None, 0, None) == -1
    assert b"m2_decoder_backward" in lib.m2_last_error()
    assert lib.m2_decoder_backward(None, 60, 64, 2, 2, None, 1, 4, None, None, None, None, 0, None, 0, None) == -2
    assert lib.m2_decoder_train_forward(None, *d, None, 0, 4, None, None, 0, None) == 0  # nothing to do
    assert lib.m2_decoder_backward(None, *d, None, 3, 0, None, None, None, None, 0, None, 0, None) == 0
    assert lib.m2_debug_decoder_grad_plan(*d, 1, 4, None, 0) == -1
    assert lib.m2_attention_backward_workspace_bytes(2, 7, 4) == 2 * 4 * 7 * 3 * 4 + 256
    assert lib.m2_linear_backward_input_workspace_bytes(65, 64) == 2 * 2 * 64 * 4 + 256
    assert lib.m2_linear_backward_weight_workspace_bytes(100, 60, 64) == 0  # K is no multiple of 8
    assert lib.m2_linear_backward_weight_workspace_bytes(100, 64, 5) == 4 * (5 * 64 + 5) * 4 + 256


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


def test_switch_is_a_plain_attribute():
    from models.tts_model import M2TTSModel, MelDecoder
    dec = MelDecoder()
    keys = list(dec.state_dict())
    assert dec.backward_enabled is False and MelDecoder.backward_enabled is False
    assert dec.enable_backward() is dec and dec.backward_enabled is True
    assert list(dec.state_dict()) == keys and len(keys) == 26
    assert keys[:3] == ["layers.0.self_attn.qkv.weight", "layers.0.self_attn.out_proj.weight",
                        "layers.0.self_attn.out_proj.bias"]
    assert keys[3:11] == [f"layers.0.{n}" for n in ("ffn.linear1.weight", "ffn.linear1.bias", "ffn.linear2.weight",
                                                    "ffn.linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
                                                    "norm2.bias")]
    assert keys[22:] == ["norm.weight", "norm.bias", "mel_projection.weight", "mel_projection.bias"]
    assert len(MelDecoder(96, 80, 3, 2).state_dict()) == 37
    assert "backward_enabled" not in dict(dec.named_buffers()) and "backward_enabled" not in dict(dec.named_parameters())
    assert dec.enable_backward(False) is dec and dec.backward_enabled is False
    assert dec.enable_backward(enabled=True).backward_enabled is True
    assert MelDecoder.backward_enabled is False  # the switch follows the instance
    for bad in (dict(hidden_dim=160, num_heads=4), dict(hidden_dim=64, num_heads=8),
                dict(hidden_dim=40, num_heads=1), dict(num_layers=0)):
        with pytest.raises(NotImplementedError):
            MelDecoder(**bad).enable_backward()
        assert MelDecoder(**bad).enable_backward(False).backward_enabled is False
    model = M2TTSModel()
    assert model.decoder.backward_enabled is False and model.decoder.enable_backward() is model.decoder
    assert len(model.decoder.state_dict()) == 26
    # with the switch on, CPU tensors are refused: there is no CPU path
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        dec(torch.zeros(1, 4, 64))
