"""Host-side checks of the text encoder's backward and the length regulator's
adjoint (no GPU): the masked float64 oracle the GPU tests compare against
equals plain torch autograd when its masks come from itself; the formulas the
three new kernels implement (the embedding's sum by ids, the stand-alone
LayerNorm backward, the regulator's adjoint as a segment sum) reproduce float64
autograd to 1e-12 relative; the cases' inputs sit on the same side of every
ReLU kink in float32 and float64; the plan (tape, workspace, the embedding's
split, launch rows, the printed line) agrees with a restatement of its
formulas; the switches are plain attributes; the entry points are exported and
bound with the header's signatures."""
import ctypes
import re
import sys

import pytest
import torch

from conftest import GOLDEN
from test_ragged_host import header_signature

sys.path.insert(0, str(GOLDEN))
import encoder_backward_oracle as orc  # noqa: E402

ENTRIES = {"m2_encoder_tape_bytes": 6, "m2_encoder_tape_map": 9, "m2_encoder_train_forward": 14,
           "m2_encoder_backward_workspace_bytes": 6, "m2_encoder_backward": 16, "m2_debug_encoder_grad_plan": 8,
           "m2_embedding_backward_workspace_bytes": 3, "m2_embedding_backward": 11,
           "m2_layer_norm_backward_workspace_bytes": 2, "m2_layer_norm_backward": 12,
           "m2_length_regulator_backward": 8}
TOL = 1e-12
EPS = 1e-5


def _close(a, b):
    return float((a - b).abs().max()) <= TOL * max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("case", list(orc.CASES))
def test_masked_oracle_equals_plain_autograd_with_its_own_masks(case):
    V, H, layers, heads, B, S, _ = orc.CASES[case]
    enc = orc.cpu_copy(orc.make_encoder(case), torch.float64)
    params = orc.parameters(enc)
    assert len(params) == 1 + 11 * layers + 2 and all(a is b for a, b in zip(params, enc.parameters()))
    assert tuple(params[0].shape) == (V, H) and tuple(params[1].shape) == (3 * H, H)
    ids, lengths, d_out = orc.make_inputs(case)
    d_out = d_out.double()
    grads, out, pre = orc.gradients(enc, ids, lengths, d_out)
    plain, plain_out = orc.plain_gradients(enc, ids, lengths, d_out)
    assert out.shape == (B, S, H) and _close(out, plain_out)
    for g, p in zip(grads, plain):
        assert _close(g, p) and float(p.abs().max()) > 0
    positive = [u > 0 for u in pre]
    again, _, _ = orc.gradients(enc, ids, lengths, d_out, positive)
    assert all(torch.equal(a, b) for a, b in zip(again, grads))
    positive[-1] = ~positive[-1]
    flipped, _, _ = orc.gradients(enc, ids, lengths, d_out, positive)
    assert not torch.equal(flipped[0], grads[0])
    assert all(p.grad is None for p in params)
    # a vocabulary row that never occurs has no gradient at all
    unseen = torch.ones(V, dtype=torch.bool)
    unseen[ids.flatten()] = False
    assert float(grads[0][unseen].abs().sum()) == 0.0 and float(grads[0][~unseen].abs().min(dim=1).values.min()) >= 0
    if case == "odd":
        assert int(unseen.sum()) > V // 2
    if case == "tiles":
        assert int(unseen.sum()) == 0 and int(torch.bincount(ids.flatten(), minlength=V).min()) >= 2


@pytest.mark.parametrize("case", list(orc.CASES))
def test_inputs_take_one_side_of_every_kink_in_both_precisions(case):
    enc = orc.make_encoder(case)
    ids, lengths, _ = orc.make_inputs(case)
    with torch.no_grad():
        y32, pre32, _ = orc.forward(orc.cpu_copy(enc, torch.float32), ids, lengths)
        y64, pre64, _ = orc.forward(orc.cpu_copy(enc, torch.float64), ids, lengths)
    differ = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(pre32, pre64))
    total = sum(b.numel() for b in pre64)
    print(f"{case}: {differ} of {total} pre-activations differ in sign")
    V, H, layers, heads, B, S, _ = orc.CASES[case]
    assert total == layers * B * S * 2 * H and differ == 0
    assert float((y32.double() - y64).abs().max()) <= 1e-4 * float(y64.abs().max())
    assert int(ids.min()) >= 0 and int(ids.max()) < V
    # no parameter is at its degenerate initial value
    sd = enc.state_dict()
    assert float((sd["norm.weight"] - 1).abs().min()) > 0 and float(sd["norm.bias"].abs().min()) > 0
    assert float(sd["layers.0.ffn.linear2.bias"].abs().min()) > 0


# ---- the formulas of the kernels ---------------------------------------------------

@pytest.mark.parametrize("V,R,H,scale", [(5, 40, 8, 1.0), (300, 67, 16, 8.0), (1, 9, 4, 0.5), (40, 260, 8, 64 ** 0.5)])
def test_embedding_gradient_is_the_sum_by_ids(V, R, H, scale):
    """d_emb[v] = scale * sum of d_x over the positions with id v; ids outside [0, V) read a zero row in the
    forward and contribute nothing; a row that never occurs gets exactly 0."""
    g = torch.Generator().manual_seed(V + R)
    ids = torch.randint(-1, V + 1, (R,), generator=g)  # -1 and V are out of range
    ids[0], ids[-1] = -1, V
    d_x = torch.randn(R, H, generator=g, dtype=torch.float64)
    emb = torch.randn(V, H, generator=g, dtype=torch.float64, requires_grad=True)
    inside = (ids >= 0) & (ids < V)
    x0 = torch.where(inside[:, None], emb[ids.clamp(0, V - 1)], torch.zeros((), dtype=torch.float64)) * scale
    (want,) = torch.autograd.grad(x0, emb, d_x)
    got = torch.zeros(V, H, dtype=torch.float64)
    for v in range(V):
        rows = d_x[ids == v]  # ascending position
        if len(rows):
            got[v] = scale * rows.sum(0)
    assert _close(got, want)
    by_index_add = torch.zeros(V, H, dtype=torch.float64).index_add_(0, ids[inside], scale * d_x[inside])
    assert _close(by_index_add, want)
    never = torch.ones(V, dtype=torch.bool)
    never[ids[inside]] = False
    assert float(got[never].abs().sum()) == 0.0


@pytest.mark.parametrize("R,K,res", [(7, 64, True), (5, 96, False), (3, 32, True), (70, 128, False)])
def test_stand_alone_layer_norm_backward(R, K, res):
    """g_x = g_res + rstd (a - mean_k(a) - x^ mean_k(a x^)), a = g_y gamma; dgamma = sum_r g_y x^,
    dbeta = sum_r g_y: the linear's epilogue with the cotangent given instead of produced by a GEMM."""
    g = torch.Generator().manual_seed(R * K)
    x = torch.randn(R, K, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (torch.randn(K, generator=g, dtype=torch.float64) * 0.2 + 1).requires_grad_()
    beta = (torch.randn(K, generator=g, dtype=torch.float64) * 0.2).requires_grad_()
    g_y = torch.randn(R, K, generator=g, dtype=torch.float64)
    g_res = torch.randn(R, K, generator=g, dtype=torch.float64) if res else None
    y = torch.nn.functional.layer_norm(x, (K,), gamma, beta, EPS)
    outs, cots = ([y, x], [g_y, g_res]) if res else ([y], [g_y])
    want = torch.autograd.grad(outs, (x, gamma, beta), cots)
    with torch.no_grad():
        mean = x.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + EPS)
        xh = (x - mean) * rstd
        a = g_y * gamma
        g_x = rstd * (a - a.mean(1, keepdim=True) - xh * (a * xh).mean(1, keepdim=True))
        if res:
            g_x = g_res + g_x
        got = (g_x, (g_y * xh).sum(0), g_y.sum(0))
    assert all(_close(p, q) for p, q in zip(got, want))


@pytest.mark.parametrize("B,S,H,max_length", [(3, 7, 6, None), (2, 65, 8, 40), (2, 5, 4, 1000), (1, 1, 4, None)])
def test_regulator_adjoint_is_a_segment_sum(B, S, H, max_length):
    g = torch.Generator().manual_seed(B * S + H)
    durations = torch.rand(B, S, generator=g) * 4.9 - 0.5  # fractions, zeros (below 1) and negatives
    durations[-1] = 0.0  # an utterance without frames
    if B > 1:
        durations[0, 0] = 300.0 if max_length is None else 3.7
    cum = orc.frame_counts(durations)
    assert bool((cum[:, 1:] >= cum[:, :-1]).all()) and int(cum[-1, -1]) == 0
    assert torch.equal(orc.frame_counts(torch.trunc(durations).to(torch.int32)), cum)
    T = orc.output_length(cum, max_length)
    enc = torch.randn(B, S, H, generator=g, dtype=torch.float64, requires_grad=True)
    reg = orc.regulate(enc, cum, T)
    assert reg.shape == (B, T, H)
    # the index arithmetic is the repeat-and-pad of the reference
    for b in range(B):
        rows = [enc[b, s] for s in range(S) for _ in range(int(cum[b, s + 1] - cum[b, s]))][:T]
        want = torch.stack(rows + [torch.zeros(H, dtype=torch.float64)] * (T - len(rows)))
        assert torch.equal(reg[b].detach(), want.detach())
    d_reg = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(reg, enc, d_reg)
    got = orc.regulate_adjoint(d_reg, cum, S)
    assert _close(got, want) and float(got[-1].abs().sum()) == 0.0
    counts = orc.regulate_adjoint(torch.ones(B, T, H, dtype=torch.float64), cum, S)
    kept = (cum[:, 1:].clamp(max=T) - cum[:, :-1].clamp(max=T)).to(torch.float64)
    assert torch.equal(counts, kept[:, :, None].expand(B, S, H))


# ---- the plan ----------------------------------------------------------------------

def _cdiv(a, b):
    return -(-a // b)


def _up(n, a=256):
    return _cdiv(n, a) * a


def _widths(H, layers):
    return [H] + [3 * H, H, H, 2 * H, H] * layers


def _tape_layout(H, layers, B, S):
    off, at = 0, []
    for w in _widths(H, layers):
        off = _up(off)
        at.append(off // 4)
        off += 4 * B * S * w
    return at, off + 256


def _dw_split(R, N):
    tiles, chunks = _cdiv(N, 64), _cdiv(R, 32)
    want = max(1, min(chunks, _cdiv(256, tiles)))
    rps = _cdiv(chunks, want) * 32
    return tiles, _cdiv(R, rps)


def _emb_split(R, V):
    """Workgroups over R per vocabulary row: about 256 in all, whole 64-position chunks each."""
    chunks = _cdiv(R, 64)
    want = max(1, min(chunks, _cdiv(256, V)))
    rps = _cdiv(chunks, want) * 64
    return _cdiv(R, rps)


def _workspace(V, H, layers, heads, B, S):
    R = B * S
    part = max(_cdiv(R, 64) * 2 * H, _emb_split(R, V) * V * H)
    for K, N in ((2 * H, H), (H, 2 * H), (H, H), (H, 3 * H)):
        part = max(part, _dw_split(R, N)[1] * (N * K + N))
    off = 0
    for n in (R * H, R * H, R * 3 * H, B * heads * S * 3, part):
        off = _up(off) + 4 * n
    return off + 256, part


def _plan_line(lib, *dims):
    buf = ctypes.create_string_buffer(1 << 16)
    n = lib.m2_debug_encoder_grad_plan(*dims, buf, len(buf))
    assert 0 < n < len(buf)
    return buf.value.decode()


def _rows(line):
    return [(m.group(1), m.group(2), tuple(int(v) for v in m.group(3, 4, 5)), int(m.group(6)), int(m.group(7)))
            for m in re.finditer(r"(\w+):(\w+)\[grid=(\d+)x(\d+)x(\d+) thr=(\d+) lds=(\d+)\]", line)]


SWEEP = [(V, H, layers, heads, B, S) for (V, H, layers, heads) in ((256, 64, 2, 2), (256, 96, 3, 2), (5, 32, 1, 2),
                                                                   (300, 128, 1, 2), (40, 64, 1, 4), (1, 64, 1, 2))
         for B in (1, 3, 32) for S in (1, 17, 100, 130)]


def test_plan_agrees_with_a_restatement():
    from m2amd import _lib
    lib = _lib.load()
    off, width = ctypes.c_size_t(), ctypes.c_int32()
    for dims in SWEEP + [c[:6] for c in orc.CASES.values()]:
        V, H, layers, heads, B, S = dims
        R = B * S
        at, tape_bytes = _tape_layout(H, layers, B, S)
        assert lib.m2_encoder_tape_bytes(*dims) == tape_bytes
        for i, w in enumerate(_widths(H, layers)):
            assert lib.m2_encoder_tape_map(*dims, i, ctypes.byref(off), ctypes.byref(width)) == 0
            assert (off.value, width.value) == (at[i], w) and off.value % 64 == 0, (dims, i)
        assert lib.m2_encoder_tape_map(*dims, 1 + 5 * layers, ctypes.byref(off), ctypes.byref(width)) == -1
        ws_bytes, part = _workspace(*dims)
        assert lib.m2_encoder_backward_workspace_bytes(*dims) == ws_bytes, dims
        assert lib.m2_embedding_backward_workspace_bytes(R, V, H) == 4 * _emb_split(R, V) * V * H + 256
        assert lib.m2_layer_norm_backward_workspace_bytes(R, H) == 4 * _cdiv(R, 64) * 2 * H + 256
        line = _plan_line(lib, *dims)
        assert line.startswith(f"V={V} H={H} layers={layers} heads={heads} B={B} S={S} tape={tape_bytes} "
                               f"ws={ws_bytes} part={part} nx:")
        rows = _rows(line)
        assert len(line.split(" ")) == 9 + 3 * len(rows)  # every item after the header is a row
        assert all(lds <= 48 * 1024 and thr == 256 for *_, thr, lds in rows)
        assert all(0 < g[0] and 0 < g[1] <= 65535 and 0 < g[2] <= 65535 for _, _, g, _, _ in rows)
        by_step = {}
        for step, kernel, grid, thr, lds in rows:
            by_step.setdefault(step, []).append((kernel, grid, lds))
        assert list(by_step) == ["nx"] + [f"{s}{l}" for l in reversed(range(layers))
                                          for s in ("l2w", "l2x", "l1w", "l1x", "ow", "ox", "att", "qw", "qx")] + ["ew"]
        kg = lambda step: [(k, g) for k, g, _ in by_step[step]]  # noqa: E731
        fin = lambda n: ("dec_finish_kernel", (_cdiv(n, 32), 1, 1))  # noqa: E731
        dw = lambda K, N, bias: ([("lin_dw_kernel", _dw_split(R, N) + (1,)), fin(N * K)]  # noqa: E731
                                 + ([fin(N)] if bias else []))
        dx = lambda ln: [("lin_dx_kernel", (_cdiv(R, 64), 1, 1))] + ([fin(H), fin(H)] if ln else [])  # noqa: E731
        att = [(k, (_cdiv(S, 64), heads, B)) for k in ("att_bwd_q_kernel", "att_bwd_kv_kernel")]
        assert kg("nx") == [("ln_bwd_kernel", (_cdiv(R, 64), 1, 1)), fin(H), fin(H)]
        assert by_step["nx"][0][2] == 4 * (64 * (H + 1) + 128 + 8 * H)
        assert kg("ew") == [("emb_dw_kernel", (V, _emb_split(R, V), 1)), fin(V * H)] and by_step["ew"][0][2] == 0
        for l in range(layers):
            assert kg(f"l2w{l}") == dw(2 * H, H, True) and kg(f"l2x{l}") == dx(False)
            assert kg(f"l1w{l}") == dw(H, 2 * H, True) and kg(f"l1x{l}") == dx(True)
            assert kg(f"ow{l}") == dw(H, H, True) and kg(f"ox{l}") == dx(False)
            assert kg(f"att{l}") == att
            assert kg(f"qw{l}") == dw(H, 3 * H, False) and kg(f"qx{l}") == dx(True)
    # one range per vocabulary row at V >= 256, several for a small phoneme set, about 256 workgroups in all
    assert _emb_split(3200, 256) == 1 and _emb_split(3200, 300) == 1 and _emb_split(3200, 40) == 7
    assert _emb_split(4480, 1) == 70 and _emb_split(4480, 5) == 35 and _emb_split(1, 1) == 1
    bad = [(0, 64, 2, 2), (65537, 64, 2, 2), (256, 60, 2, 2), (256, 160, 2, 2), (256, 64, 2, 8), (256, 64, 0, 2),
           (256, 64, 2, 3)]
    for d in bad:
        assert lib.m2_encoder_tape_bytes(*d, 1, 4) == 0 and lib.m2_encoder_backward_workspace_bytes(*d, 1, 4) == 0, d
    assert lib.m2_encoder_tape_bytes(65536, 128, 1, 2, 1, 4) > 0
    assert lib.m2_encoder_tape_bytes(256, 64, 2, 2, 0, 4) == 256 == lib.m2_encoder_backward_workspace_bytes(256, 64, 2, 2, 2, 0)


def test_the_decoder_plan_is_unchanged_by_the_shared_walk():
    """The layer walk is stated once for both stacks: between `mx` and the end the decoder's line has the
    steps the encoder's has between `nx` and `ew`, row for row, at equal (H, layers, heads, B, rows)."""
    from m2amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    for H, layers, heads, B, N in ((64, 2, 2, 32, 100), (96, 3, 2, 8, 100), (32, 1, 2, 3, 1), (128, 1, 2, 1, 65)):
        assert lib.m2_debug_decoder_grad_plan(H, 80, layers, heads, B, N, buf, len(buf)) > 0
        dec = [r for r in _rows(buf.value.decode()) if r[0] not in ("mw", "mx")]
        enc = [r for r in _rows(_plan_line(lib, 256, H, layers, heads, B, N)) if r[0] not in ("nx", "ew")]
        assert dec == enc and len(dec) == layers * (4 * 3 - 1 + 2 * 3 + 2 + 2)


def test_bad_arguments_are_reported():
    from m2amd import _lib
    lib = _lib.load()
    d = (256, 64, 2, 2)
    assert lib.m2_encoder_train_forward(None, *d, None, None, None, 1, 4, None, None, 0, None) == -1
    assert b"m2_encoder_train_forward" in lib.m2_last_error()
    assert lib.m2_encoder_backward(None, *d, None, None, 1, 4, None, None, None, 0, None, 0, None) == -1
    assert b"m2_encoder_backward" in lib.m2_last_error()
    assert lib.m2_encoder_backward(None, 256, 60, 2, 2, None, None, 1, 4, None, None, None, 0, None, 0, None) == -2
    assert lib.m2_encoder_train_forward(None, 0, 64, 2, 2, None, None, None, 1, 4, None, None, 0, None) == -2
    assert lib.m2_encoder_train_forward(None, *d, None, None, None, 0, 4, None, None, 0, None) == 0  # nothing to do
    assert lib.m2_encoder_backward(None, *d, None, None, 3, 0, None, None, None, 0, None, 0, None) == 0
    assert lib.m2_debug_encoder_grad_plan(*d, 1, 4, None, 0) == -1
    assert lib.m2_embedding_backward(None, None, 4, 256, 64, 1.0, None, 0, None, 0, None) == -1
    assert b"m2_embedding_backward" in lib.m2_last_error()
    assert lib.m2_embedding_backward_workspace_bytes(4, 0, 64) == 0 == lib.m2_embedding_backward_workspace_bytes(4, 70000, 64)
    assert lib.m2_layer_norm_backward(None, None, None, None, 4, 64, None, None, None, None, 0, None) == -1
    assert b"m2_layer_norm_backward" in lib.m2_last_error()
    assert lib.m2_layer_norm_backward_workspace_bytes(4, 60) == 0 == lib.m2_layer_norm_backward_workspace_bytes(4, 136)
    assert lib.m2_length_regulator_backward(None, None, 2, 3, 64, 5, None, None) == -1
    assert b"m2_length_regulator_backward" in lib.m2_last_error()
    assert lib.m2_length_regulator_backward(None, None, 0, 3, 64, 5, None, None) == 0
    assert lib.m2_length_regulator_backward(None, None, 2, 0, 64, 5, None, None) == 0
    assert lib.m2_length_regulator_backward(None, None, 2, 3, 0, 5, None, None) == -1


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


def test_switches_are_plain_attributes():
    from models.tts_model import LengthRegulator, M2TTSModel, TextEncoder
    enc = TextEncoder()
    keys = list(enc.state_dict())
    assert enc.backward_enabled is False and TextEncoder.backward_enabled is False
    assert enc.enable_backward() is enc and enc.backward_enabled is True
    assert list(enc.state_dict()) == keys and len(keys) == 1 + 1 + 22 + 2  # the positional table is a buffer
    assert keys[0] == "embedding.weight" and keys[1] == "pos_encoding.pe" and keys[-2:] == ["norm.weight", "norm.bias"]
    names = [n for n, _ in enc.named_parameters()]
    assert len(names) == 25 and names[0] == "embedding.weight" and names[1] == "layers.0.self_attn.qkv.weight"
    assert names[2:12] == [f"layers.0.{n}" for n in ("self_attn.out_proj.weight", "self_attn.out_proj.bias",
                                                     "ffn.linear1.weight", "ffn.linear1.bias", "ffn.linear2.weight",
                                                     "ffn.linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
                                                     "norm2.bias")]
    assert names[-2:] == ["norm.weight", "norm.bias"]
    assert "backward_enabled" not in dict(enc.named_buffers()) and "backward_enabled" not in dict(enc.named_parameters())
    assert enc.enable_backward(False) is enc and enc.backward_enabled is False
    assert enc.enable_backward(enabled=True).backward_enabled is True
    assert TextEncoder.backward_enabled is False  # the switch follows the instance
    reg = LengthRegulator()
    assert reg.backward_enabled is False and LengthRegulator.backward_enabled is False
    assert reg.enable_backward() is reg and reg.backward_enabled is True and list(reg.state_dict()) == []
    assert reg.enable_backward(False).backward_enabled is False and LengthRegulator.backward_enabled is False
    model = M2TTSModel()
    keys = list(model.state_dict())
    assert model.text_encoder.backward_enabled is False and model.length_regulator.backward_enabled is False
    assert model.text_encoder.enable_backward() is model.text_encoder
    assert model.length_regulator.enable_backward() is model.length_regulator
    assert list(model.state_dict()) == keys
    # with the switch on, CPU tensors are refused: there is no CPU path
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        enc(torch.zeros(1, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        reg.enable_backward()(torch.zeros(1, 4, 64, requires_grad=True), torch.ones(1, 4))


def test_enable_backward_raises_on_an_unsupported_shape():
    from models.tts_model import TextEncoder
    for bad in (dict(hidden_dim=160, num_heads=4), dict(hidden_dim=64, num_heads=8), dict(hidden_dim=40, num_heads=1),
                dict(num_layers=0), dict(vocab_size=70000)):
        with pytest.raises(NotImplementedError, match="head_dim 16, 32, 48 or 64"):
            TextEncoder(**bad).enable_backward()
        enc = TextEncoder(**bad)
        assert enc.enable_backward(False).backward_enabled is False
    assert TextEncoder(vocab_size=5, hidden_dim=32, num_layers=1, num_heads=2).enable_backward().backward_enabled
