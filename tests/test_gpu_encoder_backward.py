"""GPU: the text encoder's training forward and backward (m2_encoder_train_forward,
m2_encoder_backward, TextEncoder.enable_backward), the length regulator's adjoint
(m2_length_regulator_backward, LengthRegulator.enable_backward) and the kernels
alone, against torch autograd on the CPU in float64.  Nothing here reads the
reference: the oracle is the module's own nn layers, deep-copied to the CPU
(tests/golden/encoder_backward_oracle.py).

The bar is test_gpu_decoder_backward.py's; no number comes from the GPU's
output.  Per tensor g:
    |g_gpu - g_f64| <= 32 x max(s, 2^-24) x max|g_f64|,
s the largest relative deviation, over the tensors of the case, of CPU float32
autograd from float64 autograd, computed here and printed.

ReLU kinks are accounted as there.  The float64 oracle applies each ReLU as a
product with a constant 0/1 mask taken from the GPU's stored map (h > 0), read
from the tape; wherever that predicate differs from the float64
pre-activation's sign, |pre_f64| must be within the forward bar of the map,
32 x max(s_fwd, 2^-24) x max|map|, and at most 4 elements per case may differ:
a cap, not a measurement.  The count is printed.

The optimizer step compares float32 parameters after the update with the same
update done in float64: the gradient bar times the learning rate, plus the
rounding of the stored float32 parameter itself, 2^-24 x max|p|.
"""
import copy
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

sys.path.insert(0, str(GOLDEN))
import decoder_backward_oracle as dorc  # noqa: E402
import encoder_backward_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
KINK_CAP = 4
LR = 0.05
VOCABS = (1, 5, 40, 256, 300)
EMB_ROWS = (1, 63, 64, 65, 260, 4480)
WIDTHS = (32, 64, 96, 128)
ROWS = (1, 63, 64, 65, 260)
REG_WIDTHS = (6, 64, 96, 128)
REG_PHONEMES = (1, 63, 64, 65, 130)


def _rel(a, b):
    return float((a.double() - b).abs().max()) / float(b.abs().max())


def _check(what, got, want, single):
    s = max([_rel(a, b) for a, b in zip(single, want) if float(b.abs().max()) > 0], default=0.0)
    bar = 32.0 * max(s, EPS)
    for i, (g, ref) in enumerate(zip(got, want)):
        assert g.shape == ref.shape and g.dtype == torch.float32, (what, i)
        top = float(ref.abs().max())
        err = float((g.cpu().double() - ref).abs().max())
        assert err <= bar * top, (what, i, err, bar * top)
    return bar


def _kinks(what, pre, pre32, pre64, positive):
    """The GPU's side of every kink against the float64 pre-activations: a differing predicate lies within
    the forward bar of its map; returns how many differ."""
    kinks = 0
    for l in range(len(pre)):
        top = float(pre64[l].abs().max())
        s_fwd = float((pre32[l].double() - pre64[l]).abs().max()) / top
        differ = (pre[l] > 0) != positive[l]
        assert bool((pre[l].abs()[differ] <= 32.0 * max(s_fwd, EPS) * top).all()), \
            (what, l, "a resolvable pre-activation changed sign")
        kinks += int(differ.sum())
    return kinks


_EXPECT = {}


def _expect(case, gpu):
    """The case's module on the GPU, its inputs, the ops-level result, and the float64 gradients with the
    GPU's side of every kink; computed once per case and never changed."""
    if case in _EXPECT:
        return _EXPECT[case]
    from m2amd import ops
    V, H, layers, heads, B, S, _ = orc.CASES[case]
    enc = orc.make_encoder(case)
    ids, lengths, dy = orc.make_inputs(case)
    e64, e32 = orc.cpu_copy(enc, torch.float64), orc.cpu_copy(enc, torch.float32)
    g64, _, pre64 = orc.gradients(e64, ids, lengths, dy.double())
    g32, _, pre32 = orc.gradients(e32, ids, lengths, dy)
    s = max(_rel(a, b) for a, b in zip(g32, g64))
    genc = copy.deepcopy(enc).to(gpu)
    params = [p.detach() for p in genc.parameters()]
    pe = genc.pos_encoding.pe[0]
    mask = orc.key_mask(lengths, S)
    mask = None if mask is None else mask.to(gpu)
    out, tape = ops.encoder_train_forward(params, ids.to(gpu), pe, mask, heads)
    x0, maps = ops.encoder_tape_maps(tape, V, H, layers, heads, B, S)
    positive = [m["h"].cpu() > 0 for m in maps]
    grads, _, pre = orc.gradients(e64, ids, lengths, dy.double(), positive)
    kinks = _kinks(case, pre, pre32, pre64, positive)
    print(f"{case}: {kinks} of {sum(p.numel() for p in pre)} pre-activations take the other ReLU side on the GPU; "
          f"s = {s:.3e}")
    assert kinks <= KINK_CAP, case
    got = ops.encoder_backward(params, ids.to(gpu), mask, tape, dy.to(gpu), heads)
    _EXPECT[case] = {"enc": genc, "params": params, "ids": ids.to(gpu), "lengths": None if lengths is None else
                     lengths.to(gpu), "mask": mask, "pe": pe, "dy": dy.to(gpu), "out": out, "tape": tape, "x0": x0,
                     "maps": maps, "grads": grads, "s": s, "got": got}
    return _EXPECT[case]


# ---- forward -----------------------------------------------------------------------

@pytest.mark.parametrize("case", list(orc.CASES))
def test_train_forward_is_the_module_forward_bit_for_bit(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    V, H, layers, heads, B, S, _ = orc.CASES[case]
    with torch.no_grad():
        want, mask = e["enc"](e["ids"], e["lengths"])
    assert e["enc"].backward_enabled is False and want.grad_fn is None
    assert e["out"].shape == (B, S, H) and torch.equal(e["out"], want)
    assert (mask is None) == (e["mask"] is None) and (mask is None or torch.equal(mask, e["mask"]))
    on = copy.deepcopy(e["enc"]).enable_backward()
    got, got_mask = on(e["ids"], e["lengths"])  # the parameters require grad
    assert got.grad_fn is not None and torch.equal(got.detach(), want)
    assert (got_mask is None) == (mask is None) and (mask is None or (torch.equal(got_mask, mask)
                                                                     and got_mask.dtype == mask.dtype))
    maps, p = e["maps"], e["params"][1:12]
    assert len(maps) == layers and list(maps[0]) == ["qkv", "att", "x_mid", "h", "x_out"]
    x0 = ops.embed_positional(e["ids"], e["params"][0], e["pe"][:S], ops.sqrt_hidden(H))
    assert torch.equal(e["x0"], x0)
    qkv = ops.linear(x0, p[0], ln=(p[7], p[8]))
    assert torch.equal(maps[0]["qkv"], qkv)
    att = ops.attention_core(qkv, heads, e["mask"])
    assert torch.equal(maps[0]["att"], att)
    x_mid = ops.linear(att, p[1], p[2], residual=x0)
    assert torch.equal(maps[0]["x_mid"], x_mid)
    h = ops.linear(x_mid, p[3], p[4], ln=(p[9], p[10]), act=ops.ACT_RELU)
    assert torch.equal(maps[0]["h"], h) and float(h.min()) == 0.0
    assert torch.equal(maps[0]["x_out"], ops.linear(h, p[5], p[6], residual=x_mid))
    assert torch.equal(e["out"], ops.layer_norm(maps[-1]["x_out"], e["params"][-2], e["params"][-1]))


def test_forward_inside_a_model_is_the_stand_alone_module(gpu):
    from models.tts_model import M2TTSModel
    torch.manual_seed(11)
    model = M2TTSModel().to(gpu).eval()
    ids = torch.randint(0, 256, (2, 9), device=gpu)
    lengths = torch.tensor([9, 5], device=gpu)
    alone = copy.deepcopy(model.text_encoder)
    with torch.no_grad():
        want, want_mask = alone(ids, lengths)  # the copy is no one's encoder: the per-op path
        fused, fused_mask = model.text_encoder(ids, lengths)
    assert model.text_encoder.enable_backward() is model.text_encoder
    try:
        got, mask = model.text_encoder(ids, lengths)
        assert got.grad_fn is not None and torch.equal(got.detach(), want)
        assert mask.dtype == fused_mask.dtype and torch.equal(mask, fused_mask) and torch.equal(mask, want_mask)
        got_none, no_mask = model.text_encoder(ids)
        assert got_none.grad_fn is not None and no_mask is None and torch.equal(got_none.detach(), alone(ids)[0].detach())
        with torch.no_grad():
            quiet, _ = model.text_encoder(ids, lengths)
        assert quiet.grad_fn is None and torch.equal(quiet, fused)  # today's path: the handle's fused layers
        out = model(ids[:1, :7])  # M2TTSModel.forward carries no graph
        assert out["mel_output"].grad_fn is None and out["encoder_output"].grad_fn is None
    finally:
        model.text_encoder.enable_backward(False)
    assert model.text_encoder(ids, lengths)[0].grad_fn is None


# ---- the chain ---------------------------------------------------------------------

@pytest.mark.parametrize("case", list(orc.CASES))
def test_chain_matches_float64_autograd(gpu, case):
    e = _expect(case, gpu)
    layers = orc.CASES[case][2]
    bar = 32.0 * max(e["s"], EPS)
    names = [n for n, _ in e["enc"].named_parameters()]
    assert len(e["got"]) == len(names) == 1 + 11 * layers + 2
    worst = 0.0
    for name, g, ref in zip(names, e["got"], e["grads"]):
        assert g.shape == ref.shape and g.dtype == torch.float32 and g.is_cuda, (case, name)
        err = _rel(g.cpu(), ref)
        worst = max(worst, err)
        assert err <= bar, (case, name, err, bar)
    # a vocabulary row that never occurs gets exactly 0
    unseen = torch.ones(orc.CASES[case][0], dtype=torch.bool)
    unseen[e["ids"].cpu().flatten()] = False
    assert float(e["got"][0].cpu()[unseen].abs().sum()) == 0.0
    print(f"{case}: worst rel max err {worst:.3e}, cpu float32 {e['s']:.3e}, bar {bar:.3e}")


# ---- the kernels alone -------------------------------------------------------------

@pytest.mark.parametrize("V", VOCABS)
def test_embedding_gradient_alone(gpu, V):
    from m2amd import ops
    g = torch.Generator().manual_seed(700 + V)
    for R in EMB_ROWS:
        ids = torch.randint(0, V, (R,), generator=g)
        if R >= 63:
            ids[5], ids[R - 1], ids[R // 2] = -1, V, V + 7  # out of range: a zero row in the forward
        inside = (ids >= 0) & (ids < V)
        count = torch.bincount(ids[inside], minlength=V).to(torch.float32)
        for H in WIDTHS:
            what = f"embedding V {V} R {R} H {H}"
            ones = ops.embedding_backward(ids.to(gpu), torch.ones(R, H, device=gpu), V)
            assert ones.shape == (V, H) and torch.equal(ones.cpu(), count[:, None].expand(V, H)), what
            d_x = torch.randn(R, H, generator=g)
            scale = H ** 0.5

            def by_index_add(dtype):
                return [torch.zeros(V, H, dtype=dtype).index_add_(0, ids[inside], d_x[inside].to(dtype) * scale)]

            got = ops.embedding_backward(ids.to(gpu), d_x.to(gpu), V, scale)
            _check(what, [got], by_index_add(torch.float64), by_index_add(torch.float32))
            assert float(got.cpu()[count == 0].abs().sum()) == 0.0, what  # rows that never occur: exactly 0
            assert torch.equal(got, ops.embedding_backward(ids.to(gpu), d_x.to(gpu), V, scale)), what
            onto = got.clone()
            assert ops.embedding_backward(ids.to(gpu), d_x.to(gpu), V, scale, accumulate=onto) is onto
            assert torch.equal(onto, 2.0 * got), what
            # a [B, S] batch is its flattened positions
            if R == 260:
                assert torch.equal(ops.embedding_backward(ids.view(2, 130).to(gpu), d_x.view(2, 130, H).to(gpu), V, scale),
                                   got)


@pytest.mark.parametrize("K", WIDTHS)
def test_layer_norm_backward_alone(gpu, K):
    from m2amd import ops
    g = torch.Generator().manual_seed(750 + K)
    for R in ROWS:
        x = torch.randn(R, K, generator=g) * 1.5 + 0.3
        g_y = torch.randn(R, K, generator=g)
        gamma, beta = torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.2
        g_res = torch.randn(R, K, generator=g)
        for res in (False, True):
            def autograd(dtype):
                leaf, ga, be = (t.to(dtype).requires_grad_() for t in (x, gamma, beta))
                y = F.layer_norm(leaf, (K,), ga, be, 1e-5)
                outs, cots = ([y, leaf], [g_y.to(dtype), g_res.to(dtype)]) if res else ([y], [g_y.to(dtype)])
                return torch.autograd.grad(outs, (leaf, ga, be), cots)

            args = (g_y.to(gpu), x.to(gpu), gamma.to(gpu), g_res.to(gpu) if res else None)
            got = ops.layer_norm_backward(*args)
            _check(f"layer norm K {K} R {R} res {res}", got, autograd(torch.float64), autograd(torch.float32))
            assert all(torch.equal(a, b) for a, b in zip(got, ops.layer_norm_backward(*args)))
            # the linear's epilogue on the same cotangent: g_y = g_n I
            eye = torch.eye(K, device=gpu)
            same = ops.linear_backward_input(args[0], eye, ln_x=args[1], gamma=args[2], g_res=args[3])
            assert all(torch.equal(a, b) for a, b in zip(got, same))


def _durations(B, S, g, kind):
    """float: fractions in [0, 4.9) with zeros and negatives; int: 0..4 with negatives; unit: 0 or 1.  One
    phoneme of utterance 0 has 300 frames (float, int); the last utterance has no frames at all."""
    if kind == "unit":
        d = (torch.rand(B, S, generator=g) > 0.4).to(torch.float32)
    else:
        d = torch.rand(B, S, generator=g) * 4.9
        d[torch.rand(B, S, generator=g) < 0.15] = 0.0
        d[torch.rand(B, S, generator=g) < 0.1] = -1.5
        d[0, S // 2] = 300.0
        if kind == "int":
            d = torch.trunc(d).to(torch.int64)
    d[B - 1] = 0
    return d


@pytest.mark.parametrize("H", REG_WIDTHS)
def test_regulator_adjoint_alone(gpu, H):
    from m2amd import ops
    g = torch.Generator().manual_seed(780 + H)
    B = 3
    for S in REG_PHONEMES:
        for kind in ("float", "int", "unit"):
            d = _durations(B, S, g, kind)
            cum64 = orc.frame_counts(d)
            cum, _, _ = ops.frame_counts(d.to(gpu))
            assert torch.equal(cum.cpu().to(torch.int64), cum64)
            total = int(cum64[:, -1].max())
            inside = max(1, int(cum64[0, S // 2]) + 150) if kind != "unit" else max(1, total - 1)
            for max_length in (None, inside, total + 9):  # the batch's own, a cut inside a phoneme, past the total
                T = orc.output_length(cum64, max_length)
                what = f"regulator H {H} S {S} {kind} T {T}"
                kept = (cum64[:, 1:].clamp(max=T) - cum64[:, :-1].clamp(max=T)).to(torch.float32)
                ones = ops.regulate_backward(torch.ones(B, T, H, device=gpu), cum, S)
                assert ones.shape == (B, S, H) and torch.equal(ones.cpu(), kept[:, :, None].expand(B, S, H)), what
                d_reg = torch.randn(B, T, H, generator=g)
                got = ops.regulate_backward(d_reg.to(gpu), cum, S)
                want = [orc.regulate_adjoint(d_reg.double(), cum64, S)]
                _check(what, [got], want, [orc.regulate_adjoint(d_reg, cum64, S)])
                assert float(got[B - 1].abs().max()) == 0.0, what  # the utterance without frames: exactly 0
                assert bool((got.cpu()[kept == 0] == 0).all()), what  # so is every phoneme without frames
                assert torch.equal(got, ops.regulate_backward(d_reg.to(gpu), cum, S)), what
                if kind == "unit":  # every phoneme has at most one frame: the adjoint is a gather
                    first = cum64[:, :-1].clamp(max=T - 1)
                    gather = torch.gather(d_reg, 1, first[:, :, None].expand(B, S, H)) * (kept[:, :, None] > 0)
                    assert torch.equal(got.cpu(), gather), what
                for b in range(B):  # an utterance inside a batch is the same utterance alone
                    alone = ops.regulate_backward(d_reg[b:b + 1].to(gpu), cum[b:b + 1].contiguous(), S)
                    assert torch.equal(alone[0], got[b]), (what, b)
                # the adjoint property against the forward's own launches: <expand(e), r> = <e, adjoint(r)>
                if max_length == inside and kind == "float":
                    enc = torch.randn(B, S, H, generator=g).to(gpu)
                    lhs = float((ops.expand_frames(enc, cum, T).double() * d_reg.to(gpu).double()).sum())
                    rhs = float((enc.double() * got.double()).sum())
                    assert abs(lhs - rhs) <= 1e-5 * float((enc.double() * got.double()).abs().sum()), what


def test_regulator_module(gpu):
    from m2amd import ops
    from models.tts_model import LengthRegulator
    g = torch.Generator().manual_seed(790)
    B, S, H = 3, 9, 64
    d = _durations(B, S, g, "float").to(gpu)
    enc = torch.randn(B, S, H, generator=g).to(gpu)
    reg = LengthRegulator()
    leaf = enc.clone().requires_grad_()
    want = reg(enc, d)
    assert reg(leaf, d).grad_fn is None  # the switch is off
    assert reg.enable_backward() is reg
    assert reg(enc, d).grad_fn is None  # nothing requires grad
    with torch.no_grad():
        assert reg(leaf, d).grad_fn is None
    for max_length in (None, 40, 1000):
        leaf.grad = None
        durations = d.clone().requires_grad_()
        out = reg(leaf, durations, max_length)
        assert out.grad_fn is not None and torch.equal(out.detach(), ops.regulate(enc, d, max_length))
        if max_length is None:
            assert torch.equal(out.detach(), want)
        d_reg = torch.randn(out.shape, generator=g).to(gpu)
        out.backward(d_reg)
        cum, _, _ = ops.frame_counts(d)
        assert torch.equal(leaf.grad, ops.regulate_backward(d_reg, cum, S)) and durations.grad is None
    with pytest.raises(RuntimeError):  # once differentiable
        (ge,) = torch.autograd.grad(reg(leaf, d), leaf, torch.ones_like(want), create_graph=True)
        ge.sum().backward()
    assert reg.enable_backward(False) is reg and reg(leaf, d).grad_fn is None


# ---- determinism, accumulation, need -----------------------------------------------

@pytest.mark.parametrize("case", ["tiles", "thin", "heads4"])
def test_determinism_accumulation_and_need(gpu, case):
    from m2amd import ops
    e = _expect(case, gpu)
    layers, heads = orc.CASES[case][2:4]
    n = 1 + 11 * layers + 2
    args = (e["params"], e["ids"], e["mask"], e["tape"], e["dy"], heads)
    grads = ops.encoder_backward(*args)
    assert len(grads) == n and all(torch.equal(a, b) for a, b in zip(grads, e["got"]))
    onto = [g.clone() for g in grads]
    twice = ops.encoder_backward(*args, accumulate=onto)
    assert all(t is o for t, o in zip(twice, onto)) and all(torch.equal(t, 2.0 * g) for t, g in zip(twice, grads))
    need = [i % 3 != 1 for i in range(n)]
    some = ops.encoder_backward(*args, need=need)
    for i, (g, full) in enumerate(zip(some, e["got"])):
        assert (g is None) == (not need[i]) and (g is None or torch.equal(g, full)), i
    no_emb = ops.encoder_backward(*args, need=[False] + [True] * (n - 1))  # layer 0's input cotangent is skipped
    assert no_emb[0] is None and all(torch.equal(a, b) for a, b in zip(no_emb[1:], e["got"][1:]))
    only_emb = ops.encoder_backward(*args, need=[True] + [False] * (n - 1))
    assert torch.equal(only_emb[0], e["got"][0]) and all(g is None for g in only_emb[1:])


def test_abi_conventions(gpu):
    import ctypes
    from m2amd import _lib
    lib = _lib.load()
    case = "odd"
    e = _expect(case, gpu)
    V, H, layers, heads, B, S, _ = orc.CASES[case]
    d4 = (V, H, layers, heads)
    n = 1 + 11 * layers + 2
    pp = (ctypes.c_void_p * n)(*[p.data_ptr() for p in e["params"]])
    outs = [torch.full_like(p, -1.0) for p in e["params"]]
    gp = (ctypes.c_void_p * n)(*[g.data_ptr() for g in outs])
    out = torch.full((B, S, H), -2.0, device=gpu)
    tape_bytes = lib.m2_encoder_tape_bytes(*d4, B, S)
    ws_bytes = lib.m2_encoder_backward_workspace_bytes(*d4, B, S)
    tape = torch.empty(tape_bytes, dtype=torch.uint8, device=gpu)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
    ids, pe, mask, dy = e["ids"].data_ptr(), e["pe"].data_ptr(), e["mask"].data_ptr(), e["dy"].data_ptr()
    fwd = lambda b, s, nbytes: lib.m2_encoder_train_forward(pp, *d4, ids, pe, mask, b, s, out.data_ptr(),  # noqa: E731
                                                            tape.data_ptr(), nbytes, None)
    bwd = lambda b, s, nbytes: lib.m2_encoder_backward(pp, *d4, ids, mask, b, s, e["tape"].data_ptr(), dy, gp, 0,  # noqa: E731
                                                       ws.data_ptr(), nbytes, None)
    assert fwd(B, S, tape_bytes - 512) == -1 and b"tape too small" in lib.m2_last_error()
    assert bwd(B, S, ws_bytes - 512) == -1 and b"workspace too small" in lib.m2_last_error()
    assert fwd(0, S, 0) == 0 and fwd(B, 0, 0) == 0 and bwd(0, S, 0) == 0 and bwd(B, 0, 0) == 0
    pp[5] = None
    assert fwd(B, S, tape_bytes) == -1 and bwd(B, S, ws_bytes) == -1
    pp[5] = e["params"][5].data_ptr()
    torch.cuda.synchronize()
    assert bool((out == -2.0).all()) and all(bool((g == -1.0).all()) for g in outs)  # nothing was launched
    assert fwd(B, S, tape_bytes) == 0 and bwd(B, S, ws_bytes) == 0  # the queried sizes are accepted
    torch.cuda.synchronize()
    assert torch.equal(out, e["out"]) and all(torch.equal(g, w) for g, w in zip(outs, e["got"]))


# ---- the module --------------------------------------------------------------------

def _zero(params):
    for p in params:
        p.grad = None


def test_module_backward(gpu):
    e = _expect("s1", gpu)
    enc = copy.deepcopy(e["enc"])
    params = list(enc.parameters())
    ids, lengths, dy = e["ids"], e["lengths"], e["dy"]
    assert all(p.requires_grad for p in params) and torch.is_grad_enabled()
    assert enc(ids, lengths)[0].grad_fn is None  # the switch is off
    assert enc.enable_backward() is enc
    with torch.no_grad():
        assert enc(ids, lengths)[0].grad_fn is None
    out, mask = enc(ids, lengths)
    assert out.grad_fn is not None and torch.equal(out.detach(), e["out"]) and torch.equal(mask, e["mask"])
    out.backward(dy)
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    enc(ids, lengths)[0].backward(dy)  # a second backward accumulates
    assert all(torch.equal(p.grad, 2.0 * g) for p, g in zip(params, e["got"]))
    _zero(params)
    strided = torch.stack([dy, -dy], dim=-1)[..., 0]  # any [B,S,H] tensor: made contiguous
    assert not strided.is_contiguous()
    enc(ids, lengths)[0].backward(strided)
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    with pytest.raises(RuntimeError):  # once differentiable
        (gw,) = torch.autograd.grad(enc(ids, lengths)[0], params[:1], dy, create_graph=True)
        gw.sum().backward()
    # frozen parameters get None
    frozen = [params[0], params[8], params[13], params[24]]
    for p in frozen:
        p.requires_grad_(False)
    _zero(params)
    enc(ids, lengths)[0].backward(dy)
    assert all(p.grad is None for p in frozen)
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]) if not any(p is f for f in frozen))
    for p in params:
        p.requires_grad_(False)
    assert enc(ids, lengths)[0].grad_fn is None  # nothing requires grad: today's path
    for p in params:
        p.requires_grad_(True)
    assert enc.enable_backward(False) is enc and enc(ids, lengths)[0].grad_fn is None


def test_unsupported_shapes_raise(gpu):
    from m2amd import ops
    from models.tts_model import TextEncoder
    for bad in (dict(hidden_dim=160, num_heads=4), dict(hidden_dim=64, num_heads=8), dict(hidden_dim=40, num_heads=1)):
        enc = TextEncoder(**bad).to(gpu)
        with pytest.raises(NotImplementedError):
            enc.enable_backward()
        assert enc.backward_enabled is False
        with pytest.raises(ops.M2Error):
            ops.encoder_train_forward(list(enc.parameters()), torch.zeros(1, 3, dtype=torch.int64, device=gpu),
                                      enc.pos_encoding.pe[0], None, bad["num_heads"])


def test_optimizer_step_matches_float64(gpu):
    """zero_grad, backward of sum(out dy), SGD step on a model's text encoder, and the next module call on the
    updated weights."""
    from models.tts_model import M2TTSModel
    e = _expect("s1", gpu)
    torch.manual_seed(31)
    model = M2TTSModel().to(gpu).eval()
    model.text_encoder.load_state_dict(e["enc"].state_dict())
    model.text_encoder.enable_backward()
    params = list(model.text_encoder.parameters())
    ids, lengths, dy = e["ids"], e["lengths"], e["dy"]
    opt = torch.optim.SGD(params, lr=LR)
    opt.zero_grad()
    (model.text_encoder(ids, lengths)[0] * dy).sum().backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(params, e["got"]))
    opt.step()

    p64 = [p.detach().cpu().double().requires_grad_() for p in e["params"]]
    for p, g in zip(p64, e["grads"]):
        p.grad = g.clone()
    torch.optim.SGD(p64, lr=LR).step()
    bar_g = 32.0 * max(e["s"], EPS)
    seen = torch.zeros(256, dtype=torch.bool)
    seen[ids.cpu().flatten()] = True
    for i, (p, q, g) in enumerate(zip(params, p64, e["grads"])):
        err = float((p.detach().cpu().double() - q.detach()).abs().max())
        bar = LR * bar_g * float(g.abs().max()) + EPS * float(q.detach().abs().max())
        assert err <= bar, (i, err, bar)
        assert not torch.equal(p.detach(), e["params"][i])  # every parameter moved
    moved = (params[0].detach() != e["params"][0]).any(dim=1).cpu()
    assert torch.equal(moved, seen)  # of the table, exactly the rows that occur
    after, _ = model.text_encoder(ids, lengths)
    alone = copy.deepcopy(model.text_encoder).enable_backward(False)
    with torch.no_grad():
        want, _ = alone(ids, lengths)
    assert after.grad_fn is not None and torch.equal(after.detach(), want)  # no stale pack is read
    assert not torch.equal(want, e["out"])
    model.text_encoder.enable_backward(False)


# ---- the teacher-forced mel step ---------------------------------------------------

def test_teacher_forced_mel_step(gpu):
    """A default M2TTSModel, B = 2, S = 6, lengths (6, 4), integer target durations in [0, 3]: text_encoder ->
    length_regulator(enc, target_durations) -> decoder -> L1 mel loss with all three switches on.  Every
    text-encoder and decoder .grad is the ops-level composition encoder backward o regulator adjoint o
    decoder backward, bit for bit; that composition is the float64 chain's within the bar, with both tapes'
    predicates; the duration predictor's .grad stays None."""
    from m2amd import ops
    from models.tts_model import M2TTSModel
    torch.manual_seed(41)
    model = M2TTSModel().to(gpu).eval()
    heads, B, S, H, M = 2, 2, 6, 64, 64
    g = torch.Generator().manual_seed(42)
    ids_c = torch.randint(0, 256, (B, S), generator=g)
    lengths_c = torch.tensor([6, 4])
    dur_c = torch.tensor([[2, 0, 3, 1, 2, 1], [1, 3, 0, 2, 0, 0]])
    assert int(dur_c.min()) == 0 and int(dur_c.max()) == 3
    T = int(dur_c.sum(1).max())
    target_c = torch.randn(B, T, M, generator=g)
    ids, lengths, dur, target = (t.to(gpu) for t in (ids_c, lengths_c, dur_c, target_c))
    eparams, dparams = list(model.text_encoder.parameters()), list(model.decoder.parameters())
    model.text_encoder.enable_backward()
    model.length_regulator.enable_backward()
    model.decoder.enable_backward()
    try:
        enc, mask = model.text_encoder(ids, lengths)
        reg = model.length_regulator(enc, dur)
        mel = model.decoder(reg)
        assert enc.grad_fn is not None and reg.grad_fn is not None and mel.grad_fn is not None
        assert mel.shape == (B, T, M)
        F.l1_loss(mel, target).backward()
        got = [p.grad.clone() for p in eparams + dparams]
        assert all(bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 for a in got)
        assert all(p.grad is None for p in model.duration_predictor.parameters())
        assert all(p.grad is None for p in model.vocoder.parameters())

        # the ops-level composition
        ep, dp = [p.detach() for p in eparams], [p.detach() for p in dparams]
        out, tape_e = ops.encoder_train_forward(ep, ids, model.text_encoder.pos_encoding.pe[0], mask, heads)
        assert torch.equal(out, enc.detach())
        reg2, cum = ops.regulate_with_counts(out, dur)
        assert torch.equal(reg2, reg.detach()) and torch.equal(reg2, ops.regulate(out, dur))
        mel2, tape_d = ops.decoder_train_forward(dp, reg2, heads)
        assert torch.equal(mel2, mel.detach())
        leaf = mel2.clone().requires_grad_()
        F.l1_loss(leaf, target).backward()
        g_mel = leaf.grad
        d_reg, dgrads = ops.decoder_backward(dp, reg2, tape_d, g_mel, heads)
        d_enc = ops.regulate_backward(d_reg, cum, S)
        egrads = ops.encoder_backward(ep, ids, mask, tape_e, d_enc, heads)
        assert all(torch.equal(a, b) for a, b in zip(got, egrads + dgrads))

        # the float64 chain from that cotangent, with both tapes' predicates
        _, emaps = ops.encoder_tape_maps(tape_e, 256, H, 2, heads, B, S)
        dmaps = ops.decoder_tape_maps(tape_d, H, M, 2, heads, B, T)
        pos_e, pos_d = [m["h"].cpu() > 0 for m in emaps], [m["h"].cpu() > 0 for m in dmaps]
        cum64 = orc.frame_counts(dur_c)
        assert torch.equal(cum.cpu().to(torch.int64), cum64)

        def chain(dtype, pe_=None, pd_=None):
            e_ = orc.cpu_copy(model.text_encoder, dtype)
            d_ = dorc.cpu_copy(model.decoder, dtype)
            o, pre_e, _ = orc.forward(e_, ids_c, lengths_c, pe_)
            m_, pre_d = dorc.forward(d_, orc.regulate(o, cum64, T), pd_)
            grads = torch.autograd.grad(m_, orc.parameters(e_) + dorc.parameters(d_), g_mel.cpu().to(dtype))
            return list(grads), [u.detach() for u in pre_e], [u.detach() for u in pre_d]

        g64, pre_e64, pre_d64 = chain(torch.float64)
        g32, pre_e32, pre_d32 = chain(torch.float32)
        want, pre_e, pre_d = chain(torch.float64, pos_e, pos_d)
        kinks = _kinks("mel step encoder", pre_e, pre_e32, pre_e64, pos_e) + \
            _kinks("mel step decoder", pre_d, pre_d32, pre_d64, pos_d)
        assert kinks <= KINK_CAP
        s = max(_rel(a, b) for a, b in zip(g32, g64) if float(b.abs().max()) > 0)
        bar = 32.0 * max(s, EPS)
        worst = max(_rel(a.cpu(), b) for a, b in zip(got, want))
        print(f"mel step: {kinks} kinks differ; worst rel max err {worst:.3e}, cpu float32 {s:.3e}, bar {bar:.3e}")
        for i, (a, b) in enumerate(zip(got, want)):
            assert _rel(a.cpu(), b) <= bar, (i, _rel(a.cpu(), b), bar)
    finally:
        model.text_encoder.enable_backward(False)
        model.length_regulator.enable_backward(False)
        model.decoder.enable_backward(False)
