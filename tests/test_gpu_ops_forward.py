"""GPU: the per-op fp32 forward kernels behind ``m2amd.ops`` (m2_linear, m2_layer_norm, m2_conv1d,
m2_conv1d_ex, m2_conv_transpose1d, m2_embed_positional, m2_add_positional) and the exact-f32 attention
``attention_kernel<HD>`` (M2_ATT_F32=1), each against the same operation written out in torch on the CPU in
float64 from the header's formula (include/m2tts_hip.h), at the edges of the kernels' tiles.

The bar is the one of test_gpu_vocoder_backward.py / test_gpu_decoder_backward.py and never comes from the
GPU's output:
    |y_gpu - y_f64| <= 32 x max(s, 2^-24) x max|y_f64|,
s the relative max deviation of the CPU float32 evaluation of the same formula from the float64 one, computed
here for every case.  Every test prints its worst error, that case's s and bar, and the worst error-to-bar
ratio.

The embedding's bound is elementwise, 2^-23 x (|e x scale| + |pe|) (one rounding of the product and one of the
sum, or one fma); add_positional is bit-equal to torch's float32 add.

The ``ops`` wrappers' argument checks are tested with ``_lib.call`` replaced by a stub that fails the test:
whatever the wrapper does, a mismatched shape cannot reach a launch.

m2_conv1d_ex: the lengths are those whose output length Lo is 1, 255, 256 and 257.  Where Lo = 1 would need an
empty or negative input length ((2, 1, 1) and (4, 1, 2): Lo = L + 1, (3, 2, 5): Lo = L + 6; torch refuses an
empty length too) the shortest input, L = 1, stands in.
"""
import pytest
import torch
import torch.nn.functional as F

import m2tts_oracle as orc
from conftest import MEL_MAXABS_TOL, golden_state, maxabs, stage_config
from test_gpu_attention import TOL as SPLIT_TOL
from test_gpu_attention import make_qkv

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
ENC_TOL = 1e-4  # test_gpu_parity.py


class Worst:
    """The case of a test with the largest error-to-bar ratio; ``check`` asserts every case."""

    def __init__(self, what):
        self.what, self.ratio, self.line, self.cases = what, -1.0, "", 0

    def check(self, case, got, ref64, ref32):
        got = got.detach().cpu()
        assert got.dtype == torch.float32 and got.shape == ref64.shape, (self.what, case, got.shape, ref64.shape)
        assert bool(torch.isfinite(got).all()), (self.what, case, "not finite")
        top = float(ref64.abs().max())
        err = float((got.double() - ref64).abs().max())
        self.cases += 1
        if top == 0.0:
            assert err == 0.0, (self.what, case, err)
            return
        s = float((ref32.double() - ref64).abs().max()) / top
        bar = 32.0 * max(s, EPS) * top
        if err / bar > self.ratio:
            self.ratio = err / bar
            self.line = f"worst err {err:.3e}, cpu float32 s {s:.3e}, bar {bar:.3e} at {case}"
        assert err <= bar, (self.what, case, err, s, bar)

    def report(self):
        print(f"{self.what}: {self.cases} cases, {self.line}, err/bar {self.ratio:.3f}")


def _gen(*seed):
    n = 0
    for v in seed:
        n = n * 1009 + int(v) + 1
    return torch.Generator().manual_seed(n)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ---- m2_linear ---------------------------------------------------------------------

def ref_layer_norm(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def ref_linear(dt, x, w, b=None, ln=None, relu=False, res=None):
    """y = act(LN?(x) . w^T + b) (+ res), the header's m2_linear."""
    x = x.to(dt)
    if ln is not None:
        x = ref_layer_norm(x, ln[0].to(dt), ln[1].to(dt))
    y = x @ w.to(dt).t()
    if b is not None:
        y = y + b.to(dt)
    if relu:
        y = y.clamp(min=0)
    if res is not None:
        y = y + res.to(dt)
    return y


LINEAR_N = (1, 31, 32, 33, 64, 65, 80)
LINEAR_R = (1, 63, 64, 65, 130)
# name: bias, ln, relu, residual, out=
LINEAR_FORMS = {"plain": (0, 0, 0, 0, 0), "bias": (1, 0, 0, 0, 0), "bias_relu": (1, 0, 1, 0, 0), "ln": (0, 1, 0, 0, 0),
                "ln_bias_relu": (1, 1, 1, 0, 0), "bias_res": (1, 0, 0, 1, 0), "ln_bias_res": (1, 1, 0, 1, 0),
                "out": (1, 0, 0, 0, 1)}


@pytest.mark.parametrize("K", [8, 64, 96, 256])
def test_linear_tile_edges(gpu, K):
    """N across the 32-column wave sub-tile and the 64-column tile (a whole sub-tile past N returns early, a
    partial one drops lanes), R across the 64-row tile (zero-padded rows, through the LN prologue too), every
    epilogue, and each call repeated bit for bit."""
    from m2amd import ops
    worst = Worst(f"linear K={K}")
    for N in LINEAR_N:
        for R in LINEAR_R:
            g = _gen(K, N, R)
            x, w, b, res = 1.5 * _randn(g, R, K) + 0.25, _randn(g, N, K) / K ** 0.5, _randn(g, N), _randn(g, R, N)
            ln = (1.0 + 0.3 * _randn(g, K), 0.5 * _randn(g, K))
            d = [t.to(gpu) for t in (x, w, b, res, *ln)]
            for name, (ub, ul, ur, us, uo) in LINEAR_FORMS.items():
                kw = dict(b=b if ub else None, ln=ln if ul else None, relu=bool(ur), res=res if us else None)
                ref64, ref32 = ref_linear(torch.float64, x, w, **kw), ref_linear(torch.float32, x, w, **kw)
                out = torch.full((R, N), float("nan"), device=gpu) if uo else None

                def run(out=out):
                    return ops.linear(d[0], d[1], d[2] if ub else None, ln=(d[4], d[5]) if ul else None,
                                      act=ops.ACT_RELU if ur else ops.ACT_NONE, residual=d[3] if us else None, out=out)
                y = run()
                if uo:
                    assert y is out
                worst.check((name, N, R), y, ref64, ref32)
                again = run(None if not uo else torch.full((R, N), float("nan"), device=gpu))
                assert torch.equal(y, again), (name, K, N, R)
    worst.report()


@pytest.mark.parametrize("R", [1, 65, 130])
def test_linear_ln_constant_rows(gpu, R):
    """K = 64, every element 1.5: each partial sum is exact in fp32, the variance is 0 and the normalised row
    is exactly beta, so the result is the plain linear of beta, bit for bit."""
    from m2amd import ops
    g = _gen(R)
    K, N = 64, 33
    w, b, gamma, beta = (t.to(gpu) for t in (_randn(g, N, K), _randn(g, N), 1.0 + _randn(g, K), _randn(g, K)))
    x = torch.full((R, K), 1.5, device=gpu)
    y = ops.linear(x, w, b, ln=(gamma, beta))
    want = ops.linear(beta.expand(R, K), w, b)
    assert bool(torch.isfinite(y).all()) and torch.equal(y, want)


def test_linear_refusals_leave_the_output_alone(gpu):
    from m2amd import ops
    R, N = 5, 7
    for K in (0, 12, 264):
        out = torch.full((R, N), 7.0, device=gpu)
        with pytest.raises(ops.M2Error):
            ops.linear(torch.ones(R, K, device=gpu), torch.ones(N, K, device=gpu), out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), K
    out = torch.full((R, N), 7.0, device=gpu)
    with pytest.raises(ops.M2Error):
        ops.linear(torch.ones(R, 64, device=gpu), torch.ones(N, 64, device=gpu), act=ops.ACT_LEAKY, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_linear_empty(gpu):
    from m2amd import ops
    w = torch.ones(7, 64, device=gpu)
    y = ops.linear(torch.ones(0, 64, device=gpu), w, torch.ones(7, device=gpu))
    assert y.shape == (0, 7) and y.dtype == torch.float32 and y.is_cuda
    y = ops.linear(torch.ones(2, 0, 64, device=gpu), w)
    assert y.shape == (2, 0, 7)
    y = ops.linear(torch.ones(5, 64, device=gpu), torch.ones(0, 64, device=gpu))
    assert y.shape == (5, 0) and y.dtype == torch.float32 and y.is_cuda
    torch.cuda.synchronize()


# ---- m2_layer_norm -----------------------------------------------------------------

LN_R = (1, 3, 4, 5, 260)


@pytest.mark.parametrize("K", [1, 5, 63, 64, 65, 96, 300])
def test_layer_norm_edges(gpu, K):
    """One wave per row, four rows per workgroup: K across the 64 lanes, R across the four rows."""
    from m2amd import ops
    worst = Worst(f"layer_norm K={K}")
    for R in LN_R:
        g = _gen(K, R)
        x, gamma, beta = 2.0 * _randn(g, R, K) + 0.5, 1.0 + 0.3 * _randn(g, K), _randn(g, K)
        y = ops.layer_norm(x.to(gpu), gamma.to(gpu), beta.to(gpu))
        if K == 1:
            assert torch.equal(y.cpu(), beta.expand(R, 1)), R
        worst.check(R, y, ref_layer_norm(x.double(), gamma.double(), beta.double()), ref_layer_norm(x, gamma, beta))
        assert torch.equal(y, ops.layer_norm(x.to(gpu), gamma.to(gpu), beta.to(gpu)))
    worst.report()


@pytest.mark.parametrize("K", [64, 96])
def test_linear_ln_prologue_agrees_with_layer_norm(gpu, K):
    """ops.linear(x, I, ln=(g, b)) is LayerNorm(x): the prologue's rows through an exact product."""
    from m2amd import ops
    worst = Worst(f"linear LN prologue vs layer_norm K={K}")
    for R in LN_R:
        g = _gen(K, R, 1)
        x, gamma, beta = 2.0 * _randn(g, R, K) + 0.5, 1.0 + 0.3 * _randn(g, K), _randn(g, K)
        ref64, ref32 = ref_layer_norm(x.double(), gamma.double(), beta.double()), ref_layer_norm(x, gamma, beta)
        ln = ops.layer_norm(x.to(gpu), gamma.to(gpu), beta.to(gpu))
        lin = ops.linear(x.to(gpu), torch.eye(K, device=gpu), ln=(gamma.to(gpu), beta.to(gpu)))
        worst.check(("prologue", R), lin, ref64, ref32)
        top = float(ref64.abs().max())
        s = float((ref32.double() - ref64).abs().max()) / top
        assert maxabs(lin, ln) <= 32.0 * max(s, EPS) * top, R
    worst.report()


# ---- m2_conv1d, m2_conv1d_ex -------------------------------------------------------

def ref_act(v, act):
    if act == 1:
        return F.leaky_relu(v, 0.1)
    if act == 2:
        return torch.tanh(v)
    if act == 3:
        return torch.relu(v)
    if act == 4:
        return F.softplus(v, beta=1, threshold=20)
    return v


def ref_epilogue(v, act=0, affine=None, res=None):
    """act(v [* alpha + beta]) (+ res) of v = conv1d(x; w, b): affine, then act, then the residual (the header's
    order); also the value the activation saw."""
    dt = v.dtype
    if affine is not None:
        v = v * affine[0].to(dt)[None, :, None] + affine[1].to(dt)[None, :, None]
    pre = v
    v = ref_act(v, act)
    if res is not None:
        v = v + res.to(dt)
    return v, pre


def ref_conv(dt, x, w, b, dilation=1, padding=None, **epilogue):
    pad = w.shape[2] // 2 if padding is None else padding
    return ref_epilogue(F.conv1d(x.to(dt), w.to(dt), b.to(dt), padding=pad, dilation=dilation), **epilogue)


CONV_L = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2049)


@pytest.mark.parametrize("Cout", [1, 2, 6, 8, 12, 24])
@pytest.mark.parametrize("k", [1, 3])
def test_conv1d_tiled_edges(gpu, k, Cout):
    """conv_kernel: four steps per thread and 1024 per workgroup (L around both), 1 / 2 / 4 / 8 output channels
    per workgroup (Cout 1, 2 and 6, 12, 8 and 24), every activation, with and without the affine and the
    residual.  Softplus runs on inputs scaled so that its pre-activations pass 20 and fall below -30."""
    from m2amd import ops
    B = 2
    worst = Worst(f"conv1d k={k} Cout={Cout}")
    above, below = False, False
    for Cin in (1, 3, 16):
        for L in CONV_L:
            g = _gen(k, Cout, Cin, L)
            x, w, b = _randn(g, B, Cin, L), _randn(g, Cout, Cin, k) / (Cin * k) ** 0.5, 0.5 * _randn(g, Cout)
            aff, res = (1.0 + 0.3 * _randn(g, Cout), 0.5 * _randn(g, Cout)), _randn(g, B, Cout, L)
            d = {"x": x.to(gpu), "xs": (18.0 * x).to(gpu), "w": w.to(gpu), "b": b.to(gpu), "res": res.to(gpu),
                 "aff": (aff[0].to(gpu), aff[1].to(gpu))}
            conv = {(key, dt): F.conv1d(xin.to(dt), w.to(dt), b.to(dt), padding=k // 2)
                    for key, xin in (("x", x), ("xs", 18.0 * x)) for dt in (torch.float64, torch.float32)}
            for act in range(5):
                key = "xs" if act == 4 else "x"
                for ua in (False, True):
                    for us in (False, True):
                        kw = dict(act=act, affine=aff if ua else None, res=res if us else None)
                        ref64, pre = ref_epilogue(conv[key, torch.float64], **kw)
                        ref32, _ = ref_epilogue(conv[key, torch.float32], **kw)
                        if act == 4:
                            above, below = above or bool((pre > 20).any()), below or bool((pre < -30).any())
                        y = ops.conv1d(d[key], d["w"], d["b"], act=act, affine=d["aff"] if ua else None,
                                       residual=d["res"] if us else None)
                        worst.check((Cin, L, act, ua, us), y, ref64, ref32)
    assert above and below, "softplus never saw both of its branches' ends"
    worst.report()


CONV_EX = ((2, 1, 1), (4, 1, 2), (5, 1, 2), (5, 3, 6), (7, 2, 6), (3, 1, 0), (3, 2, 5))


@pytest.mark.parametrize("k,dil,pad", CONV_EX)
def test_conv1d_general_edges(gpu, k, dil, pad):
    """conv_general_kernel: one output step per thread, 256 per workgroup (Lo around it), 1 / 2 / 4 output
    channels per workgroup, even kernels, dilation, no padding and more padding than the kernel needs; plain,
    affine + leaky, and relu + residual where the length is kept."""
    from m2amd import ops
    B, Cin = 2, 3
    worst = Worst(f"conv1d_ex k={k} dil={dil} pad={pad}")
    shift = 2 * pad - dil * (k - 1)  # Lo - L
    for Cout in (1, 2, 4):
        for Lo in (1, 255, 256, 257):
            L = max(Lo - shift, 1)
            g = _gen(k, dil, pad, Cout, Lo)
            x, w, b = _randn(g, B, Cin, L), _randn(g, Cout, Cin, k) / (Cin * k) ** 0.5, 0.5 * _randn(g, Cout)
            aff = (1.0 + 0.3 * _randn(g, Cout), 0.5 * _randn(g, Cout))
            forms = [dict(), dict(act=1, affine=aff)]
            if shift == 0:
                forms.append(dict(act=3, res=_randn(g, B, Cout, L)))
            for kw in forms:
                ref64, _ = ref_conv(torch.float64, x, w, b, dilation=dil, padding=pad, **kw)
                ref32, _ = ref_conv(torch.float32, x, w, b, dilation=dil, padding=pad, **kw)
                assert ref64.shape[2] == L + shift
                a = kw.get("affine")
                y = ops.conv1d(x.to(gpu), w.to(gpu), b.to(gpu), act=kw.get("act", 0), dilation=dil, padding=pad,
                               affine=None if a is None else (a[0].to(gpu), a[1].to(gpu)),
                               residual=None if "res" not in kw else kw["res"].to(gpu))
                worst.check((Cout, L, sorted(kw)), y, ref64, ref32)
    worst.report()


def test_conv1d_general_lengths(gpu):
    """Lo = 0 is an empty tensor, Lo < 0 and a residual of another length are errors."""
    from m2amd import ops
    w, b = torch.ones(2, 3, 7, device=gpu), torch.ones(2, device=gpu)
    y = ops.conv1d(torch.ones(2, 3, 12, device=gpu), w, b, dilation=2, padding=0)  # 12 - 12
    assert y.shape == (2, 2, 0) and y.dtype == torch.float32 and y.is_cuda
    with pytest.raises(RuntimeError):
        ops.conv1d(torch.ones(2, 3, 3, device=gpu), w, b, dilation=2, padding=0)  # 3 - 12
    x = torch.ones(2, 3, 10, device=gpu)
    with pytest.raises(RuntimeError):
        ops.conv1d(x, torch.ones(3, 3, 4, device=gpu), torch.ones(3, device=gpu), padding=2, residual=x)  # Lo = 11
    torch.cuda.synchronize()


# ---- m2_conv_transpose1d -----------------------------------------------------------

@pytest.mark.parametrize("rate", [2, 4])
def test_conv_transpose1d_edges(gpu, rate):
    """convT_kernel: two input frames per thread, 512 per workgroup (L around both), 1 / 2 / 4 / 8 output
    channels per workgroup, against F.conv_transpose1d(stride r, padding r // 2)."""
    from m2amd import ops
    B = 2
    worst = Worst(f"conv_transpose1d rate={rate}")
    for Cout in (1, 2, 4, 8):
        for Cin in (1, 16):
            for L in (1, 2, 3, 511, 512, 513):
                g = _gen(rate, Cout, Cin, L)
                x, w, b = _randn(g, B, Cin, L), _randn(g, Cin, Cout, 2 * rate) / (2 * Cin) ** 0.5, 0.5 * _randn(g, Cout)
                for act in (ops.ACT_NONE, ops.ACT_LEAKY):
                    def ref(dt):
                        return ref_act(F.conv_transpose1d(x.to(dt), w.to(dt), b.to(dt), stride=rate,
                                                          padding=rate // 2), act)
                    y = ops.conv_transpose1d(x.to(gpu), w.to(gpu), b.to(gpu), rate, act=act)
                    assert y.shape == (B, Cout, rate * L)
                    worst.check((Cout, Cin, L, act), y, ref(torch.float64), ref(torch.float32))
    worst.report()


def test_conv_transpose1d_rate_3_is_refused(gpu):
    from m2amd import ops
    with pytest.raises(ops.M2Error):
        ops.conv_transpose1d(torch.ones(1, 2, 5, device=gpu), torch.ones(2, 2, 6, device=gpu),
                             torch.ones(2, device=gpu), 3)
    torch.cuda.synchronize()


# ---- m2_embed_positional, m2_add_positional ----------------------------------------

@pytest.mark.parametrize("B,S,H", [(2, 5, 8), (17, 1000, 64)])
def test_positional_kernels(gpu, B, S, H):
    """(17, 1000, 64) is 1.09 M elements: past the 4096 x 256 threads of the capped grid, so the grid-stride
    loop takes a second turn.  ids outside [0, vocab) read a zero row: those outputs are pe[s] exactly."""
    from m2amd import ops
    vocab = 37
    g = _gen(B, S, H)
    ids = torch.randint(0, vocab, (B, S), generator=g)
    ids[0, 0], ids[B - 1, S - 1], ids[1, S // 2] = -1, vocab, vocab + 5
    emb, pe = _randn(g, vocab, H), _randn(g, S + 3, H)
    scale = ops.sqrt_hidden(H)
    y = ops.embed_positional(ids.to(gpu), emb.to(gpu), pe.to(gpu), scale).cpu()
    assert y.shape == (B, S, H) and y.dtype == torch.float32
    inside = (ids >= 0) & (ids < vocab)
    e = emb[ids.clamp(0, vocab - 1)].double() * inside[..., None]
    es = e * float(torch.tensor(scale, dtype=torch.float32))  # scale = sqrt(H) as fp32
    ref = es + pe[:S].double()
    bound = 2.0 ** -23 * (es.abs() + pe[:S].double().abs())
    err = (y.double() - ref).abs()
    print(f"embed_positional {(B, S, H)}: worst err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    for b_, s_ in ((0, 0), (B - 1, S - 1), (1, S // 2)):
        assert torch.equal(y[b_, s_], pe[s_])
    x = _randn(g, B, S, H)
    z = ops.add_positional(x.to(gpu), pe.to(gpu)).cpu()
    assert torch.equal(z, x + pe[:S])
    assert torch.equal(ops.add_positional(x.to(gpu), pe[None].to(gpu)).cpu(), z)


# ---- the exact-f32 attention -------------------------------------------------------

def ref_attention(dt, qkv, heads, mask):
    """softmax(q k^T / sqrt(hd), masked_fill(-1e9)) v for qkv [B,N,3H] laid out (3, heads, hd)."""
    B, N, H3 = qkv.shape
    H = H3 // 3
    hd = H // heads
    q, k, v = qkv.to(dt).view(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / hd ** 0.5
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], -1e9)
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H)


ATT_N = (1, 63, 64, 65, 129, 511)


@pytest.mark.parametrize("hd", [16, 32, 48, 64])
def test_attention_f32_shapes(gpu, hd, monkeypatch):
    """attention_kernel<HD> (M2_ATT_F32=1): N around the 64-query workgroup and the 64-key chunk, unmasked and
    with lengths (N, max(1, N // 2), 0); the fully masked utterance is the uniform mean of V over its N keys."""
    from m2amd import ops
    monkeypatch.setenv("M2_ATT_F32", "1")
    heads, H, B = 2, 2 * hd, 3
    worst = Worst(f"attention f32 hd={hd}")
    for N in ATT_N:
        qkv = make_qkv(B, N, H, heads, "random", _gen(hd, N))
        lens = torch.tensor([N, max(1, N // 2), 0])
        for mask in (None, torch.arange(N)[None, :] < lens[:, None]):
            got = ops.attention_core(qkv.to(gpu), heads, None if mask is None else mask.to(gpu))
            ref64 = ref_attention(torch.float64, qkv, heads, mask)
            worst.check((N, mask is not None), got, ref64, ref_attention(torch.float32, qkv, heads, mask))
            if mask is not None:
                mean = qkv[2, :, 2 * H:].double().mean(0)
                assert maxabs(ref64[2], mean.expand(N, H)) <= 1e-12
                assert torch.equal(got, ops.attention_core(qkv.to(gpu), heads, mask.to(torch.uint8).to(gpu)))
    worst.report()


@pytest.mark.parametrize("pattern", ["ramp", "fall", "large"])
@pytest.mark.parametrize("hd,N", [(32, 500), (64, 300)])
def test_attention_f32_rescale_patterns(gpu, pattern, hd, N, monkeypatch):
    """The running maximum moves on every chunk (ramp), never after the first (fall), and large logits."""
    from m2amd import ops
    monkeypatch.setenv("M2_ATT_F32", "1")
    heads, H = 2, 2 * hd
    qkv = make_qkv(2, N, H, heads, pattern, _gen(hd, N, len(pattern)))
    worst = Worst(f"attention f32 {pattern} hd={hd} N={N}")
    got = ops.attention_core(qkv.to(gpu), heads, None)
    worst.check(pattern, got, ref_attention(torch.float64, qkv, heads, None),
                ref_attention(torch.float32, qkv, heads, None))
    worst.report()


def test_attention_switch_selects_the_f32_kernel(gpu, monkeypatch):
    """hd 32, N 129: the result under M2_ATT_F32=1 is not the split-f16 kernel's bits, and each is within its
    own bar; the generic kernel (head_dim 20) is the same under the switch, bit for bit."""
    from m2amd import ops
    monkeypatch.delenv("M2_ATT_F32", raising=False)
    heads = 2
    qkv = make_qkv(3, 129, 64, heads, "random", _gen(129))
    odd = make_qkv(3, 65, 40, heads, "random", _gen(65))
    split = ops.attention_core(qkv.to(gpu), heads, None)
    generic = ops.attention_core(odd.to(gpu), heads, None)
    monkeypatch.setenv("M2_ATT_F32", "1")
    exact = ops.attention_core(qkv.to(gpu), heads, None)
    assert torch.equal(ops.attention_core(odd.to(gpu), heads, None), generic)
    ref64 = ref_attention(torch.float64, qkv, heads, None)
    worst = Worst("attention f32 vs split-f16")
    worst.check("exact", exact, ref64, ref_attention(torch.float32, qkv, heads, None))
    worst.check("generic", generic, ref_attention(torch.float64, odd, heads, None),
                ref_attention(torch.float32, odd, heads, None))
    worst.report()
    assert maxabs(split, ref64) <= SPLIT_TOL
    assert not torch.equal(exact, split)


# ---- a model created under M2_ATT_F32=1 --------------------------------------------

def build_model(stage, dev):
    from models.tts_model import M2TTSModel
    m = M2TTSModel(**stage_config(stage).as_dict())
    m.load_state_dict(golden_state(stage))
    return m.to(dev).eval()


@pytest.mark.parametrize("stage", ["s1", "s2"])
def test_model_under_att_f32(gpu, stage, monkeypatch):
    """M2_ATT_F32=1 at handle creation: the fp32 transformer path (m2_transformer_path 0), attention_kernel<32>
    (stage1) / <48> (stage2) in the decoder and the masked encoder, against the CPU oracle."""
    from m2amd import _lib
    monkeypatch.setenv("M2_ATT_F32", "1")
    cfg, sd = stage_config(stage), golden_state(stage)
    m = build_model(stage, gpu)
    assert _lib.load().m2_transformer_path(m._hip(gpu).handle) == 0
    worst = 0.0
    for T in (63, 64, 65, 129, 300):
        x = torch.randn(2, T, cfg.hidden_dim, generator=_gen(T))
        mel = m.decoder(x.to(gpu))
        ref = orc.mel_decoder(sd, cfg, x)
        assert mel.shape == ref.shape
        worst = max(worst, maxabs(mel, ref))
        assert maxabs(mel, ref) <= MEL_MAXABS_TOL, (T, maxabs(mel, ref))
    ids = torch.randint(0, 42, (3, 65), generator=_gen(65))
    lens = torch.tensor([65, 33, 1])
    enc, mask = m.text_encoder(ids.to(gpu), lens.to(gpu))
    ref, ref_mask = orc.text_encoder(sd, cfg, ids, lens)
    print(f"{stage} under M2_ATT_F32: decoder worst max-abs {worst:.3e} (bar {MEL_MAXABS_TOL:.0e}), "
          f"encoder max-abs {maxabs(enc, ref):.3e} (bar {ENC_TOL:.0e})")
    assert torch.equal(mask.cpu(), ref_mask)
    assert maxabs(enc, ref) <= ENC_TOL


# ---- the wrappers' argument checks: nothing may reach a launch ----------------------

@pytest.fixture
def no_launch(gpu, monkeypatch):
    """``ops`` with ``_lib.call`` replaced by a stub that fails the test."""
    from m2amd import _lib, ops

    def stub(name, *args):
        pytest.fail(f"{name} was called with mismatched arguments")
    monkeypatch.setattr(_lib, "call", stub)
    return ops


def _t(gpu, *shape, dtype=torch.float32):
    return torch.ones(*shape, device=gpu, dtype=dtype)


def test_linear_arguments(gpu, no_launch):
    ops = no_launch
    x, w = _t(gpu, 5, 64), _t(gpu, 7, 64)
    bad = [dict(weight=_t(gpu, 7, 72)), dict(weight=_t(gpu, 7, 56)), dict(weight=_t(gpu, 7, 8, 8)),
           dict(bias=_t(gpu, 8)), dict(bias=_t(gpu, 7, 1)), dict(ln=(_t(gpu, 63), _t(gpu, 64))),
           dict(ln=(_t(gpu, 64), _t(gpu, 65))), dict(residual=_t(gpu, 5, 8)), dict(residual=_t(gpu, 7, 5)),
           dict(out=_t(gpu, 5, 8)), dict(out=_t(gpu, 35)), dict(out=_t(gpu, 7, 5).t())]
    for kw in bad:
        args = dict(weight=w)
        args.update(kw)
        shapes = [tuple(t.shape) for v in kw.values() for t in (v if isinstance(v, tuple) else (v,))]
        with pytest.raises(RuntimeError) as e:
            ops.linear(x, **args)
        assert not isinstance(e.value, ops.M2Error) and any(str(s) in str(e.value) for s in shapes), (kw, str(e.value))
    for kw in (dict(bias=_t(gpu, 7, dtype=torch.float64)), dict(ln=(_t(gpu, 64, dtype=torch.float64), _t(gpu, 64))),
               dict(residual=_t(gpu, 5, 7, dtype=torch.float16)), dict(out=_t(gpu, 5, 7, dtype=torch.float64))):
        with pytest.raises(TypeError):
            ops.linear(x, w, **kw)


def test_layer_norm_arguments(gpu, no_launch):
    ops = no_launch
    x = _t(gpu, 3, 10)
    for g, b in ((_t(gpu, 9), _t(gpu, 10)), (_t(gpu, 10), _t(gpu, 11)), (_t(gpu, 1, 10), _t(gpu, 10))):
        with pytest.raises(RuntimeError, match=r"must be \[10\]"):
            ops.layer_norm(x, g, b)
    with pytest.raises(TypeError):
        ops.layer_norm(x, _t(gpu, 10, dtype=torch.float64), _t(gpu, 10))


def test_conv_arguments(gpu, no_launch):
    ops = no_launch
    x, w, b = _t(gpu, 2, 3, 10), _t(gpu, 4, 3, 3), _t(gpu, 4)
    with pytest.raises(RuntimeError, match=r"\(4, 2, 3\)"):
        ops.conv1d(x, _t(gpu, 4, 2, 3), b)
    with pytest.raises(RuntimeError, match=r"\(5,\)"):
        ops.conv1d(x, w, _t(gpu, 5))
    with pytest.raises(RuntimeError, match=r"\(3,\)"):
        ops.conv1d(x, w, b, affine=(_t(gpu, 3), _t(gpu, 4)))
    with pytest.raises(RuntimeError, match=r"\(5,\)"):
        ops.conv1d(x, w, b, affine=(_t(gpu, 4), _t(gpu, 5)), dilation=2, padding=2)
    with pytest.raises(RuntimeError, match=r"\(2, 3, 10\)"):
        ops.conv1d(x, w, b, residual=x)
    with pytest.raises(RuntimeError, match=r"\(2, 4, 9\)"):
        ops.conv1d(x, w, b, residual=_t(gpu, 2, 4, 9), dilation=2, padding=2)
    with pytest.raises(TypeError):
        ops.conv1d(x, w, b, affine=(_t(gpu, 4, dtype=torch.float64), _t(gpu, 4)))
    with pytest.raises(TypeError):
        ops.conv1d(x, w, _t(gpu, 4, dtype=torch.float64))
    wt = _t(gpu, 3, 4, 8)
    with pytest.raises(RuntimeError, match=r"\(2, 4, 8\)"):
        ops.conv_transpose1d(x, _t(gpu, 2, 4, 8), b, 4)
    with pytest.raises(RuntimeError, match=r"\(3, 4, 8\)"):
        ops.conv_transpose1d(x, wt, b, 2)
    with pytest.raises(RuntimeError, match=r"\(3,\)"):
        ops.conv_transpose1d(x, wt, _t(gpu, 3), 4)
    with pytest.raises(TypeError):
        ops.conv_transpose1d(x, wt, _t(gpu, 4, dtype=torch.float64), 4)


def test_attention_arguments(gpu, no_launch):
    ops = no_launch
    with pytest.raises(RuntimeError, match=r"\(2, 5, 64\)"):
        ops.attention_core(_t(gpu, 2, 5, 64), 2, None)
    qkv = _t(gpu, 2, 5, 96)
    for shape in ((2, 4), (5, 2), (2, 5, 1), (10,)):
        with pytest.raises(RuntimeError, match="key mask"):
            ops.attention_core(qkv, 2, _t(gpu, *shape, dtype=torch.bool))
    with pytest.raises(TypeError):
        ops.attention_core(qkv.double(), 2, None)


def test_positional_arguments(gpu, no_launch):
    ops = no_launch
    ids, emb = torch.zeros(2, 6, dtype=torch.int64, device=gpu), _t(gpu, 11, 8)
    for pe in (_t(gpu, 5, 8), _t(gpu, 6, 4), _t(gpu, 6, 16), _t(gpu, 48)):
        with pytest.raises(RuntimeError, match="positional table"):
            ops.embed_positional(ids, emb, pe, 1.0)
    for bad in (_t(gpu, 88), _t(gpu, 1, 11, 8)):
        with pytest.raises(RuntimeError, match="emb"):
            ops.embed_positional(ids, bad, _t(gpu, 6, 8), 1.0)
    with pytest.raises(TypeError):
        ops.embed_positional(ids, emb, _t(gpu, 6, 8, dtype=torch.float64), 1.0)
    x = _t(gpu, 2, 6, 8)
    for pe in (_t(gpu, 5, 8), _t(gpu, 6, 4), _t(gpu, 2, 6, 8)):
        with pytest.raises(RuntimeError):
            ops.add_positional(x, pe)
    with pytest.raises(TypeError):
        ops.add_positional(x, _t(gpu, 6, 8, dtype=torch.float64))


def test_strided_and_float64_vectors(gpu):
    """A strided bias, LayerNorm pair and affine give the result of their contiguous copies, bit for bit (they
    were read as contiguous before); a float64 one is a TypeError."""
    from m2amd import ops
    g = _gen(3)
    x, w = _randn(g, 9, 64).to(gpu), _randn(g, 33, 64).to(gpu)
    b2, g2, be2 = _randn(g, 66).to(gpu), _randn(g, 128).to(gpu), _randn(g, 128).to(gpu)
    want = ops.linear(x, w, b2[::2].contiguous(), ln=(g2[::2].contiguous(), be2[::2].contiguous()))
    assert torch.equal(ops.linear(x, w, b2[::2], ln=(g2[::2], be2[::2])), want)
    assert torch.equal(ops.layer_norm(x, g2[::2], be2[::2]), ops.layer_norm(x, g2[::2].contiguous(), be2[::2].contiguous()))
    xc, wc = _randn(g, 2, 3, 50).to(gpu), _randn(g, 33, 3, 3).to(gpu)
    aff = (g2[:66:2], be2[:66:2])
    assert torch.equal(ops.conv1d(xc, wc, b2[::2], affine=aff),
                       ops.conv1d(xc, wc, b2[::2].contiguous(), affine=(aff[0].contiguous(), aff[1].contiguous())))
    with pytest.raises(TypeError):
        ops.linear(x, w, b2[::2].double())
    torch.cuda.synchronize()
