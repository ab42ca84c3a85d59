"""GPU: the three-launch transformer layers (csrc/transformer_fused.hip:
ln_gemm_kernel with its SRC_X / SRC_EMBED / SRC_EXPAND row sources,
post_attn_kernel<H, NN, NW>, forms 0 to 2 of the launch plan that run_tf_plan
of m2_runtime.hip executes) and the model shapes off the two stages: what every handle
with num_heads != 2 runs, and what M2_TF_LAYER=0 selects.

Reference: the CPU oracle (oracle/m2tts_oracle.py) in float64 (ref64).  The
bar of a case is max(2e-5, 8 x e32), e32 = max|oracle in float32 - ref64| on
the same inputs: 2e-5 is test_gpu_tf_layer.py's ENC_TOL / DEC_TOL, 8 = 4 for
the split-f16 products (2^-22 relative against fp32's 2^-24) x 2 for another
summation order.  It comes from the reference alone.  The fp32 path (hidden
128, a mel width that is no multiple of 16) is held to the same bar.
Whole-inference cases use the suite's MEL_MAXABS_TOL / AUDIO_RMS_TOL on
weights with pinned durations (orc.pin_durations).

Every case asserts the driver it means to test (m2_debug_transformer_form).
The rows of a batch are flattened into 32-row tiles, so the shapes put
utterance boundaries inside a tile (S = 11, 13; T = 21), leave a one-row last
tile (R = 33, 65) and sit on both sides of the tile (31, 32, 33; 64, 65).

Forms (models c, e, s2): M2_TF_WAVES=4 | 8 and M2_TF_CHAIN=0, alone and
together, under the same bar and bit-identical to the default form: a
16-column block is accumulated by one wave over the whole K in the same order
whatever the wave count, and the chained kernels feed the same fp32 rows into
the same LayerNorm / GEMM code.

Each test prints one "TF3L family ... err bar e32" line per comparison
(pytest -s) for the record of the worst error-to-bar ratios."""
import functools

import pytest
import torch

import m2tts_oracle as orc
from conftest import AUDIO_RMS_TOL, MEL_MAXABS_TOL, golden_state, maxabs, rms, stage_config

pytestmark = pytest.mark.gpu

FLOOR = 2e-5  # test_gpu_tf_layer.py ENC_TOL / DEC_TOL
FACTOR = 8.0  # 4 (split-f16 product against an fp32 one) x 2 (summation order)

# id: hidden, heads, mel, encoder layers, decoder layers
GEOM = {
    "a": (32, 1, 64, 2, 2),   # (32,96), (32,64), head_dim 32
    "b": (32, 1, 32, 1, 1),   # (32,32), one-layer stacks
    "c": (64, 4, 80, 2, 2),   # (64,192), (64,80), head_dim 16
    "d": (64, 1, 64, 2, 1),   # (64,64), head_dim 64
    "e": (96, 3, 96, 2, 2),   # (96,288), (96,96), head_dim 32
    "f": (96, 6, 80, 1, 2),   # (96,80), head_dim 16
    "g": (64, 4, 64, 0, 0),   # zero-layer stacks
    "h": (128, 2, 80, 1, 1),  # fp32 layers, duration_kernel<128>
    "i": (128, 4, 64, 1, 1),  # the same at head_dim 32
    "j": (64, 2, 48, 1, 1),   # mel width without an ln_gemm instance, one-launch driver
    "k": (64, 4, 48, 1, 1),   # the same, three-launch driver
    "l": (96, 2, 40, 1, 1),   # mel width no multiple of 16: fp32 path
}
STAGE_IDS = ("s1", "s2")  # golden weights under M2_TF_LAYER=0: head_dim 32 and 48
# driver of (encoder, decoder) in the default form (m2_debug_transformer_form);
# s1 / s2: under M2_TF_LAYER=0
FORM = {"a": 2, "b": 2, "c": 2, "d": 2, "e": 2, "f": 2, "g": 2, "h": 0, "i": 0, "j": 3, "k": 2, "l": 0, "s1": 2,
        "s2": 2}
TPATH = {"h": 0, "i": 0, "l": 0}  # m2_transformer_path; every other model: 1

EDGE_MODELS = ["a", "b", "c", "d", "e", "f", "g", "s1", "s2"]
FORM_MODELS = ["c", "e", "s2"]
FORMS = {"w4": {"M2_TF_WAVES": "4"}, "w8": {"M2_TF_WAVES": "8"}, "c0": {"M2_TF_CHAIN": "0"},
         "c0w4": {"M2_TF_CHAIN": "0", "M2_TF_WAVES": "4"}}
ENC_SHAPES = [(1, 1), (1, 31), (1, 32), (3, 11), (2, 33), (5, 13)]
DEC_SHAPES = [(1, 1), (1, 33), (3, 21), (2, 64), (2, 65)]


def model_forms(models, forms=tuple(FORMS)):
    """(model, form) pairs: every model in the default form, FORM_MODELS in every form."""
    return [(mid, "default") for mid in models] + [(mid, f) for mid in models if mid in FORM_MODELS for f in forms]


# ---------------------------------------------------------------- models
def oracle_cfg(mid):
    if mid in STAGE_IDS:
        return stage_config(mid)
    h, heads, mel, le, ld = GEOM[mid]
    return orc.OracleConfig(vocab_size=50, hidden_dim=h, mel_channels=mel, text_encoder_layers=le, decoder_layers=ld,
                            num_heads=heads, vocoder_channels=64)


@functools.lru_cache(maxsize=None)
def state(mid, pinned):
    """The float32 state dict of a model: random init under a fixed seed (the
    stage models: the golden weights, whose durations are pinned already).
    The init leaves every bias at 0 and every LayerNorm / BatchNorm at the
    identity, which would hide a dropped bias or affine term (the golden
    weights do): outside the vocoder those are drawn at random too."""
    if mid in STAGE_IDS:
        return golden_state(mid)
    from models.tts_model import M2TTSModel
    seed = 1000 + sorted(GEOM).index(mid)
    torch.manual_seed(seed)
    kw = oracle_cfg(mid).as_dict()
    sd = {k: v.detach().clone() for k, v in M2TTSModel(**kw).state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    for k, v in sd.items():
        if k.startswith("vocoder.") or not v.is_floating_point():
            continue
        if k.endswith(".bias") or k.endswith(".running_mean"):
            sd[k] = 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith(".running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif ".norm" in k and k.endswith(".weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
    return orc.pin_durations(sd) if pinned else sd


@functools.lru_cache(maxsize=None)
def state64(mid, pinned):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in state(mid, pinned).items()}


@pytest.fixture(scope="module")
def zoo(gpu):
    """model(mid, pinned=False): each M2TTSModel built once per module."""
    from models.tts_model import M2TTSModel
    built = {}

    def model(mid, pinned=False):
        pinned = pinned or mid in STAGE_IDS
        if (mid, pinned) not in built:
            m = M2TTSModel(**oracle_cfg(mid).as_dict())
            m.load_state_dict(state(mid, pinned))
            built[(mid, pinned)] = m.to(gpu).eval()
        return built[(mid, pinned)]

    return model


def set_form(monkeypatch, mid, form):
    """The switches of a form (conftest's monkeypatch re-reads the library's
    table; the drivers consult it at every call), M2_TF_LAYER=0 for the stage
    models; returns the driver the form must report."""
    for name in ("M2_TF_WAVES", "M2_TF_CHAIN", "M2_TF_LAYER"):
        monkeypatch.delenv(name, raising=False)
    if mid in STAGE_IDS:
        monkeypatch.setenv("M2_TF_LAYER", "0")
    env = FORMS.get(form, {})
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    return 1 if env.get("M2_TF_CHAIN") == "0" and FORM[mid] == 2 else FORM[mid]


def assert_form(m, gpu, want, stacks=(0, 1)):
    from m2amd import _lib
    hm = m._hip(gpu)
    lib = _lib.load()
    for stack in stacks:
        got = lib.m2_debug_transformer_form(hm.handle, stack)
        assert got == want, f"stack {stack}: driver {got}, expected {want}"
    return hm


def check(family, tag, out, ref64, ref32):
    """out against ref64 under max(FLOOR, FACTOR x e32)."""
    e32 = maxabs(ref32, ref64)
    bar = max(FLOOR, FACTOR * e32)
    err = maxabs(out, ref64)
    print(f"TF3L {family} {tag} err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} e32 {e32:.3e}")
    assert tuple(out.shape) == tuple(ref64.shape)
    assert err <= bar, (tag, err, bar, e32)


# ---------------------------------------------------------------- inputs and references (computed once)
@functools.lru_cache(maxsize=None)
def enc_inputs(B, S):
    """lens[0] = S; B >= 3: lens[1] = 0 (every key masked), lens[2] = 1; one
    length past S where an utterance is left for it (B = 2, 5)."""
    g = torch.Generator().manual_seed(B * 1000 + S)
    ids = torch.randint(0, 42, (B, S), generator=g)
    lens = torch.randint(0, S + 1, (B,), generator=g)
    lens[0] = S
    if B >= 3:
        lens[1] = 0
        lens[2] = 1
    if B == 2 or B > 3:
        lens[B - 2 if B > 3 else 1] = S + 2
    return ids, lens


@functools.lru_cache(maxsize=None)
def enc_refs(mid, B, S, with_lens):
    ids, lens = enc_inputs(B, S)
    lens = lens if with_lens else None
    cfg = oracle_cfg(mid)
    r64, mask = orc.text_encoder(state64(mid, False), cfg, ids, lens)
    r32, _ = orc.text_encoder(state(mid, False), cfg, ids, lens)
    return r64, r32, mask


@functools.lru_cache(maxsize=None)
def dec_refs(mid, B, T):
    cfg = oracle_cfg(mid)
    x = torch.randn(B, T, cfg.hidden_dim, generator=torch.Generator().manual_seed(7 * T + B))
    return x, orc.mel_decoder(state64(mid, False), cfg, x.double()), orc.mel_decoder(state(mid, False), cfg, x)


def run_encoder(m, gpu, B, S, with_lens):
    ids, lens = enc_inputs(B, S)
    return m.text_encoder(ids.to(gpu), lens.to(gpu) if with_lens else None)


def encoder_case(m, gpu, mid, B, S, tag):
    outs = []
    for with_lens in (True, False):
        enc, mask = run_encoder(m, gpu, B, S, with_lens)
        r64, r32, ref_mask = enc_refs(mid, B, S, with_lens)
        check("encoder", f"{tag} B{B} S{S} lens{int(with_lens)}", enc, r64, r32)
        if with_lens:
            assert torch.equal(mask.cpu(), ref_mask)
        else:
            assert mask is None
        outs.append(enc.clone())
    return outs


def decoder_case(m, gpu, mid, B, T, tag, family="decoder"):
    x, r64, r32 = dec_refs(mid, B, T)
    mel = m.decoder(x.to(gpu))
    check(family, f"{tag} B{B} T{T}", mel, r64, r32)
    return mel.clone()


# ---------------------------------------------------------------- 1, 2, 4: edges, in every form
@pytest.mark.parametrize("B,S", ENC_SHAPES)
@pytest.mark.parametrize("mid,form", model_forms(EDGE_MODELS))
def test_text_encoder_edges(gpu, zoo, monkeypatch, mid, form, B, S):
    m = zoo(mid)
    base = None
    if form != "default":
        assert_form(m, gpu, set_form(monkeypatch, mid, "default"), stacks=(0,))
        base = [run_encoder(m, gpu, B, S, w)[0].clone() for w in (True, False)]
    assert_form(m, gpu, set_form(monkeypatch, mid, form), stacks=(0,))
    outs = encoder_case(m, gpu, mid, B, S, f"{mid}/{form}")
    if base is not None:
        for a, b in zip(outs, base):
            assert torch.equal(a, b), f"{form} differs from the default form by {maxabs(a, b):.3e}"


@pytest.mark.parametrize("B,T", DEC_SHAPES)
@pytest.mark.parametrize("mid,form", model_forms(EDGE_MODELS))
def test_mel_decoder_edges(gpu, zoo, monkeypatch, mid, form, B, T):
    m = zoo(mid)
    base = None
    if form != "default":
        assert_form(m, gpu, set_form(monkeypatch, mid, "default"), stacks=(1,))
        base = m.decoder(dec_refs(mid, B, T)[0].to(gpu)).clone()
    assert_form(m, gpu, set_form(monkeypatch, mid, form), stacks=(1,))
    mel = decoder_case(m, gpu, mid, B, T, f"{mid}/{form}")
    if base is not None:
        assert torch.equal(mel, base), f"{form} differs from the default form by {maxabs(mel, base):.3e}"


# ---------------------------------------------------------------- 3: the expanded first launch (SRC_EXPAND)
EXP_B, EXP_S, EXP_LENS = 3, 7, (7, 3, 1)
# a predicted duration times the scale stays this far from an integer: 10 x the
# duration bar (FLOOR), so no frame count can flip on the GPU's rounding
EXP_MARGIN = 10 * FLOOR


@functools.lru_cache(maxsize=None)
def expand_case(mid, want_multiple):
    """(ids, lens, scale, ref mel, ref audio): the duration scale is picked from
    the oracle's own durations so that T_max % 32 is 0 (want_multiple) or not,
    and every scaled duration sits EXP_MARGIN from an integer, in float32 and
    float64 alike.  With every duration pinned near 5.5 the seven phonemes of
    an utterance get the same count k, and 7 k is a multiple of 32 first at
    k = 32: T_max = 224 at a scale near 5.9, the decoder's 672 rows."""
    cfg, sd = oracle_cfg(mid), state(mid, True)
    ids = torch.randint(0, 42, (EXP_B, EXP_S), generator=torch.Generator().manual_seed(77))
    lens = torch.tensor(EXP_LENS)
    with torch.no_grad():
        enc, _ = orc.text_encoder(sd, cfg, ids, lens)
        dur = orc.duration_predictor(sd, enc).double()
    best = None
    for k in range(200, 6501):
        scale = k / 1000.0
        d = dur * float(torch.tensor(scale, dtype=torch.float32))  # the library takes the scale as a float
        margin = float((d - d.round()).abs().min())
        tmax = int(torch.trunc(d).sum(1).max())
        if margin >= EXP_MARGIN and tmax >= 1 and (tmax % 32 == 0) == want_multiple:
            if want_multiple and (best is None or margin > best[0]):
                best = (margin, scale, tmax)
            elif not want_multiple and (best is None or abs(scale - 1.0) < abs(best[1] - 1.0)):
                best = (margin, scale, tmax)
    assert best is not None, (mid, want_multiple)
    scale = best[1]
    ref_mel, ref_audio = orc.inference(sd, cfg, ids, lens, duration_scale=scale, as_written=False)
    assert ref_mel.shape[1] == best[2]
    return ids, lens, scale, ref_mel, ref_audio


def run_expand(m, hm, gpu, case):
    from m2amd import ops
    ids, lens, scale = case[0].to(gpu), case[1].to(gpu), case[2]
    mel, audio = m.inference(ids, lens, duration_scale=scale)
    enc, _ = hm.text_encoder(ids, lens)
    smel = hm.decoder(ops.regulate(enc, hm.duration(enc), None, scale=scale))
    return mel.clone(), audio.clone(), smel.clone()


@pytest.mark.parametrize("multiple", [False, True], ids=["odd", "x32"])
@pytest.mark.parametrize("mid,form", model_forms(["c", "e", "s1", "s2"]))
def test_expanded_inference(gpu, zoo, monkeypatch, mid, form, multiple):
    """inference (the frame expansion inside the first LN1 -> QKV launch) and
    the staged path (lr_expand, then SRC_X): both against the oracle, their
    mels bit-identical."""
    case = expand_case(mid, multiple)
    m = zoo(mid, pinned=True)
    base = None
    if form != "default":
        hm = assert_form(m, gpu, set_form(monkeypatch, mid, "default"))
        base = run_expand(m, hm, gpu, case)
    hm = assert_form(m, gpu, set_form(monkeypatch, mid, form))
    mel, audio, smel = run_expand(m, hm, gpu, case)
    ref_mel, ref_audio = case[3], case[4]
    assert mel.shape == ref_mel.shape, (mel.shape, ref_mel.shape, case[2])
    err, arms = maxabs(mel, ref_mel), rms(audio, ref_audio)
    print(f"TF3L expanded {mid}/{form} T{mel.shape[1]} scale {case[2]} err {err:.3e} bar {MEL_MAXABS_TOL:.3e} "
          f"ratio {err / MEL_MAXABS_TOL:.3f} audio_rms {arms:.3e} ratio {arms / AUDIO_RMS_TOL:.3f}")
    assert err <= MEL_MAXABS_TOL
    assert arms <= AUDIO_RMS_TOL
    assert torch.equal(mel, smel), f"inference and the staged path differ by {maxabs(mel, smel):.3e}"
    if base is not None:
        assert torch.equal(mel, base[0]) and torch.equal(audio, base[1]) and torch.equal(smel, base[2])


# ---------------------------------------------------------------- 5: hidden 128 and 32 through the duration kernel
@pytest.mark.parametrize("S", [1, 13, 14, 15, 29, 30, 31])
@pytest.mark.parametrize("mid", ["h", "i", "a"])
def test_duration_hidden_128_and_32(gpu, zoo, monkeypatch, mid, S):
    """duration_kernel<128> / <32> on both sides of the 14- and 30-phoneme
    tiles, against the oracle on the GPU's own encoder output; the one- and
    two-row-block tiles bit-identical.  Unpinned weights: the projection is
    not scaled down, so the convs' error shows in full."""
    m = zoo(mid)
    assert_form(m, gpu, set_form(monkeypatch, mid, "default"))
    g = torch.Generator().manual_seed(100 * S + 2)
    ids = torch.randint(0, 42, (2, S), generator=g)
    lens = torch.tensor([S, max(1, S // 2)])
    out = {}
    for rb in ("1", "2"):
        monkeypatch.setenv("M2_DUR_RB", rb)
        with torch.no_grad():
            r = m(ids.to(gpu), lens.to(gpu))
        out[rb] = (r["duration_pred"].clone(), r["encoder_output"].clone())
    assert torch.equal(out["1"][0], out["2"][0]) and torch.equal(out["1"][1], out["2"][1])
    enc = out["1"][1].cpu()
    r64 = orc.duration_predictor(state64(mid, False), enc.double())
    r32 = orc.duration_predictor(state(mid, False), enc)
    check("duration", f"{mid} S{S}", out["1"][0], r64, r32)
    e64, e32, _ = enc_refs_for(mid, ids, lens)
    check("duration-encoder", f"{mid} S{S}", out["1"][1], e64, e32)


def enc_refs_for(mid, ids, lens):
    cfg = oracle_cfg(mid)
    r64, mask = orc.text_encoder(state64(mid, False), cfg, ids, lens)
    return r64, orc.text_encoder(state(mid, False), cfg, ids, lens)[0], mask


# ---------------------------------------------------------------- 5, 6: whole inference off the stage shapes
@pytest.mark.parametrize("mid", ["h", "i", "a", "j", "k", "l"])
def test_inference_off_stage_shapes(gpu, zoo, monkeypatch, mid):
    from m2amd import _lib
    m = zoo(mid, pinned=True)
    hm = assert_form(m, gpu, set_form(monkeypatch, mid, "default"))
    assert _lib.load().m2_transformer_path(hm.handle) == TPATH.get(mid, 1)
    ids = torch.randint(0, 42, (2, 9), generator=torch.Generator().manual_seed(9))
    lens = torch.tensor([9, 5])
    mel, audio = m.inference(ids.to(gpu), lens.to(gpu))
    ref_mel, ref_audio = orc.inference(state(mid, True), oracle_cfg(mid), ids, lens, as_written=False)
    assert mel.shape == ref_mel.shape
    err, arms = maxabs(mel, ref_mel), rms(audio, ref_audio)
    print(f"TF3L inference {mid} err {err:.3e} bar {MEL_MAXABS_TOL:.3e} ratio {err / MEL_MAXABS_TOL:.3f} "
          f"audio_rms {arms:.3e} ratio {arms / AUDIO_RMS_TOL:.3f}")
    assert err <= MEL_MAXABS_TOL
    assert arms <= AUDIO_RMS_TOL


# ---------------------------------------------------------------- 6: mel widths without an ln_gemm instance, hidden 128
@pytest.mark.parametrize("B,N", [(3, 11), (2, 33)])
@pytest.mark.parametrize("mid", ["j", "k", "l", "h", "i"])
def test_unlisted_mel_widths_and_hidden_128(gpu, zoo, monkeypatch, mid, B, N):
    """A fused handle whose mel width has no ln_gemm / post_attn instance
    (j: one-launch driver, k: three-launch driver) keeps its fused layers and
    projects through the fp32 linear; l (mel 40) and hidden 128 run the fp32
    path.  Encoder and decoder at the edge shapes, under the same bar."""
    from m2amd import _lib
    m = zoo(mid)
    hm = assert_form(m, gpu, set_form(monkeypatch, mid, "default"))
    assert _lib.load().m2_transformer_path(hm.handle) == TPATH.get(mid, 1)
    family = "unlisted-mel" if mid in "jkl" else "hidden-128"
    for with_lens in (True, False):
        enc, mask = run_encoder(m, gpu, B, N, with_lens)
        r64, r32, ref_mask = enc_refs(mid, B, N, with_lens)
        check(family, f"{mid} enc B{B} S{N} lens{int(with_lens)}", enc, r64, r32)
        if with_lens:
            assert torch.equal(mask.cpu(), ref_mask)
    decoder_case(m, gpu, mid, B, N, f"{mid} dec", family=family)
