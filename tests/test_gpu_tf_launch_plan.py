"""GPU: the transformer stacks' launch plan (csrc/transformer_plan.h) is what a
text-encoder or mel-decoder forward launches.  m2_debug_transformer_plan
prints the plan of a call as one line; the cases parse it and hold it against
what the library answers elsewhere (m2_debug_transformer_form,
m2_mel_decoder_ragged, m2_inference_dev_supported), then run the planned call
in every form against the float64 oracle - a smoke check that the executor
runs every form end to end; the edge shapes stay with test_gpu_tf_layer.py
and test_gpu_tf_three_launch.py.

Models: the two stage models on golden weights and five geometries of
test_gpu_tf_three_launch.py's GEOM under its seeds rule (seed 1000 + the
index of the id among 'a'..'l'): a chained, g zero layers, h fp32 layers,
j one-launch layers without a fused projection, k the same mel width on the
three-launch layers.

Numerics bar: test_gpu_tf_three_launch.py's, from the reference alone:
max(2e-5, 8 x e32), e32 = max|oracle in float32 - oracle in float64|.

Row count of a form (L layers; the encoder's call builds its rows from the
embedding, the decoder's takes them as given and ends with the projection):
  3: 1 + L, + 1 ending when the decoder's last layer did not project
  2: L > 0: 1 + 2 L (+ 1 ending); L = 0: embed_pe (encoder), the ending (decoder)
  1: 3 L, + embed_pe (encoder), + the ending (decoder)
  0: 5 L, + embed_pe (encoder), + the ending (decoder)
"""
import ctypes
import functools
import re

import pytest
import torch

import m2tts_oracle as orc
from conftest import golden_state, maxabs, stage_config

pytestmark = pytest.mark.gpu

FLOOR = 2e-5
FACTOR = 8.0

# id: hidden, heads, mel, encoder layers, decoder layers (test_gpu_tf_three_launch.py's GEOM)
GEOM = {
    "a": (32, 1, 64, 2, 2),
    "g": (64, 4, 64, 0, 0),
    "h": (128, 2, 80, 1, 1),
    "j": (64, 2, 48, 1, 1),
    "k": (64, 4, 48, 1, 1),
}
STAGE_IDS = ("s1", "s2")
MODELS = ["a", "g", "h", "j", "k", "s1", "s2"]
SWITCHES = {"default": {}, "l0": {"M2_TF_LAYER": "0"}, "c0": {"M2_TF_CHAIN": "0"},
            "l0c0": {"M2_TF_LAYER": "0", "M2_TF_CHAIN": "0"}}
ENC = (2, 33)  # B, S, with lengths
DEC = (3, 21)  # B, T


def oracle_cfg(mid):
    if mid in STAGE_IDS:
        return stage_config(mid)
    h, heads, mel, le, ld = GEOM[mid]
    return orc.OracleConfig(vocab_size=50, hidden_dim=h, mel_channels=mel, text_encoder_layers=le, decoder_layers=ld,
                            num_heads=heads, vocoder_channels=64)


@functools.lru_cache(maxsize=None)
def state(mid):
    if mid in STAGE_IDS:
        return golden_state(mid)
    from models.tts_model import M2TTSModel
    seed = 1000 + ord(mid) - ord("a")
    torch.manual_seed(seed)
    sd = {k: v.detach().clone() for k, v in M2TTSModel(**oracle_cfg(mid).as_dict()).state_dict().items()}
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
    return sd


@functools.lru_cache(maxsize=None)
def state64(mid):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in state(mid).items()}


@pytest.fixture(scope="module")
def zoo(gpu):
    from models.tts_model import M2TTSModel
    built = {}
    for mid in MODELS:
        m = M2TTSModel(**oracle_cfg(mid).as_dict())
        m.load_state_dict(state(mid))
        built[mid] = m.to(gpu).eval()
    return built


def lib():
    from m2amd import _lib
    return _lib.load()


def set_switches(monkeypatch, env):
    for name in ("M2_TF_LAYER", "M2_TF_CHAIN", "M2_TF_WAVES", "M2_TFL_RB", "M2_TFL_QS2"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


# ---------------------------------------------------------------- the line
def plan_line(hm, stack, B, N, masked=False, source=0, device_T=False, ragged=False):
    buf = ctypes.create_string_buffer(4096)
    n = lib().m2_debug_transformer_plan(hm.handle, stack, B, N, int(masked), source, int(device_T), int(ragged), buf, 4096)
    assert 0 < n < 4096, n
    line = buf.value.decode()
    assert len(line) == n
    return line


def parse(line):
    """{'stack': 'dec', 'form': 3, ..., 'error': None | text, 'rows': [(kind, layer, {field: int})]}"""
    tok = line.split(" ", 12)
    out = {"stack": tok[0], "error": None, "rows": []}
    for kv in tok[1:12]:
        k, v = kv.split("=")
        out[k] = v if k == "src" else int(v)
    rest = tok[12] if len(tok) > 12 else ""
    if rest.startswith('error="'):
        assert rest.endswith('"')
        out["error"] = rest[len('error="'):-1]
        return out
    for item in re.findall(r'[^\s\[]+(?:\[[^\]]*\])?', rest):
        kind, layer, inner = re.fullmatch(r'([a-z_]+?)(\d*)(?:\[([^\]]*)\])?', item).groups()
        fields = {k: int(v) for k, v in (kv.split("=") for kv in (inner or "").split())}
        out["rows"].append((kind, int(layer) if layer else None, fields))
    return out


def enc_line(hm, B=ENC[0], S=ENC[1]):
    return plan_line(hm, 0, B, S, masked=True, source=1)


def dec_line(hm, B=DEC[0], T=DEC[1], **kw):
    return plan_line(hm, 1, B, T, **kw)


def expected_rows(p):
    L, dec = p["layers"], p["stack"] == "dec"
    ending = 1 if dec and not p["projected"] else 0
    first = 0 if dec else 1  # the encoder's rows come from the embedding
    if p["form"] == 3:
        return 1 + L + ending
    if p["form"] == 2:
        return (1 + 2 * L if L else first) + ending
    return first + (3 if p["form"] == 1 else 5) * L + ending


@pytest.mark.parametrize("sw", list(SWITCHES))
@pytest.mark.parametrize("mid", MODELS)
def test_line_form_rows_projected(gpu, zoo, monkeypatch, mid, sw):
    set_switches(monkeypatch, SWITCHES[sw])
    hm = zoo[mid]._hip(gpu)
    for stack, line in ((0, enc_line(hm)), (1, dec_line(hm))):
        print(f"TFPLAN {mid}/{sw}: {line}")
        p = parse(line)
        assert p["error"] is None
        assert p["stack"] == ("dec" if stack else "enc")
        assert p["form"] == lib().m2_debug_transformer_form(hm.handle, stack)
        assert len(p["rows"]) == expected_rows(p), line
        kind, _, fields = p["rows"][-1]
        assert p["projected"] == int(fields.get("next") == 2), line
        if stack and not p["projected"]:
            assert kind in ("final_ln_gemm", "final_linear"), line
        assert not any(k.startswith("final_") for k, _, _ in p["rows"][:-1]), line
        if not stack:
            assert not p["projected"] and not kind.startswith("final_"), line


def strip(line, names):
    return re.sub(r'\b(%s)=\d+' % "|".join(names), r'\1=*', line)


def field_values(line, name):
    return [int(v) for v in re.findall(r'\b%s=(\d+)' % name, line)]


# the switch, its field, its forced value, the fields that follow from it (grid = B x tiles of rb
# sixteen-row blocks; thr = 64 x waves)
FORCED = [("M2_TFL_RB", "rb", 2, ("grid",)), ("M2_TFL_QS2", "qs2", 3, ()), ("M2_TF_WAVES", "waves", 4, ("thr",))]


@pytest.mark.parametrize("name,field,value,derived", FORCED)
@pytest.mark.parametrize("mid", MODELS)
def test_forced_switch_changes_its_field_only(gpu, zoo, monkeypatch, mid, name, field, value, derived):
    hm = zoo[mid]._hip(gpu)
    set_switches(monkeypatch, {})
    base = [enc_line(hm), dec_line(hm)]
    set_switches(monkeypatch, {name: str(value)})
    forced = [enc_line(hm), dec_line(hm)]
    for b, f, (B, N) in zip(base, forced, (ENC, DEC)):
        print(f"TFPLAN {mid} {name}={value}: {f}")
        assert strip(b, (field,) + derived) == strip(f, (field,) + derived)
        assert all(v == value for v in field_values(f, field)), f
        for kind, _, fields in parse(f)["rows"]:
            if field == "rb" and "rb" in fields:
                npad = (N + 63) // 64 * 64
                assert fields["grid"] == B * -(-npad // (16 * fields["rb"])), f
            if field == "waves" and "waves" in fields:
                assert fields["thr"] == 64 * fields["waves"], f
        if not field_values(f, field):  # no row carries the field: the same line
            assert b == f


def test_ragged_error_is_the_plans(gpu, zoo, monkeypatch):
    from m2amd import _lib
    set_switches(monkeypatch, {})
    hm = zoo["k"]._hip(gpu)
    p = parse(dec_line(hm, ragged=True))
    assert p["error"] and not p["rows"]
    x = torch.zeros(DEC[0], DEC[1], GEOM["k"][0], device=gpu)
    with pytest.raises(_lib.M2Error) as e:
        hm.decoder_ragged(x, torch.tensor([21, 5, 1], dtype=torch.int32, device=gpu))
    assert e.value.status == _lib.M2_E_SHAPE
    assert p["error"] in str(e.value)
    # the one-launch layers take the same call
    assert parse(dec_line(zoo["j"]._hip(gpu), ragged=True))["error"] is None


@pytest.mark.parametrize("sw", ["default", "l0"])
def test_dev_supported_is_the_plans(gpu, zoo, monkeypatch, sw):
    set_switches(monkeypatch, SWITCHES[sw])
    hm = zoo["s1"]._hip(gpu)
    p = parse(dec_line(hm, B=2, T=40, source=2, device_T=True))
    assert bool(lib().m2_inference_dev_supported(hm.handle, 40)) == (p["error"] is None)
    assert (p["error"] is None) == (sw == "default")


# ---------------------------------------------------------------- the planned calls, run
def check(tag, out, ref64, ref32):
    e32 = maxabs(ref32, ref64)
    bar = max(FLOOR, FACTOR * e32)
    err = maxabs(out, ref64)
    print(f"TFPLAN {tag} err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} e32 {e32:.3e}")
    assert tuple(out.shape) == tuple(ref64.shape)
    assert err <= bar, (tag, err, bar, e32)


@functools.lru_cache(maxsize=None)
def enc_case(mid, B, S):
    g = torch.Generator().manual_seed(B * 1000 + S)
    ids = torch.randint(0, 42, (B, S), generator=g)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = S
    cfg = oracle_cfg(mid)
    r64, mask = orc.text_encoder(state64(mid), cfg, ids, lens)
    r32, _ = orc.text_encoder(state(mid), cfg, ids, lens)
    return ids, lens, r64, r32, mask


@functools.lru_cache(maxsize=None)
def dec_case(mid, B, T):
    cfg = oracle_cfg(mid)
    x = torch.randn(B, T, cfg.hidden_dim, generator=torch.Generator().manual_seed(7 * T + B))
    return x, orc.mel_decoder(state64(mid), cfg, x.double()), orc.mel_decoder(state(mid), cfg, x)


@pytest.mark.parametrize("sw", list(SWITCHES))
@pytest.mark.parametrize("mid", MODELS)
def test_planned_calls_against_the_oracle(gpu, zoo, monkeypatch, mid, sw):
    set_switches(monkeypatch, SWITCHES[sw])
    m = zoo[mid]
    ids, lens, r64, r32, ref_mask = enc_case(mid, *ENC)
    enc, mask = m.text_encoder(ids.to(gpu), lens.to(gpu))
    check(f"{mid}/{sw} encoder", enc, r64, r32)
    assert torch.equal(mask.cpu(), ref_mask)
    x, d64, d32 = dec_case(mid, *DEC)
    check(f"{mid}/{sw} decoder", m.decoder(x.to(gpu)), d64, d32)


# ---------------------------------------------------------------- the rb thresholds on stage1
@pytest.mark.parametrize("stack,B,N,rb", [(0, 16, 256, 1), (0, 17, 256, 2), (1, 64, 256, 4)])
def test_rb_thresholds(gpu, zoo, monkeypatch, stack, B, N, rb):
    """256 sixteen-row tiles keep rb 1, 272 take 2, 1024 take 4; the call meets
    the oracle under the bar above and is bit-equal to the one with that rb
    forced."""
    m = zoo["s1"]
    hm = m._hip(gpu)
    if stack:
        x, r64, r32 = dec_case("s1", B, N)
        run = lambda: m.decoder(x.to(gpu)).clone()
        line_of = lambda: dec_line(hm, B, N)
    else:
        ids, lens, r64, r32, _ = enc_case("s1", B, N)
        run = lambda: m.text_encoder(ids.to(gpu), lens.to(gpu))[0].clone()
        line_of = lambda: enc_line(hm, B, N)
    set_switches(monkeypatch, {})
    line = line_of()
    print(f"TFPLAN s1 rb: {line}")
    layer_rbs = [f["rb"] for k, _, f in parse(line)["rows"] if k == "tfl_layer"]
    assert layer_rbs and all(v == rb for v in layer_rbs), line
    out = run()
    check(f"s1 rb={rb} {'decoder' if stack else 'encoder'} B{B} N{N}", out, r64, r32)
    set_switches(monkeypatch, {"M2_TFL_RB": str(rb)})
    assert line_of() == line
    assert torch.equal(run(), out)


