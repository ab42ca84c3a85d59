"""GPU: the vocoder's launch plan (csrc/vocoder_launch.h) is what m2_vocoder
launches.  m2_debug_vocoder_plan prints the plan of a call as one line; each
case prints it, runs the call and checks the line against what the library can
observe of the launch: the fused head + mid launch counter
(m2_debug_headmid_launches) and the kernel names of the handle
(m2_profile_kernel_name_for).  A forced developer switch shows in the line and
changes nothing else in it.  Shapes: stage1 on either side of one, two and
three headmid strips (4T = 248, 252, 504), stage2 on either side of the 16- and
19-frame head windows.  The audio of every variant is compared bit for bit
elsewhere (test_gpu_headmid, test_gpu_tailp, test_gpu_tailp2,
test_gpu_head_comp, test_gpu_f32_forms).
"""
import ctypes
import re

import pytest
import torch

from conftest import golden_state, stage_config

pytestmark = pytest.mark.gpu

SLOT_NAMES = ["head16", "head19", "head24", "head27", "mid", "mid_alt", "tail", "tail_alt"]


def build(stage, gpu):
    from models.tts_model import M2TTSModel
    m = M2TTSModel(**stage_config(stage).as_dict())
    m.load_state_dict(golden_state(stage))
    return m.to(gpu).eval()


@pytest.fixture(scope="module")
def models(gpu):
    return {s: build(s, gpu) for s in ("s1", "s2")}


def lib():
    from m2amd import _lib
    return _lib.load()


def plan_line(hm, B, T, btm=False, device_T=False):
    buf = ctypes.create_string_buffer(1024)
    n = lib().m2_debug_vocoder_plan(hm.handle, B, T, int(btm), int(device_T), buf, 1024)
    assert 0 < n < 1024, n
    line = buf.value.decode()
    assert len(line) == n
    return line


def items(line):
    """{'path': 'split', 'stage': '1', 'headmid': {'n': '2', ...}, 'redo': 'none', ...}"""
    out = {"path": line.split()[0]}
    rest = line.split(" ", 1)[1] if " " in line else ""
    for name, inner in re.findall(r'(\w+)\[([^\]]*)\]', rest):
        if name != "guarded":
            out[name] = dict(kv.split("=") for kv in inner.split() if "=" in kv)
    flat = re.sub(r'\w+\[[^\]]*\]', "", rest)
    for key, quoted, plain in re.findall(r'([\w-]+)=(?:"([^"]*)"|(\S*))', flat):
        out[key] = quoted or plain
    if "redo=guarded[" in line:
        out["redo"] = "guarded"
    return out


def fused_launches():
    return int(lib().m2_debug_headmid_launches())


def kernel_names(hm):
    return [lib().m2_profile_kernel_name_for(hm.handle, i).decode().split()[0] for i in range(3)]


def run_and_check(model, gpu, stage, B, T, btm=False):
    """Prints the plan, runs the call, checks the plan against the launch; returns the parsed plan."""
    hm = model._hip(gpu)
    line = plan_line(hm, B, T, btm)
    print(f"{stage} B={B} T={T}: {line}")
    it = items(line)
    M = stage_config(stage).mel_channels
    mel = torch.randn(B, M, T, generator=torch.Generator().manual_seed(7 * T + B)).to(gpu)
    if btm:
        mel = mel.transpose(1, 2).contiguous()
    n0 = fused_launches()
    audio = hm.vocoder(mel, layout_btm=btm)
    torch.cuda.synchronize()
    n1 = fused_launches()
    assert audio.shape == (B, 1, 64 * T)
    assert it["path"] in ("split", "f32")
    assert ("headmid" in it) == (n1 == n0 + 1) and n1 - n0 in (0, 1), (line, n0, n1)
    names = kernel_names(hm)
    if it["path"] == "split":
        mid = "midp" if ("headmid" in it or "midp" in it) else "x3mid"
        assert mid in it or "headmid" in it
        assert names[1] == {"midp": "midp_kernel", "x3mid": "x3_mid_kernel"}[mid], (line, names)
        tail = [k for k in ("tailp", "tailp2", "x3tail") if k in it]
        assert len(tail) == 1
        assert names[2] == {"tailp": "tailp_kernel", "tailp2": "tailp2_kernel", "x3tail": "x3_tail_kernel"}[tail[0]]
        assert ("no-headmid" in it) == ("headmid" not in it)
    else:
        assert names == ["voc_head_kernel", "voc_mid_kernel", "voc_tail_kernel"]
    for k, v in it.items():  # every launch: a grid over the batch, threads in whole waves, LDS within a CU
        if isinstance(v, dict) and "grid" in v:
            gx, gy = map(int, v["grid"].split("x"))
            assert gx >= 1 and gy == B and int(v["thr"]) % 64 == 0 and 0 <= int(v["lds"]) <= 160 * 1024, line
    return it


def test_slots_printed(gpu, models):
    """The device's workgroup slots per tiling, as the plan's rules weigh them."""
    models["s2"]._hip(gpu)
    out = (ctypes.c_int64 * 8)()
    assert lib().m2_debug_vocoder_slots(out) == 0
    print("VocSlots: " + " ".join(f"{n}={v}" for n, v in zip(SLOT_NAMES, out)))
    assert all(v >= 1 for v in out)


@pytest.mark.parametrize("T", [1, 62, 63, 126])
@pytest.mark.parametrize("B", [1, 3])
def test_stage1_plan_is_the_launch(gpu, models, B, T):
    it = run_and_check(models["s1"], gpu, "s1", B, T, btm=bool(B & 2))
    assert it["stage"] == "1" and "headmid" in it and "tailp" in it
    hm = it["headmid"]
    n = {1: 1, 62: 1, 63: 2, 126: 3}[T]  # one strip up to 4T = 250 columns
    S = -(-4 * T // n)
    assert (int(hm["n"]), int(hm["S"]), int(hm["nch"])) == (n, S, -(-S // 16))
    assert hm["grid"] == f"{n}x{B}" and hm["trans"] == str(int(bool(B & 2)))
    tp = it["tailp"]
    assert tp["nl"] == "6" and int(tp["grid"].split("x")[0]) == -(-T // int(tp["nch"]))


@pytest.mark.parametrize("T", [1, 16, 17, 19, 20, 37])
@pytest.mark.parametrize("B", [1, 3])
def test_stage2_plan_is_the_launch(gpu, models, B, T):
    it = run_and_check(models["s2"], gpu, "s2", B, T)
    assert it["stage"] == "2" and "headmid" not in it and it["no-headmid"] == "not the stage1 shapes"
    head = it["head"]
    # small grids: one round of slots either way, so the smaller (16-frame) window
    assert head["tf"] == "16" and head["comp"] == "1" and head["grid"] == f"{-(-T // 16)}x{B}"
    assert "x3mid" in it and "tailp2" in it
    w = int(it["x3mid"]["w"])
    assert w in (30, 33) and it["x3mid"]["alt"] == str(int(w == 33))
    assert it["x3mid"]["grid"] == f"{-(-4 * T // w)}x{B}"
    assert int(it["tailp2"]["grid"].split("x")[0]) == -(-T // int(it["tailp2"]["nch"]))


def forced(models, gpu, monkeypatch, stage, B, T, env, changed):
    """The plan with the switches of env set: only the items named in `changed` differ from the default's."""
    base = run_and_check(models[stage], gpu, stage, B, T)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    it = run_and_check(models[stage], gpu, stage, B, T)
    for k in env:
        monkeypatch.delenv(k)
    diff = {k for k in set(base) | set(it) if base.get(k) != it.get(k)}
    assert diff == set(changed), (diff, base, it)
    return base, it


def test_forced_headmid_off(gpu, models, monkeypatch):
    base, it = forced(models, gpu, monkeypatch, "s1", 3, 63, {"M2_HEADMID": "0"}, {"headmid", "head", "midp", "no-headmid"})
    assert it["no-headmid"] == "M2_HEADMID=0" and it["head"]["comp"] == "1"


def test_forced_midp_nch(gpu, models, monkeypatch):
    base, it = forced(models, gpu, monkeypatch, "s1", 3, 63, {"M2_MIDP_NCH": "5"}, {"headmid", "head", "midp", "no-headmid"})
    assert it["midp"]["nch"] == "5" and it["midp"]["grid"] == f"{-(-4 * 63 // 80)}x3"
    assert it["no-headmid"].startswith("M2_MIDP_NCH")


def test_forced_tailp(gpu, models, monkeypatch):
    base, it = forced(models, gpu, monkeypatch, "s1", 3, 63, {"M2_TAILP_NCH": "9"}, {"tailp"})
    assert it["tailp"]["nch"] == "9" and it["tailp"]["grid"] == "7x3" and it["tailp"]["nl"] == "6"
    base, it = forced(models, gpu, monkeypatch, "s1", 3, 63, {"M2_TAILP_SEVEN": "1"}, {"tailp"})
    assert it["tailp"]["nl"] == "7" and base["tailp"]["nl"] == "6" and it["tailp"]["thr"] == str(8 * 64)


def test_forced_tailp2(gpu, models, monkeypatch):
    base, it = forced(models, gpu, monkeypatch, "s2", 3, 37, {"M2_TAILP2_NCH": "9"}, {"tailp2"})
    assert it["tailp2"]["nch"] == "9" and it["tailp2"]["grid"] == "5x3" and it["tailp2"]["nl"] == "6"
    base, it = forced(models, gpu, monkeypatch, "s2", 3, 37, {"M2_TAILP2_SEVEN": "1"}, {"tailp2"})
    assert it["tailp2"]["nl"] == "7" and it["tailp2"]["thr"] == str(14 * 64)


@pytest.mark.parametrize("tf", [19, 24, 27])
def test_forced_s2_head_window(gpu, models, monkeypatch, tf):
    base, it = forced(models, gpu, monkeypatch, "s2", 3, 37, {"M2_S2_HEAD_TF": str(tf)}, {"head"})
    assert it["head"]["tf"] == str(tf) and it["head"]["grid"] == f"{-(-37 // tf)}x3"
    assert it["head"]["thr"] == str((8 if tf == 19 else 16) * 64)


def test_forced_s2_mid_window(gpu, models, monkeypatch):
    base = items(plan_line(models["s2"]._hip(gpu), 3, 37))
    for alt in ("0", "1"):
        changed = set() if base["x3mid"]["alt"] == alt else {"x3mid"}
        _, it = forced(models, gpu, monkeypatch, "s2", 3, 37, {"M2_S2_MID_ALT": alt}, changed)
        assert it["x3mid"]["alt"] == alt and it["x3mid"]["w"] == {"0": "30", "1": "33"}[alt]


def test_forced_head_inconv(gpu, models, monkeypatch):
    base, it = forced(models, gpu, monkeypatch, "s1", 3, 63, {"M2_HEAD_INCONV": "1"}, {"headmid", "head", "midp", "no-headmid"})
    assert it["head"]["comp"] == "0" and it["head"]["tf"] == "63" and "M2_HEAD_INCONV" in it["no-headmid"]
    base, it = forced(models, gpu, monkeypatch, "s2", 3, 37, {"M2_HEAD_INCONV": "1"}, {"head"})
    assert it["head"]["comp"] == "0" and it["head"]["tf"] == "16"


def test_forced_exact_f32_forms(gpu, monkeypatch):
    """M2_VOC_F32=1 (read when the handle is created) with each M2_F32_MT: the form's name, and the
    mid / tail windows it stands for (half windows: 63 / 250 positions)."""
    monkeypatch.setenv("M2_VOC_F32", "1")
    model = build("s1", gpu)
    hm = model._hip(gpu)
    want = {0: (125, 500), 1: (63, 500), 2: (125, 250), 3: (63, 250), 4: (125, 250)}
    # B = 3, T = 64: 6 windows of the 16-wave head waste no more of their round than 9 of the 8-wave one
    for mt, (w2, w3) in want.items():
        monkeypatch.setenv("M2_F32_MT", str(mt))
        it = run_and_check(model, gpu, "s1", 3, 64)
        assert it["path"] == "f32" and it["form"] == f"S1_W16_MT{mt}" and it["redo"] == "none"
        assert it["head"]["tf"] == "63" and it["mid"]["w"] == str(w2) and it["tail"]["w"] == str(w3)
        assert it["mid"]["grid"] == f"{-(-4 * 64 // w2)}x3" and it["tail"]["grid"] == f"{-(-16 * 64 // w3)}x3"
    monkeypatch.delenv("M2_F32_MT")
    assert hm is model._hip(gpu)
