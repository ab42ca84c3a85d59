"""M2_HEADMID (the stage1 vocoder's head and mid as one launch or two) takes 0
or 1; anything else is an error named at handle creation, as M2_RANGE_POLICY's
bad values are."""
import pytest


def test_headmid_switch_values(monkeypatch):
    from m2amd.runtime import headmid_switch
    monkeypatch.delenv("M2_HEADMID", raising=False)
    assert headmid_switch() is True
    monkeypatch.setenv("M2_HEADMID", "0")
    assert headmid_switch() is False
    monkeypatch.setenv("M2_HEADMID", "1")
    assert headmid_switch() is True
    for bad in ("2", "on", "01", "-1"):
        monkeypatch.setenv("M2_HEADMID", bad)
        with pytest.raises(ValueError, match="M2_HEADMID"):
            headmid_switch()
