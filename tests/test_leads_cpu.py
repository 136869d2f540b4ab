"""beat.ecg.LeadRecorder without a device: which column belongs to which electrode (signal, leads12), how full buffers kept on
the host and the rows still on the device are put together (values, len), and what it refuses before it touches a device."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def _stubbed(names, done, on_device):
    """A recorder that was never constructed on a device: ``done`` are the host copies of full buffers, ``on_device`` is what a
    read-back of the rows still in the device buffer returns."""
    from beat.ecg import LeadRecorder

    rec = object.__new__(LeadRecorder)
    rec.names = tuple(names)
    rec.nleads = len(rec.names)
    rec._done = [np.array(a, dtype=np.float64) for a in done]
    rec._rows = len(on_device)
    rec._read = lambda: np.array(on_device, dtype=np.float64).reshape(len(on_device), rec.nleads)
    return rec


def test_columns_follow_the_electrodes():
    from beat.ecg import Leads12

    names = ("V2", "LL", "RA", "apex", "LA", "V1")
    rows = np.arange(5 * 6, dtype=np.float64).reshape(5, 6) ** 1.5
    rec = _stubbed(names, [rows[:2], rows[2:4]], rows[4:])
    assert len(rec) == 5
    np.testing.assert_array_equal(rec.values(), rows)
    for col, name in enumerate(names):
        np.testing.assert_array_equal(rec.signal(name), rows[:, col])
    with pytest.raises(KeyError):
        rec.signal("V3")
    l12 = rec.leads12()
    assert isinstance(l12, Leads12)
    assert l12.RL is None and l12.V3 is None and l12.V6 is None
    np.testing.assert_array_equal(l12.RA, rows[:, 2])
    np.testing.assert_array_equal(l12.LA, rows[:, 4])
    np.testing.assert_array_equal(l12.LL, rows[:, 1])
    np.testing.assert_array_equal(l12.V1, rows[:, 5])
    np.testing.assert_array_equal(l12.V2, rows[:, 0])
    np.testing.assert_array_equal(l12.I, rows[:, 4] - rows[:, 2])
    np.testing.assert_array_equal(l12.II, rows[:, 1] - rows[:, 2])
    np.testing.assert_array_equal(l12.V1_, rows[:, 5] - (rows[:, 2] + rows[:, 4] + rows[:, 1]) / 3.0)
    with pytest.raises(AttributeError):
        l12.V3_


def test_nothing_recorded_and_nothing_on_the_device():
    rec = _stubbed(("RA", "LA", "LL"), [], [])
    assert len(rec) == 0 and rec.values().shape == (0, 3) and rec.signal("LA").shape == (0,)
    full = _stubbed(("RA", "LA", "LL"), [np.ones((4, 3))], [])  # a buffer that has just been read back: no second read
    full._read = None
    assert len(full) == 4 and full.values().shape == (4, 3)


def test_leads12_needs_the_limb_electrodes():
    rec = _stubbed(("RA", "LA", "V1"), [], [[1.0, 2.0, 3.0]])
    with pytest.raises(KeyError, match="LL"):
        rec.leads12()


def test_lead_limit_is_one_number():
    """BEAT_MAX_LEADS of the header, beat._hip.MAX_LEADS, and the class is exported from the package."""
    import beat
    from beat import _hip

    text = (ROOT / "include" / "beat_hip.h").read_text()
    assert int(re.search(r"#define\s+BEAT_MAX_LEADS\s+(\d+)", text).group(1)) == _hip.MAX_LEADS == 16
    assert beat.LeadRecorder is beat.ecg.LeadRecorder and "LeadRecorder" in beat.__all__
