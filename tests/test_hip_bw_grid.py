"""Butterworth band-pass (sosfiltfilt) on the device against the scipy oracle, bit-exact: orders 1..16 and 32 on narrow,
wide and non-default-fs bands, record lengths around the pad length, extreme values, several scratch batches in one
call, and per-channel groups that mix Butterworth orders with Savitzky-Golay."""

import numpy as np
import pytest

from oracle import wfa_oracle as O
from waveformanalysis_amd import _lib
from waveformanalysis_amd.device import DeviceSession
from waveformanalysis_amd.dtypes import RECORDS_DTYPE
from waveformanalysis_amd.filter_engine import MAX_BW_ORDER, design_bw
from waveformanalysis_amd.plugin_api import SimpleContext
from waveformanalysis_amd.plugins import HipWavePoolFilteredPlugin

pytestmark = pytest.mark.gpu

BANDS = {
    "narrow_low": (0.001, 0.004, 0.5),
    "wide": (0.01, 0.2499, 0.5),
    "fs250": (5.0, 60.0, 250.0),
}


def _records(lengths, gap=5, channels=None):
    rec = np.zeros(len(lengths), dtype=RECORDS_DTYPE)
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64) + gap)[:-1]]) if len(lengths) else []
    rec["record_id"] = np.arange(len(rec))
    rec["event_length"] = lengths
    rec["wave_offset"] = off
    rec["dt"] = 4
    if channels is not None:
        rec["channel"] = channels
    return rec, int(off[-1] + lengths[-1] + gap) if len(lengths) else 0


def _values(rec, n, seed):
    rng = np.random.default_rng(seed)
    pool = np.full(n, 777, dtype=np.uint16)  # gap samples: must not leak into the output
    for k, (o, L) in enumerate(zip(rec["wave_offset"], rec["event_length"])):
        t = np.arange(L)
        kind = k % 5
        if kind == 0:
            v = 8000 + rng.integers(-300, 301, L)
        elif kind == 1:
            v = np.where(t % 2 == 0, 0, 65535)
        elif kind == 2:
            v = np.full(L, 65535)
        elif kind == 3:
            v = np.zeros(L, dtype=np.int64)
        else:
            v = 8000 - np.maximum(0, 7000 - 700 * np.abs(t - L // 3))
        pool[o : o + L] = v
    return pool


def _case(order, band, seed=0):
    sos, zi, padlen = design_bw(*band, order)
    lengths = []
    for L in (padlen - 1, padlen, padlen + 1, padlen + 2, 3 * padlen + 17):
        lengths += [max(L, 1)] * 5
    rec, n = _records(lengths)
    return rec, _values(rec, n, seed + order), (sos, zi, padlen)


def _run(rec, pool, sos, zi, padlen):
    with DeviceSession(0) as s:
        s.upload_pool(pool)
        s.upload_records(rec)
        s.profile(True)
        got = s.sosfiltfilt(sos, zi, padlen)
        assert "k_sosfiltfilt" in s.profile_report()
    return got


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("order", list(range(1, 17)) + [MAX_BW_ORDER])
def test_orders_and_bands_bit_exact(order, band):
    rec, pool, (sos, zi, padlen) = _case(order, BANDS[band])
    assert sos.shape[0] == order
    want = O.filter_wave_pool(rec, pool, "BW", bw_sos=sos)
    got = _run(rec, pool, sos, zi, padlen)
    np.testing.assert_array_equal(got, want)
    short = rec["event_length"] <= padlen
    assert short.any() and (~short).any()


def test_order_above_the_limit_is_refused_before_any_launch():
    with pytest.raises(ValueError, match="exceeds the supported maximum 32"):
        design_bw(0.01, 0.2, 0.5, MAX_BW_ORDER + 1)
    rec, pool, (sos, zi, padlen) = _case(4, BANDS["wide"])
    big = np.tile(sos, (9, 1))[: MAX_BW_ORDER + 1]
    with DeviceSession(0) as s:
        s.upload_pool(pool)
        s.upload_records(rec)
        with pytest.raises(Exception, match="n_sections must be in"):
            s.sosfiltfilt(big, np.tile(zi, (9, 1))[: MAX_BW_ORDER + 1], padlen)
    ctx = SimpleContext({"filter_type": "BW", "lowcut": 0.01, "highcut": 0.2, "fs": 0.5, "filter_order": 33},
                        {"records": rec, "wave_pool": pool}, plugins=[HipWavePoolFilteredPlugin()])
    with pytest.raises(RuntimeError, match="exceeds the supported maximum") as err:  # the context wraps plugin errors
        ctx.get_data("run", "wave_pool_filtered")
    assert isinstance(err.value.__cause__, ValueError)


@pytest.mark.parametrize("order", [4, 12])
def test_several_scratch_batches(order):
    """One record of the longest supported length among 5300 short ones: the float64 forward scratch holds 2048 records
    per batch, so the call runs three launches and records of the later ones start at r_begin > 0.  This pins that
    every batch's records are filtered; it cannot detect a missing `- r_begin` in the scratch index: that shifts a
    later batch's records by whole scratch rows, still inside the allocation here, and changes no output."""
    sos, zi, padlen = design_bw(0.01, 0.2, 0.5, order)
    long_len = 130432  # WFA_MAX_RECORD_SAMPLES
    lengths = [60] * 1000 + [long_len] + [60 + (k % 50) for k in range(4300)]
    rec, n = _records(lengths)
    pool = _values(rec, n, 99)
    n_ext = long_len + 2 * padlen
    batch = (2**31 // (n_ext * 8)) // 256 * 256
    assert 3 <= -(-len(rec) // batch), batch
    want = O.filter_wave_pool(rec, pool, "BW", bw_sos=sos)
    got = _run(rec, pool, sos, zi, padlen)
    np.testing.assert_array_equal(got, want)


def test_plugin_groups_mix_orders_and_sg():
    """Per-channel settings: Butterworth orders 3, 9 and 16 and SG(15,4) in one wave_pool_filtered call.  Every group
    writes only its own records (filter_keep): samples between records stay 0."""
    lengths = [150 + (k * 37) % 400 for k in range(64)]
    channels = np.arange(64) % 4
    rec, n = _records(lengths, gap=9, channels=channels)
    pool = _values(rec, n, 5)
    cfg = {"0:1": {"filter_order": 9}, "0:2": {"filter_order": 16, "lowcut": 0.002, "highcut": 0.1},
           "0:3": {"filter_type": "SG", "sg_window_size": 15, "sg_poly_order": 4}}
    base = {"filter_type": "BW", "lowcut": 0.01, "highcut": 0.2, "fs": 0.5, "filter_order": 3}
    ctx = SimpleContext({**base, "channel_config": cfg}, {"records": rec, "wave_pool": pool},
                        plugins=[HipWavePoolFilteredPlugin()])
    got = ctx.get_data("run", "wave_pool_filtered")
    sos = {c: design_bw(v.get("lowcut", 0.01), v.get("highcut", 0.2), 0.5, v.get("filter_order", 3))[0]
           for c, v in [(0, {}), (1, cfg["0:1"]), (2, cfg["0:2"])]}

    def per_record(i):
        c = int(channels[i])
        if c == 3:
            return {"filter_type": "SG", "sg_window_size": 15, "sg_poly_order": 4}
        return {"filter_type": "BW", "bw_sos": sos[c]}

    want = O.filter_wave_pool(rec, pool, "BW", bw_sos=sos[0], per_record_cfg=per_record)
    inside = np.zeros(n, dtype=bool)
    for o, L in zip(rec["wave_offset"], rec["event_length"]):
        inside[o : o + L] = True
    assert not np.any(got[~inside])
    np.testing.assert_array_equal(got, want)


FIXTURES = ["sgbw_bw1", "sgbw_bw9", "sgbw_bw12"]


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixtures_bit_exact(name):
    """Butterworth orders 1, 9 and 12 through the reference's WavePoolFilteredPlugin / ThresholdHitPlugin
    (tests/golden/sgbw_bw*.npz): the filtered pool bit for bit, records not longer than padlen copied, and the hits on it,
    through the device session and through the plugin."""
    from tests import golden_util as G

    c = G.load_case(name)
    fp = G.filter_params(c)
    sos, zi, padlen = design_bw(fp["lowcut"], fp["highcut"], fp["fs"], fp["filter_order"])
    hp = G.hit_params(c)
    with DeviceSession(0) as s:
        s.upload_pool(c["wave_pool"])
        s.upload_records(c["records"], hp["thresholds"])
        np.testing.assert_array_equal(s.sosfiltfilt(sos, zi, padlen), c["wave_pool_filtered"])
        G.assert_struct_equal(s.threshold_hits(_lib.SRC_F32, hp["left_extension"], hp["right_extension"]),
                              c["hits_filt"], float_rtol=1e-6, what=name)
    ctx = SimpleContext({k: fp[k] for k in ("filter_type", "lowcut", "highcut", "fs", "filter_order")},
                        {"records": c["records"], "wave_pool": c["wave_pool"]}, plugins=[HipWavePoolFilteredPlugin()])
    np.testing.assert_array_equal(ctx.get_data("run", "wave_pool_filtered"), c["wave_pool_filtered"])
