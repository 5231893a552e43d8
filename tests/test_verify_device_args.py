"""The device verify entry points' argument handling (hge_verify.hip), which runs before
the device is touched: an empty batch is HGE_OK with empty outputs, descending offsets
and a key index outside [0, n_keys) are HGE_ERR_ARG.  No GPU needed."""
import numpy as np
import pytest

from babble_amd import engine

HGE_ERR_ARG = -8


def test_empty_batches_are_ok():
    assert engine.sha256_batch_device([]).shape == (0, 32)
    keys = np.zeros((2, 65), np.uint8)
    ok = engine.verify_digests_device(np.zeros((0, 32), np.uint8), keys, np.zeros(0, np.int32),
                                      np.zeros((0, 64), np.uint8))
    assert ok.shape == (0,) and ok.dtype == bool
    ok, hashes, ms = engine.verify_events_device([], keys, np.zeros(0, np.int32), np.zeros((0, 64), np.uint8))
    assert ok.shape == (0,) and hashes.shape == (0, 32) and ms == 0.0
    # no keys at all is still an empty batch
    ok, hashes, _ = engine.verify_events_device([], np.zeros((0, 65), np.uint8), np.zeros(0, np.int32),
                                                np.zeros((0, 64), np.uint8))
    assert len(ok) == 0 and len(hashes) == 0


def test_descending_offsets_are_refused():
    bad = (np.zeros(8, np.uint8), np.array([0, 5, 3], np.int64))
    with pytest.raises(engine.HgeError) as e:
        engine.sha256_batch_device(bad)
    assert e.value.code == HGE_ERR_ARG
    with pytest.raises(engine.HgeError) as e:
        engine.verify_events_device(bad, np.zeros((2, 65), np.uint8), np.zeros(2, np.int32),
                                    np.zeros((2, 64), np.uint8))
    assert e.value.code == HGE_ERR_ARG


@pytest.mark.parametrize("idx", [[0, 2], [-1, 0], [0, 1 << 20]])
def test_key_index_out_of_range_is_refused(idx):
    keys = np.zeros((2, 65), np.uint8)
    idx = np.array(idx, np.int32)
    with pytest.raises(engine.HgeError) as e:
        engine.verify_digests_device(np.zeros((2, 32), np.uint8), keys, idx, np.zeros((2, 64), np.uint8))
    assert e.value.code == HGE_ERR_ARG
    with pytest.raises(engine.HgeError) as e:
        engine.verify_events_device([b"ab", b"c"], keys, idx, np.zeros((2, 64), np.uint8))
    assert e.value.code == HGE_ERR_ARG
    # with no keys every index is out of range
    with pytest.raises(engine.HgeError) as e:
        engine.verify_digests_device(np.zeros((2, 32), np.uint8), np.zeros((0, 65), np.uint8),
                                     np.zeros(2, np.int32), np.zeros((2, 64), np.uint8))
    assert e.value.code == HGE_ERR_ARG
