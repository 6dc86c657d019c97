"""routecheck.assert_guarded, the one comparison behind every guarded-buffer check of the device-route cases, fails on each defect it is
there to find: planted one at a time into a buffer it accepts (numpy only)."""
import numpy as np
import pytest

from routecheck import assert_guarded

GUARD = 0xA5A5A5A5
HELD, SLACK = 37, 8


def clean():
    """(buffer, expected records, written offsets, expected offsets): HELD records of a list query and SLACK guard rows behind them"""
    want = np.random.default_rng(3).integers(0, 1 << 32, (HELD, 4), dtype=np.uint64).astype(np.uint32)
    got = np.full((HELD + SLACK, 4), GUARD, np.uint32)
    got[:HELD] = want
    off = np.arange(0, HELD + 1, dtype=np.int64)
    return got, want, off.copy(), off


def test_the_clean_buffer_passes():
    got, want, off, want_off = clean()
    assert_guarded(got, want, GUARD, offsets=(off, want_off))
    assert_guarded(got, want, GUARD)
    assert_guarded(got[HELD:], want[:0], GUARD)           # capacity 0: nothing but the guard


def plant(got, off, defect):
    if defect == "a record at index held":
        got[HELD] = 7
    elif defect == "one word of the last guard row":
        got[-1, 3] ^= 1
    elif defect == "one word inside the prefix":
        got[HELD // 2, 2] ^= 0x80000000
    elif defect == "one offset":
        off[5] += 1


@pytest.mark.parametrize("defect", ["a record at index held", "one word of the last guard row", "one word inside the prefix", "one offset"])
def test_each_planted_defect_is_found(defect):
    got, want, off, want_off = clean()
    plant(got, off, defect)
    with pytest.raises(AssertionError):
        assert_guarded(got, want, GUARD, offsets=(off, want_off))
