"""Round trip over the engine's options: every key that can be read is set and read back, inside its range and past both ends.  The expected
values are written out from the rules of the set_option / get_option chains that the option table (engine.cpp, find_option) replaced."""
import pytest

from conftest import model_path

pytestmark = pytest.mark.gpu

BIG = 10 ** 6


@pytest.fixture(scope="module")
def gpu(mi):
    if mi.device_count() < 1:
        pytest.fail("no HIP device: the GPU suite must run on an MI355X box")
    return mi


def _clamp(lo, hi, mid):
    return [(lo - 3, lo), (hi + 3, hi), (mid, mid), (lo, lo), (hi, hi)]


_BOOL = [(0, 0), (5, 1), (-3, 1), (1, 1), (0, 0)]

# key: (default, [(value set, value read back), ...])
READ_WRITE = {
    "chunk": (0, [(-5, 0), (7, 7), (BIG, BIG), (0, 0)]),                 # max(0, value)
    "graph": (1, _BOOL),
    "fuse": (5, _clamp(0, 5, 3)),
    "res_budget": (156, _clamp(16, 156, 64)),                            # KiB on both sides, bytes inside
    "pipe": (4, _clamp(0, 4, 2)),
    "small_chain": (16, _clamp(0, 64, 8)),
    "pipe_rows": (0, [(1, 1), (2, 2), (4, 4), (3, 0), (5, 0), (-1, 0), (0, 0), (36, 0), (BIG, 0)]),   # 1, 2 or 4, else 0
    "pipe_band": (0, _clamp(0, 4096, 16)),
    "strip": (1, _BOOL),
    "stem_fuse": (1, _BOOL),
    "stem_mfma": (1, _BOOL),
    "pair_fuse": (1, _BOOL),
    "mdb_band": (0, _clamp(0, 4096, 12)),
    "mchain": (1, _BOOL),
    "tail": (1, _BOOL),
    "tail_pre": (0, _clamp(0, 2, 1)),
    "tail_g": (0, _clamp(0, 64, 5)),
    "band": (1, _clamp(0, 2, 1)),
    "band_fork": (1, _BOOL),
    "band_wide": (1, _BOOL),
    "band_nw": (128, _clamp(8, 256, 64)),
    "fork": (1, _BOOL),
    "heads": (1, _clamp(1, 4, 2)),
    "reuse": (1, _BOOL),
    "lanes": (1, _clamp(1, 4, 2)),
    "test_poison": (0, [(1, 1), (2, 2), (3, 0), (-1, 0), (0, 0), (33, 0)]),   # 1 or 2, else 0
}
READ_ONLY = {"band_fail_streak": 0, "band_wraps": 0}
WRITE_ONLY = ["band_test_fail", "band_test_absent", "band_test_gen"]


def test_every_readable_option_round_trips_and_clamps(gpu):
    m = gpu.Model(model_path("front"))
    for key, (default, pairs) in READ_WRITE.items():
        assert m.get_option(key) == default, key
        for value, back in pairs:
            m.set_option(key, value)
            assert m.get_option(key) == back, (key, value)
        m.set_option(key, default)
        assert m.get_option(key) == default, key
    for key, (default, _) in READ_WRITE.items():   # no set reached a neighbour's field
        assert m.get_option(key) == default, key


def test_read_only_write_only_and_unknown_keys(gpu):
    m = gpu.Model(model_path("front"))
    for key, value in READ_ONLY.items():
        assert m.get_option(key) == value
        with pytest.raises(gpu.MiError, match="unknown option '%s'" % key):
            m.set_option(key, 1)
        assert m.get_option(key) == value
    for key in WRITE_ONLY:
        m.set_option(key, 0)
        with pytest.raises(gpu.MiError, match="unknown option '%s'" % key):
            m.get_option(key)
    for call in (lambda: m.set_option("nope", 1), lambda: m.get_option("nope")):
        with pytest.raises(gpu.MiError, match="unknown option 'nope'"):
            call()
