"""oc_rollout_record's argument checks, without a GPU: every refusal comes before the first device call, so stand-in pointers
are never dereferenced."""
import ctypes

import pytest

from overcooked_ai_amd import _lib

FAKE = 0x10000  # a 16-byte aligned stand-in device pointer: never touched


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _batch(two_players=True, n_layouts=2):
    b = _lib.OcBatch()
    b.d_layouts, b.d_layout_id = FAKE, FAKE
    b.n_envs, b.n_layouts, b.width, b.height, b.max_pots = 1000, n_layouts, 5, 4, 1
    b.batch_flags = _lib.BATCH_TWO_PLAYERS if two_players else 0
    b.max_free_cells = 6
    return b


def _call(lib, b=None, actions=FAKE, states=FAKE, options=_lib.OPT_AUTO_RESET, start=None, horizon=400, n_steps=8):
    b = b if b is not None else _batch()
    return lib.oc_rollout_record(ctypes.byref(b), FAKE, actions, states, None, None, None, horizon, options, 1, 0, 0, n_steps,
                                 ctypes.byref(start) if start is not None else None, None)


def _refused(lib, **kw):
    assert _call(lib, **kw) == -1  # OC_EINVAL
    return lib.oc_last_error().decode()


def test_exported(lib):
    assert "oc_rollout_record" in _lib.EXPORTS and hasattr(lib, "oc_rollout_record")


def test_needs_an_output(lib):
    assert "both NULL" in _refused(lib, actions=None, states=None)


def test_misaligned_states(lib):
    assert "16-byte" in _refused(lib, states=FAKE + 8)


def test_refused_options(lib):
    for opt in (_lib.OPT_FLAGS_TILED8, _lib.OPT_LANE_PAIR, _lib.OPT_PREDICATE_INTERACT):
        assert "options" in _refused(lib, options=_lib.OPT_AUTO_RESET | opt)


def test_layout_redraws_refused(lib):
    sp = _lib.OcStartSpec()
    sp.regen_first, sp.regen_count = 0, 2
    assert "regen_count" in _refused(lib, start=sp)


def test_one_player_tables_refused(lib):
    assert "two-player" in _refused(lib, b=_batch(two_players=False))


def test_nothing_to_do_is_ok_without_touching_the_device(lib):
    # (one-wavefront option accepted; zero steps returns before any launch)
    assert _call(lib, options=_lib.OPT_AUTO_RESET | _lib.OPT_ONE_WAVEFRONT, n_steps=0) == 0
    assert _call(lib, actions=None, n_steps=0) == 0
