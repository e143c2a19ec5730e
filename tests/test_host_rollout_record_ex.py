"""oc_rollout_record_ex without a GPU: its export and record sink, every refusal (all before the first device call, so stand-in
pointers are never dereferenced), and trajectories.recorded_trajectories with event masks and layout ids on hand-built host
arrays."""
import ctypes
import os
import re

import numpy as np
import pytest

from overcooked_ai_amd import _lib

FAKE = 0x10000  # a 16-byte aligned stand-in device pointer: never touched
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _sink(actions=FAKE, states=FAKE, layouts=FAKE):
    return _lib.OcRecordSink(actions, states, layouts)


def _call(lib, b=None, rec="default", options=_lib.OPT_AUTO_RESET, start=None, events=None, horizon=400, n_steps=8):
    b = b if b is not None else _batch()
    rec = _sink() if isinstance(rec, str) else rec
    return lib.oc_rollout_record_ex(ctypes.byref(b), FAKE, ctypes.byref(rec) if rec is not None else None, None, None, None,
                                    horizon, options, 1, 0, 0, n_steps, ctypes.byref(start) if start is not None else None,
                                    ctypes.byref(events) if events is not None else None, None)


def _refused(lib, **kw):
    assert _call(lib, **kw) == -1  # OC_EINVAL
    msg = lib.oc_last_error().decode()
    assert msg.startswith("oc_rollout_record_ex:"), msg
    return msg


def test_exported(lib):
    assert "oc_rollout_record_ex" in _lib.EXPORTS and hasattr(lib, "oc_rollout_record_ex")


def test_record_sink_matches_the_header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        body = re.search(r"typedef struct OcRecordSink \{(.*?)\} OcRecordSink;", f.read(), re.S).group(1)
    fields = re.findall(r"^\s*[\w ]+?\*\s*(\w+);", body, re.M)
    assert fields == [name for name, _ in _lib.OcRecordSink._fields_] == ["d_actions", "d_states", "d_layout_ids"]
    # three pointers in declaration order
    assert [getattr(_lib.OcRecordSink, n).offset for n in fields] == [0, 8, 16]
    assert ctypes.sizeof(_lib.OcRecordSink) == 24


def test_needs_a_sink_with_an_array(lib):
    assert "NULL" in _refused(lib, rec=None)
    assert "NULL" in _refused(lib, rec=_sink(None, None, None))
    # any one array is enough (zero steps: nothing is launched)
    for rec in (_sink(FAKE, None, None), _sink(None, FAKE, None), _sink(None, None, FAKE)):
        assert _call(lib, rec=rec, n_steps=0) == 0


def test_misaligned_arrays(lib):
    assert "16-byte" in _refused(lib, rec=_sink(states=FAKE + 8))
    assert "d_actions" in _refused(lib, rec=_sink(actions=FAKE + 1))
    assert "d_layout_ids" in _refused(lib, rec=_sink(layouts=FAKE + 1))


def test_refused_options(lib):
    for opt in (_lib.OPT_FLAGS_TILED8, _lib.OPT_LANE_PAIR, _lib.OPT_PREDICATE_INTERACT, _lib.OPT_ONE_KERNEL):
        assert "options" in _refused(lib, options=_lib.OPT_AUTO_RESET | opt)


def test_one_player_tables_refused(lib):
    assert "two-player" in _refused(lib, b=_batch(two_players=False))


def test_start_spec_errors(lib):
    sp = _lib.OcStartSpec()
    sp.rnd_obj_prob_thresh = 1.5
    assert "rnd_obj_prob_thresh" in _refused(lib, start=sp)
    sp = _lib.OcStartSpec()
    sp.regen_first, sp.regen_count = 1, 2  # beyond the table of 2 layouts
    assert "regen range" in _refused(lib, start=sp)
    sp = _lib.OcStartSpec()
    sp.env_offset = 5  # the call's env_offset is 0
    assert "env_offset" in _refused(lib, start=sp)


def test_redraws_and_event_sinks_are_accepted(lib):
    # the same start spec oc_rollout_record refuses, with every kind of sink; zero steps: nothing is launched
    sp = _lib.OcStartSpec()
    sp.regen_first, sp.regen_count = 0, 2
    ev = _lib.OcEventSink(FAKE, FAKE, FAKE)
    assert _call(lib, start=sp, events=ev, n_steps=0) == 0
    assert _call(lib, start=sp, n_steps=0) == 0
    assert _call(lib, options=_lib.OPT_AUTO_RESET | _lib.OPT_ONE_WAVEFRONT, events=ev, n_steps=0) == 0
    assert _call(lib, n_steps=0) == 0


def test_launch_shape_errors(lib):
    assert "horizon" in _refused(lib, horizon=0)
    assert "n_steps" in _refused(lib, n_steps=-1)


# ---- recorded_trajectories with events_out / layouts_out, on host arrays

class _StubEnv:
    """What recorded_trajectories reads of a VecOvercookedEnv."""

    def __init__(self, table, layout_id, horizon):
        self.table, self.layout_id_host, self.horizon, self.n_envs = table, np.asarray(layout_id, np.uint16), horizon, len(layout_id)

    def _refresh_layout_ids(self):
        pass

    def spec_of(self, e):
        return self.table.specs[int(self.layout_id_host[e])]


def _table():
    from overcooked_ai_amd.layouts import LayoutTable, spec_from_name

    return LayoutTable([spec_from_name("cramped_room"), spec_from_name("asymmetric_advantages")], pad_to=(9, 5))


def _recording(table, episodes, H):
    """One env that plays `episodes` (a list of layout ids) back to back, H steps each: standard start states with the
    timestep of each step, every action STAY, rewards / events only where set below."""
    from overcooked_ai_amd.mdp import OvercookedGridworld
    from overcooked_ai_amd.state import pack_states

    K = H * len(episodes)
    S = np.zeros((K, table.n_planes, 1, 16), np.uint8)
    for g, lid in enumerate(episodes):
        spec = table.specs[lid]
        d = OvercookedGridworld.from_spec(spec).get_standard_start_state().to_dict()
        for t in range(H):
            d["timestep"] = t
            S[g * H + t] = pack_states(spec, [d], table.n_planes)
    A = np.full((K, 1, 2), 4, np.uint8)  # Action.STAY
    R = np.zeros((K, 1, 4), np.float32)
    F = np.zeros((K, 1), np.uint8)
    F[H - 1::H, 0] = _lib.F_DONE | _lib.F_RESET
    E = np.zeros((K, 1), np.int64)
    Lid = np.repeat(np.asarray(episodes, np.uint16), H).reshape(K, 1)
    return S, A, R, F, E, Lid


def test_converter_game_stats_and_layouts():
    from overcooked_ai_amd.mdp import EVENT_TYPES
    from overcooked_ai_amd.trajectories import recorded_trajectories

    table, H = _table(), 6
    S, A, R, F, E, Lid = _recording(table, [1, 0], H)
    onion, soup = EVENT_TYPES.index("onion_pickup"), EVENT_TYPES.index("soup_delivery")
    E[2, 0] = 1 << (2 * onion + 1)                      # episode 0, timestep 2: player 1 picks up an onion
    E[4, 0] = (1 << (2 * onion)) | (1 << (2 * soup))   # timestep 4: player 0 picks up an onion and delivers a soup
    R[4, 0] = [20, 0, 0, 0]
    R[3, 0] = [0, 0, 0, 3]                             # player 1 pots an onion
    E[H + 1, 0] = 1 << (2 * soup + 1)                  # episode 1, timestep 1
    env = _StubEnv(table, [0], H)  # (the env's layout NOW is 0: the first episode's must come from layouts_out)
    traj = recorded_trajectories(env, S, A, R, F, events_out=E, layouts_out=Lid.view(np.int16))
    assert list(traj["ep_lengths"]) == [H, H]
    assert [p["layout_name"] for p in traj["mdp_params"]] == ["asymmetric_advantages", "cramped_room"]
    g0 = traj["ep_infos"][0][-1]["episode"]["ep_game_stats"]
    g1 = traj["ep_infos"][1][-1]["episode"]["ep_game_stats"]
    assert set(g0) == set(EVENT_TYPES) | {"cumulative_sparse_rewards_by_agent", "cumulative_shaped_rewards_by_agent"}
    assert g0["onion_pickup"] == [[4], [2]] and g0["soup_delivery"] == [[4], []]
    assert all(g0[n] == [[], []] for n in EVENT_TYPES if n not in ("onion_pickup", "soup_delivery"))
    assert g1["soup_delivery"] == [[], [1]] and g1["onion_pickup"] == [[], []]
    for g, sparse, shaped in ((g0, [20, 0], [0, 3]), (g1, [0, 0], [0, 0])):
        for key, want in (("cumulative_sparse_rewards_by_agent", sparse), ("cumulative_shaped_rewards_by_agent", shaped)):
            assert g[key].dtype == np.int64 and list(g[key]) == want  # (the drop-in's int64 arrays)
    # the states are unpacked on each episode's own layout
    from overcooked_ai_amd.mdp import OvercookedGridworld

    for j, lid in enumerate((1, 0)):
        start = OvercookedGridworld.from_spec(table.specs[lid]).get_standard_start_state()
        assert [p.position for p in traj["ep_states"][j][0].players] == [p.position for p in start.players]
    # without the two arrays: the dict of today (no ep_game_stats; every episode on the env's layout now)
    plain = recorded_trajectories(env, S, A, R, F)
    assert "ep_game_stats" not in plain["ep_infos"][0][-1]["episode"]
    assert [p["layout_name"] for p in plain["mdp_params"]] == ["cramped_room", "cramped_room"]


def test_converter_refuses_a_layout_change_inside_an_episode():
    from overcooked_ai_amd.trajectories import recorded_trajectories

    table, H = _table(), 5
    S, A, R, F, E, Lid = _recording(table, [0, 1], H)
    Lid[H + 2, 0] = 0
    with pytest.raises(ValueError, match="layout id changes"):
        recorded_trajectories(_StubEnv(table, [0], H), S, A, R, F, layouts_out=Lid)


def test_converter_checks_step_counts():
    from overcooked_ai_amd.trajectories import recorded_trajectories

    table, H = _table(), 4
    S, A, R, F, E, Lid = _recording(table, [0], H)
    with pytest.raises(ValueError, match="number of steps"):
        recorded_trajectories(_StubEnv(table, [0], H), S, A, R, F, events_out=E[:-1])
